// genl_adj_kernels.h -- adjoint sweep of the state path for Solver's value-function ansatz on the run-time-shaped value-net kernels
// (genl_kernels.h): adaptive_forward_process with detach_forward=False, reference solver.py:449-478 (c = -Z stays attached).
// At a fixed sample (n, k) everything the loss sees of theta goes through V(X_n, n) and grad_x V(X_n, n), so attached or not
//   dL/dtheta = sum_{n,k} grad_theta [ a_{n,k} V(X_n, n) + grad_x V(X_n, n) . U_{n,k} ]   at fixed X_n:
// the form genl_bwd_kernel consumes with per-sample weights.  Attaching the state path only changes WHICH a and U a sample gets:
// they depend on the adjoint lambda of the states, a reverse-time recursion per trajectory.  In the ansatz's orientation Z = B g,
// g_n = grad_x V(X_n, n), with the forward step of genl_kernels.h (X_{n+1} = X_n + b(X_n) dt - dt B Z_n + B xi sqrt(dt),
// Y_{n+1} = Y_n + (-|Z_n|^2 / 2 + f(X_{n+1})) dt + Z_n . xi sqrt(dt)):
//   mu_N = w^D (dLoss/dD),  mu_n = mu_{n+1} - (2/K) r_n  (r_n = V(X_n, n) - Y_n: the adjoint of Y_n),  lambda = -w^D grad g(X_N);
//   for n = N-1 .. 0:
//       Lam   = lambda + mu_{n+1} dt grad f(X_{n+1})                          (f enters Y_{n+1} at the MOVED state)
//       Zbar  = mu_{n+1} (xi sqrt(dt) - dt Z_n) - dt B^T Lam                  (adjoint of Z_n: through Y and through the move)
//       U_n   = B^T Zbar = mu_{n+1} U_fwd - dt B^T (mu_{n+1} Z_n + B^T Lam)   (U_fwd = B^T xi sqrt(dt): what the forward stored)
//       a_n   = mu_1 (n = 0),  (2/K) r_n (n >= 1)
//       lambda = Lam + dt J_b(X_n)^T Lam + a_n grad_x V(X_n, n) + grad_x^2 V(X_n, n) U_n.
// The last two terms are the input-segment adjoint of S = a V + grad V . U: the adjoint sweep of genl_bwd_kernel continued through
// layer 0.  genl_adj_kernel: one workgroup per 16-trajectory tile (the forward's grid and waves per tile), n = N-1 .. 0; per step
// it loads (x_n, t_n) and U_fwd from the tile's block of the path store, recomputes the activations (genl_value), forms g_n by
// the reverse sweep (genl_input_gradient), U_n by three d x d products (tables tSB / tSBT; sigma = s I: scalings), runs the tangent
// along U_n and the two-image adjoint down to the input segment, and updates lambda ((dt A)^T Lam from a table of its own, built
// by genl_adj_tables_kernel behind everything genl_tables_kernel writes; the element-wise drift kinds: their diagonal Jacobian).
// It overwrites the stored direction with U_n (mu folded in), writes a_n into the coefficient array and 1 / 0 into the
// tangent-weight array; genl_bwd_kernel then runs as it is.  Products are fp32 MFMA through genl_gemm1 / genl_gemm1x2.
// LDS: A, Ad (a, a'), AB, ABd (abar, abar' over ALL TB blocks: the input segment included; AB first serves as the image of the
// reverse sweep) and three images of DB0 blocks (Lam, its successor / B^T products, U_fwd).
#pragma once
#include "genl_kernels.h"

namespace psp {

struct GenlAdjArgs {
    GenlArgs a;                     // as the forward's: tables, params, path (rewritten), problem and net description
    const float* mu;                // (N + 1, Kpad): mu_n; row 0 unused
    const float* resid;             // (N + 1, Kpad): a_n
    const float* lamN;              // (K_local, d): -w^D grad g(X_N)
    float* lam0;                    // (K_local, d) dLoss/dX_0, or NULL
    float* coef_out;                // (N + 1, Kpad): the backward's coefficient array <- a_n (0 at n = N and on padding rows)
    float* wt_out;                  // (N + 1, Kpad): the backward's tangent weights <- 1 (0 at n = N and on padding rows)
    long long tAT;                  // float offset of the A-operand table of (dt A)^T (layout of tSB)
};

__host__ __device__ inline int genl_adj_lds_bytes(int TB, int DB0) { return (4 * TB + 3 * DB0) * 1024; }

// (the kernels themselves are compiled by the one unit that launches them, genl_adj_instance.hip, which defines PSP_GENL_ADJ_KERNELS)
#ifdef PSP_GENL_ADJ_KERNELS
// (dt A)^T in the forward layout of genl_tables_kernel: [mb][ks / 4][lane][ks & 3], row = 16 mb + rowmap(lane & 15), k = 4 ks + q
__global__ __launch_bounds__(256) void genl_adj_tables_kernel(const GenlAdjArgs aa) {
    const GenlArgs& a = aa.a;
    if (!a.driftA) return;
    float* T = a.tables_w + aa.tAT;
    const int DBs = a.DB0, KSs = 4 * DBs, d = a.d;
    const long long gtid = (long long)blockIdx.x * blockDim.x + threadIdx.x, gn = (long long)gridDim.x * blockDim.x;
    for (long long idx = gtid; idx < (long long)DBs * KSs * 64; idx += gn) {
        const int lane = (int)((idx >> 2) & 63);
        const long long t = idx >> 8;
        const int ks = 4 * (int)(t % (KSs / 4)) + (int)(idx & 3), mb = (int)(t / (KSs / 4));
        const int ii = lane & 15, q = lane >> 4;
        const int row = 16 * mb + 4 * (ii & 3) + (ii >> 2), col = 4 * ks + q;
        T[idx] = (row < d && col < d) ? a.g.dt * a.driftA[(size_t)col * d + row] : 0.f;
    }
}

template <int NW>
__global__ __launch_bounds__(64 * NW) void genl_adj_kernel(const GenlAdjArgs aa_) {
    PSP_COND_EXIT(aa_.a.g);
    const GenlAdjArgs* aa = &aa_;
    const KArgs ga = &aa_.a;
    const KGen a = &ga->g;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int TB = ga->TB, DB0 = ga->DB0, D = ga->d, L = ga->L;
    float* A = lds;
    float* Ad = A + TB * 256;
    float* AB = Ad + TB * 256;
    float* ABd = AB + TB * 256;
    float* Lam = ABd + TB * 256;                                     // lambda, then Lam of the step
    float* T1 = Lam + DB0 * 256;                                     // mu Z + B^T Lam; then the next lambda (the two swap roles)
    float* Uf = T1 + DB0 * 256;                                      // U_fwd
    const float* __restrict__ T = ga->tables;
    const int lane = threadIdx.x & 63, j = lane & 15, q = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int t16 = blockIdx.x, k = t16 * 16 + j;
    const bool kvalid = k < a->K_local;
    const int Kpad = a->ntile16 * 16, N = a->N;
    const float dt = a->dt, sig = a->sigma_scale;
    const bool dense = ga->dense != 0;
    const int KSd = 4 * DB0;
    const size_t PBL = (size_t)2 * DB0 * 256;
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    for (int i = threadIdx.x; i < (4 * TB + 3 * DB0) * 256; i += 64 * NW) lds[i] = 0.f;
    tile_sync<NW>();
    for (int b = wave; b < DB0; b += NW) {
        f32x4 v;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int f = 16 * b + 4 * r + q;
            v[r] = (f < D && kvalid) ? aa->lamN[(size_t)k * D + f] : 0.f;
        }
        img_put(Lam, b, v, lane);
    }
    if (wave == 0 && q == 0) { aa->coef_out[(size_t)N * Kpad + k] = 0.f; aa->wt_out[(size_t)N * Kpad + k] = 0.f; }
    tile_sync<NW>();
    f32x4 Rr[GenlGeo<NW>::MAXSLOT], Zr[GenlGeo<NW>::MAXSLOT];
#pragma unroll
    for (int s = 0; s < GenlGeo<NW>::MAXSLOT; ++s) { Rr[s] = zero4; Zr[s] = zero4; }
    // y = M x for the tile (M = B or B^T from its table; sigma = s I: a scaling of the state rows), one output block
    auto sigma_block = [&](long long tbl, const float* img, int ob) __attribute__((always_inline)) {
        f32x4 acc = zero4;
        if (dense) {
            genl_gemm1<8>(acc, T + tbl + (size_t)ob * KSd * 64, KSd, img, lane);
        } else {
            const f32x4 v = img_get(img, ob, lane);
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[r] = (16 * ob + 4 * r + q) < D ? sig * v[r] : 0.f;
        }
        return acc;
    };
    for (int n = N - 1; n >= 0; --n) {
        const float mu = kvalid ? aa->mu[(size_t)(n + 1) * Kpad + k] : 0.f;
        const float an = kvalid ? aa->resid[(size_t)n * Kpad + k] : 0.f;
        const float wt = kvalid ? 1.f : 0.f;
        float* pb = a->path + ((size_t)n * a->ntile16 + t16) * PBL + lane;
        const float* pn = a->path + ((size_t)(n + 1) * a->ntile16 + t16) * PBL + lane;       // X_{n+1}
        for (int ks = wave; ks < 4 * DB0; ks += NW) { A[ks * 64 + lane] = pb[ks * 64]; Uf[ks * 64 + lane] = pb[(size_t)DB0 * 256 + ks * 64]; }
        if (ga->runcost_kind != 0) {                                 // Lam = lambda + mu dt grad f(X_{n+1}), f = sum_i p_i x_i^2
            for (int b = wave; b < DB0; b += NW) {
                f32x4 lv = img_get(Lam, b, lane);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int f = 16 * b + 4 * r + q;
                    if (f < D) lv[r] = fmaf((mu * dt) * (2.0f * ga->runcost[f]), pn[(4 * b + r) * 64], lv[r]);
                }
                img_put(Lam, b, lv, lane);
            }
        }
        tile_sync<NW>();
        genl_value<NW>(ga, T, A, Rr, lane, q, wave);
        genl_input_gradient<NW>(ga, T, Rr, AB, lane, q, wave);      // blocks 0 .. DB0 - 1 of AB: grad_{[x, t]} V
        // ---- U_n = mu U_fwd - dt B^T (mu Z_n + B^T Lam), Z_n = B g_n (the tables' rows and columns >= d are zero: no time row)
        for (int ob = wave; ob < DB0; ob += NW) {
            const f32x4 Z = sigma_block(ga->tSB, AB, ob), BL = sigma_block(ga->tSBT, Lam, ob);
            img_put(T1, ob, mu * Z + BL, lane);
        }
        tile_sync<NW>();
        for (int ob = wave; ob < DB0; ob += NW) {
            const f32x4 U = mu * img_get(Uf, ob, lane) - dt * sigma_block(ga->tSBT, T1, ob);
            img_put(Ad, ob, U, lane);
#pragma unroll
            for (int r = 0; r < 4; ++r) pb[(size_t)DB0 * 256 + (4 * ob + r) * 64] = U[r];
        }
        // ---- adjoint seeds over the whole concatenation: abar = a w_out, abar' = w_out
        for (int b = wave; b < TB; b += NW) {
            const f32x4 w = vec_get(T + ga->vW, b, q);
            img_put(AB, b, an * w, lane);
            img_put(ABd, b, wt * w, lane);
        }
        tile_sync<NW>();
        // ---- tangent along U_n: z_i' = W_i^T a_{i-1}', a_i' = phi1(r_i) z_i'
        for (int i = 0; i < L; ++i) {
            const int seg = ga->off[i + 1];
            const int KSin = 4 * seg, HBi = ga->HB[i], hoff = seg - DB0;
#pragma unroll
            for (int s = 0; s < GenlGeo<NW>::MAXSLOT; ++s) {
                const int mb = wave + NW * s - hoff;
                if (mb >= 0 && mb < HBi) {
                    f32x4 acd = zero4;
                    genl_gemm1<8>(acd, T + ga->tF[i] + (size_t)mb * KSin * 64, KSin, Ad, lane);
                    Zr[s] = acd;
                    img_put(Ad, seg + mb, gact_h1(ga->act, Rr[s]) * acd, lane);
                }
            }
            tile_sync<NW>();
        }
        // ---- adjoint of S = a V + V' down to the input segment (genl_bwd_kernel's sweep, continued through layer 0; only abar
        // of the input blocks is needed: abar_0 = a grad_x V + grad_x^2 V U)
        for (int i = L - 1; i >= 0; --i) {
            const int seg = ga->off[i + 1];
            const int HBi = ga->HB[i], KSh = 4 * HBi, hoff = seg - DB0;
#pragma unroll
            for (int s = 0; s < GenlGeo<NW>::MAXSLOT; ++s) {
                const int hb = wave + NW * s;
                if (hb >= hoff && hb < hoff + HBi) {
                    const f32x4 gh = img_get(AB, DB0 + hb, lane), ghd = img_get(ABd, DB0 + hb, lane);
                    const f32x4 p1 = gact_h1(ga->act, Rr[s]);
                    img_put(AB, DB0 + hb, gh * p1 + ghd * (gact_h2(ga->act, Rr[s]) * Zr[s]), lane);
                    img_put(ABd, DB0 + hb, ghd * p1, lane);
                }
            }
            tile_sync<NW>();
            for (int ob = wave; ob < seg; ob += NW) {
                const float* tbl = T + ga->tR[i] + (size_t)ob * KSh * 64;
                f32x4 acc = img_get(AB, ob, lane);
                if (ob >= DB0) {
                    f32x4 acd = img_get(ABd, ob, lane);
                    genl_gemm1x2<4>(acc, acd, tbl, KSh, AB + seg * 256, ABd + seg * 256, lane);
                    img_put(ABd, ob, acd, lane);
                } else {
                    genl_gemm1<8>(acc, tbl, KSh, AB + seg * 256, lane);
                }
                img_put(AB, ob, acc, lane);
            }
            tile_sync<NW>();
        }
        // ---- lambda = Lam + dt J_b(X_n)^T Lam + abar_0 (state rows only), into the other image: the product reads all of Lam
        for (int b = wave; b < DB0; b += NW) {
            const f32x4 lv = img_get(Lam, b, lane), ab = img_get(AB, b, lane), x = img_get(A, b, lane);
            f32x4 jl = zero4;
            if (ga->driftA) genl_gemm1<8>(jl, T + aa->tAT + (size_t)b * KSd * 64, KSd, Lam, lane);
            f32x4 nl;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int f = 16 * b + 4 * r + q;
                float jd = 0.f;
                if (f < D && a->drift_kind == DRIFT_DIAG) jd = a->drift[f];
                else if (f < D && a->drift_kind == DRIFT_DWELL) jd = -4.0f * a->drift[f] * (3.0f * x[r] * x[r] - 1.0f);
                nl[r] = f < D ? lv[r] + jl[r] + dt * jd * lv[r] + ab[r] : 0.f;
            }
            img_put(T1, b, nl, lane);
        }
        if (wave == 0 && q == 0) { aa->coef_out[(size_t)n * Kpad + k] = an; aa->wt_out[(size_t)n * Kpad + k] = wt; }
        tile_sync<NW>();
        float* sw = Lam; Lam = T1; T1 = sw;
    }
    if (aa->lam0) {
        for (int b = wave; b < DB0; b += NW) {
            const f32x4 lv = img_get(Lam, b, lane);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int f = 16 * b + 4 * r + q;
                if (f < D && kvalid) aa->lam0[(size_t)k * D + f] = lv[r];
            }
        }
    }
}

#endif  // PSP_GENL_ADJ_KERNELS

// defined in genl_adj_instance.hip: the (dt A)^T table, then the sweep with nw = 1, 4 or 8 waves per tile
hipError_t genl_adj_launch(const GenlAdjArgs& a, int nw, int ntile16, int lds_bytes, hipStream_t st);

}  // namespace psp
