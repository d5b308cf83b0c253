// PINN residual of a dense-concat value net by forward-Laplacian propagation, and its parameter gradient (psp_pinn_*).
//
// Per sample the net input a_0 = [x] or [x, t] carries a tangent e_j for every input column j and a Laplacian row:
//     z = W^T a + b     z'_j = W^T a'_j     Dz = W^T Da              (a'_{j,0} = e_j, Da_0 = 0)
//     h = phi(z)        h'_j = phi'(z) z'_j Dh = phi''(z) S + phi'(z) Dz,   S = sum over the SPACE directions of z'_j^2
//     a <- [a, h]       (same for a' and Da);   V = w^T a + b,  V'_j = w^T a'_j,  Lap V = w^T Da
// The recursion for (S, D) is linear in the directions, so a tile = (one sample, one block of kPinnDirs directions) is
// independent of every other tile: it carries the value row (row 0), its own partial-Laplacian row (row 1) and kPinnDirs tangent
// rows -- the 16 rows of one v_mfma_f32_16x16x4_f32 operand.  Only Lap V is summed over a sample's direction blocks.
//
// Nothing in the recursion needs the directions to be unit vectors.  A sample's directions are, in this order, n_grad gradient
// directions e_0 .. e_{n_in-1} (they give grad V and V_t; the space ones are counted in S only on the scaled-identity path, where
// they are the second-order directions as well) and n_hess second-order directions u_j read from the table `dirs` (n_hess, d),
// time column 0.  With sum_j u_j u_j^T = B B^T the row D ends as sum_j u_j^T (Hess_x V) u_j = trace(B B^T Hess_x V): a dense
// sigma.  The u_j are counted in S, their first derivatives are not stored and their tangent rows get adjoint seed 0.  The
// directions counted in S are the global indices [cnt_lo, cnt_hi): [0, d) with a scaled identity (n_grad = n_in, n_hess = 0, seeds
// 1.0, lap_coef = s^2 / 2), [n_grad, n_grad + n_hess) with a table (lap_coef = 1 / 2: the scale sits in the directions).
//
//   pinn_forward_kernel   per tile: V, V'_j of its directions, its part of Lap V           -> scratch
//   pinn_finish_kernel    per sample: R = [V_t] + lap_coef Lap V + b . grad V + h(x, V, s grad V) and the seed coefficients
//                         dR/dV, dR/dV'_j of the adjoint (dR/dLap V = lap_coef is a constant)
//   pinn_backward_kernel  per tile: the forward again (everything stays in LDS), the adjoint sweep, every weight gradient as MFMA
//                         outer products over the 16 rows; a workgroup adds the tiles it owns into its own partial gradient
//                         (first tile stores), the partials are summed in a fixed order by reduce_grad_kernel.
// Every matrix product is fp32 MFMA; the activations sit in LDS row-major with a stride = 4 (mod 64) floats, which spreads the
// A-operand read (16 rows x 4 k) over all banks.  Weights are read from global memory (L2) through (k, column) strides, so the
// (in, out) layout of DenseNet and the (out, in) layout of nn.Linear need no copy.
//
// An h that reads t (psp_pinn_pairs_*): the reference hands h the times as a (K, 1) column, so the residual is the (K, K) matrix
//     R[i, j] = A_j + nl(exp(2 al |x_j|^2 + 2 tau t_i) - y_j^2)         i: times, j: samples, y_j = V(x_j, t_j)
// and the loss is alpha0 / K^2 sum_ij R[i, j]^2.  Everything that passes through the net is per sample j:
//   pinn_finish_kernel<true>   writes A_j (the residual without the pair term) where R goes, dA/dV = -lin_j in the dR/dV slot
//   pinn_pair_kernel           one wave per sample j, the lanes over the times i (staged once per workgroup in LDS): lane partials of
//                              sum_i R, sum_i R^2, sum_i R nl' in i order, a butterfly over the lanes, then
//                              rho_j = c sum_i R, nu_j = c (-2 y_j) sum_i R nl', c = 2 alpha0 / K^2, and sum_i R^2 in double -> work[j]
//   pinn_pair_loss_kernel      one wave: lane l adds its run of work[j] in index order in double, lane 0 adds the 64 runs in lane
//                              order: loss = alpha0 / K^2 sum.  No atomics anywhere: the same bits on every run.
//   pinn_backward_kernel<true> rbar = rho, and nu_j added to the value row's seed of sample j (direction block 0)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "gh_kinds.h"

namespace psp {

constexpr int kPinnDirs = 14;          // tangent rows of a tile (rows 2 .. 15)
constexpr int kPinnZS = 132;           // row stride of a layer's pre-activation image: >= 128 columns, = 4 (mod 64)
constexpr int kPinnThreads = 256;      // four waves
constexpr int kPinnMaxWg = 256;        // partial gradients of the backward kernel

// (DRIFT_* live in hjb_kernels.h with the MFMA machinery this header does without: api_pinn.hip ties these to PSP_DRIFT_*, api_hjb.hip those)
enum { PINN_DRIFT_ZERO = 0, PINN_DRIFT_DIAG = 2, PINN_DRIFT_DWELL = 3 };                      // PSP_DRIFT_*
enum { PINN_ACT_RELU2 = 0, PINN_ACT_TANH2 = 1, PINN_ACT_TANH = 2 };                           // PSP_ACT_*

struct PinnArgs {
    int d, n_in, K, L, act;
    int nblk, ntiles;                  // direction blocks per sample, tiles = K * nblk (tile = k * nblk + blk)
    int n_grad, n_hess;                // gradient directions (0 or n_in), second-order directions of the table
    int cnt_lo, cnt_hi;                // global direction indices [cnt_lo, cnt_hi) are counted in S
    int TOT, AST;                      // columns of the concatenation, its LDS row stride
    int H[4], fan[5];                  // widths; fan[i] = inputs of layer i = first column of h_i; fan[L] = TOT
    int offW[5], offb[5], sk[5], sc[5];   // flat-parameter offsets and the (k, column) strides of every weight; [L]: output layer
    int P, G;                          // parameters; workgroups (= partial gradients) of the backward kernel
    int drift_kind, h_kind;
    float s, h_par[4];
    float lap_coef;                    // dR / dLap V: s^2 / 2, or 1 / 2 with a direction table
    const float* drift;
    const float* dirs;                 // (n_hess, d) or null
    const float* params;
    const float* x;                    // (K, d)
    const float* t;                    // (K) or null
    float* V;                          // scratch: V (K), lap (K, nblk), gradV (K, n_grad), cV (K), cG (K, n_grad)
    float* lap;
    float* gradV;
    float* cV;
    float* cG;
    float* R;                          // (K) residual
    const float* rbar;                 // (K) dLoss/dR
    float* gpart;                      // (G, P)
    int pairs;                         // psp_pinn_pairs_*: the finish kernel leaves the pair term of h out
    const float* vadd;                 // (K) added to the value-row seed, or null
};

struct PinnPairArgs {
    int d, K, h_kind;
    float al, tau2;                    // h_par[0], 2 h_par[3]
    float coef;                        // 2 alpha0 / K^2
    double loss_coef;                  // alpha0 / K^2
    const float* x;                    // (K, d)
    const float* t;                    // (K)
    const float* V;                    // (K) of the scratch
    const float* A;                    // (K) of pinn_finish_kernel<true>
    float* rho;                        // (K)
    float* nu;                         // (K)
    double* work;                      // (K) sum_i R[i, j]^2
    float* loss;                       // (1)
};

constexpr int kPinnPairMaxK = 16384;   // K^2 <= 2.7e8 pairs; the staged times take 4 K <= 64 KiB of LDS
constexpr int kPinnPairMaxWg = 1024;

inline int pinn_row_stride(int tot) { int a = (tot + 3) & ~3; while ((a & 63) != 4) a += 4; return a; }
inline int pinn_lds_bytes(int ast, int L, bool backward) { return 4 * ((backward ? 2 : 1) * 16 * ast + L * 16 * kPinnZS + 64 + 16 + 16); }

hipError_t pinn_launch_forward(const PinnArgs& a, int lds_bytes, hipStream_t stream);
hipError_t pinn_launch_backward(const PinnArgs& a, int lds_bytes, hipStream_t stream);
hipError_t pinn_launch_pairs(const PinnPairArgs& a, hipStream_t stream);

#ifdef PSP_PINN_KERNELS

typedef float pinn_f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ pinn_f32x4 pinn_mfma(float a, float b, pinn_f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// phi and its first three derivatives
__device__ __forceinline__ void pinn_act(int act, float z, float& p0, float& p1, float& p2, float& p3) {
    if (act == PINN_ACT_RELU2) {
        const float r = fmaxf(z, 0.f);
        p0 = r * r; p1 = 2.f * r; p2 = z > 0.f ? 2.f : 0.f; p3 = 0.f;
        return;
    }
    const float r = tanhf(z), q = 1.f - r * r;
    if (act == PINN_ACT_TANH) {
        p0 = r; p1 = q; p2 = -2.f * r * q; p3 = -2.f * q * (1.f - 3.f * r * r);
    } else {
        p0 = r * r; p1 = 2.f * r * q; p2 = 2.f * q * (1.f - 3.f * r * r); p3 = -8.f * r * q * (2.f - 3.f * r * r);
    }
}

// Z (16 x H, stride kPinnZS) = A (16 x fan, stride ast) . W (fan x H through strides); wave w takes the column tiles w, w + 4, ..
__device__ __forceinline__ void pinn_rows_times_w(const float* A, int ast, int fan, const float* __restrict__ W, int sk, int sc,
                                                  int H, float* Z) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, row = lane & 15, kq = lane >> 4;
    const int nct = (H + 15) >> 4, nks = (fan + 3) >> 2;
    for (int ct = wave; ct < nct; ct += 4) {
        const int col = ct * 16 + row;
        const bool cok = col < H;
        pinn_f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
        for (int ks = 0; ks < nks; ks += 2) {                   // two accumulators: the MFMA's dependent latency exceeds its issue time
            const int k0 = ks * 4 + kq, k1 = k0 + 4;
            const float a0 = k0 < fan ? A[row * ast + k0] : 0.f;
            const float b0 = (k0 < fan && cok) ? W[(size_t)k0 * sk + (size_t)col * sc] : 0.f;
            const float a1 = k1 < fan ? A[row * ast + k1] : 0.f;
            const float b1 = (k1 < fan && cok) ? W[(size_t)k1 * sk + (size_t)col * sc] : 0.f;
            acc0 = pinn_mfma(a0, b0, acc0);
            acc1 = pinn_mfma(a1, b1, acc1);
        }
        const pinn_f32x4 acc = acc0 + acc1;
#pragma unroll
        for (int r = 0; r < 4; ++r) Z[(4 * kq + r) * kPinnZS + col] = acc[r];      // col < 128 <= kPinnZS
    }
}

// The forward of one tile: fills Act (16 x TOT) and the pre-activation images Zp (layer i at Zp + i * 16 * kPinnZS; row 0 with its
// bias), leaves out16[r] = w . Act[r] in red[64 + r] (16 floats behind the four waves' parts).  Ends with a barrier.
__device__ __forceinline__ void pinn_forward_tile(const PinnArgs& a, int k, int blk, float* Act, float* Zp, float* red) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ast = a.AST, n_in = a.n_in, d = a.d;
    const int j0 = blk * kPinnDirs - 2;                            // row r >= 2 carries the direction j0 + r
    for (int idx = tid; idx < 16 * n_in; idx += kPinnThreads) {
        const int r = idx / n_in, c = idx - r * n_in;
        float v = 0.f;
        if (r == 0) v = c < d ? a.x[(size_t)k * d + c] : a.t[k];
        else if (r >= 2) {
            const int j = j0 + r;
            if (j < a.n_grad) v = j == c ? 1.f : 0.f;
            else if (j < a.n_grad + a.n_hess) v = c < d ? a.dirs[(size_t)(j - a.n_grad) * d + c] : 0.f;
        }
        Act[r * ast + c] = v;
    }
    __syncthreads();
    for (int i = 0; i < a.L; ++i) {
        float* Z = Zp + i * 16 * kPinnZS;
        const int fan = a.fan[i], H = a.H[i];
        pinn_rows_times_w(Act, ast, fan, a.params + a.offW[i], a.sk[i], a.sc[i], H, Z);
        __syncthreads();
        for (int c = tid; c < H; c += kPinnThreads) {
            const float z0 = Z[c] + a.params[a.offb[i] + c];
            Z[c] = z0;
            float p0, p1, p2, p3;
            pinn_act(a.act, z0, p0, p1, p2, p3);
            float S = 0.f;
            for (int r = 2; r < 16; ++r) {
                const float zp = Z[r * kPinnZS + c];
                if (j0 + r >= a.cnt_lo && j0 + r < a.cnt_hi) S = fmaf(zp, zp, S);
                Act[r * ast + fan + c] = p1 * zp;
            }
            Act[fan + c] = p0;
            Act[ast + fan + c] = fmaf(p2, S, p1 * Z[kPinnZS + c]);
        }
        __syncthreads();
    }
    {   // out16 = Act (16 x TOT) . w: the k-steps are dealt to the four waves, column 0 of the product carries w
        const int row = lane & 15, kq = lane >> 4, tot = a.TOT, nks = (tot + 3) >> 2;
        const float* w = a.params + a.offW[a.L];
        pinn_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int ks = wave; ks < nks; ks += 4) {
            const int k0 = ks * 4 + kq;
            const float a0 = k0 < tot ? Act[row * ast + k0] : 0.f;
            const float b0 = (k0 < tot && row == 0) ? w[k0] : 0.f;
            acc = pinn_mfma(a0, b0, acc);
        }
        if (row == 0) {
#pragma unroll
            for (int r = 0; r < 4; ++r) red[wave * 16 + 4 * kq + r] = acc[r];
        }
        __syncthreads();
        if (tid < 16) red[64 + tid] = (red[tid] + red[16 + tid]) + (red[32 + tid] + red[48 + tid]);
        __syncthreads();
    }
}

__global__ __launch_bounds__(kPinnThreads) void pinn_forward_kernel(const PinnArgs a) {
    extern __shared__ float pinn_lds[];
    float* Act = pinn_lds;
    float* Zp = Act + 16 * a.AST;
    float* red = Zp + a.L * 16 * kPinnZS;
    for (int tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
        const int k = tile / a.nblk, blk = tile - k * a.nblk;
        pinn_forward_tile(a, k, blk, Act, Zp, red);
        const int tid = threadIdx.x;
        if (tid < 16) {
            const float o = red[64 + tid];
            if (tid == 0) { if (blk == 0) a.V[k] = o + a.params[a.offb[a.L]]; }
            else if (tid == 1) a.lap[(size_t)k * a.nblk + blk] = o;
            else {
                const int j = blk * kPinnDirs + tid - 2;
                if (j < a.n_grad) a.gradV[(size_t)k * a.n_grad + j] = o;
            }
        }
        // (the next tile writes `red` only behind the barriers of its forward)
    }
}

// One thread per sample: the residual and what the adjoint is seeded with.  kPairs: without the pair term nl(..) of
// GH_EXPBALL_SQ / GH_EXPBALL_SIN, which pinn_pair_kernel adds per (time, sample).
template <bool kPairs>
__global__ void pinn_finish_kernel(const PinnArgs a) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= a.K) return;
    const int d = a.d, n_in = a.n_in;
    const float s = a.s, y = a.V[k];
    const float* g = a.gradV + (size_t)k * n_in;                   // (read only with n_grad = n_in)
    const float* x = a.x + (size_t)k * d;
    float* cg = a.cG + (size_t)k * n_in;
    float lap = 0.f;
    for (int b = 0; b < a.nblk; ++b) lap += a.lap[(size_t)k * a.nblk + b];
    float bg = 0.f, g2 = 0.f, rr = 0.f, sx = 0.f;
    for (int j = 0; j < d; ++j) {
        const float xj = x[j];
        rr = fmaf(xj, xj, rr);
        sx += xj;
        if (a.n_grad == 0) continue;                               // no drift, no time input, an h that does not read z
        float bj = 0.f;
        if (a.drift_kind == PINN_DRIFT_DWELL) bj = -(4.0f * a.drift[j] * (xj * (xj * xj - 1.0f)));
        else if (a.drift_kind == PINN_DRIFT_DIAG) bj = a.drift[j] * xj;
        bg = fmaf(bj, g[j], bg);
        g2 = fmaf(g[j], g[j], g2);
        // dR / dg_j = b_j + 2 p2 s^2 g_j for h = .. + p2 |s grad V|^2 (GH_QUAD: p2 = -1 / 2)
        if (a.h_kind == GH_QUAD) cg[j] = bj - s * s * g[j];
        else if (a.h_kind == GH_AFFINE_EXP) cg[j] = bj + (2.0f * a.h_par[2]) * (s * s) * g[j];
        else cg[j] = bj;
    }
    float h = 0.f, hy = 0.f;
    if (a.h_kind == GH_QUAD) h = -0.5f * s * s * g2;
    else if (a.h_kind == GH_ALLEN_CAHN) { h = y - y * y * y; hy = 1.0f - 3.0f * y * y; }
    else if (a.h_kind == GH_AFFINE_EXP) {                        // (g2 = 0 with n_grad = 0: the host refuses p2 != 0 there)
        float minus_h;
        gh_affine_exp(a.h_par, y, s * s * g2, minus_h, hy);
        h = -minus_h;
    } else if (a.h_kind == GH_SINE_SOURCE) {                     // (sub-mode 1 reads x_0 only: d = 1 has no x[1])
        float minus_h;
        gh_sine_source(a.h_par, y, x[0], d > 1 ? x[1] : 0.f, minus_h, hy);
        h = -minus_h;
    } else if (a.h_kind >= GH_EXPBALL_LIN) {                           // the exponential-on-the-ball family (gen_kernels.h)
        const float al = a.h_par[0];
        const float rl = a.h_kind == GH_EXPBALL_SIN_FULL ? sx * sx : rr;    // the exponent keeps |x|^2
        const float lin = 2.0f * al * (2.0f * al * rl + a.h_par[1]) + a.h_par[2];
        float nl = 0.f, nly = 0.f;
        if (a.h_kind != GH_EXPBALL_LIN && !(kPairs && (a.h_kind == GH_EXPBALL_SQ || a.h_kind == GH_EXPBALL_SIN))) {
            const float arg = expf(2.0f * al * rr) - y * y;
            if (a.h_kind == GH_EXPBALL_SQ) { nl = arg; nly = -2.0f * y; }
            else { nl = sinf(arg); nly = -2.0f * y * cosf(arg); }
        }
        h = nl - y * lin;
        hy = nly - lin;
    }
    float R = a.lap_coef * lap + bg + h;
    if (n_in > d) { R += g[d]; cg[d] = 1.0f; }                     // (a time input implies n_grad = n_in)
    a.R[k] = R;
    a.cV[k] = hy;
}

// kVadd: a.vadd[k] joins the value-row seed of sample k (its direction block 0).
template <bool kVadd>
__global__ __launch_bounds__(kPinnThreads) void pinn_backward_kernel(const PinnArgs a) {
    extern __shared__ float pinn_lds[];
    float* Act = pinn_lds;
    float* Zp = Act + 16 * a.AST;
    float* red = Zp + a.L * 16 * kPinnZS;
    float* sd = red + 64 + 16;
    float* Adj = sd + 16;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, row = lane & 15, kq = lane >> 4;
    const int ast = a.AST, tot = a.TOT, L = a.L;
    float* gp = a.gpart + (size_t)blockIdx.x * a.P;
    bool first = true;
    for (int tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x, first = false) {
        const int k = tile / a.nblk, blk = tile - k * a.nblk;
        pinn_forward_tile(a, k, blk, Act, Zp, red);
        if (tid < 16) {                                            // dLoss / d(V, Lap V, V'_j) of this tile's rows
            const float rb = a.rbar[k];
            float v;
            if (tid == 0) {                                        // the value itself enters R once per sample
                v = blk == 0 ? rb * a.cV[k] : 0.f;
                if (kVadd && blk == 0) v += a.vadd[k];
            }
            else if (tid == 1) v = a.lap_coef * rb;
            else {
                const int j = blk * kPinnDirs + tid - 2;
                v = j < a.n_grad ? rb * a.cG[(size_t)k * a.n_grad + j] : 0.f;
            }
            sd[tid] = v;
        }
        __syncthreads();
        const float* w = a.params + a.offW[L];
        for (int c = tid; c < tot; c += kPinnThreads) {            // output layer: dw, and the adjoint of the concatenation
            const float wc = w[c];
            float gsum = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                gsum = fmaf(sd[r], Act[r * ast + c], gsum);
                Adj[r * ast + c] = sd[r] * wc;
            }
            gp[a.offW[L] + c] = first ? gsum : gp[a.offW[L] + c] + gsum;
        }
        if (tid == 0) gp[a.offb[L]] = first ? sd[0] : gp[a.offb[L]] + sd[0];
        __syncthreads();
        for (int i = L - 1; i >= 0; --i) {
            float* Z = Zp + i * 16 * kPinnZS;
            const int fan = a.fan[i], H = a.H[i];
            for (int c = tid; c < H; c += kPinnThreads) {          // through the activation: Z becomes (z-bar, Dz-bar, z'-bar_j)
                const int col = fan + c;
                const float z0 = Z[c], dz = Z[kPinnZS + c];
                const float hb = Adj[col], dhb = Adj[ast + col];
                float p0, p1, p2, p3;
                pinn_act(a.act, z0, p0, p1, p2, p3);
                float S = 0.f, dot = 0.f;
                for (int r = 2; r < 16; ++r) {
                    const float zp = Z[r * kPinnZS + c], hbr = Adj[r * ast + col];
                    const int j = blk * kPinnDirs + r - 2;
                    const bool space = j >= a.cnt_lo && j < a.cnt_hi;
                    if (space) S = fmaf(zp, zp, S);
                    dot = fmaf(zp, hbr, dot);
                    Z[r * kPinnZS + c] = space ? fmaf(2.f * p2 * zp, dhb, p1 * hbr) : p1 * hbr;
                }
                Z[kPinnZS + c] = p1 * dhb;
                const float zb = p1 * hb + p2 * dot + (p3 * S + p2 * dz) * dhb;
                Z[c] = zb;
                gp[a.offb[i] + c] = first ? zb : gp[a.offb[i] + c] + zb;
            }
            __syncthreads();
            const float* W = a.params + a.offW[i];
            const int sk = a.sk[i], sc = a.sc[i];
            const int nft = (fan + 15) >> 4, nct = (H + 15) >> 4;
            // dW_i (fan x H) = Act^T (fan x 16 rows) . Z (16 rows x H): one MFMA tile per (16 inputs, 16 outputs)
            for (int tl = wave; tl < nft * nct; tl += 4) {
                const int ft = tl / nct, ct = tl - ft * nct;
                const int f = ft * 16 + row, c = ct * 16 + row;
                pinn_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) {
                    const int r = kk * 4 + kq;
                    const float av = f < fan ? Act[r * ast + f] : 0.f;
                    const float bv = c < H ? Z[r * kPinnZS + c] : 0.f;
                    acc = pinn_mfma(av, bv, acc);
                }
                if (c < H) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int ff = ft * 16 + 4 * kq + r;
                        if (ff < fan) {
                            float* dst = gp + a.offW[i] + (size_t)ff * sk + (size_t)c * sc;
                            *dst = first ? acc[r] : *dst + acc[r];
                        }
                    }
                }
            }
            // Adj[:, :fan] += Z (16 x H) . W_i^T (H x fan)   (the input's own adjoint is not needed)
            if (i > 0) {
                const int nks = (H + 3) >> 2;
                for (int ft = wave; ft < nft; ft += 4) {
                    const int f = ft * 16 + row;
                    const bool fok = f < fan;
                    pinn_f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
                    for (int ks = 0; ks < nks; ks += 2) {
                        const int c0 = ks * 4 + kq, c1 = c0 + 4;
                        const float a0 = c0 < H ? Z[row * kPinnZS + c0] : 0.f;
                        const float b0 = (c0 < H && fok) ? W[(size_t)f * sk + (size_t)c0 * sc] : 0.f;
                        const float a1 = c1 < H ? Z[row * kPinnZS + c1] : 0.f;
                        const float b1 = (c1 < H && fok) ? W[(size_t)f * sk + (size_t)c1 * sc] : 0.f;
                        acc0 = pinn_mfma(a0, b0, acc0);
                        acc1 = pinn_mfma(a1, b1, acc1);
                    }
                    if (fok) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) Adj[(4 * kq + r) * ast + f] += acc0[r] + acc1[r];
                    }
                }
            }
            __syncthreads();
        }
    }
}

// The (K, K) part of an h that reads t.  Wave w of workgroup g takes the samples j = 4 g + w, + 4 gridDim.x, ..
__global__ __launch_bounds__(kPinnThreads) void pinn_pair_kernel(const PinnPairArgs a) {
    extern __shared__ float pinn_lds[];                            // 2 tau t_i, i < K
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, K = a.K, d = a.d;
    for (int i = tid; i < K; i += kPinnThreads) pinn_lds[i] = a.tau2 * a.t[i];
    __syncthreads();
    const bool sq = a.h_kind == GH_EXPBALL_SQ, pair = sq || a.h_kind == GH_EXPBALL_SIN;
    for (int j = blockIdx.x * 4 + wave; j < K; j += gridDim.x * 4) {
        const float* x = a.x + (size_t)j * d;
        float rr = 0.f;
        for (int c = 0; c < d; ++c) rr = fmaf(x[c], x[c], rr);
        const float ex = 2.0f * a.al * rr, y = a.V[j], y2 = y * y, Aj = a.A[j];
        float sR = 0.f, sD = 0.f, sQ = 0.f;
        for (int i = lane; i < K; i += 64) {
            float R = Aj, dn = 0.f;
            if (pair) {
                const float arg = expf(ex + pinn_lds[i]) - y2;     // one exponential of the sum, as the reference takes it
                if (sq) { R += arg; dn = 1.f; }
                else { R += sinf(arg); dn = cosf(arg); }
            }
            sR += R;
            sQ = fmaf(R, R, sQ);
            sD = fmaf(R, dn, sD);
        }
        double q = (double)sQ;
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            sR += __shfl_xor(sR, m, 64);
            sD += __shfl_xor(sD, m, 64);
            q += __shfl_xor(q, m, 64);
        }
        if (lane == 0) {
            a.rho[j] = a.coef * sR;
            a.nu[j] = a.coef * (-2.0f * y) * sD;
            a.work[j] = q;
        }
    }
}

// One wave: the K per-sample sums of squares in index order, in double.
__global__ void pinn_pair_loss_kernel(const PinnPairArgs a) {
    __shared__ double part[64];
    const int lane = threadIdx.x, per = (a.K + 63) / 64;
    const int lo = lane * per, hi = lo + per < a.K ? lo + per : a.K;
    double s = 0.0;
    for (int j = lo; j < hi; ++j) s += a.work[j];
    part[lane] = s;
    __syncthreads();
    if (lane == 0) {
        double tot = 0.0;
        for (int l = 0; l < 64; ++l) tot += part[l];
        a.loss[0] = (float)(a.loss_coef * tot);
    }
}

#endif  // PSP_PINN_KERNELS

}  // namespace psp
