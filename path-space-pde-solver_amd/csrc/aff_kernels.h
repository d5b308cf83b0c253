// aff_kernels.h -- Solver.train with a linear, affine or constant control per time step (time_approx='outer', z_n a list of
// function_space.Linear / Affine / Constant): Z_n(x) = M_n x + c_n.  Compiled by aff_instance.hip for the d buckets 16, 32, 64.
//
// Three kernels:
//   aff_fwd_kernel  forward rollout (reference solver.py:449-486), one lane per trajectory
//   aff_adj_kernel  reverse-time adjoint sweep for gradients through the state path (detach_forward=False), one lane per trajectory
//   aff_bwd_kernel  dM_n = sum_k delta_{n,k} X_{n,k}^T, dc_n = sum_k delta_{n,k} per (time step, slice of trajectories)
//
// Why lanes and not MFMA tiles (hjbd_kernels.h): there is no net.  A step is one to four d x d products against ONE vector per
// trajectory; on gfx950 the fp32 vector and fp32 matrix peaks are equal, a 16x16x4 tile would have to move the state through
// LDS between products, and the sequential time loop leaves nothing to overlap it with.  This is the shape of hjbe_kernels.h:
// state, control and increment of a lane are DB floats in VGPRs, whatever all trajectories share (A, B, the maps and gains of the
// CURRENT step, the coefficient vectors) is read from LDS by broadcast.  The maps of all steps (N d^2 floats) stay in global
// memory and are staged step by step.  Products y = M x run row by row (row i from LDS against x in registers, y_i into a
// lane-private LDS column P); transposed products y = M^T v run as axpys over the same rows (v_i from the column, y in
// registers), so the sweep needs no transposed tables.
//
// Everything is zero padded to the bucket DB by the caller (maps, vectors, x0, supplied noise); components d .. DB-1 of the state
// stay exactly zero.  fp32 throughout, every accumulation sequential; (sum D, sum D^2) per workgroup in fp64 in lane order.
//
// Path store: one row of 2 DB floats per (step, trajectory), [X_n | image], rows of a step consecutive.  A lane writes and the
// sweep reads whole rows with 16-byte accesses; the gradient kernel streams a slice of rows into LDS as it lies in memory.
// image (psp_hjb_config.store_path): 1: xi, or xi + sqrt(dt) Z when the forward process is not adaptive; 2: xi - sqrt(dt) Z;
// 3: Z.  The sweep overwrites it with delta_n / sqrt(dt), so that aff_bwd_kernel (delta = w_k sqrt(dt) image) serves both.
#pragma once
#include "hjb_kernels.h"

namespace psp {

struct AffArgs {
    const float* x0;          // (DB) or (K_local, DB)
    const float* y0;          // optional device scalar
    const float* xi;          // supplied noise (N + 1, K_local, DB), slice n + 1 drives step n
    const float* drift;       // DENSE: A (DB x DB); DIAG: a (DB); DOUBLE_WELL: kappa (DB)
    const float* sigma;       // DENSE: B (DB x DB)
    const float* runcost;     // DIAG_QUAD: p (DB)
    const float* term;        // (DB)
    const float* M;           // (N, DB, DB) effective maps or null (Constant)
    const float* c;           // (N, DB) effective shifts or null (Linear)
    const float* uref;        // u_L2 log: TABLE (N, DB) u*(t_n); LINEAR (N, DB, DB) gains
    float* ul2;               // (K_local) or null: no log
    float* D;                 // (K_local)
    float* XN;                // (K_local, DB): written by the forward (optional), read by the sweep
    float* Yout;              // optional (K_local)
    double* fwd_partial;      // (grid, 2)
    float* path;              // (N, K_local, 2 DB)
    const float* mu;          // sweep: dL/dY_N
    const float* nu;          // sweep: dL/dZsum_N (optional)
    const float* wT;          // sweep: weight of grad g(X_N) in lambda_N (optional: nu - mu)
    const float* w;           // gradient: (K_local) trajectory weights
    float* partial;           // gradient: (N * slices, DB * DB + DB)
    long long k_offset;
    int d, K_local, N, x0_stride;
    int drift_kind, sigma_kind, runcost_kind, term_kind, adaptive, loss_kind, noise_mode, store_path, ul2_kind;
    int slices, slice_len, has_matrix;                             // gradient: a Constant has no outer products to sum
    float dt, sqdt, sigma_scale;
    uint32_t seed_lo, seed_hi, iter;
};

enum { AFF_UL2_OFF = -1, AFF_UL2_TABLE = 0, AFF_UL2_LINEAR = 1 };      // include/psp.h PSP_UL2_*
constexpr int kAffMaxThreads = 256;
constexpr int kAffBwdThreads = 256;
constexpr int kAffBwdChunk = 32;                                       // trajectories per LDS stage of the gradient kernel

// LDS layout in floats: [drift vector | running cost | terminal cost | c_n] (4 DB), dense A, dense B, M_n, the u_L2 data of the
// step (TABLE: DB, LINEAR: DB x DB), then the lane-private columns P (element i of thread t at P[i * threads + t])
struct AffLds { int A, B, M, G, P, total; };
__host__ __device__ inline AffLds aff_lds_layout(int DB, int threads, bool denseA, bool denseB, bool hasM, int ul2_kind) {
    AffLds L;
    L.A = 4 * DB;
    L.B = L.A + (denseA ? DB * DB : 0);
    L.M = L.B + (denseB ? DB * DB : 0);
    L.G = L.M + (hasM ? DB * DB : 0);
    L.P = L.G + (ul2_kind == AFF_UL2_LINEAR ? DB * DB : ul2_kind == AFF_UL2_TABLE ? DB : 0);
    L.total = L.P + DB * threads;
    return L;
}

template <int DB>
__device__ __forceinline__ float aff_dot(const float* __restrict__ Mrow, const float (&v)[DB]) {
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < DB; ++j) acc = fmaf(Mrow[j], v[j], acc);
    return acc;
}
// y += s * row
template <int DB>
__device__ __forceinline__ void aff_axpy(const float* __restrict__ Mrow, float s, float (&y)[DB]) {
#pragma unroll
    for (int j = 0; j < DB; ++j) y[j] = fmaf(Mrow[j], s, y[j]);
}

// b_i(x) of the element-wise drift kinds and its derivative (problems.py: DIAG a_i x; double well -4 kappa_i x (x^2 - 1))
__device__ __forceinline__ float aff_drift_elem(int kind, float xv, float c) {
    if (kind == DRIFT_DIAG) return c * xv;
    if (kind == DRIFT_DWELL) return -((4.0f * c) * (xv * (xv * xv - 1.0f)));
    return 0.f;
}
__device__ __forceinline__ float aff_drift_elem_dx(int kind, float xv, float c) {
    if (kind == DRIFT_DIAG) return c;
    if (kind == DRIFT_DWELL) return -((4.0f * c) * (3.0f * xv * xv - 1.0f));
    return 0.f;
}

// coefficient vectors and the dense matrices into LDS (once per workgroup; the caller synchronises)
template <int DB>
__device__ __forceinline__ void aff_stage_static(const AffArgs& a, float* lds, const AffLds& L, int tid, int T) {
    const bool denseA = a.drift_kind == DRIFT_DENSE, denseB = a.sigma_kind == SIGMA_DENSE;
    for (int i = tid; i < DB; i += T) {
        const bool in = i < a.d;
        lds[i] = (in && (a.drift_kind == DRIFT_DIAG || a.drift_kind == DRIFT_DWELL)) ? a.drift[i] : 0.f;
        lds[DB + i] = (in && a.runcost_kind == RUN_DIAGQ) ? a.runcost[i] : 0.f;
        lds[2 * DB + i] = in ? a.term[i] : 0.f;
        lds[3 * DB + i] = 0.f;
    }
    for (int i = tid; i < DB * DB; i += T) {
        const bool in = (i / DB) < a.d && (i % DB) < a.d;
        if (denseA) lds[L.A + i] = in ? a.drift[i] : 0.f;
        if (denseB) lds[L.B + i] = in ? a.sigma[i] : 0.f;
    }
}

template <int DB>
__global__ void __launch_bounds__(kAffMaxThreads) aff_fwd_kernel(AffArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, T = blockDim.x, d = a.d;
    const bool denseA = a.drift_kind == DRIFT_DENSE, denseB = a.sigma_kind == SIGMA_DENSE;
    const bool hasM = a.M != nullptr, hasC = a.c != nullptr;
    const int ukind = a.ul2 ? a.ul2_kind : AFF_UL2_OFF;
    const AffLds L = aff_lds_layout(DB, T, denseA, denseB, hasM, ukind);
    aff_stage_static<DB>(a, lds, L, tid, T);

    const long long k = (long long)blockIdx.x * T + tid;
    const bool kvalid = k < a.K_local;
    const long long kc = kvalid ? k : 0;
    const uint32_t kglob = (uint32_t)(a.k_offset + k);
    const float dt = a.dt, sqdt = a.sqdt, s = a.sigma_scale;
    const bool scaled = a.sigma_kind == SIGMA_SCALE, adaptive = a.adaptive != 0;

    float x[DB], z[DB], xi[DB];
    {
        const float* xr = a.x0 + (a.x0_stride ? kc * a.x0_stride : 0);
#pragma unroll
        for (int i = 0; i < DB; ++i) {
            const float v = xr[i < d ? i : d - 1];
            x[i] = i < d ? v : 0.f;
        }
    }
    float Y = a.y0 ? a.y0[0] : 0.f, Zs = 0.f, ul = 0.f;

    for (int n = 0; n < a.N; ++n) {
        // the static tables are re-read every step through opaque offsets: loop-invariant LDS reads would be hoisted out of the time
        // loop and kept live (hjbe_kernels.h)
        const float* sA = lds + opaque_i(L.A);
        const float* sB = lds + opaque_i(L.B);
        const float* sM = lds + opaque_i(L.M);
        const float* sG = lds + opaque_i(L.G);
        float* P = lds + opaque_i(L.P) + tid;                       // lane-private column: element i at P[i * T]
        const float* sv = lds + opaque_i(0);
        // ---- the maps of this step into LDS
        __syncthreads();                                            // every lane is done with the previous step's data
        if (hasM) {
            const float4* src = reinterpret_cast<const float4*>(a.M + (size_t)n * DB * DB);
            float4* dst = reinterpret_cast<float4*>(lds + L.M);
            for (int i = tid; i < DB * DB / 4; i += T) dst[i] = src[i];
        }
        if (tid < DB) lds[3 * DB + tid] = hasC ? a.c[(size_t)n * DB + tid] : 0.f;
        if (ukind == AFF_UL2_TABLE) {
            if (tid < DB) lds[L.G + tid] = a.uref[(size_t)n * DB + tid];
        } else if (ukind == AFF_UL2_LINEAR) {
            const float4* src = reinterpret_cast<const float4*>(a.uref + (size_t)n * DB * DB);
            float4* dst = reinterpret_cast<float4*>(lds + L.G);
            for (int i = tid; i < DB * DB / 4; i += T) dst[i] = src[i];
        }
        __syncthreads();

        // ---- Z = M_n X_n + c_n (solver.py:453)
        if (hasM) {
#pragma unroll 1
            for (int i = 0; i < d; ++i) P[i * T] = aff_dot<DB>(sM + i * DB, x);
        }
#pragma unroll
        for (int i = 0; i < DB; ++i) {
            float v = sv[3 * DB + i];
            if (hasM) {
                const float pv = P[i * T];
                v = v + (i < d ? pv : 0.f);
            }
            z[i] = i < d ? v : 0.f;
        }

        // ---- Brownian increment xi_{n+1}: supplied, or the Philox counters every rollout kernel uses
        if (a.noise_mode == NOISE_PHILOX) {
#pragma unroll
            for (int b = 0; b < (DB + 15) / 16; ++b)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    f32x4 r4 = {0.f, 0.f, 0.f, 0.f};
                    if (16 * b + q < d)
                        r4 = philox_block((uint32_t)opaque_i((int)kglob), (uint32_t)n, (uint32_t)opaque_i(4 * b + q), a.iter,
                                          a.seed_lo, a.seed_hi);
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int f = 16 * b + 4 * r + q;
                        xi[f] = f < d ? r4[r] : 0.f;
                    }
                }
        } else {
            const float* row = a.xi + ((size_t)(n + 1) * a.K_local + kc) * DB;
#pragma unroll
            for (int f = 0; f < DB; ++f) {
                const float v = row[f < d ? f : d - 1];
                xi[f] = f < d ? v : 0.f;
            }
        }

        float zz = 0.f, zx = 0.f;
#pragma unroll
        for (int i = 0; i < DB; ++i) {
            zz = fmaf(z[i], z[i], zz);
            zx = fmaf(z[i], xi[i], zx);
        }

        // ---- path store: [X_n | image]
        if (a.store_path && kvalid) {
            f32x4* row = reinterpret_cast<f32x4*>(a.path + ((size_t)n * a.K_local + k) * (2 * DB));
#pragma unroll
            for (int i = 0; i < DB; i += 4) {
                f32x4 vx, vi;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    vx[r] = x[i + r];
                    float im;
                    if (a.store_path == 3) im = z[i + r];
                    else if (a.store_path == 2) im = xi[i + r] - sqdt * z[i + r];
                    else im = adaptive ? xi[i + r] : xi[i + r] + sqdt * z[i + r];
                    vi[r] = im;
                }
                PSP_PATH_STORE(row + i / 4, vx);
                PSP_PATH_STORE(row + (DB + i) / 4, vi);
            }
        }

        // ---- Euler-Maruyama step (solver.py:455-469): w = xi sqrt(dt) + c dt, c = -Z (adaptive) or 0; X += b(X) dt + B w
#pragma unroll
        for (int j = 0; j < DB; ++j) xi[j] = adaptive ? fmaf(-z[j], dt, xi[j] * sqdt) : xi[j] * sqdt;
        if (denseB) {
#pragma unroll
            for (int j = 0; j < DB; ++j) P[j * T] = x[j];
#pragma unroll 1
            for (int i = 0; i < d; ++i) {
                const float xv = P[i * T];
                const float b = denseA ? aff_dot<DB>(sA + i * DB, x) : aff_drift_elem(a.drift_kind, xv, sv[i]);
                P[i * T] = (xv + b * dt) + aff_dot<DB>(sB + i * DB, xi);
            }
#pragma unroll
            for (int i = 0; i < DB; ++i) {
                const float v = P[i * T];
                x[i] = i < d ? v : 0.f;
            }
        } else {
            if (denseA) {
#pragma unroll 1
                for (int i = 0; i < d; ++i) P[i * T] = aff_dot<DB>(sA + i * DB, x);
            }
#pragma unroll
            for (int i = 0; i < DB; ++i) {
                float b;
                if (denseA) {
                    const float v = P[i * T];
                    b = i < d ? v : 0.f;
                } else {
                    b = aff_drift_elem(a.drift_kind, x[i], sv[i]);
                }
                x[i] = (x[i] + b * dt) + (scaled ? s * xi[i] : xi[i]);
            }
        }

        // ---- Y and Zsum (solver.py:471-476): h sees the updated state
        float f = 0.f;
        if (a.runcost_kind == RUN_DIAGQ) {
#pragma unroll
            for (int i = 0; i < DB; ++i) f = fmaf(x[i], sv[DB + i] * x[i], f);
        }
        const float run = 0.5f * zz + f;
        Y = Y + (run + (adaptive ? -zz : 0.f)) * dt + zx * sqdt;
        Zs = Zs + run * dt;

        // ---- u_L2 log (solver.py:479-481): |-Z_n(X_n) - u*(X_{n+1}, t_n)|^2 dt
        if (ukind == AFF_UL2_TABLE) {
            float e2 = 0.f;
#pragma unroll
            for (int i = 0; i < DB; ++i) {
                const float e = -z[i] - sG[i];
                e2 = fmaf(e, e, e2);
            }
            ul = fmaf(e2, dt, ul);
        } else if (ukind == AFF_UL2_LINEAR) {
#pragma unroll 1
            for (int i = 0; i < d; ++i) P[i * T] = aff_dot<DB>(sG + i * DB, x);
            float e2 = 0.f;
#pragma unroll
            for (int i = 0; i < DB; ++i) {
                const float pv = P[i * T];
                const float e = -z[i] - (i < d ? pv : 0.f);
                e2 = fmaf(e, e, e2);
            }
            ul = fmaf(e2, dt, ul);
        }
    }

    // ---- terminal cost and D = Y - g(X_N)   (PSP_LOSS_REL_ENTROPY: Y = -Zsum, include/psp.h)
    float g = 0.f;
#pragma unroll
    for (int i = 0; i < DB; ++i) {
        const float tv = lds[2 * DB + i], xv = x[i];
        if (a.term_kind == TERM_LINEAR) g = fmaf(tv, xv, g);
        else if (a.term_kind == TERM_DIAGQ) g = fmaf(xv, tv * xv, g);
        else { const float e = xv - 1.0f; g = fmaf(tv, e * e, g); }
    }
    const float Yf = a.loss_kind == LOSS_RELENT ? -Zs : Y;
    const float Dk = Yf - g;
    if (kvalid) {
        a.D[k] = Dk;
        if (a.Yout) a.Yout[k] = Yf;
        if (a.ul2) a.ul2[k] = ul;
        if (a.XN) {
            float4* row = reinterpret_cast<float4*>(a.XN + (size_t)k * DB);
#pragma unroll
            for (int i = 0; i < DB; i += 4) row[i / 4] = make_float4(x[i], x[i + 1], x[i + 2], x[i + 3]);
        }
    }
    // ---- (sum D, sum D^2) of the workgroup in fp64, lane order
    __syncthreads();
    double* sd = reinterpret_cast<double*>(lds);
    sd[tid] = kvalid ? (double)Dk : 0.0;
    __syncthreads();
    if (tid == 0) {
        double s1 = 0.0, s2 = 0.0;
        for (int t = 0; t < T; ++t) { const double v = sd[t]; s1 += v; s2 += v * v; }
        a.fwd_partial[2 * blockIdx.x] = s1;
        a.fwd_partial[2 * blockIdx.x + 1] = s2;
    }
}

// Adjoint sweep (include/psp.h psp_aff_adjoint_sweep).  Per trajectory, with mu = dL/dY_N, nu = dL/dZsum_N and
// lambda_N = wT grad g(X_N), for n = N-1 .. 0:
//     Lam     = lambda + (mu + nu) dt grad f(X_{n+1})
//     delta_n = mu sqrt(dt) (xi - sqrt(dt) Z_n) + nu dt Z_n - dt B^T Lam        (store_path 2 keeps the first image, 3 the second)
//     lambda  = Lam + dt J_b(X_n)^T Lam + M_n^T delta_n
// and the image slot of step n becomes delta_n / sqrt(dt).
template <int DB>
__global__ void __launch_bounds__(kAffMaxThreads) aff_adj_kernel(AffArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, T = blockDim.x, d = a.d;
    const bool denseA = a.drift_kind == DRIFT_DENSE, denseB = a.sigma_kind == SIGMA_DENSE;
    const bool hasM = a.M != nullptr;
    const AffLds L = aff_lds_layout(DB, T, denseA, denseB, hasM, AFF_UL2_OFF);
    aff_stage_static<DB>(a, lds, L, tid, T);
    __syncthreads();

    const long long k = (long long)blockIdx.x * T + tid;
    const bool kvalid = k < a.K_local;
    const long long kc = kvalid ? k : 0;
    const float dt = a.dt, sqdt = a.sqdt, s = a.sigma_scale;
    const bool scaled = a.sigma_kind == SIGMA_SCALE;
    const float mu = a.mu[kc], nu = a.nu ? a.nu[kc] : 0.f;
    const float wT = a.wT ? a.wT[kc] : nu - mu;
    const float isq = 1.0f / sqdt;

    float lam[DB], y[DB];
    {
        const float* xN = a.XN + (size_t)kc * DB;
#pragma unroll
        for (int i = 0; i < DB; ++i) {
            const float tv = lds[2 * DB + i], xv = xN[i];
            float gg;
            if (a.term_kind == TERM_LINEAR) gg = tv;
            else if (a.term_kind == TERM_DIAGQ) gg = 2.0f * tv * xv;
            else gg = 2.0f * tv * (xv - 1.0f);
            lam[i] = i < d ? wT * gg : 0.f;
        }
    }

    for (int n = a.N - 1; n >= 0; --n) {
        const float* sA = lds + opaque_i(L.A);
        const float* sB = lds + opaque_i(L.B);
        const float* sM = lds + opaque_i(L.M);
        float* P = lds + opaque_i(L.P) + tid;
        const float* sv = lds + opaque_i(0);
        if (hasM) {
            __syncthreads();
            const float4* src = reinterpret_cast<const float4*>(a.M + (size_t)n * DB * DB);
            float4* dst = reinterpret_cast<float4*>(lds + L.M);
            for (int i = tid; i < DB * DB / 4; i += T) dst[i] = src[i];
            __syncthreads();
        }
        float* row = a.path + ((size_t)n * a.K_local + kc) * (2 * DB);
        const float* xnext = n == a.N - 1 ? a.XN + (size_t)kc * DB : row + (size_t)a.K_local * (2 * DB);

        // ---- Lam = lambda + (mu + nu) dt grad f(X_{n+1})
        if (a.runcost_kind == RUN_DIAGQ) {
            const float cf = (mu + nu) * dt * 2.0f;
#pragma unroll
            for (int i = 0; i < DB; ++i) lam[i] = fmaf(cf * sv[DB + i], xnext[i], lam[i]);
        }
        if (denseA || denseB) {
#pragma unroll
            for (int i = 0; i < DB; ++i) P[i * T] = lam[i];
        }
        // ---- y = B^T Lam
        if (denseB) {
#pragma unroll
            for (int j = 0; j < DB; ++j) y[j] = 0.f;
#pragma unroll 1
            for (int i = 0; i < d; ++i) aff_axpy<DB>(sB + i * DB, P[i * T], y);
        } else {
#pragma unroll
            for (int j = 0; j < DB; ++j) y[j] = scaled ? s * lam[j] : lam[j];
        }
        // ---- lambda <- Lam + dt J_b(X_n)^T Lam
        if (denseA) {
#pragma unroll 1
            for (int i = 0; i < d; ++i) aff_axpy<DB>(sA + i * DB, dt * P[i * T], lam);
        } else if (a.drift_kind != DRIFT_ZERO) {
#pragma unroll
            for (int i = 0; i < DB; ++i) lam[i] = fmaf(dt * aff_drift_elem_dx(a.drift_kind, row[i], sv[i]), lam[i], lam[i]);
        }
        // ---- delta_n from the stored image; the slot becomes delta_n / sqrt(dt)
        const float ci = a.store_path == 3 ? nu * dt : mu * sqdt;
#pragma unroll
        for (int j = 0; j < DB; ++j) {
            const float de = fmaf(ci, row[DB + j], -dt * y[j]);
            y[j] = j < d ? de : 0.f;
        }
        if (kvalid) {
#pragma unroll
            for (int j = 0; j < DB; j += 4)
                reinterpret_cast<float4*>(row + DB)[j / 4] = make_float4(y[j] * isq, y[j + 1] * isq, y[j + 2] * isq, y[j + 3] * isq);
        }
        // ---- lambda += M_n^T delta_n
        if (hasM) {
#pragma unroll
            for (int j = 0; j < DB; ++j) P[j * T] = y[j];
#pragma unroll 1
            for (int i = 0; i < d; ++i) aff_axpy<DB>(sM + i * DB, P[i * T], lam);
        }
    }
}

// Gradient reduction: work item (step n, slice s of the trajectories); thread (ti, tj) of 16 x 16 owns the R x R block of dM_n at
// rows ti R .., columns tj R .. (R = DB / 16) and sums its trajectories sequentially; column 0 threads also keep dc_n.  The rows
// of the path store are streamed through LDS kAffBwdChunk trajectories at a time exactly as they lie in memory, the image half
// scaled by w_k sqrt(dt) on the way in.  partial: (N * slices, DB * DB + DB); the caller sums the slices of a step in order.
template <int DB>
__global__ void __launch_bounds__(kAffBwdThreads) aff_bwd_kernel(AffArgs a) {
    constexpr int R = DB / 16, ROW = 2 * DB, KC = kAffBwdChunk;
    __shared__ __attribute__((aligned(16))) float sh[KC * ROW];
    const int tid = threadIdx.x;
    const int n = blockIdx.x / a.slices, sl = blockIdx.x % a.slices;
    const int k0 = min(a.K_local, sl * a.slice_len), k1 = min(a.K_local, k0 + a.slice_len);
    const int ti = tid / 16, tj = tid % 16;
    const bool hasM = a.has_matrix != 0;
    float acc[R][R], accb[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        accb[r] = 0.f;
#pragma unroll
        for (int q = 0; q < R; ++q) acc[r][q] = 0.f;
    }
    const float* base = a.path + (size_t)n * a.K_local * ROW;
    for (int kb = k0; kb < k1; kb += KC) {
        __syncthreads();
        for (int e = tid; e < KC * ROW / 4; e += kAffBwdThreads) {
            const int kk = e / (ROW / 4), c4 = e % (ROW / 4), k = kb + kk;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (k < k1) {
                v = reinterpret_cast<const float4*>(base + (size_t)k * ROW)[c4];
                if (c4 >= DB / 4) {
                    const float sc = a.w[k] * a.sqdt;
                    v.x *= sc; v.y *= sc; v.z *= sc; v.w *= sc;
                }
            }
            reinterpret_cast<float4*>(sh)[e] = v;
        }
        __syncthreads();
#pragma unroll 4
        for (int kk = 0; kk < KC; ++kk) {
            float dv[R], xv[R];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                dv[r] = sh[kk * ROW + DB + ti * R + r];
                xv[r] = sh[kk * ROW + tj * R + r];
            }
#pragma unroll
            for (int r = 0; r < R; ++r) {
                accb[r] += dv[r];
                if (hasM) {
#pragma unroll
                    for (int q = 0; q < R; ++q) acc[r][q] = fmaf(dv[r], xv[q], acc[r][q]);
                }
            }
        }
    }
    float* out = a.partial + (size_t)blockIdx.x * (DB * DB + DB);
#pragma unroll
    for (int r = 0; r < R; ++r) {
#pragma unroll
        for (int q = 0; q < R; ++q) out[(ti * R + r) * DB + tj * R + q] = acc[r][q];
        if (tj == 0) out[DB * DB + ti * R + r] = accb[r];
    }
}

// aff_instance.hip: the three kernels of one d bucket
struct AffInstance {
    hipError_t (*launch_fwd)(const AffArgs&, int grid, int threads, int lds_bytes, hipStream_t);
    hipError_t (*launch_adj)(const AffArgs&, int grid, int threads, int lds_bytes, hipStream_t);
    hipError_t (*launch_bwd)(const AffArgs&, int grid, hipStream_t);
};
AffInstance aff_instance_16();
AffInstance aff_instance_32();
AffInstance aff_instance_64();

}  // namespace psp
