// hjbe_kernels.h -- forward-only evaluation rollout under the problem's REFERENCE control u* or under no control at all, for the
// importance-sampling estimators of utilities.do_importance_sampling_me (reference utilities.py:287-359): control='true' (IS with
// u*) and simulate_naive=True (plain Monte Carlo on the uncontrolled process).  Compiled by hjbe_instance.hip.
//
// One lane per trajectory; the state, the increment and the control of a lane are DB floats in VGPRs (DB = the d bucket, 1, 4,
// 16, 32 or 64; components d .. DB-1 stay exactly zero: zero noise, zero control, zero coefficients).  There is no net here, and
// on gfx950 the fp32 vector and fp32 matrix peaks are equal, so the matrix pipe has nothing to offer at d <= 64.  Everything that
// is the same for all trajectories -- the coefficient vectors, dense A and B, the gains M_n and the current rows of the grid
// tables -- sits in LDS and is read by broadcast (every lane of a wave reads the same address, except the grid lookup).
//
// Arithmetic: fp32, every accumulation sequential in n.  The whole kernel body is compiled WITHOUT fma contraction, so that the
// elementwise drift / sigma kinds round the state update op by op as the torch ops of the reference do
//     X <- X + (b(X) + s u) dt + (s xi) sqrt(dt)
// and a grid lookup of u* sees the same X as the composite plan on the same noise.  The dense products (A X, B v, M_n X) are
// sequential fma chains; their summation order is not torch's anyway.
#pragma once
#include "hjb_kernels.h"
#include "ugrid.h"

namespace psp {

enum { ISC_NONE = 0, ISC_TABLE = 1, ISC_LINEAR = 2, ISC_GRID = 3 };     // include/psp.h PSP_ISC_*

struct IsArgs {
    const float* x0;          // (d) initial state, broadcast
    const float* xi;          // supplied noise (N + 1, K_local, d), slice n + 1 drives step n
    const float* drift;       // DENSE: A (d x d); DIAG: a (d); DOUBLE_WELL: kappa (d)
    const float* sigma;       // DENSE: B (d x d)
    const float* runcost;     // DIAG_QUAD: p (d)
    const float* term;        // (d)
    const float* uref;        // TABLE: (N, d) u*(t_n); LINEAR: (N, d, d) M_n; GRID: (G, nrows, ncols) tables
    const int* ugroup;        // GRID: (d) table of every coordinate
    const int* urow;          // GRID: (N) table row of step n
    float* logw;              // (K_local) -int f dt - g(X_N) - int u.dW - 0.5 int |u|^2 dt
    float* XN;                // optional (K_local, d)
    long long k_offset, K_global;
    int d, K_local, N, ctrl;
    int drift_kind, sigma_kind, runcost_kind, term_kind, noise_mode, dwell_form;
    int u_ntables, u_nrows, u_ncols;
    float dt, sqdt, sigma_scale, u_xb, u_dx, u_xhi;
    uint32_t seed_lo, seed_hi, iter;
};

constexpr int kIsThreads = 256;

// the compiled d buckets (native range d <= 64)
constexpr int kIsMaxD = 64;
__host__ __device__ constexpr int is_bucket(int d) { return d <= 1 ? 1 : d <= 4 ? 4 : d <= 16 ? 16 : d <= 32 ? 32 : 64; }

// LDS layout in floats: [drift vector | running cost | terminal cost | grid group (int)] (4 DB), dense A, dense B, u* data of the
// current step (TABLE: DB, LINEAR: DB x DB, GRID: G x ncols), then a lane-private column of DB floats per thread (P: the rows of
// the broadcast products land there, element i of thread t at P[i * kIsThreads + t]) when a product is needed
struct IsLds { int A, B, U, P, total; };
__host__ __device__ inline IsLds is_lds_layout(int DB, int ctrl, bool denseA, bool denseB, int ntables, int ncols) {
    IsLds L;
    L.A = 4 * DB;
    L.B = L.A + (denseA ? DB * DB : 0);
    L.U = L.B + (denseB ? DB * DB : 0);
    const int u = ctrl == ISC_TABLE ? DB : ctrl == ISC_LINEAR ? DB * DB : ctrl == ISC_GRID ? ntables * ncols : 0;
    L.P = L.U + u;
    L.total = L.P + ((ctrl == ISC_LINEAR || denseA || denseB) ? DB * kIsThreads : 0);
    return L;
}

// The broadcast products y = M x run ROW BY ROW in a loop that is not unrolled: row i reads M[i][0 .. DB) from LDS (every lane
// the same address, DB / 4 ds_read_b128 at immediate offsets) against the lane's x[0 .. DB) in registers and writes y_i to the
// lane-private column P.  Fully unrolled DB x DB products made the register allocation blow up (256 VGPRs plus AGPR spills at
// DB = 16, scratch at DB = 32 / 64); this shape keeps the three per-lane arrays and one row in registers.
template <int DB>
__device__ __forceinline__ float row_dot(const float* __restrict__ Mrow, const float (&v)[DB]) {
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < DB; ++j) acc = fmaf(Mrow[j], v[j], acc);
    return acc;
}

template <int DB, int CTRL>
__global__ void __launch_bounds__(kIsThreads) hjbe_rollout_kernel(IsArgs a) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x;
    const int d = a.d;
    const bool denseA = a.drift_kind == DRIFT_DENSE, denseB = a.sigma_kind == SIGMA_DENSE;
    const IsLds L = is_lds_layout(DB, CTRL, denseA, denseB, a.u_ntables, a.u_ncols);
    float* sdr = lds;
    float* srun = lds + DB;
    float* sterm = lds + 2 * DB;
    int* sgrp = reinterpret_cast<int*>(lds + 3 * DB);
    float* sU = lds + L.U;

    // ---- coefficients (once per workgroup)
    for (int i = tid; i < DB; i += kIsThreads) {
        float vd = 0.f, vr = 0.f, vt = 0.f;
        int gr = 0;
        if (i < d) {
            if (a.drift_kind == DRIFT_DIAG || a.drift_kind == DRIFT_DWELL) vd = a.drift[i];
            if (a.runcost_kind == RUN_DIAGQ) vr = a.runcost[i];
            vt = a.term[i];
            if (CTRL == ISC_GRID) gr = min(max(a.ugroup[i], 0), a.u_ntables - 1);
        }
        sdr[i] = vd; srun[i] = vr; sterm[i] = vt; sgrp[i] = gr;
    }
    for (int i = tid; i < DB * DB; i += kIsThreads) {
        const int r = i / DB, c = i % DB;
        const bool in = r < d && c < d;
        if (denseA) lds[L.A + i] = in ? a.drift[in ? r * d + c : 0] : 0.f;
        if (denseB) lds[L.B + i] = in ? a.sigma[in ? r * d + c : 0] : 0.f;
    }

    const long long k = (long long)blockIdx.x * kIsThreads + tid;
    const bool kvalid = k < a.K_local;
    const uint32_t kglob = (uint32_t)(a.k_offset + k);
    const bool last = a.k_offset + k == a.K_global - 1;           // the reference's i[-1] -= 2 (GRID)
    const float dt = a.dt, sqdt = a.sqdt, s = a.sigma_scale;
    const bool scaled = a.sigma_kind == SIGMA_SCALE;

    float x[DB], xi[DB], u[DB];
#pragma unroll
    for (int i = 0; i < DB; ++i) {
        const float v = a.x0[i < d ? i : d - 1];
        x[i] = i < d ? v : 0.f;
        u[i] = 0.f;
    }
    float fint = 0.f, ito = 0.f, riem = 0.f;
    if (CTRL == ISC_NONE) __syncthreads();                        // (the controlled kinds synchronise at the top of every step)

    for (int n = 0; n < a.N; ++n) {
        // the staged tables are re-read every step (opaque offsets): loop-invariant LDS reads would be hoisted out of the time
        // loop and kept live
        const float* sA = lds + opaque_i(L.A);
        const float* sB = lds + opaque_i(L.B);
        float* P = lds + opaque_i(L.P) + tid;                     // lane-private column: element i at P[i * kIsThreads]
        const float* sv = lds + opaque_i(0);
        const float* sdrn = sv;
        const float* srunn = sv + DB;
        const int* sgrpn = reinterpret_cast<const int*>(sv + 3 * DB);
        // ---- u* data of this step into LDS
        if constexpr (CTRL != ISC_NONE) {
            __syncthreads();                                      // every lane is done with the previous step's data
            if constexpr (CTRL == ISC_TABLE) {
                for (int i = tid; i < DB; i += kIsThreads) sU[i] = i < d ? a.uref[(size_t)n * d + i] : 0.f;
            } else if constexpr (CTRL == ISC_LINEAR) {
                const float* M = a.uref + (size_t)n * d * d;
                for (int i = tid; i < DB * DB; i += kIsThreads) {
                    const int r = i / DB, c = i % DB;
                    sU[i] = (r < d && c < d) ? M[(r < d && c < d) ? r * d + c : 0] : 0.f;
                }
            } else {
                const int row = min(max(a.urow[n], 0), a.u_nrows - 1);
                const int nc = a.u_ncols, tot = a.u_ntables * nc;
                for (int i = tid; i < tot; i += kIsThreads) {
                    const int g = i / nc, c = i - g * nc;
                    sU[i] = a.uref[((size_t)g * a.u_nrows + row) * nc + c];
                }
            }
            __syncthreads();
        }

        // ---- control u = u*(X_n, t_n), taken BEFORE the update (utilities.py:322)
        if constexpr (CTRL == ISC_TABLE) {
#pragma unroll
            for (int i = 0; i < DB; ++i) u[i] = sU[i];
        } else if constexpr (CTRL == ISC_LINEAR) {
#pragma unroll 1
            for (int i = 0; i < d; ++i) P[i * kIsThreads] = row_dot<DB>(sU + i * DB, x);
#pragma unroll
            for (int i = 0; i < DB; ++i) {
                const float v = P[i * kIsThreads];
                u[i] = i < d ? v : 0.f;
            }
        } else if constexpr (CTRL == ISC_GRID) {
            const int nc = a.u_ncols;
#pragma unroll
            for (int i = 0; i < DB; ++i) {
                float v = 0.f;
                if (i < d) v = sU[sgrpn[i] * nc + ugrid_cell(x[i], a.u_xb, a.u_xhi, a.u_dx, last, nc)];
                u[i] = v;
            }
        }

        // ---- Brownian increment xi_{n+1} (utilities.py:310): supplied, or the Philox counters of psp_hjb_rollout_eval
        if (a.noise_mode == NOISE_PHILOX) {
#pragma unroll
            for (int b = 0; b < (DB + 15) / 16; ++b)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    if (16 * b + q >= DB) continue;               // (compile time) a call that only feeds padding
                    f32x4 z = {0.f, 0.f, 0.f, 0.f};
                    // (opaque counters: the rounds' loop-invariant parts would be hoisted out of the time loop and kept live)
                    if (16 * b + q < d)
                        z = philox_block((uint32_t)opaque_i((int)kglob), (uint32_t)n, (uint32_t)opaque_i(4 * b + q), a.iter,
                                         a.seed_lo, a.seed_hi);
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int f = 16 * b + 4 * r + q;
                        if (f < DB) xi[f] = f < d ? z[r] : 0.f;
                    }
                }
        } else {
            const float* row = a.xi + ((size_t)(n + 1) * a.K_local + (kvalid ? k : 0)) * d;
#pragma unroll
            for (int f = 0; f < DB; ++f) {
                const float v = row[f < d ? f : d - 1];
                xi[f] = f < d ? v : 0.f;
            }
        }

        // ---- Girsanov sums (utilities.py:325-326): sum(u xi) sqrt(dt), sum(u^2) dt
        if constexpr (CTRL != ISC_NONE) {
            float pu = 0.f, uu = 0.f;
#pragma unroll
            for (int i = 0; i < DB; ++i) {
                pu = pu + u[i] * xi[i];
                uu = uu + u[i] * u[i];
            }
            ito = ito + pu * sqdt;
            riem = riem + uu * dt;
        }

        // ---- Euler-Maruyama step (utilities.py:313, 323-324).  b_i(X_n) of the elementwise kinds:
        auto drift_elem = [&](float xv, float c) __attribute__((always_inline)) {
            if (a.drift_kind == DRIFT_DIAG) return c * xv;
            if (a.drift_kind == DRIFT_DWELL) {
                // b = -grad V: DoubleWell_multidim 4 kappa_i (x (x^2 - 1)); DoubleWell ((4 kappa) x) (x^2 - 1) (problems.py)
                const float k4 = 4.0f * c;
                return a.dwell_form ? -((k4 * xv) * (xv * xv - 1.0f)) : -(k4 * (xv * (xv * xv - 1.0f)));
            }
            return 0.f;
        };
        if (denseB) {
            // X + b(X) dt + B (u dt + xi sqrt(dt)): v in xi; row i reads its own x_i from the lane-private copy and writes
            // X_{n+1,i} over it
#pragma unroll
            for (int j = 0; j < DB; ++j) {
                xi[j] = (CTRL != ISC_NONE) ? (u[j] * dt + xi[j] * sqdt) : xi[j] * sqdt;
                P[j * kIsThreads] = x[j];
            }
#pragma unroll 1
            for (int i = 0; i < d; ++i) {
                const float xv = P[i * kIsThreads];
                const float b = denseA ? row_dot<DB>(sA + i * DB, x) : drift_elem(xv, sdrn[i]);
                P[i * kIsThreads] = (xv + b * dt) + row_dot<DB>(sB + i * DB, xi);
            }
#pragma unroll
            for (int i = 0; i < DB; ++i) {
                const float v = P[i * kIsThreads];
                x[i] = i < d ? v : 0.f;
            }
        } else {
            // sigma = s I: X <- (X + (b(X) + s u) dt) + (s xi) sqrt(dt), op by op; a dense A X first, row by row into P
            if (denseA) {
#pragma unroll 1
                for (int i = 0; i < d; ++i) P[i * kIsThreads] = row_dot<DB>(sA + i * DB, x);
            }
#pragma unroll
            for (int i = 0; i < DB; ++i) {
                float b;
                if (denseA) {
                    const float v = P[i * kIsThreads];
                    b = i < d ? v : 0.f;
                } else {
                    b = drift_elem(x[i], sdrn[i]);
                }
                if constexpr (CTRL != ISC_NONE) b = b + (scaled ? s * u[i] : u[i]);
                x[i] = (x[i] + b * dt) + (scaled ? s * xi[i] : xi[i]) * sqdt;
            }
        }

        // ---- running cost f(X_{n+1}, t_n) dt (utilities.py:314, 327: the state AFTER the update)
        if (a.runcost_kind == RUN_DIAGQ) {
            float f = 0.f;
#pragma unroll
            for (int i = 0; i < DB; ++i) f = f + x[i] * (srunn[i] * x[i]);
            fint = fint + f * dt;
        }
    }

    // ---- terminal cost g(X_N) (problems.py:49, 164, 334) and the log-weight
    float g = 0.f;
#pragma unroll
    for (int i = 0; i < DB; ++i) {
        const float tv = sterm[i], xv = x[i];
        if (a.term_kind == TERM_LINEAR) g = g + tv * xv;
        else if (a.term_kind == TERM_DIAGQ) g = g + xv * (tv * xv);
        else { const float e = xv - 1.0f; g = g + tv * (e * e); }
    }
    if (kvalid) {
        float lw = -fint - g;
        if constexpr (CTRL != ISC_NONE) lw = (lw - ito) - 0.5f * riem;
        a.logw[k] = lw;
        if (a.XN) {
#pragma unroll
            for (int i = 0; i < DB; ++i)
                if (i < d) a.XN[(size_t)k * d + i] = x[i];
        }
    }
}

// hjbe_instance.hip: every (bucket, control kind) instance; lds_bytes = 4 * is_lds_layout(..).total
hipError_t is_rollout_launch(const IsArgs& a, int grid, int lds_bytes, hipStream_t stream);

}  // namespace psp
