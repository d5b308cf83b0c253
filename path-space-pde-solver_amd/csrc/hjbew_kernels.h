// hjbew_kernels.h -- the wide-state twin of hjbe_kernels.h: the forward-only evaluation rollout under the problem's reference
// control u* or under no control (psp_is_config, include/psp.h) for run-time d up to kIswMaxD.  Compiled by hjbew_instance.hip.
//
// One wave owns one 16-trajectory tile; a workgroup is four waves (four tiles).  The state sits feature-major in the accumulator
// layout of v_mfma_f32_16x16x4_f32 (the T layout of hjb_kernels.h): lane (j, q) = j + 16 q holds X[b][r] = feature 16 b + 4 r + q
// of trajectory j, so the result of one product is the operand of the next without a transpose.  The dense products A X,
// B (u dt + xi sqrt(dt)) and M_n X are fp32 MFMAs whose A operands come from a pre-tiled scratch in global memory (L2-resident,
// every element fetched feeds 16 trajectories) that isw_tables_kernel writes once per call: the per-feature vectors, A and B
// once, the TABLE rows / the gains M_n once per step n.  LDS holds the current step's GRID rows and nothing else.
//
// Arithmetic: as hjbe_rollout_kernel -- fp32, no fma contraction in the elementwise parts, so an elementwise drift, an identity
// or scaled sigma and a control of kind NONE / TABLE / GRID round the state update op by op as the reference's torch ops do.  The
// sums over features (u.xi, |u|^2, f, g) run over the lane's own features in ascending order and then over the four lanes of a
// trajectory as (q0 + q1) + (q2 + q3): a fixed order, no atomics, equal arguments give equal bits -- but not the narrow
// kernel's order.
//
// Registers: X, u and xi (which also takes A X, then v) are DB f32x4 each (DB = 16-feature blocks of the bucket), plus two panels
// of A operands in flight.  The step applies the drift half of the update before it draws the noise, so that no fourth array is
// live; at DB = 16 (d <= 256) every instance is free of scratch on the 512 registers one wave per SIMD has (the compiler's
// kernel-resource-usage report).  DB = 32 (d = 512) is 128 registers per array, 384 before a panel or a temporary, and was not
// brought under 512 without scratch: kIswMaxD = 256.
#pragma once
#include "hjbe_kernels.h"

namespace psp {

constexpr int kIswMaxD = 256;
constexpr int kIswWaves = 4, kIswThreads = 64 * kIswWaves;

// the compiled buckets: 4, 8, 12 or 16 blocks of 16 features
__host__ __device__ constexpr int isw_bucket(int d) {
    const int nb = (d + 15) / 16;
    return nb <= 4 ? 4 : nb <= 8 ? 8 : nb <= 12 ? 12 : 16;
}

// The scratch in floats, P = 16 DB padded features: five vectors [x0 | drift | running cost | terminal cost | grid group (int)]
// in the layout of stage_vec, A and B (P x P each, when dense), then per step n the TABLE row (P) or the gain M_n (P x P).
// A matrix is tiled as [((mb DB + b) 64 + lane) 4 + r] = M(16 mb + 4 (i & 3) + (i >> 2), 16 b + 4 r + q), lane = i + 16 q: one
// 16-byte load per lane is the A operand of the four k-steps of input block b for output block mb.
struct IswTables { long long A, B, U, total; int P; };
__host__ __device__ inline IswTables isw_table_layout(int d, int N, int ctrl, bool denseA, bool denseB) {
    IswTables L;
    L.P = 16 * isw_bucket(d);
    const long long PP = (long long)L.P * L.P;
    L.A = 5 * L.P;
    L.B = L.A + (denseA ? PP : 0);
    L.U = L.B + (denseB ? PP : 0);
    L.total = L.U + (ctrl == ISC_TABLE ? (long long)N * L.P : ctrl == ISC_LINEAR ? (long long)N * PP : 0);
    return L;
}

struct IswArgs {
    IsArgs a;
    float* tab;               // the scratch (isw_table_layout)
    IswTables L;
};

// (a template so that the header can be included by more than one unit)
template <int UNUSED = 0>
__global__ void __launch_bounds__(256) isw_tables_kernel(IswArgs w) {
    const IsArgs& a = w.a;
    const int d = a.d, P = w.L.P, DB = P / 16;
    const long long PP = (long long)P * P;
    const long long stride = (long long)gridDim.x * blockDim.x, t0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    auto tiled = [&](const float* M, long long idx) {
        const int r = (int)(idx & 3), lane = (int)((idx >> 2) & 63);
        const int t = (int)(idx >> 8), b = t % DB, mb = t / DB;
        const int i = lane & 15, q = lane >> 4;
        const int row = 16 * mb + 4 * (i & 3) + (i >> 2), col = 16 * b + 4 * r + q;
        return (row < d && col < d) ? M[(size_t)row * d + col] : 0.f;
    };
    // feature of slot idx of a stage_vec vector
    auto feat = [](int idx) { return 16 * (idx >> 4) + 4 * (idx & 3) + ((idx >> 2) & 3); };
    for (long long idx = t0; idx < P; idx += stride) {
        const int f = feat((int)idx);
        const bool in = f < d;
        w.tab[idx] = in ? a.x0[f] : 0.f;
        w.tab[P + idx] = (in && (a.drift_kind == DRIFT_DIAG || a.drift_kind == DRIFT_DWELL)) ? a.drift[f] : 0.f;
        w.tab[2 * P + idx] = (in && a.runcost_kind == RUN_DIAGQ) ? a.runcost[f] : 0.f;
        w.tab[3 * P + idx] = in ? a.term[f] : 0.f;
        reinterpret_cast<int*>(w.tab)[4 * P + idx] = (in && a.ctrl == ISC_GRID) ? min(max(a.ugroup[f], 0), a.u_ntables - 1) : 0;
    }
    if (a.drift_kind == DRIFT_DENSE)
        for (long long idx = t0; idx < PP; idx += stride) w.tab[w.L.A + idx] = tiled(a.drift, idx);
    if (a.sigma_kind == SIGMA_DENSE)
        for (long long idx = t0; idx < PP; idx += stride) w.tab[w.L.B + idx] = tiled(a.sigma, idx);
    if (a.ctrl == ISC_TABLE) {
        for (long long idx = t0; idx < (long long)a.N * P; idx += stride) {
            const long long n = idx / P;
            const int f = feat((int)(idx - n * P));
            w.tab[w.L.U + idx] = f < d ? a.uref[(size_t)n * d + f] : 0.f;
        }
    } else if (a.ctrl == ISC_LINEAR) {
        for (long long idx = t0; idx < (long long)a.N * PP; idx += stride) {
            const long long n = idx / PP;
            w.tab[w.L.U + idx] = tiled(a.uref + (size_t)n * d * d, idx - n * PP);
        }
    }
}

// acc (DB output blocks) += M (tiled table in global memory) . in, over the input blocks that hold a feature < d.
// A panel is the A operands of one input block for CH output blocks (CH 16-byte loads; CH = DB up to 8 blocks, DB / 2 above, so
// that two panels in flight stay at 64 registers); the next panel is fetched before the MFMAs of the current one issue, and
// consecutive MFMAs go to different accumulators.
template <int DB>
__device__ __forceinline__ void isw_gemm(f32x4 (&acc)[DB], const float* __restrict__ tab, const f32x4 (&in)[DB], int lane, int d) {
    constexpr int CH = DB <= 8 ? DB : DB / 2, NH = DB / CH;
    const f32x4* t4 = reinterpret_cast<const f32x4*>(tab) + opaque_i(lane);
    f32x4 w[2][CH];
#pragma unroll
    for (int m = 0; m < CH; ++m) w[0][m] = t4[(m * DB) * 64];
#pragma unroll
    for (int p = 0; p < DB * NH; ++p) {
        const int b = p / NH, h = p % NH;
        if (16 * b < d) {
            const int b1 = (p + 1) / NH, h1 = (p + 1) % NH;
            if (p + 1 < DB * NH && 16 * b1 < d) {
#pragma unroll
                for (int m = 0; m < CH; ++m) w[(p + 1) & 1][m] = t4[((h1 * CH + m) * DB + b1) * 64];
            }
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int m = 0; m < CH; ++m) acc[h * CH + m] = mfma16(w[p & 1][m][r], in[b][r], acc[h * CH + m]);
        }
    }
}

// After every fourth block of an elementwise loop nothing may be scheduled across: without it the loads of all DB blocks (group
// indices, coefficients) are issued up front and kept live, which at DB = 16 costs the registers the state needs.
__device__ __forceinline__ void isw_fence(int b) {
    if ((b & 3) == 3) __builtin_amdgcn_sched_barrier(0);
}

// sum over the four lanes (q = 0 .. 3) that hold one trajectory: (q0 + q1) + (q2 + q3) in every lane
__device__ __forceinline__ float isw_sum_q(float v) {
    v = v + __shfl_xor(v, 16);
    return v + __shfl_xor(v, 32);
}

template <int DB, int CTRL>
__global__ void __launch_bounds__(kIswThreads) isw_rollout_kernel(IswArgs w) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) float lds[];        // GRID: the current step's rows (G x ncols)
    const IsArgs& a = w.a;
    const int tid = threadIdx.x, lane = tid & 63, j = lane & 15, q = lane >> 4;
    const int d = a.d, P = w.L.P;
    const bool denseA = a.drift_kind == DRIFT_DENSE, denseB = a.sigma_kind == SIGMA_DENSE;
    const float* __restrict__ tab = w.tab;

    const long long k = ((long long)blockIdx.x * kIswWaves + (tid >> 6)) * 16 + j;
    const bool kvalid = k < a.K_local;
    const long long kread = kvalid ? k : a.K_local - 1;               // lanes past the end compute a copy and store nothing
    const uint32_t kglob = (uint32_t)(a.k_offset + kread);
    const bool last = kvalid && a.k_offset + k == a.K_global - 1;     // the reference's i[-1] -= 2 (GRID)
    const float dt = a.dt, sqdt = a.sqdt, s = a.sigma_scale;
    const bool scaled = a.sigma_kind == SIGMA_SCALE;

    f32x4 X[DB], xi[DB], u[DB];
#pragma unroll
    for (int b = 0; b < DB; ++b) {
        X[b] = *reinterpret_cast<const f32x4*>(tab + (b * 4 + q) * 4);
        u[b] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    float fint = 0.f, ito = 0.f, riem = 0.f;

    for (int n = 0; n < a.N; ++n) {
        // per-step base of the vectors (opaque: loop-invariant loads would be hoisted out of the time loop and kept live)
        const float* vec = tab + opaque_i((q * 4));
        // (and the lane's q for the feature masks f < d: 64 hoisted compare results would be spilled to register lanes)
        const int qn = opaque_i(q);
        // ---- the GRID rows of this step into LDS
        if constexpr (CTRL == ISC_GRID) {
            __syncthreads();                                          // every wave is done with the previous step's rows
            const int row = min(max(a.urow[n], 0), a.u_nrows - 1);
            const int nc = a.u_ncols, tot = a.u_ntables * nc;
            for (int i = tid; i < tot; i += kIswThreads) {
                const int g = i / nc, c = i - g * nc;
                lds[i] = a.uref[((size_t)g * a.u_nrows + row) * nc + c];
            }
            __syncthreads();
        }

        // ---- control u = u*(X_n, t_n), taken BEFORE the update
        if constexpr (CTRL == ISC_TABLE) {
            const float* ut = vec + w.L.U + (long long)n * P;
#pragma unroll
            for (int b = 0; b < DB; ++b) u[b] = *reinterpret_cast<const f32x4*>(ut + b * 16);
        } else if constexpr (CTRL == ISC_LINEAR) {
#pragma unroll
            for (int b = 0; b < DB; ++b) u[b] = f32x4{0.f, 0.f, 0.f, 0.f};
            isw_gemm<DB>(u, tab + w.L.U + (long long)n * P * P, X, lane, d);
        } else if constexpr (CTRL == ISC_GRID) {
            const int nc = a.u_ncols;
#pragma unroll
            for (int b = 0; b < DB; ++b) {
                const int4 grp = *reinterpret_cast<const int4*>(vec + 4 * P + b * 16);
                const int g4[4] = {grp.x, grp.y, grp.z, grp.w};
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float v = 0.f;
                    if (16 * b + 4 * r + qn < d) v = lds[g4[r] * nc + ugrid_cell(X[b][r], a.u_xb, a.u_xhi, a.u_dx, last, nc)];
                    u[b][r] = v;
                }
                isw_fence(b);
            }
        }

        // ---- Euler-Maruyama step, drift half: X <- X + (b(X) + s u) dt (dense sigma: X + b(X) dt), before the noise exists, so
        // that the accumulators of A X and the noise never live at the same time.  Per element the operations and their order
        // are those of hjbe_rollout_kernel.  b_i(X_n) of the elementwise kinds:
        auto drift_elem = [&](float xv, float c) __attribute__((always_inline)) {
            if (a.drift_kind == DRIFT_DIAG) return c * xv;
            if (a.drift_kind == DRIFT_DWELL) {
                const float k4 = 4.0f * c;
                return a.dwell_form ? -((k4 * xv) * (xv * xv - 1.0f)) : -(k4 * (xv * (xv * xv - 1.0f)));
            }
            return 0.f;
        };
        if (denseA) {
#pragma unroll
            for (int b = 0; b < DB; ++b) xi[b] = f32x4{0.f, 0.f, 0.f, 0.f};
            isw_gemm<DB>(xi, tab + w.L.A, X, lane, d);
        }
#pragma unroll
        for (int b = 0; b < DB; ++b) {
            const f32x4 c = *reinterpret_cast<const f32x4*>(vec + P + b * 16);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float bb = denseA ? xi[b][r] : drift_elem(X[b][r], c[r]);
                if (CTRL != ISC_NONE && !denseB) bb = bb + (scaled ? s * u[b][r] : u[b][r]);
                X[b][r] = X[b][r] + bb * dt;
            }
            isw_fence(b);
        }

        // ---- Brownian increment xi_{n+1}: supplied, or the Philox counters of psp_hjb_rollout_eval / psp_is_rollout
        if (a.noise_mode == NOISE_PHILOX) {
#pragma unroll
            for (int b = 0; b < DB; ++b) {
                f32x4 z = {0.f, 0.f, 0.f, 0.f};
                if (16 * b < d)
                    z = philox_block((uint32_t)opaque_i((int)kglob), (uint32_t)n, (uint32_t)opaque_i(4 * b + q), a.iter, a.seed_lo,
                                     a.seed_hi);
#pragma unroll
                for (int r = 0; r < 4; ++r) xi[b][r] = 16 * b + 4 * r + qn < d ? z[r] : 0.f;
            }
        } else {
            // (a block that lies inside d whole reads at immediate offsets from one base; only the ragged block selects)
            const float* row = a.xi + ((size_t)(n + 1) * a.K_local + kread) * d + qn;
#pragma unroll
            for (int b = 0; b < DB; ++b) {
                if (16 * b + 16 <= d) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) xi[b][r] = row[16 * b + 4 * r];
                } else {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const bool in = 16 * b + 4 * r + qn < d;
                        const float v = row[in ? 16 * b + 4 * r : -qn];
                        xi[b][r] = in ? v : 0.f;
                    }
                }
            }
        }

        // ---- Girsanov sums: sum(u xi) sqrt(dt), sum(u^2) dt
        if constexpr (CTRL != ISC_NONE) {
            float pu = 0.f, uu = 0.f;
#pragma unroll
            for (int b = 0; b < DB; ++b)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    pu = pu + u[b][r] * xi[b][r];
                    uu = uu + u[b][r] * u[b][r];
                }
            ito = ito + isw_sum_q(pu) * sqdt;
            riem = riem + isw_sum_q(uu) * dt;
        }

        // ---- Euler-Maruyama step, noise half
        if (denseB) {
            // + B (u dt + xi sqrt(dt)): v in xi, B v in u
#pragma unroll
            for (int b = 0; b < DB; ++b)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    xi[b][r] = (CTRL != ISC_NONE) ? (u[b][r] * dt + xi[b][r] * sqdt) : xi[b][r] * sqdt;
                    u[b][r] = 0.f;
                }
            isw_gemm<DB>(u, tab + w.L.B, xi, lane, d);
#pragma unroll
            for (int b = 0; b < DB; ++b)
#pragma unroll
                for (int r = 0; r < 4; ++r) X[b][r] = X[b][r] + u[b][r];
        } else {
            // sigma = s I: + (s xi) sqrt(dt)
#pragma unroll
            for (int b = 0; b < DB; ++b)
#pragma unroll
                for (int r = 0; r < 4; ++r) X[b][r] = X[b][r] + (scaled ? s * xi[b][r] : xi[b][r]) * sqdt;
        }

        // ---- running cost f(X_{n+1}, t_n) dt (the state AFTER the update)
        if (a.runcost_kind == RUN_DIAGQ) {
            float f = 0.f;
#pragma unroll
            for (int b = 0; b < DB; ++b) {
                const f32x4 p = *reinterpret_cast<const f32x4*>(vec + 2 * P + b * 16);
#pragma unroll
                for (int r = 0; r < 4; ++r) f = f + X[b][r] * (p[r] * X[b][r]);
                isw_fence(b);
            }
            fint = fint + isw_sum_q(f) * dt;
        }
    }

    // ---- terminal cost g(X_N) and the log-weight
    float g = 0.f;
#pragma unroll
    for (int b = 0; b < DB; ++b) {
        const f32x4 t = *reinterpret_cast<const f32x4*>(tab + 3 * P + (b * 4 + q) * 4);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float tv = t[r], xv = X[b][r];
            if (a.term_kind == TERM_LINEAR) g = g + tv * xv;
            else if (a.term_kind == TERM_DIAGQ) g = g + xv * (tv * xv);
            else { const float e = xv - 1.0f; g = g + tv * (e * e); }
        }
    }
    g = isw_sum_q(g);
    if (kvalid) {
        if (q == 0) {
            float lw = -fint - g;
            if constexpr (CTRL != ISC_NONE) lw = (lw - ito) - 0.5f * riem;
            a.logw[k] = lw;
        }
        if (a.XN) {
#pragma unroll
            for (int b = 0; b < DB; ++b)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int f = 16 * b + 4 * r + q;
                    if (f < d) a.XN[(size_t)k * d + f] = X[b][r];
                }
        }
    }
}

// hjbew_instance.hip: the table kernel, then the (bucket, control kind) instance of the rollout on the same stream
hipError_t isw_rollout_launch(const IswArgs& w, int grid, int lds_bytes, hipStream_t stream);

}  // namespace psp
