// genl_eval_kernels.h -- the K_test_log diagnostic of GeneralSolver / EllipticSolver on the device (reference
// utilities.py:440-472 compute_test_error; solver.py:1193-1197 / :821-825): K fresh points of the domain, the value net V and the
// problem's closed-form solution v_true on them, and the three error statistics of the log -- sampled, evaluated and reduced
// without the host.  Forward only: one 16-point tile per workgroup, V through genl_value() of genl_kernels.h on tables of the
// current parameters (any dense-concat net those kernels take), so the LDS holds the activation image A alone (TB KiB instead
// of the rollout's 2 TB: no gradient image) and as many tiles fit a CU as its wave slots allow.
//
// Points.  Supplied (x (K, d), t (K) row-major), or drawn from Philox4x32-7 on a stream of their own:
//     key     = (seed & 0xffffffff, (seed >> 32) ^ 0x54455354)       -- every training stream uses (seed_lo, seed_hi) itself
//     counter = (global point index k_offset + k, c1, c2, iter)
//     c1 = 0, c2 = 4 b + q : the four outputs are features 16 b + 4 r + q, r = 0..3 (the T layout of the rollout's noise):
//                            normals through normal4 for the ball kinds, 24-bit uniforms ((r >> 8) + 1/2) 2^-24 for the box
//     c1 = 1, c2 = 0       : output 0 = the radial uniform u, output 1 = the time uniform u_t (t = u_t T, with a time input)
//     TS_BALL(R)      x = R g / |g| u^(1/d)                          ('sphere', 'unbounded')
//     TS_ANNULUS      the ball of radius r2; a point with |x| <= r1 is rejected: it contributes nothing and is not counted
//                     (the reference's X[selection], 'two_spheres')
//     TS_BOX(l, r)    x = (r - l) u + l                              ('square', 'unbounded_square')
// v_true in fp32 from r2 = |x|^2 and t (|x|^2 itself is summed in fp64 -- the squares of fp32 values are exact there -- because
// the committor solution vanishes on the inner sphere: a^2 - r^(2-d) a^d = -a^2 expm1((2 - d) log(r / a)) with
// log(r / a) = log1p((r2 - a^2) / a^2) / 2 keeps its relative accuracy there only if r2 - a^2 is formed before rounding to fp32).
// Statistics per kept point, e = (double) v_true - (double) V: sum e^2, sum |e|, sum |e| / v_true (the reference's formula, signs
// and infinities included) and the count, in fp64; one partial per workgroup, summed in a fixed order by genl_eval_reduce_kernel
// into log_out[4 slot .. 4 slot + 3].  Equal arguments give bit-identical output.
#pragma once
#include "genl_kernels.h"

namespace psp {

enum { TS_SUPPLIED = 0, TS_BALL = 1, TS_ANNULUS = 2, TS_BOX = 3 };
enum { VT_EXP = 0, VT_QUAD = 1, VT_COMMITTOR = 2,
       // the solutions of the exit-time and box problems (problems.py:1611, :1654, :1693, :1730), a group of its own from 16 on:
       // the kernel hands them the coordinates x_0, x_1 beside r2
       VT_LOGQ = 16,                   // log((r2 + 1) / p0)
       VT_SINPROD = 17,                // sin(p0 x_0) sin(p1 x_1)
       VT_SINSUM = 18,                 // sin(p0 x_0) + p2 sin(p1 x_0)
       VT_SINR2 = 19 };                // sin(pi r2)
constexpr uint32_t kTestKeyXor = 0x54455354u;
constexpr int kEvalStats = 4;

struct GenlEvalArgs {
    GenlArgs n;                     // the net (make_genl_plan): tables, n.g.params, shapes; nothing of the rollout is read
    const float* x;                 // TS_SUPPLIED: (K, d)
    const float* t;                 // TS_SUPPLIED with a time input: (K)
    long long k_offset;
    int K;
    int sample_kind;                // TS_*
    float lo, hi;                   // BALL: hi = R; ANNULUS: r1, r2; BOX: l, r
    float T;
    int vtrue_kind;                 // VT_*
    float vp[4];
    float vden;                     // VT_COMMITTOR: a^2 - c^(2-d) a^d (formed in double on the host)
    uint32_t key0, key1, iter;
    double* partial;                // (gridDim.x, 4)
    double* log_out;                // (log_slots, 4)
    const uint32_t* slot_dev;       // optional device slot index (a psp_iter_state.iter); NULL: `slot`
    int slot, log_slots;
    float* x_out; float* t_out; float* v_out; float* vtrue_out; int* keep_out;   // optional per-point dumps
};

__host__ __device__ inline int genl_eval_lds_bytes(int TB) { return TB * 1024; }

// all launches of a call (genl_eval_instance.hip, the one unit that defines the kernels below); nw = 1 or 8
hipError_t genl_eval_launch(const GenlEvalArgs& a, int nw, int grid, int lds_bytes, hipStream_t stream);

#ifdef PSP_GENL_EVAL_KERNELS
__device__ __forceinline__ float uniform24(uint32_t r) {             // ((r >> 8) + 1/2) 2^-24, as normal4 forms it
    return __builtin_fmaf((float)(r >> 8), 1.0f / 16777216.0f, 0.5f / 16777216.0f);
}

template <int NW>
__global__ __launch_bounds__(64 * NW) void genl_eval_kernel(const GenlEvalArgs ea_) {
    const GenlEvalArgs* ea = &ea_;
    const KArgs ga = &ea->n;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* A = lds;
    const float* __restrict__ T = ga->tables;
    const int lane = threadIdx.x & 63, j = lane & 15, q = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const bool w0 = wave == 0;                                       // every wave carries the tile's points; wave 0 writes
    const int D = ga->d, DB0 = ga->DB0;
    const int k = blockIdx.x * 16 + j;
    const bool kvalid = k < ea->K;
    const int kind = ea->sample_kind;

    // ---- a. the points: lane (j, q) holds features 16 b + 4 r + q of point j; padded features and points are zero
    f32x4 X[GENL_MAXDB];
    float tval = 0.f;
    if (kind == TS_SUPPLIED) {
#pragma unroll
        for (int b = 0; b < GENL_MAXDB; ++b)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int f = 16 * b + 4 * r + q;
                const float v = (b < DB0) ? ea->x[(size_t)(kvalid ? k : 0) * D + (f < D ? f : D - 1)] : 0.f;
                X[b][r] = (f < D && kvalid) ? v : 0.f;
            }
        if (kvalid && ga->has_time) tval = ea->t[k];
    } else {
        const bool box = kind == TS_BOX;
        const uint32_t kglob = (uint32_t)(ea->k_offset + k);
        const int DBx = (D + 15) >> 4;                               // blocks that hold a state feature (the time may add one)
        float gg = 0.f;
#pragma unroll
        for (int b = 0; b < GENL_MAXDB; ++b) {
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (b < DBx) {
                uint32_t rr[4];
                philox4x32_R(kglob, 0u, (uint32_t)(4 * b + q), ea->iter, ea->key0, ea->key1, rr);
                if (box) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) v[r] = (ea->hi - ea->lo) * uniform24(rr[r]) + ea->lo;
                } else {
                    v = normal4(rr);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    v[r] = ((16 * b + 4 * r + q) < D && kvalid) ? v[r] : 0.f;
                    gg = fmaf(v[r], v[r], gg);
                }
            }
            X[b] = v;
        }
        uint32_t ru[4];
        philox4x32_R(kglob, 1u, 0u, ea->iter, ea->key0, ea->key1, ru);
        if (ga->has_time && kvalid) tval = uniform24(ru[1]) * ea->T;
        if (!box) {
            gg = qsum(gg);
            const float sc = kvalid ? ea->hi * expf(logf(uniform24(ru[0])) / (float)D) / sqrtf(gg) : 0.f;
#pragma unroll
            for (int b = 0; b < GENL_MAXDB; ++b) X[b] = sc * X[b];
        }
    }
    double r2d = 0.0;                                                // |x|^2 (header comment)
#pragma unroll
    for (int b = 0; b < GENL_MAXDB; ++b)
#pragma unroll
        for (int r = 0; r < 4; ++r) r2d = fma((double)X[b][r], (double)X[b][r], r2d);
    r2d += __shfl_xor(r2d, 16);
    r2d += __shfl_xor(r2d, 32);
    const float r2 = (float)r2d;
    const bool keep = kvalid && (kind != TS_ANNULUS || sqrtf(r2) > ea->lo);
    // coordinates 0 and 1 (lanes q = 0, 1; taken before the time joins the image: with d = 1 it is feature 1)
    const float xc0 = qsum(q == 0 ? X[0][0] : 0.f), xc1 = qsum(q == 1 ? X[0][0] : 0.f);

    if (w0) {                                                        // dumps: the points as the net sees them
        if (ea->x_out && kvalid) {
#pragma unroll
            for (int b = 0; b < GENL_MAXDB; ++b)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int f = 16 * b + 4 * r + q;
                    if (b < DB0 && f < D) ea->x_out[(size_t)k * D + f] = X[b][r];
                }
        }
        if (ea->t_out && kvalid && q == 0) ea->t_out[k] = tval;
    }
    if (ga->has_time) {                                              // the time is input feature D
        const int TBq = D >> 4, TRq = (D & 15) >> 2, TQq = D & 3;
#pragma unroll
        for (int b = 0; b < GENL_MAXDB; ++b)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (b == TBq && r == TRq && q == TQq) X[b][r] = tval;
    }
    if (w0) {
#pragma unroll
        for (int b = 0; b < GENL_MAXDB; ++b) if (b < DB0) img_put(A, b, X[b], lane);
    }
    tile_sync<NW>();

    // ---- b. V: the hidden segments of A are written whole by genl_value, nothing of the image is read before it is written
    f32x4 Rr[GenlGeo<NW>::MAXSLOT];
#pragma unroll
    for (int s = 0; s < GenlGeo<NW>::MAXSLOT; ++s) Rr[s] = f32x4{0.f, 0.f, 0.f, 0.f};
    const float V = genl_value<NW>(ga, T, A, Rr, lane, q, wave);
    if (!w0) return;                                                 // (no barrier below)

    // ---- c. v_true
    float vt;
    if (ea->vtrue_kind == VT_EXP) {
        vt = expf(fmaf(ea->vp[0], r2, ea->vp[1] * tval));
    } else if (ea->vtrue_kind == VT_QUAD) {
        vt = r2 + ea->vp[0] * (ea->vp[1] - tval);
    } else if (ea->vtrue_kind == VT_LOGQ) {
        vt = logf((r2 + 1.0f) / ea->vp[0]);
    } else if (ea->vtrue_kind == VT_SINPROD) {
        vt = sinf(ea->vp[0] * xc0) * sinf(ea->vp[1] * xc1);
    } else if (ea->vtrue_kind == VT_SINSUM) {
        vt = sinf(ea->vp[0] * xc0) + ea->vp[2] * sinf(ea->vp[1] * xc0);
    } else if (ea->vtrue_kind == VT_SINR2) {
        vt = sinf(3.14159265358979323846f * r2);
    } else {
        const float a2 = ea->vp[0] * ea->vp[0];
        const float delta = (float)(r2d - (double)ea->vp[0] * (double)ea->vp[0]);
        const float lr = 0.5f * log1pf(delta / a2);                  // log(r / a)
        vt = -a2 * expm1f((2.0f - ea->vp[2]) * lr) / ea->vden;
    }
    // ---- d. statistics of the kept points; a rejected or padded point enters as an exact zero
    const double e = (double)vt - (double)V, ae = fabs(e);
    const double s0 = jsum(keep ? e * e : 0.0), s1 = jsum(keep ? ae : 0.0), s2 = jsum(keep ? ae / (double)vt : 0.0),
                 s3 = jsum(keep ? 1.0 : 0.0);
    if (lane == 0) {
        double* p = ea->partial + (size_t)blockIdx.x * kEvalStats;
        p[0] = s0; p[1] = s1; p[2] = s2; p[3] = s3;
    }
    if (kvalid && q == 0) {
        if (ea->v_out) ea->v_out[k] = V;
        if (ea->vtrue_out) ea->vtrue_out[k] = vt;
        if (ea->keep_out) ea->keep_out[k] = keep ? 1 : 0;
    }
}

// partials -> log_out[4 slot + s]: one wave per statistic, lane i sums partials i, i + 64, .. in order, then a butterfly.
__global__ __launch_bounds__(64 * kEvalStats) void genl_eval_reduce_kernel(const double* __restrict__ part, int n, double* __restrict__ log_out,
                                                                    const uint32_t* __restrict__ slot_dev, int slot, int log_slots) {
    constexpr int NS = kEvalStats;
    const int lane = threadIdx.x & 63, s = threadIdx.x >> 6;
    double a = 0.0;
    for (int i = lane; i < n; i += 64) a += part[(size_t)i * NS + s];
    for (int o = 1; o < 64; o <<= 1) a += __shfl_xor(a, o);
    const long long sl = slot_dev ? (long long)*slot_dev : (long long)slot;
    if (lane == 0 && sl >= 0 && sl < log_slots) log_out[sl * NS + s] = a;       // a slot outside the log is dropped, never written
}

#endif  // PSP_GENL_EVAL_KERNELS

}  // namespace psp
