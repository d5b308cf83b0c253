// Statistics of the loss estimators over per-trajectory (Y_N, D = Y_N - g(X_N)) in double (psp_loss_stats_*, include/psp.h):
// what utilities.loss_relative_errors reduces its chunks with.  Per trajectory the samples are
//     terminal exp(-g)    cross-entropy Y exp(-g)    detached cross-entropy Y exp(-g + Y)    the same restricted to |v| < 100
//     moment D^2          and D itself up to its fourth central moment                        (g = Y - D, exact in double)
// A call adds one chunk to a device-resident state of mergeable moments (count, mean, M2; for D also M3, M4) in three launches:
//     lstat_sum_kernel     per-workgroup sums of the samples                                   -> partA
//     lstat_centred_kernel chunk means from partA (every workgroup sums it in the same order), then per-workgroup power sums
//                          of the samples about those means                                    -> partB
//     lstat_merge_kernel   one workgroup: chunk means again, partB in index order, the first-order correction of the rounded
//                          mean, and the merge of the chunk into the state (Chan et al. / Pebay update formulas)
// The chunk is read twice (8 B per trajectory each time; the second read finds it in L2 / MALL).  Every sum has a fixed order:
// a strided per-thread sum, a butterfly over the 64 lanes, the waves of a workgroup in index order, the workgroups in index
// order.  The grid depends on n alone, so equal calls give equal bits.  No atomics, plain vector loads and stores only.
// Stands alone: the HIP runtime is all it needs.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace psp {

constexpr int kLstatThreads = 256;
constexpr int kLstatPerWg = 2048;        // trajectories a workgroup takes before the grid stops growing
constexpr int kLstatMaxWg = 512;
constexpr int kLstatNV = 5;              // three-moment accumulators: terminal, CE, CE detached, its selection, moment
constexpr int kLstatNA = 7;              // partA: sums of the five samples, selection count, sum of D
constexpr int kLstatNB = 14;             // partB: (S1, S2) of the five samples, S1 .. S4 of D
// state, in doubles: accumulator a < 5 at [8 a]: n, mean, M2;  D at [40]: n, mean, M2, M3, M4;  [48 .. 55]: the chunk's means
// and counts between the kernels of one call;  then partA (kLstatMaxWg x kLstatNA) and partB (kLstatMaxWg x kLstatNB)
constexpr int kLstatHead = 56;
constexpr int kLstatDBase = 40;
constexpr int kLstatStateDoubles = kLstatHead + kLstatMaxWg * (kLstatNA + kLstatNB);
constexpr double kLstatSelect = 100.0;

struct LstatArgs {
    const float* Y;
    const float* D;
    int64_t n;
    double* state;
    int G;
};

inline int lstat_grid(int64_t n) {
    const int64_t g = (n + kLstatPerWg - 1) / kLstatPerWg;
    return g < 1 ? 1 : (g > kLstatMaxWg ? kLstatMaxWg : (int)g);
}

hipError_t lstat_launch_accumulate(const LstatArgs& a, hipStream_t stream);
hipError_t lstat_launch_finish(const double* state, double* out, hipStream_t stream);

#ifdef PSP_LSTAT_KERNELS

struct LstatSample { double v[kLstatNV]; double d; bool sel; };

__device__ __forceinline__ LstatSample lstat_sample(float y32, float d32) {
    LstatSample s;
    const double y = (double)y32, d = (double)d32;
    const double g = y - d;
    const double t = exp(-g);
    s.v[0] = t;
    s.v[1] = y * t;
    s.v[2] = y * exp(-g + y);
    s.v[3] = s.v[2];
    s.v[4] = d * d;
    s.d = d;
    s.sel = fabs(s.v[2]) < kLstatSelect;               // false for NaN and inf, as the boolean mask of the notebook
    return s;
}

// sum of NV per-thread values over the workgroup: lanes by butterfly, then the waves in index order; thread 0 holds the result
template <int NV>
__device__ __forceinline__ void lstat_block_sum(double (&acc)[NV], double* lds) {
    constexpr int kWaves = kLstatThreads / 64;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        double x = acc[i];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) x += __shfl_xor(x, off, 64);
        acc[i] = x;
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    __syncthreads();
    if (lane == 0)
        for (int i = 0; i < NV; ++i) lds[wave * NV + i] = acc[i];
    __syncthreads();
    if (threadIdx.x == 0)
        for (int i = 0; i < NV; ++i) {
            double x = lds[i];
            for (int w = 1; w < kWaves; ++w) x += lds[w * NV + i];
            acc[i] = x;
        }
}

// the chunk's counts and means from partA, workgroups in index order: m[0 .. 4] the five samples, m[5] D; cnt[0] n, cnt[1] selected
__device__ __forceinline__ void lstat_chunk_means(const LstatArgs& a, double* lds_m) {
    const double* partA = a.state + kLstatHead;
    if (threadIdx.x < kLstatNA) {
        double x = partA[threadIdx.x];
        for (int g = 1; g < a.G; ++g) x += partA[g * kLstatNA + threadIdx.x];
        lds_m[8 + threadIdx.x] = x;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double n = (double)a.n, ns = lds_m[8 + 5];
        for (int i = 0; i < kLstatNV; ++i) lds_m[i] = lds_m[8 + i] / (i == 3 ? ns : n);     // ns = 0: NaN, and no sample reads it
        lds_m[5] = lds_m[8 + 6] / n;
        lds_m[6] = n;
        lds_m[7] = ns;
    }
    __syncthreads();
}

__global__ __launch_bounds__(kLstatThreads) void lstat_sum_kernel(LstatArgs a) {
    __shared__ double lds[(kLstatThreads / 64) * kLstatNA];
    double acc[kLstatNA] = {0, 0, 0, 0, 0, 0, 0};
    const int64_t stride = (int64_t)a.G * kLstatThreads;
    for (int64_t k = (int64_t)blockIdx.x * kLstatThreads + threadIdx.x; k < a.n; k += stride) {
        const LstatSample s = lstat_sample(a.Y[k], a.D[k]);
        acc[0] += s.v[0]; acc[1] += s.v[1]; acc[2] += s.v[2]; acc[4] += s.v[4];
        if (s.sel) { acc[3] += s.v[3]; acc[5] += 1.0; }
        acc[6] += s.d;
    }
    lstat_block_sum<kLstatNA>(acc, lds);
    if (threadIdx.x == 0) {
        double* out = a.state + kLstatHead + (int64_t)blockIdx.x * kLstatNA;
        for (int i = 0; i < kLstatNA; ++i) out[i] = acc[i];
    }
}

__global__ __launch_bounds__(kLstatThreads) void lstat_centred_kernel(LstatArgs a) {
    __shared__ double lds[(kLstatThreads / 64) * kLstatNB];
    __shared__ double m[16];
    lstat_chunk_means(a, m);
    double mean[kLstatNV + 1];
    for (int i = 0; i <= kLstatNV; ++i) mean[i] = m[i];
    double acc[kLstatNB] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    const int64_t stride = (int64_t)a.G * kLstatThreads;
    for (int64_t k = (int64_t)blockIdx.x * kLstatThreads + threadIdx.x; k < a.n; k += stride) {
        const LstatSample s = lstat_sample(a.Y[k], a.D[k]);
#pragma unroll
        for (int i = 0; i < kLstatNV; ++i) {
            if (i == 3 && !s.sel) continue;
            const double c = s.v[i] - mean[i];
            acc[2 * i] += c;
            acc[2 * i + 1] += c * c;
        }
        const double c = s.d - mean[5], c2 = c * c;
        acc[10] += c; acc[11] += c2; acc[12] += c2 * c; acc[13] += c2 * c2;
    }
    lstat_block_sum<kLstatNB>(acc, lds);
    if (threadIdx.x == 0) {
        double* out = a.state + kLstatHead + kLstatMaxWg * kLstatNA + (int64_t)blockIdx.x * kLstatNB;
        for (int i = 0; i < kLstatNB; ++i) out[i] = acc[i];
    }
}

// mean of the union; an infinite mean (a sample overflowed) stays infinite instead of meeting itself as inf - inf
__device__ __forceinline__ double lstat_merged_mean(double na, double ma, double nb, double mb) {
    const double delta = mb - ma;
    return isfinite(delta) ? ma + delta * (nb / (na + nb)) : (na * ma + nb * mb) / (na + nb);
}

// S1 / n, the distance from the rounded mean to the chunk's mean; 0 where the sums are not finite (the mean is then inf or NaN as it is)
__device__ __forceinline__ double lstat_mean_shift(double S1, double n) { return isfinite(S1) ? S1 / n : 0.0; }

// the chunk (nb, mb, M2b) into (n, mean, M2) at acc[0 .. 2]
__device__ __forceinline__ void lstat_merge3(double* acc, double nb, double mb, double M2b) {
    if (nb == 0.0) return;
    const double na = acc[0], n = na + nb, delta = mb - acc[1];
    acc[0] = n;
    acc[1] = na == 0.0 ? mb : lstat_merged_mean(na, acc[1], nb, mb);
    acc[2] = na == 0.0 ? M2b : acc[2] + M2b + delta * delta * (na * nb / n);
}

__global__ __launch_bounds__(kLstatThreads) void lstat_merge_kernel(LstatArgs a) {
    __shared__ double m[16];
    __shared__ double S[kLstatNB];
    lstat_chunk_means(a, m);
    const double* partB = a.state + kLstatHead + kLstatMaxWg * kLstatNA;
    if (threadIdx.x < kLstatNB) {
        double x = partB[threadIdx.x];
        for (int g = 1; g < a.G; ++g) x += partB[g * kLstatNB + threadIdx.x];
        S[threadIdx.x] = x;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    double* st = a.state;
    // sums about the rounded mean m' -> moments about the chunk's mean m' + e, e = S1 / n
    for (int i = 0; i < kLstatNV; ++i) {
        const double nb = i == 3 ? m[7] : m[6];
        if (nb == 0.0) continue;
        const double e = lstat_mean_shift(S[2 * i], nb);
        lstat_merge3(st + 8 * i, nb, m[i] + e, S[2 * i + 1] - nb * e * e);
    }
    {
        const double nb = m[6], e = lstat_mean_shift(S[10], nb), e2 = e * e;
        const double mb = m[5] + e;
        const double M2b = S[11] - nb * e2;
        const double M3b = S[12] - 3.0 * e * S[11] + 2.0 * nb * e2 * e;
        const double M4b = S[13] - 4.0 * e * S[12] + 6.0 * e2 * S[11] - 3.0 * nb * e2 * e2;
        double* d = st + kLstatDBase;
        const double na = d[0];
        if (na == 0.0) {
            d[0] = nb; d[1] = mb; d[2] = M2b; d[3] = M3b; d[4] = M4b;
        } else {
            const double n = na + nb, dl = mb - d[1], dl2 = dl * dl, M2a = d[2], M3a = d[3], M4a = d[4];
            d[0] = n;
            d[1] = lstat_merged_mean(na, d[1], nb, mb);
            d[2] = M2a + M2b + dl2 * (na * nb / n);
            d[3] = M3a + M3b + dl2 * dl * (na * nb * (na - nb) / (n * n)) + 3.0 * dl * (na * M2b - nb * M2a) / n;
            d[4] = M4a + M4b + dl2 * dl2 * (na * nb * (na * na - na * nb + nb * nb) / (n * n * n))
                   + 6.0 * dl2 * (na * na * M2b + nb * nb * M2a) / (n * n) + 4.0 * dl * (na * M3b - nb * M3a) / n;
        }
    }
}

// out: (mean, variance, relative error) of terminal, cross_entropy, cross_entropy_detach, cross_entropy_detach_selection,
// log_variance, moment;  out[18] = selected count, out[19] = count
__global__ void lstat_finish_kernel(const double* st, double* out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const int slot[kLstatNV] = {0, 1, 2, 3, 5};
    for (int i = 0; i < kLstatNV; ++i) {
        const double n = st[8 * i], mean = n > 0.0 ? st[8 * i + 1] : nan(""), var = st[8 * i + 2] / (n - 1.0);
        double* o = out + 3 * slot[i];
        o[0] = mean; o[1] = var; o[2] = sqrt(var) / fabs(mean);
    }
    const double* d = st + kLstatDBase;
    const double n = d[0], var = d[2] / (n - 1.0), vv = d[4] / n - var * var;
    out[12] = var; out[13] = vv; out[14] = sqrt(vv) / fabs(var);
    out[18] = st[8 * 3];
    out[19] = n;
}

#endif  // PSP_LSTAT_KERNELS

}  // namespace psp
