// hjb_basis_kernels.h -- the two per-iteration transforms of a plan that rolls the state out in the sigma basis
// (X~ = B^-1 X: plan_native.py).  The rollout kernels then see drift B^-1 A B and sigma = I, the control net
// sees W1x X = (W1x B) X~, and the backward leaves dW~1x = sum dz1 X~^T, so that
//     parameters:  W~1x = W1x B        (before the forward, into the kernel-layout parameter buffer)
//     gradient:    dW1x = dW~1x B^T    (after the backward's fixed-order partial sum, before the all-reduce and Adam)
// Both are a (H x d) (d x d) product on the x columns of W1 (row stride d + 1, column 0 is the time input and passes through).
// A workgroup owns kBasisRows rows of W1: it stages them and the matrix in LDS (under 64 KiB up to d = 112: no attribute call),
// then forms one fp32 fmaf chain per output in the order i = 0 .. d - 1 -- the same bits on every launch, whatever the grid.
// Four rows per workgroup: at H = 64, d = 100 that is sixteen workgroups of two outputs per thread, so the launch is a few
// microseconds of latency, not a 700-fma chain per thread on one CU.
#pragma once
#include <hip/hip_runtime.h>
#include "launch.h"

namespace psp {

constexpr int kBasisThreads = 256, kBasisRows = 4;
inline int basis_lds_bytes(int d) { return (kBasisRows * (d + 1) + d * d) * 4; }

// dst[h, 1 + j] = sum_i src[h, 1 + i] M[i, j],  M = B (TRANSPOSE = false) or B^T (true); dst[h, 0] = src[h, 0]; entries
// [H (d + 1), n) are copied when dst != src (the other parameters).  dst may be src (so neither is __restrict__): a workgroup
// reads only its own rows of W1, all of them before the barrier, and writes only those rows.
template <bool TRANSPOSE>
__global__ __launch_bounds__(kBasisThreads) void hjb_basis_w1_kernel(const float* src, float* dst, const float* __restrict__ B,
                                                                     int d, int H, long long n) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, nthr = blockDim.x;
    const int h0 = blockIdx.x * kBasisRows;
    const int rows = (H - h0) < kBasisRows ? (H - h0) : kBasisRows;
    const int nw = rows * (d + 1);
    const float* wsrc = src + (long long)h0 * (d + 1);
    float* wdst = dst + (long long)h0 * (d + 1);
    float* w = lds;                                // this workgroup's rows of W1 as they came in
    float* m = lds + kBasisRows * (d + 1);         // m[i * d + j] = M[i, j]
    for (int idx = tid; idx < nw; idx += nthr) w[idx] = wsrc[idx];
    for (int idx = tid; idx < d * d; idx += nthr) {
        const int i = idx / d, j = idx - i * d;
        m[TRANSPOSE ? j * d + i : idx] = B[idx];   // (coalesced read either way)
    }
    if (dst != src) {
        const long long base = (long long)H * (d + 1);
        for (long long idx = base + (long long)blockIdx.x * nthr + tid; idx < n; idx += (long long)gridDim.x * nthr) dst[idx] = src[idx];
    }
    __syncthreads();
    for (int idx = tid; idx < nw; idx += nthr) {
        const int h = idx / (d + 1), c = idx - h * (d + 1);
        float v = w[idx];
        if (c > 0) {
            const float* row = w + h * (d + 1) + 1;
            const int j = c - 1;
            v = 0.f;
            for (int i = 0; i < d; ++i) v = fmaf(row[i], m[i * d + j], v);
        }
        wdst[idx] = v;
    }
}

template <bool TRANSPOSE>
inline hipError_t launch_basis_w1(const float* src, float* dst, const float* B, int d, int H, long long n, hipStream_t s) {
    const int grid = (H + kBasisRows - 1) / kBasisRows;
    return launch<hjb_basis_w1_kernel<TRANSPOSE>>(dim3(grid), dim3(kBasisThreads), basis_lds_bytes(d), s, src, dst, B, d, H, n);
}

}  // namespace psp
