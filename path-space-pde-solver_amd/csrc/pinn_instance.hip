// The PINN kernels (pinn_kernels.h): forward-Laplacian residual, per-sample finish, adjoint + weight gradients.
#define PSP_PINN_KERNELS
#include "pinn_kernels.h"

namespace psp {

namespace {
template <class Kernel>
hipError_t allow_lds(Kernel* kernel, int lds_bytes) {
    return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
}
}  // namespace

hipError_t pinn_launch_forward(const PinnArgs& a, int lds_bytes, hipStream_t stream) {
    hipError_t e = allow_lds(&pinn_forward_kernel, lds_bytes);
    if (e != hipSuccess) return e;
    const int grid = a.ntiles < 1024 ? a.ntiles : 1024;
    hipLaunchKernelGGL(pinn_forward_kernel, dim3(grid), dim3(kPinnThreads), lds_bytes, stream, a);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (a.pairs) hipLaunchKernelGGL(pinn_finish_kernel<true>, dim3((a.K + 63) / 64), dim3(64), 0, stream, a);
    else hipLaunchKernelGGL(pinn_finish_kernel<false>, dim3((a.K + 63) / 64), dim3(64), 0, stream, a);
    return hipGetLastError();
}

hipError_t pinn_launch_backward(const PinnArgs& a, int lds_bytes, hipStream_t stream) {
    if (a.vadd) {
        const hipError_t e = allow_lds(&pinn_backward_kernel<true>, lds_bytes);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(pinn_backward_kernel<true>, dim3(a.G), dim3(kPinnThreads), lds_bytes, stream, a);
        return hipGetLastError();
    }
    hipError_t e = allow_lds(&pinn_backward_kernel<false>, lds_bytes);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(pinn_backward_kernel<false>, dim3(a.G), dim3(kPinnThreads), lds_bytes, stream, a);
    return hipGetLastError();
}

hipError_t pinn_launch_pairs(const PinnPairArgs& a, hipStream_t stream) {
    const int lds_bytes = 4 * a.K;                                 // <= 64 KiB (kPinnPairMaxK)
    hipError_t e = allow_lds(&pinn_pair_kernel, lds_bytes);
    if (e != hipSuccess) return e;
    const int ncb = (a.K + 3) / 4;
    hipLaunchKernelGGL(pinn_pair_kernel, dim3(ncb < kPinnPairMaxWg ? ncb : kPinnPairMaxWg), dim3(kPinnThreads), lds_bytes, stream, a);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(pinn_pair_loss_kernel, dim3(1), dim3(64), 0, stream, a);
    return hipGetLastError();
}

}  // namespace psp
