// The PINN kernels (pinn_kernels.h): forward-Laplacian residual, per-sample finish, adjoint + weight gradients.
#define PSP_PINN_KERNELS
#include "pinn_kernels.h"
#include "launch.h"

namespace psp {

hipError_t pinn_launch_forward(const PinnArgs& a, int lds_bytes, hipStream_t stream) {
    const int grid = a.ntiles < 1024 ? a.ntiles : 1024;
    const hipError_t e = launch_lds<pinn_forward_kernel>(dim3(grid), dim3(kPinnThreads), lds_bytes, stream, a);
    if (e != hipSuccess) return e;
    const dim3 per_sample((a.K + 63) / 64);
    return a.pairs ? launch<pinn_finish_kernel<true>>(per_sample, dim3(64), 0, stream, a) : launch<pinn_finish_kernel<false>>(per_sample, dim3(64), 0, stream, a);
}

namespace {
template <bool VADD>
hipError_t backward_as(const PinnArgs& a, int lds_bytes, hipStream_t stream) {
    return launch_lds<pinn_backward_kernel<VADD>>(dim3(a.G), dim3(kPinnThreads), lds_bytes, stream, a);
}
}  // namespace

hipError_t pinn_launch_backward(const PinnArgs& a, int lds_bytes, hipStream_t stream) {
    return a.vadd ? backward_as<true>(a, lds_bytes, stream) : backward_as<false>(a, lds_bytes, stream);
}

hipError_t pinn_launch_pairs(const PinnPairArgs& a, hipStream_t stream) {
    const int lds_bytes = 4 * a.K;                                 // <= 64 KiB (kPinnPairMaxK)
    const int ncb = (a.K + 3) / 4;
    const hipError_t e = launch_lds<pinn_pair_kernel>(dim3(ncb < kPinnPairMaxWg ? ncb : kPinnPairMaxWg), dim3(kPinnThreads), lds_bytes, stream, a);
    return e != hipSuccess ? e : launch<pinn_pair_loss_kernel>(dim3(1), dim3(64), 0, stream, a);
}

}  // namespace psp
