// The instances of the linear / affine / constant control kernels (aff_kernels.h): the d buckets 16, 32 and 64.
#include "aff_kernels.h"

namespace psp {

namespace {
template <int DB>
hipError_t launch_fwd(const AffArgs& a, int grid, int threads, int lds_bytes, hipStream_t stream) {
    return launch_lds<aff_fwd_kernel<DB>>(dim3(grid), dim3(threads), lds_bytes, stream, a);
}
template <int DB>
hipError_t launch_adj(const AffArgs& a, int grid, int threads, int lds_bytes, hipStream_t stream) {
    return launch_lds<aff_adj_kernel<DB>>(dim3(grid), dim3(threads), lds_bytes, stream, a);
}
template <int DB>
hipError_t launch_bwd(const AffArgs& a, int grid, hipStream_t stream) {
    return launch<aff_bwd_kernel<DB>>(dim3(grid), dim3(kAffBwdThreads), 0, stream, a);
}
template <int DB>
AffInstance make_instance() { return AffInstance{&launch_fwd<DB>, &launch_adj<DB>, &launch_bwd<DB>}; }
}  // namespace

AffInstance aff_instance_16() { return make_instance<16>(); }
AffInstance aff_instance_32() { return make_instance<32>(); }
AffInstance aff_instance_64() { return make_instance<64>(); }

}  // namespace psp
