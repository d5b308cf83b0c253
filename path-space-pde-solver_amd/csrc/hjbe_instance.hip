// The instances of the reference-control / uncontrolled evaluation rollout (hjbe_kernels.h): every d bucket x control kind.
#include "hjbe_kernels.h"

namespace psp {

namespace {
template <int DB, int CTRL>
hipError_t launch_one(const IsArgs& a, int grid, int lds_bytes, hipStream_t stream) {
    return launch_lds<hjbe_rollout_kernel<DB, CTRL>>(dim3(grid), dim3(kIsThreads), lds_bytes, stream, a);
}

template <int DB>
hipError_t launch_bucket(const IsArgs& a, int grid, int lds_bytes, hipStream_t stream) {
    switch (a.ctrl) {
        case ISC_NONE: return launch_one<DB, ISC_NONE>(a, grid, lds_bytes, stream);
        case ISC_TABLE: return launch_one<DB, ISC_TABLE>(a, grid, lds_bytes, stream);
        case ISC_LINEAR: return launch_one<DB, ISC_LINEAR>(a, grid, lds_bytes, stream);
        case ISC_GRID: return launch_one<DB, ISC_GRID>(a, grid, lds_bytes, stream);
        default: return hipErrorInvalidValue;
    }
}
}  // namespace

hipError_t is_rollout_launch(const IsArgs& a, int grid, int lds_bytes, hipStream_t stream) {
    switch (is_bucket(a.d)) {
        case 1: return launch_bucket<1>(a, grid, lds_bytes, stream);
        case 4: return launch_bucket<4>(a, grid, lds_bytes, stream);
        case 16: return launch_bucket<16>(a, grid, lds_bytes, stream);
        case 32: return launch_bucket<32>(a, grid, lds_bytes, stream);
        default: return launch_bucket<64>(a, grid, lds_bytes, stream);
    }
}

}  // namespace psp
