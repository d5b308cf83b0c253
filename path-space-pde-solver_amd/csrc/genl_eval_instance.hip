// The instances of the device-side test-error evaluation (genl_eval_kernels.h): one and eight waves per 16-point tile.
// This unit defines the two kernels of genl_eval_kernels.h; of genl_kernels.h it needs the device helpers only.
#define PSP_GENL_DEVICE_HELPERS_ONLY
#define PSP_GENL_EVAL_KERNELS
#include "genl_eval_kernels.h"

namespace psp {

namespace {
template <int NW>
hipError_t launch_one(const GenlEvalArgs& a, int grid, int lds_bytes, hipStream_t stream) {
    return launch_lds<genl_eval_kernel<NW>>(dim3(grid), dim3(64 * NW), lds_bytes, stream, a);
}
}  // namespace

hipError_t genl_eval_launch(const GenlEvalArgs& a, int nw, int grid, int lds_bytes, hipStream_t stream) {
    hipError_t e = nw == 1 ? launch_one<1>(a, grid, lds_bytes, stream) : launch_one<8>(a, grid, lds_bytes, stream);
    if (e != hipSuccess) return e;
    return launch<genl_eval_reduce_kernel>(dim3(1), dim3(64 * kEvalStats), 0, stream, a.partial, grid, a.log_out, a.slot_dev, a.slot, a.log_slots);
}

}  // namespace psp
