// The linear-quadratic instances of the run-time-shaped forward kernel (genl_kernels.h: genl_fwd_kernel<NW, true, true> -- Z = B grad_x V,
// the drift product (dt A) X, the running cost at the moved state), one, four and eight waves per 16-trajectory tile.
// A unit of their own: api_genl.hip keeps the set of kernels the API unit had.  genl_tables_kernel stays where it is launched.
#define PSP_GENL_DEVICE_HELPERS_ONLY
#include "genl_kernels.h"

namespace psp {

hipError_t genl_lq_launch_fwd(const GenlArgs& a, int nw, int ntile16, int lds_bytes, hipStream_t st) {
    return nw == 1 ? genl_launch_fwd<1, true, true>(a, ntile16, lds_bytes, st)
           : nw == 4 ? genl_launch_fwd<4, true, true>(a, ntile16, lds_bytes, st) : genl_launch_fwd<8, true, true>(a, ntile16, lds_bytes, st);
}

}  // namespace psp
