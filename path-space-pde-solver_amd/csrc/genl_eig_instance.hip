// The eigenvalue instances of the run-time-shaped forward kernel (genl_kernels.h: genl_fwd_kernel<NW, false, false, false, true> --
// sigma = s I, a trained lambda read from device memory, the gate of an output ReLU, the per-trajectory S_k and the h / drift kinds
// of the Fokker-Planck and nonlinear Schroedinger eigenvalue problems), one, four and eight waves per 16-trajectory tile.  A unit
// of their own: api_genl.hip and the other instance units keep the kernels they had.
#define PSP_GENL_DEVICE_HELPERS_ONLY
#include "genl_kernels.h"

namespace psp {

hipError_t genl_eig_launch_fwd(const GenlEigFwdArgs& a, int nw, int ntile16, int lds_bytes, hipStream_t st) {
    return nw == 1 ? genl_launch_fwd<1, false, false, false, true>(a, ntile16, lds_bytes, st)
           : nw == 4 ? genl_launch_fwd<4, false, false, false, true>(a, ntile16, lds_bytes, st)
                     : genl_launch_fwd<8, false, false, false, true>(a, ntile16, lds_bytes, st);
}

}  // namespace psp
