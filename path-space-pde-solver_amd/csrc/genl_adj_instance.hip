// The adjoint sweep of the state path for the value-function ansatz (genl_adj_kernels.h: genl_adj_kernel, one, four and eight waves
// per 16-trajectory tile, and the kernel that builds the table of (dt A)^T).  A unit of its own: api_genl.hip, genl_lq_instance.hip
// and genl_ul2_instance.hip keep the kernels they had.
#define PSP_GENL_DEVICE_HELPERS_ONLY
#define PSP_GENL_ADJ_KERNELS
#include "genl_adj_kernels.h"

namespace psp {

template <int NW> static hipError_t genl_adj_launch_nw(const GenlAdjArgs& a, int ntile16, int lds_bytes, hipStream_t st) {
    return launch_lds<genl_adj_kernel<NW>>(dim3(ntile16), dim3(64 * NW), lds_bytes, st, a);
}

hipError_t genl_adj_launch(const GenlAdjArgs& a, int nw, int ntile16, int lds_bytes, hipStream_t st) {
    if (a.a.driftA) {
        const hipError_t e = launch<genl_adj_tables_kernel>(dim3(8), dim3(256), 0, st, a);
        if (e != hipSuccess) return e;
    }
    return nw == 1 ? genl_adj_launch_nw<1>(a, ntile16, lds_bytes, st)
           : nw == 4 ? genl_adj_launch_nw<4>(a, ntile16, lds_bytes, st) : genl_adj_launch_nw<8>(a, ntile16, lds_bytes, st);
}

}  // namespace psp
