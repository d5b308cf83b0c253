// The loss-statistics kernels (lstat_kernels.h): per-workgroup sums, centred power sums, merge into the state, finish.
#define PSP_LSTAT_KERNELS
#include "lstat_kernels.h"
#include "launch.h"

namespace psp {

hipError_t lstat_launch_accumulate(const LstatArgs& a, hipStream_t stream) {
    hipError_t e = launch<lstat_sum_kernel>(dim3(a.G), dim3(kLstatThreads), 0, stream, a);
    if (e != hipSuccess) return e;
    e = launch<lstat_centred_kernel>(dim3(a.G), dim3(kLstatThreads), 0, stream, a);
    if (e != hipSuccess) return e;
    return launch<lstat_merge_kernel>(dim3(1), dim3(kLstatThreads), 0, stream, a);
}

hipError_t lstat_launch_finish(const double* state, double* out, hipStream_t stream) {
    return launch<lstat_finish_kernel>(dim3(1), dim3(64), 0, stream, state, out);
}

}  // namespace psp
