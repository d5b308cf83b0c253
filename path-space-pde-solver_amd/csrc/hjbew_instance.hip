// The instances of the wide-state evaluation rollout (hjbew_kernels.h): every block bucket x control kind, and its table kernel.
#include "hjbew_kernels.h"

namespace psp {

namespace {
template <int DB, int CTRL>
hipError_t launch_one(const IswArgs& w, int grid, int lds_bytes, hipStream_t stream) {
    return launch_lds<isw_rollout_kernel<DB, CTRL>>(dim3(grid), dim3(kIswThreads), lds_bytes, stream, w);
}

template <int DB>
hipError_t launch_bucket(const IswArgs& w, int grid, int lds_bytes, hipStream_t stream) {
    switch (w.a.ctrl) {
        case ISC_NONE: return launch_one<DB, ISC_NONE>(w, grid, lds_bytes, stream);
        case ISC_TABLE: return launch_one<DB, ISC_TABLE>(w, grid, lds_bytes, stream);
        case ISC_LINEAR: return launch_one<DB, ISC_LINEAR>(w, grid, lds_bytes, stream);
        case ISC_GRID: return launch_one<DB, ISC_GRID>(w, grid, lds_bytes, stream);
        default: return hipErrorInvalidValue;
    }
}
}  // namespace

hipError_t isw_rollout_launch(const IswArgs& w, int grid, int lds_bytes, hipStream_t stream) {
    // the scratch first: a few workgroups per 64 Ki elements, at most 1024
    const long long blocks = (w.L.total + 256 * 64 - 1) / (256 * 64);
    hipError_t e = launch<isw_tables_kernel<>>(dim3((unsigned)(blocks < 1 ? 1 : blocks > 1024 ? 1024 : blocks)), dim3(256), 0, stream, w);
    if (e != hipSuccess) return e;
    switch (isw_bucket(w.a.d)) {
        case 4: return launch_bucket<4>(w, grid, lds_bytes, stream);
        case 8: return launch_bucket<8>(w, grid, lds_bytes, stream);
        case 12: return launch_bucket<12>(w, grid, lds_bytes, stream);
        default: return launch_bucket<16>(w, grid, lds_bytes, stream);
    }
}

}  // namespace psp
