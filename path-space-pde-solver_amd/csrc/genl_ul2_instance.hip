// The u_L2-log instances of the run-time-shaped forward kernel (genl_kernels.h: genl_fwd_kernel<NW, false, false, true> -- sigma = s I,
// element-wise drift: the double wells, diagonal LLGC -- and genl_fwd_kernel<NW, true, true, true> -- the linear-quadratic
// coefficients: dense LLGC, LQGC), one, four and eight waves per 16-trajectory tile, and the kernel that stages the gains of a
// reference control linear in x.  A unit of their own: api_genl.hip and genl_lq_instance.hip keep the kernels they had.
#define PSP_GENL_DEVICE_HELPERS_ONLY
#include "genl_kernels.h"

namespace psp {

// PSP_UL2_LINEAR: the gains M_n (N, d, d row-major, u.ref) as N A-operand tables in the layout of tSB (genl_tables_kernel:
// [mb][ks / 4][lane][ks & 3], row = 16 mb + rowmap(lane & 15), k = 4 ks + q), DB0 x DB0 blocks each; rows and columns >= d are
// zero, so the time input and the padding never enter u* = M_n X_{n+1}.  Once per plan: the gains do not depend on the parameters,
// and genl_tables_kernel writes nothing behind a.tA.
__global__ __launch_bounds__(256) void genl_ul2_stage_kernel(const GenlLogArgs la) {
    const GenlArgs& a = la.a;
    float* T = a.tables_w + la.u.tUL;
    const int DBs = a.DB0, KSs = 4 * DBs, d = a.d;
    const long long per = (long long)DBs * KSs * 64;
    const long long gtid = (long long)blockIdx.x * blockDim.x + threadIdx.x, gn = (long long)gridDim.x * blockDim.x;
    for (long long gi = gtid; gi < per * a.g.N; gi += gn) {
        const long long n = gi / per, idx = gi - n * per;
        const int lane = (int)((idx >> 2) & 63);
        const long long t = idx >> 8;                               // (mb, ks / 4)
        const int ks = 4 * (int)(t % (KSs / 4)) + (int)(idx & 3), mb = (int)(t / (KSs / 4));
        const int ii = lane & 15, q = lane >> 4;
        const int row = 16 * mb + 4 * (ii & 3) + (ii >> 2), col = 4 * ks + q;
        T[gi] = (row < d && col < d) ? la.u.ref[((size_t)n * d + row) * d + col] : 0.f;
    }
}

hipError_t genl_ul2_launch_stage(const GenlLogArgs& a, hipStream_t st) {
    return launch<genl_ul2_stage_kernel>(dim3(128), dim3(256), 0, st, a);
}

hipError_t genl_ul2_launch_fwd(const GenlLogArgs& a, int nw, int ntile16, int lds_bytes, hipStream_t st) {
    if (a.a.lq)
        return nw == 1 ? genl_launch_fwd<1, true, true, true>(a, ntile16, lds_bytes, st)
               : nw == 4 ? genl_launch_fwd<4, true, true, true>(a, ntile16, lds_bytes, st)
                         : genl_launch_fwd<8, true, true, true>(a, ntile16, lds_bytes, st);
    return nw == 1 ? genl_launch_fwd<1, false, false, true>(a, ntile16, lds_bytes, st)
           : nw == 4 ? genl_launch_fwd<4, false, false, true>(a, ntile16, lds_bytes, st)
                     : genl_launch_fwd<8, false, false, true>(a, ntile16, lds_bytes, st);
}

}  // namespace psp
