// api_common.h -- what the units of the C ABI layer (api_*.hip; see include/psp.h) share: the error report, the instance tables,
// the checked launches and the range guard, the checks and argument fills that more than one family uses, and host-callable
// wrappers of the small kernels that several families launch.  Everything declared and not defined here is defined once, in
// api_common.hip.  No __global__ function lives here: a kernel is defined in the one unit that launches it.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/psp.h"
#include "launch.h"

// The kernels keep the header's enums numerically (device code does not include the C header): every such numbering is tied
// once, in the API unit that includes the kernel header which holds it.
#define PSP_SAME(a, b) static_assert(int(a) == int(b), #a " != " #b)

namespace psp_api {

// the message psp_last_error() returns on this thread (one thread_local buffer, in api_common.hip), and the code handed back
int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
int fail_hip(hipError_t e, const char* where);                                         // "<where>: <HIP error>", -10
inline int hip_rc(hipError_t e, const char* where) { return e == hipSuccess ? 0 : fail_hip(e, where); }   // how a launching entry point ends

// psp_debug_set_stamp_buffer (api_hjb.hip) sets them; the HJB and the GeneralSolver launches read them
extern unsigned long long* g_dbg;
extern long long g_dbg_n;

// one (d, H) -> instance table per kernel family (the .def files list what build.py compiled)
template <class Inst> struct Entry { int d, H; Inst (*fn)(); };
template <class Inst, size_t N> bool find_in(const Entry<Inst> (&table)[N], int d, int H, Inst* out) {
    for (const Entry<Inst>& e : table)
        if (e.d == d && e.H == H) { *out = e.fn(); return true; }
    return false;
}
template <class Inst, size_t N> constexpr int table_count(const Entry<Inst> (&)[N]) { return (int)N; }
template <class Inst, size_t N> int table_get(const Entry<Inst> (&table)[N], int i, int32_t* d, int32_t* H) {
    if (i < 0 || i >= (int)N || !d || !H) return fail(-1, "instance index out of range");
    *d = table[i].d; *H = table[i].H;
    return 0;
}

// launch one of a unit's small kernels and report a refused launch as "<kernel> launch: <HIP error>" (0, or the code of fail_hip)
template <auto Kernel, class... Args>
int launch_checked(const char* what, dim3 grid, dim3 block, size_t lds_bytes, void* stream, Args... args) {
    return hip_rc(psp::launch<Kernel>(grid, block, lds_bytes, (hipStream_t)stream, args...), what);
}
#define PSP_LAUNCH(kernel, ...) launch_checked<kernel>(#kernel " launch", __VA_ARGS__)

// Range guard of the split-product mode (include/psp.h: range_flag), either-or shape: the split kernel runs where
// range_flag[0] == 0 and its fp32-MFMA twin where it is 1 -- both are enqueued, on the same grid and the same output layout.
// Without a flag the split kernel runs alone, unpredicated.  cond / cond_want: the predicate fields of the launches' arguments.
template <class Split, class Fp32>
hipError_t launch_either(const int* range_flag, const int*& cond, int& cond_want, Split split, Fp32 fp32) {
    if (!range_flag) return split();
    const int* const cond0 = cond;
    const int want0 = cond_want;
    cond = range_flag; cond_want = 0;
    hipError_t e = split();
    if (e == hipSuccess) { cond_want = 1; e = fp32(); }
    cond = cond0; cond_want = want0;
    return e;
}
// ... raise-then-redo shape (forwards): the split kernel runs unpredicated, `raise` enqueues the kernel that sets range_flag[0]
// from what it left (and returns 0 or a failure code), then the fp32-MFMA kernel runs where the flag is 1 and overwrites it.
// what: the "<kernel> launch" of a refused split / fp32 launch.
template <class Split, class Raise, class Fp32>
int launch_redo(const int* range_flag, const int*& cond, int& cond_want, const char* what, Split split, Raise raise, Fp32 fp32) {
    hipError_t e = split();
    if (e == hipSuccess && range_flag) {
        if (const int rc = raise()) return rc;
        const int* const cond0 = cond;
        const int want0 = cond_want;
        cond = range_flag; cond_want = 1;
        e = fp32();
        cond = cond0; cond_want = want0;
    }
    return e == hipSuccess ? 0 : fail_hip(e, what);
}

constexpr int kMaxLds = 160 * 1024;

int n_cus();      // compute units of the current device, read once per process (256 when no device is visible)

// tile-per-wave kernels: one 16-trajectory tile per wave; 1..8 waves per workgroup so that small K still spreads over CUs
// (wide family: 1..4 waves, one per SIMD)
int tile_waves(int ntile16, bool wide);

// the coefficient kinds and the noise mode that psp_hjb_config and psp_is_config share
template <class Cfg> bool coeff_kinds_ok(const Cfg& c) {
    return c.drift_kind >= 0 && c.drift_kind <= 3 && c.sigma_kind >= 0 && c.sigma_kind <= 2 && c.runcost_kind >= 0 &&
           c.runcost_kind <= 1 && c.term_kind >= 0 && c.term_kind <= 2 && c.noise_mode >= 0 && c.noise_mode <= 1;
}

// the coefficient pointers of a psp_hjb_config (psp_hjb_*, psp_dnet_* and psp_aff_* launches)
int check_ptrs(const psp_hjb_config* c);

// the problem description every kernel that takes an HjbArgs reads the same way: coefficients, sizes, step, image kind.
// Each caller adds its buffers and what only it sets (the other fields stay zero).  Args: psp::HjbArgs
template <class Args> void fill_problem(const psp_hjb_config* c, int ntile16, Args* a) {
    a->drift = c->drift; a->sigma = c->sigma; a->runcost = c->runcost; a->term = c->term;
    a->drift_kind = c->drift_kind; a->sigma_kind = c->sigma_kind; a->runcost_kind = c->runcost_kind; a->term_kind = c->term_kind;
    a->K_local = c->K_local; a->N = c->N; a->ntile16 = ntile16;
    a->dt = c->dt; a->sqdt = c->sqrt_dt; a->sigma_scale = c->sigma_scale;
    a->adaptive = c->adaptive; a->store_path = c->store_path;
}

// the h kinds of the exit-time and box problems (PSP_GH_AFFINE_EXP, _SINE_SOURCE, _SINNORM2): what their h_par must hold.  d is the
// number of real coordinates
int check_gh_par(int32_t h_kind, const float* h_par, int32_t d);

// the stopping domain of a psp_gen_config (psp_gen_* and, through its base, psp_genl_*)
int check_gen_domain(const psp_gen_config& c);

// the problem of a psp_gen_config as the psp_gen_* and the psp_genl_* kernels read it; the other fields are each caller's own.
// Args: psp::GenArgs
template <class Args> void fill_gen_problem(const psp_gen_config& c, int ntile16, Args* a) {
    a->drift = c.drift; a->k_offset = c.k_offset; a->K_local = c.K_local; a->N = c.N; a->ntile16 = ntile16;
    a->dt = c.dt; a->sqdt = c.sqrt_dt; a->T = c.T; a->sigma_scale = c.sigma_scale;
    a->drift_kind = c.drift_kind; a->h_kind = c.h_kind; a->adaptive = c.adaptive;
    a->noise_mode = c.noise_mode; a->store_path = c.store_path;
    a->domain_kind = c.domain_kind; a->dom_a = c.dom_a; a->dom_b = c.dom_b;
    for (int i = 0; i < 4; ++i) a->h_par[i] = c.h_par[i];
    a->dwell_form = c.dwell_form ? 1 : 0;
}

// ---- the small kernels of api_common.hip that several families launch: 0, or "<kernel> launch: <HIP error>" -----------------
int reduce_partials(const double* part, int n, double* out, void* stream);             // reduce_partials_kernel: (sum D, sum D^2)
int reduce_grad(const float* part, int nwg, int P, float* out, void* stream);          // reduce_grad_kernel: partial gradients -> gradient
int range_flag_partials(const double* part, int n, int* flag, void* stream);           // range_flag_partials_kernel

// ---- device code that kernels of two units inline (api_common.hip and api_hjb.hip) -----------------------------------------
// the n pairs of `part` summed by a single workgroup of 256 threads in a fixed order: thread t sums entries t, t+256, ... then
// a tree; thread 0 gets the two sums
__device__ __forceinline__ void block_pair_sum(const double* __restrict__ part, int n, double* sum0, double* sum1) {
    __shared__ double s0[256], s1[256];
    double a = 0.0, b = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) { a += part[2 * i]; b += part[2 * i + 1]; }
    s0[threadIdx.x] = a; s1[threadIdx.x] = b;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) { s0[threadIdx.x] += s0[threadIdx.x + w]; s1[threadIdx.x] += s1[threadIdx.x + w]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { *sum0 = s0[0]; *sum1 = s1[0]; }
}

// Fixed-order sum over the workgroup partials of parameter i, spread over EIGHT threads (slice u sums the workgroups
// w = u (mod 8) in increasing order, the slices meet in LDS as ((s0+s1)+(s2+s3))+((s4+s5)+(s6+s7))): the same grouping -- and
// the same bits -- as one thread with eight accumulators, but nwg / 8 dependent loads deep instead of nwg (256 partials of a
// 17 k-parameter net took 12.7 us, a fifteenth of the K = 1024 iteration).  blockDim = (32 parameters) x (8 slices).
__device__ __forceinline__ float reduce_partials_8way(const float* __restrict__ part, int nwg, int P, int i, float* sh) {
    const int tx = threadIdx.x & 31, u = threadIdx.x >> 5;
    float s = 0.f;
    if (i < P) {
        int w = u;
        for (; w + 24 < nwg; w += 32) {                        // four loads in flight
            const float a0 = part[(size_t)w * P + i], a1 = part[(size_t)(w + 8) * P + i];
            const float a2 = part[(size_t)(w + 16) * P + i], a3 = part[(size_t)(w + 24) * P + i];
            s += a0; s += a1; s += a2; s += a3;
        }
        for (; w < nwg; w += 8) s += part[(size_t)w * P + i];
    }
    sh[u * 32 + tx] = s;
    __syncthreads();
    return ((sh[tx] + sh[32 + tx]) + (sh[64 + tx] + sh[96 + tx])) + ((sh[128 + tx] + sh[160 + tx]) + (sh[192 + tx] + sh[224 + tx]));
}

}  // namespace psp_api
