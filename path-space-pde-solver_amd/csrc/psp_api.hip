// psp_api.hip -- C ABI of libpsp_hip.so (see include/psp.h) + the small streaming kernels.
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <rccl/rccl.h>   // types only: the entry points are bound with dlsym at first use (psp_comm_*)

#include "../../include/psp.h"
#include "launch.h"
#include "hjb_kernels.h"
#include "hjb_basis_kernels.h"
#include "gen_kernels.h"
#include "hjbw_kernels.h"
#include "hjbd_kernels.h"
#include "genl_kernels.h"
#include "genl_eval_kernels.h"
#include "genl_adj_kernels.h"
#include "hjbe_kernels.h"
#include "hjbew_kernels.h"
#include "aff_kernels.h"
#include "pinn_kernels.h"
#include "lstat_kernels.h"

// The kernels keep the header's enums numerically (device code does not include the C header): every such numbering, tied here.
#define PSP_SAME(a, b) static_assert(int(a) == int(b), #a " != " #b)
PSP_SAME(psp::GH_ZERO, PSP_GH_ZERO); PSP_SAME(psp::GH_QUAD, PSP_GH_QUAD); PSP_SAME(psp::GH_ALLEN_CAHN, PSP_GH_ALLEN_CAHN);
PSP_SAME(psp::GH_EXPBALL_LIN, PSP_GH_EXPBALL_LIN); PSP_SAME(psp::GH_EXPBALL_SQ, PSP_GH_EXPBALL_SQ);
PSP_SAME(psp::GH_EXPBALL_SIN, PSP_GH_EXPBALL_SIN); PSP_SAME(psp::GH_EXPBALL_SIN_FULL, PSP_GH_EXPBALL_SIN_FULL);
PSP_SAME(psp::GH_AFFINE_EXP, PSP_GH_AFFINE_EXP); PSP_SAME(psp::GH_SINE_SOURCE, PSP_GH_SINE_SOURCE);
PSP_SAME(psp::GH_SINNORM2, PSP_GH_SINNORM2); PSP_SAME(psp::GH_EIG_FP, PSP_GH_EIG_FP); PSP_SAME(psp::GH_EIG_NLS, PSP_GH_EIG_NLS);
PSP_SAME(psp::DOM_NONE, PSP_DOM_NONE); PSP_SAME(psp::DOM_SPHERE, PSP_DOM_SPHERE); PSP_SAME(psp::DOM_BOX, PSP_DOM_BOX);
PSP_SAME(psp::DOM_BOX_UPPER_ALL, PSP_DOM_BOX_UPPER_ALL); PSP_SAME(psp::DOM_BOX_UPPER_ANY, PSP_DOM_BOX_UPPER_ANY);
PSP_SAME(psp::DOM_ANNULUS, PSP_DOM_ANNULUS);
PSP_SAME(psp::DRIFT_ZERO, PSP_DRIFT_ZERO); PSP_SAME(psp::DRIFT_DENSE, PSP_DRIFT_DENSE); PSP_SAME(psp::DRIFT_DIAG, PSP_DRIFT_DIAG);
PSP_SAME(psp::DRIFT_DWELL, PSP_DRIFT_DOUBLE_WELL); PSP_SAME(psp::DRIFT_EIG_FP, PSP_DRIFT_EIG_FP);
PSP_SAME(psp::PINN_DRIFT_ZERO, psp::DRIFT_ZERO); PSP_SAME(psp::PINN_DRIFT_DIAG, psp::DRIFT_DIAG);
PSP_SAME(psp::PINN_DRIFT_DWELL, psp::DRIFT_DWELL);
PSP_SAME(psp::DRIFT_WELL_DIAG, PSP_DRIFT_WELL_DIAG); PSP_SAME(psp::DRIFT_RADIAL, PSP_DRIFT_RADIAL_WELL);
PSP_SAME(psp::TERM_QUADLIN, PSP_TERM_QUAD_LINEAR); PSP_SAME(psp::TERM_RADIAL, PSP_TERM_RADIAL_QUAD);
PSP_SAME(psp::GACT_RELU2, PSP_ACT_RELU2); PSP_SAME(psp::GACT_TANH2, PSP_ACT_TANH2); PSP_SAME(psp::GACT_TANH, PSP_ACT_TANH);
PSP_SAME(psp::PINN_ACT_RELU2, PSP_ACT_RELU2); PSP_SAME(psp::PINN_ACT_TANH2, PSP_ACT_TANH2); PSP_SAME(psp::PINN_ACT_TANH, PSP_ACT_TANH);
#undef PSP_SAME

#define X(D_, H_) PSP_DECLARE_DNET_INSTANCE(D_, H_)
#include "dense_instances.def"
#undef X
#define X(D_, H_) PSP_DECLARE_INSTANCE(D_, H_)
#include "instances.def"
#undef X
#define X(D_, H_) PSP_DECLARE_WIDE_INSTANCE(D_, H_)
#include "wide_instances.def"
#undef X
#define X(D_, H_) PSP_DECLARE_GEN_INSTANCE(D_, H_)
#include "gen_instances.def"
#undef X

namespace {

thread_local char g_err[512] = "";
unsigned long long* g_dbg = nullptr;   // psp_debug_set_stamp_buffer
long long g_dbg_n = 0;

int fail(int code, const char* fmt, const char* detail = "") {
    snprintf(g_err, sizeof(g_err), fmt, detail);
    return code;
}
int fail_hip(hipError_t e, const char* where) {
    snprintf(g_err, sizeof(g_err), "%s: %s", where, hipGetErrorString(e));
    return -10;
}
int hip_rc(hipError_t e, const char* where) { return e == hipSuccess ? 0 : fail_hip(e, where); }   // how a launching entry point ends

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

const Entry<psp::HjbInstance> kTable[] = {
#define X(D_, H_) {D_, H_, &psp_instance_##D_##_##H_},
#include "instances.def"
#undef X
};
const Entry<psp::HjbInstance> kWideTable[] = {
#define X(D_, H_) {D_, H_, &psp_wide_instance_##D_##_##H_},
#include "wide_instances.def"
#undef X
};
const Entry<psp::GenInstance> kGenTable[] = {
#define X(D_, H_) {D_, H_, &psp_gen_instance_##D_##_##H_},
#include "gen_instances.def"
#undef X
};
const Entry<psp::DnetInstance> kDnetTable[] = {
#define X(D_, H_) {D_, H_, &psp_dnet_instance_##D_##_##H_},
#include "dense_instances.def"
#undef X
};

// narrow family first (state panel in 256 registers, tables in LDS); the wide family covers larger d.
// PSP_FORCE_WIDE=1 prefers the wide instance where both exist (parity tests of one family against the other).
bool find_instance(int d, int H, psp::HjbInstance* out) {
    static const char* fw = getenv("PSP_FORCE_WIDE");
    const bool force_wide = fw && fw[0] == '1';
    if (!force_wide && find_in(kTable, d, H, out)) return true;
    if (find_in(kWideTable, d, H, out)) return true;
    return force_wide && find_in(kTable, d, H, out);
}

// launch one of the small kernels below and report a refused launch as "<kernel> launch: <HIP error>" (0, or the code of fail_hip)
template <auto Kernel, class... Args>
int launch_checked(const char* what, dim3 grid, dim3 block, size_t lds_bytes, void* stream, Args... args) {
    return hip_rc(psp::launch<Kernel>(grid, block, lds_bytes, (hipStream_t)stream, args...), what);
}
#define PSP_LAUNCH(kernel, ...) launch_checked<kernel>(#kernel " launch", __VA_ARGS__)
using psp::genl_tables_kernel;     // (so that its message reads "genl_tables_kernel launch" like the others)

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

struct Plan {
    psp::HjbInstance inst;
    int ntile16, fwd_waves, fwd_grid, bwd_grid;
    bool fwd_coop = false;   // wide family, split products, d > 256: hjbc_fwd_kernel (fwd_waves = 2 or 4 TILES per 512-thread workgroup)
    bool fwd_split;             // hjbs_fwd_kernel (four waves per tile) instead of hjb_fwd_kernel
    bool fwd_quad;              // hjbq_fwd_kernel (four trajectories per workgroup) for the smallest K
};

int n_cus() {
    static int cus = 0;
    if (cus == 0) {
        int dev = 0;
        hipDeviceProp_t prop;
        if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess)
            cus = prop.multiProcessorCount;
        if (cus <= 0) cus = 256;     // MI355X; also used when no device is visible (size queries on CPU)
    }
    return cus;
}

// tile-per-wave kernels: one 16-trajectory tile per wave; 1..8 waves per workgroup so that small K still spreads over CUs
// (wide family: 1..4 waves, one per SIMD)
int tile_waves(int ntile16, bool wide) {
    const int cus = n_cus(), cap = wide ? 4 : 8;
    const int fw = (ntile16 + cus - 1) / cus;
    return fw < 1 ? 1 : fw > cap ? cap : fw;
}

// the coefficient kinds and the noise mode that psp_hjb_config and psp_is_config share
template <class Cfg> bool coeff_kinds_ok(const Cfg& c) {
    return c.drift_kind >= 0 && c.drift_kind <= 3 && c.sigma_kind >= 0 && c.sigma_kind <= 2 && c.runcost_kind >= 0 &&
           c.runcost_kind <= 1 && c.term_kind >= 0 && c.term_kind <= 2 && c.noise_mode >= 0 && c.noise_mode <= 1;
}

int make_plan(const psp_hjb_config* c, Plan* p) {
    if (!c) return fail(-1, "null config");
    if (c->d <= 0 || c->H <= 0 || c->K_local <= 0 || c->N <= 0) return fail(-1, "non-positive d/H/K/N");
    if (!find_instance(c->d, c->H, &p->inst)) {
        snprintf(g_err, sizeof(g_err), "no compiled HJB kernel instance for d=%d H=%d", c->d, c->H);
        return -2;
    }
    if (!coeff_kinds_ok(*c) || c->loss_kind < 0 || c->loss_kind > 3 || c->store_path < 0 || c->store_path > 4)
        return fail(-1, "config enum out of range");
    if (c->store_path == 4) {                                  // the backward regenerates xi: only where the image IS xi
        if (p->inst.wide) return fail(-2, "store_path 4 (xi regenerated by the backward) exists in the narrow kernel family only");
        if (c->noise_mode != PSP_NOISE_PHILOX || !c->adaptive)
            return fail(-1, "store_path 4 needs on-device noise and the adaptive forward process (the stored image is then xi itself)");
    }
    if (c->mlp_dtype == PSP_MLP_F16X3) {
        if (!p->inst.launch_fwd_x3) return fail(-3, "the split-product mode (PSP_MLP_F16X3) is not built for this kernel family");
        if (p->inst.fwd_x3_lds_bytes(c->drift_kind, c->sigma_kind) > kMaxLds)
            return fail(-3, "split-product forward tables do not fit the 160 KiB LDS for this (d,H,drift,sigma)");
        if (c->range_flag && p->inst.fwd_lds_bytes(c->drift_kind, c->sigma_kind) > kMaxLds)
            return fail(-3, "range guard: the fp32-MFMA forward tables do not fit the 160 KiB LDS for this (d,H,drift,sigma)");
    } else if (p->inst.fwd_lds_bytes(c->drift_kind, c->sigma_kind) > kMaxLds)
        return fail(-3, "forward kernel weights do not fit the 160 KiB LDS for this (d,H,drift,sigma)");
    p->ntile16 = (c->K_local + 15) / 16;
    if ((long long)c->N * p->ntile16 >= (1LL << 31)) return fail(-1, "N * ceil(K/16) must stay below 2^31");
    const int cus = n_cus();
    int fw = tile_waves(p->ntile16, p->inst.wide);
    if (p->inst.wide && c->mlp_dtype == PSP_MLP_F16X3) fw = 4;   // its split-product forward shares the table stream between FOUR waves
    // ... unless the cooperative forward serves the launch (hjbc_kernels.h: on-device noise, no running cost, no u_L2 log): TWO tiles
    // per workgroup; the range guard's fp32 twin then runs hjbw_fwd_kernel on the same grid with two waves per workgroup
    // (PSP_FWD_COOP=0 keeps the tile-per-wave kernel: A/B and parity tests of one against the other)
    {
        const char* fc = getenv("PSP_FWD_COOP");
        // four tiles per workgroup while that still gives every CU one (a single round at K = 16 384), else two
        const int nt = (fc && (fc[0] == '2' || fc[0] == '4')) ? fc[0] - '0' : (p->ntile16 >= 4 * cus ? 4 : 2);
        // measured (same box, K = 32 768): d = 200 tile-per-wave 3.53, two tiles 3.81, four tiles 3.27 ms; d = 256: 5.47 / 4.59 / 3.98; d = 500
        // (K = 16 384): 16.9 / 12.5 / 11.9.  The KERNEL must not depend on the launch size -- a K-chunked run reproduces the resident
        // run's D bit for bit (tests/test_gpu_full_size.py), and two and four tiles sum in the same order while the tile-per-wave
        // kernel does not -- so the cooperative kernel serves every size where it exists (8 % slower at d = 200 below K = 16 384)
        const bool coop_default = true;
        p->fwd_coop = p->inst.wide && c->mlp_dtype == PSP_MLP_F16X3 && p->inst.launch_fwd_coop && p->inst.coop_lds_bytes(nt) <= kMaxLds &&
                      c->noise_mode == PSP_NOISE_PHILOX && c->runcost_kind == 0 && c->u_ref == nullptr && !(fc && fc[0] == '0') &&
                      (coop_default || (fc && fc[0] != '0'));
        if (p->fwd_coop) fw = nt;
    }
    p->fwd_waves = fw;
    p->fwd_grid = (p->ntile16 + fw - 1) / fw;
    // few tiles: the feature-split forward (four waves per tile, weights in registers) cuts the per-step latency ~3x.
    // It wins while one-wave-per-tile would leave SIMDs idle: up to 2 tiles per CU (PSP_FWD_VARIANT=1 / 2 / 3 force the
    // tile-per-wave, the feature-split or the quad kernel)
    const char* fv = getenv("PSP_FWD_VARIANT");       // (read per call: tests switch variants inside one process)
    p->fwd_split = !p->inst.wide && p->inst.launch_fwd_split && p->inst.split_lds_bytes() <= kMaxLds &&
                   c->mlp_dtype != PSP_MLP_BF16_FWD && c->mlp_dtype != PSP_MLP_F16X3 &&   // (these modes exist in hjb_fwd_kernel only)
                   ((fv && fv[0] == '2') || (!(fv && fv[0] == '1') && p->ntile16 <= 2 * cus));
    if (p->fwd_split) { p->fwd_waves = 8; p->fwd_grid = p->ntile16; }   // (the kernel itself fixes 4 or 8 waves per tile)
    // fewer tiles than a quarter of the CUs: four trajectories per workgroup (hjbq_kernels.h), so that K = 1024 still covers the
    // chip (PSP_FWD_VARIANT=3 forces it, 1 / 2 exclude it)
    p->fwd_quad = !p->inst.wide && p->inst.launch_fwd_quad && p->inst.quad_lds_bytes() <= kMaxLds &&
                  c->mlp_dtype != PSP_MLP_BF16_FWD && c->mlp_dtype != PSP_MLP_F16X3 &&
                  ((fv && fv[0] == '3') || (!fv && 4 * p->ntile16 <= cus));
    if (p->fwd_quad) { p->fwd_split = false; p->fwd_waves = 8; p->fwd_grid = 4 * p->ntile16; }
    // backward: persistent over rounds of 4 sample blocks, one workgroup per CU (fewer when there is little work): the
    // role-specialised hjb_bwd2_kernel, whose double-buffered exchange area must fit the LDS, or the wide family's launch_bwd2
    // (where that is the 4-wave hjbw_bwd_kernel at d <= 256: two workgroups per CU)
    const long long nblk = (long long)c->N * p->ntile16;
    const long long nround = (nblk + 3) / 4;
    if (!p->inst.wide && p->inst.bwd2_lds_bytes() > kMaxLds)
        return fail(-3, "the role-specialised backward kernel's exchange area does not fit the 160 KiB LDS for this (d,H)");
    long long g = nround;
    const long long gmax = (p->inst.wide && c->d <= 256 && !p->inst.bwd2_one_per_cu) ? 2LL * cus : cus;
    if (g > gmax) g = gmax;
    if (g < 1) g = 1;
    p->bwd_grid = (int)g;
    return 0;
}

// the problem description every kernel that takes an HjbArgs reads the same way: coefficients, sizes, step, image kind.
// Each caller adds its buffers and what only it sets (the other fields stay zero)
void fill_problem(const psp_hjb_config* c, int ntile16, psp::HjbArgs* a) {
    a->drift = c->drift; a->sigma = c->sigma; a->runcost = c->runcost; a->term = c->term;
    a->drift_kind = c->drift_kind; a->sigma_kind = c->sigma_kind; a->runcost_kind = c->runcost_kind; a->term_kind = c->term_kind;
    a->K_local = c->K_local; a->N = c->N; a->ntile16 = ntile16;
    a->dt = c->dt; a->sqdt = c->sqrt_dt; a->sigma_scale = c->sigma_scale;
    a->adaptive = c->adaptive; a->store_path = c->store_path;
}

void fill_args(const psp_hjb_config* c, const Plan& p, psp::HjbArgs* a) {
    memset(a, 0, sizeof(*a));
    fill_problem(c, p.ntile16, a);
    a->k_offset = c->k_offset; a->K_global = c->K_global; a->loss_kind = c->loss_kind; a->noise_mode = c->noise_mode;
    a->uref = c->u_ref; a->ul2 = c->u_l2_out;
    a->iter_dev = c->iter_dev;
    // diagnostic stamp buffer: [forward: fwd_grid x 8 waves x 8][backward: bwd_grid x 4 waves x 8]
    a->dbg = (g_dbg && g_dbg_n >= ((long long)p.fwd_grid * 8 + (long long)p.bwd_grid * 8) * 8) ? g_dbg : nullptr;
}

int check_ptrs(const psp_hjb_config* c) {
    if ((c->drift_kind != PSP_DRIFT_ZERO) && !c->drift) return fail(-1, "drift parameters missing");
    if (c->sigma_kind == PSP_SIGMA_DENSE && !c->sigma) return fail(-1, "sigma matrix missing");
    if (c->runcost_kind == PSP_RUNCOST_DIAG_QUAD && !c->runcost) return fail(-1, "running-cost vector missing");
    if (!c->term) return fail(-1, "terminal-cost vector missing");
    if (c->u_ref && !c->u_l2_out) return fail(-1, "u_ref set but u_l2_out is null");
    return 0;
}

struct GenPlan {
    psp::GenInstance inst;
    int ntile16, fwd_waves, fwd_grid, bwd_grid;
};

// the h kinds of the exit-time and box problems (PSP_GH_AFFINE_EXP, _SINE_SOURCE, _SINNORM2): what their h_par must hold.  d is the
// number of real coordinates
int check_gh_par(int32_t h_kind, const float* h_par, int32_t d) {
    if (h_kind == PSP_GH_SINE_SOURCE) {
        if (h_par[0] != 0.f && h_par[0] != 1.f) return fail(-1, "PSP_GH_SINE_SOURCE: the sub-mode h_par[0] is 0 (Helmholtz) or 1 (Oscillations)");
        if (h_par[0] == 0.f && d < 2) return fail(-1, "PSP_GH_SINE_SOURCE: sub-mode 0 reads the coordinates x_0 and x_1 (d >= 2)");
    }
    return 0;
}

// the stopping domain of a psp_gen_config (psp_gen_* and, through its base, psp_genl_*)
int check_gen_domain(const psp_gen_config& c) {
    if (c.domain_kind == PSP_DOM_SPHERE && !(c.dom_a > 0.f)) return fail(-1, "sphere radius must be positive");
    if (c.domain_kind == PSP_DOM_BOX && !(c.dom_a < c.dom_b)) return fail(-1, "box bounds must satisfy X_l < X_r");
    if (c.domain_kind == PSP_DOM_ANNULUS && !(c.dom_a >= 0.f && c.dom_a < c.dom_b)) return fail(-1, "annulus radii must satisfy 0 <= r_1 < r_2");
    return 0;
}

int make_gen_plan(const psp_gen_config* c, GenPlan* p) {
    if (!c) return fail(-1, "null config");
    if (c->d <= 0 || c->H <= 0 || c->K_local <= 0 || c->N <= 0) return fail(-1, "non-positive d/H/K/N");
    if (!find_in(kGenTable, c->d, c->H, &p->inst)) {
        snprintf(g_err, sizeof(g_err), "no compiled GeneralSolver kernel instance for d=%d H=%d", c->d, c->H);
        return -2;
    }
    if ((c->drift_kind != PSP_DRIFT_ZERO && c->drift_kind != PSP_DRIFT_DOUBLE_WELL && c->drift_kind != PSP_DRIFT_DIAG) || c->h_kind < 0 ||
        c->h_kind > PSP_GH_SINE_SOURCE || c->h_kind == PSP_GH_EXPBALL_SIN_FULL || c->noise_mode < 0 || c->noise_mode > 1 ||
        c->domain_kind < 0 || c->domain_kind > PSP_DOM_ANNULUS)        // (_SIN_FULL and _SINNORM2 read sum_i x_i: psp_genl_* only)
        return fail(-1, "config enum out of range");
    if (int rc = check_gh_par(c->h_kind, c->h_par, (c->d_real > 0 && c->d_real < c->d) ? c->d_real : c->d)) return rc;
    if (int rc = check_gen_domain(*c)) return rc;
    if (c->drift_kind != PSP_DRIFT_ZERO && !c->drift) return fail(-1, "drift vector missing (double-well kappa / diagonal of A)");
    if ((c->v_steps_out == nullptr) != (c->y_steps_out == nullptr)) return fail(-1, "v_steps_out and y_steps_out go together");
    if (p->inst.fwd_lds_bytes() > kMaxLds)
        return fail(-3, "GeneralSolver kernel tables do not fit the 160 KiB LDS for this (d,H)");
    if (c->mlp_dtype == PSP_MLP_F16X3 && (!p->inst.launch_fwd_x3 || p->inst.fwd_x3_lds_bytes() > kMaxLds))
        return fail(-3, "split-product forward tables do not fit the 160 KiB LDS for this (d,H)");
    p->ntile16 = (c->K_local + 15) / 16;
    const int cus = n_cus();
    const int fw = tile_waves(p->ntile16, false);
    p->fwd_waves = fw;
    p->fwd_grid = (p->ntile16 + fw - 1) / fw;
    const long long nround = ((long long)(c->N + 1) * p->ntile16 + 3) / 4;
    if (p->inst.bwd2_lds_bytes() > kMaxLds)             // gen_bwd2_kernel: one 8-wave workgroup per CU
        return fail(-3, "the role-specialised backward kernel's exchange area does not fit the 160 KiB LDS for this (d,H)");
    long long g = nround;
    if (g > cus) g = cus;
    if (g < 1) g = 1;
    p->bwd_grid = (int)g;
    return 0;
}

// the problem of a psp_gen_config as the psp_gen_* and the psp_genl_* kernels read it; the other fields are each caller's own
void fill_gen_problem(const psp_gen_config& c, int ntile16, psp::GenArgs* a) {
    a->drift = c.drift; a->k_offset = c.k_offset; a->K_local = c.K_local; a->N = c.N; a->ntile16 = ntile16;
    a->dt = c.dt; a->sqdt = c.sqrt_dt; a->T = c.T; a->sigma_scale = c.sigma_scale;
    a->drift_kind = c.drift_kind; a->h_kind = c.h_kind; a->adaptive = c.adaptive;
    a->noise_mode = c.noise_mode; a->store_path = c.store_path;
    a->domain_kind = c.domain_kind; a->dom_a = c.dom_a; a->dom_b = c.dom_b;
    for (int i = 0; i < 4; ++i) a->h_par[i] = c.h_par[i];
    a->dwell_form = c.dwell_form ? 1 : 0;
}

void fill_gen_args(const psp_gen_config* c, const GenPlan& p, psp::GenArgs* a) {
    memset(a, 0, sizeof(*a));
    fill_gen_problem(*c, p.ntile16, a);
    a->d_real = (c->d_real > 0 && c->d_real < c->d) ? c->d_real : c->d;
    a->Vsteps = c->v_steps_out; a->Ysteps = c->y_steps_out; a->per_sample = c->per_sample_weights ? 1 : 0;
    a->path16 = (c->mlp_dtype == PSP_MLP_BF16) ? 1 : 0;       // both kernels on bf16 MFMA: bf16-pair path block
}

// ---- small kernels -------------------------------------------------------------------
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

__global__ void reduce_partials_kernel(const double* __restrict__ part, int n, double* __restrict__ out) {
    double sD = 0.0, sD2 = 0.0;
    block_pair_sum(part, n, &sD, &sD2);
    if (threadIdx.x == 0) { out[0] = sD; out[1] = sD2; }
}

// partial sums -> (sum D, sum D^2) and the loss value (single rank: local sums are global)
__global__ void reduce_partials_loss_kernel(const double* __restrict__ part, int n, double* __restrict__ out, int loss_kind,
                                            double invK, float* __restrict__ loss_log, const uint32_t* __restrict__ index_dev) {
    double sD = 0.0, sD2 = 0.0;
    block_pair_sum(part, n, &sD, &sD2);
    if (threadIdx.x == 0) {
        out[0] = sD; out[1] = sD2;
        if (loss_log) {
            const double m = sD * invK;
            double loss = sD2 * invK - m * m;                         // log-variance: mean(D^2) - mean(D)^2 (solver.py:167-168)
            if (loss_kind == PSP_LOSS_MOMENT) loss = sD2 * invK;      // :165-166
            if (loss_kind == PSP_LOSS_REL_ENTROPY) loss = -m;         // D = -(Zsum + g) (:179-180)
            loss_log[index_dev ? *index_dev : 0u] = (float)loss;
        }
    }
}

// Range guard of the split-product mode (include/psp.h: range_flag).  flag[0] = 1 iff any of the n doubles is non-finite
// (a per-workgroup partial of (sum D, sum D^2): an f16x3 operand beyond 65504 makes D_k NaN), flag[1] counts the 1s.
__global__ void range_flag_partials_kernel(const double* __restrict__ part, int n, int* __restrict__ flag) {
    __shared__ int bad;
    if (threadIdx.x == 0) bad = 0;
    __syncthreads();
    int mine = 0;
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const double v = part[i];
        mine |= !(fabs(v) <= 1.7976931348623157e308);            // NaN and +-inf
    }
    if (mine) bad = 1;                                           // benign race: every writer stores 1
    __syncthreads();
    if (threadIdx.x == 0) { flag[0] = bad; flag[1] += bad; }
}
__global__ void snapshot_u64_kernel(const unsigned long long* src, unsigned long long* dst) { *dst = *src; }
// the same from two fp32 arrays of n entries (GeneralSolver: V(X_N) and Y_N per trajectory)
__global__ void range_flag_arrays_kernel(const float* __restrict__ a, const float* __restrict__ b, int n, int* __restrict__ flag,
                                         unsigned long long* counter, const unsigned long long* counter_before) {
    __shared__ int bad;
    if (threadIdx.x == 0) bad = 0;
    __syncthreads();
    int mine = 0;
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        mine |= !(fabsf(a[i]) <= 3.402823466e38f);
        mine |= !(fabsf(b[i]) <= 3.402823466e38f);
    }
    if (mine) bad = 1;
    __syncthreads();
    if (threadIdx.x == 0) {
        flag[0] = bad; flag[1] += bad;
        if (bad && counter) *counter = *counter_before;          // the predicated fp32 kernel counts the active steps afresh
    }
}

__global__ void iter_advance_kernel(psp_iter_state* st, double b1, double b2) {
    st->iter += 1u; st->step += 1u; st->beta1_pow *= b1; st->beta2_pow *= b2;
}

// torch.optim.Adam single-tensor semantics (torch/optim/adam.py, _single_tensor_adam) for parameter i with gradient gi.
// step_size = lr / (1 - b1^step) and bc2_sqrt = sqrt(1 - b2^step) come from the caller, formed in
// double and rounded to fp32
__device__ __forceinline__ void adam_update(float* __restrict__ p, float* __restrict__ m, float* __restrict__ v, long long i, float gi,
                                            float b1, float b2, float eps, float step_size, float bc2_sqrt) {
    const float mi = m[i] + (gi - m[i]) * (1.0f - b1);              // exp_avg.lerp_(grad, 1-beta1)
    const float vi = v[i] * b2 + (1.0f - b2) * gi * gi;             // exp_avg_sq.mul_(b2).addcmul_(g,g,1-b2)
    m[i] = mi; v[i] = vi;
    const float denom = sqrtf(vi) / bc2_sqrt + eps;
    p[i] = p[i] - step_size * (mi / denom);                         // param.addcdiv_(exp_avg, denom, -step_size)
}

// Adam with the bias corrections of the step held in a device psp_iter_state (the host path of psp_adam_step forms step_size
// and bc2_sqrt in double and rounds to fp32, so does every thread here)
__global__ void adam_dev_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                float* __restrict__ v, long long n, const psp_iter_state* __restrict__ st, float lr, float b1,
                                float b2, float eps) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float step_size = (float)((double)lr / (1.0 - st->beta1_pow));
    const float bc2_sqrt = (float)sqrt(1.0 - st->beta2_pow);
    adam_update(p, m, v, i, g[i], b1, b2, eps, step_size, bc2_sqrt);
}

// Launch-bound sizes (graph replay): partial gradients -> gradient -> Adam -> iteration state, ONE launch instead of three.
// Per parameter: fixed-order sum of the workgroup partials (reduce_partials_8way, as reduce_grad_kernel), the Adam update of
// adam_dev_kernel with the bias corrections of the CURRENT state, then the last workgroup to finish advances the state
// (every other workgroup has read it before its ticket).  grad_out still receives the gradient (diagnostics, tests).
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

__global__ void reduce_grad_adam_advance_kernel(const float* __restrict__ part, int nwg, int P, float* __restrict__ grad_out,
                                                float* __restrict__ p, float* __restrict__ m, float* __restrict__ v,
                                                psp_iter_state* st, unsigned int* ticket, float lr, float b1, float b2, float eps) {
    __shared__ float sh[256];
    const int i = blockIdx.x * 32 + (threadIdx.x & 31);
    const double b1p = st->beta1_pow, b2p = st->beta2_pow;
    const float gi = reduce_partials_8way(part, nwg, P, i, sh);
    if (i < P && threadIdx.x < 32) {
        grad_out[i] = gi;
        const float step_size = (float)((double)lr / (1.0 - b1p));
        const float bc2_sqrt = (float)sqrt(1.0 - b2p);
        // Spelled out, not adam_update(): inlined here the compiler contracts the second-moment line as fma(b2, v, ((1 - b2) g) g),
        // in the two kernels above as fma((1 - b2) g, g, b2 v).  Sharing the function moves every graph-replay result by an ulp
        const float mi = m[i] + (gi - m[i]) * (1.0f - b1);
        const float vi = v[i] * b2 + (1.0f - b2) * gi * gi;
        m[i] = mi; v[i] = vi;
        const float denom = sqrtf(vi) / bc2_sqrt + eps;
        p[i] = p[i] - step_size * (mi / denom);
    }
    __syncthreads();                                           // every thread of this workgroup has read the state
    if (threadIdx.x == 0) {
        __threadfence();
        const unsigned int t = atomicAdd(ticket, 1u);
        if (t == gridDim.x - 1) {                              // last workgroup: all others read the state before their ticket
            st->iter += 1u; st->step += 1u; st->beta1_pow = b1p * (double)b1; st->beta2_pow = b2p * (double)b2;
            *ticket = 0u;
        }
    }
}

__global__ void reduce_grad_kernel(const float* __restrict__ part, int nwg, int P, float* __restrict__ out) {
    __shared__ float sh[256];
    const int p = blockIdx.x * 32 + (threadIdx.x & 31);
    const float g = reduce_partials_8way(part, nwg, P, p, sh);
    if (p < P && threadIdx.x < 32) out[p] = g;
}

__global__ void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                            float* __restrict__ v, long long n, float lr, float b1, float b2, float eps,
                            float step_size, float bc2_sqrt) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    adam_update(p, m, v, i, g[i], b1, b2, eps, step_size, bc2_sqrt);
}

__global__ void philox_fill_kernel(float* __restrict__ out, int N, int K, int d, long long k_offset,
                                   uint32_t seed_lo, uint32_t seed_hi, uint32_t iter) {
    // one thread per Philox call: (step n, trajectory k, call idx = 4b+q) -> features 16b+4r+q
    const int ncall = ((d + 15) / 16) * 4;
    const long long total = (long long)N * K * ncall;
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const int idx = (int)(t % ncall);
    const long long r0 = t / ncall;
    const int k = (int)(r0 % K), n = (int)(r0 / K);
    const psp::f32x4 z = psp::philox_block((uint32_t)(k_offset + k), (uint32_t)n, (uint32_t)idx, iter, seed_lo, seed_hi);
    const int b = idx >> 2, q = idx & 3;
    for (int r = 0; r < 4; ++r) {
        const int f = 16 * b + 4 * r + q;
        if (f < d) out[((size_t)(n + 1) * K + k) * d + f] = z[r];
    }
}

__global__ void zero_kernel(float* __restrict__ out, long long n) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = 0.f;
}

// u = -Z(t, x): plain per-output kernel (evaluation only, not on the training hot path)
__global__ void control_eval_kernel(int d, int H, const float* __restrict__ P, const float* __restrict__ X,
                                    int K, float t, float* __restrict__ out) {
    extern __shared__ float sm[];                 // h1[H], h2[H] for one trajectory per workgroup
    float* h1 = sm; float* h2 = sm + H;
    const int k = blockIdx.x;
    const int oW1 = 0, ob1 = H * (d + 1), oW2 = ob1 + H, ob2 = oW2 + H * H, oW3 = ob2 + H, ob3 = oW3 + d * H;
    for (int o = threadIdx.x; o < H; o += blockDim.x) {
        float s = P[ob1 + o];
        s = fmaf(P[oW1 + o * (d + 1)], t, s);
        for (int i = 0; i < d; ++i) s = fmaf(P[oW1 + o * (d + 1) + 1 + i], X[(size_t)k * d + i], s);
        h1[o] = tanhf(s);
    }
    __syncthreads();
    for (int o = threadIdx.x; o < H; o += blockDim.x) {
        float s = P[ob2 + o];
        for (int i = 0; i < H; ++i) s = fmaf(P[oW2 + o * H + i], h1[i], s);
        h2[o] = tanhf(s);
    }
    __syncthreads();
    for (int o = threadIdx.x; o < d; o += blockDim.x) {
        float s = P[ob3 + o];
        for (int i = 0; i < H; ++i) s = fmaf(P[oW3 + o * H + i], h2[i], s);
        out[(size_t)k * d + o] = -s;
    }
}

}  // namespace

extern "C" {

int psp_version(void) { return PSP_VERSION; }
int psp_abi_struct_sizes(int32_t out[6]) {
    static_assert(sizeof(psp_iter_state) == 24, "psp_iter_state layout");
    if (!out) return fail(-1, "null output");
    out[0] = (int32_t)sizeof(psp_hjb_config); out[1] = (int32_t)sizeof(psp_hjb_sizes);
    out[2] = (int32_t)sizeof(psp_gen_config); out[3] = (int32_t)sizeof(psp_gen_sizes);
    out[4] = (int32_t)sizeof(psp_dnet_config); out[5] = (int32_t)sizeof(psp_dnet_sizes);
    return 0;
}
int psp_abi_struct_sizes2(int32_t out[2]) {
    if (!out) return fail(-1, "null output");
    out[0] = (int32_t)sizeof(psp_genl_config); out[1] = (int32_t)sizeof(psp_genl_sizes);
    return 0;
}
const char* psp_last_error(void) { return g_err; }

int psp_abi_struct_sizes3(int32_t out[1]) {
    if (!out) return fail(-1, "null output");
    out[0] = (int32_t)sizeof(psp_is_config);
    return 0;
}

// ---- importance sampling under the reference control u* / no control (hjbe_kernels.h) -----------------------------------------
namespace {
// every check of a psp_is_config, the LDS budget included (psp_is_query and psp_is_rollout share it)
int is_validate(const psp_is_config* c, int* lds_bytes) {
    if (!c) return fail(-1, "null config");
    if (c->K_local <= 0 || c->N <= 0 || c->d <= 0) return fail(-1, "non-positive d / K / N");
    if (c->d > psp::kIsMaxD) {
        snprintf(g_err, sizeof(g_err), "psp_is_rollout: d = %d is outside the native range d <= %d", c->d, psp::kIsMaxD);
        return -2;
    }
    if (c->control_kind < PSP_ISC_NONE || c->control_kind > PSP_ISC_GRID)
        return fail(-1, "control_kind out of range (PSP_ISC_NONE, PSP_ISC_TABLE, PSP_ISC_LINEAR, PSP_ISC_GRID)");
    if (!coeff_kinds_ok(*c)) return fail(-1, "config enum out of range");
    if (c->k_offset < 0 || c->K_global < (int64_t)c->K_local + c->k_offset) return fail(-1, "K_global must cover k_offset + K_local");
    if (!c->x0) return fail(-1, "null x0 in psp_is_config");
    if (c->drift_kind != PSP_DRIFT_ZERO && !c->drift) return fail(-1, "drift parameters missing");
    if (c->sigma_kind == PSP_SIGMA_DENSE && !c->sigma) return fail(-1, "sigma matrix missing");
    if (c->runcost_kind == PSP_RUNCOST_DIAG_QUAD && !c->runcost) return fail(-1, "running-cost vector missing");
    if (!c->term) return fail(-1, "terminal-cost vector missing");
    if (c->control_kind != PSP_ISC_NONE && !c->u_ref) return fail(-1, "control kinds TABLE / LINEAR / GRID need u_ref");
    long long ucells = 0;
    if (c->control_kind == PSP_ISC_GRID) {
        if (!c->u_group || !c->u_row) return fail(-1, "control kind PSP_ISC_GRID needs u_group and u_row");
        if (c->u_ntables <= 0 || c->u_nrows <= 0 || c->u_ncols <= 0) return fail(-1, "u_ntables / u_nrows / u_ncols must be positive");
        if (!(c->u_dx > 0.f) || !(c->u_xb > 0.f)) return fail(-1, "u_xb / u_dx must be positive");
        ucells = (long long)c->u_ntables * c->u_ncols;
    }
    const char* too_big = "psp_is_rollout: the coefficient tables and the u* data of one step do not fit the 160 KiB LDS";
    if (ucells > kMaxLds / 4) return fail(-3, too_big);
    const psp::IsLds L = psp::is_lds_layout(psp::is_bucket(c->d), c->control_kind, c->drift_kind == PSP_DRIFT_DENSE,
                                            c->sigma_kind == PSP_SIGMA_DENSE, c->u_ntables, c->u_ncols);
    if ((long long)L.total * 4 > kMaxLds) return fail(-3, too_big);
    const long long total = L.total;
    *lds_bytes = (int)(total * 4);
    return 0;
}
}  // namespace

int psp_is_query(const psp_is_config* c, int32_t* lds_bytes) {
    int bytes = 0;
    const int rc = is_validate(c, &bytes);
    if (rc) return rc;
    if (lds_bytes) *lds_bytes = bytes;
    return 0;
}

int psp_is_rollout(const psp_is_config* c, const float* xi, uint64_t seed, uint32_t iter, float* logw_out, float* XN_out,
                   void* stream) {
    int lds_bytes = 0;
    const int rc = is_validate(c, &lds_bytes);
    if (rc) return rc;
    if (!logw_out) return fail(-1, "null logw_out passed to psp_is_rollout");
    if (c->noise_mode == PSP_NOISE_SUPPLIED && !xi) return fail(-1, "supplied-noise mode needs xi");
    if ((long long)c->N * c->K_local * c->d >= (1LL << 40)) return fail(-1, "N * K_local * d too large");
    psp::IsArgs a;
    memset(&a, 0, sizeof(a));
    a.x0 = c->x0; a.xi = xi; a.drift = c->drift; a.sigma = c->sigma; a.runcost = c->runcost; a.term = c->term;
    a.uref = c->u_ref; a.ugroup = c->u_group; a.urow = c->u_row; a.logw = logw_out; a.XN = XN_out;
    a.k_offset = c->k_offset; a.K_global = c->K_global;
    a.d = c->d; a.K_local = c->K_local; a.N = c->N; a.ctrl = c->control_kind;
    a.drift_kind = c->drift_kind; a.sigma_kind = c->sigma_kind; a.runcost_kind = c->runcost_kind; a.term_kind = c->term_kind;
    a.noise_mode = c->noise_mode; a.dwell_form = c->dwell_form ? 1 : 0;
    a.u_ntables = c->u_ntables; a.u_nrows = c->u_nrows; a.u_ncols = c->u_ncols;
    a.dt = c->dt; a.sqdt = c->sqrt_dt; a.sigma_scale = c->sigma_scale; a.u_xb = c->u_xb; a.u_dx = c->u_dx; a.u_xhi = c->u_xhi;
    a.seed_lo = (uint32_t)seed; a.seed_hi = (uint32_t)(seed >> 32); a.iter = iter;
    const long long grid = ((long long)c->K_local + psp::kIsThreads - 1) / psp::kIsThreads;
    hipError_t e = psp::is_rollout_launch(a, (int)grid, lds_bytes, (hipStream_t)stream);
    return hip_rc(e, "hjbe_rollout_kernel launch");
}

// ---- the same rollout for wide states (hjbew_kernels.h) -------------------------------------------------------------------------
namespace {
// every check of a psp_is_config for the wide kernel (psp_isw_query and psp_isw_rollout share it); the pointer and kind checks
// word for word those of is_validate
int isw_validate(const psp_is_config* c, psp_isw_sizes* out) {
    if (!c) return fail(-1, "null config");
    if (c->K_local <= 0 || c->N <= 0 || c->d <= 0) return fail(-1, "non-positive d / K / N");
    if (c->d > PSP_ISW_MAX_D) {
        snprintf(g_err, sizeof(g_err), "psp_isw_rollout: d = %d is outside the native range d <= %d (a wider tile does not fit one "
                 "wave's registers without scratch)", c->d, PSP_ISW_MAX_D);
        return -2;
    }
    if (c->control_kind < PSP_ISC_NONE || c->control_kind > PSP_ISC_GRID)
        return fail(-1, "control_kind out of range (PSP_ISC_NONE, PSP_ISC_TABLE, PSP_ISC_LINEAR, PSP_ISC_GRID)");
    if (!coeff_kinds_ok(*c)) return fail(-1, "config enum out of range");
    if (c->k_offset < 0 || c->K_global < (int64_t)c->K_local + c->k_offset) return fail(-1, "K_global must cover k_offset + K_local");
    if (!c->x0) return fail(-1, "null x0 in psp_is_config");
    if (c->drift_kind != PSP_DRIFT_ZERO && !c->drift) return fail(-1, "drift parameters missing");
    if (c->sigma_kind == PSP_SIGMA_DENSE && !c->sigma) return fail(-1, "sigma matrix missing");
    if (c->runcost_kind == PSP_RUNCOST_DIAG_QUAD && !c->runcost) return fail(-1, "running-cost vector missing");
    if (!c->term) return fail(-1, "terminal-cost vector missing");
    if (c->control_kind != PSP_ISC_NONE && !c->u_ref) return fail(-1, "control kinds TABLE / LINEAR / GRID need u_ref");
    long long lds = 0;
    if (c->control_kind == PSP_ISC_GRID) {
        if (!c->u_group || !c->u_row) return fail(-1, "control kind PSP_ISC_GRID needs u_group and u_row");
        if (c->u_ntables <= 0 || c->u_nrows <= 0 || c->u_ncols <= 0) return fail(-1, "u_ntables / u_nrows / u_ncols must be positive");
        if (!(c->u_dx > 0.f) || !(c->u_xb > 0.f)) return fail(-1, "u_xb / u_dx must be positive");
        lds = 4LL * c->u_ntables * c->u_ncols;
        if (lds > kMaxLds) return fail(-3, "psp_isw_rollout: the u* rows of one step do not fit the 160 KiB LDS");
    }
    const psp::IswTables L = psp::isw_table_layout(c->d, c->N, c->control_kind, c->drift_kind == PSP_DRIFT_DENSE,
                                                   c->sigma_kind == PSP_SIGMA_DENSE);
    static_assert(PSP_ISW_MAX_D == psp::kIswMaxD, "include/psp.h and hjbew_kernels.h disagree");
    out->struct_bytes = (int32_t)sizeof(psp_isw_sizes);
    out->lds_bytes = (int32_t)lds;
    out->table_bytes = 4 * L.total;
    out->workgroups = (int32_t)((((long long)c->K_local + 15) / 16 + psp::kIswWaves - 1) / psp::kIswWaves);
    out->max_d = PSP_ISW_MAX_D;
    return 0;
}
}  // namespace

int psp_isw_query(const psp_is_config* c, psp_isw_sizes* sizes) {
    if (!sizes) return fail(-1, "null sizes passed to psp_isw_query");
    if (sizes->struct_bytes != (int32_t)sizeof(psp_isw_sizes)) {
        snprintf(g_err, sizeof(g_err), "psp_isw_sizes.struct_bytes = %d, the library's struct has %d bytes", sizes->struct_bytes,
                 (int)sizeof(psp_isw_sizes));
        return -1;
    }
    psp_isw_sizes s;
    const int rc = isw_validate(c, &s);
    if (rc) return rc;
    *sizes = s;
    return 0;
}

int psp_isw_rollout(const psp_is_config* c, const float* xi, uint64_t seed, uint32_t iter, float* tables, float* logw_out,
                    float* XN_out, void* stream) {
    psp_isw_sizes s;
    const int rc = isw_validate(c, &s);
    if (rc) return rc;
    if (!logw_out) return fail(-1, "null logw_out passed to psp_isw_rollout");
    if (!tables || ((uintptr_t)tables & 15)) return fail(-1, "psp_isw_rollout needs 16-byte aligned tables (psp_isw_sizes.table_bytes)");
    if (c->noise_mode == PSP_NOISE_SUPPLIED && !xi) return fail(-1, "supplied-noise mode needs xi");
    if ((long long)c->N * c->K_local * c->d >= (1LL << 40)) return fail(-1, "N * K_local * d too large");
    psp::IswArgs w;
    memset(&w, 0, sizeof(w));
    psp::IsArgs& a = w.a;
    a.x0 = c->x0; a.xi = xi; a.drift = c->drift; a.sigma = c->sigma; a.runcost = c->runcost; a.term = c->term;
    a.uref = c->u_ref; a.ugroup = c->u_group; a.urow = c->u_row; a.logw = logw_out; a.XN = XN_out;
    a.k_offset = c->k_offset; a.K_global = c->K_global;
    a.d = c->d; a.K_local = c->K_local; a.N = c->N; a.ctrl = c->control_kind;
    a.drift_kind = c->drift_kind; a.sigma_kind = c->sigma_kind; a.runcost_kind = c->runcost_kind; a.term_kind = c->term_kind;
    a.noise_mode = c->noise_mode; a.dwell_form = c->dwell_form ? 1 : 0;
    a.u_ntables = c->u_ntables; a.u_nrows = c->u_nrows; a.u_ncols = c->u_ncols;
    a.dt = c->dt; a.sqdt = c->sqrt_dt; a.sigma_scale = c->sigma_scale; a.u_xb = c->u_xb; a.u_dx = c->u_dx; a.u_xhi = c->u_xhi;
    a.seed_lo = (uint32_t)seed; a.seed_hi = (uint32_t)(seed >> 32); a.iter = iter;
    w.tab = tables;
    w.L = psp::isw_table_layout(c->d, c->N, c->control_kind, c->drift_kind == PSP_DRIFT_DENSE, c->sigma_kind == PSP_SIGMA_DENSE);
    hipError_t e = psp::isw_rollout_launch(w, s.workgroups, s.lds_bytes, (hipStream_t)stream);
    return hip_rc(e, "isw_rollout_kernel launch");
}

// ---- DenseNet control (hjbd_kernels.h): time_approx='outer' and DenseNet(d+1 -> d) controls ---------------------
namespace {
// The DenseNet-control family takes four coefficient kinds more than the families that share coeff_kinds_ok (include/psp.h:
// PSP_DRIFT_WELL_DIAG / _RADIAL_WELL, PSP_TERM_QUAD_LINEAR / _RADIAL_QUAD): they are mapped onto kinds of the shared check here
bool dnet_kinds_ok(const psp_hjb_config& b) {
    psp_hjb_config c = b;
    if (c.drift_kind == PSP_DRIFT_WELL_DIAG || c.drift_kind == PSP_DRIFT_RADIAL_WELL) c.drift_kind = PSP_DRIFT_DIAG;
    if (c.term_kind == PSP_TERM_QUAD_LINEAR || c.term_kind == PSP_TERM_RADIAL_QUAD) c.term_kind = PSP_TERM_LINEAR;
    return coeff_kinds_ok(c);
}
struct DnetPlan { psp::DnetInstance inst; int ntile16, grid; long long table_floats, n_params; int slices, bwd_grid, bwd_ok; bool ul2;
                  long long ul2_gofs; };
int make_dnet_plan(const psp_dnet_config* c, DnetPlan* p) {
    if (!c) return fail(-1, "null config");
    const psp_hjb_config& b = c->base;
    if (b.d <= 0 || b.H <= 0 || b.K_local <= 0 || b.N <= 0) return fail(-1, "non-positive d/H/K/N");
    if (!find_in(kDnetTable, b.d, b.H, &p->inst)) {
        snprintf(g_err, sizeof(g_err), "no compiled DenseNet-control kernel instance for d=%d H=%d", b.d, b.H);
        return -2;
    }
    if (c->d_real <= 0 || c->d_real > b.d || c->H_real <= 0 || c->H_real > b.H)
        return fail(-1, "d_real / H_real must lie in [1, d] / [1, H] of the instance");
    if (!dnet_kinds_ok(b) || b.store_path < 0 || b.store_path > 3 || b.loss_kind < 0 || b.loss_kind > 3)
        return fail(-1, "config enum out of range");
    if ((b.drift_kind == PSP_DRIFT_WELL_DIAG || b.term_kind == PSP_TERM_QUAD_LINEAR) && (b.coord_split < 0 || b.coord_split > c->d_real))
        return fail(-1, "coord_split must lie in [0, d_real] (PSP_DRIFT_WELL_DIAG / PSP_TERM_QUAD_LINEAR)");
    const bool own_kinds = b.drift_kind >= PSP_DRIFT_WELL_DIAG || b.term_kind >= PSP_TERM_QUAD_LINEAR;
    if (own_kinds && b.mlp_dtype == PSP_MLP_F16X3 && b.store_path >= 2 && !psp::dnet_adj_x3_has_kinds(b.d, b.H))
        return fail(-3, "the split-product adjoint sweep of this instance does not carry the per-coordinate / radial kinds (they would "
                        "cost it scratch registers): use PSP_MLP_FP32");
    if (b.drift_kind == PSP_DRIFT_RADIAL_WELL && b.mlp_dtype == PSP_MLP_F16X3 && b.store_path >= 2 && !psp::dnet_adj_x3_has_radial(b.d, b.H))
        return fail(-3, "the split-product adjoint sweep of this instance does not carry the radial drift (it would cost it occupancy): "
                        "use PSP_MLP_FP32");
    if (own_kinds && c->ul2_kind == PSP_UL2_TABLE && b.u_ref)
        return fail(-3, "the u_L2 log of an x-independent u* (PSP_UL2_TABLE) is not built for the per-coordinate / radial kinds");
    if (p->inst.lds_bytes > kMaxLds) return fail(-3, "DenseNet-control kernel images do not fit the 160 KiB LDS");
    if (b.mlp_dtype == PSP_MLP_F16X3 && (!p->inst.launch_fwd_x3 || p->inst.lds_bytes_x3 > kMaxLds))
        return fail(-3, "split-product forward images do not fit the 160 KiB LDS for this (d,H)");
    p->ntile16 = (b.K_local + 15) / 16;
    p->grid = (p->ntile16 + 3) / 4;
    p->table_floats = (long long)p->inst.shared_floats + (long long)(c->per_step ? b.N : 1) * p->inst.set_floats +
                      (long long)b.N * p->inst.vec_floats;
    // u_L2 log (psp_dnet_config.ul2_*), validated before any launch
    if (c->ul2_kind < PSP_UL2_TABLE || c->ul2_kind > PSP_UL2_GRID)
        return fail(-1, "ul2_kind out of range (PSP_UL2_TABLE, PSP_UL2_LINEAR, PSP_UL2_GRID)");
    p->ul2 = b.u_ref != nullptr || c->ul2_kind != PSP_UL2_TABLE;
    if (c->ul2_kind != PSP_UL2_TABLE) {
        if (b.u_ref) return fail(-1, "base.u_ref is the PSP_UL2_TABLE reference; ul2_kind 1 / 2 read ul2_tables");
        if (!c->ul2_tables) return fail(-1, "ul2_kind 1 / 2 needs ul2_tables");
    }
    if (c->ul2_kind == PSP_UL2_GRID) {
        if (!c->ul2_group) return fail(-1, "ul2_kind PSP_UL2_GRID needs ul2_group");
        if (!c->ul2_row) return fail(-1, "ul2_kind PSP_UL2_GRID needs ul2_row");
        if (c->ul2_ntables <= 0 || c->ul2_nrows <= 0 || c->ul2_ncols <= 0)
            return fail(-1, "ul2_ntables / ul2_nrows / ul2_ncols must be positive");
        if (!(c->ul2_dx > 0.f) || !(c->ul2_xb > 0.f)) return fail(-1, "ul2_xb / ul2_dx must be positive");
    }
    if (p->ul2 && !b.u_l2_out) return fail(-1, "the u_L2 log (base.u_ref or ul2_kind) needs base.u_l2_out");
    // kind 1: the gains M_n as fp32 A-operand tables (N x d^2 floats, DGeo::GAINF) behind the rollout's tables
    p->ul2_gofs = p->table_floats;
    if (c->ul2_kind == PSP_UL2_LINEAR) p->table_floats += (long long)b.N * b.d * b.d;
    const long long di = c->d_real + (c->time_input ? 1 : 0), h = c->H_real, d = c->d_real;
    p->n_params = di * h + h + (di + h) * h + h + (di + 2 * h) * d + d;
    // backward work items = (step, slice): about two waves of workgroups over the chip, at least one round per item
    const int cus = n_cus();
    int S = (2 * cus + b.N / 2) / b.N;
    const int smax = (p->ntile16 + 3) / 4;
    if (S > smax) S = smax;
    if (S < 1) S = 1;
    p->slices = S;
    const long long items = (long long)b.N * S;
    p->bwd_grid = (int)(items < cus ? items : cus);
    p->bwd_ok = (p->inst.bwd_lds_bytes <= kMaxLds && p->inst.bwd_passes > 0) ? 1 : 0;   // else: too many accumulator tiles per wave
    return 0;
}
// the net's own shape, as every psp_dnet_* launch passes it
void fill_dnet_shape(const psp_dnet_config* c, psp::DnetArgs* a) {
    a->d_real = c->d_real; a->h_real = c->H_real; a->time_input = c->time_input ? 1 : 0; a->per_step = c->per_step ? 1 : 0;
}
// the arguments of the weight-gradient outer products (psp_dnet_rollout_bwd and psp_dnet_rollout_bwd_sq)
psp::DnetArgs dnet_bwd_args(const psp_dnet_config* c, const DnetPlan& p, const float* params, const float* images, const float* w,
                            float* partial) {
    const psp_hjb_config* b = &c->base;
    psp::DnetArgs a;
    memset(&a, 0, sizeof(a));
    a.h.params = params; a.h.K_local = b->K_local; a.h.N = b->N; a.h.ntile16 = p.ntile16; a.h.sqdt = b->sqrt_dt; a.h.dt = b->dt;
    a.pimg = const_cast<float*>(images); a.wts = w; a.partial = partial; a.slices = p.slices;
    fill_dnet_shape(c, &a);
    return a;
}
}  // namespace

extern "C" int psp_dnet_instance_count(void) { return table_count(kDnetTable); }
extern "C" int psp_dnet_instance_get(int32_t i, int32_t* d, int32_t* H) { return table_get(kDnetTable, i, d, H); }

extern "C" int psp_dnet_query(const psp_dnet_config* cfg, psp_dnet_sizes* out) {
    DnetPlan p;
    int rc = make_dnet_plan(cfg, &p);
    if (rc) return rc;
    if (!out) return fail(-1, "null output");
    out->table_bytes = p.table_floats * 4;
    out->fwd_partial_bytes = (int64_t)p.grid * 2 * 8;
    out->n_params_per_set = p.n_params;
    out->fwd_workgroups = p.grid;
    out->reserved = 0;
    out->image_bytes = (int64_t)cfg->base.N * p.ntile16 * p.inst.image_block_floats * 4;
    out->partial_bytes = (int64_t)cfg->base.N * p.slices * p.inst.partial_floats * 4;
    out->bwd_supported = p.bwd_ok; out->slices = p.slices; out->padded_params = p.inst.partial_floats;
    out->bwd_workgroups = p.bwd_grid;
    return 0;
}

extern "C" int psp_dnet_terminal_reduce(const psp_dnet_config* cfg, const double* fwd_partial, double* sums_out, void* stream) {
    DnetPlan p;
    int rc = make_dnet_plan(cfg, &p);
    if (rc) return rc;
    if (!fwd_partial || !sums_out) return fail(-1, "null buffer passed to psp_dnet_terminal_reduce");
    return PSP_LAUNCH(reduce_partials_kernel, dim3(1), dim3(256), 0, stream, fwd_partial, p.grid, sums_out);
}

extern "C" int psp_dnet_rollout_bwd(const psp_dnet_config* cfg, const float* params, const float* images, const float* w,
                                    float* partial, void* stream) {
    DnetPlan p;
    int rc = make_dnet_plan(cfg, &p);
    if (rc) return rc;
    if (!p.bwd_ok) return fail(-3, "the hand-written DenseNet-control backward does not cover this instance (accumulator tiles)");
    if (!params || !images || !w || !partial) return fail(-1, "null buffer passed to psp_dnet_rollout_bwd");
    const psp_hjb_config* b = &cfg->base;
    psp::DnetArgs a = dnet_bwd_args(cfg, p, params, images, w, partial);
    // split-product outer products where the stored image is the Brownian increment itself (detached adaptive run: the power-of-two
    // scale of the weight-carrying tiles then needs nothing but the weights); guarded by the fp32 kernel like the other split kernels
    const bool x3 = b->mlp_dtype == PSP_MLP_F16X3 && b->adaptive && b->store_path == 1 && p.inst.launch_bwd_x3;
    auto fp32 = [&]() { return p.inst.launch_bwd(a, p.bwd_grid, (hipStream_t)stream); };
    const hipError_t e = !x3 ? fp32() : launch_either(b->range_flag, a.h.cond, a.h.cond_want,
                                                      [&]() { return p.inst.launch_bwd_x3(a, p.bwd_grid, (hipStream_t)stream); }, fp32);
    return hip_rc(e, "hjbd_bwd_kernel launch");
}

extern "C" int psp_dnet_rollout_bwd_sq(const psp_dnet_config* cfg, const float* params, const float* images, const float* w,
                                       float* partial, void* stream) {
    DnetPlan p;
    int rc = make_dnet_plan(cfg, &p);
    if (rc) return rc;
    if (!p.bwd_ok || !p.inst.launch_bwd_sq)
        return fail(-3, "the hand-written DenseNet-control backward does not cover this instance (accumulator tiles)");
    if (!params || !images || !w || !partial) return fail(-1, "null buffer passed to psp_dnet_rollout_bwd_sq");
    // always the fp32 MFMAs, never predicated on the range flag: squares of ~1/K-scaled tiles have no place on the f16 pipe
    const psp::DnetArgs a = dnet_bwd_args(cfg, p, params, images, w, partial);
    return hip_rc(p.inst.launch_bwd_sq(a, p.bwd_grid, (hipStream_t)stream), "hjbd_bwd_kernel (squared outer products) launch");
}

// ---- gradient-variance diagnostic: slices -> moments -> sqrt(var) / mean, one workgroup per time step -----------------------
namespace {
struct GradvarArgs {
    const float *pS, *pQ, *pS2, *pS1, *gg;
    const long long* gidx;
    const double* csums;
    float *mean, *var, *rel;
    double* step_sums;
    long long Pset, PP;
    int N, slices, K, kind;
};
// The raw moments are combined in double: sum f = 2 (S - B sum c), sum f^2 = 4 (Q - 2 B S2 + B^2 sum c^2) with B = Gg (moment;
// 0 without it) or S[1] / K (log-variance).  mean, var are rounded to fp32 and rel formed in fp32 from them, as the reference's
// fp32 tensors are; var is clamped at 0 BEFORE the root (a rounding-negative raw moment must not turn into a NaN that the NaN -> 0
// rule then hides); NaN -> 0 (0 / 0 of a dead unit), inf and negative values stay.
__global__ __launch_bounds__(256) void gradvar_finish_kernel(const GradvarArgs a) {
    __shared__ double red[256];
    const int n = blockIdx.x;
    const double K = (double)a.K, sc = a.csums[0], sc2 = a.csums[1];
    double acc = 0.0;
    for (long long q = threadIdx.x; q < a.Pset; q += blockDim.x) {
        const long long col = a.gidx[q];
        double S = 0.0, Q = 0.0, S2 = 0.0, S1 = 0.0;
        for (int sl = 0; sl < a.slices; ++sl) {
            const size_t o = ((size_t)n * a.slices + sl) * (size_t)a.PP + (size_t)col;
            S += (double)a.pS[o];
            Q += (double)a.pQ[o];
            if (a.pS2) S2 += (double)a.pS2[o];
            if (a.pS1) S1 += (double)a.pS1[o];
        }
        const double B = a.kind == 1 ? S1 / K : (a.gg ? (double)a.gg[(size_t)n * a.Pset + q] : 0.0);
        const double sf = 2.0 * (S - B * sc);
        const double sf2 = 4.0 * (Q - 2.0 * B * S2 + B * B * sc2);
        double var = (sf2 - sf * sf / K) / (K - 1.0);
        if (var < 0.0) var = 0.0;
        const float mf = (float)(sf / K), vf = (float)var;
        // fp32 root and quotient, correctly rounded (through double: 53 >= 2 * 24 + 2 bits make both roundings exact), so that rel is
        // bit for bit what torch.sqrt(var) / mean gives for the fp32 mean and var written above
        const float root = (float)sqrt((double)vf);
        float r = (float)((double)root / (double)mf);
        if (r != r) r = 0.f;
        const size_t o = (size_t)n * a.Pset + q;
        a.mean[o] = mf; a.var[o] = vf; a.rel[o] = r;
        acc += (double)r;
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) a.step_sums[n] = red[0];
}
__global__ __launch_bounds__(64) void gradvar_mean_kernel(const double* __restrict__ step_sums, int N, long long Pset,
                                                          float* __restrict__ out) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        double s = 0.0;
        for (int n = 0; n < N; ++n) s += step_sums[n];
        out[0] = (float)(s / ((double)N * (double)Pset));
    }
}
}  // namespace

extern "C" int psp_gradvar_finish(const float* pS, const float* pQ, const float* pS2, const float* pS1, const float* gg,
                                  const int64_t* gather_index, int32_t N, int32_t slices, int64_t padded_params,
                                  int64_t n_params_per_set, int32_t K, int32_t loss_kind, const double* csums,
                                  float* mean_out, float* var_out, float* rel_out, double* step_sums, float* rel_mean_out,
                                  void* stream) {
    if (!pS || !pQ || !gather_index || !csums || !mean_out || !var_out || !rel_out || !step_sums || !rel_mean_out)
        return fail(-1, "null buffer passed to psp_gradvar_finish");
    if (N <= 0 || slices <= 0 || padded_params <= 0 || n_params_per_set <= 0 || n_params_per_set > padded_params)
        return fail(-1, "psp_gradvar_finish: N, slices, padded_params, n_params_per_set must be positive, n_params_per_set <= padded_params");
    if (K < 2) return fail(-1, "psp_gradvar_finish: the unbiased variance needs K >= 2");
    if (loss_kind != PSP_LOSS_MOMENT && loss_kind != PSP_LOSS_LOG_VARIANCE)
        return fail(-1, "psp_gradvar_finish: loss_kind must be PSP_LOSS_MOMENT or PSP_LOSS_LOG_VARIANCE");
    if (loss_kind == PSP_LOSS_LOG_VARIANCE && (!pS2 || !pS1)) return fail(-1, "psp_gradvar_finish: log-variance needs S[c^2] and S[1]");
    if (loss_kind == PSP_LOSS_MOMENT && gg && !pS2) return fail(-1, "psp_gradvar_finish: moment with Gg needs S[c^2]");
    GradvarArgs a;
    memset(&a, 0, sizeof(a));
    a.pS = pS; a.pQ = pQ; a.pS2 = pS2; a.pS1 = loss_kind == PSP_LOSS_LOG_VARIANCE ? pS1 : nullptr;
    a.gg = loss_kind == PSP_LOSS_MOMENT ? gg : nullptr;
    a.gidx = reinterpret_cast<const long long*>(gather_index); a.csums = csums;
    a.mean = mean_out; a.var = var_out; a.rel = rel_out; a.step_sums = step_sums;
    a.Pset = n_params_per_set; a.PP = padded_params; a.N = N; a.slices = slices; a.K = K;
    a.kind = loss_kind == PSP_LOSS_LOG_VARIANCE ? 1 : 0;
    int rc = PSP_LAUNCH(gradvar_finish_kernel, dim3(N), dim3(256), 0, stream, a);
    if (rc) return rc;
    return PSP_LAUNCH(gradvar_mean_kernel, dim3(1), dim3(64), 0, stream, (const double*)step_sums, (int)N, (long long)n_params_per_set,
                      rel_mean_out);
}

extern "C" int psp_dnet_adjoint_sweep(const psp_dnet_config* cfg, const float* params, float* images, const float* XN,
                                      const float* mu, const float* nu, const float* wT, float* tables, void* stream) {
    DnetPlan p;
    int rc = make_dnet_plan(cfg, &p);
    if (rc) return rc;
    const psp_hjb_config* b = &cfg->base;
    if ((rc = check_ptrs(b))) return rc;
    if (!params || !images || !XN || !mu || !tables) return fail(-1, "null buffer passed to psp_dnet_adjoint_sweep");
    if (b->store_path != 2 && b->store_path != 3) return fail(-1, "psp_dnet_adjoint_sweep needs store_path 2 or 3 (the forward's image kind)");
    if (b->store_path == 3 && !nu) return fail(-1, "store_path 3 (relative entropy) needs nu");
    psp::DnetArgs a;
    memset(&a, 0, sizeof(a));
    psp::HjbArgs& h = a.h;
    fill_problem(b, p.ntile16, &h);
    h.params = params; h.XN = const_cast<float*>(XN); h.adj_mu = mu; h.adj_nu = nu; h.adj_wT = wT;
    a.tbl = tables; a.pimg = images;
    fill_dnet_shape(cfg, &a);
    a.coord_split = b->coord_split;
    const bool x3 = b->mlp_dtype == PSP_MLP_F16X3 && p.inst.launch_adj_x3 && p.inst.lds_bytes_x3 <= kMaxLds;
    auto fp32 = [&]() { return p.inst.launch_adj(a, p.grid, (hipStream_t)stream); };
    const hipError_t e = !x3 ? fp32() : launch_either(b->range_flag, h.cond, h.cond_want,           // range guard: both sweeps, predicated
                                                      [&]() { return p.inst.launch_adj_x3(a, p.grid, (hipStream_t)stream); }, fp32);
    return hip_rc(e, "hjbd_adj_kernel launch");
}

extern "C" int psp_dnet_ul2_stage(const psp_dnet_config* cfg, float* tables, void* stream) {
    DnetPlan p;
    int rc = make_dnet_plan(cfg, &p);
    if (rc) return rc;
    if (cfg->ul2_kind != PSP_UL2_LINEAR) return 0;
    if (!tables) return fail(-1, "null buffer passed to psp_dnet_ul2_stage");
    psp::DnetArgs a;
    memset(&a, 0, sizeof(a));
    a.h.N = cfg->base.N; a.h.uref = cfg->ul2_tables;
    a.tbl = tables; a.ul2_gofs = p.ul2_gofs;
    hipError_t e = p.inst.launch_ul2_stage(a, (hipStream_t)stream);
    return hip_rc(e, "hjbd_tables_kernel (gain tables) launch");
}

extern "C" int psp_dnet_rollout_fwd(const psp_dnet_config* cfg, const float* params, const float* x0, int32_t x0_stride,
                                    const float* y0, const float* xi, uint64_t seed, uint32_t iter, const float* tfeat,
                                    float* px, float* pxi, float* D_out, float* Fint_out, float* XN_out, float* Y_out,
                                    double* fwd_partial, float* tables, void* stream) {
    DnetPlan p;
    int rc = make_dnet_plan(cfg, &p);
    if (rc) return rc;
    const psp_hjb_config* b = &cfg->base;
    if ((rc = check_ptrs(b))) return rc;
    if (!params || !x0 || !D_out || !fwd_partial || !tables) return fail(-1, "null buffer passed to psp_dnet_rollout_fwd");
    if (x0_stride != 0 && x0_stride != b->d) return fail(-1, "x0_stride must be 0 or d");
    if (b->noise_mode == PSP_NOISE_SUPPLIED && !xi) return fail(-1, "supplied-noise mode needs xi");
    if (b->store_path && !cfg->images_out && (!px || !pxi)) return fail(-1, "store_path set but the X / xi stores are null");
    if (b->store_path >= 2 && !cfg->images_out)
        return fail(-1, "store_path 2 / 3 (adjoint sweep) need the register images (psp_dnet_config.images_out)");
    psp::DnetArgs a;
    memset(&a, 0, sizeof(a));
    psp::HjbArgs& h = a.h;
    fill_problem(b, p.ntile16, &h);
    h.k_offset = b->k_offset; h.K_global = b->K_global; h.loss_kind = b->loss_kind; h.noise_mode = b->noise_mode;
    h.params = params; h.x0 = x0; h.x0_stride = x0_stride; h.y0 = y0; h.xi = xi; h.tfeat = tfeat;
    h.D = D_out; h.Fint = Fint_out; h.XN = XN_out; h.Yout = Y_out; h.fwd_partial = fwd_partial;
    h.seed_lo = (uint32_t)seed; h.seed_hi = (uint32_t)(seed >> 32); h.iter = iter;
    a.tbl = tables; a.px = px; a.pxi = pxi;
    if ((cfg->r1_out == nullptr) != (cfg->r2_out == nullptr)) return fail(-1, "r1_out and r2_out go together");
    a.pr1 = cfg->r1_out; a.pr2 = cfg->r2_out; a.pimg = cfg->images_out;
    fill_dnet_shape(cfg, &a);
    a.coord_split = b->coord_split;
    if (p.ul2) {                               // u_L2 log: h.uref = the kind's reference data (non-null selects the LOGU kernels)
        h.uref = cfg->ul2_kind == PSP_UL2_TABLE ? b->u_ref : cfg->ul2_tables;
        h.ul2 = b->u_l2_out;
        a.ul2_kind = cfg->ul2_kind; a.ul2_group = cfg->ul2_group; a.ul2_row = cfg->ul2_row;
        a.ul2_ntables = cfg->ul2_ntables; a.ul2_nrows = cfg->ul2_nrows; a.ul2_ncols = cfg->ul2_ncols;
        a.ul2_xb = cfg->ul2_xb; a.ul2_dx = cfg->ul2_dx; a.ul2_xhi = cfg->ul2_xhi; a.ul2_gofs = p.ul2_gofs;
    }
    const bool x3 = b->mlp_dtype == PSP_MLP_F16X3 && p.inst.launch_fwd_x3 && p.inst.lds_bytes_x3 <= kMaxLds;
    if (b->mlp_dtype == PSP_MLP_F16X3 && !x3) return fail(-3, "split-product forward images do not fit the 160 KiB LDS for this (d,H)");
    auto fp32 = [&]() { return p.inst.launch_fwd(a, p.grid, (hipStream_t)stream); };
    if (x3)     // range guard (psp_hjb_config.range_flag): non-finite partials -> flag -> the fp32-MFMA rollout, predicated
        return launch_redo(b->range_flag, h.cond, h.cond_want, "hjbd_fwd_kernel launch",
                           [&]() { return p.inst.launch_fwd_x3(a, p.grid, (hipStream_t)stream); },
                           [&]() { return PSP_LAUNCH(range_flag_partials_kernel, dim3(1), dim3(256), 0, stream, fwd_partial, 2 * p.grid, b->range_flag); },
                           fp32);
    const hipError_t e = fp32();
    return hip_rc(e, "hjbd_fwd_kernel launch");
}

// ---- linear / affine / constant controls (aff_kernels.h): time_approx='outer' with a list of Linear / Affine / Constant ---------
namespace {
const Entry<psp::AffInstance> kAffTable[] = {{16, 0, &psp::aff_instance_16}, {32, 0, &psp::aff_instance_32}, {64, 0, &psp::aff_instance_64}};

struct AffPlan { psp::AffInstance inst; int threads, grid, lds_fwd, lds_adj, slices, slice_len, bwd_grid; bool ul2; };
// every check of a psp_aff_config (psp_aff_query and the four entry points share it)
int make_aff_plan(const psp_aff_config* c, AffPlan* p) {
    if (!c) return fail(-1, "null config");
    if (c->struct_bytes != (int32_t)sizeof(psp_aff_config)) return fail(-1, "psp_aff_config.struct_bytes is not sizeof(psp_aff_config)");
    const psp_hjb_config& b = c->base;
    if (b.H != 0) return fail(-3, "psp_aff_config: base.H must be 0 (the control has no hidden layer)");
    if (b.mlp_dtype != PSP_MLP_FP32) return fail(-3, "psp_aff_config: base.mlp_dtype must be PSP_MLP_FP32 (fp32 arithmetic only)");
    if (b.d <= 0 || b.K_local <= 0 || b.N <= 0) return fail(-1, "non-positive d/K/N");
    if (!find_in(kAffTable, b.d, 0, &p->inst)) {
        snprintf(g_err, sizeof(g_err), "no compiled linear-control kernel bucket of width d=%d (16, 32, 64)", b.d);
        return -2;
    }
    if (c->d_real <= 0 || c->d_real > b.d) return fail(-1, "d_real must lie in [1, d] of the bucket");
    if (!coeff_kinds_ok(b) || b.store_path < 0 || b.store_path > 3 || b.loss_kind < 0 || b.loss_kind > 3)
        return fail(-1, "config enum out of range");
    if (b.k_offset < 0 || b.K_global < (int64_t)b.K_local + b.k_offset) return fail(-1, "K_global must cover k_offset + K_local");
    if (!c->has_matrix && !c->has_bias) return fail(-1, "psp_aff_config: has_matrix or has_bias (a control with neither is zero)");
    p->ul2 = b.u_l2_out != nullptr;
    if (p->ul2) {
        if (c->ul2_kind == PSP_UL2_GRID)
            return fail(-3, "psp_aff_config: PSP_UL2_GRID is not built for linear controls (PSP_UL2_TABLE, PSP_UL2_LINEAR are)");
        if (c->ul2_kind != PSP_UL2_TABLE && c->ul2_kind != PSP_UL2_LINEAR) return fail(-1, "ul2_kind out of range");
        if (!c->ul2_ref) return fail(-1, "the u_L2 log (base.u_l2_out) needs ul2_ref");
    }
    if ((long long)b.N * b.K_local * 2 * b.d >= (1LL << 40)) return fail(-1, "N * K_local * d too large");
    // one lane per trajectory: single-wave workgroups while they leave CUs idle, four waves beyond
    p->threads = (long long)b.K_local <= 64LL * n_cus() ? 64 : psp::kAffMaxThreads;
    p->grid = (b.K_local + p->threads - 1) / p->threads;
    const bool dA = b.drift_kind == PSP_DRIFT_DENSE, dB = b.sigma_kind == PSP_SIGMA_DENSE;
    p->lds_fwd = 4 * psp::aff_lds_layout(b.d, p->threads, dA, dB, c->has_matrix != 0, p->ul2 ? c->ul2_kind : psp::AFF_UL2_OFF).total;
    p->lds_adj = 4 * psp::aff_lds_layout(b.d, p->threads, dA, dB, c->has_matrix != 0, psp::AFF_UL2_OFF).total;
    if (p->lds_fwd > kMaxLds) return fail(-3, "linear-control kernel tables do not fit the 160 KiB LDS");
    // gradient work items = (step, slice): about two rounds of workgroups over the chip, slices of whole LDS stages
    const int cus = n_cus(), nchunk = (b.K_local + psp::kAffBwdChunk - 1) / psp::kAffBwdChunk;
    int S = (2 * cus + b.N / 2) / b.N;
    if (S > nchunk) S = nchunk;
    if (S < 1) S = 1;
    p->slice_len = ((nchunk + S - 1) / S) * psp::kAffBwdChunk;
    p->slices = (b.K_local + p->slice_len - 1) / p->slice_len;
    p->bwd_grid = b.N * p->slices;
    return 0;
}

void aff_fill(const psp_aff_config* c, const AffPlan& p, psp::AffArgs* a) {
    const psp_hjb_config& b = c->base;
    memset(a, 0, sizeof(*a));
    a->drift = b.drift; a->sigma = b.sigma; a->runcost = b.runcost; a->term = b.term;
    a->k_offset = b.k_offset; a->d = c->d_real; a->K_local = b.K_local; a->N = b.N;
    a->drift_kind = b.drift_kind; a->sigma_kind = b.sigma_kind; a->runcost_kind = b.runcost_kind; a->term_kind = b.term_kind;
    a->adaptive = b.adaptive ? 1 : 0; a->loss_kind = b.loss_kind; a->noise_mode = b.noise_mode; a->store_path = b.store_path;
    a->ul2_kind = c->ul2_kind; a->slices = p.slices; a->slice_len = p.slice_len;
    a->dt = b.dt; a->sqdt = b.sqrt_dt; a->sigma_scale = b.sigma_scale;
}
}  // namespace

int psp_aff_instance_count(void) { return table_count(kAffTable); }
int psp_aff_instance_get(int32_t i, int32_t* d) {
    int32_t H = 0;
    return table_get(kAffTable, i, d, &H);
}

int psp_aff_query(const psp_aff_config* cfg, psp_aff_sizes* out) {
    AffPlan p;
    const int rc = make_aff_plan(cfg, &p);
    if (rc) return rc;
    if (!out) return fail(-1, "null output");
    const psp_hjb_config& b = cfg->base;
    out->path_bytes = b.store_path ? (int64_t)b.N * b.K_local * 2 * b.d * 4 : 0;
    out->fwd_partial_bytes = (int64_t)p.grid * 2 * 8;
    out->padded_params = b.d * b.d + b.d;
    out->partial_bytes = (int64_t)b.N * p.slices * out->padded_params * 4;
    out->fwd_workgroups = p.grid; out->fwd_threads = p.threads; out->slices = p.slices;
    out->bwd_workgroups = p.bwd_grid; out->lds_bytes = p.lds_fwd;
    return 0;
}

int psp_aff_rollout_fwd(const psp_aff_config* cfg, const float* maps, const float* shifts, const float* x0, int32_t x0_stride,
                        const float* y0, const float* xi, uint64_t seed, uint32_t iter, float* path, float* D_out, float* XN_out,
                        float* Y_out, double* fwd_partial, void* stream) {
    AffPlan p;
    int rc = make_aff_plan(cfg, &p);
    if (rc) return rc;
    const psp_hjb_config* b = &cfg->base;
    if ((rc = check_ptrs(b))) return rc;
    if (!x0 || !D_out || !fwd_partial) return fail(-1, "null buffer passed to psp_aff_rollout_fwd");
    if ((cfg->has_matrix != 0) != (maps != nullptr)) return fail(-1, "psp_aff_rollout_fwd: maps go with has_matrix");
    if ((cfg->has_bias != 0) != (shifts != nullptr)) return fail(-1, "psp_aff_rollout_fwd: shifts go with has_bias");
    if (x0_stride != 0 && x0_stride != b->d) return fail(-1, "x0_stride must be 0 or d");
    if (b->noise_mode == PSP_NOISE_SUPPLIED && !xi) return fail(-1, "supplied-noise mode needs xi");
    if (b->store_path && !path) return fail(-1, "store_path set but path is null");
    psp::AffArgs a;
    aff_fill(cfg, p, &a);
    a.x0 = x0; a.x0_stride = x0_stride; a.y0 = y0; a.xi = xi; a.M = maps; a.c = shifts;
    a.uref = p.ul2 ? cfg->ul2_ref : nullptr; a.ul2 = b->u_l2_out;
    a.D = D_out; a.XN = XN_out; a.Yout = Y_out; a.fwd_partial = fwd_partial; a.path = path;
    a.seed_lo = (uint32_t)seed; a.seed_hi = (uint32_t)(seed >> 32); a.iter = iter;
    const hipError_t e = p.inst.launch_fwd(a, p.grid, p.threads, p.lds_fwd, (hipStream_t)stream);
    return hip_rc(e, "aff_fwd_kernel launch");
}

int psp_aff_terminal_reduce(const psp_aff_config* cfg, const double* fwd_partial, double* sums_out, void* stream) {
    AffPlan p;
    const int rc = make_aff_plan(cfg, &p);
    if (rc) return rc;
    if (!fwd_partial || !sums_out) return fail(-1, "null buffer passed to psp_aff_terminal_reduce");
    return PSP_LAUNCH(reduce_partials_kernel, dim3(1), dim3(256), 0, stream, fwd_partial, p.grid, sums_out);
}

int psp_aff_adjoint_sweep(const psp_aff_config* cfg, const float* maps, float* path, const float* XN, const float* mu,
                          const float* nu, const float* wT, void* stream) {
    AffPlan p;
    int rc = make_aff_plan(cfg, &p);
    if (rc) return rc;
    const psp_hjb_config* b = &cfg->base;
    if ((rc = check_ptrs(b))) return rc;
    if (!path || !XN || !mu) return fail(-1, "null buffer passed to psp_aff_adjoint_sweep");
    if ((cfg->has_matrix != 0) != (maps != nullptr)) return fail(-1, "psp_aff_adjoint_sweep: maps go with has_matrix");
    if (b->store_path != 2 && b->store_path != 3) return fail(-1, "psp_aff_adjoint_sweep needs store_path 2 or 3 (the forward's image kind)");
    if (b->store_path == 3 && !nu) return fail(-1, "store_path 3 (relative entropy) needs nu");
    if (!b->adaptive) return fail(-1, "psp_aff_adjoint_sweep: the state path carries parameters only with base.adaptive = 1");
    psp::AffArgs a;
    aff_fill(cfg, p, &a);
    a.M = maps; a.path = path; a.XN = const_cast<float*>(XN); a.mu = mu; a.nu = nu; a.wT = wT;
    const hipError_t e = p.inst.launch_adj(a, p.grid, p.threads, p.lds_adj, (hipStream_t)stream);
    return hip_rc(e, "aff_adj_kernel launch");
}

int psp_aff_rollout_bwd(const psp_aff_config* cfg, const float* path, const float* w, float* partial, void* stream) {
    AffPlan p;
    const int rc = make_aff_plan(cfg, &p);
    if (rc) return rc;
    if (!path || !w || !partial) return fail(-1, "null buffer passed to psp_aff_rollout_bwd");
    if (!cfg->base.store_path) return fail(-1, "psp_aff_rollout_bwd needs the path store (store_path 1, 2 or 3)");
    psp::AffArgs a;
    aff_fill(cfg, p, &a);
    a.path = const_cast<float*>(path); a.w = w; a.partial = partial; a.has_matrix = cfg->has_matrix ? 1 : 0;
    const hipError_t e = p.inst.launch_bwd(a, p.bwd_grid, (hipStream_t)stream);
    return hip_rc(e, "aff_bwd_kernel launch");
}

int psp_debug_set_stamp_buffer(unsigned long long* buf, int64_t n_entries) {
    g_dbg = buf;
    g_dbg_n = buf ? n_entries : 0;
#ifdef PSP_STAMPS
    return 1;
#else
    return 0;
#endif
}

static int64_t grad_rows_bytes(const Plan& p) {       // partial-gradient rows, padded to 256 B
    const int64_t b = (int64_t)p.bwd_grid * p.inst.n_params * 4;
    return (b + 255) / 256 * 256;
}

int psp_hjb_supported(int32_t d, int32_t H) {
    psp::HjbInstance inst;
    return find_instance(d, H, &inst) ? 1 : 0;
}

int psp_hjb_family(int32_t d, int32_t H) {
    psp::HjbInstance inst;
    if (!find_instance(d, H, &inst)) return 0;
    return inst.wide ? 2 : 1;
}

int psp_hjb_instance_count(void) { return table_count(kTable) + table_count(kWideTable); }

int psp_hjb_instance_get(int32_t i, int32_t* d, int32_t* H, int32_t* family) {      // the narrow table, then the wide one
    const int nn = table_count(kTable);
    if (!family) return fail(-1, "instance index out of range");
    const int rc = i < nn ? table_get(kTable, i, d, H) : table_get(kWideTable, i - nn, d, H);
    if (rc == 0) *family = i < nn ? 1 : 2;
    return rc;
}

int psp_hjb_query(const psp_hjb_config* cfg, psp_hjb_sizes* out) {
    Plan p;
    int rc = make_plan(cfg, &p);
    if (rc) return rc;
    if (!out) return fail(-1, "null output");
    memset(out, 0, sizeof(*out));
    out->n_params = p.inst.n_params;
    out->fwd_workgroups = p.fwd_grid;
    out->bwd_workgroups = p.bwd_grid;
    out->fwd_coop_tiles = p.fwd_coop ? p.fwd_waves : 0;
    out->path_bytes = cfg->store_path
        ? (int64_t)cfg->N * p.ntile16 * (int64_t)p.inst.path_floats_per_tile_step * 4 : 0;
    // the wide family keeps its A-operand tables behind the partial sums in the same caller-owned scratch
    out->fwd_partial_bytes = (int64_t)p.fwd_grid * 2 * 8 + (int64_t)p.inst.fwd_table_floats * 4;
    out->grad_partial_bytes = grad_rows_bytes(p) + (int64_t)p.inst.bwd_table_floats * 4;
    return 0;
}

int psp_hjb_rollout_fwd(const psp_hjb_config* cfg, const float* params, const float* x0, int32_t x0_stride,
                        const float* y0, const float* xi, uint64_t seed, uint32_t iter, float* path,
                        float* D_out, float* XN_out, float* Y_out, double* fwd_partial, void* stream) {
    Plan p;
    int rc = make_plan(cfg, &p);
    if (rc) return rc;
    if ((rc = check_ptrs(cfg))) return rc;
    if (!params || !x0 || !D_out || !fwd_partial) return fail(-1, "null buffer passed to psp_hjb_rollout_fwd");
    if (x0_stride != 0 && x0_stride != cfg->d) return fail(-1, "x0_stride must be 0 or d");
    if (cfg->noise_mode == PSP_NOISE_SUPPLIED && !xi) return fail(-1, "supplied-noise mode needs xi");
    if (cfg->store_path && !path) return fail(-1, "store_path set but path buffer is null");
    psp::HjbArgs a;
    fill_args(cfg, p, &a);
    a.params = params; a.x0 = x0; a.x0_stride = x0_stride; a.y0 = y0; a.xi = xi; a.path = path;
    a.D = D_out; a.XN = XN_out; a.Yout = Y_out; a.fwd_partial = fwd_partial;
    a.tables = reinterpret_cast<float*>(fwd_partial + 2 * (size_t)p.fwd_grid);
    a.seed_lo = (uint32_t)seed; a.seed_hi = (uint32_t)(seed >> 32); a.iter = iter;
    hipError_t e;
    if (cfg->mlp_dtype == PSP_MLP_BF16_FWD) {
        if (!p.inst.launch_fwd_bf16) return fail(-3, "the bf16 control-net mode exists for the narrow kernel family only");
        e = p.inst.launch_fwd_bf16(a, p.fwd_grid, p.fwd_waves * 64, (hipStream_t)stream);      // make_plan kept the tile-per-wave forward
    } else if (cfg->mlp_dtype == PSP_MLP_F16X3) {
        // range guard: non-finite partials -> flag -> the fp32-MFMA forward of the same launch, predicated on the flag
        // (same grid, same partials / D / path-store layout; it overwrites what the split kernel left)
        return launch_redo(cfg->range_flag, a.cond, a.cond_want, "hjb_fwd_kernel launch",
                           [&]() { return p.fwd_coop ? p.inst.launch_fwd_coop(a, p.fwd_grid, p.fwd_waves, (hipStream_t)stream)
                                                     : p.inst.launch_fwd_x3(a, p.fwd_grid, p.fwd_waves * 64, (hipStream_t)stream); },
                           [&]() { return PSP_LAUNCH(range_flag_partials_kernel, dim3(1), dim3(256), 0, stream, fwd_partial, 2 * p.fwd_grid, cfg->range_flag); },
                           [&]() { return p.inst.launch_fwd(a, p.fwd_grid, p.fwd_waves * 64, (hipStream_t)stream); });
    } else if (cfg->mlp_dtype != PSP_MLP_FP32) {
        return fail(-1, "mlp_dtype out of range for the HJB rollout (fp32, bf16_fwd or f16x3)");
    } else {
        e = p.fwd_quad ? p.inst.launch_fwd_quad(a, p.fwd_grid, (hipStream_t)stream)
            : p.fwd_split ? p.inst.launch_fwd_split(a, p.fwd_grid, (hipStream_t)stream)
                          : p.inst.launch_fwd(a, p.fwd_grid, p.fwd_waves * 64, (hipStream_t)stream);
    }
    return hip_rc(e, "hjb_fwd_kernel launch");
}

int psp_hjb_rollout_eval(const psp_hjb_config* cfg, const float* params, const float* x0, int32_t x0_stride,
                         const float* xi, uint64_t seed, uint32_t iter, const float* tfeat, float* D_out,
                         float* Fint_out, float* XN_out, double* fwd_partial, void* stream) {
    Plan p;
    int rc = make_plan(cfg, &p);
    if (rc) return rc;
    if ((rc = check_ptrs(cfg))) return rc;
    if (!params || !x0 || !D_out || !fwd_partial) return fail(-1, "null buffer passed to psp_hjb_rollout_eval");
    if (x0_stride != 0 && x0_stride != cfg->d) return fail(-1, "x0_stride must be 0 or d");
    if (cfg->noise_mode == PSP_NOISE_SUPPLIED && !xi) return fail(-1, "supplied-noise mode needs xi");
    psp::HjbArgs a;
    fill_args(cfg, p, &a);
    a.store_path = 0;
    a.uref = nullptr; a.ul2 = nullptr;      // the evaluation grid is not the training grid (utilities.py:296-299)
    a.params = params; a.x0 = x0; a.x0_stride = x0_stride; a.xi = xi; a.tfeat = tfeat;
    a.D = D_out; a.Fint = Fint_out; a.XN = XN_out; a.fwd_partial = fwd_partial;
    a.tables = reinterpret_cast<float*>(fwd_partial + 2 * (size_t)p.fwd_grid);
    a.seed_lo = (uint32_t)seed; a.seed_hi = (uint32_t)(seed >> 32); a.iter = iter;
    hipError_t e = p.fwd_quad ? p.inst.launch_fwd_quad(a, p.fwd_grid, (hipStream_t)stream)
                   : p.fwd_split ? p.inst.launch_fwd_split(a, p.fwd_grid, (hipStream_t)stream)
                                 : p.inst.launch_fwd(a, p.fwd_grid, p.fwd_waves * 64, (hipStream_t)stream);
    return hip_rc(e, "hjb_fwd_kernel (eval) launch");
}

int psp_hjb_terminal_reduce(const psp_hjb_config* cfg, const double* fwd_partial, double* sums_out, void* stream) {
    Plan p;
    int rc = make_plan(cfg, &p);
    if (rc) return rc;
    if (!fwd_partial || !sums_out) return fail(-1, "null buffer passed to psp_hjb_terminal_reduce");
    return PSP_LAUNCH(reduce_partials_kernel, dim3(1), dim3(256), 0, stream, fwd_partial, p.fwd_grid, sums_out);
}

int psp_hjb_terminal_reduce_loss(const psp_hjb_config* cfg, const double* fwd_partial, double* sums_out, float* loss_log,
                                 const uint32_t* index_dev, void* stream) {
    Plan p;
    int rc = make_plan(cfg, &p);
    if (rc) return rc;
    if (!fwd_partial || !sums_out) return fail(-1, "null buffer passed to psp_hjb_terminal_reduce_loss");
    if (loss_log && cfg->loss_kind == PSP_LOSS_WEIGHTS)
        return fail(-1, "psp_hjb_terminal_reduce_loss: the caller forms the loss of a PSP_LOSS_WEIGHTS run");
    if (cfg->K_global <= 0) return fail(-1, "K_global must be positive");
    return PSP_LAUNCH(reduce_partials_loss_kernel, dim3(1), dim3(256), 0, stream, fwd_partial, p.fwd_grid, sums_out, cfg->loss_kind,
                      1.0 / (double)cfg->K_global, loss_log, index_dev);
}

int psp_iter_state_init(psp_iter_state* host_out, uint32_t iter, int32_t step, float beta1, float beta2) {
    if (!host_out || step <= 0) return fail(-1, "psp_iter_state_init needs an output struct and a 1-based step");
    host_out->iter = iter; host_out->step = (uint32_t)step;
    host_out->beta1_pow = pow((double)beta1, (double)step);
    host_out->beta2_pow = pow((double)beta2, (double)step);
    return 0;
}

int psp_iter_state_advance(psp_iter_state* dev_state, float beta1, float beta2, void* stream) {
    if (!dev_state) return fail(-1, "null state passed to psp_iter_state_advance");
    return PSP_LAUNCH(iter_advance_kernel, dim3(1), dim3(1), 0, stream, dev_state, (double)beta1, (double)beta2);
}

int psp_adam_step_dev(float* params, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                      const psp_iter_state* dev_state, float lr, float beta1, float beta2, float eps, void* stream) {
    if (!params || !grad || !exp_avg || !exp_avg_sq || !dev_state) return fail(-1, "null buffer passed to psp_adam_step_dev");
    if (n <= 0) return fail(-1, "psp_adam_step_dev needs n > 0");
    return PSP_LAUNCH(adam_dev_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, params, grad, exp_avg, exp_avg_sq,
                      (long long)n, dev_state, lr, beta1, beta2, eps);
}

namespace {
// the backward kernel(s) of a config: the split-product kernel where it exists, guarded by its fp32-MFMA twin when
// cfg->range_flag is set (both enqueued, predicated on range_flag[0] == 0 / == 1; same grid and partial-gradient layout)
hipError_t launch_hjb_bwd(const psp_hjb_config* cfg, const Plan& p, psp::HjbArgs& a, hipStream_t st) {
    const bool bwd_x3 = cfg->mlp_dtype == PSP_MLP_F16X3 && p.inst.launch_bwd2_x3 &&
                        (p.inst.wide || p.inst.bwd2_x3_lds_bytes() <= kMaxLds);   // (else the fp32 backward: same results, same store)
    auto fp32 = [&]() { return p.inst.launch_bwd2(a, p.bwd_grid, st); };
    if (!bwd_x3) return fp32();
    return launch_either(cfg->range_flag, a.cond, a.cond_want, [&]() { return p.inst.launch_bwd2_x3(a, p.bwd_grid, st); }, fp32);
}
}  // namespace

int psp_hjb_rollout_bwd(const psp_hjb_config* cfg, const float* params, const float* xi, uint64_t seed,
                        uint32_t iter, const float* path, const float* D, const double* sums,
                        float* grad_partial, float* grad_out, void* stream) {
    Plan p;
    int rc = make_plan(cfg, &p);
    if (rc) return rc;
    if (!params || !path || !D || !sums || !grad_partial || !grad_out)
        return fail(-1, "null buffer passed to psp_hjb_rollout_bwd");
    if (cfg->noise_mode == PSP_NOISE_SUPPLIED && !xi) return fail(-1, "supplied-noise mode needs xi");
    psp::HjbArgs a;
    fill_args(cfg, p, &a);
    a.params = params; a.xi = xi; a.path = const_cast<float*>(path); a.D = const_cast<float*>(D);
    a.sums = sums; a.grad_partial = grad_partial;
    a.tables = reinterpret_cast<float*>(reinterpret_cast<char*>(grad_partial) + grad_rows_bytes(p));
    if (a.dbg) a.dbg += (size_t)p.fwd_grid * 8 * 8;
    a.seed_lo = (uint32_t)seed; a.seed_hi = (uint32_t)(seed >> 32); a.iter = iter;
    hipError_t e = launch_hjb_bwd(cfg, p, a, (hipStream_t)stream);
    if (e != hipSuccess) return fail_hip(e, "backward kernel launch");
    const int P = p.inst.n_params;
    return PSP_LAUNCH(reduce_grad_kernel, dim3((P + 31) / 32), dim3(256), 0, stream, grad_partial, p.bwd_grid, P, grad_out);
}

int psp_hjb_rollout_bwd_step(const psp_hjb_config* cfg, float* params, const float* path, const float* D, const double* sums,
                             float* grad_partial, float* grad_out, float* exp_avg, float* exp_avg_sq, psp_iter_state* dev_state,
                             uint32_t* ticket, float lr, float beta1, float beta2, float eps, void* stream) {
    Plan p;
    int rc = make_plan(cfg, &p);
    if (rc) return rc;
    if (!params || !path || !D || !sums || !grad_partial || !grad_out || !exp_avg || !exp_avg_sq || !dev_state || !ticket)
        return fail(-1, "null buffer passed to psp_hjb_rollout_bwd_step");
    if (cfg->store_path == 4) return fail(-1, "psp_hjb_rollout_bwd_step takes no Philox seed: store_path 4 goes through psp_hjb_rollout_bwd");
    psp::HjbArgs a;
    fill_args(cfg, p, &a);
    a.params = params; a.path = const_cast<float*>(path); a.D = const_cast<float*>(D);
    a.sums = sums; a.grad_partial = grad_partial;
    a.tables = reinterpret_cast<float*>(reinterpret_cast<char*>(grad_partial) + grad_rows_bytes(p));
    if (a.dbg) a.dbg += (size_t)p.fwd_grid * 8 * 8;
    hipError_t e = launch_hjb_bwd(cfg, p, a, (hipStream_t)stream);
    if (e != hipSuccess) return fail_hip(e, "backward kernel launch");
    const int P = p.inst.n_params;
    return PSP_LAUNCH(reduce_grad_adam_advance_kernel, dim3((P + 31) / 32), dim3(256), 0, stream, grad_partial, p.bwd_grid, P, grad_out,
                      params, exp_avg, exp_avg_sq, dev_state, ticket, lr, beta1, beta2, eps);
}

int psp_hjb_adjoint_sweep(const psp_hjb_config* cfg, const float* params, float* path, const float* XN,
                          const float* mu, const float* nu, const float* wT, double* fwd_partial, void* stream) {
    Plan p;
    int rc = make_plan(cfg, &p);
    if (rc) return rc;
    if ((rc = check_ptrs(cfg))) return rc;
    if (!p.inst.launch_adj) return fail(-2, "the adjoint sweep is not built for this kernel instance");
    if (!params || !path || !XN || !mu || !fwd_partial) return fail(-1, "null buffer passed to psp_hjb_adjoint_sweep");
    if (cfg->store_path != 2 && cfg->store_path != 3)
        return fail(-1, "psp_hjb_adjoint_sweep needs the path written with store_path = 2 or 3");
    if (!cfg->adaptive) return fail(-1, "without the adaptive forward process the state path carries no gradient");
    psp::HjbArgs a;
    fill_args(cfg, p, &a);
    a.params = params; a.path = path; a.XN = const_cast<float*>(XN); a.adj_mu = mu; a.adj_nu = nu; a.adj_wT = wT;
    // the wide family keeps its (transposed) operand tables where the forward kernel kept its own: behind the partial
    // sums of the forward scratch, whatever forward variant wrote them
    a.tables = reinterpret_cast<float*>(fwd_partial + 2 * (size_t)p.fwd_grid);
    if (p.fwd_quad && p.inst.launch_adj_quad) {           // smallest K: four trajectories per workgroup (hjbq_adj_kernel)
        hipError_t eq = p.inst.launch_adj_quad(a, 4 * p.ntile16, (hipStream_t)stream);
        return hip_rc(eq, "hjbq_adj_kernel launch");
    }
    // one wave per 16-trajectory tile, like the forward kernels (the recursion is sequential in time)
    const int fw = tile_waves(p.ntile16, p.inst.wide);
    const int grid = (p.ntile16 + fw - 1) / fw;
    const bool adj_x3 = cfg->mlp_dtype == PSP_MLP_F16X3 && p.inst.launch_adj_x3;    // (make_plan checked the LDS fit of the forward carve)
    auto fp32 = [&]() { return p.inst.launch_adj(a, grid, fw * 64, (hipStream_t)stream); };
    const hipError_t e = !adj_x3 ? fp32() : launch_either(cfg->range_flag, a.cond, a.cond_want,    // range guard: both sweeps, predicated
                                                          [&]() { return p.inst.launch_adj_x3(a, grid, fw * 64, (hipStream_t)stream); }, fp32);
    return hip_rc(e, "hjb_adj_kernel launch");
}

int psp_gen_supported(int32_t d, int32_t H) {
    psp::GenInstance inst;
    return find_in(kGenTable, d, H, &inst) ? 1 : 0;
}

int psp_gen_instance_count(void) { return table_count(kGenTable); }

int psp_gen_instance_get(int32_t i, int32_t* d, int32_t* H) { return table_get(kGenTable, i, d, H); }

int psp_gen_query(const psp_gen_config* cfg, psp_gen_sizes* out) {
    GenPlan p;
    int rc = make_gen_plan(cfg, &p);
    if (rc) return rc;
    if (!out) return fail(-1, "null output");
    memset(out, 0, sizeof(*out));
    out->n_params = p.inst.n_params;
    out->fwd_workgroups = p.fwd_grid;
    out->bwd_workgroups = p.bwd_grid;
    const int64_t blk = cfg->mlp_dtype == PSP_MLP_BF16 ? p.inst.path_dwords_per_block16 : p.inst.path_floats_per_block;
    out->path_bytes = cfg->store_path ? (int64_t)(cfg->N + 1) * p.ntile16 * blk * 4 : 0;
    out->ahat_bytes = (int64_t)(cfg->N + 1) * p.ntile16 * 16 * 4;
    out->grad_partial_bytes = (int64_t)p.bwd_grid * p.inst.n_params * 4;
    return 0;
}

int psp_gen_rollout_fwd(const psp_gen_config* cfg, const float* params, const float* x0, const float* t0,
                        const float* xi, uint64_t seed, uint32_t iter, float* path, float* ahat, float* VN,
                        float* YN, float* XN, float* tN, unsigned long long* kcount, void* stream) {
    GenPlan p;
    int rc = make_gen_plan(cfg, &p);
    if (rc) return rc;
    if (!params || !x0 || !t0 || !VN || !YN || !XN || !tN || !kcount)
        return fail(-1, "null buffer passed to psp_gen_rollout_fwd");
    if (cfg->noise_mode == PSP_NOISE_SUPPLIED && !xi) return fail(-1, "supplied-noise mode needs xi");
    if (cfg->store_path && (!path || !ahat)) return fail(-1, "store_path set but path / ahat buffer is null");
    psp::GenArgs a;
    fill_gen_args(cfg, p, &a);
    a.params = params; a.x0 = x0; a.t0 = t0; a.xi = xi; a.path = path; a.ahat = ahat;
    a.VN = VN; a.YN = YN; a.XN = XN; a.tN = tN; a.kcount = kcount;
    a.seed_lo = (uint32_t)seed; a.seed_hi = (uint32_t)(seed >> 32); a.iter = iter;
    if (cfg->mlp_dtype < PSP_MLP_FP32 || cfg->mlp_dtype > PSP_MLP_F16X3) return fail(-1, "mlp_dtype out of range");
    if (cfg->mlp_dtype == PSP_MLP_F16X3 && (!p.inst.launch_fwd_x3 || p.inst.fwd_x3_lds_bytes() > kMaxLds))
        return fail(-3, "split-product forward tables do not fit the 160 KiB LDS for this (d,H)");
    auto fp32 = [&]() { return p.inst.launch_fwd(a, p.fwd_grid, p.fwd_waves * 64, (hipStream_t)stream); };
    if (cfg->mlp_dtype == PSP_MLP_F16X3) {
        // range guard (psp_gen_config.range_flag): a non-finite V(X_N) / Y_N -> flag -> the fp32-MFMA forward, predicated.
        // kcount accumulates (atomicAdd): the flag kernel takes back what the split kernel added when it raises the flag
        unsigned long long* const kcount_before = cfg->range_flag ? reinterpret_cast<unsigned long long*>(cfg->range_flag + 2) : nullptr;
        if (cfg->range_flag && (rc = PSP_LAUNCH(snapshot_u64_kernel, dim3(1), dim3(1), 0, stream, kcount, kcount_before))) return rc;
        return launch_redo(cfg->range_flag, a.cond, a.cond_want, "gen_fwd_kernel launch",
                           [&]() { return p.inst.launch_fwd_x3(a, p.fwd_grid, p.fwd_waves * 64, (hipStream_t)stream); },
                           [&]() { return PSP_LAUNCH(range_flag_arrays_kernel, dim3(1), dim3(1024), 0, stream, VN, YN, cfg->K_local, cfg->range_flag, kcount, kcount_before); },
                           fp32);
    }
    const hipError_t e = cfg->mlp_dtype != PSP_MLP_FP32 ? p.inst.launch_fwd_bf16(a, p.fwd_grid, p.fwd_waves * 64, (hipStream_t)stream) : fp32();
    return hip_rc(e, "gen_fwd_kernel launch");
}

int psp_gen_rollout_bwd(const psp_gen_config* cfg, const float* params, const float* path, const float* ahat,
                        const float* wY, const float* wV, float* grad_partial, float* grad_out, void* stream) {
    GenPlan p;
    int rc = make_gen_plan(cfg, &p);
    if (rc) return rc;
    if (!params || !path || !ahat || !wY || (!wV && !cfg->per_sample_weights) || !grad_partial || !grad_out)
        return fail(-1, "null buffer passed to psp_gen_rollout_bwd");
    psp::GenArgs a;
    fill_gen_args(cfg, p, &a);
    a.params = params; a.path = const_cast<float*>(path); a.ahat = const_cast<float*>(ahat);
    a.wY = wY; a.wV = wV; a.grad_partial = grad_partial;
    a.dbg = (g_dbg && g_dbg_n >= (long long)p.bwd_grid * 8 * 8) ? g_dbg : nullptr;      // (-DPSP_STAMPS builds; the kernels ignore it otherwise)
    if (cfg->mlp_dtype < PSP_MLP_FP32 || cfg->mlp_dtype > PSP_MLP_F16X3) return fail(-1, "mlp_dtype out of range");
    // (PSP_MLP_F16X3 with shared trajectory weights: the split-product consumers; per-sample weights keep the fp32 kernel)
    const bool bwd_x3 = cfg->mlp_dtype == PSP_MLP_F16X3 && !cfg->per_sample_weights && p.inst.launch_bwd2_x3;
    auto fp32 = [&]() { return p.inst.launch_bwd2(a, p.bwd_grid, (hipStream_t)stream); };
    const hipError_t e = cfg->mlp_dtype == PSP_MLP_BF16 ? p.inst.launch_bwd2_bf16(a, p.bwd_grid, (hipStream_t)stream)
                         : !bwd_x3 ? fp32()
                                   : launch_either(cfg->range_flag, a.cond, a.cond_want,       // range guard: split and fp32-MFMA backward, predicated
                                                   [&]() { return p.inst.launch_bwd2_x3(a, p.bwd_grid, (hipStream_t)stream); }, fp32);
    if (e != hipSuccess) return fail_hip(e, "gen_bwd2_kernel launch");
    const int P = p.inst.n_params;
    return PSP_LAUNCH(reduce_grad_kernel, dim3((P + 31) / 32), dim3(256), 0, stream, grad_partial, p.bwd_grid, P, grad_out);
}


// ---- value nets of any depth (genl_kernels.h) ----------------------------------------------------------------------------
namespace {
struct GenlPlan { psp::GenlArgs a; psp::GenlUl2Args u; int ul2_on; int ntile16; long long table_floats; long long n_params; int fwd_lds, bwd_lds, nw_fwd, nw_bwd,
                  bwd_grid, bwd_groups; };
// q: the linear-quadratic coefficients of psp_genl_query_lq / psp_genl_rollout_fwd_lq (NULL or all zero: none -- the plan, the
// table layout and the kernel instance of psp_genl_rollout_fwd)
// u: the u_L2 log of psp_genl_query_ul2 / psp_genl_ul2_stage / psp_genl_rollout_fwd_ul2 (NULL: none -- nothing changes)
// e: the eigenvalue problems of psp_genl_query_eig / psp_genl_rollout_fwd_eig (NULL: none -- nothing changes; with it the kinds
// PSP_GH_EIG_* / PSP_DRIFT_EIG_FP are accepted and the forward runs the instances of genl_eig_instance.hip)
int make_genl_plan(const psp_genl_config* c, GenlPlan* p, const psp_genl_coeffs* q = nullptr, const psp_genl_ul2* u = nullptr,
                   const psp_genl_eig* e = nullptr) {
    if (!c) return fail(-1, "null config");
    if (e) {
        if (e->struct_bytes != (int32_t)sizeof(psp_genl_eig)) return fail(-1, "psp_genl_eig.struct_bytes is not sizeof(psp_genl_eig)");
        if (e->output_relu != 0 && e->output_relu != 1) return fail(-1, "psp_genl_eig.output_relu is 0 or 1");
        if (q || u) return fail(-1, "psp_genl_eig excludes psp_genl_coeffs and psp_genl_ul2");
        if (c->sigma_kind != PSP_GENL_SIGMA_SCALED || c->base.h_kind == PSP_GH_EXPBALL_SIN_FULL || c->base.h_kind == PSP_GH_SINNORM2)
            return fail(-1, "psp_genl_eig is built for sigma = s I (no dense sigma, no h kind that runs on the dense path)");
        if (c->base.adaptive) return fail(-1, "psp_genl_eig is built for base.adaptive = 0 (the detached, uncontrolled state path)");
    }
    const bool eig_h = c->base.h_kind == PSP_GH_EIG_FP || c->base.h_kind == PSP_GH_EIG_NLS;
    const bool eig_b = c->base.drift_kind == PSP_DRIFT_EIG_FP;
    if ((eig_h || eig_b) && !e) return fail(-1, "PSP_GH_EIG_FP / PSP_GH_EIG_NLS / PSP_DRIFT_EIG_FP need a psp_genl_eig (psp_genl_rollout_fwd_eig)");
    if (c->base.h_kind == PSP_GH_EIG_FP && !eig_b) return fail(-1, "PSP_GH_EIG_FP reads the vector c of PSP_DRIFT_EIG_FP (set both)");
    if (c->base.h_kind == PSP_GH_EIG_NLS && !(c->base.h_par[1] > 0.f)) return fail(-1, "PSP_GH_EIG_NLS: h_par = (1 / c^2, d, -, -) with d > 0");
    if (u) {
        if (u->struct_bytes != (int32_t)sizeof(psp_genl_ul2)) return fail(-1, "psp_genl_ul2.struct_bytes is not sizeof(psp_genl_ul2)");
        if (u->kind < PSP_UL2_TABLE || u->kind > PSP_UL2_GRID) return fail(-1, "psp_genl_ul2.kind out of range");
        if (!u->u_l2_out) return fail(-1, "the u_L2 log needs psp_genl_ul2.u_l2_out");
        if (u->kind == PSP_UL2_TABLE && !u->u_ref) return fail(-1, "PSP_UL2_TABLE needs psp_genl_ul2.u_ref");
        if (u->kind != PSP_UL2_TABLE && !u->tables) return fail(-1, "PSP_UL2_LINEAR / PSP_UL2_GRID need psp_genl_ul2.tables");
        if (u->kind == PSP_UL2_GRID) {
            if (!u->group) return fail(-1, "PSP_UL2_GRID needs psp_genl_ul2.group");
            if (!u->row) return fail(-1, "PSP_UL2_GRID needs psp_genl_ul2.row");
            if (u->ntables <= 0 || u->nrows <= 0 || u->ncols <= 0) return fail(-1, "PSP_UL2_GRID: ntables / nrows / ncols must be positive");
            if (!(u->xb > 0.f) || !(u->dx > 0.f)) return fail(-1, "PSP_UL2_GRID: xb / dx must be positive");
            if (u->K_global <= 0) return fail(-1, "PSP_UL2_GRID: K_global must be positive");
        }
        if (c->base.domain_kind != PSP_DOM_NONE || !(c->base.T > 3.0e38f))
            return fail(-1, "the u_L2 log is defined for runs that never stop (domain_kind = PSP_DOM_NONE, T = inf)");
    }
    if (q) {
        static const psp_genl_coeffs zero = {};
        if (memcmp(q, &zero, sizeof(zero)) == 0) q = nullptr;
    }
    if (q) {
        if (q->struct_bytes != (int32_t)sizeof(psp_genl_coeffs)) return fail(-1, "psp_genl_coeffs.struct_bytes is not sizeof(psp_genl_coeffs)");
        if (q->z_kind < PSP_GENL_Z_SIGMA_T || q->z_kind > PSP_GENL_Z_SIGMA || q->runcost_kind < PSP_RUNCOST_ZERO ||
            q->runcost_kind > PSP_RUNCOST_DIAG_QUAD)
            return fail(-1, "coefficient enum out of range");
        if (q->runcost_kind == PSP_RUNCOST_DIAG_QUAD && !q->runcost) return fail(-1, "running-cost vector missing");
        if (q->runcost_kind != PSP_RUNCOST_ZERO && c->base.h_kind != PSP_GH_QUAD)
            return fail(-1, "a running cost is defined for h = -|z|^2 / 2 - f(x) only (PSP_GH_QUAD)");
        if (q->drift_matrix && c->base.drift_kind != PSP_DRIFT_ZERO)
            return fail(-1, "a drift matrix excludes base.drift_kind (give A alone, or the diagonal kind alone)");
        if (q->z_kind == PSP_GENL_Z_SIGMA_T && q->runcost_kind == PSP_RUNCOST_ZERO && !q->drift_matrix) q = nullptr;   // nothing asked
    }
    const psp_gen_config& b = c->base;
    if (b.d <= 0 || b.K_local <= 0 || b.N <= 0) return fail(-1, "non-positive d/K/N");
    const int L = c->n_hidden;
    if (L < 1 || L > psp::GENL_MAXL) return fail(-2, "value net: 1 to 4 hidden layers");
    const int D0 = b.d + (c->has_time ? 1 : 0);
    if (D0 > 16 * psp::GENL_MAXDB) return fail(-2, "value net: input width above 112");
    if ((b.drift_kind != PSP_DRIFT_ZERO && b.drift_kind != PSP_DRIFT_DOUBLE_WELL && b.drift_kind != PSP_DRIFT_DIAG && !eig_b) || b.h_kind < 0 ||
        (b.h_kind > PSP_GH_SINNORM2 && !eig_h) || b.noise_mode < 0 || b.noise_mode > 1 || b.domain_kind < 0 || b.domain_kind > PSP_DOM_ANNULUS ||
        c->sigma_kind < PSP_GENL_SIGMA_SCALED || c->sigma_kind > PSP_GENL_SIGMA_DENSE)
        return fail(-1, "config enum out of range");
    if ((b.h_kind == PSP_GH_AFFINE_EXP || b.h_kind == PSP_GH_SINE_SOURCE) && (c->sigma_kind == PSP_GENL_SIGMA_DENSE || q))
        return fail(-1, "PSP_GH_AFFINE_EXP / PSP_GH_SINE_SOURCE are built for sigma = s I without psp_genl_coeffs");
    if (b.h_kind == PSP_GH_SINNORM2 && q) return fail(-1, "PSP_GH_SINNORM2 is not built for psp_genl_coeffs");
    if (int rc = check_gh_par(b.h_kind, b.h_par, b.d)) return rc;
    if (c->sigma_kind == PSP_GENL_SIGMA_DENSE && !c->sigma) return fail(-1, "sigma matrix missing");
    if (c->activation < 0 || c->activation > PSP_ACT_TANH) return fail(-1, "value net: unknown activation");
    if (int rc = check_gen_domain(b)) return rc;
    if (b.drift_kind != PSP_DRIFT_ZERO && !b.drift) return fail(-1, "drift vector missing (double-well kappa / diagonal of A)");
    psp::GenlArgs& a = p->a;
    memset(&a, 0, sizeof(a));
    memset(&p->u, 0, sizeof(p->u)); p->ul2_on = 0;
    a.d = b.d; a.D0 = D0; a.has_time = c->has_time ? 1 : 0; a.L = L;
    a.act = c->activation; a.linear_layout = c->linear_layout ? 1 : 0;
    a.time_first = (c->has_time && c->time_first) ? 1 : 0;
    a.time_scale = (c->has_time && c->time_scale != 0.f) ? c->time_scale : 1.0f;
    a.DB0 = (D0 + 15) / 16;
    a.off[0] = 0; a.roff[0] = 0;
    int blocks = a.DB0, real = D0, hbsum = 0, tiles = 0;
    long long pofs = 0, tofs = 0;
    for (int i = 0; i < L; ++i) {
        const int Hi = c->widths[i];
        if (Hi < 1 || Hi > 16 * psp::GENL_MAXHB) return fail(-2, "value net: hidden widths between 1 and 128");
        a.H[i] = Hi; a.HB[i] = (Hi + 15) / 16;
        a.off[i + 1] = blocks; a.roff[i + 1] = real; a.inw[i] = real;
        a.oW[i] = (int)pofs; pofs += (long long)real * Hi;
        a.ob[i] = (int)pofs; pofs += Hi;
        a.tF[i] = tofs; tofs += (long long)a.HB[i] * 4 * blocks * 64;           // [HB_i][4 * input blocks][64]
        a.tR[i] = tofs; tofs += (long long)blocks * 4 * a.HB[i] * 64;           // [input blocks][4 HB_i][64]
        a.vB[i] = tofs; tofs += (long long)a.HB[i] * 16;
        a.tcum[i] = tiles; tiles += blocks * a.HB[i];
        blocks += a.HB[i]; real += Hi; hbsum += a.HB[i];
    }
    a.tcum[L] = tiles;
    a.inw[L] = real;                                                            // (input width of the output layer)
    a.oW[L] = (int)pofs; pofs += real;
    a.ob[L] = (int)pofs; pofs += 1;
    a.TB = blocks; a.HBsum = hbsum; a.P = pofs;
    tiles += blocks;                                                            // the output layer as a layer of one unit
    a.n_tiles = tiles;
    a.vW = tofs; tofs += (long long)blocks * 16;
    // a dense sigma -- or the h of the full-Hessian problem, whose (sum x)^2 only the dense-sigma instances of the forward kernel
    // form (with a scaled identity the tables kernel writes s I) -- adds the tables of B and B^T
    a.dense = (c->sigma_kind == PSP_GENL_SIGMA_DENSE || b.h_kind == PSP_GH_EXPBALL_SIN_FULL || b.h_kind == PSP_GH_SINNORM2) ? 1 : 0;
    a.sigmaB = c->sigma_kind == PSP_GENL_SIGMA_DENSE ? c->sigma : nullptr;
    if (q) {                                                                     // (they run on the dense path: s I through the tables)
        a.dense = 1; a.lq = 1;
        a.z_sigma = q->z_kind == PSP_GENL_Z_SIGMA ? 1 : 0;
        a.runcost_kind = q->runcost_kind; a.runcost = q->runcost_kind ? q->runcost : nullptr;
        a.driftA = q->drift_matrix;
    }
    if (a.dense) {
        tofs = (tofs + 3) & ~3LL;                                                // (16-byte table loads)
        a.tSB = tofs; tofs += (long long)a.DB0 * 4 * a.DB0 * 64;
        a.tSBT = tofs; tofs += (long long)a.DB0 * 4 * a.DB0 * 64;
        if (a.driftA) { a.tA = tofs; tofs += (long long)a.DB0 * 4 * a.DB0 * 64; }   // dt A, behind the tables psp_genl_rollout_bwd reads
    }
    if (u) {
        // two instance shapes carry the log: sigma = s I with an element-wise drift, and the linear-quadratic one
        if (a.dense && !a.lq)
            return fail(-1, "the u_L2 log on the dense-sigma path runs on the linear-quadratic instances (give psp_genl_coeffs)");
        if (u->kind == PSP_UL2_LINEAR && !a.lq)
            return fail(-1, "PSP_UL2_LINEAR runs on the linear-quadratic instances (give psp_genl_coeffs)");
        psp::GenlUl2Args& ua = p->u;
        p->ul2_on = 1; ua.kind = u->kind; ua.out = u->u_l2_out;
        ua.ref = u->kind == PSP_UL2_TABLE ? u->u_ref : u->tables;
        ua.group = u->group; ua.row = u->row;
        ua.ntables = u->ntables; ua.nrows = u->nrows; ua.ncols = u->ncols;
        ua.xb = u->xb; ua.dx = u->dx; ua.xhi = u->xhi; ua.Kglobal = u->K_global;
        if (u->kind == PSP_UL2_LINEAR) {                                         // the gains of every step, staged once per plan:
            tofs = (tofs + 3) & ~3LL;                                            // behind everything genl_tables_kernel rewrites
            ua.tUL = tofs; tofs += (long long)b.N * a.DB0 * 4 * a.DB0 * 64;
        }
    }
    p->table_floats = tofs; p->n_params = pofs;
    p->ntile16 = (b.K_local + 15) / 16;
    // waves per tile: one (no barriers, many tiles per CU) for small nets -- always for the smallest, for the others once the
    // batch fills the chip several times over --, else eight waves cutting every product by output block
    const bool small = hbsum <= 8 && blocks <= 16;
    const int cus = n_cus();
    const char* force = getenv("PSP_GENL_NW");
    int nw = (small && (hbsum <= 5 || p->ntile16 >= 4 * cus)) ? 1 : 8;
    if (force && force[0] == '1' && small) nw = 1;
    if (force && force[0] == '8') nw = 8;
    p->nw_fwd = nw; p->nw_bwd = nw;
    if (nw == 8 && p->ntile16 >= 2 * cus) p->nw_fwd = 4;                        // two tiles per CU in flight (genl_kernels.h)
    if (force && force[0] == '4' && nw == 8) p->nw_fwd = 4;
    if (force && force[0] == '8') p->nw_fwd = 8;
    p->fwd_lds = a.dense ? psp::genl_fwd_lds_bytes_dense(a.TB, a.DB0) : psp::genl_fwd_lds_bytes(a.TB); p->bwd_lds = psp::genl_bwd_lds_bytes(a.TB, a.DB0, p->nw_bwd);
    if (p->ul2_on && a.dense && p->u.kind != PSP_UL2_TABLE) p->fwd_lds = psp::genl_fwd_lds_bytes_dense_log(a.TB, a.DB0);   // Z_n kept until X_{n+1} exists
    a.table_floats = tofs;
    if (p->fwd_lds > kMaxLds || p->bwd_lds > kMaxLds)
        return fail(-3, "value net: the activation images exceed the 160 KiB LDS (sum of the padded widths too large)");
    const long long nblk = (long long)(b.N + 1) * p->ntile16;
    if (nblk >= (1LL << 31)) return fail(-1, "(N + 1) * ceil(K/16) must stay below 2^31");
    const int per_group = p->nw_bwd * psp::GenlGeo<1>::MAXT;
    p->bwd_groups = (tiles + per_group - 1) / per_group;
    // workgroups of the backward kernel: what the CUs hold at once (LDS-limited), never more than there are sample blocks
    long long per_cu = nw == 1 ? 8 : (p->bwd_lds > kMaxLds / 2 ? 1 : 2);
    if (nw == 1 && (long long)p->bwd_lds * per_cu > kMaxLds) per_cu = kMaxLds / p->bwd_lds;
    long long grid = per_cu * cus;
    if (grid > nblk) grid = nblk;
    p->bwd_grid = (int)grid;
    fill_gen_problem(b, p->ntile16, &a.g);
    a.g.d_real = b.d;                                      // (every coordinate is real here)
    return 0;
}
// the step counts of the tiles live behind the (N + 1) x 16 ceil(K/16) coefficients of `ahat`
int* genl_nexec(const psp_genl_config* cfg, const GenlPlan& p, const float* ahat) {
    return reinterpret_cast<int*>(const_cast<float*>(ahat)) + (size_t)(cfg->base.N + 1) * p.ntile16 * 16;
}
int genl_sizes_of(const psp_genl_config* cfg, const GenlPlan& p, psp_genl_sizes* out) {
    if (!out) return fail(-1, "null output");
    memset(out, 0, sizeof(*out));
    const int64_t nblk = (int64_t)(cfg->base.N + 1) * p.ntile16;
    out->table_bytes = p.table_floats * 4;
    out->path_bytes = cfg->base.store_path ? nblk * 2 * p.a.DB0 * 256 * 4 : 0;
    out->ahat_bytes = nblk * 16 * 4 + (int64_t)p.ntile16 * 4;
    out->n_params = p.n_params;
    out->grad_partial_bytes = (int64_t)p.bwd_grid * p.n_params * 4;
    out->n_blocks = (int32_t)nblk;
    out->fwd_workgroups = p.ntile16;
    out->bwd_workgroups = p.bwd_grid * p.bwd_groups;
    out->waves_per_tile = p.nw_fwd;
    for (int i = 0; i <= p.a.L; ++i) out->seg_block_offset[i] = p.a.off[i];
    return 0;
}
}  // namespace

int psp_genl_query(const psp_genl_config* cfg, psp_genl_sizes* out) { return psp_genl_query_lq(cfg, nullptr, out); }

int psp_genl_query_lq(const psp_genl_config* cfg, const psp_genl_coeffs* coeffs, psp_genl_sizes* out) {
    return psp_genl_query_ul2(cfg, coeffs, nullptr, out);
}

int psp_genl_query_ul2(const psp_genl_config* cfg, const psp_genl_coeffs* coeffs, const psp_genl_ul2* ul2, psp_genl_sizes* out) {
    GenlPlan p;
    int rc = make_genl_plan(cfg, &p, coeffs, ul2);
    if (rc) return rc;
    return genl_sizes_of(cfg, p, out);
}

int psp_genl_query_eig(const psp_genl_config* cfg, const psp_genl_eig* eig, psp_genl_sizes* out) {
    GenlPlan p;
    int rc = make_genl_plan(cfg, &p, nullptr, nullptr, eig);
    if (rc) return rc;
    return genl_sizes_of(cfg, p, out);
}

int psp_genl_rollout_fwd(const psp_genl_config* cfg, const float* params, const float* x0, const float* t0,
                                    const float* xi, uint64_t seed, uint32_t iter, float* tables, float* path, float* ahat,
                                    float* VN, float* YN, float* XN, float* tN, unsigned long long* kcount, void* stream) {
    return psp_genl_rollout_fwd_lq(cfg, nullptr, params, x0, t0, xi, seed, iter, tables, path, ahat, VN, YN, XN, tN, kcount, stream);
}

int psp_genl_rollout_fwd_lq(const psp_genl_config* cfg, const psp_genl_coeffs* coeffs, const float* params, const float* x0,
                            const float* t0, const float* xi, uint64_t seed, uint32_t iter, float* tables, float* path, float* ahat,
                            float* VN, float* YN, float* XN, float* tN, unsigned long long* kcount, void* stream) {
    return psp_genl_rollout_fwd_ul2(cfg, coeffs, nullptr, params, x0, t0, xi, seed, iter, tables, path, ahat, VN, YN, XN, tN, kcount, stream);
}

int psp_genl_ul2_stage(const psp_genl_config* cfg, const psp_genl_coeffs* coeffs, const psp_genl_ul2* ul2, float* tables, void* stream) {
    if (!ul2) return fail(-1, "psp_genl_ul2_stage: null psp_genl_ul2");
    GenlPlan p;
    int rc = make_genl_plan(cfg, &p, coeffs, ul2);
    if (rc) return rc;
    if (!tables) return fail(-1, "null buffer passed to psp_genl_ul2_stage");
    if (p.u.kind != PSP_UL2_LINEAR) return 0;                                    // nothing to stage
    p.a.tables = tables; p.a.tables_w = tables;
    const psp::GenlLogArgs la = {p.a, p.u};
    hipError_t e = psp::genl_ul2_launch_stage(la, (hipStream_t)stream);          // (genl_ul2_instance.hip)
    return hip_rc(e, "genl_ul2_stage_kernel launch");
}

namespace {
int genl_rollout_fwd_any(const psp_genl_config* cfg, const psp_genl_coeffs* coeffs, const psp_genl_ul2* ul2, const psp_genl_eig* eig,
                         const float* params, const float* x0, const float* t0, const float* xi, uint64_t seed, uint32_t iter,
                         float* tables, float* path, float* ahat, float* VN, float* YN, float* XN, float* tN,
                         unsigned long long* kcount, void* stream) {
    GenlPlan p;
    int rc = make_genl_plan(cfg, &p, coeffs, ul2, eig);
    if (rc) return rc;
    if (!params || !x0 || !tables || !VN || !YN || !XN || !tN || !kcount || !ahat) return fail(-1, "null buffer passed to psp_genl_rollout_fwd");
    if (cfg->has_time && !t0) return fail(-1, "t0 missing");
    if (cfg->base.noise_mode == PSP_NOISE_SUPPLIED && !xi) return fail(-1, "supplied-noise mode needs xi");
    if (cfg->base.store_path && !path) return fail(-1, "store_path set but the path buffer is null");
    psp::GenlArgs& a = p.a;
    a.tables = tables; a.tables_w = tables;
    a.nexec = genl_nexec(cfg, p, ahat);
    psp::GenArgs& g = a.g;
    g.params = params; g.x0 = x0; g.t0 = t0; g.xi = xi; g.path = path; g.ahat = ahat;
    g.VN = VN; g.YN = YN; g.XN = XN; g.tN = tN; g.kcount = kcount;
    g.Vsteps = cfg->base.v_steps_out; g.Ysteps = cfg->base.y_steps_out;
    g.seed_lo = (uint32_t)seed; g.seed_hi = (uint32_t)(seed >> 32); g.iter = iter;
    hipStream_t st = (hipStream_t)stream;
    if ((rc = PSP_LAUNCH(genl_tables_kernel, dim3(128), dim3(256), 0, st, a))) return rc;
    hipError_t e;
    if (eig) {
        psp::GenlEigFwdArgs ea;
        ea.a = p.a;
        ea.e.lam = eig->lambda; ea.e.S_out = eig->s_out; ea.e.out_relu = eig->output_relu; ea.e.reserved = 0;
        e = psp::genl_eig_launch_fwd(ea, p.nw_fwd, p.ntile16, p.fwd_lds, st);        // (genl_eig_instance.hip)
    } else if (p.ul2_on) {
        const psp::GenlLogArgs la = {p.a, p.u};
        e = psp::genl_ul2_launch_fwd(la, p.nw_fwd, p.ntile16, p.fwd_lds, st);        // (genl_ul2_instance.hip)
    } else if (p.a.lq)
        e = psp::genl_lq_launch_fwd(p.a, p.nw_fwd, p.ntile16, p.fwd_lds, st);        // (genl_lq_instance.hip)
    else if (p.a.dense)
        e = p.nw_fwd == 1 ? psp::genl_launch_fwd<1, true>(p.a, p.ntile16, p.fwd_lds, st)
            : p.nw_fwd == 4 ? psp::genl_launch_fwd<4, true>(p.a, p.ntile16, p.fwd_lds, st) : psp::genl_launch_fwd<8, true>(p.a, p.ntile16, p.fwd_lds, st);
    else
    e = p.nw_fwd == 1 ? psp::genl_launch_fwd<1>(p.a, p.ntile16, p.fwd_lds, st)
        : p.nw_fwd == 4 ? psp::genl_launch_fwd<4>(p.a, p.ntile16, p.fwd_lds, st) : psp::genl_launch_fwd<8>(p.a, p.ntile16, p.fwd_lds, st);
    return hip_rc(e, "genl_fwd_kernel launch");
}
}  // namespace

int psp_genl_rollout_fwd_ul2(const psp_genl_config* cfg, const psp_genl_coeffs* coeffs, const psp_genl_ul2* ul2, const float* params,
                             const float* x0, const float* t0, const float* xi, uint64_t seed, uint32_t iter, float* tables,
                             float* path, float* ahat, float* VN, float* YN, float* XN, float* tN, unsigned long long* kcount,
                             void* stream) {
    return genl_rollout_fwd_any(cfg, coeffs, ul2, nullptr, params, x0, t0, xi, seed, iter, tables, path, ahat, VN, YN, XN, tN, kcount, stream);
}

int psp_genl_rollout_fwd_eig(const psp_genl_config* cfg, const psp_genl_eig* eig, const float* params, const float* x0, const float* t0,
                             const float* xi, uint64_t seed, uint32_t iter, float* tables, float* path, float* ahat, float* VN,
                             float* YN, float* XN, float* tN, unsigned long long* kcount, void* stream) {
    return genl_rollout_fwd_any(cfg, nullptr, nullptr, eig, params, x0, t0, xi, seed, iter, tables, path, ahat, VN, YN, XN, tN, kcount, stream);
}

int psp_genl_rollout_bwd(const psp_genl_config* cfg_in, const float* params, const float* tables, const float* path,
                         const float* ahat, const float* wY, const float* wV, float* grad_partial, float* grad_out, void* stream) {
    if (!cfg_in) return fail(-1, "null config");
    // the backward reads (x, t), U and a^ and no coefficient: a config of psp_genl_rollout_fwd_eig is planned as what it is
    // without the kinds only that entry point accepts
    psp_genl_config cfg_v = *cfg_in;
    if (cfg_v.base.h_kind == PSP_GH_EIG_FP || cfg_v.base.h_kind == PSP_GH_EIG_NLS) cfg_v.base.h_kind = PSP_GH_ZERO;
    if (cfg_v.base.drift_kind == PSP_DRIFT_EIG_FP) cfg_v.base.drift_kind = PSP_DRIFT_ZERO;
    const psp_genl_config* cfg = &cfg_v;
    GenlPlan p;
    int rc = make_genl_plan(cfg, &p);
    if (rc) return rc;
    if (!params || !tables || !path || !ahat || !wY || (!wV && !cfg->base.per_sample_weights) || !grad_partial || !grad_out)
        return fail(-1, "null buffer passed to psp_genl_rollout_bwd");
    psp::GenlArgs& a = p.a;
    a.tables = tables;
    a.nexec = genl_nexec(cfg, p, ahat);
    a.gpart = grad_partial;
    psp::GenArgs& g = a.g;
    g.params = params; g.path = const_cast<float*>(path); g.ahat = const_cast<float*>(ahat); g.wY = wY; g.wV = wV;
    g.per_sample = cfg->base.per_sample_weights ? 1 : 0;
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = p.nw_bwd == 1 ? psp::genl_launch_bwd<1>(p.a, p.bwd_grid, p.bwd_groups, p.bwd_lds, st)
                   : p.a.HBsum <= 24 ? psp::genl_launch_bwd<8, 3>(p.a, p.bwd_grid, p.bwd_groups, p.bwd_lds, st)   // (three slots per wave suffice: genl_kernels.h)
                                     : psp::genl_launch_bwd<8>(p.a, p.bwd_grid, p.bwd_groups, p.bwd_lds, st);
    if (e != hipSuccess) return fail_hip(e, "genl_bwd_kernel launch");
    const int P = (int)p.n_params;
    return PSP_LAUNCH(reduce_grad_kernel, dim3((P + 31) / 32), dim3(256), 0, st, grad_partial, p.bwd_grid, P, grad_out);
}

// ---- adjoint sweep of the state path, value-function ansatz (genl_adj_kernels.h) ------------------------------------------------
namespace {
// every check psp_genl_query_adj and psp_genl_adjoint_sweep share; *tAT: where the table of (dt A)^T goes when nothing else follows
// the tables of `u` (behind everything genl_tables_kernel and psp_genl_ul2_stage write), *table_floats: the scratch with it
int make_genl_adj_plan(const psp_genl_config* c, const psp_genl_coeffs* q, const psp_genl_ul2* u, const psp_genl_adj* adj, GenlPlan* p,
                       long long* tAT, long long* table_floats, int* lds) {
    if (!adj) return fail(-1, "null psp_genl_adj");
    if (adj->struct_bytes != (int32_t)sizeof(psp_genl_adj)) return fail(-1, "psp_genl_adj.struct_bytes is not sizeof(psp_genl_adj)");
    int rc = make_genl_plan(c, p, q, u);
    if (rc) return rc;
    const psp_gen_config& b = c->base;
    if (b.domain_kind != PSP_DOM_NONE || !(b.T > 3.0e38f))
        return fail(-1, "the adjoint sweep is defined for runs that never stop (domain_kind = PSP_DOM_NONE, T = inf)");
    if (!b.adaptive) return fail(-1, "the adjoint sweep needs base.adaptive = 1 (without the control in the drift the state path carries no parameter dependence)");
    if (b.h_kind != PSP_GH_QUAD) return fail(-1, "the adjoint sweep is defined for h = -|z|^2 / 2 - f(x) only (PSP_GH_QUAD)");
    if (p->a.dense && !(p->a.lq && p->a.z_sigma))
        return fail(-1, "the adjoint sweep runs in the orientation Z = sigma grad V (PSP_GENL_Z_SIGMA), not PSP_GENL_Z_SIGMA_T");
    if (!b.per_sample_weights || !b.store_path) return fail(-1, "the adjoint sweep needs base.per_sample_weights = 1 and base.store_path = 1");
    long long tofs = (p->table_floats + 3) & ~3LL;
    *tAT = tofs;
    if (p->a.driftA) tofs += (long long)p->a.DB0 * 4 * p->a.DB0 * 64;
    *table_floats = tofs;
    *lds = psp::genl_adj_lds_bytes(p->a.TB, p->a.DB0);
    if (*lds > kMaxLds) return fail(-3, "value net: the images of the adjoint sweep exceed the 160 KiB LDS (sum of the padded widths too large)");
    return 0;
}
}  // namespace

int psp_genl_query_adj(const psp_genl_config* cfg, const psp_genl_coeffs* coeffs, const psp_genl_ul2* ul2, psp_genl_adj* adj,
                       psp_genl_sizes* out) {
    GenlPlan p;
    long long tAT = 0, tf = 0;
    int lds = 0;
    int rc = make_genl_adj_plan(cfg, coeffs, ul2, adj, &p, &tAT, &tf, &lds);
    if (rc) return rc;
    rc = psp_genl_query_ul2(cfg, coeffs, ul2, out);
    if (rc) return rc;
    out->table_bytes = tf * 4;
    adj->drift_t_offset = tAT;
    return 0;
}

int psp_genl_adjoint_sweep(const psp_genl_config* cfg, const psp_genl_coeffs* coeffs, const psp_genl_adj* adj, const float* params,
                           float* tables, float* path, float* ahat, float* ws, void* stream) {
    GenlPlan p;
    long long tAT = 0, tf = 0;
    int lds = 0;
    int rc = make_genl_adj_plan(cfg, coeffs, nullptr, adj, &p, &tAT, &tf, &lds);
    if (rc) return rc;
    if (!params || !tables || !path || !ahat || !ws || !adj->mu || !adj->resid_coeff || !adj->lam_N)
        return fail(-1, "null buffer passed to psp_genl_adjoint_sweep");
    if (p.a.driftA && (adj->drift_t_offset < tAT || (adj->drift_t_offset & 3) != 0))
        return fail(-1, "psp_genl_adj.drift_t_offset is not the one psp_genl_query_adj wrote");
    psp::GenlAdjArgs aa;
    memset(&aa, 0, sizeof(aa));
    aa.a = p.a;
    aa.a.tables = tables; aa.a.tables_w = tables;
    aa.a.g.params = params; aa.a.g.path = path;
    aa.mu = adj->mu; aa.resid = adj->resid_coeff; aa.lamN = adj->lam_N; aa.lam0 = adj->lam0_out;
    aa.coef_out = ahat; aa.wt_out = ws;
    aa.tAT = adj->drift_t_offset;
    hipError_t e = psp::genl_adj_launch(aa, p.nw_fwd, p.ntile16, lds, (hipStream_t)stream);       // (genl_adj_instance.hip)
    return hip_rc(e, "genl_adj_kernel launch");
}

// ---- the K_test_log diagnostic on the device (genl_eval_kernels.h) ----------------------------------------------------------
namespace {
struct EvalPlan { GenlPlan p; int grid, nw, lds; };
// every check of a psp_genl_eval_config (psp_genl_eval_query and psp_genl_test_error share it); the net goes through
// make_genl_plan as a one-step rollout of K_points trajectories, which also applies its waves-per-tile rule to K_points.
// (Its LDS test of the rollout kernels cannot fire here: the shape limits -- 7 input and 4 x 8 hidden blocks, TB <= 39 -- keep
//  the rollout's largest request, (4 TB - 2 DB0 + 2) KiB <= 144 KiB, below the 160 KiB, so every net that passes the shape checks
//  is served; the evaluation itself asks for TB KiB.)
int make_eval_plan(const psp_genl_eval_config* c, EvalPlan* e) {
    if (!c) return fail(-1, "null config");
    if (c->K_points <= 0) return fail(-1, "K_points must be positive");
    if (c->k_offset < 0 || c->k_offset + (int64_t)c->K_points > (1LL << 32)) return fail(-1, "k_offset + K_points must stay within 2^32");
    if (c->sample_kind < PSP_TSAMPLE_SUPPLIED || c->sample_kind > PSP_TSAMPLE_BOX)
        return fail(-1, "sample_kind out of range (PSP_TSAMPLE_SUPPLIED, _BALL, _ANNULUS, _BOX)");
    if (c->vtrue_kind < PSP_VTRUE_EXP || c->vtrue_kind > PSP_VTRUE_SINR2 ||
        (c->vtrue_kind > PSP_VTRUE_COMMITTOR && c->vtrue_kind < PSP_VTRUE_LOGQ))
        return fail(-1, "vtrue_kind out of range (PSP_VTRUE_EXP, _QUAD, _COMMITTOR; _LOGQ, _SINPROD, _SINSUM, _SINR2)");
    if (c->vtrue_kind == PSP_VTRUE_LOGQ && !(c->vtrue_par[0] > 0.f)) return fail(-1, "PSP_VTRUE_LOGQ: the divisor p0 must be positive");
    if (c->vtrue_kind == PSP_VTRUE_SINPROD && c->d < 2) return fail(-1, "PSP_VTRUE_SINPROD reads the coordinates x_0 and x_1 (d >= 2)");
    if (c->sample_kind == PSP_TSAMPLE_BALL && !(c->bound_b > 0.f)) return fail(-1, "ball radius must be positive");
    if (c->sample_kind == PSP_TSAMPLE_ANNULUS && !(c->bound_a >= 0.f && c->bound_a < c->bound_b))
        return fail(-1, "annulus radii must satisfy 0 <= r_1 < r_2");
    if (c->sample_kind == PSP_TSAMPLE_BOX && !(c->bound_a < c->bound_b)) return fail(-1, "box bounds must satisfy X_l < X_r");
    if (c->vtrue_kind == PSP_VTRUE_COMMITTOR && !(c->vtrue_par[0] > 0.f)) return fail(-1, "committor: inner radius must be positive");
    if (c->log_slots <= 0) return fail(-1, "log_slots must be positive");
    psp_genl_config g;
    memset(&g, 0, sizeof(g));
    g.base.d = c->d; g.base.K_local = c->K_points; g.base.N = 1;
    g.has_time = c->has_time; g.n_hidden = c->n_hidden;
    for (int i = 0; i < 4; ++i) g.widths[i] = c->widths[i];
    g.activation = c->activation; g.linear_layout = c->linear_layout; g.time_first = c->time_first; g.time_scale = c->time_scale;
    const int rc = make_genl_plan(&g, &e->p);
    if (rc) return rc;
    e->grid = e->p.ntile16;
    e->nw = e->p.nw_bwd;                                              // 1 or 8 (nw_fwd may read 4: a refinement of the rollout only)
    e->lds = psp::genl_eval_lds_bytes(e->p.a.TB);
    return 0;
}
}  // namespace

int psp_abi_struct_sizes4(int32_t out[2]) {
    if (!out) return fail(-1, "null output");
    out[0] = (int32_t)sizeof(psp_genl_eval_config); out[1] = (int32_t)sizeof(psp_genl_eval_sizes);
    return 0;
}

int psp_genl_eval_query(const psp_genl_eval_config* cfg, psp_genl_eval_sizes* out) {
    EvalPlan e;
    const int rc = make_eval_plan(cfg, &e);
    if (rc) return rc;
    if (!out) return fail(-1, "null output");
    memset(out, 0, sizeof(*out));
    out->table_bytes = e.p.table_floats * 4;
    out->partial_bytes = (int64_t)e.grid * psp::kEvalStats * 8;
    out->n_params = e.p.n_params;
    out->workgroups = e.grid;
    out->waves_per_tile = e.nw;
    out->lds_bytes = e.lds;
    return 0;
}

int psp_genl_test_error(const psp_genl_eval_config* cfg, const float* params, const float* x, const float* t, uint64_t seed,
                        uint32_t iter, float* tables, double* partial, double* log_out, int32_t slot, const uint32_t* slot_dev,
                        float* x_out, float* t_out, float* v_out, float* vtrue_out, int32_t* keep_out, void* stream) {
    EvalPlan e;
    const int rc = make_eval_plan(cfg, &e);
    if (rc) return rc;
    if (!params || !tables || !partial || !log_out) return fail(-1, "null buffer passed to psp_genl_test_error");
    const bool supplied = cfg->sample_kind == PSP_TSAMPLE_SUPPLIED;
    if (supplied && (!x || (cfg->has_time && !t))) return fail(-1, "PSP_TSAMPLE_SUPPLIED needs x (and t with a time input)");
    if (!supplied && (x || t)) return fail(-1, "x / t are the points of PSP_TSAMPLE_SUPPLIED only");
    if (!slot_dev && (slot < 0 || slot >= cfg->log_slots)) return fail(-1, "slot outside [0, log_slots)");
    psp::GenlEvalArgs ea;
    memset(&ea, 0, sizeof(ea));
    ea.n = e.p.a;
    ea.n.tables = tables; ea.n.tables_w = tables;
    ea.n.g.params = params;
    ea.x = x; ea.t = t; ea.k_offset = cfg->k_offset; ea.K = cfg->K_points;
    ea.sample_kind = cfg->sample_kind; ea.lo = cfg->bound_a; ea.hi = cfg->bound_b; ea.T = cfg->T;
    ea.vtrue_kind = cfg->vtrue_kind;
    for (int i = 0; i < 4; ++i) ea.vp[i] = cfg->vtrue_par[i];
    if (cfg->vtrue_kind == PSP_VTRUE_COMMITTOR) {
        const double a = cfg->vtrue_par[0], c = cfg->vtrue_par[1], dd = cfg->vtrue_par[2];
        ea.vden = (float)(a * a - pow(c, 2.0 - dd) * pow(a, dd));
    }
    ea.key0 = (uint32_t)seed; ea.key1 = (uint32_t)(seed >> 32) ^ psp::kTestKeyXor; ea.iter = iter;
    ea.partial = partial; ea.log_out = log_out; ea.slot_dev = slot_dev; ea.slot = slot; ea.log_slots = cfg->log_slots;
    ea.x_out = x_out; ea.t_out = t_out; ea.v_out = v_out; ea.vtrue_out = vtrue_out; ea.keep_out = keep_out;
    hipStream_t st = (hipStream_t)stream;
    if (const int rct = PSP_LAUNCH(genl_tables_kernel, dim3(128), dim3(256), 0, st, ea.n)) return rct;
    const hipError_t err = psp::genl_eval_launch(ea, e.nw, e.grid, e.lds, st);
    return hip_rc(err, "genl_eval_kernel launch");
}

// ---- collectives: RCCL on the caller's stream, bound lazily so that the library loads without librccl ---------------
namespace {
struct Rccl {
    void* handle = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
};
Rccl g_rccl;
int bind_rccl() {
    if (g_rccl.handle) return 0;
    // a process that already loaded RCCL (torch ships its own librccl.so.1) gets that copy back: same soname
    void* h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
    if (!h) h = dlopen("/opt/rocm/lib/librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!h) return fail(-20, "cannot load librccl.so.1: %s", dlerror());
    Rccl r;
    r.handle = h;
    r.GetUniqueId = reinterpret_cast<decltype(r.GetUniqueId)>(dlsym(h, "ncclGetUniqueId"));
    r.CommInitRank = reinterpret_cast<decltype(r.CommInitRank)>(dlsym(h, "ncclCommInitRank"));
    r.CommDestroy = reinterpret_cast<decltype(r.CommDestroy)>(dlsym(h, "ncclCommDestroy"));
    r.AllReduce = reinterpret_cast<decltype(r.AllReduce)>(dlsym(h, "ncclAllReduce"));
    r.GetErrorString = reinterpret_cast<decltype(r.GetErrorString)>(dlsym(h, "ncclGetErrorString"));
    if (!r.GetUniqueId || !r.CommInitRank || !r.CommDestroy || !r.AllReduce || !r.GetErrorString)
        return fail(-20, "librccl.so.1 lacks an expected entry point");
    g_rccl = r;
    return 0;
}
int fail_rccl(ncclResult_t e, const char* where) {
    snprintf(g_err, sizeof(g_err), "%s: %s", where, g_rccl.GetErrorString ? g_rccl.GetErrorString(e) : "RCCL error");
    return -21;
}
}  // namespace

int psp_comm_unique_id(unsigned char id_out[PSP_COMM_ID_BYTES]) {
    static_assert(sizeof(ncclUniqueId) == PSP_COMM_ID_BYTES, "ncclUniqueId size");
    if (!id_out) return fail(-1, "null id buffer");
    int rc = bind_rccl();
    if (rc) return rc;
    ncclUniqueId id;
    ncclResult_t e = g_rccl.GetUniqueId(&id);
    if (e != ncclSuccess) return fail_rccl(e, "ncclGetUniqueId");
    memcpy(id_out, &id, sizeof(id));
    return 0;
}

int psp_comm_init(void** comm_out, int32_t nranks, int32_t rank, const unsigned char id[PSP_COMM_ID_BYTES]) {
    if (!comm_out || !id) return fail(-1, "null argument to psp_comm_init");
    if (nranks <= 0 || rank < 0 || rank >= nranks) return fail(-1, "psp_comm_init needs 0 <= rank < nranks");
    int rc = bind_rccl();
    if (rc) return rc;
    ncclUniqueId uid;
    memcpy(&uid, id, sizeof(uid));
    ncclComm_t comm = nullptr;
    ncclResult_t e = g_rccl.CommInitRank(&comm, nranks, uid, rank);
    if (e != ncclSuccess) return fail_rccl(e, "ncclCommInitRank");
    *comm_out = comm;
    return 0;
}

int psp_comm_destroy(void* comm) {
    if (!comm) return 0;
    int rc = bind_rccl();
    if (rc) return rc;
    ncclResult_t e = g_rccl.CommDestroy(static_cast<ncclComm_t>(comm));
    if (e != ncclSuccess) return fail_rccl(e, "ncclCommDestroy");
    return 0;
}

int psp_allreduce(void* buf, int64_t n, int32_t dtype, void* comm, void* stream) {
    if (!buf || !comm) return fail(-1, "null buffer / communicator passed to psp_allreduce");
    if (n <= 0) return fail(-1, "psp_allreduce needs n > 0");
    if (dtype != PSP_DT_F32 && dtype != PSP_DT_F64) return fail(-1, "psp_allreduce: dtype must be PSP_DT_F32 or PSP_DT_F64");
    int rc = bind_rccl();
    if (rc) return rc;
    ncclResult_t e = g_rccl.AllReduce(buf, buf, (size_t)n, dtype == PSP_DT_F32 ? ncclFloat32 : ncclFloat64, ncclSum,
                                      static_cast<ncclComm_t>(comm), (hipStream_t)stream);
    if (e != ncclSuccess) return fail_rccl(e, "ncclAllReduce");
    return 0;
}

int psp_adam_step(float* params, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                  int32_t step, float lr, float beta1, float beta2, float eps, void* stream) {
    if (!params || !grad || !exp_avg || !exp_avg_sq) return fail(-1, "null buffer passed to psp_adam_step");
    if (n <= 0 || step <= 0) return fail(-1, "psp_adam_step needs n > 0 and a 1-based step");
    // bias corrections in double on the host, as torch does for python-float steps
    const double bc1 = 1.0 - pow((double)beta1, (double)step);
    const double bc2 = 1.0 - pow((double)beta2, (double)step);
    const float step_size = (float)((double)lr / bc1);
    const float bc2_sqrt = (float)sqrt(bc2);
    return PSP_LAUNCH(adam_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, params, grad, exp_avg, exp_avg_sq,
                      (long long)n, lr, beta1, beta2, eps, step_size, bc2_sqrt);
}

// sigma-basis plans (include/psp.h): W~1x = W1x B into the kernel-layout parameters, dW1x = dW~1x B^T on the reduced gradient
static int basis_check(const void* a, const void* b, const float* B, int32_t d, int32_t H, const char* who) {
    if (!a || !b || !B) { snprintf(g_err, sizeof(g_err), "null buffer passed to %s", who); return -1; }
    if (d <= 0 || H <= 0) { snprintf(g_err, sizeof(g_err), "%s needs d > 0 and H > 0", who); return -1; }
    if (psp::basis_lds_bytes(d) > 64 * 1024) { snprintf(g_err, sizeof(g_err), "%s: B does not fit 64 KiB of LDS (narrow kernel family only, d <= 112)", who); return -3; }
    return 0;
}
int psp_hjb_basis_params(const float* params, float* params_out, const float* B, int32_t d, int32_t H, int64_t n_params,
                         void* stream) {
    int rc = basis_check(params, params_out, B, d, H, "psp_hjb_basis_params");
    if (rc) return rc;
    if (n_params < (int64_t)H * (d + 1)) return fail(-1, "psp_hjb_basis_params: n_params is smaller than W1");
    hipError_t e = psp::launch_basis_w1<false>(params, params_out, B, d, H, (long long)n_params, (hipStream_t)stream);
    return hip_rc(e, "hjb_basis_w1_kernel launch");
}
int psp_hjb_basis_grad(float* grad, const float* B, int32_t d, int32_t H, void* stream) {
    int rc = basis_check(grad, grad, B, d, H, "psp_hjb_basis_grad");
    if (rc) return rc;
    hipError_t e = psp::launch_basis_w1<true>(grad, grad, B, d, H, (long long)H * (d + 1), (hipStream_t)stream);
    return hip_rc(e, "hjb_basis_w1_kernel launch");
}

int psp_philox_normal_fill(float* out, int32_t N, int32_t K_local, int32_t d, int64_t k_offset,
                           uint64_t seed, uint32_t iter, void* stream) {
    if (!out || N <= 0 || K_local <= 0 || d <= 0) return fail(-1, "bad arguments to psp_philox_normal_fill");
    const long long n0 = (long long)K_local * d;
    if (const int rc = PSP_LAUNCH(zero_kernel, dim3((unsigned)((n0 + 255) / 256)), dim3(256), 0, stream, out, n0)) return rc;
    const long long total = (long long)N * K_local * (((d + 15) / 16) * 4);
    return PSP_LAUNCH(philox_fill_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, out, N, K_local, d,
                      (long long)k_offset, (uint32_t)seed, (uint32_t)(seed >> 32), iter);
}

int psp_hjb_control_eval(int32_t d, int32_t H, const float* params, const float* X, int32_t K, float t,
                         float* minus_Z_out, void* stream) {
    if (!params || !X || !minus_Z_out || d <= 0 || H <= 0 || K <= 0)
        return fail(-1, "bad arguments to psp_hjb_control_eval");
    return PSP_LAUNCH(control_eval_kernel, dim3(K), dim3(64), 2 * H * sizeof(float), stream, d, H, params, X, K, t, minus_Z_out);
}

// ---- the PINN loss (pinn_kernels.h) ---------------------------------------------------------------------------------------
namespace {
struct PinnPlan { psp::PinnArgs a; int lds_fwd, lds_bwd; int64_t scratch_floats; };
// every check of a psp_pinn_config (the three entry points share it) and the launch geometry; `pairs`: the psp_pinn_pairs_* entry
// points, which take an h that reads t
int make_pinn_plan(const psp_pinn_config* c, PinnPlan* p, bool pairs = false) {
    if (!c) return fail(-1, "null config");
    if (c->d <= 0 || c->K <= 0) return fail(-1, "psp_pinn: d and K must be positive");
    if (c->has_time != 0 && c->has_time != 1) return fail(-1, "psp_pinn: has_time must be 0 or 1");
    if (c->sigma_kind != PSP_GENL_SIGMA_SCALED && c->sigma_kind != PSP_GENL_SIGMA_DENSE)
        return fail(-1, "psp_pinn: sigma_kind out of range");
    const bool dense = c->sigma_kind == PSP_GENL_SIGMA_DENSE;
    if (pairs && !c->has_time) return fail(-1, "psp_pinn_pairs: the (K, K) residual needs a time input (has_time = 1)");
    if (pairs && dense) return fail(-1, "psp_pinn_pairs: a dense sigma is not built with an h that reads t");
    if (dense && !c->dirs) return fail(-4, "psp_pinn: a dense sigma needs its direction table (dirs)");
    if (dense && (c->n_dirs < 1 || c->n_dirs > c->d)) return fail(-1, "psp_pinn: n_dirs must lie in 1 .. d");
    if (c->n_hidden < 1 || c->n_hidden > 4) return fail(-2, "psp_pinn: 1 to 4 hidden layers");
    const int n_in = c->d + c->has_time;
    if (n_in > 112) return fail(-2, "psp_pinn: net input (d + has_time) above 112");
    for (int i = 0; i < c->n_hidden; ++i)
        if (c->widths[i] < 1 || c->widths[i] > 128) return fail(-2, "psp_pinn: hidden widths must lie in 1 .. 128");
    if (c->activation < PSP_ACT_RELU2 || c->activation > PSP_ACT_TANH) return fail(-1, "psp_pinn: activation out of range");
    if (c->linear_layout != 0 && c->linear_layout != 1) return fail(-1, "psp_pinn: linear_layout must be 0 or 1");
    if (c->drift_kind != PSP_DRIFT_ZERO && c->drift_kind != PSP_DRIFT_DIAG && c->drift_kind != PSP_DRIFT_DOUBLE_WELL)
        return fail(-1, "psp_pinn: drift_kind must be PSP_DRIFT_ZERO, _DIAG or _DOUBLE_WELL");
    if (c->drift_kind != PSP_DRIFT_ZERO && !c->drift) return fail(-1, "psp_pinn: this drift_kind needs the drift vector");
    if (c->h_kind < PSP_GH_ZERO || c->h_kind > PSP_GH_SINNORM2) return fail(-1, "psp_pinn: h_kind out of range");
    if (c->h_kind == PSP_GH_SINNORM2) return fail(-1, "psp_pinn: PSP_GH_SINNORM2 is not built in the PINN kernels");
    const bool catalogue = c->h_kind == PSP_GH_AFFINE_EXP || c->h_kind == PSP_GH_SINE_SOURCE;      // their h_par is no (al, d, e, tau)
    if (pairs && catalogue) return fail(-1, "psp_pinn_pairs: PSP_GH_AFFINE_EXP / PSP_GH_SINE_SOURCE do not read t; use psp_pinn_*");
    if (int rc = check_gh_par(c->h_kind, c->h_par, c->d)) return rc;
    if (!pairs && !catalogue && c->h_kind >= PSP_GH_EXPBALL_LIN && c->h_par[3] != 0.f) return fail(-1, "psp_pinn: an h that reads t is not built");
    if (pairs) {
        if (c->h_kind >= PSP_GH_EXPBALL_LIN && c->h_par[3] != 0.f && c->h_kind != PSP_GH_EXPBALL_SQ && c->h_kind != PSP_GH_EXPBALL_SIN)
            return fail(-1, "psp_pinn_pairs: only PSP_GH_EXPBALL_SQ and PSP_GH_EXPBALL_SIN read t (h_par[3] != 0)");
        if (c->K > psp::kPinnPairMaxK) return fail(-1, "psp_pinn_pairs: K above 16384 (K^2 pairs per iteration)");
    }
    if (dense && (c->h_kind == PSP_GH_QUAD || (c->h_kind == PSP_GH_AFFINE_EXP && c->h_par[2] != 0.f)))
        return fail(-1, "psp_pinn: an h that reads z = B grad V is not built for dense directions");
    // the gradient directions are dropped where nothing reads grad V: no drift, no time input, an h that does not read z
    const int n_hess = dense ? c->n_dirs : 0;
    const int n_grad = (dense && c->drift_kind == PSP_DRIFT_ZERO && !c->has_time) ? 0 : n_in;
    const int nblk = (n_grad + n_hess + psp::kPinnDirs - 1) / psp::kPinnDirs;
    if ((int64_t)c->K * nblk > (1 << 24)) return fail(-1, "psp_pinn: K too large");
    psp::PinnArgs& a = p->a;
    memset(&a, 0, sizeof(a));
    a.d = c->d; a.n_in = n_in; a.K = c->K; a.L = c->n_hidden; a.act = c->activation;
    a.nblk = nblk;
    a.ntiles = a.K * a.nblk;
    a.n_grad = n_grad; a.n_hess = n_hess;
    a.cnt_lo = dense ? n_grad : 0; a.cnt_hi = dense ? n_grad + n_hess : c->d;
    a.lap_coef = dense ? 0.5f : 0.5f * c->sigma_scale * c->sigma_scale;
    a.dirs = dense ? c->dirs : nullptr;
    int fan = n_in, off = 0;
    for (int i = 0; i <= a.L; ++i) {
        const int H = i < a.L ? c->widths[i] : 1;
        if (i < a.L) a.H[i] = H;
        a.fan[i] = fan;
        a.offW[i] = off; off += fan * H;
        a.offb[i] = off; off += H;
        a.sk[i] = c->linear_layout ? 1 : H;
        a.sc[i] = c->linear_layout ? fan : 1;
        fan += H;
    }
    a.TOT = a.fan[a.L];
    a.AST = psp::pinn_row_stride(a.TOT);
    a.P = off;
    a.G = a.ntiles < psp::kPinnMaxWg ? a.ntiles : psp::kPinnMaxWg;
    a.drift_kind = c->drift_kind; a.h_kind = c->h_kind; a.s = c->sigma_scale;
    for (int i = 0; i < 4; ++i) a.h_par[i] = c->h_par[i];
    a.drift = c->drift;
    a.pairs = pairs ? 1 : 0;
    p->lds_fwd = psp::pinn_lds_bytes(a.AST, a.L, false);
    p->lds_bwd = psp::pinn_lds_bytes(a.AST, a.L, true);
    if (p->lds_bwd > kMaxLds) return fail(-3, "psp_pinn: the activation images exceed the LDS");
    p->scratch_floats = (int64_t)a.K * (2 + a.nblk + 2 * n_grad);
    return 0;
}
void pinn_scratch(PinnPlan* p, float* scratch) {
    psp::PinnArgs& a = p->a;
    const size_t K = (size_t)a.K;
    a.V = scratch; a.lap = a.V + K; a.gradV = a.lap + K * a.nblk; a.cV = a.gradV + K * a.n_grad; a.cG = a.cV + K;
}
int pinn_fill_sizes(const PinnPlan& p, psp_pinn_sizes* out) {
    if (!out) return fail(-1, "null output");
    memset(out, 0, sizeof(*out));
    out->n_params = p.a.P;
    out->scratch_bytes = p.scratch_floats * 4;
    out->grad_partial_bytes = (int64_t)p.a.G * p.a.P * 4;
    out->dir_blocks = p.a.nblk; out->tiles = p.a.ntiles; out->bwd_workgroups = p.a.G;
    out->lds_fwd_bytes = p.lds_fwd; out->lds_bwd_bytes = p.lds_bwd;
    return 0;
}
}  // namespace

int psp_abi_struct_sizes5(int32_t out[2]) {
    if (!out) return fail(-1, "null output");
    out[0] = (int32_t)sizeof(psp_pinn_config); out[1] = (int32_t)sizeof(psp_pinn_sizes);
    return 0;
}

int psp_pinn_query(const psp_pinn_config* cfg, psp_pinn_sizes* out) {
    PinnPlan p;
    const int rc = make_pinn_plan(cfg, &p);
    if (rc) return rc;
    return pinn_fill_sizes(p, out);
}

int psp_pinn_residual(const psp_pinn_config* cfg, const float* params, const float* x, const float* t, float* scratch,
                      float* R_out, void* stream) {
    PinnPlan p;
    const int rc = make_pinn_plan(cfg, &p);
    if (rc) return rc;
    if (!params || !x || !scratch || !R_out) return fail(-1, "null buffer passed to psp_pinn_residual");
    if (cfg->has_time && !t) return fail(-1, "psp_pinn_residual: a net with a time input needs t");
    pinn_scratch(&p, scratch);
    p.a.params = params; p.a.x = x; p.a.t = t; p.a.R = R_out;
    const hipError_t e = psp::pinn_launch_forward(p.a, p.lds_fwd, (hipStream_t)stream);
    return hip_rc(e, "pinn_forward_kernel launch");
}

int psp_pinn_backward(const psp_pinn_config* cfg, const float* params, const float* x, const float* t, const float* scratch,
                      const float* rbar, float* grad_partial, float* grad_out, void* stream) {
    PinnPlan p;
    const int rc = make_pinn_plan(cfg, &p);
    if (rc) return rc;
    if (!params || !x || !scratch || !rbar || !grad_partial || !grad_out) return fail(-1, "null buffer passed to psp_pinn_backward");
    if (cfg->has_time && !t) return fail(-1, "psp_pinn_backward: a net with a time input needs t");
    pinn_scratch(&p, const_cast<float*>(scratch));
    p.a.params = params; p.a.x = x; p.a.t = t; p.a.rbar = rbar; p.a.gpart = grad_partial;
    const hipError_t e = psp::pinn_launch_backward(p.a, p.lds_bwd, (hipStream_t)stream);
    if (e != hipSuccess) return fail_hip(e, "pinn_backward_kernel launch");
    return PSP_LAUNCH(reduce_grad_kernel, dim3((p.a.P + 31) / 32), dim3(256), 0, stream, grad_partial, p.a.G, p.a.P, grad_out);
}

// ---- the (K, K) residual of an h that reads t (pinn_kernels.h) ---------------------------------------------------------------
int psp_pinn_pairs_query(const psp_pinn_config* cfg, psp_pinn_sizes* sizes_out, int64_t* pair_work_bytes_out) {
    PinnPlan p;
    const int rc = make_pinn_plan(cfg, &p, true);
    if (rc) return rc;
    if (!sizes_out || !pair_work_bytes_out) return fail(-1, "null output");
    const int rc2 = pinn_fill_sizes(p, sizes_out);
    if (rc2) return rc2;
    *pair_work_bytes_out = (int64_t)p.a.K * (int64_t)sizeof(double);
    return 0;
}

int psp_pinn_pairs_residual(const psp_pinn_config* cfg, const float* params, const float* x, const float* t, float* scratch,
                            float* A_out, void* stream) {
    PinnPlan p;
    const int rc = make_pinn_plan(cfg, &p, true);
    if (rc) return rc;
    if (!params || !x || !t || !scratch || !A_out) return fail(-1, "null buffer passed to psp_pinn_pairs_residual");
    pinn_scratch(&p, scratch);
    p.a.params = params; p.a.x = x; p.a.t = t; p.a.R = A_out;
    const hipError_t e = psp::pinn_launch_forward(p.a, p.lds_fwd, (hipStream_t)stream);
    return hip_rc(e, "pinn_forward_kernel launch");
}

int psp_pinn_pairs_reduce(const psp_pinn_config* cfg, const float* x, const float* t, const float* scratch, const float* A,
                          float alpha0, void* pair_work, float* loss_out, float* rho_out, float* nu_out, void* stream) {
    PinnPlan p;
    const int rc = make_pinn_plan(cfg, &p, true);
    if (rc) return rc;
    if (!x || !t || !scratch || !A || !pair_work || !loss_out || !rho_out || !nu_out)
        return fail(-1, "null buffer passed to psp_pinn_pairs_reduce");
    pinn_scratch(&p, const_cast<float*>(scratch));
    psp::PinnPairArgs a;
    memset(&a, 0, sizeof(a));
    const double K2 = (double)cfg->K * (double)cfg->K;
    a.d = cfg->d; a.K = cfg->K; a.h_kind = cfg->h_kind;
    a.al = cfg->h_par[0]; a.tau2 = 2.0f * cfg->h_par[3];
    a.coef = (float)(2.0 * (double)alpha0 / K2); a.loss_coef = (double)alpha0 / K2;
    a.x = x; a.t = t; a.V = p.a.V; a.A = A;
    a.rho = rho_out; a.nu = nu_out; a.work = static_cast<double*>(pair_work); a.loss = loss_out;
    const hipError_t e = psp::pinn_launch_pairs(a, (hipStream_t)stream);
    return hip_rc(e, "pinn_pair_kernel launch");
}

int psp_pinn_pairs_backward(const psp_pinn_config* cfg, const float* params, const float* x, const float* t, const float* scratch,
                            const float* rbar, const float* vadd, float* grad_partial, float* grad_out, void* stream) {
    PinnPlan p;
    const int rc = make_pinn_plan(cfg, &p, true);
    if (rc) return rc;
    if (!params || !x || !t || !scratch || !rbar || !grad_partial || !grad_out)
        return fail(-1, "null buffer passed to psp_pinn_pairs_backward");
    pinn_scratch(&p, const_cast<float*>(scratch));
    p.a.params = params; p.a.x = x; p.a.t = t; p.a.rbar = rbar; p.a.vadd = vadd; p.a.gpart = grad_partial;
    const hipError_t e = psp::pinn_launch_backward(p.a, p.lds_bwd, (hipStream_t)stream);
    if (e != hipSuccess) return fail_hip(e, "pinn_backward_kernel launch");
    return PSP_LAUNCH(reduce_grad_kernel, dim3((p.a.P + 31) / 32), dim3(256), 0, stream, grad_partial, p.a.G, p.a.P, grad_out);
}

// ---- statistics of the loss estimators over chunks of (Y_N, D) (csrc/lstat_kernels.h) ------------------------------------------
int64_t psp_loss_stats_state_bytes(void) { return (int64_t)psp::kLstatStateDoubles * 8; }

int psp_loss_stats_accumulate(const float* Y, const float* D, int64_t n, double* state, void* stream) {
    if (!Y || !D || !state) return fail(-1, "null buffer passed to psp_loss_stats_accumulate");
    if (n < 0) return fail(-1, "psp_loss_stats_accumulate: n must not be negative");
    if (n == 0) return 0;
    psp::LstatArgs a;
    a.Y = Y; a.D = D; a.n = n; a.state = state; a.G = psp::lstat_grid(n);
    return hip_rc(psp::lstat_launch_accumulate(a, (hipStream_t)stream), "lstat kernels launch");
}

int psp_loss_stats_finish(const double* state, double* out, void* stream) {
    if (!state || !out) return fail(-1, "null buffer passed to psp_loss_stats_finish");
    return hip_rc(psp::lstat_launch_finish(state, out, (hipStream_t)stream), "lstat_finish_kernel launch");
}

}  // extern "C"
