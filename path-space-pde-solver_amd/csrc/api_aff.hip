// api_aff.hip -- C ABI of the linear / affine / constant controls (include/psp.h: psp_aff_*) on aff_kernels.h: time_approx='outer'
// with a list of Linear / Affine / Constant.  The kernels are those of aff_instance.hip; the terminal sums are formed by
// reduce_partials_kernel (api_common.hip).
#include "api_common.h"
#include "aff_kernels.h"

using namespace psp_api;

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
    if (!find_in(kAffTable, b.d, 0, &p->inst))
        return fail(-2, "no compiled linear-control kernel bucket of width d=%d (16, 32, 64)", b.d);
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

extern "C" {

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
    return reduce_partials(fwd_partial, p.grid, sums_out, stream);
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

}  // extern "C"
