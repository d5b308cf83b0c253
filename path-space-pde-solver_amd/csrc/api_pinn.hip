// api_pinn.hip -- C ABI of the PINN loss (include/psp.h: psp_pinn_*, psp_pinn_pairs_*) on pinn_kernels.h.  The kernels are those of
// pinn_instance.hip; the partial gradients are summed by reduce_grad_kernel (api_common.hip).
#include "api_common.h"
#include "pinn_kernels.h"

using namespace psp_api;

PSP_SAME(psp::PINN_DRIFT_ZERO, PSP_DRIFT_ZERO); PSP_SAME(psp::PINN_DRIFT_DIAG, PSP_DRIFT_DIAG);
PSP_SAME(psp::PINN_DRIFT_DWELL, PSP_DRIFT_DOUBLE_WELL);
PSP_SAME(psp::PINN_ACT_RELU2, PSP_ACT_RELU2); PSP_SAME(psp::PINN_ACT_TANH2, PSP_ACT_TANH2); PSP_SAME(psp::PINN_ACT_TANH, PSP_ACT_TANH);

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

extern "C" {

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
    return reduce_grad(grad_partial, p.a.G, p.a.P, grad_out, stream);
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
    return reduce_grad(grad_partial, p.a.G, p.a.P, grad_out, stream);
}

}  // extern "C"
