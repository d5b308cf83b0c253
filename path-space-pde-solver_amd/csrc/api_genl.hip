// api_genl.hip -- C ABI of the value nets of any depth (include/psp.h: psp_genl_*, psp_genl_eval_*) on genl_kernels.h: the rollout
// with its lq / ul2 / eig forwards, the backward, the adjoint sweep of the state path and the K_test_log diagnostic -- everything
// that embeds a GenlPlan.  This unit compiles genl_tables_kernel and the genl_fwd_kernel / genl_bwd_kernel instances of the plain
// rollout; the other forwards, the adjoint sweep and the evaluation are those of the genl_*_instance.hip units.
#include "api_common.h"
#include "genl_kernels.h"
#include "genl_eval_kernels.h"
#include "genl_adj_kernels.h"

using namespace psp_api;

PSP_SAME(psp::GH_EIG_FP, PSP_GH_EIG_FP); PSP_SAME(psp::GH_EIG_NLS, PSP_GH_EIG_NLS); PSP_SAME(psp::DRIFT_EIG_FP, PSP_DRIFT_EIG_FP);
PSP_SAME(psp::GACT_RELU2, PSP_ACT_RELU2); PSP_SAME(psp::GACT_TANH2, PSP_ACT_TANH2); PSP_SAME(psp::GACT_TANH, PSP_ACT_TANH);

using psp::genl_tables_kernel;     // (so that its message reads "genl_tables_kernel launch" like the others)

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

extern "C" {

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

}  // extern "C"

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

extern "C" {

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
    return reduce_grad(grad_partial, p.bwd_grid, (int)p.n_params, grad_out, st);
}

}  // extern "C"

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

extern "C" {

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

}  // extern "C"

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

extern "C" {

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

}  // extern "C"
