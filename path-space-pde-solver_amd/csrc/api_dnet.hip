// api_dnet.hip -- C ABI of the DenseNet controls (include/psp.h: psp_dnet_*, psp_gradvar_finish) on hjbd_kernels.h:
// time_approx='outer' and DenseNet(d+1 -> d) controls.  The rollout kernels are those of the hjbd_instance.hip units
// (dense_instances.def); the two kernels of the gradient-variance diagnostic are defined here.
#include "api_common.h"
#include "hjbd_kernels.h"

using namespace psp_api;

PSP_SAME(psp::DRIFT_WELL_DIAG, PSP_DRIFT_WELL_DIAG); PSP_SAME(psp::DRIFT_RADIAL, PSP_DRIFT_RADIAL_WELL);
PSP_SAME(psp::TERM_QUADLIN, PSP_TERM_QUAD_LINEAR); PSP_SAME(psp::TERM_RADIAL, PSP_TERM_RADIAL_QUAD);

#define X(D_, H_) PSP_DECLARE_DNET_INSTANCE(D_, H_)
#include "dense_instances.def"
#undef X

namespace {
const Entry<psp::DnetInstance> kDnetTable[] = {
#define X(D_, H_) {D_, H_, &psp_dnet_instance_##D_##_##H_},
#include "dense_instances.def"
#undef X
};

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
    if (!find_in(kDnetTable, b.d, b.H, &p->inst))
        return fail(-2, "no compiled DenseNet-control kernel instance for d=%d H=%d", b.d, b.H);
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
    return reduce_partials(fwd_partial, p.grid, sums_out, stream);
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
                           [&]() { return range_flag_partials(fwd_partial, 2 * p.grid, b->range_flag, stream); },
                           fp32);
    const hipError_t e = fp32();
    return hip_rc(e, "hjbd_fwd_kernel launch");
}
