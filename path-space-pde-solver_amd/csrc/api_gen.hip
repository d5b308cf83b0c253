// api_gen.hip -- C ABI of the GeneralSolver / EllipticSolver rollouts with a two-hidden-layer value net (include/psp.h: psp_gen_*)
// on gen_kernels.h.  The rollout kernels are those of the gen_instance.hip units (gen_instances.def); the two kernels of this
// family's range guard are defined here, the partial gradients are summed by reduce_grad_kernel (api_common.hip).
#include "api_common.h"
#include "gen_kernels.h"

using namespace psp_api;

PSP_SAME(psp::GH_ZERO, PSP_GH_ZERO); PSP_SAME(psp::GH_QUAD, PSP_GH_QUAD); PSP_SAME(psp::GH_ALLEN_CAHN, PSP_GH_ALLEN_CAHN);
PSP_SAME(psp::GH_EXPBALL_LIN, PSP_GH_EXPBALL_LIN); PSP_SAME(psp::GH_EXPBALL_SQ, PSP_GH_EXPBALL_SQ);
PSP_SAME(psp::GH_EXPBALL_SIN, PSP_GH_EXPBALL_SIN); PSP_SAME(psp::GH_EXPBALL_SIN_FULL, PSP_GH_EXPBALL_SIN_FULL);
PSP_SAME(psp::GH_AFFINE_EXP, PSP_GH_AFFINE_EXP); PSP_SAME(psp::GH_SINE_SOURCE, PSP_GH_SINE_SOURCE);
PSP_SAME(psp::GH_SINNORM2, PSP_GH_SINNORM2);
PSP_SAME(psp::DOM_NONE, PSP_DOM_NONE); PSP_SAME(psp::DOM_SPHERE, PSP_DOM_SPHERE); PSP_SAME(psp::DOM_BOX, PSP_DOM_BOX);
PSP_SAME(psp::DOM_BOX_UPPER_ALL, PSP_DOM_BOX_UPPER_ALL); PSP_SAME(psp::DOM_BOX_UPPER_ANY, PSP_DOM_BOX_UPPER_ANY);
PSP_SAME(psp::DOM_ANNULUS, PSP_DOM_ANNULUS);

#define X(D_, H_) PSP_DECLARE_GEN_INSTANCE(D_, H_)
#include "gen_instances.def"
#undef X

namespace {
const Entry<psp::GenInstance> kGenTable[] = {
#define X(D_, H_) {D_, H_, &psp_gen_instance_##D_##_##H_},
#include "gen_instances.def"
#undef X
};

struct GenPlan {
    psp::GenInstance inst;
    int ntile16, fwd_waves, fwd_grid, bwd_grid;
};

int make_gen_plan(const psp_gen_config* c, GenPlan* p) {
    if (!c) return fail(-1, "null config");
    if (c->d <= 0 || c->H <= 0 || c->K_local <= 0 || c->N <= 0) return fail(-1, "non-positive d/H/K/N");
    if (!find_in(kGenTable, c->d, c->H, &p->inst))
        return fail(-2, "no compiled GeneralSolver kernel instance for d=%d H=%d", c->d, c->H);
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

void fill_gen_args(const psp_gen_config* c, const GenPlan& p, psp::GenArgs* a) {
    memset(a, 0, sizeof(*a));
    fill_gen_problem(*c, p.ntile16, a);
    a->d_real = (c->d_real > 0 && c->d_real < c->d) ? c->d_real : c->d;
    a->Vsteps = c->v_steps_out; a->Ysteps = c->y_steps_out; a->per_sample = c->per_sample_weights ? 1 : 0;
    a->path16 = (c->mlp_dtype == PSP_MLP_BF16) ? 1 : 0;       // both kernels on bf16 MFMA: bf16-pair path block
}

__global__ void snapshot_u64_kernel(const unsigned long long* src, unsigned long long* dst) { *dst = *src; }
// range_flag_partials_kernel (api_common.hip) from two fp32 arrays of n entries (GeneralSolver: V(X_N) and Y_N per trajectory)
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
}  // namespace

extern "C" {

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
    return reduce_grad(grad_partial, p.bwd_grid, p.inst.n_params, grad_out, stream);
}

}  // extern "C"
