// api_is.hip -- C ABI of the importance-sampling rollouts (include/psp.h): psp_is_* on hjbe_kernels.h (d <= 64) and psp_isw_* on
// hjbew_kernels.h (d <= 256).  The kernels are those of hjbe_instance.hip / hjbew_instance.hip.
#include "api_common.h"
#include "hjbe_kernels.h"
#include "hjbew_kernels.h"

using namespace psp_api;

namespace {
// The checks of a psp_is_config that both kernels share, in the order in which they fire.  max_d / d_refusal: the caller's own
// limit on d and its message (two %d: d and the limit)
int is_check_config(const psp_is_config* c, int max_d, const char* d_refusal) {
    if (!c) return fail(-1, "null config");
    if (c->K_local <= 0 || c->N <= 0 || c->d <= 0) return fail(-1, "non-positive d / K / N");
    if (c->d > max_d) return fail(-2, d_refusal, c->d, max_d);
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
    if (c->control_kind == PSP_ISC_GRID) {
        if (!c->u_group || !c->u_row) return fail(-1, "control kind PSP_ISC_GRID needs u_group and u_row");
        if (c->u_ntables <= 0 || c->u_nrows <= 0 || c->u_ncols <= 0) return fail(-1, "u_ntables / u_nrows / u_ncols must be positive");
        if (!(c->u_dx > 0.f) || !(c->u_xb > 0.f)) return fail(-1, "u_xb / u_dx must be positive");
    }
    return 0;
}

// the kernel arguments both rollouts read from the config and the call
void is_fill_args(const psp_is_config* c, const float* xi, uint64_t seed, uint32_t iter, float* logw_out, float* XN_out, psp::IsArgs* a) {
    memset(a, 0, sizeof(*a));
    a->x0 = c->x0; a->xi = xi; a->drift = c->drift; a->sigma = c->sigma; a->runcost = c->runcost; a->term = c->term;
    a->uref = c->u_ref; a->ugroup = c->u_group; a->urow = c->u_row; a->logw = logw_out; a->XN = XN_out;
    a->k_offset = c->k_offset; a->K_global = c->K_global;
    a->d = c->d; a->K_local = c->K_local; a->N = c->N; a->ctrl = c->control_kind;
    a->drift_kind = c->drift_kind; a->sigma_kind = c->sigma_kind; a->runcost_kind = c->runcost_kind; a->term_kind = c->term_kind;
    a->noise_mode = c->noise_mode; a->dwell_form = c->dwell_form ? 1 : 0;
    a->u_ntables = c->u_ntables; a->u_nrows = c->u_nrows; a->u_ncols = c->u_ncols;
    a->dt = c->dt; a->sqdt = c->sqrt_dt; a->sigma_scale = c->sigma_scale; a->u_xb = c->u_xb; a->u_dx = c->u_dx; a->u_xhi = c->u_xhi;
    a->seed_lo = (uint32_t)seed; a->seed_hi = (uint32_t)(seed >> 32); a->iter = iter;
}

// ---- importance sampling under the reference control u* / no control (hjbe_kernels.h) -----------------------------------------
// every check of a psp_is_config, the LDS budget included (psp_is_query and psp_is_rollout share it)
int is_validate(const psp_is_config* c, int* lds_bytes) {
    if (const int rc = is_check_config(c, psp::kIsMaxD, "psp_is_rollout: d = %d is outside the native range d <= %d")) return rc;
    const long long ucells = c->control_kind == PSP_ISC_GRID ? (long long)c->u_ntables * c->u_ncols : 0;
    const char* too_big = "psp_is_rollout: the coefficient tables and the u* data of one step do not fit the 160 KiB LDS";
    if (ucells > kMaxLds / 4) return fail(-3, "%s", too_big);
    const psp::IsLds L = psp::is_lds_layout(psp::is_bucket(c->d), c->control_kind, c->drift_kind == PSP_DRIFT_DENSE,
                                            c->sigma_kind == PSP_SIGMA_DENSE, c->u_ntables, c->u_ncols);
    if ((long long)L.total * 4 > kMaxLds) return fail(-3, "%s", too_big);
    const long long total = L.total;
    *lds_bytes = (int)(total * 4);
    return 0;
}

// ---- the same rollout for wide states (hjbew_kernels.h) -------------------------------------------------------------------------
// every check of a psp_is_config for the wide kernel (psp_isw_query and psp_isw_rollout share it)
int isw_validate(const psp_is_config* c, psp_isw_sizes* out) {
    if (const int rc = is_check_config(c, PSP_ISW_MAX_D, "psp_isw_rollout: d = %d is outside the native range d <= %d (a wider tile "
                                                         "does not fit one wave's registers without scratch)")) return rc;
    const long long lds = c->control_kind == PSP_ISC_GRID ? 4LL * c->u_ntables * c->u_ncols : 0;
    if (lds > kMaxLds) return fail(-3, "psp_isw_rollout: the u* rows of one step do not fit the 160 KiB LDS");
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

extern "C" {

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
    is_fill_args(c, xi, seed, iter, logw_out, XN_out, &a);
    const long long grid = ((long long)c->K_local + psp::kIsThreads - 1) / psp::kIsThreads;
    hipError_t e = psp::is_rollout_launch(a, (int)grid, lds_bytes, (hipStream_t)stream);
    return hip_rc(e, "hjbe_rollout_kernel launch");
}

int psp_isw_query(const psp_is_config* c, psp_isw_sizes* sizes) {
    if (!sizes) return fail(-1, "null sizes passed to psp_isw_query");
    if (sizes->struct_bytes != (int32_t)sizeof(psp_isw_sizes))
        return fail(-1, "psp_isw_sizes.struct_bytes = %d, the library's struct has %d bytes", sizes->struct_bytes, (int)sizeof(psp_isw_sizes));
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
    is_fill_args(c, xi, seed, iter, logw_out, XN_out, &w.a);
    w.tab = tables;
    w.L = psp::isw_table_layout(c->d, c->N, c->control_kind, c->drift_kind == PSP_DRIFT_DENSE, c->sigma_kind == PSP_SIGMA_DENSE);
    hipError_t e = psp::isw_rollout_launch(w, s.workgroups, s.lds_bytes, (hipStream_t)stream);
    return hip_rc(e, "isw_rollout_kernel launch");
}

}  // extern "C"
