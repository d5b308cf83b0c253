// api_common.hip -- the single definitions behind api_common.h (error buffer, n_cus, the shared checks and small kernels) and the
// entry points of include/psp.h that belong to no kernel family: version and struct sizes, Adam and the iteration state, the
// Philox fill, the RCCL binding, the loss statistics.
#include <dlfcn.h>
#include <stdarg.h>

#include <rccl/rccl.h>   // types only: the entry points are bound with dlsym at first use (psp_comm_*)

#include "api_common.h"
#include "hjb_kernels.h"     // philox_block
#include "lstat_kernels.h"

namespace psp_api {

namespace {
thread_local char g_err[512] = "";
}  // namespace

int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}
int fail_hip(hipError_t e, const char* where) { return fail(-10, "%s: %s", where, hipGetErrorString(e)); }

unsigned long long* g_dbg = nullptr;   // psp_debug_set_stamp_buffer
long long g_dbg_n = 0;

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

int tile_waves(int ntile16, bool wide) {
    const int cus = n_cus(), cap = wide ? 4 : 8;
    const int fw = (ntile16 + cus - 1) / cus;
    return fw < 1 ? 1 : fw > cap ? cap : fw;
}

int check_ptrs(const psp_hjb_config* c) {
    if ((c->drift_kind != PSP_DRIFT_ZERO) && !c->drift) return fail(-1, "drift parameters missing");
    if (c->sigma_kind == PSP_SIGMA_DENSE && !c->sigma) return fail(-1, "sigma matrix missing");
    if (c->runcost_kind == PSP_RUNCOST_DIAG_QUAD && !c->runcost) return fail(-1, "running-cost vector missing");
    if (!c->term) return fail(-1, "terminal-cost vector missing");
    if (c->u_ref && !c->u_l2_out) return fail(-1, "u_ref set but u_l2_out is null");
    return 0;
}

int check_gh_par(int32_t h_kind, const float* h_par, int32_t d) {
    if (h_kind == PSP_GH_SINE_SOURCE) {
        if (h_par[0] != 0.f && h_par[0] != 1.f) return fail(-1, "PSP_GH_SINE_SOURCE: the sub-mode h_par[0] is 0 (Helmholtz) or 1 (Oscillations)");
        if (h_par[0] == 0.f && d < 2) return fail(-1, "PSP_GH_SINE_SOURCE: sub-mode 0 reads the coordinates x_0 and x_1 (d >= 2)");
    }
    return 0;
}

int check_gen_domain(const psp_gen_config& c) {
    if (c.domain_kind == PSP_DOM_SPHERE && !(c.dom_a > 0.f)) return fail(-1, "sphere radius must be positive");
    if (c.domain_kind == PSP_DOM_BOX && !(c.dom_a < c.dom_b)) return fail(-1, "box bounds must satisfy X_l < X_r");
    if (c.domain_kind == PSP_DOM_ANNULUS && !(c.dom_a >= 0.f && c.dom_a < c.dom_b)) return fail(-1, "annulus radii must satisfy 0 <= r_1 < r_2");
    return 0;
}

}  // namespace psp_api

using namespace psp_api;

namespace {
// ---- small kernels -------------------------------------------------------------------
__global__ void reduce_partials_kernel(const double* __restrict__ part, int n, double* __restrict__ out) {
    double sD = 0.0, sD2 = 0.0;
    block_pair_sum(part, n, &sD, &sD2);
    if (threadIdx.x == 0) { out[0] = sD; out[1] = sD2; }
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
}  // namespace

namespace psp_api {

int reduce_partials(const double* part, int n, double* out, void* stream) {
    return PSP_LAUNCH(reduce_partials_kernel, dim3(1), dim3(256), 0, stream, part, n, out);
}
int reduce_grad(const float* part, int nwg, int P, float* out, void* stream) {
    return PSP_LAUNCH(reduce_grad_kernel, dim3((P + 31) / 32), dim3(256), 0, stream, part, nwg, P, out);
}
int range_flag_partials(const double* part, int n, int* flag, void* stream) {
    return PSP_LAUNCH(range_flag_partials_kernel, dim3(1), dim3(256), 0, stream, part, n, flag);
}

}  // namespace psp_api

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

int psp_abi_struct_sizes4(int32_t out[2]) {
    if (!out) return fail(-1, "null output");
    out[0] = (int32_t)sizeof(psp_genl_eval_config); out[1] = (int32_t)sizeof(psp_genl_eval_sizes);
    return 0;
}

int psp_abi_struct_sizes5(int32_t out[2]) {
    if (!out) return fail(-1, "null output");
    out[0] = (int32_t)sizeof(psp_pinn_config); out[1] = (int32_t)sizeof(psp_pinn_sizes);
    return 0;
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

int psp_philox_normal_fill(float* out, int32_t N, int32_t K_local, int32_t d, int64_t k_offset,
                           uint64_t seed, uint32_t iter, void* stream) {
    if (!out || N <= 0 || K_local <= 0 || d <= 0) return fail(-1, "bad arguments to psp_philox_normal_fill");
    const long long n0 = (long long)K_local * d;
    if (const int rc = PSP_LAUNCH(zero_kernel, dim3((unsigned)((n0 + 255) / 256)), dim3(256), 0, stream, out, n0)) return rc;
    const long long total = (long long)N * K_local * (((d + 15) / 16) * 4);
    return PSP_LAUNCH(philox_fill_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, out, N, K_local, d,
                      (long long)k_offset, (uint32_t)seed, (uint32_t)(seed >> 32), iter);
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
    return fail(-21, "%s: %s", where, g_rccl.GetErrorString ? g_rccl.GetErrorString(e) : "RCCL error");
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
