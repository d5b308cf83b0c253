// genl_kernels.h -- GeneralSolver / EllipticSolver rollout for value nets of ANY depth: V = dense-concat net (d [+ 1] -> 1,
// arch = [H_1 .. H_L]), 1 <= L <= 4 hidden layers of up to 128 units (reference function_space.py:116-140 DenseNet: layer i sees
// the concatenation of the input and of all earlier hidden outputs, activation relu^2; :143-158 DenseNet_tanh: tanh, nn.Linear
// weights; `Committor function.ipynb` cell 1: tanh^2).  The (d, H)-templated kernels of gen_kernels.h keep their tables in LDS
// and their activations in registers, which fixes them to two hidden layers of at most 64; the nets the reference's
// diffusion-loss notebooks actually train are deeper and wider (Allen-Cahn.ipynb:72: arch = [110, 110, 50] at d = 100;
// Committor function.ipynb: [d + 10, d, d, d] with tanh^2).  This family takes shapes and activation at RUN time:
//   * activations live in per-tile LDS images in T layout (k-step image: element (ks, lane = j + 16 q) = feature 4 ks + q of
//     sample j, hjb_kernels.h), every segment of the dense concatenation padded to whole 16-feature blocks;
//   * weights live in global memory (L2-resident: <= 1 MB) as pre-permuted A-operand tables built per call by
//     genl_tables_kernel, forward orientation (out^T = W^T in^T) and reverse orientation (g_in = W g_out) per layer;
//   * every product is a rolled, register-double-buffered loop of v_mfma_f32_16x16x4_f32 over the k-steps of the input image
//     (tables are k-quad-major: one 16-byte load per lane straight from L2 feeds four MFMAs per image).
// NW waves share a 16-trajectory tile (NW = 8: products cut by OUTPUT block, the hidden block hb of the concatenation belongs to
// wave hb % NW, which keeps that block's r = relu(z) / tanh(z) and tangent z' in REGISTERS -- the LDS holds only what a product
// reads as its B operand; NW = 1 for small nets: no barriers at all, many tiles per CU).
//   genl_fwd_kernel   per step: V(X, t), grad_x V by the reverse sweep, masked Euler-Maruyama step, Y update (h sees V(X, t) and
//                     the state BEFORE the move; exit tests of the bounded domains; solver.py:1091-1160 / :730-790) -- the same
//                     step as gen_fwd_kernel; keeps per sample only (x, t), the tangent direction s u^ and the coefficient a^.
//                     A tile whose trajectories have all stopped leaves the time loop (solver.py:1093-1097 / :742-744; the
//                     committor notebook runs N = 5000 with exits after 500 .. 1600 steps) and records its step count.
//   genl_bwd_kernel   per sample block, in parallel over all executed (n, tile): recomputes the activations and their tangent
//                     along s u^, runs the adjoint sweep of  a V + w d/d(s u^) V,  and accumulates EVERY parameter gradient in
//                     registers: the weight tiles dW_i (16 inputs x 16 units) as MFMA outer products over the 16 samples of the
//                     block straight from the LDS images (feature-on-lane reads), biases and the output layer as lane sums.
//                     Per-workgroup partial gradients, summed in a fixed order by reduce_grad_kernel.
// Derivation (per sample; a_0 = [x, t], z_i = W_i^T a_{i-1} + b_i, r_i = relu(z_i) | tanh(z_i), h_i = phi(r_i), a_i = [a_{i-1}, h_i],
// V = w^T a_L + b;  phi(r) = r^2 (relu^2, tanh^2) or r (tanh);  phi1 = dh/dz, phi2 = d^2h/dz^2 as functions of r):
//   tangent along u:  a_0' = [u, 0], z_i' = W_i^T a_{i-1}', h_i' = phi1(r_i) z_i', V' = w^T a_L'
//   adjoint of S = a V + w V':  abar_L = a w, abar_L' = w w;  for i = L..1:
//       zbar_i' = abar_h' phi1(r_i),   zbar_i = abar_h phi1(r_i) + abar_h' phi2(r_i) z_i',
//       abar_{i-1} = abar_a + W_i zbar_i,  abar_{i-1}' = abar_a' + W_i zbar_i';
//   dW_i = a_{i-1} zbar_i^T + a_{i-1}' zbar_i'^T, db_i = zbar_i, dw = a a_L + w a_L', db = a.
// Dense constant sigma(x) = B (genl_fwd_kernel<NW, true>; `Nonlinear toy problem - elliptic with full Hessian.ipynb`:
// B = sqrt(2 / d) ones(d, d)).  With g = grad_x V the step (solver.py:725-774 / :1100-1149) is
//   Z = B^T g,   w = xi sqrt(dt) + c dt  (c = -Z detached, or 0),   X += (b(X) dt + B w) alive,
//   Y += ((-h + Z . c) dt + Z . xi sqrt(dt)) act,   u = w (+ dt Z for h = -|z|^2 / 2),   U = act B u.
// Every parameter dependence of Y_N goes through V: through  Z . (xi sqrt(dt) + c dt) = grad V . B w  (c detached) and, for the
// quadratic h, through |Z|^2 / 2 = |B^T grad V|^2 / 2, whose derivative is (B Z) . d(grad V).  So dY_N / dtheta is the sum over the
// active steps of  a^ dV/dtheta + d/dtheta (grad V . U)  with the stored direction U = act B u -- the backward kernel consumes
// (x, t), U and a^ and nothing else: it is the one of sigma = s I, where U = act s u is the special case B = s I.
// The two products per step (three with the quadratic h: B w and B u share the table operands) have the shape of the layer
// products -- A operand = a k-quad-major table of B^T resp. B built by genl_tables_kernel next to the weight tables, B operand =
// a T-layout LDS image -- and run through genl_gemm1 / genl_gemm1x2; their output blocks are dealt over the tile's waves
// (block ob -> wave ob mod NW, as in the reverse sweep) and exchanged through the images.
// Linear-quadratic coefficients (genl_fwd_kernel<NW, true, true>; Solver's value-function ansatz on LLGC / LQGC, reference
// solver.py:334-339, 471-478, problems.py:14-65, 118-175): the ansatz takes Z = B grad_x V -- the OTHER orientation --, the drift
// is b(x) = A x with a dense A, and h carries the running cost f(x) = sum_i p_i x_i^2 at the state AFTER the move:
//   Z = B g (table tSB),   w = xi sqrt(dt) + c dt,   X += ((dt A) X + B w) alive,
//   Y += ((|Z|^2 / 2 + f(X_{n+1}) + Z . c) dt + Z . xi sqrt(dt)) act,   u = w (+ dt Z),   U = act B^T u.
// Z . w = g . B^T w and d(|Z|^2 / 2) = (B^T Z) . dg, so dY_N / dtheta is again the sum of  a^ dV/dtheta + d/dtheta (g . U): the same
// backward kernel.  f does not depend on theta while the state path is detached, so a^ is untouched.  (dt A) X is one more product
// of the same shape -- A operand: a table of dt A built next to tSB (rows and columns >= d zero: the time row never enters),
// B operand: the X image in A -- accumulated into the accumulator of B w, so the boxes' proposal test sees it and no image is added.
// B w and B^T u read different tables: three sigma products and the drift product per step.
// u_L2 log (genl_fwd_kernel<NW, false, false, true> and <NW, true, true, true>; Solver's value-function ansatz with
// u_l2_error_flag, reference solver.py:471-475, 491-494): per trajectory  sum_n |-Z_n - u*(X_{n+1}, n dt)|^2 dt  with the Z of the Y
// update and u* at the state AFTER the move, for the three descriptions of u* of include/psp.h PSP_UL2_*: a table of u*(t_n); the
// gains M_n of a u* linear in x -- one more d x d product per step, A operand = a per-step table of M_n staged ONCE per plan by
// genl_ul2_stage_kernel behind everything genl_tables_kernel rewrites, B operand = the image of the moved state (the input blocks
// of A are dead by then; columns >= d of the table are zero: the time row never enters); the double wells' grid tables with the cell
// arithmetic of ugrid.h.  On the dense path the Z image takes B^T u before the move, so the kinds that need X_{n+1} keep Z in an
// image of its own (ZLi, one more carve of DB0 blocks).  The sum is sequential in n, fp32, formed by every wave alike (as S and Pz
// are) and written by one lane per trajectory.  Defined for runs that never stop (no domain, T = inf): every step is active.
// Eigenvalue problems (genl_fwd_kernel<NW, false, false, false, true>; the three `Eigenvalue - *.ipynb` notebooks of the
// diffusion-loss paper: an eigenpair (lambda, V) of the generator on the periodic box, sigma = s I, state path detached):
//   Y += ((-h(X, V, Z) - lambda V) dt + Z . xi sqrt(dt)) act,   V = relu(o) for a net with linear output o (out_relu),
// lambda read from DEVICE memory once per launch (it is trained: no host read per iteration).  With the gate c = 1[o > 0]:
// V = c o, grad V = c grad o, dV/dtheta = c do/dtheta, so the forward stores the gated tangent direction c U and the gated
// coefficient c a^ with a^ = [n = 0] - (h_y + lambda) dt act -- genl_bwd_kernel consumes exactly those, unchanged (the caller gates
// the weight of V(X_N) by 1[V(X_N) > 0] itself).  One more output, S_k = sum_n act_n V(X_n) dt = -dY_N / dlambda.  Two h kinds and a
// drift kind that need row reductions of cos x / sin x (GH_EIG_FP + DRIFT_EIG_FP, GH_EIG_NLS) live in these instances only.
#pragma once
#include "gen_kernels.h"
#include "ugrid.h"

namespace psp {

constexpr int GENL_MAXL = 4;        // hidden layers
constexpr int GENL_MAXDB = 7;       // input blocks (d + 1 <= 112)
constexpr int GENL_MAXHB = 8;       // hidden blocks per layer (H <= 128)
enum { GACT_RELU2 = 0, GACT_TANH2 = 1, GACT_TANH = 2 };
// The eigenvalue problems (EIG instances of the forward kernel only; numbered away from the kinds above):
//   GH_EIG_FP   h = y (-sin(S) sum_i c_i^2 sin^2 x_i - cos(S) S),  S = sum_j c_j cos x_j, c = the drift vector (Fokker-Planck)
//   GH_EIG_NLS  h = -y^3 - y (-p0 exp((2 / d) sum_i cos x_i) + sum_i (sin^2 x_i / d^2 - cos x_i / d) - 3),  h_par = (1 / c^2, d, -, -)
//   DRIFT_EIG_FP  b_i = -cos(S) c_i sin x_i
constexpr int GH_EIG_FP = 16, GH_EIG_NLS = 17, DRIFT_EIG_FP = 16;
// GH_SINNORM2 (problems.py:1721-1724; the dense-sigma instances again: they form sx = sum_i x_i), h_par = (al, d, linear, -)
__device__ inline void gh_sinnorm2(const float* p, float y, float rr, float sx, float& minus_h, float& hy) {
    const float pi = 3.14159265358979323846f, a2 = p[0] * p[0], fp2 = 4.0f * (pi * pi), s = sinf(pi * rr);
    const float cs = ((2.0f * p[1]) * pi) * cosf(pi * rr);
    if (p[2] != 0.f) {
        minus_h = -(a2 * ((fp2 * s) * (sx * sx) - cs));
        hy = 0.f;
    } else {
        minus_h = -(a2 * (((((fp2 * y) * (sx * sx)) - cs) + s * s) - y * y));
        hy = a2 * (fp2 * (sx * sx) - 2.0f * y);
    }
}

// per-NW register-array bounds: hidden blocks per wave (HBsum <= 32; NW = 1 only for HBsum <= 8), concatenation blocks per wave
// (TB <= 39; NW = 1 only for TB <= 16)
template <int NW> struct GenlGeo {
    static constexpr int MAXSLOT = (NW == 1) ? 8 : (32 + NW - 1) / NW;
    // weight-gradient tiles per wave and launch group = accumulator quads of the backward kernel: eight waves of 32 hold the 256
    // tiles of the Allen-Cahn notebook net
    static constexpr int MAXT = 32;
};

struct GenlArgs {
    GenArgs g;                      // problem, noise, outputs, weights: same meaning as in gen_kernels.h
    const float* tables;            // table region (built by genl_tables_kernel)
    float* tables_w;                // same pointer, writable (tables kernel)
    int d, D0, has_time, L;
    int H[GENL_MAXL], HB[GENL_MAXL];
    int off[GENL_MAXL + 1];         // block offset of segment s in the padded concatenation (s = 0: the input); off[L] + HB[L-1] = TB
    int roff[GENL_MAXL + 1];        // real feature offset of segment s in a_L
    int inw[GENL_MAXL + 1];         // real input width of layer i (i = L: the output layer)
    int oW[GENL_MAXL + 1], ob[GENL_MAXL + 1];   // flat parameter offsets: W_i, b_i; index L: the output layer (in_L x 1), b
    int TB, DB0;
    long long tF[GENL_MAXL], tR[GENL_MAXL];      // float offsets of the forward / reverse tables
    long long vB[GENL_MAXL], vW;                 // float offsets of the staged bias vectors / output-layer vector
    int HBsum;                      // sum of HB[i]
    int act;                        // GACT_*
    int linear_layout;              // 1: weights stored (out, in) (nn.Linear: DenseNet_tanh) instead of (in, out)
    int* nexec;                     // (ntile16) time steps the tile executed before all of its trajectories had stopped
    // backward
    float* gpart;                   // (gridDim.x, P) partial gradients
    int n_tiles;                    // weight-gradient tiles: sum_i off[i + 1] * HB[i]
    int tcum[GENL_MAXL + 1];        // tiles of the layers below i
    long long P;
    long long table_floats;         // size of the table region -- no kernel reads it, but dropping it moves the fields below and
                                    // with them the backward kernels' register allocation
    int time_first;                 // 1: the net's input is [t, x] (Solver's value-function ansatz, solver.py:338) -- the kernels keep the
                                    // time in their LAST input row; only the parameter index map differs
    float time_scale;               // the net sees time_scale * t (value-function ansatz: the step index n = t / dt, solver.py:336, 439)
    // dense constant sigma (appended: every field above keeps its offset)
    int dense;                      // 1: genl_fwd_kernel<NW, true> runs; the tables of B and B^T are built
    const float* sigmaB;            // B (d x d row-major); NULL with dense = 1: B = g.sigma_scale I
    long long tSB, tSBT;            // float offsets of the A-operand tables of B (for B w, B u) and of B^T (for B^T grad V)
    // linear-quadratic coefficients (appended; lq = 1: genl_fwd_kernel<NW, true, true> runs)
    int lq;
    int z_sigma;                    // 1: Z = B grad_x V and U = act B^T u (Solver's value-function ansatz) instead of Z = B^T grad_x V, U = act B u
    int runcost_kind;               // 1: f(x) = sum_i runcost[i] x_i^2 enters h at the state after the move (h_kind = GH_QUAD only)
    const float* driftA;            // A (d x d row-major): b(x) = A x; NULL: g.drift_kind
    const float* runcost;           // p (d)
    long long tA;                   // float offset of the A-operand table of dt A
};
// u_L2 log: the arguments of the LOGU instances travel BEHIND GenlArgs in an argument struct of their own, so that GenlArgs, the
// kernels that take it and the offsets of their hidden arguments stay what they were
struct GenlUl2Args {
    int kind;                       // PSP_UL2_TABLE / LINEAR / GRID
    int ntables, nrows, ncols;      // GRID
    float* out;                     // (K_local)
    const float* ref;               // TABLE: (N, d) u*(t_n); GRID: (G, nrows, ncols) tables; LINEAR: (N, d, d) gains (stage kernel only)
    const int* group;               // GRID: (d) table of every coordinate
    const int* row;                 // GRID: (N) table row of step n
    float xb, dx, xhi;              // GRID: cell = floor((clamp(x, -xb, xhi) + xb) / dx) (ugrid.h)
    int reserved;
    long long Kglobal;              // GRID: the globally last trajectory's cell is lowered by two
    long long tUL;                  // LINEAR: float offset of the N A-operand tables of M_n (layout of tSB), behind tA
};
struct GenlLogArgs { GenlArgs a; GenlUl2Args u; };
// eigenvalue problems: the arguments of the EIG instances travel BEHIND GenlArgs as well
struct GenlEigArgs {
    const float* lam;               // DEVICE scalar lambda, read once per launch; NULL: 0
    float* S_out;                   // (K_local) sum_n act_n V(X_n) dt, or NULL
    int out_relu;                   // 1: V = relu(net output)
    int reserved;
};
struct GenlEigFwdArgs { GenlArgs a; GenlEigArgs e; };
enum { GUL2_TABLE = 0, GUL2_LINEAR = 1, GUL2_GRID = 2 };      // = PSP_UL2_*

// padded feature index -> real index inside the concatenation a (or -1: padding)
// (AP: pointer to the arguments -- a generic one in the tables kernel, the kernel-argument segment in the rollout kernels)
template <class AP>
__device__ __forceinline__ int genl_real_feature(AP a, int pf) {
    const int pb = pf >> 4;
    int s = 0;
#pragma unroll
    for (int i = 1; i <= GENL_MAXL; ++i) if (i <= a->L && pb >= a->off[i]) s = i;
    const int c = pf - 16 * a->off[s];
    const int width = (s == 0) ? a->D0 : a->H[s - 1];
    if (c >= width) return -1;
    if (s == 0 && a->time_first) return c == a->d ? 0 : c + 1;       // kernel rows [x, t] <-> parameter rows [t, x]
    return a->roff[s] + c;
}
// weight multiplier of a padded input feature: the time row carries time_scale (tables and gradients alike)
template <class AP>
__device__ __forceinline__ float genl_feature_scale(AP a, int pf) {
    return (a->has_time && a->time_scale != 1.0f && pf == a->d) ? a->time_scale : 1.0f;
}
// flat parameter index of W_i[input feature rf][unit u] (i = L: the output layer, u = 0)
template <class AP>
__device__ __forceinline__ int genl_w_index(AP a, int i, int rf, int u) {
    const int Hi = (i < a->L) ? a->H[i] : 1;
    return a->oW[i] + (a->linear_layout ? u * a->inw[i] + rf : rf * Hi + u);
}

// A-operand tables + staged vectors from the flat parameters (registration order W_1, b_1, .., W_out, b_out)
// (an ordinary kernel: defined in the one translation unit that launches it, api_genl.hip; a unit that includes this header for
//  its device helpers alone defines PSP_GENL_DEVICE_HELPERS_ONLY)
#ifndef PSP_GENL_DEVICE_HELPERS_ONLY
__global__ __launch_bounds__(256) void genl_tables_kernel(const GenlArgs a) {
    PSP_COND_EXIT(a.g);
    const float* __restrict__ P = a.g.params;
    float* T = a.tables_w;
    const long long gtid = (long long)blockIdx.x * blockDim.x + threadIdx.x, gn = (long long)gridDim.x * blockDim.x;
    for (int i = 0; i < a.L; ++i) {
        const int Hi = a.H[i], HBi = a.HB[i];
        const int inb = a.off[i + 1];                                   // input blocks of layer i
        const int KSin = 4 * inb, KSh = 4 * HBi;
        // forward: [mb][ks / 4][lane][ks & 3] (one 16-byte load per lane = the A operands of four consecutive k-steps),
        // row = 16 mb + rowmap(lane & 15) (an output unit), k = 4 ks + q (a padded input feature)
        for (long long idx = gtid; idx < (long long)HBi * KSin * 64; idx += gn) {
            const int lane = (int)((idx >> 2) & 63);
            const long long t = idx >> 8;                           // (mb, ks / 4)
            const int ks = 4 * (int)(t % (KSin / 4)) + (int)(idx & 3), mb = (int)(t / (KSin / 4));
            const int ii = lane & 15, q = lane >> 4;
            const int row = 16 * mb + 4 * (ii & 3) + (ii >> 2);
            const int rf = genl_real_feature(&a, 4 * ks + q);
            T[a.tF[i] + idx] = (row < Hi && rf >= 0) ? genl_feature_scale(&a, 4 * ks + q) * P[genl_w_index(&a, i, rf, row)] : 0.f;
        }
        // reverse: [ob][ks / 4][lane][ks & 3], row = 16 ob + rowmap (a padded input feature), k = 4 ks + q (an output unit)
        for (long long idx = gtid; idx < (long long)inb * KSh * 64; idx += gn) {
            const int lane = (int)((idx >> 2) & 63);
            const long long t = idx >> 8;
            const int ks = 4 * (int)(t % (KSh / 4)) + (int)(idx & 3), ob = (int)(t / (KSh / 4));
            const int ii = lane & 15, q = lane >> 4;
            const int pfr = 16 * ob + 4 * (ii & 3) + (ii >> 2);
            const int rf = genl_real_feature(&a, pfr);
            const int col = 4 * ks + q;
            T[a.tR[i] + idx] = (col < Hi && rf >= 0) ? genl_feature_scale(&a, pfr) * P[genl_w_index(&a, i, rf, col)] : 0.f;
        }
        // bias in T-layout vector staging: [(b * 4 + q) * 4 + r] <- v(16 b + 4 r + q)
        for (long long idx = gtid; idx < (long long)HBi * 16; idx += gn) {
            const int r = (int)(idx & 3), q = (int)((idx >> 2) & 3), b = (int)(idx >> 4);
            const int f = 16 * b + 4 * r + q;
            T[a.vB[i] + idx] = f < Hi ? P[a.ob[i] + f] : 0.f;
        }
    }
    if (a.dense) {
        // sigma = B as A-operand tables in the forward layout above, DB0 x DB0 blocks: tSB holds M = B (out = B in), tSBT holds
        // M = B^T (Z = B^T grad_x V, solver.py:729 / :1104); rows and columns >= d are zero, so the time input, the padding and
        // dV/dt never enter.  (The value-function ansatz of Solver takes Z = sigma grad Y, solver.py:330: the other table.)
        const int DBs = a.DB0, KSs = 4 * DBs, d = a.d;
        for (long long idx = gtid; idx < (long long)DBs * KSs * 64; idx += gn) {
            const int lane = (int)((idx >> 2) & 63);
            const long long t = idx >> 8;                           // (mb, ks / 4)
            const int ks = 4 * (int)(t % (KSs / 4)) + (int)(idx & 3), mb = (int)(t / (KSs / 4));
            const int ii = lane & 15, q = lane >> 4;
            const int row = 16 * mb + 4 * (ii & 3) + (ii >> 2), col = 4 * ks + q;
            const bool in = row < d && col < d;
            float m = 0.f, mt = 0.f;
            if (in && a.sigmaB) { m = a.sigmaB[(size_t)row * d + col]; mt = a.sigmaB[(size_t)col * d + row]; }
            else if (in && row == col) m = mt = a.g.sigma_scale;
            T[a.tSB + idx] = m;
            T[a.tSBT + idx] = mt;
            if (a.driftA) T[a.tA + idx] = in ? a.g.dt * a.driftA[(size_t)row * d + col] : 0.f;     // (dt A) X: same layout as B
        }
    }
    for (long long idx = gtid; idx < (long long)a.TB * 16; idx += gn) {       // output layer over the padded concatenation
        const int r = (int)(idx & 3), q = (int)((idx >> 2) & 3), b = (int)(idx >> 4);
        const int rf = genl_real_feature(&a, 16 * b + 4 * r + q);
        T[a.vW + idx] = rf >= 0 ? genl_feature_scale(&a, 16 * b + 4 * r + q) * P[a.oW[a.L] + rf] : 0.f;
    }
}
#endif

typedef const GenlArgs* KArgs;
typedef const GenArgs* KGen;
// argument struct of genl_fwd_kernel<.., LOGU> and its GenlArgs part
template <bool LOGU, bool EIG = false> struct GenlFwdArgsOf { typedef GenlArgs type; };
template <> struct GenlFwdArgsOf<true, false> { typedef GenlLogArgs type; };
template <> struct GenlFwdArgsOf<false, true> { typedef GenlEigFwdArgs type; };
__device__ __forceinline__ KArgs genl_base(const GenlArgs* p) { return p; }
__device__ __forceinline__ KArgs genl_base(const GenlLogArgs* p) { return &p->a; }
__device__ __forceinline__ KArgs genl_base(const GenlEigFwdArgs* p) { return &p->a; }

// ---- activation as functions of the stored r (relu(z) or tanh(z)); `act` is a kernel argument: uniform branches
__device__ __forceinline__ f32x4 gact_r(int act, f32x4 z) { return act == GACT_RELU2 ? relu4(z) : tanh4(z); }
__device__ __forceinline__ f32x4 gact_h(int act, f32x4 r) { return act == GACT_TANH ? r : r * r; }
__device__ __forceinline__ f32x4 gact_h1(int act, f32x4 r) {
    if (act == GACT_RELU2) return 2.0f * r;
    const f32x4 s = 1.0f - r * r;
    return act == GACT_TANH ? s : (2.0f * r) * s;
}
__device__ __forceinline__ f32x4 gact_h2(int act, f32x4 r) {
    if (act == GACT_RELU2) return step2(r);
    const f32x4 s = 1.0f - r * r;
    return act == GACT_TANH ? (-2.0f * r) * s : (2.0f * s) * (1.0f - 3.0f * (r * r));
}

// acc += Table . image over KS k-steps (KS a multiple of 4: whole 16-feature blocks) for ONE output block.  One 16-byte table
// load per lane feeds four MFMAs; the loads run a whole chunk of GENL_U quads ahead of the MFMAs that consume them (two register
// buffers): the products are fed from L2 (latency ~1 us), and a chunk of eight quads is 32 (64 with two images) MFMAs deep.
template <int GENL_U>
__device__ __forceinline__ void genl_gemm1(f32x4& acc, const float* __restrict__ tbl, int KS, const float* img, int lane) {
    const f32x4* t0 = reinterpret_cast<const f32x4*>(tbl) + lane;
    const int n4 = KS / 4;
    f32x4 cur[GENL_U], nxt[GENL_U];
#pragma unroll
    for (int u = 0; u < GENL_U; ++u) { cur[u] = f32x4{0.f, 0.f, 0.f, 0.f}; if (u < n4) cur[u] = t0[(size_t)u * 64]; }
    for (int base = 0; base < n4; base += GENL_U) {
#pragma unroll
        for (int u = 0; u < GENL_U; ++u) { const int k4 = base + GENL_U + u; nxt[u] = cur[u]; if (k4 < n4) nxt[u] = t0[(size_t)k4 * 64]; }
#pragma unroll
        for (int u = 0; u < GENL_U; ++u)
            if (base + u < n4) {
#pragma unroll
                for (int r = 0; r < 4; ++r) acc = mfma16(cur[u][r], img[(4 * (base + u) + r) * 64 + lane], acc);
            }
#pragma unroll
        for (int u = 0; u < GENL_U; ++u) cur[u] = nxt[u];
    }
}
// the same with two images sharing the table operands (value and tangent passes, adjoint and tangent-adjoint passes)
template <int GENL_U>
__device__ __forceinline__ void genl_gemm1x2(f32x4& acc, f32x4& acd, const float* __restrict__ tbl, int KS, const float* img,
                                             const float* imgd, int lane) {
    const f32x4* t0 = reinterpret_cast<const f32x4*>(tbl) + lane;
    const int n4 = KS / 4;
    f32x4 cur[GENL_U], nxt[GENL_U];
#pragma unroll
    for (int u = 0; u < GENL_U; ++u) { cur[u] = f32x4{0.f, 0.f, 0.f, 0.f}; if (u < n4) cur[u] = t0[(size_t)u * 64]; }
    for (int base = 0; base < n4; base += GENL_U) {
#pragma unroll
        for (int u = 0; u < GENL_U; ++u) { const int k4 = base + GENL_U + u; nxt[u] = cur[u]; if (k4 < n4) nxt[u] = t0[(size_t)k4 * 64]; }
#pragma unroll
        for (int u = 0; u < GENL_U; ++u)
            if (base + u < n4) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int o = (4 * (base + u) + r) * 64 + lane;
                    acc = mfma16(cur[u][r], img[o], acc);
                    acd = mfma16(cur[u][r], imgd[o], acd);
                }
            }
#pragma unroll
        for (int u = 0; u < GENL_U; ++u) cur[u] = nxt[u];
    }
}
__device__ __forceinline__ void img_put(float* img, int blk, const f32x4& v, int lane) {     // T-layout block -> k-steps 4 blk .. 4 blk + 3
    float* p = img + blk * 256 + lane;
    p[0] = v[0]; p[64] = v[1]; p[128] = v[2]; p[192] = v[3];
}
__device__ __forceinline__ f32x4 img_get(const float* img, int blk, int lane) {
    const float* p = img + blk * 256 + lane;
    f32x4 v;
    v[0] = p[0]; v[1] = p[64]; v[2] = p[128]; v[3] = p[192];
    return v;
}
__device__ __forceinline__ f32x4 vec_get(const float* __restrict__ vec, int blk, int q) {   // staged vector: [(b * 4 + q) * 4 + r]
    return *reinterpret_cast<const f32x4*>(vec + (blk * 4 + q) * 4);
}
// the tile's waves share the LDS images; one wave per tile needs no barrier (its LDS accesses are ordered)
template <int NW> __device__ __forceinline__ void tile_sync() { if constexpr (NW > 1) __syncthreads(); }

// layer index of hidden block hb (hidden blocks counted over the layers: hb = off[i + 1] - DB0 + mb) -- uniform
__device__ __forceinline__ int genl_layer_of(KArgs a, int hb) {
    int i = 0;
#pragma unroll
    for (int l = 1; l < GENL_MAXL; ++l) if (l < a->L && hb >= a->off[l + 1] - a->DB0) i = l;
    return i;
}

// ---- value net at the point held in image A (blocks 0 .. DB0 - 1 filled): fills the hidden segments of A (h_i); the wave keeps
// r_i of ITS hidden blocks in Rr (slot s <-> hidden block wave + NW s); returns V.  Padded rows / features carry zero weights
// and biases, so they stay exactly zero.
template <int NW>
__device__ __forceinline__ float genl_value(KArgs a, const float* __restrict__ T, float* A, f32x4 (&Rr)[GenlGeo<NW>::MAXSLOT], int lane, int q, int wave) {
    for (int i = 0; i < a->L; ++i) {
        const int HBi = a->HB[i];
        const int seg = a->off[i + 1];                                // first block of this layer's output segment = its input blocks
        const int KSin = 4 * seg, hoff = seg - a->DB0;
#pragma unroll
        for (int s = 0; s < GenlGeo<NW>::MAXSLOT; ++s) {
            const int mb = wave + NW * s - hoff;
            if (mb >= 0 && mb < HBi) {
                f32x4 acc = vec_get(T + a->vB[i], mb, q);
                genl_gemm1<8>(acc, T + a->tF[i] + (size_t)mb * KSin * 64, KSin, A, lane);
                const f32x4 r = gact_r(a->act, acc);
                Rr[s] = r;
                img_put(A, seg + mb, gact_h(a->act, r), lane);
            }
        }
        tile_sync<NW>();                                             // the next layer reads what this one wrote
    }
    float v = 0.f;                                                   // (every wave forms the same sum)
    for (int b = 0; b < a->TB; ++b) v = dot4(vec_get(T + a->vW, b, q), img_get(A, b, lane), v);
    return qsum(v) + a->g.params[a->ob[a->L]];
}

// ---- grad of V w.r.t. the input segment by the reverse sweep: G (TB blocks) <- w; for i = L..1: G_h *= phi1(r) in place (= gz),
// G[0 .. seg) += W_i gz.  On return blocks 0 .. DB0 - 1 of G hold grad_{[x, t]} V.
template <int NW>
__device__ __forceinline__ void genl_input_gradient(KArgs a, const float* __restrict__ T, const f32x4 (&Rr)[GenlGeo<NW>::MAXSLOT], float* G,
                                                    int lane, int q, int wave) {
    for (int b = wave; b < a->TB; b += NW) img_put(G, b, vec_get(T + a->vW, b, q), lane);
    tile_sync<NW>();
    for (int i = a->L - 1; i >= 0; --i) {
        const int seg = a->off[i + 1];                                // first block of h_i; also the number of input blocks of layer i
        const int HBi = a->HB[i], KSh = 4 * HBi, hoff = seg - a->DB0;
#pragma unroll
        for (int s = 0; s < GenlGeo<NW>::MAXSLOT; ++s) {
            const int mb = wave + NW * s - hoff;
            if (mb >= 0 && mb < HBi) img_put(G, seg + mb, img_get(G, seg + mb, lane) * gact_h1(a->act, Rr[s]), lane);
        }
        tile_sync<NW>();
        for (int ob = wave; ob < seg; ob += NW) {
            f32x4 acc = img_get(G, ob, lane);
            genl_gemm1<8>(acc, T + a->tR[i] + (size_t)ob * KSh * 64, KSh, G + seg * 256, lane);
            img_put(G, ob, acc, lane);
        }
        tile_sync<NW>();
    }
}

// LDS: A, G (TB blocks each), 1 KiB per block
__host__ __device__ inline int genl_fwd_lds_bytes(int TB) { return 2 * TB * 1024; }
// dense sigma: three more images of DB0 blocks (Z then B u; w; u) behind the input blocks of G.  The hidden blocks of G hold dead
// scratch once the input gradient is formed; where they are fewer than 3 DB0 the carve grows past G
__host__ __device__ inline int genl_fwd_lds_bytes_dense(int TB, int DB0) { return (2 * TB > TB + 4 * DB0 ? 2 * TB : TB + 4 * DB0) * 1024; }
// u_L2 log of the kinds that read X_{n+1} (LINEAR, GRID) on the dense path: one more image (-> ZLi) behind those three
__host__ __device__ inline int genl_fwd_lds_bytes_dense_log(int TB, int DB0) { return (2 * TB > TB + 5 * DB0 ? 2 * TB : TB + 5 * DB0) * 1024; }

// (NW = 4: two workgroups per CU at 256 registers a wave -- the step chain of a tile is bound by the L2 latency of its table
//  operands and by its barriers, not by the matrix pipe, so two tiles in flight per CU are worth more than eight waves on one
//  once the batch fills the chip; NW = 8 for small batches, where the latency of ONE tile is what counts)
// (Tried and dropped: the whole table region copied into LDS by the one-wave instances of small nets.  On the committor notebook's
//  net -- 29 KB of tables -- it shortened the step chain of a K = 200 batch by 6 % (12.1 -> 11.3 ms: the chain is bound by its
//  instruction count, not by the L2 latency of the tables) and cost a batch that fills the chip 75 % (72.7 -> 127 ms at K = 65536:
//  three workgroups per CU instead of twelve, and every workgroup copies the tables).)
// DENSE: sigma = B through the tables tSB / tSBT (header comment); a template parameter, so that the instances of sigma = s I
// stay the code they were.  LQ (with DENSE only): the linear-quadratic coefficients of the header comment, as uniform run-time
// branches inside instances of their own -- for the same reason.  LOGU: the u_L2 log of the header comment, the kind a uniform
// run-time branch; instantiated as <NW, false, false, true> (TABLE, GRID) and <NW, true, true, true> (all three kinds)
// EIG: the eigenvalue problems of the header comment (lambda, the output ReLU's gate, S_k, their h / drift kinds), sigma = s I
// only; every line of it sits behind `if constexpr (EIG)`, so the other instances stay the code they were
template <int NW, bool DENSE = false, bool LQ = false, bool LOGU = false, bool EIG = false>
__global__ __launch_bounds__(64 * NW, NW == 1 ? 1 : 2) void genl_fwd_kernel(const typename GenlFwdArgsOf<LOGU, EIG>::type ga_) {
    static_assert(DENSE || !LQ, "the linear-quadratic coefficients run on the dense-sigma path");
    static_assert(!LOGU || DENSE == LQ, "the u_L2 log: the sigma = s I instance or the linear-quadratic one");
    static_assert(!EIG || (!DENSE && !LQ && !LOGU), "the eigenvalue problems run on the sigma = s I path");
    if constexpr (LOGU || EIG) { PSP_COND_EXIT(ga_.a.g); } else { PSP_COND_EXIT(ga_.g); }
    const KArgs ga = genl_base(&ga_);
    const KGen a = &ga->g;
    [[maybe_unused]] const GenlEigArgs* eg = nullptr;
    [[maybe_unused]] float lam = 0.f, Slam = 0.f;                    // EIG: lambda; S_k = sum_n act_n V(X_n) dt
    if constexpr (EIG) { eg = &ga_.e; if (eg->lam) lam = *eg->lam; }
    [[maybe_unused]] const GenlUl2Args* ul = nullptr;
    if constexpr (LOGU) ul = &ga_.u;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* A = lds;
    float* G = A + ga->TB * 256;
    float* Zi = G + ga->DB0 * 256;                                   // DENSE: Z = B^T grad_x V, later B u
    float* Wi = Zi + ga->DB0 * 256;                                  //        w = xi sqrt(dt) + c dt
    float* Ui = Wi + ga->DB0 * 256;                                  //        u = w + dt Z (quadratic h only)
    [[maybe_unused]] float* ZLi = nullptr;                           // LOGU, DENSE: Z_n kept until X_{n+1} exists (kinds LINEAR, GRID)
    if constexpr (LOGU && DENSE) ZLi = Ui + ga->DB0 * 256;
    const float* __restrict__ T = ga->tables;
    const int lane = threadIdx.x & 63, j = lane & 15, q = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const bool w0 = wave == 0;                                       // every wave carries the tile's state; wave 0 writes the outputs
    const int D = ga->d, DB0 = ga->DB0;
    const int t16 = blockIdx.x;
    const int k = t16 * 16 + j;
    const bool kvalid = k < a->K_local;
    const uint32_t kglob = (uint32_t)(a->k_offset + k);
    const float dt = a->dt, sqdt = a->sqdt, sig = a->sigma_scale, Tend = a->T;
    const int TBq = D >> 4, TRq = (D & 15) >> 2, TQq = D & 3;        // position of the time input (feature index D) in the T layout
    unsigned long long nact = 0;
    for (int i = threadIdx.x; i < 2 * ga->TB * 256; i += 64 * NW) lds[i] = 0.f;
    tile_sync<NW>();

    f32x4 X[GENL_MAXDB];
    f32x4 Rr[GenlGeo<NW>::MAXSLOT];
#pragma unroll
    for (int s = 0; s < GenlGeo<NW>::MAXSLOT; ++s) Rr[s] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int b = 0; b < GENL_MAXDB; ++b)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int f = 16 * b + 4 * r + q;
            const float v = (b < DB0) ? a->x0[(size_t)(kvalid ? k : 0) * D + (f < D ? f : D - 1)] : 0.f;
            X[b][r] = (f < D && kvalid) ? v : 0.f;
        }
    float t = (kvalid && ga->has_time) ? a->t0[k] : 0.f;
    bool stopped = !kvalid;
    float Y = 0.f;
    int msteps = 0;                                                  // active steps of this trajectory (exact)
    auto put_time = [&](float tv) {
        if (ga->has_time) {
#pragma unroll
            for (int b = 0; b < GENL_MAXDB; ++b)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (b == TBq && r == TRq && opaque_i(q) == TQq) X[b][r] = tv;
        }
    };
    auto put_state = [&]() {
        if (w0) {
#pragma unroll
            for (int b = 0; b < GENL_MAXDB; ++b) if (b < DB0) img_put(A, b, X[b], lane);
        }
        tile_sync<NW>();
    };
    put_time(t);
    const float* vdr = a->drift;                                      // (d) kappa / diagonal of A, read per block below
    const size_t PBL = (size_t)2 * DB0 * 256;                        // path block: X image, U image

    [[maybe_unused]] float ULsum = 0.f;                              // LOGU: sum_n |-Z_n - u*(X_{n+1}, t_n)|^2 dt of this lane's features
    [[maybe_unused]] int ukind = 0;
    [[maybe_unused]] bool lastk = false;                             // the reference's i[-1] -= 2 (ugrid.h)
    if constexpr (LOGU) { ukind = ul->kind; lastk = (long long)a->k_offset + k == ul->Kglobal - 1; }
    int nex = a->N;
    for (int n = 0; n < a->N; ++n) {
        // every trajectory of the tile frozen: nothing changes any more (solver.py:1093-1097 / :742-744 leave the loop); all the
        // waves of the tile carry the same state, so the verdict is uniform over the workgroup
        if (__builtin_amdgcn_ballot_w64(!stopped) == 0ull) { nex = n; break; }
        // (feature masks (16 b + 4 r + q < D) are invariant over the time loop: hoisted, they are ~60 SGPR pairs, all spilled to VGPR
        //  lanes; an opaque copy of q per step keeps them as one v_cmp where they are used)
        const int qv = opaque_i(q);
        put_state();
        float Vnow = genl_value<NW>(ga, T, A, Rr, lane, q, wave);
        [[maybe_unused]] float gate = 1.f, eS = 0.f, eQ = 0.f, ecS = 0.f;     // EIG: 1[o > 0]; the row reductions of its h / drift kinds
        if constexpr (EIG) {
            if (eg->out_relu) { gate = Vnow > 0.f ? 1.f : 0.f; Vnow = fmaxf(Vnow, 0.f); }
        }
        if (n == 0) Y = Vnow;                                        // solver.py:1081 / :721
        if (a->Vsteps && w0 && q == 0) {                             // Solver's value-function ansatz: sum_n (Y_n(X_n) - Y)^2 (solver.py:438-440)
            a->Vsteps[(size_t)n * (a->ntile16 * 16) + k] = Vnow;
            a->Ysteps[(size_t)n * (a->ntile16 * 16) + k] = Y;
        }
        genl_input_gradient<NW>(ga, T, Rr, G, lane, q, wave);
        const float alivef = stopped ? 0.f : 1.f;
        auto noise_block = [&](int b) __attribute__((always_inline)) {
            f32x4 xi;
            if (a->noise_mode == NOISE_PHILOX) {
                xi = philox_block((uint32_t)opaque_i((int)kglob), (uint32_t)n, (uint32_t)(4 * b + opaque_i(q)), a->iter, a->seed_lo, a->seed_hi);
            } else {
                const float* xrow = a->xi + ((size_t)n * a->K_local + (kvalid ? k : 0)) * D;
#pragma unroll
                for (int r = 0; r < 4; ++r) { const int f = 16 * b + 4 * r + qv; xi[r] = xrow[f < D ? f : D - 1]; }
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) xi[r] = ((16 * b + 4 * r + qv) < D && kvalid) ? xi[r] : 0.f;
            return xi;
        };
        auto z_block = [&](int b) __attribute__((always_inline)) {       // Z = sigma^T grad_x V, sigma = s I (solver.py:1104)
            if constexpr (DENSE) return img_get(Zi, b, lane);        // (rows >= d of the B^T table are zero)
            const f32x4 gx = img_get(G, b, lane);
            f32x4 Z;
#pragma unroll
            for (int r = 0; r < 4; ++r) Z[r] = ((16 * b + 4 * r + qv) < D) ? sig * gx[r] : 0.f;
            if constexpr (EIG) Z = gate * Z;                         // grad relu(o) = 1[o > 0] grad o
            return Z;
        };
        auto drift_vec = [&](int b) __attribute__((always_inline)) {
            f32x4 v;
#pragma unroll
            for (int r = 0; r < 4; ++r) { const int f = 16 * b + 4 * r + qv; v[r] = (f < D && a->drift_kind != DRIFT_ZERO) ? vdr[f] : 0.f; }
            return v;
        };
        auto move_block = [&](int b, const f32x4& Z, const f32x4& xi) __attribute__((always_inline)) {
            const f32x4 cdt = a->adaptive ? (-dt) * Z : 0.f * Z;
            f32x4 drift = 0.f * Z;
            if (a->drift_kind == DRIFT_DWELL) {
                if (a->dwell_form) drift = -(((4.0f * drift_vec(b)) * X[b]) * (X[b] * X[b] - 1.0f));       // problems.py:1286
                else drift = -(4.0f * drift_vec(b) * (X[b] * (X[b] * X[b] - 1.0f)));
            } else if (a->drift_kind == DRIFT_DIAG) drift = drift_vec(b) * X[b];
            if constexpr (EIG) {
                if (a->drift_kind == DRIFT_EIG_FP) {                 // b_i = -cos(S) c_i sin x_i
                    const f32x4 c4 = drift_vec(b);
#pragma unroll
                    for (int r = 0; r < 4; ++r) drift[r] = ((-ecS) * c4[r]) * sinf(X[b][r]);
                }
            }
            if constexpr (DENSE) return (drift * dt + img_get(G, b, lane)) * alivef;      // B w: formed once per step, below
            return (drift * dt + sig * cdt + (sig * sqdt) * xi) * alivef;
        };
        float S = 0.f, Pz = 0.f;
        [[maybe_unused]] float UL = 0.f;
        // LOGU: this lane's part of |-Z_n - u*|^2 for state block b (the arithmetic of hjbd_fwd_kernel's LOGU branch); Xb = X_{n+1}
        [[maybe_unused]] auto ul2_table_block = [&](int b, const f32x4& Z) __attribute__((always_inline)) {
            const float* ur = ul->ref + (size_t)n * D;           // u* does not depend on X_{n+1}
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int f = 16 * b + 4 * r + qv;
                if (f < D) { const float e = Z[r] + ur[f]; UL = fmaf(e, e, UL); }
            }
        };
        [[maybe_unused]] auto ul2_grid_block = [&](int b, const f32x4& Z, const f32x4& Xb) __attribute__((always_inline)) {
            const long long rowofs = (long long)min(max(ul->row[n], 0), ul->nrows - 1) * ul->ncols;
            const long long tstride = (long long)ul->nrows * ul->ncols;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int f = 16 * b + 4 * r + qv;
                if (f < D) {                                         // (padding coordinates read no table)
                    const int cell = ugrid_cell(Xb[r], ul->xb, ul->xhi, ul->dx, lastk, ul->ncols);
                    const int grp = min(max(ul->group[f], 0), ul->ntables - 1);
                    const float e = -Z[r] - ul->ref[grp * tstride + rowofs + cell];
                    UL = fmaf(e, e, UL);
                }
            }
        };
        const float* BU = G;                                         // DENSE: the image that holds B u
        if constexpr (DENSE) {
            const int KSd = 4 * DB0;
            const bool quad = a->h_kind == GH_QUAD;
            bool zs = false;                                         // LQ: Z = B grad_x V, and the stored tangent is B^T u
            if constexpr (LQ) zs = ga->z_sigma != 0;
            for (int ob = wave; ob < DB0; ob += NW) {                // Z = B^T grad_x V
                f32x4 acc = {0.f, 0.f, 0.f, 0.f};
                genl_gemm1<8>(acc, T + (zs ? ga->tSB : ga->tSBT) + (size_t)ob * KSd * 64, KSd, G, lane);
                img_put(Zi, ob, acc, lane);
            }
            tile_sync<NW>();
#pragma unroll
            for (int b = 0; b < GENL_MAXDB; ++b)
                if (b < DB0) {
                    const f32x4 xi = noise_block(b);
                    const f32x4 Z = img_get(Zi, b, lane);
#pragma unroll
                    for (int r = 0; r < 4; ++r) { S = fmaf(Z[r], Z[r], S); Pz = fmaf(Z[r], xi[r], Pz); }
                    if constexpr (LOGU) {
                        if (ukind == GUL2_TABLE) ul2_table_block(b, Z);
                        else if (w0) img_put(ZLi, b, Z, lane);       // its own image: Zi takes B^T u below
                    }
                    const f32x4 cdt = a->adaptive ? (-dt) * Z : 0.f * Z;
                    const f32x4 w = sqdt * xi + cdt;
                    if (w0) {
                        img_put(Wi, b, w, lane);
                        if (quad) img_put(Ui, b, w + dt * Z, lane);
                    }
                }
            tile_sync<NW>();                                         // (every wave has read Z: its image may take B u)
            for (int ob = wave; ob < DB0; ob += NW) {                // B w (the move; the boxes test it) and B u (the stored tangent)
                f32x4 acw = {0.f, 0.f, 0.f, 0.f}, acu = {0.f, 0.f, 0.f, 0.f};
                if (zs) {                                            // B w and B^T u: two tables, nothing shared
                    genl_gemm1<8>(acw, T + ga->tSB + (size_t)ob * KSd * 64, KSd, Wi, lane);
                    genl_gemm1<8>(acu, T + ga->tSBT + (size_t)ob * KSd * 64, KSd, quad ? Ui : Wi, lane);
                    img_put(Zi, ob, acu, lane);
                } else if (quad) {
                    genl_gemm1x2<4>(acw, acu, T + ga->tSB + (size_t)ob * KSd * 64, KSd, Wi, Ui, lane);
                    img_put(Zi, ob, acu, lane);
                } else {
                    genl_gemm1<8>(acw, T + ga->tSB + (size_t)ob * KSd * 64, KSd, Wi, lane);
                }
                if constexpr (LQ) {                                  // + (dt A) X: the X image of this step; columns >= d of the table are zero
                    if (ga->driftA) genl_gemm1<8>(acw, T + ga->tA + (size_t)ob * KSd * 64, KSd, A, lane);
                }
                img_put(G, ob, acw, lane);
            }
            tile_sync<NW>();
            if (quad || zs) BU = Zi;
        }
        float rr = 0.f, sx = 0.f;
        if (a->domain_kind == DOM_SPHERE || a->domain_kind == DOM_ANNULUS || gh_reads_r2(a->h_kind)) {
#pragma unroll
            for (int b = 0; b < GENL_MAXDB; ++b)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (b < DB0 && (16 * b + 4 * r + qv) < D) {
                        rr = fmaf(X[b][r], X[b][r], rr);
                        if constexpr (DENSE) sx += X[b][r];
                    }
            rr = qsum(rr);
            if constexpr (DENSE) sx = qsum(sx);
        }
        if constexpr (EIG) {                                         // the state BEFORE the move, as every h here
            if (a->h_kind == GH_EIG_FP || a->h_kind == GH_EIG_NLS || a->drift_kind == DRIFT_EIG_FP) {
                const bool fp = a->h_kind != GH_EIG_NLS;
                const float dd = a->h_par[1];
#pragma unroll
                for (int b = 0; b < GENL_MAXDB; ++b)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int f = 16 * b + 4 * r + qv;
                        if (b < DB0 && f < D) {
                            const float sn = sinf(X[b][r]), cs = cosf(X[b][r]);
                            if (fp) { const float c = vdr[f]; eS += c * cs; eQ += (c * c) * (sn * sn); }
                            else { eS += cs; eQ += (sn * sn) / (dd * dd) - cs / dd; }
                        }
                    }
                eS = qsum(eS); eQ = qsum(eQ);
                ecS = cosf(eS);
            }
        }
        bool inside = true;
        if (a->domain_kind == DOM_SPHERE) {
            inside = sqrtf(rr) < a->dom_a;                            // the state BEFORE the move (:1121)
        } else if (a->domain_kind == DOM_ANNULUS) {
            const float rad = sqrtf(rr);                             // 'two_spheres' (:1122-1123 / :752-753), the state before the move
            inside = rad > a->dom_a && rad < a->dom_b;
        } else if (a->domain_kind >= DOM_BOX) {                       // the boxes test the PROPOSAL (:1126-1129)
            float n_out = 0.f, n_le = 0.f;
#pragma unroll
            for (int b = 0; b < GENL_MAXDB; ++b)
                if (b < DB0) {
                    f32x4 xi = {0.f, 0.f, 0.f, 0.f}, Zb = xi;
                    if constexpr (!DENSE) { xi = noise_block(b); Zb = z_block(b); }
                    const f32x4 Xp = X[b] + move_block(b, Zb, xi);
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if ((16 * b + 4 * r + qv) < D) {
                            const bool lo_ok = a->domain_kind != DOM_BOX || Xp[r] >= a->dom_a, hi_ok = Xp[r] <= a->dom_b;
                            n_out += (lo_ok && hi_ok) ? 0.f : 1.f;
                            n_le += hi_ok ? 1.f : 0.f;
                        }
                }
            n_out = qsum(n_out); n_le = qsum(n_le);
            inside = a->domain_kind == DOM_BOX_UPPER_ANY ? n_le > 0.f : n_out == 0.f;
        }
        // GH_SINE_SOURCE: this lane's X[0][0] of the state before the move (lane q holds coordinate q), carried in rr (gen_kernels.h)
        if (a->h_kind == GH_SINE_SOURCE) rr = X[0][0];
        const bool in_time = inside && (t + dt) <= Tend;             // new_selection (:1119-1131), fp32
        const bool act = in_time && !stopped;
        const float actf = act ? 1.f : 0.f;
        float* pblk = a->path + ((size_t)n * a->ntile16 + t16) * PBL + lane;
#pragma unroll
        for (int b = 0; b < GENL_MAXDB; ++b)
            if (b < DB0) {
                f32x4 U, step;
                [[maybe_unused]] f32x4 Zlog;
                if constexpr (DENSE) {
                    U = actf * img_get(BU, b, lane);                 // act B u
                    step = move_block(b, U, U);                      // (reads B w from its image)
                } else {
                    const f32x4 xi = noise_block(b);
                    const f32x4 Z = z_block(b);
#pragma unroll
                    for (int r = 0; r < 4; ++r) { S = fmaf(Z[r], Z[r], S); Pz = fmaf(Z[r], xi[r], Pz); }
                    const f32x4 cdt = a->adaptive ? (-dt) * Z : 0.f * Z;
                    f32x4 u = sqdt * xi + cdt;                       // u^ = act ((-h_z + c) dt + xi sqrt(dt)), -h_z = Z for h = -|z|^2 / 2
                    if (a->h_kind == GH_QUAD) u += dt * Z;
                    else if (a->h_kind == GH_AFFINE_EXP) {           // -h_z = -2 p2 z, every product with Z in it (gen_kernels.h)
                        const f32x4 pz = a->h_par[2] * Z;
                        u -= dt * (pz + pz);
                    }
                    U = (actf * sig) * u;
                    if constexpr (EIG) U = gate * U;
                    step = move_block(b, Z, xi);
                    if constexpr (LOGU) Zlog = Z;
                }
                if (a->store_path && w0) {                            // the sample point is the state BEFORE the move
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        pblk[(4 * b + r) * 64] = X[b][r];
                        pblk[(size_t)DB0 * 256 + (4 * b + r) * 64] = U[r];
                    }
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const bool fx = (16 * b + 4 * r + qv) < D;
                    X[b][r] = (fx && act) ? X[b][r] + step[r] : X[b][r];
                }
                if constexpr (LOGU && !DENSE) {                      // the log line follows the Euler step (solver.py:473-475)
                    if (ukind == GUL2_TABLE) ul2_table_block(b, Zlog);
                    else ul2_grid_block(b, Zlog, X[b]);
                }
            }
        if constexpr (LOGU && DENSE) {
            if (ukind == GUL2_LINEAR) {                              // u* = M_n X_{n+1}: the input blocks of A are dead, Wi too
                const int KSd = 4 * DB0;
                if (w0) {
#pragma unroll
                    for (int b = 0; b < GENL_MAXDB; ++b) if (b < DB0) img_put(A, b, X[b], lane);
                }
                tile_sync<NW>();
                for (int ob = wave; ob < DB0; ob += NW) {
                    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
                    genl_gemm1<8>(acc, T + ul->tUL + ((size_t)n * DB0 + ob) * KSd * 64, KSd, A, lane);
                    img_put(Wi, ob, acc, lane);
                }
                tile_sync<NW>();
#pragma unroll
                for (int b = 0; b < GENL_MAXDB; ++b)
                    if (b < DB0) {
                        const f32x4 Zn = img_get(ZLi, b, lane), Us = img_get(Wi, b, lane);
#pragma unroll
                        for (int r = 0; r < 4; ++r) { const float e = -Zn[r] - Us[r]; UL = fmaf(e, e, UL); }
                    }
            } else if (ukind == GUL2_GRID) {
#pragma unroll
                for (int b = 0; b < GENL_MAXDB; ++b) if (b < DB0) ul2_grid_block(b, img_get(ZLi, b, lane), X[b]);
            }
        }
        if constexpr (LOGU) ULsum = fmaf(UL, dt, ULsum);
        S = qsum(S); Pz = qsum(Pz);
        float minus_h = 0.f, hy = 0.f;                               // Y update (solver.py:1141-1142): h sees V(X, t), not the running Y
        if (a->h_kind == GH_QUAD) minus_h = 0.5f * S;
        else if (a->h_kind == GH_ALLEN_CAHN) { minus_h = -(Vnow - Vnow * Vnow * Vnow); hy = 1.0f - 3.0f * Vnow * Vnow; }
        else if (a->h_kind == GH_AFFINE_EXP) gh_affine_exp(a->h_par, Vnow, S, minus_h, hy);
        else if (a->h_kind == GH_SINE_SOURCE)
            gh_sine_source(a->h_par, Vnow, qsum(qv == 0 ? rr : 0.f), qsum(qv == 1 ? rr : 0.f), minus_h, hy);
        else if (a->h_kind == GH_SINNORM2) {
            if constexpr (DENSE) gh_sinnorm2(a->h_par, Vnow, rr, sx, minus_h, hy);
        } else if (EIG && a->h_kind >= GH_EIG_FP) {
            if constexpr (EIG) {
                float coef;                                          // h = y coef(x) [- y^3]
                if (a->h_kind == GH_EIG_FP) {
                    coef = (-eQ) * sinf(eS) - ecS * eS;
                    minus_h = -(Vnow * coef); hy = coef;
                } else {
                    coef = ((-a->h_par[0]) * expf((2.0f / a->h_par[1]) * eS) + eQ) - 3.0f;
                    minus_h = Vnow * Vnow * Vnow + Vnow * coef; hy = -3.0f * Vnow * Vnow - coef;
                }
            }
        } else if (a->h_kind >= GH_EXPBALL_LIN) {
            const float al = a->h_par[0];
            float rl = rr;                                           // |x|^2, or (sum x)^2 for the full-Hessian problem
            if constexpr (DENSE) { if (a->h_kind == GH_EXPBALL_SIN_FULL) rl = sx * sx; }
            const float lin = 2.0f * al * (2.0f * al * rl + a->h_par[1]) + a->h_par[2];
            float nl = 0.f, nly = 0.f;
            if (a->h_kind != GH_EXPBALL_LIN) {
                const float arg = expf(2.0f * al * rr + 2.0f * a->h_par[3] * ((float)n * dt)) - Vnow * Vnow;
                if (a->h_kind == GH_EXPBALL_SQ) { nl = arg; nly = -2.0f * Vnow; }
                else { nl = sinf(arg); nly = -2.0f * Vnow * cosf(arg); }
            }
            minus_h = Vnow * lin - nl;
            hy = nly - lin;
        }
        if constexpr (LQ) {
            if (ga->runcost_kind != 0) {                             // + f(X_{n+1}): Solver's h sees the state AFTER the move (solver.py:477)
                float fx = 0.f;
#pragma unroll
                for (int b = 0; b < GENL_MAXDB; ++b)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int f = 16 * b + 4 * r + qv;
                        if (b < DB0 && f < D) fx = fmaf(ga->runcost[f] * X[b][r], X[b][r], fx);
                    }
                minus_h += qsum(fx);
            }
        }
        const float zc = a->adaptive ? -S : 0.f;
        if constexpr (EIG) { minus_h -= lam * Vnow; hy += lam; Slam = fmaf(Vnow * actf, dt, Slam); }
        Y = Y + ((minus_h + zc) * dt + Pz * sqdt) * actf;
        float ahn = (n == 0 ? 1.f : 0.f) - hy * dt * actf;
        if constexpr (EIG) ahn *= gate;                              // dV/dtheta = 1[o > 0] do/dtheta
        if (a->store_path && w0 && q == 0) a->ahat[(size_t)n * (a->ntile16 * 16) + k] = ahn;
        t = t + dt * actf;
        put_time(t);
        if (act && q == 0) ++nact;
        msteps += act ? 1 : 0;
        stopped = stopped || !in_time;
        tile_sync<NW>();                                             // the G image is read above and rewritten by the next step
    }
    // final point: V(X_N, t_N) (solver.py:1163 / :799) as an extra value-only sample
    put_state();
    float VN = genl_value<NW>(ga, T, A, Rr, lane, q, wave);
    if constexpr (EIG) {
        if (eg->out_relu) VN = fmaxf(VN, 0.f);
        if (kvalid && w0 && q == 0 && eg->S_out) eg->S_out[k] = Slam;
    }
    if (a->store_path && w0) {
        float* pblk = a->path + ((size_t)a->N * a->ntile16 + t16) * PBL + lane;
#pragma unroll
        for (int b = 0; b < GENL_MAXDB; ++b)
            if (b < DB0) {
#pragma unroll
                for (int r = 0; r < 4; ++r) { pblk[(4 * b + r) * 64] = X[b][r]; pblk[(size_t)DB0 * 256 + (4 * b + r) * 64] = 0.f; }
            }
        if (q == 0) a->ahat[(size_t)a->N * (a->ntile16 * 16) + k] = 1.f;
    }
    if (w0 && lane == 0 && ga->nexec) ga->nexec[t16] = nex;
    // (no time input = EllipticSolver: t_N counts the active steps as m dt with one rounding, gen_kernels.h)
    if (kvalid && w0 && q == 0) { a->VN[k] = VN; a->YN[k] = Y; a->tN[k] = ga->has_time ? t : (float)msteps * dt; }
    if constexpr (LOGU) {
        const float ULt = qsum(ULsum);
        if (kvalid && w0 && q == 0) ul->out[k] = ULt;
    }
    if (kvalid && w0) {
#pragma unroll
        for (int b = 0; b < GENL_MAXDB; ++b)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int f = 16 * b + 4 * r + q;
                if (b < DB0 && f < D) a->XN[(size_t)k * D + f] = X[b][r];
            }
    }
    for (int o = 1; o < 64; o <<= 1) nact += __shfl_xor(nact, o);
    if (w0 && lane == 0 && nact) atomicAdd(a->kcount, nact);
}

// =======================================================================================
// Backward kernel: per block of 16 samples (n, tile) of the path store.
// LDS: A, Ad (a, a': TB blocks each), AB, ABd (abar, abar' of the HIDDEN segments, later zbar_i, zbar_i' in place: TB - DB0 each,
// and one more block each for the output layer seen as a layer of one unit with zbar = a, zbar' = w), then one int per
// weight-gradient tile of this launch group (its operand offsets).
// gridDim.y = launch groups of NW * MAXT weight-gradient tiles (a group recomputes the sweep and accumulates its tiles; group 0
// also carries the bias gradients): the notebooks' nets need one group.
// =======================================================================================
__host__ __device__ inline int genl_bwd_lds_bytes(int TB, int DB0, int NW) {
    return (4 * TB - 2 * DB0 + 2) * 1024 + NW * 32 * 4;
}

// MS = register slots for the hidden blocks a wave owns (hidden block hb -> wave hb mod NW, slot hb / NW): GenlGeo<NW>::MAXSLOT
// serves every net the kernels accept; the eight-wave instance with MS = 3 (sum of the hidden blocks <= 24: the Allen-Cahn notebook's
// net has 18) keeps 12 registers less per array and requests its table operands two k-step groups ahead instead of four: 37
// instead of 97 spilled dwords -- the weight-tile accumulators that lived in scratch no longer do -- and the backward of that net
// goes 3.98 -> 3.29 ms at K = 16 384 (same-box A/B).
template <int NW, int MS = GenlGeo<NW>::MAXSLOT>
__global__ __launch_bounds__(64 * NW) void genl_bwd_kernel(const GenlArgs ga_) {
    PSP_COND_EXIT(ga_.g);
    const KArgs ga = &ga_;
    const KGen a = &ga->g;
    const float* __restrict__ T = ga->tables;
    using Geo = GenlGeo<NW>;
    constexpr int MAXT = Geo::MAXT;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int TB = ga->TB, DB0 = ga->DB0, HBS = TB - DB0;
    float* A = lds;                   // a
    float* Ad = A + TB * 256;         // a'
    float* AB = Ad + TB * 256;        // abar of hidden block hb at AB + 256 hb; zbar_i in place once layer i has been swept
    float* ABd = AB + (HBS + 1) * 256;    // abar' / zbar_i'
    int* tdesc = reinterpret_cast<int*>(ABd + (HBS + 1) * 256);
    const int lane = threadIdx.x & 63, j = lane & 15, q = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int Kpad = a->ntile16 * 16;
    const size_t PBL = (size_t)2 * DB0 * 256;
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    const int lofsF = image_lane_offset_F(lane);
    const int tile0 = blockIdx.y * (NW * MAXT);                      // first tile of this launch group
    const bool g0 = blockIdx.y == 0;
    // tile t of layer i = (input block ib, unit block mb), mb fastest; layer L = the output layer (one unit: pseudo block HBS).
    // descriptor = A-image block | zbar-image block << 8 | layer << 16 | mb << 20
    for (int t = threadIdx.x; t < NW * MAXT; t += 64 * NW) {
        const int tt = tile0 + t;
        int dsc = -1;
        if (tt < ga->tcum[ga->L]) {
            int i = 0;
            for (int l = 1; l < GENL_MAXL; ++l) if (l < ga->L && tt >= ga->tcum[l]) i = l;
            const int loc = tt - ga->tcum[i];
            const int ib = loc / ga->HB[i], mb = loc - ib * ga->HB[i];
            dsc = ib | ((ga->off[i + 1] - DB0 + mb) << 8) | (i << 16) | (mb << 20);
        } else if (tt < ga->n_tiles) {
            dsc = (tt - ga->tcum[ga->L]) | (HBS << 8) | (ga->L << 16);
        }
        tdesc[t] = dsc;
    }
    tile_sync<NW>();
    f32x4 accW[MAXT];                 // weight tiles of this wave: slot s <-> tile tile0 + wave + NW s
    f32x4 accB[MS];         // bias gradients of the wave's hidden blocks (summed over the 16 sample lanes at the end)
    f32x4 Rr[MS], Zr[MS];
    float accb = 0.f;
#pragma unroll
    for (int s = 0; s < MAXT; ++s) accW[s] = zero4;
#pragma unroll
    for (int s = 0; s < MS; ++s) { accB[s] = zero4; Rr[s] = zero4; Zr[s] = zero4; }
    const long long nblk = (long long)(a->N + 1) * a->ntile16;
    for (long long blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
        const int n = (int)(blk / a->ntile16), t16 = (int)(blk % a->ntile16);
        const bool fin = (n == a->N);
        if (!fin && ga->nexec && n >= ga->nexec[t16]) continue;        // the tile had left the time loop: nothing was stored
        const int k = t16 * 16 + j;
        // per_sample (Solver's value-function ansatz): wY is (N + 1, Kpad) tangent weights and ahat holds the coefficient itself
        const float wy = a->wY[(a->per_sample ? (size_t)n * Kpad : 0) + k], wv = a->per_sample ? 0.f : a->wV[k];
        const float ah = a->ahat[(size_t)n * Kpad + k];
        const bool sval = k < a->K_local;
        const float av = sval ? (a->per_sample ? ah : (fin ? wv : wy * ah)) : 0.f;          // coefficient of grad_theta V
        const float ws = (sval && !fin) ? wy : 0.f;                  // weight of the tangent part
        const float* pb = a->path + (size_t)blk * PBL + lane;
        tile_sync<NW>();                                             // the previous block's tiles have been read
        for (int ks = wave; ks < 4 * DB0; ks += NW) { A[ks * 64 + lane] = pb[ks * 64]; Ad[ks * 64 + lane] = pb[(size_t)DB0 * 256 + ks * 64]; }
        tile_sync<NW>();
        // ---- recompute: z_i, z_i' (shared table operands), a = phi(r), a' = phi1(r) z'; r and z' of the wave's blocks stay in registers
        for (int i = 0; i < ga->L; ++i) {
            const int seg = ga->off[i + 1];
            const int KSin = 4 * seg, HBi = ga->HB[i], hoff = seg - DB0;
#pragma unroll
            for (int s = 0; s < MS; ++s) {
                const int mb = wave + NW * s - hoff;
                if (mb >= 0 && mb < HBi) {
                    f32x4 acc = vec_get(T + ga->vB[i], mb, q), acd = zero4;
                    genl_gemm1x2<(MS < GenlGeo<NW>::MAXSLOT ? 2 : 4)>(acc, acd, T + ga->tF[i] + (size_t)mb * KSin * 64, KSin, A, Ad, lane);
                    const f32x4 r = gact_r(ga->act, acc);
                    Rr[s] = r; Zr[s] = acd;
                    img_put(A, seg + mb, gact_h(ga->act, r), lane);
                    img_put(Ad, seg + mb, gact_h1(ga->act, r) * acd, lane);
                }
            }
            tile_sync<NW>();
        }
        // ---- adjoint seeds abar = a w_out, abar' = w w_out on the hidden segments; the output layer as a one-unit layer: its
        // "zbar" block holds a in unit 0 (dw = a a_L + w a_L' then is one more row of weight tiles), db = a
        if (g0 && wave == 0 && q == 0) accb += av;
        if (wave == 0) {
            img_put(AB, HBS, f32x4{q == 0 ? av : 0.f, 0.f, 0.f, 0.f}, lane);
            img_put(ABd, HBS, f32x4{q == 0 ? ws : 0.f, 0.f, 0.f, 0.f}, lane);
        }
#pragma unroll
        for (int s = 0; s < MS; ++s) {
            const int hb = wave + NW * s;
            if (hb < HBS) {
                const f32x4 w = vec_get(T + ga->vW, DB0 + hb, q);
                img_put(AB, hb, av * w, lane);
                img_put(ABd, hb, ws * w, lane);
            }
        }
        tile_sync<NW>();
        for (int i = ga->L - 1; i >= 0; --i) {
            const int seg = ga->off[i + 1];
            const int HBi = ga->HB[i], KSh = 4 * HBi, hoff = seg - DB0;
#pragma unroll
            for (int s = 0; s < MS; ++s) {
                const int hb = wave + NW * s;
                if (hb >= hoff && hb < hoff + HBi) {
                    const f32x4 gh = img_get(AB, hb, lane), ghd = img_get(ABd, hb, lane);
                    const f32x4 p1 = gact_h1(ga->act, Rr[s]);
                    const f32x4 zbd = ghd * p1;
                    const f32x4 zb = gh * p1 + ghd * (gact_h2(ga->act, Rr[s]) * Zr[s]);
                    img_put(AB, hb, zb, lane); img_put(ABd, hb, zbd, lane);
                    if (g0) accB[s] += zb;
                }
            }
            tile_sync<NW>();
            if (i > 0) {                                             // (the input segment's adjoint is not needed: no input gradient)
                // hidden segments below layer i only; two products with the same reverse table: abar += W zbar, abar' += W zbar'
                for (int ohb = wave; ohb < hoff; ohb += NW) {
                    f32x4 acc = img_get(AB, ohb, lane), acd = img_get(ABd, ohb, lane);
                    genl_gemm1x2<(MS < GenlGeo<NW>::MAXSLOT ? 2 : 4)>(acc, acd, T + ga->tR[i] + (size_t)(DB0 + ohb) * KSh * 64, KSh, AB + hoff * 256, ABd + hoff * 256, lane);
                    img_put(AB, ohb, acc, lane); img_put(ABd, ohb, acd, lane);
                }
                tile_sync<NW>();
            }
        }
        // ---- weight-gradient tiles: dW_i[16 inputs of block ib][16 units of block mb] += sum over the 16 samples of a zbar^T + a' zbar'^T.
        // Both operands are feature-on-lane reads of the images (lane (i, q') holds feature i of samples 4 q' .. 4 q' + 3, so
        // component r is k-step r of a 16x16x4 product whose k index q' stands for sample 4 q' + r on both sides)
#pragma unroll
        for (int s = 0; s < MAXT; ++s) {
            const int dsc = __builtin_amdgcn_readfirstlane(tdesc[wave + NW * s]);
            if (dsc >= 0) {
                const int ib = dsc & 0xff, hb = (dsc >> 8) & 0xff;
                const f32x4 a4 = image_get_F(A + ib * 256, lofsF), ad4 = image_get_F(Ad + ib * 256, lofsF);
                const f32x4 z4 = image_get_F(AB + hb * 256, lofsF), zd4 = image_get_F(ABd + hb * 256, lofsF);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    accW[s] = mfma16(a4[r], z4[r], accW[s]);
                    accW[s] = mfma16(ad4[r], zd4[r], accW[s]);
                }
            }
        }
    }
    // ---- partial gradients of this workgroup: row blockIdx.x of gpart; every entry of the row is written by exactly one lane
    float* gp = ga->gpart + (size_t)blockIdx.x * (size_t)ga->P;
#pragma unroll
    for (int s = 0; s < MAXT; ++s) {
        const int dsc = __builtin_amdgcn_readfirstlane(tdesc[wave + NW * s]);
        if (dsc >= 0) {
            const int ib = dsc & 0xff, i = (dsc >> 16) & 0xf, mb = (dsc >> 20) & 0xf;
            const int u = 16 * mb + j;                               // C layout: lane (column j, q) holds rows 4 q + r
            const int Hi = i < ga->L ? ga->H[i] : 1;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int rf = genl_real_feature(ga, 16 * ib + 4 * q + r);
                if (rf >= 0 && u < Hi) gp[genl_w_index(ga, i, rf, u)] = genl_feature_scale(ga, 16 * ib + 4 * q + r) * accW[s][r];
            }
        }
    }
    if (g0) {
#pragma unroll
        for (int s = 0; s < MS; ++s) {
            const int hb = wave + NW * s;
            if (hb < HBS) {
                const int i = genl_layer_of(ga, hb);
                const int mb = hb - (ga->off[i + 1] - DB0);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float v = jsumf(accB[s][r]);
                    const int u = 16 * mb + 4 * r + q;
                    if (j == 0 && u < ga->H[i]) gp[ga->ob[i] + u] = v;
                }
            }
        }
        if (wave == 0) {
            const float v = jsumf(accb);
            if (lane == 0) gp[ga->ob[ga->L]] = v;
        }
    }
}

// host side: launches (the dynamic LDS size exceeds the 64 KiB default)
template <int NW, bool DENSE = false, bool LQ = false, bool LOGU = false, bool EIG = false> inline hipError_t genl_launch_fwd(const typename GenlFwdArgsOf<LOGU, EIG>::type& a, int ntile16, int lds_bytes, hipStream_t st) {
    return launch_lds<genl_fwd_kernel<NW, DENSE, LQ, LOGU, EIG>>(dim3(ntile16), dim3(64 * NW), lds_bytes, st, a);
}
// the linear-quadratic instances <NW, true, true> are compiled in a unit of their own (genl_lq_instance.hip), so that the unit
// of the other instances holds the kernels it held; nw = 1, 4 or 8
hipError_t genl_lq_launch_fwd(const GenlArgs& a, int nw, int ntile16, int lds_bytes, hipStream_t st);
// the u_L2-log instances <NW, false, false, true> / <NW, true, true, true> (a.lq picks) and the kernel that stages the gains of
// PSP_UL2_LINEAR (N tables behind u.tUL from u.ref): a unit of their own as well (genl_ul2_instance.hip)
hipError_t genl_ul2_launch_fwd(const GenlLogArgs& a, int nw, int ntile16, int lds_bytes, hipStream_t st);
hipError_t genl_ul2_launch_stage(const GenlLogArgs& a, hipStream_t st);
// the eigenvalue instances <NW, false, false, false, true>: a unit of their own (genl_eig_instance.hip)
hipError_t genl_eig_launch_fwd(const GenlEigFwdArgs& a, int nw, int ntile16, int lds_bytes, hipStream_t st);
template <int NW, int MS = GenlGeo<NW>::MAXSLOT> inline hipError_t genl_launch_bwd(const GenlArgs& a, int grid, int groups, int lds_bytes, hipStream_t st) {
    return launch_lds<genl_bwd_kernel<NW, MS>>(dim3(grid, groups), dim3(64 * NW), lds_bytes, st, a);
}

}  // namespace psp
