/*
 * psp.h -- C ABI of the MI355X-native path-space hot path (libpsp_hip.so).
 *
 * The reference (lorenzrichter/path-space-PDE-solver) is pure Python and exposes no
 * FFI; its boundary is the duck-typed Solver / Problem / FunctionSpace API.  This
 * library sits underneath this repo's Python mirror of that API and replaces the
 * body of the training iteration for the supported catalogue:
 *   Solver.train (reference solver.py:420-557)
 *     psp_hjb_*   approx_method='control', time_approx='inner', one tanh MLP with two hidden layers
 *                 (function_space.py:177-195); losses log-variance / moment (in the kernels), variance /
 *                 cross_entropy (caller-supplied trajectory weights), relative_entropy; detach_forward True, or
 *                 False through psp_hjb_adjoint_sweep (gradients through the state path); importance-sampling
 *                 evaluation (psp_hjb_rollout_eval, utilities.py:287-359)
 *     psp_dnet_*  DenseNet controls (function_space.py:116-140): time_approx='outer' (one net per time step) and a
 *                 DenseNet(d+1 -> d) swapped into z_n; forward rollout AND hand-written parameter gradient
 *                 (psp_dnet_rollout_bwd; instances whose accumulators do not fit report bwd_supported = 0);
 *                 detach_forward False and relative_entropy through psp_dnet_adjoint_sweep
 *   GeneralSolver.train / EllipticSolver.train (solver.py:1001-1206, :628-826)
 *     psp_gen_*   diffusion / BSDE loss on unbounded, sphere and box domains, V = DenseNet(d+1 -> 1) / DenseNet(d -> 1)
 *     psp_genl_*  the same for dense-concat value nets of one to four hidden layers; psp_genl_test_error: the K_test_log
 *                 diagnostic (utilities.py:440-472) sampled, evaluated and reduced on the device
 *   shared: psp_adam_step (per-net Adam, function_space.py:185), psp_allreduce + psp_comm_* (trajectory sharding over
 *   the GPUs of a node), diagnostics.
 *
 * Conventions
 *  - plain pointers and sizes only; every device buffer is owned by the caller
 *    (torch tensors on the Python side); nothing here allocates or frees.
 *  - all functions are asynchronous on the given hipStream_t (passed as void*),
 *    return 0 on success and a negative code on failure; psp_last_error() gives text.
 *  - everything is fp32 ("dtype f32"); partial sums of D are fp64.
 *  - parameters / gradients use the torch nn.Linear flat layout of the control net:
 *        [W1 (H x (d+1)), b1 (H), W2 (H x H), b2 (H), W3 (d x H), b3 (d)]
 *    where input column 0 of W1 is the time feature (reference solver.py:355).
 */
#ifndef PSP_H_
#define PSP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PSP_VERSION 400 /* 0.3.0: range_flag in psp_hjb_config / psp_gen_config (guarded split-product mode); 0.3.1: store_path 4;
                         * 0.4.0: PSP_DOM_ANNULUS; psp_genl_config.activation / linear_layout, psp_genl_rollout_bwd replaces
                         *        psp_genl_adjoints (hand-written weight gradient), psp_genl_sizes re-laid out; the backward side of
                         *        the range guard; psp_hjb_sizes.fwd_coop_tiles (the former `reserved`); the on-device noise is
                         *        Philox4x32-7 (psp_philox_normal_fill and every rollout kernel: 10 rounds before);
                         *        later in 0.4.0 (appended, no version bump): psp_dnet_config.ul2_* -- the u_L2 log of the
                         *        DenseNet-control forward for reference controls that depend on x (PSP_UL2_LINEAR / PSP_UL2_GRID);
                         *        psp_is_config / psp_is_rollout / psp_is_query / psp_abi_struct_sizes3 -- the reference-control and
                         *        uncontrolled importance-sampling rollout (PSP_ISC_*);
                         *        psp_isw_sizes / psp_isw_query / psp_isw_rollout -- the same rollout for wide states, d <= PSP_ISW_MAX_D;
                         *        psp_genl_config.sigma_kind / sigma -- a dense constant diffusion matrix in the run-time-shaped
                         *        value-net kernels (PSP_GENL_SIGMA_*), and PSP_GH_EXPBALL_SIN_FULL;
                         *        psp_hjb_basis_params / psp_hjb_basis_grad -- the per-iteration transforms of a rollout in the
                         *        sigma basis;
                         *        psp_genl_eval_config / psp_genl_eval_query / psp_genl_test_error / psp_abi_struct_sizes4 -- the
                         *        K_test_log diagnostic sampled, evaluated and reduced on the device (PSP_TSAMPLE_*, PSP_VTRUE_*);
                         *        psp_genl_coeffs / psp_genl_query_lq / psp_genl_rollout_fwd_lq -- Z = sigma grad V, a dense drift matrix
                         *        and the diagonal running cost in the run-time-shaped value-net kernels (Solver's value-function
                         *        ansatz on LLGC / LQGC); the struct carries its own size instead of joining psp_abi_struct_sizes*;
                         *        psp_genl_adj / psp_genl_query_adj / psp_genl_adjoint_sweep -- the adjoint sweep of the state path for the value-function
 *        ansatz with detach_forward=False (csrc/genl_adj_kernels.h).
 *        psp_genl_ul2 / psp_genl_query_ul2 / psp_genl_ul2_stage / psp_genl_rollout_fwd_ul2 -- the u_L2 log of
                         *        that ansatz inside the run-time-shaped forward kernel (PSP_UL2_*); its own size again;
                         *        psp_pinn_config.n_dirs (the former `reserved`) / dirs (appended) -- second-order directions of a
                         *        dense sigma in the PINN kernels (PSP_GENL_SIGMA_DENSE, PSP_GH_EXPBALL_SIN_FULL);
                         *        PSP_GH_AFFINE_EXP / _SINE_SOURCE / _SINNORM2 (the exit-time and box problems),
                         *        psp_gen_config.dwell_form (the former `reserved`), PSP_VTRUE_LOGQ / _SINPROD / _SINSUM / _SINR2;
                         *        PSP_DRIFT_WELL_DIAG / _RADIAL_WELL, PSP_TERM_QUAD_LINEAR / _RADIAL_QUAD and psp_hjb_config.coord_split
                         *        (the former `reserved`) -- psp_dnet_* only;
                         *        psp_loss_stats_state_bytes / psp_loss_stats_accumulate / psp_loss_stats_finish -- the loss
                         *        estimators' statistics over chunks of (Y_N, D) in double (no struct: the state is a buffer) */

/* drift b(x): reference problems.py:36-37,154-155 (dense), :311-315 (double well) */
enum { PSP_DRIFT_ZERO = 0, PSP_DRIFT_DENSE = 1, PSP_DRIFT_DIAG = 2, PSP_DRIFT_DOUBLE_WELL = 3 };
/* DenseNet-control family only (psp_dnet_*; every other entry point answers -1 to them, as to any unknown kind):
 *   PSP_DRIFT_WELL_DIAG    per-coordinate kinds (DoubleWell_OU, problems.py:865-866): coordinates i < coord_split are wells,
 *                          b_i = -((4 kappa_i) x_i) (x_i^2 - 1) with kappa_i = drift[i]; the others are linear, b_i = a_i x_i
 *                          with a_i = drift[i].  b'_i = -4 kappa_i (3 x_i^2 - 1) / a_i.
 *   PSP_DRIFT_RADIAL_WELL  b = -(phi(r) / r) x,  r = |x|,  phi(r) = 4 kappa (r - r0) ((r - r0)^2 - w),  drift = {kappa, r0, w}
 *                          (DoubleWell_multidim_2, problems.py:705-709: r0 = 3, w = 1).  The Jacobian is symmetric:
 *                          b'^T l = -(phi / r) l - ((phi' - phi / r) / r^2) (x . l) x,  phi' = 4 kappa (3 (r - r0)^2 - w). */
enum { PSP_DRIFT_WELL_DIAG = 8, PSP_DRIFT_RADIAL_WELL = 9 };
/* sigma(x) = B constant: problems.py:39-40,157-158,317-318 */
enum { PSP_SIGMA_IDENTITY = 0, PSP_SIGMA_DENSE = 1, PSP_SIGMA_SCALED_IDENTITY = 2 };
/* running cost f(x) inside h = -0.5|z|^2 - f(x): problems.py:46 (zero), :161,167 (x'Px, diagonal P) */
enum { PSP_RUNCOST_ZERO = 0, PSP_RUNCOST_DIAG_QUAD = 1 };
/* terminal cost g(x): problems.py:49 (alpha.x), :164 (x'Rx, diagonal R), :334 (sum eta_j (x_j-1)^2) */
enum { PSP_TERM_LINEAR = 0, PSP_TERM_DIAG_QUAD = 1, PSP_TERM_SHIFTED_QUAD = 2 };
/* DenseNet-control family only (psp_dnet_*), like the two drift kinds above:
 *   PSP_TERM_QUAD_LINEAR   g = sum_{i < coord_split} term[i] (x_i - 1)^2 + sum_{i >= coord_split} term[i] x_i
 *                          (DoubleWell_OU, problems.py:880-881)
 *   PSP_TERM_RADIAL_QUAD   g = alpha (r - rho)^2,  r = |x|,  term = {alpha, rho};  grad g = 2 alpha (r - rho) x / r
 *                          (DoubleWell_multidim_2, problems.py:720-721: rho = 2) */
enum { PSP_TERM_QUAD_LINEAR = 8, PSP_TERM_RADIAL_QUAD = 9 };
/* loss: solver.py:167-168 (log-variance), :165-166 (moment) */
/* PSP_LOSS_WEIGHTS: psp_hjb_rollout_bwd takes w_k = dLoss/dY_k itself in its D argument (losses whose
 * weights are not affine in D: variance :171-172, cross_entropy :183-186) */
/* PSP_LOSS_REL_ENTROPY (solver.py:179-180, 484-486): the forward kernel accumulates Y = -Zsum =
 * -sum_n (|Z_n|^2 / 2 + f(X_{n+1})) dt, so D = Y - g(X_N) = -(Zsum + g) and the loss is -mean D = -sums[0] / K. */
enum { PSP_LOSS_LOG_VARIANCE = 0, PSP_LOSS_MOMENT = 1, PSP_LOSS_WEIGHTS = 2, PSP_LOSS_REL_ENTROPY = 3 };
/* Brownian increments: supplied = the reference's host-generated xi (solver.py:381), philox = on device */
enum { PSP_NOISE_SUPPLIED = 0, PSP_NOISE_PHILOX = 1 };

/* arithmetic type of the matrix products (operands; accumulation is always fp32) */
enum { PSP_MLP_FP32 = 0, PSP_MLP_BF16_FWD = 1, PSP_MLP_BF16 = 2, PSP_MLP_F16X3 = 3 };

/* POD description of one HJB rollout problem on one rank. */
typedef struct psp_hjb_config {
    int32_t d;            /* state dimension                                    */
    int32_t H;            /* hidden width of the control MLP (two hidden layers) */
    int32_t K_local;      /* trajectories on this rank                           */
    int32_t N;            /* time steps, floor(T/dt) (solver.py:41)              */
    int64_t K_global;     /* trajectories over all ranks (loss normalisation)    */
    int64_t k_offset;     /* global index of local trajectory 0 (Philox counter) */
    float dt;             /* fp32 step (solver.py:39)                            */
    float sqrt_dt;        /* fp32 sqrt(dt) (solver.py:40)                        */
    int32_t drift_kind;
    int32_t sigma_kind;
    int32_t runcost_kind;
    int32_t term_kind;
    int32_t adaptive;     /* 1: c = -Z (solver.py:456), 0: c = 0 (solver.py:451) */
    int32_t loss_kind;
    int32_t noise_mode;
    int32_t store_path;   /* 0: forward only; 1: keep X_n, h1, h2, xi for the backward pass;
                           * 2 / 3: same with xi - sqrt(dt) Z / Z in the xi slot, for psp_hjb_adjoint_sweep;
                           * 4: keep X_n, h1, h2 only -- psp_hjb_rollout_bwd regenerates xi from the Philox counters
                           *    (seed, iter of the call = those of the forward call).  Narrow family, PSP_NOISE_PHILOX,
                           *    adaptive = 1 (the image of mode 1 is then xi itself); the block layout is that of mode 1
                           *    with the xi slot unused (same path_bytes).  Not for psp_hjb_rollout_bwd_step.        */
    float sigma_scale;    /* PSP_SIGMA_SCALED_IDENTITY                            */
    int32_t coord_split;  /* (the former `reserved`) PSP_DRIFT_WELL_DIAG / PSP_TERM_QUAD_LINEAR: the first coord_split coordinates
                           * take the first formula of the kind, the others the second; in [0, d_real].  Read by psp_dnet_* only,
                           * and only with one of these two kinds                   */
    const float* drift;   /* DENSE: A (d*d row-major); DIAG: a (d); DOUBLE_WELL: kappa (d); WELL_DIAG: kappa_i / a_i (d);
                           * RADIAL_WELL: {kappa, r0, w} (the buffer still holds d floats) */
    const float* sigma;   /* DENSE: B (d*d row-major); else NULL                  */
    const float* runcost; /* DIAG_QUAD: p (d); else NULL                          */
    const float* term;    /* alpha / r / eta (d); QUAD_LINEAR: eta_i / alpha_i (d); RADIAL_QUAD: {alpha, rho} (d floats) */
    const float* u_ref;   /* optional (N, d) + 16 floats of slack: reference control u*(t_n) of a solution that does not depend on x
                           * (LLGC, problems.py:51-53); enables the u_L2 log of solver.py:491-494 inside the
                           * forward kernels.  NULL: no logging                                             */
    float* u_l2_out;      /* (K_local): sum_n |-Z_n(X_n) - u*(t_n)|^2 dt per trajectory (mean = u_L2_loss)  */
    int32_t mlp_dtype;    /* how the matrix products are computed (accumulation is fp32 in every mode):
                           * PSP_MLP_FP32 (0): v_mfma_f32_16x16x4_f32.
                           * PSP_MLP_F16X3: fp32-GRADE split products on the f16 matrix pipe -- every operand x = hi + lo / 2048 as
                           * two f16 numbers, a.b = hi.hi + (hi.lo + lo.hi) / 2048 as three v_mfma_f32_16x16x32_f16 (16x the
                           * fp32 matrix rate); same parity bounds as PSP_MLP_FP32 (D within 2e-5, gradient 2e-4, loss 1e-4 of the
                           * reference; observed 1e-6), operands must stay below 65504 in magnitude.  Narrow family: forward
                           * (hjb_fwd_kernel mode 2, tile-per-wave kernel only), adjoint sweep and backward (hjb_bwd3_kernel); wide
                           * family: forward, adjoint sweep and backward (d > 256: hjbw_bwd_x3_kernel; d <= 256: hjbw_bwd2x_kernel); DenseNet
                           * controls (psp_dnet_*): forward and adjoint sweep; -3 where an instance does not have the mode or its
                           * tables do not fit the LDS.  The weight-carrying operands of the backward passes (~1 / K) are scaled by
                           * a power of two inside the kernels and the results scaled back (exact).
                           * PSP_MLP_BF16_FWD: the three products of the control net in the FORWARD rollout on
                           * v_mfma_f32_16x16x32_bf16 (bf16 operands: its OWN tolerance, not the 1e-4 bar); drift / sigma
                           * products, state, sums and the backward pass stay fp32.  Narrow kernel family only (-3 otherwise) */
    int32_t reserved2;
    const uint32_t* iter_dev; /* optional DEVICE-resident iteration counter (the `iter` member of a psp_iter_state): when set, the
                           * forward kernels key Philox with *iter_dev instead of the `iter` argument, so that a captured
                           * hipGraph of the iteration can be replayed without per-iteration host arguments.  NULL: `iter` */
    int32_t* range_flag;  /* optional DEVICE int32[4] (8-byte aligned; [2..3] are scratch of the library), read only with mlp_dtype == PSP_MLP_F16X3: the RANGE GUARD of the split-product
                           * mode.  The reference computes in fp32 (solver.py:39-40); an f16x3 operand beyond 65504 has hi = +inf and
                           * lo = -inf, so main and correction chains of every product it enters meet as inf - inf: every output of
                           * that trajectory is NaN from that step on and D_k is NaN -- an overflow can never go unnoticed, and it
                           * costs nothing to detect.  The narrow family's forward (hjb_fwd_kernel) keeps its products on ONE accumulator
                           * with both operands scaled by a power of two (csrc/hjb_kernels.h, split_tab); there the scaled hi part
                           * overflows sooner and hi = +inf, lo = -inf meet in that accumulator -- the same NaN.  Its thresholds:
                           * |weight| (net, dt A, sigma) < 1023 and |state|, |activation| < 2047.  With range_flag set,
                           *   psp_hjb_rollout_fwd / psp_dnet_rollout_fwd run the split kernel, set range_flag[0] = 1 iff a per-workgroup
                           *     partial of (sum D, sum D^2) is non-finite (else 0; range_flag[1] counts the 1s), and enqueue the
                           *     fp32-MFMA kernel of the same launch PREDICATED on range_flag[0] (its workgroups return at once when it
                           *     is 0; when it runs it overwrites D, the partials and the path store, whose format the two share);
                           *   psp_hjb_adjoint_sweep, psp_hjb_rollout_bwd(_step), psp_dnet_adjoint_sweep enqueue the split kernel
                           *     predicated on range_flag[0] == 0 and its fp32-MFMA twin predicated on range_flag[0] == 1.
                           * A guarded iteration therefore returns the fp32-MFMA result wherever the split kernels left their range
                           * (and the same non-finite loss as the reference when fp32 itself overflows), with no host sync.
                           * NULL: unguarded split kernels.                                                                       */
} psp_hjb_config;

/* Sizes of the caller-owned scratch buffers for a config. */
typedef struct psp_hjb_sizes {
    int64_t path_bytes;       /* X_n store for the backward pass (0 if !store_path)  */
    int64_t fwd_partial_bytes;/* per-workgroup (sum D, sum D^2) fp64 pairs            */
    int64_t grad_partial_bytes;/* per-workgroup partial gradients                     */
    int32_t n_params;         /* p = (d+1)H+H + H*H+H + H*d+d                         */
    int32_t fwd_workgroups;
    int32_t bwd_workgroups;
    int32_t fwd_coop_tiles;   /* 0.4.0 (the former `reserved`): 2 or 4 when psp_hjb_rollout_fwd runs the cooperative wide forward
                               * (hjbc_fwd_kernel: that many 16-trajectory tiles per 512-thread workgroup), else 0 */
} psp_hjb_sizes;

int psp_version(void);
const char* psp_last_error(void);
/* sizeof() of the six structs above / below, in declaration order (psp_hjb_config, psp_hjb_sizes, psp_gen_config,
 * psp_gen_sizes, psp_dnet_config, psp_dnet_sizes): lets a binding check its own struct declarations at load time. */
int psp_abi_struct_sizes(int32_t out[6]);
/* ... and of psp_genl_config, psp_genl_sizes (added in 0.3.0). */
int psp_abi_struct_sizes2(int32_t out[2]);

/* 1 if a compiled kernel instantiation exists for (d, H), else 0. */
int psp_hjb_supported(int32_t d, int32_t H);
/* Kernel family that serves (d, H): 0 none, 1 narrow (state panel in registers, tables in LDS; any flag
 * combination of psp_hjb_config), 2 wide (large d: tables in global memory). */
int psp_hjb_family(int32_t d, int32_t H);
/* Enumeration of the compiled (d, H) instances (family as above).  A configuration whose (d, H) is not in the
 * list runs EXACTLY on any instance with larger d and H after zero padding (padded state components never couple
 * back: zero weight rows / columns, zero drift, sigma, running- and terminal-cost entries); the host mirror
 * (native_shapes.py) picks the cheapest one and keeps the index map between the real and the padded flat
 * parameter / gradient vectors. */
int psp_hjb_instance_count(void);
int psp_hjb_instance_get(int32_t i, int32_t* d, int32_t* H, int32_t* family);

/* Fills *out; returns <0 if the config is not supported. */
int psp_hjb_query(const psp_hjb_config* cfg, psp_hjb_sizes* out);

/*
 * Forward rollout: replaces the n-loop of Solver.train (solver.py:440-478) plus
 * initialize_training_data (:364-382) and D = Y - g(X_N) of loss_function (:167-168).
 *   params   : flat control-net parameters (device)
 *   x0       : initial states, x0_stride = 0 -> one (d) vector broadcast (solver.py:365),
 *              x0_stride = d -> (K_local, d) row-major (random_X_0, solver.py:367)
 *   y0       : device pointer to the learnable scalar Y_0 (solver.py:372-373) or NULL (Y=0)
 *   xi       : PSP_NOISE_SUPPLIED: (N+1, K_local, d) fp32, slice n+1 drives step n
 *              (the reference's (K,d,N+1) tensor permuted); ignored for PHILOX
 *   seed,iter: Philox key / iteration counter
 *   path     : X_n store (path_bytes) or NULL
 *   D_out    : (K_local) fp32, D_k = Y_k - g(X_N,k)
 *   XN_out   : optional (K_local, d) final states or NULL
 *   Y_out    : optional (K_local) Y_N (losses that need Y and g separately) or NULL
 *   fwd_partial: fwd_partial_bytes scratch
 * Three kernels implement this call for the narrow family (d <= 112), chosen from the trajectory count of the launch so that
 * the chip stays busy: one 16-trajectory tile per wave (hjb_fwd_kernel), a tile split over the eight waves of a workgroup
 * when there are at most two tiles per CU (hjbs_fwd_kernel, K <= 8192 on 256 CUs), four trajectories per workgroup on
 * v_mfma_f32_4x4x1 when there are at most CUs / 4 tiles (hjbq_fwd_kernel, K <= 1024).  Same Philox counters and path-store
 * format; D agrees to summation order.  The environment variable PSP_FWD_VARIANT=1 / 2 / 3 forces one (tests, A/B timing).
 */
int psp_hjb_rollout_fwd(const psp_hjb_config* cfg, const float* params, const float* x0, int32_t x0_stride,
                        const float* y0, const float* xi, uint64_t seed, uint32_t iter, float* path,
                        float* D_out, float* XN_out, float* Y_out, double* fwd_partial, void* stream);

/*
 * Forward-only controlled rollout for importance-sampling evaluation: replaces the n-loop of
 * utilities.do_importance_sampling_me (reference utilities.py:309-328) with u = -Z_n (control='approx').
 * Same kernel as psp_hjb_rollout_fwd with store_path = 0 and
 *   tfeat    : (N) fp32 network time input per step -- the reference maps t = n*delta_t to
 *              ceil(t / model.delta_t) * model.delta_t (solver.py:360-362); NULL -> n*dt
 *   D_out    : Y_N - g(X_N) with Y accumulated as in Solver.train; the Girsanov log-weight of
 *              utilities.py:330-336 is  D_out - 2*Fint_out  (-int f - g - int u.dW - 0.5 int |u|^2)
 *   Fint_out : optional (K_local) sum_n f(X_{n+1}) dt
 */
int psp_hjb_rollout_eval(const psp_hjb_config* cfg, const float* params, const float* x0, int32_t x0_stride,
                         const float* xi, uint64_t seed, uint32_t iter, const float* tfeat, float* D_out,
                         float* Fint_out, float* XN_out, double* fwd_partial, void* stream);

/* Sums the per-workgroup partials in a fixed order: sums_out[0] = sum_k D_k, sums_out[1] = sum_k D_k^2
 * over this rank's trajectories (fp64, device).  The caller all-reduces sums_out across ranks. */
int psp_hjb_terminal_reduce(const psp_hjb_config* cfg, const double* fwd_partial, double* sums_out, void* stream);

/*
 * Backward pass: replaces loss.backward() of solver.py:221 with the analytic gradient
 * (detach_forward=True: dL/dZ_n[k] = w_k ((Z_n + c) dt + xi_{n+1} sqrt(dt)),
 *  w_k = (2/K)(D_k - mean D) for log-variance, (2/K) D_k for moment).
 *   path     : the path store written by psp_hjb_rollout_fwd with store_path != 0 (register images of
 *              X_n, h1, h2 and of the Brownian increment xi_{n+1} per step and 16-trajectory tile)
 *   xi, seed, iter : accepted for symmetry with the forward call and ignored -- the increments are read
 *              back from `path`, whatever the noise mode (a VALU cycle next to the fp32 MFMA stream
 *              costs more than the extra 448 B per trajectory-step of path store)
 *   sums     : GLOBAL (sum D, sum D^2), fp64 on device (after the all-reduce)
 *   grad_partial : grad_partial_bytes scratch (per-workgroup partial gradients; the wide kernel family
 *              also keeps an operand table there)
 *   grad_out : flat gradient (n_params fp32) for this rank's trajectories, summed in a fixed
 *              order (bitwise reproducible).  The gradient of the learnable Y_0 (moment loss)
 *              is (2/K) sum_k D_k and is formed by the caller from `sums`.
 */
int psp_hjb_rollout_bwd(const psp_hjb_config* cfg, const float* params, const float* xi, uint64_t seed,
                        uint32_t iter, const float* path, const float* D, const double* sums,
                        float* grad_partial, float* grad_out, void* stream);

/*
 * Gradients THROUGH the state path: adaptive_forward_process=True with detach_forward=False, the reference's default
 * flags (solver.py:451-469: c = -Z_n(X_n) is not detached, so loss.backward() of solver.py:221 also differentiates the
 * Euler-Maruyama recursion :471-478).  Call sequence per iteration:
 *     psp_hjb_rollout_fwd   with store_path = 2 (losses of Y_N - g(X_N)) or 3 (PSP_LOSS_REL_ENTROPY), XN_out given
 *     [loss and per-trajectory weights  mu_k = dL/dY_N[k],  nu_k = dL/dZsum_N[k]  from D on the caller's side]
 *     psp_hjb_adjoint_sweep  reverse-time adjoint recursion per trajectory (kernel: csrc/hjba_kernels.h); rewrites the
 *                            xi slot of `path` with dL/dZ_n / sqrt(dt)
 *     psp_hjb_rollout_bwd   with loss_kind = PSP_LOSS_WEIGHTS and D = 1 for every trajectory
 *   XN : (K_local, d) terminal states from the forward call;  mu, nu : K_local floats each (nu may be NULL = 0);
 *   wT : K_local weights of grad g(X_N) in lambda_N, or NULL for nu - mu (losses that depend on X_N only through
 *        Y_N - g(X_N) resp. Zsum_N + g(X_N)); cross_entropy passes -Y_N exp(D) / K (solver.py:183-185);
 *   fwd_partial : the forward call's scratch (the large-d kernel family rebuilds its operand tables in it).
 */
int psp_hjb_adjoint_sweep(const psp_hjb_config* cfg, const float* params, float* path, const float* XN,
                          const float* mu, const float* nu, const float* wT, double* fwd_partial, void* stream);

/* torch.optim.Adam(lr, betas=(b1,b2), eps, weight_decay=0, amsgrad=False) on a flat buffer
 * (function_space.py:185, solver.py:198-200).  step is 1-based. */
int psp_adam_step(float* params, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                  int32_t step, float lr, float beta1, float beta2, float eps, void* stream);

/*
 * Launch-bound regime (BASELINE.json configs[1]: K = 1024, N = 50 -- a whole iteration is ~0.3 ms): the six launches of an
 * iteration are captured ONCE into a hipGraph by the caller (any stream-capture API: the entry points only enqueue
 * kernels on the given stream) and replayed.  Everything that changes from one iteration to the next then has to live in
 * device memory: psp_iter_state holds the Philox iteration index and Adam's step count / running beta powers;
 *   psp_hjb_config.iter_dev = &state->iter         forward kernels
 *   psp_hjb_terminal_reduce_loss(..., &state->iter) partial sums -> (sum D, sum D^2) AND the loss value of solver.py:167-168 /
 *                                                   :165-166 / :179-180 into loss_log[state->iter] (single rank: the local
 *                                                   sums are the global ones; replaces six tiny element-wise launches)
 *   psp_adam_step_dev                               Adam with bias corrections 1 - beta^step taken from the state
 *   psp_iter_state_advance                          iter += 1, step += 1, beta powers *= beta (last node of the graph)
 */
typedef struct psp_iter_state {
    uint32_t iter;        /* iteration index l of Solver.train (Philox counter, index into the loss log) */
    uint32_t step;        /* 1-based Adam step the NEXT psp_adam_step_dev applies                        */
    double beta1_pow;     /* beta1 ** step, beta2 ** step (fp64, as torch forms its bias corrections)    */
    double beta2_pow;
} psp_iter_state;
/* Fills a HOST copy (the caller uploads it): state for iteration `iter` whose Adam step is `step` (1-based). */
int psp_iter_state_init(psp_iter_state* host_out, uint32_t iter, int32_t step, float beta1, float beta2);
int psp_iter_state_advance(psp_iter_state* dev_state, float beta1, float beta2, void* stream);
/* psp_hjb_terminal_reduce + the loss of cfg->loss_kind (log-variance / moment / relative entropy) from these sums with
 * K = cfg->K_global, written as fp32 to loss_log[index_dev ? *index_dev : 0].  Only valid when the rank's sums ARE the
 * global sums (one rank); with several ranks call psp_hjb_terminal_reduce, all-reduce, and form the loss from the result. */
int psp_hjb_terminal_reduce_loss(const psp_hjb_config* cfg, const double* fwd_partial, double* sums_out, float* loss_log,
                                 const uint32_t* index_dev, void* stream);
/* psp_hjb_rollout_bwd + gradient reduction + Adam + psp_iter_state_advance as TWO launches instead of four (launch-bound sizes:
 * each tiny launch costs ~4 us inside a replayed graph): the reduction kernel applies the Adam update to the parameter it has
 * just summed and the last of its workgroups advances the state.  Only for the exact (unpadded) parameter layout, one rank,
 * loss kinds the kernels weight themselves; `ticket` is one zero-initialised device uint32 owned by the caller. */
int psp_hjb_rollout_bwd_step(const psp_hjb_config* cfg, float* params, const float* path, const float* D, const double* sums,
                             float* grad_partial, float* grad_out, float* exp_avg, float* exp_avg_sq, psp_iter_state* dev_state,
                             uint32_t* ticket, float lr, float beta1, float beta2, float eps, void* stream);
/* psp_adam_step with step / bias corrections read from a device psp_iter_state. */
int psp_adam_step_dev(float* params, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                      const psp_iter_state* dev_state, float lr, float beta1, float beta2, float eps, void* stream);

/* Materialises the device noise stream exactly as the rollout kernels consume it:
 * out is (N+1, K_local, d) fp32 with slice 0 zero.  Test / diagnostics helper. */
int psp_philox_normal_fill(float* out, int32_t N, int32_t K_local, int32_t d, int64_t k_offset,
                           uint64_t seed, uint32_t iter, void* stream);

/* Control evaluation u = -Z on a batch (solver.py:349-362): out (K, d) = -MLP([t, X]). */
int psp_hjb_control_eval(int32_t d, int32_t H, const float* params, const float* X, int32_t K, float t,
                         float* minus_Z_out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * GeneralSolver.train hot path (reference solver.py:1001-1206): diffusion / BSDE loss on unbounded and bounded
 * (sphere / box) domains, V = DenseNet(d+1 -> 1, two hidden layers of width H, relu^2; function_space.py:116-140).
 * EllipticSolver.train (solver.py:628-826, V = DenseNet(d -> 1)) runs through the same entry points with T = +inf
 * and a zero time row in the parameter map (the padded-shape index map of the host adds it).
 * Flat parameter layout = the DenseNet's registration order, weights stored (in, out), input [x, t]:
 *     [W1 ((d+1) x H), b1 (H), W2 ((d+1+H) x H), b2 (H), W3 (d+1+2H), b3 (1)]
 * ------------------------------------------------------------------------------------------------ */
/* nonlinearity h(t,x,y,z): problems.py:1755 (0), :519 (-|z|^2/2), :1204 (y - y^3), and the exponential-on-the-ball
 * family  h = -2 al y (2 al |x|^2 + d) - e y + nl,  nl = 0 (LIN: problems.py:985, :1130 with e = 1),
 * E - y^2 (SQ: :1022), sin(E - y^2) (SIN: :1058, :1166 with e = 1 and the time term), E = exp(2 al |x|^2 + 2 tau t_n);
 * h_par = {al, d, e, tau}.  SIN_FULL (:1094, the full-Hessian problem; psp_genl_* only): SIN with (sum_i x_i)^2 = sum_ij x_i x_j
 * in place of |x|^2 in the linear term, |x|^2 kept in E
 *
 * The exit-time and box problems (problems.py:1220-1730), h_par = {p0, p1, p2, p3} with another meaning per kind:
 *   AFFINE_EXP   h = p0 + p1 y + p2 |z|^2 + p3 exp(-y);  h_y = p1 - p3 exp(-y), -h_z = -2 p2 z (the stored tangent direction carries
 *                (-2 p2) dt Z where PSP_GH_QUAD carries dt Z).  DoubleWell_stopping (1, 0, -1/2, 0), _stopping_linear (0, -1, 0, 0),
 *                _expectation_hitting_time (1, 0, 0, 0), QuadraticGradient (0, 0, 1 / B_00^2, -2)
 *   SINE_SOURCE  h = c y + s(x), sub-mode p0:  0 (Helmholtz, d >= 2): with S = sin(p1 x_0) sin(p2 x_1), c = p3 (= k^2),
 *                h = ((c y + p1^2 S) + p2^2 S) - c S;  1 (Oscillations): c = 0, h = p1^2 sin(p1 x_0) + (p2^2 p3) sin(p2 x_0)
 *   SINNORM2     (dense sigma: psp_genl_* only) with r2 = |x|^2, sx = sum_i x_i, al = p0, d = p1:  p2 != 0 (linear):
 *                h = al^2 (4 pi^2 sin(pi r2) sx^2 - 2 d pi cos(pi r2));  p2 = 0: h = al^2 (4 pi^2 y sx^2 - 2 d pi cos(pi r2)
 *                + sin(pi r2)^2 - y^2)
 * None of the three is built for the adjoint sweep, a running cost or psp_pinn_pairs_*; SINNORM2 not for psp_gen_* */
enum { PSP_GH_ZERO = 0, PSP_GH_QUAD = 1, PSP_GH_ALLEN_CAHN = 2, PSP_GH_EXPBALL_LIN = 3, PSP_GH_EXPBALL_SQ = 4,
       PSP_GH_EXPBALL_SIN = 5, PSP_GH_EXPBALL_SIN_FULL = 6, PSP_GH_AFFINE_EXP = 7, PSP_GH_SINE_SOURCE = 8, PSP_GH_SINNORM2 = 9 };
/* exit test of a bounded domain: a trajectory stays active while (solver.py:1119-1129; EllipticSolver :758-767)
 *   SPHERE        |X_n| < dom_a               (the state BEFORE the move, as the reference tests it)
 *   BOX           dom_a <= X_proposal <= dom_b in every coordinate
 *   BOX_UPPER_ALL X_proposal <= dom_b in every coordinate   (EllipticSolver, one_boundary)
 *   BOX_UPPER_ANY X_proposal <= dom_b in some coordinate    (GeneralSolver, one_boundary; also the exit test of
 *                                                            'square-corner', solver.py:759-760)
 *   ANNULUS       dom_a < |X_n| < dom_b       ('two_spheres', solver.py:1122-1123, :752-753; the state before the move) */
enum { PSP_DOM_NONE = 0, PSP_DOM_SPHERE = 1, PSP_DOM_BOX = 2, PSP_DOM_BOX_UPPER_ALL = 3, PSP_DOM_BOX_UPPER_ANY = 4,
       PSP_DOM_ANNULUS = 5 };

typedef struct psp_gen_config {
    int32_t d, H, K_local, N;
    int64_t k_offset;     /* global index of local trajectory 0 (Philox counter)            */
    float dt, sqrt_dt;    /* fp32 step and its fp32 square root (solver.py:950-951)          */
    float T;              /* terminal time: a trajectory freezes once t + dt > T (:1131)     */
    float sigma_scale;    /* sigma = s I (problems.py:493 s = 1; :1183,1740 s = sqrt 2)      */
    int32_t drift_kind;   /* PSP_DRIFT_ZERO, PSP_DRIFT_DIAG or PSP_DRIFT_DOUBLE_WELL               */
    int32_t h_kind;
    int32_t adaptive;     /* 1: c = -Z detached (solver.py:1111-1114), 0: c = 0              */
    int32_t noise_mode;   /* PSP_NOISE_SUPPLIED: xi is (N, K_local, d); PSP_NOISE_PHILOX      */
    int32_t store_path;   /* 1: keep what the backward pass needs                            */
    int32_t domain_kind;  /* PSP_DOM_*                                                         */
    const float* drift;   /* DOUBLE_WELL: kappa (d); DIAG: a (d); else NULL                  */
    float dom_a, dom_b;   /* sphere radius (dom_a), box bounds X_l, X_r, or annulus radii r_1, r_2 */
    float h_par[4];       /* PSP_GH_EXPBALL_*: al, d (the REAL dimension, not a padded one), e, tau; PSP_GH_AFFINE_EXP,
                           * _SINE_SOURCE, _SINNORM2: p0 .. p3 as listed at the enum                     */
    int32_t d_real;       /* components the exit test and |x|^2 read when d is a zero-padded instance (0: all d);
                           * the padding carries device noise, which nothing else ever reads                */
    int32_t mlp_dtype;    /* PSP_MLP_FP32 (0); PSP_MLP_BF16_FWD: the value-net products of the forward rollout (V, grad_x V,
                           * tangent pass) on v_mfma_f32_16x16x32_bf16 -- bf16 operands, fp32 accumulate; PSP_MLP_BF16: also the
                           * adjoint products and the weight-gradient outer products of the backward kernel.  State, Y,
                           * accumulators and every element-wise step stay fp32 (BASELINE.json configs[2]); with PSP_MLP_BF16 the
                           * path store holds the six images as bf16 pairs (960 instead of 1 920 bytes per sample:
                           * psp_gen_query reports the size), with PSP_MLP_BF16_FWD it stays fp32.
                           * PSP_MLP_F16X3: fp32-GRADE split products (psp_hjb_config.mlp_dtype) in the forward rollout and -- with
                           * shared trajectory weights -- in the backward kernel (per_sample_weights keeps fp32 MFMA there); fp32
                           * path store, the 1e-4 bounds of PSP_MLP_FP32; the network factors multiplying the scaled weights in
                           * the backward pass (w3 phi', W2 products) must stay below 256 in magnitude                        */
    /* Solver.train with approx_method='value_function' (solver.py:93-97, 334-339, 438-440: Z = sigma grad_x Y_n(X), loss +
     * mean_k sum_{n>=1} (Y_n(X_n) - Y)^2) runs on these kernels too (plan_value_native.py):                              */
    float* v_steps_out;   /* optional (N, 16*ceil(K_local/16)): V(X_n, t_n) at every step, written by psp_gen_rollout_fwd       */
    float* y_steps_out;   /* optional, same shape: the running Y before the increment of step n (both or neither)               */
    int32_t per_sample_weights; /* psp_gen_rollout_bwd: 1 -> wY is (N+1, 16*ceil(K_local/16)) = weight of the TANGENT part of every
                           * sample (0 in slot N) and `ahat` holds the coefficient of grad_theta V of every sample itself
                           * (wV is ignored): losses with a term at every step.  0: per-trajectory wY, wV as described below     */
    int32_t dwell_form;   /* (the former `reserved`) PSP_DRIFT_DOUBLE_WELL rounding, as psp_is_config.dwell_form: 0 =
                           * -(4 kappa_i) (x (x^2 - 1)) (the DoubleWell_multidim family), 1 = -((4 kappa_i) x) (x^2 - 1) (the
                           * exit-time double wells, problems.py:1286); read by the forward rollouts only                      */
    int32_t* range_flag;  /* optional DEVICE int32[4]: range guard of PSP_MLP_F16X3 as in psp_hjb_config.range_flag -- the forward sets
                           * range_flag[0] iff V(X_N) or Y_N of any trajectory is non-finite and enqueues the fp32-MFMA forward
                           * predicated on it; psp_gen_rollout_bwd enqueues both backward kernels, predicated.  NULL: unguarded    */
} psp_gen_config;

typedef struct psp_gen_sizes {
    int64_t path_bytes;        /* (N+1) sample slots x K/16 blocks of register images               */
    int64_t ahat_bytes;        /* (N+1) x 16*ceil(K/16) floats                                       */
    int64_t grad_partial_bytes;
    int32_t n_params, fwd_workgroups, bwd_workgroups, reserved;
} psp_gen_sizes;

int psp_gen_supported(int32_t d, int32_t H);
/* enumeration of the compiled GeneralSolver instances; zero padding works as for the HJB kernels (the time input stays
 * the LAST row of W1 / the x-t block of W2, W3: the host index map moves it from row d to row d_pad) */
int psp_gen_instance_count(void);
int psp_gen_instance_get(int32_t i, int32_t* d, int32_t* H);
int psp_gen_query(const psp_gen_config* cfg, psp_gen_sizes* out);

/* Forward rollout (solver.py:1076-1160 and V(X_N,t_N) of :1163): x0 (K_local,d), t0 (K_local) initial
 * points/times; outputs per trajectory V(X_N,t_N), Y_N, X_N (K_local,d), t_N and the active-step count
 * (K_log, :1152,1168) accumulated into *kcount (device u64, zeroed by the caller). */
int psp_gen_rollout_fwd(const psp_gen_config* cfg, const float* params, const float* x0, const float* t0,
                        const float* xi, uint64_t seed, uint32_t iter, float* path, float* ahat, float* VN,
                        float* YN, float* XN, float* tN, unsigned long long* kcount, void* stream);

/* Backward pass (replaces loss.backward() of solver.py:1187 for the domain part of the loss):
 *   grad_out = sum_k [ wV_k dV(X_N,t_N)/dtheta + wY_k dY_N/dtheta ]   over this rank's trajectories,
 * wY = dLoss/dY_N, wV = dLoss/dV(X_N,t_N) per trajectory, each ZERO-PADDED to 16*ceil(K_local/16)
 * floats (the kernel reads them with unconditional 16-byte loads), formed by the caller from
 * VN, YN (diffusion: wV = 2 a0 (VN - YN)/K = -wY ; BSDE: wV = 0, wY = 2 (YN - f(XN))/K). */
int psp_gen_rollout_bwd(const psp_gen_config* cfg, const float* params, const float* path, const float* ahat,
                        const float* wY, const float* wV, float* grad_partial, float* grad_out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * GeneralSolver / EllipticSolver with a value net of ANY depth: V = dense-concat net (d [+ 1] -> 1, arch = [H_1 .. H_L]),
 * 1 <= L <= 4, H_i <= 128, d + 1 <= 112 (reference function_space.py:116-140 DenseNet, relu^2; :143-158 DenseNet_tanh, tanh with
 * nn.Linear weights; the nets the diffusion-loss notebooks swap into model.V: Allen-Cahn.ipynb:72 arch = [110, 110, 50],
 * [30, 30, 30, 30], `Committor function.ipynb` cell 1: [d + 10, d, d, d] with tanh^2).  Shapes and activation are run-time
 * arguments: activations in per-tile LDS images, weights as A-operand tables in global memory (csrc/genl_kernels.h).  The
 * step is the one of psp_gen_rollout_fwd (same noise counters, exit tests, h kinds, outputs); a tile whose trajectories have
 * all stopped leaves the time loop early (solver.py:1093-1097 / :742-744) and the backward pass skips what it did not execute.
 */
/* diffusion matrix of psp_genl_config: s I from base.sigma_scale (what a zero-initialised struct means), or a dense constant
 * B (problems.py:1072: sqrt(2 / d) ones(d, d)).  Dense: per step Z = B^T grad_x V, X += (b dt + B (xi sqrt(dt) + c dt)) alive,
 * and the stored tangent direction is B u^ -- two d x d fp32-MFMA products per step (three with PSP_GH_QUAD) from tables of B
 * and B^T built next to the weight tables; psp_genl_rollout_bwd is the same kernel for both kinds. */
enum { PSP_GENL_SIGMA_SCALED = 0, PSP_GENL_SIGMA_DENSE = 1 };
enum { PSP_ACT_RELU2 = 0,   /* h = relu(z)^2   (function_space.py:138)                       */
       PSP_ACT_TANH2 = 1,   /* h = tanh(z)^2   (Committor function.ipynb, DenseNet_tanh_2)    */
       PSP_ACT_TANH = 2 };  /* h = tanh(z)     (function_space.py:157)                        */

typedef struct psp_genl_config {
    psp_gen_config base;      /* d = state dimension; H, mlp_dtype, d_real, range_flag unused */
    int32_t has_time;         /* 1: network input [x, t] (GeneralSolver), 0: [x] (EllipticSolver; base.T = +inf)                 */
    int32_t n_hidden;         /* L                                                                                              */
    int32_t widths[4];        /* H_1 .. H_L                                                                                     */
    int32_t activation;       /* PSP_ACT_*                                                                                      */
    int32_t linear_layout;    /* 0: weights stored (in, out) (DenseNet); 1: (out, in) (nn.Linear, DenseNet_tanh)                */
    int32_t time_first;       /* 1: the net's input is [t, x] (Solver.Y_n, solver.py:338) instead of [x, t]: only the parameter
                               * index map changes, the kernels keep the time in their last input row                          */
    float time_scale;         /* the net sees time_scale * t (0 = 1): Solver's value-function ansatz feeds the STEP INDEX
                               * n = t / dt as the time (solver.py:336, 439)                                                    */
    /* appended in 0.4.0 (the fields above keep their offsets) */
    int32_t sigma_kind;       /* PSP_GENL_SIGMA_SCALED (0): sigma = base.sigma_scale I; PSP_GENL_SIGMA_DENSE: sigma = B           */
    int32_t reserved;
    const float* sigma;       /* DENSE: B, DEVICE, d*d row-major fp32 (read by every psp_genl_rollout_fwd call); else NULL       */
} psp_genl_config;
/* base.v_steps_out / y_steps_out / per_sample_weights of the embedded psp_gen_config are honoured by psp_genl_rollout_fwd /
 * psp_genl_rollout_bwd exactly as by the psp_gen_* entry points (Solver(approx_method='value_function'), plan_value_native.py) */

typedef struct psp_genl_sizes {
    int64_t table_bytes;      /* scratch for the operand tables (rebuilt by every forward call; a dense sigma adds those of B, B^T) */
    int64_t path_bytes;       /* (N + 1) x ceil(K/16) blocks of x and s u^ images                                               */
    int64_t ahat_bytes;       /* (N + 1) x 16 ceil(K/16) floats, then ceil(K/16) int32: the step count of every tile            */
    int64_t n_params;         /* registration order W_1, b_1, .., W_out, b_out                                                  */
    int64_t grad_partial_bytes;     /* per-workgroup partial gradients of psp_genl_rollout_bwd                                  */
    int32_t n_blocks;         /* (N + 1) x ceil(K/16) sample blocks                                                              */
    int32_t fwd_workgroups, bwd_workgroups;
    int32_t waves_per_tile;   /* 1 (small nets, no barriers) or 8                                                               */
    int32_t seg_block_offset[5];    /* first padded 16-feature block of segment s (0: input, s: h_s); [L] + ceil(H_L/16) = TB    */
    int32_t reserved;
} psp_genl_sizes;

/* <0: shape outside the limits above, the activation images (with a dense sigma: plus its three product images where they
 * do not fit the dead part of the gradient image) exceed 160 KiB, or PSP_GENL_SIGMA_DENSE without a matrix. */
int psp_genl_query(const psp_genl_config* cfg, psp_genl_sizes* out);
/* Forward rollout; arguments as psp_gen_rollout_fwd plus the table scratch.  `ahat` is required (it carries the tiles' step
 * counts behind the coefficients). */
int psp_genl_rollout_fwd(const psp_genl_config* cfg, const float* params, const float* x0, const float* t0, const float* xi,
                         uint64_t seed, uint32_t iter, float* tables, float* path, float* ahat, float* VN, float* YN,
                         float* XN, float* tN, unsigned long long* kcount, void* stream);
/* Backward pass (replaces loss.backward() of solver.py:1187 / :814 for the domain part of the loss), arguments as
 * psp_gen_rollout_bwd: wY, wV per-trajectory loss weights zero padded to 16 ceil(K/16).  One kernel recomputes the activations
 * of every executed sample block, runs the adjoint sweep and accumulates all parameter gradients (weight tiles as MFMA outer
 * products over the samples of the block); grad_partial (psp_genl_sizes.grad_partial_bytes) is summed in a fixed order.
 * `tables` must hold the tables of the SAME parameters (psp_genl_rollout_fwd leaves them there). */
int psp_genl_rollout_bwd(const psp_genl_config* cfg, const float* params, const float* tables, const float* path,
                         const float* ahat, const float* wY, const float* wV, float* grad_partial, float* grad_out, void* stream);

/* Linear-quadratic coefficients of the forward rollout (appended in 0.4.0, no version bump): what
 * Solver(approx_method='value_function') needs on LLGC with off-diagonal entries and on LQGC (reference problems.py:14-65,
 * 118-175; solver.py:334-339, 471-478).  They travel beside psp_genl_config, which keeps its layout.  With g = grad_x V(X_n, t_n):
 *   Z  = B^T g (PSP_GENL_Z_SIGMA_T: GeneralSolver / EllipticSolver, solver.py:729 / :1104) or B g (PSP_GENL_Z_SIGMA: the ansatz of
 *        Solver, solver.py:338);  B = cfg->sigma, or base.sigma_scale I;
 *   w  = xi sqrt(dt) + c dt,  c = -Z (base.adaptive) or 0;   X += (b(X) dt + B w) alive,  b(X) = A X with `drift_matrix`
 *        (one more d x d product per step from a table of dt A; the boxes' exit test sees the whole proposal), else base.drift_kind;
 *   Y += ((-h + Z . c) dt + Z . xi sqrt(dt)) act;  DIAG_QUAD: -h = |Z|^2 / 2 + sum_i runcost[i] x_i^2 at the state AFTER the move
 *        (solver.py:477: h sees the updated X), PSP_GH_QUAD only;
 *   stored tangent U = act B u (Z_SIGMA_T) or act B^T u (Z_SIGMA), u = w (+ dt Z with PSP_GH_QUAD): Z . w = g . B^T w and
 *        d(|Z|^2 / 2) = (B^T Z) . dg, so psp_genl_rollout_bwd consumes (x, t), U and a^ unchanged -- call it with the same cfg.
 * The running cost does not depend on the parameters while the state path is detached: a^ is what it is without it.
 * Any coefficient that is set runs the dense-sigma path (s I then goes through the tables of B).  A NULL or all-zero struct --
 * and one that asks for nothing: Z_SIGMA_T, RUNCOST_ZERO, no matrix -- means psp_genl_query / psp_genl_rollout_fwd exactly: the
 * same plan, kernel instance and bits. */
enum { PSP_GENL_Z_SIGMA_T = 0, PSP_GENL_Z_SIGMA = 1 };
typedef struct psp_genl_coeffs {
    int32_t struct_bytes;        /* sizeof(psp_genl_coeffs): checked by the library (this struct is not in psp_abi_struct_sizes*) */
    int32_t z_kind;              /* PSP_GENL_Z_*                                                                                 */
    int32_t runcost_kind;        /* PSP_RUNCOST_ZERO | PSP_RUNCOST_DIAG_QUAD                                                     */
    int32_t reserved;
    const float* drift_matrix;   /* A, DEVICE, d*d row-major fp32: b(x) = A x (base.drift_kind must be PSP_DRIFT_ZERO); NULL:
                                  * base.drift_kind as in psp_genl_rollout_fwd                                                    */
    const float* runcost;        /* DIAG_QUAD: p, DEVICE, d floats; else NULL                                                    */
} psp_genl_coeffs;
/* psp_genl_query with the coefficients: table_bytes grows by the table of dt A (and by those of B, B^T where the config alone
 * would not build them).  <0 as psp_genl_query, or: wrong struct_bytes, an enum out of range, DIAG_QUAD without a vector or with
 * another h than PSP_GH_QUAD, a drift matrix together with a non-zero base.drift_kind.  No GPU needed. */
int psp_genl_query_lq(const psp_genl_config* cfg, const psp_genl_coeffs* coeffs, psp_genl_sizes* out);
/* psp_genl_rollout_fwd with the coefficients (every other argument as there; `tables`: psp_genl_query_lq's table_bytes). */
int psp_genl_rollout_fwd_lq(const psp_genl_config* cfg, const psp_genl_coeffs* coeffs, const float* params, const float* x0,
                            const float* t0, const float* xi, uint64_t seed, uint32_t iter, float* tables, float* path,
                            float* ahat, float* VN, float* YN, float* XN, float* tN, unsigned long long* kcount, void* stream);

/* The u_L2 log of the forward rollout (appended in 0.4.0, no version bump): what Solver(approx_method='value_function') logs
 * whenever the problem has a reference control u* (reference solver.py:471-475, 491-494).  With Z_n the Z of the Y update above,
 *   u_l2_out[k] = sum_{n < N} sum_i (-Z_{n,i} - u*_i(X_{n+1}, n dt))^2 dt        (u* at the state AFTER the move),
 * sequential in n, fp32, one float per local trajectory.  The description of u* travels beside the config and the coefficients,
 * which keep their layouts; its kinds are those of psp_dnet_config.ul2_kind (PSP_UL2_*, below), with the same semantics:
 *   PSP_UL2_TABLE   u_ref  = (N, d) table of u*(t_n), DEVICE;
 *   PSP_UL2_LINEAR  tables = (N, d, d) row-major gains M_n, u* = M_n X_{n+1}: one more d x d product per step from per-step
 *                   operand tables that psp_genl_ul2_stage writes into the table scratch ONCE (behind the region every
 *                   psp_genl_rollout_fwd* call rewrites); needs the linear-quadratic instances (a psp_genl_coeffs that asks for
 *                   something);
 *   PSP_UL2_GRID    u*_i = table_{group[i]}[row[n], cell(X_{n+1,i})], tables = (ntables, nrows, ncols), group = (d), row = (N);
 *                   cell = floor((clamp(x, -xb, xhi) + xb) / dx) in fp32 with a true division, lowered by two for the globally
 *                   last trajectory (k_offset + k == K_global - 1), a negative cell counting from the end of the row.
 * The log is defined for runs that never stop: base.domain_kind = PSP_DOM_NONE and base.T = inf.  Two kernel shapes carry it:
 * sigma = s I with an element-wise drift (TABLE, GRID) and the linear-quadratic one (all kinds); a dense sigma without
 * psp_genl_coeffs is refused.  A NULL psp_genl_ul2 means the entry point without it exactly: same plan, instance and bits. */
typedef struct psp_genl_ul2 {
    int32_t struct_bytes;        /* sizeof(psp_genl_ul2): checked by the library (this struct is not in psp_abi_struct_sizes*) */
    int32_t kind;                /* PSP_UL2_TABLE | PSP_UL2_LINEAR | PSP_UL2_GRID                                              */
    float* u_l2_out;             /* DEVICE, K_local floats, written by every psp_genl_rollout_fwd_ul2 call                     */
    const float* u_ref;          /* TABLE: (N, d); else NULL                                                                   */
    const float* tables;         /* LINEAR: (N, d, d) gains (read by psp_genl_ul2_stage only); GRID: (ntables, nrows, ncols)    */
    const int32_t* group;        /* GRID: (d) table of every coordinate, in [0, ntables)                                       */
    const int32_t* row;          /* GRID: (N) row of step n, ceil(t_n / dt_ref) formed on the host, in [0, nrows)              */
    int32_t ntables, nrows, ncols;
    float xb, dx, xhi;           /* GRID: as psp_dnet_config.ul2_xb / ul2_dx / ul2_xhi                                         */
    int64_t K_global;            /* GRID: locates the globally last trajectory                                                 */
} psp_genl_ul2;
/* psp_genl_query_lq with the log: table_bytes grows by the staged gains of PSP_UL2_LINEAR (N operand tables of
 * ceil((d + has_time) / 16)^2 blocks of 256 floats, 16-byte aligned) and not at all for the other kinds; the LDS rule counts the
 * image that keeps Z_n (LINEAR and GRID on the linear-quadratic instances).  <0 as psp_genl_query_lq, or: wrong struct_bytes, a
 * kind out of range, a pointer the kind needs missing, a stopping domain or a finite T.  No GPU needed. */
int psp_genl_query_ul2(const psp_genl_config* cfg, const psp_genl_coeffs* coeffs, const psp_genl_ul2* ul2, psp_genl_sizes* out);
/* PSP_UL2_LINEAR: writes the gains ul2->tables into the table scratch `tables` (psp_genl_query_ul2's table_bytes) in the layout
 * the forward reads.  Call once per plan and per set of gains, before the first psp_genl_rollout_fwd_ul2; a no-op for the other
 * kinds. */
int psp_genl_ul2_stage(const psp_genl_config* cfg, const psp_genl_coeffs* coeffs, const psp_genl_ul2* ul2, float* tables,
                       void* stream);
/* psp_genl_rollout_fwd_lq with the log (every other argument as there). */
int psp_genl_rollout_fwd_ul2(const psp_genl_config* cfg, const psp_genl_coeffs* coeffs, const psp_genl_ul2* ul2,
                             const float* params, const float* x0, const float* t0, const float* xi, uint64_t seed, uint32_t iter,
                             float* tables, float* path, float* ahat, float* VN, float* YN, float* XN, float* tN,
                             unsigned long long* kcount, void* stream);

/* Eigenvalue problems on the forward rollout (appended in 0.4.0, no version bump): what EigenvalueSolver needs for the eigenpairs
 * (lambda, V) of the diffusion-loss paper's `Eigenvalue - *.ipynb` notebooks -- Fokker-Planck and the nonlinear Schroedinger equation
 * on the periodic box [0, 2 pi]^d, sigma = s I, uncontrolled and detached state path.  The struct travels beside psp_genl_config,
 * which keeps its layout.  With o the net's linear output, V = relu(o) (output_relu) or o, c = 1[o > 0] (or 1), Z = c s grad_x o:
 *   X += (b(X) dt + s xi sqrt(dt)) alive   (the boxes test the proposal, as ever),
 *   Y += ((-h(X, V, Z) - lambda V) dt + Z . xi sqrt(dt)) act,          Y_0 = V(X_0),
 *   s_out[k] = sum_n act_n V(X_n) dt   (= -dY_N / dlambda: dLoss/dlambda of a loss in D = V(X_N) - Y_N is sum_k dLoss/dD_k s_out[k]).
 * lambda is read from DEVICE memory once per launch -- it is a trained scalar, and passing it by value would cost a host read
 * per iteration.  The path store holds the gated tangent direction c act s u and `ahat` the gated coefficient
 * c ([n = 0] - (h_y + lambda) dt act): psp_genl_rollout_bwd consumes them unchanged -- call it with the same cfg; with output_relu
 * the CALLER multiplies wV by 1[VN > 0] (VN is V(X_N) = relu(o_N), so VN > 0 is the gate of the final point).
 * Kinds that only these entry points accept (numbered away from the others; psp_genl_query / psp_genl_rollout_fwd refuse them):
 *   PSP_DRIFT_EIG_FP  b_i = -cos(S) c_i sin x_i,  S = sum_j c_j cos x_j,  c = base.drift (d floats)
 *   PSP_GH_EIG_FP     h = y (-sin(S) sum_i c_i^2 sin^2 x_i - cos(S) S), the same c (needs PSP_DRIFT_EIG_FP)
 *   PSP_GH_EIG_NLS    h = -y^3 - y (-p0 exp((2 / p1) sum_i cos x_i) + sum_i (sin^2 x_i / p1^2 - cos x_i / p1) - 3),
 *                     h_par = (1 / c^2, d, -, -)
 * The state path is detached and uncontrolled (base.adaptive = 0), so the backward never differentiates the drift or the x
 * dependence of h: it needs h_y alone.  Every other h / drift kind of the sigma = s I path runs here as well.
 * A NULL struct means psp_genl_query / psp_genl_rollout_fwd exactly: the same plan, kernel instance and bits. */
enum { PSP_GH_EIG_FP = 16, PSP_GH_EIG_NLS = 17 };      /* psp_gen_config.h_kind, psp_genl_*_eig only     */
enum { PSP_DRIFT_EIG_FP = 16 };                        /* psp_gen_config.drift_kind, psp_genl_*_eig only */
typedef struct psp_genl_eig {
    int32_t struct_bytes;        /* sizeof(psp_genl_eig): checked by the library (this struct is not in psp_abi_struct_sizes*) */
    int32_t output_relu;         /* 1: V = relu(net output); 0: the net as it is                                              */
    const float* lambda;         /* DEVICE, one float, read by every psp_genl_rollout_fwd_eig call; NULL: lambda = 0          */
    float* s_out;                /* DEVICE, K_local floats, written by every call; NULL: not wanted                           */
} psp_genl_eig;
/* psp_genl_query with the struct: the sizes are those of psp_genl_query.  <0 as psp_genl_query, or: wrong struct_bytes,
 * output_relu outside {0, 1}, a dense sigma (or an h kind that runs on the dense path), base.adaptive = 1, PSP_GH_EIG_FP without
 * PSP_DRIFT_EIG_FP, PSP_GH_EIG_NLS with h_par[1] <= 0.  No GPU needed; reads no pointer of `eig`. */
int psp_genl_query_eig(const psp_genl_config* cfg, const psp_genl_eig* eig, psp_genl_sizes* out);
/* psp_genl_rollout_fwd with the struct (every other argument as there). */
int psp_genl_rollout_fwd_eig(const psp_genl_config* cfg, const psp_genl_eig* eig, const float* params, const float* x0,
                             const float* t0, const float* xi, uint64_t seed, uint32_t iter, float* tables, float* path,
                             float* ahat, float* VN, float* YN, float* XN, float* tN, unsigned long long* kcount, void* stream);

/* Adjoint sweep of the state path (appended in 0.4.0, no version bump; csrc/genl_adj_kernels.h): what
 * Solver(approx_method='value_function') needs with adaptive_forward_process=True and detach_forward=False (the constructor
 * defaults; reference solver.py:449-478: c = -Z stays attached, so the states carry the parameters).  At a fixed sample the loss
 * still sees the parameters only through V(X_n, n) and grad_x V(X_n, n): psp_genl_rollout_bwd stays the gradient kernel, and the
 * sweep -- one workgroup per 16-trajectory tile, n = N-1 .. 0 -- rewrites what it consumes.  With g_n = grad_x V(X_n, n), Z_n = B g_n:
 *   lambda = lam_N;  for n = N-1 .. 0:
 *     Lam = lambda + mu_{n+1} dt grad f(X_{n+1});      U_n = mu_{n+1} U_fwd - dt B^T (mu_{n+1} Z_n + B^T Lam);
 *     lambda = Lam + dt J_b(X_n)^T Lam + a_n g_n + grad_x^2 V(X_n, n) U_n
 * (U_fwd: the direction psp_genl_rollout_fwd* stored; J_b: the drift matrix, or the diagonal Jacobian of base.drift_kind).
 * On return the path store holds U_n, `ahat` holds a_n and `ws` holds 1 on executed samples, 0 on the padding rows and at n = N:
 * call psp_genl_rollout_bwd(cfg, params, tables, path, ahat, ws, NULL, ...) exactly as without the sweep.
 * Defined for: base.adaptive = 1, base.h_kind = PSP_GH_QUAD, base.domain_kind = PSP_DOM_NONE, base.T = inf,
 * base.per_sample_weights = base.store_path = 1, and the orientation Z = sigma grad V (PSP_GENL_Z_SIGMA; sigma = s I without
 * coefficients is its own transpose).  The struct travels beside the config, the coefficients and the log, which keep their layouts. */
typedef struct psp_genl_adj {
    int32_t struct_bytes;        /* sizeof(psp_genl_adj): checked by the library (this struct is not in psp_abi_struct_sizes*)    */
    int32_t reserved;
    const float* mu;             /* DEVICE, (N + 1) x 16 ceil(K/16): mu_n, the adjoint of Y_n (mu_N = dLoss/dD; row 0 unused)       */
    const float* resid_coeff;    /* DEVICE, (N + 1) x 16 ceil(K/16): a_n (a_0 = mu_1, a_n = dLoss/dV(X_n, n) for n >= 1)            */
    const float* lam_N;          /* DEVICE, K_local x d: the adjoint of X_N from the terminal cost, -dLoss/dD grad g(X_N)          */
    float* lam0_out;             /* DEVICE, K_local x d: dLoss/dX_0 per trajectory, or NULL                                       */
    int64_t drift_t_offset;      /* float offset of the sweep's table of (dt A)^T inside the table scratch: WRITTEN by
                                  * psp_genl_query_adj, read by psp_genl_adjoint_sweep (pass the same struct)                     */
} psp_genl_adj;
/* psp_genl_query_ul2 for a plan that runs the sweep: table_bytes grows by the table of (dt A)^T (a drift matrix only; behind
 * everything the forward and psp_genl_ul2_stage write, so those calls produce the same bytes), the LDS rule also counts the sweep's
 * images (four of the whole concatenation, three of the input blocks), waves_per_tile is the sweep's as well; writes
 * adj->drift_t_offset.  `ul2` may be NULL.  <0 as psp_genl_query_ul2, or: wrong struct_bytes, a stopping domain or a finite T,
 * base.adaptive = 0, another h than PSP_GH_QUAD, the orientation PSP_GENL_Z_SIGMA_T.  No GPU needed; reads no pointer of `adj`. */
int psp_genl_query_adj(const psp_genl_config* cfg, const psp_genl_coeffs* coeffs, const psp_genl_ul2* ul2, psp_genl_adj* adj,
                       psp_genl_sizes* out);
/* The sweep itself, between psp_genl_rollout_fwd* and psp_genl_rollout_bwd of the same cfg / coeffs / params / tables / path.
 * `ahat` and `ws`: the coefficient and tangent-weight arrays of psp_genl_rollout_bwd (written; distinct from adj->mu /
 * adj->resid_coeff). */
int psp_genl_adjoint_sweep(const psp_genl_config* cfg, const psp_genl_coeffs* coeffs, const psp_genl_adj* adj, const float* params,
                           float* tables, float* path, float* ahat, float* ws, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Solver.train with a DenseNet control (function_space.py:116-140: dense-concat layers, relu^2, weights (in, out)):
 *   time_approx='outer' (the constructor default, solver.py:88, 352-353): N nets DenseNet(d -> d), one per time step
 *                                                              -> per_step = 1, time_input = 0
 *   a DenseNet(d+1 -> d) swapped into z_n with time_approx='inner' (solver.py:142-162, 355: input [t, x])
 *                                                              -> per_step = 0, time_input = 1
 * Forward rollout (psp_dnet_rollout_fwd) and parameter gradient (psp_dnet_rollout_bwd, a hand-written kernel over the register
 * images the rollout leaves in psp_dnet_config.images_out).  Instances whose accumulator tiles do not fit a wave's
 * registers (psp_dnet_sizes.bwd_supported = 0: d = 256) get the rollout's row-major stores instead (px, pxi, r1_out, r2_out)
 * and the caller forms the same gradient with library GEMMs, see plan_dense_native.py.
 * base.d / base.H name the compiled instance (psp_dnet_instance_get; whole 16-blocks); d_real <= d, H_real <= H are
 * the net's sizes.  params = per_step ? N : 1 consecutive parameter sets in the DenseNet's registration order
 *     [W1 (di x H_real), b1, W2 ((di+H_real) x H_real), b2, W3 ((di+2 H_real) x d_real), b3],  di = d_real + time_input,
 * read with their real strides (no padded copy).  Problem vectors / matrices, x0 and supplied noise are padded to
 * base.d as for the other entry points.  Gradients through the state path and the relative-entropy loss run through
 * psp_dnet_adjoint_sweep (below) on the instances with bwd_supported = 1.
 * ------------------------------------------------------------------------------------------------ */
typedef struct psp_dnet_config {
    psp_hjb_config base;
    int32_t d_real, H_real;
    int32_t time_input;   /* 1: the net's input is [t, x] (time = column 0) */
    int32_t per_step;     /* 1: one parameter set per time step            */
    float* r1_out;        /* optional (N, K_local, H_real): relu(z1) and relu(z2) of every sample, row-major -- spares the   */
    float* r2_out;        /* gradient pass the recomputation of the two hidden layers (both NULL: not stored)                */
    float* images_out;    /* optional (psp_dnet_sizes.image_bytes): X_n, relu(z1), relu(z2) and the xi image as register images
                           * for psp_dnet_rollout_bwd; when set they REPLACE the row-major stores (px, pxi, r1_out, r2_out) */
    /* u_L2 log (solver.py:471-472, 491-494):  base.u_l2_out[k] = sum_n |-Z_n(X_n) - u*(X_{n+1}, t_n)|^2 dt  for three kinds of
     * reference control u*.  The log is on when base.u_ref is set (kind PSP_UL2_TABLE) or ul2_kind != 0; base.u_l2_out is then
     * required.  Every array is padded to base.d like the problem vectors.  (psp_hjb_config itself carries kind 0 only: the
     * narrow and wide families have no way to receive the other kinds.) */
    int32_t ul2_kind;     /* PSP_UL2_TABLE: base.u_ref = (N, d) table of u*(t_n), ul2_* unused;
                           * PSP_UL2_LINEAR: u*(x, t_n) = M_n x, ul2_tables = (N, d, d) row-major M_n, staged into the table
                           *   scratch once by psp_dnet_ul2_stage;
                           * PSP_UL2_GRID: u*_i(x, t_n) = table_{ul2_group[i]}[ul2_row[n], cell(x_i)] with the reference's index
                           *   arithmetic (problems.py:254-260): cell = floor((clamp(x, -xb, xhi) + xb) / dx) in fp32 with a true
                           *   division, lowered by two for the globally last trajectory (k_offset + k == K_global - 1), a negative
                           *   result counting from the end of the row (numpy indexing) */
    int32_t ul2_ntables;  /* PSP_UL2_GRID: G tables, each (ul2_nrows, ul2_ncols), consecutive in ul2_tables */
    int32_t ul2_nrows, ul2_ncols;
    const float* ul2_tables;
    const int32_t* ul2_group;  /* PSP_UL2_GRID: (d) table of every coordinate, in [0, G)                                 */
    const int32_t* ul2_row;    /* PSP_UL2_GRID: (N) row of step n, ceil(t_n / dt_ref) formed on the host, in [0, nrows) */
    float ul2_xb, ul2_dx; /* PSP_UL2_GRID: grid half-width and cell width (fp32 of the reference's values)              */
    float ul2_xhi;        /* PSP_UL2_GRID: upper clamp, fp32(xb - 2 dx) with xb - 2 dx formed in double as the reference does */
    int32_t ul2_reserved;
} psp_dnet_config;

enum { PSP_UL2_TABLE = 0, PSP_UL2_LINEAR = 1, PSP_UL2_GRID = 2 };

typedef struct psp_dnet_sizes {
    int64_t table_bytes;       /* scratch for the A-operand tables the call writes (L2-resident)   */
    int64_t fwd_partial_bytes;
    int64_t n_params_per_set;
    int32_t fwd_workgroups, reserved;
    /* hand-written backward (psp_dnet_rollout_bwd); bwd_supported = 0 when the instance's accumulators do not fit */
    int64_t image_bytes;       /* N x ceil(K/16) image blocks                                          */
    int64_t partial_bytes;     /* N x slices partial gradients of padded_params floats                 */
    int32_t bwd_supported, slices, padded_params, bwd_workgroups;
} psp_dnet_sizes;

int psp_dnet_instance_count(void);
int psp_dnet_instance_get(int32_t i, int32_t* d, int32_t* H);
int psp_dnet_query(const psp_dnet_config* cfg, psp_dnet_sizes* out);
int psp_dnet_terminal_reduce(const psp_dnet_config* cfg, const double* fwd_partial, double* sums_out, void* stream);
/* px, pxi: (N, K_local, d_real) stores of X_n and of the xi image (xi, or xi + sqrt(dt) Z when the forward process is
 * not adaptive: dL/dZ_n = w_k sqrt(dt) * image either way); written when base.store_path = 1.  tfeat: optional (N)
 * time feature per step (importance-sampling grids, utilities.py:296-299), NULL -> n * dt.  Outputs as for
 * psp_hjb_rollout_fwd / psp_hjb_rollout_eval; psp_dnet_terminal_reduce reduces fwd_partial (this family's own
 * workgroup count) to the global (sum D, sum D^2). */
/* u_L2 log, PSP_UL2_LINEAR: writes the gains cfg->ul2_tables into the table scratch `tables` in the layout the forward reads (behind
 * the rollout's own tables, which the forward and adjoint calls rewrite without touching this part).  Once per table buffer and set
 * of gains, before the first psp_dnet_rollout_fwd with ul2_kind = PSP_UL2_LINEAR; a no-op for the other kinds. */
int psp_dnet_ul2_stage(const psp_dnet_config* cfg, float* tables, void* stream);
int psp_dnet_rollout_fwd(const psp_dnet_config* cfg, const float* params, const float* x0, int32_t x0_stride,
                         const float* y0, const float* xi, uint64_t seed, uint32_t iter, const float* tfeat,
                         float* px, float* pxi, float* D_out, float* Fint_out, float* XN_out, float* Y_out,
                         double* fwd_partial, float* tables, void* stream);

/* Gradients THROUGH the state path for a DenseNet control (adaptive_forward_process=True with detach_forward=False -- the
 * reference's constructor defaults, solver.py:23-24, 451-469) and the relative-entropy loss (:179-180, 484-486): the
 * counterpart of psp_hjb_adjoint_sweep.  Call sequence per iteration:
 *     psp_dnet_rollout_fwd   with base.store_path = 2 (losses of Y_N - g(X_N)) or 3 (PSP_LOSS_REL_ENTROPY), images_out and
 *                            XN_out given
 *     [loss and per-trajectory weights mu_k = dL/dY_N[k], nu_k = dL/dZsum_N[k] from D on the caller's side]
 *     psp_dnet_adjoint_sweep reverse-time adjoint recursion per trajectory tile (csrc/hjbd_kernels.h: hjbd_adj_kernel, with the
 *                            Jacobian of the dense-concat net from the stored relu images); rewrites the xi slot of `images`
 *                            with dL/dZ_n / sqrt(dt)
 *     psp_dnet_rollout_bwd   with w = 1 for every trajectory
 *   XN : (K_local, base.d) terminal states;  mu, nu, wT as for psp_hjb_adjoint_sweep (nu / wT may be NULL);
 *   tables : the forward call's table scratch (the sweep rebuilds it with the transposed orientations). */
int psp_dnet_adjoint_sweep(const psp_dnet_config* cfg, const float* params, float* images, const float* XN,
                           const float* mu, const float* nu, const float* wT, float* tables, void* stream);

/* Parameter gradient of sum_{n,k} w_k sqrt(dt) image_n[k] . Z_n(X_n[k]) (= dL/dtheta for a detached forward process) from the
 * images the forward wrote (cfg->images_out).  w: per-trajectory weights dL/dD_k, zero padded to 16 * ceil(K_local/16).
 * partial: (N * slices, padded_params) -- per work item (time step, slice of its tiles) in the PADDED layout of the instance
 * (d x H etc., no time rows):  [W1 (d x H), b1 (H), W2 ((d+H) x H), b2, W3 ((d+2H) x d), b3 (d)];  the caller sums the slices of a
 * step, cuts the real rows / columns out and -- with time_input -- forms the time rows as sum_n t_n * (bias gradient of step n). */
int psp_dnet_rollout_bwd(const psp_dnet_config* cfg, const float* params, const float* images, const float* w,
                         float* partial, void* stream);

/* Gradient-variance diagnostic (Solver(compute_gradient_variance=m), reference solver.py:225-281) for a DenseNet control.
 * Trajectories are independent and net n sees one input per trajectory, so the per-trajectory gradient G_k of Y_N[k] with respect
 * to a layer of net n is rank one (activation row x delta row) and its SECOND moment over k is a sum of outer products of the
 * squared operands.  psp_dnet_rollout_bwd_sq takes the arguments and checks of psp_dnet_rollout_bwd and writes
 *     partial[item] = sum_k (w_k sqrt(dt) per-trajectory gradient)^2      (element-wise square, same padded layout and slices)
 * always on the fp32 MFMAs (base.mlp_dtype and base.range_flag are not read). */
int psp_dnet_rollout_bwd_sq(const psp_dnet_config* cfg, const float* params, const float* images, const float* w,
                            float* partial, void* stream);
/* psp_gradvar_finish reduces the slices of up to four such partial buffers, each (N * slices, padded_params), and combines the raw
 * moments in double.  With c the per-trajectory factor (moment: c = r = Y_N - g(X_N); log-variance: c = r - mean r),
 *     pS = S[c] = sum_k c_k G_k      pQ = Q[c] = sum_k c_k^2 G_k o G_k      pS2 = S[c^2]      pS1 = S[1]      csums = (sum c, sum c^2)
 * and B = gg (PSP_LOSS_MOMENT; the (N, n_params_per_set) gradient of g(X_N[0]), NULL -> 0 and pS2 may be NULL) or pS1 / K
 * (PSP_LOSS_LOG_VARIANCE; pS2 and pS1 required):
 *     sum f = 2 (S - B sum c)     sum f^2 = 4 (Q - 2 B S2 + B^2 sum c^2)     mean = sum f / K     var = (sum f^2 - (sum f)^2 / K) / (K - 1)
 * var is clamped at 0 before the root; rel = sqrt(var) / mean in fp32 with NaN -> 0 (inf and negative values stay).  gather_index:
 * (n_params_per_set) int64 padded position of every real parameter.  Outputs mean / var / rel: (N, n_params_per_set) fp32 in the
 * DenseNet's registration order; rel_mean_out: one float, the mean of rel; step_sums: scratch of N doubles.  csums is a DEVICE
 * pointer (no host sync).  One workgroup per step and one final reduction; plain stores, no atomics. */
int psp_gradvar_finish(const float* pS, const float* pQ, const float* pS2, const float* pS1, const float* gg,
                       const int64_t* gather_index, int32_t N, int32_t slices, int64_t padded_params, int64_t n_params_per_set,
                       int32_t K, int32_t loss_kind, const double* csums, float* mean_out, float* var_out, float* rel_out,
                       double* step_sums, float* rel_mean_out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Solver.train with a linear, affine or constant control per time step (appended in 0.4.0, no version bump; csrc/aff_kernels.h):
 * time_approx='outer' with z_n a list of function_space.Linear / Affine / Constant (reference function_space.py:24-63; the
 * notebook `Ornstein-Uhlenbeck - quadratic costs - linear ansatz.ipynb`).  The kernels see the EFFECTIVE maps only,
 *     Z_n(x) = M_n x + c_n,
 * and return (dM_n, dc_n); what lies between them and the modules' parameters (Linear: M = Q^-1 B^T F) is the caller's.
 * base.d names the compiled bucket (psp_aff_instance_get: 16, 32, 64), d_real <= base.d the real dimension; EVERY array is zero
 * padded to base.d: maps (N, d, d) row-major, shifts (N, d), problem vectors / matrices, x0, supplied noise, the u_L2 reference.
 * base.H must be 0 and base.mlp_dtype PSP_MLP_FP32 (fp32 arithmetic only; -3 otherwise); base.u_ref, iter_dev and range_flag are
 * not read.  Per step the rollout is that of psp_dnet_rollout_fwd (solver.py:449-486), every coefficient kind of psp_hjb_config,
 * the same Philox counters, (sum D, sum D^2) per workgroup in fp64.
 * u_L2 log: on when base.u_l2_out is set;  u_l2_out[k] = sum_n |-Z_n(X_n) - u*(X_{n+1}, t_n)|^2 dt  with ul2_kind
 *   PSP_UL2_TABLE: ul2_ref = (N, d) u*(t_n);  PSP_UL2_LINEAR: ul2_ref = (N, d, d) gains, u* = M*_n x;  PSP_UL2_GRID: -3.
 * Path store (base.store_path 1 / 2 / 3, images as for psp_dnet_*): N x K_local rows of 2 d floats, [X_n | image].
 * Call sequence per iteration:
 *     psp_aff_rollout_fwd -> psp_aff_terminal_reduce -> [weights from D on the caller's side]
 *     -> psp_aff_adjoint_sweep (store_path 2 / 3 only: gradients through the state path, relative entropy attached)
 *     -> psp_aff_rollout_bwd -> [sum the slices, chain rule, all-reduce] -> psp_adam_step
 * ------------------------------------------------------------------------------------------------ */
typedef struct psp_aff_config {
    psp_hjb_config base;
    int32_t struct_bytes;     /* sizeof(psp_aff_config): checked by the library (this struct is not in psp_abi_struct_sizes*) */
    int32_t d_real;
    int32_t has_matrix;       /* 1: the control has maps M_n (Linear, Affine)                                                 */
    int32_t has_bias;         /* 1: the control has shifts c_n (Affine, Constant); at least one of the two                    */
    int32_t ul2_kind;         /* PSP_UL2_TABLE | PSP_UL2_LINEAR, read when base.u_l2_out is set                               */
    int32_t reserved;
    const float* ul2_ref;     /* the kind's reference data (above), DEVICE                                                    */
} psp_aff_config;

typedef struct psp_aff_sizes {
    int64_t path_bytes;        /* N x K_local x 2 d floats (0 when store_path = 0)                                            */
    int64_t fwd_partial_bytes; /* per-workgroup (sum D, sum D^2) fp64 pairs                                                   */
    int64_t partial_bytes;     /* N x slices partial gradients of padded_params floats                                       */
    int32_t fwd_workgroups, fwd_threads;
    int32_t slices;            /* trajectory slices per time step of psp_aff_rollout_bwd                                      */
    int32_t padded_params;     /* d * d + d: [dM (d x d row-major) | dc (d)] in the bucket's width                            */
    int32_t bwd_workgroups;
    int32_t lds_bytes;         /* the forward workgroup's LDS (the sweep's is smaller)                                        */
} psp_aff_sizes;

int psp_aff_instance_count(void);
int psp_aff_instance_get(int32_t i, int32_t* d);
/* Every check the entry points below make of the config, and the sizes, without a launch (no GPU needed).  -1 invalid argument
 * (wrong struct_bytes, enum out of range, missing pointer), -2 no bucket of that width, -3 H / mlp_dtype / PSP_UL2_GRID / LDS. */
int psp_aff_query(const psp_aff_config* cfg, psp_aff_sizes* out);
/* maps: (N, d, d) or NULL (!has_matrix); shifts: (N, d) or NULL (!has_bias); x0, x0_stride, y0, xi, seed, iter, D_out, XN_out,
 * Y_out as for psp_hjb_rollout_fwd (XN_out rows are base.d floats); path: path_bytes or NULL with store_path = 0. */
int psp_aff_rollout_fwd(const psp_aff_config* cfg, const float* maps, const float* shifts, const float* x0, int32_t x0_stride,
                        const float* y0, const float* xi, uint64_t seed, uint32_t iter, float* path, float* D_out, float* XN_out,
                        float* Y_out, double* fwd_partial, void* stream);
int psp_aff_terminal_reduce(const psp_aff_config* cfg, const double* fwd_partial, double* sums_out, void* stream);
/* Gradients THROUGH the state path (adaptive_forward_process=True with detach_forward=False) and the attached relative entropy;
 * mu, nu, wT as for psp_hjb_adjoint_sweep (nu / wT may be NULL; store_path 3 needs nu and reads no mu-term: mu must be 0).  With
 * lambda_N = wT grad g(X_N), for n = N-1 .. 0:
 *     Lam     = lambda + (mu + nu) dt grad f(X_{n+1})
 *     delta_n = mu (xi_{n+1} sqrt(dt) - Z_n dt) + nu Z_n dt - dt B^T Lam
 *     lambda  = Lam + dt J_b(X_n)^T Lam + M_n^T delta_n
 * and the image slot of step n in `path` becomes delta_n / sqrt(dt): psp_aff_rollout_bwd then runs with w = 1. */
int psp_aff_adjoint_sweep(const psp_aff_config* cfg, const float* maps, float* path, const float* XN, const float* mu,
                          const float* nu, const float* wT, void* stream);
/* partial[(n * slices + s)] = [sum_k delta_{n,k} X_{n,k}^T | sum_k delta_{n,k}] over the trajectories of slice s, with
 * delta_{n,k} = w_k sqrt(dt) image_{n,k}; w: (K_local).  Every thread sums sequentially: equal arguments give equal bits. */
int psp_aff_rollout_bwd(const psp_aff_config* cfg, const float* path, const float* w, float* partial, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Importance-sampling evaluation under the problem's REFERENCE control u* or under no control (utilities.do_importance_sampling_me,
 * reference utilities.py:287-359, with control='true' and simulate_naive=True; csrc/hjbe_kernels.h).  Forward only, one lane per
 * trajectory, no net.  Per step n (t_n = n dt), from X_0 = x0:
 *     u      = u*(X_n, t_n)            (kind PSP_ISC_NONE: u = 0, the naive estimator)
 *     X_n+1  = X_n + (b(X_n) + sigma u) dt + sigma xi_n+1 sqrt(dt)
 *     logw  += -f(X_n+1) dt - u.xi_n+1 sqrt(dt) - |u|^2 dt / 2
 * and at the end logw -= g(X_N).  fp32, every sum sequential in n; the elementwise drift and sigma kinds round the update op by op
 * as the reference's torch ops do (no fma contraction).  Coefficient kinds and pointers as in psp_hjb_config (d-sized, unpadded).
 * The u* fields mirror psp_dnet_config.ul2_*; the kinds:
 *   PSP_ISC_TABLE : u_ref = (N, d) table of u*(t_n), independent of x (LLGC)
 *   PSP_ISC_LINEAR: u_ref = (N, d, d) row-major gains M_n, u* = M_n x (LQGC)
 *   PSP_ISC_GRID  : u_ref = (u_ntables, u_nrows, u_ncols) tables, u*_i = table_{u_group[i]}[u_row[n], cell(x_i)] with the index
 *                   arithmetic of psp_dnet_config.ul2_kind = PSP_UL2_GRID (the last GLOBAL trajectory, k_offset + k = K_global - 1,
 *                   lowered by two); u_row must hold rows < u_nrows for every step (the kernel clamps)
 * ------------------------------------------------------------------------------------------------ */
enum { PSP_ISC_NONE = 0, PSP_ISC_TABLE = 1, PSP_ISC_LINEAR = 2, PSP_ISC_GRID = 3 };

typedef struct psp_is_config {
    int32_t d;            /* state dimension: psp_is_rollout 1 <= d <= 64 (the compiled buckets 1, 4, 16, 32, 64);
                           * psp_isw_rollout 1 <= d <= PSP_ISW_MAX_D (blocks of 16 features, buckets of 4, 8, 12, 16 blocks)  */
    int32_t K_local;      /* trajectories of this call                                                                        */
    int32_t N;            /* time steps, ceil(T / delta_t) (utilities.py:299)                                                 */
    int32_t control_kind; /* PSP_ISC_*                                                                                        */
    int64_t K_global;     /* trajectories over all calls (the GRID kind's last trajectory)                                    */
    int64_t k_offset;     /* global index of local trajectory 0 (Philox counter, last trajectory)                             */
    float dt, sqrt_dt;    /* fp32 step and fp32(sqrt(delta_t))                                                                */
    int32_t drift_kind, sigma_kind, runcost_kind, term_kind;
    int32_t noise_mode;   /* PSP_NOISE_SUPPLIED: xi (N+1, K_local, d), slice n+1 drives step n; PSP_NOISE_PHILOX: the counters of
                           * psp_hjb_rollout_eval (the same (seed, iter) draws the same increments)                            */
    int32_t dwell_form;   /* PSP_DRIFT_DOUBLE_WELL rounding: 0 = -(4 kappa_i) (x (x^2 - 1)) (DoubleWell_multidim),
                           * 1 = -((4 kappa) x) (x^2 - 1) (DoubleWell)                                                        */
    float sigma_scale;    /* PSP_SIGMA_SCALED_IDENTITY                                                                        */
    int32_t reserved;
    const float* x0;      /* (d) initial state                                                                                */
    const float* drift;
    const float* sigma;
    const float* runcost;
    const float* term;
    const float* u_ref;   /* the kind's u* data (above); NULL for PSP_ISC_NONE                                                */
    const int32_t* u_group; /* PSP_ISC_GRID: (d) table of every coordinate, in [0, u_ntables)                                 */
    const int32_t* u_row;   /* PSP_ISC_GRID: (N) table row of step n, ceil(t_n / dt_ref) formed on the host                   */
    int32_t u_ntables, u_nrows, u_ncols;
    float u_xb, u_dx, u_xhi; /* PSP_ISC_GRID: as psp_dnet_config.ul2_xb / ul2_dx / ul2_xhi                                    */
} psp_is_config;

/* logw_out: (K_local) per-trajectory log-weight -int f dt - g(X_N) - int u.dW - 0.5 int |u|^2 dt (the last two terms are zero for
 * PSP_ISC_NONE); XN_out: optional (K_local, d) final states.  -1 invalid argument, -2 d outside the native range, -3 u* tables that
 * do not fit the LDS. */
int psp_is_rollout(const psp_is_config* cfg, const float* xi, uint64_t seed, uint32_t iter, float* logw_out, float* XN_out,
                   void* stream);
/* Every check psp_is_rollout makes of the config, without a launch (no GPU needed); *lds_bytes = the workgroup's LDS. */
int psp_is_query(const psp_is_config* cfg, int32_t* lds_bytes);
/* sizeof(psp_is_config) (added in 0.4.0). */
int psp_abi_struct_sizes3(int32_t out[1]);

/* ------------------------------------------------------------------------------------------------
 * The same rollout for wide states (appended in 0.4.0, no version bump; csrc/hjbew_kernels.h): the recursion, the kinds and the
 * psp_is_config above, for 1 <= d <= PSP_ISW_MAX_D (d <= 64 included, so that the two kernels can be held against each other).
 * One wave owns a tile of 16 trajectories with the state in the accumulator layout of v_mfma_f32_16x16x4_f32; the dense
 * products A X, B (u dt + xi sqrt(dt)) and M_n X are fp32 MFMAs on tables a small kernel of the same call tiles into `tables`.
 * The elementwise kinds round the state update op by op as psp_is_rollout does (X_N is bit-equal between the two there); the
 * sums over features are reduced in another fixed order, so logw agrees to fp32 rounding, not bit for bit.  Equal arguments
 * give equal bits.  d = 512 does not fit one wave's registers without scratch, hence PSP_ISW_MAX_D = 256.
 * With P = 64 ceil(d / 64) padded features,
 *   table_bytes = 4 (5 P + [drift DENSE] P^2 + [sigma DENSE] P^2 + (TABLE: N P | LINEAR: N P^2 | else 0)).
 * ------------------------------------------------------------------------------------------------ */
#define PSP_ISW_MAX_D 256

typedef struct psp_isw_sizes {
    int32_t struct_bytes; /* in: sizeof(psp_isw_sizes), checked by psp_isw_query                                              */
    int32_t lds_bytes;    /* the workgroup's LDS: the GRID kind's rows of one step, else 0                                    */
    int64_t table_bytes;  /* caller-owned scratch psp_isw_rollout writes before it reads (the formula above)                  */
    int32_t workgroups;   /* ceil(ceil(K_local / 16) / 4): four 16-trajectory tiles, one per wave                             */
    int32_t max_d;        /* PSP_ISW_MAX_D of the library                                                                     */
} psp_isw_sizes;

/* Every check psp_isw_rollout makes of the config, without a launch (no GPU needed).  -1 invalid argument (a wrong
 * struct_bytes, a kind out of range, K_global < k_offset + K_local, a pointer the kind needs missing), -2 d outside
 * 1 .. PSP_ISW_MAX_D, -3 GRID rows that do not fit the LDS; psp_last_error() names the reason. */
int psp_isw_query(const psp_is_config* cfg, psp_isw_sizes* sizes);
/* As psp_is_rollout; tables: table_bytes of scratch on the device (16-byte aligned), rewritten by every call. */
int psp_isw_rollout(const psp_is_config* cfg, const float* xi, uint64_t seed, uint32_t iter, float* tables, float* logw_out,
                    float* XN_out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Rollout in the sigma basis (appended in 0.4.0, no version bump).  For a constant invertible sigma = B a caller may hand the
 * rollout entry points the equivalent problem in X~ = B^-1 X -- drift B^-1 A B, PSP_SIGMA_IDENTITY, terminal vector B^T alpha,
 * x0 = B^-1 x0 -- which needs ONE d x d product per step instead of two.  Z, Y, D, h1, h2 and the noise are unchanged; the net
 * sees W1x X = (W1x B) X~.  Two launches per iteration keep parameters and gradient in the original basis (a few workgroups
 * each, fp32 fmaf chains in a fixed order, capturable, no host sync); d, H are the kernel instance's (padded) shape, B is (d, d)
 * row-major, W1 is the first H (d + 1) entries of the flat layout with the time input in column 0 of every row:
 *   psp_hjb_basis_params : params_out = params with W1[:, 1:] <- W1[:, 1:] B; every other of the n_params entries is copied
 *                          (params_out == params: in place)
 *   psp_hjb_basis_grad   : grad's W1[:, 1:] block <- (that block) B^T, in place, after psp_hjb_rollout_bwd and before the
 *                          gradient all-reduce / psp_adam_step
 * Between the two, every buffer of the iteration is in the sigma basis: the path store holds X~, and psp_hjb_rollout_bwd leaves
 * dW~1x, not dW1x.  A caller that takes these buffers from the Python plan (HjbNativePlan: cfg, path store, grad_k) and drives
 * psp_hjb_rollout_bwd itself must check plan.state_basis and apply psp_hjb_basis_grad when it reads 'sigma'.
 * -1 invalid argument, -3 B does not fit 64 KiB of LDS (d <= 112 does).
 * ------------------------------------------------------------------------------------------------ */
int psp_hjb_basis_params(const float* params, float* params_out, const float* B, int32_t d, int32_t H, int64_t n_params,
                         void* stream);
int psp_hjb_basis_grad(float* grad, const float* B, int32_t d, int32_t H, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The K_test_log diagnostic on the device (appended in 0.4.0, no version bump; csrc/genl_eval_kernels.h): the Monte-Carlo error
 * of a value net against the problem's closed-form solution on K_points fresh points of the domain (utilities.compute_test_error,
 * reference utilities.py:440-472; solver.py:1193-1197 / :821-825) -- points drawn, V and v_true evaluated and the statistics
 * reduced by two kernels, no host sync, nothing allocated, capturable.  The net is any dense-concat net psp_genl_* takes.
 * Points (PSP_TSAMPLE_*): supplied by the caller, or drawn from Philox4x32-7 on a stream no training kernel uses:
 *     key = (seed & 0xffffffff, (seed >> 32) ^ 0x54455354), counter = (k_offset + k, c1, c2, iter)
 *     c1 = 0, c2 = 4 b + q : features 16 b + 4 r + q, r = 0..3 -- N(0, 1) by two Box-Muller pairs (BALL, ANNULUS) or the 24-bit
 *                            uniforms ((r >> 8) + 1/2) 2^-24 (BOX)
 *     c1 = 1, c2 = 0       : output 0 = radial uniform u, output 1 = time uniform u_t; t = u_t T (nets with a time input)
 *     BALL    x = bound_b g / |g| u^(1/d)                                   ('sphere', 'unbounded')
 *     ANNULUS the ball of radius bound_b; points with |x| <= bound_a are rejected and not counted  ('two_spheres')
 *     BOX     x = (bound_b - bound_a) u + bound_a                           ('square', 'unbounded_square')
 * v_true (PSP_VTRUE_*), fp32, from r2 = |x|^2 and t:
 *     EXP        exp(p0 r2 + p1 t)                                          (exponential on the ball; parabolic: p1 = 1)
 *     QUAD       r2 + p0 (p1 - t)                                           (HeatEquation p0 = 2 d, p1 = T; QuadraticOnBox p0 = 0)
 *     COMMITTOR  (a^2 - r^(2-d) a^d) / (a^2 - c^(2-d) a^d), p0 = a, p1 = c, p2 = d
 *   and, in a group of its own from 16 on, the forms the kernel also hands the coordinates x_0, x_1:
 *     LOGQ       log((r2 + 1) / p0)                                         (QuadraticGradient, p0 = d)
 *     SINPROD    sin(p0 x_0) sin(p1 x_1)                                    (Helmholtz, p0 = a_1 pi, p1 = a_2 pi; d >= 2)
 *     SINSUM     sin(p0 x_0) + p2 sin(p1 x_0)                               (Oscillations, p0 = 2 pi, p1 = a pi, p2 = 0.1)
 *     SINR2      sin(pi r2)                                                 (SinNorm2)
 * log_out[4 slot .. 4 slot + 3] = sum e^2, sum |e|, sum |e| / v_true, count over the kept points, e = v_true - V, in fp64
 * (per-workgroup partials summed in a fixed order: equal arguments give bit-identical output).
 * ------------------------------------------------------------------------------------------------ */
enum { PSP_TSAMPLE_SUPPLIED = 0, PSP_TSAMPLE_BALL = 1, PSP_TSAMPLE_ANNULUS = 2, PSP_TSAMPLE_BOX = 3 };
enum { PSP_VTRUE_EXP = 0, PSP_VTRUE_QUAD = 1, PSP_VTRUE_COMMITTOR = 2,
       PSP_VTRUE_LOGQ = 16, PSP_VTRUE_SINPROD = 17, PSP_VTRUE_SINSUM = 18, PSP_VTRUE_SINR2 = 19 };   /* 3 .. 15 are no kind */

typedef struct psp_genl_eval_config {
    int32_t d;                /* state dimension                                                                                 */
    int32_t has_time, n_hidden, widths[4], activation, linear_layout, time_first;   /* the net: as in psp_genl_config            */
    float time_scale;
    int32_t K_points;         /* test points of this call                                                                        */
    int32_t sample_kind;      /* PSP_TSAMPLE_*                                                                                   */
    int64_t k_offset;         /* global index of point 0 (Philox counter); k_offset + K_points <= 2^32                           */
    float bound_a, bound_b;   /* BALL: (unused, R); ANNULUS: (r1, r2); BOX: (l, r)                                               */
    float T;                  /* sampled points of a net with a time input: t ~ U(0, T)                                          */
    int32_t vtrue_kind;       /* PSP_VTRUE_*                                                                                     */
    float vtrue_par[4];
    int32_t log_slots;        /* rows of log_out; a slot outside [0, log_slots) is dropped by the kernel, never written          */
    int32_t reserved;
} psp_genl_eval_config;

typedef struct psp_genl_eval_sizes {
    int64_t table_bytes;      /* scratch for the operand tables (rebuilt by every call)                                          */
    int64_t partial_bytes;    /* 4 doubles per workgroup                                                                         */
    int64_t n_params;         /* registration order W_1, b_1, .., W_out, b_out                                                   */
    int32_t workgroups;       /* ceil(K_points / 16): one 16-point tile each                                                     */
    int32_t waves_per_tile;   /* 1 or 8: one wave for the nets psp_genl_query gives one wave at K_local = K_points, else 8
                               * (never the rollout's 4-wave refinement for large batches)                                       */
    int32_t lds_bytes;        /* the activation image alone                                                                      */
    int32_t reserved;
} psp_genl_eval_sizes;

/* Every check psp_genl_test_error makes of the config, and the sizes, without a launch (no GPU needed).  -1 invalid argument,
 * -2 net outside the limits of psp_genl_query, -3 LDS. */
int psp_genl_eval_query(const psp_genl_eval_config* cfg, psp_genl_eval_sizes* out);
/* Rebuilds the operand tables from `params`, then launches the evaluation and the reduction.  x (K_points, d) / t (K_points):
 * the points of PSP_TSAMPLE_SUPPLIED (t with a time input), NULL otherwise.  slot_dev: optional DEVICE uint32 read by the
 * reduction kernel as the slot (a psp_iter_state.iter pointer is the intended use); NULL: `slot`.  Optional per-point dumps
 * (NULL: not written): x_out (K_points, d), t_out, v_out, vtrue_out (K_points) fp32, keep_out (K_points) int32. */
int psp_genl_test_error(const psp_genl_eval_config* cfg, const float* params, const float* x, const float* t, uint64_t seed,
                        uint32_t iter, float* tables, double* partial, double* log_out, int32_t slot, const uint32_t* slot_dev,
                        float* x_out, float* t_out, float* v_out, float* vtrue_out, int32_t* keep_out, void* stream);
/* sizeof(psp_genl_eval_config), sizeof(psp_genl_eval_sizes). */
int psp_abi_struct_sizes4(int32_t out[2]);

/* ------------------------------------------------------------------------------------------------
 * Multi-GPU: one process per GPU, trajectories sharded in contiguous blocks, parameters replicated.
 * Per iteration two in-place SUM all-reduces on the caller's stream: (sum D, sum D^2) after psp_hjb_terminal_reduce
 * (2 x fp64; the log-variance loss needs the GLOBAL mean) and the flat gradient after psp_hjb_rollout_bwd (n_params
 * fp32), then the same psp_adam_step on every rank.  The reference has no distributed code; these entry points are
 * what a C / ctypes consumer of this library uses instead of torch.distributed.  They drive RCCL (librccl.so.1 is
 * bound at first use, so the library loads on machines without it): both messages are latency-bound (16 B, 69 KB at
 * d=100), far from the per-link xGMI bandwidth.
 *   psp_comm_unique_id : rank 0 creates the 128-byte id and hands it to the other ranks by any host-side means
 *   psp_comm_init      : collective over all ranks, after hipSetDevice; *comm_out is an ncclComm_t
 *   psp_allreduce      : in-place SUM of n elements (dtype PSP_DT_F32 / PSP_DT_F64), asynchronous on `stream`
 * ------------------------------------------------------------------------------------------------ */
#define PSP_COMM_ID_BYTES 128
enum { PSP_DT_F32 = 0, PSP_DT_F64 = 1 };
int psp_comm_unique_id(unsigned char id_out[PSP_COMM_ID_BYTES]);
int psp_comm_init(void** comm_out, int32_t nranks, int32_t rank, const unsigned char id[PSP_COMM_ID_BYTES]);
int psp_comm_destroy(void* comm);
int psp_allreduce(void* buf, int64_t n, int32_t dtype, void* comm, void* stream);

/* ------------------------------------------------------------------------------------------------
 * PINN loss (appended in 0.4.0, no version bump; csrc/pinn_kernels.h): GeneralSolver.train_PINN / EllipticSolver.train_PINN
 * (reference solver.py:1208-1323, :828-931).  For a dense-concat value net (the nets psp_genl_query takes) and K points,
 *     R_k = [dV/dt] + s^2/2 Laplace_x V + b(x) . grad_x V + h(x, V, s grad_x V)            s = sigma_scale
 * by forward-Laplacian propagation (value, one tangent per input column and a Laplacian row through the net: no nested
 * differentiation), and the parameter gradient of any loss of R by the hand-written adjoint of that propagation:
 *     psp_pinn_residual -> [host: loss, rbar = dLoss/dR: 2 a0 R / K, or 2 a0 (R - mean R) / (K - 1) for the variance] ->
 *     psp_pinn_backward -> [+ the K_boundary-sized terms by autograd] -> psp_adam_step
 * Flat parameters: registration order W_1, b_1, .., W_out, b_out; net input [x] or [x, t].  Every product is fp32 MFMA.
 *
 * A dense constant sigma B (sigma_kind = PSP_GENL_SIGMA_DENSE; EllipticSolver(full_hessian=True)): the second-order term is
 *     1/2 trace(B B^T Hess_x V) = 1/2 sum_j dirs_j^T (Hess_x V) dirs_j          for any table with sum_j dirs_j dirs_j^T = B B^T
 * (the caller factors B B^T; rank(B B^T) <= d rows suffice).  The propagation is linear in its directions, so the kernels seed
 * n_dirs further tangent rows with the table's rows (time column 0) instead of unit vectors and count those in the Laplacian row;
 * sigma_scale is not read, the scale sits in the directions.  The unit directions e_0 .. e_{n_in-1} that give grad V and dV/dt
 * run first and are no longer counted; the library leaves them out where nothing reads grad V (drift_kind = PSP_DRIFT_ZERO,
 * has_time = 0; every h accepted here reads x and V only).  PSP_GH_QUAD, which reads z = B^T grad V, is refused (-1).
 * ------------------------------------------------------------------------------------------------ */
typedef struct psp_pinn_config {
    int32_t d, K;             /* state dimension, points of this call                                                          */
    int32_t has_time;         /* 1: net input [x, t] and R carries dV/dt (GeneralSolver); 0: [x] (EllipticSolver)               */
    int32_t n_hidden;         /* L, 1 .. 4                                                                                      */
    int32_t widths[4];        /* H_1 .. H_L, each <= 128; d + has_time <= 112                                                   */
    int32_t activation;       /* PSP_ACT_*                                                                                      */
    int32_t linear_layout;    /* 0: weights stored (in, out) (DenseNet); 1: (out, in) (nn.Linear, DenseNet_tanh)                */
    int32_t drift_kind;       /* PSP_DRIFT_ZERO, PSP_DRIFT_DIAG or PSP_DRIFT_DOUBLE_WELL                                       */
    int32_t h_kind;           /* PSP_GH_ZERO .. PSP_GH_EXPBALL_SIN_FULL, as psp_gen_config.h_kind; h must not read t
                               * (h_par[3] = 0; psp_pinn_pairs_* below take one that does); PSP_GH_EXPBALL_SIN_FULL on either
                               * sigma_kind; no PSP_GH_QUAD with _DENSE.  PSP_GH_AFFINE_EXP and PSP_GH_SINE_SOURCE (h_par = p0 ..
                               * p3: no time term; refused by psp_pinn_pairs_*; AFFINE_EXP with p2 != 0 reads z: not with _DENSE);
                               * PSP_GH_SINNORM2 is not built here                                                               */
    int32_t sigma_kind;       /* PSP_GENL_SIGMA_SCALED: sigma = s I, the Laplacian; PSP_GENL_SIGMA_DENSE: the table `dirs`       */
    int32_t n_dirs;           /* PSP_GENL_SIGMA_DENSE: rows of `dirs`, 1 .. d; ignored with _SCALED                             */
    float sigma_scale;        /* s (PSP_GENL_SIGMA_SCALED)                                                                      */
    float h_par[4];           /* PSP_GH_EXPBALL_*: al, d, e, tau (= 0; any tau in psp_pinn_pairs_*)                            */
    float reserved_f;
    const float* drift;       /* DOUBLE_WELL: kappa (d); DIAG: a (d); DEVICE; else NULL                                         */
    const float* dirs;        /* PSP_GENL_SIGMA_DENSE: (n_dirs, d) row-major, fp32, DEVICE; NULL there is -4; else ignored      */
} psp_pinn_config;

typedef struct psp_pinn_sizes {
    int64_t n_params;
    int64_t scratch_bytes;        /* V, the Laplacian parts, grad V and the adjoint's seed coefficients of the K points:
                                   * written by psp_pinn_residual, read by psp_pinn_backward.  Layout, in floats, for the K of
                                   * the call (n_in = d + has_time): V (K), Laplacian parts (K, dir_blocks), grad V (K, n_in),
                                   * dR/dV (K), dR/d grad V (K, n_in) = K (2 + dir_blocks + 2 n_in) floats; a larger buffer
                                   * is left untouched behind them (the kernel tests read the first three).
                                   * PSP_GENL_SIGMA_DENSE: V (K), Laplacian parts (K, dir_blocks), grad V (K, n_grad), dR/dV (K),
                                   * dR/d grad V (K, n_grad) = K (2 + dir_blocks + 2 n_grad) floats, n_grad = 0 where the unit
                                   * directions are left out (see above), else n_in                                             */
    int64_t grad_partial_bytes;   /* per-workgroup partial gradients of psp_pinn_backward                                       */
    int32_t dir_blocks;           /* blocks of 14 directions per point: a tile is (point, block).  Directions: the n_in input
                                   * columns; PSP_GENL_SIGMA_DENSE: n_grad + n_dirs                                              */
    int32_t tiles;
    int32_t bwd_workgroups;
    int32_t lds_fwd_bytes, lds_bwd_bytes;
    int32_t reserved;
} psp_pinn_sizes;

/* Every check of a psp_pinn_config and the sizes, without a launch (no GPU needed; `dirs` is only tested for NULL).  -1 invalid
 * argument (n_dirs outside 1 .. d, PSP_GH_QUAD with a table, K * dir_blocks above 2^24, ..), -2 net outside the limits of
 * psp_genl_query, -3 LDS, -4 a dense sigma without its table. */
int psp_pinn_query(const psp_pinn_config* cfg, psp_pinn_sizes* out);
/* x (K, d), t (K; NULL without a time input) -> R_out (K); `scratch`: psp_pinn_sizes.scratch_bytes. */
int psp_pinn_residual(const psp_pinn_config* cfg, const float* params, const float* x, const float* t, float* scratch,
                      float* R_out, void* stream);
/* grad_out (n_params) = sum_k rbar_k dR_k/dtheta, for the SAME cfg / params / x / t / scratch as the psp_pinn_residual call
 * before it.  grad_partial (psp_pinn_sizes.grad_partial_bytes) is summed in a fixed order. */
int psp_pinn_backward(const psp_pinn_config* cfg, const float* params, const float* x, const float* t, const float* scratch,
                      const float* rbar, float* grad_partial, float* grad_out, void* stream);
/* sizeof(psp_pinn_config), sizeof(psp_pinn_sizes). */
int psp_abi_struct_sizes5(int32_t out[2]);

/* ------------------------------------------------------------------------------------------------
 * PINN loss with an h that reads t (appended in 0.4.0, no version bump; csrc/pinn_kernels.h): the reference hands h the times
 * as a (K, 1) column (solver.py:1284-1285), so for PSP_GH_EXPBALL_SQ / PSP_GH_EXPBALL_SIN with tau = h_par[3] != 0 the residual
 * is a (K, K) matrix over (time i, sample j) and the loss its mean square:
 *     R[i, j] = A_j + nl(exp(2 al |x_j|^2 + 2 tau t_i) - y_j^2)       nl = identity (_SQ) or sin (_SIN), y_j = V(x_j, t_j)
 *     A_j     = dV/dt_j + s^2/2 Laplace_x V_j + b . grad_x V_j - y_j lin_j,    lin_j = 2 al (2 al |x_j|^2 + dd) + e
 *     loss    = alpha0 / K^2 sum_ij R[i, j]^2
 * Everything that passes through the net is per sample, so the gradient is sum_j (rho_j dA_j/dtheta + nu_j dy_j/dtheta) with
 *     rho_j = 2 alpha0 / K^2 sum_i R[i, j],      nu_j = 2 alpha0 / K^2 sum_i R[i, j] nl'(arg_ij) (-2 y_j):
 *     psp_pinn_pairs_residual -> psp_pinn_pairs_reduce -> psp_pinn_pairs_backward(rbar = rho, vadd = nu) -> psp_adam_step
 * Nothing is read on the host.  Every sum has a fixed order (lane partials over i, a butterfly over the 64 lanes, the K
 * per-sample sums of squares in index order in double; no atomics): the same bits on every run.
 * psp_pinn_config and psp_pinn_sizes are the ones above, the scratch has the same layout and size; its dR/dV slot holds
 * dA/dV = -lin_j.  The three entry points above keep refusing h_par[3] != 0; these take any tau, and with tau = 0 every h_kind
 * (R[i, j] = R_j then, and psp_pinn_pairs_backward with vadd = NULL is psp_pinn_backward).
 * Limits beyond those of psp_pinn_query (-1): has_time = 1, PSP_GENL_SIGMA_SCALED, tau != 0 only with _SQ / _SIN, and
 * K <= 16384 -- a condition, not a measurement: the pair kernel visits K^2 <= 2.7e8 pairs per call and stages the K times in
 * 4 K <= 64 KiB of LDS (the reference materialises the (K, K) matrix).
 * ------------------------------------------------------------------------------------------------ */
/* Every check and the sizes without a launch (no GPU needed); pair_work_bytes_out: the buffer psp_pinn_pairs_reduce needs. */
int psp_pinn_pairs_query(const psp_pinn_config* cfg, psp_pinn_sizes* sizes_out, int64_t* pair_work_bytes_out);
/* x (K, d), t (K) -> A_out (K), the residual without its pair term; `scratch`: psp_pinn_sizes.scratch_bytes. */
int psp_pinn_pairs_residual(const psp_pinn_config* cfg, const float* params, const float* x, const float* t, float* scratch,
                            float* A_out, void* stream);
/* The K x K pairs of the SAME cfg / x / t / scratch / A as the psp_pinn_pairs_residual call before it -> loss_out (1 float),
 * rho_out (K), nu_out (K), all DEVICE; pair_work: pair_work_bytes of psp_pinn_pairs_query. */
int psp_pinn_pairs_reduce(const psp_pinn_config* cfg, const float* x, const float* t, const float* scratch, const float* A,
                          float alpha0, void* pair_work, float* loss_out, float* rho_out, float* nu_out, void* stream);
/* grad_out (n_params) = sum_j (rbar_j dA_j/dtheta + vadd_j dy_j/dtheta); vadd (K) may be NULL (= 0).  grad_partial as in
 * psp_pinn_backward. */
int psp_pinn_pairs_backward(const psp_pinn_config* cfg, const float* params, const float* x, const float* t, const float* scratch,
                            const float* rbar, const float* vadd, float* grad_partial, float* grad_out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Statistics of the loss estimators (appended in 0.4.0, no version bump; csrc/lstat_kernels.h): what
 * utilities.loss_relative_errors reduces the chunks of a forward-only rollout with (the reference's notebook
 * `Compare relative errors of losses.ipynb`).  Per trajectory, from fp32 Y = Y_N and D = Y_N - g(X_N), in double
 * (g = Y - D is exact there, exp is the double-precision one):
 *     terminal exp(-g)     cross_entropy Y exp(-g)     cross_entropy_detach Y exp(-g + Y)
 *     cross_entropy_detach_selection: the same, only samples with |v| < 100 (NaN and inf are not selected)
 *     moment D^2           log_variance: D up to its fourth central moment
 * `state` is a DEVICE buffer of psp_loss_stats_state_bytes() bytes, 8-byte aligned, ZEROED by the caller before the first
 * chunk.  It holds mergeable moments (count, mean, M2; for D also M3, M4) and the per-workgroup partials of a call; no struct
 * describes it.  psp_loss_stats_accumulate adds n trajectories in three launches: per-workgroup sums, per-workgroup power sums
 * about the chunk's means, and one workgroup that sums the partials in index order and merges the chunk into the state.
 * Every sum has a fixed order that depends on n alone (no atomics): equal sequences of calls give equal bits; another split
 * of the same samples differs by rounding only.  Non-finite samples are not filtered: they make what they enter NaN.
 * psp_loss_stats_finish writes 20 doubles (DEVICE):
 *     out[3 e + 0 .. 2] = mean, unbiased variance, sqrt(variance) / |mean|  for e = 0 terminal, 1 cross_entropy,
 *                         2 cross_entropy_detach, 3 cross_entropy_detach_selection, 5 moment;
 *     out[12 .. 14]     = log_variance: var(D) unbiased, mean((D - mean D)^4) - var(D)^2, and their relative error;
 *     out[18] = samples selected by e = 3,  out[19] = samples in all.
 * A variance over one sample is NaN (0 / 0), as torch.var gives.
 * -1: a null pointer or n < 0 (nothing is launched); n = 0 is a no-op.
 * ------------------------------------------------------------------------------------------------ */
int64_t psp_loss_stats_state_bytes(void);
int psp_loss_stats_accumulate(const float* Y, const float* D, int64_t n, double* state, void* stream);
int psp_loss_stats_finish(const double* state, double* out, void* stream);

/* Diagnostics: device buffer that receives per-wave phase cycle sums (8 u64 per wave of the
 * backward kernel).  Returns 1 if the library was built with -DPSP_STAMPS (diagnostic build,
 * never the shipped one), 0 otherwise (the pointer is then ignored). NULL clears it. */
int psp_debug_set_stamp_buffer(unsigned long long* buf, int64_t n_entries);

#ifdef __cplusplus
}
#endif
#endif /* PSP_H_ */
