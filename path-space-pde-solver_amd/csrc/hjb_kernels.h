// hjb_kernels.h -- CDNA4 (gfx950) kernels for the controlled-SDE rollout of the HJB /
// log-variance training step.  Included by the per-(d,H) instantiation units.
//
// Data layout ("T layout", trajectory-on-lane).  One wavefront owns 16 trajectories.
// A (features x 16 trajectories) panel lives in registers as one f32x4 per block of 16
// features: lane l = j + 16 q (j = trajectory 0..15, q = 0..3), component r of block b
// holds feature 16 b + 4 r + q.  This is exactly the C/D layout of
// v_mfma_f32_16x16x4_f32 (col = lane&15, row = 4 (lane>>4) + reg) when the weight rows
// fed as the A operand are permuted by rowmap(i) = 4 (i&3) + (i>>2); and component r of
// a block is, unchanged, the B operand of k-step 4 b + r (k = q <-> feature 4 (4b+r) + q).
// So every layer  out^T = W . in^T  chains register-to-register with no LDS round trip
// for activations; only the weights (shared by all waves) are staged in LDS, pre-permuted
// so that each A operand is one lane-linear ds_read_b32.
//
// fp32 MFMA is an exact k-ordered fmaf chain (no reduced precision), which is what lets
// the loss match the reference's fp32 CPU path to ~1e-6.
#pragma once
#include <cstdlib>
#include <type_traits>
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "launch.h"
#include "block_index.h"

namespace psp {

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct HjbArgs {
    const float* params;
    const float* x0;
    const float* y0;
    const float* xi;
    float* path;
    float* D;
    float* XN;
    double* fwd_partial;
    const float* drift;
    const float* sigma;
    const float* runcost;
    const float* term;
    const double* sums;
    float* grad_partial;
    const float* tfeat;        // optional (N) per-step network time input (evaluation rollouts); null -> n * dt
    float* Fint;               // optional (K_local) running-cost integral sum_n f(X_{n+1}) dt
    const float* uref;         // optional (N, D) reference control u*(t_n) of an x-independent solution (solver.py:491-494)
    float* ul2;                // (K_local) sum_n |-Z_n - u*(t_n)|^2 dt, written when uref is set
    float* Yout;               // optional (K_local) Y_N
    unsigned long long* dbg;   // diagnostic builds (-DPSP_STAMPS): per-wave phase cycle sums
    float* tables;             // wide kernels: A-operand tables in global memory (carved from the caller's scratch)
    const float* adj_mu;       // adjoint sweep (hjba_kernels.h): dL/dY_N per trajectory
    const float* adj_nu;       //                                  dL/dZsum_N per trajectory (relative entropy), may be null
    const float* adj_wT;       //   weight of grad g(X_N) in lambda_N per trajectory; null: nu - mu (losses of Y_N - g(X_N))
    const uint32_t* iter_dev;  // optional device-resident iteration counter (hipGraph replay); null: `iter` below
    const int* cond;           // optional launch predicate (range guard of the split-product mode, include/psp.h): the grid
    int cond_want;             //   returns at once unless (*cond != 0) == (cond_want != 0)
    long long k_offset;
    long long K_global;
    int x0_stride;
    int K_local;
    int N;
    int ntile16;
    float dt, sqdt, sigma_scale;
    int drift_kind, sigma_kind, runcost_kind, term_kind, adaptive, loss_kind, noise_mode, store_path;
    uint32_t seed_lo, seed_hi, iter;
};

// Predicated launch: the guarded split-product mode enqueues the f16x3 kernel AND its fp32-MFMA twin; a device flag written
// between the two (non-finite partial sums = an operand left the f16 range) decides which of them does the work.  The test is
// one scalar load per workgroup, uniform, and stands before any barrier.
#define PSP_COND_EXIT(args) do { if ((args).cond != nullptr && ((*(args).cond != 0) != ((args).cond_want != 0))) return; } while (0)

// Range guard, backward side (include/psp.h: range_flag): a split-product BACKWARD kernel can leave the f16 range where the forward
// did not (e.g. relu^2 pre-activations r in 128 .. 255: h = r^2 < 65504 is a finite forward operand, but the adjoint (W3 G) 2 r is
// not a finite backward one), and a non-finite gradient would reach Adam -- the parameters would be NaN for good.  Every value a
// split-product backward kernel writes into its partial gradient passes through see(): v * 0 is NaN exactly for NaN / inf.
// raise() at the end of the kernel sets range_flag[0] (and counts the iteration in range_flag[1]) -- BEFORE the fp32-MFMA twin of
// the same launch, which is enqueued behind every guarded split kernel predicated on that flag, reads it: the twin then redoes
// the pass and overwrites the partial gradients.  Costs one fma per stored value; nothing when the guard is off.
template <bool ON>
struct GradCheck {
    float chk = 0.f;
    __device__ __forceinline__ void see(float v) { if constexpr (ON) chk = fmaf(v, 0.f, chk); }
    __device__ __forceinline__ void raise(const int* cond) {
        if constexpr (ON) {
            if (cond != nullptr && chk != chk) {
                int* f = const_cast<int*>(cond);
                if (atomicCAS(f, 0, 1) == 0) atomicAdd(f + 1, 1);
            }
        }
    }
};

// A/B switch for the specialised forward instances (hjb_fwd_kernel FAST_ = 2 and its siblings): PSP_NO_SPEC=1 sends every launch
// to the general instance (diagnostics; read once)
inline bool spec_enabled() {
    static const bool on = [] { const char* e = getenv("PSP_NO_SPEC"); return !(e && e[0] == '1'); }();
    return on;
}

// ---- enums mirrored from include/psp.h (kept numeric here to avoid including C header in device code)
enum { DRIFT_ZERO = 0, DRIFT_DENSE = 1, DRIFT_DIAG = 2, DRIFT_DWELL = 3 };
enum { SIGMA_IDENT = 0, SIGMA_DENSE = 1, SIGMA_SCALE = 2 };
enum { RUN_ZERO = 0, RUN_DIAGQ = 1 };
enum { TERM_LINEAR = 0, TERM_DIAGQ = 1, TERM_SHIFTQ = 2 };
enum { LOSS_LOGVAR = 0, LOSS_MOMENT = 1, LOSS_WEIGHTS = 2, LOSS_RELENT = 3 };
enum { NOISE_SUPPLIED = 0, NOISE_PHILOX = 1 };

__device__ __forceinline__ f32x4 mfma16(float a, float b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

__host__ __device__ constexpr int cdiv(int a, int b) { return (a + b - 1) / b; }

// compile-time loop: f(std::integral_constant<int, I>) for I = 0 .. N - 1 (indices usable as template arguments / immediates)
template <int I, int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        static_for<I + 1, N>(f);
    }
}

// In-kernel phase stamps (diagnostic build only; the shipped kernels execute none of this).
#ifdef PSP_STAMPS
__device__ __forceinline__ unsigned long long stamp_now() {
    unsigned long long t;
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t) :: "memory");
    __builtin_amdgcn_sched_barrier(0);
    return t;
}
#define PSP_STAMP(var) const unsigned long long var = stamp_now()
#define PSP_ACC(slot, t1, t0) stamps[slot] += (t1) - (t0)
#else
#define PSP_STAMP(var)
#define PSP_ACC(slot, t1, t0)
#endif

// Makes a pointer value opaque to the optimiser at this program point.  Used inside the time /
// sample loops so that loop-invariant LDS reads (bias vectors, cost vectors) are re-issued per
// iteration instead of being hoisted out of the loop and kept live (which spills ~160 VGPRs).
// NOTE: launder an integer OFFSET, never the pointer: an asm-laundered pointer loses its LDS
// address space and every read through it becomes a flat_load instead of a ds_read.
__device__ __forceinline__ int opaque_i(int x) {
    asm volatile("" : "+v"(x));
    return x;
}
// Byte address base + 4 (blk * stride + ofs) of a path-store block as an SGPR pair (loads / stores through it are "SGPR base +
// lane offset + immediate").  The block part is made opaque BEFORE the constant offset is added: `base + 4 ofs` alone is
// invariant over the time / round loops, and the compiler used to hoist one such 64-bit sum per distinct offset out of them
// and spill it to VGPR lanes (189 pairs in the d = 500 forward, two v_readlane per load group to get them back).
__device__ __forceinline__ unsigned long long sgpr_block_addr(const void* base, unsigned long long blk, unsigned stride,
                                                              unsigned ofs) {
    unsigned long long addr = (unsigned long long)base + 4ull * (blk * stride);
    asm volatile("" : "+s"(addr));
    addr += 4ull * ofs;
    asm volatile("" : "+s"(addr));
    return addr;
}
template <class T>
__device__ __forceinline__ const T* opaque(const T* p) {   // same pointer + opaque zero offset
    return p + opaque_i(0);
}

// Path-store writes are a pure stream (read back by the next kernel, never by this one): non-temporal stores keep them from
// displacing operand tables and the other kernels' lines in L2 (measured: d = 200 forward 7.5 -> 6.9 ms).
#define PSP_PATH_STORE(ptr, val) __builtin_nontemporal_store((val), (ptr))

// ---------------------------------------------------------------------------------------
// Philox4x32-R (Salmon et al. 2011), counter = (global trajectory, step, call index, iteration)
// R = 7 since round 4 (rounds 1 - 3: 10).  Philox4x32-7 is the paper's smallest Crush-resistant member of the family (SC'11,
// section 4 / table 2: passes the whole of BigCrush; 10 is the "safety margin" default of Random123 and cuRAND).  The generator is
// a third of the forward kernel's VALU issue time at d = 100 (two v_mad_u64_u32 + two v_bitop3_b32 per round, seven calls per
// trajectory and step), and the regenerating backward producers pay it a second time; three rounds less = -30 % of that.
// oracle/philox_oracle.py and the Random123 known-answer vectors of `philox4x32 7` (tests/test_philox_oracle.py) move with it;
// -DPSP_PHILOX_ROUNDS=10 restores the old stream.
// ---------------------------------------------------------------------------------------
#ifndef PSP_PHILOX_ROUNDS
#define PSP_PHILOX_ROUNDS 7
#endif
constexpr int kPhiloxRounds = PSP_PHILOX_ROUNDS;
__device__ __forceinline__ void philox4x32_R(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                                             uint32_t k0, uint32_t k1, uint32_t (&out)[4]) {
#pragma unroll
    for (int r = 0; r < kPhiloxRounds; ++r) {
        // one 32x32->64 multiply per (hi, lo) pair: v_mad_u64_u32 instead of v_mul_hi_u32 + v_mul_lo_u32
        // (32-bit integer multiplies are quarter-rate VALU ops on CDNA)
        const unsigned long long p0 = (unsigned long long)0xD2511F53u * (unsigned long long)c0;
        const unsigned long long p1 = (unsigned long long)0xCD9E8D57u * (unsigned long long)c2;
        const uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0;
        const uint32_t hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
        // three-input xor in one instruction (v_bitop3_b32, truth table 0x96; gfx9 has no v_xor3_b32)
        const uint32_t n0 = __builtin_amdgcn_bitop3_b32(hi1, c1, k0, 0x96), n2 = __builtin_amdgcn_bitop3_b32(hi0, c3, k1, 0x96);
        c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// one round of the above with the keys of round r handed in (k0 + r W0, k1 + r W1): the forward kernels of the split-product mode
// run the ten rounds of a call as separate slices between the MFMAs of their products (hjb_fwd_kernel: philox_slice)
__device__ __forceinline__ void philox_round(uint32_t& c0, uint32_t& c1, uint32_t& c2, uint32_t& c3, uint32_t k0, uint32_t k1) {
    const unsigned long long p0 = (unsigned long long)0xD2511F53u * (unsigned long long)c0;
    const unsigned long long p1 = (unsigned long long)0xCD9E8D57u * (unsigned long long)c2;
    const uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0;
    const uint32_t hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
    const uint32_t n0 = __builtin_amdgcn_bitop3_b32(hi1, c1, k0, 0x96), n2 = __builtin_amdgcn_bitop3_b32(hi0, c3, k1, 0x96);
    c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
}

// two Box-Muller pairs -> four N(0,1) values
__device__ __forceinline__ f32x4 normal4(const uint32_t (&r)[4]) {
    // u = (m + 1/2) 2^-24, m = the upper 24 bits: as ONE fma (m 2^-24 + 2^-25 rounds once; (m + 0.5) 2^-24 rounds the sum and
    // scales it exactly by a power of two -- the same value)
    const float s24 = 1.0f / 16777216.0f, h24 = 0.5f / 16777216.0f;
    const float u0 = __builtin_fmaf((float)(r[0] >> 8), s24, h24);
    const float u1 = __builtin_fmaf((float)(r[1] >> 8), s24, h24);
    const float u2 = __builtin_fmaf((float)(r[2] >> 8), s24, h24);
    const float u3 = __builtin_fmaf((float)(r[3] >> 8), s24, h24);
    // -2 ln u = -2 ln2 * log2 u ; sin/cos hardware ops take revolutions
    const float ra = __builtin_amdgcn_sqrtf(-1.3862943611198906f * __builtin_amdgcn_logf(u0));
    const float rb = __builtin_amdgcn_sqrtf(-1.3862943611198906f * __builtin_amdgcn_logf(u2));
    f32x4 z;
    z[0] = ra * __builtin_amdgcn_cosf(u1);
    z[1] = ra * __builtin_amdgcn_sinf(u1);
    z[2] = rb * __builtin_amdgcn_cosf(u3);
    z[3] = rb * __builtin_amdgcn_sinf(u3);
    return z;
}

// Noise for block b of the T layout: lane (j,q) gets features 16b+4r+q, r=0..3, from ONE
// Philox call with index 4b+q.  (k, n, idx, iter) -> the same values in fwd, bwd and fill.
__device__ __forceinline__ f32x4 philox_block(uint32_t kglob, uint32_t step, uint32_t idx, uint32_t iter,
                                              uint32_t seed_lo, uint32_t seed_hi) {
    uint32_t r[4];
    philox4x32_R(kglob, step, idx, iter, seed_lo, seed_hi, r);
    return normal4(r);
}

// The xi image of sample block (step n, 16-trajectory tile) from the counters the forward kernel used -- store_path 4: the
// forward keeps X_n, h1, h2 only (960 instead of 1408 B per unit at d = 100, H = 64) and the backward producers pay seven
// Philox calls per block instead of 28 loads.  Padded features are zero, as in the forward.
template <int D, int DB>
__device__ __forceinline__ void regen_xi(f32x4 (&xin)[DB], uint32_t kglob, uint32_t n, int q, uint32_t iter,
                                         uint32_t seed_lo, uint32_t seed_hi) {
#pragma unroll
    for (int b = 0; b < DB; ++b) {
        xin[b] = philox_block(kglob, n, (uint32_t)(4 * b + q), iter, seed_lo, seed_hi);
        if (16 * b + 16 > D) {
#pragma unroll
            for (int r = 0; r < 4; ++r) if (16 * b + 4 * r + q >= D) xin[b][r] = 0.f;
        }
    }
}

// ---------------------------------------------------------------------------------------
// LDS staging of pre-permuted A operands and per-feature vectors
// ---------------------------------------------------------------------------------------
// dst[(mb*KS + ks)*64 + lane], lane = i + 16 q  <-  src(row = 16 mb + rowmap(i), col = 4 ks + q)
template <class F>
__device__ __forceinline__ void stage_aop(float* dst, int MB, int KS, int tid, int nthr, F src) {
    const int total = MB * KS * 64;
    for (int idx = tid; idx < total; idx += nthr) {
        const int lane = idx & 63, t = idx >> 6;
        const int ks = t % KS, mb = t / KS;
        const int i = lane & 15, q = lane >> 4;
        dst[idx] = src(16 * mb + 4 * (i & 3) + (i >> 2), 4 * ks + q);
    }
}
// dst[(b*4 + q)*4 + r] <- v(16 b + 4 r + q)   (one f32x4 per lane-q and block)
template <class F>
__device__ __forceinline__ void stage_vec(float* dst, int NBLK, int tid, int nthr, F v) {
    for (int idx = tid; idx < NBLK * 16; idx += nthr) {
        const int r = idx & 3, q = (idx >> 2) & 3, b = idx >> 4;
        dst[idx] = v(16 * b + 4 * r + q);
    }
}

// out^T (MB blocks) += W (A operand table in LDS) . in^T (KS k-steps held in registers)
//
// Software-pipelined by hand: the A operands of chunk c+1 (CH k-steps x MB blocks) are fetched
// while the MFMAs of chunk c issue, and a scheduling fence after every chunk stops hipcc from
// hoisting the remaining ds_reads of the GEMM (up to MB*KS registers) to the top.  The fence
// mask lets VALU / SALU / VMEM cross (tanh, Philox, address math fill the MFMA shadows) but not
// DS reads or MFMAs.  Prefetch distance = CH*MB MFMAs x 32 cycles >= one LDS round trip.
constexpr int kFenceMask = 0x1 | 0x2 | 0x4 | 0x10 | 0x20 | 0x40;
// fence for sample-block boundaries: only VALU / SALU may cross (pins VMEM, DS and MFMA order)
constexpr int kFenceAluOnly = 0x2 | 0x4;
template <int MB, int KS, int INB>
__device__ __forceinline__ void gemm_T(f32x4 (&acc)[MB], const float* wlds,
                                       const f32x4 (&in)[INB], int lane) {
    static_assert(INB * 4 >= KS, "input panel too small");
    static_assert(MB * KS * 256 <= 65536, "table exceeds the 16-bit ds_read immediate offset");
    constexpr int CH = (MB >= 4) ? 2 : 4;
    constexpr int NCH = cdiv(KS, CH);
    // one per-lane base address per GEMM call, every operand = base + immediate offset.  Without the
    // laundering hipcc hoists a separate precomputed address VGPR per 4-KiB stride of every table out
    // of the time loop (hundreds of registers, all spilled).
    lane = opaque_i(lane);
    float buf[2][CH * MB];
#pragma unroll
    for (int kk = 0; kk < CH; ++kk)
#pragma unroll
        for (int mb = 0; mb < MB; ++mb)
            if (kk < KS) buf[0][kk * MB + mb] = wlds[(mb * KS + kk) * 64 + lane];
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        if (c + 1 < NCH) {
#pragma unroll
            for (int kk = 0; kk < CH; ++kk)
#pragma unroll
                for (int mb = 0; mb < MB; ++mb) {
                    const int ks = (c + 1) * CH + kk;
                    if (ks < KS) buf[(c + 1) & 1][kk * MB + mb] = wlds[(mb * KS + ks) * 64 + lane];
                }
        }
#pragma unroll
        for (int kk = 0; kk < CH; ++kk) {
            const int ks = c * CH + kk;
            if (ks < KS) {
                const float bop = in[ks >> 2][ks & 3];
#pragma unroll
                for (int mb = 0; mb < MB; ++mb) acc[mb] = mfma16(buf[c & 1][kk * MB + mb], bop, acc[mb]);
            }
        }
        __builtin_amdgcn_sched_barrier(kFenceMask);
    }
}

// ---- bf16 MFMA variant of the register-chained products (BASELINE.json configs[2]: "bf16 MFMA MLP path"; also the
// opt-in bf16-MLP mode of the HJB forward kernel) --------------------------------------------------------
// v_mfma_f32_16x16x32_bf16: A (16 x 32) lane (i, g) holds k = 8g..8g+7, B (32 x 16) lane (n, g) likewise, fp32 accumulate.
// One k-step spans TWO 16-feature blocks of the T layout; lane (j, q) already holds in[2S][0..3], in[2S+1][0..3], so the
// B operand is a pack of eight local registers (no shuffle): k = 8q + e  <->  feature 32 S + (e < 4 ? 4e : 16 + 4(e-4)) + q.
// The A tables are laid out for that map (stage_aop_bf16), rows keep the rowmap of the fp32 tables, so the fp32
// accumulators chain from layer to layer exactly as in the fp32 kernels.  State, accumulators, Y and the path store stay fp32.
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
template <class F>
__device__ __forceinline__ void stage_aop_bf16(float* dstf, int MB, int NS, int tid, int nthr, F src) {
    bf16x8* dst = reinterpret_cast<bf16x8*>(dstf);
    const int total = MB * NS * 64;
    for (int idx = tid; idx < total; idx += nthr) {
        const int lane = idx & 63, t = idx >> 6;
        const int S = t % NS, mb = t / NS;
        const int i = lane & 15, g = lane >> 4;
        const int row = 16 * mb + 4 * (i & 3) + (i >> 2);
        bf16x8 v;
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = (__bf16)src(row, 32 * S + (e < 4 ? 4 * e : 16 + 4 * (e - 4)) + g);
        dst[idx] = v;
    }
}
template <int MB, int INB>
__device__ __forceinline__ void gemm_Tb(f32x4 (&acc)[MB], const float* wlds, const f32x4 (&in)[INB], int lane) {
    constexpr int NS = (INB + 1) / 2;
    const bf16x8* tbl = reinterpret_cast<const bf16x8*>(wlds) + opaque_i(lane);
#pragma unroll
    for (int S = 0; S < NS; ++S) {
        bf16x8 b;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            b[e] = (__bf16)in[2 * S][e];
            b[4 + e] = (2 * S + 1 < INB) ? (__bf16)in[(2 * S + 1 < INB) ? 2 * S + 1 : 0][e] : (__bf16)0.0f;
        }
#pragma unroll
        for (int mb = 0; mb < MB; ++mb)
            acc[mb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(tbl[(mb * NS + S) * 64], b, acc[mb], 0, 0, 0);
    }
}

// ---- fp32 products on the f16 matrix pipe: error-compensated split ("f16x3") ------------------------------------------
// An fp32 MFMA runs at 1/16 of the f16 rate on this chip (157 TFLOP/s against 2.5 PFLOP/s), so an fp32-grade product is
// cheaper as THREE f16 MFMAs than as one fp32 MFMA per four k:  every operand is split into two f16 numbers
//     x = hi + lo / 2048,   hi = f16(x) (round to nearest, 11 significant bits),   lo = f16((x - hi) * 2048)  (the next 11)
// (the residual x - hi is exact in fp32; the power-of-two scale keeps lo out of the f16 subnormals) and
//     a.b = hi_a hi_b + (hi_a lo_b + lo_a hi_b) / 2048 + O(2^-22 |a||b|)
// with both sums accumulated in fp32 by v_mfma_f32_16x16x32_f16 (main chain on the caller's accumulator, correction chain on
// its own).  Product error against fp64: 1.07 x that of an fp32 chain (numpy model of this arithmetic: tests/test_split_product.py)
// -- the same parity bar as the fp32 kernels, which is why this is a mode of the fp32 path and not a reduced-precision one.
// Range: |x| < 65504 for every operand (states, activations, matrix entries); beyond that the f16 hi part overflows.
// Layout: one k-step of 32 spans TWO 16-feature blocks of the T layout exactly as in gemm_Tb (B operand = pack of eight local
// registers, k = 8q + e <-> feature 32 S + (e < 4 ? 4e : 16 + 4(e-4)) + q); an odd trailing block runs as ONE exact fp32
// k-step when it holds at most four real features (d = 100: 3 split steps + features 96..99 in fp32; the table is then
// exactly as large as the fp32 one) and as a 16x16x16 f16 step (three MFMAs again) otherwise.
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
constexpr float kSplitScale = 2048.0f, kSplitInv = 1.0f / 2048.0f;
template <int KS, int INB>
struct SplitGeo {
    static constexpr int NS = INB / 2;                       // full 32-feature steps
    static constexpr bool ODD = (INB & 1) != 0;
    static constexpr int NKR = ODD ? KS - 8 * NS : 0;        // real fp32 k-steps of the trailing block (1..4)
    static constexpr bool ODD_F32 = ODD && NKR <= 1;
    static constexpr bool ODD_H16 = ODD && NKR > 1;
    static constexpr int per_mb = NS * 512 + (ODD_F32 ? 64 : 0) + (ODD_H16 ? 256 : 0);   // floats per 16-row block
    static constexpr int floats(int MB) { return MB * per_mb; }
};
__device__ __forceinline__ void split_f16(float v, _Float16& hi, _Float16& lo) {
    hi = (_Float16)v;
    lo = (_Float16)((v - (float)hi) * kSplitScale);
}
// One-accumulator form (the narrow split forward, hjb_fwd_kernel MODE 2).  The correction chain exists only
// because the lo parts sit on another scale than the hi parts.  Scale instead the A operand by 2^p and the B operand by 2^q, hi
// and lo alike, p + q = 11:
//     A = 2^p a = Ah + Al,   B = 2^q b = Bh + Bl   (hi = f16(.), lo = f16(. - hi): UNSCALED residuals)
//     Ah Bh + Ah Bl + Al Bh = 2048 a b - Al Bl,    |Al Bl| <= 2^-22 |A B|
// -- all three terms on one scale, one accumulator, no merge fma and no second register set.  The caller initialises the
// accumulator with 2048 x its bias and takes the 2048 out where a multiplication already stands (tanh's argument scale, the
// row sums' per-lane finish, the coefficient of the state update).
// A lo part is a residual of magnitude <= 2^-11 |hi|; below the f16 normal range (2^-14) it keeps an absolute quantum of 2^-24,
// so a scaled operand S keeps all 22 bits while |S| >= 2^-3 and loses them one by one below.
// Choice of p, q, every product: tables 2^6 (kLgFwdA), operands 2^5 (kLgFwdB).  At the headline's magnitudes: weights ~ 0.1 -> 6,
// lo ~ 2^-9; entries of dt M ~ 1e-2 -> 0.6, lo ~ 2^-12; states and activations 0.1 .. 3 -> 3 .. 100, lo ~ 2^-9 .. 2^-5: every part a
// normal f16.  (All 11 bits on the tables, p = 11, q = 0, would leave the lo part of an activation of 0.1 at 2^-15: subnormal.)
// Range: |weight| < 65504 / 64 ~ 1023, |input| < 65504 / 32 ~ 2047.
// hjb_bwd3_kernel was measured in this form too (panels 2^8, tables and stored activations 2^3, one chain for dW1): 5 % fewer VALU
// instructions and 4 % MORE wave cycles per launch, +0.05 ms -- it keeps its two chains (profiles/one_accumulator_ab.json).
// Beyond the range the scaled hi part is +inf and lo = f16(S - inf) = -inf; they meet in the SAME accumulator: NaN, which is what
// the range guard (include/psp.h: range_flag) looks for.
constexpr int kLgFwdA = 6, kLgFwdB = 5;
static_assert(kLgFwdA + kLgFwdB == 11, "p + q = 11: the accumulators hold 2048 a b");
__host__ __device__ constexpr float pow2f(int e) { return e >= 0 ? (float)(1 << e) : 1.0f / (float)(1 << -e); }
// one table entry: LG < 0 the two-chain form above, else the one-accumulator form with scale 2^LG
template <int LG>
__device__ __forceinline__ void split_tab(float v, _Float16& hi, _Float16& lo) {
    if constexpr (LG >= 0) {
        const float s = pow2f(LG) * v;
        hi = (_Float16)s;
        lo = (_Float16)(s - (float)hi);
    } else {
        split_f16(v, hi, lo);
    }
}
// Packs of four / eight values (two 16-feature blocks of the T layout side by side).  Plain C on purpose.  Round 3 tried the
// split as inline asm -- v_cvt_pk_f16_f32, one packed multiply and v_fma_mixlo/hi_f16 (lo = f16(fma(hi, -2048, 2048 x)), bit-identical,
// two instructions per value instead of the compiler's three) -- and took it out again: the hazard recogniser does not look into
// inline asm, and on this chip (a) an MFMA result read by a VALU instruction, (b) a half-register write followed directly by an
// MFMA read, and (c) a VALU write to the dead SrcC of an MFMA still in flight (v[a:b] = mfma(.., v[c:d]) is not in place) all need
// software wait states that the compiler inserts only for its own instructions.  (a) gave a 2e-4 gradient error and NaN at
// d > 256, (c) run-to-run different gradients (499 entries, 6e-5) in gen_bwd2_kernel<.., X3>; the variant that avoids all three
// needs extra moves and saves half an instruction per value (1 - 2 % of a kernel) -- not worth an unprovable rule set.

// Two values at a time (round 4): hi pair = ONE v_cvt_pk_f16_f32, 2048 x = one v_pk_mul_f32 for both, and each lo =
// f16(fma(hi, -2048, 2048 x)) = one v_fma_mixlo/mixhi_f16 that reads its half of the hi pair directly -- two instructions per value
// where the (x - float(hi)) * 2048 form compiles to four (convert back, subtract, multiply, convert).  The same value bit for bit:
// x - hi is exact, 2048 (x - hi) has at most 13 significant bits, so the fma's fp32 rounding does nothing and the f16 rounding is
// the one split_f16 applies.  Round 3 had this as inline asm and took it out (hazards the compiler does not see in asm); this is
// plain C, selected by the compiler itself -- which needs -fno-slp-vectorize (build.py): the SLP vectoriser otherwise packs the two
// fmas into a v_pk_fma_f32 behind two back-conversions.
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void split_pair(float a, float b, f16x2& hi, f16x2& lo) {
    const f32x2 v = {a, b};
    hi = __builtin_convertvector(v, f16x2);
    const f32x2 s = v * kSplitScale;
    lo[0] = (_Float16)__builtin_fmaf((float)hi[0], -kSplitScale, s[0]);
    lo[1] = (_Float16)__builtin_fmaf((float)hi[1], -kSplitScale, s[1]);
}
// (four values whose packs feed v_mfma_f32_16x16x16f16 DIRECTLY -- the trailing 16-feature step of an odd block count -- keep the
//  classic form: with the pair form below, v_fma_mixlo/hi_f16 writing the halves of the operand registers right in front of that
//  MFMA gave run-to-run different results on gfx950 (the first output block's rows, d = 200: tools/r4/det_check.py) -- a hazard the
//  compiler does not cover for this pair of instructions; packs that are combined into f16x8 operands of the 16x16x32 MFMAs first
//  are not affected: every determinism test of those paths is bitwise stable)
__device__ __forceinline__ void split4c(const f32x4& u, f16x4& hi, f16x4& lo) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        _Float16 h, l;
        split_f16(u[e], h, l);
        hi[e] = h; lo[e] = l;
    }
}
__device__ __forceinline__ void split4(const f32x4& u, f16x4& hi, f16x4& lo) {
#if defined(PSP_SPLIT_CLASSIC) && PSP_SPLIT_CLASSIC
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        _Float16 h, l;
        split_f16(u[e], h, l);
        hi[e] = h; lo[e] = l;
    }
    return;
#endif
    f16x2 h, l;
    split_pair(u[0], u[1], h, l); hi[0] = h[0]; hi[1] = h[1]; lo[0] = l[0]; lo[1] = l[1];
    split_pair(u[2], u[3], h, l); hi[2] = h[0]; hi[3] = h[1]; lo[2] = l[0]; lo[3] = l[1];
}
__device__ __forceinline__ void split8(const f32x4& u0, const f32x4& u1, f16x8& hi, f16x8& lo) {
#if defined(PSP_SPLIT_CLASSIC) && PSP_SPLIT_CLASSIC
    // (the wide family's translation units: hjbw_bwd_x3_kernel<500, 64> sits at 512 registers and spills 95 instead of 28 dwords with
    //  the pair form and the SLP vectoriser off -- 5.2 -> 6.9 ms; they keep the round-3 form and flags, build.py)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        _Float16 h, l;
        split_f16(u0[e], h, l);
        hi[e] = h; lo[e] = l;
        split_f16(u1[e], h, l);
        hi[4 + e] = h; lo[4 + e] = l;
    }
    return;
#endif
    f16x2 h, l;
    split_pair(u0[0], u0[1], h, l); hi[0] = h[0]; hi[1] = h[1]; lo[0] = l[0]; lo[1] = l[1];
    split_pair(u0[2], u0[3], h, l); hi[2] = h[0]; hi[3] = h[1]; lo[2] = l[0]; lo[3] = l[1];
    split_pair(u1[0], u1[1], h, l); hi[4] = h[0]; hi[5] = h[1]; lo[4] = l[0]; lo[5] = l[1];
    split_pair(u1[2], u1[3], h, l); hi[6] = h[0]; hi[7] = h[1]; lo[6] = l[0]; lo[7] = l[1];
}
// ... with the UNSCALED residual lo = f16(x - hi) (the weight-gradient outer products: one accumulator for all three terms); the pair
// form: lo = f16(fma(hi, -1, x)), one v_fma_mixlo/hi_f16 per value (x - hi is exact: the same bits)
__device__ __forceinline__ void split_pair_u(float a, float b, f16x2& hi, f16x2& lo) {
    const f32x2 v = {a, b};
    hi = __builtin_convertvector(v, f16x2);
    lo[0] = (_Float16)__builtin_fmaf((float)hi[0], -1.0f, v[0]);
    lo[1] = (_Float16)__builtin_fmaf((float)hi[1], -1.0f, v[1]);
}
__device__ __forceinline__ void split8u(const f32x4& u0, const f32x4& u1, f16x8& hi, f16x8& lo) {
#if defined(PSP_SPLIT_CLASSIC) && PSP_SPLIT_CLASSIC
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        _Float16 h = (_Float16)u0[e];
        hi[e] = h; lo[e] = (_Float16)(u0[e] - (float)h);
        h = (_Float16)u1[e];
        hi[4 + e] = h; lo[4 + e] = (_Float16)(u1[e] - (float)h);
    }
    return;
#endif
    f16x2 h, l;
    split_pair_u(u0[0], u0[1], h, l); hi[0] = h[0]; hi[1] = h[1]; lo[0] = l[0]; lo[1] = l[1];
    split_pair_u(u0[2], u0[3], h, l); hi[2] = h[0]; hi[3] = h[1]; lo[2] = l[0]; lo[3] = l[1];
    split_pair_u(u1[0], u1[1], h, l); hi[4] = h[0]; hi[5] = h[1]; lo[4] = l[0]; lo[5] = l[1];
    split_pair_u(u1[2], u1[3], h, l); hi[6] = h[0]; hi[7] = h[1]; lo[6] = l[0]; lo[7] = l[1];
}
// ... and of the one-accumulator form: hi = f16(c x), lo = f16(c x - hi), c a power of two.  The multiply is the one split_pair
// has already (only its constant changes; c = 1 folds it away), the residual one v_fma_mixlo/hi_f16 as in split_pair_u.
// (The -1 is handed in through a register the optimiser cannot see into: fma(hi, -1.0, s) is canonicalised to a subtraction,
// which is then selected as convert back, subtract, convert -- three instructions per value.)
__device__ __forceinline__ void split_pair_s(float a, float b, float c, f16x2& hi, f16x2& lo) {
    const f32x2 s = f32x2{a, b} * c;
    hi = __builtin_convertvector(s, f16x2);
    float m1 = -1.0f;
    asm("" : "+s"(m1));
    lo[0] = (_Float16)__builtin_fmaf((float)hi[0], m1, s[0]);
    lo[1] = (_Float16)__builtin_fmaf((float)hi[1], m1, s[1]);
}
__device__ __forceinline__ void split4s(const f32x4& u, float c, f16x4& hi, f16x4& lo) {
    f16x2 h, l;
    split_pair_s(u[0], u[1], c, h, l); hi[0] = h[0]; hi[1] = h[1]; lo[0] = l[0]; lo[1] = l[1];
    split_pair_s(u[2], u[3], c, h, l); hi[2] = h[0]; hi[3] = h[1]; lo[2] = l[0]; lo[3] = l[1];
}
__device__ __forceinline__ void split8s(const f32x4& u0, const f32x4& u1, float c, f16x8& hi, f16x8& lo) {
    f16x4 h0, l0, h1, l1;
    split4s(u0, c, h0, l0);
    split4s(u1, c, h1, l1);
    hi = __builtin_shufflevector(h0, h1, 0, 1, 2, 3, 4, 5, 6, 7);
    lo = __builtin_shufflevector(l0, l1, 0, 1, 2, 3, 4, 5, 6, 7);
}
// (the classic form for packs that feed v_mfma_f32_16x16x16f16 directly: see split4c)
__device__ __forceinline__ void split4cs(const f32x4& u, float c, f16x4& hi, f16x4& lo) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float s = c * u[e];
        const _Float16 h = (_Float16)s;
        hi[e] = h; lo[e] = (_Float16)(s - (float)h);
    }
}
// LG >= 0: the table of the one-accumulator form (split_tab: entries scaled by 2^LG, unscaled residuals; the fp32 k-step's
// entries scaled too)
template <int KS, int INB, int LG = -1, class F>
__device__ __forceinline__ void stage_aop_x3(float* dstf, int MB, int tid, int nthr, F src) {
    using SG = SplitGeo<KS, INB>;
    if constexpr (SG::NS > 0) {
        for (int idx = tid; idx < MB * SG::NS * 64; idx += nthr) {
            const int lane = idx & 63, t = idx >> 6;
            const int S = t % SG::NS, mb = t / SG::NS;
            const int i = lane & 15, g = lane >> 4;
            const int row = 16 * mb + 4 * (i & 3) + (i >> 2);
            f16x8 hi, lo;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                _Float16 h, l;
                split_tab<LG>(src(row, 32 * S + (e < 4 ? 4 * e : 16 + 4 * (e - 4)) + g), h, l);
                hi[e] = h; lo[e] = l;
            }
            f16x8* p = reinterpret_cast<f16x8*>(dstf + mb * SG::per_mb + S * 512);
            p[lane] = hi; p[64 + lane] = lo;
        }
    }
    if constexpr (SG::ODD) {
        for (int idx = tid; idx < MB * 64; idx += nthr) {
            const int lane = idx & 63, mb = idx >> 6;
            const int i = lane & 15, g = lane >> 4;
            const int row = 16 * mb + 4 * (i & 3) + (i >> 2);
            if constexpr (SG::ODD_F32) {
                dstf[mb * SG::per_mb + SG::NS * 512 + lane] = (LG >= 0 ? pow2f(LG) : 1.0f) * src(row, 32 * SG::NS + g);
            } else {
                f16x4 hi, lo;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    _Float16 h, l;
                    split_tab<LG>(src(row, 32 * SG::NS + 4 * e + g), h, l);
                    hi[e] = h; lo[e] = l;
                }
                f16x4* p = reinterpret_cast<f16x4*>(dstf + mb * SG::per_mb + SG::NS * 512);
                p[lane] = hi; p[64 + lane] = lo;
            }
        }
    }
}
// out^T (MB blocks) += W . in^T with fp32-grade products on the f16 pipe; A operands prefetched through a ring of 2 CU slots
// (unit = 16-row block x 32-deep step; CU = 2: four slots, reads three units ahead; CU = 1: two slots, 16 registers less)
struct NoBetween { __device__ __forceinline__ void operator()(int) const {} };
// `between(u)` runs after the products of unit u (u = S * MB + mb): the forward kernels hand their path stores over in
// portions so that they stand BETWEEN the MFMAs (the scheduler clusters them into bursts of 28 - 32 otherwise, and a burst
// blocks the in-order wave while the store path drains at 16 B/clk per CU), and the slices of their Philox calls so that they
// run in the MFMAs' shadow; fences with a functor let nothing cross.
// ONE (split_tab): acc += 2048 W . in^T on the caller's accumulator alone -- table staged with stage_aop_x3<.., kLgFwdA>, the operand
// split with 2^kLgFwdB here; the two lower-order products follow the main one into acc[mb]: no correction set, no merge.
template <int MB, int KS, int INB, int CU = 2, bool ONE = false, class BT = NoBetween>
__device__ __forceinline__ void gemm_Tx(f32x4 (&acc)[MB], const float* wlds, const f32x4 (&in)[INB], int lane, BT between = BT()) {
    constexpr int kFence = std::is_same<BT, NoBetween>::value ? kFenceMask : 0;      // (with a functor: nothing crosses a unit's fence)
    using SG = SplitGeo<KS, INB>;
    constexpr int NS = SG::NS;
    static_assert(MB * SG::per_mb * 4 <= 65536, "table exceeds the 16-bit ds_read immediate offset");
    lane = opaque_i(lane);
    [[maybe_unused]] f32x4 corr[ONE ? 1 : MB];                                       // (ONE: unused)
    if constexpr (!ONE) {
#pragma unroll
        for (int mb = 0; mb < MB; ++mb) corr[mb] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    if constexpr (NS > 0) {
        // units u = S * MB + mb in a ring of R = 2 CU operand slots, each unit's pair of 16-byte reads issued R - 1 units
        // (3 (R - 1) MFMAs) before its products: with CU = 2 that is 9 MFMAs of distance for the 32 registers a double-buffered
        // chunk of two gave 6 for (the forward's waves spent a quarter of their cycles in s_waitcnt on these reads)
        const f16x8* tbl = reinterpret_cast<const f16x8*>(wlds) + lane;
        constexpr int NU = NS * MB, R = 2 * CU, PF = R - 1;
        f16x8 ah[R], al[R];
#pragma unroll
        for (int u = 0; u < PF; ++u)
            if (u < NU) {
                ah[u % R] = tbl[((u % MB) * SG::per_mb + (u / MB) * 512) / 4];
                al[u % R] = tbl[((u % MB) * SG::per_mb + (u / MB) * 512) / 4 + 64];
            }
        f16x8 bh, bl;
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            if (u + PF < NU) {
                const int v = u + PF;
                ah[v % R] = tbl[((v % MB) * SG::per_mb + (v / MB) * 512) / 4];
                al[v % R] = tbl[((v % MB) * SG::per_mb + (v / MB) * 512) / 4 + 64];
            }
            const int S = u / MB, mb = u % MB;
            if (mb == 0) {
                if constexpr (ONE) split8s(in[2 * S], in[2 * S + 1], pow2f(kLgFwdB), bh, bl);
                else split8(in[2 * S], in[2 * S + 1], bh, bl);
            }
            acc[mb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[u % R], bh, acc[mb], 0, 0, 0);
            if constexpr (ONE) {
                acc[mb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[u % R], bl, acc[mb], 0, 0, 0);
                acc[mb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[u % R], bh, acc[mb], 0, 0, 0);
            } else {
                corr[mb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[u % R], bl, corr[mb], 0, 0, 0);
                corr[mb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[u % R], bh, corr[mb], 0, 0, 0);
            }
            between(u);
            __builtin_amdgcn_sched_barrier(kFence);
        }
    }
    if constexpr (SG::ODD_F32) {
        const float bop = (ONE ? pow2f(kLgFwdB) : 1.0f) * in[INB - 1][0];
#pragma unroll
        for (int mb = 0; mb < MB; ++mb) acc[mb] = mfma16(wlds[mb * SG::per_mb + NS * 512 + lane], bop, acc[mb]);
    }
    if constexpr (SG::ODD_H16) {
        f16x4 bh, bl;
        if constexpr (ONE) split4cs(in[INB - 1], pow2f(kLgFwdB), bh, bl);
        else split4c(in[INB - 1], bh, bl);
#pragma unroll
        for (int mb = 0; mb < MB; ++mb) {
            const f16x4* p = reinterpret_cast<const f16x4*>(wlds + mb * SG::per_mb + NS * 512) + lane;
            const f16x4 a_hi = p[0], a_lo = p[64];
            acc[mb] = __builtin_amdgcn_mfma_f32_16x16x16f16(a_hi, bh, acc[mb], 0, 0, 0);
            if constexpr (ONE) {
                acc[mb] = __builtin_amdgcn_mfma_f32_16x16x16f16(a_hi, bl, acc[mb], 0, 0, 0);
                acc[mb] = __builtin_amdgcn_mfma_f32_16x16x16f16(a_lo, bh, acc[mb], 0, 0, 0);
            } else {
                corr[mb] = __builtin_amdgcn_mfma_f32_16x16x16f16(a_hi, bl, corr[mb], 0, 0, 0);
                corr[mb] = __builtin_amdgcn_mfma_f32_16x16x16f16(a_lo, bh, corr[mb], 0, 0, 0);
            }
        }
    }
    if constexpr (!ONE) {
#pragma unroll
        for (int mb = 0; mb < MB; ++mb) acc[mb] = acc[mb] + kSplitInv * corr[mb];
    }
}

// The one-accumulator gemm_Tx for an input panel that feeds TWO products (the state: W1 x and (dt A) x of the same step): the
// panel is split once by split_panel8 (2^kLgFwdB) and both products read the packs; `last` = the panel's trailing block, unsplit.
// One-accumulator only: the table MUST be one staged with stage_aop_x3<.., kLgFwdA>.
template <int INB>
__device__ __forceinline__ void split_panel8(const f32x4 (&in)[INB], f16x8 (&bh)[INB / 2 > 0 ? INB / 2 : 1], f16x8 (&bl)[INB / 2 > 0 ? INB / 2 : 1]) {
#pragma unroll
    for (int S = 0; S < INB / 2; ++S) split8s(in[2 * S], in[2 * S + 1], pow2f(kLgFwdB), bh[S], bl[S]);
}
template <int MB, int KS, int INB, int CU = 2, class BT = NoBetween>
__device__ __forceinline__ void gemm_Txs(f32x4 (&acc)[MB], const float* wlds, const f16x8 (&bh)[INB / 2 > 0 ? INB / 2 : 1],
                                         const f16x8 (&bl)[INB / 2 > 0 ? INB / 2 : 1], const f32x4& last, int lane, BT between = BT()) {
    constexpr int kFence = std::is_same<BT, NoBetween>::value ? kFenceMask : 0;      // (with a functor: nothing crosses a unit's fence)
    using SG = SplitGeo<KS, INB>;
    constexpr int NS = SG::NS;
    lane = opaque_i(lane);
    if constexpr (NS > 0) {
        const f16x8* tbl = reinterpret_cast<const f16x8*>(wlds) + lane;
        constexpr int NU = NS * MB, R = 2 * CU, PF = R - 1;
        f16x8 ah[R], al[R];
#pragma unroll
        for (int u = 0; u < PF; ++u)
            if (u < NU) {
                ah[u % R] = tbl[((u % MB) * SG::per_mb + (u / MB) * 512) / 4];
                al[u % R] = tbl[((u % MB) * SG::per_mb + (u / MB) * 512) / 4 + 64];
            }
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            if (u + PF < NU) {
                const int v = u + PF;
                ah[v % R] = tbl[((v % MB) * SG::per_mb + (v / MB) * 512) / 4];
                al[v % R] = tbl[((v % MB) * SG::per_mb + (v / MB) * 512) / 4 + 64];
            }
            const int S = u / MB, mb = u % MB;
            acc[mb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[u % R], bh[S], acc[mb], 0, 0, 0);
            acc[mb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[u % R], bl[S], acc[mb], 0, 0, 0);
            acc[mb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[u % R], bh[S], acc[mb], 0, 0, 0);
            between(u);
            __builtin_amdgcn_sched_barrier(kFence);
        }
    }
    if constexpr (SG::ODD_F32) {
        const float bop = pow2f(kLgFwdB) * last[0];
#pragma unroll
        for (int mb = 0; mb < MB; ++mb) acc[mb] = mfma16(wlds[mb * SG::per_mb + NS * 512 + lane], bop, acc[mb]);
    }
    if constexpr (SG::ODD_H16) {
        f16x4 b4h, b4l;
        split4cs(last, pow2f(kLgFwdB), b4h, b4l);
#pragma unroll
        for (int mb = 0; mb < MB; ++mb) {
            const f16x4* p = reinterpret_cast<const f16x4*>(wlds + mb * SG::per_mb + NS * 512) + lane;
            const f16x4 a_hi = p[0], a_lo = p[64];
            acc[mb] = __builtin_amdgcn_mfma_f32_16x16x16f16(a_hi, b4h, acc[mb], 0, 0, 0);
            acc[mb] = __builtin_amdgcn_mfma_f32_16x16x16f16(a_hi, b4l, acc[mb], 0, 0, 0);
            acc[mb] = __builtin_amdgcn_mfma_f32_16x16x16f16(a_lo, b4h, acc[mb], 0, 0, 0);
        }
    }
}

__device__ __forceinline__ float qsum(float v) {  // sum over the 4 q-lanes of a trajectory
    v += __shfl_xor(v, 16);
    v += __shfl_xor(v, 32);
    return v;
}
__device__ __forceinline__ float jsumf(float v) {  // fp32 sum over the 16 trajectories of a wave (q fixed)
    v += __shfl_xor(v, 1);
    v += __shfl_xor(v, 2);
    v += __shfl_xor(v, 4);
    v += __shfl_xor(v, 8);
    return v;
}
__device__ __forceinline__ double jsum(double v) {  // sum over the 16 trajectories of a wave (q fixed)
    v += __shfl_xor(v, 1);
    v += __shfl_xor(v, 2);
    v += __shfl_xor(v, 4);
    v += __shfl_xor(v, 8);
    return v;
}

// Branch-free fp32 tanh (ocml tanhf is a two-way divergent branch per call):
//   tanh(x) = sign(x) (1 - 2 / (exp(2|x|) + 1)),  exp via v_exp_f32, 1/x via v_rcp_f32 (~1 ulp each): six full-rate and
//   two quarter-rate VALU ops.  Absolute error <= 2e-7 everywhere (the subtraction cancels for small |x|, so the RELATIVE
//   error grows like 1e-7 / |x|; the forward kernels are VALU-limited next to fp32 MFMA -- DESIGN.md section 4 -- and the
//   Taylor branch that kept 3e-7 relative accuracy below |x| = 0.35 cost 3.5 % of the forward kernel).
// X2048: the argument is 2048 x (the accumulator of a one-accumulator split product, gemm_Tx ONE): the power of two goes into
// the constant -- the same product bit for bit -- and copysign sees the same sign.
template <bool X2048 = false>
__device__ __forceinline__ float tanh_f32(float x) {
    const float e = __builtin_amdgcn_exp2f(fabsf(x) * (X2048 ? 2.8853900817779268f * kSplitInv : 2.8853900817779268f));  // exp(2|x|)
    const float big = fmaf(-2.0f, __builtin_amdgcn_rcpf(e + 1.0f), 1.0f);    // saturates to 1 for large |x|
    return copysignf(big, x);
}
template <bool X2048 = false>
__device__ __forceinline__ f32x4 tanh4(f32x4 v) {
    f32x4 o;
    o[0] = tanh_f32<X2048>(v[0]); o[1] = tanh_f32<X2048>(v[1]); o[2] = tanh_f32<X2048>(v[2]); o[3] = tanh_f32<X2048>(v[3]);
    return o;
}

// NaN-propagating relu for the split-product instances: v_max_f32 returns the non-NaN operand, which would turn the NaN of an
// operand beyond the f16 range (inf - inf between the main and the correction chain) into a clean 0 and hide the overflow from
// the range guard (include/psp.h: range_flag).  One compare + select instead of one max.
__device__ __forceinline__ f32x4 relu4n(f32x4 v) {
    f32x4 o;
    o[0] = v[0] < 0.f ? 0.f : v[0]; o[1] = v[1] < 0.f ? 0.f : v[1]; o[2] = v[2] < 0.f ? 0.f : v[2]; o[3] = v[3] < 0.f ? 0.f : v[3];
    return o;
}

// Geometry of one (D, H) instantiation
template <int D, int H>
struct Geo {
    static constexpr int DB = cdiv(D, 16), HB = cdiv(H, 16);
    static constexpr int KSD = cdiv(D, 4), KSH = cdiv(H, 4);
    // torch flat parameter offsets
    static constexpr int oW1 = 0, ob1 = H * (D + 1), oW2 = ob1 + H, ob2 = oW2 + H * H, oW3 = ob2 + H,
                         ob3 = oW3 + D * H, P = ob3 + D;
    // forward LDS carve (floats).  Each table holds the larger of its two images: the fp32 one (MB x KS k-steps of 64 floats)
    // and the bf16 one of MODE 1 (stage_aop_bf16: MB x ceil(INB / 2) k-steps of 64 x 16 bytes).  The bf16 image is the larger
    // one only where a 32-wide k-step is mostly padding: 4 ceil(INB / 2) > KS, i.e. an input of at most 12 features (the
    // d = 2, 4, 8, 10 instances' W1); every other instance keeps the fp32 carve to the byte (static_assert below).
    static constexpr int tbl(int MB, int KS, int INB) { return MB * (KS > 4 * ((INB + 1) / 2) ? KS : 4 * ((INB + 1) / 2)) * 64; }
    static constexpr int fW1 = 0, fW2 = fW1 + tbl(HB, KSD, DB), fW3 = fW2 + tbl(HB, KSH, HB),
                         fVec = fW3 + tbl(DB, KSH, HB);
    static_assert(D <= 12 || H <= 12 || fVec == (HB * KSD + HB * KSH + DB * KSH) * 64, "only inputs of <= 12 features change the carve");
    // vectors: b1, w1t, b2 (HB*16 each), b3, driftv, runv, termv (DB*16 each)
    static constexpr int vb1 = fVec, vw1t = vb1 + HB * 16, vb2 = vw1t + HB * 16, vb3 = vb2 + HB * 16,
                         vdr = vb3 + DB * 16, vrun = vdr + DB * 16, vterm = vrun + DB * 16,
                         fRed = vterm + DB * 16;           // 2 doubles per wave, 16 waves max
    static constexpr int fA = fRed + 64;
    static constexpr int fB_dense_off = DB * KSD * 64;      // size of one dense d x d table
    // split-product mode (gemm_Tx): table sizes of SplitGeo, the vectors / reduction area / d x d tables behind them in the
    // same order as above
    static constexpr int xW1 = 0, xW2 = xW1 + SplitGeo<KSD, DB>::floats(HB), xW3 = xW2 + SplitGeo<KSH, HB>::floats(HB),
                         xVec = xW3 + SplitGeo<KSH, HB>::floats(DB), xA = xVec + (fA - fVec);
    static constexpr int xB_dense_off = SplitGeo<KSD, DB>::floats(DB);
    static int fwd_x3_lds_floats(int drift_kind, int sigma_kind) {
        return xA + (drift_kind == DRIFT_DENSE ? xB_dense_off : 0) + (sigma_kind == SIGMA_DENSE ? xB_dense_off : 0);
    }
    static int fwd_lds_floats(int drift_kind, int sigma_kind) {
        return fA + (drift_kind == DRIFT_DENSE ? fB_dense_off : 0) + (sigma_kind == SIGMA_DENSE ? fB_dense_off : 0);
    }
    // path store: one block per (step n, 16-trajectory tile): register images of X_n, h1, h2,
    // each padded to whole 16-feature blocks (padded k-steps hold zeros) so that the backward
    // kernel's feature-on-lane reads need neither clamping nor masking
    // path block of one (time step, 16-trajectory tile): register images of X_n, h1, h2 and of the Brownian increment
    // xi_{n+1} -- the backward kernels LOAD xi instead of regenerating it: next to an fp32 MFMA stream a VALU cycle is
    // expensive (a dense MFMA wave leaves other VALU work ~1/5 of the issue time) while HBM has 6x headroom
    static constexpr int pX = 0, pH1 = 4 * DB * 64, pH2 = pH1 + 4 * HB * 64, pXi = pH2 + 4 * HB * 64, PB = pXi + 4 * DB * 64;
    // backward: 4 waves per workgroup arranged WH x WD over the (H-blocks x other-blocks) tile grids
    static constexpr int WH = (HB >= 4) ? 4 : (HB >= 2 ? 2 : 1);
    static constexpr int WD = 4 / WH;
    static constexpr int NIB = cdiv(HB, WH);     // H-blocks per wave along the WH axis
    static constexpr int NOBD = cdiv(DB, WD);    // d-blocks per wave along the WD axis
    static constexpr int NOBH = cdiv(HB, WD);    // H-blocks per wave along the WD axis (dW2 rows)
    // role-specialised backward (hjb_bwd2_kernel): per sample block the exchange area holds the G panel as
    // an exact k-step image (KSD x 64 floats) followed by the dz2 and dz1 panels; two buffers of 4 blocks
    static constexpr int EXB = KSD * 64 + 4 * HB * 64;
    static int bwd2_lds_floats() { return HB * KSD * 64 + 2 * 4 * EXB; }
};

// =======================================================================================
// Forward rollout kernel: Euler-Maruyama + control MLP + running cost, all N steps.
// Reference: solver.py:440-478 (step), :364-382 (init), :167-168 (D = Y - g).
// =======================================================================================
// BF16: the three products of the control net on v_mfma_f32_16x16x32_bf16 (bf16 operands, fp32 accumulate) -- an opt-in
// mode with its own tolerance (psp_hjb_config.mlp_dtype); the drift / sigma products, the state and every sum stay fp32.
// FAST: on-device noise, no u_L2 log, no time-feature table (decided at launch) -- the time loop of that instance has no
// vector-memory LOAD.  A load in a wave-uniform branch (the time feature of evaluation rollouts, supplied noise, the
// reference control) leaves an `s_waitcnt vmcnt(0)` at the join on the common path; vmcnt counts stores too and in order, so
// every step waited right behind its burst of 28 X-image stores for them to be acknowledged before the first product
// started.  Worth 1.3 % here (4.78 -> 4.72 ms, same-box A/B), 2 % in hjbs_fwd_kernel, 5 % in hjbq_fwd_kernel, whose steps
// are short; the larger part of the path store's cost stays (finding 7).
// FAST_ = 2 (round 4): a FAST instance whose problem switches are COMPILE-TIME too -- dense drift, dense sigma, adaptive process,
// no running cost, store_path 1 or 4, not the relative-entropy loss: the LLGC configuration of every BASELINE config.  The time loop of
// the general instance tests those wave-uniform switches at run time: ~100 scalar branches per step, each one a basic-block
// boundary that the scheduler cannot move the path stores, the Philox slices or the operand prefetches across.
// FAST_ = 3: the FAST_ = 2 instance for IDENTITY sigma -- the problem a plan hands over when it rolls the state out in the sigma
// basis (X~ = B^-1 X, plan_native.py: drift B^-1 A B, sigma I): the state panel is still split once for W1 x~ and (dt M) x~, the
// Philox slices stay in the W2 / W3 products, X~_{n+1} = Tn + v is element-wise; no B table is staged, no product of the v panel.
template <int D, int H, int MODE = 0, int FAST_ = 0>
__global__ __launch_bounds__(512) void hjb_fwd_kernel(const HjbArgs a) {
    PSP_COND_EXIT(a);
    constexpr bool FAST = FAST_ != 0, SPEC = FAST_ >= 2;
    // the problem switches: kernel arguments in the general instances, constants in the specialised ones
    const int k_drift = SPEC ? (int)DRIFT_DENSE : a.drift_kind;
    const int k_sigma = FAST_ == 3 ? (int)SIGMA_IDENT : SPEC ? (int)SIGMA_DENSE : a.sigma_kind;
    const int k_run = SPEC ? (int)RUN_ZERO : a.runcost_kind, k_loss = SPEC ? (int)LOSS_LOGVAR : a.loss_kind;
    const int k_store = a.store_path;                             // (SPEC: 1 or 4 -- the xi image is kept or regenerated; ONE instance for both,
                                                                  //  so that the two modes stay bit-identical: tests/test_gpu_path_noise.py)
    const bool k_adaptive = SPEC ? true : (a.adaptive != 0);
    const uint32_t iter_now = a.iter_dev ? *a.iter_dev : a.iter;       // wave-uniform scalar load
    using G = Geo<D, H>;
    constexpr int DB = G::DB, HB = G::HB, KSD = G::KSD, KSH = G::KSH;
    // MODE 0: fp32 MFMA; 1 (BF16): control net on bf16 MFMA; 2 (X3): every product fp32-grade on the f16 pipe (gemm_Tx)
    constexpr bool BF16 = MODE == 1, X3 = MODE == 2;
    constexpr int oW1 = X3 ? G::xW1 : G::fW1, oW2 = X3 ? G::xW2 : G::fW2, oW3 = X3 ? G::xW3 : G::fW3;
    constexpr int VEC = X3 ? G::xVec : G::fVec;              // the vectors, the reduction area and the d x d tables follow
    constexpr int VSH = VEC - G::fVec;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, nthr = blockDim.x;
    const int lane = tid & 63, wave = tid >> 6, nwave = nthr >> 6;
    const int j = lane & 15, q = lane >> 4;

    // ---- stage weights (once per workgroup; parameters are constant during an iteration)
    const float* __restrict__ P = a.params;
    auto stage_net = [&](float* dst, int MB, int KS, int INB, auto src) {
        if constexpr (BF16) stage_aop_bf16(dst, MB, (INB + 1) / 2, tid, nthr, src);
        else stage_aop(dst, MB, KS, tid, nthr, src);
    };
    auto w1src = [&](int row, int col) { return (row < H && col < D) ? P[G::oW1 + row * (D + 1) + 1 + col] : 0.f; };
    auto w2src = [&](int row, int col) { return (row < H && col < H) ? P[G::oW2 + row * H + col] : 0.f; };
    auto w3src = [&](int row, int col) { return (row < D && col < H) ? P[G::oW3 + row * H + col] : 0.f; };
    if constexpr (X3) {
        stage_aop_x3<KSD, DB, kLgFwdA>(lds + oW1, HB, tid, nthr, w1src);
        stage_aop_x3<KSH, HB, kLgFwdA>(lds + oW2, HB, tid, nthr, w2src);
        stage_aop_x3<KSH, HB, kLgFwdA>(lds + oW3, DB, tid, nthr, w3src);
    } else {
        stage_net(lds + oW1, HB, KSD, DB, w1src);
        stage_net(lds + oW2, HB, KSH, HB, w2src);
        stage_net(lds + oW3, DB, KSH, HB, w3src);
    }
    float* ldsA = lds + G::fA + VSH;
    float* ldsB = ldsA + (k_drift == DRIFT_DENSE ? (X3 ? G::xB_dense_off : G::fB_dense_off) : 0);
    if (k_drift == DRIFT_DENSE) {
        const float dt = a.dt;
        const float* __restrict__ A = a.drift;
        auto asrc = [&](int row, int col) { return (row < D && col < D) ? dt * A[row * D + col] : 0.f; };
        if constexpr (X3) stage_aop_x3<KSD, DB, kLgFwdA>(ldsA, DB, tid, nthr, asrc);
        else stage_aop(ldsA, DB, KSD, tid, nthr, asrc);
    }
    if (k_sigma == SIGMA_DENSE) {
        const float* __restrict__ B = a.sigma;
        auto bsrc = [&](int row, int col) { return (row < D && col < D) ? B[row * D + col] : 0.f; };
        if constexpr (X3) stage_aop_x3<KSD, DB, kLgFwdA>(ldsB, DB, tid, nthr, bsrc);
        else stage_aop(ldsB, DB, KSD, tid, nthr, bsrc);
    }
    // X3: the products are one-accumulator split products (gemm_Tx ONE) -- every accumulator of the control net holds 2048 x its
    // value, so the vectors that initialise them are staged times 2048 (exact)
    constexpr float kAcc = X3 ? kSplitScale : 1.0f, kAccInv = X3 ? kSplitInv : 1.0f;
    stage_vec(lds + VSH + G::vb1, HB, tid, nthr, [&](int f) { return f < H ? kAcc * P[G::ob1 + f] : 0.f; });
    stage_vec(lds + VSH + G::vw1t, HB, tid, nthr, [&](int f) { return f < H ? kAcc * P[G::oW1 + f * (D + 1)] : 0.f; });
    stage_vec(lds + VSH + G::vb2, HB, tid, nthr, [&](int f) { return f < H ? kAcc * P[G::ob2 + f] : 0.f; });
    stage_vec(lds + VSH + G::vb3, DB, tid, nthr, [&](int f) { return f < D ? kAcc * P[G::ob3 + f] : 0.f; });
    stage_vec(lds + VSH + G::vdr, DB, tid, nthr, [&](int f) {
        return (f < D && (k_drift == DRIFT_DIAG || k_drift == DRIFT_DWELL)) ? a.drift[f] : 0.f; });
    stage_vec(lds + VSH + G::vrun, DB, tid, nthr, [&](int f) {
        return (f < D && k_run == RUN_DIAGQ) ? a.runcost[f] : 0.f; });
    stage_vec(lds + VSH + G::vterm, DB, tid, nthr, [&](int f) { return f < D ? a.term[f] : 0.f; });
    __syncthreads();

    const int t16 = blockIdx.x * nwave + wave;        // 16-trajectory tile owned by this wave
    const bool wave_valid = t16 < a.ntile16;
    const int k = t16 * 16 + j;                        // local trajectory of this lane
    const bool kvalid = wave_valid && k < a.K_local;
    const uint32_t kglob = (uint32_t)(a.k_offset + k);
    const float dt = a.dt, sqdt = a.sqdt;

    const float store_cxi = SPEC ? 1.f : ((k_store == 3) ? 0.f : 1.f);     // image in the xi slot: c_xi xi + c_z Z
    const float store_cz = kAccInv * (SPEC ? 0.f : ((k_store == 3) ? 1.f : (k_store == 2 ? -a.sqdt : (k_adaptive ? 0.f : a.sqdt))));
    // FAST instances always keep the path (the launcher sends store_path = 0 to the general instance): without the
    // wave-uniform branch the stores share a scheduling region with the products instead of standing as bursts of 28 - 32
    const bool do_store = FAST ? true : (k_store != 0);
    double sD = 0.0, sD2 = 0.0;
    if (wave_valid) {
        // per-lane-q views of the staged vectors
        const f32x4* vecs0 = reinterpret_cast<const f32x4*>(lds + VEC) + q;   // index by block*4
        const f32x4* vterm = vecs0 + (G::vterm - G::fVec) / 4;

        // ---- X_0 (solver.py:365-367) in T layout
        f32x4 X[DB];
#pragma unroll
        for (int b = 0; b < DB; ++b) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int f = 16 * b + 4 * r + q;
                const float v = a.x0[(size_t)(kvalid ? k : 0) * a.x0_stride + (f < D ? f : D - 1)];
                X[b][r] = (f < D && kvalid) ? v : 0.f;
            }
        }
        float Y = a.y0 ? a.y0[0] : 0.f;               // solver.py:368 / :373
        float Fsum = 0.f, ULsum = 0.f;
#ifdef PSP_STAMPS
        unsigned long long stamps[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#endif

        for (int n = 0; n < a.N; ++n) {
            PSP_STAMP(fs0);
            // solver.py:355: ones * n * delta_t ; evaluation rollouts pass the table of solver.py:360-362
            float tn = (float)n * dt;
            if constexpr (!FAST) { if (a.tfeat) tn = a.tfeat[n]; }
            const f32x4* vecs = opaque(vecs0);         // re-read the small vectors each step (no hoisting)
            const f32x4* vb1 = vecs + (G::vb1 - G::fVec) / 4;
            const f32x4* vw1t = vecs + (G::vw1t - G::fVec) / 4;
            const f32x4* vb2 = vecs + (G::vb2 - G::fVec) / 4;
            const f32x4* vb3 = vecs + (G::vb3 - G::fVec) / 4;
            const f32x4* vdr = vecs + (G::vdr - G::fVec) / 4;
            const f32x4* vrun = vecs + (G::vrun - G::fVec) / 4;
            float* pblk = a.path + ((size_t)n * a.ntile16 + t16) * (size_t)G::PB + lane;
            // portion [u n / NU, (u + 1) n / NU) of n stores behind unit u of NU (split-product instances: see gemm_Tx)
            auto x_store = [&](int u, int NU) __attribute__((always_inline)) {
                if (do_store) {
#pragma unroll
                    for (int ks = 0; ks < 4 * DB; ++ks)
                        if (ks >= u * (4 * DB) / NU && ks < (u + 1) * (4 * DB) / NU)
                            PSP_PATH_STORE(pblk + (G::pX / 64 + ks) * 64, X[ks >> 2][ks & 3]);
                }
            };
            if (!X3 && do_store) {
#pragma unroll
                for (int ks = 0; ks < 4 * DB; ++ks) PSP_PATH_STORE(pblk + (G::pX / 64 + ks) * 64, X[ks >> 2][ks & 3]);
            }
            // ---- control net: Z = W3 tanh(W2 tanh(W1 [t,x] + b1) + b2) + b3 (function_space.py:190-195)
            f32x4 h1[HB];
#pragma unroll
            for (int m = 0; m < HB; ++m) h1[m] = vb1[m * 4] + tn * vw1t[m * 4];
            // split products with a dense drift: the state panel is split ONCE for W1 x and (dt A) x (Tn = X + dt A X is formed
            // here, next to the first layer, instead of after the control)
            f32x4 Tn[DB];
            const bool early_drift = X3 && k_drift == DRIFT_DENSE;
            if constexpr (X3) {
                if (k_drift == DRIFT_DENSE) {
                    f16x8 xh[DB / 2 > 0 ? DB / 2 : 1], xl[DB / 2 > 0 ? DB / 2 : 1];
                    constexpr int NU1 = (DB / 2) * HB, NU2 = (DB / 2) * DB;
                    split_panel8<DB>(X, xh, xl);
                    gemm_Txs<HB, KSD, DB, 2>(h1, lds + oW1, xh, xl, X[DB - 1], lane, [&](int u) __attribute__((always_inline)) { x_store(u, NU1 + NU2); });
#pragma unroll
                    for (int b = 0; b < DB; ++b) Tn[b] = f32x4{0.f, 0.f, 0.f, 0.f};             // 2048 (dt A) X; X joins it in the update below
                    gemm_Txs<DB, KSD, DB, 2>(Tn, ldsA, xh, xl, X[DB - 1], lane, [&](int u) __attribute__((always_inline)) { x_store(NU1 + u, NU1 + NU2); });
                    if constexpr (NU1 + NU2 == 0) x_store(0, 1);
                } else {
                    constexpr int NU1 = (DB / 2) * HB;
                    gemm_Tx<HB, KSD, DB, 2, true>(h1, lds + oW1, X, lane, [&](int u) __attribute__((always_inline)) { x_store(u, NU1); });
                    if constexpr (NU1 == 0) x_store(0, 1);
                }
            }
            else if constexpr (BF16) gemm_Tb<HB, DB>(h1, lds + oW1, X, lane);
            else gemm_T<HB, KSD, DB>(h1, lds + oW1, X, lane);
            PSP_STAMP(fs1);
#pragma unroll
            for (int m = 0; m < HB; ++m) h1[m] = tanh4<X3>(h1[m]);
            PSP_STAMP(fs2);
            f32x4 h2[HB];
#pragma unroll
            for (int m = 0; m < HB; ++m) h2[m] = vb2[m * 4];
            // Split-product FAST instances: the Brownian increments of this step are generated IN the W2 and W3 products --
            // the (R + 1) DB slices of the step's Philox calls (the R rounds and the Box-Muller finish per call) are dealt out over the
            // products' units and stand between their MFMAs.  An f16 MFMA stream hides three VALU instructions per MFMA
            // completely, even within one wave (tools/r3/ubench/mfma_valu_overlap.hip: 1 MFMA + 3 VALU 11.9 ns against 14.8 ns for
            // the MFMA alone); the noise was 22 % of the step standing by itself.  Bit-identical to philox_block.
            constexpr int NUH2 = (HB / 2) * HB, NUH3 = (HB / 2) * DB;
            constexpr bool PREGEN = X3 && FAST && (NUH2 + NUH3 > 0);
            [[maybe_unused]] f32x4 xig[PREGEN ? DB : 1];
            [[maybe_unused]] uint32_t pc0 = 0, pc1 = 0, pc2 = 0, pc3 = 0;
            constexpr int NSPC = kPhiloxRounds + 1;                                // slices per call: the rounds, then the Box-Muller finish
            auto philox_slice = [&](int sidx) __attribute__((always_inline)) {
                const int b = sidx / NSPC, sub = sidx % NSPC;
                if (sub == 0) { pc0 = kglob; pc1 = (uint32_t)n; pc2 = (uint32_t)(4 * b + q); pc3 = iter_now; }
                if (sub < kPhiloxRounds) {
                    philox_round(pc0, pc1, pc2, pc3, a.seed_lo + (uint32_t)sub * 0x9E3779B9u, a.seed_hi + (uint32_t)sub * 0xBB67AE85u);
                    // (pins the round to this unit: pure arithmetic is otherwise sunk to its use in the noise phase, past the fences)
                    asm volatile("" : "+v"(pc0), "+v"(pc1), "+v"(pc2), "+v"(pc3));
                } else {
                    const uint32_t rr[4] = {pc0, pc1, pc2, pc3};
                    f32x4 xi = normal4(rr);
                    if (16 * b + 16 > D) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) if (16 * b + 4 * r + q >= D) xi[r] = 0.f;
                    }
                    asm volatile("" : "+v"(xi));
                    xig[b < DB ? b : 0] = xi;
                }
            };
            auto philox_portion = [&](int u) __attribute__((always_inline)) {      // slices of unit u of the NUH2 + NUH3 units
                if constexpr (PREGEN) {
#pragma unroll
                    for (int sidx = 0; sidx < NSPC * DB; ++sidx)
                        if (sidx >= u * (NSPC * DB) / (NUH2 + NUH3) && sidx < (u + 1) * (NSPC * DB) / (NUH2 + NUH3)) philox_slice(sidx);
                }
            };
            // hidden activations for the backward pass (no recompute); split-product instances: h1 between the units of the
            // W2 product, h2 between those of the W3 product
            auto h_store = [&](const f32x4 (&h)[HB], int slot, int u, int NU) __attribute__((always_inline)) {
                if (do_store) {
#pragma unroll
                    for (int ks = 0; ks < 4 * HB; ++ks)
                        if (ks >= u * (4 * HB) / NU && ks < (u + 1) * (4 * HB) / NU)
                            PSP_PATH_STORE(pblk + (slot / 64 + ks) * 64, h[ks >> 2][ks & 3]);
                }
            };
            if constexpr (X3) {
                gemm_Tx<HB, KSH, HB, 2, true>(h2, lds + oW2, h1, lane, [&](int u) __attribute__((always_inline)) { h_store(h1, G::pH1, u, NUH2); philox_portion(u); });
                if constexpr (NUH2 == 0) h_store(h1, G::pH1, 0, 1);
            }
            else if constexpr (BF16) gemm_Tb<HB, HB>(h2, lds + oW2, h1, lane);
            else gemm_T<HB, KSH, HB>(h2, lds + oW2, h1, lane);
#pragma unroll
            for (int m = 0; m < HB; ++m) h2[m] = tanh4<X3>(h2[m]);
            if (!X3 && do_store) {
#pragma unroll
                for (int ks = 0; ks < 4 * HB; ++ks) {
                    PSP_PATH_STORE(pblk + (G::pH1 / 64 + ks) * 64, h1[ks >> 2][ks & 3]);
                    PSP_PATH_STORE(pblk + (G::pH2 / 64 + ks) * 64, h2[ks >> 2][ks & 3]);
                }
            }
            f32x4 Z[DB];
#pragma unroll
            for (int m = 0; m < DB; ++m) Z[m] = vb3[m * 4];
            if constexpr (X3) {
                gemm_Tx<DB, KSH, HB, 2, true>(Z, lds + oW3, h2, lane, [&](int u) __attribute__((always_inline)) { h_store(h2, G::pH2, u, NUH3); philox_portion(NUH2 + u); });
                if constexpr (NUH3 == 0) h_store(h2, G::pH2, 0, 1);
            }
            else if constexpr (BF16) gemm_Tb<DB, HB>(Z, lds + oW3, h2, lane);
            else gemm_T<DB, KSH, HB>(Z, lds + oW3, h2, lane);
            PSP_STAMP(fs3);

            // ---- Brownian increment xi_{n+1} and the two row sums |Z|^2, Z.xi (solver.py:477-478)
            // (X3: Z holds 2048 Z.  The row sums are formed of it and rescaled once per lane; the stored image, the u_L2 term
            // and the increment v take the 2^-11 in a coefficient they have anyway.)
            float S = 0.f, Pz = 0.f, UL = 0.f;
#pragma unroll
            for (int b = 0; b < DB; ++b) {
                f32x4 xi;
                if constexpr (PREGEN) {
                    xi = xig[b];
                } else if (FAST || a.noise_mode == NOISE_PHILOX) {
                    xi = philox_block(kglob, (uint32_t)n, (uint32_t)(4 * b + q), iter_now, a.seed_lo, a.seed_hi);
                } else {
                    // unconditional clamped loads + select: no per-element branch around the load
                    const float* xrow = a.xi + ((size_t)(n + 1) * a.K_local + (kvalid ? k : 0)) * D;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int f = 16 * b + 4 * r + q;
                        const float v = xrow[f < D ? f : D - 1];
                        xi[r] = (f < D && kvalid) ? v : 0.f;
                    }
                }
                if (16 * b + 16 > D) {                 // partial last block: keep padded features at zero
#pragma unroll
                    for (int r = 0; r < 4; ++r) if (16 * b + 4 * r + q >= D) xi[r] = 0.f;
                }
                if (do_store && k_store != 4) {   // (4: the backward regenerates xi from the Philox counters)
                    // 1: xi, or xi + sqrt(dt) Z when the forward process is NOT adaptive (then dL/dZ_n = w (Z dt + xi sqrt(dt))
                    //    = w sqrt(dt) * image, the same expression the backward kernels evaluate); attached process (hjba_kernels.h):
                    // 2: xi - sqrt(dt) Z, 3: Z  -- the adjoint sweep replaces it by dL/dZ_n / sqrt(dt)
                    // (as an affine combination with wave-uniform coefficients: a nested vector select here was lowered to
                    // a switch whose Z arm read a stale accumulator)
                    const f32x4 wv = store_cxi * xi + store_cz * Z[b];
#pragma unroll
                    for (int r = 0; r < 4; ++r) PSP_PATH_STORE(pblk + (G::pXi / 64 + 4 * b + r) * 64, wv[r]);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    S = fmaf(Z[b][r], Z[b][r], S);
                    Pz = fmaf(Z[b][r], xi[r], Pz);
                }
                if (!FAST && a.uref) {                 // u_L2 logging: |-Z_n - u*(t_n)|^2 (solver.py:491-494)
                    const float* ur = a.uref + (size_t)n * D;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int f = 16 * b + 4 * r + q;
                        const float e = (f < D) ? (X3 ? fmaf(Z[b][r], kSplitInv, ur[f < D ? f : D - 1]) : Z[b][r] + ur[f < D ? f : D - 1]) : 0.f;
                        UL = fmaf(e, e, UL);
                    }
                }
                // v = c dt + xi sqrt(dt), c = -Z (adaptive) or 0  (solver.py:451-456,471-472)
                if constexpr (X3) Z[b] = k_adaptive ? (sqdt * xi - (dt * kSplitInv) * Z[b]) : (sqdt * xi);
                else Z[b] = k_adaptive ? (sqdt * xi - dt * Z[b]) : (sqdt * xi);
            }
            ULsum = fmaf(UL, dt, ULsum);
            S = qsum(S);
            Pz = qsum(Pz);
            if constexpr (X3) { S *= kSplitInv * kSplitInv; Pz *= kSplitInv; }
            PSP_STAMP(fs4);

            // ---- X_{n+1} = X + b(X) dt + sigma v      (solver.py:471-472)
            if (!early_drift) {
#pragma unroll
                for (int b = 0; b < DB; ++b) Tn[b] = X[b];
            } else {
#pragma unroll
                for (int b = 0; b < DB; ++b) Tn[b] = X[b] + kSplitInv * Tn[b];        // X + (dt A) X of the first layer's pass
            }
            if (k_drift == DRIFT_DENSE) {
                if constexpr (!X3) gemm_T<DB, KSD, DB>(Tn, ldsA, X, lane);     // + (dt A) X
            } else if (k_drift == DRIFT_DIAG) {
#pragma unroll
                for (int b = 0; b < DB; ++b) Tn[b] += dt * (vdr[b * 4] * X[b]);
            } else if (k_drift == DRIFT_DWELL) {            // b = -4 kappa x (x^2 - 1), problems.py:311-315
#pragma unroll
                for (int b = 0; b < DB; ++b) Tn[b] -= dt * (4.0f * vdr[b * 4] * (X[b] * (X[b] * X[b] - 1.0f)));
            }
            if (k_sigma == SIGMA_DENSE) {
                if constexpr (X3) {
                    f32x4 Bv[DB];
#pragma unroll
                    for (int b = 0; b < DB; ++b) Bv[b] = f32x4{0.f, 0.f, 0.f, 0.f};
                    gemm_Tx<DB, KSD, DB, 2, true>(Bv, ldsB, Z, lane);
#pragma unroll
                    for (int b = 0; b < DB; ++b) Tn[b] = Tn[b] + kSplitInv * Bv[b];
                }
                else gemm_T<DB, KSD, DB>(Tn, ldsB, Z, lane);     // + B v
            } else if (k_sigma == SIGMA_SCALE) {
#pragma unroll
                for (int b = 0; b < DB; ++b) Tn[b] += a.sigma_scale * Z[b];
            } else {
#pragma unroll
                for (int b = 0; b < DB; ++b) Tn[b] += Z[b];
            }
#pragma unroll
            for (int b = 0; b < DB; ++b) X[b] = Tn[b];
            PSP_STAMP(fs5);

            // ---- running cost f(X_{n+1}) (h sees the UPDATED state, solver.py:477) and Y update
            float fX = 0.f;
            if (k_run == RUN_DIAGQ) {
#pragma unroll
                for (int b = 0; b < DB; ++b) {
                    const f32x4 pv = vrun[b * 4];
#pragma unroll
                    for (int r = 0; r < 4; ++r) fX = fmaf(pv[r] * X[b][r], X[b][r], fX);
                }
                fX = qsum(fX);
            }
            // Y += (-h + Z.c) dt + Z.xi sqrt(dt);  -h = 0.5|Z|^2 + f ; Z.c = -|Z|^2 (adaptive) or 0
            if (k_loss == LOSS_RELENT) {
                // relative entropy (solver.py:179-180, 484-486): Y carries -Zsum = -sum (|Z|^2 / 2 + f(X_{n+1})) dt,
                // so D = Y - g = -(Zsum + g) and the loss is -mean D
                Y = Y - (0.5f * S + fX) * dt;
            } else {
                const float drift_y = k_adaptive ? (fX - 0.5f * S) : (fX + 0.5f * S);
                Y = Y + drift_y * dt + Pz * sqdt;
            }
            Fsum = fmaf(fX, dt, Fsum);
            PSP_STAMP(fs6);
            PSP_ACC(0, fs1, fs0);   // path store of X + L1 GEMM
            PSP_ACC(1, fs2, fs1);   // tanh 1
            PSP_ACC(2, fs3, fs2);   // L2 + tanh 2 + h store + L3
            PSP_ACC(3, fs4, fs3);   // noise + row sums
            PSP_ACC(4, fs5, fs4);   // SDE GEMMs
            PSP_ACC(5, fs6, fs5);   // running cost + Y
            PSP_ACC(6, fs6, fs0);   // whole step
        }
#ifdef PSP_STAMPS
        if (a.dbg && lane == 0) {
            stamps[7] = (unsigned long long)a.N;
            for (int i = 0; i < 8; ++i) a.dbg[((size_t)blockIdx.x * 8 + wave) * 8 + i] = stamps[i];
        }
#endif

        // ---- terminal cost g(X_N) and D = Y - g  (problems.py:49,164,334; solver.py:167-168)
        float g = 0.f;
#pragma unroll
        for (int b = 0; b < DB; ++b) {
            const f32x4 tv = vterm[b * 4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float x = X[b][r];
                if (a.term_kind == TERM_LINEAR) g = fmaf(tv[r], x, g);
                else if (a.term_kind == TERM_DIAGQ) g = fmaf(tv[r] * x, x, g);
                else g = fmaf(tv[r] * (x - 1.0f), (x - 1.0f), g);
            }
        }
        g = qsum(g);
        const float Dk = Y - g;
        if (kvalid && q == 0) a.D[k] = Dk;
        if (a.Fint && kvalid && q == 0) a.Fint[k] = Fsum;
        if (a.uref) {
            const float ULt = qsum(ULsum);
            if (kvalid && q == 0) a.ul2[k] = ULt;
        }
        if (a.Yout && kvalid && q == 0) a.Yout[k] = Y;
        if (a.XN && kvalid) {
#pragma unroll
            for (int b = 0; b < DB; ++b)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int f = 16 * b + 4 * r + q;
                    if (f < D) a.XN[(size_t)k * D + f] = X[b][r];
                }
        }
        if (kvalid && q == 0) { sD = (double)Dk; sD2 = (double)Dk * (double)Dk; }
    }
    // ---- per-workgroup partial (sum D, sum D^2) in fp64, fixed order
    sD = jsum(sD); sD2 = jsum(sD2);
    double* red = reinterpret_cast<double*>(lds + G::fRed + VSH);
    if (lane == 0) { red[2 * wave] = sD; red[2 * wave + 1] = sD2; }
    __syncthreads();
    if (tid == 0) {
        double t0 = 0.0, t1 = 0.0;
        for (int w = 0; w < nwave; ++w) { t0 += red[2 * w]; t1 += red[2 * w + 1]; }
        a.fwd_partial[2 * blockIdx.x] = t0;
        a.fwd_partial[2 * blockIdx.x + 1] = t1;
    }
}

// =======================================================================================
// Backward kernel: analytic gradient of the loss w.r.t. the control-net parameters.
// With detach_forward=True the state path carries no gradient (solver.py:468-472), so
//   dL/dZ_n[k,:] = w_k ((Z_n + c) dt + xi_{n+1} sqrt(dt)),  (Z + c = 0 when adaptive)
// and the parameter gradient is one batched MLP backward over all (n, k) samples, using the
// X_n, h1, h2 panels the forward kernel stored (register-image layout); workgroups are summed by
// reduce_grad_kernel in a fixed order.
// =======================================================================================
__device__ __forceinline__ void tile_put(float* tile, f32x4 v, int lane) {
    tile[lane] = v[0]; tile[64 + lane] = v[1]; tile[128 + lane] = v[2]; tile[192 + lane] = v[3];
}
__device__ __forceinline__ f32x4 tile_get(const float* tile, int lane) {
    return *reinterpret_cast<const f32x4*>(tile + (lane & 15) * 16 + 4 * (lane >> 4));
}
// Feature-on-lane read of one 16-feature block (1 KiB, wave-uniform pointer) of a stored register
// image: lane (i, q') gets feature i of samples 4q'..4q'+3.  Image element (ks, j + 16 q) = feature
// 4ks+q, sample j, so the lane offset is 64 (i>>2) + 16 (i&3) + 4 q' floats -- the same for every block.
__device__ __forceinline__ int image_lane_offset_F(int lane) {
    const int i = lane & 15, qq = lane >> 4;
    return 64 * (i >> 2) + 16 * (i & 3) + 4 * qq;
}
__device__ __forceinline__ f32x4 image_get_F(const float* block, int lofs) {
    return *reinterpret_cast<const f32x4*>(block + lofs);
}
// accumulate-in-place MFMA (vDst tied to SrcC): keeps a persistent accumulator in ONE register quad across a
// long unrolled stream (the builtin lets the allocator rename it, which costs copies and spills there).
// Only for accumulators that no VALU / store reads until well after the stream (no hazard tracking in asm).
__device__ __forceinline__ void mfma16_inplace(f32x4& c, float a, float b) {
    asm volatile("v_mfma_f32_16x16x4_f32 %0, %1, %2, %0" : "+v"(c) : "v"(a), "v"(b));
}
__device__ __forceinline__ float hsum4(f32x4 v) { return (v[0] + v[1]) + (v[2] + v[3]); }

// =======================================================================================
// Backward kernel, role-specialised variant (adaptive forward process only).
// One 8-wave workgroup per CU.  Waves 0-3 are PRODUCERS: each forms G, dz2, dz1 of one sample block
// (Philox + two data-gradient GEMMs: VALU-heavy, no persistent accumulators) and writes the three
// panels to the LDS exchange buffer of the NEXT round.  Waves 4-7 are CONSUMERS: each owns a fixed
// subset of the weight-gradient tiles and contracts the CURRENT round's four blocks (MFMA-heavy).
// A producer and a consumer share every SIMD, so the VALU work of one fills the MFMA shadows of the
// other by construction instead of by the accident of two workgroups being out of phase; the two
// exchange buffers are swapped at the single barrier per round.
// =======================================================================================
template <int D, int H>
__global__ __launch_bounds__(512) void hjb_bwd2_kernel(const HjbArgs a) {
    PSP_COND_EXIT(a);
    using G = Geo<D, H>;
    constexpr int DB = G::DB, HB = G::HB, KSD = G::KSD, KSH = G::KSH, EXB = G::EXB;
    constexpr int WH = G::WH, WD = G::WD, NIB = G::NIB, NOBD = G::NOBD, NOBH = G::NOBH;
    constexpr int oDZ2 = KSD * 64;                                     // dz2 panel inside one block's exchange area
    constexpr int RS = 16 * DB + 16 * HB;                              // per-producer bias-sum slots (G | dz2)
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, nthr = blockDim.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 15, q = lane >> 4;
    const bool producer = wave < 4;
    const int sub = wave & 3;                         // producer: block within the round; consumer: tile subset
    const int wh = (WH == 1) ? 0 : sub % WH, wd = (WD == 1) ? 0 : sub / WH;
    const int lofsF = image_lane_offset_F(lane);
    const float* __restrict__ P = a.params;

    stage_aop(lds, HB, KSD, tid, nthr, [&](int row, int col) {          // W3^T as A-operand table (producers)
        return (row < H && col < D) ? P[G::oW3 + col * H + row] : 0.f; });
    __syncthreads();
    float* bufs = lds + HB * KSD * 64;                // [2 buffers][4 blocks][EXB]
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};

    const double invK = 1.0 / (double)a.K_global;
    const float meanD = (a.loss_kind == LOSS_LOGVAR) ? (float)(a.sums[0] * invK) : 0.f;
    const float coef = (float)(2.0 * invK);
    const bool regen = a.store_path == 4;                       // xi from the Philox counters instead of the path store
    const uint32_t iter_now = a.iter_dev ? *a.iter_dev : a.iter;
    const float sqdt = a.sqdt, dt = a.dt;
    const long long nblk = (long long)a.N * a.ntile16;
    const long long nround = (nblk + 3) / 4;
    const int R = (int)((nround - blockIdx.x + gridDim.x - 1) / gridDim.x);   // rounds of this workgroup (>= 1)

    if (producer) {
        // ================================================================================ producers
        // Per block: G = w sqrt(dt) xi (xi loaded from the path store), dz2 = (W3^T G)(1 - h2^2); both panels go to
        // the exchange buffer of the next round.  db3 = sum G and db2 = sum dz2 are kept as element-wise running
        // sums in registers (reduced over the wave's 16 trajectories once, after the loop).
        f32x4 sG[DB], sZ2[HB];
#pragma unroll
        for (int b = 0; b < DB; ++b) sG[b] = zero4;
#pragma unroll
        for (int m = 0; m < HB; ++m) sZ2[m] = zero4;
#ifdef PSP_STAMPS
        unsigned long long stamps[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#endif
        // software pipeline over this wave's blocks: xi and the trajectory weight of the NEXT round are requested at
        // the top of an iteration (a whole iteration of lead), h2 of the current block right after G is formed
        // (consumed after the GEMM)
        // this wave's block of the current round and of the next (block_index.h: no division in the round loop); a slot outside
        // the store rests on the stand-in block nblk - 1, with weight zero
        BlockCursor cur = BlockCursor::start(blockIdx.x, (uint32_t)sub, gridDim.x, (uint32_t)a.ntile16, (uint32_t)a.N);
        BlockCursor nxt = cur;
        nxt.advance();
        f32x4 xin[DB];
        float dkn;
        {
            const float* pb = a.path + (size_t)cur.blk * (size_t)G::PB + lane;
            const int k0 = (int)cur.t16 * 16 + j;
            dkn = a.D[k0 < a.K_local ? k0 : 0];
            if (regen) {
                regen_xi<D, DB>(xin, (uint32_t)(a.k_offset + k0), cur.n, q, iter_now, a.seed_lo, a.seed_hi);
            } else {
#pragma unroll
                for (int b = 0; b < DB; ++b)
#pragma unroll
                    for (int r = 0; r < 4; ++r) xin[b][r] = pb[G::pXi + (4 * b + r) * 64];
            }
        }
        for (int it = 0; it <= R; ++it) {
            PSP_STAMP(tp0);
            if (it < R) {
                // ---------------------------------------------------------- produce round r into bufs[it & 1]
                const int k = (int)cur.t16 * 16 + j;
                const bool kvalid = cur.valid && k < a.K_local;
                const float* pb = a.path + (size_t)cur.blk * (size_t)G::PB + lane;
                float* ex = bufs + ((it & 1) * 4 + sub) * EXB + lane;
                // LOSS_WEIGHTS: the caller supplies w_k = dLoss/dY_k directly in the D argument
                const float dk = dkn;
                const float wk = kvalid ? (a.loss_kind == LOSS_WEIGHTS ? dk : coef * (dk - meanD)) : 0.f;
                f32x4 Gt[DB];
#pragma unroll
                for (int b = 0; b < DB; ++b) {
                    Gt[b] = (wk * sqdt) * xin[b];                   // adaptive: the (Z + c) dt term cancels
                    sG[b] += Gt[b];
                }
                f32x4 h2[HB];
#pragma unroll
                for (int m = 0; m < HB; ++m)
#pragma unroll
                    for (int r = 0; r < 4; ++r) h2[m][r] = pb[G::pH2 + (4 * m + r) * 64];
                {
                    const float* pn = a.path + (size_t)nxt.blk * (size_t)G::PB + lane;
                    const int k1 = (int)nxt.t16 * 16 + j;
                    dkn = a.D[k1 < a.K_local ? k1 : 0];
                    if (regen) {
                        regen_xi<D, DB>(xin, (uint32_t)(a.k_offset + k1), nxt.n, q, iter_now, a.seed_lo, a.seed_hi);
                    } else {
#pragma unroll
                        for (int b = 0; b < DB; ++b)
#pragma unroll
                            for (int r = 0; r < 4; ++r) xin[b][r] = pn[G::pXi + (4 * b + r) * 64];
                    }
                }
                PSP_STAMP(tp1);
                PSP_ACC(0, tp1, tp0);                 // weights -> G, issue of this block's h2 loads and next round's xi
#pragma unroll
                for (int ks = 0; ks < KSD; ++ks) ex[ks * 64] = Gt[ks >> 2][ks & 3];     // exact k-step image of G
                f32x4 dz2[HB];
#pragma unroll
                for (int m = 0; m < HB; ++m) dz2[m] = zero4;
                gemm_T<HB, KSD, DB>(dz2, lds, Gt, lane);
#pragma unroll
                for (int m = 0; m < HB; ++m) { dz2[m] = dz2[m] * (1.0f - h2[m] * h2[m]); sZ2[m] += dz2[m]; }
                PSP_STAMP(tp2);
                PSP_ACC(1, tp2, tp1);                 // G store + GEMM W3^T G + tanh'
#pragma unroll
                for (int ks = 0; ks < 4 * HB; ++ks) ex[oDZ2 + ks * 64] = dz2[ks >> 2][ks & 3];
                PSP_STAMP(tp4);
                PSP_ACC(3, tp4, tp2);                 // dz2 store
                cur = nxt;                                // block it + 1 of this round is block it of the next
                nxt.advance();
            }
            PSP_STAMP(tp5);
            __syncthreads();                              // swap the exchange buffers (pairs with the consumer loop)
            PSP_STAMP(tp6);
            PSP_ACC(4, tp6, tp5);                     // barrier wait
            PSP_ACC(6, tp6, tp0);
        }
#ifdef PSP_STAMPS
        if (a.dbg && lane == 0) {
            stamps[7] = (unsigned long long)R;
            for (int i = 0; i < 8; ++i) a.dbg[((size_t)blockIdx.x * 8 + wave) * 8 + i] = stamps[i];
        }
#endif
        // per-wave bias sums -> LDS (the exchange area is free after the last barrier); lane (j = 0, q), component r
        // of block b holds feature 16 b + 4 r + q
        float* red = bufs + sub * RS;
#pragma unroll
        for (int b = 0; b < DB; ++b)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float v = jsumf(sG[b][r]);
                if (j == 0) red[16 * b + 4 * r + q] = v;
            }
#pragma unroll
        for (int m = 0; m < HB; ++m)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float v2 = jsumf(sZ2[m][r]);
                if (j == 0) red[16 * DB + 16 * m + 4 * r + q] = v2;
            }
        __syncthreads();                                  // pairs with the consumers' barrier before the bias write-out
        return;
    }
    // ==================================================================================== consumers
    // Wave `sub` owns hidden block(s) ib = wh + WH t of every weight-gradient tile row and, per sample block b:
    //   dz1 tile   = (dz2^T W2[:, ib])  (1 - h1^2)   computed HERE as the transposed product: the MFMA output layout
    //                (lane = feature, registers = samples) is exactly the A-operand layout the dW1 tiles need, W2's
    //                block stays in KSH registers, h1 is already loaded for dW2 -- no LDS round trip, no redundancy
    //   dW3 += G^T h2,  dW2 += dz2^T h1,  dW1 += dz1^T X_n,  db1 / time column += sums of the dz1 tile
    // HBM operands (feature-on-lane images) are requested a whole block ahead: h1(b+1), X(b+1) during layer 3 of
    // block b (into the other buffer), h2(b+1) during layers 2/1 of block b; LDS operands one phase ahead.
    // A wave issues in order, so everything that is not a weight-gradient MFMA is placed BETWEEN those MFMAs
    // (slot = one MFMA + a few auxiliary items, closed by a scheduling fence).
    f32x4 acc3[NOBD][NIB], acc2[NOBH][NIB], acc1[NIB][NOBD];
#pragma unroll
    for (int s = 0; s < NOBD; ++s)
#pragma unroll
        for (int t = 0; t < NIB; ++t) { acc3[s][t] = zero4; acc1[t][s] = zero4; }
#pragma unroll
    for (int s = 0; s < NOBH; ++s)
#pragma unroll
        for (int t = 0; t < NIB; ++t) acc2[s][t] = zero4;
    f32x4 bs1[NIB], bt1[NIB];                         // element-wise partial sums of the dz1 tiles (db1, time column)
#pragma unroll
    for (int t = 0; t < NIB; ++t) { bs1[t] = zero4; bt1[t] = zero4; }
    f32x4 oh2[NIB], oh1[2][NIB], ox[2][NOBD];         // HBM operands; h1 / X double-buffered
    f32x4 g3[NOBD], a2[NOBH], a1[NIB];                // G and dz2 tiles from LDS; dz1 tiles computed in registers
    float azk[4];                                     // rotating A operands (dz2 k-steps) of the dz1 product
    float w2b[NIB][KSH];                              // B operands of the dz1 product: W2[4 ks + q][16 ib + n]
    int ibc[NIB], obc[NOBD], o2c[NOBH];
#pragma unroll
    for (int t = 0; t < NIB; ++t) {
        const int hb = (wh + WH * t) < HB ? (wh + WH * t) : HB - 1;
        ibc[t] = hb * 256;
#pragma unroll
        for (int ks = 0; ks < KSH; ++ks) {
            const int o = 4 * ks + q, i = 16 * hb + j;
            w2b[t][ks] = (o < H && i < H) ? P[G::oW2 + o * H + i] : 0.f;
        }
    }
#pragma unroll
    for (int s2 = 0; s2 < NOBD; ++s2) obc[s2] = ((wd + WD * s2) < DB ? (wd + WD * s2) : DB - 1) * 256;
#pragma unroll
    for (int s2 = 0; s2 < NOBH; ++s2) o2c[s2] = oDZ2 + ((wd + WD * s2) < HB ? (wd + WD * s2) : HB - 1) * 256;
    const int nblk_i = (int)nblk;                     // N * ntile16 < 2^31 is checked by the host
    auto blk_at = [&](long long c0) __attribute__((always_inline)) {
        const int c = (c0 < (long long)nblk_i) ? (int)c0 : nblk_i - 1;
        return __builtin_amdgcn_readfirstlane(c);
    };
    // wave-uniform tile base pointers are forced into SGPRs so every load is "SGPR base + lane offset"
    typedef const __attribute__((address_space(1))) float* gptr_t;
    auto sbase = [&](int blk, int ofs) __attribute__((always_inline)) {
        return (gptr_t)sgpr_block_addr(a.path, (unsigned long long)blk, (unsigned)G::PB, (unsigned)ofs);
    };
    const unsigned lofsU = (unsigned)lofsF;
    auto get_F = [&](gptr_t base) __attribute__((always_inline)) {
        return *reinterpret_cast<const __attribute__((address_space(1))) f32x4*>(base + lofsU);
    };
    auto load_first = [&](int blk) __attribute__((always_inline)) {
#pragma unroll
        for (int t = 0; t < NIB; ++t) oh2[t] = get_F(sbase(blk, G::pH2 + ibc[t]));
#pragma unroll
        for (int t = 0; t < NIB; ++t) oh1[0][t] = get_F(sbase(blk, G::pH1 + ibc[t]));
#pragma unroll
        for (int s2 = 0; s2 < NOBD; ++s2) ox[0][s2] = get_F(sbase(blk, G::pX + obc[s2]));
    };
    auto load_lds_first = [&](const float* ex) __attribute__((always_inline)) {     // round start: G tiles, first dz2 k-steps
#pragma unroll
        for (int s2 = 0; s2 < NOBD; ++s2) g3[s2] = tile_get(ex + obc[s2], lane);
#pragma unroll
        for (int i = 0; i < 4; ++i) azk[i] = ex[oDZ2 + i * 64 + lane];
    };
    // ---- layer 3 of block cb (buffer pb): dW3 += G^T h2, and the dz1 tile;
    //      fetch h1(nb), X(nb) from HBM/L2, the dz2 tiles and the remaining dz2 k-steps of this block from LDS
    auto phase_l3 = [&](int pb, int cb, int nb, const float* ex) __attribute__((always_inline)) {
        constexpr int nM = 4 * NOBD * NIB, nC = KSH * NIB, nAux = NIB + NOBD + NOBH, kPer = (nAux + nM - 1) / nM;
        f32x4 dzt[NIB];
#pragma unroll
        for (int t = 0; t < NIB; ++t) dzt[t] = zero4;
        auto aux = [&](int u) __attribute__((always_inline)) {
            if (u < NIB) { oh1[pb ^ 1][u] = get_F(sbase(nb, G::pH1 + ibc[u])); return; }
            u -= NIB;
            if (u < NOBD) { ox[pb ^ 1][u] = get_F(sbase(nb, G::pX + obc[u])); return; }
            u -= NOBD;
            if (u < NOBH) a2[u] = tile_get(ex + o2c[u], lane);
        };
#pragma unroll
        for (int m = 0; m < nM; ++m) {
            const int r = m / (NOBD * NIB), s2 = (m % (NOBD * NIB)) / NIB, t = m % NIB;
            mfma16_inplace(acc3[s2][t], g3[s2][r], oh2[t][r]);
#pragma unroll
            for (int c = 0; c < nC; ++c) {                       // dz1 product, spread evenly over the slots
                if (c * nM / nC == m) {
                    const int ks = c / NIB, tt = c % NIB;
                    dzt[tt] = mfma16(azk[ks & 3], w2b[tt][ks], dzt[tt]);
                    if (tt == NIB - 1 && ks + 4 < KSH) azk[ks & 3] = ex[oDZ2 + (ks + 4) * 64 + lane];
                }
            }
#pragma unroll
            for (int c = 0; c < kPer; ++c) aux(m * kPer + c);
            __builtin_amdgcn_sched_barrier(0);
        }
        const float tn = (float)(cb / a.ntile16) * dt;
#pragma unroll
        for (int t = 0; t < NIB; ++t) {
            a1[t] = dzt[t] * (1.0f - oh1[pb][t] * oh1[pb][t]);
            bs1[t] += a1[t];
            bt1[t] += tn * a1[t];
        }
        __builtin_amdgcn_sched_barrier(0);
    };
    // ---- layers 2 and 1 of block b (buffer pb): dW2 += dz2^T h1, dW1 += dz1^T X_n;
    //      fetch h2(nb) from HBM/L2 and, inside a round, the next block's G tiles and first dz2 k-steps from LDS
    auto phase_l21 = [&](int pb, int nb, const float* exn) __attribute__((always_inline)) {
        constexpr int nT = (NOBH + NOBD) * NIB, nM = 4 * nT, nAux = NIB + NOBD + 4, kPer = (nAux + nM - 1) / nM;
        auto aux = [&](int u) __attribute__((always_inline)) {
            if (u < NIB) { oh2[u] = get_F(sbase(nb, G::pH2 + ibc[u])); return; }
            u -= NIB;
            if (u < NOBD) { if (exn) g3[u] = tile_get(exn + obc[u], lane); return; }
            u -= NOBD;
            if (u < 4) { if (exn) azk[u] = exn[oDZ2 + u * 64 + lane]; }
        };
#pragma unroll
        for (int m = 0; m < nM; ++m) {
            const int r = m / nT, e = m % nT;
            if (e < NOBH * NIB) {
                const int s2 = e / NIB, t = e % NIB;
                mfma16_inplace(acc2[s2][t], a2[s2][r], oh1[pb][t][r]);
            } else {
                const int s2 = (e - NOBH * NIB) / NIB, t = (e - NOBH * NIB) % NIB;
                mfma16_inplace(acc1[t][s2], a1[t][r], ox[pb][s2][r]);
            }
#pragma unroll
            for (int c = 0; c < kPer; ++c) aux(m * kPer + c);
            __builtin_amdgcn_sched_barrier(0);
        }
    };

    load_first(blk_at((long long)blockIdx.x * 4));   // first block's operands, while the producers start
    __syncthreads();                                      // pairs with producer iteration 0
#ifdef PSP_STAMPS
    unsigned long long stamps[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#endif
    for (int it = 1; it <= R; ++it) {
        PSP_STAMP(tc0);
        // -------------------------------------------------------------- consume round r from bufs[(it-1) & 1]
        const int rb = (blockIdx.x + (it - 1) * gridDim.x) * 4;
        const float* exch = bufs + ((it - 1) & 1) * 4 * EXB;
        const int b0 = blk_at(rb), b1 = blk_at(rb + 1), b2 = blk_at(rb + 2), b3 = blk_at(rb + 3);
        const int bn = blk_at((long long)rb + 4LL * gridDim.x);       // first block of this workgroup's next round
        load_lds_first(exch);
        __builtin_amdgcn_sched_barrier(0);
        phase_l3(0, b0, b1, exch);
        phase_l21(0, b1, exch + EXB);
        phase_l3(1, b1, b2, exch + EXB);
        phase_l21(1, b2, exch + 2 * EXB);
        phase_l3(0, b2, b3, exch + 2 * EXB);
        phase_l21(0, b3, exch + 3 * EXB);
        phase_l3(1, b3, bn, exch + 3 * EXB);
        phase_l21(1, bn, nullptr);
        PSP_STAMP(tc1);
        __syncthreads();                                  // swap the exchange buffers (pairs with the producer loop)
        PSP_STAMP(tc2);
        PSP_ACC(0, tc1, tc0);                             // eight phases of one round
        PSP_ACC(4, tc2, tc1);                             // barrier wait
        PSP_ACC(6, tc2, tc0);
    }
#ifdef PSP_STAMPS
    if (a.dbg && lane == 0) {
        stamps[7] = (unsigned long long)R;
        for (int i = 0; i < 8; ++i) a.dbg[((size_t)blockIdx.x * 8 + wave) * 8 + i] = stamps[i];
    }
#endif

    asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");   // matrix-pipe results settle before VALU / stores read them
    // ---- consumers write their tiles into the workgroup's partial gradient
    float* gp = a.grad_partial + (size_t)blockIdx.x * G::P;
    const int col = lane & 15, qq = lane >> 4;
#pragma unroll
    for (int s = 0; s < NOBD; ++s)
#pragma unroll
        for (int t = 0; t < NIB; ++t) {
            const int ob = wd + WD * s, ib = wh + WH * t;
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                const int o3 = 16 * ob + 4 * qq + rr, i3 = 16 * ib + col;
                if (ob < DB && ib < HB && o3 < D && i3 < H) gp[G::oW3 + o3 * H + i3] = acc3[s][t][rr];
                const int o1 = 16 * ib + 4 * qq + rr, i1 = 16 * ob + col;
                if (ob < DB && ib < HB && o1 < H && i1 < D) gp[G::oW1 + o1 * (D + 1) + 1 + i1] = acc1[t][s][rr];
            }
        }
#pragma unroll
    for (int s = 0; s < NOBH; ++s)
#pragma unroll
        for (int t = 0; t < NIB; ++t) {
            const int ob = wd + WD * s, ib = wh + WH * t;
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                const int o2 = 16 * ob + 4 * qq + rr, i2 = 16 * ib + col;
                if (ob < HB && ib < HB && o2 < H && i2 < H) gp[G::oW2 + o2 * H + i2] = acc2[s][t][rr];
            }
        }
    // db1 and the time column of dW1: sums of this wave's dz1 tiles (lane = feature, 16 samples over q' and registers)
#pragma unroll
    for (int t = 0; t < NIB; ++t) {
        const float v1 = qsum(hsum4(bs1[t])), vt = qsum(hsum4(bt1[t]));
        const int f = 16 * (wh + WH * t) + col;
        if (wd == 0 && qq == 0 && (wh + WH * t) < HB && f < H) {
            gp[G::ob1 + f] = v1;
            gp[G::oW1 + f * (D + 1)] = vt;
        }
    }
    // db3, db2: fixed-order sum of the four producers' partial sums (LDS)
    __syncthreads();                                      // pairs with the producers' barrier after their LDS write
    {
        const float* red = bufs;
        const int ct = tid - 256;
        for (int f = ct; f < D; f += 256)
            gp[G::ob3 + f] = (red[f] + red[RS + f]) + (red[2 * RS + f] + red[3 * RS + f]);
        for (int f = ct; f < H; f += 256) {
            const float* r2 = red + 16 * DB + f;
            gp[G::ob2 + f] = (r2[0] + r2[RS]) + (r2[2 * RS] + r2[3 * RS]);
        }
    }
}

// host-side launch table entry
struct HjbInstance {
    int d, H, n_params;
    int (*fwd_lds_bytes)(int drift_kind, int sigma_kind);
    hipError_t (*launch_fwd)(const HjbArgs&, int grid, int block, hipStream_t);
    int path_floats_per_tile_step;   // Geo::PB
    int (*bwd2_lds_bytes)();
    hipError_t (*launch_bwd2)(const HjbArgs&, int grid, hipStream_t);   // role-specialised variant, 512 threads
    int wide;                        // 1: hjbw_kernels.h family (tables in global memory, 256-thread workgroups)
    int fwd_table_floats, bwd_table_floats;
    int (*split_lds_bytes)();        // hjbs_kernels.h: feature-split forward for small K (null: not built for this instance)
    hipError_t (*launch_fwd_split)(const HjbArgs&, int grid, hipStream_t);
    hipError_t (*launch_adj)(const HjbArgs&, int grid, int block, hipStream_t);   // hjba_kernels.h adjoint sweep (null: not built)
    hipError_t (*launch_fwd_bf16)(const HjbArgs&, int grid, int block, hipStream_t);   // control net on bf16 MFMA (null: not built)
    int (*quad_lds_bytes)();         // hjbq_kernels.h: four trajectories per workgroup for the smallest K (null: not built)
    hipError_t (*launch_fwd_quad)(const HjbArgs&, int grid, hipStream_t);
    hipError_t (*launch_adj_quad)(const HjbArgs&, int grid, hipStream_t);          // quad-trajectory adjoint sweep (same selection rule)
    int bwd2_one_per_cu;             // wide family: 1 when launch_bwd2 is the 8-wave hjbw_bwd2_kernel (one workgroup per CU)
    int (*fwd_x3_lds_bytes)(int drift_kind, int sigma_kind);                           // split-product forward (null: not built)
    hipError_t (*launch_fwd_x3)(const HjbArgs&, int grid, int block, hipStream_t);
    int (*bwd2_x3_lds_bytes)();                                                        // split-product backward, hjbx_kernels.h
    hipError_t (*launch_bwd2_x3)(const HjbArgs&, int grid, hipStream_t);               // (null: not built)
    hipError_t (*launch_adj_x3)(const HjbArgs&, int grid, int block, hipStream_t);     // split-product adjoint sweep (same LDS as the forward)
    int (*coop_lds_bytes)(int tiles);                                                  // hjbc_kernels.h: cooperative split-product forward of the wide
    hipError_t (*launch_fwd_coop)(const HjbArgs&, int grid, int tiles, hipStream_t);   // family, 2 or 4 tiles per 512-thread workgroup (null: not built)
};

template <int D, int H>
struct HjbLaunch {
    using G = Geo<D, H>;
    static int fwd_lds(int dk, int sk) { return G::fwd_lds_floats(dk, sk) * 4; }
    static int fwd_x3_lds(int dk, int sk) { return G::fwd_x3_lds_floats(dk, sk) * 4; }
    template <int MODE, int FAST>
    static hipError_t fwd_as(const HjbArgs& a, int grid, int block, hipStream_t s) {
        const int bytes = MODE == 2 ? fwd_x3_lds(a.drift_kind, a.sigma_kind) : fwd_lds(a.drift_kind, a.sigma_kind);
        return launch_lds<hjb_fwd_kernel<D, H, MODE, FAST>>(dim3(grid), dim3(block), bytes, s, a);
    }
    // FAST (no vector-memory load in the time loop): Philox noise, no u_L2 log, no time-feature table -- every training launch
    static bool fast(const HjbArgs& a) { return a.noise_mode == NOISE_PHILOX && a.uref == nullptr && a.tfeat == nullptr && a.store_path != 0; }
    static hipError_t fwd(const HjbArgs& a, int grid, int block, hipStream_t s) {
        return fast(a) ? fwd_as<0, 1>(a, grid, block, s) : fwd_as<0, 0>(a, grid, block, s);
    }
    static hipError_t fwd_bf16(const HjbArgs& a, int grid, int block, hipStream_t s) {
        return fast(a) ? fwd_as<1, 1>(a, grid, block, s) : fwd_as<1, 0>(a, grid, block, s);
    }
    // every product fp32-grade on the f16 matrix pipe (gemm_Tx)
    static hipError_t fwd_x3(const HjbArgs& a, int grid, int block, hipStream_t s) {
        // (the specialised instances: dense drift, dense (FAST_ = 2) or identity (FAST_ = 3) sigma, adaptive, no running cost,
        //  store_path 1 / 4 -- hjb_fwd_kernel)
        const bool spec = spec_enabled() && fast(a) && a.drift_kind == DRIFT_DENSE && a.adaptive && a.runcost_kind == RUN_ZERO &&
                          (a.store_path == 4 || a.store_path == 1) && a.loss_kind != LOSS_RELENT;
        if (spec && a.sigma_kind == SIGMA_DENSE) return fwd_as<2, 2>(a, grid, block, s);
        if (spec && a.sigma_kind == SIGMA_IDENT) return fwd_as<2, 3>(a, grid, block, s);
        return fast(a) ? fwd_as<2, 1>(a, grid, block, s) : fwd_as<2, 0>(a, grid, block, s);
    }
    static int bwd2_lds() { return G::bwd2_lds_floats() * 4; }
    static hipError_t bwd2(const HjbArgs& a, int grid, hipStream_t s) {
        return launch_lds<hjb_bwd2_kernel<D, H>>(dim3(grid), dim3(512), bwd2_lds(), s, a);
    }
    static HjbInstance instance() {
        return HjbInstance{D, H, G::P, &fwd_lds, &fwd, G::PB, &bwd2_lds, &bwd2};
    }
};

}  // namespace psp

#define PSP_DEFINE_INSTANCE(D_, H_) \
    extern "C" psp::HjbInstance psp_instance_##D_##_##H_() { return psp::HjbLaunch<D_, H_>::instance(); }
#define PSP_DECLARE_INSTANCE(D_, H_) extern "C" psp::HjbInstance psp_instance_##D_##_##H_();
