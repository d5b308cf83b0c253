// block_index.h -- the sample blocks of one producer wave of the role-specialised backward kernels (hjb_bwd2_kernel,
// hjb_bwd3_kernel), walked without a division per round.
//
// The path store is a row of blocks b = n * ntile16 + t16 (time step n < N, 16-trajectory tile t16 < ntile16).  Workgroup `bid`
// of `grid` takes the rounds bid, bid + grid, ... of four blocks; its producer `sub` owns block
//     b(it) = (bid + it * grid) * 4 + sub
// of round it.  b advances by the constant S = 4 grid, so (t16, n) advances by the constant pair (r, q) = (S mod ntile16,
// S / ntile16) and at most one carry: t16 + r < 2 ntile16.  The block is in the store iff n < N (t16 < ntile16 always holds).
// Once a slot has left the store it stays out -- b only grows -- and the cursor then rests on the STAND-IN block nblk - 1 =
// (ntile16 - 1, N - 1): the block whose path addresses and D[k] an idle producer touches (its weight is zero).
// All fields are 32-bit: the host refuses N * ntile16 >= 2^31, so a block in the store and its (t16, n) fit, and the cursor stops
// advancing at the first block outside (a cursor that went on adding q would overflow for large N).  The divisions of start()
// run once per kernel; advance() is additions, compares and selects on wave-uniform values.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PSP_BLOCK_HD __host__ __device__ __forceinline__
#else
#define PSP_BLOCK_HD inline
#endif

namespace psp {

struct BlockCursor {
    uint32_t t16, n, blk;        // tile, time step and number of the block -- of the stand-in when !valid
    bool valid;                  // the slot's block is in the store
    uint32_t r, q, stride;       // per-round advance of (t16, n) and of blk; stride = 0: the next round is outside for every slot
    uint32_t ntile16, N;

    // the cursor of producer `sub` (0..3) of workgroup `bid` at round 0
    PSP_BLOCK_HD static BlockCursor start(uint32_t bid, uint32_t sub, uint32_t grid, uint32_t ntile16, uint32_t N) {
        BlockCursor c;
        c.ntile16 = ntile16; c.N = N;
        const uint32_t nblk = N * ntile16;                            // < 2^31 (host)
        const unsigned long long s = 4ull * grid, b0 = 4ull * bid + sub;
        if (s < nblk) { c.stride = (uint32_t)s; c.r = c.stride % ntile16; c.q = c.stride / ntile16; }
        else { c.stride = 0; c.r = 0; c.q = 0; }
        if (b0 < nblk) { c.blk = (uint32_t)b0; c.t16 = c.blk % ntile16; c.n = c.blk / ntile16; c.valid = true; }
        else c.park();
        return c;
    }
    PSP_BLOCK_HD void park() { t16 = ntile16 - 1; n = N - 1; blk = N * ntile16 - 1; valid = false; }
    // to the slot's block of the next round
    PSP_BLOCK_HD void advance() {
        if (!valid) return;
        if (stride == 0) { park(); return; }
        n += q; t16 += r; blk += stride;
        if (t16 >= ntile16) { t16 -= ntile16; ++n; }
        if (n >= N) park();
    }
};

}  // namespace psp
