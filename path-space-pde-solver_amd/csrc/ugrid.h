// ugrid.h -- grid cell of the double wells' tabulated reference control u*, shared by the u_L2 log of the DenseNet-control
// forward (hjbd_kernels.h) and the reference-control evaluation rollout (hjbe_kernels.h).
#pragma once
#include <hip/hip_runtime.h>

namespace psp {

// u*_i = table[row(t_n), cell(x_i)] with the reference's index arithmetic (problems.py:254-260): x clamped to [-xb, xhi]
// (xhi = fp32(xb - 2 dx)), floor((x + xb) / dx) with a true fp32 division, the globally LAST trajectory's cell lowered by two
// (the reference's i[-1] -= 2), a negative cell counting from the end of the row as numpy indexing does.  The final clamp has no
// effect on data the host builder describes (plan_dense_native.ul2_reference); it keeps every read inside the row.
__device__ __forceinline__ int ugrid_cell(float x, float xb, float xhi, float dx, bool last, int ncols) {
    const float xc = fminf(fmaxf(x, -xb), xhi);
    int cell = (int)floorf((xc + xb) / dx);
    if (last) cell -= 2;
    if (cell < 0) cell += ncols;
    return min(max(cell, 0), ncols - 1);
}

}  // namespace psp
