// gh_kinds.h -- the h kinds of the value-net kernels (PSP_GH_* of include/psp.h; api_gen.hip asserts the numbering) and the
// arithmetic of the kinds that more than one kernel family evaluates: the rollout kernels (gen_kernels.h, genl_kernels.h) and the
// PINN finish kernel (pinn_kernels.h).  Nothing here needs the MFMA machinery of hjb_kernels.h.
#pragma once
#include <hip/hip_runtime.h>

namespace psp {

enum { GH_ZERO = 0, GH_QUAD = 1, GH_ALLEN_CAHN = 2, GH_EXPBALL_LIN = 3, GH_EXPBALL_SQ = 4, GH_EXPBALL_SIN = 5,
       // h of ExponentialOnBallNonlinearSinHessian (problems.py:1094): GH_EXPBALL_SIN with (sum_i x_i)^2 = sum_ij x_i x_j in the
       // linear term, |x|^2 kept in the exponent.  Rollouts: the dense-sigma instances of genl_kernels.h only.
       GH_EXPBALL_SIN_FULL = 6,
       // the exit-time and box problems (include/psp.h), h_par = p0 .. p3:
       GH_AFFINE_EXP = 7,      // h = p0 + p1 y + p2 |z|^2 + p3 exp(-y)
       GH_SINE_SOURCE = 8,     // h = c y + s(x_0, x_1): Helmholtz (p0 = 0), Oscillations (p0 = 1)
       GH_SINNORM2 = 9 };      // SinNorm2.h, from |x|^2 and sum_i x_i (dense sigma: genl_kernels.h only)
// the kinds whose h reads |x|^2
__host__ __device__ inline bool gh_reads_r2(int kind) { return kind >= GH_EXPBALL_LIN && kind != GH_AFFINE_EXP && kind != GH_SINE_SOURCE; }

// GH_AFFINE_EXP (problems.py:1301, :1393, :1488, :1605): -h and h_y from y = V(X) and S = |z|^2; exp only where p3 asks for it
__device__ inline void gh_affine_exp(const float* p, float y, float S, float& minus_h, float& hy) {
    float e = 0.f;
    if (p[3] != 0.f) e = p[3] * expf(-y);
    minus_h = -(((p[2] * S + p[0]) + p[1] * y) + e);
    hy = p[1] - e;
}
// GH_SINE_SOURCE (problems.py:1646-1648, :1687), the terms summed in the order written there.  A squared coefficient meets its
// sine one factor at a time, p (p s): a product of two launch constants is loop-invariant, would be hoisted out of the time loop
// into a register of its own and from there -- the split-product instance of d = 100 has none to spare -- into scratch
__device__ inline void gh_sine_source(const float* p, float y, float x0, float x1, float& minus_h, float& hy) {
    if (p[0] == 0.f) {
        const float c = p[3], s1 = sinf(p[1] * x0), s2 = sinf(p[2] * x1);
        minus_h = -(((c * y + (p[1] * (p[1] * s1)) * s2) + (p[2] * (p[2] * s1)) * s2) - (c * s1) * s2);
        hy = c;
    } else {
        minus_h = -(p[1] * (p[1] * sinf(p[1] * x0)) + p[2] * (p[2] * (p[3] * sinf(p[2] * x0))));
        hy = 0.f;
    }
}

}  // namespace psp
