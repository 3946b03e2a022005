// steps.h -- the arithmetic of the BiCGSTAB loop (pbicgstab.cu:67-151), each step stated once.  The streaming vector kernels
// (kernels.hip), the K-column kernels (batch.hip) and the fused and resident loops of small systems (small_loops.hip) all call
// these, so a value has the same bits whichever loop form produced it.  Every body sits under contract(off) (lexical: see
// the note above spmv_finish_row_fused in device.h) and writes fma() where one rounding is meant: nothing is left to the
// compiler.  One flavour per step: no site rounds differently from another.
#pragma once
#include <hip/hip_runtime.h>

namespace cm {

// ------------------------------------------------------------------ scalar steps
__device__ __forceinline__ double step_beta(double rho, double rho_prev, double alpha, double omega)     // :84
{
#pragma clang fp contract(off)
    return (rho / rho_prev) * (alpha / omega);
}

__device__ __forceinline__ double step_alpha(double rho, double rw_v) { return rho / rw_v; }            // :107

__device__ __forceinline__ double step_omega(double t_s, double t_t) { return t_s / t_t; }              // :137

// ------------------------------------------------------------------ element steps
__device__ __forceinline__ double step_r0(double b, double ax) { return b - ax; }                        // :67-70  r = b - A x

// :86-88  p = r + beta (p - omega v): TWO roundings (the reference's axpy, scal, axpy make three)
__device__ __forceinline__ double step_p(double r, double p, double v, double beta, double omega)
{
#pragma clang fp contract(off)
    return fma(beta, fma(-omega, v, p), r);
}

__device__ __forceinline__ double step_r_half(double r, double v, double alpha)                           // :109  r -= alpha v
{
#pragma clang fp contract(off)
    return fma(-alpha, v, r);
}

__device__ __forceinline__ double step_x_half(double x, double pw, double alpha)                          // :110  x += alpha pw
{
#pragma clang fp contract(off)
    return fma(alpha, pw, x);
}

__device__ __forceinline__ double step_x_full(double x, double s, double omega)                           // :139  x += omega s
{
#pragma clang fp contract(off)
    return fma(omega, s, x);
}

__device__ __forceinline__ double step_r_full(double r, double t, double omega)                           // :140  r -= omega t
{
#pragma clang fp contract(off)
    return fma(-omega, t, r);
}

// ------------------------------------------------------------------ BiCGSTAB(2) (CUDAMAT_LOOP_BICGSTAB_L2, bicgstab_l2.hip)
// The BiCG half of a sweep: beta = alpha rho1 / rho0 with rho0 = -omega rho0' at j = 0, alpha = rho0 / gamma.
__device__ __forceinline__ double step_l2_beta(double alpha, double rho1, double rho0)
{
#pragma clang fp contract(off)
    return (alpha * rho1) / rho0;
}

__device__ __forceinline__ double step_l2_alpha(double rho0, double gamma) { return rho0 / gamma; }

// The minimal-residual half: [[a11, a12], [a12, a22]] (g1, g2) = (b1, b2) by elimination on the pivot a11 = r1.r1:
//   s = a12 / a11;  t = a22 - s a12;  g2 = (b2 - s b1) / t;  g1 = (b1 - a12 g2) / a11      (one fma per difference)
// Under (c b, c x0), c a power of two, the five dots scale with c^2, and so do t and both numerators; s, g1, g2 do not scale.
// Under (c A, b, x0 / c): b1 ~ c, a11, b2 ~ c^2, a12 ~ c^3, a22 ~ c^4, and s ~ c, t ~ c^4, g1 ~ 1 / c, g2 ~ 1 / c^2.  No
// intermediate carries a higher power of c than the dots themselves (the determinant of Cramer's rule carries c^4 under the
// first scaling and c^6 under the second, and leaves the range of a double where the dots do not), and a scaling by a power of
// two commutes with every rounding here: the bits of g1 and g2 are those of the unscaled system, scaled.  *s_out and *piv
// (= t) are what the caller tests, with a11, for a singular system.
__device__ __forceinline__ void step_l2_mr(double a11, double a12, double a22, double b1, double b2, double *s_out, double *piv,
                                           double *g1, double *g2)
{
#pragma clang fp contract(off)
    const double s = a12 / a11;
    const double t = fma(-s, a12, a22);
    const double gg2 = fma(-s, b1, b2) / t;
    *s_out = s;
    *piv = t;
    *g2 = gg2;
    *g1 = fma(-a12, gg2, b1) / a11;
}

__device__ __forceinline__ double step_l2_u(double r, double u, double beta)              // u_i = r_i - beta u_i
{
#pragma clang fp contract(off)
    return fma(-beta, u, r);
}

__device__ __forceinline__ double step_l2_r(double r, double u, double alpha)             // r_i -= alpha u_(i+1)
{
#pragma clang fp contract(off)
    return fma(-alpha, u, r);
}

__device__ __forceinline__ double step_l2_y(double y, double u, double alpha)             // y += alpha u0
{
#pragma clang fp contract(off)
    return fma(alpha, u, y);
}

// y += g1 a + g2 b, and v -= g1 a + g2 b: two roundings each, the g1 term first
__device__ __forceinline__ double step_l2_add2(double y, double a, double b, double g1, double g2)
{
#pragma clang fp contract(off)
    return fma(g2, b, fma(g1, a, y));
}

__device__ __forceinline__ double step_l2_sub2(double v, double a, double b, double g1, double g2)
{
#pragma clang fp contract(off)
    return fma(-g2, b, fma(-g1, a, v));
}

// ------------------------------------------------------------------ conjugate gradients (CUDAMAT_LOOP_CG, cg.hip)
__device__ __forceinline__ double step_cg_beta(double rho, double rho_prev) { return rho / rho_prev; }

__device__ __forceinline__ double step_cg_alpha(double rho, double gamma) { return rho / gamma; }

__device__ __forceinline__ double step_cg_p(double z, double p, double beta)               // p = z + beta p
{
#pragma clang fp contract(off)
    return fma(beta, p, z);
}

__device__ __forceinline__ double step_cg_x(double x, double p, double alpha)              // x += alpha p
{
#pragma clang fp contract(off)
    return fma(alpha, p, x);
}

__device__ __forceinline__ double step_cg_r(double r, double q, double alpha)              // r -= alpha q
{
#pragma clang fp contract(off)
    return fma(-alpha, q, r);
}

// the dots that ride with the steps (:74, :81, :106, :111, :136, :142): one more term into a thread's partial sum, one rounding
__device__ __forceinline__ void dot_step(double &acc, double a, double b)
{
#pragma clang fp contract(off)
    acc = fma(a, b, acc);
}

}  // namespace cm
