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

// the dots that ride with the steps (:74, :81, :106, :111, :136, :142): one more term into a thread's partial sum, one rounding
__device__ __forceinline__ void dot_step(double &acc, double a, double b)
{
#pragma clang fp contract(off)
    acc = fma(a, b, acc);
}

}  // namespace cm
