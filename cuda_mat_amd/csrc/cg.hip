// cg.hip -- the vector kernels of CUDAMAT_LOOP_CG: Hestenes-Stiefel preconditioned conjugate gradients, gfx950.
//
// One iteration = ONE product with A and one application of M^-1 (loops.hip iterate_cg strings the launches together):
//   M = I:    k_cg_p | SpMV q = A p (+ p.q) | k_cg_step
//   ILU(0):   k_cg_p | SpMV q = A p (+ p.q) | k_cg_step | z = M^-1 r | k_cg_rz       (once, before the loop: z = M^-1 r0 | k_cg_rz)
// As in kernels.hip and bicgstab_l2.hip: HBM-bound fp64 streaming, 16 bytes per lane where the operands allow it, every dot
// product produced by the kernel that already streams its operands and summed in a fixed order in the prologue of the kernel that
// consumes it (load_scalars); the arithmetic of each step is stated once, in steps.h; pair_loop deals the elements in one order
// for both alignments, so the bits of a solve do not depend on where the caller's x starts.  The scalars live in CgState
// (common.h), in the slot behind the solve's LoopState.  The stopping test is ||r|| after the step (check_iteration_end: in the
// prologue of the next iteration's k_cg_p, and once after the loop); a breakdown -- p.Ap or r.z not positive, a scalar that is
// not finite -- is noticed by the kernel that forms the scalar, which freezes the loop (state 3) before it touches a vector.
//
// Vector traffic per row and iteration, in doubles read + written: p 2 + 1, step 4 + 2 = 72 bytes (+ rz 2 with a
// preconditioner), beside the w operand of the SpMV epilogue.
#include "kernels.h"
#include "device.h"

#pragma clang fp contract(off)      // no product-sum here is left to the compiler: fma() is written where one rounding is meant

namespace cm {

__global__ __launch_bounds__(kBlock) void k_cg_check(LoopArgs la, ScalarSrc full)
{
    __shared__ double lds[8];
    if (uniform_state(la.st) != 0) return;
    double sc[2];
    load_scalars<2>(full, sc, lds);
    check_iteration_end(la, sc[1]);
}

int launch_cg_check(hipStream_t s, LoopArgs la, ScalarSrc full)
{
    hipLaunchKernelGGL(k_cg_check, dim3(1), dim3(kBlock), 0, s, la, full);
    CM_HIP(hipGetLastError());
    return CUDAMAT_OK;
}

// rho' = r.z; beta = it == 0 ? 0 : rho' / rho; p = z + beta p (z is r when M = I)
template <int VEC>
__global__ __launch_bounds__(kBlock) void k_cg_p(LoopArgs la, ScalarSrc full, int64_t n, const double *z, double *p)
{
    __shared__ double lds[8];
    LoopState *st = la.st;
    CgState *q = cg_state(st);
    if (uniform_state(st) != 0) return;
    const int it = st->it;
    double sc[2];
    load_scalars<2>(full, sc, lds);
    if (check_iteration_end(la, sc[1])) return;
    const double rho = sc[0];
    const double beta = it == 0 ? 0.0 : step_cg_beta(rho, q->rho[(it + 1) & 1]);
    if (leader()) {
        q->rho[it & 1] = rho;
        q->rho_now = rho;
        q->beta = beta;
    }
    if (loop_breakdown(la, !(rho > 0.0) || !isfinite(rho) || !isfinite(beta))) {
        if (leader()) q->why = 1;
        return;
    }
    pair_loop<VEC>(n, [&](int64_t i, auto w) {
        constexpr int W = decltype(w)::value;
        double zz[W], pp[W];
        load_row<W>(z, i, zz); load_row<W>(p, i, pp);
#pragma unroll
        for (int j = 0; j < W; j++) pp[j] = step_cg_p(zz[j], pp[j], beta);
        store_row<W>(p, i, pp, kAll);
    });
}

int launch_cg_p(hipStream_t s, LoopArgs la, ScalarSrc full, int64_t n, const double *z, double *p)
{
    CM_VEC_LAUNCH(all_aligned16(z, p), vec_grid(n), k_cg_p<VEC>, la, full, n, z, p);
}

// gamma = p.q; alpha = rho / gamma; x += alpha p; r -= alpha q; (r.r, r.r); it++.  The last kernel of an iteration that every
// solve runs: it publishes the progress word, frozen or not.
template <int VEC>
__global__ __launch_bounds__(kBlock) void k_cg_step(LoopArgs la, ScalarSrc gam, int64_t n, double *x, double *r, const double *p,
                                                    const double *q, double *parts)
{
    __shared__ double lds[8];
    LoopState *st = la.st;
    CgState *c = cg_state(st);
    const int frozen = uniform_state(st);
    if (frozen != 0) {                // still tell the host that this iteration's launches have drained
        publish_progress(la, frozen);
        return;
    }
    double sc[1];
    load_scalars<1>(gam, sc, lds);
    const double gamma = sc[0];
    const double alpha = step_cg_alpha(c->rho_now, gamma);
    if (leader()) c->gamma = gamma;
    if (loop_breakdown(la, !(gamma > 0.0) || !isfinite(gamma) || !isfinite(alpha))) {
        if (leader()) c->why = 2;
        publish_progress(la, 3);
        return;
    }
    double acc[1] = {0.0};
    pair_loop<VEC>(n, [&](int64_t i, auto w) {
        constexpr int W = decltype(w)::value;
        double xx[W], rr[W], pp[W], qq[W];
        load_row<W>(x, i, xx); load_row<W>(r, i, rr); load_row<W>(p, i, pp); load_row<W>(q, i, qq);
#pragma unroll
        for (int j = 0; j < W; j++) {
            xx[j] = step_cg_x(xx[j], pp[j], alpha);
            rr[j] = step_cg_r(rr[j], qq[j], alpha);
            dot_step(acc[0], rr[j], rr[j]);
        }
        store_row<W>(x, i, xx, kAll); store_row<W>(r, i, rr, kAll);
    });
    block_sum<1>(acc, lds);
    if (threadIdx.x == 0) {
        parts[2 * blockIdx.x] = acc[0];       // rho' of the next iteration when M = I
        parts[2 * blockIdx.x + 1] = acc[0];   // the stopping test
    }
    if (leader()) {
        c->alpha = alpha;
        st->it = st->it + 1;
    }
    publish_progress(la, 0);
}

int launch_cg_step(hipStream_t s, LoopArgs la, ScalarSrc gam, int64_t n, double *x, double *r, const double *p, const double *q,
                   double *parts, int *nparts)
{
    const int g = vec_grid(n);
    *nparts = g;
    CM_VEC_LAUNCH(all_aligned16(x, r, p, q), g, k_cg_step<VEC>, la, gam, n, x, r, p, q, parts);
}

// with a preconditioner: (r.z, r.r) once z = M^-1 r exists.  r.r takes the terms of k_cg_step's sum in the same order.
template <int VEC>
__global__ __launch_bounds__(kBlock) void k_cg_rz(LoopArgs la, int64_t n, const double *r, const double *z, double *parts)
{
    __shared__ double lds[8];
    if (uniform_state(la.st) != 0) return;
    double acc[2] = {0.0, 0.0};
    pair_loop<VEC>(n, [&](int64_t i, auto w) {
        constexpr int W = decltype(w)::value;
        double rr[W], zz[W];
        load_row<W>(r, i, rr); load_row<W>(z, i, zz);
#pragma unroll
        for (int j = 0; j < W; j++) {
            dot_step(acc[0], rr[j], zz[j]);
            dot_step(acc[1], rr[j], rr[j]);
        }
    });
    block_sum<2>(acc, lds);
    if (threadIdx.x == 0) {
        parts[2 * blockIdx.x] = acc[0];
        parts[2 * blockIdx.x + 1] = acc[1];
    }
}

int launch_cg_rz(hipStream_t s, LoopArgs la, int64_t n, const double *r, const double *z, double *parts, int *nparts)
{
    const int g = vec_grid(n);
    *nparts = g;
    CM_VEC_LAUNCH(all_aligned16(r, z), g, k_cg_rz<VEC>, la, n, r, z, parts);
}

}  // namespace cm
