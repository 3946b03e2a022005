// bicgstab_l2.hip -- the vector kernels of CUDAMAT_LOOP_BICGSTAB_L2: BiCGSTAB(2) (Sleijpen & Fokkema 1993, l = 2), gfx950.
//
// One sweep = two BiCG steps and one degree-2 minimal-residual step = four products with A^ = A M^-1 (loops.hip
// iterate_l2 strings the launches together):
//   (once: k_l2_start, the start sums)
//   k_l2_u0 | [M^-1] SpMV u1 (+ u1.r~) | k_l2_step0 | [M^-1] SpMV r1 (+ r1.r~) | k_l2_u1 | [M^-1] SpMV u2 (+ u2.r~) |
//   k_l2_step1 (+ r1.r1, r1.r0) | [M^-1] SpMV r2 (+ r2.r1, r2.r2) | k_l2_dot (r2.r0) | k_l2_mr (+ r0.r~, r0.r0)
// As in kernels.hip: HBM-bound fp64 streaming, 16 bytes per lane where the operands allow it, every dot product produced by
// the kernel that already streams its operands and summed in a fixed order in the prologue of the kernel that consumes it
// (load_scalars); the arithmetic of each step is stated once, in steps.h.  The scalars live in L2State (common.h), in the slot
// behind the solve's LoopState.  The only stopping test is ||r0|| after the minimal-residual step
// (check_iteration_end, device.h: in the prologue of the next sweep's first kernel, and once after the loop); a breakdown -- a zero divisor or a scalar that is not finite -- is
// noticed by the kernel that forms the scalar, which freezes the loop (state 3) before it touches a vector.
//
// Vector traffic per row and sweep, in doubles read + written: u0 2 + 1, step0 4 + 2, u1 4 + 2, step1 6 + 3, dot 2,
// mr 8 + 3 = 37 doubles = 296 bytes, beside the w operand of the four SpMV epilogues.
#include "kernels.h"
#include "device.h"

#pragma clang fp contract(off)      // no product-sum here is left to the compiler: fma() is written where one rounding is meant

namespace cm {

__global__ __launch_bounds__(kBlock) void k_l2_check(LoopArgs la, ScalarSrc full)
{
    __shared__ double lds[8];
    if (uniform_state(la.st) != 0) return;
    double sc[2];
    load_scalars<2>(full, sc, lds);
    check_iteration_end(la, sc[1]);
}

int launch_l2_check(hipStream_t s, LoopArgs la, ScalarSrc full)
{
    hipLaunchKernelGGL(k_l2_check, dim3(1), dim3(kBlock), 0, s, la, full);
    CM_HIP(hipGetLastError());
    return CUDAMAT_OK;
}

// The start sums of this loop: parts = (r0.r~, r0.r0) = (r0.r0, r0.r0), stride 2, as launch_init leaves them -- but summed with
// pair_loop's dealing (device.h).  launch_init streams the caller's b and deals rows, not pairs, when b is 8 bytes off a 16-byte boundary;
// its sum would then differ in the last bits, and with it ||r_init||, the first rho and every iterate after it.  r0 itself is
// formed element by element and has the same bits either way.
template <int VEC>
__global__ __launch_bounds__(kBlock) void k_l2_start(int64_t n, const double *r0, double *parts)
{
    __shared__ double lds[4];
    double acc[1] = {0.0};
    pair_loop<VEC>(n, [&](int64_t i, auto w) {
        constexpr int W = decltype(w)::value;
        double rr[W];
        load_row<W>(r0, i, rr);
#pragma unroll
        for (int j = 0; j < W; j++) dot_step(acc[0], rr[j], rr[j]);
    });
    block_sum<1>(acc, lds);
    if (threadIdx.x == 0) {
        parts[2 * blockIdx.x] = acc[0];
        parts[2 * blockIdx.x + 1] = acc[0];
    }
}

int launch_l2_start(hipStream_t s, int64_t n, const double *r0, double *parts, int *nparts)
{
    const int g = vec_grid(n);
    *nparts = g;
    CM_VEC_LAUNCH(all_aligned16(r0), g, k_l2_start<VEC>, n, r0, parts);
}

// j = 0, first part: rho0 = -omega rho0; rho1 = r0.r~; beta = alpha rho1 / rho0; rho0 = rho1; u0 = r0 - beta u0
template <int VEC>
__global__ __launch_bounds__(kBlock) void k_l2_u0(LoopArgs la, ScalarSrc full, int64_t n, const double *r0, double *u0)
{
    __shared__ double lds[8];
    LoopState *st = la.st;
    L2State *q = l2_state(la.st);
    if (uniform_state(st) != 0) return;
    const int it = st->it;
    double sc[2];
    load_scalars<2>(full, sc, lds);
    if (check_iteration_end(la, sc[1])) return;
    const double rho1 = sc[0];
    const double rho_prev = it == 0 ? 1.0 : q->rho_b, alpha = it == 0 ? 0.0 : q->alpha_b, omega = it == 0 ? 1.0 : q->omega;
    const double rho0 = -omega * rho_prev;
    const double beta = step_l2_beta(alpha, rho1, rho0);
    if (loop_breakdown(la, rho0 == 0.0 || !isfinite(rho0) || !isfinite(rho1) || !isfinite(beta))) return;
    if (leader()) q->rho_a = rho1;
    pair_loop<VEC>(n, [&](int64_t i, auto w) {
        constexpr int W = decltype(w)::value;
        double rr[W], uu[W];
        load_row<W>(r0, i, rr); load_row<W>(u0, i, uu);
#pragma unroll
        for (int j = 0; j < W; j++) uu[j] = step_l2_u(rr[j], uu[j], beta);
        store_row<W>(u0, i, uu, kAll);
    });
}

int launch_l2_u0(hipStream_t s, LoopArgs la, ScalarSrc full, int64_t n, const double *r0, double *u0)
{
    CM_VEC_LAUNCH(all_aligned16(r0, u0), vec_grid(n), k_l2_u0<VEC>, la, full, n, r0, u0);
}

// j = 0, second part: gamma = u1.r~; alpha = rho0 / gamma; r0 -= alpha u1; y += alpha u0
template <int VEC>
__global__ __launch_bounds__(kBlock) void k_l2_step0(LoopArgs la, ScalarSrc gam, int64_t n, double *r0, const double *u1,
                                                     const double *u0, double *y)
{
    __shared__ double lds[8];
    L2State *q = l2_state(la.st);
    if (uniform_state(la.st) != 0) return;
    double sc[1];
    load_scalars<1>(gam, sc, lds);
    const double gamma = sc[0];
    const double alpha = step_l2_alpha(q->rho_a, gamma);
    if (loop_breakdown(la, gamma == 0.0 || !isfinite(gamma) || !isfinite(alpha))) return;
    if (leader()) q->alpha_a = alpha;
    pair_loop<VEC>(n, [&](int64_t i, auto w) {
        constexpr int W = decltype(w)::value;
        double rr[W], u1v[W], u0v[W], yy[W];
        load_row<W>(r0, i, rr); load_row<W>(u1, i, u1v); load_row<W>(u0, i, u0v); load_row<W>(y, i, yy);
#pragma unroll
        for (int j = 0; j < W; j++) {
            rr[j] = step_l2_r(rr[j], u1v[j], alpha);
            yy[j] = step_l2_y(yy[j], u0v[j], alpha);
        }
        store_row<W>(r0, i, rr, kAll); store_row<W>(y, i, yy, kAll);
    });
}

int launch_l2_step0(hipStream_t s, LoopArgs la, ScalarSrc gam, int64_t n, double *r0, const double *u1, const double *u0, double *y)
{
    CM_VEC_LAUNCH(all_aligned16(r0, u1, u0, y), vec_grid(n), k_l2_step0<VEC>, la, gam, n, r0, u1, u0, y);
}

// j = 1, first part: rho1 = r1.r~; beta = alpha rho1 / rho0; rho0 = rho1; u0 = r0 - beta u0; u1 = r1 - beta u1
template <int VEC>
__global__ __launch_bounds__(kBlock) void k_l2_u1(LoopArgs la, ScalarSrc rho, int64_t n, const double *r0, const double *r1,
                                                  double *u0, double *u1)
{
    __shared__ double lds[8];
    L2State *q = l2_state(la.st);
    if (uniform_state(la.st) != 0) return;
    double sc[1];
    load_scalars<1>(rho, sc, lds);
    const double rho1 = sc[0], rho0 = q->rho_a;
    const double beta = step_l2_beta(q->alpha_a, rho1, rho0);
    if (loop_breakdown(la, rho0 == 0.0 || !isfinite(rho1) || !isfinite(beta))) return;
    if (leader()) q->rho_b = rho1;
    pair_loop<VEC>(n, [&](int64_t i, auto w) {
        constexpr int W = decltype(w)::value;
        double r0v[W], r1v[W], u0v[W], u1v[W];
        load_row<W>(r0, i, r0v); load_row<W>(r1, i, r1v); load_row<W>(u0, i, u0v); load_row<W>(u1, i, u1v);
#pragma unroll
        for (int j = 0; j < W; j++) {
            u0v[j] = step_l2_u(r0v[j], u0v[j], beta);
            u1v[j] = step_l2_u(r1v[j], u1v[j], beta);
        }
        store_row<W>(u0, i, u0v, kAll); store_row<W>(u1, i, u1v, kAll);
    });
}

int launch_l2_u1(hipStream_t s, LoopArgs la, ScalarSrc rho, int64_t n, const double *r0, const double *r1, double *u0, double *u1)
{
    CM_VEC_LAUNCH(all_aligned16(r0, r1, u0, u1), vec_grid(n), k_l2_u1<VEC>, la, rho, n, r0, r1, u0, u1);
}

// j = 1, second part: gamma = u2.r~; alpha = rho0 / gamma; r0 -= alpha u1; r1 -= alpha u2; y += alpha u0; (r1.r1, r1.r0)
template <int VEC>
__global__ __launch_bounds__(kBlock) void k_l2_step1(LoopArgs la, ScalarSrc gam, int64_t n, double *r0, double *r1, const double *u0,
                                                     const double *u1, const double *u2, double *y, double *parts)
{
    __shared__ double lds[8];
    L2State *q = l2_state(la.st);
    if (uniform_state(la.st) != 0) return;
    double sc[1];
    load_scalars<1>(gam, sc, lds);
    const double gamma = sc[0];
    const double alpha = step_l2_alpha(q->rho_b, gamma);
    if (loop_breakdown(la, gamma == 0.0 || !isfinite(gamma) || !isfinite(alpha))) return;
    if (leader()) q->alpha_b = alpha;
    double acc[2] = {0.0, 0.0};
    pair_loop<VEC>(n, [&](int64_t i, auto w) {
        constexpr int W = decltype(w)::value;
        double r0v[W], r1v[W], u0v[W], u1v[W], u2v[W], yy[W];
        load_row<W>(r0, i, r0v); load_row<W>(r1, i, r1v); load_row<W>(u0, i, u0v); load_row<W>(u1, i, u1v);
        load_row<W>(u2, i, u2v); load_row<W>(y, i, yy);
#pragma unroll
        for (int j = 0; j < W; j++) {
            r0v[j] = step_l2_r(r0v[j], u1v[j], alpha);
            r1v[j] = step_l2_r(r1v[j], u2v[j], alpha);
            yy[j] = step_l2_y(yy[j], u0v[j], alpha);
            dot_step(acc[0], r1v[j], r1v[j]);
            dot_step(acc[1], r1v[j], r0v[j]);
        }
        store_row<W>(r0, i, r0v, kAll); store_row<W>(r1, i, r1v, kAll); store_row<W>(y, i, yy, kAll);
    });
    block_sum<2>(acc, lds);
    if (threadIdx.x == 0) {
        parts[2 * blockIdx.x] = acc[0];
        parts[2 * blockIdx.x + 1] = acc[1];
    }
}

int launch_l2_step1(hipStream_t s, LoopArgs la, ScalarSrc gam, int64_t n, double *r0, double *r1, const double *u0, const double *u1,
                    const double *u2, double *y, double *parts, int *nparts)
{
    const int g = vec_grid(n);
    *nparts = g;
    CM_VEC_LAUNCH(all_aligned16(r0, r1, u0, u1, u2, y), g, k_l2_step1<VEC>, la, gam, n, r0, r1, u0, u1, u2, y, parts);
}

// r2.r0: r2 exists only once the fourth SpMV has run, and that SpMV's epilogue carries r2.r1 and r2.r2
template <int VEC>
__global__ __launch_bounds__(kBlock) void k_l2_dot(LoopArgs la, int64_t n, const double *r2, const double *r0, double *parts)
{
    __shared__ double lds[4];
    if (uniform_state(la.st) != 0) return;
    double acc[1] = {0.0};
    pair_loop<VEC>(n, [&](int64_t i, auto w) {
        constexpr int W = decltype(w)::value;
        double a[W], b[W];
        load_row<W>(r2, i, a); load_row<W>(r0, i, b);
#pragma unroll
        for (int j = 0; j < W; j++) dot_step(acc[0], a[j], b[j]);
    });
    block_sum<1>(acc, lds);
    if (threadIdx.x == 0) parts[blockIdx.x] = acc[0];
}

int launch_l2_dot(hipStream_t s, LoopArgs la, int64_t n, const double *r2, const double *r0, double *parts, int *nparts)
{
    const int g = vec_grid(n);
    *nparts = g;
    CM_VEC_LAUNCH(all_aligned16(r2, r0), g, k_l2_dot<VEC>, la, n, r2, r0, parts);
}

// the minimal-residual step: (g1, g2) from the five dots, by elimination (step_l2_mr: exact under powers of two; a zero
// pivot r1.r1 or t, or a quotient that is not finite, is the breakdown); y += g1 r0 + g2 r1; u0 -= g1 u1 + g2 u2; r0 -= g1 r1 + g2 r2;
// omega = g2; (r0.r~, r0.r0); it++.  The last kernel of a sweep: it publishes the progress word, frozen or not.
template <int VEC>
__global__ __launch_bounds__(kBlock) void k_l2_mr(LoopArgs la, ScalarSrc d11, ScalarSrc d2, ScalarSrc d20, int64_t n, double *y,
                                                  double *r0, const double *r1, const double *r2, double *u0, const double *u1,
                                                  const double *u2, const double *rt, double *parts)
{
    __shared__ double lds[8];
    LoopState *st = la.st;
    const int frozen = uniform_state(st);
    if (frozen != 0) {                // still tell the host that this sweep's launches have drained
        publish_progress(la, frozen);
        return;
    }
    double a[2], c[2], e[1];
    load_scalars<2>(d11, a, lds);      // r1.r1, r1.r0
    load_scalars<2>(d2, c, lds);       // r2.r1, r2.r2
    load_scalars<1>(d20, e, lds);      // r2.r0
    double sq, piv, g1, g2;
    step_l2_mr(a[0], c[0], c[1], a[1], e[0], &sq, &piv, &g1, &g2);
    if (loop_breakdown(la, a[0] == 0.0 || piv == 0.0 || !isfinite(sq) || !isfinite(piv) || !isfinite(g1) || !isfinite(g2))) {
        publish_progress(la, 3);
        return;
    }
    double acc[2] = {0.0, 0.0};
    pair_loop<VEC>(n, [&](int64_t i, auto w) {
        constexpr int W = decltype(w)::value;
        double yy[W], r0v[W], r1v[W], r2v[W], u0v[W], u1v[W], u2v[W], tv[W];
        load_row<W>(y, i, yy); load_row<W>(r0, i, r0v); load_row<W>(r1, i, r1v); load_row<W>(r2, i, r2v);
        load_row<W>(u0, i, u0v); load_row<W>(u1, i, u1v); load_row<W>(u2, i, u2v); load_row<W>(rt, i, tv);
#pragma unroll
        for (int j = 0; j < W; j++) {
            yy[j] = step_l2_add2(yy[j], r0v[j], r1v[j], g1, g2);
            u0v[j] = step_l2_sub2(u0v[j], u1v[j], u2v[j], g1, g2);
            r0v[j] = step_l2_sub2(r0v[j], r1v[j], r2v[j], g1, g2);
            dot_step(acc[0], tv[j], r0v[j]);               // rho1 of the next sweep
            dot_step(acc[1], r0v[j], r0v[j]);              // the stopping test
        }
        store_row<W>(y, i, yy, kAll); store_row<W>(u0, i, u0v, kAll); store_row<W>(r0, i, r0v, kAll);
    });
    block_sum<2>(acc, lds);
    if (threadIdx.x == 0) {
        parts[2 * blockIdx.x] = acc[0];
        parts[2 * blockIdx.x + 1] = acc[1];
    }
    if (leader()) {
        l2_state(st)->omega = g2;
        st->omega = g2;
        st->it = st->it + 1;
    }
    publish_progress(la, 0);
}

int launch_l2_mr(hipStream_t s, LoopArgs la, ScalarSrc d11, ScalarSrc d2, ScalarSrc d20, int64_t n, double *y, double *r0,
                 const double *r1, const double *r2, double *u0, const double *u1, const double *u2, const double *rt,
                 double *parts, int *nparts)
{
    const int g = vec_grid(n);
    *nparts = g;
    CM_VEC_LAUNCH(all_aligned16(y, r0, r1, r2, u0, u1, u2, rt), g, k_l2_mr<VEC>, la, d11, d2, d20, n, y, r0, r1, r2, u0, u1, u2, rt,
                  parts);
}

}  // namespace cm
