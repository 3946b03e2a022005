// kernels.hip -- the streaming vector kernels of the BiCGSTAB inner loop (gfx950) and the BLAS-1 pieces.
//
// Everything on this path is HBM-bandwidth-bound fp64 streaming / gather work (<= 0.17 flop/byte): no MFMA.
// What matters is (a) coalesced 16-byte-per-lane loads on the streamed vectors, (b) one pass per fused update instead of
// the reference's copy/scal/axpy triplets (pbicgstab.cu:86-88,109-110,139-140,668-672,...; the arithmetic of each update is
// stated once, in steps.h, and each kernel body once: vec_loop runs it pair-wide and on the tail), (c) dot products produced by
// the kernel that already streams the operands, reduced wave64-shuffle -> LDS -> per-workgroup partial -> fixed-order
// sum in the consumer's prologue (bitwise reproducible, no atomics, no host sync).
// Scalars (rho, alpha, omega, norms) never leave the device: see LoopState.
// The SpMV forms on CSR live in spmv_csr.hip, the pipelined loop's kernels in pipelined.hip, the three- and one-launch
// loops of small systems in small_loops.hip.
#include <algorithm>
#include <cstring>
#include <vector>

#include "kernels.h"
#include "device.h"

#pragma clang fp contract(off)      // no product-sum here is left to the compiler: fma() is written where one rounding is meant

namespace cm {

__global__ __launch_bounds__(kBlock) void k_check(LoopArgs la, ScalarSrc src, int which)
{
    __shared__ double lds[8];
    if (which != CHECK_HALF && uniform_state(la.st) != 0) return;   // (check_half reads the state itself)
    if (which == CHECK_HALF) {
        check_half(la, src, lds);
    } else {
        double sc[2];
        load_scalars<2>(src, sc, lds);
        check_full(la, sc);
    }
}

int launch_check(hipStream_t s, LoopArgs la, ScalarSrc src, int which)
{
    hipLaunchKernelGGL(k_check, dim3(1), dim3(kBlock), 0, s, la, src, which);
    CM_HIP(hipGetLastError());
    return CUDAMAT_OK;
}

__global__ __launch_bounds__(kBlock) void k_reduce_parts(ScalarSrc in, int K, double *out, int sqrt_it)
{
    __shared__ double lds[8];
    for (int k = 0; k < K; k++) {
        ScalarSrc one{in.ptr + k, in.count, in.stride};
        double sc[1];
        load_scalars<1>(one, sc, lds);
        if (threadIdx.x == 0) out[k] = sqrt_it ? sqrt(sc[0]) : sc[0];
    }
}

int launch_reduce_parts(hipStream_t s, ScalarSrc in, int K, double *out, int sqrt_it)
{
    hipLaunchKernelGGL(k_reduce_parts, dim3(1), dim3(kBlock), 0, s, in, K, out, sqrt_it);
    CM_HIP(hipGetLastError());
    return CUDAMAT_OK;
}

// ||x|| over the whole range of doubles, like the scaled cublasDnrm2 it stands for.  `sq` holds the partials of the plain
// sum of squares: wherever that sum is trustworthy the result is its square root, with the bits it always had.  Where it
// is inf, 0, or below DBL_MIN / DBL_EPSILON (squares that overflowed, underflowed, or lost bits as subnormals) this one
// workgroup sums again with x scaled by the power of two that brings max|x| into [0.5, 1): a rare path, not a fast one.
// A NaN in x makes the plain sum NaN, which is returned; an inf makes the norm inf.
__global__ __launch_bounds__(kBlock) void k_nrm2_finish(ScalarSrc sq, int64_t n, const double *x, double *out)
{
    __shared__ double lds[8];
    double sc[1];
    load_scalars<1>(sq, sc, lds);                  // (every thread holds the sum)
    const double plain = sc[0];
    if (!(plain == 0.0 || plain == INFINITY || plain < 0x1p-970)) {      // in range, or NaN
        if (threadIdx.x == 0) out[0] = sqrt(plain);
        return;
    }
    double big = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += kBlock) big = fmax(big, fabs(x[i]));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) big = fmax(big, __shfl_xor(big, o, 64));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = big;
    __syncthreads();
    big = fmax(fmax(lds[0], lds[1]), fmax(lds[2], lds[3]));
    if (big == 0.0 || big == INFINITY) {
        if (threadIdx.x == 0) out[0] = big;
        return;
    }
    int e = 0;
    (void)frexp(big, &e);                          // big = f * 2^e, f in [0.5, 1)
    double acc[1] = {0.0};
    for (int64_t i = threadIdx.x; i < n; i += kBlock) {
        const double v = ldexp(x[i], -e);          // exact, but for entries below 2^-1022 max|x|: they do not count
        dot_step(acc[0], v, v);
    }
    block_sum<1>(acc, lds);                        // in [0.25, n)
    if (threadIdx.x == 0) out[0] = ldexp(sqrt(acc[0]), e);
}

int launch_nrm2_finish(hipStream_t s, ScalarSrc sq, int64_t n, const double *x, double *out)
{
    hipLaunchKernelGGL(k_nrm2_finish, dim3(1), dim3(kBlock), 0, s, sq, n, x, out);
    CM_HIP(hipGetLastError());
    return CUDAMAT_OK;
}

// ------------------------------------------------------- streaming vector kernels
// 16 bytes per lane (double2) whenever every operand is 16-byte aligned; a fixed
// grid (<= kVecGridMax workgroups) walks the vector grid-stride so that the number
// of partial sums is bounded and the reduction order depends on n only.
int vec_grid(int64_t n)
{
    int64_t g = (n / 2 + kBlock - 1) / kBlock;
    if (g < 1) g = 1;
    if (g > kVecGridMax) g = kVecGridMax;
    return (int)g;
}

template <int VEC>
__global__ __launch_bounds__(kBlock) void k_init(int64_t n, const double *b, double *r, double *rw,
                                                 double *p, double *parts)
{
    __shared__ double lds[8];
    double acc[1] = {0.0};
    vec_loop<VEC>(n, [&](int64_t i, auto w) {
        constexpr int W = decltype(w)::value;
        double bb[W], rr[W];
        load_row<W>(b, i, bb); load_row<W>(r, i, rr);
#pragma unroll
        for (int j = 0; j < W; j++) {
            rr[j] = step_r0(bb[j], rr[j]);
            dot_step(acc[0], rr[j], rr[j]);
        }
        store_row<W>(r, i, rr, kAll); store_row<W>(rw, i, rr, kAll); store_row<W>(p, i, rr, kAll);      // :72-73
    });
    block_sum<1>(acc, lds);
    if (threadIdx.x == 0) {
        parts[2 * blockIdx.x] = acc[0];       // rho0 = rw.r = r.r
        parts[2 * blockIdx.x + 1] = acc[0];   // ||r0||^2
    }
}

int launch_init(hipStream_t s, int64_t n, const double *b, double *r, double *rw, double *p,
                double *parts, int *nparts)
{
    const int g = vec_grid(n);
    *nparts = g;
    CM_VEC_LAUNCH(all_aligned16(b, r, rw, p), g, k_init<VEC>, n, b, r, rw, p, parts);
}

// r / n: this rank's r0, looked at only when the sum of squares is exactly 0 (NULL in a sharded run: see init_refusal)
__global__ __launch_bounds__(kBlock) void k_init_finish(LoopState *st, ScalarSrc init, double tol, double abs_tol, int no_exit,
                                                        const double *r, int64_t n)
{
    __shared__ double lds[8];
    double sc[2];
    load_scalars<2>(init, sc, lds);                // (every thread holds the sums)
    int any = 0;
    if (sc[1] == 0.0 && r) {                       // workgroup-uniform, and rare: is r0 zero, or did every square underflow?
        for (int64_t i = threadIdx.x; i < n; i += kBlock) any |= r[i] != 0.0;
        any = __syncthreads_or(any);
    }
    if (threadIdx.x == 0) {
        const double nrm0 = sqrt(sc[1]);           // pbicgstab.cu:74 / :655
        const double tolabs = abs_tol > 0.0 ? abs_tol : tol * nrm0;
        // x0 already solves the system exactly (r0 = 0): the reference's loop would divide 0 by 0 and hand back NaNs;
        // here the loop starts frozen in the 'converged' state and x0 is returned untouched
        // abs_tol > 0 (a restart that verifies an iterate): stop at that ABSOLUTE residual, and if the residual of the
        // initial guess is already within twice of it (a recursive residual drifts by about that much) there is nothing to do
        int state = (nrm0 == 0.0 || (abs_tol > 0.0 && nrm0 <= 2.0 * abs_tol)) ? 2 : 0;
        // (a restart with abs_tol, itself >= kTolabsMin, whose true residual underflows to 0 IS below its target: not refused)
        if (!no_exit && (tol > 0.0 || abs_tol > 0.0) && init_refusal(nrm0, tolabs, any != 0 && !(abs_tol > 0.0))) state = 3;
        st->state = state;
        st->it = 0;
        st->rho[0] = 1.0;                          // pbicgstab.cu:617 (rho = 1)
        st->rho[1] = 1.0;
        st->alpha = 1.0;                           // :615
        st->omega = 1.0;                           // :614
        st->nrm0 = nrm0;
        st->tolabs = tolabs;
        st->nrm = nrm0;
    }
}

int launch_init_finish(hipStream_t s, LoopState *st, ScalarSrc init, double tol, double abs_tol, int no_exit, const double *r,
                       int64_t n)
{
    hipLaunchKernelGGL(k_init_finish, dim3(1), dim3(kBlock), 0, s, st, init, tol, abs_tol, no_exit, r, n);
    CM_HIP(hipGetLastError());
    return CUDAMAT_OK;
}

// p = r + beta (p - omega v)          pbicgstab.cu:83-89 (axpy, scal, axpy) fused: step_p
// GUARD (guarded solves): `full` carries a third sum, sum |rw_i| |r_i|, from iteration 1 on (k_full<VEC, true>; at it = 0 the
// sums are k_init's two), and the test on rho follows the full-step test: check_rho.
template <int VEC, bool GUARD>
__global__ __launch_bounds__(kBlock) void k_update_p(LoopArgs la, ScalarSrc full, int64_t n,
                                                     const double *r, double *p, const double *v, double rho_eps)
{
    __shared__ double lds[GUARD ? 12 : 8];
    LoopState *st = la.st;
    if (uniform_state(st) != 0) return;
    const int it = st->it;
    double sc[2];
    [[maybe_unused]] double mag = 0.0;
    if (GUARD && it != 0) {
        double sc3[3];
        load_scalars<3>(full, sc3, lds);
        sc[0] = sc3[0]; sc[1] = sc3[1]; mag = sc3[2];
    } else {
        load_scalars<2>(full, sc, lds);
    }
    if (check_full(la, sc)) return;
    const double rho = sc[0];                              // :81  rho = rw.r
    if (GUARD && it != 0 && check_rho(la, rho, mag, rho_eps)) return;
    const double rhop = st->rho[(it + 1) & 1];             // :80
    const double alpha = st->alpha, omega = st->omega;
    if (leader()) st->rho[it & 1] = rho;
    if (it == 0) return;                                   // :83  p = r already (:73)
    const double beta = step_beta(rho, rhop, alpha, omega);
    vec_loop<VEC>(n, [&](int64_t i, auto w) {
        constexpr int W = decltype(w)::value;
        double rr[W], vv[W], pp[W];
        load_row<W>(r, i, rr); load_row<W>(v, i, vv); load_row<W>(p, i, pp);
#pragma unroll
        for (int j = 0; j < W; j++) pp[j] = step_p(rr[j], pp[j], vv[j], beta, omega);
        store_row<W>(p, i, pp, kAll);
    });
}

int launch_update_p(hipStream_t s, LoopArgs la, ScalarSrc full, int64_t n, const double *r,
                    double *p, const double *v, double rho_eps)
{
    if (rho_eps > 0.0) CM_VEC_LAUNCH(all_aligned16(r, p, v), vec_grid(n), (k_update_p<VEC, true>), la, full, n, r, p, v, rho_eps);
    CM_VEC_LAUNCH(all_aligned16(r, p, v), vec_grid(n), (k_update_p<VEC, false>), la, full, n, r, p, v, 0.0);
}

// alpha = rho/(rw.v); r -= alpha v; ||r||^2     pbicgstab.cu:106-111
// The reference's x += alpha pw (:110) is carried out by k_full of the same iteration (same operation on the same
// operands, in the reference's order; an exit at the half step applies it on the way out, loops.hip): x is read and
// written once per iteration, not twice, and this kernel moves 24 B per row.
template <int VEC>
__global__ __launch_bounds__(kBlock) void k_half(LoopArgs la, ScalarSrc rv, int64_t n, double *r,
                                                 const double *v, double *parts)
{
    __shared__ double lds[8];
    LoopState *st = la.st;
    if (st->state != 0) return;
    const int it = st->it;
    double sc[1];
    load_scalars<1>(rv, sc, lds);
    const double alpha = step_alpha(st->rho[it & 1], sc[0]);
    if (leader()) st->alpha = alpha;
    double acc[1] = {0.0};
    vec_loop<VEC>(n, [&](int64_t i, auto w) {
        constexpr int W = decltype(w)::value;
        double vv[W], rr[W];
        load_row<W>(v, i, vv); load_row<W>(r, i, rr);
#pragma unroll
        for (int j = 0; j < W; j++) {
            rr[j] = step_r_half(rr[j], vv[j], alpha);
            dot_step(acc[0], rr[j], rr[j]);                // :111
        }
        store_row<W>(r, i, rr, kAll);
    });
    block_sum<1>(acc, lds);
    if (threadIdx.x == 0) parts[blockIdx.x] = acc[0];
}

int launch_half(hipStream_t s, LoopArgs la, ScalarSrc rv, int64_t n, double *r, const double *v, double *parts, int *nparts)
{
    const int g = vec_grid(n);
    *nparts = g;
    CM_VEC_LAUNCH(all_aligned16(r, v), g, k_half<VEC>, la, rv, n, r, v, parts);
}

// omega = (t.r)/(t.t); x += omega s; r -= omega t; (rw.r, r.r); it++   pbicgstab.cu:135-151
// s may alias r (no preconditioner): s is read before r is written, per element.
// GUARD (guarded solves): a third sum rides with the two, sum |rw_i| |r_i| -- the magnitudes rho = rw.r was summed from, term
// by term in the same order -- and the partials have stride 3 (check_rho in the next k_update_p); the same bytes are moved.
template <int VEC, bool GUARD>
__global__ __launch_bounds__(kBlock) void k_full(LoopArgs la, ScalarSrc tt, int64_t n, double *x,
                                                 const double *sv, double *r, const double *t,
                                                 const double *rw, double *parts, ScalarSrc half, const double *pw)
{
    constexpr int NS = GUARD ? 3 : 2;
    __shared__ double lds[4 * NS];
    LoopState *st = la.st;
    // With a half-step test inside this launch (fused loop) the state is read once per workgroup, so a
    // workgroup can never split into waves that saw the leader's exit and waves that go on to update x and r.
    const int frozen = half.ptr ? uniform_state(st) : st->state;
    if (frozen != 0) {                // frozen: still tell the host this iteration's launches have drained
        publish_progress(la, frozen);
        return;
    }
    if (half.ptr && check_half(la, half, lds)) {   // fused small-system loop: the half-step test is evaluated here
        publish_progress(la, 1);
        return;
    }
    double sc[2];
    load_scalars<2>(tt, sc, lds);
    const double omega = step_omega(sc[0], sc[1]);
    double acc[NS] = {};
    // PW: the half step's x += alpha pw (:110), left out by k_half, first -- then :139: two roundings in the reference's order
    auto sweep = [&](auto with_pw) {
        constexpr bool PW = decltype(with_pw)::value != 0;
        const double alpha = PW ? st->alpha : 0.0;
        vec_loop<VEC>(n, [&](int64_t i, auto w) {
            constexpr int W = decltype(w)::value;
            [[maybe_unused]] double pp[W];
            double ss[W], tv[W], ww[W], rr[W], xx[W];
            load_row<W>(sv, i, ss); load_row<W>(t, i, tv); load_row<W>(rw, i, ww);
            if constexpr (PW) load_row<W>(pw, i, pp);
            load_row<W>(r, i, rr); load_row<W>(x, i, xx);
#pragma unroll
            for (int j = 0; j < W; j++) {
                if constexpr (PW) xx[j] = step_x_half(xx[j], pp[j], alpha);
                xx[j] = step_x_full(xx[j], ss[j], omega);
                rr[j] = step_r_full(rr[j], tv[j], omega);
                dot_step(acc[0], ww[j], rr[j]);            // :81 of i+1
                dot_step(acc[1], rr[j], rr[j]);            // :142
                if constexpr (GUARD) dot_step(acc[2], fabs(ww[j]), fabs(rr[j]));
            }
            store_row<W>(x, i, xx, kAll); store_row<W>(r, i, rr, kAll);
        });
    };
    if (pw) sweep(Width<1>{});
    else sweep(Width<0>{});
    block_sum<NS>(acc, lds);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < NS; k++) parts[NS * blockIdx.x + k] = acc[k];
    }
    if (leader()) {
        st->omega = omega;
        st->it = st->it + 1;                               // :148 / :151
    }
    publish_progress(la, 0);
}

int launch_full(hipStream_t s, LoopArgs la, ScalarSrc tt, int64_t n, double *x, const double *sv,
                double *r, const double *t, const double *rw, double *parts, int *nparts, ScalarSrc half, const double *pw,
                bool guard)
{
    const int g = vec_grid(n);
    *nparts = g;
    if (guard) CM_VEC_LAUNCH(all_aligned16(x, sv, r, t, rw, pw), g, (k_full<VEC, true>), la, tt, n, x, sv, r, t, rw, parts, half, pw);
    CM_VEC_LAUNCH(all_aligned16(x, sv, r, t, rw, pw), g, (k_full<VEC, false>), la, tt, n, x, sv, r, t, rw, parts, half, pw);
}

// ---------------------------------------------------------------- BLAS-1 pieces
template <int VEC>
__global__ __launch_bounds__(kBlock) void k_dot(int64_t n, const double *x, const double *y,
                                                double *parts)
{
    __shared__ double lds[8];
    double acc[1] = {0.0};
    vec_loop<VEC>(n, [&](int64_t i, auto w) {
        constexpr int W = decltype(w)::value;
        double a[W], b[W];
        load_row<W>(x, i, a); load_row<W>(y, i, b);
#pragma unroll
        for (int j = 0; j < W; j++) dot_step(acc[0], a[j], b[j]);
    });
    block_sum<1>(acc, lds);
    if (threadIdx.x == 0) parts[blockIdx.x] = acc[0];
}

int launch_dot_parts(hipStream_t s, int64_t n, const double *x, const double *y, double *parts,
                     int *nparts)
{
    const int g = vec_grid(n);
    *nparts = g;
    CM_VEC_LAUNCH(all_aligned16(x, y), g, k_dot<VEC>, n, x, y, parts);
}

template <int VEC>
__global__ __launch_bounds__(kBlock) void k_axpy(int64_t n, double alpha, const double *x, double *y)
{
    vec_loop<VEC>(n, [&](int64_t i, auto w) {
        constexpr int W = decltype(w)::value;
        double a[W], b[W];
        load_row<W>(x, i, a); load_row<W>(y, i, b);
#pragma unroll
        for (int j = 0; j < W; j++) b[j] = fma(alpha, a[j], b[j]);
        store_row<W>(y, i, b, kAll);
    });
}

int launch_axpy(hipStream_t s, int64_t n, double alpha, const double *x, double *y)
{
    CM_VEC_LAUNCH(all_aligned16(x, y), vec_grid(n), k_axpy<VEC>, n, alpha, x, y);
}

template <int VEC>
__global__ __launch_bounds__(kBlock) void k_scal(int64_t n, double alpha, double *x, int fill)
{
    vec_loop<VEC>(n, [&](int64_t i, auto w) {
        constexpr int W = decltype(w)::value;
        double a[W];
        load_row<W>(x, i, a);
#pragma unroll
        for (int j = 0; j < W; j++) {
            const double scaled = alpha * a[j];
            a[j] = fill ? alpha : scaled;
        }
        store_row<W>(x, i, a, kAll);
    });
}

int launch_scal(hipStream_t s, int64_t n, double alpha, double *x)
{
    CM_VEC_LAUNCH(all_aligned16(x), vec_grid(n), k_scal<VEC>, n, alpha, x, 0);
}

int launch_fill(hipStream_t s, int64_t n, double value, double *x)
{
    CM_VEC_LAUNCH(all_aligned16(x), vec_grid(n), k_scal<VEC>, n, value, x, 1);
}

__global__ __launch_bounds__(kBlock) void k_rebase(int64_t n, const int *in, int shift, int *out)
{
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride)
        out[i] = in[i] + shift;
}

int launch_rebase(hipStream_t s, int64_t n, const int *in, int shift, int *out)
{
    hipLaunchKernelGGL(k_rebase, dim3(row_grid(n)), dim3(kBlock), 0, s, n, in, shift, out);
    CM_HIP(hipGetLastError());
    return CUDAMAT_OK;
}

}  // namespace cm
