// batch.hip -- the kernels of the multi-column loop (batch.h): a CSR SpMM over interleaved vectors, the loop's vector kernels
// for K columns at once, and the transposes between the caller's column-major blocks and the interleaved work vectors.
//
// The SpMM reads the matrix (12 B per entry) once for K columns; each entry then gathers K contiguous doubles of X (one
// 8K-byte piece, dwordx4 loads for K >= 2) instead of one double per column and SpMV.  Every column keeps the arithmetic of
// the single-vector kernels: the vector kernels call the steps k_init, k_update_p, k_half and k_full call (steps.h), the SpMM
// sums a row as k_spmv<L> does and finishes it with the fused epilogue (device.h), so that column j of k_spmm_csr<L, K> is
// bit-identical to k_spmv<L> on column j alone.  A thread owns whole rows (all K columns), the
// grid and the row partition depend on n and L only: the reduction order of a column does not depend on K.  Within a column
// the reduction order of a ROW depends on the row's own length and L only: rows of at most 4096 entries are summed by their
// L lanes, every longer one by the whole workgroup -- however many long rows share a partition (device.h: LongRows).
// A column whose state is not 0 is never written again: its x, r, p and history keep their bits (stores are masked by
// column; the mask is uniform over the workgroup, so the branches do not diverge).
#include "batch.h"
#include "device.h"

#pragma clang fp contract(off)      // no product-sum here is left to the compiler: fma() is written where one rounding is meant

namespace cm {

namespace {

__device__ __forceinline__ LoopArgs col_args(const BatchArgs &b, int j)
{
    LoopArgs l{};
    l.st = b.st + j;
    l.hist = b.hist ? b.hist + (size_t)j * (size_t)b.hist_cap : nullptr;
    l.hist_cap = b.hist_cap;
    l.loop = b.loop;
    l.no_exit = b.no_exit;
    l.k = b.k;
    return l;
}

// bit j set: column j is running (state 0), as ONE thread of the workgroup read the states (see uniform_state)
template <int K>
__device__ __forceinline__ unsigned live_mask(const LoopState *st, int want = 0)
{
    __shared__ unsigned s_mask;
    if (threadIdx.x == 0) {
        unsigned m = 0;
        for (int j = 0; j < K; j++)
            if (st[j].state == want) m |= 1u << j;
        s_mask = m;
    }
    __syncthreads();
    const unsigned v = s_mask;
    __syncthreads();
    return v;
}

// N partial sums per workgroup (stride N), summed in load_scalars' fixed order; lds: 4 N doubles
template <int N>
__device__ __forceinline__ void load_parts(const double *parts, int count, double (&out)[N], double *lds)
{
#pragma unroll
    for (int q = 0; q < N; q++) out[q] = 0.0;
    for (int c = threadIdx.x; c < count; c += kBlock) {
#pragma unroll
        for (int q = 0; q < N; q++) out[q] += parts[(size_t)c * N + q];
    }
    block_sum<N>(out, lds);
}

__device__ __forceinline__ void publish_b(const BatchArgs &la, int all_stopped)
{
    if (la.snap && leader())
        __hip_atomic_store(&la.snap[la.k % la.snap_slots],
                           ((unsigned long long)(unsigned)(la.k + 1) << 32) | (unsigned long long)(unsigned)all_stopped,
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

}  // namespace

// ------------------------------------------------------------------------------------------------------------- SpMM
// Long rows as in k_spmv (spmv_csr.hip), through the same helpers (device.h: LongRows): never summed by their group, swept by the
// whole workgroup in increasing row order however many a partition holds.
// S: per-column shifts (a.dk, interleaved) in place of the shared a.d -- the same term at the same place in both epilogues, so
// column j is what the S = false kernel gives with d = column j of the shifts.  A template parameter: the S = false
// instantiations compile to what they were before the shifts existed.

template <int L, int K, bool S>
__global__ __launch_bounds__(kBlock) void k_spmm_csr(SpmmArgs a, int rows_per_block)
{
    __shared__ double lds[8 * K];
    if (a.loop.st) {
        if (a.check == CHECK_HALF) {
            for (int j = 0; j < K; j++) {
                const LoopArgs lj = col_args(a.loop, j);
                (void)check_half(lj, ScalarSrc{a.half + j, a.half_count, K}, lds);
            }
        }
        if (live_mask<K>(a.loop.st) == 0) return;
    }
    constexpr int RPB = kBlock / L;
    const int lane = threadIdx.x & (L - 1);
    const int group = threadIdx.x / L;
    const int nb = gridDim.x, b = blockIdx.x;
    const int cid = xcd_chunk(b, nb);
    const long long r0 = (long long)cid * rows_per_block;
    const int row_begin = (int)(r0 < a.n ? r0 : a.n);
    const int row_end = (int)(r0 + rows_per_block < a.n ? r0 + rows_per_block : a.n);

    __shared__ LongRows lr;
    if (threadIdx.x == 0) lr.noted = 0;
    __syncthreads();

    double acc[2 * K];
#pragma unroll
    for (int q = 0; q < 2 * K; q++) acc[q] = 0.0;
    for (int row = row_begin + group; row < row_end; row += RPB) {
        const int s = a.rp[row], e = a.rp[row + 1];
        if (e - s > kLongRow) {
            if (lane == 0) long_rows_note(lr, row);
            continue;
        }
        double sum[K];
#pragma unroll
        for (int j = 0; j < K; j++) sum[j] = 0.0;
        for (int k = s + lane; k < e; k += L) {
            const double v = __builtin_nontemporal_load(a.val + k);
            double xv[K];
            load_row<K>(a.x, __builtin_nontemporal_load(a.ci + k), xv);
#pragma unroll
            for (int j = 0; j < K; j++) sum[j] = fma(v, xv[j], sum[j]);
        }
#pragma unroll
        for (int j = 0; j < K; j++) sum[j] = group_sum<L>(sum[j]);
        if (lane == 0) spmm_finish_row<K, S>(a, row, sum, acc);
    }
    __syncthreads();
    for (int done = 0, nl; (nl = long_rows_round(lr, a.rp, row_begin, row_end, done)) > 0; done += nl) {
        for (int i = 0; i < nl; i++) {
            const int row = lr.rows[i];
            const int s = a.rp[row], e = a.rp[row + 1];
            double part[K];
#pragma unroll
            for (int j = 0; j < K; j++) part[j] = 0.0;
            for (int k = s + (int)threadIdx.x; k < e; k += kBlock) {
                const double v = __builtin_nontemporal_load(a.val + k);
                double xv[K];
                load_row<K>(a.x, __builtin_nontemporal_load(a.ci + k), xv);
#pragma unroll
                for (int j = 0; j < K; j++) part[j] = fma(v, xv[j], part[j]);
            }
            block_sum<K>(part, lds);
            if (threadIdx.x == 0) spmm_finish_row<K, S>(a, row, part, acc);
        }
    }
    if (a.dot) {
        block_sum<2 * K>(acc, lds);
        if (threadIdx.x == 0) {
#pragma unroll
            for (int q = 0; q < 2 * K; q++) a.parts[(size_t)b * 2 * K + q] = acc[q];
        }
    }
}

template <int L, bool S>
static int launch_spmm_l(hipStream_t s, int K, const SpmmArgs &a, int grid, int rpb)
{
    switch (K) {
    case 1: hipLaunchKernelGGL((k_spmm_csr<L, 1, S>), dim3(grid), dim3(kBlock), 0, s, a, rpb); break;
    case 2: hipLaunchKernelGGL((k_spmm_csr<L, 2, S>), dim3(grid), dim3(kBlock), 0, s, a, rpb); break;
    case 4: hipLaunchKernelGGL((k_spmm_csr<L, 4, S>), dim3(grid), dim3(kBlock), 0, s, a, rpb); break;
    case 8: hipLaunchKernelGGL((k_spmm_csr<L, 8, S>), dim3(grid), dim3(kBlock), 0, s, a, rpb); break;
    default: set_error("SpMM: %d columns per batch", K); return CUDAMAT_ERR_ARG;
    }
    CM_HIP(hipGetLastError());
    return CUDAMAT_OK;
}

template <bool S>
static int launch_spmm_s(hipStream_t s, int L, int K, const SpmmArgs &a, int grid, int rpb)
{
    switch (L) {
    case 2: return launch_spmm_l<2, S>(s, K, a, grid, rpb);
    case 4: return launch_spmm_l<4, S>(s, K, a, grid, rpb);
    case 8: return launch_spmm_l<8, S>(s, K, a, grid, rpb);
    case 16: return launch_spmm_l<16, S>(s, K, a, grid, rpb);
    case 32: return launch_spmm_l<32, S>(s, K, a, grid, rpb);
    case 64: return launch_spmm_l<64, S>(s, K, a, grid, rpb);
    }
    set_error("SpMM: %d lanes per row", L);
    return CUDAMAT_ERR_ARG;
}

int launch_spmm(hipStream_t s, int L, int K, const SpmmArgs &a)
{
    if (a.dk && a.d) {
        set_error("SpMM: a shared shift and per-column shifts together");
        return CUDAMAT_ERR_ARG;
    }
    int grid = 1, rpb = 1;
    spmv_partition(L, a.n, &grid, &rpb);
    return a.dk ? launch_spmm_s<true>(s, L, K, a, grid, rpb) : launch_spmm_s<false>(s, L, K, a, grid, rpb);
}

#define CM_BATCH_DISPATCH(KERNEL, GRID, ...)                                                                  \
    switch (K) {                                                                                              \
    case 1: hipLaunchKernelGGL(KERNEL<1>, dim3(GRID), dim3(kBlock), 0, s, __VA_ARGS__); break;                \
    case 2: hipLaunchKernelGGL(KERNEL<2>, dim3(GRID), dim3(kBlock), 0, s, __VA_ARGS__); break;                \
    case 4: hipLaunchKernelGGL(KERNEL<4>, dim3(GRID), dim3(kBlock), 0, s, __VA_ARGS__); break;                \
    case 8: hipLaunchKernelGGL(KERNEL<8>, dim3(GRID), dim3(kBlock), 0, s, __VA_ARGS__); break;                \
    default: set_error("batch of %d columns", K); return CUDAMAT_ERR_ARG;                                     \
    }                                                                                                         \
    CM_HIP(hipGetLastError());                                                                                \
    return CUDAMAT_OK;

// --------------------------------------------------------------------------------------------------- transposes
template <int K>
__global__ __launch_bounds__(kBlock) void k_batch_in(int kc, int64_t rows, int64_t rows_out, const double *src, int64_t ld,
                                                     double fill, double *dst)
{
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < rows_out; i += stride) {
        double v[K];
#pragma unroll
        for (int j = 0; j < K; j++) v[j] = (j < kc && i < rows) ? src[(size_t)j * ld + i] : fill;
        store_row<K>(dst, i, v, kAll);
    }
}

template <int K>
__global__ __launch_bounds__(kBlock) void k_batch_out(int kc, int64_t rows, const double *src, double *dst, int64_t ld)
{
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < rows; i += stride) {
        double v[K];
        load_row<K>(src, i, v);
#pragma unroll
        for (int j = 0; j < K; j++)
            if (j < kc) dst[(size_t)j * ld + i] = v[j];
    }
}

int launch_batch_in(hipStream_t s, int K, int kc, int64_t rows, int64_t rows_out, const double *src, int64_t ld, double fill,
                    double *dst)
{
    const int g = row_grid(rows_out);
    CM_BATCH_DISPATCH(k_batch_in, g, kc, rows, rows_out, src, ld, fill, dst)
}

int launch_batch_out(hipStream_t s, int K, int kc, int64_t rows, const double *src, double *dst, int64_t ld)
{
    const int g = row_grid(rows);
    CM_BATCH_DISPATCH(k_batch_out, g, kc, rows, src, dst, ld)
}

// ----------------------------------------------------------------------------------------------- vector kernels
// r = b - r, rw = r, p = r; (r.r, r.r) per column                                       pbicgstab.cu:67-74
template <int K>
__global__ __launch_bounds__(kBlock) void k_init_b(int64_t n, const double *b, double *r, double *rw, double *p, double *parts)
{
    __shared__ double lds[4 * K];
    double acc[K];
#pragma unroll
    for (int j = 0; j < K; j++) acc[j] = 0.0;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        double bb[K], rr[K];
        load_row<K>(b, i, bb);
        load_row<K>(r, i, rr);
#pragma unroll
        for (int j = 0; j < K; j++) {
            rr[j] = step_r0(bb[j], rr[j]);
            dot_step(acc[j], rr[j], rr[j]);
        }
        store_row<K>(r, i, rr, kAll);
        store_row<K>(rw, i, rr, kAll);
        store_row<K>(p, i, rr, kAll);
    }
    block_sum<K>(acc, lds);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int j = 0; j < K; j++) {
            parts[(size_t)blockIdx.x * 2 * K + 2 * j] = acc[j];
            parts[(size_t)blockIdx.x * 2 * K + 2 * j + 1] = acc[j];
        }
    }
}

int launch_init_b(hipStream_t s, int K, int64_t n, const double *b, double *r, double *rw, double *p, double *parts, int *nparts)
{
    const int g = vec_grid(n);
    *nparts = g;
    CM_BATCH_DISPATCH(k_init_b, g, n, b, r, rw, p, parts)
}

// r (interleaved, n rows): looked at only for a column whose sum of squares is exactly 0 (device.h: init_refusal)
template <int K>
__global__ __launch_bounds__(kBlock) void k_init_finish_b(int kc, LoopState *st, const double *parts, int count, double tol,
                                                          int no_exit, const double *r, int64_t n)
{
    __shared__ double lds[8 * K];
    double sc[2 * K];
    load_parts<2 * K>(parts, count, sc, lds);      // (every thread holds the sums)
    unsigned nonzero = 0;
    for (int j = 0; j < kc; j++) {
        if (sc[2 * j + 1] != 0.0) continue;        // workgroup-uniform, and rare: is the column's r0 zero, or did every square underflow?
        int any = 0;
        for (int64_t i = threadIdx.x; i < n; i += kBlock) any |= r[(size_t)i * K + j] != 0.0;
        if (__syncthreads_or(any)) nonzero |= 1u << j;
    }
    if (threadIdx.x == 0) {
        for (int j = 0; j < K; j++) {
            const double nrm0 = j < kc ? sqrt(sc[2 * j + 1]) : 0.0;     // pbicgstab.cu:74 / :655
            LoopState *q = st + j;
            int state = nrm0 == 0.0 ? 2 : 0;     // x0 solves the system (or a padding column): frozen from the start
            if (j < kc && !no_exit && tol > 0.0 && init_refusal(nrm0, tol * nrm0, (nonzero >> j) & 1u)) state = 3;
            q->state = state;
            q->it = 0;
            q->rho[0] = 1.0;
            q->rho[1] = 1.0;
            q->alpha = 1.0;
            q->omega = 1.0;
            q->nrm0 = nrm0;
            q->tolabs = tol * nrm0;
            q->nrm = nrm0;
        }
    }
}

int launch_init_finish_b(hipStream_t s, int K, int kc, LoopState *st, const double *parts, int count, double tol, int no_exit,
                         const double *r, int64_t n)
{
    CM_BATCH_DISPATCH(k_init_finish_b, 1, kc, st, parts, count, tol, no_exit, r, n)
}

// full-step test of the previous iteration; p = r + beta (p - omega v)                 pbicgstab.cu:80-89
template <int K>
__global__ __launch_bounds__(kBlock) void k_update_p_b(BatchArgs la, const double *full, int full_count, int64_t n,
                                                       const double *r, double *p, const double *v)
{
    __shared__ double lds[8 * K];
    unsigned live = live_mask<K>(la.st);
    if (!live) return;
    double sc[2 * K];
    load_parts<2 * K>(full, full_count, sc, lds);
    double beta[K], omega[K];
    unsigned upd = 0;
#pragma unroll
    for (int j = 0; j < K; j++) {
        beta[j] = 0.0;
        omega[j] = 0.0;
        if (!(live & (1u << j))) continue;
        LoopState *st = la.st + j;
        const int it = st->it;
        const double two[2] = {sc[2 * j], sc[2 * j + 1]};
        if (check_full(col_args(la, j), two)) continue;
        const double rho = two[0];                             // :81
        const double rhop = st->rho[(it + 1) & 1];             // :80
        if (leader()) st->rho[it & 1] = rho;
        if (it == 0) continue;                                 // :83  p = r already (:73)
        omega[j] = st->omega;
        beta[j] = step_beta(rho, rhop, st->alpha, omega[j]);
        upd |= 1u << j;
    }
    if (!upd) return;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        double rr[K], vv[K], pp[K];
        load_row<K>(r, i, rr);
        load_row<K>(v, i, vv);
        load_row<K>(p, i, pp);
#pragma unroll
        for (int j = 0; j < K; j++) pp[j] = step_p(rr[j], pp[j], vv[j], beta[j], omega[j]);
        store_row<K>(p, i, pp, upd);
    }
}

int launch_update_p_b(hipStream_t s, int K, BatchArgs la, const double *full, int full_count, int64_t n, const double *r,
                      double *p, const double *v)
{
    const int g = vec_grid(n);
    CM_BATCH_DISPATCH(k_update_p_b, g, la, full, full_count, n, r, p, v)
}

// alpha = rho / (rw.v); r -= alpha v; ||r||^2 per column                             pbicgstab.cu:106-111
template <int K>
__global__ __launch_bounds__(kBlock) void k_half_b(BatchArgs la, const double *rv, int rv_count, int64_t n, double *r,
                                                   const double *v, double *parts)
{
    __shared__ double lds[8 * K];
    const unsigned live = live_mask<K>(la.st);
    if (!live) return;
    double sc[2 * K];
    load_parts<2 * K>(rv, rv_count, sc, lds);
    double alpha[K];
#pragma unroll
    for (int j = 0; j < K; j++) {
        alpha[j] = 0.0;
        if (!(live & (1u << j))) continue;
        LoopState *st = la.st + j;
        alpha[j] = step_alpha(st->rho[st->it & 1], sc[2 * j]);
        if (leader()) st->alpha = alpha[j];
    }
    double acc[K];
#pragma unroll
    for (int j = 0; j < K; j++) acc[j] = 0.0;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        double rr[K], vv[K];
        load_row<K>(r, i, rr);
        load_row<K>(v, i, vv);
#pragma unroll
        for (int j = 0; j < K; j++) {
            rr[j] = step_r_half(rr[j], vv[j], alpha[j]);
            dot_step(acc[j], rr[j], rr[j]);                    // :111
        }
        store_row<K>(r, i, rr, live);
    }
    block_sum<K>(acc, lds);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int j = 0; j < K; j++) parts[(size_t)blockIdx.x * K + j] = acc[j];
    }
}

int launch_half_b(hipStream_t s, int K, BatchArgs la, const double *rv, int rv_count, int64_t n, double *r, const double *v,
                  double *parts, int *nparts)
{
    const int g = vec_grid(n);
    *nparts = g;
    CM_BATCH_DISPATCH(k_half_b, g, la, rv, rv_count, n, r, v, parts)
}

// omega = (t.r)/(t.t); x += alpha pw; x += omega s; r -= omega t; (rw.r, r.r); it++   pbicgstab.cu:110, :135-151
// s may alias r: a row's s is read before its r is written.
template <int K>
__global__ __launch_bounds__(kBlock) void k_full_b(BatchArgs la, const double *tt, int tt_count, int64_t n, double *x,
                                                   const double *sv, double *r, const double *t, const double *rw,
                                                   const double *pw, double *parts)
{
    __shared__ double lds[8 * K];
    const unsigned live = live_mask<K>(la.st);
    if (!live) {                      // every column stopped: still tell the host this iteration's launches have drained
        publish_b(la, 1);
        return;
    }
    double sc[2 * K];
    load_parts<2 * K>(tt, tt_count, sc, lds);
    double omega[K], alpha[K];
#pragma unroll
    for (int j = 0; j < K; j++) {
        omega[j] = step_omega(sc[2 * j], sc[2 * j + 1]);
        alpha[j] = (live & (1u << j)) ? la.st[j].alpha : 0.0;
    }
    double acc[2 * K];
#pragma unroll
    for (int q = 0; q < 2 * K; q++) acc[q] = 0.0;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        double ss[K], tv[K], ww[K], pp[K], rr[K], xx[K];
        load_row<K>(sv, i, ss);
        load_row<K>(t, i, tv);
        load_row<K>(rw, i, ww);
        load_row<K>(pw, i, pp);
        load_row<K>(r, i, rr);
        load_row<K>(x, i, xx);
#pragma unroll
        for (int j = 0; j < K; j++) {
            xx[j] = step_x_half(xx[j], pp[j], alpha[j]);
            xx[j] = step_x_full(xx[j], ss[j], omega[j]);
            rr[j] = step_r_full(rr[j], tv[j], omega[j]);
            dot_step(acc[2 * j], ww[j], rr[j]);                // :81 of i+1
            dot_step(acc[2 * j + 1], rr[j], rr[j]);            // :142
        }
        store_row<K>(x, i, xx, live);
        store_row<K>(r, i, rr, live);
    }
    block_sum<2 * K>(acc, lds);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int q = 0; q < 2 * K; q++) parts[(size_t)blockIdx.x * 2 * K + q] = acc[q];
    }
    if (leader()) {
        for (int j = 0; j < K; j++) {
            if (!(live & (1u << j))) continue;
            la.st[j].omega = omega[j];
            la.st[j].it = la.st[j].it + 1;                     // :148 / :151
        }
    }
    publish_b(la, 0);
}

int launch_full_b(hipStream_t s, int K, BatchArgs la, const double *tt, int tt_count, int64_t n, double *x, const double *sv,
                  double *r, const double *t, const double *rw, const double *pw, double *parts, int *nparts)
{
    const int g = vec_grid(n);
    *nparts = g;
    CM_BATCH_DISPATCH(k_full_b, g, la, tt, tt_count, n, x, sv, r, t, rw, pw, parts)
}

template <int K>
__global__ __launch_bounds__(kBlock) void k_check_full_b(BatchArgs la, const double *full, int full_count)
{
    __shared__ double lds[8 * K];
    const unsigned live = live_mask<K>(la.st);
    if (!live) return;
    double sc[2 * K];
    load_parts<2 * K>(full, full_count, sc, lds);
#pragma unroll
    for (int j = 0; j < K; j++) {
        if (!(live & (1u << j))) continue;
        const double two[2] = {sc[2 * j], sc[2 * j + 1]};
        (void)check_full(col_args(la, j), two);
    }
}

int launch_check_full_b(hipStream_t s, int K, BatchArgs la, const double *full, int full_count)
{
    CM_BATCH_DISPATCH(k_check_full_b, 1, la, full, full_count)
}

// the half-step tests of every column on their own (one workgroup): the preconditioned loop must decide them before it
// computes M^-1 r, so they cannot ride in the second SpMM's prologue; the same check_half per column, from the same partials
template <int K>
__global__ __launch_bounds__(kBlock) void k_check_half_b(BatchArgs la, const double *half, int half_count)
{
    __shared__ double lds[8 * K];
    for (int j = 0; j < K; j++) (void)check_half(col_args(la, j), ScalarSrc{half + j, half_count, K}, lds);
}

int launch_check_half_b(hipStream_t s, int K, BatchArgs la, const double *half, int half_count)
{
    CM_BATCH_DISPATCH(k_check_half_b, 1, la, half, half_count)
}

template <int K>
__global__ __launch_bounds__(kBlock) void k_half_exit_b(const LoopState *st, int64_t n, const double *pw, double *x)
{
    const unsigned half = live_mask<K>(st, 1);
    if (!half) return;
    double alpha[K];
#pragma unroll
    for (int j = 0; j < K; j++) alpha[j] = (half & (1u << j)) ? st[j].alpha : 0.0;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        double pp[K], xx[K];
        load_row<K>(pw, i, pp);
        load_row<K>(x, i, xx);
#pragma unroll
        for (int j = 0; j < K; j++) xx[j] = step_x_half(xx[j], pp[j], alpha[j]);
        store_row<K>(x, i, xx, half);
    }
}

int launch_half_exit_b(hipStream_t s, int K, const LoopState *st, int64_t n, const double *pw, double *x)
{
    const int g = vec_grid(n);
    CM_BATCH_DISPATCH(k_half_exit_b, g, st, n, pw, x)
}

}  // namespace cm
