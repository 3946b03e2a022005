// device.h -- device-side helpers shared by the kernels of libcudamat_hip.so: fixed-order workgroup reductions, the
// scalars that live in HBM (per-workgroup partial sums summed by every consumer), the loop state as a workgroup reads
// it, the half-step stopping test that SpMV kernels evaluate in their prologue, and the pieces every SpMV-shaped kernel
// shares: prologue, XCD-aware dealing, row epilogue (two rounding flavours), dot partials.  256-thread workgroups (kBlock).
#pragma once
#include <hip/hip_runtime.h>

#include "batch.h"
#include "kernels.h"
#include "steps.h"

namespace cm {

// ------------------------------------------------------------------ reductions
__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

template <int L>
__device__ __forceinline__ double group_sum(double v)
{
#pragma unroll
    for (int o = L / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// every thread of the 256-thread workgroup receives the K sums (fixed order)
template <int K>
__device__ __forceinline__ void block_sum(double (&v)[K], double *lds)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < K; k++) v[k] = wave_sum(v[k]);
    __syncthreads();  // lds may still be read from a previous use
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < K; k++) lds[wave * K + k] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; k++)
        v[k] = ((lds[0 * K + k] + lds[1 * K + k]) + lds[2 * K + k]) + lds[3 * K + k];
}

// ------------------------------------ long rows of the lanes-per-row kernels (k_spmv<L>, k_spmm_csr<L, K>)
// A row with more than kLongRow entries is NEVER summed by its group of L lanes: the group's first lane notes it
// (long_rows_note), and after the short rows the whole workgroup sweeps every noted row with its 256 lanes (lane-strided
// partial sums, block_sum) in increasing row order.  The contract: the reduction order of a row depends on its own length
// and L only -- not on how many long rows share its partition, nor on the order in which the waves met them.
// The table holds kLongRowSlots ids.  A partition with more long rows than that (rows_per_block >= 64: L <= 4, or
// n > 2048 * 256 / L) takes them in rounds: the ids the groups wrote are dropped (which rows found a slot depends on wave
// scheduling) and thread 0 lists the partition's long rows straight from rp, in order, kLongRowSlots per round.
constexpr int kLongRow = 4096;
constexpr int kLongRowSlots = 32;

struct LongRows {                 // one per workgroup, in LDS; noted = 0 before the short-row loop
    int rows[kLongRowSlots];
    int noted;                    // long rows the groups met (may exceed the slots)
    int count;                    // ids in rows[] for the round being swept
    int next;                     // more long rows than slots: the first row not examined yet
};

__device__ __forceinline__ void long_rows_note(LongRows &t, int row)
{
    const int slot = atomicAdd(&t.noted, 1);
    if (slot < kLongRowSlots) t.rows[slot] = row;
}

// Called by the whole workgroup after the barrier that ends the short-row loop, and again after each round's sweep (`done` =
// long rows swept so far; a sweep of >= 1 row passes block_sum's barriers, so nobody still reads the previous round's ids).
// Returns the number of ids now in t.rows, increasing; 0: every long row has been swept.  Uniform over the workgroup.
__device__ __forceinline__ int long_rows_round(LongRows &t, const int *rp, int row_begin, int row_end, int done)
{
    const int total = t.noted;
    if (done >= total) return 0;
    if (threadIdx.x == 0) {
        if (total <= kLongRowSlots) {      // insertion sort of a handful of ids
            for (int i = 1; i < total; i++) {
                const int r = t.rows[i];
                int j = i - 1;
                while (j >= 0 && t.rows[j] > r) { t.rows[j + 1] = t.rows[j]; j--; }
                t.rows[j + 1] = r;
            }
            t.count = total;
        } else {
            int r = done == 0 ? row_begin : t.next, m = 0;
            for (; r < row_end && m < kLongRowSlots; r++)
                if (rp[r + 1] - rp[r] > kLongRow) t.rows[m++] = r;
            t.count = m;
            t.next = r;
        }
    }
    __syncthreads();
    return t.count;
}

template <int K>
__device__ __forceinline__ void load_scalars(const ScalarSrc &s, double (&out)[K], double *lds)
{
    if (s.count == 0) {
#pragma unroll
        for (int k = 0; k < K; k++) out[k] = s.ptr[k];
        return;
    }
#pragma unroll
    for (int k = 0; k < K; k++) out[k] = 0.0;
    for (int j = threadIdx.x; j < s.count; j += kBlock) {
#pragma unroll
        for (int k = 0; k < K; k++) out[k] += s.ptr[(size_t)j * s.stride + k];
    }
    block_sum<K>(out, lds);
}

__device__ __forceinline__ bool leader() { return blockIdx.x == 0 && threadIdx.x == 0; }

// The loop state as ONE thread of the workgroup reads it, handed to the others through LDS.  A stopping
// test's leader may publish state != 0 while this very launch is still starting waves; waves of one
// workgroup must not disagree about it (those that carried on would reduce over LDS slots the others never
// wrote).  Different workgroups may still read different values: each then evaluates the same test on the
// same partial sums and reaches the same decision.  Used by every kernel that contains a stopping test.
__device__ __forceinline__ int uniform_state(const LoopState *st)
{
    __shared__ int s_state;
    if (threadIdx.x == 0) s_state = st->state;
    __syncthreads();
    const int v = s_state;
    __syncthreads();
    return v;
}

__device__ __forceinline__ void publish_progress(const LoopArgs &la, int state)
{
    if (la.snap && leader())
        __hip_atomic_store(&la.snap[la.k % la.snap_slots],
                           ((unsigned long long)(unsigned)(la.k + 1) << 32) | (unsigned long long)(unsigned)state,
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// ------------------------------------------------------------- stopping tests
// The range in which `nrm < tolabs` on plain sums of squares means what it says.  The loops neither rescale nor carry
// scaled norms: a solve whose stopping tests cannot be trusted is REFUSED when its state is initialised (state 3, no
// iteration, x0 untouched) instead of reporting a convergence it has not computed:
//   - ||r0|| is not finite (the sum of squares overflowed, or holds a NaN): tolabs would be inf or NaN;
//   - ||r0|| == 0 although r0 has a non-zero entry: every square underflowed (r0 == 0 itself is the 'x0 solves the
//     system' case and stays converged).  r_nonzero comes from a look at r0 that only this case pays for.  A sharded run
//     does not take it yet: each rank holds a slice of r0 and the ranks must agree, so the answer would have to travel
//     with the all-reduce of the initial sums (its first slot only repeats the second); until then total underflow there
//     still reads as r0 == 0;
//   - 0 < tolabs < kTolabsMin = sqrt(DBL_MIN / DBL_EPSILON) = 2^-485: a residual at the tolerance has squares below
//     DBL_MIN / DBL_EPSILON = 2^-970, where the spacing of doubles (2^-1074, subnormal) exceeds DBL_EPSILON times the
//     square: the terms of the sum are no longer held to full precision and vanish altogether below 2^-537, so the sum
//     can pass the test for a residual that does not.
// Only called where a stopping test applies (no FLAG_NO_EXIT, a tolerance > 0).
constexpr double kTolabsMin = 0x1p-485;

__device__ __forceinline__ bool init_refusal(double nrm0, double tolabs, bool r_nonzero)
{
    return !isfinite(nrm0) || (nrm0 == 0.0 && r_nonzero) || (tolabs > 0.0 && tolabs < kTolabsMin);
}

// half-step test, pbicgstab.cu:111-118.  Returns true when the caller must return.
__device__ __forceinline__ bool check_half(const LoopArgs &la, const ScalarSrc &half, double *lds)
{
    LoopState *st = la.st;
    if (uniform_state(st) != 0) return true;
    double sc[1];
    load_scalars<1>(half, sc, lds);
    const double nrm = sqrt(sc[0]);
    const int it = st->it;
    if (la.loop == CUDAMAT_LOOP_PBICGSTAB) {
        if (leader()) {
            st->nrm = nrm;
            if (la.hist && 2 * it < la.hist_cap) la.hist[2 * it] = nrm;
        }
        if (!la.no_exit && nrm < st->tolabs) {
            if (leader()) st->state = 1;
            return true;
        }
        // A NaN residual never passes a test: the reference would spin to maxit on NaNs (pbicgstab.cu:116 has no guard);
        // here the loop stops and reports a breakdown, like the reference's own guard of the other loop (:735-742).
        if (!la.no_exit && isnan(nrm)) {
            if (leader()) st->state = 3;
            return true;
        }
    }
    return false;
}

// full-step test of iteration it-1, pbicgstab.cu:142-151 / :723-742.  sc = (rw.r, r.r)
__device__ __forceinline__ bool check_full(const LoopArgs &la, const double (&sc)[2])
{
    LoopState *st = la.st;
    const int it = st->it;
    if (it == 0) return false;
    const double nrm = sqrt(sc[1]);
    const double omega = st->omega;
    if (leader()) {
        st->nrm = nrm;
        if (la.hist) {
            const int slot = (la.loop != CUDAMAT_LOOP_PBICGSTAB2) ? 2 * (it - 1) + 1 : it - 1;
            if (slot < la.hist_cap) la.hist[slot] = nrm;
        }
    }
    if (la.no_exit) return false;
    if (nrm < st->tolabs) {
        if (leader()) st->state = 2;
        return true;
    }
    if (la.loop == CUDAMAT_LOOP_PBICGSTAB2 && (fabs(omega) < 1e-5 || isnan(omega))) {
        if (leader()) st->state = 3;
        return true;
    }
    if (isnan(nrm)) {                       // (see check_half)
        if (leader()) st->state = 3;
        return true;
    }
    return false;
}

// The one stopping test of the loops that test once per iteration (BiCGSTAB(2): per sweep; CG): ||r|| of iteration it - 1
// against the tolerance, one history entry per iteration, at slot it - 1.  rr = r.r.  Returns true when the caller must
// return.  Called by every workgroup with the same sums: they reach the same decision.
__device__ __forceinline__ bool check_iteration_end(const LoopArgs &la, double rr)
{
    LoopState *st = la.st;
    const int it = st->it;
    if (it == 0) return false;
    const double nrm = sqrt(rr);
    if (leader()) {
        st->nrm = nrm;
        if (la.hist && it - 1 < la.hist_cap) la.hist[it - 1] = nrm;
    }
    if (la.no_exit) return false;
    if (nrm < st->tolabs) {
        if (leader()) st->state = 2;
        return true;
    }
    if (isnan(nrm)) {
        if (leader()) st->state = 3;
        return true;
    }
    return false;
}

// a scalar the loop cannot go on with; under FLAG_NO_EXIT no test is taken.  Returns true when the caller must return.
__device__ __forceinline__ bool loop_breakdown(const LoopArgs &la, bool bad)
{
    if (!bad || la.no_exit) return false;
    if (leader()) la.st->state = 3;
    return true;
}

// The test on rho of a guarded solve (CUDAMAT_FLAG_GUARD), at the top of iteration it >= 1 after check_full, so that a
// convergence exit wins (at it = 0, rho = r.r).  rho = rw.r and mag = sum |rw_i| |r_i| come from the same terms in the same
// order (k_full<VEC, true>), so |rho| <= mag holds in floating point too; eps = GUARD_RHO_ULPS * 2^-52 (exact).  When
// |rho| <= eps * mag -- rho = 0 and a NaN rho included -- rho has not one significant bit left and every later beta would
// divide rounding noise: state 4, the loop freezes with x the complete iterate of iteration it - 1 (k_full applied both
// updates) and r, p untouched, and the host restarts from the true residual of x.  Under FLAG_NO_EXIT the test is evaluated
// and never taken.  Returns true when the caller must return.
__device__ __forceinline__ bool check_rho(const LoopArgs &la, double rho, double mag, double eps)
{
#pragma clang fp contract(off)
    const bool lost = !(fabs(rho) > eps * mag);
    if (!lost || la.no_exit) return false;
    if (leader()) la.st->state = 4;
    return true;
}

// ------------------------------------------------- interleaved vectors (batch.h)
// row i of an n x K row-major block (K in {1, 2, 4, 8}): K contiguous doubles, moved 16 bytes at a time for K >= 2
template <int K>
__device__ __forceinline__ void load_row(const double *p, int64_t i, double (&v)[K])
{
    if constexpr (K == 1) {
        v[0] = p[i];
    } else {
        const double2 *q = (const double2 *)(p + (size_t)i * K);
#pragma unroll
        for (int h = 0; h < K / 2; h++) {
            const double2 t = q[h];
            v[2 * h] = t.x;
            v[2 * h + 1] = t.y;
        }
    }
}

// the columns of `mask` only
template <int K>
__device__ __forceinline__ void store_row(double *p, int64_t i, const double (&v)[K], unsigned mask)
{
    if constexpr (K == 1) {
        if (mask & 1u) p[i] = v[0];
    } else {
        double *row = p + (size_t)i * K;
#pragma unroll
        for (int h = 0; h < K / 2; h++) {
            const unsigned m = (mask >> (2 * h)) & 3u;
            if (m == 3u) ((double2 *)row)[h] = make_double2(v[2 * h], v[2 * h + 1]);
            else if (m == 1u) row[2 * h] = v[2 * h];
            else if (m == 2u) row[2 * h + 1] = v[2 * h + 1];
        }
    }
}

constexpr unsigned kAll = 0xffu;       // store_row: every column

// entries of one stream tile (kernels.h: SpmvPlan.stream_rows); LDS: kStreamNnz products + R+1 row pointers
constexpr int kStreamNnz = 2048;

// exclusive scan of one int per thread over the workgroup; *total = the sum
__device__ __forceinline__ int block_scan_int(int v, int *lds_waves, int *total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
    }
    __syncthreads();                       // lds_waves may still be read from the previous round
    if (lane == 63) lds_waves[wave] = inc;
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < kBlock / 64; w++) {
        const int t = lds_waves[w];
        if (w < wave) before += t;
        all += t;
    }
    *total = all;
    return before + inc - v;
}

// ------------------------------------------------------------------ the parts every SpMV-shaped kernel shares
// Prologue of a kernel that may evaluate the half-step test: true when the launch must return (the loop is frozen, or the
// test it evaluated here stopped it).  Kernels that never evaluate the test look at state alone and do not call this.
__device__ __forceinline__ bool spmv_enter(const SpmvArgs &a, double *lds)
{
    if (!a.loop.st) return false;
    if (a.check == CHECK_HALF) return check_half(a.loop, a.half, lds);
    return a.loop.st->state != 0;
}

// Work is dealt to workgroups XCD by XCD (workgroup b runs on XCD b & 7 when the grid is a multiple of 8): each XCD gets a
// contiguous eighth, so rows that share x entries (banded matrices) meet in one 4 MiB L2.
// Chunks -- one contiguous run of rows or tiles per workgroup: the chunk of workgroup b.
__device__ __forceinline__ int xcd_chunk(int b, int nb)
{
    return ((nb & 7) == 0) ? (b & 7) * (nb >> 3) + (b >> 3) : b;
}

// Tiles -- tiles_per_block of them per workgroup, dealt CYCLICALLY inside the XCD's contiguous share: the t-th tile of
// workgroup b.  At any moment the workgroups of one XCD sit on neighbouring tiles, so the three uses of an x entry by a
// stencil row (rows i - nx, i, i + nx) fall into the same few microseconds and hit the XCD's L2 instead of being re-fetched
// after 20 MB of streamed entries.
__device__ __forceinline__ long long xcd_tile(int b, int nb, int tiles_per_block, int t)
{
    const bool xcd_split = (nb & 7) == 0;
    const int wg_per_set = xcd_split ? nb >> 3 : nb;
    const int set = xcd_split ? (b & 7) : 0;
    const int w = xcd_split ? (b >> 3) : b;
    const long long set_tile0 = (long long)set * wg_per_set * tiles_per_block;
    return set_tile0 + (long long)t * wg_per_set + w;
}

// Row epilogue: y = alpha*(sum + d.*xd) + beta*y for one row, and the row's share of the fused dots (w.y, y.y).
// Two flavours, and a kernel's bits depend on which one it calls.  Both bodies sit under
// contract(off) -- the pragma is lexical, an inlined helper keeps the setting of the place it is written in, not its
// caller's -- so each says exactly what it computes:
//   fused: fma(d, xd, sum); fma(beta, y, alpha*sum); fma(out, w, acc0); fma(out, out, acc1)  -- spmv_csr.hip, k_spmm_csr
//   exact: one rounding per product and per sum (the CPU loop's)                           -- pattern and SELL forms
__device__ __forceinline__ void spmv_finish_row_fused(const SpmvArgs &a, int row, double sum, double (&acc)[2])
{
#pragma clang fp contract(off)
    if (a.d) sum = fma(a.d[row], a.xd[row], sum);
    double out = a.alpha * sum;
    if (a.beta != 0.0) out = fma(a.beta, a.y[row], out);
    a.y[row] = out;
    if (a.dot) {
        acc[0] = fma(out, a.w[row], acc[0]);
        acc[1] = fma(out, out, acc[1]);
    }
}

__device__ __forceinline__ void spmv_finish_row_exact(const SpmvArgs &a, int row, double sum, double (&acc)[2])
{
#pragma clang fp contract(off)
    if (a.d) sum += a.d[row] * a.xd[row];
    double out = a.alpha * sum;
    if (a.beta != 0.0) out += a.beta * a.y[row];
    a.y[row] = out;
    if (a.dot) {
        acc[0] += out * a.w[row];
        acc[1] += out * out;
    }
}

// The K-column form of the fused flavour (k_spmm_csr): column j does what spmv_finish_row_fused does, in the same order.
// S: per-column shifts a.dk in place of the shared a.d.
template <int K, bool S>
__device__ __forceinline__ void spmm_finish_row(const SpmmArgs &a, int row, const double (&sum)[K], double (&acc)[2 * K])
{
#pragma clang fp contract(off)
    double out[K], yo[K], xd[K], w[K], dk[K];
    if (a.beta != 0.0) load_row<K>(a.y, row, yo);
    if (S || a.d) load_row<K>(a.xd, row, xd);
    if (S) load_row<K>(a.dk, row, dk);
    if (a.dot) load_row<K>(a.w, row, w);
#pragma unroll
    for (int j = 0; j < K; j++) {
        double sj = sum[j];
        if (S) sj = fma(dk[j], xd[j], sj);
        else if (a.d) sj = fma(a.d[row], xd[j], sj);
        double o = a.alpha * sj;
        if (a.beta != 0.0) o = fma(a.beta, yo[j], o);
        out[j] = o;
        if (a.dot) {
            acc[2 * j] = fma(o, w[j], acc[2 * j]);
            acc[2 * j + 1] = fma(o, o, acc[2 * j + 1]);
        }
    }
    store_row<K>(a.y, row, out, kAll);
}

// the workgroup's two dot partials -> parts[2 * slot], parts[2 * slot + 1] (slot: the workgroup's place among the launch's)
__device__ __forceinline__ void spmv_store_dots(const SpmvArgs &a, int slot, double (&acc)[2], double *lds)
{
    if (!a.dot) return;
    block_sum<2>(acc, lds);
    if (threadIdx.x == 0) {
        a.parts[2 * slot] = acc[0];
        a.parts[2 * slot + 1] = acc[1];
    }
}

// Tail of a stream tile (rows r0 .. r0 + nr, products in prod, row i's at [srp[i] - base, srp[i + 1] - base)): thread i < nr
// adds its row's products in column order (the rounding sequence of the CPU loop) and finishes the row.
__device__ __forceinline__ void stream_finish_rows(const SpmvArgs &a, int r0, int nr, const int *srp, int base,
                                                   const double *prod, double (&acc)[2])
{
    const int tid = threadIdx.x;
    if (tid >= nr) return;
    double sum = 0.0;
    for (int j = srp[tid] - base; j < srp[tid + 1] - base; j++) sum += prod[j];
    spmv_finish_row_fused(a, r0 + tid, sum, acc);
}

// ---- streaming vector kernels: 16 bytes per lane (double2) whenever every operand is 16-byte aligned
template <int W> struct Width { static constexpr int value = W; };

// body(i, Width<W>): VEC = 1 runs it at W = 2 over the n / 2 pairs (i: the pair, load_row<2> / store_row<2> with kAll) and at
// W = 1 over the odd tail; VEC = 0 at W = 1 over every element.  Grid-stride, and the tail after the pairs: a thread's
// partial sums take the pairs in that order, .x before .y, then its tail element.
template <int VEC, class Body>
__device__ __forceinline__ void vec_loop(int64_t n, Body body)
{
    const int64_t n2 = VEC ? n / 2 : 0;
    const int64_t first = (int64_t)blockIdx.x * kBlock + threadIdx.x, stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = first; i < n2; i += stride) body(i, Width<2>{});
    for (int64_t i = 2 * n2 + first; i < n; i += stride) body(i, Width<1>{});
}

// vec_loop's dealing for both alignments.  VEC = 1 is vec_loop<1>.  VEC = 0 (an operand 8 bytes off a 16-byte boundary) keeps
// the pairs and visits their elements one by one, .x before .y, then the odd tail: a thread's partial sums take the same
// terms in the same order, so the bits of a solve do not depend on where the caller's vectors start.
template <int VEC, class Body>
__device__ __forceinline__ void pair_loop(int64_t n, Body body)
{
    if constexpr (VEC) {
        vec_loop<1>(n, body);
    } else {
        const int64_t n2 = n / 2;
        const int64_t first = (int64_t)blockIdx.x * kBlock + threadIdx.x, stride = (int64_t)gridDim.x * kBlock;
        for (int64_t i = first; i < n2; i += stride) {
            body(2 * i, Width<1>{});
            body(2 * i + 1, Width<1>{});
        }
        for (int64_t i = 2 * n2 + first; i < n; i += stride) body(i, Width<1>{});
    }
}

// a null pointer counts as aligned (an operand the launch does not use)
template <class... P>
static inline bool all_aligned16(const P *...p) { return (((((uintptr_t)p) & 15) == 0) && ...); }

// Launches KERNEL -- an expression in VEC, such as k_dot<VEC> -- on grid G of stream s with VEC = 1 when ALIGNED, else 0, and
// returns from the launcher.
#define CM_VEC_LAUNCH(ALIGNED, G, KERNEL, ...)                                                              \
    do {                                                                                                    \
        if (ALIGNED) { constexpr int VEC = 1; hipLaunchKernelGGL(KERNEL, dim3(G), dim3(kBlock), 0, s, __VA_ARGS__); } \
        else { constexpr int VEC = 0; hipLaunchKernelGGL(KERNEL, dim3(G), dim3(kBlock), 0, s, __VA_ARGS__); }         \
        CM_HIP(hipGetLastError());                                                                          \
        return CUDAMAT_OK;                                                                                  \
    } while (0)

}  // namespace cm
