// trsv.hip -- application of the ILU(0) factors: t = L^-1 y (unit diagonal), U^-1 t (cusparseDcsrsv_solve x4 per
// iteration, pbicgstab.cu:92-98,:121-127), for one vector (trsv_apply) and for K interleaved columns (trsm.h: the batched
// loop of loops_batch.hip, cudamat_solver_precond_apply_many).  The forms and when each is taken are described at the top
// of ilu.hip.
//
// The level-scheduled forms are ONE kernel family templated on the lanes per row and on the columns K in {1, 2, 4, 8}:
//   * k_trsm_level<LANES, K>         one launch per wide level
//   * k_trsm_small_levels<LANES, K>  a run of narrow levels in one workgroup (workgroup-scope fence + barrier per level)
//   * k_trsm_lds<LANES, K>           the whole solve in one workgroup with the n x K block in LDS, when n K 8 bytes fit the
//                                    128 KiB the single-column form asks for and the factor's levels are narrow (TriHost::lds)
// A single vector is the K = 1 instantiation, so column j of a K-column solve is bit-identical to the single-column solve
// of column j by construction: lane k of a row's team takes entries k, k + LANES, ..., every column keeps its own partial
// sum, the same xor tree per column, one rounding per operation, no atomics -- and the grid and the row partition depend on
// the factor only, never on K: a column's bits do not depend on the batch it sits in.  With the columns interleaved
// (V[i*K + j], batch.h) one gathered column index yields K contiguous doubles (dwordx4 loads for K >= 2), one level hop
// serves K columns, and the factor's indices and values (12 B per entry) are read once instead of K times.
// Every column of the block is computed (padding columns of a short batch too: plain arithmetic on whatever they hold, NaN
// or Inf included); the callers never copy a padding column back.
// One more template parameter, PV: the factor VALUES are per column too (fval[k*K + j], dinv[pr*K + j]: the ILU(0) of K shifted
// matrices on one pattern, ilu.hip) -- trsm_apply_cols / precond_apply_cols.  Indices, levels, grids and form choice are the
// solver's own; by the argument above column j is bit-identical to the K = 1 kernel on the factors of column j alone.
//
// Single-column only: the dependency-driven k_trsv_syncfree.  Its protocol publishes one 8-byte value per row; a K-wide row
// would be K publications read by 16-byte loads, which needs an argument about tearing that has not been made.  Also not
// covered by the multi-column path (trsm_covered; the callers then run column by column): hybrid factors in level-major
// spaces (TriFactor::lm -- their far parts are blocked SpMVs without a multi-column form), block-Jacobi ILU(0), sharded
// solvers.
#include <stdio.h>

#include <algorithm>
#include <type_traits>
#include <vector>

#include "batch.h"
#include "device.h"
#include "ilu.h"
#include "trsm.h"

using namespace cm;

namespace cm {

// ---------------------------------------------------------------- triangular solves
// out[o(pr)][j] = (rhs[i(pr)][j] - sum_k val[k] out[col[k]][j]) * dinv   for the permuted rows [r0, r1), K columns.
// Index spaces: a permuted row pr reads rhs at rhs_of[pr] and writes out at out_of[pr] (a nullptr map = pr itself);
// the stored columns are indices into `out`.  Factors in ORIGINAL index space have rhs_of = out_of = row_of; factors
// in LEVEL-MAJOR space (hybrid, TriFactor::lm) have out_of = nullptr -- the solve writes a contiguous stream -- and
// rhs_of = nullptr (L: the right-hand side is in L's space) or the U-position -> L-position map (U).
// LANES lanes per row, exactly the SpMV inner loop; rows of one level are independent.  far (K = 1 only: hybrid factors
// have no multi-column form) holds the entries whose column lies in an earlier group.
// PV ("per-column values", the factors of K shifted matrices on one pattern: cudamat_solver_solve_shifts_ilu0): fval and dinv
// hold K values per entry / row, interleaved like the vectors -- fval[k*K + j], dinv[pr*K + j] -- and column j takes its own:
// the same operations in the same order as the K = 1 kernel on the factors of column j alone, so the same bits.
template <int K, bool PV>
__device__ __forceinline__ void load_vals(const double *v, int64_t k, double (&a)[PV ? K : 1])
{
    if constexpr (PV) load_row<K>(v, k, a);
    else a[0] = v[k];
}

template <int LANES, int K, bool PV = false>
__device__ __forceinline__ void tri_rows(int r0, int r1, int first, int stride, const int *frp, const int *fci,
                                         const double *fval, const int *rhs_of, const int *out_of, const double *dinv,
                                         const double *far, const double *rhs, double *out)
{
    const int lane = threadIdx.x & (LANES - 1);
    for (int pr = r0 + first; pr < r1; pr += stride) {
        const int s = frp[pr], e = frp[pr + 1];
        double sum[K];
#pragma unroll
        for (int j = 0; j < K; j++) sum[j] = 0.0;
        for (int k = s + lane; k < e; k += LANES) {
            double a[PV ? K : 1];
            load_vals<K, PV>(fval, k, a);
            double xv[K];
            load_row<K>(out, fci[k], xv);
#pragma unroll
            for (int j = 0; j < K; j++) sum[j] += a[PV ? j : 0] * xv[j];
        }
#pragma unroll
        for (int j = 0; j < K; j++) sum[j] = group_sum<LANES>(sum[j]);
        if (lane == 0) {
            double v[K];
            load_row<K>(rhs, rhs_of ? rhs_of[pr] : pr, v);
            double di[PV ? K : 1];
            if (dinv) load_vals<K, PV>(dinv, pr, di);
#pragma unroll
            for (int j = 0; j < K; j++) {
                v[j] = v[j] - sum[j];
                if constexpr (K == 1) {
                    if (far) v[j] -= far[pr];
                }
                if (dinv) v[j] *= di[PV ? j : 0];
            }
            store_row<K>(out, out_of ? out_of[pr] : pr, v, kAll);
        }
    }
}

template <int LANES, int K, bool PV = false>
__global__ __launch_bounds__(kBlock) void k_trsm_level(int r0, int r1, const int *frp, const int *fci, const double *fval,
                                                       const int *rhs_of, const int *out_of, const double *dinv,
                                                       const double *far, const double *rhs, double *out)
{
    constexpr int RPB = kBlock / LANES;
    tri_rows<LANES, K, PV>(r0, r1, blockIdx.x * RPB + threadIdx.x / LANES, gridDim.x * RPB, frp, fci, fval, rhs_of, out_of,
                           dinv, far, rhs, out);
}

// several consecutive small levels in ONE workgroup: a workgroup-scope fence + barrier publishes a
// level's results (same CU, same L1) to the threads that consume them in the next level.
template <int LANES, int K, bool PV = false>
__global__ __launch_bounds__(kBlock) void k_trsm_small_levels(int l0, int l1, const int *level_ptr, const int *frp,
                                                              const int *fci, const double *fval, const int *rhs_of,
                                                              const int *out_of, const double *dinv, const double *far,
                                                              const double *rhs, double *out)
{
    constexpr int RPB = kBlock / LANES;
    for (int l = l0; l < l1; l++) {
        tri_rows<LANES, K, PV>(level_ptr[l], level_ptr[l + 1], threadIdx.x / LANES, RPB, frp, fci, fval, rhs_of, out_of, dinv,
                               far, rhs, out);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __syncthreads();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    }
}

// ---- dependency-driven ("sync-free") solve of a whole group of levels in ONE launch
// Rows are stored level-major, so every dependency of permuted row pr sits at a smaller pr.  Workgroups CLAIM
// chunks of consecutive rows from an atomic ticket, so chunk t is only ever held by a workgroup that is already
// running, and it is claimed after every chunk < t: a waiting row waits for rows of its own wave or of chunks
// held by resident workgroups, and the lowest unfinished chunk never waits for anything unclaimed -- forward
// progress does not depend on the order or the number of workgroups the dispatcher starts (the grid may be
// smaller or larger than what fits; other kernels may hold part of the GPU).  A workgroup fetches its next
// ticket while it works on the current one (the atomic's round trip is off the chain); holding a ticket early is
// harmless: its owner is resident and working on a lower chunk.  Readiness travels with
// the data: `out` is pre-filled with a SIGNALLING-NaN bit pattern that no arithmetic result can have (every
// operation quiets a signalling NaN), a producer publishes its value with one 8-byte write-through (sc1)
// store and consumers poll the value itself with 8-byte sc1 loads -- no flags, no fences (one naturally
// aligned 8-byte granule written by one store).  Each row is still summed by its own LANES lanes in the
// level kernel's order, so the result is bit-identical to the level-by-level solve.
// Every spin is still bounded (defence in depth): a lane that gives up sets *err (pinned host word) and proceeds
// with what it read; cudamat_solver_solve then redoes the solve level by level and counts it (trsv_fallbacks).
constexpr unsigned long long kNotReady = 0x7FF4C0DEC0DEC0DEull;

__global__ __launch_bounds__(kBlock) void k_fill_not_ready(long long n, unsigned long long *out)
{
    for (long long i = blockIdx.x * (long long)kBlock + threadIdx.x; i < n; i += (long long)gridDim.x * kBlock)
        out[i] = kNotReady;
}

template <int LANES, int BLOCK>
__global__ __launch_bounds__(BLOCK) void k_trsv_syncfree(int r0, int r1, const int *frp, const int *fci,
                                                          const double *fval, const int *rhs_of, const int *out_of,
                                                          const double *dinv, const double *far,
                                                          const double *rhs, double *out, int *err, int spin_limit,
                                                          int nap, unsigned *ticket, int steps)
{
    typedef __attribute__((address_space(1))) unsigned long long gu64;
    constexpr int RPB = BLOCK / LANES;
    const int lane = threadIdx.x & (LANES - 1);
    const int team_shift = (threadIdx.x & 63) & ~(LANES - 1);
    constexpr unsigned long long team_bits = LANES == 64 ? ~0ull : ((1ull << LANES) - 1ull);
    __shared__ unsigned s_ticket[2];
    const long long nsub = ((long long)(r1 - r0) + RPB - 1) / RPB;       // sub-chunks of RPB rows
    if (threadIdx.x == 0) s_ticket[0] = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  for (int turn = 0;; turn ^= 1) {
    __syncthreads();                                   // this turn's ticket is in LDS (the slots alternate)
    const long long first = (long long)s_ticket[turn] * steps;
    if (first >= nsub) return;
    unsigned next_ticket = 0;                          // in flight while this chunk is solved, stored at its end
    if (threadIdx.x == 0) next_ticket = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
   for (int step = 0; step < steps && first + step < nsub; step++) {
    const long long prl = (long long)r0 + (first + step) * RPB + threadIdx.x / LANES;
    const bool valid = prl < r1;
    const int pr = valid ? (int)prl : r0;
    int k = 0, e = 0;
    if (valid) {
        k = frp[pr] + lane;
        e = frp[pr + 1];
    }
    bool have = k < e;
    int c = 0;
    double a = 0.0;
    if (have) {
        c = fci[k];
        a = fval[k];
    }
    // everything the row's last step needs is fetched up front: only the polled values are on the chain
    int r = 0;
    double base = 0.0, fr = 0.0, di = 1.0;
    if (valid && lane == 0) {
        r = out_of ? out_of[pr] : pr;
        base = rhs[rhs_of ? rhs_of[pr] : pr];
        if (far) fr = far[pr];
        if (dinv) di = dinv[pr];
    }
    double sum = 0.0;
    bool done = !valid;
    int spins = 0;
    for (;;) {
        if (have) {
            const unsigned long long bits = __hip_atomic_load((gu64 *)(out + c), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const bool ready = bits != kNotReady;
            // give up after kSpinLimit polls -- or at once when another row already has (checked every 1024 polls),
            // so that a broken dependency costs one timeout, not one per waiting row
            bool give_up = false;
            if (!ready && (++spins & 1023) == 0)
                give_up = spins > spin_limit || __hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0;
            if (ready || give_up) {
                if (!ready) __hip_atomic_store(err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                sum += a * __longlong_as_double((long long)bits);
                spins = 0;
                k += LANES;
                have = k < e;
                if (have) {
                    c = fci[k];
                    a = fval[k];
                }
            }
        }
        const unsigned long long pending = __ballot(have);
        if (!done && ((pending >> team_shift) & team_bits) == 0) {      // uniform over the row's lanes
            double tot = sum;
#pragma unroll
            for (int o = LANES / 2; o > 0; o >>= 1) tot += __shfl_xor(tot, o, 64);
            if (lane == 0) {
                double v = base - tot;
                if (far) v -= fr;
                if (dinv) v *= di;
                __hip_atomic_store((gu64 *)(out + r), (unsigned long long)__double_as_longlong(v), __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
            }
            done = true;
        }
        if (__ballot(!done) == 0) break;
        if (pending) {
            if (nap == 1) __builtin_amdgcn_s_sleep(1);
            else if (nap == 2) __builtin_amdgcn_s_sleep(2);
            else if (nap >= 4) {
                for (int q = 0; q < nap; q += 4) __builtin_amdgcn_s_sleep(8);      // nap/4 x 512 cycles
            }
        }
    }
   }   // steps of one ticket
    if (threadIdx.x == 0) s_ticket[turn ^ 1] = next_ticket;
  }    // tickets
}

// ---- small systems (n K <= 16384): the whole solve in ONE workgroup with the n x K block in LDS
// The level-by-level chain is then LDS read -> multiply-add -> shuffle -> LDS write -> barrier (~0.15 us per level):
// each team's row of the NEXT level (row pointers, first entries, right-hand sides, 1/diagonal) is fetched from
// global memory before the barrier, so nothing but LDS sits between two levels (mat10000: 199 levels per factor).
// Same per-row summation as tri_rows (lane k takes entries k, k + LANES, ...; xor tree per column) => bit-identical.
// Factors in the original index space only (row_of): a hybrid factor never takes this form.
template <int LANES, int K, bool PV = false>
__global__ __launch_bounds__(kBlock) void k_trsm_lds(int n, int nlev, const int *level_ptr, const int *frp, const int *fci,
                                                     const double *fval, const int *row_of, const double *dinv,
                                                     const double *rhs, double *out)
{
    extern __shared__ __attribute__((aligned(16))) double xs[];       // n x K doubles, original row numbering
    constexpr int RPB = kBlock / LANES;
    const int lane = threadIdx.x & (LANES - 1), team = threadIdx.x / LANES;
    constexpr int KV = PV ? K : 1;                                     // values per entry / row: one shared, or one per column
    int pr = 0, s = 0, e = 0, r = 0, c = 0;
    double a[KV], di[KV];
#pragma unroll
    for (int j = 0; j < KV; j++) {
        a[j] = 0.0;
        di[j] = 1.0;
    }
    double b[K];
#pragma unroll
    for (int j = 0; j < K; j++) b[j] = 0.0;
    bool mine = false;
    auto fetch = [&](int l) {
        mine = false;
        if (l >= nlev) return;
        pr = level_ptr[l] + team;
        mine = pr < level_ptr[l + 1];
        if (!mine) return;
        s = frp[pr];
        e = frp[pr + 1];
        if (s + lane < e) {
            c = fci[s + lane];
            load_vals<K, PV>(fval, s + lane, a);
        }
        if (lane == 0) {
            r = row_of[pr];
            load_row<K>(rhs, r, b);
            if (dinv) load_vals<K, PV>(dinv, pr, di);
        }
    };
    fetch(0);
    for (int l = 0; l < nlev; l++) {
        const int lend = level_ptr[l + 1];
        const bool have = mine;
        const int pr0 = pr, s0 = s, e0 = e, r0 = r;
        double di0[KV];
#pragma unroll
        for (int j = 0; j < KV; j++) di0[j] = di[j];
        double b0[K], sum[K];
#pragma unroll
        for (int j = 0; j < K; j++) {
            b0[j] = b[j];
            sum[j] = 0.0;
        }
        if (have) {
            if (s0 + lane < e0) {
                double xv[K];
                load_row<K>(xs, c, xv);
#pragma unroll
                for (int j = 0; j < K; j++) sum[j] = a[PV ? j : 0] * xv[j];
            }
            for (int k = s0 + lane + LANES; k < e0; k += LANES) {
                double av[KV];
                load_vals<K, PV>(fval, k, av);
                double xv[K];
                load_row<K>(xs, fci[k], xv);
#pragma unroll
                for (int j = 0; j < K; j++) sum[j] += av[PV ? j : 0] * xv[j];
            }
        }
#pragma unroll
        for (int j = 0; j < K; j++) sum[j] = group_sum<LANES>(sum[j]);
        if (have && lane == 0) {
            double v[K];
#pragma unroll
            for (int j = 0; j < K; j++) {
                v[j] = b0[j] - sum[j];
                if (dinv) v[j] *= di0[PV ? j : 0];
            }
            store_row<K>(xs, r0, v, kAll);
            store_row<K>(out, r0, v, kAll);
        }
        // further rows of a level wider than the workgroup's teams
        for (int q = pr0 + RPB; have && q < lend; q += RPB) {
            const int qs = frp[q], qe = frp[q + 1];
            double t[K];
#pragma unroll
            for (int j = 0; j < K; j++) t[j] = 0.0;
            for (int k = qs + lane; k < qe; k += LANES) {
                double av[KV];
                load_vals<K, PV>(fval, k, av);
                double xv[K];
                load_row<K>(xs, fci[k], xv);
#pragma unroll
                for (int j = 0; j < K; j++) t[j] += av[PV ? j : 0] * xv[j];
            }
#pragma unroll
            for (int j = 0; j < K; j++) t[j] = group_sum<LANES>(t[j]);
            if (lane == 0) {
                const int rr = row_of[q];
                double v[K];
                load_row<K>(rhs, rr, v);
                double dq[KV];
                if (dinv) load_vals<K, PV>(dinv, q, dq);
#pragma unroll
                for (int j = 0; j < K; j++) {
                    v[j] = v[j] - t[j];
                    if (dinv) v[j] *= dq[PV ? j : 0];
                }
                store_row<K>(xs, rr, v, kAll);
                store_row<K>(out, rr, v, kAll);
            }
        }
        fetch(l + 1);                      // global loads of the next level overlap the barrier
        __syncthreads();
    }
}

// the far SpMV of one group: far_buf[rows of the group] = far_g . out
static int launch_far(hipStream_t st, const TriFactor &F, const TriHost &H, int grp, const double *out)
{
    const int r0 = F.level_ptr[(size_t)H.grp_level[(size_t)grp]];
    SpmvArgs a{};
    a.n = H.far[(size_t)grp].n;
    a.x = out;
    a.alpha = 1.0;
    a.beta = 0.0;
    a.y = H.far_buf + r0;
    a.dot = 0;
    a.loop = LoopArgs{nullptr, nullptr, 0, 0, 0};
    a.check = CHECK_NONE;
    a.half = ScalarSrc{nullptr, 0, 1};
    a.pb_strict = H.pb_strict;
    return launch_spmv_pb(st, H.far[(size_t)grp], a);
}

// f(std::integral_constant<int, LANES>()) for the lanes per row of a factor's plan: the one place where TriHost::lanes
// becomes a template argument
template <class Fn>
static int with_lanes(int lanes, Fn &&f)
{
    switch (lanes) {
    case 2:  return f(std::integral_constant<int, 2>());
    case 4:  return f(std::integral_constant<int, 4>());
    case 8:  return f(std::integral_constant<int, 8>());
    case 16: return f(std::integral_constant<int, 16>());
    case 32: return f(std::integral_constant<int, 32>());
    default: return f(std::integral_constant<int, 64>());
    }
}

// the same for the columns of a batch
template <class Fn>
static int with_cols(int K, Fn &&f)
{
    switch (K) {
    case 1: return f(std::integral_constant<int, 1>());
    case 2: return f(std::integral_constant<int, 2>());
    case 4: return f(std::integral_constant<int, 4>());
    case 8: return f(std::integral_constant<int, 8>());
    }
    set_error("triangular solve: %d columns per batch", K);
    return CUDAMAT_ERR_ARG;
}

// the level-by-level launch plan (TriHost::seg_begin / seg_end): a wide level is its own launch, a run of narrow levels
// one single-workgroup launch.  The grids depend on the factor only.  A hybrid factor (K = 1 only, trsm_covered) gets one
// blocked SpMV per group for its far entries.
// val / dinv: the factor's own (F.val, F.dinv), or with PV the K-wide values of a block of shifted factors on F's pattern.
template <int LANES, int K, bool PV = false>
static int launch_level_segments(hipStream_t st, const TriFactor &F, const TriHost &H, const double *val, const double *dinv,
                                 const double *rhs, double *out)
{
    constexpr int RPB = kBlock / LANES;
    int cur_group = -1;
    for (size_t g = 0; g < H.seg_begin.size(); g++) {
        const int grp = H.seg_group.empty() ? 0 : H.seg_group[g];
        const double *far = nullptr;
        if (H.hybrid && grp > 0 && H.far[(size_t)grp].nnz > 0) {
            if (grp != cur_group) CM_TRY(launch_far(st, F, H, grp, out));
            far = H.far_buf;
        }
        cur_group = grp;
        const int l0 = H.seg_begin[g], l1 = H.seg_end[g];
        const int r0 = F.level_ptr[(size_t)l0], r1 = F.level_ptr[(size_t)l1];
        if (segment_is_wide(F, H, g)) {
            hipLaunchKernelGGL((k_trsm_level<LANES, K, PV>), dim3(row_grid(r1 - r0, RPB)), dim3(kBlock), 0, st, r0, r1, F.rp, F.ci,
                               val, F.rhs_of, F.out_of, dinv, far, rhs, out);
        } else {
            hipLaunchKernelGGL((k_trsm_small_levels<LANES, K, PV>), dim3(1), dim3(kBlock), 0, st, l0, l1, H.level_ptr_dev, F.rp,
                               F.ci, val, F.rhs_of, F.out_of, dinv, far, rhs, out);
        }
    }
    return CUDAMAT_OK;
}

template <int LANES, int K, bool PV = false>
static int launch_lds(cudamat_solver *s, const TriFactor &F, const TriHost &H, const double *val, const double *dinv,
                      const double *rhs, double *out)
{
    const size_t bytes = sizeof(double) * (size_t)s->n * (size_t)K;
    CM_TRY(set_max_lds((const void *)k_trsm_lds<LANES, K, PV>));
    hipLaunchKernelGGL((k_trsm_lds<LANES, K, PV>), dim3(1), dim3(kBlock), bytes, s->ctx->stream, s->n, F.nlevels, H.level_ptr_dev,
                       F.rp, F.ci, val, F.row_of, dinv, rhs, out);
    return CUDAMAT_OK;
}

template <int LANES, int BLOCK>
static int launch_trsv_syncfree_b(hipStream_t st, const TriFactor &F, const TriHost &H, int n, const double *rhs,
                                  double *out, int *err, int per_cu)
{
    constexpr int RPB = BLOCK / LANES;
    int fill_grid = (int)(((long long)n + kBlock - 1) / kBlock);
    if (fill_grid > kVecGridMax) fill_grid = kVecGridMax;
    hipLaunchKernelGGL(k_fill_not_ready, dim3(fill_grid ? fill_grid : 1), dim3(kBlock), 0, st, (long long)n,
                       (unsigned long long *)out);
    const int K = (int)H.grp_level.size() - 1;
    CM_HIP(hipMemsetAsync(H.tickets, 0, sizeof(unsigned) * (size_t)(K > 0 ? K : 1), st));     // one ticket counter per launch
    for (int g = 0; g < K; g++) {
        const int r0 = F.level_ptr[(size_t)H.grp_level[(size_t)g]], r1 = F.level_ptr[(size_t)H.grp_level[(size_t)g + 1]];
        if (r1 <= r0) continue;
        const double *far = nullptr;
        if (H.hybrid && g > 0 && H.far[(size_t)g].nnz > 0) {
            CM_TRY(launch_far(st, F, H, g, out));
            far = H.far_buf;
        }
        // A ticket = `steps` consecutive sub-chunks of RPB rows: at least 256 rows, so that the one counter sees an
        // atomic per 256 rows at most (far below what one address sustains).  The rows in flight are
        // (resident workgroups) x (rows per ticket): kept as narrow as a level or two, because a row far ahead of the
        // lowest unfinished one would mostly wait -- hence big workgroups (BLOCK = 256 x occ threads, one per CU)
        // rather than many small ones.
        const long long nsub = ((long long)(r1 - r0) + RPB - 1) / RPB;
        int steps = 256 / RPB > 0 ? 256 / RPB : 1;
        while (steps > 1 && nsub / steps < 1024) steps >>= 1;
        const long long ntick = (nsub + steps - 1) / steps;
        // no more workgroups than can be resident; more would only queue behind the persistent ones
        const long long cap = (long long)per_cu * 256;
        const unsigned grid = (unsigned)(ntick < cap ? ntick : cap);
        // residency is pinned with an (unused) dynamic LDS request: fewer waiting workgroups, fewer pollers
        const size_t lds_pad = (size_t)(152 * 1024) / (size_t)per_cu;
        CM_TRY(set_max_lds((const void *)k_trsv_syncfree<LANES, BLOCK>));
        hipLaunchKernelGGL((k_trsv_syncfree<LANES, BLOCK>), dim3(grid), dim3(BLOCK), lds_pad, st, r0, r1, F.rp, F.ci, F.val,
                           F.rhs_of, F.out_of, F.dinv, far, rhs, out, err, H.spin_limit, H.nap, H.tickets + g, steps);
    }
    return CUDAMAT_OK;
}

// occ = resident waves per CU / 4 (1, 2, 4, 8): one workgroup of 256 x occ threads per CU (two of 1024 at occ = 8)
template <int LANES>
static int launch_trsv_syncfree(hipStream_t st, const TriFactor &F, const TriHost &H, int n, const double *rhs,
                                double *out, int *err)
{
    const int occ = H.occ >= 8 ? 8 : H.occ >= 4 ? 4 : H.occ >= 2 ? 2 : 1;
    if (occ == 1) return launch_trsv_syncfree_b<LANES, 256>(st, F, H, n, rhs, out, err, 1);
    if (occ == 2) return launch_trsv_syncfree_b<LANES, 512>(st, F, H, n, rhs, out, err, 1);
    return launch_trsv_syncfree_b<LANES, 1024>(st, F, H, n, rhs, out, err, occ == 8 ? 2 : 1);
}

bool trsv_syncfree_active(cudamat_solver *s)
{
    IluPlans *pl = plans_of(s, false);
    return pl && s->has_ilu && (pl->L.syncfree || pl->U.syncfree);
}

int trsv_form_code(cudamat_solver *s)
{
    IluPlans *pl = plans_of(s, false);
    if (!pl || !s->has_ilu) return 0;
    if (pl->L.syncfree || pl->U.syncfree) return 1;
    if (pl->L.lds || pl->U.lds) return 2;
    return 0;
}

void trsv_group_counts(cudamat_solver *s, int *groups_l, int *groups_u)
{
    *groups_l = *groups_u = 0;
    IluPlans *pl = plans_of(s, false);
    if (!pl || !s->has_ilu) return;
    if (pl->L.hybrid) *groups_l = (int)pl->L.grp_level.size() - 1;
    if (pl->U.hybrid) *groups_u = (int)pl->U.grp_level.size() - 1;
}

void trsv_disable_syncfree(cudamat_solver *s)
{
    if (IluPlans *pl = plans_of(s, false)) pl->L.syncfree = pl->U.syncfree = false;
}

int trsv_status(cudamat_solver *s)
{
    IluPlans *pl = plans_of(s, false);
    if (pl && pl->err_host && *pl->err_host) {
        *pl->err_host = 0;
        set_error("triangular solve: a dependency never became ready (spin limit reached)");
        return CUDAMAT_ERR_HIP;
    }
    return CUDAMAT_OK;
}

int trsv_apply(cudamat_solver *s, const TriFactor &F, bool upper, const double *rhs, double *out)
{
    IluPlans *pl = plans_of(s, false);
    if (!pl || !s->has_ilu) { set_error("ILU(0) factors missing"); return CUDAMAT_ERR_ARG; }
    const TriHost &H = upper ? pl->U : pl->L;
    if (H.syncfree && rhs == out) { set_error("triangular solve: rhs and out must not alias"); return CUDAMAT_ERR_ARG; }
    CM_TRY(with_lanes(H.lanes, [&](auto lanes) {
        constexpr int LANES = decltype(lanes)::value;
        if (H.lds && !H.syncfree) return launch_lds<LANES, 1>(s, F, H, F.val, F.dinv, rhs, out);
        if (H.syncfree) return launch_trsv_syncfree<LANES>(s->ctx->stream, F, H, s->n, rhs, out, pl->err_dev);
        return launch_level_segments<LANES, 1>(s->ctx->stream, F, H, F.val, F.dinv, rhs, out);
    }));
    CM_HIP(hipGetLastError());
    return CUDAMAT_OK;
}

// ---- vectors between the original row numbering and the level-major spaces
__global__ __launch_bounds__(kBlock) void k_perm_gather(long long n, const int *map, const double *in, double *out)
{
    for (long long i = blockIdx.x * (long long)kBlock + threadIdx.x; i < n; i += (long long)gridDim.x * kBlock) out[i] = in[map[i]];
}
__global__ __launch_bounds__(kBlock) void k_perm_scatter(long long n, const int *map, const double *in, double *out)
{
    for (long long i = blockIdx.x * (long long)kBlock + threadIdx.x; i < n; i += (long long)gridDim.x * kBlock) out[map[i]] = in[i];
}

// out[pr] = in[row at position pr of L's (upper: U's) level-major order]
int perm_to_space(cudamat_solver *s, bool upper, const double *in, double *out)
{
    const TriFactor &F = upper ? s->U : s->L;
    hipLaunchKernelGGL(k_perm_gather, dim3(row_grid(s->n)), dim3(kBlock), 0, s->ctx->stream, (long long)s->n, F.row_of, in, out);
    CM_HIP(hipGetLastError());
    return CUDAMAT_OK;
}

// out[row at position pr] = in[pr]
int perm_from_space(cudamat_solver *s, bool upper, const double *in, double *out)
{
    const TriFactor &F = upper ? s->U : s->L;
    hipLaunchKernelGGL(k_perm_scatter, dim3(row_grid(s->n)), dim3(kBlock), 0, s->ctx->stream, (long long)s->n, F.row_of, in, out);
    CM_HIP(hipGetLastError());
    return CUDAMAT_OK;
}

// M^-1 on vectors in ORIGINAL numbering while the factors live in level-major spaces: permute in, solve, permute out
int precond_apply_original(cudamat_solver *s, const double *in, double *tmp, double *out)
{
    IluPlans *pl = plans_of(s, false);
    if (!pl || !pl->perm_a || !pl->perm_b) { set_error("level-major scratch vectors missing"); return CUDAMAT_ERR_ARG; }
    CM_TRY(perm_to_space(s, false, in, pl->perm_a));
    CM_TRY(trsv_apply(s, s->L, false, pl->perm_a, tmp));
    CM_TRY(trsv_apply(s, s->U, true, tmp, pl->perm_b));
    return perm_from_space(s, true, pl->perm_b, out);
}

// ---- K interleaved columns (trsm.h)
// the single-workgroup form: the factor's levels are narrow (TriHost::lds, decided at set-up for the single-column form) and
// the K-column block fits the LDS that form asks for
static bool takes_lds(const cudamat_solver *s, const TriHost &H, int K)
{
    return H.lds && (size_t)s->n * (size_t)K <= (size_t)kLdsTrsvRows;
}

bool trsm_covered(cudamat_solver *s)
{
    IluPlans *pl = plans_of(s, false);
    return pl && s->has_ilu && !s->ilu_block && !s->sharded && !s->L.lm && !s->U.lm && !pl->L.hybrid && !pl->U.hybrid &&
           s->n_cols == s->n && s->n > 0;
}

int trsm_form_code(cudamat_solver *s, bool upper, int K)
{
    IluPlans *pl = plans_of(s, false);
    if (!pl || !s->has_ilu) return 0;
    return takes_lds(s, upper ? pl->U : pl->L, K) ? 2 : 0;
}

int trsm_apply(cudamat_solver *s, const TriFactor &F, bool upper, int K, const double *rhs, double *out)
{
    IluPlans *pl = plans_of(s, false);
    if (!pl || !trsm_covered(s)) { set_error("ILU(0) factors missing or not covered by the multi-column solves"); return CUDAMAT_ERR_ARG; }
    if (rhs == out) { set_error("triangular solve: rhs and out must not alias"); return CUDAMAT_ERR_ARG; }
    const TriHost &H = upper ? pl->U : pl->L;
    CM_TRY(with_lanes(H.lanes, [&](auto lanes) {
        return with_cols(K, [&](auto cols) {
            constexpr int LANES = decltype(lanes)::value, KC = decltype(cols)::value;
            if (takes_lds(s, H, KC)) return launch_lds<LANES, KC>(s, F, H, F.val, F.dinv, rhs, out);
            return launch_level_segments<LANES, KC>(s->ctx->stream, F, H, F.val, F.dinv, rhs, out);
        });
    }));
    CM_HIP(hipGetLastError());
    return CUDAMAT_OK;
}

int precond_apply_b(cudamat_solver *s, int K, const double *in, double *tmp, double *out)
{
    CM_TRY(trsm_apply(s, s->L, false, K, in, tmp));     // pbicgstab.cu:92-94 / :121-123
    CM_TRY(trsm_apply(s, s->U, true, K, tmp, out));     // pbicgstab.cu:96-98 / :125-127
    return CUDAMAT_OK;
}

// ---- K columns, each with the values of its own factors (PV): the solver's pattern, levels, launch plan and form choice --
// the same grids as trsm_apply, so column j runs the very schedule of the single-column solve on the factors of column j
int trsm_apply_cols(cudamat_solver *s, bool upper, int K, const double *val_b, const double *dinv_b, const double *rhs, double *out)
{
    IluPlans *pl = plans_of(s, false);
    if (!pl || !trsm_covered(s)) { set_error("ILU(0) structure missing or not covered by the multi-column solves"); return CUDAMAT_ERR_ARG; }
    if (rhs == out) { set_error("triangular solve: rhs and out must not alias"); return CUDAMAT_ERR_ARG; }
    const TriHost &H = upper ? pl->U : pl->L;
    const TriFactor &F = upper ? s->U : s->L;
    CM_TRY(with_lanes(H.lanes, [&](auto lanes) {
        return with_cols(K, [&](auto cols) {
            constexpr int LANES = decltype(lanes)::value, KC = decltype(cols)::value;
            if (takes_lds(s, H, KC)) return launch_lds<LANES, KC, true>(s, F, H, val_b, dinv_b, rhs, out);
            return launch_level_segments<LANES, KC, true>(s->ctx->stream, F, H, val_b, dinv_b, rhs, out);
        });
    }));
    CM_HIP(hipGetLastError());
    return CUDAMAT_OK;
}

int precond_apply_cols(cudamat_solver *s, int K, const ColFactors &f, const double *in, double *tmp, double *out)
{
    CM_TRY(trsm_apply_cols(s, false, K, f.lval, nullptr, in, tmp));
    CM_TRY(trsm_apply_cols(s, true, K, f.uval, f.dinv, tmp, out));
    return CUDAMAT_OK;
}

}  // namespace cm

// the kernels a multi-column application of the factors launches, as a kernel trace shows them
extern "C" int cudamat_solver_trsm_kernel(cudamat_solver *s, int nrhs, char *name, int cap)
{
    CM_ARG(s && name && cap > 0, "null pointer");
    CM_ARG(nrhs >= 1, "nrhs < 1");
    CM_ARG(s->has_ilu, "call cudamat_solver_ilu0 first");
    name[0] = 0;
    if (!trsm_covered(s)) return CUDAMAT_OK;          // "": the factors run column by column (trsv_apply)
    IluPlans *pl = plans_of(s, false);
    const int K = pow2_cols(nrhs);
    int used = 0;
    for (int u = 0; u < 2 && used < cap; u++) {
        const TriHost &H = u ? pl->U : pl->L;
        const TriFactor &F = u ? s->U : s->L;
        used += snprintf(name + used, (size_t)(cap - used), "%s", u ? "; U: " : "L: ");
        if (used >= cap) break;
        if (takes_lds(s, H, K)) {
            used += snprintf(name + used, (size_t)(cap - used), "k_trsm_lds<%d, %d>", H.lanes, K);
            continue;
        }
        bool big = false, small = false;
        for (size_t g = 0; g < H.seg_begin.size(); g++) {
            const bool b = segment_is_wide(F, H, g);
            big = big || b;
            small = small || !b;
        }
        if (big) used += snprintf(name + used, (size_t)(cap - used), "k_trsm_level<%d, %d>", H.lanes, K);
        if (big && small && used < cap) used += snprintf(name + used, (size_t)(cap - used), " + ");
        if (small && used < cap) used += snprintf(name + used, (size_t)(cap - used), "k_trsm_small_levels<%d, %d>", H.lanes, K);
    }
    return CUDAMAT_OK;
}