// trsm.hip -- the ILU(0) factors applied to several right-hand sides at once: T = L^-1 Y (unit diagonal), U^-1 T for K
// interleaved columns (trsm.h), the triangular solves of the preconditioned batched loop (loops_batch.hip) and of
// cudamat_solver_precond_apply_many.
//
// A triangular solve is bound by dependent hops and by one gather per entry, not by bytes.  With the columns
// interleaved (V[i*K + j], batch.h) one gathered column index yields K contiguous doubles (dwordx4 loads for K >= 2), one level
// hop serves K columns, and the factor's indices and values (12 B per entry) are read once instead of K times.
//
// Three level-scheduled forms on the TriFactor storage (level-major rows, original index space), the multi-column
// counterparts of trsv.hip's:
//   * k_trsm_level<LANES, K>         one launch per wide level
//   * k_trsm_small_levels<LANES, K>  a run of narrow levels in one workgroup (workgroup-scope fence + barrier per level)
//   * k_trsm_lds<LANES, K>           the whole solve in one workgroup with the n x K block in LDS, when n K 8 bytes fit the
//                                    128 KiB the single-column form asks for and the factor's levels are narrow (TriHost::lds)
// CONTRACT: column j is bit-identical to trsv_apply on column j -- lane k of a row's team takes entries k, k + LANES, ...,
// every column keeps its own partial sum, the same xor tree per column, one rounding per operation, no atomics -- and the
// grid and the row partition depend on the factor only, never on K: a column's bits do not depend on the batch it sits in.
// Every column of the block is computed (padding columns of a short batch too: plain arithmetic on whatever they hold, NaN
// or Inf included); the callers never copy a padding column back.
//
// NOT here, on purpose: a dependency-driven (k_trsv_syncfree-style) multi-column kernel.  Its protocol publishes one 8-byte
// value per row; a K-wide row would be K publications read by 16-byte loads, which needs an argument about tearing that has
// not been made.  The level-scheduled forms cannot hang.  Also not covered (trsm_covered; the callers then run column by
// column): hybrid factors in level-major spaces (TriFactor::lm -- their far parts are blocked SpMVs without a multi-column
// form), block-Jacobi ILU(0), sharded solvers.
#include <stdio.h>

#include "batch.h"
#include "device.h"
#include "ilu.h"
#include "trsm.h"

using namespace cm;

namespace cm {

// out[row_of[pr]][j] = (rhs[row_of[pr]][j] - sum_k val[k] out[col[k]][j]) * dinv[pr]   for the permuted rows [r0, r1):
// trsv_rows<LANES> (trsv.hip) with K partial sums per lane
template <int LANES, int K>
__device__ __forceinline__ void trsm_rows(int r0, int r1, int first, int stride, const int *frp, const int *fci,
                                          const double *fval, const int *row_of, const double *dinv, const double *rhs,
                                          double *out)
{
    const int lane = threadIdx.x & (LANES - 1);
    for (int pr = r0 + first; pr < r1; pr += stride) {
        const int s = frp[pr], e = frp[pr + 1];
        double sum[K];
#pragma unroll
        for (int j = 0; j < K; j++) sum[j] = 0.0;
        for (int k = s + lane; k < e; k += LANES) {
            const double a = fval[k];
            double xv[K];
            load_row<K>(out, fci[k], xv);
#pragma unroll
            for (int j = 0; j < K; j++) sum[j] += a * xv[j];
        }
#pragma unroll
        for (int j = 0; j < K; j++) sum[j] = group_sum<LANES>(sum[j]);
        if (lane == 0) {
            const int r = row_of[pr];
            double v[K];
            load_row<K>(rhs, r, v);
#pragma unroll
            for (int j = 0; j < K; j++) {
                v[j] = v[j] - sum[j];
                if (dinv) v[j] *= dinv[pr];
            }
            store_row<K>(out, r, v, kAll);
        }
    }
}

template <int LANES, int K>
__global__ __launch_bounds__(kBlock) void k_trsm_level(int r0, int r1, const int *frp, const int *fci, const double *fval,
                                                       const int *row_of, const double *dinv, const double *rhs, double *out)
{
    constexpr int RPB = kBlock / LANES;
    trsm_rows<LANES, K>(r0, r1, blockIdx.x * RPB + threadIdx.x / LANES, gridDim.x * RPB, frp, fci, fval, row_of, dinv, rhs,
                        out);
}

// consecutive narrow levels in ONE workgroup (k_trsv_small_levels): a workgroup-scope release + barrier + acquire hands a
// level's rows (same CU, same L1) to the threads that gather them in the next level
template <int LANES, int K>
__global__ __launch_bounds__(kBlock) void k_trsm_small_levels(int l0, int l1, const int *level_ptr, const int *frp,
                                                              const int *fci, const double *fval, const int *row_of,
                                                              const double *dinv, const double *rhs, double *out)
{
    constexpr int RPB = kBlock / LANES;
    for (int l = l0; l < l1; l++) {
        trsm_rows<LANES, K>(level_ptr[l], level_ptr[l + 1], threadIdx.x / LANES, RPB, frp, fci, fval, row_of, dinv, rhs, out);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __syncthreads();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    }
}

// the whole solve in ONE workgroup with the n x K block in LDS (k_trsv_lds): the chain between two levels is LDS read ->
// multiply-add -> shuffle -> LDS write -> barrier; each team's first row of the NEXT level (row pointers, first entry,
// right-hand sides, 1/diagonal) is fetched from global memory before the barrier.  The arithmetic per column is k_trsv_lds's:
// the first entry starts the sum, the others are added in the lane's order, the same xor tree.
template <int LANES, int K>
__global__ __launch_bounds__(kBlock) void k_trsm_lds(int n, int nlev, const int *level_ptr, const int *frp, const int *fci,
                                                     const double *fval, const int *row_of, const double *dinv,
                                                     const double *rhs, double *out)
{
    extern __shared__ __attribute__((aligned(16))) double xs[];       // n x K doubles, original row numbering
    constexpr int RPB = kBlock / LANES;
    const int lane = threadIdx.x & (LANES - 1), team = threadIdx.x / LANES;
    int pr = 0, s = 0, e = 0, r = 0, c = 0;
    double a = 0.0, di = 1.0;
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
            a = fval[s + lane];
        }
        if (lane == 0) {
            r = row_of[pr];
            load_row<K>(rhs, r, b);
            if (dinv) di = dinv[pr];
        }
    };
    fetch(0);
    for (int l = 0; l < nlev; l++) {
        const int lend = level_ptr[l + 1];
        const bool have = mine;
        const int pr0 = pr, s0 = s, e0 = e, r0 = r;
        const double di0 = di;
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
                for (int j = 0; j < K; j++) sum[j] = a * xv[j];
            }
            for (int k = s0 + lane + LANES; k < e0; k += LANES) {
                const double av = fval[k];
                double xv[K];
                load_row<K>(xs, fci[k], xv);
#pragma unroll
                for (int j = 0; j < K; j++) sum[j] += av * xv[j];
            }
        }
#pragma unroll
        for (int j = 0; j < K; j++) sum[j] = group_sum<LANES>(sum[j]);
        if (have && lane == 0) {
            double v[K];
#pragma unroll
            for (int j = 0; j < K; j++) {
                v[j] = b0[j] - sum[j];
                if (dinv) v[j] *= di0;
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
                const double av = fval[k];
                double xv[K];
                load_row<K>(xs, fci[k], xv);
#pragma unroll
                for (int j = 0; j < K; j++) t[j] += av * xv[j];
            }
#pragma unroll
            for (int j = 0; j < K; j++) t[j] = group_sum<LANES>(t[j]);
            if (lane == 0) {
                const int rr = row_of[q];
                double v[K];
                load_row<K>(rhs, rr, v);
#pragma unroll
                for (int j = 0; j < K; j++) {
                    v[j] = v[j] - t[j];
                    if (dinv) v[j] *= dinv[q];
                }
                store_row<K>(xs, rr, v, kAll);
                store_row<K>(out, rr, v, kAll);
            }
        }
        fetch(l + 1);                      // global loads of the next level overlap the barrier
        __syncthreads();
    }
}

namespace {

// the single-workgroup form: the factor's levels are narrow (TriHost::lds, decided at set-up for the single-column form) and
// the K-column block fits the LDS that form asks for
bool takes_lds(const cudamat_solver *s, const TriHost &H, int K)
{
    return H.lds && (size_t)s->n * (size_t)K <= (size_t)kLdsTrsvRows;
}

// the launch plan of trsv.hip's level-by-level form, as it is (TriHost::seg_begin / seg_end): a wide level is its own
// launch, a run of narrow levels one single-workgroup launch.  The grids depend on the factor only.
template <int LANES, int K>
int launch_trsm_segments(hipStream_t st, const TriFactor &F, const TriHost &H, const double *rhs, double *out)
{
    constexpr int RPB = kBlock / LANES;
    for (size_t g = 0; g < H.seg_begin.size(); g++) {
        const int l0 = H.seg_begin[g], l1 = H.seg_end[g];
        const int r0 = F.level_ptr[(size_t)l0], r1 = F.level_ptr[(size_t)l1];
        if (segment_is_wide(F, H, g)) {
            hipLaunchKernelGGL((k_trsm_level<LANES, K>), dim3(row_grid(r1 - r0, RPB)), dim3(kBlock), 0, st, r0, r1, F.rp, F.ci, F.val, F.row_of,
                               F.dinv, rhs, out);
        } else {
            hipLaunchKernelGGL((k_trsm_small_levels<LANES, K>), dim3(1), dim3(kBlock), 0, st, l0, l1, H.level_ptr_dev, F.rp,
                               F.ci, F.val, F.row_of, F.dinv, rhs, out);
        }
    }
    CM_HIP(hipGetLastError());
    return CUDAMAT_OK;
}

template <int LANES, int K>
int launch_trsm(cudamat_solver *s, const TriFactor &F, const TriHost &H, const double *rhs, double *out)
{
    hipStream_t st = s->ctx->stream;
    if (takes_lds(s, H, K)) {
        const size_t bytes = sizeof(double) * (size_t)s->n * (size_t)K;
        CM_TRY(set_max_lds((const void *)k_trsm_lds<LANES, K>));
        hipLaunchKernelGGL((k_trsm_lds<LANES, K>), dim3(1), dim3(kBlock), bytes, st, s->n, F.nlevels, H.level_ptr_dev, F.rp,
                           F.ci, F.val, F.row_of, F.dinv, rhs, out);
        CM_HIP(hipGetLastError());
        return CUDAMAT_OK;
    }
    return launch_trsm_segments<LANES, K>(st, F, H, rhs, out);
}

template <int LANES>
int launch_trsm_k(cudamat_solver *s, const TriFactor &F, const TriHost &H, int K, const double *rhs, double *out)
{
    switch (K) {
    case 1: return launch_trsm<LANES, 1>(s, F, H, rhs, out);
    case 2: return launch_trsm<LANES, 2>(s, F, H, rhs, out);
    case 4: return launch_trsm<LANES, 4>(s, F, H, rhs, out);
    case 8: return launch_trsm<LANES, 8>(s, F, H, rhs, out);
    }
    set_error("triangular solve: %d columns per batch", K);
    return CUDAMAT_ERR_ARG;
}

}  // namespace

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
    switch (H.lanes) {
    case 2:  return launch_trsm_k<2>(s, F, H, K, rhs, out);
    case 4:  return launch_trsm_k<4>(s, F, H, K, rhs, out);
    case 8:  return launch_trsm_k<8>(s, F, H, K, rhs, out);
    case 16: return launch_trsm_k<16>(s, F, H, K, rhs, out);
    case 32: return launch_trsm_k<32>(s, F, H, K, rhs, out);
    default: return launch_trsm_k<64>(s, F, H, K, rhs, out);
    }
}

int precond_apply_b(cudamat_solver *s, int K, const double *in, double *tmp, double *out)
{
    CM_TRY(trsm_apply(s, s->L, false, K, in, tmp));     // pbicgstab.cu:92-94 / :121-123
    CM_TRY(trsm_apply(s, s->U, true, K, tmp, out));     // pbicgstab.cu:96-98 / :125-127
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
    if (!trsm_covered(s)) return CUDAMAT_OK;          // "": the factors run column by column (trsv.hip)
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
