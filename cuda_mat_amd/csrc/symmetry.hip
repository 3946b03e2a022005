// symmetry.hip -- is the resident matrix symmetric?  (cudamat_solver_symmetry; CUDAMAT_LOOP_CG asks at its first solve.)
//
// For every stored off-diagonal entry (i, j) the row j is searched for column i (rows are strictly increasing: binary search).
// Work is dealt by ENTRIES, grid-stride, the row of an entry found by a binary search of the row pointers: one long row
// costs what its entries cost, spread over the whole grid.  A set-up kernel: it runs once per set of values (~3 dependent
// gathers of log2 depth per entry), and its two results per workgroup -- a count and a maximum -- are combined on the host.
#include <math.h>

#include "solver.h"
#include "device.h"

namespace cm {

namespace {

// every thread of the workgroup receives the maximum (values >= 0)
__device__ __forceinline__ double block_max(double v, double *lds)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmax(fmax(lds[0], lds[1]), fmax(lds[2], lds[3]));
}

}  // namespace

__global__ __launch_bounds__(kBlock) void k_symmetry(int n, int64_t nnz, const int *rp, const int *ci, const double *val, double *parts)
{
    __shared__ double lds[8];
    double lone[1] = {0.0};       // (a count below 2^31: exact in a double, summed by the fixed-order block_sum)
    double diff = 0.0;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < nnz; e += stride) {
        int lo = 0, hi = n - 1;                      // the row of entry e: rp[i] <= e < rp[i + 1]
        while (lo < hi) {
            const int mid = lo + (hi - lo + 1) / 2;
            if (rp[mid] <= e) lo = mid;
            else hi = mid - 1;
        }
        const int i = lo, j = ci[e];
        if (j == i) continue;
        if (j >= n) { lone[0] += 1.0; continue; }    // (a column beyond the rows: no row to hold the partner)
        int a = rp[j], b = rp[j + 1] - 1, at = -1;
        while (a <= b) {
            const int mid = a + (b - a) / 2;
            const int c = ci[mid];
            if (c == i) { at = mid; break; }
            if (c < i) a = mid + 1;
            else b = mid - 1;
        }
        if (at < 0) { lone[0] += 1.0; continue; }
        const double dd = fabs(val[e] - val[at]);
        diff = fmax(diff, isnan(dd) ? INFINITY : dd);
    }
    block_sum<1>(lone, lds);
    diff = block_max(diff, lds + 4);
    if (threadIdx.x == 0) {
        parts[2 * blockIdx.x] = lone[0];
        parts[2 * blockIdx.x + 1] = diff;
    }
}

int launch_symmetry(hipStream_t s, int n, int64_t nnz, const int *rp, const int *ci, const double *val, double *parts, int *nparts)
{
    int64_t g = (nnz + kBlock - 1) / kBlock;
    if (g < 1) g = 1;
    if (g > kVecGridMax) g = kVecGridMax;
    *nparts = (int)g;
    hipLaunchKernelGGL(k_symmetry, dim3((unsigned)g), dim3(kBlock), 0, s, n, nnz, rp, ci, val, parts);
    CM_HIP(hipGetLastError());
    return CUDAMAT_OK;
}

int ensure_symmetry(cudamat_solver *s)
{
    if (s->sym_known) return CUDAMAT_OK;
    CM_ARG(!s->sharded, "cudamat_solver_symmetry: a sharded solver holds a slice of the rows (single GPU, whole matrix only)");
    CM_ARG(s->cols_sorted, "cudamat_solver_symmetry: every row's columns must be strictly increasing");
    CM_HIP(hipSetDevice(s->ctx->device));
    hipStream_t st = s->ctx->stream;
    int np = 0;
    CM_TRY(launch_symmetry(st, s->n, s->nnz, s->rp, s->ci, s->val, s->parts_tt, &np));
    std::vector<double> h(2 * (size_t)np);
    CM_HIP(hipMemcpyAsync(h.data(), s->parts_tt, sizeof(double) * h.size(), hipMemcpyDeviceToHost, st));
    CM_HIP(hipStreamSynchronize(st));
    long long lone = 0;
    double diff = 0.0;
    for (int b = 0; b < np; b++) {
        lone += (long long)h[2 * (size_t)b];
        diff = fmax(diff, h[2 * (size_t)b + 1]);
    }
    s->sym_unmatched = lone;
    s->sym_max_diff = diff;
    s->sym_known = true;
    return CUDAMAT_OK;
}

}  // namespace cm

extern "C" int cudamat_solver_symmetry(cudamat_solver *s, long long *unmatched, double *max_abs_diff)
{
    CM_ARG(s, "cudamat_solver_symmetry: solver is NULL");
    CM_TRY(cm::ensure_symmetry(s));
    if (unmatched) *unmatched = s->sym_unmatched;
    if (max_abs_diff) *max_abs_diff = s->sym_max_diff;
    return CUDAMAT_OK;
}
