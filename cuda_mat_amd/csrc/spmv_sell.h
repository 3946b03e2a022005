// spmv_sell.h -- SELL-C-sigma copy of a CSR matrix and its SpMV (internal API; see spmv_sell.hip).
#pragma once
#include "kernels.h"

namespace cm {

struct SellPlan {
    int n = 0;
    int64_t nnz = 0;
    int nchunks = 0;               // chunks of 64 rows (the last window is padded with empty rows)
    long long slots = 0;           // stored slots incl. padding
    double fill = 1.0;             // slots / nnz
    int grid = 0, chunks_per_block = 0;
    DevBuf<double> val;            // [slots] column-major inside a chunk
    DevBuf<int> col;
    DevBuf<int> perm;             // [nchunks * 64] original row of every chunk lane, -1 = padding row
    DevBuf<int> len;              // [nchunks * 64] entries of that row
    DevBuf<long long> chunk_off;     // [nchunks + 1] first column (of 64 slots) of every chunk
    double build_seconds = 0.0;
};

// max_fill > 0: give up (CUDAMAT_ERR_ARG, nothing allocated for the entries) when slots / nnz would exceed it
int sell_build(hipStream_t st, int n, int64_t nnz, const int *rp, const int *ci, const double *val, SellPlan *out,
               double max_fill = 0.0);
void sell_free(SellPlan *p);
// new values (CSR order of `rp`) into the slots the copy holds: the layout is closed-form in (row, entry of the row)
int sell_refresh_values(hipStream_t st, const SellPlan &plan, const int *rp, const double *val);
// y = alpha*(A x + d.*xd) + beta*y with the same fused dot / prologue options as launch_spmv
int launch_spmv_sell(hipStream_t st, const SellPlan &plan, const SpmvArgs &a);

}  // namespace cm
