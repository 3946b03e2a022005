// batch.h -- kernels of the multi-column (several right-hand sides) loop (internal API, batch.hip).
//
// Inside a batch, vectors are INTERLEAVED: n rows x K columns row-major, K in {1, 2, 4, 8}; column j of row i is at
// V[i*K + j], so one gathered column index yields K contiguous doubles.  Every column is an independent BiCGSTAB run with its
// own LoopState (an array of K of them).  The grid and the row partition of every kernel here depend on n and the SpMV plan
// only, never on K: a column's bits depend on its own data alone, not on the batch it was solved in.
// Per-workgroup partial sums of S scalars per column are stored as parts[b * S*K + j*S + s].
#pragma once
#include "kernels.h"

namespace cm {

constexpr int kBatchMax = 8;       // columns of one batch
// the width K of the batch that holds kc columns: the next power of two, the rest is padding
inline int pow2_cols(int kc) { return kc <= 1 ? 1 : kc <= 2 ? 2 : kc <= 4 ? 4 : kBatchMax; }

// the loop arguments of a batch: column j uses st[j] and hist + j * hist_cap
struct BatchArgs {
    LoopState *st = nullptr;       // NULL: kernel used outside a solve
    double *hist = nullptr;
    int hist_cap = 0;
    int loop = 0;
    int no_exit = 0;
    unsigned long long *snap = nullptr;   // progress words: (k+1) << 32 | every column stopped
    int snap_slots = 0;
    int k = 0;
};

// Y = alpha (A + diag d) X + beta Y on the solver's 0-based CSR arrays, L lanes per row (the row partition of the lanes-per-row
// SpMV plan with that L).  dk (never set together with d): one shift per COLUMN, Y_j = alpha (A + diag dk_j) X_j + beta Y_j --
// column j is then bit-identical to the same launch with d = that column's shift.  dot: 0 none, 1 parts (y.w) per column, 2 (y.w, y.y); check: CHECK_HALF evaluates every column's
// half-step test from `half` (stride K) in the prologue.
struct SpmmArgs {
    int n;
    const int *rp, *ci;
    const double *val;
    const double *x;       // interleaved, indexed by column id
    const double *d;       // optional shift (local rows)
    const double *dk;      // optional per-column shifts, interleaved like x: column j of row i at dk[i*K + j]
    const double *xd;      // x of the local rows (for d .* x)
    double alpha, beta;
    double *y;
    int dot;
    const double *w;
    double *parts;         // stride 2K
    BatchArgs loop;
    int check;
    const double *half;    // k_half_b partials (stride K)
    int half_count;
};
// (the row partition is spmv_partition(L, n, ...), kernels.h; parts = its workgroups)
int launch_spmm(hipStream_t s, int L, int K, const SpmmArgs &a);

// column-major (leading dimension ld) <-> interleaved.  In: columns >= kc and rows in [rows, rows_out) become `fill`.
int launch_batch_in(hipStream_t s, int K, int kc, int64_t rows, int64_t rows_out, const double *src, int64_t ld, double fill,
                    double *dst);
int launch_batch_out(hipStream_t s, int K, int kc, int64_t rows, const double *src, double *dst, int64_t ld);

// the loop's vector kernels, column by column what kernels.h's single-vector forms do (the same steps of steps.h, in the same order)
int launch_init_b(hipStream_t s, int K, int64_t n, const double *b, double *r, double *rw, double *p, double *parts,
                  int *nparts);
// columns >= kc are dead: their state starts at 2 (stopped) and nothing touches them
int launch_init_finish_b(hipStream_t s, int K, int kc, LoopState *st, const double *parts, int count, double tol, int no_exit,
                         const double *r, int64_t n);
int launch_update_p_b(hipStream_t s, int K, BatchArgs la, const double *full, int full_count, int64_t n, const double *r,
                      double *p, const double *v);
int launch_half_b(hipStream_t s, int K, BatchArgs la, const double *rv, int rv_count, int64_t n, double *r, const double *v,
                  double *parts, int *nparts);
// x += alpha pw, x += omega s, r -= omega t, (rw.r, r.r), it++; publishes the progress word
int launch_full_b(hipStream_t s, int K, BatchArgs la, const double *tt, int tt_count, int64_t n, double *x, const double *sv,
                  double *r, const double *t, const double *rw, const double *pw, double *parts, int *nparts);
// the half-step test of every running column from k_half_b's partials (stride K), where it cannot ride in an SpMM's prologue
int launch_check_half_b(hipStream_t s, int K, BatchArgs la, const double *half, int half_count);
// the last full-step test of every running column
int launch_check_full_b(hipStream_t s, int K, BatchArgs la, const double *full, int full_count);
// columns that left through the half step: x += alpha pw (pbicgstab.cu:110)
int launch_half_exit_b(hipStream_t s, int K, const LoopState *st, int64_t n, const double *pw, double *x);

}  // namespace cm
