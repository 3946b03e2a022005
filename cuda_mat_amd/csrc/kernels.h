// kernels.h -- launch wrappers of the hand-written gfx950 kernels (internal API).
#pragma once
#include "common.h"

namespace cm {

struct LoopArgs {
    LoopState *st = nullptr;   // NULL: kernel used outside a solve (no freeze / checks)
    double *hist = nullptr;
    int hist_cap = 0;
    int loop = 0;              // CUDAMAT_LOOP_*
    int no_exit = 0;
    // per-iteration progress word in PINNED HOST memory: k_full publishes (k+1) << 32 | state with one
    // 8-byte system-scope store, so the host can look at a lagged state without a copy or an event
    unsigned long long *snap = nullptr;
    int snap_slots = 0;
    int k = 0;                 // the host's iteration index of this launch
};

struct SpmvPlan {
    int lanes;            // lanes cooperating on one row (2..64)
    int grid;             // workgroups
    int rows_per_block;   // contiguous rows owned by a workgroup
    int stream_rows;      // > 0: LDS-staged stream kernel, this many rows per LDS tile (short rows)
    // > 0: nnz-balanced tiles of 2048 entries (skewed row lengths); rows_per_block = tiles per workgroup;
    // the tables are owned by the plan
    int tiles = 0;
    int tile_nspan = 0, tile_fix_grid = 0;
    DevBuf<int> tile_S, tile_span;
    DevBuf<double> tile_heads, tile_tails;
    double lane_cost = 0.0;   // lane-iterations of the lanes-per-row kernel / nnz (1 = perfectly balanced)
    // stream kernel with compressed indices (banded matrices): 16-bit column offsets from the tile's first row,
    // 8-bit row lengths, one entry offset per tile; owned by the plan
    DevBuf<short> c_off16;
    DevBuf<unsigned char> c_len8;
    DevBuf<int> c_tile_base;
    // line-aligned copies for the compressed stream kernel (plan_spmv_align, round 3): every tile's entries start on a
    // 64-entry boundary, so each wave's 512-byte value load and 128-byte offset load covers whole 128-byte lines
    DevBuf<int> a_base;                 // ntiles + 1: first entry slot of every tile
    DevBuf<short> a_off16;
    DevBuf<double> a_val;
    // the matrix's value dictionary (valdict.h; 256 doubles on the device, not owned) when the copies below exist
    const double *c_dict = nullptr;
    // dictionary form of the compressed stream kernel (plan_spmv_dict): per tile, the entries' 16-bit offsets and 8-bit
    // value indices padded to a multiple of 8 entries, so that a thread fetches its 8 entries with one 16-byte and one
    // 8-byte load (owned by the plan)
    DevBuf<int> d_pbase;                // ntiles + 1: first padded entry of every tile
    DevBuf<short> d_off16;
    DevBuf<unsigned char> d_val8;
};
SpmvPlan plan_spmv(const Config &cfg, int n_rows, int64_t nnz);
// The row partition of the lanes-per-row kernels (k_spmv<L>, k_spmm_csr<L, K>): every workgroup owns rows_per_block
// contiguous rows, a multiple of its kBlock / L groups, on at most kSpmvGridMax workgroups.  It depends on n_rows and L
// only, and both kernels take it from here: a row is reduced the same way with one column or K.
inline void spmv_partition(int L, int n_rows, int *grid, int *rows_per_block)
{
    const int rpb = kBlock / L;
    long long groups = ((long long)n_rows + rpb - 1) / rpb;
    int g = (int)(groups < kSpmvGridMax ? groups : kSpmvGridMax);
    if (g < 1) g = 1;
    long long per = ((long long)n_rows + g - 1) / g;
    per = (per + rpb - 1) / rpb * rpb;
    if (per < rpb) per = rpb;
    *rows_per_block = (int)per;
    *grid = (int)(((long long)n_rows + per - 1) / per);
    if (*grid < 1) *grid = 1;
}
// per-workgroup dot partials one launch leaves behind
inline int plan_spmv_parts(const SpmvPlan &p) { return p.grid + (p.tiles ? p.tile_fix_grid : 0); }
// short rows (mean <= 12): switch the plan to the LDS-staged stream kernel when every tile of
// `stream_rows` consecutive rows holds at most kStreamNnz entries (checked on the device); otherwise, when
// the lanes-per-row kernel would spend > 2.5 lane-iterations per entry (skewed row lengths), switch it to the
// nnz-balanced tile kernel.  CUDAMAT_SPMV_FORM=lanes|tiles forces one of the two.
// scratch: >= 64 bytes of device memory for the plan's read-backs (cudamat_ctx::scratch); NULL: allocated and freed here
int plan_spmv_refine(hipStream_t s, const Config &cfg, int n_rows, int64_t nnz, const int *rp, int base, SpmvPlan *plan, void *scratch = nullptr);

// y = alpha*(A x + d .* xd) + beta*y  on 0- or 1-based CSR (base folded into the
// pointers by the caller).  dot: 0 none, 1: parts[2b] = sum y*w, 2: also
// parts[2b+1] = sum y*y.  check: CHECK_HALF evaluates the half-step stopping test
// from `half` in the prologue.
struct SpmvArgs {
    int n;
    const int *rp;
    const int *ci;
    const double *val;
    const double *x;      // indexed by column id
    const double *d;      // optional diagonal shift (local rows)
    const double *xd;     // x restricted to the local rows (for d .* x)
    double alpha, beta;
    double *y;
    int dot;
    const double *w;
    double *parts;
    LoopArgs loop;
    int check;
    ScalarSrc half;
    int pb_strict;        // blocked form, phase 2: add a row's products of one wave instruction rank by rank (Config::pb_strict)
    const int *xd_idx;    // blocked form, phase 2: the shift term of row i reads xd[xd_idx[i]] (nullptr: xd[i]) -- rows and x in
                          // different index spaces (the loop in level-major spaces with a shift, loops.hip)
};
int launch_spmv(hipStream_t s, const SpmvPlan &plan, const SpmvArgs &a);

// fused loop of small systems: the SpMV computes its input vector on the fly (small_loops.hip)
struct FuseArgs {
    int mode;                              // 1: p' = r + beta (p - omega v);  2: s = r - alpha v
    const double *r;
    const double *p_old, *v_old;           // mode 1 inputs
    double *p_out;                         // mode 1: p' stored by the row owners
    const double *v;                       // mode 2 input (the v just computed)
    double *s_out, *xsol;                  // mode 2: s stored by the row owners, x += alpha p'
    const double *p;
    ScalarSrc src;                         // mode 1: (rw.r, ||r||^2) partials;  mode 2: rw.v partials
    double *parts_half;                    // mode 2: ||s||^2 partial of every workgroup
};
// the whole loop in one launch (small systems; small_loops.hip)
struct ResidentArgs {
    int iters;                 // iterations this launch may run (it stops early when a test fires)
    int first_count;           // partial sums behind parts_full at this launch's first iteration
    unsigned spin_limit;       // polls a barrier wait may take (2^22 ~ seconds; CUDAMAT_RESIDENT_SPIN_LIMIT: tests)
    unsigned *bar;             // [0] barrier arrivals, [1] set when a barrier wait ran into its bound; zeroed by the host
    double *p_a, *p_b, *v_a, *v_b, *r, *s, *t, *x;
    const double *rw;
    double *parts_rv, *parts_tt, *parts_half, *parts_full;
};
bool resident_loop_supported(const SpmvPlan &plan, int n);
int launch_resident_loop(hipStream_t s, const SpmvPlan &plan, const SpmvArgs &a, const ResidentArgs &q);
bool fused_spmv_supported(const SpmvPlan &plan);
int launch_fused_spmv(hipStream_t s, const SpmvPlan &plan, const SpmvArgs &a, const FuseArgs &f);
// stream plans only: build the compressed index copy when every offset fits (no-op otherwise); rp/ci 0-based
int plan_spmv_compress(hipStream_t s, const Config &cfg, int n_rows, int64_t nnz, const int *rp, const int *ci, SpmvPlan *plan);
// compressed stream plans of a matrix with a value dictionary (valdict.h): vidx = 8-bit value index per entry in CSR
// order, dict = 256 doubles on the device (not owned); no-op when the plan has no compressed copy
int plan_spmv_align(hipStream_t s, const Config &cfg, int n_rows, int64_t nnz, const int *rp, const double *val, SpmvPlan *plan);
int plan_spmv_dict(hipStream_t s, int n_rows, int64_t nnz, const int *rp, const unsigned char *vidx, const double *dict,
                   SpmvPlan *plan);
// new values into whichever of those two copies the plan holds (same storage class; no-op for a plan without one)
int plan_spmv_refresh_values(hipStream_t s, int n_rows, int64_t nnz, const int *rp, const double *val, const unsigned char *vidx,
                             const double *dict, SpmvPlan *plan);

int vec_grid(int64_t n);
// workgroups of a grid-stride kernel over `rows` items, `per_block` of them per workgroup and sweep: at least 1, at most 4096
inline int row_grid(int64_t rows, int64_t per_block = kBlock)
{
    const int64_t g = (rows + per_block - 1) / per_block;
    return (int)(g < 1 ? 1 : g > 4096 ? 4096 : g);
}

// r = b - r (r holds A x0 on entry), rw = r, p = r; parts[2b] = parts[2b+1] = sum r^2
int launch_init(hipStream_t s, int64_t n, const double *b, double *r, double *rw, double *p,
                double *parts, int *nparts);
// one workgroup: set up LoopState from the initial reduction
// abs_tol > 0: the loop stops at this absolute residual norm (tol is ignored) and starts out 'converged' when the
// initial residual is within twice of it
int launch_init_finish(hipStream_t s, LoopState *st, ScalarSrc init, double tol, double abs_tol, int no_exit, const double *r,
                       int64_t n);
// p = r + beta (p - omega v), preceded by the full-step test of the previous iteration
// rho_eps > 0 (guarded solves): `full` holds launch_full(..., guard = true)'s three sums from iteration 1 on, and the test
// |rho| <= rho_eps * sum |rw_i| |r_i| follows the full-step test (state 4: restart requested)
int launch_update_p(hipStream_t s, LoopArgs la, ScalarSrc full, int64_t n, const double *r,
                    double *p, const double *v, double rho_eps = 0.0);
// alpha = rho / (rw.v); r -= alpha v; parts[b] = sum r^2   (the half step's x += alpha pw rides in launch_full(..., pw))
int launch_half(hipStream_t s, LoopArgs la, ScalarSrc rv, int64_t n, double *r, const double *v, double *parts, int *nparts);
// omega = (t.r)/(t.t); x += omega s; r -= omega t; parts = (rw.r, r.r); it++
// half.ptr != NULL: evaluate the half-step stopping test from `half` first (fused small-system loop)
// pw != NULL: x += alpha pw (the half step's update, with the alpha k_half stored) before x += omega s
// guard: parts = (rw.r, r.r, sum |rw_i| |r_i|), stride 3
int launch_full(hipStream_t s, LoopArgs la, ScalarSrc tt, int64_t n, double *x, const double *sv,
                double *r, const double *t, const double *rw, double *parts, int *nparts,
                ScalarSrc half = ScalarSrc{nullptr, 0, 1}, const double *pw = nullptr, bool guard = false);
// pipelined BiCGStab (pipelined.hip): partials of k_pipe_a have stride 3, of k_pipe_b stride 5
int launch_pipe_seed(hipStream_t s, ScalarSrc init, ScalarSrc rww, double *out5);
// the hatted (M^-1-applied) vectors of the preconditioned form; all NULL without a preconditioner
struct PipeHatA { const double *rh, *wh, *zh; double *sh, *qh; };
struct PipeHatB { const double *qh, *wh, *zh; double *rh; };
int launch_pipe_a(hipStream_t s, LoopArgs la, ScalarSrc B, int64_t n, const double *r, const double *w, const double *t,
                  const double *v, double *p, double *sv, double *z, double *q, double *y, const double *x, double *xh,
                  double *parts, int *nparts, PipeHatA hat);
int launch_pipe_b(hipStream_t s, LoopArgs la, ScalarSrc A, int64_t n, const double *q, const double *y, const double *t,
                  const double *v, const double *rw, const double *sv, const double *z, const double *xh, double *x, double *r,
                  double *w, double *parts, int *nparts, PipeHatB hat);
// residual replacement: r = f - ax; the five dots of k_pipe_b recomputed (stride 5 partials)
int launch_residual(hipStream_t s, const LoopArgs &la, int64_t n, const double *f, const double *ax, double *r);
int launch_pipe_dots(hipStream_t s, const LoopArgs &la, int64_t n, const double *rw, const double *r, const double *w, const double *sv,
                     const double *z, double *parts, int *nparts);
// BiCGSTAB(2), CUDAMAT_LOOP_BICGSTAB_L2 (bicgstab_l2.hip): the six vector kernels of one sweep, in launch order.  Every scalar
// is formed in the prologue of the kernel that consumes it, from the partials of the kernel or SpMV that produced its dot; a
// breakdown (a zero divisor, a scalar that is not finite) freezes the loop in state 3 unless la.no_exit.
// once, after launch_init: parts = (r0.r0, r0.r0), stride 2, summed in the pair order whatever the alignment of the caller's b
int launch_l2_start(hipStream_t s, int64_t n, const double *r0, double *parts, int *nparts);
// the stopping test of the sweep before (full = (r0.r~, r0.r0), stride 2); rho0 = -omega rho0, beta; u0 = r0 - beta u0
int launch_l2_u0(hipStream_t s, LoopArgs la, ScalarSrc full, int64_t n, const double *r0, double *u0);
// gamma = u1.r~ (gam), alpha; r0 -= alpha u1; y += alpha u0
int launch_l2_step0(hipStream_t s, LoopArgs la, ScalarSrc gam, int64_t n, double *r0, const double *u1, const double *u0, double *y);
// rho1 = r1.r~ (rho), beta; u0 = r0 - beta u0; u1 = r1 - beta u1
int launch_l2_u1(hipStream_t s, LoopArgs la, ScalarSrc rho, int64_t n, const double *r0, const double *r1, double *u0, double *u1);
// gamma = u2.r~ (gam), alpha; r0 -= alpha u1; r1 -= alpha u2; y += alpha u0; parts = (r1.r1, r1.r0), stride 2
int launch_l2_step1(hipStream_t s, LoopArgs la, ScalarSrc gam, int64_t n, double *r0, double *r1, const double *u0, const double *u1,
                    const double *u2, double *y, double *parts, int *nparts);
// parts[b] = sum r2 r0 (the one reduction pass of a sweep that rides in no other kernel); returns at once when frozen
int launch_l2_dot(hipStream_t s, LoopArgs la, int64_t n, const double *r2, const double *r0, double *parts, int *nparts);
// the 2 x 2 minimal-residual system from d11 = (r1.r1, r1.r0), d2 = (r2.r1, r2.r2), d20 = r2.r0; y += g1 r0 + g2 r1;
// u0 -= g1 u1 + g2 u2; r0 -= g1 r1 + g2 r2; omega = g2; parts = (r0.r~, r0.r0), stride 2; it++; the progress word
int launch_l2_mr(hipStream_t s, LoopArgs la, ScalarSrc d11, ScalarSrc d2, ScalarSrc d20, int64_t n, double *y, double *r0,
                 const double *r1, const double *r2, double *u0, const double *u1, const double *u2, const double *rt,
                 double *parts, int *nparts);
// the stopping test of the last sweep, after the loop (one workgroup)
int launch_l2_check(hipStream_t s, LoopArgs la, ScalarSrc full);
// Conjugate gradients, CUDAMAT_LOOP_CG (cg.hip): k_cg_p | SpMV (+ p.q) | k_cg_step | [M^-1 | k_cg_rz].  Scalars as for
// BiCGSTAB(2): formed in the consuming kernel's prologue; !(gamma > 0), !(rho > 0) or a scalar that is not finite freezes the
// loop in state 3 unless la.no_exit.
// the stopping test of the iteration before (full = (r.z, r.r), stride 2); rho, beta; p = z + beta p
int launch_cg_p(hipStream_t s, LoopArgs la, ScalarSrc full, int64_t n, const double *z, double *p);
// gamma = p.q (gam), alpha; x += alpha p; r -= alpha q; parts = (r.r, r.r), stride 2; it++; the progress word
int launch_cg_step(hipStream_t s, LoopArgs la, ScalarSrc gam, int64_t n, double *x, double *r, const double *p, const double *q,
                   double *parts, int *nparts);
// parts = (r.z, r.r), stride 2; returns at once when frozen
int launch_cg_rz(hipStream_t s, LoopArgs la, int64_t n, const double *r, const double *z, double *parts, int *nparts);
// the stopping test of the last iteration, after the loop (one workgroup)
int launch_cg_check(hipStream_t s, LoopArgs la, ScalarSrc full);
// Symmetry of a CSR matrix with strictly increasing rows (symmetry.hip): parts[2 b] = stored off-diagonal entries (i, j)
// without a stored (j, i) that workgroup b met, parts[2 b + 1] = its max |a_ij - a_ji| over the others (inf where that
// difference is NaN); *nparts workgroups
int launch_symmetry(hipStream_t s, int n, int64_t nnz, const int *rp, const int *ci, const double *val, double *parts, int *nparts);
// standalone stopping tests (one workgroup)
int launch_check(hipStream_t s, LoopArgs la, ScalarSrc src, int which);
// out[k] = sum of partials, k < K (one workgroup)
int launch_reduce_parts(hipStream_t s, ScalarSrc in, int K, double *out, int sqrt_it);
int launch_nrm2_finish(hipStream_t s, ScalarSrc sq, int64_t n, const double *x, double *out);
// generic streaming kernels
int launch_dot_parts(hipStream_t s, int64_t n, const double *x, const double *y, double *parts,
                     int *nparts);
int launch_axpy(hipStream_t s, int64_t n, double alpha, const double *x, double *y);
int launch_scal(hipStream_t s, int64_t n, double alpha, double *x);
int launch_fill(hipStream_t s, int64_t n, double value, double *x);
int launch_rebase(hipStream_t s, int64_t n, const int *in, int shift, int *out);

}  // namespace cm
