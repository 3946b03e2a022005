// loops_batch.hip -- several right-hand sides for one resident matrix: cudamat_solver_spmm, cudamat_solver_precond_apply_many,
// cudamat_solver_solve_many, cudamat_solver_history_col; and their forms with one shift vector per column,
// (A0 + I d_j) x_j = b_j: cudamat_solver_spmm_shifts, cudamat_solver_solve_shifts; with one set of ILU(0) factors per column on
// top: cudamat_solver_solve_shifts_ilu0, cudamat_solver_precond_apply_shifts, cudamat_solver_ilu0_shifts_values.
//
// Each column is an INDEPENDENT run of the reference loop (pbicgstab.cu:45-154; :581-754 for the (A0 + I d) variant) with its
// own rho, alpha, omega, stopping tests, breakdown guard and history; nothing of one column enters another (this is not
// block-BiCGSTAB).  The batched form runs up to 8 columns through the same launches: per iteration
//   k_update_p_b | SpMM (+ rw.v) | k_half_b | SpMM (+ t.r, t.t; half-step tests in its prologue) | k_full_b
// with the vectors interleaved (batch.h), so each SpMM streams the matrix once for all of them.  The host loop has the shape of
// Solve::run_host_loop and shares its pieces (solver.h: wait_progress, history_need / history_count, stats_from_state / stats_ilu0;
// defined in loops.hip): iteration k is enqueued while the progress word of iteration k - kLag, (k+1) << 32 | every column
// stopped, is looked at; a stopped column is frozen by the kernels, so the lagged look costs no accuracy.
// With CUDAMAT_PRECOND_ILU0 and the switch MANY_PRECOND = batched | auto (default: columns) the reference loop runs batched too
// (Solve::iterate_reference per column, pbicgstab.cu:92-98, :116, :121-127):
//   k_update_p_b | ph = U^-1 L^-1 p | SpMM v = A ph (+ rw.v) | k_half_b | half-step tests | sh = U^-1 L^-1 r |
//   SpMM t = A sh (+ t.r, t.t) | k_full_b(x, sv = sh, r, t, rw, pw = ph)
// with the multi-column triangular solves of trsv.hip: one gathered index yields K doubles, one level hop serves K columns, the
// factors are read once.  The half-step tests get a launch of their own (they must be decided before sh is computed).  The
// triangular solves write ph, sh and a scratch block only, for every column of the block: a stopped column's x, r, p and history
// keep their bits, and its ph -- which a half-step exit still owes to x -- is recomputed from its frozen p to the same bits.
// Form choice (MANY_FORM = auto): the first batched solve of a solver times a few iterations of the batched loop (K columns)
// against the same number of iterations of the loop a single solve uses (cudamat_solver_solve, which picks the one- or
// three-launch loops of small systems), and runs batched only when that is faster than kc single solves.  Everything the batched
// form does not cover (ILU(0) unless MANY_PRECOND asks for it, and then hybrid factors in level-major spaces; block-Jacobi ILU(0),
// the pipelined loop, sharded solvers, the DEBUG / PROFILE / GUARD flags) and a failed allocation of its buffers run column by column: cudamat_solver_solve once per column, bit for bit what a caller's loop would do.
// Per-column shifts (D != NULL): the batched form transposes D into one more interleaved block (many.dk, padding columns 0) and
// every SpMM of the loop -- r0 = b - (A0 + I d_j) x0_j included -- adds dk_j .* x_j where it would add d .* x_j; the solver's own
// shift is not read.  Column by column, the solver's shift points at column j of D for the length of that column's solve (a
// caller's set_shift + solve, bit for bit) and is put back when the call returns, whatever it returns.
// Per-column shifts WITH ILU(0) (cudamat_solver_solve_shifts_ilu0, end of this file): M_j = ILU(0)(A0 + diag d_j), one set of
// factor values per column on the solver's shared structure.  Per block: the K-wide numeric factorisation (ilu.hip) into the
// fourth buffer group (many.lu_b, lval_b, uval_b, dinv_b), then run_group with pc and shifts, whose two preconditioner
// applications read those (precond_apply_cols, trsv.hip).  cudamat_solver_solve_shifts keeps its refusal of the pair.
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "batch.h"
#include "ilu.h"
#include "solver.h"
#include "trsm.h"

using namespace cm;

namespace {

int log2_cols(int K) { return K == 1 ? 0 : K == 2 ? 1 : K == 4 ? 2 : 3; }

int64_t many_rows(const cudamat_solver *s)
{
    int64_t rows = s->n_pad > s->n ? s->n_pad : s->n;
    if (s->n_cols > rows) rows = s->n_cols;
    return rows > 0 ? rows : 1;
}

// The interleaved buffers come in four groups, each a list of (owner, doubles for K columns, zeroed at allocation?): the plain
// loop's -- seven vectors (r, rw, p, v, t, b, x), the partial sums; the K loop states go with them --, the
// three further blocks of the preconditioned loop: ph = M^-1 p, sh = M^-1 r and the scratch of L^-1; and the per-column
// shifts' one block; and the per-column factors of one block (the K-wide LU values, L's and U's values in level-major order,
// 1 / U's diagonal: sized by the solver's ILU(0) structure, which must exist).
enum Group { G_PLAIN = 0, G_PRECOND = 1, G_SHIFTS = 2, G_FACTORS = 3 };

int &group_cap(cudamat_solver *s, Group g)
{
    return g == G_PRECOND ? s->many.pcap : g == G_SHIFTS ? s->many.dcap : g == G_FACTORS ? s->many.fcap : s->many.cap;
}

struct Buf {
    DevBuf<double> *p;
    size_t count;
    bool zero;
};

std::vector<Buf> many_group(cudamat_solver *s, Group g, int K)
{
    ManyWork &m = s->many;
    const size_t nv = (size_t)K * (size_t)many_rows(s);
    if (g == G_SHIFTS) return {{&m.dk, nv, true}};
    if (g == G_FACTORS)      // (every entry of every column, padding included, is written by each factorisation)
        return {{&m.lu_b, (size_t)K * (size_t)s->pm_nnz, false}, {&m.lval_b, (size_t)K * (size_t)s->L.nnz, false},
                {&m.uval_b, (size_t)K * (size_t)s->U.nnz, false}, {&m.dinv_b, (size_t)K * (size_t)s->n, false}};
    if (g == G_PRECOND) return {{&m.pw, nv, true}, {&m.s, nv, true}, {&m.lt, nv, true}};
    const size_t pv = 2 * (size_t)K * kVecGridMax, ps = 2 * (size_t)K * kSpmvGridMax;
    return {{&m.r, nv, true}, {&m.rw, nv, true}, {&m.p, nv, true}, {&m.v, nv, true}, {&m.t, nv, true}, {&m.b, nv, true},
            {&m.x, nv, true}, {&m.parts_full, pv, false}, {&m.parts_half, pv, false}, {&m.parts_rv, ps, false},
            {&m.parts_tt, ps, false}};
}

void free_group(cudamat_solver *s, Group g)
{
    for (const Buf &b : many_group(s, g, 0)) b.p->reset();
    if (g == G_PLAIN) s->many.st.reset();
    if (g == G_FACTORS) s->many.fzp.reset();
    group_cap(s, g) = 0;
}

}  // namespace

namespace cm {

void many_release(cudamat_solver *s)
{
    ManyWork &m = s->many;
    free_group(s, G_PLAIN);
    free_group(s, G_PRECOND);
    free_group(s, G_SHIFTS);
    free_group(s, G_FACTORS);
    m.hist.reset();
    m.hist_bytes = 0;
}

}  // namespace cm

namespace {

// One group holds K columns: allocated (and zeroed) as a whole, or -- CUDAMAT_ERR_NOMEM -- not at all.  A wider plain group
// replaces everything (the other groups and the histories go with it); a failed preconditioned or shift group leaves the plain
// one in place.  The stream is drained before anything is freed.
int ensure_many(cudamat_solver *s, Group g, int K)
{
    ManyWork &mw = s->many;
    // (the factor group is sized by the ILU(0) structure: another structure -- a set-up in between -- is another size)
    const bool same_structure = mw.f_nnz == s->pm_nnz && mw.f_lnnz == s->L.nnz && mw.f_unnz == s->U.nnz;
    if (group_cap(s, g) >= K && (g != G_FACTORS || same_structure)) return CUDAMAT_OK;
    hipStream_t st = s->ctx->stream;
    CM_HIP(hipStreamSynchronize(st));
    if (g != G_PLAIN) free_group(s, g);
    else many_release(s);
    int rc = CUDAMAT_OK;
    for (const Buf &b : many_group(s, g, K)) {
        if ((rc = b.p->alloc(b.count))) break;
        if (b.zero && (rc = CM_RC(hipMemsetAsync(b.p->get(), 0, sizeof(double) * b.count, st)))) break;
    }
    if (!rc && g == G_PLAIN) rc = s->many.st.alloc((size_t)K);       // the K loop states
    if (!rc && g == G_FACTORS) rc = s->many.fzp.alloc(1);            // the zero-pivot word
    if (rc) {
        CM_DROP(hipStreamSynchronize(st));
        free_group(s, g);
        return rc;
    }
    group_cap(s, g) = K;
    if (g == G_FACTORS) { mw.f_nnz = s->pm_nnz; mw.f_lnnz = s->L.nnz; mw.f_unnz = s->U.nnz; }
    return CUDAMAT_OK;
}

// Is there room for the batched form of a call with nrhs columns (the plain group, with `precond` / `shifts` / `factors` their
// groups too, for its widest block)?  Buffers that do not fit are not an error of the call -- *room = false, it runs column by column --; any other
// failure is.
int many_room(cudamat_solver *s, int nrhs, bool precond, bool shifts, bool *room, bool factors = false)
{
    const int K = pow2_cols(nrhs < kBatchMax ? nrhs : kBatchMax);
    int rc = ensure_many(s, G_PLAIN, K);
    if (rc == CUDAMAT_OK && precond) rc = ensure_many(s, G_PRECOND, K);
    if (rc == CUDAMAT_OK && shifts) rc = ensure_many(s, G_SHIFTS, K);
    if (rc == CUDAMAT_OK && factors) rc = ensure_many(s, G_FACTORS, K);
    *room = rc == CUDAMAT_OK;
    return rc == CUDAMAT_ERR_NOMEM ? CUDAMAT_OK : rc;
}

// the columns of a call in blocks of at most kBatchMax: kc columns from c0 on, in a batch of width K (the rest is padding)
struct ColBlock {
    int c0, kc, K;
};

std::vector<ColBlock> col_blocks(int nrhs)
{
    std::vector<ColBlock> blocks;
    for (int c0 = 0; c0 < nrhs; c0 += kBatchMax) {
        const int kc = nrhs - c0 < kBatchMax ? nrhs - c0 : kBatchMax;
        blocks.push_back({c0, kc, pow2_cols(kc)});
    }
    return blocks;
}

// dk: the interleaved per-column shifts of this batch, which then stand in for the solver's own shift
SpmmArgs spmm_args(const cudamat_solver *s, const double *x, double *y, const double *dk = nullptr)
{
    SpmmArgs a{};
    a.n = s->n; a.rp = s->rp; a.ci = s->ci; a.val = s->val;
    a.x = x; a.d = dk ? nullptr : s->d; a.dk = dk; a.xd = x;
    a.alpha = 1.0; a.beta = 0.0; a.y = y;
    a.dot = 0; a.w = nullptr; a.parts = nullptr;
    a.check = CHECK_NONE; a.half = nullptr; a.half_count = 0;
    return a;
}

// the solver's own shift, put back when the scope ends: a call with per-column shifts leaves s->d as it found it on every path
struct ShiftGuard {
    cudamat_solver *s;
    const double *saved;
    explicit ShiftGuard(cudamat_solver *sv) : s(sv), saved(sv->d) {}
    ~ShiftGuard() { s->d = saved; }
    ShiftGuard(const ShiftGuard &) = delete;
    ShiftGuard &operator=(const ShiftGuard &) = delete;
};

// One batch of kc <= K columns (K a power of two, the rest padding that starts stopped).  B / X column-major with leading
// dimensions ldb / ldx; B == NULL: many.b and many.x are already filled (the timing of the form choice), X == NULL: the iterate
// stays in many.x.  fin receives the K final states; hist_out (kc vectors, or NULL) the columns' residual histories.
// precond: CUDAMAT_PRECOND_NONE, or CUDAMAT_PRECOND_ILU0 with covered factors (trsm_covered), the reference loop and
// the preconditioned group allocated (many_room).  shifts: column j is (A0 + I d_j) x_j = b_j with the shifts of many.dk, filled
// here from D (column-major, ldd) unless D == NULL (filled already); the shift group allocated (many_room).
// cf (with precond and shifts): M_j is column j of these per-column factors (trsm.h), not the solver's own.
int run_group(cudamat_solver *s, int K, int kc, const double *B, int64_t ldb, double *X, int64_t ldx, int precond, int loop,
              int maxit, double tol, int flags, LoopState *fin, std::vector<double> *hist_out, double *t_loop,
              bool shifts = false, const double *D = nullptr, int64_t ldd = 0, const ColFactors *cf = nullptr)
{
    ManyWork &m = s->many;
    const bool pc = precond != CUDAMAT_PRECOND_NONE;
    hipStream_t st = s->ctx->stream;
    const int n = s->n;
    const int L = s->plan.lanes;
    const int need = history_need(loop, maxit);      // residual history, per column
    double *hist = nullptr;
    if (hist_out) {
        const size_t bytes = sizeof(double) * (size_t)K * (size_t)need;
        if (bytes > m.hist_bytes) {
            if (m.hist) { CM_HIP(hipStreamSynchronize(st)); m.hist.reset(); m.hist_bytes = 0; }      // drained first, then released
            CM_TRY(m.hist.alloc((size_t)K * (size_t)need));
            m.hist_bytes = bytes;
        }
        hist = m.hist;
        CM_HIP(hipMemsetAsync(hist, 0xFF, bytes, st));              // NaN fill
    }
    BatchArgs la{m.st, hist, need, loop, (flags & CUDAMAT_FLAG_NO_EXIT) ? 1 : 0, s->snap_dev, kRing, 0};
    for (int i = 0; i < kRing; i++) s->snap_host[i] = 0ULL;
    const double t0 = now_s();
    if (B) {
        CM_TRY(launch_batch_in(st, K, kc, n, n, B, ldb, 0.0, m.b));
        if (flags & CUDAMAT_FLAG_X0_ONES) CM_TRY(launch_fill(st, (int64_t)K * n, 1.0, m.x));
        else CM_TRY(launch_batch_in(st, K, kc, n, n, X, ldx, 0.0, m.x));
    }
    if (D) CM_TRY(launch_batch_in(st, K, kc, n, n, D, ldd, 0.0, m.dk));       // (padding columns: shift 0)
    const double *dk = shifts ? m.dk : nullptr;
    // r = A x0; r = b - r, rw = r, p = r; the states                                        pbicgstab.cu:67-74 / :645-659
    CM_TRY(launch_spmm(st, L, K, spmm_args(s, m.x, m.r, dk)));
    int np_full = 0, np_half = 0, np_spmm = 0, rpb = 0;
    spmv_partition(L, n, &np_spmm, &rpb);
    CM_TRY(launch_init_b(st, K, n, m.b, m.r, m.rw, m.p, m.parts_full, &np_full));
    CM_TRY(launch_init_finish_b(st, K, kc, m.st, m.parts_full, np_full, tol, la.no_exit, m.r, n));
    for (int k = 0; k < maxit; k++) {
        if (k >= kLag) {              // lagged look at the progress word of iteration k - kLag
            unsigned long long w = 0;
            CM_TRY(wait_progress(s, st, k - kLag, "batched ", &w));
            if ((unsigned)(w & 0xffffffffULL) != 0u) break;    // every column has stopped
        }
        la.k = k;
        // rho, beta, full-step tests, p = r + beta (p - omega v)                            :80-89
        CM_TRY(launch_update_p_b(st, K, la, m.parts_full, np_full, n, m.r, m.p, m.v));
        const double *pw = m.p;
        if (pc) {                                                                           // :92-98
            CM_TRY(cf ? precond_apply_cols(s, K, *cf, m.p, m.lt, m.pw) : precond_apply_b(s, K, m.p, m.lt, m.pw));
            pw = m.pw;
        }
        // v = A pw, rw.v                                                                      :104-106
        SpmmArgs a1 = spmm_args(s, pw, m.v, dk);
        a1.dot = 1; a1.w = m.rw; a1.parts = m.parts_rv; a1.loop = la;
        CM_TRY(launch_spmm(st, L, K, a1));
        // alpha, r -= alpha v, ||r||                                                          :107-111
        CM_TRY(launch_half_b(st, K, la, m.parts_rv, np_spmm, n, m.r, m.v, m.parts_half, &np_half));
        // half-step tests; t = A sv (sv = r, or M^-1 r), (t.r, t.t)                           :116, :121-127, :132-136
        const double *sv = m.r;
        if (pc) {              // the tests are decided before M^-1 r is computed, as in Solve::iterate_reference
            CM_TRY(launch_check_half_b(st, K, la, m.parts_half, np_half));
            CM_TRY(cf ? precond_apply_cols(s, K, *cf, m.r, m.lt, m.s) : precond_apply_b(s, K, m.r, m.lt, m.s));
            sv = m.s;
        }
        SpmmArgs a2 = spmm_args(s, sv, m.t, dk);
        a2.dot = 2; a2.w = m.r; a2.parts = m.parts_tt; a2.loop = la;
        if (!pc) { a2.check = CHECK_HALF; a2.half = m.parts_half; a2.half_count = np_half; }
        CM_TRY(launch_spmm(st, L, K, a2));
        // omega, x += alpha pw, x += omega sv, r -= omega t, (rw.r, ||r||), i++              :110, :137-151
        CM_TRY(launch_full_b(st, K, la, m.parts_tt, np_spmm, n, m.x, sv, m.r, m.t, m.rw, pw,
                             m.parts_full, &np_full));
    }
    // the last full-step tests; columns that left through the half step still owe x += alpha pw (:110)
    CM_TRY(launch_check_full_b(st, K, la, m.parts_full, np_full));
    CM_TRY(launch_half_exit_b(st, K, m.st, n, pc ? m.pw : m.p, m.x));
    CM_HIP(hipMemcpyAsync(fin, m.st, sizeof(LoopState) * (size_t)K, hipMemcpyDeviceToHost, st));
    if (X) CM_TRY(launch_batch_out(st, K, kc, n, m.x, X, ldx));
    CM_HIP(hipStreamSynchronize(st));
    if (t_loop) *t_loop = now_s() - t0;
    if (hist_out) {
        for (int j = 0; j < kc; j++) {
            const int c = history_count(loop, fin[j], need);
            hist_out[j].assign((size_t)c, 0.0);
            if (c > 0)
                CM_HIP(hipMemcpy(hist_out[j].data(), hist + (size_t)j * (size_t)need, sizeof(double) * (size_t)c,
                                 hipMemcpyDeviceToHost));
        }
    }
    return CUDAMAT_OK;
}

// MANY_FORM / MANY_PRECOND = auto: is the batched loop with K columns faster than kc single solves?  Timed once per solver,
// loop, preconditioner, with or without per-column shifts, and K (FLAG_NO_EXIT iterations on scratch right-hand sides: b = 1,
// x0 = 0); what the timing takes is added to *t_tune.  shifts: both sides run with a shift in place (scratch values in many.dk,
// all 0: the single solve reads its first n as the solver's shift, the batched loop the block) -- the caller fills many.dk after.
int prefer_batched(cudamat_solver *s, int K, int kc, int precond, int loop, bool shifts, bool *batched, double *t_tune)
{
    ManyWork &m = s->many;
    const double t0 = now_s();
    hipStream_t st = s->ctx->stream;
    const int n = s->n;
    if (m.tune_loop != loop || m.tune_precond != precond || m.tune_shifts != (shifts ? 1 : 0)) {
        m.tune_loop = loop;
        m.tune_precond = precond;
        m.tune_shifts = shifts ? 1 : 0;
        m.t_single = -1.0;
        for (double &t : m.t_batch) t = -1.0;
        // a few iterations: enough that launch and set-up overheads do not decide (small systems run ~10 us per iteration)
        const double it = 4e7 / (double)(s->nnz + 1);
        m.tune_iters = it < 4.0 ? 4 : it > 64.0 ? 64 : (int)it;
    }
    const int N = m.tune_iters;
    ShiftGuard own(s);
    if (shifts && (m.t_single < 0.0 || m.t_batch[log2_cols(K)] < 0.0)) CM_TRY(launch_fill(st, (int64_t)K * n, 0.0, m.dk));
    if (m.t_single < 0.0) {
        CM_TRY(ensure_work(s));
        CM_TRY(ensure_spmv_mode(s));
        if (shifts) s->d = m.dk;
        for (int rep = 0; rep < 2; rep++) {       // (the first run warms up: the loop forms allocate on first use)
            CM_TRY(launch_fill(st, n, 1.0, m.b));
            CM_TRY(launch_fill(st, n, 0.0, m.x));
            CM_HIP(hipStreamSynchronize(st));
            const double t = now_s();
            cudamat_stats dummy;
            CM_TRY(cudamat_solver_solve(s, m.b, m.x, precond, loop, rep ? N : 2, 1e-8, CUDAMAT_FLAG_NO_EXIT, &dummy));
            CM_HIP(hipStreamSynchronize(st));
            m.t_single = now_s() - t;
        }
        s->d = own.saved;
    }
    double &tb = m.t_batch[log2_cols(K)];
    if (tb < 0.0) {
        LoopState fin[kBatchMax];
        for (int rep = 0; rep < 2; rep++) {
            CM_TRY(launch_fill(st, (int64_t)K * n, 1.0, m.b));
            CM_TRY(launch_fill(st, (int64_t)K * n, 0.0, m.x));
            CM_HIP(hipStreamSynchronize(st));
            const double t = now_s();
            CM_TRY(run_group(s, K, K, nullptr, 0, nullptr, 0, precond, loop, rep ? N : 2, 1e-8, CUDAMAT_FLAG_NO_EXIT, fin,
                             nullptr, nullptr, shifts));
            tb = now_s() - t;
        }
    }
    // batched only when clearly faster (3 %: below that the two are within the noise of one timing)
    *batched = tb < 0.97 * (double)kc * m.t_single;
    if (s->ctx->cfg.verbose)
        fprintf(stderr, "[cudamat] several right-hand sides%s%s: %d iterations, single loop %.3f ms x %d columns, batched (K = %d) "
                        "%.3f ms -> %s\n", precond ? " with ILU(0)" : "", shifts ? " with per-column shifts" : "", N, 1e3 * m.t_single, kc, K, 1e3 * tb,
                *batched ? "batched" : "columns");
    *t_tune += now_s() - t0;
    return CUDAMAT_OK;
}

void fill_stats(cudamat_solver *s, const LoopState &f, int precond, cudamat_stats *o)
{
    stats_from_state(f, o);
    o->loop_form = 0;
    o->spmv_mode = 0;                    // the SpMM runs on the CSR arrays
    o->t_setup = s->t_create + s->t_spmv_setup;
    if (precond) {                       // as Solve::finish reports them; the level-scheduled kernels have no fall-back
        stats_ilu0(s, true, o);
        o->trsv_fallbacks = 0;
    }
}

}  // namespace

extern "C" int cudamat_solver_spmm_shifts(cudamat_solver *s, int nrhs, const double *X, int ldx, const double *D, int ldd,
                                          double *Y, int ldy)
{
    CM_ARG(s, "solver is NULL");
    CM_ARG(nrhs >= 0, "nrhs < 0");
    if (nrhs == 0) return CUDAMAT_OK;
    CM_ARG(X && Y, "null pointer");
    CM_ARG((int64_t)ldx >= (s->sharded ? (int64_t)s->n : s->n_cols) && ldy >= s->n, "leading dimension below the rows");
    CM_ARG(!D || ldd >= s->n, "leading dimension below the rows");
    CM_HIP(hipSetDevice(s->ctx->device));
    bool batched = !s->sharded;
    if (batched) CM_TRY(many_room(s, nrhs, false, D != nullptr, &batched));
    if (!batched) {                      // sharded, or no room for the interleaved buffers: one SpMV per column
        ShiftGuard own(s);
        for (int j = 0; j < nrhs; j++) {
            if (D) s->d = D + (size_t)j * ldd;
            CM_TRY(cudamat_solver_spmv(s, X + (size_t)j * ldx, Y + (size_t)j * ldy));
        }
        return CUDAMAT_OK;
    }
    ManyWork &m = s->many;
    hipStream_t st = s->ctx->stream;
    for (const ColBlock &c : col_blocks(nrhs)) {
        CM_TRY(launch_batch_in(st, c.K, c.kc, s->n_cols, many_rows(s), X + (size_t)c.c0 * ldx, ldx, 0.0, m.x));
        if (D) CM_TRY(launch_batch_in(st, c.K, c.kc, s->n, s->n, D + (size_t)c.c0 * ldd, ldd, 0.0, m.dk));
        CM_TRY(launch_spmm(st, s->plan.lanes, c.K, spmm_args(s, m.x, m.t, D ? m.dk : nullptr)));
        CM_TRY(launch_batch_out(st, c.K, c.kc, s->n, m.t, Y + (size_t)c.c0 * ldy, ldy));
    }
    return CUDAMAT_OK;
}

extern "C" int cudamat_solver_spmm(cudamat_solver *s, int nrhs, const double *X, int ldx, double *Y, int ldy)
{
    return cudamat_solver_spmm_shifts(s, nrhs, X, ldx, nullptr, 0, Y, ldy);
}

extern "C" int cudamat_solver_precond_apply_many(cudamat_solver *s, int nrhs, const double *In, int ldin, double *Out, int ldout)
{
    CM_ARG(s, "solver is NULL");
    CM_ARG(nrhs >= 0, "nrhs < 0");
    if (nrhs == 0) return CUDAMAT_OK;
    CM_ARG(In && Out, "null pointer");
    CM_ARG(ldin >= s->n && ldout >= s->n, "leading dimension below the rows");
    CM_ARG(s->has_ilu, "call cudamat_solver_ilu0 / cudamat_solver_block_ilu0 first");
    CM_HIP(hipSetDevice(s->ctx->device));
    bool batched = trsm_covered(s);
    if (batched) CM_TRY(many_room(s, nrhs, false, false, &batched));
    if (!batched) {                      // factors the multi-column kernels do not cover, or no room: one application per column
        CM_TRY(ensure_work(s));
        for (int j = 0; j < nrhs; j++) CM_TRY(precond_apply(s, In + (size_t)j * ldin, s->t, Out + (size_t)j * ldout));
        return CUDAMAT_OK;
    }
    ManyWork &m = s->many;
    hipStream_t st = s->ctx->stream;
    for (const ColBlock &c : col_blocks(nrhs)) {
        CM_TRY(launch_batch_in(st, c.K, c.kc, s->n, s->n, In + (size_t)c.c0 * ldin, ldin, 0.0, m.b));
        CM_TRY(precond_apply_b(s, c.K, m.b, m.t, m.x));
        CM_TRY(launch_batch_out(st, c.K, c.kc, s->n, m.x, Out + (size_t)c.c0 * ldout, ldout));
    }
    return CUDAMAT_OK;
}

extern "C" int cudamat_solver_solve_shifts(cudamat_solver *s, int nrhs, const double *D, int ldd, const double *B, int ldb,
                                           double *X, int ldx, int precond, int loop, int maxit, double tol, int flags,
                                           cudamat_stats *st, int *form)
{
    CM_ARG(s, "solver is NULL");
    CM_ARG(nrhs >= 0, "nrhs < 0");
    if (form) *form = 0;
    if (nrhs == 0) return CUDAMAT_OK;
    CM_ARG(B && X, "null pointer");
    CM_ARG(ldb >= s->n && ldx >= s->n && (!D || ldd >= s->n), "leading dimension below the rows");
    CM_ARG(!(D && precond), "the (A0 + I d) variant has no preconditioner (pbicgstab.h:110)");
    // ... and neither has the solver's own shift in a batch, whichever form the columns would take and whatever factors the
    // solver holds (those of cudamat_solver_ilu0_shift serve the single solve only: loops.hip)
    CM_ARG(!(s->d && precond), "the (A0 + I d) variant has no preconditioner (pbicgstab.h:110)");
    CM_ARG(maxit >= 0, "maxit");
    // (CUDAMAT_LOOP_BICGSTAB_L2 and CUDAMAT_LOOP_CG are neither `plain` nor `pc` below: their columns run one cudamat_solver_solve
    // each, form 0)
    CM_ARG(loop == CUDAMAT_LOOP_PBICGSTAB || loop == CUDAMAT_LOOP_PBICGSTAB2 || loop == CUDAMAT_LOOP_PIPELINED ||
           loop == CUDAMAT_LOOP_BICGSTAB_L2 || loop == CUDAMAT_LOOP_CG, "loop");
    CM_HIP(hipSetDevice(s->ctx->device));
    const double t0 = now_s();
    const Config &cfg = s->ctx->cfg;
    std::vector<cudamat_stats> out((size_t)nrhs);
    std::vector<std::vector<double>> hists((size_t)nrhs);
    double t_solve = 0.0, t_tune = 0.0;
    bool any_batched = false;
    // (a guarded solve -- CUDAMAT_FLAG_GUARD or the switch GUARD -- runs column by column: each column a guarded cudamat_solver_solve)
    const bool guarded = (flags & CUDAMAT_FLAG_GUARD) || cfg.guard;
    const bool one_gpu = !s->sharded && s->n_cols == s->n && s->n > 0 && !(flags & (CUDAMAT_FLAG_DEBUG | CUDAMAT_FLAG_PROFILE)) &&
                         !guarded;
    const bool plain = precond == CUDAMAT_PRECOND_NONE && (loop == CUDAMAT_LOOP_PBICGSTAB || loop == CUDAMAT_LOOP_PBICGSTAB2) && one_gpu;
    // ILU(0): only when MANY_PRECOND asks for it (0 = columns, the default: today's behaviour bit for bit), the reference loop,
    // and factors the multi-column triangular solves cover (trsm.h); set up on first use as Solve::setup does it
    bool pc = precond == CUDAMAT_PRECOND_ILU0 && loop == CUDAMAT_LOOP_PBICGSTAB && one_gpu && cfg.many_precond != 0 &&
              cfg.many_form != 2;
    if (pc) {
        CM_ARG(!s->d, "the (A0 + I d) variant has no preconditioner (pbicgstab.h:110)");
        if (!s->has_ilu) CM_TRY(ilu0_setup(s, false));
        pc = trsm_covered(s);
        if (!pc && cfg.verbose) fprintf(stderr, "[cudamat] ILU(0) factors not covered by the multi-column solves: column by column\n");
    }
    const bool batchable = plain || pc;
    bool room = false;
    if (batchable && cfg.many_form != 2) {
        CM_TRY(many_room(s, nrhs, pc, D != nullptr, &room));
        if (!room && cfg.verbose) fprintf(stderr, "[cudamat] no room for the batched loop's buffers: column by column\n");
    }
    const int pc_precond = pc ? CUDAMAT_PRECOND_ILU0 : CUDAMAT_PRECOND_NONE;
    const bool force_batched = pc ? cfg.many_precond == 2 : cfg.many_form == 1;
    const bool by_timing = pc ? cfg.many_precond == 1 : cfg.many_form == 0;
    ShiftGuard own(s);                   // (column by column, the solver's shift is column j of D while column j is solved)
    for (const ColBlock &c : col_blocks(nrhs)) {
        const int c0 = c.c0, kc = c.kc, K = c.K;
        bool batched = room && force_batched;
        if (room && by_timing) CM_TRY(prefer_batched(s, K, kc, pc_precond, loop, D != nullptr, &batched, &t_tune));
        if (batched) {
            LoopState fin[kBatchMax];
            double tl = 0.0;
            CM_TRY(run_group(s, K, kc, B + (size_t)c0 * ldb, ldb, X + (size_t)c0 * ldx, ldx, pc_precond, loop, maxit, tol, flags,
                             fin, hists.data() + c0, &tl, D != nullptr, D ? D + (size_t)c0 * ldd : nullptr, ldd));
            t_solve += tl;
            for (int j = 0; j < kc; j++) fill_stats(s, fin[j], pc_precond, &out[(size_t)(c0 + j)]);
            any_batched = true;
            continue;
        }
        for (int j = c0; j < c0 + kc; j++) {           // column by column: today's single solve
            cudamat_stats &sj = out[(size_t)j];
            if (D) s->d = D + (size_t)j * ldd;
            CM_TRY(cudamat_solver_solve(s, B + (size_t)j * ldb, X + (size_t)j * ldx, precond, loop, maxit, tol, flags, &sj));
            t_solve += sj.t_solve;
            int cnt = 0;
            std::vector<double> &h = hists[(size_t)j];
            h.assign((size_t)(s->hist_count > 0 ? s->hist_count : 0), 0.0);
            if (!h.empty()) CM_TRY(cudamat_solver_history(s, h.data(), (int)h.size(), &cnt));
        }
    }
    s->many.hist_host.swap(hists);
    const double t_total = now_s() - t0;
    for (cudamat_stats &o : out) {
        o.t_solve = t_solve;
        o.t_total = t_total;
        o.t_tune += t_tune;
    }
    if (st) memcpy(st, out.data(), sizeof(cudamat_stats) * (size_t)nrhs);
    if (form) *form = any_batched ? 1 : 0;
    return CUDAMAT_OK;
}

extern "C" int cudamat_solver_solve_many(cudamat_solver *s, int nrhs, const double *B, int ldb, double *X, int ldx, int precond,
                                         int loop, int maxit, double tol, int flags, cudamat_stats *st, int *form)
{
    return cudamat_solver_solve_shifts(s, nrhs, nullptr, 0, B, ldb, X, ldx, precond, loop, maxit, tol, flags, st, form);
}

// ---------------------------------------------------------------- one set of ILU(0) factors per column (shifted families)
namespace {

ColFactors col_factors(cudamat_solver *s)
{
    ManyWork &m = s->many;
    ColFactors f;
    f.lu = m.lu_b; f.lval = m.lval_b; f.uval = m.uval_b; f.dinv = m.dinv_b;
    return f;
}

// a zero pivot met while column `col` was factored on its own: the message names the column too
int zero_pivot_in_column(int col)
{
    char saved[400];
    snprintf(saved, sizeof(saved), "%s", cudamat_last_error());
    set_error("column %d: %s", col, saved);
    return CUDAMAT_ERR_ZERO_PIVOT;
}

// the ILU(0) structure these calls work on: a solver without one gets it as cudamat_solver_ilu0_shift(D_0) gives it.
// *fresh0: the solver's factors are those of column 0, just built
int cols_structure(cudamat_solver *s, const double *D, bool *fresh0)
{
    *fresh0 = false;
    if (s->has_ilu) return CUDAMAT_OK;
    const int rc = ilu0_setup(s, false, D);
    if (rc == CUDAMAT_ERR_ZERO_PIVOT) return zero_pivot_in_column(0);
    CM_TRY(rc);
    *fresh0 = true;
    return CUDAMAT_OK;
}

// column by column: the solver's own factors become those of A0 + diag(d_j) -- cudamat_solver_ilu0_shift when it holds no shifted
// factors yet, cudamat_solver_ilu0_refactor otherwise: what a caller writes today
int own_factors_of(cudamat_solver *s, const double *dj, int col, bool already)
{
    if (already) return CUDAMAT_OK;
    const bool shifted = s->has_ilu && s->ilu_shifted && !s->ilu_block;
    const int rc = shifted ? ilu0_refactor(s, dj) : ilu0_setup(s, false, dj);
    return rc == CUDAMAT_ERR_ZERO_PIVOT ? zero_pivot_in_column(col) : rc;
}

// the K-wide factorisation of one block into the factor group; *seconds: what it took (it ends drained)
int factor_block(cudamat_solver *s, const ColBlock &c, const double *D, int64_t ldd, double *seconds)
{
    CM_HIP(hipStreamSynchronize(s->ctx->stream));
    const double t0 = now_s();
    int col = 0, row = 0;
    const int rc = ilu0_numeric_cols(s, c.K, c.kc, D + (size_t)c.c0 * (size_t)ldd, ldd, col_factors(s), s->many.fzp, &col, &row);
    if (rc == CUDAMAT_ERR_ZERO_PIVOT)
        set_error("ILU(0) of A0 + diag(D_j): zero pivot in column %d, row %d", c.c0 + col, row);
    if (seconds) *seconds = now_s() - t0;
    return rc;
}

// MANY_PRECOND = auto for the per-column factors: K-wide factorisation + batched loop against kc x (refactorisation + single
// solve), the factorisation on both sides; timed once per solver and K on scratch right-hand sides with the block's own shifts.
// The column side works on the solver's own factors: their values are saved first and put back, bit for bit.
int prefer_batched_cols(cudamat_solver *s, const ColBlock &c, const double *D, int64_t ldd, bool *batched, double *t_tune)
{
    ManyWork &m = s->many;
    const double t0 = now_s();
    hipStream_t st = s->ctx->stream;
    const int n = s->n, K = c.K;
    const double *Dc = D + (size_t)c.c0 * (size_t)ldd;
    const double it = 4e7 / (double)(s->nnz + 1);
    const int N = it < 4.0 ? 4 : it > 64.0 ? 64 : (int)it;
    double &tb = m.t_cols_batch[log2_cols(K)];
    if (tb < 0.0) {
        LoopState fin[kBatchMax];
        const ColFactors f = col_factors(s);
        for (int rep = 0; rep < 2; rep++) {
            CM_TRY(launch_fill(st, (int64_t)K * n, 1.0, m.b));
            CM_TRY(launch_fill(st, (int64_t)K * n, 0.0, m.x));
            CM_HIP(hipStreamSynchronize(st));
            const double t = now_s();
            CM_TRY(factor_block(s, c, D, ldd, nullptr));
            CM_TRY(run_group(s, K, c.kc, nullptr, 0, nullptr, 0, CUDAMAT_PRECOND_ILU0, CUDAMAT_LOOP_PBICGSTAB, rep ? N : 2, 1e-8,
                             CUDAMAT_FLAG_NO_EXIT, fin, nullptr, nullptr, true, Dc, ldd, &f));      // (D holds c.kc columns)
            tb = now_s() - t;
        }
    }
    if (m.t_cols_single < 0.0) {
        IluPlans *pl = plans_of(s, false);
        DevBuf<double> lu, lv, uv, di;
        CM_TRY(lu.alloc((size_t)s->pm_nnz));
        CM_TRY(lv.alloc((size_t)s->L.nnz));
        CM_TRY(uv.alloc((size_t)s->U.nnz));
        CM_TRY(di.alloc((size_t)n));
        struct Pair { double *keep, *own; size_t count; } pairs[4] = {{lu, s->lu, (size_t)s->pm_nnz}, {lv, s->L.val, (size_t)s->L.nnz},
                                                                     {uv, s->U.val, (size_t)s->U.nnz}, {di, s->U.dinv, (size_t)n}};
        for (const Pair &p : pairs)
            if (p.count) CM_HIP(hipMemcpyAsync(p.keep, p.own, sizeof(double) * p.count, hipMemcpyDeviceToDevice, st));
        const bool was_shifted = s->ilu_shifted;
        const double was_t_factor = s->t_factor, was_seconds = pl->refactor_seconds;
        const int was_refactors = pl->refactors;
        ShiftGuard own(s);
        CM_TRY(ensure_work(s));
        CM_TRY(ensure_spmv_mode(s));
        s->d = Dc;
        int rc = CUDAMAT_OK;
        for (int rep = 0; rep < 2 && !rc; rep++) {
            rc = launch_fill(st, n, 1.0, m.b);
            if (!rc) rc = launch_fill(st, n, 0.0, m.x);
            if (!rc) rc = CM_RC(hipStreamSynchronize(st));
            const double t = now_s();
            if (!rc) rc = ilu0_refactor(s, Dc);
            cudamat_stats dummy;
            if (!rc) rc = cudamat_solver_solve(s, m.b, m.x, CUDAMAT_PRECOND_ILU0, CUDAMAT_LOOP_PBICGSTAB, rep ? N : 2, 1e-8, CUDAMAT_FLAG_NO_EXIT, &dummy);
            if (!rc) rc = CM_RC(hipStreamSynchronize(st));
            m.t_cols_single = now_s() - t;
        }
        if (rc) { m.t_cols_single = -1.0; return rc; }      // (a zero pivot here cannot be: the K-wide pass of this block had none)
        for (const Pair &p : pairs)
            if (p.count) CM_HIP(hipMemcpyAsync(p.own, p.keep, sizeof(double) * p.count, hipMemcpyDeviceToDevice, st));
        CM_HIP(hipStreamSynchronize(st));
        s->ilu_shifted = was_shifted;
        s->t_factor = was_t_factor;
        pl->refactors = was_refactors;
        pl->refactor_seconds = was_seconds;
    }
    *batched = tb < 0.97 * (double)c.kc * m.t_cols_single;
    if (s->ctx->cfg.verbose)
        fprintf(stderr, "[cudamat] per-column ILU(0): %d iterations + factorisation, single %.3f ms x %d columns, batched (K = %d) %.3f ms -> %s\n",
                N, 1e3 * m.t_cols_single, c.kc, K, 1e3 * tb, *batched ? "batched" : "columns");
    *t_tune += now_s() - t0;
    return CUDAMAT_OK;
}

// the common checks of the three entry points, and which form a call may take at all
int cols_batchable(cudamat_solver *s, int nrhs, bool loop_buffers, bool *ok)
{
    *ok = s->ctx->cfg.many_form != 2 && trsm_covered(s);
    if (*ok) CM_TRY(many_room(s, nrhs, loop_buffers, loop_buffers, ok, true));
    return CUDAMAT_OK;
}

}  // namespace

extern "C" int cudamat_solver_solve_shifts_ilu0(cudamat_solver *s, int nrhs, const double *D, int ldd, const double *B, int ldb,
                                                double *X, int ldx, int maxit, double tol, int flags, cudamat_stats *st, int *form)
{
    CM_ARG(s, "solver is NULL");
    CM_ARG(nrhs >= 0, "nrhs < 0");
    if (form) *form = 0;
    if (nrhs == 0) return CUDAMAT_OK;
    CM_ARG(D && B && X, "null pointer");
    CM_ARG(ldd >= s->n && ldb >= s->n && ldx >= s->n, "leading dimension below the rows");
    CM_ARG(maxit >= 0, "maxit");
    CM_ARG(!s->sharded && s->n_cols == s->n && s->n > 0, "ILU(0) of a shifted matrix is single-GPU, whole-matrix only");
    CM_HIP(hipSetDevice(s->ctx->device));
    const double t0 = now_s();
    const Config &cfg = s->ctx->cfg;
    const int loop = CUDAMAT_LOOP_PBICGSTAB, n = s->n;
    hipStream_t stream = s->ctx->stream;
    ShiftGuard own(s);                   // (the solver's shift is column j of D while column j is solved, and what it was afterwards)
    bool fresh0 = false;
    CM_TRY(cols_structure(s, D, &fresh0));
    const bool guarded = (flags & CUDAMAT_FLAG_GUARD) || cfg.guard;
    bool may_batch = cfg.many_precond != 0 && !(flags & (CUDAMAT_FLAG_DEBUG | CUDAMAT_FLAG_PROFILE)) && !guarded;
    if (may_batch) CM_TRY(cols_batchable(s, nrhs, true, &may_batch));
    if (!may_batch && cfg.verbose) fprintf(stderr, "[cudamat] per-column ILU(0): column by column\n");
    const std::vector<ColBlock> blocks = col_blocks(nrhs);
    double t_tune = 0.0, t_solve = 0.0;
    std::vector<char> batched(blocks.size(), 0);
    for (size_t b = 0; b < blocks.size(); b++) {
        bool yes = may_batch && ilu0_cols_covered(s, blocks[b].K);
        if (yes && cfg.many_precond == 1) CM_TRY(prefer_batched_cols(s, blocks[b], D, ldd, &yes, &t_tune));
        batched[b] = yes ? 1 : 0;
    }
    // X is written only once no column can fail any more: a single batched block factors before it writes; everything else
    // works on a copy of X, which replaces X at the end.  Column j of the copy sits where column j of X sits relative to a
    // 16-byte boundary (the single solve's vector kernels choose their form by that: the caller's loop on X, bit for bit).
    const bool staged = !(blocks.size() == 1 && batched[0]);
    DevBuf<double> xs;
    double *Xw = X;
    int64_t ldw = ldx;
    if (staged) {
        ldw = (int64_t)n + ((ldx - n) & 1);
        CM_TRY(xs.alloc((size_t)ldw * (size_t)nrhs + 2));
        Xw = xs.get() + (((uintptr_t)X >> 3) & 1);
        if (!(flags & CUDAMAT_FLAG_X0_ONES))
            for (int j = 0; j < nrhs; j++)
                CM_HIP(hipMemcpyAsync(Xw + (size_t)j * ldw, X + (size_t)j * ldx, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, stream));
    }
    std::vector<cudamat_stats> out((size_t)nrhs);
    std::vector<std::vector<double>> hists((size_t)nrhs);
    bool any_batched = false;
    for (size_t b = 0; b < blocks.size(); b++) {
        const ColBlock &c = blocks[b];
        if (batched[b]) {
            double tf = 0.0, tl = 0.0;
            CM_TRY(factor_block(s, c, D, ldd, &tf));
            const ColFactors f = col_factors(s);
            LoopState fin[kBatchMax];
            CM_TRY(run_group(s, c.K, c.kc, B + (size_t)c.c0 * ldb, ldb, Xw + (size_t)c.c0 * ldw, ldw, CUDAMAT_PRECOND_ILU0, loop, maxit,
                             tol, flags, fin, hists.data() + c.c0, &tl, true, D + (size_t)c.c0 * ldd, ldd, &f));
            t_solve += tl;
            for (int j = 0; j < c.kc; j++) {
                cudamat_stats &o = out[(size_t)(c.c0 + j)];
                fill_stats(s, fin[j], CUDAMAT_PRECOND_ILU0, &o);
                o.t_factor = tf;             // the block's K-wide factorisation
            }
            any_batched = true;
            continue;
        }
        for (int j = c.c0; j < c.c0 + c.kc; j++) {
            const double *dj = D + (size_t)j * ldd;
            cudamat_stats &sj = out[(size_t)j];
            s->d = dj;
            CM_TRY(own_factors_of(s, dj, j, fresh0 && j == 0));
            CM_TRY(cudamat_solver_solve(s, B + (size_t)j * ldb, Xw + (size_t)j * ldw, CUDAMAT_PRECOND_ILU0, loop, maxit, tol, flags, &sj));
            t_solve += sj.t_solve;
            int cnt = 0;
            std::vector<double> &h = hists[(size_t)j];
            h.assign((size_t)(s->hist_count > 0 ? s->hist_count : 0), 0.0);
            if (!h.empty()) CM_TRY(cudamat_solver_history(s, h.data(), (int)h.size(), &cnt));
        }
    }
    if (staged) {
        for (int j = 0; j < nrhs; j++)
            CM_HIP(hipMemcpyAsync(X + (size_t)j * ldx, Xw + (size_t)j * ldw, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, stream));
        CM_HIP(hipStreamSynchronize(stream));
    }
    s->many.hist_host.swap(hists);
    const double t_total = now_s() - t0;
    for (cudamat_stats &o : out) {
        o.t_solve = t_solve;
        o.t_total = t_total;
        o.t_tune += t_tune;
    }
    if (st) memcpy(st, out.data(), sizeof(cudamat_stats) * (size_t)nrhs);
    if (form) *form = any_batched ? 1 : 0;
    return CUDAMAT_OK;
}

extern "C" int cudamat_solver_precond_apply_shifts(cudamat_solver *s, int nrhs, const double *D, int ldd, const double *In, int ldin,
                                                   double *Out, int ldout)
{
    CM_ARG(s, "solver is NULL");
    CM_ARG(nrhs >= 0, "nrhs < 0");
    if (nrhs == 0) return CUDAMAT_OK;
    CM_ARG(D && In && Out, "null pointer");
    CM_ARG(ldd >= s->n && ldin >= s->n && ldout >= s->n, "leading dimension below the rows");
    CM_ARG(!s->sharded && s->n_cols == s->n && s->n > 0, "ILU(0) of a shifted matrix is single-GPU, whole-matrix only");
    CM_HIP(hipSetDevice(s->ctx->device));
    bool fresh0 = false, may_batch = false;
    CM_TRY(cols_structure(s, D, &fresh0));
    CM_TRY(cols_batchable(s, nrhs, false, &may_batch));
    ManyWork &m = s->many;
    hipStream_t st = s->ctx->stream;
    for (const ColBlock &c : col_blocks(nrhs)) {
        if (may_batch && ilu0_cols_covered(s, c.K)) {
            CM_TRY(factor_block(s, c, D, ldd, nullptr));
            CM_TRY(launch_batch_in(st, c.K, c.kc, s->n, s->n, In + (size_t)c.c0 * ldin, ldin, 0.0, m.b));
            CM_TRY(precond_apply_cols(s, c.K, col_factors(s), m.b, m.t, m.x));
            CM_TRY(launch_batch_out(st, c.K, c.kc, s->n, m.x, Out + (size_t)c.c0 * ldout, ldout));
            continue;
        }
        CM_TRY(ensure_work(s));
        for (int j = c.c0; j < c.c0 + c.kc; j++) {
            CM_TRY(own_factors_of(s, D + (size_t)j * ldd, j, fresh0 && j == 0));
            CM_TRY(precond_apply(s, In + (size_t)j * ldin, s->t, Out + (size_t)j * ldout));
        }
    }
    return CUDAMAT_OK;
}

extern "C" int cudamat_solver_ilu0_shifts_values(cudamat_solver *s, int nrhs, const double *D, int ldd, double *Out, int64_t ldo)
{
    CM_ARG(s, "solver is NULL");
    CM_ARG(nrhs >= 0, "nrhs < 0");
    if (nrhs == 0) return CUDAMAT_OK;
    CM_ARG(D && Out, "null pointer");
    CM_ARG(ldd >= s->n, "leading dimension below the rows");
    CM_ARG(!s->sharded && s->n_cols == s->n && s->n > 0, "ILU(0) of a shifted matrix is single-GPU, whole-matrix only");
    CM_HIP(hipSetDevice(s->ctx->device));
    bool fresh0 = false, may_batch = false;
    CM_TRY(cols_structure(s, D, &fresh0));
    CM_ARG(ldo >= s->pm_nnz, "leading dimension below the entries of the factors (cudamat_solver_ilu0_nnz)");
    CM_TRY(cols_batchable(s, nrhs, false, &may_batch));
    hipStream_t st = s->ctx->stream;
    for (const ColBlock &c : col_blocks(nrhs)) {
        if (may_batch && ilu0_cols_covered(s, c.K)) {
            CM_TRY(factor_block(s, c, D, ldd, nullptr));
            CM_TRY(launch_batch_out(st, c.K, c.kc, s->pm_nnz, s->many.lu_b, Out + (size_t)c.c0 * (size_t)ldo, ldo));
            continue;
        }
        for (int j = c.c0; j < c.c0 + c.kc; j++) {
            CM_TRY(own_factors_of(s, D + (size_t)j * ldd, j, fresh0 && j == 0));
            CM_HIP(hipMemcpyAsync(Out + (size_t)j * (size_t)ldo, s->lu, sizeof(double) * (size_t)s->pm_nnz, hipMemcpyDeviceToDevice, st));
        }
    }
    return CUDAMAT_OK;
}

extern "C" int cudamat_solver_history_col(cudamat_solver *s, int col, double *hist_host, int cap, int *count)
{
    CM_ARG(s && count, "null pointer");
    CM_ARG(col >= 0 && (size_t)col < s->many.hist_host.size(), "no such column in the last cudamat_solver_solve_many");
    const std::vector<double> &h = s->many.hist_host[(size_t)col];
    int c = (int)h.size() < cap ? (int)h.size() : cap;
    if (c < 0) c = 0;
    if (c > 0) {
        CM_ARG(hist_host, "hist_host is NULL");
        memcpy(hist_host, h.data(), sizeof(double) * (size_t)c);
    }
    *count = c;
    return CUDAMAT_OK;
}
