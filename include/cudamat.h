/*
 * cudamat.h -- C ABI of libcudamat_hip.so: the MI355X (gfx950) BiCGSTAB hot path.
 *
 * This is the drop-in boundary for the reference's solver path.  Every entry
 * point takes plain pointers and sizes (no C++/torch types) and returns an
 * int status (CUDAMAT_OK == 0); nothing here ever calls exit() (the reference
 * does, helper_cuda.h:999-1014).  cudamat_last_error() describes the last
 * failure on the calling thread.  There is NO CPU fallback: without a HIP
 * device every compute entry point fails with CUDAMAT_ERR_HIP.
 *
 * What each group replaces in /root/reference:
 *   cudamat_solve                 bicgstab / bicgstab / bicgstab_lu_precond
 *                                 (pbicgstab.h:113,116,119; pbicgstab.cu:157-409,
 *                                 756-922, 926-1088): host CSR in, host x out.
 *   cudamat_solver_*              the same solve with everything resident in HBM
 *                                 (what pbicgstab.cu:365-374 times as dtAlg), plus
 *                                 row-sharded multi-GPU operation through two
 *                                 caller-supplied collectives (new: the reference
 *                                 is single-GPU).
 *   cudamat_spmv                  cusparseDcsrmv      pbicgstab.cu:67,104,132,469,
 *                                                     501,528,646,676,704 (+ the
 *                                                     mult_spec diagonal term :36-42)
 *   cudamat_dot / cudamat_nrm2    cublasDdot/Dnrm2    pbicgstab.cu:74,81,106,111,...
 *   cudamat_axpy / cudamat_scal   cublasDaxpy/Dscal   pbicgstab.cu:69-70,86-88,...
 *   cudamat_ilu0 / cudamat_trsv   cusparseDcsrilu0 / cusparseDcsrsv_analysis+solve
 *                                 (via cudamat_solver_ilu0 / _precond_apply)
 *   cudamat_load_mtx              loadMMSparseMatrix  mmio_wrapper.h:133-348
 *   cudamat_to_dense_vector       toDenseVector       pbicgstab.cu:1101-1115
 *   cudamat_gen_*                 synthetic inputs of SURVEY section 8d (the
 *                                 reference's O(n^2) rand() generators,
 *                                 pbicgstab.h:32-76, cannot reach 1e7 rows)
 *
 * CSR conventions are the reference's: fp64 values, int32 indices, index base
 * taken from rowptr[0] (0 or 1, pbicgstab.cu:201), columns strictly increasing
 * inside a row (mmio_wrapper.h:123).
 */
#ifndef CUDAMAT_H
#define CUDAMAT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CUDAMAT_VERSION 1

/* status codes */
#define CUDAMAT_OK              0
#define CUDAMAT_ERR_HIP         1   /* HIP runtime / no device                      */
#define CUDAMAT_ERR_ARG         2   /* bad argument                                  */
#define CUDAMAT_ERR_ZERO_PIVOT  3   /* ILU(0): zero or structurally missing diagonal */
#define CUDAMAT_ERR_NOMEM       4
#define CUDAMAT_ERR_IO          5
#define CUDAMAT_ERR_COMM        6   /* a caller-supplied collective failed           */

/* preconditioner (cudamat_solve / cudamat_solver_solve) */
#define CUDAMAT_PRECOND_NONE    0
#define CUDAMAT_PRECOND_ILU0    1
#define CUDAMAT_PRECOND_BLOCK_ILU0 2 /* block-Jacobi: ILU(0) of each rank's diagonal block.
                                       Not in the reference (single GPU); with one rank it IS
                                       CUDAMAT_PRECOND_ILU0, with more it is a different (weaker)
                                       preconditioner with its own parity statement.            */

/* which reference loop's stopping rules to follow */
#define CUDAMAT_LOOP_PBICGSTAB  0   /* pbicgstab.cu:45-154: half-step + full-step exits
                                       against tol*||r0||, no breakdown guard           */
#define CUDAMAT_LOOP_PBICGSTAB2 1   /* pbicgstab.cu:581-754: end-of-iteration exit,
                                       |omega| < 1e-5 / NaN guard => not converged      */
#define CUDAMAT_LOOP_PIPELINED  2   /* pipelined BiCGStab (Cools & Vanroose 2017, Alg. 4): the recurrences of
                                     * LOOP_PBICGSTAB re-arranged so that both reduction phases of an iteration run
                                     * while an SpMV runs; same stopping rules and history layout;
                                     * no preconditioner; iterates equal BiCGSTAB's up to rounding              */
#define CUDAMAT_LOOP_BICGSTAB_L2 3  /* BiCGSTAB(2) (Sleijpen & Fokkema 1993, l = 2): not a reference loop.  For the systems on
                                     * which BiCGSTAB's degree-1 minimal-residual step stalls (eigenvalues far from the real
                                     * axis: convection-dominated operators).  One iteration is one SWEEP: two BiCG steps and
                                     * one degree-2 minimal-residual step = FOUR products with A^ = A M^-1 (right
                                     * preconditioning) against BiCGSTAB's two, so cudamat_stats.iters counts sweeps and one
                                     * sweep costs what two iterations of the other loops cost.  With r~ = r0 = b - A x0,
                                     * rho0 = 1, alpha = 0, omega = 1, u0 = 0 at the start:
                                     *   rho0 = -omega rho0
                                     *   j=0: rho1 = r0.r~; beta = alpha rho1/rho0; rho0 = rho1; u0 = r0 - beta u0
                                     *        u1 = A^ u0; gamma = u1.r~; alpha = rho0/gamma; r0 -= alpha u1; y += alpha u0
                                     *        r1 = A^ r0
                                     *   j=1: rho1 = r1.r~; beta = alpha rho1/rho0; rho0 = rho1; u0 = r0 - beta u0;
                                     *        u1 = r1 - beta u1; u2 = A^ u1; gamma = u2.r~; alpha = rho0/gamma
                                     *        r0 -= alpha u1; r1 -= alpha u2; y += alpha u0; r2 = A^ r1
                                     *   MR:  [[r1.r1, r1.r2], [r1.r2, r2.r2]] (g1, g2) = (r1.r0, r2.r0)
                                     *        (by elimination on r1.r1, not by Cramer's rule: exact under scaling by 2^k)
                                     *        y += g1 r0 + g2 r1; u0 -= g1 u1 + g2 u2; r0 -= g1 r1 + g2 r2; omega = g2
                                     * ||r0|| < tol ||r~|| after the MR step is the only stopping test; the history has one
                                     * entry per sweep.  With a preconditioner x = x0 + M^-1 y is formed after the loop (one
                                     * more application); without one y is x.  breakdown = 1, converged = 0 when gamma = 0,
                                     * the dividing rho0 = 0, the 2 x 2 system is singular or a scalar is not finite: the
                                     * loop stops there, the sweep is not counted.  x is then what the loop had reached:
                                     * the BiCG updates of the uncounted sweep that preceded the breakdown are in it (x and
                                     * r0 still belong together); it is not the iterate of the last counted sweep unless the
                                     * breakdown came at j = 0.  CUDAMAT_FLAG_NO_EXIT takes none of these
                                     * tests.  One GPU; PRECOND_NONE or PRECOND_ILU0; a shift as for the other loops.
                                     * CUDAMAT_ERR_ARG for sharded solvers, PRECOND_BLOCK_ILU0 and CUDAMAT_FLAG_GUARD (or
                                     * the switch GUARD).  Batched entry points run its columns one by one (form 0).     */

/* flags for cudamat_solver_solve */
#define CUDAMAT_FLAG_DEBUG      1   /* print the reference's debug lines                */
#define CUDAMAT_FLAG_PROFILE    2   /* bracket every SpMV / trsv launch with HIP events */
#define CUDAMAT_FLAG_NO_EXIT    4   /* evaluate the stopping tests but never leave:
                                       fixed-length timing windows (bench.py)           */
#define CUDAMAT_FLAG_X0_ONES    8   /* start from x0 = 1 (pbicgstab.cu:306-308,827-831)
                                       instead of the contents of x                     */
#define CUDAMAT_FLAG_GUARD      16  /* guarded solve (LOOP_PBICGSTAB / LOOP_PBICGSTAB2, one GPU):
                                       the loop restarts from the true residual b - A x when rho = rw.r has lost its last
                                       significant bit (|rho| <= GUARD_RHO_ULPS * 2^-52 * sum |rw_i r_i|, the textbook
                                       BiCGSTAB breakdown), and converged = 1 is returned only for an iterate whose TRUE
                                       residual is within twice tol * ||r0||.  Needs tol > 0 (or FLAG_NO_EXIT, which runs
                                       the guarded kernels without ever taking the test).  The switch GUARD = 1 sets it
                                       for every solve of a context.  Off by default: a departure from the reference.    */
/* (conjugate gradients for symmetric positive definite systems: its loop id and its flag are in cudamat_cg.h) */
#include "cudamat_cg.h"

typedef struct cudamat_ctx cudamat_ctx;         /* device + stream + reduction workspace  */
typedef struct cudamat_solver cudamat_solver;   /* one HBM-resident linear system          */

typedef struct cudamat_stats {
    int iters;          /* the reference loop counter on exit                            */
    int half_exit;      /* left through the half-step test (pbicgstab.cu:116)            */
    int converged;      /* a stopping test fired                                         */
    int breakdown;      /* omega guard fired (pbicgstab.cu:735)                          */
    double nrm0;        /* ||r0||                                                        */
    double nrm;         /* last residual norm the loop computed                          */
    double t_analysis;  /* s, level analysis           (pbicgstab.cu:335-347)            */
    double t_factor;    /* s, ILU(0) factorisation     (pbicgstab.cu:356-363), the factors' layout and, at the first
                         * preconditioned solve of a big system, the matrix copy in the factors' index spaces */
    double t_solve;     /* s, iteration loop = dtAlg   (pbicgstab.cu:365-374)            */
    double t_total;     /* s, whole call incl. H2D/D2H                                   */
    /* CUDAMAT_FLAG_PROFILE: device time by kernel class inside the loop                */
    double ms_spmv;     int n_spmv;
    double ms_trsv;     int n_trsv;
    int n_levels_l;     int n_levels_u;
    /* triangular-solve form this solve ended with: 0 one launch per level, 1 dependency-driven
     * launches (rows wait inside the launch), 2 one workgroup with the vector in LDS          */
    int trsv_form;
    /* solves of this solver that were discarded and redone level by level because a wait of a
     * dependency-driven launch ran into its bound (0 in a healthy run; the result is the same) */
    int trsv_fallbacks;
    /* CUDAMAT_FLAG_PROFILE on a row-sharded solver: device time of the exchanges of this solve.
     * ms_gather: the all-gathers of the SpMV inputs (on the communicator's stream when the
     * gather is overlapped); ms_gather_exposed: the part of it that was not hidden behind
     * the SpMV (all of it without overlap); hidden = ms_gather - ms_gather_exposed.         */
    int n_gather;       int n_allreduce;
    double ms_gather;   double ms_gather_exposed;   double ms_allreduce;
    int overlapped;     /* 1: the gather ran in pieces behind phase 1 of the blocked SpMV; 2: only the windows
                         * of the other slices that this rank's rows reference were exchanged (halo)            */
    int loop_form;      /* how the iterations were issued: 0 five launches each, 1 three (vector updates folded into the
                         * SpMVs, small systems), 2 the whole loop in ONE launch with grid barriers (<= 32768 short rows) */
    double gather_fraction; /* doubles received per SpMV / doubles of a whole gather ((world-1) slices)        */
    double ms_spmv_alone;  /* the selected SpMV form with its input in place, as timed when it was selected
                            * (0: never timed); an overlapped gather's exposed part is what the SpMVs of the
                            * loop took beyond this                                                            */
    int loop_fallbacks;    /* solves of this solver that were discarded and redone with the three-launch loop because a
                            * grid barrier of the single-launch loop ran into its bound (GPU shared; 0 in a healthy run) */
    int restarts;          /* how often an iterate the loop called converged failed the check of its TRUE residual (one
                            * SpMV) and the loop was restarted from it (0 in most solves, at most 3): the pipelined loop
                            * always checks, the reference loops under CUDAMAT_FLAG_GUARD                                */
    /* where a call's time went beyond t_analysis / t_factor / t_solve (the reference prints "total delta time" next to
     * "algorithm delta time", example.cpp:364-365; pbicgstab.cu:365-374):                                              */
    double t_upload;       /* s, cudamat_solve / cudamat_solve_sharded: device allocations + host-to-device copies       */
    double t_setup;        /* s, solver creation (copies, validation, CSR launch plan) + choice of the SpMV form incl. the
                            * matrix copies in other layouts; 0 when the plan of the previous call was reused            */
    double t_tune;         /* s, of t_setup: timed candidate launches (0 when the choice needed none)                    */
    int spmv_mode;         /* the SpMV form the solve used: 0 CSR forms, 1 blocked two-phase, 2 SELL-C-sigma             */
    int plan_reused;       /* cudamat_solve: 1 = the previous call brought the same matrix (pattern AND values): its solver
                            * -- device copies, SpMV plan, value dictionary, ILU(0) factors -- was reused; 0 = built anew,
                            * or -- same pattern, other values -- kept with the new values written into it
                            * (cudamat_solver_set_values; t_setup is then that call's time, t_tune 0)                     */
    /* hybrid triangular solves (big factors with wide, scattered levels): groups of consecutive levels per factor; one
     * application of L^-1 (U^-1) = `groups` dependency-driven launches over the entries inside a group + `groups - 1`
     * blocked two-phase SpMVs over the entries whose column lies in an earlier group.  0: the factor is not split.    */
    int trsv_groups_l;     int trsv_groups_u;
    int rho_restarts;      /* CUDAMAT_FLAG_GUARD: how often the test on rho fired and the solve was restarted from the true
                            * residual of its iterate (0 without the flag)                                               */
} cudamat_stats;

/* Collectives for a row-sharded solve.  Either supplied by the host program (e.g.
 * torch.distributed) or the library's own RCCL binding
 * (cudamat_rccl_comm_create below).  allgather / allreduce are enqueued on / ordered
 * with the context's stream by the callee and must not block the host longer than the
 * enqueue.  Pointers are device pointers.  Return 0 on success.
 *   allgather: every rank contributes `count` doubles; recv holds world*count.
 *   allreduce: in-place sum of `count` doubles.
 *   gather_part (optional, NULL = the gather is never overlapped): one PIECE of the
 *     all-gather.  Every rank calls it with the same (stride, offset, count): rank q's
 *     send[offset .. offset+count) must arrive at recv[q*stride + offset ..) on every
 *     OTHER rank (a rank places its own piece itself).  The exchange is enqueued on
 *     `comm_stream`, a hipStream_t owned by the communicator; the solver orders it
 *     against its own stream with events, so that phase 1 of the blocked SpMV runs on
 *     the pieces that have arrived while the next ones are in flight.                  */
typedef int (*cudamat_allgather_fn)(void *user, const double *send, double *recv, int64_t count);
typedef int (*cudamat_allreduce_fn)(void *user, double *buf, int count);
typedef int (*cudamat_gather_part_fn)(void *user, const double *send, double *recv, int64_t stride,
                                      int64_t offset, int64_t count);
/* optional: a WINDOWED gather for matrices whose rows reference only part of every other slice (banded matrices:
 * a halo).  This rank sends send[send_off[q] .. + send_cnt[q]) to rank q and receives rank q's
 * [recv_off[q] .. + recv_cnt[q]) into recv[q*stride + recv_off[q] ..); the four arrays have `world` entries
 * (host memory, valid during the call; entry `rank` is ignored; counts may be 0).  Enqueued on the context's stream. */
typedef int (*cudamat_gather_window_fn)(void *user, const double *send, double *recv, int64_t stride,
                                        const int64_t *send_off, const int64_t *send_cnt,
                                        const int64_t *recv_off, const int64_t *recv_cnt);
typedef struct cudamat_comm {
    int rank;
    int world;
    void *user;
    cudamat_allgather_fn allgather;
    cudamat_allreduce_fn allreduce;
    cudamat_gather_part_fn gather_part;   /* may be NULL */
    void *comm_stream;                    /* hipStream_t gather_part enqueues on (NULL with gather_part NULL) */
    /* optional: allreduce enqueued on `reduce_stream` (a third stream of the communicator) instead of the
     * context's stream, so that CUDAMAT_LOOP_PIPELINED can run a reduction while an SpMV runs              */
    cudamat_allreduce_fn allreduce_side;  /* may be NULL: the pipelined loop then reduces on its own stream */
    void *reduce_stream;
    cudamat_gather_window_fn gather_window;   /* may be NULL: every SpMV input is gathered whole */
} cudamat_comm;

/* ---- the library's own communicator: RCCL over xGMI, bound at run time ---------------- */
/* (csrc/comm_rccl.hip; the reference has no counterpart: single device, pbicgstab.cu:223-240)
 * One rank per GPU, as threads of one process (host/example.cpp -G<n>) or as processes
 * (bench.py under torch.distributed.run).  Rank 0 makes an id and hands its bytes to the
 * other ranks by whatever channel the host program has; every rank then creates its
 * communicator (collective: returns when all `world` ranks have joined), passes it to
 * cudamat_solver_set_comm and destroys it after the solver.  The collectives run on the
 * context's stream, the pieces of an overlapped gather on a stream the communicator owns.  */
#define CUDAMAT_RCCL_ID_BYTES 384
int cudamat_rccl_available(void);                  /* 1 when librccl could be loaded */
int cudamat_rccl_unique_id(void *id);              /* fills CUDAMAT_RCCL_ID_BYTES bytes */
int cudamat_rccl_comm_create(cudamat_ctx *ctx, const void *id, int rank, int world, cudamat_comm *out);
int cudamat_rccl_comm_destroy(cudamat_comm *comm);
/* Tear the communicator down without waiting for its streams: for a rank that failed while its peers wait inside a
 * collective (every rank of the job aborts, then destroys).  Any thread; idempotent; destroy must still follow.      */
int cudamat_rccl_comm_abort(cudamat_comm *comm);

/* A communicator whose exchanges are SKIPPED (streams and call sequence are real): times one rank's share of a
 * sharded solve on a single GPU (scripts/rank_probe.py).  The iterates of such a solve are meaningless.        */
int cudamat_comm_dry_create(cudamat_ctx *ctx, int rank, int world, cudamat_comm *out);
int cudamat_comm_dry_destroy(cudamat_comm *comm);

int         cudamat_version(void);
const char *cudamat_last_error(void);
int         cudamat_device_count(int *count);

/* ---- context ------------------------------------------------------------------ */
/* stream: a hipStream_t created by the caller (e.g. torch's current stream) or
 * NULL to let the context create and own one.                                       */
int cudamat_ctx_create(int device, void *stream, cudamat_ctx **out);
int cudamat_ctx_destroy(cudamat_ctx *ctx);
/* Switches (testing / probing; the defaults are what ships).  A context reads CUDAMAT_<NAME> from the environment ONCE,
 * when it is created; afterwards a switch changes only through this call (name with or without the CUDAMAT_ prefix,
 * value as it would stand in the environment).  Whatever runs on the context after the call sees the new value: set
 * SpMV-form switches before the first use of a solver, ILU(0) ones before cudamat_solver_ilu0, loop ones before
 * cudamat_solver_solve.  CUDAMAT_ERR_ARG for an unknown name or a value outside the option's range.  cudamat_solve and
 * cudamat_solve_sharded (no caller-made context) read the environment per call.  cudamat_options_help(): one line per
 * switch -- name, accepted values, meaning (the table of csrc/config.cpp).                                            */
int cudamat_ctx_set_option(cudamat_ctx *ctx, const char *name, const char *value);
int cudamat_ctx_reset_options(cudamat_ctx *ctx);   /* back to what a context created now would hold (defaults + environment) */
const char *cudamat_options_help(void);
int cudamat_option_check(const char *name, const char *value);   /* CUDAMAT_OK when cudamat_ctx_set_option would accept the pair (no device needed) */
int cudamat_ctx_sync(cudamat_ctx *ctx);
int cudamat_ctx_stream(cudamat_ctx *ctx, void **stream);

/* device memory for hosts without an allocator of their own                         */
int cudamat_malloc(cudamat_ctx *ctx, size_t bytes, void **dev);
int cudamat_free(cudamat_ctx *ctx, void *dev);
int cudamat_h2d(cudamat_ctx *ctx, void *dev, const void *host, size_t bytes);
int cudamat_d2h(cudamat_ctx *ctx, void *host, const void *dev, size_t bytes);
int cudamat_d2d(cudamat_ctx *ctx, void *dst, const void *src, size_t bytes);   /* async, stream-ordered */
int cudamat_memset(cudamat_ctx *ctx, void *dev, int value, size_t bytes);

/* stream-ordered timers (HIP events on the context's stream)                        */
int cudamat_timer_create(cudamat_ctx *ctx, void **timer);
int cudamat_timer_start(cudamat_ctx *ctx, void *timer);
int cudamat_timer_stop(cudamat_ctx *ctx, void *timer);
int cudamat_timer_elapsed_ms(cudamat_ctx *ctx, void *timer, double *ms);  /* syncs */
int cudamat_timer_destroy(cudamat_ctx *ctx, void *timer);

/* ---- elementary kernels on device pointers ------------------------------------- */
/* y = alpha*(A x + d .* x) + beta*y ; d may be NULL ; base = index base of rowptr /
 * colidx (they are read as given).  n rows; x has as many entries as A has columns. */
int cudamat_spmv(cudamat_ctx *ctx, int n, const int *rowptr, const int *colidx,
                 const double *val, int base, double alpha, const double *x,
                 const double *d, double beta, double *y);
/* *out_dev = sum x_i y_i (device scalar, fixed reduction order => reproducible)     */
int cudamat_dot(cudamat_ctx *ctx, int64_t n, const double *x, const double *y, double *out_dev);
/* *out_dev = sqrt(sum x_i^2)                                                        */
int cudamat_nrm2(cudamat_ctx *ctx, int64_t n, const double *x, double *out_dev);
int cudamat_axpy(cudamat_ctx *ctx, int64_t n, double alpha, const double *x, double *y);
int cudamat_scal(cudamat_ctx *ctx, int64_t n, double alpha, double *x);

/* ---- HBM-resident system --------------------------------------------------------- */
/* Local row block of a (possibly row-sharded) square system.
 *   n_local : rows owned by this rank (== n for a single GPU)
 *   n_cols  : number of columns = global dimension
 *   rowptr/colidx/val : DEVICE pointers, base taken from `base`; they are copied
 *   (and rebased to 0) into the solver's own HBM arrays, so the caller may free them.
 * Work vectors and the reduction workspace are allocated here, once.
 * The arrays are validated on the device: row pointers that are not monotone from base to base + nnz or a
 * column outside [base, base + n_cols) => CUDAMAT_ERR_ARG.  Rows whose columns are not strictly increasing
 * are accepted for the un-preconditioned loops (lanes-per-row / tile SpMV); ILU(0) refuses them.        */
int cudamat_solver_create(cudamat_ctx *ctx, int n_local, int64_t n_cols, int64_t nnz,
                          const int *rowptr, const int *colidx, const double *val,
                          int base, cudamat_solver **out);
/* The same from HOST arrays (any pageable memory): creation runs beside the upload -- validation and the SpMV plan start
 * when the row pointers and column indices have landed, a blocked copy is filled behind the values.
 * rowptr[0] must equal base.                                                                                           */
int cudamat_solver_create_host(cudamat_ctx *ctx, int n_local, int64_t n_cols, int64_t nnz,
                               const int *rowptr_host, const int *colidx_host, const double *val_host,
                               int base, cudamat_solver **out);
int cudamat_solver_destroy(cudamat_solver *s);
/* (A0 + diag(d)) variant, pbicgstab.h:116; d is a device vector of n_local doubles
 * that must stay alive; NULL removes it.  A solver with a shift takes CUDAMAT_PRECOND_ILU0 only with factors built by
 * cudamat_solver_ilu0_shift (loops CUDAMAT_LOOP_PBICGSTAB / _PBICGSTAB2; any other combination is CUDAMAT_ERR_ARG): the
 * factors of A0 alone are never used, or built, silently in their place.  The shift of the factors and this one are
 * independent: factors built with one d may precondition a solve with another (a weaker, still valid M).           */
int cudamat_solver_set_shift(cudamat_solver *s, const double *d);
/* ILU(0) of the local block sharing A's pattern + level analysis of L and U
 * (pbicgstab.cu:336-359).  Single rank only.  A second call (of this or of _ilu0_shift) starts the set-up over;
 * cudamat_solver_ilu0_refactor keeps it and recomputes the values only.                                            */
int cudamat_solver_ilu0(cudamat_solver *s);
/* The same for A0 + diag(d_factor): d_factor (device, n_local doubles) is added to the copied diagonal values, one rounding
 * each, before the factorisation; it is read during the call only and has nothing to do with set_shift.  An explicit zero
 * on A0's diagonal is fine when the shifted pivot is not zero; a diagonal entry missing from the pattern stays an error.
 * NULL: cudamat_solver_ilu0.  Single GPU, whole matrix only (no block-Jacobi or sharded variant).                    */
int cudamat_solver_ilu0_shift(cudamat_solver *s, const double *d_factor);
/* *yes = 1 when the solver's factors came from cudamat_solver_ilu0_shift with a non-NULL d_factor, else 0 (after a
 * refactorisation: whether the last one had a non-NULL d_factor)                                                       */
int cudamat_solver_ilu0_shifted(cudamat_solver *s, int *yes);
/* Numeric-only refactorisation: the VALUES of the factors the solver holds become those of A0 + diag(d_factor) (device,
 * n_local doubles, read during the call only; NULL: those of A0).  Everything that depends on the pattern alone is kept --
 * the level analysis, the far / near split and its blocked copies' structure, the permutation maps, the chosen solve forms
 * and, when already built, the permuted copy of the matrix -- so the result is bit-identical to a fresh
 * cudamat_solver_ilu0_shift(d_factor) on the same matrix and switches, at a fraction of its cost.  Any transition is allowed
 * (A0 -> d, d -> d', d -> A0, A0 -> A0).  Split factors keep one int per stored entry from the first call on (see
 * _refactor_info); unsplit ones need nothing.  CUDAMAT_ERR_ARG: no factors yet, block-Jacobi factors, a sharded solver.
 * CUDAMAT_ERR_ZERO_PIVOT leaves the solver without factors, as a failed set-up does.                                   */
int cudamat_solver_ilu0_refactor(cudamat_solver *s, const double *d_factor);
/* Without touching the device: *count = refactorisations the current factors have seen since their set-up, *seconds_last =
 * wall time of the last one (stream drained), *map_bytes = device bytes of the value maps (0 before the first
 * refactorisation and for unsplit factors).  Any of the three may be NULL.                                             */
int cudamat_solver_ilu0_refactor_info(cudamat_solver *s, int *count, double *seconds_last, size_t *map_bytes);
/* New VALUES for the resident matrix on the structure the solver holds: val (device, nnz doubles in the CSR order of the
 * creation) is read during the call only, and the call ends with the stream drained.  Afterwards the solver shows what a
 * solver created from (rowptr, colidx, val) under the same switches shows, bit for bit wherever that solver runs the same
 * kernels: products (spmv, spmm, spmm_shifts), every loop form of solve / solve_many / solve_shifts and -- once the factors
 * have been brought up to date -- the preconditioned ones.  Everything that depends on the pattern alone is kept: validation,
 * launch plans, compressed indices, the blocked copy's geometry and placement, the chosen SpMV form and the timings behind
 * it, the set-up of ILU(0).  Every copy of the values is refreshed in place; the blocked copies go through a map of one int
 * per stored entry that the first call builds (see _info).  A copy holds fp64 values or 8-bit indices into the value
 * dictionary; when the new values change that (a dictionary appears or disappears) nothing is converted -- the copies are
 * dropped and the form is chosen again at the next use, as in a new solver.
 * The ILU(0) / block-Jacobi factors are NOT touched: they remain those of the old values, a lagged preconditioner that a
 * solve may still use, until cudamat_solver_ilu0_refactor (or _ilu0 / _ilu0_shift / _block_ilu0) recomputes them from the
 * new matrix.  The shift, the work vectors, the histories and the batched loop's form choice stay.
 * One GPU, whole matrix: CUDAMAT_ERR_ARG for a sharded solver and for a NULL val; the solver is unchanged then.           */
int cudamat_solver_set_values(cudamat_solver *s, const double *val);
/* Without touching the device: *count = calls since the creation, *seconds_last = wall time of the last one (stream drained),
 * *map_bytes = device bytes of the value maps the solver holds (0 before the first call and for forms that need none),
 * *rebuilt_last = 1 when the last call changed the storage class and the SpMV form is chosen again.  Any may be NULL.     */
int cudamat_solver_set_values_info(cudamat_solver *s, int *count, double *seconds_last, size_t *map_bytes, int *rebuilt_last);
/* Is the matrix the solver holds symmetric?  *unmatched = stored off-diagonal entries (i, j) without a stored (j, i),
 * *max_abs_diff = max |a_ij - a_ji| over the stored pairs (inf where a difference is NaN).  (0, 0.0): symmetric, pattern and
 * values.  Exact: no tolerance; a shift (cudamat_solver_set_shift) sits on the diagonal and does not enter.  One pass over the
 * entries on the device at the first call; the verdict is kept until cudamat_solver_set_values.  Either pointer may be NULL.
 * CUDAMAT_ERR_ARG for a sharded solver and for a matrix whose rows are not strictly increasing in their columns.            */
int cudamat_solver_symmetry(cudamat_solver *s, long long *unmatched, double *max_abs_diff);
/* the same on the rank's DIAGONAL BLOCK (rows and columns it owns) -- allowed in a sharded solver;
 * no collective is involved, neither here nor in the preconditioning steps            */
int cudamat_solver_block_ilu0(cudamat_solver *s);
/* copies the LU values (nnz doubles, same ordering as val; for the block variant: the
 * entries of the diagonal block in row order) to a device buffer                       */
int cudamat_solver_ilu0_values(cudamat_solver *s, double *out_dev);
/* how many values that is (nnz, or the entry count of the diagonal block)                */
int cudamat_solver_ilu0_nnz(cudamat_solver *s, int64_t *count);
/* which triangular-solve kernels the next preconditioning step uses: 1 = dependency-driven (one launch per
 * group of levels, rows wait for their dependencies inside the launch), 0 = one launch per level.  The first
 * form assumes no OTHER spin-waiting kernel shares the GPU (one stream per GPU); its waits are bounded, and a
 * solve that sees a timeout is redone with the second form, which then stays selected.                      */
int cudamat_solver_trsv_form(cudamat_solver *s, int *form);
/* out = U^-1 L^-1 in  (what one preconditioning step applies, pbicgstab.cu:92-98)     */
int cudamat_solver_precond_apply(cudamat_solver *s, const double *in, double *out);
/* row-sharded operation; comm is copied.  world == 1 or NULL => single GPU (unless the
 * environment sets CUDAMAT_FORCE_SHARDED=1, which keeps the collective path for testing). */
int cudamat_solver_set_comm(cudamat_solver *s, const cudamat_comm *comm);
/* which SpMV implementation the analysis chose for this matrix: 0 = one group of lanes per row on
 * the CSR arrays, 1 = blocked two-phase kernels (x / y tiles in LDS); decided at the first use.   */
int cudamat_solver_spmv_mode(cudamat_solver *s, int *mode);
/* Value dictionary: *distinct = number of distinct fp64 bit patterns among the matrix values when the SELECTED SpMV form
 * reads 8-bit indices into a dictionary of them instead of the 8-byte values (large matrices with at most 256 distinct
 * values; results are bit-identical, HBM traffic drops by 7 bytes per entry), 0 when it reads the values themselves.
 * The switch VALUE_DICT = 0 (cudamat_ctx_set_option / CUDAMAT_VALUE_DICT in the environment) disables the dictionary. */
int cudamat_solver_value_dict(cudamat_solver *s, int *distinct);
/* name(s) of the HIP kernel(s) one SpMV launch of this solver runs (e.g. "k_pb_phase1 + k_pb_phase2", "k_spmv_stream_c<256>",
 * "k_spmv<32>"): what a rocprofv3 kernel trace of the loop shows, for the bench line's `roofline.kernel`            */
int cudamat_solver_spmv_kernel(cudamat_solver *s, char *name, int cap);
/* Where the blocked copy's arrays went (round 5, csrc/spmv_pb.hip): device memory comes in classes, and a kernel that reads one
 * array while it writes another loses 5-7 % when both lie in one class, so the product stream of a large copy is placed in a
 * class of its own.  *placed: 1 placed, 0 searched without finding an arrangement, -1 not tried (another SpMV form, a copy
 * below 2 GB of products, PB_PLACE = 0, a drop-in call without PB_PLACE = 2); *slabs: 16 GB slabs classified; *seconds: what
 * the search took; classes: their 2 GB blocks by class ("00000000 11112222"), then the final check's timing (values read beside
 * writes into the product stream) between the fastest and slowest pair met, at most cap - 1 characters.            */
int cudamat_solver_placement(cudamat_solver *s, int *placed, int *slabs, double *seconds, char *classes, int cap);
/* y_local = (A + diag(d)) x ; x is the LOCAL slice, gathered through comm if sharded  */
int cudamat_solver_spmv(cudamat_solver *s, const double *x_local, double *y_local);
/* Solve.  b, x: device vectors of n_local doubles; x holds the initial guess on entry
 * (unless CUDAMAT_FLAG_X0_ONES) and the solution on return.                           */
int cudamat_solver_solve(cudamat_solver *s, const double *b, double *x, int precond,
                         int loop, int maxit, double tol, int flags, cudamat_stats *st);
/* residual-norm history of the last solve: LOOP_PBICGSTAB: hist[2i], hist[2i+1] =
 * norm after the half / full step of iteration i; LOOP_PBICGSTAB2: hist[i].  (LOOP_PIPELINED
 * as LOOP_PBICGSTAB.  When a solve was restarted -- after the check of its true residual,
 * cudamat_stats.restarts, or under CUDAMAT_FLAG_GUARD after the test on rho, cudamat_stats.rho_restarts --
 * the segments follow one another.)
 * Copies min(cap, available) doubles to the HOST buffer, returns the count in *count. */
int cudamat_solver_history(cudamat_solver *s, double *hist_host, int cap, int *count);

/* ---- several right-hand sides for one resident system (DESIGN.md section "Several right-hand sides") ------------------ */
/* Y = (A + diag(d)) X for nrhs columns, column-major device blocks (leading dimensions ldx >= n_cols, ldy >= n_local).  Up
 * to 8 columns share one pass over the matrix (CSR SpMM with the solver's lanes per row); column j is bit-identical to
 * cudamat_solver_spmv of column j with the lanes-per-row CSR kernel.  nrhs == 0 is a no-op.                             */
int cudamat_solver_spmm(cudamat_solver *s, int nrhs, const double *X, int ldx, double *Y, int ldy);
/* Solve for nrhs right-hand sides B (column-major, ldb >= n) into X (column-major, ldx >= n; the initial guesses on entry
 * unless CUDAMAT_FLAG_X0_ONES).  Every column is an independent run of cudamat_solver_solve's loop with its own scalars,
 * stopping tests and history.  PRECOND_NONE with LOOP_PBICGSTAB / LOOP_PBICGSTAB2 on one GPU may run batched (up to 8
 * columns per launch; a column's result then depends on its own data only, not on the batch); so may PRECOND_ILU0 with
 * LOOP_PBICGSTAB when the switch MANY_PRECOND = batched | auto asks for it (default: columns) and the factors are covered
 * (see cudamat_solver_precond_apply_many); everything else -- CUDAMAT_FLAG_GUARD included: each column is then a guarded
 * solve --, and the switch MANY_FORM = columns, runs cudamat_solver_solve once per column.  MANY_FORM = auto (default) times both forms at the
 * first such call of the solver (per loop and batch width) and takes the faster.  st: nrhs entries or NULL -- per column
 * iters, half_exit, converged, breakdown, nrm0, nrm, spmv_mode; t_solve / t_total are those of the whole call, t_tune
 * includes the timing of the form choice.  *form (may be NULL): 1 when columns ran batched, 0 column by column.        */
int cudamat_solver_solve_many(cudamat_solver *s, int nrhs, const double *B, int ldb, double *X, int ldx, int precond,
                              int loop, int maxit, double tol, int flags, cudamat_stats *st, int *form);
/* Out_j = U^-1 L^-1 In_j for nrhs columns, column-major device blocks (ldin, ldout >= n_local): what cudamat_solver_precond_apply
 * does, for up to 8 columns per pass over the factors (multi-column level-scheduled triangular solves: one gathered index
 * yields 8 contiguous values, one level serves all columns).  Column j is bit-identical to cudamat_solver_precond_apply of
 * column j, whatever nrhs is.  Factors the multi-column kernels do not cover (hybrid factors in level-major spaces, block-Jacobi
 * ILU(0), sharded solvers) are applied column by column.  Needs cudamat_solver_ilu0 first; nrhs == 0 is a no-op.        */
int cudamat_solver_precond_apply_many(cudamat_solver *s, int nrhs, const double *In, int ldin, double *Out, int ldout);
/* name(s) of the HIP kernel(s) that call launches per factor for a batch of nrhs (<= 8) columns, e.g.
 * "L: k_trsm_lds<8, 8>; U: k_trsm_level<16, 8> + k_trsm_small_levels<16, 8>"; "" when the factors run column by column   */
int cudamat_solver_trsm_kernel(cudamat_solver *s, int nrhs, char *name, int cap);
/* One shift vector per column: column j is (A0 + diag(D_j)) with D a column-major device block (ldd >= n_local, D_j its column
 * j), the matrix shared.  For the length of the call D REPLACES the solver's own shift (cudamat_solver_set_shift), which is
 * what it was when the call returns, on every error path too.  D == NULL: exactly cudamat_solver_spmm / _solve_many.
 * cudamat_solver_spmm_shifts: Y_j = (A0 + diag(D_j)) X_j; up to 8 columns share one pass over the matrix, and column j is
 * bit-identical to cudamat_solver_spmm (so to the lanes-per-row cudamat_solver_spmv) of column j after set_shift(D_j).
 * cudamat_solver_solve_shifts: (A0 + diag(D_j)) x_j = b_j, everything else as cudamat_solver_solve_many (statistics, histories,
 * *form, MANY_FORM -- auto times both forms with shifts in place, once per solver, loop and batch width).  The batched form
 * covers what it covers there; the rest (MANY_FORM = columns, LOOP_PIPELINED, sharded solvers -- D then holds the local rows --,
 * FLAG_DEBUG / FLAG_PROFILE / FLAG_GUARD, no room for the buffers) runs set_shift(D_j) + cudamat_solver_solve per column, bit for bit.  The
 * (A0 + I d) variant has no preconditioner (pbicgstab.h:110): precond != CUDAMAT_PRECOND_NONE with D is CUDAMAT_ERR_ARG.      */
int cudamat_solver_spmm_shifts(cudamat_solver *s, int nrhs, const double *X, int ldx, const double *D, int ldd, double *Y,
                               int ldy);
int cudamat_solver_solve_shifts(cudamat_solver *s, int nrhs, const double *D, int ldd, const double *B, int ldb, double *X,
                                int ldx, int precond, int loop, int maxit, double tol, int flags, cudamat_stats *st, int *form);
/* The shifted family WITH a preconditioner: (A0 + diag(D_j)) x_j = b_j by the reference loop (CUDAMAT_LOOP_PBICGSTAB), M_j the
 * ILU(0) of A0 + diag(D_j) -- one set of factors per column.  (cudamat_solver_solve_shifts and _solve_many keep their refusals.)
 * Blocks of at most 8 columns.  Batched form: the block's K factorisations run as ONE K-wide numeric ILU(0) on the solver's
 * ILU(0) structure (pattern, levels and searches are shared, values interleaved), then the batched loop with the multi-column
 * triangular solves reading one value per column; column j's factors, iterate and history are bit-identical to
 * cudamat_solver_ilu0_shift(D_j) + set_shift(D_j) + the same call with nrhs = 1.  st[j].t_factor: the block's factorisation.
 * Form: MANY_PRECOND = columns (default) | batched | auto (times both, each side with its factorisation), MANY_FORM = columns
 * overrides.  Batched needs factors in the original index space on one GPU (see cudamat_solver_precond_apply_many), every
 * row within the LDS limit of the K-wide factorisation (7616 / 5376 / 3392 / 1920 entries for blocks of 1 / 2 / 4 / 8 columns),
 * room for the buffers, and none of FLAG_DEBUG / _PROFILE / _GUARD.  Everything else runs column by column, per column what a
 * caller writes today: set_shift(D_j); cudamat_solver_ilu0_shift(D_j) while the solver holds no shifted factors, else
 * cudamat_solver_ilu0_refactor(D_j); cudamat_solver_solve(CUDAMAT_PRECOND_ILU0) -- bit for bit.
 * State the call leaves: the solver's own shift is what it was, on every path.  A solver without ILU(0) structure gets it as
 * cudamat_solver_ilu0_shift(D_0) gives it.  Batched: the values of factors the solver already held are untouched bit for bit
 * (the per-column factors live in scratch and are not kept across calls).  Column by column: the solver's factors are those of
 * the last column, as after the caller's loop.
 * A zero pivot in any column: CUDAMAT_ERR_ZERO_PIVOT, the message names column and row, X is untouched (a call that is not one
 * batched block iterates on a copy of X, n x nrhs doubles, which replaces X at the end).  In the batched form the factors the
 * solver held beforehand stay valid; column by column a zero pivot leaves the solver as cudamat_solver_ilu0_refactor does,
 * without factors.  nrhs == 0 is a no-op; *form (may be NULL): 1 when any block ran batched.                              */
int cudamat_solver_solve_shifts_ilu0(cudamat_solver *s, int nrhs, const double *D, int ldd, const double *B, int ldb, double *X,
                                     int ldx, int maxit, double tol, int flags, cudamat_stats *st, int *form);
/* Out_j = U_j^-1 L_j^-1 In_j with the ILU(0) factors of A0 + diag(D_j): column j is bit-identical to
 * cudamat_solver_precond_apply on a solver that holds cudamat_solver_ilu0_shift(D_j).  K-wide (the solver's own factor values
 * untouched) wherever the batched form above is possible -- MANY_FORM = columns overrides, MANY_PRECOND is not asked --, else
 * column by column through the solver's own factors, which are then those of the last column.                              */
int cudamat_solver_precond_apply_shifts(cudamat_solver *s, int nrhs, const double *D, int ldd, const double *In, int ldin,
                                        double *Out, int ldout);
/* column j of Out (device, column-major, ldo >= cudamat_solver_ilu0_nnz) = what cudamat_solver_ilu0_values returns after
 * cudamat_solver_ilu0_shift(D_j), bit for bit; forms as cudamat_solver_precond_apply_shifts                               */
int cudamat_solver_ilu0_shifts_values(cudamat_solver *s, int nrhs, const double *D, int ldd, double *Out, int64_t ldo);
/* residual history of column `col` of the last cudamat_solver_solve_many / _solve_shifts / _solve_shifts_ilu0, laid out as cudamat_solver_history's */
int cudamat_solver_history_col(cudamat_solver *s, int col, double *hist_host, int cap, int *count);

/* ---- drop-in host-pointer solve ---------------------------------------------------- */
/* One call = what the three reference entry points do: upload, (analyse, factor,)
 * iterate, download.  d / x0 may be NULL (x0 NULL => ones).  x receives the iterate
 * even when not converged.  Returns CUDAMAT_OK whenever the solve ran; convergence
 * is reported in st (may be NULL).                                                    */
int cudamat_solve(int n, int nnz, const double *A, const int *iA, const int *jA,
                  const double *d, const double *x0, const double *b, int precond,
                  int loop, int maxit, double tol, int debug, double *x,
                  cudamat_stats *st);

/* cudamat_solve for nrhs right-hand sides: B (ldb >= n) and X (ldx >= n) column-major in HOST memory; x0 (NULL => ones)
 * laid out as X; d may be NULL.  The solve is cudamat_solver_solve_many on the solver cudamat_solve keeps (the same plan
 * cache: a second call with the same matrix reuses it, st[j].plan_reused).  Arguments are checked before any device is
 * touched; nrhs == 0 is a successful no-op.  st: nrhs entries or NULL; *form as cudamat_solver_solve_many.              */
int cudamat_solve_many(int n, int nnz, const double *A, const int *iA, const int *jA, const double *d, int nrhs,
                       const double *B, int ldb, const double *x0, double *X, int ldx, int precond, int loop, int maxit,
                       double tol, cudamat_stats *st, int *form);

/* cudamat_solve_many for a family of shifted systems (A0 + diag(D_j)) x_j = b_j: D (ldd >= n) column-major in HOST memory like
 * B, one shift vector per column, uploaded beside B; no preconditioner (pbicgstab.h:110).  The plan cache compares the matrix,
 * not the shifts: a second call with the same A0 and other shifts reuses the plan (st[j].plan_reused = 1).                 */
int cudamat_solve_shifts(int n, int nnz, const double *A0, const int *iA0, const int *jA0, int nrhs, const double *D, int ldd,
                         const double *B, int ldb, const double *x0, double *X, int ldx, int loop, int maxit, double tol,
                         cudamat_stats *st, int *form);

/* cudamat_solve_shifts with the ILU(0) of A0 + diag(D_j) as column j's preconditioner (cudamat_solver_solve_shifts_ilu0 on the
 * kept solver: the reference loop, the same plan cache, the same form rules).  Arguments are checked before any device is
 * touched; nrhs == 0 is a successful no-op.                                                                                 */
int cudamat_solve_shifts_ilu0(int n, int nnz, const double *A0, const int *iA0, const int *jA0, int nrhs, const double *D, int ldd,
                              const double *B, int ldb, const double *x0, double *X, int ldx, int maxit, double tol,
                              cudamat_stats *st, int *form);

/* cudamat_solve keeps the solver of its LAST call (CSR copies, SpMV plan, ILU(0) factors: device memory on device 0 --
 * about 16 GB at 1e7 rows x 50 entries, 50 GB with ILU(0)) so that a caller who solves with the same matrix again --
 * time steps, several right-hand sides: the reference's per-call shape, pbicgstab.cu:157-409 -- pays the upload and a
 * device-side comparison but no analysis.  The next call with a different matrix (or different CUDAMAT_* switches)
 * replaces it; a call that runs out of device memory releases it and tries once more; cudamat_solve_sharded releases
 * it before it starts; cudamat_plan_cache_clear() (or CUDAMAT_PLAN_CACHE=0 in the environment) releases / disables it.  */
int cudamat_plan_cache_clear(void);

/* Device memory of this library comes from a recycling pool (csrc/pool.cpp): what a solver, a context or
 * cudamat_plan_cache_clear() frees stays with the library and serves its later requests -- on this platform a fresh
 * hipMalloc is not uniformly cheap (0.3 ms for 8 GB, but 26 ms per GB on some boxes once a process holds more than ~40 GB,
 * and seconds for single calls), and a host program that solves system after system would pay that every time.  The pool
 * keeps at most 96 GB free per device and empties itself when an allocation would fail.  cudamat_pool_trim() hands every
 * free block back to the driver -- for a host program that shares the device with other allocators; CUDAMAT_POOL=0 (read
 * once per process) turns the pool off.  The reference allocates and frees per call (pbicgstab.cu:243-255,392-405).   */
int cudamat_pool_trim(void);
/* what the driver reports free / in total on `device` (hipMemGetInfo) and, of the memory the driver counts as used, how
 * much the library's pool could hand out again without asking it; any pointer may be NULL */
int cudamat_mem_info(int device, size_t *driver_free, size_t *driver_total, size_t *pool_free);
/* device allocations of this library that are in use, over all devices of the process: every allocation counts one,
 * small, pooled or with CUDAMAT_POOL=0, until it is freed (a block still in the pool's free list does not count).  Equal
 * before and after a piece of work that destroyed everything it created: nothing leaked.  Pinned host memory is not
 * counted. */
int cudamat_mem_live(size_t *allocations);

/* The same solve over `ngpu` GPUs of this node, from one process: uniform row blocks, one host
 * thread and one RCCL rank per device (csrc/sharded.cpp).  precond: NONE or BLOCK_ILU0 (each
 * rank's diagonal block; ILU0 of the whole matrix does not shard => CUDAMAT_ERR_ARG).
 * ngpu <= 1 is cudamat_solve.  st receives rank 0's statistics (all ranks decide alike).     */
int cudamat_solve_sharded(int ngpu, int n, int nnz, const double *A, const int *iA, const int *jA,
                          const double *d, const double *x0, const double *b, int precond,
                          int loop, int maxit, double tol, int debug, double *x,
                          cudamat_stats *st);

/* ---- synthetic inputs, generated in HBM ------------------------ */
int64_t cudamat_poisson5_nnz(int nx, int ny);
int cudamat_gen_poisson5(cudamat_ctx *ctx, int nx, int ny, int64_t row0, int64_t row1,
                         int base, int *rowptr, int *colidx, double *val);
int cudamat_rand_row_nnz(int64_t n, int per_row);
int cudamat_gen_rand_rows(cudamat_ctx *ctx, int64_t n, int per_row, uint64_t seed,
                          int64_t row0, int64_t row1, int base, int *rowptr,
                          int *colidx, double *val);
int cudamat_gen_xstar(cudamat_ctx *ctx, int64_t i0, int64_t i1, uint64_t seed, double *x);

/* ---- Matrix Market I/O (host only) -------------------------------------------------- */
/* semantics of loadMMSparseMatrix(filename,'d',csr,...) mmio_wrapper.h:133-348:
 * returns 0 ok / CUDAMAT_ERR_IO; outputs are malloc'd, release with cudamat_host_free
 * (or free()).                                                                        */
int cudamat_load_mtx(const char *filename, int csr_format, int *m, int *n, int *nnz,
                     double **val, int **row, int **col);
void cudamat_host_free(void *p);
void cudamat_to_dense_vector(int n, int nnz, const double *A, const int *IA, double *out);

#ifdef __cplusplus
}
#endif
#endif /* CUDAMAT_H */
