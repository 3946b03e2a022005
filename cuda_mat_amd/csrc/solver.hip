// solver.hip -- the HBM-resident system behind cudamat_solver_*: creation, the choice of the SpMV form, the sharded
// SpMV (exchange + multiply), the set-up agreement of the ranks.  The iteration loops live in loops.hip, the host-pointer
// drop-in entry point in dropin.hip.
//
// The BiCGSTAB driver as a whole: one host loop that only ENQUEUES work.
//
// Reference behaviour restated (citations into /root/reference):
//   CUDAMAT_LOOP_PBICGSTAB  = gpu_pbicgstab  pbicgstab.cu:45-154  (ILU(0) or M = I)
//   CUDAMAT_LOOP_PBICGSTAB2 = gpu_pbicgstab2 pbicgstab.cu:581-754 (d variant; with
//                             d == NULL the intended maths of :425-578)
// MI355X-first differences from the reference's structure:
//   * the reference blocks the host 5-6 times per iteration on cuBLAS scalar
//     results; here rho/alpha/omega/norms stay in HBM (LoopState), kernels read
//     them in their prologue, and the host only looks at a snapshot that is
//     kLag iterations old -> the stream never drains.
//   * "freeze on exit": once a stopping test fires on the device, every later
//     kernel returns immediately, so the lagged host check costs no accuracy
//     and the iterate is exactly the one the reference would return.
//   * 21 (plain) / 13 (ILU) vector passes per iteration collapse into 3 fused
//     kernels; the dot products ride on the kernels that stream the operands.
//   * row-sharded operation: the same loop, with the SpMV input gathered and the
//     scalar partials all-reduced through caller-supplied collectives (RCCL).
#include <mutex>
#include <utility>
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "ilu.h"      // IluPlans complete: a solver is created and destroyed here
#include "solver.h"

using namespace cm;

namespace cm {

// everything sized by the partition (n_pad): released when the partition changes (cudamat_solver_set_comm)
static void free_work(cudamat_solver *s)
{
    DevBuf<double> *vs[] = {&s->r, &s->rw, &s->p, &s->pw, &s->s, &s->t, &s->v, &s->gather, &s->x0_save, &s->v2,
                            &s->pz, &s->pww, &s->pq, &s->py, &s->pxh, &s->pipeA, &s->pipeB, &s->red_pipe,
                            &s->prh, &s->pwh, &s->psh, &s->pzh, &s->pqh, &s->ptmp};
    for (DevBuf<double> *q : vs) q->reset();
}

void spmv_copies_drop(cudamat_solver *s)
{
    pb_free(&s->pb);
    sell_free(&s->sell);
    pat_free(&s->pat);
    s->src_pb.reset();
    s->src_pb_len = 0;
    s->spmv_mode = -1;
}

int ensure_work(cudamat_solver *s)
{
    if (s->r) return CUDAMAT_OK;
    hipStream_t st = s->ctx->stream;
    const size_t count = (size_t)(s->n_pad > 0 ? s->n_pad : 1), nb = sizeof(double) * count;
    DevBuf<double> *vs[] = {&s->r, &s->rw, &s->p, &s->pw, &s->s, &s->t, &s->v};
    for (DevBuf<double> *q : vs) {
        CM_TRY(q->alloc(count));
        CM_HIP(hipMemsetAsync(q->get(), 0, nb, st));
    }
    if (s->ctx->cfg.verbose)
        fprintf(stderr, "[cudamat] work vectors: r %p rw %p p %p pw %p s %p t %p v %p (%zu bytes each)\n", (void *)s->r, (void *)s->rw, (void *)s->p,
                (void *)s->pw, (void *)s->s, (void *)s->t, (void *)s->v, nb);
    if (s->sharded) {
        CM_TRY(s->gather.alloc(count * (size_t)s->comm.world));
        CM_HIP(hipMemsetAsync(s->gather, 0, nb * (size_t)s->comm.world, st));
    }
    return CUDAMAT_OK;
}

}  // namespace cm

// ---- input validation (once, at creation): a malformed CSR must become an error code, never a stray access
// flags[0]: row pointers not 0 = rp[0] <= rp[1] <= ... <= rp[n] = nnz;  flags[1]: a column id outside [0, n_cols);
// flags[2]: some row's columns are not strictly increasing
__global__ __launch_bounds__(kBlock) void k_check_rowptr(int n, long long nnz, const int *rp, int *flags)
{
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i > n) return;
    bool bad = false;
    if (i == 0 && rp[0] != 0) bad = true;
    if (i == n && rp[n] != nnz) bad = true;
    if (i < n && rp[i] > rp[i + 1]) bad = true;
    if (rp[i] < 0 || rp[i] > nnz) bad = true;
    if (bad) flags[0] = 1;
}

__global__ __launch_bounds__(kBlock) void k_check_columns(int n, long long n_cols, const int *rp, const int *ci, int *flags)
{
    constexpr int L = 8;
    const long long row = ((long long)blockIdx.x * kBlock + threadIdx.x) / L;
    if (row >= n) return;
    const int lane = threadIdx.x & (L - 1);
    const int s = rp[row], e = rp[row + 1];
    bool range = false, order = false;
    for (int k = s + lane; k < e; k += L) {
        const int c = ci[k];
        if (c < 0 || c >= n_cols) range = true;
        if (k > s && ci[k - 1] >= c) order = true;
    }
    if (range) flags[1] = 1;
    if (order) flags[2] = 1;
}

static int validate_csr(cudamat_solver *s)
{
    hipStream_t st = s->ctx->stream;
    int *d = (int *)s->ctx->scratch.get(), h[3] = {0, 0, 0};
    hipError_t e = hipMemsetAsync(d, 0, sizeof(h), st);
    hipLaunchKernelGGL(k_check_rowptr, dim3((unsigned)(((long long)s->n + 1 + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, s->n,
                       (long long)s->nnz, s->rp, d);
    if (e == hipSuccess) e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(h, d, sizeof(h), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess && !h[0] && s->n > 0 && s->nnz > 0) {
        hipLaunchKernelGGL(k_check_columns, dim3((unsigned)(((long long)s->n * 8 + kBlock - 1) / kBlock)), dim3(kBlock), 0, st,
                           s->n, (long long)s->n_cols, s->rp, s->ci, d);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(h, d, sizeof(h), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
    }
    if (e != hipSuccess) return fail_hip(e, "CSR validation", __FILE__, __LINE__);
    if (h[0]) { set_error("row pointers must start at the index base, never decrease and end at nnz"); return CUDAMAT_ERR_ARG; }
    if (h[1]) { set_error("a column index lies outside [base, base + n_cols)"); return CUDAMAT_ERR_ARG; }
    s->cols_sorted = h[2] == 0;
    return CUDAMAT_OK;
}

namespace cm {

// ---- creation in stages.  cudamat_solver_create runs them back to back on device arrays; the host-pointer entry
// point (dropin.hip) runs the pattern stage as soon as the row pointers and column indices have been uploaded and the
// value stage when the values have.
// (1) the solver and its allocations; rp / ci / val are EMPTY (the caller fills them: 0-based)
int solver_alloc(cudamat_ctx *ctx, int n_local, int64_t n_cols, int64_t nnz, cudamat_solver **out)
{
    *out = nullptr;
    CM_ARG(n_local >= 0 && n_cols >= n_local && nnz >= 0, "sizes");
    CM_ARG(nnz < (1LL << 31) && n_cols < (1LL << 31), "local nnz and dimension must fit int32");
    CM_HIP(hipSetDevice(ctx->device));
    std::unique_ptr<cudamat_solver> s(new cudamat_solver());
    s->ctx = ctx;
    s->n = n_local;
    s->n_pad = n_local;
    s->n_cols = n_cols;
    s->nnz = nnz;
    s->t_create0 = now_s();
    hipStream_t st = ctx->stream;
    // (a failure below leaves through the solver's own destructor: nothing but memory is held yet)
    CM_TRY(s->rp.alloc((size_t)n_local + 1));
    CM_TRY(s->ci.alloc((size_t)nnz));
    CM_TRY(s->val.alloc((size_t)nnz));
    CM_TRY(s->parts_full.alloc(2 * kMaxParts));
    CM_TRY(s->parts_rv.alloc(2 * kMaxParts));
    CM_TRY(s->parts_half.alloc(2 * kMaxParts));
    CM_TRY(s->parts_tt.alloc(2 * kMaxParts));
    CM_TRY(s->red.alloc(16));
    CM_TRY(s->st.alloc(2));                   // (the second slot: L2State, common.h)
    LoopState *ring = nullptr;
    unsigned long long *snap = nullptr;
    if (hipHostMalloc((void **)&ring, sizeof(LoopState) * kRing, hipHostMallocDefault) != hipSuccess) {
        set_error("hipHostMalloc failed");
        return CUDAMAT_ERR_HIP;
    }
    s->st_ring.adopt(ring);
    if (hipHostMalloc((void **)&snap, sizeof(unsigned long long) * kRing, hipHostMallocDefault) != hipSuccess) snap = nullptr;
    s->snap_host.adopt(snap);
    if (!snap || hipHostGetDevicePointer((void **)&s->snap_dev, snap, 0) != hipSuccess) {
        set_error("pinned progress words unavailable");
        return CUDAMAT_ERR_HIP;
    }
    if (hipMemsetAsync(s->st, 0, 2 * sizeof(LoopState), st) != hipSuccess) return CUDAMAT_ERR_HIP;
    *out = s.release();
    return CUDAMAT_OK;
}

// (2) rp and ci are in place (0-based): validation, CSR launch plan, compressed indices
int solver_setup_pattern(cudamat_solver *s)
{
    cudamat_ctx *ctx = s->ctx;
    hipStream_t st = ctx->stream;
    const bool verbose = ctx->cfg.verbose != 0;
    double t_mark = now_s();
    auto stamp = [&](const char *what) {
        if (!verbose) return;
        const double t = now_s();
        fprintf(stderr, "[cudamat] create %-34s %8.3f ms\n", what, (t - t_mark) * 1e3);
        t_mark = t;
    };
    if (verbose) fprintf(stderr, "[cudamat] create %-34s %8.3f ms\n", "allocations + copies", (t_mark - s->t_create0) * 1e3);
    CM_TRY(validate_csr(s));
    stamp("validation");
    s->plan = plan_spmv(ctx->cfg, s->n, s->nnz);
    CM_TRY(plan_spmv_refine(st, ctx->cfg, s->n, s->nnz, s->rp, 0, &s->plan, ctx->scratch));
    stamp("CSR launch plan (refine)");
    CM_TRY(plan_spmv_compress(st, ctx->cfg, s->n, s->nnz, s->rp, s->ci, &s->plan));
    stamp("compressed-index attempt");
    return CUDAMAT_OK;
}

// (3) val is in place: the value-dependent parts of the CSR launch plan
int solver_setup_values(cudamat_solver *s)
{
    cudamat_ctx *ctx = s->ctx;
    hipStream_t st = ctx->stream;
    if (s->plan.c_off16) {          // compressed stream kernel: 8-bit value indices too when the matrix has a dictionary
        CM_TRY(ensure_valdict(s));
        if (s->vd.n > 0) CM_TRY(plan_spmv_dict(st, s->n, s->nnz, s->rp, s->vd.idx, s->vd.dict, &s->plan));
        if (!s->plan.d_pbase)       // fp64 values: line-aligned copies of the two entry streams
            CM_TRY(plan_spmv_align(st, ctx->cfg, s->n, s->nnz, s->rp, s->val, &s->plan));
    }
    s->t_create = now_s() - s->t_create0;
    return CUDAMAT_OK;
}

}  // namespace cm

extern "C" int cudamat_solver_create(cudamat_ctx *ctx, int n_local, int64_t n_cols, int64_t nnz,
                                     const int *rowptr, const int *colidx, const double *val,
                                     int base, cudamat_solver **out)
{
    CM_ARG(ctx && out, "null pointer");
    *out = nullptr;
    CM_ARG(base == 0 || base == 1, "base in {0,1}");
    CM_ARG(rowptr && (nnz == 0 || (colidx && val)), "null CSR array");
    Range range_create("cudamat: solver create (copies, validation, CSR plan)");
    cudamat_solver *s = nullptr;
    CM_TRY(solver_alloc(ctx, n_local, n_cols, nnz, &s));
    hipStream_t st = ctx->stream;
    int rc = launch_rebase(st, (int64_t)n_local + 1, rowptr, -base, s->rp);
    if (!rc && nnz) {
        rc = launch_rebase(st, nnz, colidx, -base, s->ci);
        if (!rc && hipMemcpyAsync(s->val, val, sizeof(double) * (size_t)nnz, hipMemcpyDeviceToDevice, st) != hipSuccess) {
            rc = CUDAMAT_ERR_HIP; set_error("val copy failed");
        }
    }
    if (!rc && hipStreamSynchronize(st) != hipSuccess) { rc = CUDAMAT_ERR_HIP; set_error("sync after upload failed"); }
    if (!rc) rc = solver_setup_pattern(s);
    if (!rc) rc = solver_setup_values(s);
    if (rc) {
        cudamat_solver_destroy(s);
        return rc;
    }
    *out = s;
    return CUDAMAT_OK;
}

extern "C" int cudamat_solver_destroy(cudamat_solver *s)
{
    if (!s) return CUDAMAT_OK;
    CM_DROP(hipSetDevice(s->ctx->device));
    CM_DROP(hipStreamSynchronize(s->ctx->stream));
    ilu0_release(s);           // (the blocked copies it holds are PbPlans: freed by hand, like s->pb)
    pb_free(&s->pb);
    for (int i = 0; i < kRing; i++)
        if (s->ev[i]) CM_DROP(hipEventDestroy(s->ev[i]));
    for (hipEvent_t e : s->prof_ev) CM_DROP(hipEventDestroy(e));
    for (hipEvent_t e : s->comm_ev) CM_DROP(hipEventDestroy(e));
    for (int e = 0; e < 2; e++) {
        if (s->ev_red[e]) CM_DROP(hipEventDestroy(s->ev_red[e]));
        if (s->ev_red_done[e]) CM_DROP(hipEventDestroy(s->ev_red_done[e]));
    }
    if (s->ev_x) CM_DROP(hipEventDestroy(s->ev_x));
    for (hipEvent_t e : s->ev_part)
        if (e) CM_DROP(hipEventDestroy(e));
    for (hipEvent_t e : s->ev_p1)
        if (e) CM_DROP(hipEventDestroy(e));
    for (hipStream_t q : s->part_stream)
        if (q) { CM_DROP(hipStreamSynchronize(q)); CM_DROP(hipStreamDestroy(q)); }
    delete s;                  // every buffer is released by its owner
    return CUDAMAT_OK;
}

extern "C" int cudamat_solver_set_shift(cudamat_solver *s, const double *d)
{
    CM_ARG(s, "solver is NULL");
    s->d = d;
    return CUDAMAT_OK;
}

extern "C" int cudamat_solver_set_comm(cudamat_solver *s, const cudamat_comm *comm)
{
    CM_ARG(s, "solver is NULL");
    CM_HIP(hipStreamSynchronize(s->ctx->stream));
    free_work(s);
    spmv_copies_drop(s);
    ilu0_release(s);           // factors belong to the old partition
    s->overlap = false;
    s->agreed = false;
    s->windowed = false;
    s->windows_known = false;
    s->need_dev.reset();
    const bool forced = comm && comm->world == 1 && s->ctx->cfg.force_sharded;
    if (!comm || (comm->world <= 1 && !forced)) {
        s->sharded = false;
        s->n_pad = s->n;
        return CUDAMAT_OK;
    }
    CM_ARG(comm->allgather && comm->allreduce, "collectives missing");
    CM_ARG(comm->rank >= 0 && comm->rank < comm->world, "rank");
    const int64_t per = (s->n_cols + comm->world - 1) / comm->world;
    int64_t mine = s->n_cols - per * comm->rank;
    if (mine > per) mine = per;
    if (mine < 0) mine = 0;
    if (mine != s->n) {
        set_error("row block mismatch: rank %d of %d must own %lld rows of %lld (uniform blocks of %lld), has %d",
                  comm->rank, comm->world, (long long)mine, (long long)s->n_cols, (long long)per, s->n);
        return CUDAMAT_ERR_ARG;
    }
    s->comm = *comm;
    s->sharded = true;
    s->n_pad = (int)per;
    if (comm->gather_window && comm->world > 1 && comm->world <= 4096)      // compute_windows' exchange buffer: allocated
        CM_TRY(s->need_dev.alloc((size_t)2 * comm->world + (size_t)2 * comm->world * comm->world));  // here, where a failure is still rank-local
    if (comm->gather_part && comm->comm_stream && !s->ev_x) {
        CM_HIP(hipEventCreateWithFlags(&s->ev_x, hipEventDisableTiming));
        for (int c = 0; c < kPbMaxChunks; c++) {
            CM_HIP(hipEventCreateWithFlags(&s->ev_part[c], hipEventDisableTiming));
            CM_HIP(hipEventCreateWithFlags(&s->ev_p1[c], hipEventDisableTiming));
            CM_HIP(hipStreamCreateWithFlags(&s->part_stream[c], hipStreamNonBlocking));
        }
    }
    if (s->ctx->cfg.overlap_chunks >= 1 && s->ctx->cfg.overlap_chunks <= kPbMaxChunks) s->overlap_chunks = s->ctx->cfg.overlap_chunks;
    return CUDAMAT_OK;
}

namespace cm {

// profiling of the exchanges: one (start, stop) pair per call, pooled per solver
static hipEvent_t comm_event(cudamat_solver *s)
{
    if (s->comm_used == s->comm_ev.size()) {
        hipEvent_t e = nullptr;
        if (hipEventCreate(&e) != hipSuccess) s->prof_failed = true;
        s->comm_ev.push_back(e);
    }
    return s->comm_ev[s->comm_used++];
}
void comm_mark_begin(cudamat_solver *s, int kind, hipStream_t st)
{
    if (!s->profiling) return;
    s->comm_kind.push_back(kind);
    if (hipEventRecord(comm_event(s), st) != hipSuccess) s->prof_failed = true;
}
void comm_mark_end(cudamat_solver *s, hipStream_t st)
{
    if (s->profiling && hipEventRecord(comm_event(s), st) != hipSuccess) s->prof_failed = true;
}

// y = (A + diag d) x with x a LOCAL n_pad-long work vector (pad zero); gathers first
// when sharded.  dot/check as in SpmvArgs.
int spmv_local(cudamat_solver *s, const double *x_local, double *y, int dot, const double *w,
               double *parts, LoopArgs la, int check, ScalarSrc half)
{
    Range range_spmv(s->sharded ? "cudamat: SpMV + exchange of its input" : "cudamat: SpMV");
    const double *xfull = x_local;
    const bool windowed = s->sharded && s->windowed;
    const bool overlapped = s->sharded && !windowed && s->overlap && s->spmv_mode == 1;
    if (windowed) {
        // only the parts of the other slices that this rank's rows reference travel (a halo for banded matrices)
        hipStream_t st = s->ctx->stream;
        CM_HIP(hipMemcpyAsync(s->gather + (size_t)s->comm.rank * (size_t)s->n_pad, x_local, sizeof(double) * (size_t)s->n_pad,
                              hipMemcpyDeviceToDevice, st));
        comm_mark_begin(s, 2, st);
        if (s->comm.gather_window(s->comm.user, x_local, s->gather, (int64_t)s->n_pad, s->w_send_off.data(), s->w_send_cnt.data(),
                                  s->w_recv_off.data(), s->w_recv_cnt.data()) != 0) {
            set_error("gather_window callback failed");
            return CUDAMAT_ERR_COMM;
        }
        comm_mark_end(s, st);
    } else if (s->sharded && !overlapped) {
        comm_mark_begin(s, 2, s->ctx->stream);
        if (s->comm.allgather(s->comm.user, x_local, s->gather, (int64_t)s->n_pad) != 0) {
            set_error("allgather callback failed");
            return CUDAMAT_ERR_COMM;
        }
        comm_mark_end(s, s->ctx->stream);
    }
    if (s->sharded) xfull = s->gather;
    SpmvArgs a{};
    a.n = s->n;
    a.rp = s->rp;
    a.ci = s->ci;
    a.val = s->val;
    a.x = xfull;
    a.d = s->d;
    a.xd = x_local;
    a.alpha = 1.0;
    a.beta = 0.0;
    a.y = y;
    a.dot = dot;
    a.w = w;
    a.parts = parts;
    a.loop = la;
    a.check = check;
    a.half = half;
    a.pb_strict = 0;
    if (s->spmv_mode == 1 || s->perm_active) CM_TRY(pb_strict_for(s->ctx, &a.pb_strict));
    if (s->perm_active && s->d) {        // rows in L's space, x in U's: the shift in L's order meets x at the row's position in U's
        a.d = s->d_perm;
        a.xd_idx = s->xd_idx;
    }
    if (overlapped) {
        // The gather in pieces on the communicator's stream, phase 1 piece by piece behind it:
        //   comm stream  :  [wait x ready] piece 0 | piece 1 | ...
        //   part stream c:  [wait x ready, piece c] phase 1 of the blocks of piece c          (c = 0 .. pieces-1)
        //   our stream   :  own slice -> gather buffer, test, phase 1 (local blocks) | wait for every part | phase 2
        // One stream per piece, because a piece's launch alone (and the local slice's: 1/world of the blocks) does
        // not fill the GPU: back to back on one stream they would cost a round of workgroups each (5 rounds instead
        // of 3 at 8 ranks and 4 pieces).  The products do not depend on the order of the phase-1 launches and
        // phase 2 adds them in column order as always, so the result is bit-identical to the plain gather + SpMV.
        // Hazards: every stream waits for `ev_x`, recorded on our stream behind the previous SpMV (the product and
        // gather buffers are free by then); our stream has waited for every part, hence for every piece (= all of
        // this rank's sends), before anything may overwrite x_local.
        hipStream_t st = s->ctx->stream, cst = (hipStream_t)s->comm.comm_stream;
        const PbPlan &p = s->pb;
        CM_HIP(hipEventRecord(s->ev_x, st));
        CM_HIP(hipStreamWaitEvent(cst, s->ev_x, 0));
        comm_mark_begin(s, 0, cst);
        for (int c = 0; c < p.chunks; c++) {
            const int64_t off = (int64_t)c * p.chunk_len;
            int64_t cnt = (int64_t)s->n_pad - off;
            if (cnt > p.chunk_len) cnt = p.chunk_len;
            if (cnt > 0 && s->comm.gather_part(s->comm.user, x_local, s->gather, (int64_t)s->n_pad, off, cnt) != 0) {
                set_error("gather_part callback failed");
                return CUDAMAT_ERR_COMM;
            }
            CM_HIP(hipEventRecord(s->ev_part[c], cst));
        }
        comm_mark_end(s, cst);
        CM_HIP(hipMemcpyAsync(s->gather + (size_t)s->comm.rank * (size_t)s->n_pad, x_local, sizeof(double) * (size_t)s->n_pad,
                              hipMemcpyDeviceToDevice, st));
        CM_TRY(launch_pb_check(st, a));
        CM_TRY(launch_pb_phase1(st, p, a, 0));
        for (int c = 0; c < p.chunks; c++) {
            hipStream_t ps = s->part_stream[c];
            CM_HIP(hipStreamWaitEvent(ps, s->ev_x, 0));
            CM_HIP(hipStreamWaitEvent(ps, s->ev_part[c], 0));
            CM_TRY(launch_pb_phase1(ps, p, a, 1 + c));
            CM_HIP(hipEventRecord(s->ev_p1[c], ps));
        }
        for (int c = 0; c < p.chunks; c++) CM_HIP(hipStreamWaitEvent(st, s->ev_p1[c], 0));
        return launch_pb_phase2(st, p, a);
    }
    if (s->perm_active) return launch_spmv_pb(s->ctx->stream, s->pb_perm, a);      // rows in L's space, columns in U's
    if (s->spmv_mode == 1) return launch_spmv_pb(s->ctx->stream, s->pb, a);
    if (s->spmv_mode == 2) return launch_spmv_sell(s->ctx->stream, s->sell, a);
    if (s->spmv_mode == 3) return launch_spmv_pat(s->ctx->stream, s->pat, a);
    return launch_spmv(s->ctx->stream, s->plan, a);
}

// the matrix's value dictionary (valdict.hip), looked for once: large systems only (small ones live in caches and the
// small-system loops keep their values in registers)
int ensure_valdict(cudamat_solver *s)
{
    if (s->vd_tried) return CUDAMAT_OK;
    s->vd_tried = true;
    if (s->nnz < (1 << 20)) return CUDAMAT_OK;
    return valdict_build(s->ctx->stream, s->ctx->cfg, s->nnz, s->val, &s->vd);
}

// number of per-workgroup partial sums an SpMV launch leaves in `parts`
int spmv_parts(const cudamat_solver *s)
{
    if (s->perm_active) return s->pb_perm.NRB;
    return s->spmv_mode == 1 ? s->pb.NRB : s->spmv_mode == 2 ? s->sell.grid : s->spmv_mode == 3 ? s->pat.grid : plan_spmv_parts(s->plan);
}

// How scattered are a row's columns?  Mean of (last - first column) over <= 4096 evenly spaced rows (sorted rows: the
// two ends of a row are its extremes).  One tiny launch; decides whether candidates that cannot win are timed at all.
__global__ __launch_bounds__(kBlock) void k_col_span(int n, const int *rp, const int *ci, int samples, unsigned long long *sum, int *cnt)
{
    const int q = blockIdx.x * kBlock + threadIdx.x;
    if (q >= samples) return;
    const int row = (int)((long long)q * n / samples);
    const int s = rp[row], e = rp[row + 1];
    if (e - s < 2) return;
    atomicAdd(sum, (unsigned long long)(ci[e - 1] - ci[s]));
    atomicAdd(cnt, 1);
}

static int col_span_bytes(cudamat_solver *s, double *out)
{
    *out = 0.0;
    hipStream_t st = s->ctx->stream;
    unsigned long long *d = (unsigned long long *)s->ctx->scratch.get(), h[2] = {0ULL, 0ULL};
    CM_HIP(hipMemsetAsync(d, 0, sizeof(h), st));
    const int samples = s->n < 4096 ? s->n : 4096;
    hipLaunchKernelGGL(k_col_span, dim3((samples + kBlock - 1) / kBlock), dim3(kBlock), 0, st, s->n, s->rp, s->ci, samples, d, (int *)(d + 1));
    hipError_t e = hipMemcpyAsync(h, d, sizeof(h), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    CM_HIP(e);
    const int cnt = (int)(h[1] & 0xffffffffULL);
    *out = cnt > 0 ? 8.0 * (double)h[0] / cnt : 0.0;
    return CUDAMAT_OK;
}

// Choose the SpMV implementation for this matrix (once), by TIMING the candidates on this device:
//   0  the CSR forms (lanes per row / stream tiles / nnz-balanced tiles, plan_spmv_refine) -- always a candidate;
//   1  the blocked two-phase kernels, when the columns are scattered over a vector far larger than L2 (pb_candidate);
//   2  SELL-C-sigma, for rows of 8 entries and more whose padded copy stays below 1.5 x the entries (banded
//      matrices: 2-2.7 x the lanes-per-row kernel; short rows belong to the stream kernel);
//   3  the row-pattern dictionary (spmv_pat.hip), for big matrices of short rows that repeat at most 255 shapes
//      (stencils): 8 B per entry + 1 B per row, no column indices.
// The switch SPMV_MODE = csr | pb | sell | pat overrides.
// Candidates that cannot win are not timed (round 3; the drop-in entry points pay this on every call): when a row's
// columns span far more than the L2s hold (mean span >= 16 MB of x; C4: 77 MB) and rows have >= 8 entries, every gather
// of the lanes-per-row kernel and of SELL misses L2 -- measured 9.8 / 9.1 ms against 2.8 ms blocked at C4, the same
// ratio on every scattered matrix of DESIGN section 4 -- so the blocked copy is selected without building the SELL copy
// or timing anything (a sharded solver still times the blocked form alone: ms_spmv_alone feeds the exposed-gather
// figure).  CUDAMAT_SPMV_TUNE=full restores the timing of every candidate.
static int ensure_spmv_mode_inner(cudamat_solver *s);

// The part of the choice below that needs the PATTERN only: is the blocked form what ensure_spmv_mode will select without
// timing anything?  (one GPU, sorted rows, a candidate by size, not forced elsewhere, and either forced or a mean column
// span >= 16 MB of x with rows of >= 8 entries).  Same rules as ensure_spmv_mode_inner -- it calls this.
int spmv_mode_is_blocked_early(cudamat_solver *s, bool *blocked)
{
    *blocked = false;
    const Config &cfg = s->ctx->cfg;
    if (s->sharded || s->n == 0 || s->nnz == 0 || !s->cols_sorted) return CUDAMAT_OK;
    if (cfg.spmv_mode == 0 || cfg.spmv_mode == 2) return CUDAMAT_OK;
    if (cfg.spmv_mode == 1) { *blocked = true; return CUDAMAT_OK; }
    if (!pb_candidate(s->ctx->stream, s->n, s->n_cols, s->nnz, s->rp, s->ci)) return CUDAMAT_OK;
    if (cfg.spmv_tune_full || s->nnz < 8 * (int64_t)s->n) return CUDAMAT_OK;
    if (s->col_span_bytes < 0.0) CM_TRY(col_span_bytes(s, &s->col_span_bytes));
    *blocked = s->col_span_bytes >= 16.0 * 1024 * 1024;
    return CUDAMAT_OK;
}

void spmv_mode_adopt_blocked(cudamat_solver *s, const PbPlan &pb, double seconds)
{
    s->pb = pb;
    s->spmv_mode = 1;
    s->t_spmv_setup = seconds;
    if (s->ctx->cfg.verbose)
        fprintf(stderr, "[cudamat] SpMV form 1 (blocked) built beside the upload in %.3f ms (a row's columns span %.1f MB of x)\n",
                seconds * 1e3, s->col_span_bytes / 1048576.0);
}

int ensure_spmv_mode(cudamat_solver *s)
{
    if (s->spmv_mode >= 0) return CUDAMAT_OK;
    Range range_mode("cudamat: SpMV form (matrix copies, tuning)");
    const double t0 = now_s();
    int rc = ensure_spmv_mode_inner(s);
    const int rc_sync = CM_RC(hipStreamSynchronize(s->ctx->stream));
    if (!rc) rc = rc_sync;
    s->t_spmv_setup = now_s() - t0;
    if (s->ctx->cfg.verbose)
        fprintf(stderr, "[cudamat] SpMV form %d chosen in %.3f ms (blocked copy %.3f ms, timing %.3f ms)\n", s->spmv_mode,
                s->t_spmv_setup * 1e3, s->pb.build_seconds * 1e3, s->t_spmv_timing * 1e3);
    return rc;
}

static int ensure_spmv_mode_inner(cudamat_solver *s)
{
    hipStream_t st = s->ctx->stream;
    const Config &cfg = s->ctx->cfg;
    const bool force_csr = cfg.spmv_mode == 0;
    const bool force_pb = cfg.spmv_mode == 1;
    const bool force_sell = cfg.spmv_mode == 2;
    const bool force_pat = cfg.spmv_mode == 3;
    s->spmv_mode = 0;
    if (force_csr || s->n == 0 || s->nnz == 0) return CUDAMAT_OK;
    bool have[4] = {true, false, false, false};
    // ---- blocked two-phase copy
    if (!force_sell && !force_pat) {
        if (!s->cols_sorted) {    // the blocked builder ranks entries by runs of equal column block: needs sorted rows
            if (force_pb) { set_error("the blocked SpMV needs rows with increasing column indices"); return CUDAMAT_ERR_ARG; }
        } else if (force_pb || pb_candidate(st, s->n, s->n_cols, s->nnz, s->rp, s->ci)) {
            // a sharded solver cuts the column blocks at the slices (and, for an overlapped gather, the pieces) of the
            // gathered vector; the gather buffer's index IS the column id (uniform slices of n_pad)
            PbCols cols;
            const bool can_overlap = s->sharded && s->comm.world > 1 && s->comm.gather_part && s->comm.comm_stream;
            if (s->sharded && s->comm.world > 1) {
                cols.per = s->n_pad;
                cols.rank = s->comm.rank;
                cols.chunks = can_overlap ? s->overlap_chunks : 1;
            }
            CM_TRY(ensure_valdict(s));
            const int rc = pb_build(st, cfg, s->n, s->n_cols, s->nnz, s->rp, s->ci, s->val, &s->pb, &cols, &s->vd);
            if (rc != CUDAMAT_OK && force_pb) return rc;
            have[1] = rc == CUDAMAT_OK;          // e.g. out of memory for the blocked copy: keep the others
        }
        if (force_pb && !s->sharded) { s->spmv_mode = 1; return CUDAMAT_OK; }
        if (force_pb) { have[0] = false; }      // sharded: still time it (ms_spmv_alone feeds the exposed-gather figure)
    }
    // scattered columns: the gather-based forms cannot win (see above)
    bool scattered = false;
    {
        if (have[1] && !force_pb && !force_sell && !force_pat && !cfg.spmv_tune_full && s->nnz >= 8 * (int64_t)s->n) {
            if (s->col_span_bytes < 0.0) CM_TRY(col_span_bytes(s, &s->col_span_bytes));
            scattered = s->col_span_bytes >= 16.0 * 1024 * 1024;
        }
        if (scattered) {
            have[0] = false;
            if (!s->sharded) {
                s->spmv_mode = 1;
                if (cfg.verbose)
                    fprintf(stderr, "cudamat: SpMV: a row's columns span %.1f MB of x on average -> blocked, nothing timed\n", s->col_span_bytes / 1048576.0);
                return CUDAMAT_OK;
            }
        }
    }
    // ---- SELL-C-sigma copy: rows of 8 entries and more (shorter rows belong to the stream kernel, which measures
    // faster there: C3 0.174 vs 0.191 ms) whose padded copy stays below 1.5 x the entries.  Measured on 2e6-row banded
    // matrices (scripts/sell_probe.py): row lengths 14..70 0.46 ms vs 0.94 (CSR forms) / 0.66 (blocked); 13..20 0.18
    // vs 0.40 / 0.26; with scattered columns the blocked form wins (0.48 vs 1.07) -- hence: time them.
    const bool sell_off = !cfg.spmv_sell;
    if (force_sell || (!force_pb && !force_pat && !scattered && !sell_off && s->n >= 4096 && s->nnz >= (1 << 16) && s->plan.stream_rows == 0 && s->nnz >= 8 * (int64_t)s->n)) {
        const int rc = sell_build(st, s->n, s->nnz, s->rp, s->ci, s->val, &s->sell, force_sell ? 0.0 : 1.5);
        if (rc != CUDAMAT_OK && force_sell) return rc;
        have[2] = rc == CUDAMAT_OK;
        if (force_sell) { s->spmv_mode = 2; return CUDAMAT_OK; }
    }
    // ---- row-pattern dictionary: short rows (the stream-tile plan) of a system beyond the fused small-system loops whose
    // rows repeat at most 255 shapes; 25 % padding at most.  At C3 it moves 0.58 GB per launch where the compressed
    // stream kernel moves 0.77 GB -- timed like every other candidate.
    if (force_pat || (!force_pb && !scattered && s->plan.stream_rows > 0 && s->n > 300000 && s->nnz >= (1 << 20))) {
        CM_TRY(ensure_valdict(s));
        const int rc = pat_build(st, s->n, s->nnz, s->rp, s->ci, s->val, &s->pat, force_pat ? 0.0 : 1.25, &s->vd);
        if (rc != CUDAMAT_OK && (force_pat || rc != CUDAMAT_ERR_ARG) && rc != CUDAMAT_ERR_NOMEM) return rc;
        if (rc != CUDAMAT_OK && force_pat) return rc;
        have[3] = rc == CUDAMAT_OK;
        if (force_pat) { s->spmv_mode = 3; return CUDAMAT_OK; }
    }
    if (!have[1] && !have[2] && !have[3]) return CUDAMAT_OK;
    if (force_pb && !have[1]) { set_error("the blocked copy could not be built"); return CUDAMAT_ERR_NOMEM; }
    if (force_pb) have[2] = have[3] = false;
    const LoopArgs la_none{nullptr, nullptr, 0, 0, 0};
    const ScalarSrc nosrc{nullptr, 0, 1};
    const double *xin = s->sharded ? s->gather : s->p;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    CM_HIP(hipEventCreate(&e0));
    if (hipEventCreate(&e1) != hipSuccess) { CM_DROP(hipEventDestroy(e0)); return fail_hip(hipGetLastError(), "hipEventCreate", __FILE__, __LINE__); }
    float ms[4] = {0.f, 0.f, 0.f, 0.f};
    int rc = CUDAMAT_OK;
    const double t_timing0 = now_s();
    for (int mode = 0; mode < 4 && rc == CUDAMAT_OK; mode++) {
        if (!have[mode]) continue;
        SpmvArgs a{};
        a.n = s->n; a.rp = s->rp; a.ci = s->ci; a.val = s->val; a.x = xin; a.d = nullptr; a.xd = s->p;
        a.alpha = 1.0; a.beta = 0.0; a.y = s->v; a.dot = 0; a.loop = la_none; a.check = CHECK_NONE; a.half = nosrc;
        a.pb_strict = 0;
        if (mode == 1) CM_TRY(pb_strict_for(s->ctx, &a.pb_strict));
        for (int rep = 0; rep < 3 && rc == CUDAMAT_OK; rep++) {
            if (rep == 1) rc = CM_RC(hipEventRecord(e0, st));
            if (rc) break;
            rc = mode == 1 ? launch_spmv_pb(st, s->pb, a) : mode == 2 ? launch_spmv_sell(st, s->sell, a) :
                 mode == 3 ? launch_spmv_pat(st, s->pat, a) : launch_spmv(st, s->plan, a);
        }
        // (a candidate that cannot be timed must not win by its 0 ms: the error ends the selection)
        if (!rc) rc = CM_RC(hipEventRecord(e1, st));
        if (!rc) rc = CM_RC(hipEventSynchronize(e1));
        if (!rc) rc = CM_RC(hipEventElapsedTime(&ms[mode], e0, e1));
    }
    CM_DROP(hipEventDestroy(e0));
    CM_DROP(hipEventDestroy(e1));
    CM_TRY(rc);
    s->t_spmv_timing = now_s() - t_timing0;
    CM_HIP(hipMemsetAsync(s->v, 0, sizeof(double) * (size_t)(s->n_pad > 0 ? s->n_pad : 1), st));
    s->ms_csr = ms[0] / 2;
    s->ms_pb = ms[1] / 2;
    s->ms_sell = ms[2] / 2;
    s->ms_pat = ms[3] / 2;
    int best = have[0] ? 0 : 1;
    if (rc == CUDAMAT_OK)
        for (int mode = 1; mode < 4; mode++)
            if (have[mode] && (!have[best] || ms[mode] < ms[best])) best = mode;
    s->spmv_mode = best;
    s->ms_spmv_alone = ms[best] / 2;
    const double sell_fill = s->sell.fill;
    if (best != 1) pb_free(&s->pb);
    if (best != 2) sell_free(&s->sell);
    const int npat = s->pat.npat;
    if (best != 3) pat_free(&s->pat);
    if (cfg.verbose)
        fprintf(stderr, "cudamat: SpMV auto-tune csr %.3f ms, blocked %s%.3f ms, sell %s%.3f ms (fill %.2f), row patterns %s%.3f ms (%d patterns) -> %s\n",
                s->ms_csr, have[1] ? "" : "(n/a) ", s->ms_pb, have[2] ? "" : "(n/a) ", s->ms_sell, sell_fill, have[3] ? "" : "(n/a) ", s->ms_pat,
                npat, best == 1 ? "blocked" : best == 2 ? "sell" : best == 3 ? "row patterns" : "csr");
    return CUDAMAT_OK;
}

int allreduce(cudamat_solver *s, double *buf, int count)
{
    Range range_ar("cudamat: all-reduce");
    // fault injection for the tests of the failure paths: the option TEST_COMM_FAIL = "rank:k" makes the k-th all-reduce
    // of that rank's solver report an error (tests/test_gpu_dist.py: a failing rank must not strand its peers)
    if (s->ctx->cfg.fail_rank >= 0 && s->ctx->cfg.fail_rank == s->comm.rank && ++s->test_allreduces == s->ctx->cfg.fail_call) {
        set_error("injected all-reduce failure (TEST_COMM_FAIL=%d:%d)", s->ctx->cfg.fail_rank, s->ctx->cfg.fail_call);
        return CUDAMAT_ERR_COMM;
    }
    comm_mark_begin(s, 3, s->ctx->stream);
    if (s->comm.allreduce(s->comm.user, buf, count) != 0) {
        set_error("allreduce callback failed");
        return CUDAMAT_ERR_COMM;
    }
    comm_mark_end(s, s->ctx->stream);
    return CUDAMAT_OK;
}

// ---- windowed gather (halo): which part of every other rank's slice do the local rows reference?
// lo[q] / hi[q]: smallest / one past the largest column of slice q (relative to the slice) among the local entries.
// Each thread walks a contiguous run of entries and only touches the workgroup's LDS tables when an entry leaves
// the range it has already reported for that slice (rows are mostly sorted, so that is rare).
__global__ __launch_bounds__(kBlock) void k_col_windows(long long nnz, const int *ci, int per, int world, int *lo, int *hi)
{
    extern __shared__ int tab[];              // lo_s[world], hi_s[world]
    int *lo_s = tab, *hi_s = tab + world;
    for (int q = threadIdx.x; q < world; q += kBlock) { lo_s[q] = per; hi_s[q] = 0; }
    __syncthreads();
    const long long per_thread = (nnz + (long long)gridDim.x * kBlock - 1) / ((long long)gridDim.x * kBlock);
    const long long k0 = ((long long)blockIdx.x * kBlock + threadIdx.x) * per_thread;
    const long long k1 = k0 + per_thread < nnz ? k0 + per_thread : nnz;
    int cq = -1, clo = 0, chi = 0;
    for (long long k = k0; k < k1; k++) {
        const int c = ci[k], q = c / per, w = c - q * per;
        if (q == cq && w >= clo && w < chi) continue;
        if (q != cq) { cq = q; clo = w; chi = w + 1; }
        else { clo = w < clo ? w : clo; chi = w + 1 > chi ? w + 1 : chi; }
        atomicMin(&lo_s[q], w);
        atomicMax(&hi_s[q], w + 1);
    }
    __syncthreads();
    for (int q = threadIdx.x; q < world; q += kBlock) {
        if (hi_s[q] > 0) { atomicMin(&lo[q], lo_s[q]); atomicMax(&hi[q], hi_s[q]); }
    }
}

// collective: every rank learns what every rank needs from every slice; decides (identically everywhere) whether
// the windows replace the whole gather.  Every rank-local step comes BEFORE the all-gather and its outcome travels IN
// the payload (a negative entry = "this rank failed"), so a rank whose local work failed still enters the collective
// and every rank returns an error afterwards -- nobody is left alone inside it.
static int compute_windows(cudamat_solver *s)
{
    s->windows_known = true;
    s->windowed = false;
    s->gather_fraction = 1.0;
    const int W = s->comm.world, me = s->comm.rank;
    if (!s->comm.gather_window || W <= 1 || W > 4096) return CUDAMAT_OK;
    hipStream_t st = s->ctx->stream;
    const int per = s->n_pad;
    std::vector<int> h((size_t)2 * W);
    std::vector<double> mine((size_t)2 * W, 0.0), all((size_t)2 * W * W, 0.0);
    char saved[512] = "";
    auto local = [&]() -> int {
        DevBuf<int> d_lohi;
        CM_TRY(d_lohi.alloc(2 * (size_t)W));
        for (int q = 0; q < W; q++) { h[(size_t)q] = per; h[(size_t)W + q] = 0; }
        hipError_t e = hipMemcpyAsync(d_lohi, h.data(), sizeof(int) * h.size(), hipMemcpyHostToDevice, st);
        if (e == hipSuccess && s->nnz > 0) {
            hipLaunchKernelGGL(k_col_windows, dim3(row_grid(s->nnz, 4096LL * kBlock)), dim3(kBlock), sizeof(int) * 2 * (size_t)W, st, (long long)s->nnz, s->ci, per, W,
                               d_lohi, d_lohi + W);
        }
        if (e == hipSuccess) e = hipMemcpyAsync(h.data(), d_lohi, sizeof(int) * h.size(), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        CM_HIP(e);
        for (int q = 0; q < W; q++)
            if (q != me && h[(size_t)W + q] > h[(size_t)q]) { mine[(size_t)2 * q] = h[(size_t)q]; mine[(size_t)2 * q + 1] = h[(size_t)W + q]; }
        return CUDAMAT_OK;
    };
    const int rc_local = local();
    if (rc_local != CUDAMAT_OK) {
        snprintf(saved, sizeof(saved), "%s", cudamat_last_error());
        mine.assign((size_t)2 * W, -1.0);
    }
    // (need_dev was allocated by cudamat_solver_set_comm: no allocation can fail between here and the collective)
    CM_HIP(hipMemcpyAsync(s->need_dev, mine.data(), sizeof(double) * mine.size(), hipMemcpyHostToDevice, st));
    CM_HIP(hipStreamSynchronize(st));
    if (s->comm.allgather(s->comm.user, s->need_dev, s->need_dev + 2 * W, (int64_t)2 * W) != 0) {
        set_error("allgather callback failed");
        return CUDAMAT_ERR_COMM;
    }
    CM_HIP(hipMemcpyAsync(all.data(), s->need_dev + 2 * W, sizeof(double) * all.size(), hipMemcpyDeviceToHost, st));
    CM_HIP(hipStreamSynchronize(st));
    if (rc_local != CUDAMAT_OK) { set_error("%s", saved); return rc_local; }
    for (double v : all)
        if (v < 0.0) { set_error("another rank failed while it looked for its column windows"); return CUDAMAT_ERR_COMM; }
    s->w_send_off.assign((size_t)W, 0); s->w_send_cnt.assign((size_t)W, 0);
    s->w_recv_off.assign((size_t)W, 0); s->w_recv_cnt.assign((size_t)W, 0);
    double worst = 0.0;
    for (int p = 0; p < W; p++) {             // p needs [lo, hi) of slice q
        double tot = 0.0;
        for (int q = 0; q < W; q++) {
            const double lo = all[((size_t)p * W + q) * 2], hi = all[((size_t)p * W + q) * 2 + 1];
            if (q == p || hi <= lo) continue;
            tot += hi - lo;
            if (p == me) { s->w_recv_off[(size_t)q] = (int64_t)lo; s->w_recv_cnt[(size_t)q] = (int64_t)(hi - lo); }
            if (q == me) { s->w_send_off[(size_t)p] = (int64_t)lo; s->w_send_cnt[(size_t)p] = (int64_t)(hi - lo); }
        }
        const double frac = tot / ((double)(W - 1) * (double)per);
        if (p == me) s->gather_fraction = frac;
        worst = frac > worst ? frac : worst;
    }
    s->windowed = worst <= 0.5 && s->ctx->cfg.windowed;
    if (!s->windowed) s->gather_fraction = 1.0;
    if (s->ctx->cfg.verbose)
        fprintf(stderr, "cudamat: rank %d references %.4f of the other slices (worst rank %.4f) -> %s\n", me,
                s->windowed ? s->gather_fraction : worst, worst, s->windowed ? "windowed gather" : "whole gather");
    return CUDAMAT_OK;
}

// Sharded runs: the ranks agree on the outcome of the rank-local setup steps BEFORE the first collective of the
// data path -- a rank whose blocked copy, ILU(0) or allocation failed makes every rank return an error (instead of
// leaving its peers inside a collective for ever), and the gather is overlapped only if every rank runs the
// blocked SpMV (the pieces are exchanged by a different call sequence than the plain all-gather).
int setup_agree(cudamat_solver *s, int rc_local)
{
    if (!s->sharded) return rc_local;
    char saved[512];
    snprintf(saved, sizeof(saved), "%s", cudamat_last_error());
    hipStream_t st = s->ctx->stream;
    double h[2] = {rc_local != CUDAMAT_OK ? 1.0 : 0.0, s->spmv_mode == 1 ? 1.0 : 0.0};
    // (the only rank-local step in front of the collective is this 16-byte upload; if it fails the device itself is
    // gone and the all-reduce below could not run either -- the host must then abort the communicator,
    // cudamat_rccl_comm_abort, as csrc/sharded.cpp does for every failed rank)
    CM_HIP(hipMemcpyAsync(s->red + 10, h, sizeof(h), hipMemcpyHostToDevice, st));
    CM_HIP(hipStreamSynchronize(st));                       // (h is a stack buffer)
    CM_TRY(allreduce(s, s->red + 10, 2));
    CM_HIP(hipMemcpyAsync(h, s->red + 10, sizeof(h), hipMemcpyDeviceToHost, st));
    CM_HIP(hipStreamSynchronize(st));
    s->overlap = s->comm.world > 1 && s->comm.gather_part && s->comm.comm_stream && s->ev_x && s->pb.chunks >= 1 &&
                 h[1] == (double)s->comm.world && s->ctx->cfg.overlap;
    s->agreed = true;
    if (h[0] == 0.0 && !s->windows_known) CM_TRY(compute_windows(s));       // collective: same call on every rank
    if (h[0] != 0.0) {
        if (rc_local != CUDAMAT_OK) { set_error("%s", saved); return rc_local; }
        set_error("%d rank(s) of the sharded solver failed during setup", (int)h[0]);
        return CUDAMAT_ERR_COMM;
    }
    return CUDAMAT_OK;
}

}  // namespace cm

extern "C" int cudamat_solver_spmv_mode(cudamat_solver *s, int *mode)
{
    CM_ARG(s && mode, "null pointer");
    CM_HIP(hipSetDevice(s->ctx->device));
    CM_TRY(ensure_work(s));
    CM_TRY(ensure_spmv_mode(s));
    *mode = s->spmv_mode;
    return CUDAMAT_OK;
}

extern "C" int cudamat_solver_value_dict(cudamat_solver *s, int *distinct)
{
    CM_ARG(s && distinct, "null pointer");
    CM_HIP(hipSetDevice(s->ctx->device));
    CM_TRY(ensure_work(s));
    CM_TRY(ensure_spmv_mode(s));
    *distinct = 0;
    if (s->spmv_mode == 1 && s->pb.pvi) *distinct = s->pb.ndict;
    else if (s->spmv_mode == 0 && s->plan.d_pbase) *distinct = s->vd.n;
    else if (s->spmv_mode == 3 && s->pat.vidx) *distinct = s->pat.ndict;
    return CUDAMAT_OK;
}

extern "C" int cudamat_solver_placement(cudamat_solver *s, int *placed, int *slabs, double *seconds, char *classes, int cap)
{
    CM_ARG(s, "null pointer");
    CM_HIP(hipSetDevice(s->ctx->device));
    CM_TRY(ensure_work(s));
    CM_TRY(ensure_spmv_mode(s));
    // (a preconditioned loop that runs in the level-major spaces multiplies by the permuted matrix's copy)
    const PbPlan *q = s->pb_perm.P ? &s->pb_perm : s->spmv_mode == 1 && s->pb.P ? &s->pb : nullptr;
    if (placed) *placed = q ? q->placed : -1;
    if (slabs) *slabs = q ? q->place_slabs : 0;
    if (seconds) *seconds = q ? q->place_seconds : 0.0;
    if (classes && cap > 0) snprintf(classes, (size_t)cap, "%s", q ? q->place_classes : "");
    return CUDAMAT_OK;
}

extern "C" int cudamat_solver_spmv_kernel(cudamat_solver *s, char *name, int cap)
{
    CM_ARG(s && name && cap > 0, "null pointer");
    CM_HIP(hipSetDevice(s->ctx->device));
    CM_TRY(ensure_work(s));
    CM_TRY(ensure_spmv_mode(s));
    const SpmvPlan &p = s->plan;
    if (s->spmv_mode == 1) {
        int strict = 0;
        CM_TRY(pb_strict_for(s->ctx, &strict));
        snprintf(name, (size_t)cap, "%s + k_pb_phase2%s", s->pb.pvi ? "k_pb_phase1_dict" : "k_pb_phase1", strict ? " (architected order)" : "");
    }
    else if (s->spmv_mode == 2) snprintf(name, (size_t)cap, "k_spmv_sell");
    else if (s->spmv_mode == 3 && s->pat.vidx) snprintf(name, (size_t)cap, "k_spmv_pat_d<%d>", s->pat.vword / 8);
    else if (s->spmv_mode == 3) snprintf(name, (size_t)cap, "k_spmv_pat<%d>", s->pat.W <= 8 ? 8 : 16);
    else if (p.tiles > 0) snprintf(name, (size_t)cap, "k_spmv_tiles");
    else if (p.stream_rows && p.c_off16) snprintf(name, (size_t)cap, "%s<%d>", p.d_pbase ? "k_spmv_stream_d" : "k_spmv_stream_c", p.stream_rows);
    else if (p.stream_rows) snprintf(name, (size_t)cap, "k_spmv_stream<%d>", p.stream_rows);
    else snprintf(name, (size_t)cap, "k_spmv<%d>", p.lanes);
    return CUDAMAT_OK;
}

extern "C" int cudamat_solver_spmv(cudamat_solver *s, const double *x_local, double *y_local)
{
    CM_ARG(s && x_local && y_local, "null pointer");
    CM_HIP(hipSetDevice(s->ctx->device));
    {
        int rc_setup = ensure_work(s);
        if (rc_setup == CUDAMAT_OK) rc_setup = ensure_spmv_mode(s);
        if (s->sharded && !s->agreed) rc_setup = setup_agree(s, rc_setup);
        CM_TRY(rc_setup);
    }
    const double *xin = x_local;
    if (s->sharded) {   // the gather needs n_pad entries with a zero pad
        CM_HIP(hipMemcpyAsync(s->pw, x_local, sizeof(double) * (size_t)s->n, hipMemcpyDeviceToDevice,
                              s->ctx->stream));
        xin = s->pw;
    }
    return spmv_local(s, xin, y_local, 0, nullptr, nullptr, LoopArgs{nullptr, nullptr, 0, 0, 0},
                      CHECK_NONE, ScalarSrc{nullptr, 0, 1});
}

namespace cm {

hipEvent_t prof_event(cudamat_solver *s, size_t i)
{
    while (s->prof_ev.size() <= i) {
        hipEvent_t e = nullptr;
        if (hipEventCreate(&e) != hipSuccess) s->prof_failed = true;
        s->prof_ev.push_back(e);
    }
    return s->prof_ev[i];
}

// native: `in` is in L's level-major space and `out` leaves in U's (the loop that runs in those spaces); otherwise both
// are in the caller's row numbering (level-major factors then permute on the way in and out)
int precond_apply(cudamat_solver *s, const double *in, double *tmp, double *out, bool native)
{
    if (s->L.lm && !native) return precond_apply_original(s, in, tmp, out);
    CM_TRY(trsv_apply(s, s->L, false, in, tmp));    // pbicgstab.cu:92-94 / :121-123
    CM_TRY(trsv_apply(s, s->U, true, tmp, out));    // pbicgstab.cu:96-98 / :125-127
    return CUDAMAT_OK;
}

}  // namespace cm

extern "C" int cudamat_solver_precond_apply(cudamat_solver *s, const double *in, double *out)
{
    CM_ARG(s && in && out, "null pointer");
    CM_ARG(s->has_ilu, "call cudamat_solver_ilu0 / cudamat_solver_block_ilu0 first");
    CM_HIP(hipSetDevice(s->ctx->device));
    CM_TRY(ensure_work(s));
    return precond_apply(s, in, s->t, out);
}

