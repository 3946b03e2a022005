// values.hip -- new values for a resident matrix on the structure it already holds (cudamat_solver_set_values).
//
// Time stepping, Newton iterations and parameter sweeps keep the pattern and change the entries.  Everything a solver has
// built from the PATTERN stays: the validation, the CSR launch plan and its compressed indices, the geometry and the placement
// of the blocked copy, the SELL permutation, the row-pattern table, the chosen SpMV form and the tuner's timings, the level
// analysis / far-near split / permutation maps of ILU(0).  Only the NUMBERS are written again, into the arrays that hold them:
//
//   s->val                          one device-to-device copy
//   s->vd                           valdict_build on the new values (same rules as at creation)
//   CSR plan (a_val | d_val8)       the value stage's fill pass over the kept tile bases (plan_spmv_refresh_values)
//   blocked copy (pv | pvi)         one streaming gather through a map "stored entry -> CSR position" (below)
//   SELL (val), row patterns        their fill kernels' value part: both layouts are closed-form in (row, entry of the row)
//   permuted matrix (pb_perm)       the same gather through its own map
//
// The contract is bit-identity with a fresh solver created from the new values under the same switches.  A copy holds either
// fp64 values or 8-bit dictionary indices -- its storage class.  While the class stays, the refresh above writes exactly what
// the builders would have written (they place an entry by the pattern alone).  When it changes (the new values have a
// dictionary and the old ones had none, or the other way round) nothing is converted: the copies are dropped and the form is
// chosen again at the next use, which is what a fresh solver does.
//
// The maps are not computed by a second builder: the existing one runs once on TAGS -- a value array that holds every entry's
// CSR position + 1 as a double -- without dictionary, placement or output, and the positions are read out of what it leaves
// (the route of ilu.hip's refactor_maps_of).  One int per stored entry, built at the first call that finds the copy.
//
// The ILU(0) factors are NOT touched: they stay those of the old values, a lagged preconditioner (as factors may stay while d
// moves) until cudamat_solver_ilu0_refactor -- which reads the matrix through s->pm_val == s->val -- brings
// them up to date.  The solver records that they are stale (ilu_stale); the drop-in call never solves with stale factors.
#include <utility>

#include "device.h"
#include "ilu.h"
#include "solver.h"
#include "values.h"

namespace cm {

// ---------------------------------------------------------------- the gather family: to[i] = from[map[i]]
// Streams over DESTINATION order: 4 bytes of map and the store are sequential, the read of `from` is the one gather.
// fp64: 4 + 8 + 8 = 20 algorithmic bytes per entry; bytes: 4 + 1 + 1 = 6.
template <int VEC>
__global__ __launch_bounds__(kBlock) void k_refresh_values(int64_t count, const int *src, const double *lu, double *val)
{
    vec_loop<VEC>(count, [&](int64_t i, auto w) {
        constexpr int W = decltype(w)::value;
        int at[W];
        double v[W];
        if constexpr (W == 2) {
            const int2 q = ((const int2 *)src)[i];
            at[0] = q.x;
            at[1] = q.y;
        } else {
            at[0] = src[i];
        }
#pragma unroll
        for (int j = 0; j < W; j++) v[j] = at[j] >= 0 ? lu[at[j]] : 0.0;        // (-1: an alignment pad of a blocked copy)
        store_row<W>(val, i, v, kAll);
    });
}

int launch_refresh_values(hipStream_t s, int64_t count, const int *src, const double *lu, double *val)
{
    if (count <= 0) return CUDAMAT_OK;
    CM_VEC_LAUNCH(all_aligned16(val) && (((uintptr_t)src) & 7) == 0, vec_grid(count), k_refresh_values<VEC>, count, src, lu, val);
}

// 8-bit sources (dictionary indices).  VEC = 1: a thread produces 8 destination bytes -- two 16-byte map loads, eight byte
// gathers, ONE 8-byte store (byte j of the word is entry 8 i + j: little-endian) -- and the up to 7 entries of the tail are
// scalar; VEC = 0 (misaligned operands): every entry scalar.  No lane stores single bytes in the main body.
template <int VEC>
__global__ __launch_bounds__(kBlock) void k_refresh_bytes(int64_t count, const int *src, const unsigned char *from, unsigned char *to)
{
    const int64_t n8 = VEC ? count / 8 : 0;
    const int64_t first = (int64_t)blockIdx.x * kBlock + threadIdx.x, stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = first; i < n8; i += stride) {
        const int4 a = ((const int4 *)src)[2 * i], b = ((const int4 *)src)[2 * i + 1];
        const int at[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
        unsigned long long word = 0ull;
#pragma unroll
        for (int j = 0; j < 8; j++) word |= (unsigned long long)(at[j] >= 0 ? from[at[j]] : (unsigned char)0) << (8 * j);
        ((unsigned long long *)to)[i] = word;
    }
    for (int64_t i = 8 * n8 + first; i < count; i += stride) {
        const int at = src[i];
        to[i] = at >= 0 ? from[at] : (unsigned char)0;
    }
}

int launch_refresh_bytes(hipStream_t s, int64_t count, const int *src, const unsigned char *from, unsigned char *to)
{
    if (count <= 0) return CUDAMAT_OK;
    CM_VEC_LAUNCH(all_aligned16(src) && (((uintptr_t)to) & 7) == 0, vec_grid(count / 4), k_refresh_bytes<VEC>, count, src, from, to);
}

// the map of one array filled from a value array that held every entry's (source position) + 1 as a double (exact: < 2^31):
// 0.0 is an alignment pad -> -1
__global__ __launch_bounds__(kBlock) void k_src_from_tags(int64_t count, const double *tag, int *src)
{
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < count; i += stride) src[i] = (int)tag[i] - 1;
}

__global__ __launch_bounds__(kBlock) void k_tags(int64_t count, double *tag)
{
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < count; i += stride) tag[i] = (double)(i + 1);
}

int launch_value_tags(hipStream_t s, int64_t count, double *tag)
{
    if (count <= 0) return CUDAMAT_OK;
    hipLaunchKernelGGL(k_tags, dim3(row_grid(count)), dim3(kBlock), 0, s, count, tag);
    CM_HIP(hipGetLastError());
    return CUDAMAT_OK;
}

int launch_map_from_tags(hipStream_t s, int64_t count, const double *tag, int *map)
{
    if (count <= 0) return CUDAMAT_OK;
    hipLaunchKernelGGL(k_src_from_tags, dim3(row_grid(count)), dim3(kBlock), 0, s, count, tag, map);
    CM_HIP(hipGetLastError());
    return CUDAMAT_OK;
}

int pb_value_map(hipStream_t st, const PbPlan &have, const PbPlan &tagged, DevBuf<int> *map, int64_t *len)
{
    *len = 0;
    const bool same = (have.pv || have.pvi) && tagged.pv && have.n == tagged.n && have.n_cols == tagged.n_cols && have.nnz == tagged.nnz &&
                      have.NCB == tagged.NCB && have.CB == tagged.CB && have.NSUB == tagged.NSUB && have.SR == tagged.SR && have.NW == tagged.NW;
    if (!same) {
        set_error("set_values: the blocked-copy switches (PB_*) differ from those the copy was built with; create the solver again");
        return CUDAMAT_ERR_ARG;
    }
    int total = -1, total_have = -2;
    CM_HIP(hipStreamSynchronize(st));
    CM_HIP(hipMemcpy(&total, tagged.cstart + tagged.NCB, sizeof(int), hipMemcpyDeviceToHost));
    CM_HIP(hipMemcpy(&total_have, have.cstart + have.NCB, sizeof(int), hipMemcpyDeviceToHost));
    if (total != total_have || total < 0) {
        set_error("set_values: the blocked copy holds %d entry slots, its map would cover %d", total_have, total);
        return CUDAMAT_ERR_HIP;
    }
    CM_TRY(map->alloc((size_t)total + 4));           // (+ 4: a 16-byte load of the byte form's last pair of quads stays inside)
    CM_TRY(launch_map_from_tags(st, (int64_t)total, tagged.pv, map->get()));
    CM_HIP(hipStreamSynchronize(st));
    *len = total;
    return CUDAMAT_OK;
}

// ---------------------------------------------------------------- cudamat_solver_set_values
namespace {

// the fp64 | 8-bit refresh of one blocked copy through its map; a dictionary copy is re-pointed at the solver's dictionary
int pb_refresh(hipStream_t st, PbPlan *p, const int *map, int64_t len, const double *val, const ValDict &vd)
{
    if (p->pvi) {
        CM_TRY(launch_refresh_bytes(st, len, map, vd.idx, p->pvi));
        p->dict = vd.dict;
        p->ndict = vd.n;
        return CUDAMAT_OK;
    }
    return launch_refresh_values(st, len, map, val, p->pv);
}

}  // namespace

int set_values(cudamat_solver *s, const double *val)
{
    CM_ARG(!s->sharded, "set_values: a sharded solver's values are not refreshed (single GPU, whole matrix only)");
    CM_ARG(val || s->nnz == 0, "set_values: val is NULL");
    cudamat_ctx *ctx = s->ctx;
    CM_HIP(hipSetDevice(ctx->device));
    Range range_values("cudamat: new values on the kept structure");
    hipStream_t st = ctx->stream;
    const int64_t nnz = s->nnz;
    CM_HIP(hipStreamSynchronize(st));
    const double t0 = now_s();
    // ---- what can fail for want of memory comes first: the solver is intact until the numbers start to change
    // the dictionary of the new values, by the rules of the creation (ensure_valdict); built from the caller's array
    const bool dict_wanted = nnz >= (1 << 20);
    ValDict nv;
    if (dict_wanted) CM_TRY(valdict_build(st, ctx->cfg, nnz, val, &nv));
    const bool new_dict = nv.n > 0;
    // storage classes: the copies in the caller's numbering follow s->vd, the permuted matrix' copy its own dictionary
    const bool main_changed = s->vd_tried && (s->vd.n > 0) != new_dict;
    const bool have_perm = s->perm_ready && s->pb_perm.P;
    const bool perm_changed = have_perm && (s->pb_perm.pvi != nullptr) != new_dict;
    // the maps this solver needs and does not have yet
    const bool need_pb = !main_changed && s->pb.P && !s->src_pb;
    const bool need_perm = have_perm && !perm_changed && !s->src_perm;
    if (need_pb || need_perm) {
        DevBuf<double> tags;
        DevBuf<int> m_pb, m_perm;
        int64_t l_pb = 0, l_perm = 0;
        CM_TRY(tags.alloc((size_t)nnz));
        CM_TRY(launch_value_tags(st, nnz, tags));
        if (need_pb) {
            Config cfg = ctx->cfg;
            cfg.pb_place = 0;                   // a temporary: nothing to place, nothing to print
            cfg.verbose = 0;
            PbCols cols;
            PbPlan tmp;
            CM_TRY(pb_build(st, cfg, s->n, s->n_cols, nnz, s->rp, s->ci, tags, &tmp, &cols, nullptr));
            const int rc = pb_value_map(st, s->pb, tmp, &m_pb, &l_pb);
            pb_free(&tmp);
            CM_TRY(rc);
        }
        if (need_perm) CM_TRY(ilu_perm_value_map(s, tags, &m_perm, &l_perm));
        if (need_pb) { s->src_pb = std::move(m_pb); s->src_pb_len = l_pb; }
        if (need_perm) { s->src_perm = std::move(m_perm); s->src_perm_len = l_perm; }
    }
    if (perm_changed) CM_TRY(ilu_perm_drop(s));      // (allocates the U positions before it lets go of anything)
    // ---- the numbers
    s->sym_known = false;                            // (the verdict of cudamat_solver_symmetry belonged to the old values)
    if (nnz) CM_HIP(hipMemcpyAsync(s->val, val, sizeof(double) * (size_t)nnz, hipMemcpyDeviceToDevice, st));
    if (dict_wanted) {
        s->vd = std::move(nv);                       // (the old dictionary goes here; every copy is re-pointed or dropped below)
        s->vd_tried = true;
    }
    SpmvPlan &plan = s->plan;
    if (main_changed) {
        spmv_copies_drop(s);
        if (plan.c_off16) {                          // the value stage of the CSR plan from scratch, as solver_setup_values runs it
            plan.a_base.reset(); plan.a_off16.reset(); plan.a_val.reset();
            plan.d_pbase.reset(); plan.d_off16.reset(); plan.d_val8.reset();
            plan.c_dict = nullptr;
            if (s->vd.n > 0) CM_TRY(plan_spmv_dict(st, s->n, nnz, s->rp, s->vd.idx, s->vd.dict, &plan));
            if (!plan.d_pbase) CM_TRY(plan_spmv_align(st, ctx->cfg, s->n, nnz, s->rp, s->val, &plan));
        }
    } else {
        CM_TRY(plan_spmv_refresh_values(st, s->n, nnz, s->rp, s->val, s->vd.idx, s->vd.n > 0 ? s->vd.dict.get() : nullptr, &plan));
        if (s->pb.P) CM_TRY(pb_refresh(st, &s->pb, s->src_pb, s->src_pb_len, s->val, s->vd));
        if (s->sell.val) CM_TRY(sell_refresh_values(st, s->sell, s->rp, s->val));
        if (s->pat.pid) CM_TRY(pat_refresh_values(st, &s->pat, s->rp, s->val, &s->vd));
    }
    if (have_perm && !perm_changed) {
        // the permuted matrix holds the same set of bit patterns, hence the same dictionary in the same ascending order: its copy
        // takes s->vd's indices through its map and s->vd's dictionary; its own dictionary is no longer needed
        CM_TRY(pb_refresh(st, &s->pb_perm, s->src_perm, s->src_perm_len, s->val, s->vd));
        if (s->pb_perm.pvi) valdict_free(&s->vd_perm);
    }
    if (hipStreamSynchronize(st) != hipSuccess) { set_error("value refresh failed"); return CUDAMAT_ERR_HIP; }
    s->ilu_stale = s->has_ilu;
    s->values_count++;
    s->values_rebuilt = main_changed || perm_changed ? 1 : 0;
    s->values_seconds = now_s() - t0;
    if (ctx->cfg.verbose)
        fprintf(stderr, "[cudamat] set_values %8.3f ms (value maps %s; %s%s)\n", s->values_seconds * 1e3,
                need_pb || need_perm ? "built" : "kept", s->values_rebuilt ? "storage class changed: SpMV form chosen again" : "copies refreshed in place",
                s->ilu_stale ? "; factors lag until the next factorisation" : "");
    return CUDAMAT_OK;
}

}  // namespace cm

extern "C" int cudamat_solver_set_values(cudamat_solver *s, const double *val)
{
    CM_ARG(s, "set_values: solver is NULL");
    return cm::set_values(s, val);
}

extern "C" int cudamat_solver_set_values_info(cudamat_solver *s, int *count, double *seconds_last, size_t *map_bytes, int *rebuilt_last)
{
    CM_ARG(s, "set_values info: solver is NULL");
    if (count) *count = s->values_count;
    if (seconds_last) *seconds_last = s->values_seconds;
    if (map_bytes) *map_bytes = sizeof(int) * ((size_t)s->src_pb_len + (size_t)s->src_perm_len);
    if (rebuilt_last) *rebuilt_last = s->values_rebuilt;
    return CUDAMAT_OK;
}
