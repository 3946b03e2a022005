// values.h -- new numbers on a kept structure (internal API; see values.hip): the gather family dst[i] = src[map[i]] that
// refreshes every stored copy of a value array through a "stored entry -> source position" map, the tags such a map is read
// from, and the refresh of a resident matrix' own values (cudamat_solver_set_values).
#pragma once
#include "common.h"
#include "spmv_pb.h"

struct cudamat_solver;

namespace cm {

// to[i] = from[map[i]] for i < count; map[i] == -1 (an alignment pad of a blocked copy) -> 0.  fp64: what ilu0_refactor runs
// (pairs of entries per thread where `to` is 16-byte and `map` 8-byte aligned).  Bytes: a thread produces 8 of them with two
// 16-byte map loads and one 8-byte store where `map` is 16-byte and `to` 8-byte aligned; scalar otherwise and for the tail.
int launch_refresh_values(hipStream_t s, int64_t count, const int *map, const double *from, double *to);
int launch_refresh_bytes(hipStream_t s, int64_t count, const int *map, const unsigned char *from, unsigned char *to);
// tag[i] = (double)(i + 1): a value array that tells where each of its entries came from once a builder has placed it
// (exact: positions stay below 2^31); map[i] = (int)tag[i] - 1, so that the 0.0 of a pad becomes -1
int launch_value_tags(hipStream_t s, int64_t count, double *tag);
int launch_map_from_tags(hipStream_t s, int64_t count, const double *tag, int *map);
// the map of the blocked copy `have`, read out of `tagged` -- the same builder run on tags with fp64 values -- after their
// shapes have been compared (the PB_* switches may have changed since `have` was built).  *len = entries the map covers
// (cstart[NCB]: the alignment pads between column blocks included).  The stream is drained on return.
int pb_value_map(hipStream_t st, const PbPlan &have, const PbPlan &tagged, DevBuf<int> *map, int64_t *len);

// ---- ilu.hip: the permuted matrix of the loop in level-major spaces (pb_perm)
// its map, through launch_sort_rows -> pb_build on tags (the tag carries the CSR position through the permutation)
int ilu_perm_value_map(cudamat_solver *s, const double *tags, DevBuf<int> *map, int64_t *len);
// its storage class changes: the copy goes, ilu_perm_matrix builds it again at the next preconditioned solve (the U positions
// it needs are recomputed here)
int ilu_perm_drop(cudamat_solver *s);

int set_values(cudamat_solver *s, const double *val);

}  // namespace cm
