// trsm.h -- the ILU(0) factors applied to K interleaved columns at once (internal API, trsv.hip).
//
// Vectors are laid out as in batch.h: n rows x K columns row-major, K in {1, 2, 4, 8}.  The kernels are the ones trsv_apply
// launches at K = 1 (one implementation, trsv.hip), so column j of every solve here is bit-identical to trsv_apply on
// column j alone, whatever K is and whatever the other columns hold.
#pragma once
#include "solver.h"

namespace cm {

// Can this solver's factors go through the multi-column kernels?  They cover ILU(0) of the whole matrix on one GPU with the
// factors in the ORIGINAL index space.  Not covered (callers then work column by column): hybrid factors in level-major
// spaces (TriFactor::lm), block-Jacobi ILU(0), sharded solvers.
bool trsm_covered(cudamat_solver *s);
// which kernels one factor's solve with K columns launches: 2 single workgroup with the block in LDS, 0 level launches
int trsm_form_code(cudamat_solver *s, bool upper, int K);
// out = F^-1 rhs, K columns; rhs and out must not alias
int trsm_apply(cudamat_solver *s, const TriFactor &F, bool upper, int K, const double *rhs, double *out);
// out = U^-1 L^-1 in (pbicgstab.cu:92-98 / :121-127 for K columns); tmp: n x K scratch
int precond_apply_b(cudamat_solver *s, int K, const double *in, double *tmp, double *out);

// ---- one set of factor VALUES per column (the ILU(0) of A0 + diag(D_j), j < K, on the solver's pattern; ilu.hip builds them)
// Interleaved like the vectors: lu[p*K + j] on the matrix's pattern, lval / uval[k*K + j] in the level-major order of the
// solver's L / U (whose row pointers, column ids, row maps and levels are shared, not copied), dinv[pr*K + j] = 1 / U's diagonal.
struct ColFactors {
    double *lu = nullptr, *lval = nullptr, *uval = nullptr, *dinv = nullptr;
};
// The LDS the numeric ILU(0) stages a row in (the one place that says so; ilu.hip: launch_ilu0_levels).  Per wave and entry
// slot 8 K bytes of values and 12 bytes of tables (column id, the pivot's diagonal position, the end of its row), cap = the row
// rounded up to 64 plus 64 slots, against 150 KiB of the 160 KiB of a CU.  The longest row a K-wide factorisation stages,
// K = 1, 2, 4, 8: 7616, 5376, 3392, 1920.
constexpr size_t kIluLdsBudget = 150 * 1024;
// the single-column set-up and refactorisation take a prefetching kernel up to this many entry slots (cap), beyond it the
// unstaged one (k_ilu0_level_simple: 8 bytes per slot, rows up to kIluLdsBudget / 8 entries)
constexpr int kIluPrefetchCap = 1024;
inline size_t ilu0_slot_bytes(int K) { return (size_t)(8 * K + 12); }
inline int ilu0_cols_cap(int maxrow) { return ((maxrow + 63) / 64) * 64 + 64; }
inline int ilu0_cols_max_row(int K) { return (int)(kIluLdsBudget / ilu0_slot_bytes(K)) / 64 * 64 - 64; }
// waves (rows) per workgroup for that K and row length: 4, 2 or 1; 0: the row does not fit, the block runs column by column
inline int ilu0_cols_waves(int K, int maxrow)
{
    const size_t per_wave = (size_t)ilu0_cols_cap(maxrow) * ilu0_slot_bytes(K);
    const size_t w = kIluLdsBudget / per_wave;
    return w >= 4 ? 4 : w >= 2 ? 2 : (int)w;
}
// can this solver's structure carry a K-wide factorisation (trsm_covered and the LDS limit above)?
bool ilu0_cols_covered(cudamat_solver *s, int K);
// f = the factors of A0 + diag(D_c), c < kc (D column-major, leading dimension ldd; columns kc .. K-1 are padding and take
// column kc - 1's shift).  zp: one device word of scratch.  A zero pivot: CUDAMAT_ERR_ZERO_PIVOT, *zp_col / *zp_row the
// smallest (column, row) pair.  The solver's own factors are not touched.  Ends with the stream drained.
int ilu0_numeric_cols(cudamat_solver *s, int K, int kc, const double *D, int64_t ldd, const ColFactors &f, unsigned long long *zp,
                      int *zp_col, int *zp_row);
// out = F_j^-1 rhs_j per column j; rhs and out must not alias
int trsm_apply_cols(cudamat_solver *s, bool upper, int K, const double *val_b, const double *dinv_b, const double *rhs, double *out);
// out_j = U_j^-1 L_j^-1 in_j; tmp: n x K scratch
int precond_apply_cols(cudamat_solver *s, int K, const ColFactors &f, const double *in, double *tmp, double *out);

}  // namespace cm
