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

}  // namespace cm
