/* cudamat_cg.h -- the constants of the conjugate-gradient loop: its loop id and its flag, beside those of cudamat.h (which
 * includes this file: include cudamat.h, not this).  The query the loop relies on, cudamat_solver_symmetry, is declared there. */
#ifndef CUDAMAT_CG_H
#define CUDAMAT_CG_H

/* loop selector for cudamat_solver_solve, beside CUDAMAT_LOOP_PBICGSTAB .. CUDAMAT_LOOP_BICGSTAB_L2 */
#define CUDAMAT_LOOP_CG 8           /* preconditioned conjugate gradients (Hestenes & Stiefel 1952) for SYMMETRIC POSITIVE
                                     * DEFINITE systems: not a loop of pbicgstab.cu, but what the reference's CPU program
                                     * (BiCG) computes on a symmetric matrix.  (4 - 7 are not loops: CUDAMAT_ERR_ARG.)  One
                                     * iteration is ONE product with A and ONE application of M^-1, where BiCGSTAB takes two
                                     * of each.  With r = b - A x0, nrm0 = ||r||, it = 0:
                                     *   z = M^-1 r                      (M = I: z is r)
                                     *   rho' = r.z; beta = it == 0 ? 0 : rho'/rho; rho = rho'; p = z + beta p
                                     *   q = (A0 + diag d) p; gamma = p.q
                                     *   alpha = rho/gamma; x += alpha p; r -= alpha q; nrm = ||r||; it++
                                     * ||r|| < tol nrm0 after the step is the only stopping test; the history has one entry
                                     * per iteration; the carried r is the true residual up to rounding.  half_exit = 0,
                                     * loop_form = 0.  breakdown = 1, converged = 0 when !(gamma > 0) (A is not positive
                                     * definite), !(rho' > 0) (M is not) or a scalar is not finite: the loop stops before the
                                     * vectors of that iteration are touched, the iteration is not counted, x is the last
                                     * completed iterate and r belongs to it.  CUDAMAT_FLAG_NO_EXIT takes none of these tests.
                                     * The matrix must be symmetric: the first solve asks cudamat_solver_symmetry and the
                                     * solve is CUDAMAT_ERR_ARG unless that reports (0, 0.0) or CUDAMAT_FLAG_ASSUME_SYMMETRIC
                                     * is given.  One GPU; PRECOND_NONE or PRECOND_ILU0 (the ILU(0) of a symmetric A is
                                     * L (D L^T): symmetric); a shift as for the other loops.  CUDAMAT_ERR_ARG for sharded
                                     * solvers, PRECOND_BLOCK_ILU0 and CUDAMAT_FLAG_GUARD (or the switch GUARD).  Batched
                                     * entry points run its columns one by one (form 0).                                 */

/* flag for cudamat_solver_solve, beside CUDAMAT_FLAG_DEBUG .. CUDAMAT_FLAG_GUARD */
#define CUDAMAT_FLAG_ASSUME_SYMMETRIC 32  /* CUDAMAT_LOOP_CG: skip the symmetry check of the matrix -- for matrices that are
                                       symmetric up to the rounding of their assembly (the check is exact: it knows no
                                       tolerance).  Ignored by the other loops.                                          */

#endif
