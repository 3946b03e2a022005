"""BiCGSTAB(2) (Sleijpen & Fokkema 1993, l = 2) restated in numpy: test infrastructure for CUDAMAT_LOOP_BICGSTAB_L2, written
from the iteration stated in include/cudamat.h, shared by tests/test_bicgstab_l2_cpu.py and tests/test_gpu_bicgstab_l2.py.

Plain double arithmetic, dot products as np.dot.  One iteration = one sweep = four products with A^ = A M^-1 (right
preconditioning; A^ = A without M^-1):

    rho0 = -omega rho0
    j = 0:  rho1 = r0.r~ ; beta = alpha rho1 / rho0 ; rho0 = rho1 ; u0 = r0 - beta u0
            u1 = A^ u0 ; gamma = u1.r~ ; alpha = rho0 / gamma ; r0 -= alpha u1 ; y += alpha u0 ; r1 = A^ r0
    j = 1:  rho1 = r1.r~ ; beta = alpha rho1 / rho0 ; rho0 = rho1 ; u0 = r0 - beta u0 ; u1 = r1 - beta u1
            u2 = A^ u1 ; gamma = u2.r~ ; alpha = rho0 / gamma ; r0 -= alpha u1 ; r1 -= alpha u2 ; y += alpha u0 ; r2 = A^ r1
    MR:     [[r1.r1, r1.r2], [r1.r2, r2.r2]] (g1, g2) = (r1.r0, r2.r0)   by Cramer's rule HERE (the kernel eliminates on r1.r1,
            csrc/steps.h step_l2_mr: this file is an independent statement, compared to 1e-6, in range only -- the determinant
            leaves the range of a double under scalings the kernel survives)
            y += g1 r0 + g2 r1 ; u0 -= g1 u1 + g2 u2 ; r0 -= g1 r1 + g2 r2 ; omega = g2
            ||r0|| < tol ||r_init||: the only stopping test, one history entry per iteration

Start: rho0 = 1, alpha = 0, omega = 1, u0 = 0, r~ = r0 = b - A x0.  With M^-1, y starts at 0 and x = x0 + M^-1 y at the end;
without, y is x.  A breakdown (gamma = 0, the dividing rho0 = 0, a singular 2 x 2 system, any scalar not finite) stops the
loop at that iteration: breakdown = 1, converged = 0, the iteration is not counted.
"""
from dataclasses import dataclass

import numpy as np


@dataclass
class L2Result:
    x: np.ndarray
    iters: int
    converged: int
    breakdown: int
    nrm0: float
    nrm: float
    hist: np.ndarray


def _ok(*vals):
    return all(np.isfinite(v) for v in vals)


def bicgstab_l2(matvec, b, x0=None, minv=None, d=None, maxit=2000, tol=1e-8, no_exit=False):
    """matvec(v) = A0 v; d: optional shift, the operator is A0 + diag(d); minv(v) = M^-1 v or None."""
    b = np.asarray(b, dtype=np.float64)
    n = len(b)
    x = np.ones(n) if x0 is None else np.array(x0, dtype=np.float64)
    if d is not None:
        d = np.asarray(d, dtype=np.float64)

    def amul(v):
        w = matvec(v)
        return w if d is None else w + d * v

    def ahat(v):
        return amul(v if minv is None else minv(v))

    with np.errstate(all="ignore"):
        r0 = b - amul(x)
        rt = r0.copy()
        nrm0 = float(np.sqrt(np.dot(r0, r0)))
        y = x if minv is None else np.zeros(n)
        u0 = np.zeros(n)
        rho0, alpha, omega = 1.0, 0.0, 1.0
        hist, it, converged, breakdown, nrm = [], 0, 0, 0, nrm0
        exits = not no_exit          # FLAG_NO_EXIT: no test is taken, the scalars are divided as they come
        if nrm0 == 0.0:              # x0 solves the system: nothing to do
            converged = 1
        while not converged and it < maxit:
            rho0 = -omega * rho0
            # ---- j = 0
            rho1 = float(np.dot(r0, rt))
            if exits and (rho0 == 0.0 or not _ok(rho0, rho1)):
                breakdown = 1
                break
            beta = alpha * rho1 / rho0
            rho0 = rho1
            u0 = r0 - beta * u0
            u1 = ahat(u0)
            gamma = float(np.dot(u1, rt))
            if exits and (gamma == 0.0 or not _ok(gamma, beta)):
                breakdown = 1
                break
            alpha = rho0 / gamma
            if exits and (not _ok(alpha)):
                breakdown = 1
                break
            r0 = r0 - alpha * u1
            y += alpha * u0
            r1 = ahat(r0)
            # ---- j = 1
            rho1 = float(np.dot(r1, rt))
            if exits and (rho0 == 0.0 or not _ok(rho1)):
                breakdown = 1
                break
            beta = alpha * rho1 / rho0
            rho0 = rho1
            u0 = r0 - beta * u0
            u1 = r1 - beta * u1
            u2 = ahat(u1)
            gamma = float(np.dot(u2, rt))
            if exits and (gamma == 0.0 or not _ok(gamma, beta)):
                breakdown = 1
                break
            alpha = rho0 / gamma
            if exits and (not _ok(alpha)):
                breakdown = 1
                break
            r0 = r0 - alpha * u1
            r1 = r1 - alpha * u2
            y += alpha * u0
            r2 = ahat(r1)
            # ---- MR
            a11, a12, a22 = float(np.dot(r1, r1)), float(np.dot(r2, r1)), float(np.dot(r2, r2))
            b1, b2 = float(np.dot(r1, r0)), float(np.dot(r2, r0))
            det = a11 * a22 - a12 * a12
            if exits and (det == 0.0 or not _ok(det, b1, b2)):
                breakdown = 1
                break
            g1 = (b1 * a22 - b2 * a12) / det
            g2 = (a11 * b2 - a12 * b1) / det
            if exits and (not _ok(g1, g2)):
                breakdown = 1
                break
            y += g1 * r0 + g2 * r1
            u0 = u0 - (g1 * u1 + g2 * u2)
            r0 = r0 - (g1 * r1 + g2 * r2)
            omega = g2
            it += 1
            nrm = float(np.sqrt(np.dot(r0, r0)))
            hist.append(nrm)
            if no_exit:
                continue
            if nrm < tol * nrm0:
                converged = 1
            elif np.isnan(nrm):
                breakdown = 1
                break
        if minv is not None:
            x = x + minv(y)
    return L2Result(x, it, converged, breakdown, nrm0, nrm, np.array(hist))


def oracle_ops(O, A, vm=None):
    """(matvec, minv) on the oracle's kernels: A as oracle.Csr, vm its ILU(0) values (None: no preconditioner)"""
    def matvec(v):
        return O.spmv(A, v)
    if vm is None:
        return matvec, None

    def minv(v):
        return O.trsv_upper(A, vm, O.trsv_lower_unit(A, vm, v))
    return matvec, minv
