"""Hestenes-Stiefel preconditioned conjugate gradients restated in numpy: test infrastructure for CUDAMAT_LOOP_CG, written from
the iteration stated in include/cudamat_cg.h, shared by tests/test_cg_cpu.py and tests/test_gpu_cg.py.

Plain double arithmetic, dot products as np.dot.  With r = b - A x0, nrm0 = ||r||, it = 0:

    z = M^-1 r                  (M = I: z is r)
    rho' = r.z ;  beta = 0 if it == 0 else rho'/rho ;  rho = rho' ;  p = z + beta p
    q = (A0 + diag d) p ;  gamma = p.q
    alpha = rho/gamma ;  x += alpha p ;  r -= alpha q ;  nrm = ||r|| ;  it += 1
    stop when nrm < tol nrm0: the only stopping test, one history entry per iteration (slot it - 1)

One iteration is one product and one M^-1.  breakdown = 1, converged = 0 when not (gamma > 0), not (rho' > 0) or a scalar is not
finite: the loop stops before x, r (and, for rho', p) are touched, the iteration is not counted.  no_exit takes none of the tests.
"""
from dataclasses import dataclass

import numpy as np


@dataclass
class CgResult:
    x: np.ndarray
    iters: int
    converged: int
    breakdown: int
    nrm0: float
    nrm: float
    hist: np.ndarray


def cg(mv, b, x0=None, minv=None, d=None, maxit=2000, tol=1e-8, no_exit=False):
    """mv(v) = A0 v; d: optional shift, the operator is A0 + diag(d); minv(v) = M^-1 v or None."""
    b = np.asarray(b, dtype=np.float64)
    n = len(b)
    x = np.ones(n) if x0 is None else np.array(x0, dtype=np.float64)
    if d is not None:
        d = np.asarray(d, dtype=np.float64)

    def amul(v):
        w = mv(v)
        return w if d is None else w + d * v

    with np.errstate(all="ignore"):
        r = b - amul(x)
        nrm0 = float(np.sqrt(np.dot(r, r)))
        p = np.zeros(n)
        rho = 1.0
        hist, it, converged, breakdown, nrm = [], 0, 0, 0, nrm0
        exits = not no_exit
        if nrm0 == 0.0:              # x0 solves the system: nothing to do
            converged = 1
        while not converged and it < maxit:
            z = r if minv is None else minv(r)
            rho1 = float(np.dot(r, z))
            beta = 0.0 if it == 0 else rho1 / rho
            if exits and (not rho1 > 0.0 or not np.isfinite(rho1) or not np.isfinite(beta)):
                breakdown = 1
                break
            rho = rho1
            p = z + beta * p
            q = amul(p)
            gamma = float(np.dot(p, q))
            alpha = rho / gamma
            if exits and (not gamma > 0.0 or not np.isfinite(gamma) or not np.isfinite(alpha)):
                breakdown = 1
                break
            x = x + alpha * p
            r = r - alpha * q
            it += 1
            nrm = float(np.sqrt(np.dot(r, r)))
            hist.append(nrm)
            if no_exit:
                continue
            if nrm < tol * nrm0:
                converged = 1
            elif np.isnan(nrm):
                breakdown = 1
                break
    return CgResult(x, it, converged, breakdown, nrm0, nrm, np.array(hist))
