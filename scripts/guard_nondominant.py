"""What CUDAMAT_FLAG_GUARD does to the 15 non-dominant systems of tests/nondominant.py: every system through
gpu_pbicgstab with M = I, the (A0 + I d) loop with d = 0 and gpu_pbicgstab with ILU(0), without and with the flag -- outcome class,
iterations, rho_restarts, restarts and the true relative residual ||b - A x|| / ||r0||.  Needs a GPU.
    python scripts/guard_nondominant.py > profiles/guard_nondominant.log"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import cuda_mat_amd as cm  # noqa: E402
from oracle import oracle as O  # noqa: E402
from tests import nondominant as ND  # noqa: E402

MAXIT, TOL = 2000, 1e-6


def outcome(st):
    return "breakdown" if st.breakdown else "converged" if st.converged else "maxit" if st.iters == MAXIT else "stopped"


def main():
    O.build()
    O.lib()
    ctx = cm.Context(0)
    print("%-22s %-9s %-6s | %-10s %5s %10s | %-10s %5s %4s %3s %10s" % ("system", "loop", "M", "unguarded", "iters", "true res", "guarded", "iters", "rho",
                                                                          "ver", "true res"))
    for name in ND.FAMILY:
        A, b = ND.FAMILY[name](O)
        for loop, precond in ((cm.LOOP_PBICGSTAB, 0), (cm.LOOP_PBICGSTAB2, 0), (cm.LOOP_PBICGSTAB, 1)):
            s = cm.Solver.from_host_csr(ctx, A.rowptr, A.colidx, A.val)
            db = ctx.array(b)
            row = []
            try:
                if precond:
                    s.ilu0()
                for flags in (0, cm.FLAG_GUARD):
                    dx = ctx.array(np.ones(A.n))
                    st = s.solve(db, dx, precond=precond, loop=loop, maxit=MAXIT, tol=TOL, flags=flags)
                    x = dx.download()
                    dx.free()
                    row.append((outcome(st), st.iters, st.rho_restarts, st.restarts, ND.true_res(O, A, b, x) / st.nrm0))
            except cm.CudamatError as e:
                print("%-22s %-9s %-6s | %s" % (name, "loop%d" % loop, "ILU(0)" if precond else "I", e))
                continue
            finally:
                db.free()
                s.close()
            (o0, i0, _, _, r0), (o1, i1, rr, vr, r1) = row
            print("%-22s %-9s %-6s | %-10s %5d %10.2e | %-10s %5d %4d %3d %10.2e" % (name, "loop%d" % loop, "ILU(0)" if precond else "I", o0, i0, r0, o1, i1,
                                                                                      rr, vr, r1))
    ctx.close()


if __name__ == "__main__":
    main()
