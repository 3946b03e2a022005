"""BiCGSTAB(2) (CUDAMAT_LOOP_BICGSTAB_L2) against two iterations of CUDAMAT_LOOP_PBICGSTAB2 on the same resident solver.

One sweep of the new loop is four products with A (M^-1 A), two iterations of BiCGSTAB are four as well: the comparison is
like for like.  One JSON line per (system, preconditioner): ms per sweep and per product of the new loop, ms per two
iterations and per product of LOOP_PBICGSTAB2, their ratio -- both FLAG_NO_EXIT over the same number of products, the
device-side loop time (cudamat_stats.t_solve: a host clock around the enqueued loop and its final synchronise), best of
--repeat runs of each loop, alternating, after one warm-up solve of each.  Systems: the 5-point stencil on 2000 x 2000 points
and the random 1e6 x 50 matrix, without and with ILU(0).  A last line: products to tol = 1e-8 on convdiff_g2 of
tests/nondominant.py (4 per sweep + 1 against 2 per iteration + 1).
    python scripts/bicgstab_l2_bench.py [--sweeps 200] [--repeat 3] [--small]
--small: 400 x 400 and 1e5 x 50 (a quick look; not the figures of DESIGN.md).
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import cuda_mat_amd as cm  # noqa: E402


def make(ctx, name):
    if name.startswith("poisson"):
        nx, ny = (int(q) for q in name[len("poisson"):].split("x"))
        n = nx * ny
        nnz = int(cm.lib().cudamat_poisson5_nnz(nx, ny))
        rp, ci, v = ctx.empty(n + 1, np.int32), ctx.empty(nnz, np.int32), ctx.empty(nnz)
        ctx.gen_poisson5(nx, ny, 0, n, 0, rp, ci, v)
    else:
        n = int(float(name[len("rand"):].split("x")[0]))
        nnz = n * int(cm.lib().cudamat_rand_row_nnz(n, 50))
        rp, ci, v = ctx.empty(n + 1, np.int32), ctx.empty(nnz, np.int32), ctx.empty(nnz)
        ctx.gen_rand_rows(n, 50, 0x5EED, 0, n, 0, rp, ci, v)
    return cm.Solver(ctx, n, n, nnz, rp, ci, v, 0), n, nnz, (rp, ci, v)


def one(s, db, dx, precond, loop, iters):
    """device-side loop seconds of one fixed-length solve from x0 = 1"""
    st = s.solve(db, dx, precond=precond, loop=loop, maxit=iters, tol=1e-8, flags=cm.FLAG_NO_EXIT | cm.FLAG_X0_ONES)
    assert st.iters == iters, (st.iters, iters)
    return st.t_solve


def timed_pair(s, db, dx, precond, sweeps, repeat):
    """best of `repeat` runs of each loop over the same number of products, the two loops alternating; one warm-up solve of
    each first (set-up, the choice of the SpMV form and the factors' layout happen there)"""
    runs = ((cm.LOOP_BICGSTAB_L2, sweeps), (cm.LOOP_PBICGSTAB2, 2 * sweeps))
    for loop, iters in runs:
        one(s, db, dx, precond, loop, iters)
    best = [None, None]
    for _ in range(repeat):
        for k, (loop, iters) in enumerate(runs):
            t = one(s, db, dx, precond, loop, iters)
            best[k] = t if best[k] is None else min(best[k], t)
    return best


def run(ctx, name, sweeps, repeat):
    s, n, nnz, keep = make(ctx, name)
    xs, db, dx = ctx.empty(n), ctx.empty(n), ctx.empty(n)
    try:
        ctx.gen_xstar(0, n, 0x5EED + 1, xs)
        s.spmv(xs, db)
        for precond, pname in ((cm.PRECOND_NONE, "none"), (cm.PRECOND_ILU0, "ilu0")):
            if precond:
                s.ilu0()
            t_l2, t_b2 = timed_pair(s, db, dx, precond, sweeps, repeat)
            print(json.dumps({"system": name, "n": n, "nnz": nnz, "precond": pname, "sweeps": sweeps,
                              "l2_ms_per_sweep": 1e3 * t_l2 / sweeps, "l2_ms_per_product": 1e3 * t_l2 / (4 * sweeps),
                              "pbicgstab2_ms_per_2_iterations": 1e3 * t_b2 / sweeps, "pbicgstab2_ms_per_product": 1e3 * t_b2 / (4 * sweeps),
                              "l2_over_pbicgstab2": t_l2 / t_b2, "spmv_kernel": s.spmv_kernel()}), flush=True)
    finally:
        for a in (xs, db, dx) + tuple(keep):
            a.free()
        s.close()


def products_to_tolerance(ctx):
    from oracle import oracle as O
    from tests import nondominant as ND
    O.build()
    O.lib()
    A, b = ND.FAMILY["convdiff_g2"](O)
    s = cm.Solver.from_host_csr(ctx, A.rowptr, A.colidx, A.val)
    db, dx = ctx.array(b), ctx.empty(A.n)
    try:
        out = {"system": "convdiff_g2", "n": A.n, "tol": 1e-8}
        for loop, lname, per in ((cm.LOOP_BICGSTAB_L2, "l2", 4), (cm.LOOP_PBICGSTAB2, "pbicgstab2", 2)):
            st = s.solve(db, dx, loop=loop, maxit=2000, tol=1e-8, flags=cm.FLAG_X0_ONES)
            x = dx.download()
            out[lname] = {"iters": st.iters, "converged": st.converged, "products": per * st.iters + 1, "ms": 1e3 * st.t_solve,
                          "true_residual_over_nrm0": ND.true_res(O, A, b, x) / st.nrm0}
        print(json.dumps(out), flush=True)
    finally:
        db.free()
        dx.free()
        s.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sweeps", type=int, default=200)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--small", action="store_true")
    args = ap.parse_args()
    ctx = cm.Context(0)
    try:
        for name in (("poisson400x400", "rand1e5x50") if args.small else ("poisson2000x2000", "rand1e6x50")):
            run(ctx, name, args.sweeps, args.repeat)
        products_to_tolerance(ctx)
    finally:
        ctx.close()


if __name__ == "__main__":
    main()
