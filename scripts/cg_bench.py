"""Conjugate gradients (CUDAMAT_LOOP_CG) against the BiCGSTAB loops on the same resident solver, on symmetric positive
definite systems.

One iteration of CG is one product with A (and one M^-1), one iteration of BiCGSTAB is two of each: the comparison runs both
over the same number of products.  Systems: the 5-point Poisson stencil on 2000 x 2000 and on 4000 x 2500 points, without and
with ILU(0).  Two JSON lines per (system, preconditioner):
  (a) "what": "per_iteration" -- ms per iteration and per product of LOOP_CG, and of LOOP_PBICGSTAB2 (no preconditioner) or
      LOOP_PBICGSTAB (ILU(0)), both FLAG_NO_EXIT over the same number of products: the device-side loop time
      (cudamat_stats.t_solve: a host clock around the enqueued loop and its final synchronise), best of --repeat runs of each
      loop, alternating, after one warm-up solve of each;
  (b) "what": "to_tolerance" -- products and seconds to tol = 1e-8 from x0 = 1 for both loops, with the true residual
      ||b - A x|| / ||r0|| of what each returned.
    python scripts/cg_bench.py [--products 400] [--products-ilu0 40] [--repeat 3] [--maxit 40000] [--small]
(the triangular solves of a stencil this size take tens of milliseconds each -- one level per grid diagonal -- so the
preconditioned timing windows are shorter.)
--small: 400 x 400 and 500 x 300 (a quick look; not the figures of DESIGN.md).
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import cuda_mat_amd as cm  # noqa: E402


def make(ctx, nx, ny):
    n = nx * ny
    nnz = int(cm.lib().cudamat_poisson5_nnz(nx, ny))
    rp, ci, v = ctx.empty(n + 1, np.int32), ctx.empty(nnz, np.int32), ctx.empty(nnz)
    ctx.gen_poisson5(nx, ny, 0, n, 0, rp, ci, v)
    return cm.Solver(ctx, n, n, nnz, rp, ci, v, 0), n, nnz, (rp, ci, v)


def one(s, db, dx, precond, loop, iters):
    """device-side loop seconds of one fixed-length solve from x0 = 1"""
    st = s.solve(db, dx, precond=precond, loop=loop, maxit=iters, tol=1e-8, flags=cm.FLAG_NO_EXIT | cm.FLAG_X0_ONES)
    assert st.iters == iters, (st.iters, iters)
    return st.t_solve


def timed_pair(s, db, dx, precond, other, products, repeat):
    """best of `repeat` runs of each loop over the same number of products, the two loops alternating; one warm-up solve of
    each first (set-up, the symmetry check, the choice of the SpMV form and the factors' layout happen there)"""
    runs = ((cm.LOOP_CG, products), (other, products // 2))
    for loop, iters in runs:
        one(s, db, dx, precond, loop, iters)
    best = [None, None]
    for _ in range(repeat):
        for k, (loop, iters) in enumerate(runs):
            t = one(s, db, dx, precond, loop, iters)
            best[k] = t if best[k] is None else min(best[k], t)
    return best


def true_residual(ctx, s, n, db, dx, work):
    """||b - A x|| through the solver's own product"""
    s.spmv(dx, work)
    ctx.scal(n, -1.0, work)
    ctx.axpy(n, 1.0, db, work)
    return ctx.nrm2(n, work)


def run(ctx, nx, ny, products_by_precond, repeat, maxit):
    name = "poisson%dx%d" % (nx, ny)
    s, n, nnz, keep = make(ctx, nx, ny)
    xs, db, dx, work = ctx.empty(n), ctx.empty(n), ctx.empty(n), ctx.empty(n)
    try:
        ctx.gen_xstar(0, n, 0x5EED + 1, xs)
        s.spmv(xs, db)
        assert s.symmetry() == (0, 0.0)
        for precond, pname, other, oname in ((cm.PRECOND_NONE, "none", cm.LOOP_PBICGSTAB2, "pbicgstab2"),
                                             (cm.PRECOND_ILU0, "ilu0", cm.LOOP_PBICGSTAB, "pbicgstab")):
            if precond:
                s.ilu0()
            products = products_by_precond[pname]
            head = {"system": name, "n": n, "nnz": nnz, "precond": pname, "other_loop": oname}
            t_cg, t_o = timed_pair(s, db, dx, precond, other, products, repeat)
            print(json.dumps(dict(head, what="per_iteration", products=products,
                                  cg_ms_per_iteration=1e3 * t_cg / products, cg_ms_per_product=1e3 * t_cg / products,
                                  other_ms_per_iteration=1e3 * t_o / (products // 2), other_ms_per_product=1e3 * t_o / products,
                                  cg_over_other_per_product=t_cg / t_o, spmv_kernel=s.spmv_kernel())), flush=True)
            out = dict(head, what="to_tolerance", tol=1e-8)
            for loop, lname, per in ((cm.LOOP_CG, "cg", 1), (other, oname, 2)):
                st = s.solve(db, dx, precond=precond, loop=loop, maxit=maxit * (2 // per), tol=1e-8, flags=cm.FLAG_X0_ONES)
                out[lname] = {"iters": st.iters, "converged": st.converged, "breakdown": st.breakdown, "half_exit": st.half_exit,
                              "products": per * st.iters + st.half_exit + 1, "seconds": st.t_solve,
                              "true_residual_over_nrm0": true_residual(ctx, s, n, db, dx, work) / st.nrm0}
            print(json.dumps(out), flush=True)
    finally:
        for a in (xs, db, dx, work) + tuple(keep):
            a.free()
        s.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--products", type=int, default=400)
    ap.add_argument("--products-ilu0", type=int, default=40)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--maxit", type=int, default=40000, help="BiCGSTAB iterations to tolerance at most (CG: twice as many)")
    ap.add_argument("--small", action="store_true")
    args = ap.parse_args()
    assert args.products % 2 == 0 and args.products_ilu0 % 2 == 0
    ctx = cm.Context(0)
    try:
        for nx, ny in (((400, 400), (500, 300)) if args.small else ((2000, 2000), (4000, 2500))):
            run(ctx, nx, ny, {"none": args.products, "ilu0": args.products_ilu0}, args.repeat, args.maxit)
    finally:
        ctx.close()


if __name__ == "__main__":
    main()
