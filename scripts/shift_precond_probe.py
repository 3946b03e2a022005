"""ad-hoc: the ILU(0) loop with a shift against the same loop without one, on the same solver in the same process.

random 1e6 x 50 and Poisson 2000 x 2000, shift d_i = 0.25 mean|diag| (0.5 + i / n).  Per matrix and per TRSV_PERM in (1, 0):
  ilu0(shift=d)            one call, wall ms (analysis + factorisation + factor layout)
  shifted   loop           set_shift(d), ILU(0) loop, FLAG_NO_EXIT: ms per iteration (the solve's own loop time)
  unshifted loop           set_shift(None), the SAME factors and iteration count: ms per iteration
The two loops do the same work apart from the shift term of the two SpMVs and the per-solve gather of d into L's order.
  python scripts/shift_precond_probe.py [--rows 1000000] [--nx 2000] [--iters 20] [--reps 3]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import cuda_mat_amd as cm

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=1_000_000)
ap.add_argument("--per-row", type=int, default=50)
ap.add_argument("--nx", type=int, default=2000)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--reps", type=int, default=3)
args = ap.parse_args()
dev = torch.device("cuda:0")


def system(ctx, which):
    if which == "rand":
        n = args.rows
        nnz = n * cm.lib().cudamat_rand_row_nnz(n, args.per_row)
    else:
        n = args.nx * args.nx
        nnz = 5 * n
    rp = torch.empty(n + 1, dtype=torch.int32, device=dev)
    ci = torch.empty(nnz, dtype=torch.int32, device=dev)
    va = torch.empty(nnz, dtype=torch.float64, device=dev)
    if which == "rand":
        ctx.gen_rand_rows(n, args.per_row, 1, 0, n, 0, rp, ci, va)
    else:
        ctx.gen_poisson5(args.nx, args.nx, 0, n, 0, rp, ci, va)
    ctx.sync()
    nnz = int(rp[-1].item())
    rows = torch.repeat_interleave(torch.arange(n, device=dev), (rp[1:] - rp[:-1]).long())
    diag = va[:nnz][ci[:nnz].long() == rows]
    assert diag.numel() == n
    d = 0.25 * float(diag.abs().mean()) * (0.5 + torch.arange(n, dtype=torch.float64, device=dev) / n)
    return n, nnz, rp, ci, va, d


def loop_ms(s, b, x, iters):
    best = None
    for _ in range(args.reps):
        st = s.solve(b, x, precond=cm.PRECOND_ILU0, loop=cm.LOOP_PBICGSTAB, maxit=iters, tol=1e-8,
                     flags=cm.FLAG_NO_EXIT | cm.FLAG_X0_ONES)
        assert st.iters == iters
        ms = st.t_solve * 1e3 / iters
        best = ms if best is None else min(best, ms)
    return best


for which in ("rand", "poisson"):
    for perm in (1, 0):
        os.environ["CUDAMAT_TRSV_PERM"] = str(perm)
        ctx = cm.Context(0)
        n, nnz, rp, ci, va, d = system(ctx, which)
        s = cm.Solver(ctx, n, n, nnz, rp, ci, va, 0)
        xs = torch.empty(n, dtype=torch.float64, device=dev)
        ctx.gen_xstar(0, n, 2, xs)
        b, x = torch.empty_like(xs), torch.empty_like(xs)
        s.set_shift(d)
        s.spmv(xs, b)                       # b = (A0 + d) x*
        ctx.sync()
        t0 = time.perf_counter()
        s.ilu0(shift=d)
        ctx.sync()
        t_ilu = (time.perf_counter() - t0) * 1e3
        loop_ms(s, b, x, 2)                 # first solve: the permuted copy of the matrix, work vectors
        shifted = loop_ms(s, b, x, args.iters)
        s.set_shift(None)
        plain = loop_ms(s, b, x, args.iters)
        print("%-7s n=%d nnz=%d TRSV_PERM=%d  ilu0(shift) %8.1f ms | per iteration: shifted %7.3f ms, unshifted %7.3f ms (+%.1f %%)"
              % (which, n, nnz, perm, t_ilu, shifted, plain, 100.0 * (shifted / plain - 1.0)), flush=True)
        s.close()
        del rp, ci, va, d, xs, b, x
        torch.cuda.empty_cache()
        ctx.close()
