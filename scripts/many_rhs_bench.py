"""Several right-hand sides: the batched loop against k sequential solves, per config and batch width K.

One JSON line per (config, K): per-column iterations per second of the batched loop (MANY_FORM = batched) and of K
sequential Solver.solve calls (both FLAG_NO_EXIT, the same iteration count), the SpMM's time and its fraction of the HBM
roofline (bytes = 12 nnz + 4 (n + 1) + 8 K (n_cols + n)), and the form MANY_FORM = auto chose.
    python scripts/many_rhs_bench.py [--c4]        (--c4 adds the 1e7 x 50 random system, ~35 GB of device memory)

--precond ilu0: the same comparison for the preconditioned loop -- MANY_PRECOND = batched (multi-column triangular solves,
csrc/trsv.hip) against K sequential Solver.solve calls with ILU(0), on mat10000, the 4000 x 2500 stencil and a random
2e5 x 50 system (TRSV_HYBRID = 0 throughout: hybrid factors are not covered by the batched form), and what MANY_PRECOND = auto
picks.  --sequential-only measures just the K sequential solves and uses nothing newer than Solver.solve, so the same file
can be run against an older build of the library to take the sequential figure there.

--shifts: one shift vector per column, (A0 + I d_j) x_j = b_j (Solver.solve_shifts, MANY_FORM = batched) against (a) K
sequential set_shift + Solver.solve calls and (b) the shared-d batched loop (set_shift + Solver.solve_many) at the same K --
(a) and (b) use nothing newer than solve_many --, what MANY_FORM = auto picks with shifts, and the SpMM with per-column shifts
(bytes = 12 nnz + 4 (n + 1) + 8 K (n_cols + n) + 8 K n).  C2 is mat10000 with its diagonal split off and d_j = its diagonal
times (1 + j/8); the generated systems keep their matrix as A0 and get d_j = (1 + j)/8.  All FLAG_NO_EXIT.

--shifts --precond ilu0: the shifted family with one set of ILU(0) factors per column (Solver.solve_shifts_ilu0, MANY_PRECOND =
batched: K-wide factorisation + multi-column triangular solves with per-column values) against the column form as a caller
writes it -- per column set_shift + ilu0_refactor + Solver.solve, nothing newer on that side (--sequential-only runs just that).
D_j = (1 + j)/8 (0.5 + i/n) on mat10000, the 2000 x 2000 stencil and a random 2e5 x 50 system, K = 2, 4, 8, TRSV_HYBRID = 0.
Per (config, K): per-column it/s of both loops, factorisation ms per column of both, and the whole call per column.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import cuda_mat_amd as cm  # noqa: E402

HBM_PEAK = 8.0e12      # B/s, MI355X


def make(ctx, name):
    if name == "C2_mat10000":
        err, m, n, nnz, val, row, col = cm.loadMMSparseMatrix(os.path.join(ROOT, "tests", "golden", "mat10000.mtx"))
        rp, ci, v = ctx.array(row, np.int32), ctx.array(col, np.int32), ctx.array(val)
        return cm.Solver(ctx, n, n, nnz, rp, ci, v, int(row[0])), n, nnz, (rp, ci, v)
    if "poisson" in name:
        nx, ny = (int(q) for q in name.split("poisson")[1].split("x"))
        n = nx * ny
        nnz = int(cm.lib().cudamat_poisson5_nnz(nx, ny))
        rp, ci, v = ctx.empty(n + 1, np.int32), ctx.empty(nnz, np.int32), ctx.empty(nnz)
        ctx.gen_poisson5(nx, ny, 0, n, 0, rp, ci, v)
    else:
        n = 200_000 if name.startswith("rand2e5") else 2_000_000 if name.startswith("rand2e6") else 10_000_000
        nnz = n * int(cm.lib().cudamat_rand_row_nnz(n, 50))
        rp, ci, v = ctx.empty(n + 1, np.int32), ctx.empty(nnz, np.int32), ctx.empty(nnz)
        ctx.gen_rand_rows(n, 50, 0x5EED, 0, n, 0, rp, ci, v)
    return cm.Solver(ctx, n, n, nnz, rp, ci, v, 0), n, nnz, (rp, ci, v)


def run(name, iters):
    ctx = cm.Context(0)
    s, n, nnz, keep = make(ctx, name)
    out = []
    B, X, Y = ctx.empty(8 * n), ctx.empty(8 * n), ctx.empty(8 * n)
    for j in range(8):
        ctx.gen_xstar(0, n, 100 + j, X.ptr + 8 * j * n)
    s.spmm(8, X, n, B, n)
    tm = ctx.timer()
    for K in (1, 2, 4, 8):
        # SpMM
        s.spmm(K, X, n, Y, n)
        reps = 10
        tm.start()
        for _ in range(reps):
            s.spmm(K, X, n, Y, n)
        tm.stop()
        ms = tm.elapsed_ms() / reps
        nbytes = 12 * nnz + 4 * (n + 1) + 8 * K * (n + n)
        # batched
        ctx.set_option("MANY_FORM", "batched")
        check_x = ctx.empty(K * n)
        check_x.zero()
        s.solve_many(K, B, n, check_x, n, loop=cm.LOOP_PBICGSTAB, maxit=2, tol=1e-8, flags=cm.FLAG_NO_EXIT)   # warm-up
        check_x.zero()
        sts, form_b = s.solve_many(K, B, n, check_x, n, loop=cm.LOOP_PBICGSTAB, maxit=iters, tol=1e-8, flags=cm.FLAG_NO_EXIT)
        t_b = sts[0].t_solve
        # K sequential single solves
        t_s = 0.0
        for j in range(K):
            xj = check_x.ptr + 8 * j * n
            ctx.sync()
            st = s.solve(B.ptr + 8 * j * n, xj, loop=cm.LOOP_PBICGSTAB, maxit=iters, tol=1e-8, flags=cm.FLAG_NO_EXIT)
            t_s += st.t_solve
        # what auto picks (the first auto call of this solver times both forms)
        ctx.set_option("MANY_FORM", "auto")
        check_x.zero()
        sts_a, form_a = s.solve_many(K, B, n, check_x, n, loop=cm.LOOP_PBICGSTAB, maxit=iters, tol=1e-8, flags=cm.FLAG_NO_EXIT)
        check_x.free()
        line = {"config": name, "n": n, "nnz": nnz, "K": K, "iters": iters,
                "batched_col_it_s": K * iters / t_b, "sequential_col_it_s": K * iters / t_s,
                "gain_per_column": t_s / t_b, "spmm_ms": ms, "spmm_bytes": nbytes,
                "spmm_roofline": nbytes / (ms * 1e-3) / HBM_PEAK, "auto_form": "batched" if form_a else "columns",
                "auto_t_tune_s": sts_a[0].t_tune, "auto_col_it_s": K * iters / sts_a[0].t_solve}
        print(json.dumps(line), flush=True)
        out.append(line)
    for a in (B, X, Y):
        a.free()
    s.close()
    ctx.close()
    return out


def make_split(ctx, name):
    """make(), but mat10000 loses its diagonal: (solver of A0, n, nnz, kept arrays, the diagonal or None)"""
    if name != "C2_mat10000":
        return make(ctx, name) + (None,)
    err, m, n, nnz, val, row, col = cm.loadMMSparseMatrix(os.path.join(ROOT, "tests", "golden", "mat10000.mtx"))
    base = int(row[0])
    row_of = np.repeat(np.arange(n), np.diff(row))
    on_diag = (col - base) == row_of
    dg = np.zeros(n)
    dg[row_of[on_diag]] = val[on_diag]
    rp0 = np.zeros(n + 1, np.int32)
    np.cumsum(np.bincount(row_of[~on_diag], minlength=n), out=rp0[1:])
    rp, ci, v = ctx.array(rp0, np.int32), ctx.array((col[~on_diag] - base).astype(np.int32), np.int32), ctx.array(val[~on_diag])
    nnz0 = int(rp0[n])
    return cm.Solver(ctx, n, n, nnz0, rp, ci, v, 0), n, nnz0, (rp, ci, v), dg


def run_shifts(name, iters):
    ctx = cm.Context(0)
    s, n, nnz, keep, dg = make_split(ctx, name)
    B, X, Y = ctx.empty(8 * n), ctx.empty(8 * n), ctx.empty(8 * n)
    for j in range(8):
        ctx.gen_xstar(0, n, 100 + j, X.ptr + 8 * j * n)
    scale = [(1.0 + j / 8.0) if dg is not None else (1.0 + j) / 8.0 for j in range(8)]
    Dh = np.concatenate([(dg if dg is not None else np.ones(n)) * scale[j] for j in range(8)])
    D = ctx.array(Dh)
    del Dh
    s.spmm_shifts(8, X, n, D, n, B, n)
    tm = ctx.timer()
    kw = dict(loop=cm.LOOP_PBICGSTAB, tol=1e-8, flags=cm.FLAG_NO_EXIT)
    for K in (1, 2, 4, 8):
        s.spmm_shifts(K, X, n, D, n, Y, n)
        reps = 10
        tm.start()
        for _ in range(reps):
            s.spmm_shifts(K, X, n, D, n, Y, n)
        tm.stop()
        ms = tm.elapsed_ms() / reps
        nbytes = 12 * nnz + 4 * (n + 1) + 8 * K * (n + n) + 8 * K * n
        x = ctx.empty(K * n)
        # per-column shifts, batched
        ctx.set_option("MANY_FORM", "batched")
        x.zero()
        s.solve_shifts(K, D, n, B, n, x, n, maxit=2, **kw)                                       # warm-up
        x.zero()
        sts, form_k = s.solve_shifts(K, D, n, B, n, x, n, maxit=iters, **kw)
        t_k = sts[0].t_solve
        # (b) the shared-d batched loop: every column with d_0
        s.set_shift(D)
        x.zero()
        s.solve_many(K, B, n, x, n, maxit=2, **kw)                                               # warm-up
        x.zero()
        sts, form_b = s.solve_many(K, B, n, x, n, maxit=iters, **kw)
        t_b = sts[0].t_solve
        # (a) K sequential set_shift + solve
        t_s = 0.0
        for j in range(K):
            x.zero()
            ctx.sync()
            s.set_shift(D.ptr + 8 * j * n)
            st = s.solve(B.ptr + 8 * j * n, x.ptr + 8 * j * n, maxit=iters, **kw)
            t_s += st.t_solve
        s.set_shift(None)
        # what auto picks with shifts (the first such call of this solver per K times both forms)
        ctx.set_option("MANY_FORM", "auto")
        x.zero()
        sts_a, form_a = s.solve_shifts(K, D, n, B, n, x, n, maxit=iters, **kw)
        x.free()
        t_best = min(t_k, t_s)
        line = {"config": name, "shifts": "per column", "n": n, "nnz": nnz, "K": K, "iters": iters, "shifts_form": form_k,
                "shifts_col_it_s": K * iters / t_k, "shared_d_batched_col_it_s": K * iters / t_b,
                "sequential_col_it_s": K * iters / t_s, "gain_vs_sequential": t_s / t_k, "vs_shared_d_batched": t_b / t_k,
                "spmm_ms": ms, "spmm_bytes": nbytes, "spmm_roofline": nbytes / (ms * 1e-3) / HBM_PEAK,
                "auto_form": "batched" if form_a else "columns", "auto_t_tune_s": sts_a[0].t_tune,
                "auto_col_it_s": K * iters / sts_a[0].t_solve,
                "auto_picked_faster": (form_a == 1) == (t_k <= t_s), "faster_margin": abs(t_k - t_s) / t_best}
        print(json.dumps(line), flush=True)
    for a in (B, X, Y, D):
        a.free()
    s.close()
    ctx.close()


def run_precond(name, iters, sequential_only, build):
    ctx = cm.Context(0)
    ctx.set_option("TRSV_HYBRID", "0")
    s, n, nnz, keep = make(ctx, name)
    s.ilu0()
    B, X = ctx.empty(8 * n), ctx.empty(8 * n)
    for j in range(8):
        ctx.gen_xstar(0, n, 100 + j, X.ptr + 8 * j * n)
    for j in range(8):                       # (one SpMV per column: nothing newer than the single-vector interface)
        s.spmv(X.ptr + 8 * j * n, B.ptr + 8 * j * n)
    kw = dict(precond=cm.PRECOND_ILU0, loop=cm.LOOP_PBICGSTAB, tol=1e-8, flags=cm.FLAG_NO_EXIT)
    x = ctx.empty(8 * n)
    x.zero()
    st = s.solve(B, x, maxit=2, **kw)                                                            # warm-up
    for K in (1, 2, 4, 8):
        t_s = 0.0
        for j in range(K):
            x.zero()
            ctx.sync()
            st = s.solve(B.ptr + 8 * j * n, x.ptr + 8 * j * n, maxit=iters, **kw)
            t_s += st.t_solve
        line = {"config": name, "precond": "ilu0", "build": build, "n": n, "nnz": nnz, "K": K, "iters": iters,
                "levels": [st.n_levels_l, st.n_levels_u], "trsv_form_single": st.trsv_form,
                "sequential_col_it_s": K * iters / t_s, "sequential_s": t_s}
        if not sequential_only:
            ctx.set_option("MANY_PRECOND", "batched")
            x.zero()
            s.solve_many(K, B, n, x, n, maxit=2, **kw)                                           # warm-up
            x.zero()
            sts, form_b = s.solve_many(K, B, n, x, n, maxit=iters, **kw)
            t_b = sts[0].t_solve
            ctx.set_option("MANY_PRECOND", "auto")        # (the first auto call per K times both forms: t_tune)
            x.zero()
            sts_a, form_a = s.solve_many(K, B, n, x, n, maxit=iters, **kw)
            ctx.set_option("MANY_PRECOND", "columns")
            line.update({"batched_form": form_b, "batched_col_it_s": K * iters / t_b, "batched_s": t_b,
                         "gain_per_column_same_build": t_s / t_b, "trsm_kernel": s.trsm_kernel(K),
                         "auto_form": "batched" if form_a else "columns", "auto_t_tune_s": sts_a[0].t_tune,
                         "auto_col_it_s": K * iters / sts_a[0].t_solve})
        print(json.dumps(line), flush=True)
    for a in (B, X, x):
        a.free()
    s.close()
    ctx.close()


def run_shifts_precond(name, iters, sequential_only, build):
    ctx = cm.Context(0)
    ctx.set_option("TRSV_HYBRID", "0")
    s, n, nnz, keep = make(ctx, name)
    B, X = ctx.empty(8 * n), ctx.empty(8 * n)
    for j in range(8):
        ctx.gen_xstar(0, n, 100 + j, X.ptr + 8 * j * n)
    ramp = 0.5 + np.arange(n) / n
    D = ctx.array(np.concatenate([(1.0 + j) / 8.0 * ramp for j in range(8)]))
    for j in range(8):                       # b_j = (A0 + diag d_j) x*_j, one SpMV per column
        s.set_shift(D.ptr + 8 * j * n)
        s.spmv(X.ptr + 8 * j * n, B.ptr + 8 * j * n)
    s.set_shift(None)
    kw = dict(precond=cm.PRECOND_ILU0, loop=cm.LOOP_PBICGSTAB, tol=1e-8, flags=cm.FLAG_NO_EXIT)
    x = ctx.empty(8 * n)
    s.ilu0(shift=D)                          # the structure, and the first factors
    s.set_shift(D)
    x.zero()
    s.solve(B, x, maxit=2, **kw)             # warm-up
    for K in (2, 4, 8):
        t_s = t_f = 0.0
        for j in range(K):                   # the caller's loop: set_shift + ilu0_refactor + solve
            x.zero()
            ctx.sync()
            dj = D.ptr + 8 * j * n
            s.set_shift(dj)
            s.ilu0_refactor(dj)
            t_f += s.ilu0_refactor_info()[1]
            st = s.solve(B.ptr + 8 * j * n, x.ptr + 8 * j * n, maxit=iters, **kw)
            t_s += st.t_solve
        s.set_shift(None)
        line = {"config": name, "precond": "ilu0 per column", "build": build, "n": n, "nnz": nnz, "K": K, "iters": iters,
                "levels": [st.n_levels_l, st.n_levels_u], "trsv_form_single": st.trsv_form,
                "columns_col_it_s": K * iters / t_s, "columns_factor_ms_per_column": 1e3 * t_f / K,
                "columns_call_ms_per_column": 1e3 * (t_s + t_f) / K}
        if not sequential_only:
            ctx.set_option("MANY_PRECOND", "batched")
            x.zero()
            s.solve_shifts_ilu0(K, D, n, B, n, x, n, maxit=2, tol=1e-8, flags=cm.FLAG_NO_EXIT)          # warm-up
            x.zero()
            sts, form_b = s.solve_shifts_ilu0(K, D, n, B, n, x, n, maxit=iters, tol=1e-8, flags=cm.FLAG_NO_EXIT)
            ctx.set_option("MANY_PRECOND", "columns")
            t_b, t_fb = sts[0].t_solve, sts[0].t_factor
            line.update({"batched_form": form_b, "batched_col_it_s": K * iters / t_b, "batched_factor_ms_per_column": 1e3 * t_fb / K,
                         "batched_call_ms_per_column": 1e3 * (t_b + t_fb) / K, "loop_gain_per_column": t_s / t_b,
                         "factor_gain_per_column": t_f / t_fb, "call_gain_per_column": (t_s + t_f) / (t_b + t_fb),
                         "trsm_kernel": s.trsm_kernel(K)})
        print(json.dumps(line), flush=True)
    for a in (B, X, x, D):
        a.free()
    s.close()
    ctx.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--c4", action="store_true")
    ap.add_argument("--precond", choices=["none", "ilu0"], default="none")
    ap.add_argument("--shifts", action="store_true", help="one shift vector per column: solve_shifts against its two yardsticks")
    ap.add_argument("--sequential-only", action="store_true")
    ap.add_argument("--build", default="this", help="label of the library build in the output lines")
    ap.add_argument("--only", default="", help="run the configs whose name contains this")
    a = ap.parse_args()
    if a.precond == "ilu0" and a.shifts:
        for name, it in [("C2_mat10000", 100), ("poisson2000x2000", 3), ("rand2e5x50", 30)]:
            if a.only in name:
                run_shifts_precond(name, it, a.sequential_only, a.build)
        sys.exit(0)
    if a.precond == "ilu0":
        for name, it in [("C2_mat10000", 100), ("C3_poisson4000x2500", 3), ("rand2e5x50", 30)]:
            if a.only in name:
                run_precond(name, it, a.sequential_only, a.build)
        sys.exit(0)
    configs = [("C2_mat10000", 500), ("C3_poisson4000x2500", 30), ("rand2e6x50", 30)]
    if a.c4:
        configs.append(("C4_rand1e7x50", 10))
    for name, it in configs:
        if a.only in name:
            (run_shifts if a.shifts else run)(name, it)
