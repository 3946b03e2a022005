"""What a numeric-only ILU(0) refactorisation costs against a fresh set-up, on the same solver in the same process.

Systems: random n x 50 (--rows, default 1e6; 1e7 is the C5 size) and Poisson nx x nx (--nx, default 2000; 0 skips it), shift
d_i = 0.25 mean|diag| (0.5 + i / n), the default switches.  Per system, after one untimed round of everything (warm-up: kernels
loaded, pool filled), --reps repetitions (>= 5) of each, the stream drained before and after every timed call; median and
min .. max are printed:
  (a) fresh      ilu0(shift=d) + a one-iteration preconditioned solve (which builds the permuted matrix of the level-major
                 loop): wall ms of the two calls, and the statistics' t_analysis and t_factor after that solve
  (b) first      the first ilu0_refactor after a fresh set-up (it builds the value maps): wall ms
  (c) steady     ilu0_refactor with alternating shifts: wall ms, and the library's own seconds_last
  (d) refresh    with VERBOSE = 1 the library stamps the parts of a refactorisation (each between two drains of the stream):
                 `numeric ILU(0)` and `value refresh`; the latter against its algorithmic bytes (20 per stored entry of a split
                 factor: 4 map + 8 gathered + 8 stored; unsplit factors: the fill kernel, reported in ms only)
and the bytes of the maps.  One JSON line per system at the end.
  python scripts/refactor_bench.py [--rows 1000000] [--nx 2000] [--reps 5]"""
import argparse
import json
import os
import re
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import cuda_mat_amd as cm

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=1_000_000)
ap.add_argument("--per-row", type=int, default=50)
ap.add_argument("--nx", type=int, default=2000)
ap.add_argument("--reps", type=int, default=5)
args = ap.parse_args()
assert args.reps >= 5
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
    # mean |diagonal| without an nnz-sized temporary per step (the C5 size): the diagonal through a chunked scan
    total, chunk = 0.0, 1 << 26
    rows_of = torch.repeat_interleave(torch.arange(n, device=dev, dtype=torch.int32), (rp[1:] - rp[:-1]))
    for k0 in range(0, nnz, chunk):
        k1 = min(nnz, k0 + chunk)
        m = ci[k0:k1] == rows_of[k0:k1]
        total += float(va[k0:k1][m].abs().sum())
    del rows_of
    d = 0.25 * (total / n) * (0.5 + torch.arange(n, dtype=torch.float64, device=dev) / n)
    return n, nnz, rp, ci, va, d


def timed(ctx, fn):
    ctx.sync()
    t0 = time.perf_counter()
    fn()
    ctx.sync()
    return (time.perf_counter() - t0) * 1e3


def summary(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "reps": len(v)}


def show(label, v, unit="ms"):
    s = summary(v)
    print("  %-46s median %10.3f %s   (min %.3f .. max %.3f, %d reps)" % (label, s["median"], unit, s["min"], s["max"], s["reps"]), flush=True)
    return s


class Stderr:
    """the library's stderr lines of a block, through a temporary file (file descriptor 2 is the C library's)"""
    def __enter__(self):
        sys.stderr.flush()
        self.tmp = tempfile.TemporaryFile(mode="w+b")
        self.saved = os.dup(2)
        os.dup2(self.tmp.fileno(), 2)
        return self

    def __exit__(self, *exc):
        os.dup2(self.saved, 2)
        os.close(self.saved)
        self.tmp.seek(0)
        self.text = self.tmp.read().decode(errors="replace")
        self.tmp.close()
        return False


results = []
for which in ("rand", "poisson"):
    if which == "poisson" and args.nx <= 0:
        continue
    ctx = cm.Context(0)
    n, nnz, rp, ci, va, d = system(ctx, which)
    d2 = 8.0 * d
    s = cm.Solver(ctx, n, n, nnz, rp, ci, va, 0)
    xs = torch.empty(n, dtype=torch.float64, device=dev)
    ctx.gen_xstar(0, n, 2, xs)
    b, x = torch.empty_like(xs), torch.empty_like(xs)
    s.set_shift(d)
    s.spmv(xs, b)
    ctx.sync()
    free0, total_mem = torch.cuda.mem_get_info()
    print("%s n=%d nnz=%d   (device memory free %.1f of %.1f GB)" % (which, n, nnz, free0 / 2**30, total_mem / 2**30), flush=True)

    def one_solve():
        return s.solve(b, x, precond=cm.PRECOND_ILU0, loop=cm.LOOP_PBICGSTAB, maxit=1, tol=1e-8, flags=cm.FLAG_NO_EXIT | cm.FLAG_X0_ONES)

    fresh_wall, fresh_factor, fresh_analysis, first_wall = [], [], [], []
    for rep in range(args.reps + 1):                     # (rep 0: warm-up, not recorded)
        stats = []
        w = timed(ctx, lambda: (s.ilu0(shift=d), stats.append(one_solve())))
        f = timed(ctx, lambda: s.ilu0_refactor(d2))
        if rep:
            fresh_wall.append(w)
            fresh_factor.append(stats[0].t_factor * 1e3)
            fresh_analysis.append(stats[0].t_analysis * 1e3)
            first_wall.append(f)
    st = one_solve()
    groups = (st.trsv_groups_l, st.trsv_groups_u)
    map_bytes = s.ilu0_refactor_info()[2]
    steady_wall, steady_own = [], []
    for rep in range(args.reps + 1):
        w = timed(ctx, lambda: s.ilu0_refactor(d if rep % 2 == 0 else d2))
        if rep:
            steady_wall.append(w)
            steady_own.append(s.ilu0_refactor_info()[1] * 1e3)
    ctx.set_option("VERBOSE", 1)
    with Stderr() as cap:
        for rep in range(args.reps):
            s.ilu0_refactor(d2 if rep % 2 == 0 else d)
    ctx.set_option("VERBOSE", 0)
    numeric = [float(v) for v in re.findall(r"ilu0 numeric ILU\(0\)\s+([0-9.]+) ms", cap.text)]
    refresh = [float(v) for v in re.findall(r"ilu0 value refresh\s+([0-9.]+) ms", cap.text)]
    assert len(numeric) == args.reps and len(refresh) == args.reps, cap.text
    print("  factors split into groups (L, U): %s; value maps %.1f MB" % (groups, map_bytes / 1e6))
    a = show("(a) fresh ilu0(shift) + first solve, wall", fresh_wall)
    af = show("    of that: t_factor (numbers, split, permuted copy)", fresh_factor)
    aa = show("    of that: t_analysis (both level analyses)", fresh_analysis)
    bb = show("(b) first refactor (builds the maps), wall", first_wall)
    c = show("(c) steady refactor, wall", steady_wall)
    co = show("    the library's seconds_last", steady_own)
    dn = show("(d) numeric ILU(0) alone", numeric)
    dr = show("(d) value refresh alone", refresh)
    entries = map_bytes // 4
    alg = 20.0 * entries + 24.0 * n
    tbs = alg / (dr["median"] * 1e-3) / 1e12 if entries else 0.0
    print("  (c) / (a) = %.3f   (c) / t_factor of (a) = %.3f   refresh: %.3f GB algorithmic -> %.2f TB/s" %
          (c["median"] / a["median"], c["median"] / af["median"], alg / 1e9 if entries else 0.0, tbs))
    if bb["median"] > a["median"] and a["median"] > c["median"]:
        print("  (b) exceeds (a): the maps have paid for themselves after %.1f refactorisations" % ((bb["median"] - c["median"]) / (a["median"] - c["median"])))
    results.append({"system": which, "n": n, "nnz": nnz, "groups": groups, "map_bytes": map_bytes, "fresh_wall_ms": a, "fresh_t_factor_ms": af,
                    "fresh_t_analysis_ms": aa, "first_refactor_ms": bb, "steady_refactor_ms": c, "steady_seconds_last_ms": co,
                    "numeric_ms": dn, "refresh_ms": dr, "refresh_alg_bytes": alg if entries else 0.0, "refresh_TBps": tbs,
                    "steady_below_fresh": c["median"] < af["median"]})
    s.close()
    del rp, ci, va, d, d2, xs, b, x
    torch.cuda.empty_cache()
    ctx.close()
for r in results:
    print(json.dumps(r), flush=True)
