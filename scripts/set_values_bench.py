"""What new values on a kept structure cost against a fresh set-up, on the same arrays in the same process.

Cases (--case, default all; each runs in a child process of its own under a time limit, and the first one that fails ends the
run):
  c4          random 1e7 x 50, default switches (the blocked copy; the generator's values have a dictionary)
  c4-fp64     the same with VALUE_DICT = 0: fp64 values in every copy -- THE pass condition: steady set_values < fresh set-up
  c3          Poisson 4000 x 2500, default switches
  rand1e6-ilu random 1e6 x 50 with ILU(0): ilu0 + one preconditioned iteration (which builds the permuted matrix) before the
              first call; set_values + ilu0_refactor + one iteration on one side, close + create + SpMV + ilu0 + one iteration on
              the other
Per case, the stream drained before and after every timed call:
  (a) first     the first set_values (it builds the value maps): wall ms
  (b) steady    --reps (>= 5) later ones with alternating values (2 v1, v1: the storage class stays): median wall ms, the
                library's own seconds_last, and -- for forms with a map -- the refresh against its algorithmic bytes
  (c) fresh     close() + create + first SpMV on the same arrays (the form choice included): wall ms, --fresh-reps times
One JSON line per case at the end; "steady_below_fresh" is the pass condition where it applies.
  python scripts/set_values_bench.py [--case c4-fp64] [--reps 5] [--scale 1.0]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {                   # name: (kind, rows | (nx, ny), switches, ILU(0), seconds the child may take)
    "c4": ("rand", 10_000_000, {}, False, 420),
    "c4-fp64": ("rand", 10_000_000, {"VALUE_DICT": 0}, False, 420),
    "c3": ("poisson", (4000, 2500), {}, False, 240),
    "rand1e6-ilu": ("rand", 1_000_000, {}, True, 240),
}

ap = argparse.ArgumentParser()
ap.add_argument("--case", choices=list(CASES), default=None)
ap.add_argument("--child", action="store_true", help="run --case in this process (what the parent starts)")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--fresh-reps", type=int, default=3)
ap.add_argument("--scale", type=float, default=1.0, help="shrink every system (rows / grid side) by this factor: a quick look")
args = ap.parse_args()
assert args.reps >= 5

if not args.child:
    rc = 0
    for name in ([args.case] if args.case else list(CASES)):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--case", name, "--reps", str(args.reps),
               "--fresh-reps", str(args.fresh_reps), "--scale", str(args.scale)]
        try:
            rc = subprocess.run(cmd, timeout=CASES[name][4]).returncode
        except subprocess.TimeoutExpired:
            print("case %s ran into its time limit of %d s: stopping" % (name, CASES[name][4]), flush=True)
            rc = 124
        if rc != 0:              # (nothing more is started on the device after a failure)
            print("case %s ended with status %d: stopping" % (name, rc), flush=True)
            break
    sys.exit(rc)

import torch

import cuda_mat_amd as cm

dev = torch.device("cuda:0")
kind, size, switches, with_ilu, _ = CASES[args.case]
for k, v in switches.items():
    os.environ["CUDAMAT_" + k] = str(v)
ctx = cm.Context(0)
if kind == "rand":
    n = max(1024, int(size * args.scale))
    nnz = n * cm.lib().cudamat_rand_row_nnz(n, 50)
else:
    nx, ny = max(32, int(size[0] * args.scale)), max(32, int(size[1] * args.scale))
    n = nx * ny
    nnz = cm.lib().cudamat_poisson5_nnz(nx, ny)
rp = torch.empty(n + 1, dtype=torch.int32, device=dev)
ci = torch.empty(nnz, dtype=torch.int32, device=dev)
v1 = torch.empty(nnz, dtype=torch.float64, device=dev)
if kind == "rand":
    ctx.gen_rand_rows(n, 50, 1, 0, n, 0, rp, ci, v1)
else:
    ctx.gen_poisson5(nx, ny, 0, n, 0, rp, ci, v1)
ctx.sync()
nnz = int(rp[-1].item())
v2 = 2.0 * v1                        # (exact: as many distinct bit patterns as v1, so the storage class stays)
xs = torch.empty(n, dtype=torch.float64, device=dev)
ctx.gen_xstar(0, n, 2, xs)
b, x, y = torch.empty_like(xs), torch.empty_like(xs), torch.empty_like(xs)


def timed(fn):
    ctx.sync()
    t0 = time.perf_counter()
    fn()
    ctx.sync()
    return (time.perf_counter() - t0) * 1e3


def summary(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "reps": len(v)}


def show(label, v):
    s = summary(v)
    print("  %-58s median %10.3f ms   (min %.3f .. max %.3f, %d reps)" % (label, s["median"], s["min"], s["max"], s["reps"]), flush=True)
    return s


def one_iteration(s):
    return s.solve(b, x, precond=cm.PRECOND_ILU0, loop=cm.LOOP_PBICGSTAB, maxit=1, tol=1e-8, flags=cm.FLAG_NO_EXIT | cm.FLAG_X0_ONES)


def create(values):
    """what a caller without set_values does for new values: a solver from the arrays, its first SpMV (the form choice and every
    copy in another layout), and with ILU(0) the factors and the first preconditioned iteration (the permuted matrix)"""
    s = cm.Solver(ctx, n, n, nnz, rp, ci, values, 0)
    s.spmv(xs, y)
    if with_ilu:
        s.ilu0()
        one_iteration(s)
    return s


def refresh(s, values):
    s.set_values(values)
    if with_ilu:
        s.ilu0_refactor()
        one_iteration(s)


s = create(v1)
s.spmv(xs, b)
ctx.sync()
free0, total_mem = torch.cuda.mem_get_info()
print("%s: %s n=%d nnz=%d switches %s%s   kernel %s, value dictionary %d   (device memory free %.1f of %.1f GB)" %
      (args.case, kind, n, nnz, switches, " + ILU(0)" if with_ilu else "", s.spmv_kernel(), s.value_dict(), free0 / 2**30, total_mem / 2**30), flush=True)
first = timed(lambda: refresh(s, v2))
first_own = s.set_values_info()[1] * 1e3
map_bytes = s.set_values_info()[2]
steady, steady_own = [], []
for rep in range(args.reps + 1):                         # (rep 0: warm-up, not recorded)
    w = timed(lambda: refresh(s, v1 if rep % 2 == 0 else v2))
    assert s.set_values_info()[3] == 0 and s.set_values_info()[2] == map_bytes
    if rep:
        steady.append(w)
        steady_own.append(s.set_values_info()[1] * 1e3)
fresh = []
for rep in range(args.fresh_reps + 1):
    def again():
        global s
        s.close()
        s = create(v2 if rep % 2 == 0 else v1)
    w = timed(again)
    if rep:
        fresh.append(w)
print("  value maps %.1f MB; the first call took %.3f ms (the library's own figure: %.3f ms)" % (map_bytes / 1e6, first, first_own), flush=True)
c = show("(b) steady set_values%s, wall" % (" + ilu0_refactor + 1 iteration" if with_ilu else ""), steady)
co = show("    of that: set_values alone (seconds_last)", steady_own)
f = show("(c) fresh: close + create + SpMV%s, wall" % (" + ilu0 + 1 iteration" if with_ilu else ""), fresh)
entries = map_bytes // 4
per_entry = 6.0 if s.value_dict() else 20.0              # 4 map + 1 gathered + 1 stored, or 4 + 8 + 8
alg = per_entry * entries + 16.0 * nnz                   # ... + the copy into the solver's own values
print("  (b) / (c) = %.3f   set_values alone: %.3f GB algorithmic -> %.2f TB/s   %s" %
      (c["median"] / f["median"], alg / 1e9, alg / (co["median"] * 1e-3) / 1e12,
       "steady below fresh" if c["median"] < f["median"] else "THE REFRESH DOES NOT BEAT THE REBUILD HERE"), flush=True)
result = {"case": args.case, "n": n, "nnz": nnz, "kernel": s.spmv_kernel(), "value_dict": s.value_dict(), "map_bytes": map_bytes,
          "first_ms": first, "first_seconds_last_ms": first_own, "steady_ms": c, "steady_seconds_last_ms": co, "fresh_ms": f,
          "steady_below_fresh": c["median"] < f["median"]}
s.close()
ctx.close()
print(json.dumps(result), flush=True)
