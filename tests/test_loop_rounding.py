"""The reference BiCGSTAB loops (pbicgstab.cu:67-151 and :581-754) as every loop form computes them, restated on the CPU bit
for bit: the steps of csrc/steps.h and the reduction orders of the kernels that call them.

  steps       step_p = fma(beta, fma(-omega, v, p), r) (two roundings), r -= alpha v, x += alpha p, x += omega s, r -= omega t
              (one fma each), every dot term fma(a, b, acc); beta = (rho / rho') (alpha / omega), alpha and omega one quotient
  a thread    vec_loop (device.h): VEC = 1 deals the n / 2 pairs grid-stride, .x before .y, then the odd tail; VEC = 0 and the
              K-column kernels of batch.hip deal single rows grid-stride
  a workgroup block_sum: xor butterfly 32 .. 1 inside a wave, then ((w0 + w1) + w2) + w3
  a launch    load_scalars / load_parts: thread j adds partials j, j + 256, ..., then block_sum; vec_grid workgroups for the
              vector kernels, spmv_partition for the SpMV's fused dots (k_spmv<L> and k_spmm_csr<L, K>: one group of L lanes
              per row, the group's first lane holds its rows' terms)

The loop forms (FORMS) differ in the thread dealing behind each group of dots and in nothing else:

  dots                form 0 (five launches)      form 1, lanes plan    form 1, stream plan        form 2 (one launch)
  r0.r0               k_init: vec_threads         the same              the same                   the same (first_count partials)
  rw.v, (t.s, t.t)    the SpMV's own: lanes/tile  spmv_threads(n, L)    tile                       tile
  ||s||^2             k_half: vec_threads         spmv_threads(n, L)    tile                       tile
  (rw.r, r.r)         k_full: vec_threads         k_full: vec_threads   k_full: vec_threads        tile

  tile                a stream tile (plan_spmv_refine, restated in stream_plan): R = 256 rows when no 256-row tile holds more than
                      kStreamNnz = 2048 entries, ceil(n / R) workgroups of one tile each below 2048 tiles; thread tid owns row
                      r0 + tid and holds ONE term (k_resident_loop writes that term as a plain product: fma(a, b, 0) has the same
                      bits).  Workgroups of more than one tile exist only above 524 288 rows, beyond what this mirror can
                      replay: stream_plan refuses them.
  scalars             every consumer forms a scalar with load_scalars; the third phase of k_resident_loop writes that order out by
                      hand (j = tid; j < G; j += kBlock, then block_sum) and the mirror uses the one function for it too
  row sums            a stream tile adds separately rounded products in column order, sum += fl(a_ij x_j) (stream_finish_rows,
                      k_fspmv_stream, k_resident_loop; the oracle's order); the lanes forms stay on the diagonal system
  shift               fma(d_i, x_i, sum) after the row sum (spmv_finish_row_fused, fused_finish_row_x, k_resident_loop), in r0 too
  LOOP_PBICGSTAB2     the same arithmetic; no half-step test, one history entry per iteration at slot it - 1, and the guard
                      |omega| < 1e-5 of device.h:212 (asserted not to fire)
  ILU(0), form 0      on the diagonal system L = I and U = diag(a): one application is tri_rows on empty rows, rhs - 0 and then
                      (. - 0) * dinv with dinv = fl(1 / a_i); pw = M^-1 p, v = A pw, s = M^-1 r, t = A s, the SpMV's dots are
                      (t.r, t.t), and k_full applies x += alpha pw, then x += omega s
  exits               tolabs = tol * nrm0 from the mirror's own nrm0 (k_init_finish); the full-step test of iteration it - 1 in
                      the prologue of iteration it (after the last one: k_check), the half-step test after ||s||^2; after an exit
                      at the half step x carries x += alpha p and nothing more (finish() in form 0, FUSE_HALF's unconditional
                      store in form 1, x_cur = x_half in form 2)

Two systems.  Diagonal (n = 601, entries in [1, 2)): a row sum of any SpMV form is the single rounding fl(a_i x_i), so only the
dot dealing has to be restated: of the forced lanes form (SPMV_LANES = 64) and of 3 stream tiles; n is odd (a tail), the vector
grid is 2 workgroups, the SpMV grids 151 and 3: none is a multiple of 8, so xcd_chunk / xcd_tile are the identity.  Banded
(n = 777, columns i, i +- 1, i +- 257; stream plans only): three full tiles and one of 9 rows, and every workgroup gathers p'
and s at rows another workgroup owns, so a stale or wrong half of the double buffers shows in bits.  b and x0 are standard
normal with fixed seeds.
The seeds are picked (SEEDS, inputs): at these n an accumulator of a vector kernel takes two or three terms and one of the SpMV a
single one, so for most right-hand sides a dot summed as fl(a b) + acc rounds to the very scalars the fma form gives and x cannot
tell the two apart (7 of the first 40 seeds can with pairs per thread, 3 with rows per thread); the p-update's third rounding
shows in 4 to 123 entries of x.  Columns 0 and 1 tell all three neighbours apart in the row dealings, column 2 in the pair
dealing, column 4 in the three-launch forms, column 8 in the single-launch form.
The GPU tests that pin the kernels to this mirror are test_loop_bits_* in test_gpu_parity.py and test_gpu_many_rhs.py; here,
without a GPU, the check that the mirror can tell the pinned arithmetic from its neighbours at all, on the inputs those use.
Not restated: the pipelined loop, sharded runs, solves that cross the 8192-iteration launch chunk of form 2."""
import collections
import functools
import math

import numpy as np

from test_spmv_rounding import MIN_DIFFERING_ROWS, fma

N, ITERS, LANES = 601, 3, 64
KBLOCK, VEC_GRID_MAX, SPMV_GRID_MAX = 256, 1024, 2048


# ------------------------------------------------------------------ csrc/steps.h
def step_beta(rho, rho_prev, alpha, omega): return (rho / rho_prev) * (alpha / omega)       # :84
def step_alpha(rho, rw_v): return rho / rw_v                                                # :107
def step_omega(t_s, t_t): return t_s / t_t                                                  # :137
def step_r0(b, ax): return b - ax                                                           # :67-70
def step_p(r, p, v, beta, omega): return fma(beta, fma(-omega, v, p), r)                    # :86-88
def step_r_half(r, v, alpha): return fma(-alpha, v, r)                                      # :109
def step_x_half(x, pw, alpha): return fma(alpha, pw, x)                                     # :110
def step_x_full(x, s, omega): return fma(omega, s, x)                                       # :139
def step_r_full(r, t, omega): return fma(-omega, t, r)                                      # :140
def dot_step(acc, a, b): return fma(a, b, acc)


# the neighbours the pinned arithmetic must be told apart from
def step_p_three_roundings(r, p, v, beta, omega):
    return float(r) + float(beta) * fma(-omega, v, p)


def dot_step_two_roundings(acc, a, b):
    return float(acc) + float(a) * float(b)


def each(f, *cols):
    return np.array([f(*row) for row in zip(*cols)])


# ------------------------------------------------------------------ reduction orders (csrc/device.h, kernels.h)
_XOR = [np.arange(KBLOCK) ^ o for o in (32, 16, 8, 4, 2, 1)]


def block_sum(v):
    """one value per thread of a 256-thread workgroup -> the sum every thread receives"""
    v = np.asarray(v, np.float64)
    for idx in _XOR:
        v = v + v[idx]                       # (lanes o apart never leave their wave of 64)
    return float(((v[0] + v[64]) + v[128]) + v[192])


def load_scalars(parts):
    """per-workgroup partials -> their sum as a consumer's prologue forms it (load_parts of batch.hip: the same order)"""
    out = np.zeros(KBLOCK)
    for j, pj in enumerate(parts):
        out[j % KBLOCK] += pj
    return block_sum(out)


def vec_grid(n):
    return min(max((n // 2 + KBLOCK - 1) // KBLOCK, 1), VEC_GRID_MAX)


def vec_threads(n, vec):
    """vec_loop<VEC>: [workgroup][thread] -> the elements the thread handles, in its order"""
    g, n2 = vec_grid(n), n // 2 if vec else 0
    stride, deal = g * KBLOCK, []
    for b in range(g):
        deal.append([])
        for t in range(KBLOCK):
            first = b * KBLOCK + t
            mine = [e for i in range(first, n2, stride) for e in (2 * i, 2 * i + 1)]
            mine += list(range(2 * n2 + first, n, stride))
            deal[-1].append(mine)
    return deal


def spmv_partition(L, n):
    rpb = KBLOCK // L
    g = max(min((n + rpb - 1) // rpb, SPMV_GRID_MAX), 1)
    per = max(((n + g - 1) // g + rpb - 1) // rpb * rpb, rpb)
    return max((n + per - 1) // per, 1), per


def spmv_threads(n, L):
    """k_spmv<L> / k_spmm_csr<L, K>: group q of L lanes takes rows row_begin + q, + 256 / L, ...; its first lane holds the terms"""
    grid, per = spmv_partition(L, n)
    assert grid % 8 != 0, "xcd_chunk would permute the chunks"
    deal = []
    for b in range(grid):
        deal.append([[] for _ in range(KBLOCK)])
        for q in range(KBLOCK // L):
            deal[-1][q * L] = list(range(b * per + q, min((b + 1) * per, n), KBLOCK // L))
    return deal


def dot_parts(deal, a, b, term):
    parts = []
    for block in deal:
        acc = np.zeros(KBLOCK)
        for t, mine in enumerate(block):
            for i in mine:
                acc[t] = term(acc[t], a[i], b[i])
        parts.append(block_sum(acc))
    return parts


# ------------------------------------------------------------------ stream tiles (spmv_csr.hip: plan_spmv_refine)
STREAM_NNZ, STREAM_MIN_ROWS, STREAM_MAX_MEAN, RESIDENT_GRID_MAX = 2048, 64, 12.0, 128


class Csr:
    """rows with sorted columns, base 0"""

    def __init__(self, rp, ci, val):
        self.rp, self.ci, self.val = np.asarray(rp, np.int64), np.asarray(ci, np.int64), np.asarray(val, np.float64)
        self.n = len(self.rp) - 1


def rowptr(A):
    return A.rp if isinstance(A, Csr) else np.arange(len(A) + 1)


def stream_plan(rp):
    """(R, workgroups) of the stream plan: R = 256, 128, 64 -- the tallest tile of which none holds more than kStreamNnz
    entries (k_tile_nnz_max looks at tiles that start at multiples of R); ceil(n / R) workgroups, one tile each below 2048"""
    n = len(rp) - 1
    assert n >= STREAM_MIN_ROWS and (rp[n] - rp[0]) / n <= STREAM_MAX_MEAN, "not a stream plan: lanes per row"
    for R in (256, 128, 64):
        if max(rp[min(r0 + R, n)] - rp[r0] for r0 in range(0, n, R)) <= STREAM_NNZ:
            tiles = (n + R - 1) // R
            grid = min(tiles, SPMV_GRID_MAX)
            per = (tiles + grid - 1) // grid
            assert per == 1, "more than one tile per workgroup (above 524 288 rows): not restated"
            return R, (tiles + per - 1) // per
    raise AssertionError("not a stream plan: nnz-balanced tiles")


def tile_threads(n, R, grid):
    """k_spmv_stream* (stream_finish_rows), k_fspmv_stream, k_resident_loop: workgroup g holds rows g R .. g R + R - 1, thread
    tid the one term of row g R + tid"""
    assert grid % 8 != 0 and grid * R >= n, "xcd_tile would permute the tiles"
    return [[[g * R + t] if t < R and g * R + t < n else [] for t in range(KBLOCK)] for g in range(grid)]


# ------------------------------------------------------------------ loop forms: the thread dealing behind every group of dots
# (the initial r.r is always k_init's: vec_threads)                     rw.v, (t.s, t.t)   ||s||^2    (rw.r, r.r)
FORMS = {
    "five/lanes":    dict(loop_form=0, spmv="lanes", half="vec", full="vec"),      # iterate_reference on k_spmv<64>
    "five/stream":   dict(loop_form=0, spmv="tile", half="vec", full="vec"),       # iterate_reference on k_spmv_stream*<R>
    "fused/lanes":   dict(loop_form=1, spmv="lanes", half="lanes", full="vec"),    # k_fspmv_lanes<64, .> + k_full
    "fused/stream":  dict(loop_form=1, spmv="tile", half="tile", full="vec"),      # k_fspmv_stream<R, .> + k_full
    "single":        dict(loop_form=2, spmv="tile", half="tile", full="tile"),     # k_resident_loop<R>
}


def dealings(A, form, vec):
    n, rp = len(rowptr(A)) - 1, rowptr(A)
    deal = {"vec": None, "lanes": None, "tile": None}
    f = FORMS[form]
    if "lanes" in f.values():
        deal["lanes"] = spmv_threads(n, LANES)
    if "tile" in f.values():
        R, grid = stream_plan(rp)
        assert f["loop_form"] != 2 or grid <= RESIDENT_GRID_MAX
        deal["tile"] = tile_threads(n, R, grid)
    d_init, d_half, d_full = (vec_threads(n, v) for v in vec)
    return d_init, deal[f["spmv"]], deal[f["half"]] or d_half, deal[f["full"]] or d_full


# ------------------------------------------------------------------ products
def row_sum_products(val, xs):
    """a stream tile: separately rounded products added in column order (stream_finish_rows, the oracle's loop)"""
    s = 0.0
    for q in val * xs:
        s = s + q
    return s


def row_sum_fma_chain(val, xs):             # a neighbour
    s = 0.0
    for aij, xj in zip(val, xs):
        s = fma(aij, xj, s)
    return s


def shift_fused(d, x, s): return fma(d, x, s)                 # spmv_finish_row_fused, fused_finish_row_x, k_resident_loop
def shift_two_roundings(d, x, s): return float(s) + float(d) * float(x)       # a neighbour


def product(A, x, d, row_sum, shift):
    """(A + diag d) x.  A diagonal A (a vector): a row sum is the single rounding fl(a_i x_i) in every SpMV form."""
    if isinstance(A, Csr):
        y = np.array([row_sum(A.val[s:e], x[A.ci[s:e]]) for s, e in zip(A.rp[:-1], A.rp[1:])])
    else:
        y = A * x
    return y if d is None else each(shift, d, x, y)


# ILU(0) of a diagonal matrix: L = I, U = diag(a); one application is two tri_rows passes over empty rows: rhs - 0, then
# (. - 0) * dinv with dinv = fl(1 / a_i) (fill_factor)
def minv_dinv(a, v): return ((v - 0.0) - 0.0) * (1.0 / a)
def minv_divide(a, v): return ((v - 0.0) - 0.0) / a           # a neighbour


Run = collections.namedtuple("Run", "iters half_exit x history")
OMEGA_MIN = 1e-5      # device.h:212


# ------------------------------------------------------------------ the loop
def loop(A, b, x0, vec=(1, 1, 1), p_update=step_p, term=dot_step, swap_x=False, form="five/lanes", kind="pbicgstab", d=None,
         iters=ITERS, tol=None, precond=False, row_sum=row_sum_products, shift=shift_fused, minv=minv_dinv, snapshots=None):
    """At most `iters` iterations of CUDAMAT_LOOP_PBICGSTAB (kind "pbicgstab") or CUDAMAT_LOOP_PBICGSTAB2 ("pbicgstab2") in
    the loop form FORMS[form].  A: a vector (the diagonal of a diagonal system) or a Csr; d: the shift of (A + I d), or None.
    vec: VEC of (k_init, k_half, k_full) -- k_init follows b's alignment, k_full x's, k_half sees the solver's own vectors
    only; (0, 0, 0): one row per thread, the K-column kernels.  tol = None: FLAG_NO_EXIT; else the stopping tests in the
    device's order against tolabs = tol * nrm0 (k_init_finish).  precond: ILU(0) of a diagonal A (form 0 only).
    snapshots: a list that receives x after every completed iteration.
    Returns Run(iters, half_exit, x, history): the history is [half 0, full 0, half 1, ...] for "pbicgstab", [full 0, full
    1, ...] for "pbicgstab2" (check_half stores nothing there, and nothing stops at a half step); after an exit at the half
    step x carries x += alpha p and nothing more."""
    assert kind in ("pbicgstab", "pbicgstab2")
    assert not precond or (FORMS[form]["loop_form"] == 0 and not isinstance(A, Csr) and d is None)
    two = kind == "pbicgstab2"
    n = len(b)
    d_init, d_spmv, d_half, d_full = dealings(A, form, vec)
    def mv(z): return product(A, z, d, row_sum, shift)
    x = np.array(x0, np.float64)
    r = each(step_r0, b, mv(x))                                  # r = b - (A + d) x0
    rw, p, v = r.copy(), r.copy(), np.zeros(n)
    full = [dot_parts(d_init, r, r, term)] * 2                   # (rw.r, r.r) = (r.r, r.r)
    tolabs = None if tol is None else tol * math.sqrt(load_scalars(full[1]))      # k_init_finish
    rho_s, alpha, omega, hist, it = [1.0, 1.0], 1.0, 1.0, [], 0
    while True:
        rho, rr = load_scalars(full[0]), load_scalars(full[1])   # k_update_p / FUSE_P / phase 1; after the last iteration k_check
        if it:                                                   # check_full: the full-step test of iteration it - 1
            hist.append(math.sqrt(rr))
            if tolabs is not None and hist[-1] < tolabs:
                return Run(it, False, x, np.array(hist))
            assert tolabs is None or not two or abs(omega) >= OMEGA_MIN, "breakdown: not restated"
        if it == iters:
            return Run(it, False, x, np.array(hist))
        rho_prev, rho_s[it & 1] = rho_s[(it + 1) & 1], rho
        if it:
            beta = step_beta(rho, rho_prev, alpha, omega)
            p = each(lambda ri, pi, vi: p_update(ri, pi, vi, beta, omega), r, p, v)
        pw = minv(A, p) if precond else p
        v = mv(pw)                                               # SpMV with (rw.v)
        alpha = step_alpha(rho, load_scalars(dot_parts(d_spmv, v, rw, term)))       # k_half / FUSE_HALF / phase 2
        r = each(lambda ri, vi: step_r_half(ri, vi, alpha), r, v)
        nrm_half = math.sqrt(load_scalars(dot_parts(d_half, r, r, term)))           # the half-step test's norm (check_half)
        if not two:
            hist.append(nrm_half)
            if tolabs is not None and nrm_half < tolabs:
                return Run(it, True, each(lambda xi, pi: step_x_half(xi, pi, alpha), x, pw), np.array(hist))
        s = minv(A, r) if precond else r
        t = mv(s)                                                # SpMV with (t.r, t.t); without M, s = r
        omega = step_omega(load_scalars(dot_parts(d_spmv, t, r, term)), load_scalars(dot_parts(d_spmv, t, t, term)))   # k_full / phase 3
        if swap_x:
            x = each(lambda xi, pi, si: step_x_half(step_x_full(xi, si, omega), pi, alpha), x, pw, s)
        else:
            x = each(lambda xi, pi, si: step_x_full(step_x_half(xi, pi, alpha), si, omega), x, pw, s)
        r = each(lambda ri, ti: step_r_full(ri, ti, omega), r, t)
        full = [dot_parts(d_full, rw, r, term), dot_parts(d_full, r, r, term)]
        it += 1
        if snapshots is not None:
            snapshots.append(x.copy())


SEEDS = (10, 16, 33, 7, 8, 18, 21, 32, 85)      # of columns 0 .. 7 (see above); column 8: the single-launch loop's (INPUTS)


def system(col):
    """(a, b, x0) of column `col`: the diagonal is shared, b and x0 are the column's own"""
    a = 1.0 + np.random.default_rng(601).random(N)
    return a, np.random.default_rng(1000 + SEEDS[col]).standard_normal(N), np.random.default_rng(2000 + SEEDS[col]).standard_normal(N)


BAND_N, BAND_OFFSETS, BAND_SEED = 777, (-257, -1, 0, 1, 257), 777


@functools.lru_cache(maxsize=None)
def banded():
    """777 rows (three stream tiles of 256 rows and one of 9), columns i - 257, i - 1, i, i + 1, i + 257 where they exist:
    off-diagonals uniform in (-1, 0), the diagonal 1 + U(0, 1) + the sum of their magnitudes.  The +-257 columns lie in
    another workgroup's tile, so every workgroup gathers p' and s at rows another one stored."""
    rng = np.random.default_rng(BAND_SEED)
    off, dia = -rng.random((BAND_N, len(BAND_OFFSETS))), 1.0 + rng.random(BAND_N)
    rp, ci, val = [0], [], []
    for i in range(BAND_N):
        cols = [(i + o, k) for k, o in enumerate(BAND_OFFSETS) if 0 <= i + o < BAND_N]
        mag = sum(-off[i, k] for c, k in cols if c != i)
        ci += [c for c, k in cols]
        val += [dia[i] + mag if c == i else off[i, k] for c, k in cols]
        rp.append(len(ci))
    A = Csr(rp, ci, val)
    for arr in (A.rp, A.ci, A.val):
        arr.setflags(write=False)
    return A


def banded_system(seed):
    """(A, b, x0) on the banded matrix"""
    return banded(), np.random.default_rng(3000 + seed).standard_normal(BAND_N), np.random.default_rng(4000 + seed).standard_normal(BAND_N)


def shift_of(n):
    """the d of (A + I d): 0.5 + U(0, 1)"""
    return 0.5 + np.random.default_rng(5000 + n).random(n)


LAYOUTS = {"aligned": (1, 1, 1), "offset8": (0, 1, 0), "rows": (0, 0, 0)}
TELLING = (("aligned", 2), ("offset8", 0), ("rows", 0), ("rows", 1))    # (dealing, column) pairs that tell every neighbour apart


@functools.lru_cache(maxsize=None)
def pinned(layout, col):
    """x and the history after ITERS iterations; shared between tests, not to be written"""
    _, _, x, h = loop(*system(col), vec=LAYOUTS[layout])
    x.setflags(write=False)
    h.setflags(write=False)
    return x, h


def differing(a, b):
    return int(np.count_nonzero(a != b))


# ------------------------------------------------------------------ the inputs of the pinning tests of the other loop forms
# Picked as SEEDS was (module docstring), by running the mirror and its neighbours over seeds -- never from GPU output.  Diagonal:
# columns 4 and 6 tell every neighbour apart in both three-launch forms (4 is taken); in the single-launch form k_init's are the
# only accumulators with more than one term, no column 0 .. 7 has forms 1 and 2 differ AND every neighbour show, and of seeds
# 0 .. 159 only 85 does (column 8).  Banded right-hand sides: of seeds 0 .. 191 only 86 tells all neighbours apart in all three
# stream forms, has forms 1 and 2 differ, and has a history entry in the first three iterations on which forms 0 and 1 differ;
# with the shift, seeds 11 and 24 of 0 .. 31 tell all neighbours apart in all three forms (24 is taken).
MAX_ITERS = 4                     # the GPU tests run 3 and 4 iterations: an odd and an even number of buffer swaps
TOL_HALF, TOL_FULL = 3.6e-3, 1.7e-3     # banded, unshifted: an exit at the half step of iteration 3, at the full step of iteration 3
EXIT_MARGIN = 0.01


def inputs(which, form, shifted=False, col=None):
    """(A, b, x0, d) of the pinning tests: which = "diagonal" or "banded"; col: another form's diagonal column"""
    if which == "diagonal":
        a, b, x0 = system(col if col is not None else 8 if form == "single" else 4)
        return a, b, x0, shift_of(N) if shifted else None
    A, b, x0 = banded_system(24 if shifted else 86)
    return A, b, x0, shift_of(BAND_N) if shifted else None


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def mirror_run(which, form, kind="pbicgstab", shifted=False, col=None, **neighbour):
    """MAX_ITERS iterations without a stopping test on inputs(which, form, shifted, col): (x after 1, 2, ... iterations,
    history).  Shared between tests, not to be written."""
    A, b, x0, d = inputs(which, form, shifted, col)
    snaps = []
    run = loop(A, b, x0, form=form, kind=kind, d=d, iters=MAX_ITERS, snapshots=snaps, **neighbour)
    assert run.iters == MAX_ITERS and all(np.all(np.isfinite(x)) for x in snaps) and np.all(np.isfinite(run.history))
    return frozen(*snaps), frozen(run.history)[0]


def pinned_form(which, form, kind="pbicgstab", shifted=False, iters=ITERS, **neighbour):
    """x and the history after `iters` <= MAX_ITERS iterations with FLAG_NO_EXIT.  (Without a stopping test the first
    iterations of a longer run ARE the shorter run, and its last full-step norm comes from the same partial sums in the same
    order whether the next iteration's prologue or k_check forms it: test_a_shorter_run_is_a_prefix.)"""
    xs, h = mirror_run(which, form, kind, shifted, **neighbour)
    return xs[iters - 1], h[:(2 if kind == "pbicgstab" else 1) * iters]


@functools.lru_cache(maxsize=None)
def pinned_ilu0(**neighbour):
    """ITERS iterations of the ILU(0) loop on the diagonal system (M = A up to the rounding of 1 / a_i, so the residual
    collapses in the first iteration and a fourth one would divide by a sum that has underflowed to 0)"""
    a, b, x0, _ = inputs("diagonal", "five/lanes")
    run = loop(a, b, x0, precond=True, **neighbour)
    assert run.iters == ITERS and np.all(np.isfinite(run.x)) and np.all(np.isfinite(run.history))
    return frozen(run.x, run.history)


@functools.lru_cache(maxsize=None)
def pinned_exit(form, tol, maxit=20):
    """the banded system solved to `tol`: Run(iters, half_exit, x, history)"""
    A, b, x0, _ = inputs("banded", form)
    run = loop(A, b, x0, form=form, iters=maxit, tol=tol)
    frozen(run.x, run.history)
    return run


NEIGHBOURS = (("three-rounding p-update", "p_update", step_p_three_roundings), ("two-rounding dot terms", "term", dot_step_two_roundings),
              ("x steps swapped", "swap_x", True))
NEW_FORMS = (("diagonal", "fused/lanes"), ("diagonal", "fused/stream"), ("diagonal", "single"),
             ("banded", "five/stream"), ("banded", "fused/stream"), ("banded", "single"))


def least_differing(which, form, kind="pbicgstab", shifted=False, **neighbour):
    """entries of x in which the neighbour differs from the pinned arithmetic, the smaller of the counts after 3 and 4 iterations"""
    xs, _ = mirror_run(which, form, kind, shifted)
    xa, _ = mirror_run(which, form, kind, shifted, **neighbour)
    return min(differing(xa[k - 1], xs[k - 1]) for k in (ITERS, MAX_ITERS))


def test_partitions_are_the_ones_described():
    assert vec_grid(N) == 2 and spmv_partition(LANES, N) == (151, 4)
    pairs, rows = vec_threads(N, 1), vec_threads(N, 0)
    assert pairs[0][0] == [0, 1, 600] and pairs[1][43] == [598, 599] and pairs[1][44] == []
    assert rows[0][0] == [0, 512] and rows[1][0] == [256] and rows[0][88] == [88, 600]
    for deal in (pairs, rows, spmv_threads(N, LANES)):
        assert sorted(i for block in deal for mine in block for i in mine) == list(range(N))
    assert spmv_threads(N, LANES)[150][0] == [600] and spmv_threads(N, LANES)[7][128] == [30]
    # stream tiles: the diagonal system without SPMV_LANES (3 tiles of 256 rows), the banded one (3 full tiles and one of 9 rows)
    A = banded()
    assert A.n == BAND_N and A.rp[-1] == 5 * BAND_N - 2 * (1 + 257) and np.all(A.val[A.ci != np.repeat(np.arange(A.n), np.diff(A.rp))] < 0.0)
    assert all(list(A.ci[s:e]) == sorted(A.ci[s:e]) for s, e in zip(A.rp[:-1], A.rp[1:]))
    assert list(A.ci[A.rp[300]:A.rp[301]]) == [43, 299, 300, 301, 557] and list(A.ci[:3]) == [0, 1, 257]
    assert stream_plan(rowptr(system(0)[0])) == (256, 3) and stream_plan(A.rp) == (256, 4)
    assert max(A.rp[min(r + 256, A.n)] - A.rp[r] for r in range(0, A.n, 256)) == 1279 <= STREAM_NNZ
    tiles = tile_threads(BAND_N, 256, 4)
    assert tiles[0][0] == [0] and tiles[2][255] == [767] and tiles[3][8] == [776] and tiles[3][9] == []
    assert tile_threads(N, 256, 3)[2][88] == [600] and tile_threads(N, 256, 3)[2][89] == []
    for deal in (tiles, tile_threads(N, 256, 3)):
        assert sorted(i for block in deal for mine in block for i in mine) == list(range(len(deal) * 256 - 256 + sum(map(bool, deal[-1]))))
    # the dealings each form draws its four groups of dots from: (r0.r0 | rw.v, t.s, t.t | ||s||^2 | rw.r, r.r)
    vecd, lanes = vec_threads(BAND_N, 1), spmv_threads(N, LANES)
    assert dealings(A, "five/stream", (1, 1, 1)) == (vecd, tiles, vecd, vecd)
    assert dealings(A, "fused/stream", (1, 1, 1)) == (vecd, tiles, tiles, vecd)
    assert dealings(A, "single", (1, 1, 1)) == (vecd, tiles, tiles, tiles)
    assert dealings(system(0)[0], "fused/lanes", (1, 1, 1)) == (pairs, lanes, lanes, pairs)
    assert dealings(system(0)[0], "five/lanes", (0, 1, 0)) == (rows, lanes, pairs, rows)


def test_the_loop_mirror_tells_its_neighbours_apart():
    """without a GPU: after three iterations the pinned arithmetic differs in >= 20 entries of x from each of: the p-update
    with the reference's three roundings, dots as fl(a b) then add, x += alpha p and x += omega s in the other order -- in
    the pair dealing (column 2, the aligned single solve) and in the row dealings (columns 0 and 1: the single solve with
    b and x off by 8 bytes, the K-column kernels).  The pair and the row dealing differ from one another as well."""
    for layout, col in TELLING:
        x, h = pinned(layout, col)
        assert len(h) == 2 * ITERS and np.all(np.isfinite(h)) and np.all(np.isfinite(x))
        for name, kw in (("three-rounding p-update", dict(p_update=step_p_three_roundings)),
                         ("two-rounding dot terms", dict(term=dot_step_two_roundings)), ("x steps swapped", dict(swap_x=True))):
            _, _, xa, ha = loop(*system(col), vec=LAYOUTS[layout], **kw)
            print(layout, col, name, "differs in", differing(xa, x), "entries of x and", differing(ha, h), "of", len(h), "residuals")
            assert differing(xa, x) >= MIN_DIFFERING_ROWS, (layout, col, name)
        # the iteration is a real one: the residual falls, and the mirror's x solves the system better than x0
        a, b, x0 = system(col)
        assert h[-1] < h[0] and np.linalg.norm(b - a * x) < np.linalg.norm(b - a * x0)
    for col in (0, 2):
        print("column", col, "pairs against rows:", differing(pinned("aligned", col)[0], pinned("rows", col)[0]), "entries of x")
    assert differing(pinned("aligned", 0)[0], pinned("rows", 0)[0]) >= MIN_DIFFERING_ROWS
    # (b and x off by 8 bytes: only k_half keeps pairs, and its dot feeds the history alone -- x is the row dealing's)
    np.testing.assert_array_equal(pinned("offset8", 0)[0], pinned("rows", 0)[0])


def test_form0_configuration_reproduces_the_recorded_values():
    """the generalised mirror in its five-launch, lanes-per-row, M = I configuration gives the values the three-iteration
    mirror gave before it learnt the other forms (tests/golden/loop_form0_pinned.npz: x and history of every layout and
    column 0 .. 7), bit for bit"""
    import os
    want = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "loop_form0_pinned.npz"))
    for layout in LAYOUTS:
        for col in range(8):
            x, h = pinned(layout, col)
            np.testing.assert_array_equal(x, want["%s_%d_x" % (layout, col)])
            np.testing.assert_array_equal(h, want["%s_%d_h" % (layout, col)])
    # and the two ways to ask for it agree
    np.testing.assert_array_equal(pinned_form("diagonal", "five/lanes")[0], pinned("aligned", 4)[0])
    np.testing.assert_array_equal(pinned_form("diagonal", "five/lanes")[1], pinned("aligned", 4)[1])


def test_a_shorter_run_is_a_prefix():
    """what pinned_form relies on: three iterations asked for as such equal the first three of four, history included"""
    for which, form, kind, shifted in (("banded", "single", "pbicgstab", False), ("diagonal", "fused/stream", "pbicgstab2", True)):
        A, b, x0, d = inputs(which, form, shifted)
        run = loop(A, b, x0, form=form, kind=kind, d=d, iters=ITERS)
        x, h = pinned_form(which, form, kind, shifted, ITERS)
        assert (run.iters, run.half_exit, len(h)) == (ITERS, False, 2 * ITERS if kind == "pbicgstab" else ITERS)
        np.testing.assert_array_equal(run.x, x)
        np.testing.assert_array_equal(run.history, h)


def test_the_loop_forms_differ_where_their_dealings_do():
    """without a GPU, on the inputs of the GPU tests: the stream plan against today's pinned form (lanes per row), the
    single-launch loop against the three-launch one, differ in >= 20 entries of x after 3 and after 4 iterations.  Forms 0 and
    1 on the SAME plan differ in the dealing of ||s||^2 alone, which feeds nothing but the history: x is equal by construction
    (asserted), and at least one history entry differs."""
    def count(xa, xb):
        return min(differing(xa[k - 1], xb[k - 1]) for k in (ITERS, MAX_ITERS))
    n01 = count(mirror_run("diagonal", "fused/stream")[0], mirror_run("diagonal", "five/lanes")[0])
    print("diagonal: form 1 (stream) against form 0 (lanes):", n01, "entries of x")
    assert n01 >= MIN_DIFFERING_ROWS
    for which in ("diagonal", "banded"):
        # (both on the single-launch test's inputs: on the diagonal system that is column 8)
        n12 = count(mirror_run(which, "single")[0], mirror_run(which, "fused/stream", col=8 if which == "diagonal" else None)[0])
        print(which, ": form 2 against form 1 (stream):", n12, "entries of x")
        assert n12 >= MIN_DIFFERING_ROWS
    for which, five, fused in (("diagonal", "five/lanes", "fused/lanes"), ("banded", "five/stream", "fused/stream")):
        (x0s, h0), (x1s, h1) = mirror_run(which, five), mirror_run(which, fused)
        for xa, xb in zip(x0s, x1s):
            np.testing.assert_array_equal(xa, xb)
        print(which, ": forms 0 and 1 on one plan: x equal,", differing(h0[:2 * ITERS], h1[:2 * ITERS]), "of", 2 * ITERS, "residuals differ")
        assert differing(h0[:2 * ITERS], h1[:2 * ITERS]) >= 1 and np.all(h0[1::2] == h1[1::2])


def test_the_new_forms_tell_the_neighbours_apart():
    """without a GPU, on the inputs of the GPU tests (test_loop_bits_* in test_gpu_parity.py): in every new form the pinned
    arithmetic differs in >= 20 entries of x, after 3 and after 4 iterations, from the three neighbours of
    test_the_loop_mirror_tells_its_neighbours_apart; on the banded system also from row sums formed as fma chains; in the
    shifted loop also from the shift applied as fl(s + fl(d x)); in the ILU(0) loop from M^-1 as a division by a_i."""
    for which, form in NEW_FORMS:
        for name, key, value in NEIGHBOURS:
            k = least_differing(which, form, **{key: value})
            print(which, form, name, "differs in", k, "entries of x")
            assert k >= MIN_DIFFERING_ROWS, (which, form, name)
        if which == "banded":
            k = least_differing(which, form, row_sum=row_sum_fma_chain)
            print(which, form, "row sums as fma chains differ in", k, "entries of x")
            assert k >= MIN_DIFFERING_ROWS, (which, form)
        if form != "fused/lanes":
            k = least_differing(which, form, "pbicgstab2", True, shift=shift_two_roundings)
            print(which, form, "shifted loop, the shift in two roundings differs in", k, "entries of x")
            assert k >= MIN_DIFFERING_ROWS, (which, form)
            # CUDAMAT_LOOP_PBICGSTAB2 without a shift: the arithmetic of CUDAMAT_LOOP_PBICGSTAB, the full-step norms alone as history
            (xa, ha), (xb, hb) = mirror_run(which, form, "pbicgstab2"), mirror_run(which, form)
            assert all(np.array_equal(p, q) for p, q in zip(xa, xb)) and np.array_equal(ha, hb[1::2])
    x, h = pinned_ilu0()
    xd, hd = pinned_ilu0(minv=minv_divide)
    print("ILU(0) loop: M^-1 as a division differs in", differing(xd, x), "entries of x and", differing(hd, h), "of", len(h), "residuals")
    assert differing(xd, x) >= MIN_DIFFERING_ROWS and len(h) == 2 * ITERS
    # (after the first iteration this loop moves x by less than an ulp: of the three neighbours only the two that act in
    # iteration 0 can show -- the p-update is first applied in iteration 1)
    for name, key, value in NEIGHBOURS[1:]:
        k = differing(pinned_ilu0(**{key: value})[0], x)
        print("ILU(0) loop:", name, "differs in", k, "entries of x")
        assert k >= MIN_DIFFERING_ROWS, name
    a, b, x0, _ = inputs("diagonal", "five/lanes")
    assert np.linalg.norm(b - a * x) < 1e-10 * np.linalg.norm(b - a * x0)


def test_the_exit_cases_end_where_intended():
    """the banded system solved to TOL_HALF leaves at the half step of iteration 3, to TOL_FULL at the full step of iteration 3
    (4 iterations), in every form; the deciding residual is >= 1 % below tolabs and every earlier one >= 1 % above, so a kernel
    wrong in the last bit fails on bits and not on a flipped decision.  After the half-step exit x is the x of three full
    iterations plus alpha p: neither the x before that iteration nor the x after it."""
    A, b, x0, _ = inputs("banded", "single")
    for form in ("five/stream", "fused/stream", "single"):
        xs, h = mirror_run("banded", form)
        nrm0 = math.sqrt(load_scalars(dot_parts(vec_threads(BAND_N, 1), *[each(step_r0, b, product(A, x0, None, row_sum_products, None))] * 2, dot_step)))
        for tol, want_iters, want_half in ((TOL_HALF, 3, True), (TOL_FULL, 4, False)):
            run = pinned_exit(form, tol)
            tolabs, hist = tol * nrm0, run.history
            print(form, "tol", tol, "-> iters", run.iters, "half step" if run.half_exit else "full step", "deciding residual / tolabs",
                  hist[-1] / tolabs, "smallest earlier one / tolabs", hist[:-1].min() / tolabs)
            assert (run.iters, run.half_exit, len(hist)) == (want_iters, want_half, 2 * want_iters + (1 if want_half else 0))
            assert hist[-1] <= (1.0 - EXIT_MARGIN) * tolabs and hist[:-1].min() >= (1.0 + EXIT_MARGIN) * tolabs
            np.testing.assert_array_equal(hist, h[:len(hist)])          # the same iterations as the run without exits
            if want_half:       # x += alpha p and nothing more: neither the x before this iteration nor the x after it
                assert differing(run.x, xs[2]) >= MIN_DIFFERING_ROWS and differing(run.x, xs[3]) >= MIN_DIFFERING_ROWS
            else:
                np.testing.assert_array_equal(run.x, xs[3])
