"""Three iterations of the reference BiCGSTAB loop (pbicgstab.cu:67-151, M = I) as the five-launch loop computes them,
restated on the CPU bit for bit: the steps of csrc/steps.h and the reduction orders of the kernels that call them.

  steps       step_p = fma(beta, fma(-omega, v, p), r) (two roundings), r -= alpha v, x += alpha p, x += omega s, r -= omega t
              (one fma each), every dot term fma(a, b, acc); beta = (rho / rho') (alpha / omega), alpha and omega one quotient
  a thread    vec_loop (device.h): VEC = 1 deals the n / 2 pairs grid-stride, .x before .y, then the odd tail; VEC = 0 and the
              K-column kernels of batch.hip deal single rows grid-stride
  a workgroup block_sum: xor butterfly 32 .. 1 inside a wave, then ((w0 + w1) + w2) + w3
  a launch    load_scalars / load_parts: thread j adds partials j, j + 256, ..., then block_sum; vec_grid workgroups for the
              vector kernels, spmv_partition for the SpMV's fused dots (k_spmv<L> and k_spmm_csr<L, K>: one group of L lanes
              per row, the group's first lane holds its rows' terms)

The system is diagonal (n = 601, entries in [1, 2)), so a row sum of any SpMV form is the single rounding fl(a_i x_i) and only
the dot partition of the forced form (SPMV_LANES = 64) has to be restated; n is odd (a tail), the vector grid is 2 workgroups and
the SpMV grid 151: neither is a multiple of 8, so xcd_chunk is the identity.  b and x0 are standard normal with fixed seeds.
The seeds are picked (SEEDS): at this n an accumulator of a vector kernel takes two or three terms and one of the SpMV a single
one, so for most right-hand sides a dot summed as fl(a b) + acc rounds to the very scalars the fma form gives and x cannot tell
the two apart (7 of the first 40 seeds can with pairs per thread, 3 with rows per thread); the p-update's third rounding
shows in 4 to 123 entries of x.  Columns 0 and 1 tell all three neighbours apart in the row dealings, column 2 in the pair dealing.
The GPU tests that pin the kernels to this mirror are test_loop_bits_* in test_gpu_parity.py and test_gpu_many_rhs.py; here,
without a GPU, the check that the mirror can tell the pinned arithmetic from its neighbours at all."""
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


# ------------------------------------------------------------------ the loop
def loop(a, b, x0, vec=(1, 1, 1), p_update=step_p, term=dot_step, swap_x=False):
    """ITERS iterations without a stopping test.  vec: VEC of (k_init, k_half, k_full) -- k_init follows b's alignment, k_full
    x's, k_half sees the solver's own vectors only; (0, 0, 0): one row per thread, the K-column kernels.
    Returns x and the residual history [half 0, full 0, half 1, ...]."""
    n = len(a)
    d_init, d_half, d_full = (vec_threads(n, v) for v in vec)
    d_spmv = spmv_threads(n, LANES)
    x = np.array(x0)
    r = each(step_r0, b, a * x)                                  # r = b - A x0; A x: one rounding per row
    rw, p, v = r.copy(), r.copy(), np.zeros(n)
    full = [dot_parts(d_init, r, r, term)] * 2                   # (rw.r, r.r) = (r.r, r.r)
    rho_s, alpha, omega, hist = [1.0, 1.0], 1.0, 1.0, []
    for it in range(ITERS):
        rho, rr = load_scalars(full[0]), load_scalars(full[1])   # k_update_p
        if it:
            hist.append(math.sqrt(rr))
        rho_prev, rho_s[it & 1] = rho_s[(it + 1) & 1], rho
        if it:
            beta = step_beta(rho, rho_prev, alpha, omega)
            p = each(lambda ri, pi, vi: p_update(ri, pi, vi, beta, omega), r, p, v)
        v = a * p                                                # SpMV with (rw.v)
        alpha = step_alpha(rho, load_scalars(dot_parts(d_spmv, v, rw, term)))       # k_half
        r = each(lambda ri, vi: step_r_half(ri, vi, alpha), r, v)
        hist.append(math.sqrt(load_scalars(dot_parts(d_half, r, r, term))))         # the half-step test's norm
        t = a * r                                                # SpMV with (t.s, t.t), s = r
        omega = step_omega(load_scalars(dot_parts(d_spmv, t, r, term)), load_scalars(dot_parts(d_spmv, t, t, term)))   # k_full
        if swap_x:
            x = each(lambda xi, pi, si: step_x_half(step_x_full(xi, si, omega), pi, alpha), x, p, r)
        else:
            x = each(lambda xi, pi, si: step_x_full(step_x_half(xi, pi, alpha), si, omega), x, p, r)
        r = each(lambda ri, ti: step_r_full(ri, ti, omega), r, t)
        full = [dot_parts(d_full, rw, r, term), dot_parts(d_full, r, r, term)]
    hist.append(math.sqrt(load_scalars(full[1])))                # the last full-step test (k_check)
    return x, np.array(hist)


SEEDS = (10, 16, 33, 7, 8, 18, 21, 32)      # of columns 0 .. 7 (see above)


def system(col):
    """(a, b, x0) of column `col`: the diagonal is shared, b and x0 are the column's own"""
    a = 1.0 + np.random.default_rng(601).random(N)
    return a, np.random.default_rng(1000 + SEEDS[col]).standard_normal(N), np.random.default_rng(2000 + SEEDS[col]).standard_normal(N)


LAYOUTS = {"aligned": (1, 1, 1), "offset8": (0, 1, 0), "rows": (0, 0, 0)}
TELLING = (("aligned", 2), ("offset8", 0), ("rows", 0), ("rows", 1))    # (dealing, column) pairs that tell every neighbour apart


@functools.lru_cache(maxsize=None)
def pinned(layout, col):
    """x and the history after ITERS iterations; shared between tests, not to be written"""
    x, h = loop(*system(col), vec=LAYOUTS[layout])
    x.setflags(write=False)
    h.setflags(write=False)
    return x, h


def differing(a, b):
    return int(np.count_nonzero(a != b))


def test_partitions_are_the_ones_described():
    assert vec_grid(N) == 2 and spmv_partition(LANES, N) == (151, 4)
    pairs, rows = vec_threads(N, 1), vec_threads(N, 0)
    assert pairs[0][0] == [0, 1, 600] and pairs[1][43] == [598, 599] and pairs[1][44] == []
    assert rows[0][0] == [0, 512] and rows[1][0] == [256] and rows[0][88] == [88, 600]
    for deal in (pairs, rows, spmv_threads(N, LANES)):
        assert sorted(i for block in deal for mine in block for i in mine) == list(range(N))
    assert spmv_threads(N, LANES)[150][0] == [600] and spmv_threads(N, LANES)[7][128] == [30]


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
            xa, ha = loop(*system(col), vec=LAYOUTS[layout], **kw)
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
