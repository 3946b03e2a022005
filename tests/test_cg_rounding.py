"""CUDAMAT_LOOP_CG (csrc/cg.hip, loops.hip: Solve::setup, cg_prologue, iterate_cg, finish) restated on the CPU bit for bit: the
steps of csrc/steps.h and the reduction orders of the kernels that call them.  What test_loop_rounding.py already restates
(block_sum, load_scalars, the thread dealings, the stream plan, products, M^-1 on a diagonal matrix, fma) is imported from there.

  steps       beta = rho / rho', alpha = rho / gamma (one quotient each); p = fma(beta, p, z), also at it = 0 with beta = 0;
              x = fma(alpha, p, x); r = fma(-alpha, q, r); every dot term fma(a, b, acc)
  start       r0 = b - (A + d) x0 element by element (k_init); the start sums (r0.r0, r0.r0) are formed AGAIN by k_l2_start in
              the pair dealing (vec_threads(n, 1)) whatever the alignment of b; tolabs = tol * sqrt(that sum) (k_init_finish)
  vectors     k_cg_p, k_cg_step and k_cg_rz run on pair_loop, which deals pairs for both alignments: a solve with b and x
              8 bytes off a 16-byte boundary has the aligned solve's mirror, not a second one
  gamma       p.q comes from the SpMV's own partials (spmv_finish_row_fused: fma(q_i, p_i, acc), the epilogue operand w is the
              SpMV's x): the lanes dealing (SPMV_LANES = 64) on the diagonal system, the stream-tile dealing on the banded one
  rho, ||r||  M = I: k_cg_step, both slots hold r.r; with a preconditioner k_cg_rz: (r.z, r.r) in one pass, pair dealing
  rho ring    k_cg_p of iteration it reads rho[(it + 1) & 1] and writes rho[it & 1]
  exits       ||r|| of iteration it - 1 is tested in the prologue of iteration it (k_cg_p), after the last one by k_cg_check;
              one history entry per iteration, at slot it - 1
  M^-1        ILU(0) of the diagonal system: minv_dinv, as in test_loop_rounding.pinned_ilu0; z = M^-1 r0 before the loop
              (cg_prologue) and z = M^-1 r after every step

Two systems.  The diagonal one of test_loop_rounding.system (n = 601, lanes per row).  A SYMMETRIC banded one built here
(n = 777, columns i, i +- 1, i +- 257 as test_loop_rounding.banded(); entry (i, j) and entry (j, i) come from one draw, the
diagonal is 1 + U(0, 1) + the row's off-diagonal magnitudes): cudamat_solver_symmetry answers (0, 0.0), the stream plan is
(256, 4), every workgroup gathers p at rows whose p another workgroup of k_cg_p stored.

The seeds of b and x0 are picked as test_loop_rounding.SEEDS was: by running this mirror and its neighbours over seeds here,
on the CPU -- never from GPU output.  An accumulator of a vector kernel takes two or three terms and one of the SpMV a single
one, so for most right-hand sides dot terms as fl(a b) + acc round to the very scalars the fma form gives (and x cannot tell
the two apart).  Seeds on which EVERY neighbour of the case differs in >= MIN_DIFFERING_ROWS entries of x after 3 and after 4
iterations, each case taking the first:
  diagonal          3, 4, 7, 8, 15, 18, 21, 27, 29, 31, 36 of 0 .. 39      (DIAG_SEED = 3)
  banded            9, 14, 15, 16, 26, 29, 32, 35, 36 of 0 .. 39            (BAND_SEED_RHS = 9)
  banded, shifted   0, 4, 8, 25, 28, 29, 33, 38 of 0 .. 39                  (BAND_SEED_SHIFTED = 0)
  diagonal, ILU(0)  84, 105, 130, 140 of 0 .. 239                           (ILU_SEED = 84; what "differs" means there: below)

ILU(0) on the diagonal system: M is A up to the rounding of 1 / a_i, so every iteration multiplies ||r|| by ~1e-16 and rows whose
update is exact drop out as zeros.  Decided here, on the CPU (ilu0_finite_iterations, test_ilu0_iteration_count): the mirror
completes ILU_ITERS = 11 iterations with rho, beta, gamma, alpha finite and rho, gamma > 0 -- not 3: CG carries no omega whose
divisor underflows -- its last r.r underflows to 0 and a twelfth iteration would form 0 / 0.  The GPU test runs 10 and 11.  (The
other choice, the shifted system on the unshifted factors, is not open: a shift with the factors of A0 alone is refused,
test_gpu_shift_precond.py test_what_stays_refused.)  From its second iteration on this loop moves x by less than an ulp, so the
neighbours that first act in iteration 1 or later -- the p-update (beta = 0 at it = 0) and the ring slot (it >= 2) -- cannot
show in x by construction: for those two the history counts (>= 1 of its 11 entries); the x step, the r step, the dot terms and
M^-1 as a division show in >= MIN_DIFFERING_ROWS entries of x.

The GPU tests that pin the kernels to this mirror are in test_gpu_cg_bits.py; here, without a GPU: the partitions, the mirror
against its neighbours on the inputs those tests use, prefixes, the exit case, and the recorded values
(tests/golden/cg_pinned.npz, written by tests/golden/make_golden.py cg_pinned from this mirror)."""
import collections
import functools
import math
import os

import numpy as np

from test_loop_rounding import (BAND_N, BAND_OFFSETS, EXIT_MARGIN, LANES, MIN_DIFFERING_ROWS, N, Csr, differing,
                                dot_parts, dot_step, dot_step_two_roundings, each, fma, frozen, load_scalars, minv_dinv, minv_divide,
                                product, row_sum_fma_chain, row_sum_products, rowptr, shift_fused, shift_of, shift_two_roundings,
                                spmv_partition, spmv_threads, step_r0, stream_plan, system, tile_threads, vec_grid, vec_threads)

ITERS, MAX_ITERS = 3, 4           # the GPU tests run 3 and 4 iterations: both halves of the rho ring written an even and an odd time


# ------------------------------------------------------------------ csrc/steps.h
def step_cg_beta(rho, rho_prev): return rho / rho_prev
def step_cg_alpha(rho, gamma): return rho / gamma
def step_cg_p(z, p, beta): return fma(beta, p, z)
def step_cg_x(x, p, alpha): return fma(alpha, p, x)
def step_cg_r(r, q, alpha): return fma(-alpha, q, r)


# the neighbours the pinned arithmetic must be told apart from
def step_cg_p_two_roundings(z, p, beta): return float(z) + float(beta) * float(p)
def step_cg_x_two_roundings(x, p, alpha): return float(x) + float(alpha) * float(p)
def step_cg_r_two_roundings(r, q, alpha): return float(r) - float(alpha) * float(q)


# ------------------------------------------------------------------ the systems
SYM_SEED = 778


@functools.lru_cache(maxsize=None)
def sym_banded():
    """777 rows, columns i - 257, i - 1, i, i + 1, i + 257 where they exist, SYMMETRIC: the entry at (i, i + o) and the one at
    (i + o, i) are one draw, uniform in (-1, 0); the diagonal is 1 + U(0, 1) + the sum of the row's off-diagonal magnitudes
    (strictly dominant and positive: symmetric positive definite)"""
    rng = np.random.default_rng(SYM_SEED)
    ups = {o: -rng.random(BAND_N) for o in BAND_OFFSETS if o > 0}         # ups[o][i] = a(i, i + o) = a(i + o, i)
    dia = 1.0 + rng.random(BAND_N)
    rp, ci, val = [0], [], []
    for i in range(BAND_N):
        cols = [i + o for o in BAND_OFFSETS if 0 <= i + o < BAND_N]
        offd = {c: (ups[c - i][i] if c > i else ups[i - c][c]) for c in cols if c != i}
        ci += cols
        val += [dia[i] + sum(-v for v in offd.values()) if c == i else offd[c] for c in cols]
        rp.append(len(ci))
    A = Csr(rp, ci, val)
    frozen(A.rp, A.ci, A.val)
    return A


DIAG_SEED, BAND_SEED_RHS, BAND_SEED_SHIFTED, ILU_SEED = 3, 9, 0, 84
SEEDS_TRIED = 40


def diag_system(seed):
    """(a, b, x0): the diagonal of test_loop_rounding.system, b and x0 standard normal by seed"""
    return system(0)[0], np.random.default_rng(1000 + seed).standard_normal(N), np.random.default_rng(2000 + seed).standard_normal(N)


def band_system(seed):
    return sym_banded(), np.random.default_rng(3000 + seed).standard_normal(BAND_N), np.random.default_rng(4000 + seed).standard_normal(BAND_N)


def inputs(which, shifted=False, precond=False, seed=None):
    """(A, b, x0, d) of the pinning tests: which = "diagonal" (lanes per row; with ILU(0) when precond) or "banded" (stream tiles)"""
    if which == "diagonal":
        assert not shifted
        a, b, x0 = diag_system((ILU_SEED if precond else DIAG_SEED) if seed is None else seed)
        return a, b, x0, None
    A, b, x0 = band_system((BAND_SEED_SHIFTED if shifted else BAND_SEED_RHS) if seed is None else seed)
    return A, b, x0, shift_of(BAND_N) if shifted else None


# ------------------------------------------------------------------ the loop
Run = collections.namedtuple("Run", "iters converged x history nrm0 scalars")


def spmv_dealing(A):
    """the thread dealing behind gamma: k_spmv<64> on the diagonal system, one stream tile per workgroup on a Csr"""
    n = len(rowptr(A)) - 1
    if isinstance(A, Csr):
        R, grid = stream_plan(A.rp)
        return tile_threads(n, R, grid)
    return spmv_threads(n, LANES)


def loop(A, b, x0, d=None, iters=ITERS, tol=None, precond=False, p_update=step_cg_p, x_step=step_cg_x, r_step=step_cg_r,
         term=dot_step, ring_back=1, row_sum=row_sum_products, shift=shift_fused, minv=minv_dinv, snapshots=None, strict=True):
    """At most `iters` iterations of CUDAMAT_LOOP_CG.  A: a vector (the diagonal of a diagonal system, SPMV_LANES = 64) or a
    Csr (stream tiles); d: the shift of (A + I d), or None.  tol = None: FLAG_NO_EXIT; else the stopping test in the device's
    order against tolabs = tol * nrm0.  precond: ILU(0) of a diagonal A.  ring_back = 2 is a neighbour: beta divides by the rho
    of two iterations back (the slot of the ring that k_cg_p is about to overwrite) from iteration 2 on.  snapshots: a list that
    receives x after every completed iteration.  strict = False: stop in front of the first iteration whose rho, gamma, alpha or
    beta is not finite or whose rho or gamma is not positive, instead of failing.  Run.scalars: (rho, beta, gamma, alpha) of every
    completed iteration."""
    assert not precond or (not isinstance(A, Csr) and d is None)
    n = len(b)
    d_vec, d_spmv = vec_threads(n, 1), spmv_dealing(A)
    def mv(v): return product(A, v, d, row_sum, shift)
    def sums(z):                                                 # k_cg_step (z is r: both slots r.r) / k_cg_rz: (r.z, r.r)
        rr = dot_parts(d_vec, r, r, term)
        return [rr if z is r else dot_parts(d_vec, r, z, term), rr]
    x = np.array(x0, np.float64)
    r = each(step_r0, b, mv(x))                                  # k_init: r = b - (A + d) x0, p = r
    p = r.copy()
    full = sums(r)                                               # k_l2_start: the pair dealing whatever b's alignment
    nrm0 = math.sqrt(load_scalars(full[1]))                      # k_init_finish
    tolabs = None if tol is None else tol * nrm0
    z = r
    if precond:                                                  # cg_prologue
        z = minv(A, r)
        full = sums(z)
    ring, hist, scalars, it = [0.0, 0.0], [], [], 0              # CgState starts as zeros (hipMemsetAsync)
    while True:
        rho, rr = load_scalars(full[0]), load_scalars(full[1])   # k_cg_p; after the last iteration k_cg_check
        if it:                                                   # check_iteration_end: the test of iteration it - 1
            hist.append(math.sqrt(rr))
            if tolabs is not None and hist[-1] < tolabs:
                return Run(it, True, x, np.array(hist), nrm0, scalars)
        if it == iters:
            return Run(it, False, x, np.array(hist), nrm0, scalars)
        rho_prev = ring[(it + 1) & 1] if ring_back == 1 or it < 2 else ring[it & 1]
        ok = rho > 0.0 and math.isfinite(rho) and (it == 0 or rho_prev != 0.0)
        beta = 0.0 if it == 0 else step_cg_beta(rho, rho_prev) if ok else math.nan
        ok = ok and math.isfinite(beta)
        if ok:
            ring[it & 1] = rho
            p_new = each(lambda zi, pi: p_update(zi, pi, beta), z, p)
            q = mv(p_new)                                        # SpMV with p.q in its epilogue
            gamma = load_scalars(dot_parts(d_spmv, q, p_new, term))
            ok = gamma > 0.0 and math.isfinite(gamma)
            alpha = step_cg_alpha(rho, gamma) if ok else math.nan           # k_cg_step
            ok = ok and math.isfinite(alpha)
        if not ok:
            assert not strict, "breakdown in iteration %d: not restated" % it
            return Run(it, False, x, np.array(hist), nrm0, scalars)
        p = p_new
        x = each(lambda xi, pi: x_step(xi, pi, alpha), x, p)
        r = each(lambda ri, qi: r_step(ri, qi, alpha), r, q)
        z = minv(A, r) if precond else r
        full = sums(z)
        scalars.append((rho, beta, gamma, alpha))
        it += 1
        if snapshots is not None:
            snapshots.append(x.copy())


def mirror_run(which, shifted=False, precond=False, seed=None, iters=MAX_ITERS, **neighbour):
    return _mirror_run(which, shifted, precond, seed, iters, tuple(sorted(neighbour.items(), key=lambda kv: kv[0])))


@functools.lru_cache(maxsize=None)
def _mirror_run(which, shifted, precond, seed, iters, neighbour):
    """`iters` iterations without a stopping test on inputs(which, shifted, precond, seed): (x after 1, 2, ... iterations,
    history).  Shared between tests, not to be written."""
    A, b, x0, d = inputs(which, shifted, precond, seed)
    snaps = []
    run = loop(A, b, x0, d=d, iters=iters, precond=precond, snapshots=snaps, **dict(neighbour))
    assert run.iters == iters and all(np.all(np.isfinite(x)) for x in snaps) and np.all(np.isfinite(run.history))
    return frozen(*snaps), frozen(run.history)[0]


def pinned(which, shifted=False, precond=False, iters=ITERS, **neighbour):
    """x and the history after `iters` iterations with FLAG_NO_EXIT (a shorter run is a prefix of a longer one: the last norm
    comes from the same partial sums in the same order whether k_cg_p or k_cg_check forms it -- test_a_shorter_run_is_a_prefix)"""
    xs, h = mirror_run(which, shifted, precond, iters=max(iters, ILU_ITERS if precond else MAX_ITERS), **neighbour)
    return xs[iters - 1], h[:iters]


@functools.lru_cache(maxsize=None)
def ilu0_finite_iterations(seed=None, cap=40):
    """iterations of the ILU(0) loop on the diagonal system that the mirror completes with rho, beta, gamma, alpha finite and
    rho, gamma > 0, and the history it leaves"""
    a, b, x0, _ = inputs("diagonal", precond=True, seed=seed)
    run = loop(a, b, x0, precond=True, iters=cap, strict=False)
    return run.iters, frozen(run.history)[0]


ILU_ITERS = 11            # (module docstring; asserted by test_ilu0_iteration_count)
IN_HISTORY_ONLY = ("p-update as z + fl(beta p)", "beta from the ring slot two back")        # with ILU(0): x cannot differ

TOL_EXIT = 7.5e-2          # banded, unshifted: leaves at iteration 3 (test_the_exit_case_ends_where_intended)


@functools.lru_cache(maxsize=None)
def pinned_exit(tol=TOL_EXIT, maxit=20):
    A, b, x0, _ = inputs("banded")
    run = loop(A, b, x0, iters=maxit, tol=tol)
    frozen(run.x, run.history)
    return run


NEIGHBOURS = (("p-update as z + fl(beta p)", dict(p_update=step_cg_p_two_roundings)),
              ("x step in two roundings", dict(x_step=step_cg_x_two_roundings)),
              ("r step in two roundings", dict(r_step=step_cg_r_two_roundings)),
              ("dot terms in two roundings", dict(term=dot_step_two_roundings)),
              ("beta from the ring slot two back", dict(ring_back=2)))
CASES = (("diagonal", False, False), ("banded", False, False), ("banded", True, False), ("diagonal", False, True))


def neighbours_of(which, shifted, precond):
    out = list(NEIGHBOURS)
    if which == "banded":
        out.append(("row sums as an fma chain", dict(row_sum=row_sum_fma_chain)))
    if shifted:
        out.append(("the shift in two roundings", dict(shift=shift_two_roundings)))
    if precond:
        out.append(("M^-1 as a division", dict(minv=minv_divide)))
    return out


def least_differing(which, shifted=False, precond=False, seed=None, **neighbour):
    """entries of x in which the neighbour differs from the pinned arithmetic: the smaller of the counts after the two iteration
    counts the GPU tests run, and the number of history entries that differ"""
    top = ILU_ITERS if precond else MAX_ITERS
    xs, h = mirror_run(which, shifted, precond, seed, iters=top)
    xa, ha = mirror_run(which, shifted, precond, seed, iters=top, **neighbour)
    return min(differing(xa[k - 1], xs[k - 1]) for k in (top - 1, top)), differing(ha, h)


# ------------------------------------------------------------------ tests
def test_partitions_are_the_ones_described():
    A = sym_banded()
    assert A.n == BAND_N and A.rp[-1] == 5 * BAND_N - 2 * (1 + 257)
    rows = np.repeat(np.arange(A.n), np.diff(A.rp))
    assert all(list(A.ci[s:e]) == sorted(A.ci[s:e]) for s, e in zip(A.rp[:-1], A.rp[1:]))
    assert list(A.ci[A.rp[300]:A.rp[301]]) == [43, 299, 300, 301, 557] and list(A.ci[:3]) == [0, 1, 257]
    # symmetric bit for bit, off-diagonals in (-1, 0), the diagonal strictly dominant
    dense = np.zeros((A.n, A.n))
    dense[rows, A.ci] = A.val
    assert np.array_equal(dense, dense.T) and np.all(A.val[A.ci != rows] < 0.0) and np.all(A.val[A.ci != rows] > -1.0)
    assert np.all(np.diag(dense) >= 1.0 + (np.abs(dense).sum(axis=1) - np.diag(dense)) - 1e-12)
    assert np.linalg.eigvalsh(dense).min() > 0.9
    # gamma: 4 stream tiles of 256 rows (the last of 9) on the banded system, 151 workgroups of 4 one-row groups on the diagonal one
    assert stream_plan(A.rp) == (256, 4) and spmv_partition(LANES, N) == (151, 4)
    assert spmv_dealing(A) == tile_threads(BAND_N, 256, 4) and spmv_dealing(system(0)[0]) == spmv_threads(N, LANES)
    assert spmv_dealing(A)[3][8] == [776] and spmv_dealing(A)[3][9] == [] and spmv_dealing(system(0)[0])[150][0] == [600]
    # every vector kernel: pairs, two workgroups (an odd tail at n = 601, at n = 777 too)
    assert vec_grid(N) == 2 and vec_grid(BAND_N) == 2
    assert vec_threads(N, 1)[0][0] == [0, 1, 600] and vec_threads(BAND_N, 1)[0][0] == [0, 1, 776]
    assert vec_threads(BAND_N, 1)[1][131] == [774, 775] and vec_threads(BAND_N, 1)[1][132] == []
    for deal, n in ((vec_threads(BAND_N, 1), BAND_N), (spmv_dealing(A), BAND_N), (spmv_dealing(system(0)[0]), N)):
        assert sorted(i for block in deal for mine in block for i in mine) == list(range(n))
    # a thread of the SpMV holds one term, one of a vector kernel two or three
    assert max(len(mine) for block in spmv_dealing(A) for mine in block) == 1
    assert max(len(mine) for block in spmv_dealing(system(0)[0]) for mine in block) == 1
    assert sorted({len(mine) for block in vec_threads(N, 1) for mine in block}) == [0, 2, 3]


def test_the_cg_mirror_tells_its_neighbours_apart():
    """without a GPU, on the inputs of test_gpu_cg_bits.py: after 3 and after 4 iterations (ILU(0): after ILU_ITERS - 1 and
    ILU_ITERS) the pinned arithmetic differs in >= MIN_DIFFERING_ROWS entries of x from every neighbour of its case; with
    ILU(0) the two neighbours that cannot reach x (IN_HISTORY_ONLY, module docstring) differ in the history"""
    for which, shifted, precond in CASES:
        for name, kw in neighbours_of(which, shifted, precond):
            k, kh = least_differing(which, shifted, precond, **kw)
            print(which, "shifted" if shifted else "", "ILU(0)" if precond else "", name, "differs in", k, "entries of x and", kh,
                  "residuals")
            if precond and name in IN_HISTORY_ONLY:
                assert k == 0 and kh >= 1, (which, shifted, precond, name)
            else:
                assert k >= MIN_DIFFERING_ROWS, (which, shifted, precond, name)
        # the iteration is a real one: the residual falls and the mirror's x solves the system better than x0
        A, b, x0, d = inputs(which, shifted, precond)
        x, h = pinned(which, shifted, precond, iters=ILU_ITERS if precond else MAX_ITERS)
        res = lambda v: np.linalg.norm(b - product(A, v, d, row_sum_products, shift_fused))
        assert h[-1] < h[0] and res(x) < res(x0)


def test_a_shorter_run_is_a_prefix():
    """what pinned() relies on: three iterations asked for as such equal the first three of four, history included"""
    for which, shifted, precond in CASES:
        A, b, x0, d = inputs(which, shifted, precond)
        short = (ILU_ITERS - 1) if precond else ITERS
        run = loop(A, b, x0, d=d, precond=precond, iters=short)
        x, h = pinned(which, shifted, precond, iters=short)
        assert (run.iters, run.converged, len(h)) == (short, False, short)
        np.testing.assert_array_equal(run.x, x)
        np.testing.assert_array_equal(run.history, h)


def test_the_exit_case_ends_where_intended():
    """the banded system solved to TOL_EXIT leaves at iteration 3: the deciding residual is >= 1 % below tolabs and every
    earlier one >= 1 % above, so a kernel wrong in the last bit fails on bits and not on a flipped decision"""
    run = pinned_exit()
    xs, h = mirror_run("banded")
    tolabs = TOL_EXIT * run.nrm0
    print("tol", TOL_EXIT, "-> iters", run.iters, "deciding residual / tolabs", run.history[-1] / tolabs,
          "smallest earlier one / tolabs", run.history[:-1].min() / tolabs)
    assert (run.iters, run.converged, len(run.history)) == (3, True, 3)
    assert run.history[-1] <= (1.0 - EXIT_MARGIN) * tolabs and run.history[:-1].min() >= (1.0 + EXIT_MARGIN) * tolabs
    np.testing.assert_array_equal(run.history, h[:3])
    np.testing.assert_array_equal(run.x, xs[2])


def test_ilu0_iteration_count():
    """how long the ILU(0) loop on the diagonal system keeps every scalar finite and rho, gamma positive: ILU_ITERS
    iterations, which is what the GPU test runs; the last sum of squares has underflowed to 0"""
    count, h = ilu0_finite_iterations()
    print("ILU(0) on the diagonal system: the mirror completes", count, "iterations; history", h)
    assert count == ILU_ITERS and h[-1] == 0.0 and np.all(h[:-1] > 0.0)
    a, b, x0, _ = inputs("diagonal", precond=True)
    x, hh = pinned("diagonal", precond=True, iters=ILU_ITERS)
    np.testing.assert_array_equal(hh, h[:ILU_ITERS])
    assert np.linalg.norm(b - a * x) < 1e-10 * np.linalg.norm(b - a * x0)


def test_the_mirror_reproduces_the_recorded_values():
    """tests/golden/cg_pinned.npz holds x and the history the mirror gave for every pinned case when the file was written
    (tests/golden/make_golden.py cg_pinned; produced by this mirror, on the CPU): an edit of the mirror cannot move the target
    of the GPU tests silently"""
    want = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cg_pinned.npz"))
    got = recorded_values()
    assert sorted(want.files) == sorted(got)
    for key, value in got.items():
        np.testing.assert_array_equal(value, want[key], err_msg=key)


def recorded_values():
    out = {}
    for which, shifted, precond in CASES:
        tag = which + ("_shifted" if shifted else "") + ("_ilu0" if precond else "")
        for iters in ((ILU_ITERS - 1, ILU_ITERS) if precond else (ITERS, MAX_ITERS)):
            x, h = pinned(which, shifted, precond, iters=iters)
            out["%s_%d_x" % (tag, iters)], out["%s_%d_h" % (tag, iters)] = np.array(x), np.array(h)
    run = pinned_exit()
    out["exit_x"], out["exit_h"] = np.array(run.x), np.array(run.history)
    return out
