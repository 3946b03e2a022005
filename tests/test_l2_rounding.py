"""CUDAMAT_LOOP_BICGSTAB_L2 (csrc/bicgstab_l2.hip, loops.hip: Solve::setup, l2_prologue, l2_ahat, iterate_l2, finish) restated
on the CPU bit for bit: the steps of csrc/steps.h and the reduction orders of the kernels that call them.  What
test_loop_rounding.py already restates (block_sum, load_scalars, the thread dealings, the stream plan, products, M^-1 on a diagonal
matrix, fma) is imported from there.

  steps       beta = (alpha rho1) / rho0 (two roundings), alpha = rho0 / gamma; u = fma(-beta, u, r); r = fma(-alpha, u', r);
              y = fma(alpha, u0, y); y = fma(g2, r1, fma(g1, r0, y)); v = fma(-g2, b, fma(-g1, a, v)) for u0 and r0; every dot
              term fma(a, b, acc)
  (g1, g2)    by elimination on the pivot a11 = r1.r1 (step_l2_mr): s = a12 / a11, t = fma(-s, a12, a22),
              g2 = fma(-s, b1, b2) / t, g1 = fma(-a12, g2, b1) / a11
  start       r0 = b - (A + d) x0 element by element (k_init), which leaves u0 = p = r0 and r~ = r0; the start sums
              (r0.r~, r0.r0) = (r0.r0, r0.r0) are formed AGAIN by k_l2_start in the pair dealing whatever the alignment of b;
              tolabs = tol * sqrt(that sum) (k_init_finish).  The first sweep has rho' = 1, alpha = 0, omega = 1:
              beta = (0 rho1) / (-1) = -0.0 and u0 = fma(0, u0, r0) = r0
  dealings    vec_threads(n, 1) (pair_loop, for both alignments) for (r1.r1, r1.r0) of k_l2_step1, r2.r0 of k_l2_dot and
              (r0.r~, r0.r0) of k_l2_mr; the SpMV's own for the three r~ dots (u1.r~, r1.r~, u2.r~) and for (r2.r1, r2.r2)
              (spmv_finish_row_fused: fma(out, w, acc), fma(out, out, acc)): the lanes dealing (SPMV_LANES = 64) on the diagonal
              system, the stream-tile dealing on the banded one
  exits       ||r0|| of sweep it - 1 is tested in the prologue of sweep it (k_l2_u0), after the last one by k_l2_check; one
              history entry per completed sweep, at slot it - 1
  M^-1        ILU(0) of the diagonal system (minv_dinv): A^ = A M^-1, y starts at 0 and x = x0 + M^-1 y is formed in finish(),
              whatever ended the loop; launch_axpy is fma(1, M^-1 y, x): one rounding
  breakdown   the kernel that forms a scalar freezes the loop (state 3) before it touches a vector; what earlier kernels of that
              sweep stored stays (y and r0 of k_l2_step0 and k_l2_step1 among it); iters counts completed sweeps.  Under
              FLAG_NO_EXIT no test is taken (loop_breakdown, device.h) and the scalars are divided as they come

Three systems.  The diagonal one of test_loop_rounding.system (n = 601, lanes per row), the non-symmetric banded one of
test_loop_rounding.banded() (n = 777, stream plan (256, 4)), and the banded one with the shift shift_of(777); b and x0 standard
normal by seed as test_cg_rounding.diag_system and test_loop_rounding.banded_system draw them.

The seeds are picked by running this mirror and its neighbours over seeds here, on the CPU -- never from GPU output.  Seeds of
0 .. 39 on which EVERY neighbour of the case differs in >= MIN_DIFFERING_ROWS entries of x after 3 and after 4 sweeps, each case
taking the first (scan_seeds):
  diagonal          7, 8, 18, 21, 27, 31 of 0 .. 39                                            (DIAG_SEED = 7)
  banded            3, 4, 7, 8, 12, 15, 19, 20, 21, 23, 30, 31, 32, 35, 37, 38, 39 of 0 .. 39   (BAND_SEED_RHS = 3)
  banded, shifted   5, 7, 8, 12, 15, 17, 20, 22, 24, 25, 26, 27, 33, 35, 36, 39 of 0 .. 39      (BAND_SEED_SHIFTED = 5)
  diagonal, ILU(0)  72, 119, 137 of 0 .. 239                                  (ILU_SEED = 72; what qualifies there: below)
The scarce neighbours are beta as alpha (rho1 / rho0) and the dot terms as fl(a b) + acc, which round to the pinned scalars on
about half the seeds.

ILU(0) on the diagonal system: M is A up to the rounding of 1 / a_i, so A^ = I up to rounding, r1 = r0 up to rounding and the
2 x 2 system of the minimal-residual step is singular up to rounding.  Decided here, on the CPU (ilu0_run,
test_ilu0_sweeps_and_breakdown), with tol = 0 (every stopping and breakdown test taken, no residual passes): of seeds 0 .. 239,
126 break down after >= 1 complete sweep and 66 after >= 2 (two to ten sweeps, each multiplying ||r0|| by ~1e-15; in k_l2_u0,
k_l2_step1 or k_l2_mr).  On ILU_SEED = 72 the mirror completes ILU_SWEEPS = 2 sweeps and k_l2_mr of the third reports the breakdown:
the GPU test runs maxit = 2 (no breakdown) and maxit = 3 (breakdown = 1, iters = 2, the same history, x = x0 + M^-1 y with the y
k_l2_step0 and k_l2_step1 of the interrupted sweep left).  A seed qualifies when, in the breakdown run, every neighbour differs
from the pinned arithmetic in >= MIN_DIFFERING_ROWS entries of x -- but the omega of the sweep before, which first acts in the
third sweep's k_l2_u0, where x moves by less than an ulp: for that one (IN_HISTORY_ONLY) a history entry, iters or the
breakdown flag has to differ (ilu0_differing: what a GPU run can see).  With two more neighbours let off that way (beta as
alpha (rho1 / rho0), the dot terms) seeds 50, 73, 123 and 159 would qualify as well.

The GPU tests that pin the kernels to this mirror are in test_gpu_l2_bits.py; here, without a GPU: the partitions, the mirror
against its neighbours on the inputs those tests use, prefixes, the exit case, the range claims of DESIGN.md section 4 on the
mirror itself, and the recorded values (tests/golden/l2_pinned.npz, written by tests/golden/make_golden.py l2_pinned from this
mirror)."""
import collections
import functools
import math
import os

import numpy as np

from test_loop_rounding import (BAND_N, EXIT_MARGIN, LANES, MIN_DIFFERING_ROWS, N, Csr, banded, banded_system, differing,
                                dot_parts, dot_step, dot_step_two_roundings, each, fma, frozen, load_scalars, minv_dinv, minv_divide,
                                product, row_sum_fma_chain, row_sum_products, rowptr, shift_fused, shift_of, shift_two_roundings,
                                spmv_partition, spmv_threads, step_r0, stream_plan, system, tile_threads, vec_grid, vec_threads)

SWEEPS, MAX_SWEEPS = 3, 4         # the GPU tests run 3 and 4 sweeps: the neighbour with a stale omega cannot act before the third
EXPONENTS, MAT_EXPONENTS = (-440, -200, -40, 40, 200, 440), (-200, -40, 40, 200)        # test_gpu_scaling's (asserted equal there)


# ------------------------------------------------------------------ csrc/steps.h
def step_l2_u(r, u, beta): return fma(-beta, u, r)
def step_l2_r(r, u, alpha): return fma(-alpha, u, r)
def step_l2_y(y, u, alpha): return fma(alpha, u, y)
def step_l2_add2(y, a, b, g1, g2): return fma(g2, b, fma(g1, a, y))
def step_l2_sub2(v, a, b, g1, g2): return fma(-g2, b, fma(-g1, a, v))


def _div(a, b):
    """a / b as the device divides: inf or nan where Python raises"""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def step_l2_beta(alpha, rho1, rho0): return _div(alpha * rho1, rho0)
def step_l2_alpha(rho0, gamma): return _div(rho0, gamma)


def _fma_any(a, b, c):
    """fma, also of operands that are not finite (the exact-rational fma takes none): the result is then inf or nan as the
    device's, which is all k_l2_mr looks at before it freezes the loop"""
    if all(math.isfinite(v) for v in (a, b, c)):
        return fma(a, b, c)
    with np.errstate(all="ignore"):
        return float(np.float64(a) * np.float64(b) + np.float64(c))


def step_l2_mr(a11, a12, a22, b1, b2):
    """-> (False where k_l2_mr reports a breakdown: a11 or t zero, or s, t, g1 or g2 not finite; g1; g2)"""
    s = _div(a12, a11)
    t = _fma_any(-s, a12, a22)
    g2 = _div(_fma_any(-s, b1, b2), t)
    g1 = _div(_fma_any(-a12, g2, b1), a11)
    return (a11 != 0.0 and t != 0.0 and all(math.isfinite(v) for v in (s, t, g1, g2))), g1, g2


# the neighbours the pinned arithmetic must be told apart from
def step_l2_u_two_roundings(r, u, beta): return float(r) - float(beta) * float(u)
def step_l2_r_two_roundings(r, u, alpha): return float(r) - float(alpha) * float(u)
def step_l2_y_two_roundings(y, u, alpha): return float(y) + float(alpha) * float(u)
def step_l2_add2_g2_first(y, a, b, g1, g2): return fma(g1, a, fma(g2, b, y))
def step_l2_sub2_g2_first(v, a, b, g1, g2): return fma(-g1, a, fma(-g2, b, v))
def step_l2_add2_three_roundings(y, a, b, g1, g2): return float(y) + fma(g1, a, float(g2) * float(b))
def step_l2_beta_quotient_first(alpha, rho1, rho0): return alpha * _div(rho1, rho0)


def step_l2_mr_plain_products(a11, a12, a22, b1, b2):
    """the elimination with every product rounded on its own"""
    with np.errstate(all="ignore"):
        a11, a12, a22, b1, b2 = (np.float64(v) for v in (a11, a12, a22, b1, b2))
        s = a12 / a11
        t = a22 - s * a12
        g2 = (b2 - s * b1) / t
        g1 = (b1 - a12 * g2) / a11
    return (a11 != 0.0 and t != 0.0 and all(math.isfinite(v) for v in (s, t, g1, g2))), float(g1), float(g2)


def step_l2_mr_cramer(a11, a12, a22, b1, b2):
    """Cramer's rule, as the kernel had it before: det carries c^4 under (c b, c x0) and c^6 under (c A, b, x0 / c)"""
    with np.errstate(all="ignore"):
        a11, a12, a22, b1, b2 = (np.float64(v) for v in (a11, a12, a22, b1, b2))
        det = a11 * a22 - a12 * a12
        g1 = (b1 * a22 - b2 * a12) / det
        g2 = (a11 * b2 - a12 * b1) / det
    return (det != 0.0 and all(math.isfinite(v) for v in (det, g1, g2))), float(g1), float(g2)


# ------------------------------------------------------------------ the systems
DIAG_SEED, BAND_SEED_RHS, BAND_SEED_SHIFTED, ILU_SEED = 7, 3, 5, 72
SEEDS_DIAGONAL = (7, 8, 18, 21, 27, 31)                                                    # (module docstring)
SEEDS_BANDED = (3, 4, 7, 8, 12, 15, 19, 20, 21, 23, 30, 31, 32, 35, 37, 38, 39)
SEEDS_SHIFTED = (5, 7, 8, 12, 15, 17, 20, 22, 24, 25, 26, 27, 33, 35, 36, 39)
SEEDS_ILU = (72, 119, 137)
SEEDS_TRIED, ILU_SEEDS_TRIED = 40, 240


def diag_system(seed):
    """(a, b, x0): the diagonal of test_loop_rounding.system, b and x0 standard normal by seed (as test_cg_rounding.diag_system)"""
    return system(0)[0], np.random.default_rng(1000 + seed).standard_normal(N), np.random.default_rng(2000 + seed).standard_normal(N)


def inputs(which, shifted=False, precond=False, seed=None):
    """(A, b, x0, d) of the pinning tests: which = "diagonal" (lanes per row; with ILU(0) when precond) or "banded" (stream tiles)"""
    if which == "diagonal":
        assert not shifted
        a, b, x0 = diag_system((ILU_SEED if precond else DIAG_SEED) if seed is None else seed)
        return a, b, x0, None
    assert not precond
    A, b, x0 = banded_system((BAND_SEED_SHIFTED if shifted else BAND_SEED_RHS) if seed is None else seed)
    return A, b, x0, shift_of(BAND_N) if shifted else None


# ------------------------------------------------------------------ the loop
Run = collections.namedtuple("Run", "iters converged breakdown where x history nrm0 scalars")
ARITHMETIC = dict(u_step=step_l2_u, r_step=step_l2_r, y_step=step_l2_y, add2=step_l2_add2, sub2=step_l2_sub2, beta_of=step_l2_beta,
                  mr=step_l2_mr, term=dot_step, stale_omega=False, row_sum=row_sum_products, shift=shift_fused, minv=minv_dinv)


def spmv_dealing(A):
    """the thread dealing behind the SpMV's dots: k_spmv<64> on the diagonal system, one stream tile per workgroup on a Csr"""
    n = len(rowptr(A)) - 1
    if isinstance(A, Csr):
        R, grid = stream_plan(A.rp)
        return tile_threads(n, R, grid)
    return spmv_threads(n, LANES)


def _finite(*vals):
    return all(math.isfinite(v) for v in vals)


def loop(A, b, x0, d=None, iters=SWEEPS, tol=None, precond=False, snapshots=None, **arithmetic):
    """At most `iters` sweeps of CUDAMAT_LOOP_BICGSTAB_L2.  A: a vector (the diagonal of a diagonal system, SPMV_LANES = 64) or a
    Csr (stream tiles); d: the shift of (A + I d), or None.  tol = None: FLAG_NO_EXIT -- no stopping test and no breakdown test is
    taken; else both, in the device's order, against tolabs = tol * nrm0 (tol = 0: every test taken, no residual passes).
    precond: ILU(0) of a diagonal A.  arithmetic: the neighbours, by the keys of ARITHMETIC; stale_omega = True takes the omega of
    sweep it - 2 in the rho0 of sweep it >= 2.  snapshots: a list that receives x (M = I) or y after every completed sweep.
    Run.where: the kernel that froze the loop at a breakdown.  Run.scalars: (beta0, alpha0, beta1, alpha1, g1, g2) of every
    completed sweep."""
    k = dict(ARITHMETIC, **arithmetic)
    assert sorted(k) == sorted(ARITHMETIC) and (not precond or (not isinstance(A, Csr) and d is None))
    u_step, r_step, y_step, add2, sub2, term, minv = (k[key] for key in ("u_step", "r_step", "y_step", "add2", "sub2", "term", "minv"))
    n, exits = len(b), tol is not None
    d_vec, d_spmv = vec_threads(n, 1), spmv_dealing(A)
    def mv(v): return product(A, v, d, k["row_sum"], k["shift"])
    def ahat(v): return mv(minv(A, v) if precond else v)                       # l2_ahat
    def dot(deal, p, q): return load_scalars(dot_parts(deal, p, q, term))
    x = np.array(x0, np.float64)
    r0 = each(step_r0, b, mv(x))                                               # k_init: r = b - (A + d) x0, p = r, r~ = r
    rt, u0 = r0.copy(), r0.copy()
    u1 = r1 = u2 = r2 = None
    y = np.zeros(n) if precond else x                                          # l2_prologue
    rr = dot(d_vec, r0, r0)                                                    # k_l2_start: the pair dealing whatever b's alignment
    rho1, nrm0 = rr, math.sqrt(rr)                                             # k_init_finish
    tolabs = tol * nrm0 if exits else None
    hist, scalars, omegas, it = [], [], [], 0
    rho_b = alpha_b = None

    def end(converged, where):
        with np.errstate(all="ignore"):
            xe = each(lambda xi, zi: fma(1.0, zi, xi), x, minv(A, y)) if precond else y        # finish: launch_axpy(1.0, M^-1 y, x)
        return Run(it, converged, where is not None, where, xe, np.array(hist), nrm0, scalars)

    with np.errstate(all="ignore"):
        while True:
            if it:                                                             # check_iteration_end: k_l2_u0, or k_l2_check after the last sweep
                hist.append(math.sqrt(rr))
                if exits and hist[-1] < tolabs:
                    return end(True, None)
                if exits and math.isnan(hist[-1]):
                    return end(False, "k_l2_u0")
            if it == iters:
                return end(False, None)
            # ---- k_l2_u0
            omega = 1.0 if it == 0 else omegas[-2] if k["stale_omega"] and it >= 2 else omegas[-1]
            rho0 = -omega * (1.0 if it == 0 else rho_b)
            beta0 = k["beta_of"](0.0 if it == 0 else alpha_b, rho1, rho0)
            if exits and (rho0 == 0.0 or not _finite(rho0, rho1, beta0)):
                return end(False, "k_l2_u0")
            rho_a = rho1
            u0 = each(lambda ri, ui: u_step(ri, ui, beta0), r0, u0)
            u1 = ahat(u0)                                                      # SpMV with u1.r~
            # ---- k_l2_step0
            gamma = dot(d_spmv, u1, rt)
            alpha_a = step_l2_alpha(rho_a, gamma)
            if exits and (gamma == 0.0 or not _finite(gamma, alpha_a)):
                return end(False, "k_l2_step0")
            r0 = each(lambda ri, ui: r_step(ri, ui, alpha_a), r0, u1)
            y = each(lambda yi, ui: y_step(yi, ui, alpha_a), y, u0)
            r1 = ahat(r0)                                                      # SpMV with r1.r~
            # ---- k_l2_u1
            rho1 = dot(d_spmv, r1, rt)
            beta1 = k["beta_of"](alpha_a, rho1, rho_a)
            if exits and (rho_a == 0.0 or not _finite(rho1, beta1)):
                return end(False, "k_l2_u1")
            rho_b = rho1
            u0 = each(lambda ri, ui: u_step(ri, ui, beta1), r0, u0)
            u1 = each(lambda ri, ui: u_step(ri, ui, beta1), r1, u1)
            u2 = ahat(u1)                                                      # SpMV with u2.r~
            # ---- k_l2_step1
            gamma = dot(d_spmv, u2, rt)
            alpha_b = step_l2_alpha(rho_b, gamma)
            if exits and (gamma == 0.0 or not _finite(gamma, alpha_b)):
                return end(False, "k_l2_step1")
            r0 = each(lambda ri, ui: r_step(ri, ui, alpha_b), r0, u1)
            r1 = each(lambda ri, ui: r_step(ri, ui, alpha_b), r1, u2)
            y = each(lambda yi, ui: y_step(yi, ui, alpha_b), y, u0)
            a11, b1 = dot(d_vec, r1, r1), dot(d_vec, r1, r0)
            r2 = ahat(r1)                                                      # SpMV with (r2.r1, r2.r2)
            a12, a22 = dot(d_spmv, r2, r1), dot(d_spmv, r2, r2)
            b2 = dot(d_vec, r2, r0)                                            # k_l2_dot
            # ---- k_l2_mr
            ok, g1, g2 = k["mr"](a11, a12, a22, b1, b2)
            if exits and not ok:
                return end(False, "k_l2_mr")
            y = each(lambda yi, ai, bi: add2(yi, ai, bi, g1, g2), y, r0, r1)
            u0 = each(lambda vi, ai, bi: sub2(vi, ai, bi, g1, g2), u0, u1, u2)
            r0 = each(lambda vi, ai, bi: sub2(vi, ai, bi, g1, g2), r0, r1, r2)
            rho1, rr = dot(d_vec, rt, r0), dot(d_vec, r0, r0)
            omegas.append(g2)
            scalars.append((beta0, alpha_a, beta1, alpha_b, g1, g2))
            it += 1
            if snapshots is not None:
                snapshots.append(y.copy())


def mirror_run(which, shifted=False, seed=None, iters=MAX_SWEEPS, **neighbour):
    return _mirror_run(which, shifted, seed, iters, tuple(sorted(neighbour.items(), key=lambda kv: kv[0])))


@functools.lru_cache(maxsize=None)
def _mirror_run(which, shifted, seed, iters, neighbour):
    """`iters` sweeps without a stopping test on inputs(which, shifted, seed=seed), M = I: (x after 1, 2, ... sweeps, history).
    Shared between tests, not to be written."""
    A, b, x0, d = inputs(which, shifted, seed=seed)
    snaps = []
    run = loop(A, b, x0, d=d, iters=iters, snapshots=snaps, **dict(neighbour))
    assert run.iters == iters and all(np.all(np.isfinite(x)) for x in snaps) and np.all(np.isfinite(run.history))
    return frozen(*snaps), frozen(run.history)[0]


def pinned(which, shifted=False, iters=SWEEPS, **neighbour):
    """x and the history after `iters` sweeps with FLAG_NO_EXIT (a shorter run is a prefix of a longer one: the last norm comes
    from the same partial sums in the same order whether k_l2_u0 or k_l2_check forms it -- test_a_shorter_run_is_a_prefix)"""
    xs, h = mirror_run(which, shifted, iters=max(iters, MAX_SWEEPS), **neighbour)
    return xs[iters - 1], h[:iters]


@functools.lru_cache(maxsize=None)
def _ilu0_run(seed, maxit, neighbour):
    a, b, x0, _ = inputs("diagonal", precond=True, seed=seed)
    run = loop(a, b, x0, precond=True, iters=maxit, tol=0.0, **dict(neighbour))
    frozen(run.x, run.history)
    return run


def ilu0_run(seed=None, maxit=40, **neighbour):
    """the ILU(0) loop on the diagonal system with tol = 0: every stopping and breakdown test taken, no residual passes"""
    return _ilu0_run(seed, maxit, tuple(sorted(neighbour.items(), key=lambda kv: kv[0])))


ILU_SWEEPS = 2            # (module docstring; asserted by test_ilu0_sweeps_and_breakdown)
ILU_WHERE = "k_l2_mr"
# with ILU(0) x cannot differ for these (module docstring): the history, iters or the breakdown flag must
IN_HISTORY_ONLY = ("omega of the sweep before",)

TOL_EXIT = 2e-4           # banded, unshifted: leaves after 3 sweeps (test_the_exit_case_ends_where_intended)
EXIT_SWEEPS = 3


@functools.lru_cache(maxsize=None)
def pinned_exit(tol=None, maxit=20):
    A, b, x0, _ = inputs("banded")
    run = loop(A, b, x0, iters=maxit, tol=TOL_EXIT if tol is None else tol)
    frozen(run.x, run.history)
    return run


NEIGHBOURS = (("u-update as r - fl(beta u)", dict(u_step=step_l2_u_two_roundings)),
              ("r step in two roundings", dict(r_step=step_l2_r_two_roundings)),
              ("y step in two roundings", dict(y_step=step_l2_y_two_roundings)),
              ("add2 with the g2 term first", dict(add2=step_l2_add2_g2_first)),
              ("sub2 with the g2 term first", dict(sub2=step_l2_sub2_g2_first)),
              ("add2 in three roundings", dict(add2=step_l2_add2_three_roundings)),
              ("beta as alpha (rho1 / rho0)", dict(beta_of=step_l2_beta_quotient_first)),
              ("(g1, g2) with plain products", dict(mr=step_l2_mr_plain_products)),
              ("(g1, g2) by Cramer's rule", dict(mr=step_l2_mr_cramer)),
              ("dot terms in two roundings", dict(term=dot_step_two_roundings)),
              ("omega of the sweep before", dict(stale_omega=True)))
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


def least_differing(which, shifted=False, seed=None, **neighbour):
    """entries of x in which the neighbour differs from the pinned arithmetic (M = I): the smaller of the counts after the two
    sweep counts the GPU tests run, and the number of history entries that differ"""
    xs, h = mirror_run(which, shifted, seed)
    xa, ha = mirror_run(which, shifted, seed, **neighbour)
    return min(differing(xa[k - 1], xs[k - 1]) for k in (SWEEPS, MAX_SWEEPS)), differing(ha, h)


def ilu0_differing(seed=None, **neighbour):
    """the ILU(0) case against a neighbour, both with tol = 0 and the maxit of the GPU test's breakdown run (one more than the sweeps
    the pinned arithmetic completes on that seed): (entries of x that differ, history entries that differ or exist on one side only,
    whether iters or the breakdown flag differ) -- what a GPU run can see"""
    maxit = ilu0_run(seed).iters + 1
    p, q = ilu0_run(seed, maxit), ilu0_run(seed, maxit, **neighbour)
    m = min(len(p.history), len(q.history))
    kh = differing(p.history[:m], q.history[:m]) + abs(len(p.history) - len(q.history))
    return differing(p.x, q.x), kh, (p.iters, p.breakdown) != (q.iters, q.breakdown)


def scan_seeds(which, shifted=False, tried=SEEDS_TRIED):
    """the seeds of 0 .. tried - 1 on which every neighbour of the case (M = I) shows in >= MIN_DIFFERING_ROWS entries of x"""
    return [seed for seed in range(tried)
            if all(least_differing(which, shifted, seed, **kw)[0] >= MIN_DIFFERING_ROWS for _, kw in neighbours_of(which, shifted, False))]


def scan_ilu0_seeds(tried=ILU_SEEDS_TRIED, least_sweeps=2):
    """seeds of 0 .. tried - 1 on which the ILU(0) loop completes >= least_sweeps sweeps and then breaks down, and on which every
    neighbour shows: in >= MIN_DIFFERING_ROWS entries of x, or (IN_HISTORY_ONLY) in the history, iters or the breakdown flag"""
    out = []
    for seed in range(tried):
        run = ilu0_run(seed)
        if not run.breakdown or run.iters < least_sweeps:
            continue
        shows = {name: ilu0_differing(seed, **kw) for name, kw in neighbours_of("diagonal", False, True)}
        if all((kx >= MIN_DIFFERING_ROWS) or (name in IN_HISTORY_ONLY and (kh >= 1 or other)) for name, (kx, kh, other) in shows.items()):
            out.append(seed)
    return out


# ------------------------------------------------------------------ tests
def test_partitions_are_the_ones_described():
    A = banded()
    assert A.n == BAND_N and stream_plan(A.rp) == (256, 4) and spmv_partition(LANES, N) == (151, 4)
    # the SpMV's dots: 4 stream tiles of 256 rows (the last of 9) on the banded system, 151 workgroups of 4 one-row groups on the
    # diagonal one; a thread holds one term
    assert spmv_dealing(A) == tile_threads(BAND_N, 256, 4) and spmv_dealing(system(0)[0]) == spmv_threads(N, LANES)
    assert spmv_dealing(A)[3][8] == [776] and spmv_dealing(A)[3][9] == [] and spmv_dealing(system(0)[0])[150][0] == [600]
    assert max(len(mine) for block in spmv_dealing(A) for mine in block) == 1
    assert max(len(mine) for block in spmv_dealing(system(0)[0]) for mine in block) == 1
    # every vector kernel: pairs, two workgroups, an odd tail; a thread holds two or three terms
    assert vec_grid(N) == 2 and vec_grid(BAND_N) == 2
    assert vec_threads(N, 1)[0][0] == [0, 1, 600] and vec_threads(BAND_N, 1)[0][0] == [0, 1, 776]
    assert vec_threads(BAND_N, 1)[1][131] == [774, 775] and vec_threads(BAND_N, 1)[1][132] == []
    assert sorted({len(mine) for block in vec_threads(N, 1) for mine in block}) == [0, 2, 3]
    for deal, n in ((vec_threads(BAND_N, 1), BAND_N), (vec_threads(N, 1), N), (spmv_dealing(A), BAND_N), (spmv_dealing(system(0)[0]), N)):
        assert sorted(i for block in deal for mine in block for i in mine) == list(range(n))
    # the inputs are the draws of the files this one borrows from
    import test_cg_rounding as G
    for got, want in zip(diag_system(5), G.diag_system(5)):
        np.testing.assert_array_equal(got, want)
    assert inputs("banded")[0] is banded() and np.array_equal(inputs("banded", shifted=True)[3], shift_of(BAND_N))


def test_the_first_sweep_starts_as_described():
    """rho' = 1, alpha = 0, omega = 1 in the first k_l2_u0: beta is -0.0 and u0 stays r0"""
    assert math.copysign(1.0, step_l2_beta(0.0, 3.0, -1.0 * 1.0)) == -1.0 and step_l2_beta(0.0, 3.0, -1.0) == 0.0
    for r in (1.5, 0.0, -2.0 ** -1074, 2.0 ** 1023):
        assert step_l2_u(r, r, -0.0) == r
    A, b, x0, _ = inputs("banded")
    run = loop(A, b, x0, iters=1)
    assert run.scalars[0][0] == 0.0 and math.copysign(1.0, run.scalars[0][0]) == -1.0


def test_the_l2_mirror_tells_its_neighbours_apart():
    """without a GPU, on the inputs of test_gpu_l2_bits.py: after 3 and after 4 sweeps the pinned arithmetic differs in
    >= MIN_DIFFERING_ROWS entries of x from every neighbour of its case; with ILU(0) the comparison is of the two breakdown
    runs, and the neighbour that cannot reach x there (IN_HISTORY_ONLY, module docstring) differs in the history, in iters or in
    the breakdown flag"""
    for which, shifted, precond in CASES:
        for name, kw in neighbours_of(which, shifted, precond):
            if precond:
                k, kh, other = ilu0_differing(**kw)
                print("diagonal ILU(0)", name, "differs in", k, "entries of x,", kh, "residuals; iters or the breakdown flag differ:", other)
                if name in IN_HISTORY_ONLY:
                    assert k < MIN_DIFFERING_ROWS and (kh >= 1 or other), name
                else:
                    assert k >= MIN_DIFFERING_ROWS, name
                continue
            k, kh = least_differing(which, shifted, **kw)
            print(which, "shifted" if shifted else "", name, "differs in", k, "entries of x and", kh, "residuals")
            assert k >= MIN_DIFFERING_ROWS, (which, shifted, name)
        if precond:
            continue
        # the iteration is a real one: the residual falls and the mirror's x solves the system better than x0
        A, b, x0, d = inputs(which, shifted)
        x, h = pinned(which, shifted, iters=MAX_SWEEPS)
        res = lambda v: np.linalg.norm(b - product(A, v, d, row_sum_products, shift_fused))
        assert h[-1] < h[0] and res(x) < 1e-3 * res(x0)


def test_the_pinned_seeds_are_the_first_listed():
    """each case takes the first seed of its list (module docstring; the lists are what scan_seeds and scan_ilu0_seeds return -- half a
    minute per case, so not redone here: test_the_l2_mirror_tells_its_neighbours_apart checks the seeds taken)"""
    assert (SEEDS_DIAGONAL[0], SEEDS_BANDED[0], SEEDS_SHIFTED[0], SEEDS_ILU[0]) == (DIAG_SEED, BAND_SEED_RHS, BAND_SEED_SHIFTED, ILU_SEED)
    assert max(SEEDS_DIAGONAL + SEEDS_BANDED + SEEDS_SHIFTED) < SEEDS_TRIED and max(SEEDS_ILU) < ILU_SEEDS_TRIED


def test_a_shorter_run_is_a_prefix():
    """what pinned() relies on: three sweeps asked for as such equal the first three of four, history included"""
    for which, shifted, _ in CASES[:3]:
        A, b, x0, d = inputs(which, shifted)
        run = loop(A, b, x0, d=d, iters=SWEEPS)
        x, h = pinned(which, shifted, iters=SWEEPS)
        assert (run.iters, run.converged, run.breakdown, len(h)) == (SWEEPS, False, False, SWEEPS)
        np.testing.assert_array_equal(run.x, x)
        np.testing.assert_array_equal(run.history, h)
    # ILU(0): the run that stops at ILU_SWEEPS is the start of the one that breaks down in the next sweep
    short, broken = ilu0_run(maxit=ILU_SWEEPS), ilu0_run(maxit=ILU_SWEEPS + 1)
    np.testing.assert_array_equal(short.history, broken.history)


def test_the_exit_case_ends_where_intended():
    """the banded system solved to TOL_EXIT leaves after EXIT_SWEEPS sweeps: the deciding residual is >= 1 % below tolabs and every
    earlier one >= 1 % above, so a kernel wrong in the last bit fails on bits and not on a flipped decision"""
    run = pinned_exit()
    xs, h = mirror_run("banded")
    tolabs = TOL_EXIT * run.nrm0
    print("tol", TOL_EXIT, "-> sweeps", run.iters, "deciding residual / tolabs", run.history[-1] / tolabs,
          "smallest earlier one / tolabs", run.history[:-1].min() / tolabs)
    assert EXIT_SWEEPS in (2, 3)
    assert (run.iters, run.converged, run.breakdown, len(run.history)) == (EXIT_SWEEPS, True, False, EXIT_SWEEPS)
    assert run.history[-1] <= (1.0 - EXIT_MARGIN) * tolabs and run.history[:-1].min() >= (1.0 + EXIT_MARGIN) * tolabs
    np.testing.assert_array_equal(run.history, h[:EXIT_SWEEPS])
    np.testing.assert_array_equal(run.x, xs[EXIT_SWEEPS - 1])


def test_ilu0_sweeps_and_breakdown():
    """ILU(0) on the diagonal system, tol = 0: the mirror completes ILU_SWEEPS sweeps and the kernel ILU_WHERE of the next one
    reports the breakdown; x = x0 + M^-1 y carries the updates of the interrupted sweep that preceded it (k_l2_step0's and
    k_l2_step1's y), and solves the system to rounding either way"""
    short, broken = ilu0_run(maxit=ILU_SWEEPS), ilu0_run(maxit=ILU_SWEEPS + 1)
    print("ILU(0) on the diagonal system: sweeps", broken.iters, "then a breakdown in", broken.where, "history", broken.history)
    assert (short.iters, short.converged, short.breakdown, len(short.history)) == (ILU_SWEEPS, False, False, ILU_SWEEPS)
    assert (broken.iters, broken.converged, broken.breakdown, broken.where) == (ILU_SWEEPS, False, True, ILU_WHERE)
    assert len(broken.history) == ILU_SWEEPS and ILU_SWEEPS >= 2
    full = ilu0_run()
    assert (full.iters, full.where) == (broken.iters, broken.where)
    np.testing.assert_array_equal(full.x, broken.x)
    a, b, x0, _ = inputs("diagonal", precond=True)
    for run in (short, broken):
        assert np.linalg.norm(b - a * run.x) < 1e-10 * np.linalg.norm(b - a * x0)


def _scaled(A, c):
    if isinstance(A, Csr):
        return Csr(A.rp, A.ci, A.val * c)
    return A * c


@functools.lru_cache(maxsize=None)
def _range_base(which):
    A, b, x0, _ = inputs(which)
    run = loop(A, b, x0, iters=SWEEPS, tol=0.0)
    assert (run.iters, run.breakdown) == (SWEEPS, False)
    return run


def test_rhs_scaling_is_bitwise_on_the_mirror():
    """DESIGN.md section 4, Range, on the mirror itself, with every breakdown test taken (tol = 0): (c b, c x0) at c = 2^k, k of
    test_gpu_scaling.EXPONENTS, gives c x and c times the history with 0 entries differing -- and with Cramer's rule in the
    place of the elimination the first sweep's k_l2_mr reports a breakdown at k = +-440 (det ~ c^4 is inf or 0)"""
    for which in ("diagonal", "banded"):
        A, b, x0, _ = inputs(which)
        base = _range_base(which)
        for k in EXPONENTS:
            c = 2.0 ** k
            run = loop(A, c * b, c * x0, iters=SWEEPS, tol=0.0)
            assert (run.iters, run.breakdown, run.nrm0) == (SWEEPS, False, c * base.nrm0), (which, k)
            assert differing(run.x, c * base.x) == 0 and differing(run.history, c * base.history) == 0, (which, k)
            assert run.scalars == base.scalars, (which, k)
        for k in (-440, 440):
            c = 2.0 ** k
            run = loop(A, c * b, c * x0, iters=SWEEPS, tol=0.0, mr=step_l2_mr_cramer)
            assert (run.iters, run.breakdown, run.where, len(run.history)) == (0, True, "k_l2_mr", 0), (which, k)
        assert loop(A, b, x0, iters=SWEEPS, tol=0.0, mr=step_l2_mr_cramer).iters == SWEEPS


def test_matrix_scaling_is_bitwise_on_the_mirror():
    """(c A, b, x0 / c) at c = 2^k, k of test_gpu_scaling.MAT_EXPONENTS: x / c and the same history, 0 entries differing; the
    largest intermediate is the pivot t ~ c^4 (2^+-800 at k = +-200).  Cramer's rule (det ~ c^6) breaks down in the first sweep
    at k = +-200."""
    for which in ("diagonal", "banded"):
        A, b, x0, _ = inputs(which)
        base = _range_base(which)
        for k in MAT_EXPONENTS:
            c = 2.0 ** k
            run = loop(_scaled(A, c), b, x0 / c, iters=SWEEPS, tol=0.0)
            assert (run.iters, run.breakdown, run.nrm0) == (SWEEPS, False, base.nrm0), (which, k)
            assert differing(run.x, base.x / c) == 0 and differing(run.history, base.history) == 0, (which, k)
        for k in (-200, 200):
            c = 2.0 ** k
            run = loop(_scaled(A, c), b, x0 / c, iters=SWEEPS, tol=0.0, mr=step_l2_mr_cramer)
            assert (run.iters, run.breakdown, run.where) == (0, True, "k_l2_mr"), (which, k)


def test_the_mirror_reproduces_the_recorded_values():
    """tests/golden/l2_pinned.npz holds x and the history the mirror gave for every pinned case when the file was written
    (tests/golden/make_golden.py l2_pinned; produced by this mirror, on the CPU): an edit of the mirror cannot move the target
    of the GPU tests silently"""
    want = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "l2_pinned.npz"))
    got = recorded_values()
    assert sorted(want.files) == sorted(got)
    for key, value in got.items():
        np.testing.assert_array_equal(value, want[key], err_msg=key)


def recorded_values():
    out = {}
    for which, shifted, precond in CASES:
        tag = which + ("_shifted" if shifted else "") + ("_ilu0" if precond else "")
        for iters in ((ILU_SWEEPS, ILU_SWEEPS + 1) if precond else (SWEEPS, MAX_SWEEPS)):
            if precond:
                run = ilu0_run(maxit=iters)
                x, h = run.x, run.history
            else:
                x, h = pinned(which, shifted, iters=iters)
            out["%s_%d_x" % (tag, iters)], out["%s_%d_h" % (tag, iters)] = np.array(x), np.array(h)
    run = pinned_exit()
    out["exit_x"], out["exit_h"] = np.array(run.x), np.array(run.history)
    return out
