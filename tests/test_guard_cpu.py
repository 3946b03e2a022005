"""Guarded solves (CUDAMAT_FLAG_GUARD, the switches GUARD and GUARD_RHO_ULPS) without a GPU: the switch table and the flag, and
the guarded loop restated on the CPU bit for bit from the pieces of test_loop_rounding.py.

The guarded loop is the five-launch loop of that file (form "five/lanes") plus
  the sum     k_full<VEC, true> forms sum |rw_i| |r_i| beside (rw.r, r.r): dot_step(acc, fabs(rw_i), fabs(r_i)) in k_full's own
              dealing, block_sum<3>, partials of stride 3, summed by load_scalars like the other two;
  the test    check_rho (device.h) at the top of iteration it >= 1, after the full-step test of iteration it - 1 (a convergence
              exit wins; at it = 0, rho = r.r): |rho| <= eps * sum with eps = GUARD_RHO_ULPS * 2^-52 (exact) and one rounding
              in the product -- rho = 0 and a NaN rho fire too.  It ends the SEGMENT in state 4 with x the complete iterate of
              iteration it - 1; k_check after the last iteration of a segment does not run it; under FLAG_NO_EXIT (tol = None)
              it is never taken;
  a restart   a new segment from x: r = b - (A + d) x through `product` and k_init's dealing, rw = p = r, rho = alpha = omega =
              1, towards tolabs = tol * nrm0 of the FIRST segment; it starts 'converged' (state 2, no iteration) when its
              nrm0 <= 2 tolabs (k_init_finish's rule for abs_tol);
  the host    cudamat_solver_solve (loops.hip): a segment ended by the test -> rho_restarts += 1, restart with the iterations
              that are left; a segment that reports convergence -> verified by a restart (`restarts`, at most three; then, or
              when no iteration is left, a segment of no iterations evaluates the true residual once more and a failure returns
              converged = 0); converged = 1 only from a segment that started within 2 tolabs.  Histories follow one another.
The GPU tests that pin the kernels to this mirror are test_guard_bits_* in test_gpu_guard.py."""
import collections
import ctypes
import functools
import math
import os
import re

import numpy as np

import test_loop_rounding as L
from test_loop_rounding import MIN_DIFFERING_ROWS, dot_parts, dot_step, each, load_scalars

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ULPS_MAX = 1 << 52
FORM = "five/lanes"

Segment = collections.namedtuple("Segment", "state it x history nrm0 nrm fired_at")
GRun = collections.namedtuple("GRun", "iters half_exit converged rho_restarts restarts x history nrm fired")


def rho_eps(ulps):
    """GUARD_RHO_ULPS * 2^-52 as Solve::setup forms it: (double)ulps * 0x1p-52, exact for ulps <= 2^52"""
    return float(ulps) * 2.0 ** -52


def segment(A, b, x0, vec, kind, d, precond, iters, tol, tolabs, eps):
    """One segment of a guarded solve: Solve::setup, at most `iters` iterations of iterate_reference with the GUARD kernels,
    Solve::finish.  tolabs = None: the first segment (tolabs = tol * nrm0; tol = None: FLAG_NO_EXIT); else a restart towards
    that absolute target.  eps: rho_eps(GUARD_RHO_ULPS).  state as LoopState.state: 0 ran out of iterations, 1 half-step exit,
    2 full-step exit (or converged at once), 4 the test on rho fired."""
    two = kind == "pbicgstab2"
    n = len(b)
    d_init, d_spmv, d_half, d_full = L.dealings(A, FORM, vec)
    def mv(z): return L.product(A, z, d, L.row_sum_products, L.shift_fused)
    minv = L.minv_dinv
    x = np.array(x0, np.float64)
    r = each(L.step_r0, b, mv(x))                                # r = b - (A + d) x
    rw, p, v = r.copy(), r.copy(), np.zeros(n)
    init = dot_parts(d_init, r, r, dot_step)
    nrm0 = math.sqrt(load_scalars(init))
    assert math.isfinite(nrm0), "a refused restart: not restated"
    restart = tolabs is not None
    if not restart and tol is not None:
        tolabs = tol * nrm0                                      # k_init_finish
    if nrm0 == 0.0 or (restart and nrm0 <= 2.0 * tolabs):
        return Segment(2, 0, x, [], nrm0, nrm0, None)
    full = [init, init, None]                                    # (rw.r, r.r) = (r.r, r.r); no third sum before k_full has run
    rho_s, alpha, omega, hist, it, nrm = [1.0, 1.0], 1.0, 1.0, [], 0, nrm0
    while True:
        rho, rr = load_scalars(full[0]), load_scalars(full[1])   # k_update_p<VEC, true>; after the last iteration k_check
        if it:                                                   # check_full
            nrm = math.sqrt(rr)
            hist.append(nrm)
            if tolabs is not None and nrm < tolabs:
                return Segment(2, it, x, hist, nrm0, nrm, None)
            assert tolabs is None or not two or abs(omega) >= L.OMEGA_MIN, "breakdown: not restated"
            assert not math.isnan(nrm), "breakdown: not restated"
        if it == iters:
            return Segment(0, it, x, hist, nrm0, nrm, None)      # (k_check: no test on rho)
        if it:                                                   # check_rho
            mag = load_scalars(full[2])
            assert abs(rho) <= mag
            if not abs(rho) > eps * mag and tolabs is not None:
                return Segment(4, it, x, hist, nrm0, nrm, it)
        rho_prev, rho_s[it & 1] = rho_s[(it + 1) & 1], rho
        if it:
            beta = L.step_beta(rho, rho_prev, alpha, omega)
            p = each(lambda ri, pi, vi: L.step_p(ri, pi, vi, beta, omega), r, p, v)
        pw = minv(A, p) if precond else p
        v = mv(pw)
        alpha = L.step_alpha(rho, load_scalars(dot_parts(d_spmv, v, rw, dot_step)))
        r = each(lambda ri, vi: L.step_r_half(ri, vi, alpha), r, v)
        nrm_half = math.sqrt(load_scalars(dot_parts(d_half, r, r, dot_step)))
        if not two:
            nrm = nrm_half
            hist.append(nrm)
            assert not math.isnan(nrm), "breakdown: not restated"
            if tolabs is not None and nrm < tolabs:
                return Segment(1, it, each(lambda xi, pi: L.step_x_half(xi, pi, alpha), x, pw), hist, nrm0, nrm, None)
        s = minv(A, r) if precond else r
        t = mv(s)
        omega = L.step_omega(load_scalars(dot_parts(d_spmv, t, r, dot_step)), load_scalars(dot_parts(d_spmv, t, t, dot_step)))
        x = each(lambda xi, pi, si: L.step_x_full(L.step_x_half(xi, pi, alpha), si, omega), x, pw, s)
        r = each(lambda ri, ti: L.step_r_full(ri, ti, omega), r, t)
        full = [dot_parts(d_full, rw, r, dot_step), dot_parts(d_full, r, r, dot_step),
                dot_parts(d_full, np.abs(rw), np.abs(r), dot_step)]
        it += 1


def guarded(A, b, x0, vec=(1, 1, 1), kind="pbicgstab", d=None, precond=False, maxit=L.ITERS, tol=None, ulps=4):
    """cudamat_solver_solve with CUDAMAT_FLAG_GUARD (tol = None: | FLAG_NO_EXIT) as the five-launch loop on the lanes plan runs
    it.  fired: the iterations, counted over the whole solve, at whose top the test on rho fired."""
    eps = rho_eps(ulps)
    seg = segment(A, b, x0, vec, kind, d, precond, maxit, tol, None, eps)
    iters, half_exit, converged, nrm = seg.it, seg.state == 1, seg.state in (1, 2), seg.nrm
    rho_restarts = restarts = 0
    x, hist, state, fired = seg.x, list(seg.history), seg.state, []
    target = None if tol is None else tol * seg.nrm0
    while target is not None and target > 0.0 and (state == 4 or converged):
        verify = state != 4
        left = 0 if verify and restarts >= 3 else maxit - iters
        if not verify:
            rho_restarts += 1
            fired.append(iters)
        seg = segment(A, b, x, vec, kind, d, precond, left, tol, target, eps)
        state, nrm, x = seg.state, seg.nrm, seg.x
        hist += seg.history
        if seg.it == 0 and seg.state == 2:
            converged = True
            break
        if verify and left == 0:
            converged, half_exit = False, False
            break
        if verify:
            restarts += 1
        iters += seg.it
        converged, half_exit = seg.state in (1, 2), seg.state == 1
    return GRun(iters, half_exit, converged, rho_restarts, restarts, x, np.array(hist), nrm, tuple(fired))


# ------------------------------------------------------------------ the cases the GPU tests pin (test_gpu_guard.py)
# Found here on the CPU, by running this mirror -- never from GPU output.  On the n = 601 diagonal system, M = I, the unguarded
# run has |rho| / sum |rw_i r_i| = 0.9998, 0.855, 0.552, 0.350, 0.212, 0.117, 0.066 at the top of iterations 1 .. 7 (column 2,
# pairs; 1.0000, 0.883, 0.535, 0.331, ... for column 0, rows; 0.998, 0.927, 0.674, 0.426, ... with the shift): a healthy rho, which
# the default of 4 ulp is 2^50 away from.  So the middle setting is a large one, ULPS_MIDDLE = 0.7 * 2^52: the test passes at
# iterations 1 and 2 and fires at iteration 3, and again later in the restarted segments (FIRED_MIDDLE: the iterations, counted
# over the whole solve).  TOL and MAXIT are chosen so that the unguarded solve takes 7 iterations.
TOL, MAXIT = 1e-9, 12
TOL_TIGHT = 1e-17              # ILU(0) only: below what the true residual can reach, so that every verification fails
ULPS_MIDDLE = 3152519739159347
LAYOUT_COL = {"aligned": 2, "offset8": 0}
CASES = {                      # kind, shifted, precond
    "pbicgstab": ("pbicgstab", False, False), "pbicgstab2": ("pbicgstab2", False, False),
    "pbicgstab2_shift": ("pbicgstab2", True, False), "ilu0": ("pbicgstab", False, True),
}
assert ULPS_MIDDLE == round(0.7 * ULPS_MAX)


@functools.lru_cache(maxsize=None)
def pinned_guard(layout, case, ulps, maxit=MAXIT, tol=TOL):
    """the guarded mirror on the diagonal system: shared between tests, not to be written"""
    kind, shifted, precond = CASES[case]
    a, b, x0 = L.system(LAYOUT_COL[layout])
    run = guarded(a, b, x0, vec=L.LAYOUTS[layout], kind=kind, d=L.shift_of(L.N) if shifted else None, precond=precond,
                  maxit=maxit, tol=tol, ulps=ulps)
    L.frozen(run.x, run.history)
    return run


ZERO_A = L.Csr([0, 3, 6, 7], [0, 1, 2, 0, 1, 2, 2], [2.0, -2.0, 1.0, 2.0, 2.0, -2.0, 1.0])
ZERO_B, ZERO_X = np.array([0.0, 0.0, 2.0]), np.array([0.5, 1.5, 2.0])


# ------------------------------------------------------------------ switches and the flag
def test_the_switches_are_validated_and_listed():
    import cuda_mat_amd as cm
    lib = cm.lib()
    ok = [("GUARD", "0"), ("GUARD", "1"), ("CUDAMAT_GUARD", "1"), ("GUARD_RHO_ULPS", "1"), ("GUARD_RHO_ULPS", "4"),
          ("GUARD_RHO_ULPS", "4503599627370496")]
    bad = [("GUARD", "2"), ("GUARD", "x"), ("GUARD_RHO_ULPS", "0"), ("GUARD_RHO_ULPS", "-1"), ("GUARD_RHO_ULPS", "x"),
           ("GUARD_RHO_ULPS", "4503599627370497")]
    assert ULPS_MAX == 4503599627370496
    for name, value in ok:
        assert lib.cudamat_option_check(name.encode(), value.encode()) == 0, (name, value)
    for name, value in bad:
        assert lib.cudamat_option_check(name.encode(), value.encode()) != 0, (name, value)
        assert name in lib.cudamat_last_error().decode()
    text = lib.cudamat_options_help().decode()
    assert re.search(r"^CUDAMAT_GUARD = 0 \| 1 ", text, re.M) and re.search(r"^CUDAMAT_GUARD_RHO_ULPS = N in \[1, 4503599627370496\]", text, re.M)


def test_the_flag_has_a_bit_of_its_own_and_the_statistic_is_the_last_field():
    import cuda_mat_amd as cm
    hdr = open(os.path.join(ROOT, "include", "cudamat.h")).read()
    flags = dict((k, int(v)) for k, v in re.findall(r"^#define (CUDAMAT_FLAG_[A-Z0-9_]+)\s+(\d+)", hdr, re.M))
    assert flags["CUDAMAT_FLAG_GUARD"] == 16 == cm.FLAG_GUARD
    assert len(flags) == 5 and all(v & (v - 1) == 0 for v in flags.values()) and len(set(flags.values())) == len(flags)
    from cuda_mat_amd import api
    assert api.FLAG_GUARD == 16
    assert cm.Stats._fields_[-1] == ("rho_restarts", ctypes.c_int) and cm.Stats._fields_[-2][0] == "trsv_groups_u"
    assert "rho_restarts" in cm.Stats().as_dict()


# ------------------------------------------------------------------ the mirror
@functools.lru_cache(maxsize=None)
def _unguarded(layout, case, tol=None, maxit=L.ITERS):
    kind, shifted, precond = CASES[case]
    a, b, x0 = L.system(LAYOUT_COL[layout])
    return L.loop(a, b, x0, vec=L.LAYOUTS[layout], kind=kind, d=L.shift_of(L.N) if shifted else None, precond=precond,
                  iters=maxit, tol=tol)


def test_a_guard_that_never_fires_is_the_unguarded_loop():
    """no stopping test (FLAG_NO_EXIT: the test on rho is evaluated and never taken) and a threshold of 1 ulp: x and the
    history of test_loop_rounding.loop bit for bit, in both layouts, for both loops, with a shift and with ILU(0)"""
    for layout in LAYOUT_COL:
        for case in CASES:
            kind, shifted, precond = CASES[case]
            a, b, x0 = L.system(LAYOUT_COL[layout])
            want = _unguarded(layout, case)
            for ulps in (1, ULPS_MAX):
                got = guarded(a, b, x0, vec=L.LAYOUTS[layout], kind=kind, d=L.shift_of(L.N) if shifted else None, precond=precond,
                              maxit=L.ITERS, tol=None, ulps=ulps)
                assert (got.iters, got.half_exit, got.rho_restarts, got.restarts, got.fired) == (L.ITERS, False, 0, 0, ())
                np.testing.assert_array_equal(got.x, want.x)
                np.testing.assert_array_equal(got.history, want.history)
    # with a stopping test, the default of 4 ulp does not fire on this system either: the iterations are the unguarded
    # run's, followed by the verification of its iterate (here: accepted at once, no restart)
    got, want = pinned_guard("aligned", "pbicgstab", 4), _unguarded("aligned", "pbicgstab", TOL, MAXIT)
    assert got.converged and (got.iters, got.half_exit, got.rho_restarts, got.restarts) == (want.iters, want.half_exit, 0, 0)
    assert 1 <= want.iters < MAXIT
    np.testing.assert_array_equal(got.x, want.x)
    np.testing.assert_array_equal(got.history, want.history)


def test_the_largest_threshold_restarts_at_every_iteration():
    """GUARD_RHO_ULPS = 2^52: |rho| <= sum |rw_i r_i| always holds (the same terms in the same order), so every segment is
    ended by the test at the top of its iteration 1"""
    for layout in LAYOUT_COL:
        run = pinned_guard(layout, "pbicgstab", ULPS_MAX)
        print(layout, "2^52 ulp:", run.iters, "iterations, converged", run.converged, "restarts at", run.fired, "verification restarts", run.restarts)
        assert run.iters >= 3 and run.fired == tuple(range(1, len(run.fired) + 1)) and run.rho_restarts == len(run.fired)
        assert run.rho_restarts in (run.iters, run.iters - 1) and run.converged
        assert differing(run.x, _unguarded(layout, "pbicgstab", TOL, MAXIT).x) >= MIN_DIFFERING_ROWS


def differing(a, b):
    return int(np.count_nonzero(a != b))


FIRED_MIDDLE = {"aligned": (3, 5), "offset8": (3, 5)}      # of 6 iterations; the unguarded solve takes 7


def test_the_middle_setting_fires_at_some_iterations_and_not_at_others():
    """ULPS_MIDDLE on the diagonal system: within the first ITERS iterations the test fires at least once and at least one
    iteration >= 1 passes without firing; x differs from the unguarded mirror's in >= MIN_DIFFERING_ROWS rows"""
    for layout in LAYOUT_COL:
        run = pinned_guard(layout, "pbicgstab", ULPS_MIDDLE)
        early = [k for k in run.fired if k <= L.ITERS]
        print(layout, "middle setting: fires at", run.fired, "of", run.iters, "iterations")
        assert run.fired == FIRED_MIDDLE[layout]
        assert len(early) >= 1 and len(early) < min(run.iters, L.ITERS)
        assert differing(run.x, _unguarded(layout, "pbicgstab", TOL, MAXIT).x) >= MIN_DIFFERING_ROWS
        assert np.all(np.isfinite(run.x)) and np.all(np.isfinite(run.history))


def test_the_exact_zero_system():
    """A = [[2, -2, 1], [2, 2, -2], [0, 0, 1]], b = (0, 0, 2), x0 = 0, M = I: rho of iteration 1 is exactly 0 with r = (1, 3, 0).
    Every intermediate of iterations 0 and 1 and of the restarted segment is a small dyadic number (alpha = 1, omega = 1 / 4,
    x = (-1/2, 1, 2) at the restart; checked in exact rational arithmetic), so no order of summation matters: the unguarded loop
    ends in 0 / 0, the guarded one restarts once and reaches x = (1/2, 3/2, 2) with a residual of exactly 0."""
    from fractions import Fraction as F
    A = [[F(2), F(-2), F(1)], [F(2), F(2), F(-2)], [F(0), F(0), F(1)]]
    def mv(z): return [sum(a * zj for a, zj in zip(row, z)) for row in A]
    def dot(u, w): return sum(p * q for p, q in zip(u, w))
    r = [F(0), F(0), F(2)]
    rw, p, x = list(r), list(r), [F(0)] * 3
    v = mv(p); alpha = dot(rw, r) / dot(rw, v)
    s = [ri - alpha * vi for ri, vi in zip(r, v)]
    t = mv(s); omega = dot(t, s) / dot(t, t)
    x = [xi + alpha * pi + omega * si for xi, pi, si in zip(x, p, s)]
    r = [si - omega * ti for si, ti in zip(s, t)]
    assert (alpha, omega, x, r, dot(rw, r)) == (1, F(1, 4), [F(-1, 2), 1, 2], [1, 3, 0], 0)
    # (CUDAMAT_LOOP_PBICGSTAB: the restarted segment ends at the half step of its iteration 1 with s = 0 exactly.  The other loop
    # has no half-step test, pbicgstab.cu:581-754, and goes on to omega = 0 / 0 there: guarded or not, that is its breakdown.)
    for vec in L.LAYOUTS.values():
        first = segment(ZERO_A, ZERO_B, np.zeros(3), vec, "pbicgstab", None, False, 50, 1e-8, None, rho_eps(4))
        assert (first.state, first.it) == (4, 1) and list(first.x) == [-0.5, 1.0, 2.0]
        run = guarded(ZERO_A, ZERO_B, np.zeros(3), vec=vec, maxit=50, tol=1e-8, ulps=4)
        assert (run.converged, run.half_exit, run.iters, run.rho_restarts, run.restarts, run.fired) == (True, True, 2, 1, 0, (1,))
        np.testing.assert_array_equal(run.x, ZERO_X)
        assert run.nrm == 0.0 and np.all(L.product(ZERO_A, run.x, None, L.row_sum_products, None) == ZERO_B)
        # the unguarded loop divides by rho = 0 in iteration 2 (Python raises where the device gets inf and NaN)
        try:
            plain = L.loop(ZERO_A, ZERO_B, np.zeros(3), vec=vec, iters=3)
            assert not np.all(np.isfinite(plain.x))
        except ZeroDivisionError:
            pass


# ------------------------------------------------------------------ what the GPU tests may assert on the non-dominant systems
def numpy_guarded(S, b, maxit, tol, ulps=4, guard=True):
    """The guarded gpu_pbicgstab (M = I, x0 = 1) in plain numpy on a scipy CSR matrix: numpy's own dot products, no fma -- NOT the
    GPU's arithmetic, only what decides which assertions test_gpu_guard.py makes on a system (a restart happens / the solve
    converges for b and its perturbations).  The same rules as `guarded`: the test at the top of iteration it >= 1 after the
    full-step test, restarts from b - A x towards the first target, three verification restarts and a last evaluation.
    Returns (converged, iters, rho_restarts, restarts, true relative residual); a NaN residual ends it unconverged."""
    eps = rho_eps(ulps)
    x = np.ones(len(b))
    iters = rho_restarts = restarts = 0
    target, converged, state = None, False, 0
    with np.errstate(all="ignore"):
        while True:
            verify = state != 4 and target is not None
            left = 0 if verify and restarts >= 3 else maxit - iters
            r = b - S @ x
            nrm0 = float(np.sqrt(r @ r))
            if target is None:
                target = tol * nrm0
            elif nrm0 <= 2.0 * target:
                converged = True
                break
            elif verify and left == 0:
                converged = False
                break
            elif verify:
                restarts += 1
            rw, p, v = r.copy(), r.copy(), np.zeros(len(b))
            rho = rho_prev = alpha = omega = 1.0
            it, state = 0, 0
            full = (r @ r, r @ r, 0.0)
            while True:
                rho_prev, rho = rho, full[0]
                if it and np.sqrt(full[1]) < target:
                    state = 2
                    break
                if it and np.isnan(full[1]):
                    state = 3
                    break
                if it == left:
                    break
                if guard and it and not abs(rho) > eps * full[2]:
                    state = 4
                    break
                if it:
                    p = r + (rho / rho_prev) * (alpha / omega) * (p - omega * v)
                v = S @ p
                alpha = rho / (rw @ v)
                r = r - alpha * v
                hh = r @ r
                if np.sqrt(hh) < target:
                    x, state = x + alpha * p, 1
                    break
                if np.isnan(hh):
                    state = 3
                    break
                t = S @ r
                omega = (t @ r) / (t @ t)
                x = x + alpha * p + omega * r
                r = r - omega * t
                full = (rw @ r, r @ r, np.abs(rw) @ np.abs(r))
                it += 1
            iters += it
            converged = state in (1, 2)
            if state == 4:
                rho_restarts += 1
            elif not converged:
                break
        res = float(np.linalg.norm(b - S @ x)) / (target / tol)
    return converged, iters, rho_restarts, restarts, res


# On which systems test_gpu_guard.py asserts rho_restarts >= 1 / converged = 1: decided here, on the CPU, over b and b (1 + k eps),
# k in nondominant.PERTURB -- seven runs, and only what ALL seven show is asserted of the GPU.
#   converged = 1     numpy_guarded converges in all seven runs: both systems (convdiff_g2 in 302 .. 355 iterations, convdiff_g8 in
#                     535 .. 905 with 13 .. 18 restarts, where the unguarded loop ends in NaNs after 1511).
#   rho_restarts >= 1 two CPU arithmetics must agree, since the GPU's is neither: numpy_guarded restarts in all seven runs, AND in
#                     the oracle's restatement of the unguarded reference loop (sequential dots; its trace holds rho and the sum of
#                     magnitudes) the smallest |rho| / (eps sum |rw_i r_i|) over the solve is <= 4 in all seven runs.
#                     convdiff_g8 passes both (the oracle's rho falls to 0 .. 0.01 eps sum in every run).  convdiff_g2 passes the
#                     first (1 or 2 restarts in each run) and NOT the second: the oracle's smallest ratios are 3.0, 1.1, 2.9, 12.8,
#                     10.3, 2.5, 8.2 -- at iterations 200, 119, 245, 192, 165, 83, 81 --: its rho grazes the threshold at an
#                     iteration that moves with an ulp of b, and whether a run dips below 4 is a matter of its rounding.  So a
#                     restart is asserted on convdiff_g8 only.
ND_MAXIT, ND_TOL = 2000, 1e-6          # the reference CLI's constants (example.cpp:179-180)
ND_RESTARTS = {"convdiff_g2": False, "convdiff_g8": True}
ND_CONVERGES = {"convdiff_g2": True, "convdiff_g8": True}


def test_the_nondominant_tables_are_what_the_cpu_restatements_give(oracle):
    import scipy.sparse as sp
    from tests import nondominant as ND
    before = oracle.num_threads()
    oracle.set_num_threads(1)
    try:
        for name in ND_RESTARTS:
            A, b = ND.FAMILY[name](oracle)
            base = int(A.rowptr[0])
            S = sp.csr_matrix((A.val, A.colidx - base, A.rowptr - base), shape=(A.n, A.n))
            runs, ratios = [], []
            for k in (0,) + ND.PERTURB:
                bk = b * (1.0 + k * ND.EPS)
                runs.append(numpy_guarded(S, bk, ND_MAXIT, ND_TOL))
                _, so, _, tr = oracle.pbicgstab(A, bk, vm=None, maxit=ND_MAXIT, tol=ND_TOL, want_trace=True)
                with np.errstate(all="ignore"):
                    ratios.append(float(np.nanmin(np.abs(tr[1:so.iters, 0]) / (ND.EPS * tr[1:so.iters, 1]))))
            print(name, runs, "the oracle's smallest |rho| / (eps sum):", ratios)
            assert all(r[0] for r in runs) == ND_CONVERGES[name]
            assert (all(r[2] >= 1 for r in runs) and all(q <= 4.0 for q in ratios)) == ND_RESTARTS[name]
            assert all(r[4] <= 2.5 * ND_TOL for r in runs if r[0])          # converged = 1 is backed by the true residual
    finally:
        oracle.set_num_threads(before)
