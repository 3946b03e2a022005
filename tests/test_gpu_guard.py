"""Guarded solves on the GPU (CUDAMAT_FLAG_GUARD, the switches GUARD / GUARD_RHO_ULPS):
 1. test_guard_bits_*: the GUARD kernels and the host's restart rule against the CPU mirror of test_guard_cpu.py, bit for bit;
 2. a guard that never fires changes nothing;
 3. the system on which rho is exactly 0 at iteration 1;
 4. two of the non-dominant systems of tests/nondominant.py, and the ILU(0) solve of DESIGN.md 5a that used to report a
    convergence it had not reached;
 5. what the mode refuses.
Run on the GPU box with:  python -m pytest tests -m gpu"""
import ctypes as C
import os

import numpy as np
import pytest

from tests import nondominant as ND

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cm():
    import cuda_mat_amd as cm
    assert cm.device_count() > 0, "no HIP device: the product has no CPU fallback"
    return cm


@pytest.fixture(scope="module")
def ctx(cm):
    c = cm.Context(0)
    yield c
    c.close()


@pytest.fixture
def sw(ctx, monkeypatch):
    """set a library switch for the rest of this test, on the module's context and in the environment (test_gpu_parity.py)"""
    def _sw(name, value):
        monkeypatch.setenv("CUDAMAT_" + name, str(value))
        ctx.set_option(name, value)
    yield _sw
    monkeypatch.undo()
    ctx.reset_options()


@pytest.fixture(autouse=True)
def _serial_oracle(oracle):
    before = oracle.num_threads()
    oracle.set_num_threads(1)
    yield
    oracle.set_num_threads(before)


def _solve(cm, ctx, s, b, x0, off=0, **kw):
    """solve on device copies of b and x0 that start `off` doubles past a 16-byte boundary: (stats, x, history)"""
    db, dx = ctx.array(np.concatenate([np.zeros(off), b])), ctx.array(np.concatenate([np.zeros(off), x0]))
    try:
        st = s.solve(db.ptr + 8 * off, dx.ptr + 8 * off, **kw)
        return st, dx.download()[off:], s.history()
    finally:
        db.free()
        dx.free()


# ------------------------------------------------------------------ 1. bits against the mirror
@pytest.mark.parametrize("which", ["middle", "max"])
@pytest.mark.parametrize("layout", ["aligned", "offset8"])
@pytest.mark.parametrize("case,tight", [("pbicgstab", False), ("pbicgstab2", False), ("pbicgstab2_shift", False), ("ilu0", False),
                                        ("ilu0", True)])
def test_guard_bits_against_the_mirror(cm, ctx, sw, case, tight, layout, which):
    """the n = 601 diagonal system of test_loop_rounding.py solved to a tolerance with the flag set (which alone forces the
    five-launch loop; SPMV_LANES = 64 is the plan the mirror restates), GUARD_RHO_ULPS at the middle setting of test_guard_cpu.py
    (M = I: fires at iterations 3 and 5) and at 2^52 (fires at every iteration), b and x 16-byte aligned (k_init<1>, k_full<1,
    true>) and 8 bytes off (k_init<0>, k_full<0, true>), both loops, a shift, ILU(0): iters, half_exit, converged, rho_restarts,
    restarts, x and the concatenated history equal the guarded mirror's bit for bit.  ILU(0) of a diagonal matrix is exact, so
    that loop converges at the first half step and only the verification runs; with the tolerance of 1e-17 every verification
    fails (three restarts, then converged = 0 with the true residual as nrm)."""
    import test_guard_cpu as G
    import test_loop_rounding as L
    kind, shifted, precond = G.CASES[case]
    ulps = G.ULPS_MIDDLE if which == "middle" else G.ULPS_MAX
    tol = G.TOL_TIGHT if tight else G.TOL
    want = G.pinned_guard(layout, case, ulps, G.MAXIT, tol)
    a, b, x0 = L.system(G.LAYOUT_COL[layout])
    for name, value in (("SPMV_MODE", "csr"), ("SPMV_LANES", L.LANES), ("GUARD_RHO_ULPS", ulps)):
        sw(name, value)
    s = cm.Solver.from_host_csr(ctx, np.arange(L.N + 1), np.arange(L.N), a)
    try:
        assert s.spmv_kernel().startswith("k_spmv<64>")
        if shifted:
            s.set_shift(ctx.array(L.shift_of(L.N)))
        if precond:
            s.ilu0()
        st, x, h = _solve(cm, ctx, s, b, x0, off=1 if layout == "offset8" else 0, precond=cm.PRECOND_ILU0 if precond else cm.PRECOND_NONE,
                          loop=cm.LOOP_PBICGSTAB if kind == "pbicgstab" else cm.LOOP_PBICGSTAB2, maxit=G.MAXIT, tol=tol, flags=cm.FLAG_GUARD)
    finally:
        s.close()
    got = (st.iters, bool(st.half_exit), bool(st.converged), st.rho_restarts, st.restarts, st.breakdown, st.loop_form)
    print(case, layout, which, "GPU", got, "mirror", want[:5], "fired at", want.fired, "entries of x that differ:", L.differing(x, want.x),
          "history", len(h), len(want.history))
    assert got == (want.iters, want.half_exit, want.converged, want.rho_restarts, want.restarts, 0, 0)
    np.testing.assert_array_equal(h, want.history)
    np.testing.assert_array_equal(x, want.x)
    assert st.nrm == want.nrm
    if which == "middle" and not precond:
        assert want.fired == (3, 5)
    if tight:
        assert (want.converged, want.restarts, want.iters) == (False, 3, 1)


# ------------------------------------------------------------------ 2. a guard that never fires changes nothing
@pytest.mark.parametrize("system", ["mat900", "diagonal"])
def test_a_guard_that_never_fires_changes_nothing(cm, ctx, sw, oracle, golden_dir, system):
    """the default of 4 ulp on well-behaved systems: x, history and iters are those of the same solve without the flag in the
    five-launch loop (FUSED = 0, RESIDENT = 0), bit for bit; no restart of either kind; and the iterate is what it claims"""
    import test_guard_cpu as G
    import test_loop_rounding as L
    if system == "mat900":
        A = oracle.mtx_load(os.path.join(golden_dir, "mat900.mtx"))
        b, x0, tol = oracle.spmv(A, 1.0 + np.sin(np.arange(A.n))), np.zeros(A.n), 1e-8
    else:
        a, b, x0 = L.system(2)
        A, tol = oracle.Csr(L.N, np.arange(L.N + 1, dtype=np.int32), np.arange(L.N, dtype=np.int32), a.copy(), L.N), G.TOL
    sw("FUSED", 0)
    sw("RESIDENT", 0)
    s = cm.Solver.from_host_csr(ctx, A.rowptr, A.colidx, A.val)
    try:
        st0, xa, ha = _solve(cm, ctx, s, b, x0, loop=cm.LOOP_PBICGSTAB, maxit=2000, tol=tol)
        st1, xb, hb = _solve(cm, ctx, s, b, x0, loop=cm.LOOP_PBICGSTAB, maxit=2000, tol=tol, flags=cm.FLAG_GUARD)
    finally:
        s.close()
    assert (st0.converged, st0.loop_form, st0.rho_restarts, st0.restarts) == (1, 0, 0, 0)
    assert (st1.converged, st1.loop_form, st1.rho_restarts, st1.restarts, st1.breakdown) == (1, 0, 0, 0, 0)
    assert (st1.iters, st1.half_exit, st1.nrm0) == (st0.iters, st0.half_exit, st0.nrm0) and st1.iters >= 3
    np.testing.assert_array_equal(hb, ha)
    np.testing.assert_array_equal(xb, xa)
    res = float(np.linalg.norm(b - oracle.spmv(A, xb)))
    print(system, "iters", st1.iters, "true residual / (tol nrm0)", res / (tol * st1.nrm0), "verified nrm / (tol nrm0)", st1.nrm / (tol * st1.nrm0))
    assert res <= 2.5 * tol * st1.nrm0          # (the margin of test_gpu_parity.py for the same check)


# ------------------------------------------------------------------ 3. rho exactly 0
def _zero_system(cm, ctx):
    import test_guard_cpu as G
    return cm.Solver.from_host_csr(ctx, G.ZERO_A.rp, G.ZERO_A.ci, G.ZERO_A.val), G.ZERO_B, G.ZERO_X


def _assert_zero_solved(st, x, want):
    assert (st.converged, st.rho_restarts, st.breakdown, st.restarts, st.iters) == (1, 1, 0, 0, 2)
    np.testing.assert_array_equal(x, want)
    assert st.nrm == 0.0


@pytest.mark.parametrize("how", ["flag", "switch"])
def test_rho_exactly_zero_restarts_once_and_solves(cm, ctx, sw, how):
    """A = [[2, -2, 1], [2, 2, -2], [0, 0, 1]], b = (0, 0, 2), x0 = 0: rho of iteration 1 is exactly 0 with r = (1, 3, 0), every
    intermediate a small dyadic number (test_guard_cpu.py).  Unguarded the solve ends in NaNs and breakdown = 1; guarded -- by
    the flag, or by the switch GUARD without the flag -- it restarts once and returns x = (1/2, 3/2, 2) exactly."""
    s, b, want = _zero_system(cm, ctx)
    try:
        st, x, h = _solve(cm, ctx, s, b, np.zeros(3), maxit=50, tol=1e-8)
        assert (st.converged, st.breakdown, st.rho_restarts) == (0, 1, 0)
        if how == "switch":
            sw("GUARD", 1)
        st, x, h = _solve(cm, ctx, s, b, np.zeros(3), maxit=50, tol=1e-8, flags=cm.FLAG_GUARD if how == "flag" else 0)
    finally:
        s.close()
    _assert_zero_solved(st, x, want)
    assert len(h) == 5 and h[-1] == 0.0 and st.half_exit == 1 and st.loop_form == 0


def test_rho_exactly_zero_through_solve_many(cm, ctx, sw):
    """two copies of that right-hand side through solve_many with the flag: column by column (form 0), each a guarded solve"""
    s, b, want = _zero_system(cm, ctx)
    dB, dX = ctx.array(np.concatenate([b, b])), ctx.array(np.zeros(6))
    try:
        sts, form = s.solve_many(2, dB, 3, dX, 3, maxit=50, tol=1e-8, flags=cm.FLAG_GUARD)
        X = dX.download().reshape(2, 3)
    finally:
        dB.free()
        dX.free()
        s.close()
    assert form == 0
    for j in range(2):
        _assert_zero_solved(sts[j], X[j], want)


# ------------------------------------------------------------------ 4. non-dominant systems
# MAXIT, TOL: the reference CLI's constants.  What is asserted beyond the flags' meaning is decided on the CPU over b and its six
# perturbations (test_guard_cpu.py: ND_RESTARTS, ND_CONVERGES and the test that keeps them honest): both systems converge in all
# seven runs of the numpy restatement, so converged = 1 is asserted on both; a restart is asserted on convdiff_g8 only -- on
# convdiff_g2 rho grazes the 4-ulp threshold (the oracle's smallest |rho| / (eps sum) is 1.1 .. 12.8 over the seven runs), and
# whether a run dips below it is a matter of its rounding.  Iteration counts are never pinned.
from test_guard_cpu import ND_CONVERGES, ND_MAXIT as MAXIT, ND_RESTARTS, ND_TOL as TOL  # noqa: E402


def _nd_run(cm, ctx, A, b, precond):
    s = cm.Solver.from_host_csr(ctx, A.rowptr, A.colidx, A.val)
    db, dx = ctx.array(b), ctx.array(np.ones(A.n))
    try:
        if precond:
            s.ilu0()
        st = s.solve(db, dx, precond=precond, loop=cm.LOOP_PBICGSTAB, maxit=MAXIT, tol=TOL, flags=cm.FLAG_GUARD)
        return st, dx.download()
    finally:
        db.free()
        dx.free()
        s.close()


@pytest.mark.parametrize("name", ["convdiff_g2", "convdiff_g8"])
def test_guarded_solves_of_nondominant_systems(cm, ctx, oracle, name):
    """convection-dominated stencils on which the unguarded loop loses rho, M = I, tol 1e-6, maxit 2000, flag set:
    x finite, no breakdown, converged = 1 backed by the true residual, converged = 0 only at maxit; a restart / convergence is
    asserted only where the CPU restatements restart / converge for b and its six perturbations (the tables above).
    Seen on an MI355X: convdiff_g2 converges in 312 iterations without a restart, convdiff_g8
    in 1093 iterations with 23 restarts, true residuals 0.74 and 0.85 of tol ||r0||."""
    A, b = ND.FAMILY[name](oracle)
    st, x = _nd_run(cm, ctx, A, b, cm.PRECOND_NONE)
    res = ND.true_res(oracle, A, b, x)
    print(name, "iters", st.iters, "converged", st.converged, "rho_restarts", st.rho_restarts, "restarts", st.restarts, "breakdown", st.breakdown,
          "true residual / (tol nrm0)", res / (TOL * st.nrm0))
    assert np.all(np.isfinite(x))
    assert st.breakdown == 0
    if st.converged:
        assert res <= 2.5 * TOL * st.nrm0
    else:
        assert st.iters == MAXIT
    if ND_RESTARTS[name]:
        assert st.rho_restarts >= 1
    if ND_CONVERGES[name]:
        assert st.converged == 1


def test_ilu0_no_longer_reports_a_convergence_it_has_not_reached(cm, ctx, oracle):
    """convdiff_g8 with ILU(0): the recursive residual leaves the true one, and the unguarded loop 'converges' at a true residual
    of 1e5.  With the flag the solve may end either way, but never with converged = 1 at a true residual above
    2.5 tol ||r0||."""
    A, b = ND.FAMILY["convdiff_g8"](oracle)
    st, x = _nd_run(cm, ctx, A, b, cm.PRECOND_ILU0)
    res = ND.true_res(oracle, A, b, x)
    print("convdiff_g8 ILU(0): iters", st.iters, "converged", st.converged, "rho_restarts", st.rho_restarts, "restarts", st.restarts,
          "breakdown", st.breakdown, "true residual / (tol nrm0)", res / (TOL * st.nrm0))
    assert not (st.converged and not res <= 2.5 * TOL * st.nrm0)


# ------------------------------------------------------------------ 5. refusals
def test_what_the_mode_refuses(cm, ctx, sw):
    """FLAG_GUARD with CUDAMAT_LOOP_PIPELINED (which verifies its iterates itself) and on a sharded solver (FORCE_SHARDED = 1 keeps
    the collective path at world size 1) are CUDAMAT_ERR_ARG with a message that says so; with FLAG_NO_EXIT the guarded kernels
    run and the test is never taken, even at 2^52 ulp"""
    import test_guard_cpu as G
    import test_loop_rounding as L
    a, b, x0 = L.system(2)
    s = cm.Solver.from_host_csr(ctx, np.arange(L.N + 1), np.arange(L.N), a)
    try:
        with pytest.raises(cm.CudamatError) as e:
            _solve(cm, ctx, s, b, x0, loop=cm.LOOP_PIPELINED, maxit=5, tol=1e-8, flags=cm.FLAG_GUARD)
        assert e.value.code == 2 and "CUDAMAT_LOOP_PIPELINED" in str(e.value) and "CUDAMAT_FLAG_GUARD" in str(e.value)
        sw("GUARD_RHO_ULPS", G.ULPS_MAX)
        st, x, h = _solve(cm, ctx, s, b, x0, maxit=5, tol=1e-8, flags=cm.FLAG_GUARD | cm.FLAG_NO_EXIT)
        assert (st.iters, st.rho_restarts, st.restarts, st.loop_form) == (5, 0, 0, 0) and len(h) == 10
        # ... and the guarded kernels compute what the five-launch loop computes without the flag, bit for bit
        sw("FUSED", 0)
        sw("RESIDENT", 0)
        st2, x2, h2 = _solve(cm, ctx, s, b, x0, maxit=5, tol=1e-8, flags=cm.FLAG_NO_EXIT)
    finally:
        s.close()
    assert (st2.iters, st2.loop_form) == (5, 0)
    np.testing.assert_array_equal(x, x2)
    np.testing.assert_array_equal(h, h2)
    sw("FORCE_SHARDED", 1)
    comm = cm.Comm()
    cm._lib.check(cm.lib().cudamat_comm_dry_create(ctx.h, 0, 1, C.byref(comm)))
    s = cm.Solver.from_host_csr(ctx, np.arange(L.N + 1), np.arange(L.N), a)
    try:
        s.set_comm(comm)
        with pytest.raises(cm.CudamatError) as e:
            _solve(cm, ctx, s, b, x0, maxit=5, tol=1e-8, flags=cm.FLAG_GUARD)
        assert e.value.code == 2 and "sharded" in str(e.value) and "CUDAMAT_FLAG_GUARD" in str(e.value)
    finally:
        s.close()
        cm.lib().cudamat_comm_dry_destroy(C.byref(comm))
