"""CUDAMAT_LOOP_BICGSTAB_L2 on the GPU against its CPU mirror (tests/test_l2_rounding.py), bit for bit: x, the residual history
and ||r0|| of the kernels of csrc/bicgstab_l2.hip, of k_init / k_l2_start, and of the SpMV's fused dots with w = r~ and w = r1, on
the two plans the mirror restates -- lanes per row (SPMV_LANES = 64) on the diagonal system, stream tiles on the banded one.
What each comparison can tell apart is checked there, without a GPU (test_the_l2_mirror_tells_its_neighbours_apart): the u, r and
y steps in two roundings, the two-term updates with their terms swapped or in three roundings, beta as alpha (rho1 / rho0), the
2 x 2 solve with plain products or by Cramer's rule, the dot terms in two roundings, an omega taken one sweep late, row sums as
fma chains, the shift in two roundings, M^-1 as a division."""
import numpy as np
import pytest

from tests.test_gpu_parity import _LOOP_SWITCHES

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
    """set (value) or unset (None) a library switch for the rest of this test, on the module's context and in the environment;
    afterwards the context is back to what the environment outside the test says"""
    def _sw(name, value):
        if value is None:
            monkeypatch.delenv("CUDAMAT_" + name, raising=False)
            ctx.reset_options()
        else:
            monkeypatch.setenv("CUDAMAT_" + name, str(value))
            ctx.set_option(name, value)
    yield _sw
    monkeypatch.undo()
    ctx.reset_options()


def _solver(cm, ctx, sw, which, A, d=None):
    """a solver on A (a diagonal as a vector, or test_loop_rounding.Csr) on the plan the mirror restates for it"""
    import test_loop_rounding as L
    lanes = _LOOP_SWITCHES["five/lanes" if which == "diagonal" else "five/stream"][0]
    assert lanes == (64 if which == "diagonal" else None)
    sw("SPMV_MODE", "csr")
    sw("SPMV_LANES", lanes)
    if isinstance(A, L.Csr):
        s = cm.Solver.from_host_csr(ctx, A.rp, A.ci, A.val)
    else:
        s = cm.Solver.from_host_csr(ctx, np.arange(len(A) + 1), np.arange(len(A)), A)
    assert s.spmv_kernel().startswith("k_spmv<64>" if lanes else "k_spmv_stream"), (which, s.spmv_kernel())
    if d is not None:
        s.set_shift(ctx.array(d))
    return s


def _solve(cm, ctx, s, b, x0, off=0, **kw):
    """(stats, x, history); b and x start `off` doubles past a 16-byte boundary"""
    db, dx = ctx.array(np.concatenate([np.zeros(off), b])), ctx.array(np.concatenate([np.zeros(off), x0]))
    try:
        st = s.solve(db.ptr + 8 * off, dx.ptr + 8 * off, loop=cm.LOOP_BICGSTAB_L2, **kw)
        return st, dx.download()[off:], s.history()
    finally:
        db.free()
        dx.free()


def _assert_bits(tag, got, want, iters, breakdown=False):
    import test_loop_rounding as L
    (st, x, h), (want_x, want_h) = got, want
    print(tag, "entries of x that differ:", L.differing(x, want_x), "of", len(x), "residuals:",
          L.differing(h, want_h) if len(h) == len(want_h) else (len(h), len(want_h)), h, want_h)
    assert (st.loop_form, st.iters, bool(st.breakdown), bool(st.half_exit)) == (0, iters, breakdown, False)
    np.testing.assert_array_equal(h, want_h)
    np.testing.assert_array_equal(x, want_x)


@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "offset8"])
@pytest.mark.parametrize("iters", [3, 4])
@pytest.mark.parametrize("which", ["diagonal", "banded"])
def test_l2_bits(cm, ctx, sw, which, iters, off):
    """3 and 4 sweeps with FLAG_NO_EXIT, lanes per row on the diagonal system and stream tiles on the banded one: x, the history
    and ||r0|| equal the mirror bit for bit -- with b and x 16-byte aligned and with both 8 bytes off, which has the aligned
    solve's mirror (pair_loop; the start sums formed again by k_l2_start) and the aligned run's bits on the same solver"""
    import test_l2_rounding as T
    A, b, x0, _ = T.inputs(which)
    s = _solver(cm, ctx, sw, which, A)
    try:
        got = _solve(cm, ctx, s, b, x0, off=off, maxit=iters, tol=1e-8, flags=cm.FLAG_NO_EXIT)
        if off:
            sta, xa, ha = _solve(cm, ctx, s, b, x0, maxit=iters, tol=1e-8, flags=cm.FLAG_NO_EXIT)
            assert (sta.iters, sta.nrm0, sta.nrm) == (got[0].iters, got[0].nrm0, got[0].nrm)
            np.testing.assert_array_equal(got[2], ha)
            np.testing.assert_array_equal(got[1], xa)
    finally:
        s.close()
    _assert_bits("%s %d off %d:" % (which, iters, off), got, T.pinned(which, iters=iters), iters)
    assert got[0].nrm0 == T.loop(A, b, x0, iters=0).nrm0 and not got[0].converged


@pytest.mark.parametrize("iters", [3, 4])
def test_l2_bits_shifted(cm, ctx, sw, iters):
    """the banded system with set_shift(d): fma(d_i, x_i, sum) after the row sum, in r0 and in all four products of a sweep"""
    import test_l2_rounding as T
    A, b, x0, d = T.inputs("banded", shifted=True)
    s = _solver(cm, ctx, sw, "banded", A, d)
    try:
        got = _solve(cm, ctx, s, b, x0, maxit=iters, tol=1e-8, flags=cm.FLAG_NO_EXIT)
    finally:
        s.close()
    _assert_bits("banded shifted %d:" % iters, got, T.pinned("banded", shifted=True, iters=iters), iters)


def test_l2_bits_ilu0(cm, ctx, sw):
    """the diagonal system with ILU(0) (L = I, U = diag(a)): the factors are a itself and one application is rhs fl(1 / a_i)
    bitwise; A^ = A M^-1 in all four products, y from 0, x = x0 + M^-1 y in finish().  tol = 0: every stopping and breakdown test
    is taken and no residual passes.  As decided on the CPU (test_l2_rounding.test_ilu0_sweeps_and_breakdown): maxit = ILU_SWEEPS
    completes them without a breakdown; maxit = ILU_SWEEPS + 1 breaks down in the next sweep's k_l2_mr -- breakdown = 1,
    iters = ILU_SWEEPS, the same history, and x = x0 + M^-1 y with the y k_l2_step0 and k_l2_step1 of the interrupted sweep left
    (which on this system moves no entry of x any more: the mirror's two x are equal, and each is compared on its own)"""
    import test_loop_rounding as L
    import test_l2_rounding as T
    a, b, x0, _ = T.inputs("diagonal", precond=True)
    s = _solver(cm, ctx, sw, "diagonal", a)
    try:
        s.ilu0()
        np.testing.assert_array_equal(s.ilu0_values(), a)
        dr, do = ctx.array(b), ctx.empty(L.N)
        s.precond_apply(dr, do)
        np.testing.assert_array_equal(do.download(), b * (1.0 / a))
        dr.free()
        do.free()
        assert L.differing(b * (1.0 / a), b / a) >= L.MIN_DIFFERING_ROWS
        runs = [_solve(cm, ctx, s, b, x0, precond=cm.PRECOND_ILU0, maxit=maxit, tol=0.0) for maxit in (T.ILU_SWEEPS, T.ILU_SWEEPS + 1)]
    finally:
        s.close()
    for got, maxit in zip(runs, (T.ILU_SWEEPS, T.ILU_SWEEPS + 1)):
        want = T.ilu0_run(maxit=maxit)
        assert (want.iters, want.breakdown) == (T.ILU_SWEEPS, maxit > T.ILU_SWEEPS) and not got[0].converged
        _assert_bits("ILU(0) maxit %d:" % maxit, got, (want.x, want.history), T.ILU_SWEEPS, breakdown=want.breakdown)
        assert got[0].nrm0 == want.nrm0


def test_l2_bits_exit(cm, ctx, sw):
    """the banded system solved to TOL_EXIT leaves after EXIT_SWEEPS sweeps (the deciding residual >= 1 % off the tolerance:
    test_the_exit_case_ends_where_intended): converged, the sweeps, x and the history equal the mirror's"""
    import test_l2_rounding as T
    A, b, x0, _ = T.inputs("banded")
    want = T.pinned_exit()
    s = _solver(cm, ctx, sw, "banded", A)
    try:
        got = _solve(cm, ctx, s, b, x0, maxit=20, tol=T.TOL_EXIT)
    finally:
        s.close()
    st, x, h = got
    assert bool(st.converged) and want.converged and st.iters == want.iters == T.EXIT_SWEEPS
    _assert_bits("exit:", got, (want.x, want.history), want.iters)
    assert len(h) == st.iters and st.nrm0 == want.nrm0
    assert h[-1] < T.TOL_EXIT * st.nrm0 <= min(h[:-1])


@pytest.mark.parametrize("which", ["diagonal", "banded"])
def test_l2_bits_second_solve_on_one_solver(cm, ctx, sw, which):
    """one solver, a solve of 3 sweeps and then one of 4 from a fresh copy of the same x0: nothing of L2State leaks into the
    second solve -- each equals its mirror bit for bit"""
    import test_l2_rounding as T
    A, b, x0, _ = T.inputs(which)
    s = _solver(cm, ctx, sw, which, A)
    try:
        for iters in (3, 4):
            got = _solve(cm, ctx, s, b, x0, maxit=iters, tol=1e-8, flags=cm.FLAG_NO_EXIT)
            _assert_bits("%s, solve of %d sweeps:" % (which, iters), got, T.pinned(which, iters=iters), iters)
    finally:
        s.close()


def test_l2_bits_second_solve_with_ilu0(cm, ctx, sw):
    """the same with ILU(0) on the diagonal system, where y and the two other extra vectors are the solver's own: the breakdown run
    and then the complete-sweeps run, each equal to its mirror -- nothing of l2_y stays from the first"""
    import test_l2_rounding as T
    a, b, x0, _ = T.inputs("diagonal", precond=True)
    s = _solver(cm, ctx, sw, "diagonal", a)
    try:
        s.ilu0()
        for maxit in (T.ILU_SWEEPS + 1, T.ILU_SWEEPS):
            got = _solve(cm, ctx, s, b, x0, precond=cm.PRECOND_ILU0, maxit=maxit, tol=0.0)
            want = T.ilu0_run(maxit=maxit)
            _assert_bits("ILU(0), maxit %d on one solver:" % maxit, got, (want.x, want.history), T.ILU_SWEEPS, breakdown=want.breakdown)
    finally:
        s.close()
