"""CUDAMAT_LOOP_CG on the GPU against its CPU mirror (tests/test_cg_rounding.py), bit for bit: x, the residual history and
||r0|| of the kernels of csrc/cg.hip, of k_init / k_l2_start, and of the SpMV's fused dot p.q with the epilogue operand equal to the
SpMV's x, on the two plans the mirror restates -- lanes per row (SPMV_LANES = 64) on the diagonal system, stream tiles on the
symmetric banded one.  What each comparison can tell apart is checked there, without a GPU
(test_the_cg_mirror_tells_its_neighbours_apart): the p-update, the x and r steps and the dot terms in two roundings, beta from the
wrong slot of the rho ring, row sums as fma chains, the shift in two roundings, M^-1 as a division."""
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
    if isinstance(A, L.Csr):
        assert s.symmetry() == (0, 0.0)
    if d is not None:
        s.set_shift(ctx.array(d))
    return s


def _solve(cm, ctx, s, b, x0, off=0, **kw):
    """(stats, x, history); b and x start `off` doubles past a 16-byte boundary"""
    db, dx = ctx.array(np.concatenate([np.zeros(off), b])), ctx.array(np.concatenate([np.zeros(off), x0]))
    try:
        st = s.solve(db.ptr + 8 * off, dx.ptr + 8 * off, loop=cm.LOOP_CG, **kw)
        return st, dx.download()[off:], s.history()
    finally:
        db.free()
        dx.free()


def _assert_bits(tag, got, want, iters):
    import test_loop_rounding as L
    (st, x, h), (want_x, want_h) = got, want
    print(tag, "entries of x that differ:", L.differing(x, want_x), "of", len(x), "residuals:",
          L.differing(h, want_h) if len(h) == len(want_h) else (len(h), len(want_h)), h, want_h)
    assert (st.loop_form, st.iters, bool(st.breakdown), bool(st.half_exit)) == (0, iters, False, False)
    np.testing.assert_array_equal(h, want_h)
    np.testing.assert_array_equal(x, want_x)


@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "offset8"])
@pytest.mark.parametrize("iters", [3, 4])
@pytest.mark.parametrize("which", ["diagonal", "banded"])
def test_cg_bits(cm, ctx, sw, which, iters, off):
    """3 and 4 iterations with FLAG_NO_EXIT, lanes per row on the diagonal system and stream tiles on the banded one: x, the
    history and ||r0|| equal the mirror bit for bit -- with b and x 16-byte aligned and with both 8 bytes off, which has the
    aligned solve's mirror (pair_loop; the start sums formed again by k_l2_start)"""
    import test_cg_rounding as G
    A, b, x0, _ = G.inputs(which)
    s = _solver(cm, ctx, sw, which, A)
    try:
        got = _solve(cm, ctx, s, b, x0, off=off, maxit=iters, tol=1e-8, flags=cm.FLAG_NO_EXIT)
        if off:                                     # ... and the aligned run's bits, on the same solver
            sta, xa, ha = _solve(cm, ctx, s, b, x0, maxit=iters, tol=1e-8, flags=cm.FLAG_NO_EXIT)
            assert (sta.iters, sta.nrm0, sta.nrm) == (got[0].iters, got[0].nrm0, got[0].nrm)
            np.testing.assert_array_equal(got[2], ha)
            np.testing.assert_array_equal(got[1], xa)
    finally:
        s.close()
    _assert_bits("%s %d off %d:" % (which, iters, off), got, G.pinned(which, iters=iters), iters)
    assert got[0].nrm0 == G.loop(A, b, x0, iters=0).nrm0 and not got[0].converged


@pytest.mark.parametrize("iters", [3, 4])
def test_cg_bits_shifted(cm, ctx, sw, iters):
    """the banded system with set_shift(d): fma(d_i, p_i, sum) after the row sum, in r0 and in every product"""
    import test_cg_rounding as G
    A, b, x0, d = G.inputs("banded", shifted=True)
    s = _solver(cm, ctx, sw, "banded", A, d)
    try:
        got = _solve(cm, ctx, s, b, x0, maxit=iters, tol=1e-8, flags=cm.FLAG_NO_EXIT)
    finally:
        s.close()
    _assert_bits("banded shifted %d:" % iters, got, G.pinned("banded", shifted=True, iters=iters), iters)


@pytest.mark.parametrize("iters", [10, 11])
def test_cg_bits_ilu0(cm, ctx, sw, iters):
    """the diagonal system with ILU(0) (L = I, U = diag(a)): the factors are a itself and one application is rhs fl(1 / a_i) bitwise;
    z = M^-1 r0 and (r.z, r.r) before the loop, then one M^-1 and one k_cg_rz per iteration, for as many iterations as the mirror
    keeps every scalar finite (test_cg_rounding.ILU_ITERS = 11, decided on the CPU) and for one fewer: x and the history, down to
    the sum of squares that underflows to 0, equal the mirror bit for bit"""
    import test_loop_rounding as L
    import test_cg_rounding as G
    assert iters in (G.ILU_ITERS - 1, G.ILU_ITERS)
    a, b, x0, _ = G.inputs("diagonal", precond=True)
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
        got = _solve(cm, ctx, s, b, x0, precond=cm.PRECOND_ILU0, maxit=iters, tol=1e-8, flags=cm.FLAG_NO_EXIT)
    finally:
        s.close()
    _assert_bits("ILU(0) %d:" % iters, got, G.pinned("diagonal", precond=True, iters=iters), iters)


def test_cg_bits_exit(cm, ctx, sw):
    """the banded system solved to TOL_EXIT leaves at iteration 3 (the deciding residual >= 1 % off the tolerance:
    test_the_exit_case_ends_where_intended): converged, the iterations, x and the history equal the mirror's"""
    import test_cg_rounding as G
    A, b, x0, _ = G.inputs("banded")
    want = G.pinned_exit()
    s = _solver(cm, ctx, sw, "banded", A)
    try:
        got = _solve(cm, ctx, s, b, x0, maxit=20, tol=G.TOL_EXIT)
    finally:
        s.close()
    st, x, h = got
    assert bool(st.converged) and want.converged and st.iters == want.iters == 3
    _assert_bits("exit:", got, (want.x, want.history), want.iters)
    assert len(h) == st.iters and st.nrm0 == want.nrm0
    assert h[-1] < G.TOL_EXIT * st.nrm0 <= min(h[:-1])


@pytest.mark.parametrize("which", ["diagonal", "banded"])
def test_cg_bits_second_solve_on_one_solver(cm, ctx, sw, which):
    """one solver, a solve of 3 iterations and then one of 4 from a fresh copy of the same x0: nothing of CgState or of the rho ring
    leaks into the second solve -- each equals its mirror bit for bit"""
    import test_cg_rounding as G
    A, b, x0, _ = G.inputs(which)
    s = _solver(cm, ctx, sw, which, A)
    try:
        for iters in (3, 4):
            got = _solve(cm, ctx, s, b, x0, maxit=iters, tol=1e-8, flags=cm.FLAG_NO_EXIT)
            _assert_bits("%s, solve of %d iterations:" % (which, iters), got, G.pinned(which, iters=iters), iters)
    finally:
        s.close()
