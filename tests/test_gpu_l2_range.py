"""CUDAMAT_LOOP_BICGSTAB_L2 under the range contract of DESIGN.md section 4 (GPU): the tests of tests/test_gpu_scaling.py and
tests/test_gpu_cg_forms.py (d, e) with this loop, on mat900, with M = I and with ILU(0).

In range the loop is exactly equivariant under c = 2^k.  (c b, c x0) multiplies every vector by c and every dot by c^2; alpha, beta
and (g1, g2) keep their bits, because the 2 x 2 system of the minimal-residual step is solved by elimination (step_l2_mr,
csrc/steps.h) and no intermediate carries a higher power of c than the dots do.  (c A, b, x0 / c) leaves r0 alone, multiplies r1
and the u_j by powers of c, and the largest scalar is the pivot t ~ c^4.  By Cramer's rule det ~ c^4 resp. c^6 left the range of a
double at k = +-440 resp. +-200 and k_l2_mr reported a breakdown the mathematics does not have: every test here but the
refusals and the fixed-sweep runs fails on that form (tests/test_l2_rounding.py shows both on the CPU).  Out of range the loop is
refused by k_init_finish as every loop is."""
import math
import os

import numpy as np
import pytest

from tests.test_gpu_scaling import EXPONENTS, MAT_EXPONENTS, _bits, _columns, _many, _scaled_matrix, _summary

pytestmark = pytest.mark.gpu

TOL, MAXIT = 1e-8, 2000


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
    """a library switch for the rest of this test, on the shared context and in the environment"""
    def _sw(name, value):
        monkeypatch.setenv("CUDAMAT_" + name, str(value))
        ctx.set_option(name, value)
    yield _sw
    monkeypatch.undo()
    ctx.reset_options()


@pytest.fixture(scope="module")
def mat900(oracle, golden_dir):
    """(A, b = A (1 + sin i)): built once, read-only"""
    A = oracle.mtx_load(os.path.join(golden_dir, "mat900.mtx"))
    b = oracle.spmv(A, 1.0 + np.sin(np.arange(A.n)))
    b.setflags(write=False)
    return A, b


def _solver(cm, ctx, A, precond):
    s = cm.Solver.from_host_csr(ctx, A.rowptr, A.colidx, A.val)
    if precond:
        s.ilu0()
    return s


def _solve(ctx, s, b, x0, **kw):
    db, dx = ctx.array(b), ctx.array(x0)
    try:
        st = s.solve(db, dx, **kw)
        return dx.download(), st, s.history()
    finally:
        db.free()
        dx.free()


def _kw(cm, precond, **more):
    return dict(dict(loop=cm.LOOP_BICGSTAB_L2, precond=cm.PRECOND_ILU0 if precond else cm.PRECOND_NONE, maxit=MAXIT, tol=TOL), **more)


def test_the_exponents_are_the_contracts(cm):
    import test_l2_rounding as T
    assert T.EXPONENTS == EXPONENTS and T.MAT_EXPONENTS == MAT_EXPONENTS


@pytest.mark.parametrize("precond", [0, 1], ids=["plain", "ilu0"])
def test_rhs_scaling_is_bitwise(cm, ctx, mat900, sw, precond):
    """one Solver: (c b, c x0) gives c x, c times the history and c ||r0|| bit for bit, with the same sweeps and exit, at every
    exponent of EXPONENTS, solved to 1e-8"""
    sw("SPMV_MODE", "csr")
    A, b = mat900
    kw = _kw(cm, precond)
    s = _solver(cm, ctx, A, precond)
    try:
        x0 = np.ones(A.n)
        x, st, h = _solve(ctx, s, b, x0, **kw)
        assert st.converged and st.iters > 0 and not st.breakdown and st.loop_form == 0, _summary(st)
        assert len(h) == st.iters and np.isfinite(h).all() and np.isfinite(x).all()
        for k in EXPONENTS:
            c = 2.0 ** k
            xc, stc, hc = _solve(ctx, s, c * b, c * x0, **kw)
            print("precond", precond, "k", k, _summary(stc), "nrm", stc.nrm, "unscaled", _summary(st), "nrm", st.nrm)
            assert _summary(stc) == _summary(st), (precond, k)
            assert stc.nrm0 == c * st.nrm0, (precond, k)
            np.testing.assert_array_equal(_bits(hc), _bits(c * h), err_msg="history, precond %d, k = %d" % (precond, k))
            np.testing.assert_array_equal(_bits(xc), _bits(c * x), err_msg="x, precond %d, k = %d" % (precond, k))
    finally:
        s.close()


@pytest.mark.parametrize("precond", [0, 1], ids=["plain", "ilu0"])
def test_matrix_scaling_is_bitwise(cm, ctx, oracle, mat900, sw, precond):
    """(2^k A, b, 2^-k x0) at MAT_EXPONENTS: x is 2^-k times the unscaled x and the history is the same, bit for bit.  Two solvers, so
    the plan is pinned (SPMV_MODE, SPMV_LANES, TRSV_LANES, TRSV_LDS)."""
    sw("SPMV_MODE", "csr")
    sw("SPMV_LANES", 4)
    sw("TRSV_LANES", 4)
    sw("TRSV_LDS", 0)
    A, b = mat900
    kw = _kw(cm, precond)
    x0 = np.ones(A.n)
    s = _solver(cm, ctx, A, precond)
    try:
        x, st, h = _solve(ctx, s, b, x0, **kw)
        assert st.converged and not st.breakdown and s.spmv_kernel() == "k_spmv<4>", (_summary(st), s.spmv_kernel())
    finally:
        s.close()
    for k in MAT_EXPONENTS:
        c = 2.0 ** k
        sc = _solver(cm, ctx, _scaled_matrix(oracle, A, c), precond)
        try:
            xc, stc, hc = _solve(ctx, sc, b, x0 / c, **kw)
            print("precond", precond, "k", k, _summary(stc), "unscaled", _summary(st))
            assert _summary(stc) == _summary(st) and stc.nrm0 == st.nrm0, (precond, k)
            np.testing.assert_array_equal(_bits(hc), _bits(h), err_msg="history, precond %d, k = %d" % (precond, k))
            np.testing.assert_array_equal(_bits(xc), _bits(x / c), err_msg="x, precond %d, k = %d" % (precond, k))
        finally:
            sc.close()


@pytest.mark.parametrize("precond", [0, 1], ids=["plain", "ilu0"])
def test_out_of_range_solves_are_refused(cm, ctx, mat900, sw, precond):
    """x0 = c, b c, tol 1e-8.  k = +520: ||r0|| = inf.  k = -600: every r0^2 is 0 although r0 is not.  k = -520: tol ||r0|| is far
    below 2^-485.  Each returns at once: no sweep, not converged, breakdown, x bitwise x0, an empty history; the same solver then
    solves the in-range system to the bits it gave before."""
    sw("SPMV_MODE", "csr")
    A, b = mat900
    kw = _kw(cm, precond)
    s = _solver(cm, ctx, A, precond)
    try:
        x, st, h = _solve(ctx, s, b, np.ones(A.n), **kw)
        assert st.converged and not st.breakdown
        for k in (520, -600, -520):
            c = 2.0 ** k
            x0 = np.full(A.n, c)
            xc, stc, hc = _solve(ctx, s, c * b, x0, **kw)
            print(precond, k, _summary(stc), stc.nrm0, len(hc))
            assert (stc.iters, bool(stc.converged), bool(stc.breakdown)) == (0, False, True), (precond, k, _summary(stc))
            np.testing.assert_array_equal(_bits(xc), _bits(x0))
            assert len(hc) == 0
            if k == 520:
                assert stc.nrm0 == math.inf
            elif k == -600:
                assert stc.nrm0 == 0.0
        x2, st2, h2 = _solve(ctx, s, b, np.ones(A.n), **kw)
        assert _summary(st2) == _summary(st)
        np.testing.assert_array_equal(_bits(h2), _bits(h))
        np.testing.assert_array_equal(_bits(x2), _bits(x))
    finally:
        s.close()


@pytest.mark.parametrize("precond", [0, 1], ids=["plain", "ilu0"])
def test_exact_initial_guess_returns_at_once_at_2_pow_minus_600(cm, ctx, oracle, precond):
    """the twin of test_gpu_scaling's test of that name: r0 == 0 exactly at c = 2^-600 is 'x0 solves the system' -- converged at
    once -- and not the underflow of a non-zero r0"""
    A = oracle.rand_rows(500, 10, 3)
    c = 2.0 ** -600
    b = c * oracle.spmv(A, np.ones(A.n))
    x0 = np.full(A.n, c)
    s = _solver(cm, ctx, A, precond)
    try:
        x, st, h = _solve(ctx, s, b, x0, **_kw(cm, precond, maxit=50))
    finally:
        s.close()
    assert st.converged and st.iters == 0 and not st.breakdown and st.nrm0 == 0.0 and len(h) == 0
    np.testing.assert_array_equal(_bits(x), _bits(x0))


@pytest.mark.parametrize("precond", [0, 1], ids=["plain", "ilu0"])
def test_fixed_sweep_runs_are_not_refused(cm, ctx, mat900, precond):
    """FLAG_NO_EXIT: no stopping test applies, so nothing is refused -- 5 sweeps at 2^520 and at 2^-520.  Without M^-1 the five
    sweeps at 2^-520 stay in finite arithmetic and the iterate moves.  With ILU(0) five sweeps are a whole solve of mat900
    (||r0|| falls by 4e-9): at 2^-520 the squares of such a residual (2^-1100) are 0, the loop divides 0 by 0 as FLAG_NO_EXIT says
    it will, and only "not refused" is asserted."""
    A, b = mat900
    s = _solver(cm, ctx, A, precond)
    try:
        for k in (520, -520):
            c = 2.0 ** k
            x0 = np.full(A.n, c)
            x, st, h = _solve(ctx, s, c * b, x0, **_kw(cm, precond, maxit=5, flags=cm.FLAG_NO_EXIT))
            assert st.iters == 5 and len(h) == 5 and not st.breakdown and not st.converged, (k, _summary(st))
            if k == -520 and not precond:  # (finite arithmetic all the way: the iterate moved)
                assert np.isfinite(x).all() and np.any(x != x0)
    finally:
        s.close()


@pytest.mark.parametrize("precond", [0, 1], ids=["plain", "ilu0"])
def test_a_solve_many_column_at_2_pow_440_equals_its_single_solve(cm, ctx, oracle, mat900, sw, precond):
    """solve_many runs this loop column by column: a column scaled by 2^440 beside one at 2^0 is bitwise its single solve, which is
    bitwise 2^440 times the unscaled column's"""
    sw("SPMV_MODE", "csr")
    A, _ = mat900
    kw = _kw(cm, precond)
    C = 2.0 ** np.array([440, 0])
    B = _columns(oracle, A, 2)
    X0 = np.ones((A.n, 2))
    s = _solver(cm, ctx, A, precond)
    try:
        X, sts, hs, form = _many(ctx, s, B * C, X0 * C, **kw)
        assert form == 0
        for j in range(2):
            xj, stj, hj = _solve(ctx, s, B[:, j] * C[j], X0[:, j] * C[j], **kw)
            assert sts[j].converged and sts[j].iters > 0 and not sts[j].breakdown, (j, _summary(sts[j]))
            assert _summary(sts[j]) == _summary(stj) and sts[j].nrm0 == stj.nrm0, j
            np.testing.assert_array_equal(_bits(hs[j]), _bits(hj), err_msg="history of column %d" % j)
            np.testing.assert_array_equal(_bits(X[:, j]), _bits(xj), err_msg="column %d" % j)
        x0u, st0u, h0u = _solve(ctx, s, B[:, 0], X0[:, 0], **kw)
        assert _summary(sts[0]) == _summary(st0u)
        np.testing.assert_array_equal(_bits(hs[0]), _bits(C[0] * h0u))
        np.testing.assert_array_equal(_bits(X[:, 0]), _bits(C[0] * x0u))
    finally:
        s.close()
