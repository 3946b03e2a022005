"""Several right-hand sides for one resident matrix (cudamat_solver_spmm / cudamat_solver_solve_many / cudamat_solve_many):
the SpMM against the oracle and against the single-vector SpMV, the batched loop against the oracle column by column, the
independence of a column from the batch it is solved in, freeze on exit per column, the (A0 + I d) loop, the column-by-column
fall-back and the host-pointer entry point.  Run on the GPU box with:  python -m pytest tests -m gpu"""
import os

import numpy as np
import pytest

from tests import nondominant as ND

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps


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
    """a library switch for the rest of this test, on the shared context and in the environment (cudamat_solve_many)"""
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


def _load(oracle, golden_dir, name):
    return oracle.mtx_load(os.path.join(golden_dir, name + ".mtx"))


def _block(ctx, M, ld):
    """device copy of the (n, k) array M, column-major with leading dimension ld (the pad rows hold NaN)"""
    n, k = M.shape
    buf = np.full((k, ld), np.nan)
    buf[:, :n] = M.T
    return ctx.array(buf.ravel())


def _unblock(d, n, k, ld):
    return d.download().reshape(k, ld)[:, :n].T.copy()


def _matrix(oracle, golden_dir, name):
    if name == "rand20000x50":
        return oracle.rand_rows(20000, 50, 0x5EED)
    if name == "poisson":
        return oracle.poisson5(120, 90, base=1)
    return _load(oracle, golden_dir, name)


def _solve_many(cm, ctx, A, B, X0=None, d=None, ldb=None, ldx=None, **kw):
    n, k = B.shape
    ldb, ldx = ldb or n, ldx or n
    s = cm.Solver.from_host_csr(ctx, A.rowptr, A.colidx, A.val)
    try:
        if d is not None:
            s.set_shift(ctx.array(d))
        dB = _block(ctx, B, ldb)
        dX = _block(ctx, np.ones((n, k)) if X0 is None else X0, ldx)
        sts, form = s.solve_many(k, dB, ldb, dX, ldx, **kw)
        X = _unblock(dX, n, k, ldx)
        hs = [s.history(col=j) for j in range(k)]
        return X, sts, hs, form
    finally:
        s.close()


def _solve_one(cm, ctx, A, b, x0=None, d=None, precond=0, ilu=False, **kw):
    s = cm.Solver.from_host_csr(ctx, A.rowptr, A.colidx, A.val)
    try:
        if d is not None:
            s.set_shift(ctx.array(d))
        if ilu:
            s.ilu0()
        db, dx = ctx.array(b), ctx.array(np.ones(A.n) if x0 is None else x0)
        st = s.solve(db, dx, precond=precond, **kw)
        return dx.download(), st, s.history()
    finally:
        s.close()


def _xstars(n, k, seed=0):
    """k different solutions: two shapes (1 + sin(i c) plus noise) and their multiples by 2, -1, 1/2, ... (exact in fp64, so a
    multiple takes exactly the iterations of its shape).  mat10000 and the 120 x 90 stencil need 150-190 iterations at 1e-8,
    and on them other shapes move the count of ANY implementation by more than the +-10 % rule allows (two roundings
    of the same x* differ that much)"""
    rng = np.random.default_rng(0)
    i = np.arange(n)
    shapes = [1.0 + np.sin(i * c) + 0.1 * rng.random(n) for c in (1.0, 1.37)]
    scales = (1.0, 1.0, 2.0, -1.0, 0.5, -2.0, 4.0, -0.5, 0.25, -4.0, 8.0)
    rot = seed % 2
    return np.stack([scales[j] * shapes[(j + rot) % 2] for j in range(k)], axis=1)


# ---------------------------------------------------------------------------------------------------------------- SpMM
@pytest.mark.parametrize("name", ["mat3", "mat900", "mat10000", "rand20000x50", "poisson"])
@pytest.mark.parametrize("lanes", [None, 2, 16, 64])
def test_spmm_bit_exact_on_integer_data(cm, ctx, oracle, golden_dir, name, lanes, sw):
    """integer-valued A and X: exact in fp64, so every column equals the oracle's SpMV bit for bit, for every lanes-per-row
    variant, every batch width (nrhs 1..11: groups of 8 with padding), leading dimensions above n, with and without d"""
    if lanes:
        sw("SPMV_LANES", str(lanes))
    A = _matrix(oracle, golden_dir, name)
    rng = np.random.default_rng(3)
    A = oracle.Csr(A.n, A.rowptr, A.colidx, rng.integers(-8, 9, A.nnz).astype(np.float64), A.m)
    d = rng.integers(-3, 4, A.n).astype(np.float64)
    s = cm.Solver.from_host_csr(ctx, A.rowptr, A.colidx, A.val)
    try:
        for shift in (False, True):
            if shift:
                s.set_shift(ctx.array(d))
            for k in (1, 2, 3, 8, 11):
                X = rng.integers(-8, 9, (A.n, k)).astype(np.float64)
                ldx, ldy = A.n + 3, A.n + 5
                dX, dY = _block(ctx, X, ldx), _block(ctx, np.zeros((A.n, k)), ldy)
                s.spmm(k, dX, ldx, dY, ldy)
                Y = dY.download().reshape(k, ldy)
                for j in range(k):
                    want = oracle.spmv(A, X[:, j]) + (d * X[:, j] if shift else 0.0)
                    np.testing.assert_array_equal(Y[j, :A.n], want)
                    assert np.all(np.isnan(Y[j, A.n:]))           # the pad rows of Y are not touched
    finally:
        s.close()


def test_spmm_real_data_tolerance(cm, ctx, oracle):
    """real-valued data: |y - y_ref| <= 4 nnz_row eps sum|a_ij x_j| per column"""
    A = oracle.rand_rows(20000, 50, 3)
    rng = np.random.default_rng(2)
    A.val[:] = rng.standard_normal(A.nnz)
    X = rng.standard_normal((A.n, 5))
    absA = oracle.Csr(A.n, A.rowptr, A.colidx, np.abs(A.val), A.m)
    s = cm.Solver.from_host_csr(ctx, A.rowptr, A.colidx, A.val)
    try:
        dX, dY = _block(ctx, X, A.n), ctx.empty(5 * A.n)
        s.spmm(5, dX, A.n, dY, A.n)
        Y = dY.download().reshape(5, A.n)
    finally:
        s.close()
    for j in range(5):
        bound = 4 * 50 * EPS * oracle.spmv(absA, np.abs(X[:, j]))
        assert np.all(np.abs(Y[j] - oracle.spmv(A, X[:, j])) <= bound)


@pytest.mark.parametrize("lanes", [2, 8, 32])
def test_spmm_column_is_the_single_spmv(cm, ctx, oracle, lanes, sw):
    """SPMV_MODE = csr, SPMV_LANES = L: column j of the SpMM is bit-identical to Solver.spmv of column j (k_spmv<L>), on
    real-valued data with 12 entries per row: every row is summed by its group of L lanes.  (Rows above 4096 entries, which the
    whole workgroup sweeps, are in tests/test_gpu_long_rows.py::test_spmm_sweep_is_the_spmv_sweep.)"""
    sw("SPMV_MODE", "csr")
    sw("SPMV_LANES", str(lanes))
    rng = np.random.default_rng(lanes)
    A = oracle.rand_rows(30000, 12, 7)
    A.val[:] = rng.standard_normal(A.nnz)
    X = rng.standard_normal((A.n, 6))
    d = rng.standard_normal(A.n)
    s = cm.Solver.from_host_csr(ctx, A.rowptr, A.colidx, A.val)
    try:
        s.set_shift(ctx.array(d))
        dX, dY = _block(ctx, X, A.n), ctx.empty(6 * A.n)
        s.spmm(6, dX, A.n, dY, A.n)
        Y = dY.download().reshape(6, A.n)
        for j in range(6):
            dx, dy = ctx.array(X[:, j]), ctx.empty(A.n)
            s.spmv(dx, dy)
            np.testing.assert_array_equal(Y[j], dy.download())
    finally:
        s.close()


# ---------------------------------------------------------------------------------------------------- the batched loop
@pytest.mark.parametrize("name", ["mat900", "mat10000", "rand20000x50", "poisson"])
def test_batched_solve_vs_oracle(cm, ctx, oracle, golden_dir, name, sw):
    """MANY_FORM = batched, 5 columns with different x*: every column against gpu_pbicgstab's restatement with the tolerances
    of test_pbicgstab_no_precond_vs_oracle"""
    sw("MANY_FORM", "batched")
    tol = 1e-8
    A = _matrix(oracle, golden_dir, name)
    XS = _xstars(A.n, 5)
    B = np.stack([oracle.spmv(A, XS[:, j]) for j in range(5)], axis=1)
    X, sts, hs, form = _solve_many(cm, ctx, A, B, ldb=A.n + 7, ldx=A.n + 1, loop=cm.LOOP_PBICGSTAB, maxit=2000, tol=tol)
    assert form == 1
    for j in range(5):
        b, x, st, h = B[:, j], X[:, j], sts[j], hs[j]
        xo, so, ho = oracle.pbicgstab(A, b, maxit=2000, tol=tol, want_hist=True)
        assert st.converged and so.converged, j
        # +-10 % (>= 2) of the oracle's count, or of the counts the oracle itself gives when b moves by a few ulp
        # (tests/nondominant.py, the rule tests/soak.py applies: mat10000 and the stencil amplify rounding at these x*)
        inside, band = ND.iters_inside_oracle_spread(oracle, A, b, 0, None, st.iters, so.iters, 2000, tol)
        assert inside, (j, st.iters, so.iters, band)
        assert np.linalg.norm(x - xo) / np.linalg.norm(xo) <= 1e-5
        assert np.linalg.norm(b - oracle.spmv(A, x)) <= 10 * tol * so.nrm0
        assert abs(st.nrm0 - so.nrm0) <= 1e-12 * so.nrm0
        k = min(len(h), 8)
        np.testing.assert_allclose(h[:k], ho[:k], rtol=1e-9)
        assert len(h) == 2 * st.iters + (1 if st.half_exit else 0)
        assert h[-1] < tol * st.nrm0 and np.all(h[:-1] >= tol * st.nrm0)


def test_column_does_not_depend_on_its_batch(cm, ctx, oracle, golden_dir, sw):
    """bitwise: column j of an 11-column batch = the same column solved alone (nrhs = 1, batched) = the same column in a
    permuted batch; iteration counts and histories too"""
    sw("MANY_FORM", "batched")
    A = _load(oracle, golden_dir, "mat900")
    XS = _xstars(A.n, 11, seed=5)
    B = np.stack([oracle.spmv(A, XS[:, j]) for j in range(11)], axis=1)
    X0 = np.cos(np.arange(A.n))[:, None] * (1.0 + np.arange(11))[None, :]
    kw = dict(loop=cm.LOOP_PBICGSTAB, maxit=2000, tol=1e-9)
    X, sts, hs, form = _solve_many(cm, ctx, A, B, X0=X0, **kw)
    assert form == 1
    perm = np.random.default_rng(0).permutation(11)
    Xp, stp, hp, _ = _solve_many(cm, ctx, A, B[:, perm], X0=X0[:, perm], **kw)
    for q, j in enumerate(perm):
        np.testing.assert_array_equal(Xp[:, q], X[:, j])
        assert stp[q].iters == sts[j].iters
        np.testing.assert_array_equal(hp[q], hs[j])
    for j in (0, 4, 10):
        X1, st1, h1, f1 = _solve_many(cm, ctx, A, B[:, j:j + 1], X0=X0[:, j:j + 1], **kw)
        assert f1 == 1
        np.testing.assert_array_equal(X1[:, 0], X[:, j])
        assert st1[0].iters == sts[j].iters and st1[0].half_exit == sts[j].half_exit
        np.testing.assert_array_equal(h1[0], hs[j])


def test_freeze_and_mixed_exits(cm, ctx, oracle, golden_dir, sw):
    """a column started at the exact solution (iters 0) beside columns that iterate; cutting maxit at the fast column's exit
    leaves that column's x bit-identical, and every column that had stopped by then reports what the uncut run reports"""
    sw("MANY_FORM", "batched")
    A = _load(oracle, golden_dir, "mat900")
    n = A.n
    XS = _xstars(n, 4, seed=9)
    s = cm.Solver.from_host_csr(ctx, A.rowptr, A.colidx, A.val)
    try:
        dXS, dB = _block(ctx, XS, n), ctx.empty(4 * n)
        s.spmm(4, dXS, n, dB, n)                           # b = A x* by the same kernel: x0 = x* leaves r0 = 0 exactly
        B = dB.download().reshape(4, n).T.copy()
    finally:
        s.close()
    X0 = np.ones((n, 4))
    X0[:, 1] = XS[:, 1]
    tols = dict(loop=cm.LOOP_PBICGSTAB, tol=1e-10)
    X, sts, _, _ = _solve_many(cm, ctx, A, B, X0=X0, maxit=2000, **tols)
    assert sts[1].iters == 0 and sts[1].converged and sts[1].nrm0 == 0.0
    np.testing.assert_array_equal(X[:, 1], XS[:, 1])
    # the iterating column that stops first decides the cut
    its = [(sts[j].iters + sts[j].half_exit, j) for j in (0, 2, 3)]
    cut, fast = min(its)
    assert all(sts[j].converged for j in range(4))
    Xc, stc, _, _ = _solve_many(cm, ctx, A, B, X0=X0, maxit=cut, **tols)
    np.testing.assert_array_equal(Xc[:, fast], X[:, fast])
    np.testing.assert_array_equal(Xc[:, 1], X[:, 1])
    for j in range(4):
        if sts[j].iters + sts[j].half_exit <= cut:
            assert (stc[j].iters, stc[j].half_exit, stc[j].converged) == (sts[j].iters, sts[j].half_exit, sts[j].converged)
        else:
            assert not stc[j].converged and stc[j].iters == cut


def test_batched_pbicgstab2_with_shift(cm, ctx, oracle, golden_dir, sw):
    """gpu_pbicgstab2 (pbicgstab.cu:581-754) per column: mat3_A0 + vec3_d with B = [b, 2b, -b], x0 = [1, 2, -1] (scaling by
    2 and -1 is exact: the known answer scaled, 3 iterations each); mat900 with its diagonal split off against the oracle"""
    sw("MANY_FORM", "batched")
    A0 = _load(oracle, golden_dir, "mat3_A0")
    d = oracle.to_dense_vector(_load(oracle, golden_dir, "vec3_d"))
    b = oracle.to_dense_vector(_load(oracle, golden_dir, "vec3"))
    sc = np.array([1.0, 2.0, -1.0])
    X, sts, hs, form = _solve_many(cm, ctx, A0, b[:, None] * sc, X0=np.ones((3, 1)) * sc, d=d,
                                   loop=cm.LOOP_PBICGSTAB2, maxit=2000, tol=1e-5)
    assert form == 1
    for j in range(3):
        assert sts[j].converged and sts[j].iters == 3 and len(hs[j]) == 3
        np.testing.assert_allclose(X[:, j], sc[j] * np.array([7 / 6, 17 / 3, -23 / 6]), rtol=1e-7)
    np.testing.assert_array_equal(X[:, 1], 2 * X[:, 0])
    np.testing.assert_array_equal(X[:, 2], -X[:, 0])

    A = _load(oracle, golden_dir, "mat900")
    S = A.to_scipy().tolil()
    dg = S.diagonal().copy()
    S.setdiag(0)
    S = S.tocsr()
    S.eliminate_zeros()
    S.sort_indices()
    A0 = oracle.Csr(A.n, (S.indptr + 1).astype(np.int32), (S.indices + 1).astype(np.int32), S.data, A.n)
    XS = _xstars(A.n, 3, seed=2)
    B = np.stack([oracle.spmv(A, XS[:, j]) for j in range(3)], axis=1)
    X0 = np.cos(np.arange(A.n))[:, None] * np.array([1.0, 0.5, -2.0])[None, :]
    X, sts, _, _ = _solve_many(cm, ctx, A0, B, X0=X0, d=dg, loop=cm.LOOP_PBICGSTAB2, maxit=2000, tol=1e-8)
    for j in range(3):
        ok, xo, so = oracle.pbicgstab2(A0, B[:, j], d=dg, x0=X0[:, j], tol=1e-8)
        assert ok and sts[j].converged and abs(sts[j].iters - so.iters) <= max(2, 0.1 * so.iters)
        assert np.linalg.norm(X[:, j] - xo) / np.linalg.norm(xo) <= 1e-5
        assert np.linalg.norm(B[:, j] - oracle.spmv(A, X[:, j])) <= 1e-7 * so.nrm0


def _outcome(st):
    return "breakdown" if st.breakdown else "converged" if st.converged else "maxit"


@pytest.mark.parametrize("name", ["convdiff_g2", "weakdiag_t0.3", "example300_p98_seed3"])
def test_batched_loop_on_nondominant_systems(cm, ctx, oracle, name, sw):
    """systems that amplify rounding (tests/nondominant.py), 3 right-hand sides: every batched column holds to the rules
    test_gpu_nondominant.py applies between the GPU's loop and the oracle's (compare_loop); where the oracle's run keeps a
    significant bit in rho throughout (no rho-noise point), the column's outcome class is that of a single solve of it"""
    sw("MANY_FORM", "batched")
    MAXIT, TOL = 2000, 1e-6
    A, b0 = ND.FAMILY[name](oracle)
    B = np.stack([b0, ND.rhs_for(oracle, A, 40), ND.rhs_for(oracle, A, 41)], axis=1)
    X, sts, hs, form = _solve_many(cm, ctx, A, B, loop=cm.LOOP_PBICGSTAB, maxit=MAXIT, tol=TOL)
    assert form == 1
    findings = []
    for j in range(3):
        line, bad, k_nb = ND.compare_loop(oracle, A, B[:, j], 0, None, (X[:, j], sts[j], hs[j]), MAXIT, TOL)
        print(name, j, line)
        findings += ["%s col %d: %s" % (name, j, m) for m in bad]
        _, st1, _ = _solve_one(cm, ctx, A, B[:, j], loop=cm.LOOP_PBICGSTAB, maxit=MAXIT, tol=TOL)
        if k_nb is None or k_nb[0] is None:
            if _outcome(st1) != _outcome(sts[j]):
                findings.append("%s col %d: batched %s, single %s" % (name, j, _outcome(sts[j]), _outcome(st1)))
    assert not findings, "\n".join(findings)


# ------------------------------------------------------------------------------------------------------------ fall-back
def test_fallback_is_the_single_solve(cm, ctx, oracle, golden_dir, sw):
    """ILU(0) through solve_many runs column by column (form 0) and is bitwise the per-column Solver.solve; with
    MANY_FORM = columns so is the plain loop"""
    A = _load(oracle, golden_dir, "mat900")
    XS = _xstars(A.n, 3, seed=4)
    B = np.stack([oracle.spmv(A, XS[:, j]) for j in range(3)], axis=1)
    kw = dict(loop=cm.LOOP_PBICGSTAB, maxit=2000, tol=1e-8)
    s = cm.Solver.from_host_csr(ctx, A.rowptr, A.colidx, A.val)
    try:
        s.ilu0()
        dB, dX = _block(ctx, B, A.n), _block(ctx, np.ones((A.n, 3)), A.n)
        sts, form = s.solve_many(3, dB, A.n, dX, A.n, precond=cm.PRECOND_ILU0, **kw)
        X = _unblock(dX, A.n, 3, A.n)
        assert form == 0
        for j in range(3):
            db, dx = ctx.array(B[:, j]), ctx.array(np.ones(A.n))
            st = s.solve(db, dx, precond=cm.PRECOND_ILU0, **kw)
            np.testing.assert_array_equal(X[:, j], dx.download())
            assert st.iters == sts[j].iters and sts[j].converged
    finally:
        s.close()
    sw("MANY_FORM", "columns")
    for loop in (cm.LOOP_PBICGSTAB, cm.LOOP_PBICGSTAB2):
        X, sts, hs, form = _solve_many(cm, ctx, A, B, loop=loop, maxit=2000, tol=1e-8)
        assert form == 0
        for j in range(3):
            x1, st1, h1 = _solve_one(cm, ctx, A, B[:, j], loop=loop, maxit=2000, tol=1e-8)
            np.testing.assert_array_equal(X[:, j], x1)
            np.testing.assert_array_equal(hs[j], h1)
            assert st1.iters == sts[j].iters


def test_auto_form_is_a_valid_choice(cm, ctx, oracle, golden_dir):
    """MANY_FORM = auto (default): whichever form the timing picks, the answers hold to the oracle's tolerances"""
    A = _load(oracle, golden_dir, "mat10000")
    XS = _xstars(A.n, 4, seed=6)
    B = np.stack([oracle.spmv(A, XS[:, j]) for j in range(4)], axis=1)
    X, sts, _, form = _solve_many(cm, ctx, A, B, loop=cm.LOOP_PBICGSTAB, maxit=2000, tol=1e-8)
    assert form in (0, 1)
    for j in range(4):
        assert sts[j].converged and sts[j].t_tune >= 0.0
        assert np.linalg.norm(B[:, j] - oracle.spmv(A, X[:, j])) <= 10 * 1e-8 * sts[j].nrm0


@pytest.mark.parametrize("form_sw", ["batched", "columns"])
def test_bicgstab_many_drop_in(cm, oracle, golden_dir, form_sw, monkeypatch):
    """api.bicgstab_many / cudamat_solve_many on mat10000 with 4 columns against bicgstab per column; bitwise with
    MANY_FORM = columns; the second call with the same matrix reuses the plan"""
    monkeypatch.setenv("CUDAMAT_MANY_FORM", form_sw)
    A = _load(oracle, golden_dir, "mat10000")
    n, nnz = A.n, A.nnz
    XS = _xstars(n, 4, seed=8)
    B = np.stack([oracle.spmv(A, XS[:, j]) for j in range(4)], axis=1)
    ok, X, dt, sts, form = cm.bicgstab_many(n, nnz, A.val, A.rowptr, A.colidx, B, 2000, 1e-8)
    assert form == (1 if form_sw == "batched" else 0)
    assert all(ok) and X.shape == (n, 4)
    for j in range(4):
        ok1, x1, _, st1 = cm.bicgstab(n, nnz, A.val, A.rowptr, A.colidx, B[:, j], 2000, 1e-8)
        assert ok1
        if form_sw == "columns":
            np.testing.assert_array_equal(X[:, j], x1)
            assert sts[j].iters == st1.iters
        else:
            so = oracle.pbicgstab2(A, B[:, j], x0=np.ones(n), tol=1e-8)[2]
            inside, band = ND.iters_inside_oracle_spread(oracle, A, B[:, j], 1, None, sts[j].iters, so.iters, 2000, 1e-8)
            assert inside, (j, sts[j].iters, st1.iters, so.iters, band)
            assert np.linalg.norm(X[:, j] - x1) / np.linalg.norm(x1) <= 1e-5
            assert np.linalg.norm(B[:, j] - oracle.spmv(A, X[:, j])) <= 10 * 1e-8 * st1.nrm0
            assert abs(sts[j].nrm0 - st1.nrm0) <= 1e-12 * st1.nrm0
    ok2, X2, _, sts2, _ = cm.bicgstab_many(n, nnz, A.val, A.rowptr, A.colidx, B, 2000, 1e-8)
    assert all(s.plan_reused == 1 for s in sts2)
    np.testing.assert_array_equal(X2, X)


@pytest.mark.parametrize("nrhs", [1, 2, 3, 8])
def test_loop_bits_batched_solve(cm, ctx, sw, nrhs):
    """three iterations of the batched loop (K = 1, 2, 4 with a padding column, 8) on the diagonal system of
    test_loop_rounding.py: every column's x and residual history equal the column's own CPU mirror bit for bit -- the steps
    of csrc/steps.h, a row per thread in the K-column vector kernels, the SpMM's fused dots in k_spmv<64>'s partition"""
    import test_loop_rounding as L
    assert ("rows", 0) in L.TELLING and ("rows", 1) in L.TELLING
    for name, value in (("MANY_FORM", "batched"), ("SPMV_MODE", "csr"), ("SPMV_LANES", L.LANES), ("FUSED", 0), ("RESIDENT", 0)):
        sw(name, value)
    cols = [L.system(j) for j in range(nrhs)]
    a = cols[0][0]
    s = cm.Solver.from_host_csr(ctx, np.arange(L.N + 1), np.arange(L.N), a)
    try:
        dB, dX = _block(ctx, np.stack([c[1] for c in cols], axis=1), L.N), _block(ctx, np.stack([c[2] for c in cols], axis=1), L.N)
        sts, form = s.solve_many(nrhs, dB, L.N, dX, L.N, loop=cm.LOOP_PBICGSTAB, maxit=L.ITERS, tol=1e-8, flags=cm.FLAG_NO_EXIT)
        X = _unblock(dX, L.N, nrhs, L.N)
        hs = [s.history(col=j) for j in range(nrhs)]
    finally:
        s.close()
    assert form == 1 and [st.iters for st in sts] == [L.ITERS] * nrhs
    for j in range(nrhs):
        want_x, want_h = L.pinned("rows", j)
        print("column", j, "entries of x that differ:", L.differing(X[:, j], want_x), "residuals:", L.differing(hs[j], want_h))
        np.testing.assert_array_equal(hs[j], want_h)
        np.testing.assert_array_equal(X[:, j], want_x)
