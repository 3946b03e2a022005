"""One shift vector per column for one resident matrix, (A0 + I d_j) x_j = b_j (cudamat_solver_spmm_shifts /
cudamat_solver_solve_shifts / cudamat_solve_shifts): the SpMM against the oracle and, bit for bit, against the shared-d path in
both of its epilogues (rows summed by their lanes, rows above 4096 entries swept by the workgroup); the batched loop bit for bit
against the shared-d batched loop column by column, and against the oracle; freeze per column; the column-by-column fall-back;
the host-pointer entry point and its plan cache.  Run on the GPU box with:  python -m pytest tests -m gpu"""
import os

import numpy as np
import pytest

from tests.test_gpu_long_rows import _matrix as _long_matrix

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
    """a library switch for the rest of this test, on the shared context and in the environment (cudamat_solve_shifts)"""
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


def _xstars(n, k, seed=0):
    """k different solutions: two shapes and their multiples (tests/test_gpu_many_rhs.py)"""
    rng = np.random.default_rng(0)
    i = np.arange(n)
    shapes = [1.0 + np.sin(i * c) + 0.1 * rng.random(n) for c in (1.0, 1.37)]
    scales = (1.0, 1.0, 2.0, -1.0, 0.5, -2.0, 4.0, -0.5, 0.25, -4.0, 8.0)
    rot = seed % 2
    return np.stack([scales[j] * shapes[(j + rot) % 2] for j in range(k)], axis=1)


def _split_diagonal(oracle, A):
    """(A0, dg): A with its diagonal taken out (1-based CSR, the recipe of test_batched_pbicgstab2_with_shift), and the diagonal"""
    S = A.to_scipy().tolil()
    dg = S.diagonal().copy()
    S.setdiag(0)
    S = S.tocsr()
    S.eliminate_zeros()
    S.sort_indices()
    return oracle.Csr(A.n, (S.indptr + 1).astype(np.int32), (S.indices + 1).astype(np.int32), S.data, A.n), dg


def _solve_shifts(cm, ctx, A0, D, B, X0, ldd=None, ldb=None, ldx=None, **kw):
    n, k = B.shape
    ldd, ldb, ldx = ldd or n, ldb or n, ldx or n
    s = cm.Solver.from_host_csr(ctx, A0.rowptr, A0.colidx, A0.val)
    try:
        dD, dB, dX = _block(ctx, D, ldd), _block(ctx, B, ldb), _block(ctx, X0, ldx)
        sts, form = s.solve_shifts(k, dD, ldd, dB, ldb, dX, ldx, **kw)
        return _unblock(dX, n, k, ldx), sts, [s.history(col=j) for j in range(k)], form
    finally:
        s.close()


def _solve_many(cm, ctx, A0, d, B, X0, **kw):
    """the existing shared-d path: set_shift(d) + solve_many"""
    n, k = B.shape
    s = cm.Solver.from_host_csr(ctx, A0.rowptr, A0.colidx, A0.val)
    try:
        s.set_shift(ctx.array(d))
        dB, dX = _block(ctx, B, n), _block(ctx, X0, n)
        sts, form = s.solve_many(k, dB, n, dX, n, **kw)
        return _unblock(dX, n, k, n), sts, [s.history(col=j) for j in range(k)], form
    finally:
        s.close()


def _solve_one(cm, ctx, A0, d, b, x0, **kw):
    """a caller's set_shift(d) + Solver.solve"""
    s = cm.Solver.from_host_csr(ctx, A0.rowptr, A0.colidx, A0.val)
    try:
        s.set_shift(ctx.array(d))
        db, dx = ctx.array(b), ctx.array(x0)
        st = s.solve(db, dx, **kw)
        return dx.download(), st, s.history()
    finally:
        s.close()


@pytest.fixture(scope="module")
def family(oracle, golden_dir):
    """mat900 with its diagonal split off and 11 shifted systems on it: D[:, j] = dg (1 + j/8) -- the shifts only add to
    mat900's diagonal dominance --, b_j = (A0 + I d_j) x*_j, a different x0 per column.  Read-only."""
    A = _load(oracle, golden_dir, "mat900")
    A0, dg = _split_diagonal(oracle, A)
    k = 11
    D = dg[:, None] * (1.0 + np.arange(k) / 8.0)[None, :]
    XS = _xstars(A.n, k, seed=2)
    B = np.stack([oracle.spmv(A0, XS[:, j]) + D[:, j] * XS[:, j] for j in range(k)], axis=1)
    X0 = np.cos(np.arange(A.n))[:, None] * (1.0 + np.arange(k))[None, :]
    for a in (D, B, X0, dg):
        a.setflags(write=False)
    return A0, dg, D, B, X0


def _check_vs_oracle(oracle, A0, d, b, x0, x, st):
    """the tolerances of test_batched_pbicgstab2_with_shift: iteration count +-10 % (at least +-2), solution 1e-5, true
    residual <= 1e-7 ||r0||"""
    ok, xo, so = oracle.pbicgstab2(A0, b, d=d, x0=x0, tol=1e-8)
    assert ok and st.converged
    assert abs(st.iters - so.iters) <= max(2, 0.1 * so.iters), (st.iters, so.iters)
    assert np.linalg.norm(x - xo) / np.linalg.norm(xo) <= 1e-5
    assert np.linalg.norm(b - (oracle.spmv(A0, x) + d * x)) <= 1e-7 * so.nrm0


# ---------------------------------------------------------------------------------------------------------------- SpMM
@pytest.mark.parametrize("name", ["mat900", "long_few"])
@pytest.mark.parametrize("lanes", [None, 2, 64])
def test_spmm_shifts_bit_exact_on_integer_data(cm, ctx, oracle, golden_dir, name, lanes, sw):
    """integer-valued A, X and D: exact in fp64, so every column equals oracle.spmv(A, x_j) + D[:, j] * x_j bit for bit, for the
    lanes-per-row variants, batch widths with padding (nrhs 1, 3, 8, 11), leading dimensions above n with three different pads;
    the 6000-row matrix has rows of 4097, 5000 and 6000 entries, which the kernel's other epilogue finishes"""
    if lanes:
        sw("SPMV_LANES", str(lanes))
    rng = np.random.default_rng(5)
    if name == "long_few":
        A = _long_matrix(oracle, "few", integer=True)
    else:
        A = _load(oracle, golden_dir, name)
        A = oracle.Csr(A.n, A.rowptr, A.colidx, rng.integers(-8, 9, A.nnz).astype(np.float64), A.m)
    n = A.n
    s = cm.Solver.from_host_csr(ctx, A.rowptr, A.colidx, A.val)
    try:
        for k in (1, 3, 8, 11):
            X = rng.integers(-8, 9, (n, k)).astype(np.float64)
            D = rng.integers(-3, 4, (n, k)).astype(np.float64)
            ldx, ldd, ldy = n + 3, n + 1, n + 5
            dX, dD, dY = _block(ctx, X, ldx), _block(ctx, D, ldd), _block(ctx, np.zeros((n, k)), ldy)
            s.spmm_shifts(k, dX, ldx, dD, ldd, dY, ldy)
            Y = dY.download().reshape(k, ldy)
            for j in range(k):
                np.testing.assert_array_equal(Y[j, :n], oracle.spmv(A, X[:, j]) + D[:, j] * X[:, j])
                assert np.all(np.isnan(Y[j, n:]))                  # the pad rows of Y are not touched
    finally:
        s.close()


@pytest.mark.parametrize("name", ["rand30000x12", "long_few"])
@pytest.mark.parametrize("lanes", [2, 8, 32])
def test_spmm_shifts_column_is_the_shared_shift_spmv(cm, ctx, oracle, name, lanes, sw):
    """SPMV_MODE = csr, SPMV_LANES = L, real-valued data: column j of spmm_shifts(D) is bit-identical to Solver.spmv of column j
    after set_shift(D[:, j]) (k_spmv<L>), in rows summed by their L lanes and in rows the workgroup sweeps; afterwards the
    solver's own shift is the one set before the call"""
    sw("SPMV_MODE", "csr")
    sw("SPMV_LANES", str(lanes))
    rng = np.random.default_rng(lanes)
    if name == "long_few":
        A = _long_matrix(oracle, "few")
    else:
        A = oracle.rand_rows(30000, 12, 7)
        A.val[:] = rng.standard_normal(A.nnz)
    n, k = A.n, 6
    X = rng.standard_normal((n, k))
    D = rng.standard_normal((n, k))
    own = rng.standard_normal(n)
    s = cm.Solver.from_host_csr(ctx, A.rowptr, A.colidx, A.val)
    try:
        d_own = ctx.array(own)
        s.set_shift(d_own)
        dX, dD, dY = _block(ctx, X, n), _block(ctx, D, n + 2), ctx.empty(k * n)
        s.spmm_shifts(k, dX, n, dD, n + 2, dY, n)
        Y = dY.download().reshape(k, n)
        dx, dy = ctx.array(X[:, 0]), ctx.empty(n)
        s.spmv(dx, dy)                                             # the solver's own shift is still in place
        y_own = dy.download()
        s.set_shift(None)
        s.spmv(dx, dy)
        y_none = dy.download()
        assert np.any(y_own != y_none)
        s.set_shift(d_own)
        s.spmv(dx, dy)
        np.testing.assert_array_equal(y_own, dy.download())
        for j in range(k):
            s.set_shift(ctx.array(D[:, j]))
            dx = ctx.array(X[:, j])
            s.spmv(dx, dy)
            np.testing.assert_array_equal(Y[j], dy.download())
    finally:
        s.close()


# ---------------------------------------------------------------------------------------------------- the batched loop
@pytest.mark.parametrize("loop_name", ["LOOP_PBICGSTAB", "LOOP_PBICGSTAB2"])
def test_batched_shifts_bitwise(cm, ctx, family, loop_name, sw):
    """MANY_FORM = batched, 11 columns (the second group is padded from 3 to 4): column j equals the existing solve_many of that
    one column (nrhs = 1, form 1) after set_shift(D[:, j]) in x, iters, half_exit and history; a permutation of the columns,
    shifts permuted alike, gives the same bits; with all 11 shift columns equal to dg the result is the shared-d solve_many's"""
    sw("MANY_FORM", "batched")
    A0, dg, D, B, X0 = family
    kw = dict(loop=getattr(cm, loop_name), maxit=2000, tol=1e-9)
    X, sts, hs, form = _solve_shifts(cm, ctx, A0, D, B, X0, ldd=A0.n + 2, ldb=A0.n + 7, ldx=A0.n + 1, **kw)
    assert form == 1 and all(st.converged for st in sts)
    for j in range(11):
        X1, st1, h1, f1 = _solve_many(cm, ctx, A0, D[:, j], B[:, j:j + 1], X0[:, j:j + 1], **kw)
        assert f1 == 1
        np.testing.assert_array_equal(X[:, j], X1[:, 0])
        assert (sts[j].iters, sts[j].half_exit) == (st1[0].iters, st1[0].half_exit)
        np.testing.assert_array_equal(hs[j], h1[0])
    perm = np.random.default_rng(0).permutation(11)
    Xp, stp, hp, _ = _solve_shifts(cm, ctx, A0, D[:, perm], B[:, perm], X0[:, perm], **kw)
    for q, j in enumerate(perm):
        np.testing.assert_array_equal(Xp[:, q], X[:, j])
        assert (stp[q].iters, stp[q].half_exit) == (sts[j].iters, sts[j].half_exit)
        np.testing.assert_array_equal(hp[q], hs[j])
    Dsame = np.repeat(dg[:, None], 11, axis=1)
    Xs, sts_s, hs_s, form_s = _solve_shifts(cm, ctx, A0, Dsame, B, X0, **kw)
    Xm, sts_m, hs_m, form_m = _solve_many(cm, ctx, A0, dg, B, X0, **kw)
    assert form_s == 1 and form_m == 1
    np.testing.assert_array_equal(Xs, Xm)
    for j in range(11):
        assert (sts_s[j].iters, sts_s[j].half_exit) == (sts_m[j].iters, sts_m[j].half_exit)
        np.testing.assert_array_equal(hs_s[j], hs_m[j])


def test_batched_shifts_vs_oracle(cm, ctx, oracle, family, sw):
    """the same family, 3 columns, against oracle.pbicgstab2 with each column's own shift"""
    sw("MANY_FORM", "batched")
    A0, dg, D, B, X0 = family
    X, sts, _, form = _solve_shifts(cm, ctx, A0, D[:, :3], B[:, :3], X0[:, :3], loop=cm.LOOP_PBICGSTAB2, maxit=2000, tol=1e-8)
    assert form == 1
    for j in range(3):
        _check_vs_oracle(oracle, A0, D[:, j], B[:, j], X0[:, j], X[:, j], sts[j])


def test_shifts_freeze(cm, ctx, family, sw):
    """4 columns, one started at its exact solution -- b built by spmm_shifts itself, so r0 = 0 exactly --: it reports iters 0
    and keeps its x bit for bit while the others iterate"""
    sw("MANY_FORM", "batched")
    A0, dg, D, _, _ = family
    n = A0.n
    XS = _xstars(n, 4, seed=9)
    s = cm.Solver.from_host_csr(ctx, A0.rowptr, A0.colidx, A0.val)
    try:
        dXS, dD, dB = _block(ctx, XS, n), _block(ctx, D[:, :4], n), ctx.empty(4 * n)
        s.spmm_shifts(4, dXS, n, dD, n, dB, n)
        B = dB.download().reshape(4, n).T.copy()
    finally:
        s.close()
    X0 = np.ones((n, 4))
    X0[:, 1] = XS[:, 1]
    X, sts, _, form = _solve_shifts(cm, ctx, A0, D[:, :4], B, X0, loop=cm.LOOP_PBICGSTAB, maxit=2000, tol=1e-10)
    assert form == 1
    assert sts[1].iters == 0 and sts[1].converged and sts[1].nrm0 == 0.0
    np.testing.assert_array_equal(X[:, 1], XS[:, 1])
    for j in (0, 2, 3):
        assert sts[j].converged and sts[j].iters > 0
        assert np.linalg.norm(X[:, j] - XS[:, j]) <= 1e-6 * np.linalg.norm(XS[:, j])


# ------------------------------------------------------------------------------------------------------------ fall-back
def test_shifts_fallback_is_set_shift_and_solve(cm, ctx, oracle, family, sw):
    """MANY_FORM = columns: form 0, bitwise set_shift(D[:, j]) + Solver.solve per column, histories included; LOOP_PIPELINED with
    D: form 0 and every column converges; a preconditioner with D is an argument error"""
    A0, dg, D, B, X0 = family
    D, B, X0 = D[:, :3], B[:, :3], X0[:, :3]
    sw("MANY_FORM", "columns")
    for loop in (cm.LOOP_PBICGSTAB, cm.LOOP_PBICGSTAB2):
        kw = dict(loop=loop, maxit=2000, tol=1e-8)
        X, sts, hs, form = _solve_shifts(cm, ctx, A0, D, B, X0, **kw)
        assert form == 0
        for j in range(3):
            x1, st1, h1 = _solve_one(cm, ctx, A0, D[:, j], B[:, j], X0[:, j], **kw)
            np.testing.assert_array_equal(X[:, j], x1)
            np.testing.assert_array_equal(hs[j], h1)
            assert (st1.iters, st1.half_exit) == (sts[j].iters, sts[j].half_exit)
    sw("MANY_FORM", "batched")
    X, sts, _, form = _solve_shifts(cm, ctx, A0, D, B, X0, loop=cm.LOOP_PIPELINED, maxit=2000, tol=1e-8)
    assert form == 0
    for j in range(3):
        assert sts[j].converged
        assert np.linalg.norm(B[:, j] - (oracle.spmv(A0, X[:, j]) + D[:, j] * X[:, j])) <= 1e-7 * sts[j].nrm0
    with pytest.raises(cm.CudamatError) as e:
        _solve_shifts(cm, ctx, A0, D, B, X0, precond=cm.PRECOND_ILU0, loop=cm.LOOP_PBICGSTAB, maxit=10, tol=1e-8)
    assert e.value.code == 2 and "no preconditioner" in str(e.value)


def test_shifts_auto_form_is_a_valid_choice(cm, ctx, oracle, family):
    """MANY_FORM = auto (default): whichever form the timing picks, the answers hold to the oracle's tolerances"""
    A0, dg, D, B, X0 = family
    X, sts, _, form = _solve_shifts(cm, ctx, A0, D[:, :3], B[:, :3], X0[:, :3], loop=cm.LOOP_PBICGSTAB2, maxit=2000, tol=1e-8)
    assert form in (0, 1)
    for j in range(3):
        assert sts[j].t_tune >= 0.0
        _check_vs_oracle(oracle, A0, D[:, j], B[:, j], X0[:, j], X[:, j], sts[j])


# -------------------------------------------------------------------------------------------------------------- drop-in
@pytest.mark.parametrize("form_sw", ["batched", "columns"])
def test_bicgstab_d_many_drop_in(cm, oracle, golden_dir, form_sw, monkeypatch):
    """api.bicgstab_d_many / cudamat_solve_shifts on mat10000 with its diagonal split off, 4 scalar shifts sigma_j = its mean
    diagonal times {1.25, 1.5, 2, 3}.  mat10000's diagonal is the constant 4 and equals its rows' off-diagonal sums: the matrix
    itself (factor 1) is only weakly dominant and takes the oracle 169 iterations, which amplify rounding beyond the +-10 % rule
    (tests/test_gpu_many_rhs.py: _xstars); from 1.25 on A0 + sigma I is strictly dominant and the oracle needs 5 to 18
    iterations for each of the 8 systems solved here (run on the CPU beforehand).  Bitwise bicgstab_d per column with
    MANY_FORM = columns, the oracle's tolerances with batched; a second call with the same A0 and OTHER shifts reuses the plan
    and solves the new systems"""
    monkeypatch.setenv("CUDAMAT_MANY_FORM", form_sw)
    A = _load(oracle, golden_dir, "mat10000")
    A0, dg = _split_diagonal(oracle, A)
    n, nnz = A0.n, A0.nnz
    sigma = float(np.mean(dg)) * np.array([1.25, 1.5, 2.0, 3.0])
    XS = _xstars(n, 4, seed=8)
    X0 = np.ones((n, 4))

    def rhs(sig):
        return np.stack([oracle.spmv(A0, XS[:, j]) + sig[j] * XS[:, j] for j in range(4)], axis=1)

    def check(sig, B, X, sts):
        for j in range(4):
            d = np.full(n, sig[j])
            if form_sw == "columns":
                ok1, x1, _, st1 = cm.bicgstab_d(n, nnz, A0.val, A0.rowptr, A0.colidx, d, X0[:, j], B[:, j], 2000, 1e-8)
                assert ok1
                np.testing.assert_array_equal(X[:, j], x1)
                assert sts[j].iters == st1.iters
            else:
                _check_vs_oracle(oracle, A0, d, B[:, j], X0[:, j], X[:, j], sts[j])

    B = rhs(sigma)
    ok, X, dt, sts, form = cm.bicgstab_d_many(n, nnz, A0.val, A0.rowptr, A0.colidx, sigma, X0, B, 2000, 1e-8)
    assert form == (1 if form_sw == "batched" else 0)
    assert all(ok) and X.shape == (n, 4)
    check(sigma, B, X, sts)
    # (the per-column bicgstab_d calls above went through the same plan cache with the same A0: the matrix is still cached)
    sigma2 = sigma[::-1] * 1.25
    B2 = rhs(sigma2)
    ok2, X2, _, sts2, form2 = cm.bicgstab_d_many(n, nnz, A0.val, A0.rowptr, A0.colidx, sigma2, X0, B2, 2000, 1e-8)
    assert all(ok2) and form2 == form
    assert all(s.plan_reused == 1 for s in sts2)
    check(sigma2, B2, X2, sts2)
