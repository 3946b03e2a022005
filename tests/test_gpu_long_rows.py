"""Rows above 4096 entries -- the whole-workgroup sweep of k_spmv<L> (csrc/spmv_csr.hip) and k_spmm_csr<L, K> (csrc/batch.hip) --
and the edge systems of the several-right-hand-sides path.  The contract checked here: the bits of a row of the SpMV / SpMM
are a function of the row, x and L alone -- not of how many long rows sit beside it, not of wave scheduling, not of the batch.
One small matrix builder (n = 6000, at most 0.24 M entries) serves every test; real-valued data wherever the summation ORDER is
the subject (on integer data every order gives the same sum).  Run on the GPU box with:  python -m pytest tests -m gpu"""
import functools
import math

import numpy as np
import pytest

from tests.test_gpu_many_rhs import (cm, ctx, sw, _serial_oracle, _load, _block, _unblock, _solve_many,  # noqa: F401
                                     _solve_one, _xstars, _outcome)

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
N = 6000
SHORT = 6
LONG = 4096                      # kLongRow: a row with MORE entries than this is swept by the whole workgroup

FEW = {0: 4097, 1: 5000, 10: 4096, 3000: 6000, N - 1: 4097}
CROWD = {r: 4200 for r in range(128, 128 + 48)}


# ------------------------------------------------------------------------------------------------------------ the builder
@functools.lru_cache(maxsize=None)
def _rows(kind, integer):
    """per row: sorted distinct columns (the diagonal among them) and values; short rows 6 entries, the rows of `kind` their
    lengths.  The random stream depends on kind and integer only, so crowd_q holds the very entries of crowd."""
    long_rows = FEW if kind == "few" else CROWD
    rng = np.random.default_rng(77 if kind == "few" else 78)
    cols, vals = [], []
    for r in range(N):
        length = long_rows.get(r, SHORT)
        if length == N:
            c = np.arange(N)
        else:
            others = rng.choice(N - 1, size=length - 1, replace=False)
            others[others >= r] += 1                                   # every column but r
            c = np.sort(np.concatenate([others, [r]]))
        v = rng.integers(-8, 9, length).astype(np.float64) if integer else rng.standard_normal(length)
        cols.append(c)
        vals.append(v)
    return cols, vals


@functools.lru_cache(maxsize=None)
def _csr_arrays(kind, integer, diag_dominant):
    """kind: "few", "crowd", or "crowd_q" (q = 0..3: of crowd's long rows only those with row % 4 == q stay long, the others
    keep their first 6 entries)"""
    base = kind.split("_")[0]
    cols, vals = _rows(base, integer)
    if base != kind:
        q = int(kind.split("_")[1])
        cols = [c if (r not in CROWD or r % 4 == q) else c[:SHORT] for r, c in enumerate(cols)]
        vals = [v if (r not in CROWD or r % 4 == q) else v[:SHORT] for r, v in enumerate(vals)]
    rp = np.zeros(N + 1, np.int32)
    np.cumsum([len(c) for c in cols], out=rp[1:])
    ci = np.concatenate(cols).astype(np.int32)
    val = np.concatenate(vals)
    if diag_dominant:                                                  # the recipe of test_spmv_skewed_rows
        row_of = np.repeat(np.arange(N), np.diff(rp))
        on_diag = ci == row_of
        off = np.where(on_diag, 0.0, np.abs(val))
        val = val.copy()
        val[on_diag] = np.add.reduceat(off, rp[:-1]) + 1.0
    for a in (rp, ci, val):
        a.setflags(write=False)
    return rp, ci, val


def _matrix(oracle, kind, integer=False, diag_dominant=False):
    rp, ci, val = _csr_arrays(kind, integer, diag_dominant)
    return oracle.Csr(N, rp, ci, val, N)                               # sorted, base 0


def test_builder_shapes(oracle):
    """(runs on the GPU box with the rest; checks the matrices are what the tests below say they are)"""
    few, crowd = _matrix(oracle, "few"), _matrix(oracle, "crowd")
    lf, lc = np.diff(few.rowptr), np.diff(crowd.rowptr)
    assert [lf[r] for r in (0, 1, 10, 3000, N - 1)] == [4097, 5000, 4096, 6000, 4097]
    assert np.sum(lf > LONG) == 4 and np.sum(lf == SHORT) == N - 5
    assert np.all(lc[128:176] == 4200) and np.sum(lc > LONG) == 48 and crowd.nnz < 250000
    for q in range(4):
        cq = _matrix(oracle, "crowd_%d" % q)
        lq = np.diff(cq.rowptr)
        assert [r for r in range(N) if lq[r] > LONG] == [r for r in range(128, 176) if r % 4 == q]
        for r in range(128 + q, 176, 4):                               # the very entries of crowd
            a, b = crowd.rowptr[r], cq.rowptr[r]
            np.testing.assert_array_equal(crowd.colidx[a:a + 4200], cq.colidx[b:b + 4200])
            np.testing.assert_array_equal(crowd.val[a:a + 4200], cq.val[b:b + 4200])
    dd = _matrix(oracle, "few", diag_dominant=True)
    D = dd.to_scipy()
    assert np.all(2 * np.abs(D.diagonal()) > np.asarray(abs(D).sum(axis=1)).ravel())
    for A in (few, crowd, dd):
        assert A.rowptr[0] == 0
        for r in (0, 1, 10, 128, 175, 3000, N - 1):
            c = A.colidx[A.rowptr[r]:A.rowptr[r + 1]]
            assert np.all(np.diff(c) > 0) and r in c


# ------------------------------------------------------------------------------------------------------------- helpers
def _solver_spmv(cm, ctx, A, x, d=None, repeat=1, kernel=None):
    """Solver.spmv, `repeat` launches; returns the list of results"""
    s = cm.Solver.from_host_csr(ctx, A.rowptr, A.colidx, A.val)
    try:
        if d is not None:
            s.set_shift(ctx.array(d))
        if kernel:
            assert s.spmv_kernel() == kernel, s.spmv_kernel()
        dx = ctx.array(x)
        out = []
        for _ in range(repeat):
            dy = ctx.array(np.full(A.n, np.nan))
            s.spmv(dx, dy)
            out.append(dy.download())
            dy.free()
        dx.free()
        return out
    finally:
        s.close()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _reference(A, x):
    """row sums in a wider format than fp64: longdouble products and sums where longdouble is wider (x86: 64-bit mantissa,
    a rounding of 2^-64 per operation, 2^-11 eps), else the exactly rounded math.fsum of the fp64 products"""
    if np.finfo(np.longdouble).eps < EPS:
        prod = A.val.astype(np.longdouble) * x[A.colidx].astype(np.longdouble)
        return np.add.reduceat(prod, A.rowptr[:-1])                    # (no empty rows in these matrices)
    return np.array([math.fsum(A.val[a:b] * x[A.colidx[a:b]]) for a, b in zip(A.rowptr[:-1], A.rowptr[1:])])


# -------------------------------------------------------------------------------- 1. a long row and the rows beside it
@pytest.mark.parametrize("lanes", [2, 4])
def test_long_row_does_not_depend_on_its_neighbours(cm, ctx, oracle, lanes, sw):
    """48 adjacent rows of 4200 entries in one partition of k_spmv<L> (L = 2: 128 rows, L = 4: 64 rows) -- more than the 32
    slots of the long-row table.  y[row] must be, bit for bit, what it is in the matrix where only every fourth of them is
    long (12 per partition: all fit the table), and the same launch repeated gives the same bits.
    (Before the sweep took every long row, the 16 rows that found the table full were summed by their L lanes, another order
    of 4200 real-valued products; WHICH rows those were depended on the order in which the waves reached the table.)"""
    sw("SPMV_MODE", "csr")
    sw("SPMV_LANES", str(lanes))
    kernel = "k_spmv<%d>" % lanes
    x = np.random.default_rng(5).standard_normal(N)
    runs = _solver_spmv(cm, ctx, _matrix(oracle, "crowd"), x, repeat=5, kernel=kernel)
    y = runs[0]
    differ = []
    for q in range(4):
        yq = _solver_spmv(cm, ctx, _matrix(oracle, "crowd_%d" % q), x, kernel=kernel)[0]
        differ += [r for r in range(128 + q, 176, 4) if _bits(y[r:r + 1])[0] != _bits(yq[r:r + 1])[0]]
    unstable = [k for k in range(1, 5) if not np.array_equal(_bits(runs[k]), _bits(y))]
    print("lanes", lanes, "rows whose bits depend on their neighbours:", sorted(differ), "repeats that differ:", unstable)
    assert not differ, "rows %s differ between crowd and crowd_q" % sorted(differ)
    assert not unstable


# ------------------------------------------------------------------------------------- 2. accuracy against a wide reference
@pytest.mark.parametrize("kind", ["few", "crowd"])
@pytest.mark.parametrize("lanes", [None, 2, 4, 64])
def test_long_rows_accuracy(cm, ctx, oracle, kind, lanes, sw):
    """every row: |y - y_ref| <= 4 nnz_row eps sum|a_ij x_j| (the bound of test_spmm_real_data_tolerance) on real
    data, equality with the oracle on integer data; through the raw lanes-per-row kernel (Context.spmv) and through
    Solver.spmv with SPMV_MODE = csr"""
    sw("SPMV_MODE", "csr")
    if lanes:
        sw("SPMV_LANES", str(lanes))
    rng = np.random.default_rng(6)
    A = _matrix(oracle, kind)
    x = rng.standard_normal(N)
    absA = oracle.Csr(N, A.rowptr, A.colidx, np.abs(A.val), N)
    bound = 4 * np.diff(A.rowptr) * EPS * oracle.spmv(absA, np.abs(x))
    ref = _reference(A, x)
    Ai = _matrix(oracle, kind, integer=True)
    xi = rng.integers(-8, 9, N).astype(np.float64)
    want_i = oracle.spmv(Ai, xi)
    for M, v, check in ((A, x, "real"), (Ai, xi, "int")):
        rp, ci, val = ctx.array(M.rowptr), ctx.array(M.colidx), ctx.array(M.val)
        dx, dy = ctx.array(v), ctx.array(np.full(N, np.nan))
        ctx.spmv(N, rp, ci, val, 0, dx, dy)
        got = [dy.download(), _solver_spmv(cm, ctx, M, v)[0]]
        for a in (rp, ci, val, dx, dy):
            a.free()
        for y in got:
            if check == "int":
                np.testing.assert_array_equal(y, want_i)
            else:
                err = np.abs(y.astype(np.longdouble) - ref).astype(np.float64)
                worst = int(np.argmax(err / bound))
                print(kind, lanes, "worst row", worst, "err / bound", err[worst] / bound[worst])
                assert np.all(err <= bound), (worst, err[worst], bound[worst])


# --------------------------------------------------------------------------------- 3. the SpMM's sweep is the SpMV's sweep
@pytest.mark.parametrize("kind", ["few", "crowd"])
@pytest.mark.parametrize("lanes", [2, 4, 32])
def test_spmm_sweep_is_the_spmv_sweep(cm, ctx, oracle, kind, lanes, sw):
    """SPMV_MODE = csr, SPMV_LANES = L on matrices WITH rows above 4096 entries: column j of Solver.spmm (k_spmm_csr<L, K>) is
    bit-identical to Solver.spmv of column j (k_spmv<L>) for nrhs 1..11 (K = 1, 2, 4, 8 and a padded second block), with and
    without the shift d, leading dimensions above n; the pad rows of Y keep their NaN; on integer data every column equals
    the oracle"""
    sw("SPMV_MODE", "csr")
    sw("SPMV_LANES", str(lanes))
    rng = np.random.default_rng(lanes)
    ldx, ldy = N + 3, N + 5
    for integer in (False, True):
        A = _matrix(oracle, kind, integer=integer)
        draw = (lambda *sh: rng.integers(-8, 9, sh).astype(np.float64)) if integer else (lambda *sh: rng.standard_normal(sh))
        d = rng.integers(-3, 4, N).astype(np.float64) if integer else rng.standard_normal(N)
        s = cm.Solver.from_host_csr(ctx, A.rowptr, A.colidx, A.val)
        try:
            assert s.spmv_kernel() == "k_spmv<%d>" % lanes
            for shift in (False, True):
                if shift:
                    s.set_shift(ctx.array(d))
                for k in (1, 2, 3, 8, 11):
                    X = draw(N, k)
                    dX, dY = _block(ctx, X, ldx), _block(ctx, np.zeros((N, k)), ldy)
                    s.spmm(k, dX, ldx, dY, ldy)
                    Y = dY.download().reshape(k, ldy)
                    for j in range(k):
                        dx, dy = ctx.array(X[:, j]), ctx.empty(N)
                        s.spmv(dx, dy)
                        y1 = dy.download()
                        bad = np.flatnonzero(_bits(Y[j, :N]) != _bits(y1))
                        assert bad.size == 0, (integer, shift, k, j, bad[:8])
                        assert np.all(np.isnan(Y[j, N:]))              # the pad rows of Y are not touched
                        if integer:
                            np.testing.assert_array_equal(y1, oracle.spmv(A, X[:, j]) + (d * X[:, j] if shift else 0.0))
                        for a in (dx, dy):
                            a.free()
                    for a in (dX, dY):
                        a.free()
        finally:
            s.close()


# --------------------------------------------------------------------------------------- 4. the batched loop over long rows
def _check_column_vs_oracle(oracle, A, b, x, st, h, tol, maxit):
    xo, so = oracle.pbicgstab(A, b, maxit=maxit, tol=tol)
    ho = oracle.pbicgstab(A, b, maxit=4, tol=1e-30, want_hist=True)[2]
    res = np.linalg.norm(b - oracle.spmv(A, x))
    print("iters", st.iters, "oracle", so.iters, "res / (tol nrm0)", res / (tol * so.nrm0), "nrm0", st.nrm0, so.nrm0)
    assert st.converged and so.converged
    assert abs(st.nrm0 - so.nrm0) <= 1e-12 * so.nrm0
    assert res <= 10 * tol * so.nrm0
    k = min(len(h), 8)
    # (diagonals of thousands next to 6: histories agree for the first iterations and then drift with the rounding order of
    #  the long dots -- the figures and the reason of test_spmv_skewed_rows)
    np.testing.assert_allclose(h[:k], ho[:k], rtol=1e-7)
    assert abs(st.iters - so.iters) <= max(3, 0.3 * so.iters), (st.iters, so.iters)


@pytest.mark.parametrize("kind", ["few", "crowd"])
def test_batched_loop_over_long_rows(cm, ctx, oracle, kind, sw):
    """MANY_FORM = batched, SPMV_LANES = 2 on the diagonally dominant matrices: the sweep's fused (w.y, y.y) partials for K
    columns.  Every column is bitwise the column solved alone and in a permuted batch (x, iterations, history), and holds to
    the oracle's loop"""
    sw("MANY_FORM", "batched")
    sw("SPMV_LANES", "2")
    tol, maxit = 1e-10, 200
    A = _matrix(oracle, kind, diag_dominant=True)
    XS = _xstars(N, 3, seed=1)
    XS[:, 2] = 1.0 + np.cos(0.37 * np.arange(N))                       # (a third shape: _xstars' third is twice its first)
    B = np.stack([oracle.spmv(A, XS[:, j]) for j in range(3)], axis=1)
    kw = dict(loop=cm.LOOP_PBICGSTAB, maxit=maxit, tol=tol)
    X, sts, hs, form = _solve_many(cm, ctx, A, B, **kw)
    assert form == 1
    perm = np.array([2, 0, 1])
    Xp, stp, hp, fp = _solve_many(cm, ctx, A, B[:, perm], **kw)
    assert fp == 1
    for q, j in enumerate(perm):
        np.testing.assert_array_equal(_bits(Xp[:, q]), _bits(X[:, j]))
        assert (stp[q].iters, stp[q].half_exit) == (sts[j].iters, sts[j].half_exit)
        np.testing.assert_array_equal(_bits(hp[q]), _bits(hs[j]))
    for j in range(3):
        X1, st1, h1, f1 = _solve_many(cm, ctx, A, B[:, j:j + 1], **kw)
        assert f1 == 1
        np.testing.assert_array_equal(_bits(X1[:, 0]), _bits(X[:, j]))
        assert (st1[0].iters, st1[0].half_exit) == (sts[j].iters, sts[j].half_exit)
        np.testing.assert_array_equal(_bits(h1[0]), _bits(hs[j]))
        _check_column_vs_oracle(oracle, A, B[:, j], X[:, j], sts[j], hs[j], tol, maxit)


def test_batched_ilu0_loop_over_long_rows(cm, ctx, oracle, sw):
    """the same with ILU(0) and MANY_PRECOND = batched on `few`, against the per-column Solver.solve(precond = ILU0) with the
    tolerances of test_batched_ilu0_solve_vs_oracle"""
    sw("MANY_FORM", "batched")
    sw("MANY_PRECOND", "batched")
    sw("SPMV_LANES", "2")
    tol, maxit = 1e-10, 200
    A = _matrix(oracle, "few", diag_dominant=True)
    XS = _xstars(N, 3, seed=1)
    XS[:, 2] = 1.0 + np.cos(0.37 * np.arange(N))
    B = np.stack([oracle.spmv(A, XS[:, j]) for j in range(3)], axis=1)
    kw = dict(loop=cm.LOOP_PBICGSTAB, maxit=maxit, tol=tol)
    X, sts, hs, form = _solve_many(cm, ctx, A, B, precond=cm.PRECOND_ILU0, **kw)
    assert form == 1
    for j in range(3):
        x1, st1, h1 = _solve_one(cm, ctx, A, B[:, j], precond=cm.PRECOND_ILU0, ilu=True, **kw)
        res = np.linalg.norm(B[:, j] - oracle.spmv(A, X[:, j]))
        print("col", j, "iters", sts[j].iters, "single", st1.iters, "res / (tol nrm0)", res / (tol * st1.nrm0))
        assert sts[j].converged and st1.converged
        assert abs(sts[j].iters - st1.iters) <= max(2, 0.1 * st1.iters)
        assert np.linalg.norm(X[:, j] - x1) / np.linalg.norm(x1) <= 1e-5
        assert res <= 10 * tol * st1.nrm0
        k = min(len(hs[j]), len(h1), 6)
        np.testing.assert_allclose(hs[j][:k], h1[:k], rtol=1e-8)
        assert len(hs[j]) == 2 * sts[j].iters + (1 if sts[j].half_exit else 0)


# ------------------------------------------------------------------------------- 5. edge systems through solve_many / spmm
def _dense_csr(oracle, M):
    n = M.shape[0]
    return oracle.Csr(n, np.arange(0, n * n + 1, n, dtype=np.int32), np.tile(np.arange(n, dtype=np.int32), n), M.ravel().copy(), n)


def _summary(st):
    return (st.iters, int(st.half_exit), bool(st.converged), bool(st.breakdown))


def test_edge_1x1(cm, ctx, oracle, sw):
    """[4] x = b for b = 2, 4, -2 from x0 = 0: gpu_pbicgstab leaves through the half step at 0 iterations with x = b / 4
    (s = r - alpha v = 0); gpu_pbicgstab2 has no half-step test and reports the breakdown (omega = 0 / 0) the single loop and
    the oracle report"""
    sw("MANY_FORM", "batched")
    A1 = oracle.Csr(1, np.array([1, 2], np.int32), np.array([1], np.int32), np.array([4.0]), 1)
    B = np.array([[2.0, 4.0, -2.0]])
    X0 = np.zeros((1, 3))
    X, sts, hs, form = _solve_many(cm, ctx, A1, B, X0=X0, loop=cm.LOOP_PBICGSTAB, maxit=10, tol=1e-10)
    assert form == 1
    for j in range(3):
        x1, st1, h1 = _solve_one(cm, ctx, A1, B[:, j], x0=X0[:, j], loop=cm.LOOP_PBICGSTAB, maxit=10, tol=1e-10)
        assert _summary(sts[j]) == _summary(st1) == (0, 1, True, False)
        assert abs(X[0, j] - B[0, j] / 4.0) < 1e-15 and abs(x1[0] - B[0, j] / 4.0) < 1e-15
        assert len(hs[j]) == len(h1) == 1
    X, sts, hs, form = _solve_many(cm, ctx, A1, B, X0=X0, loop=cm.LOOP_PBICGSTAB2, maxit=10, tol=1e-10)
    assert form == 1
    for j in range(3):
        _, st1, _ = _solve_one(cm, ctx, A1, B[:, j], x0=X0[:, j], loop=cm.LOOP_PBICGSTAB2, maxit=10, tol=1e-10)
        oko, _, so = oracle.pbicgstab2(A1, B[:, j], x0=X0[:, j], maxit=10, tol=1e-10)
        assert not oko and sts[j].breakdown == st1.breakdown == so.breakdown == 1
        assert sts[j].iters == st1.iters == so.iters and not sts[j].converged


@pytest.mark.parametrize("n", [2, 3])
def test_edge_tiny_dense(cm, ctx, oracle, n, sw):
    """n = 2 and 3, dense and dominant, 8 right-hand sides: every column converges to the residual bound 10 tol ||r0|| as its
    single solve does, so the two answers differ by at most ||A^-1|| (10 + 10) tol ||r0||"""
    sw("MANY_FORM", "batched")
    rng = np.random.default_rng(n)
    M = rng.standard_normal((n, n)) + np.diag(2.0 * n + rng.random(n))
    A = _dense_csr(oracle, M)
    B = rng.standard_normal((n, 8))
    tol = 1e-10
    X, sts, hs, form = _solve_many(cm, ctx, A, B, loop=cm.LOOP_PBICGSTAB, maxit=50, tol=tol)
    assert form == 1
    inv_norm = np.linalg.norm(np.linalg.inv(M), 2)
    for j in range(8):
        x1, st1, _ = _solve_one(cm, ctx, A, B[:, j], loop=cm.LOOP_PBICGSTAB, maxit=50, tol=tol)
        nrm0 = np.linalg.norm(B[:, j] - M @ np.ones(n))
        assert sts[j].converged and st1.converged and not sts[j].breakdown
        assert abs(sts[j].nrm0 - nrm0) <= 1e-12 * nrm0
        assert np.linalg.norm(B[:, j] - M @ X[:, j]) <= 10 * tol * nrm0
        assert np.linalg.norm(X[:, j] - x1) <= inv_norm * 20 * tol * nrm0
        assert sts[j].iters + sts[j].half_exit <= n + 1                # (n steps in exact arithmetic)


def test_edge_diagonal(cm, ctx, oracle, sw):
    """the diagonal system of test_degenerate_systems, 3 columns: the plain batched loop converges to b / d; with ILU(0)
    (exact for a diagonal matrix) and MANY_PRECOND = batched every column needs at most 1 iteration, as its single solve"""
    sw("MANY_FORM", "batched")
    sw("MANY_PRECOND", "batched")
    n = 1000
    dg = 1.0 + np.arange(n) % 7
    A = oracle.Csr(n, np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), dg, n)
    B = dg[:, None] * np.stack([1.0 + np.arange(n) % 3, 2.0 + np.arange(n) % 5, -1.0 - np.arange(n) % 2], axis=1)
    X, sts, _, form = _solve_many(cm, ctx, A, B, loop=cm.LOOP_PBICGSTAB, maxit=50, tol=1e-12)
    assert form == 1 and all(st.converged for st in sts)
    np.testing.assert_allclose(X, B / dg[:, None], rtol=1e-10)
    X, sts, _, form = _solve_many(cm, ctx, A, B, precond=cm.PRECOND_ILU0, loop=cm.LOOP_PBICGSTAB, maxit=50, tol=1e-12)
    assert form == 1
    for j in range(3):
        x1, st1, _ = _solve_one(cm, ctx, A, B[:, j], precond=cm.PRECOND_ILU0, ilu=True, loop=cm.LOOP_PBICGSTAB, maxit=50,
                                tol=1e-12)
        assert sts[j].converged and st1.converged and sts[j].iters <= 1 and st1.iters <= 1
        np.testing.assert_allclose(X[:, j], B[:, j] / dg, rtol=1e-12)
        np.testing.assert_allclose(x1, B[:, j] / dg, rtol=1e-12)


def test_edge_spmm_empty_rows_and_no_entries(cm, ctx, oracle):
    """spmm on the 4-row matrix with two empty rows of test_degenerate_systems and on a matrix with no entries (Y = 0, or
    Y = d X with a shift): every column is bitwise Solver.spmv of that column, and what the arithmetic says"""
    rng = np.random.default_rng(4)
    E = oracle.Csr(4, np.array([0, 1, 1, 2, 2], np.int32), np.array([0, 2], np.int32), np.array([2.0, 3.0]), 4)
    Z = oracle.Csr(5, np.zeros(6, np.int32), np.zeros(0, np.int32), np.zeros(0), 5)
    for A, dense in ((E, np.array([[2.0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 3.0, 0], [0, 0, 0, 0]])), (Z, np.zeros((5, 5)))):
        n = A.n
        d = rng.integers(-3, 4, n).astype(np.float64)
        s = cm.Solver.from_host_csr(ctx, A.rowptr, A.colidx, A.val)
        try:
            for shift in (False, True):
                if shift:
                    s.set_shift(ctx.array(d))
                for k in (1, 3, 9):
                    X = rng.integers(-8, 9, (n, k)).astype(np.float64)
                    dX, dY = _block(ctx, X, n + 2), _block(ctx, np.full((n, k), 7.0), n + 1)
                    s.spmm(k, dX, n + 2, dY, n + 1)
                    Y = dY.download().reshape(k, n + 1)
                    for j in range(k):
                        dx, dy = ctx.array(X[:, j]), ctx.array(np.full(n, 7.0))
                        s.spmv(dx, dy)
                        np.testing.assert_array_equal(_bits(Y[j, :n]), _bits(dy.download()))
                        np.testing.assert_array_equal(Y[j, :n], dense @ X[:, j] + (d * X[:, j] if shift else 0.0))
                        assert np.isnan(Y[j, n])
        finally:
            s.close()


def test_edge_maxit_zero_and_no_columns(cm, ctx, oracle, golden_dir, sw):
    """maxit = 0: X comes back bitwise X0, no iteration, not converged, no history -- per column what the single solve reports;
    nrhs = 0: OK, nothing is read or written"""
    sw("MANY_FORM", "batched")
    A = _load(oracle, golden_dir, "mat900")
    n = A.n
    B = np.stack([oracle.spmv(A, _xstars(n, 3)[:, j]) for j in range(3)], axis=1)
    X0 = np.cos(np.arange(n))[:, None] * np.array([1.0, 2.0, -3.0])[None, :]
    X, sts, hs, form = _solve_many(cm, ctx, A, B, X0=X0, ldx=n + 2, loop=cm.LOOP_PBICGSTAB, maxit=0, tol=1e-8)
    assert form == 1
    np.testing.assert_array_equal(_bits(X), _bits(X0))
    for j in range(3):
        x1, st1, h1 = _solve_one(cm, ctx, A, B[:, j], x0=X0[:, j], loop=cm.LOOP_PBICGSTAB, maxit=0, tol=1e-8)
        np.testing.assert_array_equal(_bits(x1), _bits(X0[:, j]))
        assert _summary(sts[j]) == _summary(st1) == (0, 0, False, False)
        assert len(hs[j]) == len(h1) == 0
        assert abs(sts[j].nrm0 - st1.nrm0) <= 1e-12 * st1.nrm0 and st1.nrm0 > 0.0
    s = cm.Solver.from_host_csr(ctx, A.rowptr, A.colidx, A.val)
    try:
        keep_b, keep_x = np.arange(2.0 * n), -np.arange(2.0 * n)
        dB, dX = ctx.array(keep_b), ctx.array(keep_x)
        sts, form = s.solve_many(0, dB, n, dX, n, loop=cm.LOOP_PBICGSTAB, maxit=10, tol=1e-8)
        assert sts == [] and form == 0
        s.spmm(0, dB, n, dX, n)
        sts, form = s.solve_many(0, None, n, None, n)
        assert sts == [] and form == 0
        s.spmm(0, None, n, None, n)
        np.testing.assert_array_equal(dB.download(), keep_b)
        np.testing.assert_array_equal(dX.download(), keep_x)
    finally:
        s.close()


def test_edge_block_boundaries(cm, ctx, oracle, golden_dir, sw):
    """nrhs = 8, 9, 16, 17 on mat900 (blocks of 8 columns; 9 and 17 end in a block of one): the first and the last column of
    every block is bitwise that column solved alone"""
    sw("MANY_FORM", "batched")
    A = _load(oracle, golden_dir, "mat900")
    n = A.n
    rng = np.random.default_rng(8)
    XS = 1.0 + np.sin(np.outer(np.arange(n), 0.1 + rng.random(17))) + 0.1 * rng.random((n, 17))
    B = np.stack([oracle.spmv(A, XS[:, j]) for j in range(17)], axis=1)
    kw = dict(loop=cm.LOOP_PBICGSTAB, maxit=2000, tol=1e-9)
    alone = {}
    for nrhs in (8, 9, 16, 17):
        X, sts, hs, form = _solve_many(cm, ctx, A, B[:, :nrhs], **kw)
        assert form == 1 and all(st.converged for st in sts)
        ends = sorted({c for c0 in range(0, nrhs, 8) for c in (c0, min(c0 + 7, nrhs - 1))})
        for j in ends:
            if j not in alone:
                X1, st1, h1, f1 = _solve_many(cm, ctx, A, B[:, j:j + 1], **kw)
                assert f1 == 1
                alone[j] = (X1[:, 0], _summary(st1[0]), h1[0])
            np.testing.assert_array_equal(_bits(X[:, j]), _bits(alone[j][0]))
            assert _summary(sts[j]) == alone[j][1]
            np.testing.assert_array_equal(_bits(hs[j]), _bits(alone[j][2]))


def test_edge_nan_column_and_frozen_column(cm, ctx, oracle, golden_dir, sw):
    """a column of B holding one NaN between two ordinary columns reports breakdown (as its single solve), and the other two
    are bitwise what they are beside a column of zeros instead; a column with b = 0 and x0 = 0 starts frozen (nrm0 = 0,
    converged, no iteration, x untouched) while its neighbours iterate"""
    sw("MANY_FORM", "batched")
    A = _load(oracle, golden_dir, "mat900")
    n = A.n
    XS = _xstars(n, 3, seed=3)
    B = np.stack([oracle.spmv(A, XS[:, j]) for j in range(3)], axis=1)
    kw = dict(loop=cm.LOOP_PBICGSTAB, maxit=2000, tol=1e-9)
    Bz = B.copy()
    Bz[:, 1] = 0.0
    Bn = Bz.copy()
    Bn[n // 2, 1] = np.nan
    Xz, stz, hz, fz = _solve_many(cm, ctx, A, Bz, **kw)
    Xn, stn, hn, fn = _solve_many(cm, ctx, A, Bn, **kw)
    assert fz == 1 and fn == 1
    _, st1, _ = _solve_one(cm, ctx, A, Bn[:, 1], **kw)
    assert _outcome(stn[1]) == _outcome(st1) == "breakdown"
    assert stz[1].converged                                              # (b = 0 from x0 = 1: an ordinary solve, x -> 0)
    for j in (0, 2):
        assert stn[j].converged
        np.testing.assert_array_equal(_bits(Xn[:, j]), _bits(Xz[:, j]))
        assert _summary(stn[j]) == _summary(stz[j])
        np.testing.assert_array_equal(_bits(hn[j]), _bits(hz[j]))
    X0 = np.ones((n, 3))
    X0[:, 1] = 0.0
    X, sts, hs, form = _solve_many(cm, ctx, A, Bz, X0=X0, **kw)
    assert form == 1
    assert _summary(sts[1]) == (0, 0, True, False) and sts[1].nrm0 == 0.0 and len(hs[1]) == 0
    np.testing.assert_array_equal(_bits(X[:, 1]), _bits(np.zeros(n)))
    _, st1, _ = _solve_one(cm, ctx, A, Bz[:, 1], x0=np.zeros(n), **kw)
    assert _summary(st1) == (0, 0, True, False) and st1.nrm0 == 0.0
    for j in (0, 2):                                                     # the neighbours iterate, to the same bits as before
        assert sts[j].converged and sts[j].iters > 0
        np.testing.assert_array_equal(_bits(X[:, j]), _bits(Xz[:, j]))
        np.testing.assert_array_equal(_bits(hs[j]), _bits(hz[j]))
