"""Several right-hand sides with ILU(0): the multi-column triangular solves (cudamat_solver_precond_apply_many, csrc/trsv.hip)
bit for bit against the single-column ones and against the oracle's substitutions, the preconditioned batched loop
(MANY_PRECOND = batched) against the oracle column by column, the independence of a column from the batch it is solved in,
freeze on exit per column, the column-by-column fall-backs, the form choice and the host-pointer entry point.
Run on the GPU box with:  python -m pytest tests -m gpu"""
import os

import numpy as np
import pytest

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


def _wide_levels(oracle):
    """12 500 rows whose factors have levels wider than the 2048 rows a single-workgroup launch takes: row i < 12000 has
    entries in columns i - 6000, i - 3000, i, i + 3000, i + 6000 (where they exist), which gives four levels of 3000 rows per
    factor; then a chain of 500 rows (one row per level) -- so one factor application launches k_trsm_level AND
    k_trsm_small_levels"""
    n, h, tail = 12500, 6000, 500
    rng = np.random.default_rng(17)
    rows = []
    for i in range(n):
        if i < 2 * h:
            cols = [c for c in (i - h, i - h // 2, i, i + h // 2, i + h) if 0 <= c < 2 * h]
        else:
            cols = [c for c in (i - 1, i, i + 1) if 2 * h - 1 <= c < n]
        rows.append(sorted(set(cols)))
    rp = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    ci = np.concatenate(rows).astype(np.int32)
    val = rng.uniform(-1.0, 1.0, len(ci))
    row_of = np.repeat(np.arange(n), np.diff(rp))
    val[ci == row_of] = 6.0 + rng.random(n)
    assert n - 2 * h == tail
    return oracle.Csr(n, rp, ci, val, n)


def _matrix(oracle, golden_dir, name):
    if name == "rand20000x50":
        return oracle.rand_rows(20000, 50, 0x5EED)
    if name == "poisson":
        return oracle.poisson5(120, 90, base=1)
    if name == "wide":
        return _wide_levels(oracle)
    return _load(oracle, golden_dir, name)


def _solve_many(cm, ctx, A, B, X0=None, ldb=None, ldx=None, prepare=None, **kw):
    n, k = B.shape
    ldb, ldx = ldb or n, ldx or n
    s = cm.Solver.from_host_csr(ctx, A.rowptr, A.colidx, A.val)
    try:
        if prepare:
            prepare(s)
        dB = _block(ctx, B, ldb)
        dX = _block(ctx, np.ones((n, k)) if X0 is None else X0, ldx)
        sts, form = s.solve_many(k, dB, ldb, dX, ldx, precond=cm.PRECOND_ILU0, **kw)
        X = _unblock(dX, n, k, ldx)
        hs = [s.history(col=j) for j in range(k)]
        return X, sts, hs, form
    finally:
        s.close()


# (c, scale) of the five solutions x* = scale (1 + sin(i c) + 0.1 noise_i) of the loop tests
STABLE = ((1.0, 1.0), (0.5, -1.0), (2.0, 1.0), (0.7, 2.0), (0.3, 1.0))


def _stable_xstars(n):
    """Five different solutions in the family of test_gpu_many_rhs._xstars (1 + sin(i c) plus its noise, scaled), kept after
    running the ORACLE ALONE on the CPU: with ILU(0), x0 = 1 and tol 1e-8, mat10000 needs 43-60 iterations and amplifies
    rounding -- for most (c, scale) the oracle's own count moves by 3-12 iterations when b changes by a few ulp (two roundings
    of the same x*), more than the +-10 % rule allows any implementation.  Of 56 candidates (14 values of c x scales 1, 2, -1,
    1/2) these five, and one more, kept their count under 7 perturbations of b by -8..13 ulp, and the five (43, 61, 47,
    57, 45 iterations) under 12 by -13..13 ulp; on mat900 (7-13 iterations at 1e-6 / 1e-8) every candidate does.  So all five columns are held to the rule."""
    noise = np.random.default_rng(0).random(n)
    i = np.arange(n)
    return np.stack([sc * (1.0 + np.sin(i * c) + 0.1 * noise) for c, sc in STABLE], axis=1)


def _check_against_oracle(oracle, A, vm, b, x, st, h, tol):
    """the tolerances of test_pbicgstab_ilu0_vs_oracle, per column"""
    xo, so, ho = oracle.pbicgstab(A, b, vm=vm, maxit=2000, tol=tol, want_hist=True)
    print("iters", st.iters, "oracle", so.iters, "half", st.half_exit, so.half_exit,
          "err", np.linalg.norm(x - xo) / np.linalg.norm(xo), "res", np.linalg.norm(b - oracle.spmv(A, x)) / so.nrm0)
    assert st.converged and so.converged
    assert abs(st.iters - so.iters) <= max(2, 0.1 * so.iters), (st.iters, so.iters)
    assert np.linalg.norm(x - xo) / np.linalg.norm(xo) <= 1e-5
    assert np.linalg.norm(b - oracle.spmv(A, x)) <= 10 * tol * so.nrm0
    k = min(len(h), 6)
    np.testing.assert_allclose(h[:k], ho[:k], rtol=1e-8)
    assert len(h) == 2 * st.iters + (1 if st.half_exit else 0)


# ------------------------------------------------------------------------------------------- 1. the kernels, bitwise
@pytest.mark.parametrize("name", ["mat900", "mat10000", "rand20000x50", "poisson", "wide"])
@pytest.mark.parametrize("config", ["default", "lds0", "lanes2", "lanes16", "lanes64"])
def test_precond_apply_many_is_the_single_column_solve(cm, ctx, oracle, golden_dir, name, config, sw):
    """column j of cudamat_solver_precond_apply_many == cudamat_solver_precond_apply of column j, bit for bit, for every batch
    width (nrhs 1..11: groups of 8, a short last group with padding columns), leading dimensions above n with NaN in the pad
    rows; and within the tolerance of test_ilu0_factors_and_trsv_vs_oracle of the oracle's substitutions.  Which kernels ran
    is asked of the library (Solver.trsm_kernel), not assumed: the LDS form where the block fits (mat900 up to 8 columns,
    mat10000 one), runs of narrow levels otherwise, one launch per level on the matrix with wide levels."""
    if config == "lds0":
        sw("TRSV_LDS", 0)
    elif config.startswith("lanes"):
        sw("TRSV_LANES", config[5:])
    A = _matrix(oracle, golden_dir, name)
    n = A.n
    vm = oracle.ilu0(A)
    rng = np.random.default_rng(5)
    s = cm.Solver.from_host_csr(ctx, A.rowptr, A.colidx, A.val)
    try:
        s.ilu0()
        names = {k: s.trsm_kernel(k) for k in (1, 2, 4, 8)}
        print(name, config, names)
        for k, nm in names.items():
            assert nm.startswith("L: ") and "; U: " in nm, nm
            if config.startswith("lanes"):
                assert nm.count("<%s, %d>" % (config[5:], k)) >= 2, nm
            if config == "lds0":
                assert "k_trsm_lds" not in nm, nm
        if name == "wide":
            for nm in names.values():
                assert "k_trsm_level<" in nm and "k_trsm_small_levels<" in nm and "k_trsm_lds" not in nm, nm
        if name in ("mat900", "mat10000", "poisson") and config == "lds0":
            for nm in names.values():
                assert nm.count("k_trsm_small_levels<") == 2 and "k_trsm_level<" not in nm, nm
        if name == "mat900" and config != "lds0":
            for nm in names.values():
                assert nm.count("k_trsm_lds<") == 2, nm
        if name == "mat10000" and config != "lds0":
            assert names[1].count("k_trsm_lds<") == 2, names[1]
            for k in (2, 4, 8):           # 10000 x K x 8 bytes do not fit the 128 KiB of the LDS form
                assert "k_trsm_lds" not in names[k] and names[k].count("k_trsm_small_levels<") == 2, names[k]
        for k in (1, 2, 3, 5, 8, 11):
            R = rng.standard_normal((n, k))
            ldin, ldout = n + 3, n + 5
            dIn, dOut = _block(ctx, R, ldin), _block(ctx, np.zeros((n, k)), ldout)
            s.precond_apply_many(k, dIn, ldin, dOut, ldout)
            Y = dOut.download().reshape(k, ldout)
            for j in range(k):
                dr, do = ctx.array(R[:, j]), ctx.empty(n)
                s.precond_apply(dr, do)
                np.testing.assert_array_equal(Y[j, :n], do.download())
                assert np.all(np.isnan(Y[j, n:]))                     # the pad rows of Out are not touched
                if j in (0, k - 1):
                    ref = oracle.trsv_upper(A, vm, oracle.trsv_lower_unit(A, vm, R[:, j]))
                    np.testing.assert_allclose(Y[j, :n], ref, rtol=1e-10, atol=1e-12)
                for q in (dr, do):
                    q.free()
            for q in (dIn, dOut):
                q.free()
        # In == Out is allowed (the block is staged through the interleaved buffers)
        R = rng.standard_normal((n, 3))
        d1, d2 = _block(ctx, R, n), ctx.empty(3 * n)
        s.precond_apply_many(3, d1, n, d2, n)
        s.precond_apply_many(3, d1, n, d1, n)
        np.testing.assert_array_equal(d1.download(), d2.download())
        s.precond_apply_many(0, None, n, None, n)                    # a no-op
    finally:
        s.close()


def test_precond_apply_many_needs_factors(cm, ctx, oracle, golden_dir):
    A = _load(oracle, golden_dir, "mat900")
    s = cm.Solver.from_host_csr(ctx, A.rowptr, A.colidx, A.val)
    try:
        d = ctx.empty(2 * A.n)
        with pytest.raises(cm.CudamatError) as e:
            s.precond_apply_many(2, d, A.n, d, A.n)
        assert e.value.code == 2
        s.ilu0()
        with pytest.raises(cm.CudamatError) as e:
            s.precond_apply_many(2, d, A.n - 1, d, A.n)
        assert e.value.code == 2
    finally:
        s.close()


# --------------------------------------------------------------------------------------------- 2. the loop vs the oracle
@pytest.mark.parametrize("name,tol", [("mat900", 1e-6), ("mat900", 1e-8), ("mat10000", 1e-8)])
def test_batched_ilu0_solve_vs_oracle(cm, ctx, oracle, golden_dir, name, tol, sw):
    """MANY_PRECOND = batched, 5 columns with different x*: every column against the oracle's restatement of
    bicgstab_lu_precond's loop with the tolerances of test_pbicgstab_ilu0_vs_oracle"""
    sw("MANY_PRECOND", "batched")
    A = _load(oracle, golden_dir, name)
    vm = oracle.ilu0(A)
    XS = _stable_xstars(A.n)
    B = np.stack([oracle.spmv(A, XS[:, j]) for j in range(5)], axis=1)
    X, sts, hs, form = _solve_many(cm, ctx, A, B, ldb=A.n + 7, ldx=A.n + 1, loop=cm.LOOP_PBICGSTAB, maxit=2000, tol=tol)
    assert form == 1
    nl, nu = oracle.levels(A, upper=False)[0], oracle.levels(A, upper=True)[0]
    for j in range(5):
        _check_against_oracle(oracle, A, vm, B[:, j], X[:, j], sts[j], hs[j], tol)
        assert (sts[j].n_levels_l, sts[j].n_levels_u, sts[j].trsv_fallbacks) == (nl, nu, 0)
        assert hs[j][-1] < tol * sts[j].nrm0 and np.all(hs[j][:-1] >= tol * sts[j].nrm0)


# ----------------------------------------------------------------------------------- 3. a column and the batch it sits in
@pytest.mark.parametrize("name", ["mat900", "mat10000"])
def test_column_does_not_depend_on_its_batch(cm, ctx, oracle, golden_dir, name, sw):
    """bitwise: the same column solved alone (nrhs = 1), as one of 8, and as the 9th of 11 (first column of a short second
    group): x, history and iteration count.  On mat10000 the three runs go through different kernels (LDS form at one column,
    runs of narrow levels at eight and at four)."""
    sw("MANY_PRECOND", "batched")
    A = _load(oracle, golden_dir, name)
    n = A.n
    rng = np.random.default_rng(12)
    XS = 1.0 + np.sin(np.outer(np.arange(n), 0.1 + rng.random(11))) + 0.1 * rng.random((n, 11))
    B = np.stack([oracle.spmv(A, XS[:, j]) for j in range(11)], axis=1)
    X0 = np.cos(np.arange(n))[:, None] * (1.0 + np.arange(11))[None, :]
    kw = dict(loop=cm.LOOP_PBICGSTAB, maxit=2000, tol=1e-9)
    X, sts, hs, form = _solve_many(cm, ctx, A, B, X0=X0, **kw)
    assert form == 1 and all(st.converged for st in sts)
    c = 8                                                         # the 9th of 11
    X8, st8, h8, f8 = _solve_many(cm, ctx, A, B[:, c - 7:c + 1], X0=X0[:, c - 7:c + 1], **kw)      # the last of 8
    X1, st1, h1, f1 = _solve_many(cm, ctx, A, B[:, c:c + 1], X0=X0[:, c:c + 1], **kw)              # alone
    assert f8 == 1 and f1 == 1
    for Xq, stq, hq, q in ((X8, st8, h8, 7), (X1, st1, h1, 0)):
        np.testing.assert_array_equal(Xq[:, q], X[:, c])
        np.testing.assert_array_equal(hq[q], hs[c])
        assert (stq[q].iters, stq[q].half_exit, stq[q].converged) == (sts[c].iters, sts[c].half_exit, sts[c].converged)
    # every column of the group of 8, too
    for q in range(8):
        np.testing.assert_array_equal(X8[:, q], X[:, c - 7 + q])
        np.testing.assert_array_equal(h8[q], hs[c - 7 + q])


# ------------------------------------------------------------------------------------------------------ 4. freeze on exit
def test_freeze_and_half_step_exits(cm, ctx, oracle, golden_dir, sw):
    """a column started at the exact solution (b = A x0 by the library's own SpMM: r0 = 0, stops at once) beside columns that
    iterate: its x keeps its bits, and equals what it is when solved alone.  Columns that leave through the half step (they owe
    x += alpha M^-1 p after the loop, with the M^-1 p of THEIR last iteration) equal their runs alone bit for bit although
    the batch went on iterating for other columns.  Cutting maxit at the fastest column's exit leaves its x bit-identical."""
    sw("MANY_PRECOND", "batched")
    A = _load(oracle, golden_dir, "mat900")
    n = A.n
    XS = np.concatenate([_stable_xstars(n), 3.0 * _stable_xstars(n)[:, :3]], axis=1)       # 8 columns
    k = XS.shape[1]
    s = cm.Solver.from_host_csr(ctx, A.rowptr, A.colidx, A.val)
    try:
        dXS, dB = _block(ctx, XS, n), ctx.empty(k * n)
        s.spmm(k, dXS, n, dB, n)
        B = dB.download().reshape(k, n).T.copy()
    finally:
        s.close()
    X0 = np.ones((n, k))
    X0[:, 1] = XS[:, 1]
    tols = dict(loop=cm.LOOP_PBICGSTAB, tol=1e-6)
    X, sts, hs, form = _solve_many(cm, ctx, A, B, X0=X0, maxit=2000, **tols)
    assert form == 1 and all(st.converged for st in sts)
    assert sts[1].iters == 0 and sts[1].nrm0 == 0.0
    np.testing.assert_array_equal(X[:, 1], XS[:, 1])
    its = [sts[j].iters + sts[j].half_exit for j in range(k) if j != 1]
    assert len(set(its)) > 1, its                                   # the columns stop at different iterations
    halves = [j for j in range(k) if sts[j].half_exit]
    early_halves = [j for j in halves if sts[j].iters + 1 < max(its)]
    assert early_halves, (halves, its)                              # a half-step exit while the batch goes on (oracle: most columns)
    for j in [1] + halves:
        X1, st1, h1, f1 = _solve_many(cm, ctx, A, B[:, j:j + 1], X0=X0[:, j:j + 1], maxit=2000, **tols)
        assert f1 == 1
        np.testing.assert_array_equal(X1[:, 0], X[:, j])
        np.testing.assert_array_equal(h1[0], hs[j])
        assert (st1[0].iters, st1[0].half_exit) == (sts[j].iters, sts[j].half_exit)
    cut, fast = min((sts[j].iters + sts[j].half_exit, j) for j in range(k) if j != 1)
    Xc, stc, _, _ = _solve_many(cm, ctx, A, B, X0=X0, maxit=cut, **tols)
    np.testing.assert_array_equal(Xc[:, fast], X[:, fast])
    np.testing.assert_array_equal(Xc[:, 1], X[:, 1])
    for j in range(k):
        if sts[j].iters + sts[j].half_exit <= cut:
            assert (stc[j].iters, stc[j].half_exit, stc[j].converged) == (sts[j].iters, sts[j].half_exit, sts[j].converged)
        else:
            assert not stc[j].converged and stc[j].iters == cut


# ----------------------------------------------------------------------------------------------------------- 5. fall-backs
def _columns_are_single_solves(cm, ctx, A, B, precond, loop, prepare=None):
    n, k = B.shape
    kw = dict(loop=loop, maxit=2000, tol=1e-8)
    s = cm.Solver.from_host_csr(ctx, A.rowptr, A.colidx, A.val)
    try:
        if prepare:
            prepare(s)
        dB, dX = _block(ctx, B, n), _block(ctx, np.ones((n, k)), n)
        sts, form = s.solve_many(k, dB, n, dX, n, precond=precond, **kw)
        X = _unblock(dX, n, k, n)
        assert form == 0
        for j in range(k):
            h_many = s.history(col=j)
            db, dx = ctx.array(B[:, j]), ctx.array(np.ones(n))
            st = s.solve(db, dx, precond=precond, **kw)
            np.testing.assert_array_equal(X[:, j], dx.download())
            np.testing.assert_array_equal(h_many, s.history())
            assert st.iters == sts[j].iters and sts[j].converged
        return s.trsm_kernel(k) if precond == cm.PRECOND_ILU0 else None
    finally:
        s.close()


def test_default_is_still_column_by_column(cm, ctx, oracle, golden_dir):
    """default switches (MANY_PRECOND = columns): ILU(0) through solve_many reports form 0 and is bitwise Solver.solve per
    column -- the pin of test_gpu_many_rhs.test_fallback_is_the_single_solve, restated"""
    A = _load(oracle, golden_dir, "mat900")
    XS = _stable_xstars(A.n)[:, :3]
    B = np.stack([oracle.spmv(A, XS[:, j]) for j in range(3)], axis=1)
    _columns_are_single_solves(cm, ctx, A, B, cm.PRECOND_ILU0, cm.LOOP_PBICGSTAB)
    _columns_are_single_solves(cm, ctx, A, B, cm.PRECOND_ILU0, cm.LOOP_PBICGSTAB, prepare=lambda s: s.ilu0())


@pytest.mark.parametrize("case", ["hybrid", "block_ilu0", "pipelined", "many_form_columns"])
def test_batched_switch_falls_back_where_not_covered(cm, ctx, oracle, golden_dir, case, sw):
    """MANY_PRECOND = batched on what the multi-column solves do not cover: hybrid factors in level-major spaces
    (TRSV_HYBRID = 1 on mat10000), block-Jacobi ILU(0), the pipelined loop; and MANY_FORM = columns wins over it.  form 0,
    answers bitwise the single solve's."""
    sw("MANY_PRECOND", "batched")
    A = _load(oracle, golden_dir, "mat10000" if case == "hybrid" else "mat900")
    XS = _stable_xstars(A.n)[:, :3]
    B = np.stack([oracle.spmv(A, XS[:, j]) for j in range(3)], axis=1)
    if case == "hybrid":
        sw("TRSV_HYBRID", 1)
        name = _columns_are_single_solves(cm, ctx, A, B, cm.PRECOND_ILU0, cm.LOOP_PBICGSTAB)
        assert name == ""                                          # level-major factors: no multi-column kernels
    elif case == "block_ilu0":
        _columns_are_single_solves(cm, ctx, A, B, cm.PRECOND_BLOCK_ILU0, cm.LOOP_PBICGSTAB)
    elif case == "pipelined":
        _columns_are_single_solves(cm, ctx, A, B, cm.PRECOND_ILU0, cm.LOOP_PIPELINED)
    else:
        sw("MANY_FORM", "columns")
        name = _columns_are_single_solves(cm, ctx, A, B, cm.PRECOND_ILU0, cm.LOOP_PBICGSTAB)
        assert name != ""                                          # covered, but switched off


def test_shift_with_preconditioner_stays_an_argument_error(cm, ctx, oracle, golden_dir, sw):
    """the (A0 + I d) variant has no preconditioner: CUDAMAT_ERR_ARG under either switch"""
    A = _load(oracle, golden_dir, "mat900")
    for mode in ("columns", "batched"):
        sw("MANY_PRECOND", mode)
        with pytest.raises(cm.CudamatError) as e:
            _solve_many(cm, ctx, A, np.ones((A.n, 2)), prepare=lambda s: s.set_shift(ctx.array(np.ones(A.n))),
                        loop=cm.LOOP_PBICGSTAB, maxit=10, tol=1e-8)
        assert e.value.code == 2


# ------------------------------------------------------------------------------------------------------------------ 6. auto
def test_auto_form_is_a_valid_choice(cm, ctx, oracle, golden_dir, sw):
    """MANY_PRECOND = auto: whichever form the timing picks, the answers hold to the oracle's tolerances"""
    sw("MANY_PRECOND", "auto")
    A = _load(oracle, golden_dir, "mat10000")
    vm = oracle.ilu0(A)
    XS = _stable_xstars(A.n)[:, :4]
    B = np.stack([oracle.spmv(A, XS[:, j]) for j in range(4)], axis=1)
    X, sts, hs, form = _solve_many(cm, ctx, A, B, loop=cm.LOOP_PBICGSTAB, maxit=2000, tol=1e-8)
    print("auto picked form", form, "t_tune", sts[0].t_tune)
    assert form in (0, 1)
    for j in range(4):
        assert sts[j].t_tune >= 0.0
        _check_against_oracle(oracle, A, vm, B[:, j], X[:, j], sts[j], hs[j], 1e-8)


# --------------------------------------------------------------------------------------------------------------- 7. drop-in
@pytest.mark.parametrize("mode", ["batched", "columns"])
def test_bicgstab_lu_precond_many_drop_in(cm, oracle, golden_dir, mode, monkeypatch):
    """api.bicgstab_lu_precond_many / cudamat_solve_many with ILU(0) on mat10000 with 4 columns against bicgstab_lu_precond
    per column: bitwise with MANY_PRECOND = columns, the oracle's tolerances with batched; the second call with the same
    matrix reuses the plan"""
    monkeypatch.setenv("CUDAMAT_MANY_PRECOND", mode)
    A = _load(oracle, golden_dir, "mat10000")
    n, nnz = A.n, A.nnz
    vm = oracle.ilu0(A)
    XS = _stable_xstars(n)[:, :4]
    B = np.stack([oracle.spmv(A, XS[:, j]) for j in range(4)], axis=1)
    ok, X, dt, sts, form = cm.bicgstab_lu_precond_many(n, nnz, A.val, A.rowptr, A.colidx, B, 2000, 1e-8)
    assert form == (1 if mode == "batched" else 0)
    assert ok == [True] * 4 and X.shape == (n, 4)
    for j in range(4):
        ok1, x1, _, st1 = cm.bicgstab_lu_precond(n, nnz, A.val, A.rowptr, A.colidx, B[:, j], 2000, 1e-8)
        assert ok1 and st1.converged
        if mode == "columns":
            np.testing.assert_array_equal(X[:, j], x1)
            assert sts[j].iters == st1.iters
        else:
            xo, so, ho = oracle.pbicgstab(A, B[:, j], vm=vm, maxit=2000, tol=1e-8, want_hist=True)
            print("col", j, "iters", sts[j].iters, "single", st1.iters, "oracle", so.iters)
            assert sts[j].converged and abs(sts[j].iters - so.iters) <= max(2, 0.1 * so.iters)
            assert np.linalg.norm(X[:, j] - xo) / np.linalg.norm(xo) <= 1e-5
            assert np.linalg.norm(B[:, j] - oracle.spmv(A, X[:, j])) <= 10 * 1e-8 * so.nrm0
            assert sts[j].n_levels_l == 199
    ok2, X2, _, sts2, form2 = cm.bicgstab_lu_precond_many(n, nnz, A.val, A.rowptr, A.colidx, B, 2000, 1e-8)
    assert all(s.plan_reused == 1 for s in sts2) and form2 == form
    np.testing.assert_array_equal(X2, X)
    ok3, X3, _, sts3, _ = cm.bicgstab_lu_precond_many(n, nnz, A.val, A.rowptr, A.colidx, B, 2, 1e-8)
    assert ok3 == [True] * 4 and not any(s.converged for s in sts3)       # `ok` says the solve ran (pbicgstab.cu:408)
    cm.lib().cudamat_plan_cache_clear()


# ---------------------------------------------------------------------------------------------------- 8. a missing diagonal
def test_missing_diagonal_fails_like_ilu0(cm, ctx, oracle, golden_dir, sw):
    """mat3 has no (2, 2) entry (violates pbicgstab.h:118): the batched call fails as Solver.ilu0() does, leaves nothing
    behind, and a well-formed call on a fresh solver succeeds afterwards"""
    sw("MANY_PRECOND", "batched")
    A3 = _load(oracle, golden_dir, "mat3")
    s = cm.Solver.from_host_csr(ctx, A3.rowptr, A3.colidx, A3.val)
    try:
        with pytest.raises(cm.CudamatError) as e0:
            s.ilu0()
        dB, dX = ctx.array(np.ones(6)), ctx.array(np.ones(6))
        with pytest.raises(cm.CudamatError) as e:
            s.solve_many(2, dB, 3, dX, 3, precond=cm.PRECOND_ILU0, loop=cm.LOOP_PBICGSTAB, maxit=10, tol=1e-8)
        assert e.value.code == e0.value.code == 3
        np.testing.assert_array_equal(dX.download(), np.ones(6))      # nothing was written
        with pytest.raises(cm.CudamatError):
            s.precond_apply_many(2, dB, 3, dX, 3)                      # no factors were left behind
    finally:
        s.close()
    A = _load(oracle, golden_dir, "mat900")
    B = oracle.spmv(A, _stable_xstars(A.n)[:, 0])[:, None] * np.array([1.0, 2.0])[None, :]
    X, sts, _, form = _solve_many(cm, ctx, A, B, loop=cm.LOOP_PBICGSTAB, maxit=2000, tol=1e-8)
    assert form == 1 and all(st.converged for st in sts)
    for j in range(2):
        assert np.linalg.norm(B[:, j] - oracle.spmv(A, X[:, j])) <= 10 * 1e-8 * sts[j].nrm0
