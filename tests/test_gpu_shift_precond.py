"""ILU(0)-preconditioned solves of (A0 + I d) on the GPU (cudamat_solver_ilu0_shift, Solver.ilu0(shift=...), bicgstab_d_lu_precond;
DESIGN.md sections 3, 9 and 10):
 1. the factors of A0 + diag(d) and their application against the oracle's ILU(0) of the explicit matrix;
 2. the five-launch preconditioned loop with a shift against the CPU mirror of test_shift_precond_cpu.py, bit for bit;
 3. parity with the oracle on the explicit matrix: the resident solver, the drop-in function, stale factors;
 4. hybrid (level-major) factors with a shift: TRSV_PERM = 1 against TRSV_PERM = 0 and the oracle;
 5. FLAG_GUARD on top;
 6. what stays refused, and the drop-in call's plan cache.
Run on the GPU box with:  python -m pytest tests -m gpu"""
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OLD_MESSAGE = "has no preconditioner"


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


# ------------------------------------------------------------------ systems
def _diag_mask(A):
    rows = np.repeat(np.arange(A.n), np.diff(A.rowptr))
    mask = (A.colidx - A.base) == rows
    assert int(mask.sum()) == A.n
    return rows, mask


def _explicit(oracle, A0, d):
    """A0 + diag(d) as a matrix of its own: one add per diagonal entry"""
    rows, mask = _diag_mask(A0)
    val = A0.val.copy()
    val[mask] = val[mask] + d[rows[mask]]
    return oracle.Csr(A0.n, A0.rowptr.copy(), A0.colidx.copy(), val, A0.n)


def _ramp(n):
    return 0.5 + np.arange(n) / n


@functools.lru_cache(maxsize=None)
def _reference(oracle, golden_dir, name, mult=1.0):
    """(A0, d, E, b, xo, so, ho): name with d = mult * (0.5 + i / n), b = E (1 + sin i), the oracle's ILU(0) solve of the explicit
    matrix from x0 = 1.  Computed once, shared between tests, not to be written."""
    A0 = oracle.mtx_load(os.path.join(golden_dir, name + ".mtx"))
    d = mult * _ramp(A0.n)
    E = _explicit(oracle, A0, d)
    b = oracle.spmv(E, 1.0 + np.sin(np.arange(A0.n)))
    xo, so, ho = oracle.pbicgstab(E, b, vm=oracle.ilu0(E), maxit=2000, tol=1e-8, want_hist=True)
    for arr in (d, b, xo, ho):
        arr.setflags(write=False)
    return A0, d, E, b, xo, so, ho


def _solve(cm, ctx, s, b, x0, off=0, **kw):
    """solve on device copies of b and x0 that start `off` doubles past a 16-byte boundary: (stats, x, history)"""
    db, dx = ctx.array(np.concatenate([np.zeros(off), b])), ctx.array(np.concatenate([np.zeros(off), x0]))
    try:
        st = s.solve(db.ptr + 8 * off, dx.ptr + 8 * off, **kw)
        return st, dx.download()[off:], s.history()
    finally:
        db.free()
        dx.free()


def _shifted_solver(cm, ctx, A0, d_solver, d_factor):
    """a resident solver on A0 with the shift d_solver and the factors of A0 + diag(d_factor) (None: no factors)"""
    s = cm.Solver.from_host_csr(ctx, A0.rowptr, A0.colidx, A0.val)
    if d_solver is not None:
        s.set_shift(ctx.array(d_solver))
    if d_factor is not None:
        df = ctx.array(d_factor)
        s.ilu0(shift=df)
        df.free()                       # read during the call only
    return s


# ------------------------------------------------------------------ 1. factors
@pytest.mark.parametrize("system", ["ramp", "moved"])
def test_factors_of_the_shifted_matrix(cm, ctx, oracle, golden_dir, system):
    """mat900 (base 1) with d_i = 0.5 + i / n, and mat900 with its whole diagonal moved into d (A0 holds explicit zeros there):
    ilu0_values() after ilu0(shift=d) against the oracle's ILU(0) of the explicit matrix (rtol 1e-12), precond_apply against the
    oracle's substitutions with those factors (1e-10) -- the tolerances of test_ilu0_factors_and_trsv_vs_oracle.  On the moved
    diagonal plain ilu0() is a zero pivot (code 3) and ilu0(shift=d) succeeds; a second call starts over."""
    A = oracle.mtx_load(os.path.join(golden_dir, "mat900.mtx"))
    assert A.base == 1
    if system == "ramp":
        A0, d = A, _ramp(A.n)
        E = _explicit(oracle, A0, d)
    else:
        rows, mask = _diag_mask(A)
        d = np.zeros(A.n)
        d[rows[mask]] = A.val[mask]
        val = A.val.copy()
        val[mask] = 0.0
        A0, E = oracle.Csr(A.n, A.rowptr.copy(), A.colidx.copy(), val, A.n), A
        np.testing.assert_array_equal(_explicit(oracle, A0, d).val, A.val)
    s = cm.Solver.from_host_csr(ctx, A0.rowptr, A0.colidx, A0.val)
    dd = ctx.array(d)
    try:
        assert s.ilu0_shifted() is False
        if system == "moved":
            with pytest.raises(cm.CudamatError) as e:
                s.ilu0()
            assert e.value.code == 3
            assert s.ilu0_shifted() is False
        s.ilu0(shift=dd)
        assert s.ilu0_shifted() is True
        want = oracle.ilu0(E)
        np.testing.assert_allclose(s.ilu0_values(), want, rtol=1e-12, atol=1e-14)
        rhs = np.random.default_rng(0).standard_normal(A.n)
        dr, do = ctx.array(rhs), ctx.empty(A.n)
        s.precond_apply(dr, do)
        ref = oracle.trsv_upper(E, want, oracle.trsv_lower_unit(E, want, rhs))
        np.testing.assert_allclose(do.download(), ref, rtol=1e-10, atol=1e-12)
        if system == "ramp":            # a second call starts the set-up over: the factors of A0 alone, and shift=None means just that
            s.ilu0(shift=None)
            assert s.ilu0_shifted() is False
            np.testing.assert_allclose(s.ilu0_values(), oracle.ilu0(A0), rtol=1e-12, atol=1e-14)
            assert not np.allclose(s.ilu0_values(), want, rtol=1e-6)
        dr.free()
        do.free()
    finally:
        dd.free()
        s.close()


# ------------------------------------------------------------------ 2. bits against the mirror
@pytest.mark.parametrize("case", ["exact", "stale"])
@pytest.mark.parametrize("layout", ["aligned", "offset8"])
def test_shift_precond_bits(cm, ctx, sw, layout, case):
    """the n = 601 diagonal system of test_loop_rounding.py (SPMV_MODE = csr, SPMV_LANES = 64: the plan the mirror restates), b and
    x 16-byte aligned and 8 bytes off, the solver's shift shift_of(N):
      exact   factors of the same shift, solved to 1e-8: M is A up to the rounding of 1 / (a_i + d_i), a half-step exit at
              iteration 0;
      stale   factors of half that shift, FLAG_NO_EXIT, ITERS iterations.
    x and the history equal the mirror of test_shift_precond_cpu.py bit for bit."""
    import test_loop_rounding as L
    import test_shift_precond_cpu as P
    a, b, x0 = L.system(P.LAYOUT_COL[layout])
    d = L.shift_of(L.N)
    for name, value in (("SPMV_MODE", "csr"), ("SPMV_LANES", L.LANES)):
        sw(name, value)
    A0 = type("Diag", (), dict(rowptr=np.arange(L.N + 1), colidx=np.arange(L.N), val=a))
    d_f = d if case == "exact" else 0.5 * d
    s = _shifted_solver(cm, ctx, A0, d, d_f)
    try:
        assert s.spmv_kernel().startswith("k_spmv<64>")
        np.testing.assert_array_equal(s.ilu0_values(), a + d_f)                  # one add, one rounding
        off = 1 if layout == "offset8" else 0
        if case == "exact":
            want = P.pinned_exact(layout)
            st, x, h = _solve(cm, ctx, s, b, x0, off=off, precond=cm.PRECOND_ILU0, loop=cm.LOOP_PBICGSTAB, maxit=20, tol=P.TOL)
            assert (bool(st.half_exit), bool(st.converged)) == (True, True) and want.half_exit and want.iters == 0
        else:
            want = P.pinned_stale(layout)
            st, x, h = _solve(cm, ctx, s, b, x0, off=off, precond=cm.PRECOND_ILU0, loop=cm.LOOP_PBICGSTAB, maxit=L.ITERS, tol=P.TOL,
                              flags=cm.FLAG_NO_EXIT)
    finally:
        s.close()
    print(layout, case, "iters", st.iters, "entries of x that differ:", L.differing(x, want.x), "history", h, want.history)
    assert (st.iters, st.loop_form, st.breakdown) == (want.iters, 0, 0)
    np.testing.assert_array_equal(h, want.history)
    np.testing.assert_array_equal(x, want.x)


# ------------------------------------------------------------------ 3. parity with the oracle
@pytest.mark.parametrize("name", ["mat900", "mat10000"])
def test_shifted_ilu0_solve_vs_oracle(cm, ctx, oracle, golden_dir, name):
    """d_i = 0.5 + i / n, x0 = 1, tol 1e-8, maxit 2000, through the resident solver and through bicgstab_d_lu_precond, against the
    oracle's ILU(0) loop on the explicit matrix: iterations within max(2, 10 %), x to 1e-5, true residual (the d x term
    included) <= 1e-7 ||r0||; fewer iterations than the un-preconditioned d-loop on the GPU (the oracle: 4 against 17, 5 against
    20).  Stale factors -- built with d, solving with 2 d -- converge to the same residual bound."""
    A0, d, E, b, xo, so, ho = _reference(oracle, golden_dir, name)
    n, ones = A0.n, np.ones(A0.n)
    assert so.converged
    s = _shifted_solver(cm, ctx, A0, d, d)
    try:
        st, x, h = _solve(cm, ctx, s, b, ones, precond=cm.PRECOND_ILU0, loop=cm.LOOP_PBICGSTAB, maxit=2000, tol=1e-8)
        stn, xn, hn = _solve(cm, ctx, s, b, ones, precond=cm.PRECOND_NONE, loop=cm.LOOP_PBICGSTAB2, maxit=2000, tol=1e-8)
        # stale factors: the solver's shift becomes 2 d, the factors stay those of d
        d2 = 2.0 * d
        E2 = _explicit(oracle, A0, d2)
        b2 = oracle.spmv(E2, 1.0 + np.sin(np.arange(n)))
        s.set_shift(ctx.array(d2))
        assert s.ilu0_shifted() is True
        st2, x2, h2 = _solve(cm, ctx, s, b2, ones, precond=cm.PRECOND_ILU0, loop=cm.LOOP_PBICGSTAB, maxit=2000, tol=1e-8)
        stn2, _, _ = _solve(cm, ctx, s, b2, ones, precond=cm.PRECOND_NONE, loop=cm.LOOP_PBICGSTAB2, maxit=2000, tol=1e-8)
    finally:
        s.close()
    res = np.linalg.norm(b - oracle.spmv(E, x))
    print(name, "resident: iters", st.iters, "oracle", so.iters, "un-preconditioned", stn.iters, "residual / nrm0", res / so.nrm0,
          "| stale: iters", st2.iters, "un-preconditioned", stn2.iters)
    assert st.converged and st.loop_form == 0 and abs(st.iters - so.iters) <= max(2, 0.1 * so.iters)
    assert abs(st.nrm0 - so.nrm0) <= 1e-12 * so.nrm0
    assert np.linalg.norm(x - xo) / np.linalg.norm(xo) <= 1e-5
    assert res <= 1e-7 * so.nrm0
    assert stn.converged and st.iters < stn.iters
    assert st2.converged and np.linalg.norm(b2 - oracle.spmv(E2, x2)) <= 1e-7 * st2.nrm0
    assert stn2.converged and st2.iters < stn2.iters
    # the drop-in function
    cm.lib().cudamat_plan_cache_clear()
    ok, xd, dt, std = cm.bicgstab_d_lu_precond(n, A0.nnz, A0.val, A0.rowptr, A0.colidx, d, ones, b, 2000, 1e-8)
    cm.lib().cudamat_plan_cache_clear()
    assert ok is True and std.converged and abs(std.iters - so.iters) <= max(2, 0.1 * so.iters)
    assert np.linalg.norm(xd - xo) / np.linalg.norm(xo) <= 1e-5
    assert np.linalg.norm(b - oracle.spmv(E, xd)) <= 1e-7 * so.nrm0


# ------------------------------------------------------------------ 4. level-major factors
@pytest.mark.parametrize("name", ["rand20000x50", "mat10000"])
def test_level_major_factors_with_a_shift(cm, ctx, oracle, golden_dir, name, sw, capfd):
    """hybrid factors (TRSV_HYBRID = 1) and a shift of 0.25 mean|diag| (0.5 + i / n): TRSV_PERM = 1 against TRSV_PERM = 0 by the
    rules of test_loop_in_level_major_spaces_matches_the_permuting_loop (iterations +-1, x to 1e-9, the first history entries to
    1e-8), and both against the oracle on the explicit matrix.  With TRSV_PERM = 1 the loop does run in the level-major spaces
    (VERBOSE = 1: the solve builds the permuted copy of the matrix and says so), with TRSV_PERM = 0 it does not.
    On the level-major loop also: FLAG_GUARD (every segment permutes b and x and gathers d anew) gives the unguarded run's x and
    history bit for bit without a restart; and PB_DEPTH = 8, a depth the kernels with the index map are not built for (they run
    with 4), gives the bits of the depth the plan has by its shape."""
    sw("TRSV_HYBRID", "1")
    sw("VERBOSE", 1)
    A0 = oracle.rand_rows(20000, 50, 0x5EED) if name == "rand20000x50" else oracle.mtx_load(os.path.join(golden_dir, name + ".mtx"))
    n = A0.n
    rows, mask = _diag_mask(A0)
    d = 0.25 * np.abs(A0.val[mask]).mean() * _ramp(n)
    E = _explicit(oracle, A0, d)
    b = oracle.spmv(E, 1.0 + np.sin(np.arange(n)))
    x0 = 1.0 + 0.25 * np.cos(np.arange(n))
    xo, so, ho = oracle.pbicgstab(E, b, x0=x0, vm=oracle.ilu0(E), maxit=500, tol=1e-8, want_hist=True)
    res = {}
    for perm in ("1", "0"):
        sw("TRSV_PERM", perm)
        s = _shifted_solver(cm, ctx, A0, d, d)
        try:
            capfd.readouterr()
            res[perm] = _solve(cm, ctx, s, b, x0, precond=cm.PRECOND_ILU0, loop=cm.LOOP_PBICGSTAB, maxit=500, tol=1e-8)
            assert ("ilu0 permuted matrix" in capfd.readouterr().err) == (perm == "1")
            assert res[perm][0].trsv_groups_l > 0 and res[perm][0].trsv_groups_u > 0           # the factors are split: level-major
            if perm == "1":
                stg, xg, hg = _solve(cm, ctx, s, b, x0, precond=cm.PRECOND_ILU0, loop=cm.LOOP_PBICGSTAB, maxit=500, tol=1e-8,
                                     flags=cm.FLAG_GUARD)
        finally:
            s.close()
        if perm == "1":
            st1, x1, h1 = res["1"]
            assert (stg.converged, stg.rho_restarts, stg.restarts, stg.breakdown) == (1, 0, 0, 0)
            assert (stg.iters, stg.half_exit, stg.nrm0) == (st1.iters, st1.half_exit, st1.nrm0)
            np.testing.assert_array_equal(hg, h1)
            np.testing.assert_array_equal(xg, x1)
    (st1, x1, h1), (st0, x0_, h0) = res["1"], res["0"]
    print(name, "iters perm", st1.iters, "no perm", st0.iters, "oracle", so.iters)
    assert st1.converged and st0.converged and abs(st1.iters - st0.iters) <= 1
    assert np.linalg.norm(x1 - x0_) / np.linalg.norm(x0_) <= 1e-9
    k = min(len(h1), len(h0), 6)
    np.testing.assert_allclose(h1[:k], h0[:k], rtol=1e-8)
    for st, x, h in (res["1"], res["0"]):
        np.testing.assert_allclose(h[:k], ho[:k], rtol=1e-8)
        assert abs(st.iters - so.iters) <= max(2, 0.1 * so.iters)
        assert np.linalg.norm(x - xo) / np.linalg.norm(xo) <= 1e-5
        assert np.linalg.norm(b - oracle.spmv(E, x)) <= 1e-7 * st.nrm0
    sw("TRSV_PERM", "1")
    sw("PB_DEPTH", 8)
    s = _shifted_solver(cm, ctx, A0, d, d)
    try:
        st8, x8, h8 = _solve(cm, ctx, s, b, x0, precond=cm.PRECOND_ILU0, loop=cm.LOOP_PBICGSTAB, maxit=500, tol=1e-8)
    finally:
        s.close()
    assert st8.iters == st1.iters
    np.testing.assert_array_equal(h8, h1)
    np.testing.assert_array_equal(x8, x1)


# ------------------------------------------------------------------ 5. the guard on top
def test_guard_on_a_shifted_preconditioned_solve(cm, ctx, oracle, golden_dir):
    """FLAG_GUARD on the mat900 system of section 3: x, history and iters of the unguarded five-launch run, bit for bit; no
    restart of either kind"""
    A0, d, E, b, xo, so, ho = _reference(oracle, golden_dir, "mat900")
    ones = np.ones(A0.n)
    s = _shifted_solver(cm, ctx, A0, d, d)
    try:
        st0, xa, ha = _solve(cm, ctx, s, b, ones, precond=cm.PRECOND_ILU0, loop=cm.LOOP_PBICGSTAB, maxit=2000, tol=1e-8)
        st1, xb, hb = _solve(cm, ctx, s, b, ones, precond=cm.PRECOND_ILU0, loop=cm.LOOP_PBICGSTAB, maxit=2000, tol=1e-8, flags=cm.FLAG_GUARD)
    finally:
        s.close()
    assert (st0.converged, st0.loop_form) == (1, 0)
    assert (st1.converged, st1.loop_form, st1.rho_restarts, st1.restarts, st1.breakdown) == (1, 0, 0, 0, 0)
    assert (st1.iters, st1.half_exit, st1.nrm0) == (st0.iters, st0.half_exit, st0.nrm0)
    np.testing.assert_array_equal(hb, ha)
    np.testing.assert_array_equal(xb, xa)
    assert np.linalg.norm(b - oracle.spmv(E, xb)) <= 1e-7 * st1.nrm0


# ------------------------------------------------------------------ 6. refusals and the plan cache
def test_what_stays_refused(cm, ctx, oracle, golden_dir, sw):
    """a shift with no factors, and a shift with the factors of A0 alone, are CUDAMAT_ERR_ARG with the old message -- and A0 is not
    factored on the way; the pipelined loop with a preconditioner and a shift is CUDAMAT_ERR_ARG even with shifted factors, and so
    is solve_many under every MANY_PRECOND setting, both loops and with the guard (batched or column by column alike)"""
    A0, d, E, b, xo, so, ho = _reference(oracle, golden_dir, "mat900")
    ones = np.ones(A0.n)
    s = _shifted_solver(cm, ctx, A0, d, None)
    try:
        for loop in (cm.LOOP_PBICGSTAB, cm.LOOP_PBICGSTAB2, cm.LOOP_PIPELINED):
            with pytest.raises(cm.CudamatError) as e:
                _solve(cm, ctx, s, b, ones, precond=cm.PRECOND_ILU0, loop=loop, maxit=5, tol=1e-8)
            assert e.value.code == 2 and OLD_MESSAGE in str(e.value)
        assert s.ilu0_shifted() is False
        with pytest.raises(cm.CudamatError) as e:               # nothing was factored silently
            s.ilu0_values()
        assert e.value.code == 2
        s.ilu0()
        with pytest.raises(cm.CudamatError) as e:
            _solve(cm, ctx, s, b, ones, precond=cm.PRECOND_ILU0, loop=cm.LOOP_PBICGSTAB, maxit=5, tol=1e-8)
        assert e.value.code == 2 and OLD_MESSAGE in str(e.value)
        assert s.ilu0_shifted() is False
        np.testing.assert_allclose(s.ilu0_values(), oracle.ilu0(A0), rtol=1e-12, atol=1e-14)      # ... and nothing was replaced
        dd = ctx.array(d)
        s.ilu0(shift=dd)
        dd.free()
        with pytest.raises(cm.CudamatError) as e:
            _solve(cm, ctx, s, b, ones, precond=cm.PRECOND_ILU0, loop=cm.LOOP_PIPELINED, maxit=5, tol=1e-8)
        assert e.value.code == 2
        with pytest.raises(cm.CudamatError) as e:
            _solve(cm, ctx, s, b, ones, precond=cm.PRECOND_BLOCK_ILU0, loop=cm.LOOP_PBICGSTAB, maxit=5, tol=1e-8)
        assert e.value.code == 2 and OLD_MESSAGE in str(e.value)
        st, x, h = _solve(cm, ctx, s, b, ones, precond=cm.PRECOND_ILU0, loop=cm.LOOP_PBICGSTAB2, maxit=2000, tol=1e-8)
        assert st.converged and np.linalg.norm(x - xo) / np.linalg.norm(xo) <= 1e-5        # the second allowed loop
        # solve_many on this solver -- a shift and shifted factors -- stays refused whichever form its columns would take
        dB, dX = ctx.array(np.concatenate([b, b])), ctx.array(np.ones(2 * A0.n))
        try:
            for mode in ("columns", "batched", "auto"):
                sw("MANY_PRECOND", mode)
                for loop, flags in ((cm.LOOP_PBICGSTAB, 0), (cm.LOOP_PBICGSTAB2, 0), (cm.LOOP_PBICGSTAB, cm.FLAG_GUARD)):
                    with pytest.raises(cm.CudamatError) as e:
                        s.solve_many(2, dB, A0.n, dX, A0.n, precond=cm.PRECOND_ILU0, loop=loop, maxit=5, tol=1e-8, flags=flags)
                    assert e.value.code == 2 and OLD_MESSAGE in str(e.value), (mode, loop, flags)
            np.testing.assert_array_equal(dX.download(), np.ones(2 * A0.n))          # nothing ran
        finally:
            dB.free()
            dX.free()
    finally:
        s.close()


def test_drop_in_cache_keeps_factors_only_for_the_same_shift(cm, ctx, oracle, golden_dir):
    """bicgstab_d_lu_precond twice with the same d, then with 8 d: correct answers each time; the second call reuses plan and
    factors, the third reuses the plan and factors anew.  That its factors are those of the new d shows in its iteration count:
    that of a resident solver with fresh factors (the oracle: 2), not that of one with the first call's (the oracle: 9)."""
    A0, d, E, b, xo, so, ho = _reference(oracle, golden_dir, "mat900")
    _, d8, E8, b8, xo8, so8, _ = _reference(oracle, golden_dir, "mat900", 8.0)
    n, ones = A0.n, np.ones(A0.n)
    cm.lib().cudamat_plan_cache_clear()
    try:
        runs = [cm.bicgstab_d_lu_precond(n, A0.nnz, A0.val, A0.rowptr, A0.colidx, dj, ones, bj, 2000, 1e-8)
                for dj, bj in ((d, b), (d.copy(), b), (d8, b8))]
    finally:
        cm.lib().cudamat_plan_cache_clear()
    for (ok, x, dt, st), Ej, bj, xj, sj in zip(runs, (E, E, E8), (b, b, b8), (xo, xo, xo8), (so, so, so8)):
        assert ok is True and st.converged and abs(st.iters - sj.iters) <= max(2, 0.1 * sj.iters)
        assert np.linalg.norm(x - xj) / np.linalg.norm(xj) <= 1e-5
        assert np.linalg.norm(bj - oracle.spmv(Ej, x)) <= 1e-7 * sj.nrm0
    (_, x1, _, st1), (_, x2, _, st2), (_, x3, _, st3) = runs
    assert (st1.plan_reused, st2.plan_reused, st3.plan_reused) == (0, 1, 1)
    assert st1.t_factor > 0.0 and st2.t_factor == 0.0 and st3.t_factor > 0.0       # factored, kept, factored again
    np.testing.assert_array_equal(x2, x1)
    fresh = _shifted_solver(cm, ctx, A0, d8, d8)
    stale = _shifted_solver(cm, ctx, A0, d8, d)
    try:
        stf, xf, _ = _solve(cm, ctx, fresh, b8, ones, precond=cm.PRECOND_ILU0, loop=cm.LOOP_PBICGSTAB, maxit=2000, tol=1e-8)
        sts, _, _ = _solve(cm, ctx, stale, b8, ones, precond=cm.PRECOND_ILU0, loop=cm.LOOP_PBICGSTAB, maxit=2000, tol=1e-8)
    finally:
        fresh.close()
        stale.close()
    print("third call: iters", st3.iters, "fresh factors", stf.iters, "the first call's factors", sts.iters)
    assert sts.converged and sts.iters >= stf.iters + 3          # (the oracle: 9 against 2) the two can be told apart
    assert st3.iters == stf.iters
    assert np.linalg.norm(x3 - xf) <= 1e-12 * np.linalg.norm(xf)
