"""The numeric-only ILU(0) refactorisation on the GPU (cudamat_solver_ilu0_refactor, Solver.ilu0_refactor, the drop-in call's
reused plan; DESIGN.md sections 3, 4d and 10).  The contract: for the same matrix, switches and d2, a solver that was set up
with any d1 and then given refactor(d2) is BIT-IDENTICAL to a fresh solver given ilu0(shift=d2) -- both run the same numeric
kernels in the same launch shapes on the same inputs, so no tolerance appears below where the two are compared.
 1. bits, every storage form of the factors, along the chain set-up(d1) -> refactor(d2) -> refactor(None) -> refactor(d1);
 2. the set-up is not repeated (VERBOSE = 1: no second permuted matrix, one refactor line, the maps are built once);
 3. against the oracle on the explicit matrix, and against stale factors;
 4. zero pivot and refusals;
 5. the drop-in call;
 6. device memory: nothing stays behind.
Run on the GPU box with:  python -m pytest tests -m gpu"""
import ctypes as C
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_ZERO_PIVOT = 2, 3
REFACTOR_LINE = "[cudamat] ilu0 refactor"


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


# ------------------------------------------------------------------ systems (the helpers of test_gpu_shift_precond.py)
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
def _matrix(oracle, golden_dir, name):
    if name == "rand20000x50":
        return oracle.rand_rows(20000, 50, 0x5EED)
    return oracle.mtx_load(os.path.join(golden_dir, name + ".mtx"))


def _d1(A0):
    """d1 = 0.25 mean|diag| (0.5 + i / n)"""
    rows, mask = _diag_mask(A0)
    return 0.25 * np.abs(A0.val[mask]).mean() * _ramp(A0.n)


@functools.lru_cache(maxsize=None)
def _reference(oracle, golden_dir, name, mult=1.0):
    """(A0, d, E, b, xo, so): name with d = mult * (0.5 + i / n), b = E (1 + sin i), the oracle's ILU(0) solve of the explicit
    matrix from x0 = 1.  Computed once, shared between tests, not to be written."""
    A0 = _matrix(oracle, golden_dir, name)
    d = mult * _ramp(A0.n)
    E = _explicit(oracle, A0, d)
    b = oracle.spmv(E, 1.0 + np.sin(np.arange(A0.n)))
    xo, so = oracle.pbicgstab(E, b, vm=oracle.ilu0(E), maxit=2000, tol=1e-8)
    for arr in (d, b, xo):
        arr.setflags(write=False)
    return A0, d, E, b, xo, so


def _new_solver(cm, ctx, A0):
    return cm.Solver.from_host_csr(ctx, A0.rowptr, A0.colidx, A0.val)


def _with_device(ctx, d, fn):
    """fn(device copy of d, or None); the copy is read during the call only"""
    if d is None:
        return fn(None)
    dd = ctx.array(d)
    try:
        return fn(dd)
    finally:
        dd.free()


def _solve(cm, ctx, s, b, x0, **kw):
    db, dx = ctx.array(b), ctx.array(x0)
    try:
        st = s.solve(db.ptr, dx.ptr, **kw)
        return st, dx.download(), s.history()
    finally:
        db.free()
        dx.free()


def _observe(cm, ctx, s, d, n):
    """what the contract covers, of solver s whose factors are those of A0 + diag(d) (None: of A0): the factors' values, M^-1 of a
    fixed vector, M^-1 of 3 columns, and a PRECOND_ILU0 solve of (A0 + diag d) x = b from a fixed x0.  Device buffers are freed."""
    rng = np.random.default_rng(12345)
    rhs, cols = rng.standard_normal(n), rng.standard_normal(3 * n)
    b, x0 = 1.0 + np.sin(np.arange(n)), 1.0 + 0.25 * np.cos(np.arange(n))
    out = {"lu": s.ilu0_values()}
    dr, do, dc, dco = ctx.array(rhs), ctx.empty(n), ctx.array(cols), ctx.empty(3 * n)
    dshift = None if d is None else ctx.array(d)
    try:
        s.precond_apply(dr, do)
        out["apply"] = do.download()
        s.precond_apply_many(3, dc, n, dco, n)
        out["apply_many"] = dco.download()
        s.set_shift(dshift)
        st, x, h = _solve(cm, ctx, s, b, x0, precond=cm.PRECOND_ILU0, loop=cm.LOOP_PBICGSTAB, maxit=200, tol=1e-8)
        s.set_shift(None)
    finally:
        for a in (dr, do, dc, dco) + (() if dshift is None else (dshift,)):
            a.free()
    out["x"], out["history"] = x, h
    out["scalars"] = (st.iters, st.half_exit, st.nrm0, st.converged)
    out["stats"] = st
    return out


def _same(got, want, what):
    for key in ("lu", "apply", "apply_many", "x", "history"):
        np.testing.assert_array_equal(got[key], want[key], err_msg="%s: %s" % (what, key))
    assert got["scalars"] == want["scalars"], (what, got["scalars"], want["scalars"])


def _fresh(cm, ctx, A0, d):
    """what a fresh solver with ilu0(shift=d) shows"""
    s = _new_solver(cm, ctx, A0)
    try:
        _with_device(ctx, d, lambda dd: s.ilu0(shift=dd))
        assert s.ilu0_shifted() is (d is not None)
        assert s.ilu0_refactor_info()[0] == 0
        return _observe(cm, ctx, s, d, A0.n)
    finally:
        s.close()


# ------------------------------------------------------------------ 1. bits, every storage form
FORMS = {
    "mat900-lds": ("mat900", {}),                                                     # single-workgroup LDS solves
    "mat10000-levels": ("mat10000", {"TRSV_LDS": 0}),                                 # one launch per level / run of small levels
    "mat10000-syncfree": ("mat10000", {"TRSV_LDS": 0, "TRSV_SYNCFREE": 1}),           # dependency-driven
    "rand20000x50-split-perm": ("rand20000x50", {"TRSV_HYBRID": 1, "TRSV_PERM": 1}),  # split factors, loop in level-major spaces
    "rand20000x50-split": ("rand20000x50", {"TRSV_HYBRID": 1, "TRSV_PERM": 0}),
    "mat10000-split-perm": ("mat10000", {"TRSV_HYBRID": 1, "TRSV_PERM": 1}),
    "mat10000-split": ("mat10000", {"TRSV_HYBRID": 1, "TRSV_PERM": 0}),
}


@pytest.mark.parametrize("form", list(FORMS))
def test_refactor_is_a_fresh_factorisation_bit_for_bit(cm, ctx, oracle, golden_dir, sw, form):
    """set-up(d1) -> refactor(d2 = 8 d1) -> refactor(None) -> refactor(d1): after each link the solver shows what a fresh solver
    with ilu0(shift=that d) shows, bit for bit (factor values, M^-1 of one vector and of 3 columns, a preconditioned solve: x,
    history, iters, half_exit, nrm0); ilu0_shifted and the refactor count follow.  Split factors report their groups and, from
    the first refactor on, the bytes of their value maps (unsplit ones: 0)."""
    name, switches = FORMS[form]
    for k, v in switches.items():
        sw(k, v)
    split = "TRSV_HYBRID" in switches
    A0 = _matrix(oracle, golden_dir, name)
    n = A0.n
    d1 = _d1(A0)
    d2 = 8.0 * d1
    s = _new_solver(cm, ctx, A0)
    try:
        _with_device(ctx, d1, lambda dd: s.ilu0(shift=dd))
        assert s.ilu0_refactor_info() == (0, 0.0, 0)
        first = _observe(cm, ctx, s, d1, n)                   # (also: the permuted matrix exists before the first refactor)
        _same(first, _fresh(cm, ctx, A0, d1), form + " set-up")
        assert (first["stats"].trsv_groups_l > 0 and first["stats"].trsv_groups_u > 0) == split
        map_bytes = None
        for link, d in enumerate((d2, None, d1), start=1):
            _with_device(ctx, d, lambda dd: s.ilu0_refactor(dd))
            assert s.ilu0_shifted() is (d is not None)
            count, seconds, nbytes = s.ilu0_refactor_info()
            assert count == link and seconds > 0.0
            assert (nbytes > 0) == split
            assert map_bytes in (None, nbytes)                # built once
            map_bytes = nbytes
            got = _observe(cm, ctx, s, d, n)
            _same(got, _fresh(cm, ctx, A0, d), "%s link %d" % (form, link))
            assert (got["stats"].trsv_groups_l > 0 and got["stats"].trsv_groups_u > 0) == split
        _same(got, first, form + " back at d1")
        assert not np.array_equal(got["lu"], _fresh(cm, ctx, A0, d2)["lu"])           # (the links do differ)
    finally:
        s.close()


def test_refactor_before_the_first_solve_builds_the_shift_map(cm, ctx, oracle, golden_dir, sw):
    """split factors set up WITHOUT a shift have no map for the shift term of the level-major loop; the A0 -> d transition builds
    it -- before the permuted matrix exists (the U positions are still there) and after (they are recomputed)"""
    sw("TRSV_HYBRID", 1)
    A0 = _matrix(oracle, golden_dir, "mat10000")
    d1 = _d1(A0)
    want = _fresh(cm, ctx, A0, d1)
    for solve_first in (False, True):
        s = _new_solver(cm, ctx, A0)
        try:
            s.ilu0()
            if solve_first:
                _observe(cm, ctx, s, None, A0.n)
            _with_device(ctx, d1, lambda dd: s.ilu0_refactor(dd))
            _same(_observe(cm, ctx, s, d1, A0.n), want, "A0 -> d1, solve first: %s" % solve_first)
        finally:
            s.close()


# ------------------------------------------------------------------ 2. the set-up is not repeated
def test_the_set_up_is_not_repeated(cm, ctx, oracle, golden_dir, sw, capfd):
    sw("TRSV_HYBRID", 1)
    sw("TRSV_PERM", 1)
    sw("VERBOSE", 1)
    A0 = _matrix(oracle, golden_dir, "rand20000x50")
    d1 = _d1(A0)
    d2 = 8.0 * d1
    s = _new_solver(cm, ctx, A0)
    try:
        _with_device(ctx, d1, lambda dd: s.ilu0(shift=dd))
        capfd.readouterr()
        _observe(cm, ctx, s, d1, A0.n)
        err = capfd.readouterr().err
        assert "ilu0 permuted matrix" in err and REFACTOR_LINE not in err
        _with_device(ctx, d2, lambda dd: s.ilu0_refactor(dd))
        got = _observe(cm, ctx, s, d2, A0.n)
        err = capfd.readouterr().err
        assert "ilu0 permuted matrix" not in err
        assert err.count(REFACTOR_LINE) == 1, err
        for gone in ("L levels", "U levels", "level sort", "factor row pointers", "far plans (pb_build)"):    # the set-up's stamps
            assert gone not in err, (gone, err)
        assert "value maps (built once)" in err
        bytes1 = s.ilu0_refactor_info()[2]
        assert bytes1 > 0
        _with_device(ctx, d1, lambda dd: s.ilu0_refactor(dd))
        err = capfd.readouterr().err
        assert err.count(REFACTOR_LINE) == 1 and "far plans" not in err and "split" not in err, err
        assert s.ilu0_refactor_info()[2] == bytes1
        assert s.ilu0_refactor_info()[0] == 2
    finally:
        s.close()
    sw("VERBOSE", 0)
    _same(got, _fresh(cm, ctx, A0, d2), "after refactor(d2)")


# ------------------------------------------------------------------ 3. against the oracle
@pytest.mark.parametrize("name", ["mat900", "mat10000"])
def test_refactored_factors_vs_oracle(cm, ctx, oracle, golden_dir, name):
    """factors of d, refactor(8 d), set_shift(8 d), x0 = 1, tol 1e-8: against the oracle's ILU(0) loop on the explicit matrix by
    the tolerances of SURVEY 8c (iterations within max(2, 10 %), x to 1e-5, true residual <= 1e-7 nrm0), and at least 3
    iterations fewer than the same solve with the stale factors of d (the oracle on mat900: 2 against 9)."""
    A0, d, E, b, xo, so = _reference(oracle, golden_dir, name)
    _, d8, E8, b8, xo8, so8 = _reference(oracle, golden_dir, name, 8.0)
    ones = np.ones(A0.n)
    assert so8.converged
    s = _new_solver(cm, ctx, A0)
    dd8 = ctx.array(d8)
    try:
        _with_device(ctx, d, lambda dd: s.ilu0(shift=dd))
        s.set_shift(dd8)
        sts, xs, _ = _solve(cm, ctx, s, b8, ones, precond=cm.PRECOND_ILU0, loop=cm.LOOP_PBICGSTAB, maxit=2000, tol=1e-8)
        s.ilu0_refactor(dd8)
        st, x, _ = _solve(cm, ctx, s, b8, ones, precond=cm.PRECOND_ILU0, loop=cm.LOOP_PBICGSTAB, maxit=2000, tol=1e-8)
    finally:
        s.close()
        dd8.free()
    res = np.linalg.norm(b8 - oracle.spmv(E8, x))
    print(name, "refactored: iters", st.iters, "oracle", so8.iters, "stale", sts.iters, "|x - xo| / |xo|",
          np.linalg.norm(x - xo8) / np.linalg.norm(xo8), "residual / nrm0", res / so8.nrm0)
    assert st.converged and abs(st.iters - so8.iters) <= max(2, 0.1 * so8.iters)
    assert np.linalg.norm(x - xo8) / np.linalg.norm(xo8) <= 1e-5
    assert res <= 1e-7 * so8.nrm0
    assert sts.converged and sts.iters >= st.iters + 3


# ------------------------------------------------------------------ 4. zero pivot and refusals
def test_zero_pivot_and_refusals(cm, ctx, oracle, golden_dir):
    A0 = _matrix(oracle, golden_dir, "mat900")
    n = A0.n
    d1 = _d1(A0)
    rows, mask = _diag_mask(A0)
    a00 = A0.val[mask][0]
    assert rows[mask][0] == 0
    dz = d1.copy()
    dz[0] = -a00                                    # a00 + dz[0] == 0.0 exactly
    assert a00 + dz[0] == 0.0
    b, ones = 1.0 + np.sin(np.arange(n)), np.ones(n)
    s = _new_solver(cm, ctx, A0)
    dd1 = ctx.array(d1)
    try:
        with pytest.raises(cm.CudamatError) as e:           # before any factors
            s.ilu0_refactor(dd1)
        assert e.value.code == ERR_ARG and "no factors" in str(e.value)
        assert s.ilu0_refactor_info() == (0, 0.0, 0)
        s.block_ilu0()
        with pytest.raises(cm.CudamatError) as e:
            s.ilu0_refactor(dd1)
        assert e.value.code == ERR_ARG and "block-Jacobi" in str(e.value)
        s.ilu0(shift=dd1)
        with pytest.raises(cm.CudamatError) as e:
            _with_device(ctx, dz, lambda dd: s.ilu0_refactor(dd))
        assert e.value.code == ERR_ZERO_PIVOT and "zero pivot" in str(e.value)
        # no factors are left, exactly as after a failed ilu0(shift=...)
        assert s.ilu0_shifted() is False
        assert s.ilu0_refactor_info() == (0, 0.0, 0)
        with pytest.raises(cm.CudamatError) as e:
            s.ilu0_values()
        assert e.value.code == ERR_ARG
        s.set_shift(dd1)
        with pytest.raises(cm.CudamatError) as e:           # (with a shift nothing is factored silently)
            _solve(cm, ctx, s, b, ones, precond=cm.PRECOND_ILU0, loop=cm.LOOP_PBICGSTAB, maxit=5, tol=1e-8)
        assert e.value.code == ERR_ARG
        with pytest.raises(cm.CudamatError) as e:
            s.ilu0_refactor(dd1)
        assert e.value.code == ERR_ARG
        s.set_shift(None)
        s.ilu0(shift=dd1)                                   # a fresh set-up works
        _same(_observe(cm, ctx, s, d1, n), _fresh(cm, ctx, A0, d1), "after the zero pivot")
    finally:
        s.close()
        dd1.free()


def test_zero_pivot_names_the_row(cm, ctx, sw):
    """Two diagonal blocks [[1, 1], [1, 1]]: rows 1 and 3 both eliminate to an exact 0.0 and neither depends on the other, so no
    NaN hides either.  The single-column factorisation names the LARGEST such row, with the prefetching and with the simple level
    kernel; the K-wide one (ilu0_shifts_values on the kept structure, a zero shift in both columns) the smallest (column, row)."""
    rowptr = np.array([0, 2, 4, 6, 8], np.int32)
    colidx = np.array([0, 1, 0, 1, 2, 3, 2, 3], np.int32)
    val, n = np.ones(8), 4
    for simple in ("0", "1"):
        sw("ILU0_SIMPLE", simple)
        s = cm.Solver.from_host_csr(ctx, rowptr, colidx, val)
        try:
            with pytest.raises(cm.CudamatError) as e:
                s.ilu0()
        finally:
            s.close()
        print(e.value)
        assert e.value.code == ERR_ZERO_PIVOT and str(e.value).endswith("zero pivot in row 3"), str(e.value)
    sw("ILU0_SIMPLE", "0")
    sw("MANY_PRECOND", "batched")
    s = cm.Solver.from_host_csr(ctx, rowptr, colidx, val)
    good, dD = ctx.array(np.ones(n)), ctx.array(np.zeros(2 * n))
    try:
        s.ilu0(shift=good)                                  # [[2, 1], [1, 2]]: the structure the K-wide pass works on
        with pytest.raises(cm.CudamatError) as e:
            s.ilu0_shifts_values(2, dD, n)
    finally:
        s.close()
        good.free()
        dD.free()
    print(e.value)
    assert e.value.code == ERR_ZERO_PIVOT and str(e.value).endswith("zero pivot in column 0, row 1"), str(e.value)


# ------------------------------------------------------------------ 5. the drop-in call
def test_drop_in_call_refactors_on_a_reused_plan(cm, oracle, golden_dir, monkeypatch, capfd):
    """bicgstab_d_lu_precond on mat900 with d, 8 d, d under VERBOSE = 1: the second and third calls reuse the plan, print the
    refactor line, report t_factor > 0 and return the x of a cleared-cache call with the same arguments bit for bit; with
    ILU0_REFACTOR = 0 no refactor line appears and x is the same."""
    A0, d, E, b, xo, so = _reference(oracle, golden_dir, "mat900")
    _, d8, E8, b8, xo8, so8 = _reference(oracle, golden_dir, "mat900", 8.0)
    n, ones = A0.n, np.ones(A0.n)
    monkeypatch.setenv("CUDAMAT_VERBOSE", "1")
    calls = ((d, b), (d8, b8), (d, b))

    def call(dj, bj):
        capfd.readouterr()
        ok, x, dt, st = cm.bicgstab_d_lu_precond(n, A0.nnz, A0.val, A0.rowptr, A0.colidx, dj, ones, bj, 2000, 1e-8)
        assert ok is True and st.converged
        return x, st, capfd.readouterr().err

    cm.lib().cudamat_plan_cache_clear()
    try:
        chained = [call(dj, bj) for dj, bj in calls]
        alone = []
        for dj, bj in calls:
            cm.lib().cudamat_plan_cache_clear()
            alone.append(call(dj, bj))
        monkeypatch.setenv("CUDAMAT_ILU0_REFACTOR", "0")
        cm.lib().cudamat_plan_cache_clear()
        old_path = [call(dj, bj) for dj, bj in calls]
    finally:
        cm.lib().cudamat_plan_cache_clear()
    assert chained[0][1].plan_reused == 0 and REFACTOR_LINE not in chained[0][2]
    for k in (1, 2):
        x, st, err = chained[k]
        assert st.plan_reused == 1 and st.t_factor > 0.0
        assert err.count(REFACTOR_LINE) == 1, err
        np.testing.assert_array_equal(x, alone[k][0])
        assert (st.iters, st.half_exit, st.nrm0) == (alone[k][1].iters, alone[k][1].half_exit, alone[k][1].nrm0)
    for k in range(3):
        assert alone[k][1].plan_reused == 0 and REFACTOR_LINE not in alone[k][2]
        x, st, err = old_path[k]
        assert REFACTOR_LINE not in err
        assert st.plan_reused == (1 if k else 0) and st.t_factor > 0.0
        np.testing.assert_array_equal(x, chained[k][0])
    for (x, st, _), Ej, bj, xj, sj in zip(chained, (E, E8, E), (b, b8, b), (xo, xo8, xo), (so, so8, so)):
        assert abs(st.iters - sj.iters) <= max(2, 0.1 * sj.iters)
        assert np.linalg.norm(x - xj) / np.linalg.norm(xj) <= 1e-5
        assert np.linalg.norm(bj - oracle.spmv(Ej, x)) <= 1e-7 * sj.nrm0


# ------------------------------------------------------------------ 6. memory
def test_nothing_stays_behind(cm, ctx, oracle, golden_dir, sw):
    """cudamat_mem_live before the solver is created equals the count after close(), with split factors, their value maps and
    three refactors in between (the pattern of tests/pool_check.py and tests/live_check.py)"""
    def live():
        v = C.c_size_t()
        assert cm.lib().cudamat_mem_live(C.byref(v)) == 0
        return v.value

    sw("TRSV_HYBRID", 1)
    A0 = _matrix(oracle, golden_dir, "mat10000")
    d1 = _d1(A0)
    ctx.sync()
    before = live()
    s = _new_solver(cm, ctx, A0)
    try:
        _with_device(ctx, d1, lambda dd: s.ilu0(shift=dd))
        with_factors = live()
        _with_device(ctx, 8.0 * d1, lambda dd: s.ilu0_refactor(dd))
        assert s.ilu0_refactor_info()[2] > 0
        with_maps = live()
        assert with_maps > with_factors                      # the maps are device memory the solver owns ...
        _observe(cm, ctx, s, 8.0 * d1, A0.n)
        _with_device(ctx, None, lambda dd: s.ilu0_refactor(dd))
        _with_device(ctx, d1, lambda dd: s.ilu0_refactor(dd))
        s.ilu0()                                             # ... and a new set-up releases them with the rest
        assert s.ilu0_refactor_info() == (0, 0.0, 0)
        _with_device(ctx, d1, lambda dd: s.ilu0_refactor(dd))
    finally:
        s.close()
    ctx.sync()
    assert live() == before
