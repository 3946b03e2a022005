"""New values for a resident matrix on the structure it already holds (cudamat_solver_set_values, Solver.set_values, the drop-in
call's cached plan; DESIGN.md sections 2, 3, 4d).  The contract: after set_values(v2) on a solver created with (rp, ci, v1) the
solver shows what a FRESH solver created with (rp, ci, v2) under the same switches shows, bit for bit -- the tests force the
SpMV form, so both run the same kernels, and no tolerance appears below where the two are compared.
 1. SpMV bits, every storage form, along the chain v1 -> v2 -> v3 -> v1;
 2. storage-class transitions (dictionary <-> fp64 values);
 3. every loop form, the batched loops;
 4. with ILU(0): stale factors directly after the call, bit-identity after the refactorisation, the set-up is not repeated;
 5. refusals;
 6. the drop-in calls;
 7. device memory: nothing stays behind.
Run on the GPU box with:  python -m pytest tests -m gpu"""
import ctypes as C
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ERR_ARG = 2
VALUES_LINE = "[cudamat] set_values"
REFACTOR_LINE = "[cudamat] ilu0 refactor"
SETUP_STAMPS = ("create validation", "L levels", "U levels", "far plans (pb_build)", "ilu0 permuted matrix")


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


# ------------------------------------------------------------------ matrices and value sets (computed once, not to be written)
@functools.lru_cache(maxsize=None)
def _matrix(oracle, golden_dir, name):
    if name.startswith("poisson"):
        nx, ny = name[7:].split("x")
        A = oracle.poisson5(int(nx), int(ny))
    elif name.startswith("rand"):
        n, per = name[4:].split("x")
        A = oracle.rand_rows(int(n), int(per), 0x5EED)
    else:
        A = oracle.mtx_load(os.path.join(golden_dir, name + ".mtx"))
    for arr in (A.rowptr, A.colidx, A.val):
        arr.setflags(write=False)
    return A


@functools.lru_cache(maxsize=None)
def _values(oracle, golden_dir, name, which):
    """v1: the matrix' own; ints7 / ints3: integer-valued, 7 / 3 distinct, different from v1 and from each other in every entry;
    reals: v1 (1 + 0.05 sin k), more than 256 distinct bit patterns (the loop tests' v2)"""
    A = _matrix(oracle, golden_dir, name)
    k = np.arange(A.nnz)
    if which == "v1":
        v = A.val
    elif which == "ints7":
        v = 100.0 + (k % 7)
    elif which == "ints3":
        v = -200.0 - (k % 3)
    else:
        assert which == "reals"
        v = A.val * (1.0 + 0.05 * np.sin(k))
        assert len(np.unique(v[:4096])) > 256
    v = np.ascontiguousarray(v, dtype=np.float64)
    if which.startswith("ints"):
        assert np.all(v != A.val)                    # a forgotten copy cannot pass
    if which != "v1":
        v.setflags(write=False)
    return v


def _with(A, oracle, val):
    return oracle.Csr(A.n, A.rowptr, A.colidx, val, A.m)


def _new_solver(cm, ctx, A, val=None):
    return cm.Solver.from_host_csr(ctx, A.rowptr, A.colidx, A.val if val is None else val)


def _set(ctx, s, val):
    """set_values from a device copy that is freed right after the call (val is read during the call only)"""
    dv = ctx.array(val)
    try:
        s.set_values(dv)
    finally:
        dv.free()


def _live(cm):
    v = C.c_size_t()
    assert cm.lib().cudamat_mem_live(C.byref(v)) == 0
    return v.value


def _int_x(n):
    return ((np.arange(n) * 7) % 13 - 6).astype(np.float64)


def _products(ctx, s, n):
    """spmv of an integer-valued x, and spmm / spmm_shifts of 2 columns"""
    x = _int_x(n)
    X = np.concatenate([x, x[::-1]])
    D = np.concatenate([0.5 + np.arange(n) / n, np.cos(np.arange(n))])
    dx, dy, dX, dD, dY = ctx.array(x), ctx.empty(n), ctx.array(X), ctx.array(D), ctx.empty(2 * n)
    try:
        s.spmv(dx, dy)
        out = {"spmv": dy.download()}
        s.spmm(2, dX, n, dY, n)
        out["spmm"] = dY.download()
        s.spmm_shifts(2, dX, n, dD, n, dY, n)
        out["spmm_shifts"] = dY.download()
        return out
    finally:
        for a in (dx, dy, dX, dD, dY):
            a.free()


def _spmv(ctx, s, n):
    dx, dy = ctx.array(_int_x(n)), ctx.empty(n)
    try:
        s.spmv(dx, dy)
        return dy.download()
    finally:
        dx.free()
        dy.free()


def _same_products(got, want, what):
    for key in ("spmv", "spmm", "spmm_shifts"):
        np.testing.assert_array_equal(got[key], want[key], err_msg="%s: %s" % (what, key))


def _fresh_products(cm, ctx, A, val, kernel):
    s = _new_solver(cm, ctx, A, val)
    try:
        name = s.spmv_kernel()
        assert name.startswith(kernel), name
        return _products(ctx, s, A.n), name, s.value_dict()
    finally:
        s.close()


# ------------------------------------------------------------------ 1. SpMV bits, every storage form
SPMV_FORMS = {
    "stream_c":          ("poisson40x30", {"SPMV_MODE": "csr", "VALUE_DICT": 0, "SPMV_ALIGN": 0}, "k_spmv_stream_c<"),
    "stream_c-aligned":  ("poisson40x30", {"SPMV_MODE": "csr", "VALUE_DICT": 0, "SPMV_ALIGN": 1}, "k_spmv_stream_c<"),
    "stream_d":          ("poisson460x460", {"SPMV_MODE": "csr"}, "k_spmv_stream_d<"),
    "pat":               ("poisson40x30", {"SPMV_MODE": "pat"}, "k_spmv_pat<"),
    "pat_d":             ("poisson460x460", {"SPMV_MODE": "pat"}, "k_spmv_pat_d<"),
    "lanes":             ("rand600x50", {"SPMV_MODE": "csr"}, "k_spmv<"),
    "tiles":             ("rand600x50", {"SPMV_MODE": "csr", "SPMV_FORM": "tiles"}, "k_spmv_tiles"),
    "sell":              ("rand600x50", {"SPMV_MODE": "sell"}, "k_spmv_sell"),
    "blocked":           ("rand600x50", {"SPMV_MODE": "pb"}, "k_pb_phase1 +"),
    "blocked-dict":      ("rand21000x50", {"SPMV_MODE": "pb"}, "k_pb_phase1_dict +"),
    "blocked-dict-1024": ("rand21000x50", {"SPMV_MODE": "pb", "PB_MIN_WAVES": 1024}, "k_pb_phase1_dict +"),
}


@pytest.mark.parametrize("form", list(SPMV_FORMS))
def test_products_are_those_of_a_fresh_solver(cm, ctx, oracle, golden_dir, sw, form):
    """v1 -> ints7 -> ints3 -> v1: after each link spmv, spmm and spmm_shifts equal those of a fresh solver holding that link's
    values, bit for bit, through the same kernel; the integer links also equal the oracle (exact on integers); the copies keep
    their storage class, so nothing is rebuilt; the links do differ."""
    name, switches, kernel = SPMV_FORMS[form]
    for k, v in switches.items():
        sw(k, v)
    A = _matrix(oracle, golden_dir, name)
    n = A.n
    s = _new_solver(cm, ctx, A)
    try:
        assert s.spmv_kernel().startswith(kernel), s.spmv_kernel()
        first = _products(ctx, s, n)
        want1, kname, ndict = _fresh_products(cm, ctx, A, A.val, kernel)
        _same_products(first, want1, form + " creation")
        assert s.set_values_info() == (0, 0.0, 0, 0)
        seen = {}
        for link, which in enumerate(("ints7", "ints3", "v1"), start=1):
            v = _values(oracle, golden_dir, name, which)
            _set(ctx, s, v)
            count, seconds, nbytes, rebuilt = s.set_values_info()
            assert count == link and seconds > 0.0 and rebuilt == 0
            assert (nbytes > 0) == form.startswith("blocked")
            got = _products(ctx, s, n)
            want, fresh_kernel, fresh_dict = _fresh_products(cm, ctx, A, v, kernel)
            assert s.spmv_kernel() == fresh_kernel == kname
            assert s.value_dict() == fresh_dict
            _same_products(got, want, "%s link %d" % (form, link))
            if which != "v1":
                np.testing.assert_array_equal(got["spmv"], oracle.spmv(_with(A, oracle, v), _int_x(n)))
            seen[which] = got
        _same_products(seen["v1"], first, form + " back at v1")
        assert not np.array_equal(seen["ints7"]["spmv"], first["spmv"])
        assert not np.array_equal(seen["ints7"]["spmv"], seen["ints3"]["spmv"])
    finally:
        s.close()


def test_a_host_array_is_uploaded_for_the_call(cm, ctx, oracle, golden_dir, sw):
    sw("SPMV_MODE", "csr")
    A = _matrix(oracle, golden_dir, "rand600x50")
    v = _values(oracle, golden_dir, "rand600x50", "ints7")
    s = _new_solver(cm, ctx, A)
    try:
        _products(ctx, s, A.n)
        before = _live(cm)
        s.set_values(v)                              # a numpy array
        assert _live(cm) == before                   # (the temporary is gone)
        np.testing.assert_array_equal(_products(ctx, s, A.n)["spmv"], oracle.spmv(_with(A, oracle, v), _int_x(A.n)))
    finally:
        s.close()


# ------------------------------------------------------------------ 2. storage-class transitions
@pytest.mark.parametrize("name", ["poisson460x460", "rand21000x50"])
@pytest.mark.parametrize("mode", ["pb", "default"])
def test_storage_class_transitions(cm, ctx, oracle, golden_dir, sw, name, mode):
    """v1 (dictionary) -> ints7 (dictionary: refreshed in place, the new count) -> ints7 again (the maps stay) -> reals (no
    dictionary: rebuilt) -> v1 (dictionary again: rebuilt) -> ints7 (in place again); every link against a fresh solver"""
    if mode == "pb":
        sw("SPMV_MODE", "pb")
    A = _matrix(oracle, golden_dir, name)
    n = A.n

    def fresh(v):
        f = _new_solver(cm, ctx, A, v)
        try:
            return _products(ctx, f, n), f.spmv_kernel(), f.value_dict()
        finally:
            f.close()

    s = _new_solver(cm, ctx, A)
    try:
        got = _products(ctx, s, n)
        want, kernel1, ndict1 = fresh(A.val)
        _same_products(got, want, "creation")
        assert (s.spmv_kernel(), s.value_dict()) == (kernel1, ndict1)
        if mode == "pb":
            assert kernel1.startswith("k_pb_phase1_dict +") and ndict1 > 0
        assert s.set_values_info() == (0, 0.0, 0, 0)
        chain = (("ints7", 0), ("ints7", 0), ("reals", 1), ("v1", 1), ("ints7", 0))
        maps = None
        for link, (which, rebuilt_want) in enumerate(chain, start=1):
            v = _values(oracle, golden_dir, name, which)
            _set(ctx, s, v)
            count, seconds, nbytes, rebuilt = s.set_values_info()
            assert (count, rebuilt) == (link, rebuilt_want), (which, count, rebuilt)
            got = _products(ctx, s, n)
            want, kernel, ndict = fresh(v)
            assert (s.spmv_kernel(), s.value_dict()) == (kernel, ndict), (which, s.spmv_kernel(), kernel)
            _same_products(got, want, "%s %s link %d (%s)" % (name, mode, link, which))
            if which == "reals":
                assert s.value_dict() == 0
            if mode == "pb":
                assert ndict == {"ints7": 7, "reals": 0, "v1": ndict1}[which]
            if which == "ints7":                     # while the form is kept the maps are what the first call built
                assert maps in (None, nbytes)
                maps = nbytes
                assert (nbytes > 0) == kernel.startswith("k_pb_phase1")
    finally:
        s.close()


# ------------------------------------------------------------------ 3. loops
def _system(oracle, golden_dir, name):
    """(A, v2, b, x0): v2 = v1 (1 + 0.05 sin k), b = A2 (1 + sin i), x0 = 1 + 0.25 cos i"""
    A = _matrix(oracle, golden_dir, name)
    v2 = _values(oracle, golden_dir, name, "reals")
    return A, v2, _rhs(oracle, golden_dir, name), 1.0 + 0.25 * np.cos(np.arange(A.n))


@functools.lru_cache(maxsize=None)
def _rhs(oracle, golden_dir, name):
    A = _matrix(oracle, golden_dir, name)
    b = oracle.spmv(_with(A, oracle, _values(oracle, golden_dir, name, "reals")), 1.0 + np.sin(np.arange(A.n)))
    b.setflags(write=False)
    return b


def _solve(cm, ctx, s, b, x0, **kw):
    db, dx = ctx.array(b), ctx.array(x0)
    try:
        st = s.solve(db.ptr, dx.ptr, **kw)
        return st, dx.download(), s.history()
    finally:
        db.free()
        dx.free()


def _loops(cm, ctx, s, b, x0):
    out = {}
    for loop in (cm.LOOP_PBICGSTAB, cm.LOOP_PBICGSTAB2, cm.LOOP_PIPELINED):
        st, x, h = _solve(cm, ctx, s, b, x0, loop=loop, maxit=60, tol=1e-8)
        out[loop] = (x, h, (st.iters, st.half_exit, st.nrm0, st.loop_form))
    return out


def _same_loops(got, want, what):
    for loop in want:
        np.testing.assert_array_equal(got[loop][0], want[loop][0], err_msg="%s loop %d: x" % (what, loop))
        np.testing.assert_array_equal(got[loop][1], want[loop][1], err_msg="%s loop %d: history" % (what, loop))
        assert got[loop][2] == want[loop][2], (what, loop, got[loop][2], want[loop][2])


@pytest.mark.parametrize("name", ["mat900", "mat10000", "rand20000x50"])
@pytest.mark.parametrize("forms", ["default", "FUSED=0", "RESIDENT=0"])
def test_loops_are_those_of_a_fresh_solver(cm, ctx, oracle, golden_dir, sw, name, forms):
    """the three loops (x, history, iters, half_exit, nrm0 and the loop form that ran) after set_values(v2), against a fresh
    solver with v2: the default small-system forms, the three-launch fused loop alone, the reference loops alone"""
    if forms != "default":
        sw(*forms.split("="))
    A, v2, b, x0 = _system(oracle, golden_dir, name)
    s = _new_solver(cm, ctx, A)
    try:
        _loops(cm, ctx, s, b, x0)                    # (every copy and work vector exists before the values change)
        _set(ctx, s, v2)
        got = _loops(cm, ctx, s, b, x0)
    finally:
        s.close()
    f = _new_solver(cm, ctx, A, v2)
    try:
        want = _loops(cm, ctx, f, b, x0)
    finally:
        f.close()
    _same_loops(got, want, "%s %s" % (name, forms))


def _batched(cm, ctx, s, n, b, x0):
    K = 3
    B = np.concatenate([b, 2.0 * b, b[::-1]])
    X0 = np.concatenate([x0, x0, np.ones(n)])
    D = np.concatenate([np.zeros(n), 0.5 + np.arange(n) / n, 0.25 * np.ones(n)])
    out = {}
    dB, dD = ctx.array(B), ctx.array(D)
    try:
        for what in ("solve_many", "solve_shifts"):
            dX = ctx.array(X0)
            try:
                if what == "solve_many":
                    sts, form = s.solve_many(K, dB, n, dX, n, loop=cm.LOOP_PBICGSTAB2, maxit=60, tol=1e-8)
                else:
                    sts, form = s.solve_shifts(K, dD, n, dB, n, dX, n, loop=cm.LOOP_PBICGSTAB2, maxit=60, tol=1e-8)
                assert form == 1
                out[what] = (dX.download(), [s.history(col=j) for j in range(K)], [(t.iters, t.half_exit, t.nrm0) for t in sts])
            finally:
                dX.free()
    finally:
        dB.free()
        dD.free()
    return out


@pytest.mark.parametrize("name", ["mat900", "mat10000", "rand20000x50"])
def test_batched_loops_are_those_of_a_fresh_solver(cm, ctx, oracle, golden_dir, sw, name):
    """solve_many and solve_shifts with K = 3 under MANY_FORM = batched after set_values(v2), against a fresh solver with v2"""
    sw("MANY_FORM", "batched")
    A, v2, b, x0 = _system(oracle, golden_dir, name)
    s = _new_solver(cm, ctx, A)
    try:
        _batched(cm, ctx, s, A.n, b, x0)
        _set(ctx, s, v2)
        got = _batched(cm, ctx, s, A.n, b, x0)
    finally:
        s.close()
    f = _new_solver(cm, ctx, A, v2)
    try:
        want = _batched(cm, ctx, f, A.n, b, x0)
    finally:
        f.close()
    for what in want:
        np.testing.assert_array_equal(got[what][0], want[what][0], err_msg=what + ": X")
        for j in range(3):
            np.testing.assert_array_equal(got[what][1][j], want[what][1][j], err_msg="%s: history of column %d" % (what, j))
        assert got[what][2] == want[what][2], (what, got[what][2], want[what][2])


# ------------------------------------------------------------------ 4. with ILU(0)
ILU_FORMS = {
    "mat900-lds": ("mat900", {}, False),                                                     # single-workgroup LDS solves
    "mat10000-levels": ("mat10000", {"TRSV_LDS": 0}, False),                                 # one launch per level / run of small levels
    "mat10000-syncfree": ("mat10000", {"TRSV_LDS": 0, "TRSV_SYNCFREE": 1}, False),           # dependency-driven
    "rand20000x50-split": ("rand20000x50", {"TRSV_HYBRID": 1, "TRSV_PERM": 0}, False),       # split factors
    "rand20000x50-split-perm": ("rand20000x50", {"TRSV_HYBRID": 1, "TRSV_PERM": 1}, False),  # ... loop in level-major spaces,
    "rand20000x50-split-perm-solved": ("rand20000x50", {"TRSV_HYBRID": 1, "TRSV_PERM": 1}, True),   # the permuted matrix exists
    "mat10000-split-perm-solved": ("mat10000", {"TRSV_HYBRID": 1, "TRSV_PERM": 1}, True),
}


def _with_device(ctx, d, fn):
    if d is None:
        return fn(None)
    dd = ctx.array(d)
    try:
        return fn(dd)
    finally:
        dd.free()


def _observe_ilu(cm, ctx, s, d, n, b, x0):
    """the factors, M^-1 of one vector and of 3 columns, a PRECOND_ILU0 solve of (A + diag d) x = b from x0"""
    rng = np.random.default_rng(12345)
    rhs, cols = rng.standard_normal(n), rng.standard_normal(3 * n)
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
    return out


def _shifts_ilu0(cm, ctx, s, n, b, d):
    """solve_shifts_ilu0 with K = 2 under both MANY_PRECOND forms (switched on the context by the caller's sw)"""
    K = 2
    B = np.concatenate([b, b[::-1]])
    D = np.concatenate([d, 2.0 * d])
    dB, dD, dX = ctx.array(B), ctx.array(D), ctx.array(np.ones(K * n))
    try:
        sts, form = s.solve_shifts_ilu0(K, dD, n, dB, n, dX, n, maxit=60, tol=1e-8)
        return dX.download(), [(t.iters, t.half_exit, t.nrm0) for t in sts], form
    finally:
        for a in (dB, dD, dX):
            a.free()


def _same_ilu(got, want, what):
    for key in ("lu", "apply", "apply_many", "x", "history"):
        np.testing.assert_array_equal(got[key], want[key], err_msg="%s: %s" % (what, key))
    assert got["scalars"] == want["scalars"], (what, got["scalars"], want["scalars"])


def _shift_of(A):
    rows = np.repeat(np.arange(A.n), np.diff(A.rowptr))
    mask = (A.colidx - A.base) == rows
    return 0.25 * np.abs(A.val[mask]).mean() * (0.5 + np.arange(A.n) / A.n)


@pytest.mark.parametrize("form", list(ILU_FORMS))
def test_refactored_factors_are_those_of_a_fresh_solver(cm, ctx, oracle, golden_dir, sw, form):
    """ilu0() on v1, set_values(v2): the factors are still those of v1, bit for bit.  Then ilu0_refactor(None) and
    ilu0_refactor(d): factors, precond_apply, precond_apply_many (3 columns), the preconditioned solve and solve_shifts_ilu0
    (K = 2, MANY_PRECOND = columns and batched) equal those of a fresh solver with v2 and ilu0() / ilu0(shift=d).  The split
    forms in level-major spaces run once without and once with a preconditioned solve -- hence the permuted matrix and, after the
    call, its value map -- in front of set_values."""
    name, switches, solve_first = ILU_FORMS[form]
    for k, v in switches.items():
        sw(k, v)
    A, v2, b, x0 = _system(oracle, golden_dir, name)
    n = A.n
    d = _shift_of(A)

    def everything(s, dj):
        out = _observe_ilu(cm, ctx, s, dj, n, b, x0)
        for many in ("columns", "batched"):
            ctx.set_option("MANY_PRECOND", many)
            out["shifts-" + many] = _shifts_ilu0(cm, ctx, s, n, b, d)
            # (column by column the call leaves its last column's factors in the solver: back to those under test)
            _with_device(ctx, dj, lambda dd: s.ilu0_refactor(dd))
        ctx.set_option("MANY_PRECOND", "columns")
        return out

    def same(got, want, what):
        _same_ilu(got, want, what)
        for many in ("columns", "batched"):
            key = "shifts-" + many
            np.testing.assert_array_equal(got[key][0], want[key][0], err_msg="%s: %s X" % (what, key))
            assert got[key][1:] == want[key][1:], (what, key, got[key][1:], want[key][1:])

    s = _new_solver(cm, ctx, A)
    try:
        s.ilu0()
        lu1 = s.ilu0_values()
        if solve_first:
            _observe_ilu(cm, ctx, s, None, n, b, x0)
        _set(ctx, s, v2)
        assert (s.set_values_info()[2] > 0) == solve_first           # the permuted matrix' map, when that matrix exists
        np.testing.assert_array_equal(s.ilu0_values(), lu1)          # (a) the factors lag
        got = {}
        for dj, key in ((None, "A0"), (d, "d")):
            _with_device(ctx, dj, lambda dd: s.ilu0_refactor(dd))
            got[key] = everything(s, dj)
        assert not np.array_equal(got["A0"]["lu"], lu1)
    finally:
        s.close()
    for dj, key in ((None, "A0"), (d, "d")):
        f = _new_solver(cm, ctx, A, v2)
        try:
            _with_device(ctx, dj, lambda dd: f.ilu0(shift=dd))
            want = everything(f, dj)
        finally:
            f.close()
        same(got[key], want, "%s refactor(%s)" % (form, key))


def test_permuted_matrix_follows_its_storage_class(cm, ctx, oracle, golden_dir, sw):
    """rand_rows(21000, 50) (a value dictionary), split factors, the loop in level-major spaces with its permuted matrix built:
    2 v1 (dictionary -> dictionary: the permuted copy's indices are gathered through its map) -> reals (no dictionary: the copy
    is dropped and built again at the next preconditioned solve) -> v1 (dictionary again); after each link and ilu0_refactor the
    factors, M^-1 and the preconditioned solve are those of a fresh solver"""
    sw("TRSV_HYBRID", 1)
    sw("TRSV_PERM", 1)
    name = "rand21000x50"
    A, reals, b, x0 = _system(oracle, golden_dir, name)
    n = A.n
    twice = 2.0 * A.val
    assert len(np.unique(twice)) == len(np.unique(A.val)) <= 256
    s = _new_solver(cm, ctx, A)
    try:
        s.ilu0()
        _observe_ilu(cm, ctx, s, None, n, b, x0)                     # (builds the permuted matrix)
        for link, (v, rebuilt_want) in enumerate(((twice, 0), (reals, 1), (A.val, 1)), start=1):
            _set(ctx, s, v)
            count, _, nbytes, rebuilt = s.set_values_info()
            assert (count, rebuilt) == (link, rebuilt_want)
            assert (nbytes > 0) == (rebuilt == 0)                    # the map goes with the copy it belongs to
            s.ilu0_refactor()
            got = _observe_ilu(cm, ctx, s, None, n, b, x0)
            f = _new_solver(cm, ctx, A, v)
            try:
                f.ilu0()
                want = _observe_ilu(cm, ctx, f, None, n, b, x0)
            finally:
                f.close()
            _same_ilu(got, want, "link %d" % link)
    finally:
        s.close()


@pytest.mark.parametrize("name", ["mat900", "mat10000"])
def test_stale_factors_still_precondition(cm, ctx, oracle, golden_dir, name):
    """directly after set_values(v2) the factors of v1 are a lagged preconditioner: a PRECOND_ILU0 solve of the v2 system from
    x0 = 1 at tol 1e-8 converges to a true residual <= 1e-7 ||r0||.  The oracle with the same stale factors takes
    12 iterations on mat900 and 38 on mat10000 (fresh factors: 11 and 32), all four below 1e-8 ||r0||."""
    A, v2, b, _ = _system(oracle, golden_dir, name)
    n = A.n
    A2 = _with(A, oracle, v2)
    ones = np.ones(n)
    s = _new_solver(cm, ctx, A)
    try:
        s.ilu0()
        lu1 = s.ilu0_values()
        _set(ctx, s, v2)
        np.testing.assert_array_equal(s.ilu0_values(), lu1)
        st, x, _ = _solve(cm, ctx, s, b, ones, precond=cm.PRECOND_ILU0, loop=cm.LOOP_PBICGSTAB, maxit=2000, tol=1e-8)
        s.ilu0_refactor()
        st_new, x_new, _ = _solve(cm, ctx, s, b, ones, precond=cm.PRECOND_ILU0, loop=cm.LOOP_PBICGSTAB, maxit=2000, tol=1e-8)
    finally:
        s.close()
    nrm0 = np.linalg.norm(b - oracle.spmv(A2, ones))
    res, res_new = np.linalg.norm(b - oracle.spmv(A2, x)), np.linalg.norm(b - oracle.spmv(A2, x_new))
    print(name, "stale factors: iters", st.iters, "residual / nrm0", res / nrm0, "-- refactored: iters", st_new.iters, "residual / nrm0", res_new / nrm0)
    assert st.converged and res <= 1e-7 * nrm0
    assert st_new.converged and res_new <= 1e-7 * nrm0


def test_the_set_up_is_not_repeated(cm, ctx, oracle, golden_dir, sw, capfd):
    """VERBOSE = 1, split factors, loop in level-major spaces, the permuted matrix built: exactly one set_values line per call,
    none of the set-up's stamps (not even from the temporary builds behind the maps of the first call), the placement as before"""
    sw("TRSV_HYBRID", 1)
    sw("TRSV_PERM", 1)
    sw("SPMV_MODE", "pb")
    sw("VERBOSE", 1)
    A, v2, b, x0 = _system(oracle, golden_dir, "rand20000x50")
    n = A.n
    s = _new_solver(cm, ctx, A)
    try:
        s.ilu0()
        _products(ctx, s, n)
        _observe_ilu(cm, ctx, s, None, n, b, x0)
        err = capfd.readouterr().err
        assert "ilu0 permuted matrix" in err and "create validation" in err and VALUES_LINE not in err
        placement = s.placement()
        for call, v in enumerate((v2, A.val, v2), start=1):
            _set(ctx, s, v)
            err = capfd.readouterr().err
            assert err.count(VALUES_LINE) == 1, err
            assert ("value maps built" in err) == (call == 1), err
            for gone in SETUP_STAMPS + ("pb plan", "pb arrays", "SpMV form"):
                assert gone not in err, (gone, err)
            assert s.placement() == placement
        maps = s.set_values_info()[2]
        assert maps > 0
        s.ilu0_refactor()
        got = _observe_ilu(cm, ctx, s, None, n, b, x0)
        prod = _products(ctx, s, n)
        err = capfd.readouterr().err
        assert err.count(REFACTOR_LINE) == 1 and VALUES_LINE not in err
        for gone in SETUP_STAMPS:
            assert gone not in err, (gone, err)
        assert s.set_values_info()[2] == maps and s.placement() == placement
    finally:
        s.close()
    sw("VERBOSE", 0)
    f = _new_solver(cm, ctx, A, v2)
    try:
        f.ilu0()
        _same_products(prod, _products(ctx, f, n), "after three calls")
        _same_ilu(got, _observe_ilu(cm, ctx, f, None, n, b, x0), "after three calls")
    finally:
        f.close()


# ------------------------------------------------------------------ 5. refusals
def test_refusals_leave_the_solver_as_it_was(cm, ctx, oracle, golden_dir, sw):
    A = _matrix(oracle, golden_dir, "rand600x50")
    v = _values(oracle, golden_dir, "rand600x50", "ints7")
    s = _new_solver(cm, ctx, A)
    try:
        before = _products(ctx, s, A.n)
        with pytest.raises(cm.CudamatError) as e:
            s.set_values(None)
        assert e.value.code == ERR_ARG and "val is NULL" in str(e.value)
        assert s.set_values_info() == (0, 0.0, 0, 0)
        _same_products(_products(ctx, s, A.n), before, "after the refused call")
    finally:
        s.close()
    sw("FORCE_SHARDED", 1)
    comm = cm.Comm()
    cm._lib.check(cm.lib().cudamat_comm_dry_create(ctx.h, 0, 1, C.byref(comm)))
    s = _new_solver(cm, ctx, A)
    try:
        s.set_comm(comm)
        before = _spmv(ctx, s, A.n)
        with pytest.raises(cm.CudamatError) as e:
            _set(ctx, s, v)
        assert e.value.code == ERR_ARG and "sharded" in str(e.value)
        assert s.set_values_info() == (0, 0.0, 0, 0)
        np.testing.assert_array_equal(_spmv(ctx, s, A.n), before)
    finally:
        s.close()
        cm.lib().cudamat_comm_dry_destroy(C.byref(comm))


# ------------------------------------------------------------------ 6. the drop-in calls
def _drop_in_calls(cm, A, b, n):
    """name -> (fn(val) -> (x, iters), uses ILU(0))"""
    ones = np.ones(n)
    d = 0.5 + np.arange(n) / n
    B = np.stack([b, 2.0 * b, b[::-1]], axis=1)
    D = np.stack([d, 2.0 * d, 0.5 * d], axis=1)
    it = lambda sts: [t.iters for t in sts]

    def one(r):
        return r[1], r[3].iters

    def many(r):
        return r[1], it(r[3])

    return {
        "bicgstab": (lambda v: one(cm.bicgstab(n, A.nnz, v, A.rowptr, A.colidx, b, 60, 1e-8)), False),
        "bicgstab_d": (lambda v: one(cm.bicgstab_d(n, A.nnz, v, A.rowptr, A.colidx, d, ones, b, 60, 1e-8)), False),
        "bicgstab_lu_precond": (lambda v: one(cm.bicgstab_lu_precond(n, A.nnz, v, A.rowptr, A.colidx, b, 60, 1e-8)), True),
        "bicgstab_d_lu_precond": (lambda v: one(cm.bicgstab_d_lu_precond(n, A.nnz, v, A.rowptr, A.colidx, d, ones, b, 60, 1e-8)), True),
        "bicgstab_many": (lambda v: many(cm.bicgstab_many(n, A.nnz, v, A.rowptr, A.colidx, B, 60, 1e-8)), False),
        # (one set of factors per column, made inside the call: how many of them are refactorisations is not this test's matter)
        "bicgstab_d_lu_precond_many": (lambda v: many(cm.bicgstab_d_lu_precond_many(n, A.nnz, v, A.rowptr, A.colidx, D, None, B, 60, 1e-8)), None),
    }


@pytest.mark.parametrize("name", ["mat10000", "rand20000x50"])
@pytest.mark.parametrize("entry", ["bicgstab", "bicgstab_d", "bicgstab_lu_precond", "bicgstab_d_lu_precond", "bicgstab_many",
                                   "bicgstab_d_lu_precond_many"])
def test_drop_in_call_refreshes_a_cached_plan(cm, oracle, golden_dir, monkeypatch, capfd, name, entry):
    """(pattern, v1) then (pattern, v2) under VERBOSE = 1: the second call prints the set_values line (and the refactor line where
    the solver's own ILU(0) factors serve the solve), no `create validation`, and returns the x and iteration counts of the same
    call under PLAN_CACHE = 0, bit for bit; VALUES_REFRESH = 0 validates a new solver instead, with the same result."""
    A, v2, b, _ = _system(oracle, golden_dir, name)
    fn, refactors = _drop_in_calls(cm, A, b, A.n)[entry]
    monkeypatch.setenv("CUDAMAT_VERBOSE", "1")

    def call(v):
        capfd.readouterr()
        x, iters = fn(v)
        return x, iters, capfd.readouterr().err

    cm.lib().cudamat_plan_cache_clear()
    try:
        call(A.val)
        x, iters, err = call(v2)
        assert err.count(VALUES_LINE) == 1 and "create validation" not in err, err
        if refactors is not None:
            assert err.count(REFACTOR_LINE) == (1 if refactors else 0), err
        x_again, iters_again, err = call(v2)                         # the same matrix once more: a plain reuse
        assert VALUES_LINE not in err and "create validation" not in err, err
        assert refactors is None or REFACTOR_LINE not in err, err
        monkeypatch.setenv("CUDAMAT_VALUES_REFRESH", "0")
        cm.lib().cudamat_plan_cache_clear()
        call(A.val)
        x_old, iters_old, err = call(v2)
        assert VALUES_LINE not in err and "create validation" in err, err
        monkeypatch.delenv("CUDAMAT_VALUES_REFRESH")
        monkeypatch.setenv("CUDAMAT_PLAN_CACHE", "0")
        x_alone, iters_alone, err = call(v2)
        assert VALUES_LINE not in err and "create validation" in err, err
    finally:
        cm.lib().cudamat_plan_cache_clear()
    for other, other_iters, what in ((x_again, iters_again, "reused"), (x_old, iters_old, "VALUES_REFRESH=0"), (x_alone, iters_alone, "PLAN_CACHE=0")):
        np.testing.assert_array_equal(x, other, err_msg="%s %s against %s" % (name, entry, what))
        assert iters == other_iters, (what, iters, other_iters)


# ------------------------------------------------------------------ 7. memory
def test_nothing_stays_behind(cm, ctx, oracle, golden_dir, sw):
    """cudamat_mem_live after three set_values calls is what it was after the first (the maps are built once, every temporary is
    gone), and after close() what it was before the solver -- with the blocked copy, split factors and the permuted matrix"""
    sw("TRSV_HYBRID", 1)
    sw("SPMV_MODE", "pb")
    A, v2, b, x0 = _system(oracle, golden_dir, "mat10000")
    ctx.sync()
    before = _live(cm)
    s = _new_solver(cm, ctx, A)
    try:
        s.ilu0()
        _products(ctx, s, A.n)
        _observe_ilu(cm, ctx, s, None, A.n, b, x0)
        built = _live(cm)
        _set(ctx, s, v2)
        first = _live(cm)
        assert s.set_values_info()[2] > 0 and first > built          # the maps are device memory the solver owns
        _set(ctx, s, A.val)
        _set(ctx, s, v2)
        assert _live(cm) == first
        s.ilu0_refactor()
        _observe_ilu(cm, ctx, s, None, A.n, b, x0)
    finally:
        s.close()
    ctx.sync()
    assert _live(cm) == before
