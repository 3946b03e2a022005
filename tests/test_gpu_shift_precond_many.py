"""One set of ILU(0) factors per column: (A0 + diag D_j) x_j = b_j with M_j = ILU(0)(A0 + diag D_j) -- the K-wide numeric
factorisation (csrc/ilu.hip), the triangular solves with per-column values (csrc/trsv.hip), the batched loop on top
(cudamat_solver_solve_shifts_ilu0, csrc/loops_batch.hip) and the drop-in function.
 1. factors, bit for bit against ilu0(shift = D_j) -> ilu0_values(), and against the oracle;
 2. triangular solves, bit for bit against precond_apply on a solver holding ilu0(shift = D_j), and against the oracle;
 3. the loop against the oracle, column by column;
 4. a column does not depend on its batch (which is also the freeze test);
 5. the column form is the caller's loop, bit for bit;
 6. per-column factors matter (fails with any shortcut that shares one factor set);
 7. state and errors;  8. MANY_PRECOND = auto;  9. the drop-in function.
Shifts D_j = m_j (0.5 + i / n), b_j = E_j ((1 + sin i)(1 + 0.1 m_j)) with E_j the explicit matrix, x0 = 1.  The oracle alone gives,
at tol 1e-8, for m = 0, 0.01, 0.03, 0.1, 0.25, 0.5, 1, 2, 4: 10 10 10 8 7 6 5 4 3 iterations on mat900 and 16 21 17 12 9 7 6 4 3
on mat10000, each unchanged when b moves by a few ulp -- so the +-max(2, 10 %) rule is fair to every column.
Run on the GPU box with:  python -m pytest tests -m gpu"""
import functools
import os
import re

import numpy as np
import pytest

from tests.test_gpu_long_rows import _matrix as _long_matrix
from tests.test_gpu_many_precond import _block, _check_against_oracle, _unblock, _wide_levels
from tests.test_gpu_shift_precond import _diag_mask, _explicit

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_ZERO_PIVOT = 2, 3
OLD_MESSAGE = "has no preconditioner"
M900 = (0.01, 0.03, 0.1, 0.25, 0.5, 1.0, 2.0, 4.0)          # test 3: all eight m > 0 of the table
M10000 = (0.01, 0.1, 0.5, 2.0, 4.0)
M_ANY = (0.5, 0.0, 1.0, 2.0, 4.0, 0.25, 0.1, 0.03, 0.01)      # factors and triangular solves: the first nrhs of these


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
    """a library switch for the rest of this test, on the shared context and in the environment (the drop-in function)"""
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


# ------------------------------------------------------------------ systems, shifts, right-hand sides
@functools.lru_cache(maxsize=None)
def _system(oracle, golden_dir, name):
    if name == "wide":
        return _wide_levels(oracle)
    if name == "few":
        return _long_matrix(oracle, "few", diag_dominant=True)
    return oracle.mtx_load(os.path.join(golden_dir, name + ".mtx"))


def _shift(n, m):
    return m * (0.5 + np.arange(n) / n)


@functools.lru_cache(maxsize=None)
def _column(oracle, golden_dir, name, m):
    """(d, E, b) of one column: computed once, shared, not to be written"""
    A0 = _system(oracle, golden_dir, name)
    d = _shift(A0.n, m)
    E = _explicit(oracle, A0, d)
    b = oracle.spmv(E, (1.0 + np.sin(np.arange(A0.n))) * (1.0 + 0.1 * m))
    for a in (d, b):
        a.setflags(write=False)
    return d, E, b


def _family(oracle, golden_dir, name, ms):
    cols = [_column(oracle, golden_dir, name, m) for m in ms]
    return np.stack([c[0] for c in cols], axis=1), [c[1] for c in cols], np.stack([c[2] for c in cols], axis=1)


_REF_VALUES = {}


def _ref_values(cm, ctx, oracle, golden_dir, name, m):
    """ilu0(shift = D_j) -> ilu0_values() on a solver of its own, once per (system, m)"""
    key = (name, m)
    if key not in _REF_VALUES:
        A0 = _system(oracle, golden_dir, name)
        s = cm.Solver.from_host_csr(ctx, A0.rowptr, A0.colidx, A0.val)
        dd = ctx.array(_column(oracle, golden_dir, name, m)[0])
        try:
            s.ilu0(shift=dd)
            v = s.ilu0_values()
        finally:
            dd.free()
            s.close()
        v.setflags(write=False)
        _REF_VALUES[key] = v
    return _REF_VALUES[key]


def _new_solver(cm, ctx, A0):
    return cm.Solver.from_host_csr(ctx, A0.rowptr, A0.colidx, A0.val)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _solve_family(cm, ctx, s, D, B, ldd=None, ldb=None, ldx=None, X0=None, **kw):
    """solve_shifts_ilu0 on device blocks with leading dimensions above n (NaN in the pad rows): (X, stats, histories, form)"""
    n, k = B.shape
    ldd, ldb, ldx = ldd or n + 1, ldb or n + 3, ldx or n + 5
    dD, dB = _block(ctx, D, ldd), _block(ctx, B, ldb)
    dX = _block(ctx, np.ones((n, k)) if X0 is None else X0, ldx)
    try:
        sts, form = s.solve_shifts_ilu0(k, dD, ldd, dB, ldb, dX, ldx, **kw)
        raw = dX.download().reshape(k, ldx)
        assert np.all(np.isnan(raw[:, n:]))                            # the pad rows of X are not touched
        return raw[:, :n].T.copy(), sts, [s.history(col=j) for j in range(k)], form
    finally:
        for q in (dD, dB, dX):
            q.free()


# ------------------------------------------------------------------ 1. factors
@pytest.mark.parametrize("name,nrhs", [(nm, k) for nm in ("mat900", "wide") for k in (1, 2, 3, 5, 8, 9)] + [("few", 1), ("few", 2)])
def test_factors_bit_for_bit(cm, ctx, oracle, golden_dir, sw, name, nrhs):
    """column j of ilu0_shifts_values (k_ilu0_level<K, WAVES>) == ilu0(shift = D_j) -> ilu0_values() as raw bits: mat900 (base 1,
    rows of 7: the set-up's k_ilu0_level_fast), the matrix with wide levels, and `few` (rows of 6000 entries: the set-up's
    one-wave k_ilu0_level_simple<1>); nrhs 1, 2, 3, 5, 8,
    9 = padding to 4 and 8 and a second block.  On `few` a block of one column fits the LDS limit (7616 entries) and a block of
    two does not (5376): the second runs column by column and must give the same bits.  Which form ran shows in the solver's
    own factors afterwards: K-wide leaves them those of D_0 (the structure's set-up), column by column those of the last
    column.  Columns 0 and nrhs - 1 also against the oracle's ilu0(E_j) at rtol 1e-12."""
    sw("MANY_PRECOND", "batched")
    A0 = _system(oracle, golden_dir, name)
    ms = M_ANY[:nrhs]
    D, Es, _ = _family(oracle, golden_dir, name, ms)
    want = [_ref_values(cm, ctx, oracle, golden_dir, name, m) for m in ms]
    s = _new_solver(cm, ctx, A0)
    ldd = A0.n + 2
    dD = _block(ctx, D, ldd)
    try:
        got = s.ilu0_shifts_values(nrhs, dD, ldd)
        own = s.ilu0_values()
    finally:
        dD.free()
        s.close()
    assert got.shape == (A0.nnz, nrhs)
    for j in range(nrhs):
        np.testing.assert_array_equal(_bits(got[:, j]), _bits(want[j]), err_msg="column %d" % j)
    for j in {0, nrhs - 1}:
        np.testing.assert_allclose(got[:, j], oracle.ilu0(Es[j]), rtol=1e-12, atol=1e-14)
    covered = not (name == "few" and nrhs == 2)
    np.testing.assert_array_equal(_bits(own), _bits(want[0] if covered else want[-1]))
    if nrhs >= 2:
        assert not np.array_equal(want[0], want[-1])


# ------------------------------------------------------------------ 2. triangular solves
@pytest.mark.parametrize("name,nrhs,kernels", [("mat900", 8, ("k_trsm_lds<",)), ("mat10000", 2, ("k_trsm_small_levels<",)),
                                               ("wide", 3, ("k_trsm_level<", "k_trsm_small_levels<")), ("mat900", 9, ("k_trsm_lds<",))])
def test_triangular_solves_bit_for_bit(cm, ctx, oracle, golden_dir, sw, name, nrhs, kernels):
    """column j of precond_apply_shifts == precond_apply on a solver holding ilu0(shift = D_j), bit for bit, leading dimensions
    above n with NaN in the pad rows: mat900 with K = 8 runs k_trsm_lds, mat10000 with K = 2 (n K > 16384) the runs of narrow
    levels, the matrix with wide levels k_trsm_level and k_trsm_small_levels (the form depends on the pattern and K only:
    Solver.trsm_kernel says which); 9 columns = a second block.  Columns 0 and nrhs - 1 against the oracle's substitutions, 1e-10."""
    sw("MANY_PRECOND", "batched")
    A0 = _system(oracle, golden_dir, name)
    n = A0.n
    ms = M_ANY[:nrhs]
    D, Es, _ = _family(oracle, golden_dir, name, ms)
    R = np.random.default_rng(5).standard_normal((n, nrhs))
    ldd, ldin, ldout = n + 1, n + 3, n + 5
    s = _new_solver(cm, ctx, A0)
    dD, dIn, dOut = _block(ctx, D, ldd), _block(ctx, R, ldin), _block(ctx, np.zeros((n, nrhs)), ldout)
    try:
        s.precond_apply_shifts(nrhs, dD, ldd, dIn, ldin, dOut, ldout)
        Y = dOut.download().reshape(nrhs, ldout)
        nm = s.trsm_kernel(min(nrhs, 8))
        own = s.ilu0_values()
    finally:
        for q in (dD, dIn, dOut):
            q.free()
        s.close()
    print(name, nrhs, nm)
    for kname in kernels:
        assert kname in nm, nm
    if name != "mat900":
        assert "k_trsm_lds" not in nm, nm
    np.testing.assert_array_equal(_bits(own), _bits(_ref_values(cm, ctx, oracle, golden_dir, name, ms[0])))      # K-wide: D_0's stay
    r = _new_solver(cm, ctx, A0)
    try:
        for j in range(nrhs):
            dd, dr, do = ctx.array(D[:, j]), ctx.array(R[:, j]), ctx.empty(n)
            try:
                r.ilu0(shift=dd)
                r.precond_apply(dr, do)
                np.testing.assert_array_equal(_bits(Y[j, :n]), _bits(do.download()), err_msg="column %d" % j)
            finally:
                for q in (dd, dr, do):
                    q.free()
            assert np.all(np.isnan(Y[j, n:]))
            if j in (0, nrhs - 1):
                vm = oracle.ilu0(Es[j])
                ref = oracle.trsv_upper(Es[j], vm, oracle.trsv_lower_unit(Es[j], vm, R[:, j]))
                np.testing.assert_allclose(Y[j, :n], ref, rtol=1e-10, atol=1e-12)
    finally:
        r.close()


# ------------------------------------------------------------------ 3. the loop against the oracle
LOOP_CASES = [("mat900", M900), ("mat10000", M10000)]


@functools.lru_cache(maxsize=None)
def _batched_run(cm, ctx, oracle, golden_dir, name, ms):
    """the full block of test 3 under MANY_PRECOND = batched (the caller sets the switch): computed once, shared with tests 4, 5"""
    A0 = _system(oracle, golden_dir, name)
    D, Es, B = _family(oracle, golden_dir, name, ms)
    s = _new_solver(cm, ctx, A0)
    try:
        X, sts, hs, form = _solve_family(cm, ctx, s, D, B, maxit=2000, tol=1e-8)
    finally:
        s.close()
    X.setflags(write=False)
    return X, [(st.iters, st.half_exit, st.converged, st.nrm0, st.t_factor) for st in sts], sts, hs, form


@pytest.mark.parametrize("name,ms", LOOP_CASES)
def test_loop_against_the_oracle(cm, ctx, oracle, golden_dir, sw, name, ms):
    """solve_shifts_ilu0, batched: every column against oracle.pbicgstab(E_j, b_j, vm = oracle.ilu0(E_j)) by the tolerances of
    _check_against_oracle (count within max(2, 10 %), x to 1e-5, true residual <= 10 tol ||r0||, first six history entries to
    1e-8, history length 2 iters (+1 on a half exit)); form == 1; t_factor is the block's factorisation"""
    sw("MANY_PRECOND", "batched")
    D, Es, B = _family(oracle, golden_dir, name, ms)
    X, _, sts, hs, form = _batched_run(cm, ctx, oracle, golden_dir, name, ms)
    assert form == 1
    for j in range(len(ms)):
        print(name, "m", ms[j], end=" ")
        _check_against_oracle(oracle, Es[j], oracle.ilu0(Es[j]), B[:, j], X[:, j], sts[j], hs[j], 1e-8)
        assert sts[j].t_factor > 0.0 and sts[j].t_factor == sts[0].t_factor


# ------------------------------------------------------------------ 4. a column does not depend on its batch
@pytest.mark.parametrize("name,ms,j", [("mat900", M900, 2), ("mat10000", M10000, 1), ("mat10000", M10000, 4)])
def test_a_column_does_not_depend_on_its_batch(cm, ctx, oracle, golden_dir, sw, name, ms, j):
    """column j of test 3 alone (nrhs = 1, batched all the same: K = 1 of the K-wide kernels), as the second column of a block of
    2, and in the full block: x and the history are bit-identical each time.  The columns of the full block stop after 3 to 21
    iterations, so this is the freeze test too: a stopped column's x keeps its bits while the others run on."""
    sw("MANY_PRECOND", "batched")
    A0 = _system(oracle, golden_dir, name)
    D, Es, B = _family(oracle, golden_dir, name, ms)
    Xf, _, stf, hf, _ = _batched_run(cm, ctx, oracle, golden_dir, name, ms)
    other = (j + 1) % len(ms)
    s = _new_solver(cm, ctx, A0)
    try:
        X1, st1, h1, form1 = _solve_family(cm, ctx, s, D[:, [j]], B[:, [j]], maxit=2000, tol=1e-8)
        X2, st2, h2, form2 = _solve_family(cm, ctx, s, D[:, [other, j]], B[:, [other, j]], maxit=2000, tol=1e-8)
    finally:
        s.close()
    assert form1 == 1 and form2 == 1
    assert (st1[0].iters, st1[0].half_exit) == (st2[1].iters, st2[1].half_exit) == (stf[j].iters, stf[j].half_exit)
    for x, h in ((X1[:, 0], h1[0]), (X2[:, 1], h2[1])):
        np.testing.assert_array_equal(_bits(h), _bits(hf[j]))
        np.testing.assert_array_equal(_bits(x), _bits(Xf[:, j]))
    np.testing.assert_array_equal(_bits(X2[:, 0]), _bits(Xf[:, other]))
    assert len({st.iters for st in stf}) > 1                            # the columns of the full block do stop at different times


# ------------------------------------------------------------------ 5. the column form is the caller's loop
@pytest.mark.parametrize("name,ms", LOOP_CASES)
def test_column_form_is_the_callers_loop(cm, ctx, oracle, golden_dir, sw, name, ms):
    """the same call under MANY_FORM = columns: form == 0; x and history bit-identical to set_shift(D_j) + ilu0(shift = D_0) /
    ilu0_refactor(D_j) + solve(precond = ILU0) written out here; within test 3's tolerances of the oracle and of the batched
    result; the solver's own shift is what it was before the call (its SpMV still adds it)"""
    A0 = _system(oracle, golden_dir, name)
    n = A0.n
    D, Es, B = _family(oracle, golden_dir, name, ms)
    sw("MANY_PRECOND", "batched")
    Xb, _, stb, hb, _ = _batched_run(cm, ctx, oracle, golden_dir, name, ms)
    sw("MANY_FORM", "columns")
    d_own = 0.125 + np.cos(np.arange(n)) ** 2
    xs = 1.0 + np.sin(0.3 * np.arange(n))
    s = _new_solver(cm, ctx, A0)
    dd_own, dxs, dy0, dy1 = ctx.array(d_own), ctx.array(xs), ctx.empty(n), ctx.empty(n)
    try:
        s.set_shift(dd_own)
        s.spmv(dxs, dy0)
        X, sts, hs, form = _solve_family(cm, ctx, s, D, B, maxit=2000, tol=1e-8)
        s.spmv(dxs, dy1)
        np.testing.assert_array_equal(_bits(dy1.download()), _bits(dy0.download()))
        own_after = s.ilu0_values()
    finally:
        for q in (dd_own, dxs, dy0, dy1):
            q.free()
        s.close()
    assert form == 0
    np.testing.assert_array_equal(_bits(own_after), _bits(_ref_values(cm, ctx, oracle, golden_dir, name, ms[-1])))     # the last column's
    # the caller's loop on the caller's own blocks: the same leading dimensions as _solve_family's, so every column starts where
    # it started there relative to a 16-byte boundary (the single solve's vector kernels choose their form by that)
    k = len(ms)
    ldd, ldb, ldx = n + 1, n + 3, n + 5
    c = _new_solver(cm, ctx, A0)
    dD, dB, dX = _block(ctx, D, ldd), _block(ctx, B, ldb), _block(ctx, np.ones((n, k)), ldx)
    try:
        for j in range(k):
            dj = dD.ptr + 8 * j * ldd
            c.set_shift(dj)
            if j == 0:
                c.ilu0(shift=dj)
            else:
                c.ilu0_refactor(dj)
            st = c.solve(dB.ptr + 8 * j * ldb, dX.ptr + 8 * j * ldx, precond=cm.PRECOND_ILU0, loop=cm.LOOP_PBICGSTAB, maxit=2000, tol=1e-8)
            assert (st.iters, st.half_exit, st.converged) == (sts[j].iters, sts[j].half_exit, sts[j].converged)
            np.testing.assert_array_equal(_bits(c.history()), _bits(hs[j]), err_msg="column %d" % j)
        c.set_shift(None)
        np.testing.assert_array_equal(_bits(_unblock(dX, n, k, ldx)), _bits(X))
    finally:
        for q in (dD, dB, dX):
            q.free()
        c.close()
    for j in range(len(ms)):
        _check_against_oracle(oracle, Es[j], oracle.ilu0(Es[j]), B[:, j], X[:, j], sts[j], hs[j], 1e-8)
        assert abs(sts[j].iters - stb[j].iters) <= max(2, 0.1 * stb[j].iters)
        assert np.linalg.norm(X[:, j] - Xb[:, j]) / np.linalg.norm(Xb[:, j]) <= 1e-5
        k = min(len(hs[j]), len(hb[j]), 6)
        np.testing.assert_allclose(hs[j][:k], hb[j][:k], rtol=1e-8)


# ------------------------------------------------------------------ 6. per-column factors matter
def test_per_column_factors_matter(cm, ctx, oracle, golden_dir, sw):
    """mat10000, the columns m = 0.01 and m = 4 in one block: their factor values differ (not allclose at rtol 1e-6), and the
    m = 4 column converges in the oracle's 3 iterations (+-2) -- with the factors of m = 0.01, which any shortcut that shares one
    factor set would hand it, the oracle needs 13 and a single solve here at least 3 more than with its own"""
    sw("MANY_PRECOND", "batched")
    name, ms = "mat10000", (0.01, 4.0)
    A0 = _system(oracle, golden_dir, name)
    n = A0.n
    D, Es, B = _family(oracle, golden_dir, name, ms)
    s = _new_solver(cm, ctx, A0)
    dD = _block(ctx, D, n)
    try:
        V = s.ilu0_shifts_values(2, dD, n)
        X, sts, hs, form = _solve_family(cm, ctx, s, D, B, maxit=2000, tol=1e-8)
    finally:
        dD.free()
        s.close()
    assert form == 1
    assert not np.allclose(V[:, 0], V[:, 1], rtol=1e-6)
    xo, so, _ = oracle.pbicgstab(Es[1], B[:, 1], vm=oracle.ilu0(Es[1]), maxit=2000, tol=1e-8, want_hist=True)
    xs, ss, _ = oracle.pbicgstab(Es[1], B[:, 1], vm=oracle.ilu0(Es[0]), maxit=2000, tol=1e-8, want_hist=True)
    assert (so.iters, ss.iters) == (3, 13)
    for j in range(2):
        _check_against_oracle(oracle, Es[j], oracle.ilu0(Es[j]), B[:, j], X[:, j], sts[j], hs[j], 1e-8)
    # stale factors on the GPU: the factors of m = 0.01 under the shift of m = 4
    c = _new_solver(cm, ctx, A0)
    d0, d1, db, dx = ctx.array(D[:, 0]), ctx.array(D[:, 1]), ctx.array(B[:, 1]), ctx.array(np.ones(n))
    try:
        c.ilu0(shift=d0)
        c.set_shift(d1)
        stale = c.solve(db, dx, precond=cm.PRECOND_ILU0, loop=cm.LOOP_PBICGSTAB, maxit=2000, tol=1e-8)
    finally:
        c.set_shift(None)
        for q in (d0, d1, db, dx):
            q.free()
        c.close()
    print("m = 4: iters", sts[1].iters, "oracle", so.iters, "| with the factors of m = 0.01:", stale.iters, "oracle", ss.iters)
    assert stale.converged and stale.iters >= sts[1].iters + 3


# ------------------------------------------------------------------ 7. state and errors
def test_held_factors_keep_their_bits_through_a_batched_call(cm, ctx, oracle, golden_dir, sw):
    """a solver that holds ilu0(shift = d_held), d_held none of the call's columns: ilu0_values() is bit-identical after a batched
    call, and the solver's shift is still its own"""
    sw("MANY_PRECOND", "batched")
    name, ms = "mat900", M900[:5]
    A0 = _system(oracle, golden_dir, name)
    D, Es, B = _family(oracle, golden_dir, name, ms)
    held = _ref_values(cm, ctx, oracle, golden_dir, name, 8.0)
    s = _new_solver(cm, ctx, A0)
    dh = ctx.array(_column(oracle, golden_dir, name, 8.0)[0])
    try:
        s.ilu0(shift=dh)
        np.testing.assert_array_equal(_bits(s.ilu0_values()), _bits(held))
        X, sts, hs, form = _solve_family(cm, ctx, s, D, B, maxit=2000, tol=1e-8)
        after = s.ilu0_values()
        assert s.ilu0_shifted() is True
    finally:
        dh.free()
        s.close()
    assert form == 1 and all(st.converged for st in sts)
    np.testing.assert_array_equal(_bits(after), _bits(held))
    Xb = _batched_run(cm, ctx, oracle, golden_dir, name, M900)[0]
    np.testing.assert_array_equal(_bits(X), _bits(Xb[:, :5]))           # ... and what it held had no part in the result


@pytest.mark.parametrize("zero_col", [0, 2])
def test_zero_pivot_names_column_and_row(cm, ctx, oracle, golden_dir, sw, zero_col):
    """mat900 with its diagonal moved into d (the "moved" system of test_factors_of_the_shifted_matrix) and one column of D equal
    to 0: code 3, the message names the column and the row (K-wide: row 0, the first zero pivot), X is untouched, the solver is still
    usable -- a following call with every column the moved diagonal succeeds and agrees with the oracle on mat900 itself"""
    sw("MANY_PRECOND", "batched")
    A = _system(oracle, golden_dir, "mat900")
    n = A.n
    rows, mask = _diag_mask(A)
    d = np.zeros(n)
    d[rows[mask]] = A.val[mask]
    val = A.val.copy()
    val[mask] = 0.0
    A0 = oracle.Csr(n, A.rowptr.copy(), A.colidx.copy(), val, n)
    D = np.stack([d, d, d], axis=1)
    D[:, zero_col] = 0.0
    B = np.stack([oracle.spmv(A, 1.0 + np.sin(np.arange(n)))] * 3, axis=1)          # (the m = 0 column of the table, three times)
    X0 = np.stack([np.full(n, 2.0 + j) for j in range(3)], axis=1)
    s = _new_solver(cm, ctx, A0)
    dD, dB, dX = _block(ctx, D, n), _block(ctx, B, n), _block(ctx, X0, n)
    try:
        with pytest.raises(cm.CudamatError) as e:
            s.solve_shifts_ilu0(3, dD, n, dB, n, dX, n, maxit=2000, tol=1e-8)
        print(e.value)
        assert e.value.code == ERR_ZERO_PIVOT
        if zero_col == 0:       # met while the solver's structure was set up from D_0: the single-column pass names its row
            assert re.search(r"column 0\b.*\brow \d+", str(e.value)), str(e.value)
        else:                   # met by the K-wide pass: the smallest (column, row) pair
            assert re.search(r"column 2, row 0\b", str(e.value)), str(e.value)
        np.testing.assert_array_equal(_unblock(dX, n, 3, n), X0)
        Dm = np.stack([d, d, d], axis=1)
        X, sts, hs, form = _solve_family(cm, ctx, s, Dm, B, maxit=2000, tol=1e-8)
    finally:
        for q in (dD, dB, dX):
            q.free()
        s.close()
    assert form == 1
    vm = oracle.ilu0(A)
    for j in range(3):
        _check_against_oracle(oracle, A, vm, B[:, j], X[:, j], sts[j], hs[j], 1e-8)
        np.testing.assert_array_equal(_bits(X[:, j]), _bits(X[:, 0]))      # equal columns, equal bits


def test_refusals_fallbacks_and_edge_calls(cm, ctx, oracle, golden_dir, sw):
    """solve_shifts(..., precond = ILU0) is still refused with the old message; FLAG_GUARD and FLAG_DEBUG take the column form
    (form 0) under MANY_PRECOND = batched and still agree with the oracle; nrhs = 0 is a no-op; maxit = 0 returns x0"""
    sw("MANY_PRECOND", "batched")
    name, ms = "mat900", (0.5, 2.0)
    A0 = _system(oracle, golden_dir, name)
    n = A0.n
    D, Es, B = _family(oracle, golden_dir, name, ms)
    s = _new_solver(cm, ctx, A0)
    dD, dB, dX = _block(ctx, D, n), _block(ctx, B, n), _block(ctx, np.ones((n, 2)), n)
    try:
        with pytest.raises(cm.CudamatError) as e:
            s.solve_shifts(2, dD, n, dB, n, dX, n, precond=cm.PRECOND_ILU0, loop=cm.LOOP_PBICGSTAB, maxit=5, tol=1e-8)
        assert e.value.code == ERR_ARG and OLD_MESSAGE in str(e.value)
        np.testing.assert_array_equal(dX.download(), np.ones(2 * n))
        sts, form = s.solve_shifts_ilu0(0, None, n, None, n, None, n)
        assert (sts, form) == ([], 0)
        for flags in (cm.FLAG_GUARD, cm.FLAG_DEBUG):
            X, sts, hs, form = _solve_family(cm, ctx, s, D, B, maxit=2000, tol=1e-8, flags=flags)
            assert form == 0, flags
            for j in range(2):
                assert sts[j].converged
                assert np.linalg.norm(B[:, j] - oracle.spmv(Es[j], X[:, j])) <= 1e-7 * sts[j].nrm0
        X0 = np.stack([1.0 + np.cos(np.arange(n)), np.full(n, 3.0)], axis=1)
        X, sts, hs, form = _solve_family(cm, ctx, s, D, B, X0=X0, maxit=0, tol=1e-8)
        assert form == 1 and [st.iters for st in sts] == [0, 0]
        np.testing.assert_array_equal(_bits(X), _bits(X0))
    finally:
        for q in (dD, dB, dX):
            q.free()
        s.close()


# ------------------------------------------------------------------ 8. auto
def test_auto_returns_a_valid_result(cm, ctx, oracle, golden_dir, sw):
    """MANY_PRECOND = auto times both forms (each with its factorisation) and takes one: whichever, every column is within test
    3's tolerances of the oracle, and factors the solver held keep their bits when the batched form was taken"""
    sw("MANY_PRECOND", "auto")
    name, ms = "mat900", M900
    A0 = _system(oracle, golden_dir, name)
    D, Es, B = _family(oracle, golden_dir, name, ms)
    held = _ref_values(cm, ctx, oracle, golden_dir, name, 8.0)
    s = _new_solver(cm, ctx, A0)
    dh = ctx.array(_column(oracle, golden_dir, name, 8.0)[0])
    try:
        s.ilu0(shift=dh)
        X, sts, hs, form = _solve_family(cm, ctx, s, D, B, maxit=2000, tol=1e-8)
        after = s.ilu0_values()
    finally:
        dh.free()
        s.close()
    print("auto took form", form, "t_tune", sts[0].t_tune)
    assert form in (0, 1) and sts[0].t_tune > 0.0
    for j in range(len(ms)):
        _check_against_oracle(oracle, Es[j], oracle.ilu0(Es[j]), B[:, j], X[:, j], sts[j], hs[j], 1e-8)
    if form == 1:
        np.testing.assert_array_equal(_bits(after), _bits(held))


# ------------------------------------------------------------------ 9. the drop-in function
@pytest.mark.parametrize("mode", ["batched", "columns"])
def test_drop_in(cm, ctx, oracle, golden_dir, sw, mode):
    """bicgstab_d_lu_precond_many on mat900: D as k scalars (d_j = sigma_j 1) and as an (n, k) block, against the oracle as in
    test 3; the second call -- the same matrix, other shifts -- reuses the plan"""
    sw("MANY_PRECOND", mode)
    name = "mat900"
    A0 = _system(oracle, golden_dir, name)
    n = A0.n
    sig = np.array([0.25, 1.0, 3.0])
    Dblock, Eb, Bb = _family(oracle, golden_dir, name, M900[2:7])
    Es = [_explicit(oracle, A0, np.full(n, sg)) for sg in sig]
    Bs = np.stack([oracle.spmv(E, 1.0 + np.sin(np.arange(n))) for E in Es], axis=1)
    cm.lib().cudamat_plan_cache_clear()
    try:
        ok1, X1, dt1, st1, form1 = cm.bicgstab_d_lu_precond_many(n, A0.nnz, A0.val, A0.rowptr, A0.colidx, sig, None, Bs, 2000, 1e-8)
        ok2, X2, dt2, st2, form2 = cm.bicgstab_d_lu_precond_many(n, A0.nnz, A0.val, A0.rowptr, A0.colidx, Dblock, np.ones((n, 5)), Bb,
                                                                 2000, 1e-8)
    finally:
        cm.lib().cudamat_plan_cache_clear()
    want_form = 1 if mode == "batched" else 0
    assert (form1, form2) == (want_form, want_form) and ok1 == [True] * 3 and ok2 == [True] * 5
    assert [st.plan_reused for st in st1] == [0] * 3 and [st.plan_reused for st in st2] == [1] * 5
    for E, B, X, sts in ((Es, Bs, X1, st1), (Eb, Bb, X2, st2)):
        for j in range(len(E)):
            xo, so, ho = oracle.pbicgstab(E[j], B[:, j], vm=oracle.ilu0(E[j]), maxit=2000, tol=1e-8, want_hist=True)
            assert sts[j].converged and abs(sts[j].iters - so.iters) <= max(2, 0.1 * so.iters)
            assert np.linalg.norm(X[:, j] - xo) / np.linalg.norm(xo) <= 1e-5
            assert np.linalg.norm(B[:, j] - oracle.spmv(E[j], X[:, j])) <= 1e-7 * so.nrm0
