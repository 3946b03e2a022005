"""Scale equivariance and the edges of the fp64 range (GPU).

In range.  BiCGSTAB is exactly equivariant under c = 2^k: (c b, c x0) multiplies every vector of the loop by c and every
dot product by c^2, so alpha, omega and beta keep their bits (a power of two commutes with rounding while nothing
overflows or goes subnormal).  x and the residual history must be c times the unscaled ones BITWISE, after the same
iterations through the same exit -- in every loop form, SpMV form and triangular solve, and per column in the batched loops.
An absolute constant, a stale value mixed into a sum, or padding that does not scale breaks this where no tolerance
against the oracle would notice.  tests/test_scaling_cpu.py shows the oracle has the property at the same exponents.
With ||r0|| ~ 135 on mat900 the smallest tol ||r0|| here is ~5e-139 and the largest sum of squares ~2^900.

Out of range.  The loops compare plain sums of squares; where those cannot be trusted (||r0|| inf, or 0 with r0 != 0, or
tol ||r0|| < 2^-485) a solve is refused at once (breakdown, no iteration, x0 untouched) instead of reporting a convergence
it has not computed.  dot propagates what it cannot hold; nrm2 is correct over the whole range."""
import math
import os
from fractions import Fraction

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EXPONENTS = (-440, -200, -40, 40, 200, 440)
MAT_EXPONENTS = (-200, -40, 40, 200)
# The value dictionary is only looked for from 2^20 entries on (csrc/solver.hip ensure_valdict), so the forms that read it
# cannot be reached within the 20000 rows the other systems keep to: they run on the smallest 5-point grid with that many
# entries (5 * 459^2 - 4 * 459 = 1051569 >= 1048576; 210681 rows, two distinct values), ten iterations.
DICT_GRID = "poisson459x459"
DRIFT = "soak21_41"


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


@pytest.fixture(autouse=True)
def _free_device_arrays(ctx):
    """whatever a test allocates through the shared context is freed when the test ends, passed or failed (after the finally
    blocks that close its solvers)"""
    held = []
    array, empty = ctx.array, ctx.empty
    ctx.array = lambda *a, **k: held.append(array(*a, **k)) or held[-1]
    ctx.empty = lambda *a, **k: held.append(empty(*a, **k)) or held[-1]
    yield
    del ctx.array, ctx.empty                   # the class's methods again
    for a in held:
        a.free()


@pytest.fixture(scope="module")
def systems(oracle, golden_dir):
    """name -> (A, b = A (1 + sin i)): built once, read-only"""
    out = {}
    for name in ("mat900", "mat10000", "rand20000x50", "poisson40x30", DICT_GRID):
        if name == "rand20000x50":
            A = oracle.rand_rows(20000, 50, 0x5EED)
        elif name.startswith("poisson"):
            A = oracle.poisson5(*[int(t) for t in name[7:].split("x")])
        else:
            A = oracle.mtx_load(os.path.join(golden_dir, name + ".mtx"))
        b = oracle.spmv(A, 1.0 + np.sin(np.arange(A.n)))
        b.setflags(write=False)
        out[name] = (A, b)
    # tests/soak.py's seed 21, case 41 (11 881 rows, Pareto row lengths, three hub rows): without residual replacement the
    # pipelined loop's recursive residual drifts here, which is what its verification restart is for
    from tests.test_gpu_parity import _soak_case
    A, _, b = _soak_case(oracle, 21, 41)
    b.setflags(write=False)
    out[DRIFT] = (A, b)
    return out


def _shift(n):
    return 0.5 + np.random.default_rng(5).random(n)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _summary(st):
    return (st.iters, bool(st.half_exit), bool(st.converged), bool(st.breakdown), st.loop_form, st.restarts)


def _solve(ctx, s, b, x0, **kw):
    db, dx = ctx.array(b), ctx.array(x0)
    try:
        st = s.solve(db, dx, **kw)
        return dx.download(), st, s.history()
    finally:
        db.free()
        dx.free()


def _solver(cm, ctx, A, d=None):
    s = cm.Solver.from_host_csr(ctx, A.rowptr, A.colidx, A.val)
    if d is not None:
        s.set_shift(ctx.array(d))
    return s


def _scaled_matrix(oracle, A, c):
    return oracle.Csr(A.n, A.rowptr, A.colidx, A.val * c, A.m)


# ------------------------------------------------------------------------------------------------ the configurations
# name -> (system, switches, solve arguments, check(stats, solver)); each on the smallest system that reaches the form in the
# existing tests; maxit = 10 where convergence is slow
def _configs(cm):
    five = {"RESIDENT": 0, "FUSED": 0, "SPMV_MODE": "csr"}
    ilu = dict(precond=cm.PRECOND_ILU0, loop=cm.LOOP_PBICGSTAB)
    pipe = dict(loop=cm.LOOP_PIPELINED)
    return {
        "five_launch": ("mat900", five, dict(loop=cm.LOOP_PBICGSTAB), lambda st, s: st.loop_form == 0),
        "fused": ("mat900", {"RESIDENT": 0, "FUSED": 1000000, "SPMV_MODE": "csr"}, dict(loop=cm.LOOP_PBICGSTAB),
                  lambda st, s: st.loop_form == 1),
        "single_launch": ("mat900", {"RESIDENT": 1}, dict(loop=cm.LOOP_PBICGSTAB),
                          lambda st, s: st.loop_form == 2 and st.loop_fallbacks == 0),
        "pbicgstab2_d": ("mat900", five, dict(loop=cm.LOOP_PBICGSTAB2), lambda st, s: st.loop_form == 0),
        "pbicgstab2_d_single": ("mat900", {"RESIDENT": 1}, dict(loop=cm.LOOP_PBICGSTAB2), lambda st, s: st.loop_form == 2),
        "pipelined": ("mat900", {}, pipe, lambda st, s: st.loop_form == 0),
        "pipelined_ilu0": ("mat900", {}, dict(pipe, precond=cm.PRECOND_ILU0), lambda st, s: st.loop_form == 0),
        "pipelined_rr4": ("mat900", {"PIPE_RR": 4}, pipe, lambda st, s: st.iters > 4),      # a replacement within the solve
        # the verification restart: the scaled runs must restart as often as the unscaled one (_summary holds st.restarts).
        # Whether this device's rounding drifts far enough to restart at all is not guaranteed (test_gpu_parity.py:
        # test_pipelined_loop_verifies_its_iterate); the verification itself (one solve from the iterate) always runs
        "pipelined_rr0_drift": (DRIFT, {"PIPE_RR": 0}, dict(pipe, maxit=1000, tol=1e-9), lambda st, s: st.converged),
        "ilu0_lds": ("mat900", {"TRSV_LDS": 1, "TRSV_SYNCFREE": 0}, ilu, lambda st, s: st.trsv_form == 2),     # (2: one workgroup, in LDS)
        "ilu0_level": ("mat10000", {"TRSV_LDS": 0, "TRSV_SYNCFREE": 0}, dict(ilu, maxit=10), lambda st, s: st.trsv_form == 0),
        "ilu0_syncfree": ("mat10000", {"TRSV_LDS": 0, "TRSV_SYNCFREE": 1}, dict(ilu, maxit=10),
                          lambda st, s: st.trsv_form == 1 and st.trsv_fallbacks == 0),
        "ilu0_level_mat900": ("mat900", {"TRSV_LDS": 0, "TRSV_SYNCFREE": 0}, ilu, lambda st, s: st.trsv_form == 0),
        "ilu0_syncfree_mat900": ("mat900", {"TRSV_LDS": 0, "TRSV_SYNCFREE": 1}, ilu, lambda st, s: st.trsv_form == 1),
        "ilu0_hybrid": ("rand20000x50", {"TRSV_HYBRID": 1}, dict(ilu, maxit=10),
                        lambda st, s: st.trsv_groups_l > 0 and st.trsv_groups_u > 0),        # both factors were split
        "spmv_csr": ("mat10000", five, dict(loop=cm.LOOP_PBICGSTAB, maxit=10),
                     lambda st, s: s.spmv_mode() == 0 and s.spmv_kernel().startswith("k_spmv")),
        "spmv_pb": ("mat10000", dict(five, SPMV_MODE="pb"), dict(loop=cm.LOOP_PBICGSTAB, maxit=10),
                    lambda st, s: s.spmv_mode() == 1 and s.spmv_kernel().startswith("k_pb_phase1")),
        "spmv_sell": ("mat10000", dict(five, SPMV_MODE="sell"), dict(loop=cm.LOOP_PBICGSTAB, maxit=10),
                      lambda st, s: s.spmv_mode() == 2 and s.spmv_kernel() == "k_spmv_sell"),
        # the 5-point stencil holds two distinct values: with and without the value dictionary
        "spmv_pat_dict": (DICT_GRID, dict(five, SPMV_MODE="pat", VALUE_DICT=1), dict(loop=cm.LOOP_PBICGSTAB, maxit=10),
                          lambda st, s: s.spmv_mode() == 3 and s.value_dict() == 2 and s.spmv_kernel().startswith("k_spmv_pat_d<")),
        "spmv_pat": ("poisson40x30", dict(five, SPMV_MODE="pat", VALUE_DICT=0), dict(loop=cm.LOOP_PBICGSTAB, maxit=10),
                     lambda st, s: s.spmv_mode() == 3 and s.value_dict() == 0 and s.spmv_kernel().startswith("k_spmv_pat<")),
        "spmv_pb_dict": (DICT_GRID, dict(five, SPMV_MODE="pb", VALUE_DICT=1), dict(loop=cm.LOOP_PBICGSTAB, maxit=10),
                         lambda st, s: s.spmv_mode() == 1 and s.value_dict() == 2),
        "spmv_pb_nodict": (DICT_GRID, dict(five, SPMV_MODE="pb", VALUE_DICT=0), dict(loop=cm.LOOP_PBICGSTAB, maxit=10),
                           lambda st, s: s.spmv_mode() == 1 and s.value_dict() == 0),
    }


class _NoModule:                # the names and systems of the configurations, for parametrize (no GPU needed to list them)
    PRECOND_ILU0 = LOOP_PBICGSTAB = LOOP_PBICGSTAB2 = LOOP_PIPELINED = None


CONFIG_NAMES = list(_configs(_NoModule))
# the loop forms of the out-of-range tests: those that run on mat900
MAT900_FORMS = [k for k, v in _configs(_NoModule).items() if v[0] == "mat900"]


def _open(cm, ctx, systems, sw, config):
    """the configuration's switches set, its solver created: (solver, A, b, solve arguments, check)"""
    name, switches, kw, check = _configs(cm)[config]
    for k, v in switches.items():
        sw(k, v)
    A, b = systems[name]
    d = _shift(A.n) if config.startswith("pbicgstab2_d") else None
    if d is not None:
        b = b + d * (1.0 + np.sin(np.arange(A.n)))
    kw = dict(dict(maxit=2000, tol=1e-8), **kw)
    return _solver(cm, ctx, A, d), A, b, kw, check, d


# ------------------------------------------------------------------------------------- 2. bitwise equivariance in range
@pytest.mark.parametrize("config", CONFIG_NAMES)
def test_rhs_scaling_is_bitwise(cm, ctx, systems, sw, config):
    """one Solver (one plan, one SpMV form, one set of timing-based choices): (c b, c x0) gives c x, c times the history and
    c ||r0||, with the same iterations, exit and loop form"""
    s, A, b, kw, check, _ = _open(cm, ctx, systems, sw, config)
    try:
        x0 = np.ones(A.n)
        x, st, h = _solve(ctx, s, b, x0, **kw)
        assert check(st, s), (config, _summary(st), st.trsv_form, s.spmv_kernel())
        assert st.iters > 0 and not st.breakdown and (st.converged or kw["maxit"] == 10)
        assert len(h) > 0 and np.isfinite(h).all() and np.isfinite(x).all()
        for k in EXPONENTS:
            c = 2.0 ** k
            xc, stc, hc = _solve(ctx, s, c * b, c * x0, **kw)
            assert _summary(stc) == _summary(st), (config, k)
            assert stc.nrm0 == c * st.nrm0, (config, k)
            np.testing.assert_array_equal(_bits(hc), _bits(c * h), err_msg="history, %s, k = %d" % (config, k))
            np.testing.assert_array_equal(_bits(xc), _bits(c * x), err_msg="x, %s, k = %d" % (config, k))
    finally:
        s.close()


def _many(ctx, s, B, X0, D=None, **kw):
    """solve_many / solve_shifts on (n, k) host arrays: (X, stats, histories, form)"""
    n, k = B.shape
    dB, dX = ctx.array(B.T.ravel()), ctx.array(X0.T.ravel())
    dD = ctx.array(D.T.ravel()) if D is not None else None
    try:
        if D is None:
            sts, form = s.solve_many(k, dB, n, dX, n, **kw)
        else:
            sts, form = s.solve_shifts(k, dD, n, dB, n, dX, n, **kw)
        X = dX.download().reshape(k, n).T.copy()
        return X, sts, [s.history(col=j) for j in range(k)], form
    finally:
        for a in (dB, dX, dD):
            if a is not None:
                a.free()


def _columns(oracle, A, k, D=None):
    """k different right-hand sides b_j = (A + diag D_j) (1 + sin(i (1 + 0.37 j)))"""
    i = np.arange(A.n)
    XS = np.stack([1.0 + np.sin(i * (1.0 + 0.37 * j)) for j in range(k)], axis=1)
    B = np.stack([oracle.spmv(A, XS[:, j]) for j in range(k)], axis=1)
    return B if D is None else B + D * XS


# 13 columns = a full group of 8 holding all six exponents, then a group of K = 8 with kc = 5 live columns and 3 padding ones
BATCH_EXPONENTS = np.array([-440, -200, -40, 40, 200, 440, 0, 40, 440, -440, 200, -200, -40])


@pytest.mark.parametrize("kind", ["plain", "ilu0_batched", "shifts"])
def test_batched_columns_scale_independently(cm, ctx, oracle, systems, sw, kind):
    """every column of a batch scaled by its own 2^k_j (shifts unchanged): column j is bitwise 2^k_j times column j of the
    unscaled batch, history and ||r0|| included, with the same iterations and exit"""
    sw("MANY_FORM", "batched")
    kw = dict(loop=cm.LOOP_PBICGSTAB, maxit=2000, tol=1e-8)
    if kind == "ilu0_batched":
        sw("MANY_PRECOND", "batched")
        kw["precond"] = cm.PRECOND_ILU0
    A = systems["mat900"][0]
    nrhs = len(BATCH_EXPONENTS)
    D = None
    if kind == "shifts":
        D = np.stack([_shift(A.n) * (1.0 + 0.25 * j) for j in range(nrhs)], axis=1)
        kw["loop"] = cm.LOOP_PBICGSTAB2
    B = _columns(oracle, A, nrhs, D)
    C = 2.0 ** BATCH_EXPONENTS
    s = _solver(cm, ctx, A)
    try:
        X0 = np.ones((A.n, nrhs))
        X, sts, hs, form = _many(ctx, s, B, X0, D, **kw)
        Xc, stc, hc, formc = _many(ctx, s, B * C, X0 * C, D, **kw)
        assert form == 1 and formc == 1
        for j in range(nrhs):
            assert sts[j].converged and sts[j].iters > 0
            assert _summary(stc[j]) == _summary(sts[j]), j
            assert stc[j].nrm0 == C[j] * sts[j].nrm0, j
            np.testing.assert_array_equal(_bits(hc[j]), _bits(C[j] * hs[j]), err_msg="history of column %d" % j)
            np.testing.assert_array_equal(_bits(Xc[:, j]), _bits(C[j] * X[:, j]), err_msg="column %d" % j)
    finally:
        s.close()


MATRIX_CONFIGS = ["five_launch", "fused", "pbicgstab2_d", "pipelined", "pipelined_ilu0", "ilu0_lds", "ilu0_level_mat900",
                  "ilu0_syncfree_mat900"]


@pytest.mark.parametrize("config", MATRIX_CONFIGS)
def test_matrix_scaling_is_bitwise(cm, ctx, oracle, systems, sw, config):
    """(2^k A, 2^k d, b, 2^-k x0): x is 2^-k times the unscaled x and the history is the same, bit for bit.  Two solvers, so the
    plan is pinned (SPMV_MODE, SPMV_LANES, TRSV_LANES, TRSV_LDS come with the configuration or from here)."""
    sw("SPMV_MODE", "csr")
    sw("SPMV_LANES", 4)
    sw("TRSV_LANES", 4)
    sw("TRSV_LDS", 0)
    s, A, b, kw, check, d = _open(cm, ctx, systems, sw, config)
    try:
        x0 = np.ones(A.n)
        x, st, h = _solve(ctx, s, b, x0, **kw)
        assert check(st, s) and st.converged, (config, _summary(st))
    finally:
        s.close()
    # gpu_pbicgstab2's guard |omega| < 1e-5 is the reference's (pbicgstab.cu:735) and absolute in omega, which scales with
    # 1 / A: that loop's matrix scaling keeps to k = +-10, where omega (0.1 to 1 here) stays far above the guard
    for k in ((-10, 10) if config.startswith("pbicgstab2") else MAT_EXPONENTS):
        c = 2.0 ** k
        sc = _solver(cm, ctx, _scaled_matrix(oracle, A, c), None if d is None else c * d)
        try:
            xc, stc, hc = _solve(ctx, sc, b, x0 / c, **kw)
            assert _summary(stc) == _summary(st) and stc.nrm0 == st.nrm0, (config, k)
            np.testing.assert_array_equal(_bits(hc), _bits(h), err_msg="history, %s, k = %d" % (config, k))
            np.testing.assert_array_equal(_bits(xc), _bits(x / c), err_msg="x, %s, k = %d" % (config, k))
        finally:
            sc.close()


@pytest.mark.parametrize("name", ["mat900", "mat10000", "rand20000x50"])
def test_ilu0_factors_scale_with_the_matrix(cm, ctx, oracle, systems, name):
    """ILU(0) of 2^k A: the entries of L keep their bits, those of U are 2^k times U's"""
    A = systems[name][0]
    s = _solver(cm, ctx, A)
    s.ilu0()
    vm = s.ilu0_values()
    s.close()
    rows = np.repeat(np.arange(A.n), np.diff(A.rowptr))
    lower = (A.colidx - int(A.rowptr[0])) < rows
    assert len(vm) == A.nnz
    for k in MAT_EXPONENTS:
        c = 2.0 ** k
        sc = _solver(cm, ctx, _scaled_matrix(oracle, A, c))
        sc.ilu0()
        vmc = sc.ilu0_values()
        sc.close()
        np.testing.assert_array_equal(_bits(vmc[lower]), _bits(vm[lower]))
        np.testing.assert_array_equal(_bits(vmc[~lower]), _bits(c * vm[~lower]))


def _empty_rows_matrix(oracle):
    """three bands, n = 10007 (no multiple of anything), five empty rows, base 1"""
    import scipy.sparse as sp
    rng = np.random.default_rng(12)
    n = 10007
    S = sp.diags([rng.standard_normal(n - 7), rng.standard_normal(n), rng.standard_normal(n - 3)], [-7, 0, 3]).tolil()
    for r in (0, 5, 64, 4099, n - 1):
        S[r, :] = 0
    S = S.tocsr()
    S.eliminate_zeros()
    S.sort_indices()
    return oracle.Csr(n, (S.indptr + 1).astype(np.int32), (S.indices + 1).astype(np.int32), S.data.astype(np.float64), n)


def _long_rows_matrix(oracle):
    from tests import test_gpu_long_rows as LR          # rows of 4097 to 6000 entries among rows of 6
    return LR._matrix(oracle, "few", diag_dominant=True)


@pytest.mark.parametrize("case", ["long_rows_csr", "empty_csr", "empty_pb", "empty_sell", "empty_pat", "mat10000_csr",
                                  "poisson_pat_dict", "poisson_pb_dict"])
def test_spmv_and_spmm_are_bitwise_equivariant(cm, ctx, oracle, systems, sw, case):
    """y(c x) == c y(x) bitwise for each SpMV form, and column by column with per-column scales for the SpMM, with and
    without a shift: long rows (> 4096 entries, swept by the whole workgroup), empty rows, the value dictionary"""
    mode = case.rsplit("_", 1)[1] if not case.endswith("_dict") else case.split("_")[1]
    sw("SPMV_MODE", mode)
    if case.endswith("_dict"):
        sw("VALUE_DICT", 1)
    if case == "long_rows_csr":
        A = _long_rows_matrix(oracle)
    elif case.startswith("empty"):
        A = _empty_rows_matrix(oracle)
    elif case.startswith("poisson"):
        A = systems[DICT_GRID][0]
    else:
        A = systems["mat10000"][0]
    n = A.n
    rng = np.random.default_rng(2)
    x = rng.standard_normal(n)
    for d in (None, _shift(n)):
        s = cm.Solver.from_host_csr(ctx, A.rowptr, A.colidx, A.val, n_cols=A.m)
        try:
            if d is not None:
                s.set_shift(ctx.array(d))
            assert s.spmv_mode() == {"csr": 0, "pb": 1, "sell": 2, "pat": 3}[mode]
            if case.endswith("_dict"):
                assert s.value_dict() == 2
            dx, dy = ctx.array(x), ctx.array(np.full(n, np.nan))
            s.spmv(dx, dy)
            y = dy.download()
            assert np.isfinite(y).all() and np.any(y != 0.0)
            if case.startswith("empty") and d is None:
                assert np.all(y[[0, 5, 64, 4099, n - 1]] == 0.0)
            for k in EXPONENTS:
                c = 2.0 ** k
                dx.upload(c * x)
                dy.upload(np.full(n, np.nan))
                s.spmv(dx, dy)
                np.testing.assert_array_equal(_bits(dy.download()), _bits(c * y), err_msg="%s, k = %d" % (case, k))
            # SpMM: 13 columns (8 + a padded group of 5), each with its own scale
            nrhs = len(BATCH_EXPONENTS)
            C = 2.0 ** BATCH_EXPONENTS
            X = rng.standard_normal((n, nrhs))
            dX, dY = ctx.array(X.T.ravel()), ctx.array(np.full(n * nrhs, np.nan))
            s.spmm(nrhs, dX, n, dY, n)
            Y = dY.download().reshape(nrhs, n).T.copy()
            dX.upload((X * C).T.ravel())
            dY.upload(np.full(n * nrhs, np.nan))
            s.spmm(nrhs, dX, n, dY, n)
            Yc = dY.download().reshape(nrhs, n).T
            assert np.isfinite(Y).all()
            np.testing.assert_array_equal(_bits(Yc), _bits(Y * C), err_msg=case)
            for a in (dx, dy, dX, dY):
                a.free()
        finally:
            s.close()


@pytest.mark.parametrize("case", ["mat900_lds", "mat10000_level", "mat10000_syncfree", "rand20000x50_hybrid", "long_rows"])
def test_precond_apply_is_bitwise_equivariant(cm, ctx, oracle, systems, sw, case):
    """U^-1 L^-1 (c v) == c U^-1 L^-1 v bitwise, through precond_apply and, with per-column scales, precond_apply_many"""
    if case == "long_rows":
        A = _long_rows_matrix(oracle)
    else:
        A = systems[case.split("_")[0]][0]
        form = case.split("_")[1]
        if form == "hybrid":
            sw("TRSV_HYBRID", 1)
        else:
            sw("TRSV_LDS", 1 if form == "lds" else 0)
            sw("TRSV_SYNCFREE", 1 if form == "syncfree" else 0)
    n = A.n
    rng = np.random.default_rng(6)
    v = rng.standard_normal(n)
    s = _solver(cm, ctx, A)
    try:
        s.ilu0()
        if case.endswith("syncfree"):
            assert s.trsv_form() == 1
        dv, do = ctx.array(v), ctx.array(np.full(n, np.nan))
        s.precond_apply(dv, do)
        y = do.download()
        assert np.isfinite(y).all()
        for k in EXPONENTS:
            c = 2.0 ** k
            dv.upload(c * v)
            do.upload(np.full(n, np.nan))
            s.precond_apply(dv, do)
            np.testing.assert_array_equal(_bits(do.download()), _bits(c * y), err_msg="%s, k = %d" % (case, k))
        nrhs = len(BATCH_EXPONENTS)
        C = 2.0 ** BATCH_EXPONENTS
        V = rng.standard_normal((n, nrhs))
        dV, dO = ctx.array(V.T.ravel()), ctx.array(np.full(n * nrhs, np.nan))
        s.precond_apply_many(nrhs, dV, n, dO, n)
        Y = dO.download().reshape(nrhs, n).T.copy()
        dV.upload((V * C).T.ravel())
        dO.upload(np.full(n * nrhs, np.nan))
        s.precond_apply_many(nrhs, dV, n, dO, n)
        Yc = dO.download().reshape(nrhs, n).T
        assert np.isfinite(Y).all()
        np.testing.assert_array_equal(_bits(Yc), _bits(Y * C), err_msg=case)
        # which triangular solve these factors take, as one iteration's statistics report it (0 one launch per level, 1
        # dependency-driven, 2 one workgroup in LDS; hybrid: the groups of levels both factors were split into)
        st = s.solve(ctx.array(v), ctx.array(np.ones(n)), precond=cm.PRECOND_ILU0, loop=cm.LOOP_PBICGSTAB, maxit=1, tol=1e-8)
        print(case, st.trsv_form, st.trsv_groups_l, st.trsv_groups_u)
        if case != "long_rows":
            if form == "hybrid":
                assert st.trsv_groups_l > 0 and st.trsv_groups_u > 0
            else:
                assert st.trsv_form == {"level": 0, "syncfree": 1, "lds": 2}[form]
                assert st.trsv_groups_l == 0 and st.trsv_groups_u == 0
    finally:
        s.close()


# ------------------------------------------------------------------------------------ 3. range edges of dot and nrm2
def _exact_sum_of_products(x, y):
    """sum x_i y_i as a Fraction, exactly: integer mantissas (frexp) brought to a common exponent"""
    mx, ex = np.frexp(np.asarray(x, np.float64))
    my, ey = np.frexp(np.asarray(y, np.float64))
    ix = [int(t) for t in np.ldexp(mx, 53)]
    iy = [int(t) for t in np.ldexp(my, 53)]
    e = (ex.astype(np.int64) + ey.astype(np.int64) - 106).tolist()
    lo = min(e)
    total = sum((a * b) << (q - lo) for a, b, q in zip(ix, iy, e))
    return Fraction(total) * Fraction(2) ** lo


SIZES = [1, 3, 257, 100003]
TINY = 5e-324          # the smallest subnormal


def _check_dot(ctx, x, y):
    """1e-13 relative to the exact sum |x_i y_i|, as test_dot_nrm2_axpy_scal; the reference is exact"""
    n = len(x)
    dx, dy = ctx.array(x), ctx.array(y)
    got = ctx.dot(n, dx, dy)
    dx.free()
    dy.free()
    ref = _exact_sum_of_products(x, y)
    scale = _exact_sum_of_products(np.abs(x), np.abs(y))
    assert math.isfinite(got), got
    print("dot n=%d got=%r err/scale=%.3e" % (n, got, float(abs(Fraction(got) - ref) / scale)))
    assert abs(Fraction(got) - ref) <= Fraction(1e-13) * scale


@pytest.mark.parametrize("n", SIZES)
def test_dot_at_the_range_edges(ctx, n):
    rng = np.random.default_rng(n)
    u, w = rng.standard_normal(n), rng.standard_normal(n)
    # operands of magnitude 2^+-500 whose products are in range
    _check_dot(ctx, np.ldexp(u, 500), np.ldexp(w, -500))
    _check_dot(ctx, np.ldexp(u, -500), np.ldexp(w, 500))
    _check_dot(ctx, np.ldexp(u, 500), np.ldexp(w, 500))           # products ~2^1000
    _check_dot(ctx, np.ldexp(u, -500), np.ldexp(w, -500))         # products ~2^-1000: normal
    # subnormal operands are not flushed: 5e-324 and its neighbours against 2^1000 (products ~2^-74, exact)
    sub = TINY * rng.integers(1, 8, n).astype(np.float64)
    assert np.all(sub > 0.0) and np.all(sub < 2.3e-308)
    _check_dot(ctx, sub, np.ldexp(1.0 + rng.random(n), 1000))
    # products that overflow give +-inf or NaN, never a finite number
    big = np.ldexp(1.0 + rng.random(n), 600)
    for x, y in ((big, big), (big, -big), (np.ldexp(u, 600), np.ldexp(w, 600))):
        dx, dy = ctx.array(x), ctx.array(y)
        got = ctx.dot(n, dx, dy)
        assert not math.isfinite(got), got
        dx.free()
        dy.free()
    got = ctx.dot(n, ctx.array(big), ctx.array(big))
    assert got == math.inf
    # a NaN or inf operand propagates
    for bad in (np.nan, np.inf, -np.inf):
        x = u.copy()
        x[n // 2] = bad
        got = ctx.dot(n, ctx.array(x), ctx.array(1.0 + np.abs(w)))
        assert not math.isfinite(got), (bad, got)
        if math.isnan(bad):
            assert math.isnan(got)
        elif n == 1:
            assert got == bad


def _check_nrm2(ctx, x):
    """within 1e-13 relative of the exact norm.  The reference is the exact sum of squares S (a Fraction); the comparison is
    made on squares, lo^2 <= S <= hi^2, so no square root of S is needed.  A norm in the subnormal range cannot be closer
    than half the spacing of subnormals, 2^-1075, whatever computes it: that much is allowed on top."""
    n = len(x)
    dx = ctx.array(x)
    got = ctx.nrm2(n, dx)
    dx.free()
    S = _exact_sum_of_products(x, x)
    print("nrm2 n=%d got=%r exact~%r" % (n, got, math.sqrt(S) if S < Fraction(2) ** 1023 else None))
    assert math.isfinite(got) and got >= 0.0, got
    g = Fraction(got)
    slack = Fraction(1e-13) * g + Fraction(2) ** -1075
    lo, hi = max(g - slack, Fraction(0)), g + slack
    assert lo * lo <= S <= hi * hi, (got, float(S) if S < Fraction(2) ** 1023 else S)


@pytest.mark.parametrize("n", SIZES)
def test_nrm2_is_correct_over_the_whole_range(ctx, n):
    """like the cublasDnrm2 it stands for: entries whose squares overflow, underflow, or are subnormal"""
    rng = np.random.default_rng(100 + n)
    u = rng.standard_normal(n)
    _check_nrm2(ctx, np.ldexp(u, 600))                              # the plain sum is inf
    _check_nrm2(ctx, np.ldexp(u, -600))                             # the plain sum is 0
    _check_nrm2(ctx, TINY * rng.integers(1, 8, n).astype(np.float64))          # subnormal entries
    _check_nrm2(ctx, np.ldexp(u, -1040))                            # subnormals of many sizes (and some zeros)
    mix = np.ldexp(u, -600)
    mix[::max(1, n // 7)] = np.ldexp(1.0 + rng.random(len(mix[::max(1, n // 7)])), -540)   # a few 2^-540 among 2^-600
    _check_nrm2(ctx, mix)
    _check_nrm2(ctx, np.ldexp(u, -520))                             # squares ~2^-1040: subnormal, the plain sum loses bits
    _check_nrm2(ctx, np.ldexp(u, -480))                             # the plain sum just in range
    wide = np.ldexp(u, rng.integers(-900, 900, n))                  # every magnitude at once
    _check_nrm2(ctx, wide)
    # in range nothing changes: the bits of sqrt(plain sum), reproducibly
    dx = ctx.array(u)
    a, b = ctx.nrm2(n, dx), ctx.nrm2(n, dx)
    assert a == b and abs(a - math.sqrt(math.fsum(u * u))) <= 1e-13 * a
    dx.upload(np.ldexp(u, 200))
    assert ctx.nrm2(n, dx) == math.ldexp(a, 200)
    dx.free()
    # what cannot be held propagates
    if n == 1:
        _check_nrm2(ctx, np.array([1.5e308]))
    else:
        assert ctx.nrm2(n, ctx.array(np.full(n, 1.5e308))) == math.inf         # the true norm is beyond the range
    x = u.copy()
    x[n // 2] = np.nan
    assert math.isnan(ctx.nrm2(n, ctx.array(x)))
    x[n // 2] = -np.inf
    assert ctx.nrm2(n, ctx.array(x)) == math.inf
    assert ctx.nrm2(n, ctx.array(np.zeros(n))) == 0.0


# ---------------------------------------------------- 4. out of range: no success that has not been computed
@pytest.mark.parametrize("config", MAT900_FORMS)
def test_out_of_range_solves_are_refused(cm, ctx, systems, sw, config):
    """mat900, x0 = c, b c, tol 1e-8, maxit 2000.  k = +520: the sum of r0^2 overflows, ||r0|| = inf.  k = -600: every r0^2
    is 0 although r0 is not.  k = -520: the squares are subnormal and tol ||r0|| is far below 2^-485.  Each returns at once:
    no iteration, not converged, breakdown, x bitwise x0, an empty history."""
    s, A, b, kw, check, _ = _open(cm, ctx, systems, sw, config)
    try:
        x, st, h = _solve(ctx, s, b, np.ones(A.n), **kw)
        assert check(st, s) and st.converged                     # the form under test ran, and in range it solves
        for k in (520, -600, -520):
            c = 2.0 ** k
            x0 = np.full(A.n, c)
            xc, stc, hc = _solve(ctx, s, c * b, x0, **kw)
            print(config, k, _summary(stc), stc.nrm0, len(hc))
            assert (stc.iters, bool(stc.converged), bool(stc.breakdown)) == (0, False, True), (config, k, _summary(stc))
            np.testing.assert_array_equal(_bits(xc), _bits(x0))
            assert len(hc) == 0
            if k == 520:
                assert stc.nrm0 == math.inf
            elif k == -600:
                assert stc.nrm0 == 0.0
        # and the solver is none the worse for it
        x2, st2, h2 = _solve(ctx, s, b, np.ones(A.n), **kw)
        assert _summary(st2) == _summary(st)
        np.testing.assert_array_equal(_bits(x2), _bits(x))
    finally:
        s.close()


@pytest.mark.parametrize("precond", [0, 1])
def test_exact_initial_guess_returns_at_once_at_2_pow_minus_600(cm, ctx, oracle, precond):
    """the twin of test_exact_initial_guess_returns_at_once at c = 2^-600: r0 == 0 exactly (A (c 1) is bitwise c (A 1), and
    b = c (A 1)) is still 'x0 solves the system' -- converged at once -- and not the underflow of a non-zero r0"""
    A = oracle.rand_rows(500, 10, 3)
    c = 2.0 ** -600
    b = c * oracle.spmv(A, np.ones(A.n))
    x0 = np.full(A.n, c)
    for loop in (cm.LOOP_PBICGSTAB, cm.LOOP_PBICGSTAB2):
        if precond and loop == cm.LOOP_PBICGSTAB2:
            continue
        s = _solver(cm, ctx, A)
        try:
            x, st, h = _solve(ctx, s, b, x0, precond=precond, loop=loop, maxit=50, tol=1e-8)
        finally:
            s.close()
        assert st.converged and st.iters == 0 and not st.breakdown and st.nrm0 == 0.0
        np.testing.assert_array_equal(_bits(x), _bits(x0))


@pytest.mark.parametrize("kind", ["plain", "ilu0_batched", "shifts"])
def test_batched_out_of_range_columns_start_frozen(cm, ctx, oracle, systems, sw, kind):
    """one batch with an overflowing column (2^520), a totally underflowing one (2^-600), a partially underflowing one
    (2^-520) and in-range ones: the out-of-range columns are frozen from the start (breakdown, no iteration, x0 untouched,
    no history); the in-range columns are bitwise what they are alone"""
    sw("MANY_FORM", "batched")
    kw = dict(loop=cm.LOOP_PBICGSTAB, maxit=2000, tol=1e-8)
    if kind == "ilu0_batched":
        sw("MANY_PRECOND", "batched")
        kw["precond"] = cm.PRECOND_ILU0
    A = systems["mat900"][0]
    exps = np.array([0, 520, 40, -600, -520])
    nrhs = len(exps)
    D = None
    if kind == "shifts":
        D = np.stack([_shift(A.n) * (1.0 + 0.25 * j) for j in range(nrhs)], axis=1)
        kw["loop"] = cm.LOOP_PBICGSTAB2
    C = 2.0 ** exps
    B = _columns(oracle, A, nrhs, D) * C
    X0 = np.ones((A.n, nrhs)) * C
    s = _solver(cm, ctx, A)
    try:
        X, sts, hs, form = _many(ctx, s, B, X0, D, **kw)
        assert form == 1
        for j in (1, 3, 4):
            print(kind, j, _summary(sts[j]), sts[j].nrm0, len(hs[j]))
            assert (sts[j].iters, bool(sts[j].converged), bool(sts[j].breakdown)) == (0, False, True), (j, _summary(sts[j]))
            np.testing.assert_array_equal(_bits(X[:, j]), _bits(X0[:, j]))
            assert len(hs[j]) == 0
        assert sts[1].nrm0 == math.inf and sts[3].nrm0 == 0.0
        for j in (0, 2):
            Dj = None if D is None else D[:, j:j + 1]
            X1, st1, h1, f1 = _many(ctx, s, B[:, j:j + 1], X0[:, j:j + 1], Dj, **kw)
            assert f1 == 1 and sts[j].converged and sts[j].iters > 0
            assert _summary(sts[j]) == _summary(st1[0]) and sts[j].nrm0 == st1[0].nrm0
            np.testing.assert_array_equal(_bits(X[:, j]), _bits(X1[:, 0]))
            np.testing.assert_array_equal(_bits(hs[j]), _bits(h1[0]))
    finally:
        s.close()


def test_fixed_iteration_runs_are_not_refused(cm, ctx, systems, sw):
    """FLAG_NO_EXIT or tol == 0: no stopping test applies, so nothing is refused -- the run does its maxit iterations, single
    and batched, wherever ||r0|| lies"""
    A, b = systems["mat900"]
    s = _solver(cm, ctx, A)
    try:
        # (k = -600 is not here: ||r0|| == 0 reads as "nothing to do" with or without stopping tests, as it always has)
        for k in (520, -520):
            c = 2.0 ** k
            x0 = np.full(A.n, c)
            x, st, h = _solve(ctx, s, c * b, x0, loop=cm.LOOP_PBICGSTAB, maxit=5, tol=1e-8, flags=cm.FLAG_NO_EXIT)
            assert st.iters == 5 and not st.breakdown and not st.converged, (k, _summary(st))
            if k == -520:                  # (finite arithmetic all the way: the iterate moved)
                assert np.isfinite(x).all() and np.any(x != x0)
        c = 2.0 ** -520
        x, st, h = _solve(ctx, s, c * b, np.full(A.n, c), loop=cm.LOOP_PBICGSTAB, maxit=5, tol=0.0)
        assert st.iters == 5 and not st.breakdown and not st.converged
        sw("MANY_FORM", "batched")
        C = 2.0 ** np.array([0, 520, -520])
        B = np.stack([b] * 3, axis=1) * C
        X, sts, hs, form = _many(ctx, s, B, np.ones((A.n, 3)) * C, loop=cm.LOOP_PBICGSTAB, maxit=5, tol=1e-8,
                                 flags=cm.FLAG_NO_EXIT)
        assert form == 1 and [t.iters for t in sts] == [5, 5, 5] and not any(t.breakdown for t in sts)
    finally:
        s.close()

