"""CUDAMAT_LOOP_CG through every SpMV form and every triangular-solve form, and under the range contract (GPU).

Every iteration of this loop launches spmv_local(s, p, q, 1, p, ...): the fused dot p.q runs in the SpMV's epilogue with the
epilogue operand w equal to the SpMV's x, which no other loop does.  tests/test_gpu_cg.py reaches two forms only (the tuner's pick
and SPMV_MODE = csr).  Here:

  a. ONE iteration is exact in every form.  With integer A, b, x0 (and d): r0, p = r0, q = A p, rho = r0.r0 and gamma = p.q are
     integers below 2^53 whatever the order of summation, alpha = rho / gamma is one rounding and x1 = fma(alpha, r0, x0) is
     independent of any summation order: x after maxit = 1 is compared with that value bit for bit (rho, gamma as Python ints).  A
     form whose epilogue drops a row's term, reads w at the wrong index or counts a tile twice fails this exactly.
  b. ten iterations in every form against the numpy restatement (tests/cg_ref.py), by the rule of test_gpu_cg._check: ||r0|| to
     1e-12, the history to 1e-6 over the prefix on which the restatement agrees with itself, less 3 entries.
  c. ILU(0) in every triangular form (one workgroup in LDS, one launch per level, dependency-driven, hybrid): test_gpu_cg._check
     as it stands, the restatement with the oracle's ILU(0).
  d. scale equivariance, bitwise: test_gpu_scaling's test_rhs_scaling_is_bitwise and test_matrix_scaling_is_bitwise with LOOP_CG
     (CG has no absolute constant: every exponent of EXPONENTS and MAT_EXPONENTS).
  e. out of range: test_out_of_range_solves_are_refused, the exact initial guess at 2^-600 and the fixed-iteration runs, with LOOP_CG.

Every system has n <= 20 000 except the smallest grid that reaches the value dictionary (test_gpu_scaling.DICT_GRID, 210 681
rows), which runs one or ten iterations."""
import functools
import math
import os

import numpy as np
import pytest

from tests import bicgstab_l2_ref as R2
from tests import cg_ref as R
from tests import nondominant as ND
from tests.test_gpu_cg import TOL, _check, _self_prefix
from tests.test_gpu_scaling import DICT_GRID, EXPONENTS, MAT_EXPONENTS, _bits, _empty_rows_matrix, _scaled_matrix, _summary

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
    """a library switch for the rest of this test, on the shared context and in the environment"""
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


def _solve(ctx, s, b, x0, **kw):
    db, dx = ctx.array(b), ctx.array(x0)
    try:
        st = s.solve(db, dx, **kw)
        return dx.download(), st, s.history()
    finally:
        db.free()
        dx.free()


def _solver(cm, ctx, A, d=None):
    s = cm.Solver.from_host_csr(ctx, A.rowptr, A.colidx, A.val, n_cols=A.n)
    if d is not None:
        dd = ctx.array(d)
        s.set_shift(dd)
        s._test_shift = dd          # (held until the solver goes)
    return s


def _close(s):
    dd = getattr(s, "_test_shift", None)
    s.close()
    if dd is not None:
        dd.free()


# ------------------------------------------------------------------------------------------------ matrices
def _from_scipy(O, S, base=0):
    S = S.tocsr()
    S.sort_indices()
    n = S.shape[0]
    return O.Csr(n, (S.indptr + base).astype(np.int32), (S.indices + base).astype(np.int32), S.data.astype(np.float64).copy(), n)


def _symmetric_integers(O, P, seed, amp=3):
    """the symmetric pattern of P (P + P^T, the diagonal added) with integer values: every pair (i, j), (j, i) one draw from
    -amp .. amp without 0, the diagonal the row's absolute sum + 1"""
    import scipy.sparse as sp
    P = sp.csr_matrix(P)
    U = sp.triu(abs(P) + abs(P.T), k=1).tocoo()
    rng = np.random.default_rng(seed)
    v = rng.integers(1, amp + 1, U.nnz) * rng.choice([-1, 1], U.nnz)
    U = sp.coo_matrix((v.astype(np.float64), (U.row, U.col)), shape=P.shape).tocsr()
    S = U + U.T
    S = S + sp.diags(np.asarray(abs(S).sum(axis=1)).ravel() + 1.0)
    return _from_scipy(O, S)


def _integers_substituted(O, A, seed, amp=3):
    """A's structure (base and empty rows included) with integer values: off the diagonal a draw from -amp .. amp without 0, a
    stored diagonal entry the row's absolute sum + 1"""
    rng = np.random.default_rng(seed)
    rp = A.rowptr - A.base
    rows = np.repeat(np.arange(A.n), np.diff(rp))
    on_diag = (A.colidx - A.base) == rows
    val = (rng.integers(1, amp + 1, A.nnz) * rng.choice([-1, 1], A.nnz)).astype(np.float64)
    val[on_diag] = 0.0
    sums = np.zeros(A.n)
    np.add.at(sums, rows, np.abs(val))
    val[on_diag] = sums[rows[on_diag]] + 1.0
    return O.Csr(A.n, A.rowptr.copy(), A.colidx.copy(), val, A.n)


def _tridiagonal(O, n, seed):
    import scipy.sparse as sp
    return _symmetric_integers(O, sp.diags([np.ones(max(n - 1, 0))], [1], shape=(n, n)) if n > 1 else sp.csr_matrix((1, 1)), seed)


@functools.lru_cache(maxsize=None)
def _integer_matrix(O, name):
    """(A, symmetric)"""
    if name == "rand":                          # 3001 rows (odd, 12 workgroups of k_spmv<64> and more), ~40 entries per row
        return _symmetric_integers(O, O.rand_rows(3001, 20, 11).to_scipy(), 1), True
    if name.startswith("stencil"):              # a 5-point pattern with its own value in every symmetric pair
        nx, ny = [int(t) for t in name[7:].split("x")]
        return _symmetric_integers(O, O.poisson5(nx, ny).to_scipy(), 2), True
    if name == DICT_GRID:                       # 4 and -1: the two values the dictionary holds
        return O.poisson5(*[int(t) for t in name[7:].split("x")]), True
    if name == "empty_rows":
        return _integers_substituted(O, _empty_rows_matrix(O), 3), False
    if name == "long_rows":                     # rows of 4097 to 6000 entries among rows of 6: entries +-1, x0 in -2 .. 2
        from tests import test_gpu_long_rows as LR
        return _integers_substituted(O, LR._matrix(O, "few", diag_dominant=True), 4, amp=1), False
    if name.startswith("tri"):
        return _tridiagonal(O, int(name[3:]), 5), True
    raise KeyError(name)


# name -> (matrix, switches, what the solver must report, integer shift?)
EXACT_CASES = {
    "lanes2": ("rand", {"SPMV_MODE": "csr", "SPMV_LANES": 2}, lambda s: s.spmv_kernel() == "k_spmv<2>", False),
    "lanes16": ("rand", {"SPMV_MODE": "csr", "SPMV_LANES": 16}, lambda s: s.spmv_kernel() == "k_spmv<16>", False),
    "lanes64": ("rand", {"SPMV_MODE": "csr", "SPMV_LANES": 64}, lambda s: s.spmv_kernel() == "k_spmv<64>", False),
    "stream": ("stencil37x27", {"SPMV_MODE": "csr"}, lambda s: s.spmv_kernel().startswith("k_spmv_stream"), False),
    "tiles": ("rand", {"SPMV_MODE": "csr", "SPMV_FORM": "tiles"}, lambda s: s.spmv_kernel() == "k_spmv_tiles", False),
    "pb": ("rand", {"SPMV_MODE": "pb"}, lambda s: s.spmv_mode() == 1 and s.spmv_kernel().startswith("k_pb_phase1"), False),
    "sell": ("rand", {"SPMV_MODE": "sell"}, lambda s: s.spmv_mode() == 2 and s.spmv_kernel() == "k_spmv_sell", False),
    "pat": ("stencil40x30", {"SPMV_MODE": "pat", "VALUE_DICT": 0},
            lambda s: s.spmv_mode() == 3 and s.value_dict() == 0 and s.spmv_kernel().startswith("k_spmv_pat<"), False),
    "pat_dict": (DICT_GRID, {"SPMV_MODE": "pat", "VALUE_DICT": 1},
                 lambda s: s.spmv_mode() == 3 and s.value_dict() == 2 and s.spmv_kernel().startswith("k_spmv_pat_d<"), False),
    "pb_dict": (DICT_GRID, {"SPMV_MODE": "pb", "VALUE_DICT": 1}, lambda s: s.spmv_mode() == 1 and s.value_dict() == 2, False),
    "stream_dict": (DICT_GRID, {"SPMV_MODE": "csr", "VALUE_DICT": 1},
                    lambda s: s.value_dict() == 2 and s.spmv_kernel().startswith("k_spmv_stream_d<"), False),
    "empty_csr": ("empty_rows", {"SPMV_MODE": "csr"}, lambda s: s.spmv_mode() == 0, False),
    "empty_pb": ("empty_rows", {"SPMV_MODE": "pb"}, lambda s: s.spmv_mode() == 1, False),
    "empty_sell": ("empty_rows", {"SPMV_MODE": "sell"}, lambda s: s.spmv_mode() == 2, False),
    "empty_pat": ("empty_rows", {"SPMV_MODE": "pat"}, lambda s: s.spmv_mode() == 3, False),
    "long_rows": ("long_rows", {"SPMV_MODE": "csr", "SPMV_LANES": 4}, lambda s: s.spmv_kernel() == "k_spmv<4>", False),
    "n1": ("tri1", {"SPMV_MODE": "csr"}, lambda s: s.spmv_mode() == 0, False),
    "n2": ("tri2", {"SPMV_MODE": "csr"}, lambda s: s.spmv_mode() == 0, False),
    "n257": ("tri257", {"SPMV_MODE": "csr"}, lambda s: s.spmv_mode() == 0, False),
    "lanes16_shift": ("rand", {"SPMV_MODE": "csr", "SPMV_LANES": 16}, lambda s: s.spmv_kernel() == "k_spmv<16>", True),
    "stream_shift": ("stencil37x27", {"SPMV_MODE": "csr"}, lambda s: s.spmv_kernel().startswith("k_spmv_stream"), True),
}


def exact_inputs(O, case):
    """(A, symmetric, b, x0, d) of a one-iteration case: integers throughout"""
    name, _, _, shifted = EXACT_CASES[case]
    A, symmetric = _integer_matrix(O, name)
    rng = np.random.default_rng(sorted(EXACT_CASES).index(case))
    amp = 2 if name == "long_rows" else 8
    x0 = rng.integers(-amp, amp + 1, A.n).astype(np.float64)
    b = rng.integers(-8, 9, A.n).astype(np.float64)
    d = rng.integers(1, 5, A.n).astype(np.float64) if shifted else None
    return A, symmetric, b, x0, d


def exact_first_iterate(A, b, x0, d):
    """(x1, rho, gamma, sum |p_i q_i|): r0 = b - (A + d) x0, q = (A + d) r0 in int64 (exact: asserted), rho and gamma as Python
    ints, alpha = rho / gamma (one rounding), x1 = fma(alpha, r0, x0)"""
    from test_spmv_rounding import fma
    S = A.to_scipy().astype(np.int64)
    assert np.array_equal(S.data, A.val) and np.all(x0 == np.rint(x0)) and np.all(b == np.rint(b))
    xi, bi = x0.astype(np.int64), b.astype(np.int64)
    di = np.zeros(A.n, np.int64) if d is None else d.astype(np.int64)
    big = int(abs(S).sum(axis=1).max()) + int(di.max())
    r = bi - (S @ xi + di * xi)
    assert big * int(np.abs(xi).max()) < 2 ** 62 and big * int(np.abs(r).max()) < 2 ** 62        # int64 held every sum
    q = S @ r + di * r
    rl, ql = r.tolist(), q.tolist()
    rho = sum(v * v for v in rl)
    gamma = sum(v * w for v, w in zip(rl, ql))
    mag = sum(abs(v * w) for v, w in zip(rl, ql))
    alpha = rho / gamma
    return np.array([fma(alpha, v, w) for v, w in zip(rl, x0.tolist())]), rho, gamma, mag


# ------------------------------------------------------------------------------------- a. one iteration is exact
@pytest.mark.parametrize("case", list(EXACT_CASES))
def test_one_iteration_is_exact(cm, ctx, oracle, sw, case):
    """maxit = 1 with FLAG_NO_EXIT on integer data: x equals fma(rho / gamma, r0, x0) bit for bit, rho and gamma formed as Python
    ints, in the SpMV form the case names"""
    _, switches, reached, _ = EXACT_CASES[case]
    A, symmetric, b, x0, d = exact_inputs(oracle, case)
    want, rho, gamma, mag = exact_first_iterate(A, b, x0, d)
    print(case, "n", A.n, "rho", rho, "gamma", gamma, "sum |p q| / 2^53", mag / 2.0 ** 53)
    assert mag < 2 ** 53 and rho < 2 ** 53 and gamma > 0 and rho > 0          # conditions on the inputs
    for k, v in switches.items():
        sw(k, v)
    s = _solver(cm, ctx, A, d)
    try:
        assert reached(s), (case, s.spmv_mode(), s.spmv_kernel(), s.value_dict())
        if symmetric:
            assert s.symmetry() == (0, 0.0)
        flags = cm.FLAG_NO_EXIT | (0 if symmetric else cm.FLAG_ASSUME_SYMMETRIC)
        x, st, h = _solve(ctx, s, b, x0, loop=cm.LOOP_CG, maxit=1, tol=TOL, flags=flags)
    finally:
        _close(s)
    print(case, "entries of x that differ:", int(np.count_nonzero(x != want)), "of", A.n)
    assert (st.iters, st.loop_form, bool(st.breakdown), len(h)) == (1, 0, False, 1)
    assert st.nrm0 == math.sqrt(rho)                 # (rho is exact, the square root correctly rounded)
    np.testing.assert_array_equal(x, want)
    assert np.any(x != x0)


# ------------------------------------------------------------------------------------- systems of b .. e
@pytest.fixture(scope="module")
def systems(oracle, golden_dir):
    """name -> (A, b = A (1 + sin i)): built once, read-only"""
    out = {}
    for name in ("mat900", "mat10000", "poisson40x30", DICT_GRID, "sym20000"):
        if name == "sym20000":
            A = _hybrid_matrix(oracle)
        elif name.startswith("poisson"):
            A = oracle.poisson5(*[int(t) for t in name[7:].split("x")])
        else:
            A = oracle.mtx_load(os.path.join(golden_dir, name + ".mtx"))
        b = oracle.spmv(A, 1.0 + np.sin(np.arange(A.n)))
        b.setflags(write=False)
        out[name] = (A, b)
    return out


def _hybrid_matrix(O, n=20000, per_row=25, seed=0x5EED):
    """S = R + R^T of oracle.rand_rows(n, per_row, seed), the diagonal set to the row's absolute sum + 1, sorted columns:
    symmetric, strictly dominant, ~50 entries per row -- a matrix whose ILU(0) factors TRSV_HYBRID = 1 splits into groups"""
    import scipy.sparse as sp
    Rm = O.rand_rows(n, per_row, seed).to_scipy().tocsr()
    S = (Rm + Rm.T).tolil()
    S.setdiag(0.0)
    S = S.tocsr()
    S.eliminate_zeros()
    S = S + sp.diags(np.asarray(abs(S).sum(axis=1)).ravel() + 1.0)
    assert abs(S - S.T).max() == 0.0
    return _from_scipy(O, S)


def _cg_configs(cm):
    """name -> (system, switches, solve arguments, check(stats, solver)): the forms of (b) and (c)"""
    ilu = dict(precond=getattr(cm, "PRECOND_ILU0", None))
    csr = {"SPMV_MODE": "csr"}
    return {
        "mat900": ("mat900", csr, {}, lambda st, s: s.spmv_mode() == 0),
        "spmv_csr": ("mat10000", csr, dict(maxit=10), lambda st, s: s.spmv_mode() == 0 and s.spmv_kernel().startswith("k_spmv")),
        "spmv_pb": ("mat10000", {"SPMV_MODE": "pb"}, dict(maxit=10),
                    lambda st, s: s.spmv_mode() == 1 and s.spmv_kernel().startswith("k_pb_phase1")),
        "spmv_sell": ("mat10000", {"SPMV_MODE": "sell"}, dict(maxit=10),
                      lambda st, s: s.spmv_mode() == 2 and s.spmv_kernel() == "k_spmv_sell"),
        "spmv_pat": ("poisson40x30", {"SPMV_MODE": "pat", "VALUE_DICT": 0}, dict(maxit=10),
                     lambda st, s: s.spmv_mode() == 3 and s.value_dict() == 0 and s.spmv_kernel().startswith("k_spmv_pat<")),
        "spmv_pat_dict": (DICT_GRID, {"SPMV_MODE": "pat", "VALUE_DICT": 1}, dict(maxit=10),
                          lambda st, s: s.spmv_mode() == 3 and s.value_dict() == 2 and s.spmv_kernel().startswith("k_spmv_pat_d<")),
        "spmv_pb_dict": (DICT_GRID, {"SPMV_MODE": "pb", "VALUE_DICT": 1}, dict(maxit=10),
                         lambda st, s: s.spmv_mode() == 1 and s.value_dict() == 2),
        "ilu0_lds": ("mat900", dict(csr, TRSV_LDS=1, TRSV_SYNCFREE=0), ilu, lambda st, s: st.trsv_form == 2),
        "ilu0_level": ("mat10000", dict(csr, TRSV_LDS=0, TRSV_SYNCFREE=0), dict(ilu, maxit=10), lambda st, s: st.trsv_form == 0),
        "ilu0_syncfree": ("mat10000", dict(csr, TRSV_LDS=0, TRSV_SYNCFREE=1), dict(ilu, maxit=10),
                          lambda st, s: st.trsv_form == 1 and st.trsv_fallbacks == 0),
        "ilu0_hybrid": ("sym20000", dict(csr, TRSV_HYBRID=1), dict(ilu, maxit=10),
                        lambda st, s: st.trsv_groups_l > 0 and st.trsv_groups_u > 0),
        # mat900 in the other two triangular forms: the matrix-scaling test runs on mat900 throughout
        "ilu0_level_mat900": ("mat900", dict(csr, TRSV_LDS=0, TRSV_SYNCFREE=0), ilu, lambda st, s: st.trsv_form == 0),
        "ilu0_syncfree_mat900": ("mat900", dict(csr, TRSV_LDS=0, TRSV_SYNCFREE=1), ilu, lambda st, s: st.trsv_form == 1),
    }


CONFIG_NAMES = list(_cg_configs(None))
SPMV_CONFIGS = [k for k in CONFIG_NAMES if k.startswith("spmv_")]
RHS_CONFIGS = [k for k in CONFIG_NAMES if not k.endswith("_mat900")]
MATRIX_CONFIGS = ["mat900", "ilu0_lds", "ilu0_level_mat900", "ilu0_syncfree_mat900"]


def _open(cm, ctx, systems, sw, config):
    """the configuration's switches set, its solver created (and factored): (solver, A, b, solve arguments, check)"""
    name, switches, kw, check = _cg_configs(cm)[config]
    for k, v in switches.items():
        sw(k, v)
    A, b = systems[name]
    kw = dict(dict(loop=cm.LOOP_CG, maxit=2000, tol=TOL), **kw)
    s = _solver(cm, ctx, A)
    if kw.get("precond"):
        s.ilu0()
    return s, A, b, kw, check


# ------------------------------------------------------------------------------------- b. ten iterations in every form
def _check_ten(run, b, ref, st, hg, label):
    """the first two assertions of test_gpu_cg._check (the others are about a converged solve)"""
    assert abs(st.nrm0 - ref.nrm0) <= 1e-12 * ref.nrm0, (label, st.nrm0, ref.nrm0)
    assert len(hg) == st.iters == len(ref.hist) == 10 and not st.breakdown and st.loop_form == 0, (label, _summary(st))      # (none converges in ten)
    l_self, cap = _self_prefix(run, b, ref.hist)
    l_gpu = ND.prefix(hg[:cap], ref.hist[:cap], 1e-6)
    print("%s: history equal to 1e-6 over %d of 10 entries (restatement vs itself, b changed by up to 64 ulp: %d)" % (label, l_gpu, l_self))
    assert l_gpu >= min(l_self, len(ref.hist), len(hg), cap) - 3, (label, l_gpu, l_self)


@pytest.mark.parametrize("config", SPMV_CONFIGS)
def test_ten_iterations_in_every_spmv_form(cm, ctx, oracle, systems, sw, config):
    """x0 = 1, tol 1e-8, ten iterations: ||r0|| and the history against the restatement on the oracle's SpMV"""
    s, A, b, kw, check = _open(cm, ctx, systems, sw, config)
    try:
        x, st, h = _solve(ctx, s, b, np.ones(A.n), **kw)
        assert check(st, s), (config, s.spmv_mode(), s.spmv_kernel(), s.value_dict())
    finally:
        _close(s)
    mv, _ = R2.oracle_ops(oracle, A)
    run = lambda bb, maxit: R.cg(mv, bb, maxit=min(maxit, 10), tol=TOL)       # (ten entries are all that is compared)
    _check_ten(run, b, run(b, 10), st, h, config)


# ------------------------------------------------------------------------------------- c. ILU(0) forms
@pytest.mark.parametrize("config", ["ilu0_lds", "ilu0_level", "ilu0_syncfree", "ilu0_hybrid"])
def test_ilu0_in_every_triangular_form(cm, ctx, oracle, systems, sw, config):
    """solved to 1e-8 from x0 = 1: test_gpu_cg._check -- ||r0||, the history over the restatement's self-agreeing prefix less 3,
    convergence with a TRUE residual <= 2 tol ||r0||, iterations inside the restatement's spread -- with the oracle's ILU(0) and
    substitutions as M^-1, in the triangular form the configuration names.  CG permutes per application (the level-major loop is
    LOOP_PBICGSTAB's), so this is where it meets the hybrid factors."""
    s, A, b, kw, check = _open(cm, ctx, systems, sw, config)
    kw["maxit"] = 2000
    try:
        x, st, h = _solve(ctx, s, b, np.ones(A.n), **kw)
        assert check(st, s), (config, st.trsv_form, st.trsv_groups_l, st.trsv_groups_u, st.trsv_fallbacks)
    finally:
        _close(s)
    mv, minv = R2.oracle_ops(oracle, A, oracle.ilu0(A))
    run = lambda bb, maxit: R.cg(mv, bb, minv=minv, maxit=maxit, tol=TOL)
    _check(run, b, run(b, 2000), st, h, ND.true_res(oracle, A, b, x) / st.nrm0, config)


# ------------------------------------------------------------------------------------- d. scale equivariance, bitwise
@pytest.mark.parametrize("config", RHS_CONFIGS)
def test_rhs_scaling_is_bitwise(cm, ctx, systems, sw, config):
    """one Solver: (c b, c x0) gives c x, c times the history and c ||r0|| bit for bit, with the same iterations and exit"""
    s, A, b, kw, check = _open(cm, ctx, systems, sw, config)
    try:
        x0 = np.ones(A.n)
        x, st, h = _solve(ctx, s, b, x0, **kw)
        assert check(st, s), (config, _summary(st), st.trsv_form, s.spmv_kernel())
        assert st.iters > 0 and not st.breakdown and st.loop_form == 0 and (st.converged or kw["maxit"] == 10)
        assert len(h) == st.iters and np.isfinite(h).all() and np.isfinite(x).all()
        for k in EXPONENTS:
            c = 2.0 ** k
            xc, stc, hc = _solve(ctx, s, c * b, c * x0, **kw)
            assert _summary(stc) == _summary(st), (config, k)
            assert stc.nrm0 == c * st.nrm0, (config, k)
            np.testing.assert_array_equal(_bits(hc), _bits(c * h), err_msg="history, %s, k = %d" % (config, k))
            np.testing.assert_array_equal(_bits(xc), _bits(c * x), err_msg="x, %s, k = %d" % (config, k))
    finally:
        _close(s)


@pytest.mark.parametrize("config", MATRIX_CONFIGS)
def test_matrix_scaling_is_bitwise(cm, ctx, oracle, systems, sw, config):
    """(2^k A, b, 2^-k x0): x is 2^-k times the unscaled x and the history is the same, bit for bit.  Two solvers, so the plan is
    pinned (SPMV_MODE, SPMV_LANES, TRSV_LANES, TRSV_LDS come with the configuration or from here)."""
    sw("SPMV_LANES", 4)
    sw("TRSV_LANES", 4)
    sw("TRSV_LDS", 0)
    s, A, b, kw, check = _open(cm, ctx, systems, sw, config)
    try:
        x0 = np.ones(A.n)
        x, st, h = _solve(ctx, s, b, x0, **kw)
        assert check(st, s) and st.converged and s.spmv_kernel() == "k_spmv<4>", (config, _summary(st), s.spmv_kernel())
    finally:
        _close(s)
    for k in MAT_EXPONENTS:
        c = 2.0 ** k
        sc = _solver(cm, ctx, _scaled_matrix(oracle, A, c))
        try:
            if kw.get("precond"):
                sc.ilu0()
            xc, stc, hc = _solve(ctx, sc, b, x0 / c, **kw)
            assert _summary(stc) == _summary(st) and stc.nrm0 == st.nrm0, (config, k)
            np.testing.assert_array_equal(_bits(hc), _bits(h), err_msg="history, %s, k = %d" % (config, k))
            np.testing.assert_array_equal(_bits(xc), _bits(x / c), err_msg="x, %s, k = %d" % (config, k))
        finally:
            _close(sc)


# ------------------------------------------------------------------------------------- e. out of range
@pytest.mark.parametrize("config", ["mat900", "ilu0_lds"])
def test_out_of_range_solves_are_refused(cm, ctx, systems, sw, config):
    """mat900, x0 = c, b c, tol 1e-8, maxit 2000, plain and with ILU(0).  k = +520: ||r0|| = inf.  k = -600: every r0^2 is 0
    although r0 is not.  k = -520: tol ||r0|| is far below 2^-485.  Each returns at once: no iteration, not converged, breakdown,
    x bitwise x0, an empty history; the same solver then solves the in-range system to the bits it gave before."""
    s, A, b, kw, check = _open(cm, ctx, systems, sw, config)
    try:
        x, st, h = _solve(ctx, s, b, np.ones(A.n), **kw)
        assert check(st, s) and st.converged
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
        x2, st2, h2 = _solve(ctx, s, b, np.ones(A.n), **kw)
        assert _summary(st2) == _summary(st)
        np.testing.assert_array_equal(_bits(h2), _bits(h))
        np.testing.assert_array_equal(_bits(x2), _bits(x))
    finally:
        _close(s)


@pytest.mark.parametrize("precond", [0, 1])
def test_exact_initial_guess_returns_at_once_at_2_pow_minus_600(cm, ctx, oracle, precond):
    """the twin of test_gpu_scaling's test of that name: r0 == 0 exactly at c = 2^-600 is 'x0 solves the system' -- converged at
    once -- and not the underflow of a non-zero r0.  (The matrix is the one of that test and is not symmetric: CG is told to
    assume it is, and never iterates.)"""
    A = oracle.rand_rows(500, 10, 3)
    c = 2.0 ** -600
    b = c * oracle.spmv(A, np.ones(A.n))
    x0 = np.full(A.n, c)
    s = _solver(cm, ctx, A)
    try:
        if precond:
            s.ilu0()
        x, st, h = _solve(ctx, s, b, x0, precond=precond, loop=cm.LOOP_CG, maxit=50, tol=TOL, flags=cm.FLAG_ASSUME_SYMMETRIC)
    finally:
        _close(s)
    assert st.converged and st.iters == 0 and not st.breakdown and st.nrm0 == 0.0 and len(h) == 0
    np.testing.assert_array_equal(_bits(x), _bits(x0))


@pytest.mark.parametrize("precond", [0, 1])
def test_fixed_iteration_runs_are_not_refused(cm, ctx, systems, precond):
    """FLAG_NO_EXIT: no stopping test applies, so nothing is refused -- 5 iterations at 2^520 and at 2^-520"""
    A, b = systems["mat900"]
    s = _solver(cm, ctx, A)
    try:
        if precond:
            s.ilu0()
        for k in (520, -520):
            c = 2.0 ** k
            x0 = np.full(A.n, c)
            x, st, h = _solve(ctx, s, c * b, x0, precond=precond, loop=cm.LOOP_CG, maxit=5, tol=TOL, flags=cm.FLAG_NO_EXIT)
            assert st.iters == 5 and len(h) == 5 and not st.breakdown and not st.converged, (k, _summary(st))
            if k == -520:                  # (finite arithmetic all the way: the iterate moved)
                assert np.isfinite(x).all() and np.any(x != x0)
    finally:
        _close(s)
