"""CUDAMAT_LOOP_CG on the GPU against the numpy restatement of conjugate gradients (tests/cg_ref.py), and the symmetry query
it relies on (cudamat_solver_symmetry).

What two correct implementations of this loop can agree on, and what is asserted (the rules of tests/nondominant.py and
tests/test_gpu_bicgstab_l2.py, with the restatement in the oracle's place):
  - ||r0|| to 1e-12;
  - the history (one entry per iteration) to 1e-6 over the prefix on which the restatement agrees with ITSELF when b is changed
    by 1, 8 or 64 ulp either way, less 3 entries;
  - a converged solve has a TRUE residual ||b - A x|| <= 2 tol ||r0|| (x and r move together: the carried r is the true
    residual up to rounding), in a number of iterations inside the restatement's own spread (+-10 %, at least +-2);
  - bits where the library promises bits: two runs, 16-byte aligned and 8 bytes off, a column of solve_many and its single
    solve, the host-array entry points and the resident solves.
Every system has n <= 13 500."""
import os
import sys

import numpy as np
import pytest

from tests import bicgstab_l2_ref as R2
from tests import cg_ref as R
from tests import nondominant as ND

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))       # (tests/dist_sim.py, as tests/test_gpu_dist.py does)

pytestmark = pytest.mark.gpu

MAXIT, TOL = 2000, 1e-8
ERR_ARG = 2


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
    """set a library switch for the rest of this test, on the module's context and in the environment (for the contexts the
    host-array entry points create); afterwards the context is back to what the environment outside the test says"""
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


# ------------------------------------------------------------------ helpers
def _mat(O, golden_dir, name):
    return O.mtx_load(os.path.join(golden_dir, name + ".mtx"))


def _sin_rhs(O, A):
    return O.spmv(A, 1.0 + np.sin(np.arange(A.n)))


def _from_scipy(O, S):
    S = S.tocsr()
    S.sort_indices()
    return O.Csr(S.shape[0], S.indptr.astype(np.int32), S.indices.astype(np.int32), S.data.astype(np.float64).copy(), S.shape[0])


def _stencil(O, nx, ny):
    """5-point Laplacian on nx x ny points, row-major: symmetric positive definite"""
    import scipy.sparse as sp
    T = lambda m: sp.diags([-np.ones(m - 1), np.zeros(m), -np.ones(m - 1)], [-1, 0, 1])
    return _from_scipy(O, 4.0 * sp.identity(nx * ny) + sp.kron(sp.identity(ny), T(nx)) + sp.kron(T(ny), sp.identity(nx)))


def _system(O, golden_dir, name):
    A = _stencil(O, 37, 27) if name == "stencil37x27" else _mat(O, golden_dir, name)
    return A, _sin_rhs(O, A)


def _gpu(cm, ctx, A, b, x0=None, precond=0, d=None, ilu_shift=False, off=0, solver=None, **kw):
    """(x, stats, history) of Solver.solve with the new loop; b and x start `off` doubles past a 16-byte boundary"""
    s = solver or cm.Solver.from_host_csr(ctx, A.rowptr, A.colidx, A.val)
    x0 = np.ones(A.n) if x0 is None else x0
    db, dx = ctx.array(np.concatenate([np.zeros(off), b])), ctx.array(np.concatenate([np.zeros(off), x0]))
    dd = None
    try:
        if d is not None:
            dd = ctx.array(d)
            s.set_shift(dd)
        if precond and solver is None:
            s.ilu0(shift=dd if ilu_shift else None)
        kw.setdefault("loop", cm.LOOP_CG)
        kw.setdefault("maxit", MAXIT)
        kw.setdefault("tol", TOL)
        st = s.solve(db.ptr + 8 * off, dx.ptr + 8 * off, precond=cm.PRECOND_ILU0 if precond else cm.PRECOND_NONE, **kw)
        return dx.download()[off:], st, s.history()
    finally:
        for a in (db, dx, dd):
            if a is not None:
                a.free()
        if solver is None:
            s.close()


def _refused(cm, s, db, dx, x_before, *needles, **kw):
    """the solve is CUDAMAT_ERR_ARG, its message names `needles`, and x is untouched"""
    with pytest.raises(cm.CudamatError) as e:
        s.solve(db, dx, maxit=5, tol=TOL, **kw)
    assert e.value.code == ERR_ARG, str(e.value)
    for needle in needles:
        assert needle in str(e.value), str(e.value)
    np.testing.assert_array_equal(dx.download(), x_before)
    return str(e.value)


def _self_prefix(run, b, h0):
    """entries over which the restatement's history agrees with itself to 1e-6 when b is changed by ND.PERTURB ulp"""
    cap = ND.SELF_ITERS
    return min(ND.prefix(run(b * (1.0 + k * ND.EPS), cap).hist[:cap], h0[:cap], 1e-6) for k in ND.PERTURB), cap


def _iters_inside_spread(run, b, it_gpu, it_ref):
    if abs(it_gpu - it_ref) <= max(2, 0.1 * it_ref):
        return True, (it_ref, it_ref)
    counts = [it_ref] + [r.iters for r in (run(b * (1.0 + k * ND.EPS), MAXIT) for k in ND.PERTURB) if r.converged]
    lo, hi = min(counts), max(counts)
    return lo - max(2, 0.1 * lo, hi - lo) <= it_gpu <= hi + max(2, 0.1 * hi, hi - lo), (lo, hi)


def _check(run, b, ref, st, hg, true_rel, label):
    """nrm0, history parity, convergence with a true residual, iterations inside the restatement's spread"""
    assert abs(st.nrm0 - ref.nrm0) <= 1e-12 * ref.nrm0, (label, st.nrm0, ref.nrm0)
    assert len(hg) == st.iters, (label, len(hg), st.iters)
    l_self, cap = _self_prefix(run, b, ref.hist)
    l_gpu = ND.prefix(hg[:cap], ref.hist[:cap], 1e-6)
    print("%s: GPU iterations %d conv %d brk %d, restatement %d conv %d; history equal to 1e-6 over %d entries (restatement vs "
          "itself, b changed by up to 64 ulp: %d); true residual / ||r0|| = %.3e"
          % (label, st.iters, st.converged, st.breakdown, ref.iters, ref.converged, l_gpu, l_self, true_rel))
    assert l_gpu >= min(l_self, len(ref.hist), len(hg), cap) - 3, (label, l_gpu, l_self)
    assert ref.converged and st.converged and not st.breakdown and not st.half_exit and st.loop_form == 0, label
    assert st.nrm < TOL * st.nrm0
    assert true_rel <= 2.0 * TOL, (label, true_rel)
    ok, (lo, hi) = _iters_inside_spread(run, b, st.iters, ref.iters)
    assert ok, "%s: %d iterations, outside the restatement's own spread %d..%d" % (label, st.iters, lo, hi)


# ------------------------------------------------------------------ 1. the loop exists
@pytest.mark.parametrize("rhs", ["sin", "urand"])
def test_loop_8_solves_mat900(cm, ctx, oracle, golden_dir, rhs):
    """Solver.solve(loop=8) is CUDAMAT_OK (CUDAMAT_ERR_ARG "loop" before this loop existed), converges with a true residual
    within 2 tol ||r0||, and x is within 1e-5 of the solution the reference CPU program printed (tests/golden)"""
    O = oracle
    g = np.load(os.path.join(golden_dir, "bicg_mat900_%s.npz" % rhs))
    A = _mat(O, golden_dir, "mat900")
    b = g["b"]
    x, st, h = _gpu(cm, ctx, A, b, loop=8)
    tr = ND.true_res(O, A, b, x)
    err = np.linalg.norm(x - g["x"]) / np.linalg.norm(g["x"])
    print("mat900", rhs, "iterations", st.iters, "true residual / nrm0", tr / st.nrm0, "distance to the printed solution", err)
    assert st.converged and not st.breakdown and not st.half_exit and st.loop_form == 0
    assert tr <= 2.0 * TOL * st.nrm0
    assert err <= 1e-5
    assert len(h) == st.iters and h[-1] < TOL * st.nrm0 and np.all(h[:-1] >= TOL * st.nrm0)


# ------------------------------------------------------------------ 2. history parity
@pytest.mark.parametrize("name", ["mat10000", "mat900", "stencil37x27"])
def test_history_parity(cm, ctx, oracle, golden_dir, name):
    O = oracle
    A, b = _system(O, golden_dir, name)
    mv, _ = R2.oracle_ops(O, A)
    run = lambda bb, maxit: R.cg(mv, bb, maxit=maxit, tol=TOL)
    ref = run(b, MAXIT)
    x, st, h = _gpu(cm, ctx, A, b)
    _check(run, b, ref, st, h, ND.true_res(O, A, b, x) / st.nrm0, name)


@pytest.mark.parametrize("name", ["mat10000", "stencil37x27"])
def test_ilu0_history_parity(cm, ctx, oracle, golden_dir, name):
    """M^-1 in the restatement is the oracle's ILU(0) and triangular solves: one application per iteration and one at the start"""
    O = oracle
    A, b = _system(O, golden_dir, name)
    mv, minv = R2.oracle_ops(O, A, O.ilu0(A))
    run = lambda bb, maxit: R.cg(mv, bb, minv=minv, maxit=maxit, tol=TOL)
    ref = run(b, MAXIT)
    x, st, h = _gpu(cm, ctx, A, b, precond=1)
    _check(run, b, ref, st, h, ND.true_res(O, A, b, x) / st.nrm0, name + " ILU(0)")
    assert st.trsv_form in (0, 1, 2) and st.n_levels_l > 0
    plain = R.cg(mv, b, maxit=MAXIT, tol=TOL)
    assert st.iters < plain.iters


def test_shift_and_ilu0_of_the_shifted_matrix(cm, ctx, oracle, golden_dir):
    """set_shift(d), d = 0.5 + i / n on mat900, against the restatement on A0 + diag(d); then with ilu0(shift=d) against the
    restatement with that matrix's ILU(0)"""
    O = oracle
    A0 = _mat(O, golden_dir, "mat900")
    n = A0.n
    d = 0.5 + np.arange(n) / n
    import scipy.sparse as sp
    S = (A0.to_scipy() + sp.diags(d)).tocsr()
    S.sort_indices()
    As = O.Csr(n, (S.indptr + A0.base).astype(np.int32), (S.indices + A0.base).astype(np.int32), S.data.copy(), n)
    assert As.nnz == A0.nnz                     # (every diagonal entry of mat900 is stored: the pattern is A0's)
    b = O.spmv(As, 1.0 + np.sin(np.arange(n)))
    mv0, _ = R2.oracle_ops(O, A0)
    run0 = lambda bb, maxit: R.cg(mv0, bb, d=d, maxit=maxit, tol=TOL)
    x, st, h = _gpu(cm, ctx, A0, b, d=d)
    _check(run0, b, run0(b, MAXIT), st, h, ND.true_res(O, As, b, x) / st.nrm0, "mat900 + diag(d)")
    mv, minv = R2.oracle_ops(O, As, O.ilu0(As))
    run = lambda bb, maxit: R.cg(mv, bb, minv=minv, maxit=maxit, tol=TOL)
    x, st, h = _gpu(cm, ctx, A0, b, precond=1, d=d, ilu_shift=True)
    _check(run, b, run(b, MAXIT), st, h, ND.true_res(O, As, b, x) / st.nrm0, "mat900 + diag(d), ILU(0)")


# ------------------------------------------------------------------ 3. bits
def test_repeatability_and_offset_operands(cm, ctx, oracle, golden_dir, sw):
    """n = 999 (499 pairs and an odd tail), without and with ILU(0): a second run, and the same solve with b and x 8 bytes past a
    16-byte boundary (the VEC = 0 kernels wherever x is an operand, k_init<0> for r0), give ||r0||, the history and x bit for
    bit.  Two right-hand sides: equal sums must not be a coincidence of one."""
    O = oracle
    sw("SPMV_MODE", "csr")
    A = _stencil(O, 37, 27)
    s = cm.Solver.from_host_csr(ctx, A.rowptr, A.colidx, A.val)
    try:
        for pc in (0, 1):
            if pc:
                s.ilu0()
            for seed in (7, 11):
                b = O.spmv(A, 1.0 + np.random.default_rng(seed).random(A.n))
                x, st, h = _gpu(cm, ctx, A, b, precond=pc, solver=s)
                x2, st2, h2 = _gpu(cm, ctx, A, b, precond=pc, solver=s)
                xo, sto, ho = _gpu(cm, ctx, A, b, precond=pc, solver=s, off=1)
                assert st.converged and len(h) == st.iters
                for xx, ss, hh in ((x2, st2, h2), (xo, sto, ho)):
                    assert (ss.iters, ss.converged, ss.nrm0, ss.nrm) == (st.iters, st.converged, st.nrm0, st.nrm)
                    np.testing.assert_array_equal(hh, h)
                    np.testing.assert_array_equal(xx, x)
    finally:
        s.close()


def test_batch_and_host_entry_points(cm, ctx, oracle, golden_dir, sw):
    """solve_many runs the new loop column by column (form 0): column j is the single solve of column j, bit for bit, history
    included.  api.cg / api.cg_lu_precond on host arrays build their own solver; with the SpMV form pinned they return the x of
    the resident solves, bit for bit."""
    O = oracle
    sw("SPMV_MODE", "csr")
    A = _mat(O, golden_dir, "mat900")
    n, K = A.n, 3
    Xs = np.stack([1.0 + np.sin((j + 1) * np.arange(n)) for j in range(K)], axis=1)
    B = np.stack([O.spmv(A, Xs[:, j]) for j in range(K)], axis=1)
    s = cm.Solver.from_host_csr(ctx, A.rowptr, A.colidx, A.val)
    dB, dX = ctx.array(np.asfortranarray(B).ravel(order="F")), ctx.array(np.ones(n * K))
    try:
        sts, form = s.solve_many(K, dB, n, dX, n, loop=cm.LOOP_CG, maxit=MAXIT, tol=TOL)
        assert form == 0
        X = dX.download().reshape(n, K, order="F")
        hs = [s.history(col=j) for j in range(K)]
        singles = []
        for j in range(K):
            xj, stj, hj = _gpu(cm, ctx, A, B[:, j], solver=s)
            assert sts[j].converged and stj.converged and sts[j].iters == stj.iters
            np.testing.assert_array_equal(X[:, j], xj)
            np.testing.assert_array_equal(hs[j], hj)
            singles.append(xj)
        s.ilu0()
        x_pc, st_pc, _ = _gpu(cm, ctx, A, B[:, 0], precond=1, solver=s)
        assert st_pc.converged and st_pc.iters < sts[0].iters
    finally:
        dB.free()
        dX.free()
        s.close()
    ok, x, dt, st = cm.cg(n, A.nnz, A.val, A.rowptr, A.colidx, None, None, B[:, 0], MAXIT, TOL)
    assert ok and st.converged and st.iters == sts[0].iters and st.nrm0 == sts[0].nrm0
    np.testing.assert_array_equal(x, singles[0])
    assert ND.true_res(O, A, B[:, 0], x) <= 2.0 * TOL * st.nrm0
    ok, x, dt, st = cm.cg_lu_precond(n, A.nnz, A.val, A.rowptr, A.colidx, None, None, B[:, 0], MAXIT, TOL)
    assert ok and st.converged and st.iters == st_pc.iters
    np.testing.assert_array_equal(x, x_pc)
    assert ND.true_res(O, A, B[:, 0], x) <= 2.0 * TOL * st.nrm0


# ------------------------------------------------------------------ 4. not positive definite
def test_a_negative_definite_matrix_is_a_breakdown_in_iteration_0(cm, ctx, oracle, golden_dir):
    """mat900 with the shift d = -17 (its spectrum lies in (0.06, 11.96)): gamma = p.Ap < 0.  The kernel that forms alpha
    freezes the loop before it touches x: breakdown, nothing counted, x is x0 bit for bit.  Under FLAG_NO_EXIT the same solve
    runs its 5 iterations."""
    O = oracle
    A = _mat(O, golden_dir, "mat900")
    b = _sin_rhs(O, A)
    d = np.full(A.n, -17.0)
    x0 = 1.0 + 0.25 * np.cos(np.arange(A.n))
    ref = R.cg(R2.oracle_ops(O, A)[0], b, x0=x0, d=d, maxit=5, tol=TOL)
    x, st, h = _gpu(cm, ctx, A, b, x0=x0, d=d, maxit=5)
    assert (ref.breakdown, ref.converged, ref.iters) == (1, 0, 0)
    assert (st.breakdown, st.converged, st.iters, len(h)) == (1, 0, 0, 0)
    np.testing.assert_array_equal(x, x0)
    assert st.t_solve < 5.0
    refn = R.cg(R2.oracle_ops(O, A)[0], b, x0=x0, d=d, maxit=5, tol=TOL, no_exit=True)
    x, st, h = _gpu(cm, ctx, A, b, x0=x0, d=d, maxit=5, flags=cm.FLAG_NO_EXIT)
    assert (st.breakdown, st.converged, st.iters, len(h)) == (0, 0, 5, 5)
    np.testing.assert_allclose(h, refn.hist, rtol=1e-6)


def test_no_exit_and_profile_count_one_product_per_iteration(cm, ctx, oracle, golden_dir):
    """FLAG_NO_EXIT runs every iteration; FLAG_PROFILE brackets the one SpMV of an iteration and, with ILU(0), its one M^-1 (two
    triangular solves) and the one before the loop; the iterate is the one of the unprofiled solve, bit for bit"""
    O = oracle
    A = _mat(O, golden_dir, "mat900")
    b = _sin_rhs(O, A)
    ref = R.cg(R2.oracle_ops(O, A)[0], b, maxit=7, tol=1e-2, no_exit=True)
    s = cm.Solver.from_host_csr(ctx, A.rowptr, A.colidx, A.val)
    try:
        x, st, h = _gpu(cm, ctx, A, b, solver=s, maxit=7, tol=1e-2, flags=cm.FLAG_NO_EXIT)
        assert st.iters == 7 and len(h) == 7 and not st.converged and not st.breakdown
        np.testing.assert_allclose(h, ref.hist, rtol=1e-6)
        x0, st0, _ = _gpu(cm, ctx, A, b, solver=s)
        x1, st1, _ = _gpu(cm, ctx, A, b, solver=s, flags=cm.FLAG_PROFILE)
        assert st1.iters == st0.iters and st1.converged and np.array_equal(x0, x1)
        # (the host looks at the state with a lag: up to three iterations are enqueued past the last one and return at once)
        assert st1.iters <= st1.n_spmv <= st1.iters + 3 and st1.n_trsv == 0 and st1.ms_spmv > 0.0
        s.ilu0()
        x2, st2, _ = _gpu(cm, ctx, A, b, precond=1, solver=s, flags=cm.FLAG_PROFILE)
        assert st2.converged and st2.iters <= st2.n_spmv <= st2.iters + 3
        assert st2.n_trsv == 2 * (st2.n_spmv + 1) and st2.ms_trsv > 0.0
    finally:
        s.close()


# ------------------------------------------------------------------ 5. symmetry
def _arrow(O, n):
    """first row and first column dense, the diagonal, nothing else: one row of n entries beside rows of 2"""
    import scipy.sparse as sp
    S = sp.lil_matrix((n, n))
    S[0, :] = 1.0 + np.arange(n) / n
    S[:, 0] = (1.0 + np.arange(n) / n).reshape(n, 1)
    S.setdiag(2.0 * n)
    return _from_scipy(O, S)


def test_symmetry_of_symmetric_matrices(cm, ctx, oracle, golden_dir):
    O = oracle
    for label, A in (("mat900", _mat(O, golden_dir, "mat900")), ("arrow1500", _arrow(O, 1500)), ("stencil", _stencil(O, 37, 27))):
        s = cm.Solver.from_host_csr(ctx, A.rowptr, A.colidx, A.val)
        try:
            assert s.symmetry() == (0, 0.0), label
            assert s.symmetry() == (0, 0.0), label          # (the kept verdict)
        finally:
            s.close()
    A = _arrow(O, 1500)
    assert A.rowptr[1] - A.rowptr[0] == 1500 and A.rowptr[2] - A.rowptr[1] == 2
    x, st, h = _gpu(cm, ctx, A, _sin_rhs(O, A))
    assert st.converged and ND.true_res(O, A, _sin_rhs(O, A), x) <= 2.0 * TOL * st.nrm0


def test_one_ulp_of_asymmetry_is_reported_refused_and_overridden(cm, ctx, oracle, golden_dir):
    """one off-diagonal value of mat900 raised by 1 ulp: symmetry() = (0, that ulp); LOOP_CG is CUDAMAT_ERR_ARG with both
    numbers in its message and x untouched, and solves under FLAG_ASSUME_SYMMETRIC; after set_values with the symmetric values
    the kept verdict is gone and CG solves"""
    O = oracle
    A = _mat(O, golden_dir, "mat900")
    b = _sin_rhs(O, A)
    i = 450
    k = int(A.rowptr[i] - A.base)
    if A.colidx[k] - A.base == i:
        k += 1
    val = A.val.copy()
    val[k] = np.nextafter(val[k], np.inf)
    ulp = abs(val[k] - A.val[k])
    assert ulp > 0.0
    s = cm.Solver.from_host_csr(ctx, A.rowptr, A.colidx, val)
    db, dx = ctx.array(b), ctx.array(np.ones(A.n))
    try:
        assert s.symmetry() == (0, ulp)
        msg = _refused(cm, s, db, dx, np.ones(A.n), "CUDAMAT_LOOP_CG", "symmetric", "%g" % ulp, loop=cm.LOOP_CG)
        assert "0 stored off-diagonal entries" in msg
        st = s.solve(db, dx, loop=cm.LOOP_CG, maxit=MAXIT, tol=TOL, flags=cm.FLAG_ASSUME_SYMMETRIC)
        assert st.converged and ND.true_res(O, A, b, dx.download()) <= 2.0 * TOL * st.nrm0
        s.set_values(A.val)
        assert s.symmetry() == (0, 0.0)
        dx.upload(np.ones(A.n))
        st = s.solve(db, dx, loop=cm.LOOP_CG, maxit=MAXIT, tol=TOL)
        assert st.converged and ND.true_res(O, A, b, dx.download()) <= 2.0 * TOL * st.nrm0
    finally:
        db.free()
        dx.free()
        s.close()


@pytest.mark.parametrize("name", ["mat3", "convdiff_g2"])
def test_matrices_that_are_not_symmetric_are_refused(cm, ctx, oracle, golden_dir, name):
    O = oracle
    A = _mat(O, golden_dir, "mat3") if name == "mat3" else ND.FAMILY[name](O)[0]
    import scipy.sparse as sp
    S = A.to_scipy().tocsr()
    P = sp.csr_matrix((np.ones(S.nnz), S.indices, S.indptr), shape=S.shape)       # the stored pattern
    both = P.multiply(P.T)                                                          # entries with a stored partner
    want_lone = int(round((P - both).sum()))
    want_diff = float(abs(S - S.T).multiply(both).max()) if both.nnz else 0.0
    s = cm.Solver.from_host_csr(ctx, A.rowptr, A.colidx, A.val)
    x0 = 1.0 + np.arange(A.n) / A.n
    db, dx = ctx.array(np.ones(A.n)), ctx.array(x0)
    try:
        lone, diff = s.symmetry()
        print(name, "unmatched", lone, "max |a_ij - a_ji|", diff)
        assert lone == want_lone and (lone > 0 or diff > 0.0)
        assert diff == want_diff
        _refused(cm, s, db, dx, x0, "CUDAMAT_LOOP_CG", "%d stored off-diagonal entries" % lone, "%g" % diff, loop=cm.LOOP_CG)
    finally:
        db.free()
        dx.free()
        s.close()


def test_symmetry_with_an_empty_row(cm, ctx, oracle):
    """row 2 of a 5 x 5 matrix stores nothing: symmetric when column 2 is empty too, one unmatched entry when (0, 2) is stored;
    a NaN against a number is a difference"""
    import scipy.sparse as sp
    O = oracle
    D = np.array([[4.0, 1.0, 0.0, 0.0, 2.0],
                  [1.0, 4.0, 0.0, 3.0, 0.0],
                  [0.0, 0.0, 0.0, 0.0, 0.0],
                  [0.0, 3.0, 0.0, 4.0, 0.0],
                  [2.0, 0.0, 0.0, 0.0, 4.0]])
    E = D.copy()
    E[0, 2] = 7.0
    F = D.copy()
    F[1, 3] = np.nan
    for M, want in ((D, (0, 0.0)), (E, (1, 0.0)), (F, (0, np.inf))):
        S = sp.csr_matrix(np.where(np.isnan(M), 1.0, M))
        A = _from_scipy(O, S)
        assert A.rowptr[3] == A.rowptr[2]
        val = A.val.copy()
        if np.isnan(M).any():
            val[[k for k in range(A.rowptr[1], A.rowptr[2]) if A.colidx[k] == 3][0]] = np.nan
        s = cm.Solver.from_host_csr(ctx, A.rowptr, A.colidx, val)
        try:
            assert s.symmetry() == want
        finally:
            s.close()


# ------------------------------------------------------------------ 6. refusals
def test_refusals(cm, ctx, oracle, golden_dir):
    O = oracle
    A = _mat(O, golden_dir, "mat900")
    b = _sin_rhs(O, A)
    s = cm.Solver.from_host_csr(ctx, A.rowptr, A.colidx, A.val)
    one = np.ones(A.n)
    db, dx = ctx.array(b), ctx.array(one)
    try:
        _refused(cm, s, db, dx, one, "CUDAMAT_FLAG_GUARD", "CUDAMAT_LOOP_CG", loop=cm.LOOP_CG, flags=cm.FLAG_GUARD)
        _refused(cm, s, db, dx, one, "CUDAMAT_PRECOND_BLOCK_ILU0", "CUDAMAT_LOOP_CG", loop=cm.LOOP_CG, precond=cm.PRECOND_BLOCK_ILU0)
        for loop in (4, 5, 6, 7, 9):
            _refused(cm, s, db, dx, one, "loop", loop=loop)
    finally:
        db.free()
        dx.free()
        s.close()


def test_a_sharded_solver_is_refused(cm, ctx, oracle, golden_dir):
    """rank 0 of 2 emulated ranks holding the first 450 rows of mat900: set_comm exchanges nothing, and both the loop and the
    symmetry query refuse the solver before any collective"""
    import dist_sim
    O = oracle
    A = _mat(O, golden_dir, "mat900")
    rp = A.rowptr - A.base
    s = cm.Solver.from_host_csr(ctx, rp[:451], A.colidx[:rp[450]] - A.base, A.val[:rp[450]], n_cols=900)
    comm = dist_sim.ThreadComm(cm, dist_sim.ThreadGroup(2), 0, ctx)
    one = np.ones(450)
    db, dx = ctx.array(one), ctx.array(one)
    try:
        s.set_comm(comm.struct)
        _refused(cm, s, db, dx, one, "CUDAMAT_LOOP_CG", "sharded", loop=cm.LOOP_CG)
        with pytest.raises(cm.CudamatError) as e:
            s.symmetry()
        assert e.value.code == ERR_ARG and "sharded" in str(e.value)
    finally:
        db.free()
        dx.free()
        s.close()


# ------------------------------------------------------------------ 7. edges
def _pair(cm, ctx, A, b, **kw):
    """the same call with LOOP_CG and with LOOP_PBICGSTAB2"""
    return _gpu(cm, ctx, A, b, **kw), _gpu(cm, ctx, A, b, loop=cm.LOOP_PBICGSTAB2, **kw)


def _same_outcome(a, c):
    (xa, sa, ha), (xc, sc, hc) = a, c
    assert (sa.iters, sa.converged, sa.breakdown, sa.half_exit) == (sc.iters, sc.converged, sc.breakdown, sc.half_exit)
    assert sa.nrm0 == sc.nrm0 and sa.nrm == sc.nrm and len(ha) == len(hc)
    np.testing.assert_array_equal(xa, xc)


def test_edges_return_what_the_other_loops_return(cm, ctx, oracle, golden_dir):
    O = oracle
    A = _mat(O, golden_dir, "mat900")
    b = _sin_rhs(O, A)
    # maxit = 0: no iteration, x0 comes back
    a, c = _pair(cm, ctx, A, b, maxit=0)
    _same_outcome(a, c)
    assert a[1].iters == 0 and not a[1].converged and np.array_equal(a[0], np.ones(A.n))
    # r0 = 0: x0 solves the system (b = A 1 is exact here: the entries of mat900 are small integers)
    b1 = O.spmv(A, np.ones(A.n))
    a, c = _pair(cm, ctx, A, b1)
    _same_outcome(a, c)
    assert a[1].nrm0 == 0.0 and a[1].iters == 0
    # a residual whose squares overflow: the range rules of the start refuse the solve, x0 untouched
    a, c = _pair(cm, ctx, A, b * 1e200)
    _same_outcome(a, c)
    assert a[1].breakdown and a[1].iters == 0 and np.array_equal(a[0], np.ones(A.n))


def test_one_row(cm, ctx, oracle):
    """n = 1: A = [2], b = [3], x0 = 1.  Every operation is exact: one iteration lands on x = 1.5 with r = 0"""
    O = oracle
    import scipy.sparse as sp
    A = _from_scipy(O, sp.csr_matrix(np.array([[2.0]])))
    b = np.array([3.0])
    ref = R.cg(R2.oracle_ops(O, A)[0], b, maxit=MAXIT, tol=TOL)
    x, st, h = _gpu(cm, ctx, A, b)
    assert (ref.iters, ref.converged, ref.breakdown) == (1, 1, 0) and ref.x[0] == 1.5
    assert (st.iters, st.converged, st.breakdown) == (1, 1, 0) and list(h) == [0.0]
    assert x[0] == 1.5
    x2, st2, _ = _gpu(cm, ctx, A, b, loop=cm.LOOP_PBICGSTAB2)      # context: the same call with the reference's loop
    print("n = 1, LOOP_PBICGSTAB2: iters", st2.iters, "converged", st2.converged, "breakdown", st2.breakdown, "x", x2[0])
