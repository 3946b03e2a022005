"""CUDAMAT_LOOP_BICGSTAB_L2 on the GPU against the numpy restatement of BiCGSTAB(2) (tests/bicgstab_l2_ref.py).

What two correct implementations of this loop can agree on, and what is asserted (the rules of tests/nondominant.py, with the
restatement in the oracle's place):
  - ||r_init|| to 1e-12;
  - the history (one entry per sweep) to 1e-6 over the prefix on which the restatement agrees with ITSELF when b is changed by
    1, 8 or 64 ulp either way, less 3 entries;
  - a converged solve has a TRUE residual ||b - A x|| <= 2 tol ||r_init|| (the recursive residual of this loop is the true
    one up to rounding: no preconditioned or shadow residual is carried), in a number of sweeps inside the restatement's own
    spread (+-10 %, at least +-2, widened by the counts of the perturbed runs);
  - bits where the library promises bits: two runs, 16-byte aligned and 8 bytes off, a column of solve_many and its single solve.
Every system has n <= 13 500."""
import os

import numpy as np
import pytest

from tests import bicgstab_l2_ref as R
from tests import nondominant as ND

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


def _from_dense(O, D):
    import scipy.sparse as sp
    S = sp.csr_matrix(D)
    S.sort_indices()
    return O.Csr(S.shape[0], S.indptr.astype(np.int32), S.indices.astype(np.int32), S.data.astype(np.float64).copy(), S.shape[0])


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
        kw.setdefault("loop", cm.LOOP_BICGSTAB_L2)
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


def _self_prefix(run, b, h0):
    """entries over which the restatement's history agrees with itself to 1e-6 when b is changed by ND.PERTURB ulp"""
    cap = ND.SELF_ITERS
    return min(ND.prefix(run(b * (1.0 + k * ND.EPS), cap).hist[:cap], h0[:cap], 1e-6) for k in ND.PERTURB), cap


def _iters_inside_spread(run, b, it_gpu, it_ref):
    """ND.iters_inside_oracle_spread with the restatement as the oracle"""
    if abs(it_gpu - it_ref) <= max(2, 0.1 * it_ref):
        return True, (it_ref, it_ref)
    counts = [it_ref] + [r.iters for r in (run(b * (1.0 + k * ND.EPS), MAXIT) for k in ND.PERTURB) if r.converged]
    lo, hi = min(counts), max(counts)
    return lo - max(2, 0.1 * lo, hi - lo) <= it_gpu <= hi + max(2, 0.1 * hi, hi - lo), (lo, hi)


def _check_history(run, b, ref, st, hg, label):
    assert abs(st.nrm0 - ref.nrm0) <= 1e-12 * ref.nrm0, (label, st.nrm0, ref.nrm0)
    assert len(hg) == st.iters, (label, len(hg), st.iters)
    l_self, cap = _self_prefix(run, b, ref.hist)
    l_gpu = ND.prefix(hg[:cap], ref.hist[:cap], 1e-6)
    print("%s: GPU sweeps %d conv %d brk %d, restatement sweeps %d conv %d; history equal to 1e-6 over %d entries (restatement vs "
          "itself, b changed by up to 64 ulp: %d)" % (label, st.iters, st.converged, st.breakdown, ref.iters, ref.converged, l_gpu, l_self))
    assert l_gpu >= min(l_self, len(ref.hist), len(hg), cap) - 3, (label, l_gpu, l_self)


def _check_converged(run, b, ref, st, true_rel, label):
    print("%s: true residual / ||r_init|| = %.3e (restatement's sweeps %d, GPU's %d)" % (label, true_rel, ref.iters, st.iters))
    assert ref.converged and st.converged and not st.breakdown, label
    assert st.nrm < TOL * st.nrm0
    assert true_rel <= 2.0 * TOL, (label, true_rel)
    ok, (lo, hi) = _iters_inside_spread(run, b, st.iters, ref.iters)
    assert ok, "%s: %d sweeps, outside the restatement's own spread %d..%d" % (label, st.iters, lo, hi)


# ------------------------------------------------------------------ 1. the loop exists
@pytest.mark.parametrize("rhs", ["sin", "urand"])
def test_loop_3_solves_mat900(cm, ctx, oracle, golden_dir, rhs):
    """Solver.solve(loop=3) is CUDAMAT_OK (CUDAMAT_ERR_ARG "loop" before this loop existed), converges with a true residual
    within 2 tol ||r_init||, and x is within 1e-5 of the solution the reference CPU program printed (tests/golden)"""
    O = oracle
    g = np.load(os.path.join(golden_dir, "bicg_mat900_%s.npz" % rhs))
    A = _mat(O, golden_dir, "mat900")
    b = g["b"]
    x, st, h = _gpu(cm, ctx, A, b, loop=3)
    tr = ND.true_res(O, A, b, x)
    err = np.linalg.norm(x - g["x"]) / np.linalg.norm(g["x"])
    print("mat900", rhs, "sweeps", st.iters, "true residual / nrm0", tr / st.nrm0, "distance to the printed solution", err)
    assert st.converged and not st.breakdown and not st.half_exit and st.loop_form == 0
    assert tr <= 2.0 * TOL * st.nrm0
    assert err <= 1e-5
    assert len(h) == st.iters and h[-1] < TOL * st.nrm0 and np.all(h[:-1] >= TOL * st.nrm0)


# ------------------------------------------------------------------ 2. the systems BiCGSTAB does not solve
@pytest.mark.parametrize("name", ["convdiff_g8", "convdiff_g40"])
def test_converges_where_bicgstab_does_not(cm, ctx, oracle, name):
    O = oracle
    A, b = ND.FAMILY[name](O)
    mv, _ = R.oracle_ops(O, A)
    run = lambda bb, maxit: R.bicgstab_l2(mv, bb, maxit=maxit, tol=TOL)
    ref = run(b, MAXIT)
    x, st, h = _gpu(cm, ctx, A, b)
    _check_converged(run, b, ref, st, ND.true_res(O, A, b, x) / st.nrm0, name)
    assert len(h) == st.iters
    # context (no new code runs here): the reference's loop on the same system, same tolerance, same 2000 iterations
    x2, st2, _ = _gpu(cm, ctx, A, b, loop=cm.LOOP_PBICGSTAB2)
    print(name, "LOOP_PBICGSTAB2: iters", st2.iters, "converged", st2.converged, "breakdown", st2.breakdown)
    assert not st2.converged


# ------------------------------------------------------------------ 3. history parity
def _system(O, golden_dir, name):
    if name in ND.FAMILY:
        return ND.FAMILY[name](O)
    A = _mat(O, golden_dir, name)
    return A, _sin_rhs(O, A)


@pytest.mark.parametrize("name", ["mat10000", "convdiff_g2", "weakdiag_t0.6"])
def test_history_parity(cm, ctx, oracle, golden_dir, name):
    O = oracle
    A, b = _system(O, golden_dir, name)
    mv, _ = R.oracle_ops(O, A)
    run = lambda bb, maxit: R.bicgstab_l2(mv, bb, maxit=maxit, tol=TOL)
    ref = run(b, MAXIT)
    x, st, h = _gpu(cm, ctx, A, b)
    _check_history(run, b, ref, st, h, name)
    _check_converged(run, b, ref, st, ND.true_res(O, A, b, x) / st.nrm0, name)


# ------------------------------------------------------------------ 4. ILU(0), and ILU(0) with a shift
@pytest.mark.parametrize("name", ["mat10000", "weakdiag_t1.0"])
def test_ilu0_history_parity_and_final_x(cm, ctx, oracle, golden_dir, name):
    """right preconditioning: M^-1 in the restatement is the oracle's ILU(0) and triangular solves; x = x0 + M^-1 y is formed
    after the loop and checked by its true residual"""
    O = oracle
    A, b = _system(O, golden_dir, name)
    mv, minv = R.oracle_ops(O, A, O.ilu0(A))
    run = lambda bb, maxit: R.bicgstab_l2(mv, bb, minv=minv, maxit=maxit, tol=TOL)
    ref = run(b, MAXIT)
    x, st, h = _gpu(cm, ctx, A, b, precond=1)
    _check_history(run, b, ref, st, h, name + " ILU(0)")
    _check_converged(run, b, ref, st, ND.true_res(O, A, b, x) / st.nrm0, name + " ILU(0)")
    assert st.trsv_form in (0, 1, 2) and st.n_levels_l > 0


def test_ilu0_with_a_shift(cm, ctx, oracle, golden_dir):
    """set_shift(d) + ilu0(shift=d), d = 0.5 + i / n on mat900, against the restatement on A0 + diag(d) with that matrix's ILU(0)"""
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
    mv, minv = R.oracle_ops(O, As, O.ilu0(As))
    run = lambda bb, maxit: R.bicgstab_l2(mv, bb, minv=minv, maxit=maxit, tol=TOL)
    ref = run(b, MAXIT)
    x, st, h = _gpu(cm, ctx, A0, b, precond=1, d=d, ilu_shift=True)
    _check_history(run, b, ref, st, h, "mat900 + diag(d), ILU(0)")
    _check_converged(run, b, ref, st, ND.true_res(O, As, b, x) / st.nrm0, "mat900 + diag(d), ILU(0)")
    # ... and the shift alone, no preconditioner
    mv0, _ = R.oracle_ops(O, A0)
    run0 = lambda bb, maxit: R.bicgstab_l2(mv0, bb, d=d, maxit=maxit, tol=TOL)
    ref0 = run0(b, MAXIT)
    x, st, h = _gpu(cm, ctx, A0, b, d=d)
    _check_history(run0, b, ref0, st, h, "mat900 + diag(d)")
    _check_converged(run0, b, ref0, st, ND.true_res(O, As, b, x) / st.nrm0, "mat900 + diag(d)")


# ------------------------------------------------------------------ 5. kernel edges
def _banded(n, half_width, seed):
    """non-symmetric band with a dominant diagonal: off-diagonals uniform in (-1, 1), diagonal = sum of their magnitudes + 1"""
    rng = np.random.default_rng(seed)
    D = np.zeros((n, n))
    for k in range(1, half_width + 1):
        D += np.diag(rng.uniform(-1, 1, n - k), k) + np.diag(rng.uniform(-1, 1, n - k), -k)
    return D + np.diag(np.abs(D).sum(axis=1) + 1.0)


def test_odd_tail_offset_operands_and_repeatability(cm, ctx, oracle):
    """n = 601 (300 pairs and an odd tail).  The same solve with b and x 8 bytes past a 16-byte boundary takes the VEC = 0
    kernels wherever x is an operand, and k_init<0> for r0 = b - A x0: ||r_init||, the history and x are bit-identical (the
    loop's start sums are formed from r0 in the pair order, and a thread's partial sums take the same terms in the same order
    for both alignments), and so is a second run.  Three right-hand sides: equal sums must not be a coincidence of one."""
    O = oracle
    n = 601
    A = _from_dense(O, _banded(n, 2, 601))
    b = O.spmv(A, 1.0 + np.random.default_rng(7).random(n))
    mv, _ = R.oracle_ops(O, A)
    run = lambda bb, maxit: R.bicgstab_l2(mv, bb, maxit=maxit, tol=TOL)
    ref = run(b, MAXIT)
    s = cm.Solver.from_host_csr(ctx, A.rowptr, A.colidx, A.val)
    try:
        x, st, h = _gpu(cm, ctx, A, b, solver=s)
        x_again, st_again, h_again = _gpu(cm, ctx, A, b, solver=s)
        x_off, st_off, h_off = _gpu(cm, ctx, A, b, solver=s, off=1)
        more = []
        for seed in (11, 12):
            bs = O.spmv(A, 1.0 + np.random.default_rng(seed).random(n))
            more.append((_gpu(cm, ctx, A, bs, solver=s), _gpu(cm, ctx, A, bs, solver=s, off=1)))
    finally:
        s.close()
    _check_converged(run, b, ref, st, ND.true_res(O, A, b, x) / st.nrm0, "n = 601")
    np.testing.assert_array_equal(x_again, x)
    np.testing.assert_array_equal(h_again, h)
    assert st_again.nrm0 == st.nrm0
    assert st_off.iters == st.iters and st_off.converged
    assert st_off.nrm0 == st.nrm0 and st_off.nrm == st.nrm
    np.testing.assert_array_equal(h_off, h)
    np.testing.assert_array_equal(x_off, x)
    for a, c in more:
        assert a[1].nrm0 == c[1].nrm0 and a[1].iters == c[1].iters
        np.testing.assert_array_equal(a[2], c[2])
        np.testing.assert_array_equal(a[0], c[0])


def test_several_spmv_workgroups(cm, ctx, oracle):
    """n = 777, 11 entries per row: several workgroups in every SpMV and every vector kernel, an odd tail"""
    O = oracle
    n = 777
    A = _from_dense(O, _banded(n, 5, 777))
    b = O.spmv(A, 1.0 + np.random.default_rng(8).random(n))
    mv, _ = R.oracle_ops(O, A)
    run = lambda bb, maxit: R.bicgstab_l2(mv, bb, maxit=maxit, tol=TOL)
    ref = run(b, MAXIT)
    x, st, h = _gpu(cm, ctx, A, b)
    _check_history(run, b, ref, st, h, "n = 777")
    _check_converged(run, b, ref, st, ND.true_res(O, A, b, x) / st.nrm0, "n = 777")


def test_one_row(cm, ctx, oracle):
    """n = 1: A = [2], b = [3], x0 = 1.  Every operation is exact: the first BiCG step lands on x = 1.5, r0 = 0, and the second
    finds gamma = 0 -- the restatement and the GPU stop there with the exact solution and say breakdown, not converged"""
    O = oracle
    A = _from_dense(O, np.array([[2.0]]))
    b = np.array([3.0])
    ref = R.bicgstab_l2(R.oracle_ops(O, A)[0], b, maxit=MAXIT, tol=TOL)
    x, st, h = _gpu(cm, ctx, A, b)
    assert (ref.iters, ref.converged, ref.breakdown) == (0, 0, 1) and ref.x[0] == 1.5
    assert (st.iters, st.converged, st.breakdown) == (0, 0, 1) and len(h) == 0
    assert x[0] == 1.5 and ND.true_res(O, A, b, x) == 0.0


def test_two_rows(cm, ctx, oracle):
    """n = 2: two BiCG steps span the whole space, so the first sweep's minimal-residual step works on residuals of rounding
    size.  Whatever it makes of them, x after the BiCG half solves the system to rounding: the true residual is within
    2 tol ||r_init|| on both sides, and the flags do not contradict each other."""
    O = oracle
    A = _from_dense(O, np.array([[2.0, 1.0], [1.0, 3.0]]))
    b = O.spmv(A, np.array([2.0, 3.0]))
    ref = R.bicgstab_l2(R.oracle_ops(O, A)[0], b, maxit=MAXIT, tol=TOL)
    x, st, h = _gpu(cm, ctx, A, b)
    print("n = 2: restatement sweeps %d conv %d brk %d true %g; GPU sweeps %d conv %d brk %d true %g" % (
        ref.iters, ref.converged, ref.breakdown, ND.true_res(O, A, b, ref.x), st.iters, st.converged, st.breakdown, ND.true_res(O, A, b, x)))
    assert ND.true_res(O, A, b, ref.x) <= 2.0 * TOL * ref.nrm0
    assert ND.true_res(O, A, b, x) <= 2.0 * TOL * st.nrm0
    assert st.iters <= 2 and len(h) == st.iters and not (st.converged and st.breakdown)


# ------------------------------------------------------------------ 6. breakdown
def test_breakdown_in_the_first_sweep(cm, ctx, oracle):
    """A = [[0, 1], [1, 0]], b = (1, 0), x0 = 0: u0 = r0 = (1, 0), u1 = A u0 = (0, 1), gamma = u1.r~ = 0.  The kernel that forms
    alpha freezes the loop; the host learns of it through the progress word, not by waiting for a scalar."""
    O = oracle
    A = _from_dense(O, np.array([[0.0, 1.0], [1.0, 0.0]]))
    b = np.array([1.0, 0.0])
    x, st, h = _gpu(cm, ctx, A, b, x0=np.zeros(2), maxit=500)
    assert st.breakdown == 1 and st.converged == 0 and st.iters <= 1
    assert st.iters == 0 and len(h) == 0 and np.array_equal(x, np.zeros(2))
    assert st.t_solve < 5.0


# ------------------------------------------------------------------ 7. FLAG_NO_EXIT
def test_no_exit_runs_every_sweep(cm, ctx, oracle, golden_dir):
    O = oracle
    A = _mat(O, golden_dir, "mat900")
    b = _sin_rhs(O, A)
    ref = R.bicgstab_l2(R.oracle_ops(O, A)[0], b, maxit=7, tol=1e-2, no_exit=True)
    x, st, h = _gpu(cm, ctx, A, b, maxit=7, tol=1e-2, flags=cm.FLAG_NO_EXIT)
    assert st.iters == 7 and len(h) == 7 and not st.converged and not st.breakdown
    assert np.all(np.isfinite(h))
    np.testing.assert_allclose(h, ref.hist, rtol=1e-6)


def test_profile_flag_counts_four_products_per_sweep(cm, ctx, oracle, golden_dir):
    """FLAG_PROFILE brackets every SpMV and every M^-1 of a sweep: 4 SpMVs, and with ILU(0) 4 applications = 8 triangular solves;
    the iterate is the one of the unprofiled solve, bit for bit"""
    O = oracle
    A = _mat(O, golden_dir, "mat900")
    b = _sin_rhs(O, A)
    s = cm.Solver.from_host_csr(ctx, A.rowptr, A.colidx, A.val)
    try:
        x0, st0, _ = _gpu(cm, ctx, A, b, solver=s)
        x1, st1, _ = _gpu(cm, ctx, A, b, solver=s, flags=cm.FLAG_PROFILE)
        assert st1.iters == st0.iters and st1.converged and np.array_equal(x0, x1)
        # (the host looks at the state with a lag: up to three sweeps are enqueued past the last one and return at once)
        assert st1.n_spmv % 4 == 0 and 4 * st1.iters <= st1.n_spmv <= 4 * (st1.iters + 3)
        assert st1.n_trsv == 0 and st1.ms_spmv > 0.0
        s.ilu0()
        x2, st2, _ = _gpu(cm, ctx, A, b, precond=1, solver=s, flags=cm.FLAG_PROFILE)
        assert st2.converged and st2.n_spmv % 4 == 0 and 4 * st2.iters <= st2.n_spmv <= 4 * (st2.iters + 3)
        assert st2.n_trsv == 2 * st2.n_spmv
        assert st2.ms_trsv > 0.0
    finally:
        s.close()


# ------------------------------------------------------------------ 8. refusals
def test_refusals(cm, ctx, oracle, golden_dir):
    O = oracle
    A = _mat(O, golden_dir, "mat900")
    b = _sin_rhs(O, A)
    s = cm.Solver.from_host_csr(ctx, A.rowptr, A.colidx, A.val)
    db, dx = ctx.array(b), ctx.array(np.ones(A.n))
    try:
        with pytest.raises(cm.CudamatError) as e:
            s.solve(db, dx, loop=cm.LOOP_BICGSTAB_L2, maxit=5, tol=TOL, flags=cm.FLAG_GUARD)
        assert e.value.code == ERR_ARG and "CUDAMAT_FLAG_GUARD" in str(e.value) and "CUDAMAT_LOOP_BICGSTAB_L2" in str(e.value)
        with pytest.raises(cm.CudamatError) as e:
            s.solve(db, dx, precond=cm.PRECOND_BLOCK_ILU0, loop=cm.LOOP_BICGSTAB_L2, maxit=5, tol=TOL)
        assert e.value.code == ERR_ARG and "CUDAMAT_PRECOND_BLOCK_ILU0" in str(e.value)
        with pytest.raises(cm.CudamatError) as e:
            s.solve(db, dx, loop=4, maxit=5, tol=TOL)
        assert e.value.code == ERR_ARG
        np.testing.assert_array_equal(dx.download(), np.ones(A.n))       # a refused solve touches nothing
    finally:
        db.free()
        dx.free()
        s.close()


# ------------------------------------------------------------------ 9. batch entry points, host-array entry points
def test_batch_and_host_entry_points(cm, ctx, oracle, golden_dir, sw):
    """solve_many runs the new loop column by column (form 0): column j is the single solve of column j, bit for bit, history
    included.  api.bicgstab_l2 / bicgstab_l2_lu_precond on host arrays build their own solver; with the SpMV form pinned
    (SPMV_MODE = csr: otherwise each solver chooses its form by timing) they return the x of the resident solves, bit for bit."""
    O = oracle
    sw("SPMV_MODE", "csr")
    A = _mat(O, golden_dir, "mat900")
    n, K = A.n, 3
    Xs = np.stack([1.0 + np.sin((j + 1) * np.arange(n)) for j in range(K)], axis=1)
    B = np.stack([O.spmv(A, Xs[:, j]) for j in range(K)], axis=1)
    s = cm.Solver.from_host_csr(ctx, A.rowptr, A.colidx, A.val)
    dB, dX = ctx.array(np.asfortranarray(B).ravel(order="F")), ctx.array(np.ones(n * K))
    try:
        sts, form = s.solve_many(K, dB, n, dX, n, loop=cm.LOOP_BICGSTAB_L2, maxit=MAXIT, tol=TOL)
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
    ok, x, dt, st = cm.bicgstab_l2(n, A.nnz, A.val, A.rowptr, A.colidx, None, None, B[:, 0], MAXIT, TOL)
    assert ok and st.converged and st.iters == sts[0].iters and st.nrm0 == sts[0].nrm0
    np.testing.assert_array_equal(x, singles[0])
    assert ND.true_res(O, A, B[:, 0], x) <= 2.0 * TOL * st.nrm0
    ok, x, dt, st = cm.bicgstab_l2_lu_precond(n, A.nnz, A.val, A.rowptr, A.colidx, None, None, B[:, 0], MAXIT, TOL)
    assert ok is True and st.converged and st.iters == st_pc.iters
    np.testing.assert_array_equal(x, x_pc)
    assert ND.true_res(O, A, B[:, 0], x) <= 2.0 * TOL * st.nrm0
