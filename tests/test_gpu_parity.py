"""GPU parity tests: the HIP path (through the C ABI, libcudamat_hip.so) against the CPU
oracle on the same inputs.  Integer/index work and integer-valued SpMV are bit-exact;
floating-point tolerances are the ones SURVEY.md section 8c states, written at each test.
Run on the GPU box with:  python -m pytest tests -m gpu"""
import math
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps


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
    """Set (value) or unset (None) a library switch for the rest of this test -- on the module's shared context
    (cudamat_ctx_set_option: a context reads the CUDAMAT_* environment only when it is created) AND in the environment
    (for contexts the test or the library creates later: cudamat_solve).  Afterwards the context is back to what the
    environment outside the test says."""
    def _sw(name, value):
        if value is None:
            monkeypatch.delenv("CUDAMAT_" + name, raising=False)
            ctx.reset_options()                 # = the environment, which still holds the test's other switches
        else:
            monkeypatch.setenv("CUDAMAT_" + name, str(value))
            ctx.set_option(name, value)
    yield _sw
    monkeypatch.undo()
    ctx.reset_options()


@pytest.fixture(autouse=True)
def _serial_oracle(oracle):
    """one OpenMP thread for the checker: its `reduction(+)` dots are then summed in one fixed order,
    so oracle iteration counts do not wander from run to run (the HIP path is deterministic already)"""
    before = oracle.num_threads()
    oracle.set_num_threads(1)
    yield
    oracle.set_num_threads(before)


def _load(oracle, golden_dir, name):
    return oracle.mtx_load(os.path.join(golden_dir, name + ".mtx"))


def _dev_csr(ctx, A):
    return ctx.array(A.rowptr), ctx.array(A.colidx), ctx.array(A.val)


# ------------------------------------------------------------------ generators
def test_rand_generator_matches_oracle(ctx, oracle):
    n, per_row, seed = 20000, 50, 0x5EED
    for row0, row1, base in [(0, n, 0), (5000, 9000, 1), (n - 17, n, 0)]:
        want = oracle.rand_rows(n, per_row, seed, row0, row1, base)
        nr = row1 - row0
        rp, ci, v = ctx.empty(nr + 1, np.int32), ctx.empty(nr * 50, np.int32), ctx.empty(nr * 50)
        ctx.gen_rand_rows(n, per_row, seed, row0, row1, base, rp, ci, v)
        np.testing.assert_array_equal(rp.download(), want.rowptr)
        np.testing.assert_array_equal(ci.download(), want.colidx)
        np.testing.assert_array_equal(v.download(), want.val)
        for a in (rp, ci, v):
            a.free()
    # tiny n: fewer than per_row distinct columns exist
    want = oracle.rand_rows(7, 50, 1)
    rp, ci, v = ctx.empty(8, np.int32), ctx.empty(49, np.int32), ctx.empty(49)
    ctx.gen_rand_rows(7, 50, 1, 0, 7, 0, rp, ci, v)
    np.testing.assert_array_equal(ci.download(), want.colidx)
    np.testing.assert_array_equal(v.download(), want.val)


@pytest.mark.parametrize("nx,ny", [(40, 25), (1, 9), (9, 1), (100, 100)])
def test_poisson_generator_matches_oracle(ctx, oracle, nx, ny):
    want = oracle.poisson5(nx, ny, base=1)
    n = nx * ny
    rp, ci, v = ctx.empty(n + 1, np.int32), ctx.empty(want.nnz, np.int32), ctx.empty(want.nnz)
    ctx.gen_poisson5(nx, ny, 0, n, 1, rp, ci, v)
    np.testing.assert_array_equal(rp.download(), want.rowptr)
    np.testing.assert_array_equal(ci.download(), want.colidx)
    np.testing.assert_array_equal(v.download(), want.val)
    # a row block carries a local rowptr and global column ids
    r0, r1 = n // 3, (2 * n) // 3 + 1
    k0, k1 = want.rowptr[r0] - 1, want.rowptr[r1] - 1
    rp2, ci2, v2 = ctx.empty(r1 - r0 + 1, np.int32), ctx.empty(k1 - k0, np.int32), ctx.empty(k1 - k0)
    ctx.gen_poisson5(nx, ny, r0, r1, 0, rp2, ci2, v2)
    np.testing.assert_array_equal(rp2.download(), want.rowptr[r0:r1 + 1] - want.rowptr[r0])
    np.testing.assert_array_equal(ci2.download(), want.colidx[k0:k1] - 1)
    np.testing.assert_array_equal(v2.download(), want.val[k0:k1])


def test_xstar_matches_oracle(ctx, oracle):
    x = ctx.empty(1000)
    ctx.gen_xstar(123, 1123, 77, x)
    np.testing.assert_array_equal(x.download(), oracle.xstar(5000, 77, 123, 1123))


# ------------------------------------------------------------------------ SpMV
@pytest.mark.parametrize("name", ["mat3", "mat900", "mat10000", "rand20000x50", "poisson300x200"])
@pytest.mark.parametrize("lanes", [None, 2, 16, 64])
def test_spmv_bit_exact_on_integer_data(ctx, oracle, golden_dir, name, lanes, sw):
    """integer-valued A and x: every product and partial sum is exact in fp64, so the
    result is independent of summation order => bit-exact against MatrixVectorMult
    (bicstab.cpp:69-80) for every lanes-per-row variant of the kernel."""
    if lanes:
        sw("SPMV_LANES", str(lanes))
    if name == "rand20000x50":
        A = oracle.rand_rows(20000, 50, 0x5EED)
    elif name == "poisson300x200":
        A = oracle.poisson5(300, 200, base=1)
    else:
        A = _load(oracle, golden_dir, name)
    rng = np.random.default_rng(1)
    x = rng.integers(-8, 9, A.n).astype(np.float64)
    want = oracle.spmv(A, x)
    rp, ci, v = _dev_csr(ctx, A)
    dx, dy = ctx.array(x), ctx.empty(A.n)
    ctx.spmv(A.n, rp, ci, v, A.base, dx, dy)
    np.testing.assert_array_equal(dy.download(), want)
    # the other base
    B = A.rebased(1 - A.base)
    rp2, ci2 = ctx.array(B.rowptr), ctx.array(B.colidx)
    dy.zero()
    ctx.spmv(A.n, rp2, ci2, v, B.base, dx, dy)
    np.testing.assert_array_equal(dy.download(), want)
    # csrmv call-site forms: (alpha,beta) = (-1,0) pbicgstab.cu:469, (-1,1) :646, (1,1) :676
    y0 = rng.integers(-8, 9, A.n).astype(np.float64)
    d = rng.integers(-3, 4, A.n).astype(np.float64)
    for alpha, beta in [(-1.0, 0.0), (-1.0, 1.0), (1.0, 1.0)]:
        dy.upload(y0)
        ctx.spmv(A.n, rp, ci, v, A.base, dx, dy, alpha=alpha, beta=beta)
        np.testing.assert_array_equal(dy.download(), oracle.csrmv(A, alpha, x, beta, y0))
    # fused diagonal term = mult_spec + csrmv(beta=1), pbicgstab.cu:675-676
    dd = ctx.array(d)
    ctx.spmv(A.n, rp, ci, v, A.base, dx, dy, d=dd)
    np.testing.assert_array_equal(dy.download(), oracle.csrmv(A, 1.0, x, 1.0, x * d))


# ---- which rounding the row epilogue of every SpMV form uses (csrc/device.h; mirrors and inputs: test_spmv_rounding.py)
@pytest.mark.parametrize("form", ["lanes2", "lanes16", "lanes64", "stream", "tiles"])
def test_epilogue_rounding_standalone_spmv(ctx, sw, form):
    """y = alpha (A x + d .* x) + beta y0 with real alpha, beta, d, y0 on integer A and x (exact row sums): every kernel of
    spmv_csr.hip gives fma(beta, y0, fl(alpha * fma(d, x, s))) bit for bit -- and that is not what separate roundings give."""
    import test_spmv_rounding as R
    c = R.case("poisson" if form == "stream" else "rand")
    R.assert_not_vacuous(c)
    if form.startswith("lanes"):
        sw("SPMV_LANES", form[5:])           # k_spmv<L>
    elif form == "tiles":
        sw("SPMV_FORM", "tiles")             # k_spmv_tiles (+ k_spmv_tiles_fix); "stream": rows of 5 take k_spmv_stream
    A = c["A"]
    rp, ci, v = _dev_csr(ctx, A)
    dx, dd, dy = ctx.array(c["x"]), ctx.array(c["d"]), ctx.array(c["y0"])
    ctx.spmv(A.n, rp, ci, v, A.base, dx, dy, alpha=R.ALPHA, beta=R.BETA, d=dd)
    y = dy.download()
    for a in (rp, ci, v, dx, dd, dy):
        a.free()
    print(form, "differs from fused in", R.differing(y, c["fused"]), "rows, from exact in", R.differing(y, c["exact"]))
    np.testing.assert_array_equal(y, c["fused"])


@pytest.mark.parametrize("form,which,mode,vdict,kernel,mirror", [
    ("stream_c", "poisson", "csr", "0", "k_spmv_stream_c<", "fused"),
    ("stream_d", "poisson_dict", "csr", None, "k_spmv_stream_d<", "fused"),
    ("pat", "poisson", "pat", "0", "k_spmv_pat<", "exact"),
    ("pat_d", "poisson_dict", "pat", None, "k_spmv_pat_d<", "exact"),
    ("sell", "rand", "sell", None, "k_spmv_sell", "exact"),
    ("blocked", "rand", "pb", None, "k_pb_phase1", "exact"),
])
def test_epilogue_rounding_of_a_shifted_solver_spmv(cm, ctx, sw, form, which, mode, vdict, kernel, mirror):
    """y = (A0 + I d) x through a solver (set_shift): the forms in spmv_csr.hip give fma(d, x, s); the pattern, SELL and
    blocked forms round d x and the sum separately (the oracle's csrmv).  The bits of a shifted product follow the form."""
    import test_spmv_rounding as R
    c = R.case(which)
    R.assert_not_vacuous(c)
    sw("SPMV_MODE", mode)
    if vdict is not None:
        sw("VALUE_DICT", vdict)
    A = c["A"]
    s = cm.Solver.from_host_csr(ctx, A.rowptr, A.colidx, A.val)
    assert s.spmv_kernel().startswith(kernel), s.spmv_kernel()
    s.set_shift(ctx.array(c["d"]))
    dx, dy = ctx.array(c["x"]), ctx.empty(A.n)
    s.spmv(dx, dy)
    y = dy.download()
    s.close()
    fused, exact = c["fused_shift"][:, 0], c["exact_shift"]
    print(form, "differs from fused in", R.differing(y, fused), "rows, from exact in", R.differing(y, exact))
    np.testing.assert_array_equal(y, fused if mirror == "fused" else exact)


@pytest.mark.parametrize("K", [1, 2, 8])
def test_epilogue_rounding_spmm(cm, ctx, sw, K):
    """k_spmm_csr, with the solver's one shift and with a shift per column: column j is fma(d_j, x_j, s_j), the fused
    epilogue of k_spmv<L>"""
    import test_spmv_rounding as R
    c = R.case("rand")
    R.assert_not_vacuous(c, columns=range(K))
    sw("SPMV_MODE", "csr")
    A, n = c["A"], c["n"]
    s = cm.Solver.from_host_csr(ctx, A.rowptr, A.colidx, A.val)
    assert s.spmv_kernel().startswith("k_spmv<"), s.spmv_kernel()
    s.set_shift(ctx.array(c["d"]))
    dX = ctx.array(np.asfortranarray(c["X"][:, :K]).ravel(order="F"))
    dD = ctx.array(np.asfortranarray(c["D"][:, :K]).ravel(order="F"))
    dY = ctx.empty(n * K)
    s.spmm(K, dX, n, dY, n)
    y_shift = dY.download().reshape((n, K), order="F")
    s.spmm_shifts(K, dX, n, dD, n, dY, n)
    y_shifts = dY.download().reshape((n, K), order="F")
    s.close()
    print("K", K, "one shift: differs from fused in", R.differing(y_shift, c["fused_shift"][:, :K]), "entries; per-column shifts:",
          R.differing(y_shifts, c["fused_shifts"][:, :K]))
    np.testing.assert_array_equal(y_shift, c["fused_shift"][:, :K])
    np.testing.assert_array_equal(y_shifts, c["fused_shifts"][:, :K])


def test_spmv_real_data_tolerance(ctx, oracle, golden_dir):
    """real-valued data: |y - y_ref| <= 4 nnz_row eps sum|a_ij x_j|"""
    A = oracle.rand_rows(20000, 50, 3)
    rng = np.random.default_rng(2)
    A.val[:] = rng.standard_normal(A.nnz)
    x = rng.standard_normal(A.n)
    want = oracle.spmv(A, x)
    absA = oracle.Csr(A.n, A.rowptr, A.colidx, np.abs(A.val), A.m)
    bound = 4 * 50 * EPS * oracle.spmv(absA, np.abs(x))
    rp, ci, v = _dev_csr(ctx, A)
    dx, dy = ctx.array(x), ctx.empty(A.n)
    ctx.spmv(A.n, rp, ci, v, 0, dx, dy)
    assert np.all(np.abs(dy.download() - want) <= bound)


def test_spmv_ragged_and_empty_rows(ctx, oracle):
    """empty rows, one very long row, n not a multiple of anything"""
    import scipy.sparse as sp
    rng = np.random.default_rng(5)
    n = 1237
    S = sp.random(n, n, density=0.01, random_state=7, format="lil")
    S[5, :] = 0
    S[17, :] = 1.0            # dense row
    S[n - 1, :] = 0           # empty last row
    S = S.tocsr()
    S.data[:] = rng.integers(1, 5, S.nnz)
    S.sort_indices()
    A = oracle.Csr(n, S.indptr.astype(np.int32), S.indices.astype(np.int32), S.data.astype(np.float64), n)
    x = rng.integers(-4, 5, n).astype(np.float64)
    rp, ci, v = _dev_csr(ctx, A)
    dx, dy = ctx.array(x), ctx.empty(n)
    ctx.spmv(n, rp, ci, v, 0, dx, dy)
    np.testing.assert_array_equal(dy.download(), oracle.spmv(A, x))


# ------------------------------------------------------------------- BLAS-1 pieces
@pytest.mark.parametrize("n", [1, 2, 3, 255, 256, 257, 1000, 100003, 1 << 20])
def test_dot_nrm2_axpy_scal(cm, ctx, n):
    rng = np.random.default_rng(n)
    x, y = rng.standard_normal(n), rng.standard_normal(n)
    dx, dy = ctx.array(x), ctx.array(y)
    ref = math.fsum(x * y)
    scale = math.fsum(np.abs(x * y))
    got = ctx.dot(n, dx, dy)
    assert abs(got - ref) <= 1e-13 * scale          # rel 1e-13 vs an exact sum
    assert got == ctx.dot(n, dx, dy)                # fixed reduction order => reproducible
    nr = ctx.nrm2(n, dx)
    assert abs(nr - math.sqrt(math.fsum(x * x))) <= 1e-13 * nr
    ctx.axpy(n, 0.375, dx, dy)
    np.testing.assert_allclose(dy.download(), 0.375 * x + y, rtol=4 * EPS, atol=4 * EPS)
    ctx.scal(n, -2.0, dx)
    np.testing.assert_array_equal(dx.download(), -2.0 * x)
    # misaligned operands take the scalar path: same result
    if n > 3:
        big = ctx.array(np.concatenate([[0.0], x]))
        out = ctx.empty(1)
        cm.api.check(cm.lib().cudamat_dot(ctx.h, n - 1, big.ptr + 8, big.ptr + 8, out.ptr))
        assert abs(out.download()[0] - math.fsum(x[:n - 1] ** 2)) <= 1e-13 * math.fsum(x ** 2)


# ------------------------------------------------------------------------- solver
def _solve_dev(cm, ctx, A, b, x0=None, d=None, **kw):
    s = cm.Solver.from_host_csr(ctx, A.rowptr, A.colidx, A.val)
    db = ctx.array(b)
    dx = ctx.array(np.ones(A.n) if x0 is None else x0)
    if d is not None:
        s.set_shift(ctx.array(d))
    st = s.solve(db, dx, **kw)
    x = dx.download()
    h = s.history()
    s.close()
    return x, st, h


@pytest.mark.parametrize("name,tol", [("mat900", 1e-6), ("mat900", 1e-8), ("mat10000", 1e-8)])
def test_pbicgstab_no_precond_vs_oracle(cm, ctx, oracle, golden_dir, name, tol):
    """gpu_pbicgstab (pbicgstab.cu:45-154) with M = I, x0 = 1, b = A x*.
    Tolerances: true residual <= 1e-7 * ||r0|| at tol 1e-8 (10 tol in general),
    ||x_gpu - x_cpu|| / ||x_cpu|| <= 1e-5, iteration count within +-10 % (>= +-2)."""
    A = _load(oracle, golden_dir, name)
    xs = 1.0 + np.sin(np.arange(A.n))
    b = oracle.spmv(A, xs)
    xo, so, ho = oracle.pbicgstab(A, b, maxit=2000, tol=tol, want_hist=True)
    x, st, h = _solve_dev(cm, ctx, A, b, loop=cm.LOOP_PBICGSTAB, maxit=2000, tol=tol)
    assert st.converged and so.converged
    assert abs(st.iters - so.iters) <= max(2, 0.1 * so.iters)
    assert np.linalg.norm(x - xo) / np.linalg.norm(xo) <= 1e-5
    assert np.linalg.norm(b - oracle.spmv(A, x)) <= 10 * tol * so.nrm0
    assert abs(st.nrm0 - so.nrm0) <= 1e-12 * so.nrm0
    # the convergence history starts out identical to rounding and ends below tol
    k = min(len(h), 8)
    np.testing.assert_allclose(h[:k], ho[:k], rtol=1e-9)
    assert len(h) == 2 * st.iters + (1 if st.half_exit else 0)
    assert h[-1] < tol * st.nrm0 and np.all(h[:-1] >= tol * st.nrm0)


def test_freeze_on_exit_is_exact(cm, ctx, oracle, golden_dir):
    """kernels enqueued past the stopping point must not change x: the result with a huge
    maxit is bit-identical to the result when the loop is cut at the converged iteration."""
    A = _load(oracle, golden_dir, "mat900")
    b = oracle.spmv(A, 1.0 + np.sin(np.arange(A.n)))
    x1, st1, _ = _solve_dev(cm, ctx, A, b, loop=cm.LOOP_PBICGSTAB, maxit=2000, tol=1e-8)
    cut = st1.iters + (1 if st1.half_exit else 0)
    x2, st2, _ = _solve_dev(cm, ctx, A, b, loop=cm.LOOP_PBICGSTAB, maxit=cut, tol=1e-8)
    assert st2.iters == st1.iters and st2.half_exit == st1.half_exit and st2.converged
    np.testing.assert_array_equal(x1, x2)
    # and a repeat gives the same bits (deterministic reductions)
    x3, st3, _ = _solve_dev(cm, ctx, A, b, loop=cm.LOOP_PBICGSTAB, maxit=2000, tol=1e-8)
    np.testing.assert_array_equal(x1, x3)


def test_pbicgstab2_variants_vs_oracle(cm, ctx, oracle, golden_dir):
    """gpu_pbicgstab2 (pbicgstab.cu:581-754): mat3 known answer through the (A0 + I d) form,
    then mat900 with its diagonal split off, against the oracle restatement."""
    A0 = _load(oracle, golden_dir, "mat3_A0")
    d = oracle.to_dense_vector(_load(oracle, golden_dir, "vec3_d"))
    b = oracle.to_dense_vector(_load(oracle, golden_dir, "vec3"))
    x, st, h = _solve_dev(cm, ctx, A0, b, x0=np.ones(3), d=d, loop=cm.LOOP_PBICGSTAB2, maxit=2000, tol=1e-5)
    ok, xo, so, ho = oracle.pbicgstab2(A0, b, d=d, tol=1e-5, want_hist=True)
    assert st.converged and st.iters == so.iters == 3
    np.testing.assert_allclose(x, [7 / 6, 17 / 3, -23 / 6], rtol=1e-7)
    np.testing.assert_allclose(h[:2], ho[:2], rtol=1e-6)   # the third is pure rounding noise
    assert len(h) == 3 and h[2] < 1e-5 * st.nrm0

    A = _load(oracle, golden_dir, "mat900")
    S = A.to_scipy().tolil()
    dg = S.diagonal().copy()
    S.setdiag(0)
    S = S.tocsr()
    S.eliminate_zeros()
    S.sort_indices()
    A0 = oracle.Csr(A.n, (S.indptr + 1).astype(np.int32), (S.indices + 1).astype(np.int32), S.data, A.n)
    b = oracle.spmv(A, 1.0 + np.sin(np.arange(A.n)))
    x0 = np.cos(np.arange(A.n))
    ok, xo, so = oracle.pbicgstab2(A0, b, d=dg, x0=x0, tol=1e-8)
    x, st, h = _solve_dev(cm, ctx, A0, b, x0=x0, d=dg, loop=cm.LOOP_PBICGSTAB2, maxit=2000, tol=1e-8)
    assert ok and st.converged and abs(st.iters - so.iters) <= max(2, 0.1 * so.iters)
    assert np.linalg.norm(x - xo) / np.linalg.norm(xo) <= 1e-5
    assert np.linalg.norm(b - oracle.spmv(A, x)) <= 1e-7 * so.nrm0


def test_pbicgstab2_breakdown_and_maxit(cm, ctx, oracle):
    A = oracle.poisson5(30, 30, base=0)
    b = oracle.spmv(A, 1.0 + np.sin(np.arange(A.n)))
    x, st, h = _solve_dev(cm, ctx, A, b, loop=cm.LOOP_PBICGSTAB2, maxit=3, tol=1e-12)
    ok, xo, so = oracle.pbicgstab2(A, b, maxit=3, tol=1e-12)
    assert not st.converged and not st.breakdown and st.iters == 3 == so.iters
    np.testing.assert_allclose(x, xo, rtol=1e-9)
    # omega = 0 on a skew-symmetric matrix => the |omega| < 1e-5 guard (pbicgstab.cu:735)
    Ask = oracle.Csr(2, np.array([0, 1, 2], np.int32), np.array([1, 0], np.int32), np.array([1.0, -1.0]), 2)
    x, st, h = _solve_dev(cm, ctx, Ask, np.array([1.0, 2.0]), loop=cm.LOOP_PBICGSTAB2, maxit=10, tol=1e-12)
    assert st.breakdown and not st.converged and st.iters == 1
    # maxit = 0 leaves x = x0
    x, st, h = _solve_dev(cm, ctx, A, b, loop=cm.LOOP_PBICGSTAB, maxit=0, tol=1e-8)
    assert st.iters == 0 and not st.converged and np.all(x == 1.0)
    # the same skew-symmetric system through the loops WITHOUT a reference guard (pbicgstab.cu:45-154 would spin on
    # NaNs up to maxit): t.t = ... / 0 somewhere => a NaN residual => the loop stops at once and reports a breakdown
    for loop in (cm.LOOP_PBICGSTAB, cm.LOOP_PIPELINED):
        x, st, h = _solve_dev(cm, ctx, Ask, np.array([1.0, 2.0]), loop=loop, maxit=500, tol=1e-12)
        assert not st.converged and (st.breakdown or st.iters == 500)
        if st.breakdown:
            assert st.iters <= 3


def test_drop_in_entry_points(cm, oracle, golden_dir):
    """the host-pointer functions that mirror pbicgstab.h:113,116 (bool result, x, dtAlg)"""
    A = _load(oracle, golden_dir, "mat10000")
    xs = 1.0 + np.sin(np.arange(A.n))
    b = oracle.spmv(A, xs)
    ok, x, dt, st = cm.bicgstab(A.n, A.nnz, A.val, A.rowptr, A.colidx, b, 2000, 1e-8)
    oko, xo, so = oracle.pbicgstab2(A, b, tol=1e-8)
    assert ok and oko and dt > 0
    assert np.linalg.norm(x - xo) / np.linalg.norm(xo) <= 1e-5
    assert np.linalg.norm(x - xs) / np.linalg.norm(xs) <= 5e-6
    ok, x, dt, st = cm.bicgstab(A.n, A.nnz, A.val, A.rowptr, A.colidx, b, 5, 1e-8)
    assert not ok and st.iters == 5
    # solution agrees with the reference CPU program's own output on the same system
    g = np.load(os.path.join(golden_dir, "bicg_mat10000_sin.npz"))
    ok, x, dt, st = cm.bicgstab(A.n, A.nnz, A.val, A.rowptr, A.colidx, g["b"], 2000, 1e-8)
    assert ok and np.linalg.norm(x - g["x"]) / np.linalg.norm(g["x"]) <= 2e-5   # its 6-digit print + eps 1e-6
    A0 = _load(oracle, golden_dir, "mat3_A0")
    d = oracle.to_dense_vector(_load(oracle, golden_dir, "vec3_d"))
    b3 = oracle.to_dense_vector(_load(oracle, golden_dir, "vec3"))
    ok, x, dt, st = cm.bicgstab_d(3, A0.nnz, A0.val, A0.rowptr, A0.colidx, d, np.ones(3), b3, 2000, 1e-5)
    assert ok
    np.testing.assert_allclose(x, [7 / 6, 17 / 3, -23 / 6], rtol=1e-7)


@pytest.mark.parametrize("rhs", ["sin", "urand"])
def test_mat900_solution_matches_reference_program(cm, ctx, oracle, golden_dir, rhs):
    """BASELINE configs[0] (mat900 through the reference's CPU program) against the HIP path: the UNMODIFIED
    bicstab_omp binary's printed solution (6 digits, its eps 1e-6; tests/golden/bicg_mat900_*.npz) and the
    oracle's BiCG restatement run to the 1e-8 BASELINE states, both vs the HIP BiCGSTAB solution at tol 1e-8."""
    g = np.load(os.path.join(golden_dir, "bicg_mat900_%s.npz" % rhs))
    A = _load(oracle, golden_dir, "mat900")
    b = g["b"]
    x, st, h = _solve_dev(cm, ctx, A, b, loop=cm.LOOP_PBICGSTAB, maxit=2000, tol=1e-8)
    assert st.converged
    assert np.linalg.norm(x - g["x"]) / np.linalg.norm(g["x"]) <= 2e-5          # 6-digit print + eps 1e-6
    xc, itc = oracle.bicg(A, b, maxit=2000, eps=1e-8)                            # C1 at the stated tolerance
    assert 0 < itc < 2000
    assert np.linalg.norm(x - xc) / np.linalg.norm(xc) <= 1e-5                   # SURVEY 8c (kappa(mat900) ~ 195)
    r0 = np.linalg.norm(b - oracle.spmv(A, np.ones(A.n)))
    assert np.linalg.norm(b - oracle.spmv(A, x)) <= 1e-7 * r0                    # true residual, SURVEY 8c
    assert np.linalg.norm(b - oracle.spmv(A, xc)) <= 1e-7 * np.linalg.norm(b)    # the CPU path stops on ||r|| / ||b||


def test_rand_matrix_solution_matches_reference_program(cm, ctx, oracle, golden_dir):
    """the synthetic random matrix (integer entries) at 20000 x 50: GPU BiCGSTAB solution vs the
    UNMODIFIED reference CPU program's printed solution (tests/golden/bicg_rand20000x50.npz)."""
    g = np.load(os.path.join(golden_dir, "bicg_rand20000x50.npz"))
    A = oracle.rand_rows(20000, 50, 0x5EED)
    x, st, h = _solve_dev(cm, ctx, A, g["b"], loop=cm.LOOP_PBICGSTAB, maxit=2000, tol=1e-8)
    assert st.converged
    assert np.linalg.norm(x - g["x"]) / np.linalg.norm(g["x"]) <= 1e-5
    np.testing.assert_allclose(x, oracle.xstar(20000, 0x5EED + 1), rtol=1e-7)


# ------------------------------------------------------------- ILU(0) + triangular solves
def _real_sparse(oracle, n, density, seed, base=0):
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    S = sp.random(n, n, density=density, random_state=seed, format="csr")
    S.data[:] = rng.uniform(-1, 1, S.nnz)
    S.setdiag(0)
    S.eliminate_zeros()
    # strictly diagonally dominant rows keep ILU(0) (no pivoting) well conditioned
    S = (S + sp.diags(1.0 + rng.random(n) + np.asarray(abs(S).sum(axis=1)).ravel())).tocsr()
    S.sort_indices()
    return oracle.Csr(n, (S.indptr + base).astype(np.int32), (S.indices + base).astype(np.int32),
                      S.data.copy(), n)


@pytest.mark.parametrize("name", ["mat900", "mat10000", "rand20000x50", "real3000", "longrows", "grid300", "chain70000"])
def test_ilu0_factors_and_trsv_vs_oracle(cm, ctx, oracle, golden_dir, name):
    """cusparseDcsrilu0 + csrsv_solve replacements (pbicgstab.cu:359, :92-98) against the oracle's
    sequential IKJ ILU(0) and substitutions.  Tolerance: rtol 1e-12 on the factors (same operations,
    different association only inside a row update), 1e-10 on the preconditioner application."""
    if name == "rand20000x50":
        A = oracle.rand_rows(20000, 50, 0x5EED)
    elif name == "real3000":
        A = _real_sparse(oracle, 3000, 0.004, 11, base=1)
    elif name == "longrows":
        A = _real_sparse(oracle, 400, 0.6, 5)          # ~240 entries per row, deep dependency chains
    elif name == "grid300":
        A = oracle.poisson5(300, 300)                   # 599 levels: two 8-bit passes of the device's level sort
    elif name == "chain70000":                          # a tridiagonal chain: as many levels as rows (three passes)
        n = 70000
        rp = np.concatenate([[0], np.cumsum(np.r_[2, np.full(n - 2, 3), 2])]).astype(np.int32)
        ci = np.concatenate([[0, 1]] + [[i - 1, i, i + 1] for i in range(1, n - 1)] + [[n - 2, n - 1]]).astype(np.int32)
        va = np.concatenate([[4.0, -1.0]] + [[-1.0, 4.0, -1.5]] * (n - 2) + [[-1.0, 4.0]])
        A = oracle.Csr(n, rp, ci, va, n)
    else:
        A = _load(oracle, golden_dir, name)
    s = cm.Solver.from_host_csr(ctx, A.rowptr, A.colidx, A.val)
    s.ilu0()
    want = oracle.ilu0(A)
    np.testing.assert_allclose(s.ilu0_values(), want, rtol=1e-12, atol=1e-14)
    rng = np.random.default_rng(0)
    rhs = rng.standard_normal(A.n)
    dr, do = ctx.array(rhs), ctx.empty(A.n)
    s.precond_apply(dr, do)
    ref = oracle.trsv_upper(A, want, oracle.trsv_lower_unit(A, want, rhs))
    np.testing.assert_allclose(do.download(), ref, rtol=1e-10, atol=1e-12)
    # level counts equal the dependency depth the oracle computes
    st = s.solve(dr, do, precond=cm.PRECOND_ILU0, maxit=1, tol=1e-30, flags=cm.FLAG_X0_ONES)
    assert st.n_levels_l == oracle.levels(A, upper=False)[0]
    assert st.n_levels_u == oracle.levels(A, upper=True)[0]
    s.close()


@pytest.mark.parametrize("name,tol", [("mat900", 1e-6), ("mat900", 1e-8), ("mat10000", 1e-8)])
def test_pbicgstab_ilu0_vs_oracle(cm, ctx, oracle, golden_dir, name, tol):
    """bicgstab_lu_precond's loop (pbicgstab.cu:45-154 with M = LU) vs the oracle restatement"""
    A = _load(oracle, golden_dir, name)
    xs = 1.0 + np.sin(np.arange(A.n))
    b = oracle.spmv(A, xs)
    xo, so, ho = oracle.pbicgstab(A, b, vm=oracle.ilu0(A), maxit=2000, tol=tol, want_hist=True)
    x, st, h = _solve_dev(cm, ctx, A, b, precond=cm.PRECOND_ILU0, loop=cm.LOOP_PBICGSTAB, maxit=2000, tol=tol)
    assert st.converged and abs(st.iters - so.iters) <= max(2, 0.1 * so.iters)
    assert np.linalg.norm(x - xo) / np.linalg.norm(xo) <= 1e-5
    assert np.linalg.norm(b - oracle.spmv(A, x)) <= 10 * tol * so.nrm0
    k = min(len(h), 6)
    np.testing.assert_allclose(h[:k], ho[:k], rtol=1e-8)


def test_ilu0_rejects_missing_diagonal_and_lu_drop_in(cm, ctx, oracle, golden_dir):
    A3 = _load(oracle, golden_dir, "mat3")      # no (2,2) entry: violates pbicgstab.h:118
    s = cm.Solver.from_host_csr(ctx, A3.rowptr, A3.colidx, A3.val)
    with pytest.raises(cm.CudamatError) as e:
        s.ilu0()
    assert e.value.code == 3
    s.close()
    # numerically zero pivot
    Z = oracle.Csr(2, np.array([0, 2, 4], np.int32), np.array([0, 1, 0, 1], np.int32),
                   np.array([1.0, 1.0, 1.0, 1.0]), 2)
    s = cm.Solver.from_host_csr(ctx, Z.rowptr, Z.colidx, Z.val)
    with pytest.raises(cm.CudamatError) as e:
        s.ilu0()
    assert e.value.code == 3
    s.close()
    A = _load(oracle, golden_dir, "mat10000")
    xs = 1.0 + np.sin(np.arange(A.n))
    b = oracle.spmv(A, xs)
    ok, x, dt, st = cm.bicgstab_lu_precond(A.n, A.nnz, A.val, A.rowptr, A.colidx, b, 2000, 1e-8)
    assert ok and st.converged and st.n_levels_l == 199
    assert np.linalg.norm(x - xs) / np.linalg.norm(xs) <= 5e-6
    ok, x, dt, st = cm.bicgstab_lu_precond(A.n, A.nnz, A.val, A.rowptr, A.colidx, b, 2, 1e-8)
    assert ok and not st.converged       # the reference returns true regardless (pbicgstab.cu:408)


# ------------------------------------------------- blocked (propagation blocking) SpMV
def _spmv_via_solver(cm, ctx, A, x, d=None):
    s = cm.Solver.from_host_csr(ctx, A.rowptr, A.colidx, A.val, n_cols=A.m)
    if d is not None:
        s.set_shift(ctx.array(d))
    dx, dy = ctx.array(x), ctx.empty(A.n)
    s.spmv(dx, dy)
    y = dy.download()
    s.close()
    return y


@pytest.mark.parametrize("case", ["rand_real", "rand_int_base1", "poisson", "ragged", "tiny"])
def test_blocked_spmv_is_bit_exact(cm, ctx, oracle, case, sw):
    """the two-phase kernels (csrc/spmv_pb.hip) add each row's products in increasing column order,
    one rounding per product and per addition: the SAME sequence of roundings as the reference CPU
    loop b[i] += A.Value[j] * x[A.Col[j]] (bicstab.cpp:72-77) => bit-exact even on real-valued data."""
    sw("SPMV_MODE", "pb")
    rng = np.random.default_rng(9)
    if case == "rand_real":
        A = oracle.rand_rows(20000, 50, 0x5EED)
        A.val[:] = rng.standard_normal(A.nnz)
    elif case == "rand_int_base1":
        A = oracle.rand_rows(30011, 33, 5, base=1)
    elif case == "poisson":
        A = oracle.poisson5(173, 59, base=0)
        A.val[:] = rng.standard_normal(A.nnz)
    elif case == "tiny":
        A = oracle.rand_rows(7, 50, 1)
    else:
        import scipy.sparse as sp
        n = 5000
        S = sp.random(n, n, density=0.004, random_state=3, format="lil")
        S[5, :] = 0
        S[17, :] = 1.0            # one dense row: segments longer than a wavefront
        S[n - 1, :] = 0
        S = S.tocsr()
        S.data[:] = rng.standard_normal(S.nnz)
        S.sort_indices()
        A = oracle.Csr(n, S.indptr.astype(np.int32), S.indices.astype(np.int32), S.data.astype(np.float64), n)
    x = rng.standard_normal(A.n)
    # default: one ds_add_f64 instruction per segment step, relying on the observed lane order of equal addresses;
    # CUDAMAT_PB_STRICT=1: every rank of a run of equal rows is its own instruction -- the order of a row's additions is
    # architected.  Both must reproduce the reference loop bit for bit (the 20000-column cases have runs of ~25 equal rows
    # per step, the dense row of `ragged` runs that cross the 64-entry cut): this is the guard of the observed property.
    for strict in ("0", "1"):
        sw("PB_STRICT", strict)
        np.testing.assert_array_equal(_spmv_via_solver(cm, ctx, A, x), oracle.spmv(A, x))
        d = rng.standard_normal(A.n)
        np.testing.assert_array_equal(_spmv_via_solver(cm, ctx, A, x, d=d), oracle.csrmv(A, 1.0, x, 1.0, x * d))


def test_lds_order_probe_guards_the_default_blocked_form(cm, ctx, oracle, sw, capfd):
    """The default phase 2 is bit-exact only where the LDS serves equal addresses of one ds_add_f64 in lane order -- an
    OBSERVED property of gfx950.  Every context checks it at its first blocked SpMV (k_lds_order_probe, one wave, ~30 us)
    and falls back to the architected-order form when it does not hold.  Here: the probe passes on this device (default
    form selected, nothing printed); with the probe forced to fail (PB_PROBE_FAIL=1) the context says so on stderr, runs
    `k_pb_phase2` in its architected-order form WITHOUT PB_STRICT being set, and the results -- SpMV on real data, and a
    preconditioned solve whose far parts run through the same phase 2 -- stay bit-identical to the oracle / the default."""
    sw("SPMV_MODE", "pb")
    rng = np.random.default_rng(19)
    A = oracle.rand_rows(20000, 50, 0x5EED)
    A.val[:] = rng.standard_normal(A.nnz)
    x = rng.standard_normal(A.n)
    want = oracle.spmv(A, x)

    def run():
        s = cm.Solver.from_host_csr(ctx, A.rowptr, A.colidx, A.val)
        dx, dy = ctx.array(x), ctx.empty(A.n)
        s.spmv(dx, dy)
        name, y = s.spmv_kernel(), dy.download()
        for a in (dx, dy):
            a.free()
        s.close()
        return name, y

    capfd.readouterr()
    name, y = run()
    out = capfd.readouterr()
    assert name == "k_pb_phase1 + k_pb_phase2" and "LDS order probe" not in out.err      # the property holds here
    np.testing.assert_array_equal(y, want)
    sw("PB_PROBE_FAIL", 1)
    name, y = run()
    out = capfd.readouterr()
    assert name == "k_pb_phase1 + k_pb_phase2 (architected order)", name
    assert "reported NOT in lane order (PB_PROBE_FAIL)" in out.err and "architected-order" in out.err
    np.testing.assert_array_equal(y, want)
    # the triangular solves' far parts take the same decision (hybrid form forced on this small system)
    sw("TRSV_HYBRID", 1)
    Ai = oracle.rand_rows(20000, 50, 0x5EED)
    b = oracle.spmv(Ai, oracle.xstar(20000, 0x5EEE))
    x_forced, st_f, _ = _solve_dev(cm, ctx, Ai, b, precond=cm.PRECOND_ILU0, loop=cm.LOOP_PBICGSTAB, maxit=100, tol=1e-10)
    sw("PB_PROBE_FAIL", None)
    x_default, st_d, _ = _solve_dev(cm, ctx, Ai, b, precond=cm.PRECOND_ILU0, loop=cm.LOOP_PBICGSTAB, maxit=100, tol=1e-10)
    assert st_f.converged and st_d.converged and st_f.iters == st_d.iters
    np.testing.assert_array_equal(x_forced, x_default)


@pytest.mark.parametrize("case", ["rand_real", "long_rows", "empty_and_dense", "few_values", "wide_sub_blocks"])
def test_two_pass_fill_builds_the_copy_the_single_pass_kernel_builds(cm, ctx, oracle, case, sw):
    """csrc/spmv_pb.hip, round 5: the blocked copy is filled by a two-level partition (k_pb_group: by group of column blocks
    into the wave's scratch region; k_pb_scatter: a stable counting sort per bucket, written in destination order) instead of
    k_pb_rows<true>'s 768 write streams per wave.  Same copy, bit for bit: the SpMV through either is the oracle's -- rows
    longer than a wave, empty rows, a dense row (a bucket longer than the LDS slice: straight to its place), a value
    dictionary (8-bit indices travel instead of values), sub-blocks of more rows than the LDS holds row pointers for."""
    sw("SPMV_MODE", "pb")
    rng = np.random.default_rng(23)
    if case == "rand_real":
        A = oracle.rand_rows(30000, 40, 7, base=1)
        A.val[:] = rng.standard_normal(A.nnz)
    elif case == "long_rows":
        A = _real_sparse(oracle, 2500, 0.12, 3)                   # ~300 entries per row
    elif case == "few_values":
        A = oracle.rand_rows(40000, 24, 9)                        # integer values from a set of 4 + diagonals: a value dictionary
        sw("VALUE_DICT", 1)
    elif case == "wide_sub_blocks":
        sw("PB_MIN_WAVES", 1024)                                  # 1024 sub-blocks of 2198 rows: row pointers read from L2, not LDS
        A = oracle.poisson5(1500, 1500)
        A.val[:] = rng.standard_normal(A.nnz)
    else:
        import scipy.sparse as sp
        n = 20000
        S = sp.random(n, n, density=0.0008, random_state=5, format="lil")
        S[7, :] = 1.0                                             # one dense row
        for r in (0, 5, 11, n - 1):
            S[r, :] = 0                                           # empty rows
        S = S.tocsr()
        S.data[:] = rng.standard_normal(S.nnz)
        S.sort_indices()
        A = oracle.Csr(n, S.indptr.astype(np.int32), S.indices.astype(np.int32), S.data.astype(np.float64), n)
    x = rng.standard_normal(A.n)
    d = rng.standard_normal(A.n)
    want, want_d = oracle.spmv(A, x), oracle.csrmv(A, 1.0, x, 1.0, x * d)
    for fill2 in ("1", "0"):
        sw("PB_FILL2", fill2)
        np.testing.assert_array_equal(_spmv_via_solver(cm, ctx, A, x), want)
        np.testing.assert_array_equal(_spmv_via_solver(cm, ctx, A, x, d=d), want_d)


def test_blocked_spmv_in_the_solver_loop(cm, ctx, oracle, golden_dir, sw):
    """same solves as above with the blocked kernels forced: fused dots, freeze prologue, ILU path"""
    sw("SPMV_MODE", "pb")
    A = oracle.rand_rows(20000, 50, 0x5EED)
    xs = oracle.xstar(20000, 0x5EEE)
    b = oracle.spmv(A, xs)
    xo, so, ho = oracle.pbicgstab(A, b, maxit=200, tol=1e-8, want_hist=True)
    x, st, h = _solve_dev(cm, ctx, A, b, loop=cm.LOOP_PBICGSTAB, maxit=200, tol=1e-8)
    assert st.converged and abs(st.iters - so.iters) <= 1
    np.testing.assert_allclose(x, xs, rtol=1e-7)
    np.testing.assert_allclose(h[:4], ho[:4], rtol=1e-9)
    A9 = _load(oracle, golden_dir, "mat900")
    b9 = oracle.spmv(A9, 1.0 + np.sin(np.arange(A9.n)))
    for precond in (cm.PRECOND_NONE, cm.PRECOND_ILU0):
        x1, st1, _ = _solve_dev(cm, ctx, A9, b9, precond=precond, loop=cm.LOOP_PBICGSTAB, maxit=2000, tol=1e-8)
        xo, so = oracle.pbicgstab(A9, b9, vm=oracle.ilu0(A9) if precond else None, maxit=2000, tol=1e-8)
        assert st1.converged and abs(st1.iters - so.iters) <= max(2, 0.1 * so.iters)
        assert np.linalg.norm(x1 - xo) / np.linalg.norm(xo) <= 1e-5


# ------------------------------------------------------------------- degenerate inputs
def test_degenerate_systems(cm, ctx, oracle):
    """1x1, diagonal, empty rows, zero right-hand side, exact initial guess, argument errors"""
    # 1 x 1
    A1 = oracle.Csr(1, np.array([1, 2], np.int32), np.array([1], np.int32), np.array([4.0]), 1)
    # gpu_pbicgstab (half-step exit, pbicgstab.cu:116) stops at the exact answer after half an iteration
    x, st, h = _solve_dev(cm, ctx, A1, np.array([2.0]), loop=cm.LOOP_PBICGSTAB, maxit=10, tol=1e-10)
    assert st.converged and st.half_exit and st.iters == 0 and abs(x[0] - 0.5) < 1e-15
    # gpu_pbicgstab2 has no half-step test: s = 0 => omega = 0/0 => NaN guard (:735), like the oracle
    ok, x, dt, st = cm.bicgstab(1, 1, A1.val, A1.rowptr, A1.colidx, np.array([2.0]), 10, 1e-10)
    oko, xo, so = oracle.pbicgstab2(A1, np.array([2.0]), maxit=10, tol=1e-10)
    assert ok == oko == False and st.breakdown == so.breakdown == 1 and st.iters == so.iters  # noqa: E712
    # diagonal matrix, base 0: converges in one iteration
    n = 1000
    dg = 1.0 + np.arange(n) % 7
    rp, ci = np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32)
    b = dg * (1.0 + np.arange(n) % 3)
    ok, x, dt, st = cm.bicgstab(n, n, dg, rp, ci, b, 50, 1e-12)
    assert ok and np.allclose(x, b / dg, rtol=1e-10)
    ok, x, dt, st = cm.bicgstab_lu_precond(n, n, dg, rp, ci, b, 50, 1e-12)
    assert st.converged and st.iters <= 1 and np.allclose(x, b / dg, rtol=1e-12)
    # x0 already solves the system: r0 = 0, tol*||r0|| = 0, rho = 0 -> the reference's loop divides 0/0 and runs to
    # maxit with NaNs (pbicgstab.cu:81,107 have no guard; the oracle restates that).  Deliberate difference
    # (DESIGN.md section 1): here the loop starts frozen, x0 comes back untouched and the solve reports convergence
    A = oracle.poisson5(20, 20)
    b1 = oracle.spmv(A, np.ones(A.n))
    xo, so = oracle.pbicgstab(A, b1, maxit=7, tol=1e-8)
    assert not so.converged and not np.isfinite(xo).all()              # what upstream does
    for lp in (cm.LOOP_PBICGSTAB, cm.LOOP_PBICGSTAB2):
        x, st, h = _solve_dev(cm, ctx, A, b1, loop=lp, maxit=7, tol=1e-8)
        assert st.iters == 0 and st.converged and not st.breakdown and st.nrm0 == 0.0
        np.testing.assert_array_equal(x, np.ones(A.n))
    # rows without entries (singular, but SpMV and the loop must not misbehave)
    E = oracle.Csr(4, np.array([0, 1, 1, 2, 2], np.int32), np.array([0, 2], np.int32), np.array([2.0, 3.0]), 4)
    s = cm.Solver.from_host_csr(ctx, E.rowptr, E.colidx, E.val)
    dx, dy = ctx.array(np.array([1.0, 2.0, 3.0, 4.0])), ctx.empty(4)
    s.spmv(dx, dy)
    np.testing.assert_array_equal(dy.download(), [2.0, 0.0, 9.0, 0.0])
    s.close()
    # a matrix with no entries at all
    Z = cm.Solver.from_host_csr(ctx, np.zeros(6, np.int32), np.zeros(0, np.int32), np.zeros(0))
    dz = ctx.array(np.ones(5))
    do = ctx.array(np.ones(5))
    Z.spmv(dz, do)
    np.testing.assert_array_equal(do.download(), np.zeros(5))
    Z.close()
    # argument errors come back as codes, never as exit()
    with pytest.raises(cm.CudamatError) as e:
        cm.bicgstab(3, 5, np.ones(5), np.array([1, 2, 3, 4], np.int32), np.ones(5, np.int32), np.ones(3), 10, 1e-8)
    assert e.value.code == 2          # nnz != iA[n] - iA[0]
    with pytest.raises(cm.CudamatError) as e:
        cm.bicgstab(2, 2, np.ones(2), np.array([5, 6, 7], np.int32), np.ones(2, np.int32), np.ones(2), 10, 1e-8)
    assert e.value.code == 2          # index base must be 0 or 1


# ------------------------------------------------- randomized shapes through every SpMV form
@pytest.mark.parametrize("seed", range(12))
def test_spmv_random_shapes_all_forms(cm, ctx, oracle, seed, sw):
    """random rectangular-free CSR shapes (ragged rows, empty rows, 0/1 base) through the lanes-per-row,
    the LDS-staged stream and the blocked two-phase kernels: integer data => all bit-exact vs the oracle"""
    import scipy.sparse as sp
    rng = np.random.default_rng(1000 + seed)
    n = int(rng.integers(1, 6000))
    density = float(rng.choice([0.0005, 0.003, 0.02, 0.2])) if n > 50 else 0.5
    S = sp.random(n, n, density=density, random_state=seed, format="csr")
    S.data[:] = rng.integers(-4, 5, S.nnz)
    S.eliminate_zeros()
    S.sort_indices()
    base = int(rng.integers(0, 2))
    A = oracle.Csr(n, (S.indptr + base).astype(np.int32), (S.indices + base).astype(np.int32),
                   S.data.astype(np.float64), n)
    x = rng.integers(-8, 9, n).astype(np.float64)
    d = rng.integers(-2, 3, n).astype(np.float64)
    want = oracle.spmv(A, x)
    want_d = oracle.csrmv(A, 1.0, x, 1.0, x * d)
    for mode in ("csr", "pb", "sell"):
        sw("SPMV_MODE", mode)
        np.testing.assert_array_equal(_spmv_via_solver(cm, ctx, A, x), want)
        np.testing.assert_array_equal(_spmv_via_solver(cm, ctx, A, x, d=d), want_d)
    sw("SPMV_MODE", None)
    for lanes in ("4", "32"):
        sw("SPMV_LANES", lanes)     # forces the lanes-per-row kernel (no stream tiles)
        np.testing.assert_array_equal(_spmv_via_solver(cm, ctx, A, x), want)


@pytest.mark.parametrize("name", ["rand20000x50", "real3000", "mat10000"])
def test_hybrid_triangular_solve_vs_oracle(cm, ctx, oracle, golden_dir, name, sw):
    """the group-split triangular solve (far entries through the blocked SpMV, near entries through the
    level kernels; csrc/ilu.hip split_factor) forced on small systems: same L^-1 U^-1 as the oracle"""
    sw("TRSV_HYBRID", "1")
    if name == "rand20000x50":
        A = oracle.rand_rows(20000, 50, 0x5EED)
    elif name == "real3000":
        A = _real_sparse(oracle, 3000, 0.004, 11, base=1)
    else:
        A = _load(oracle, golden_dir, name)
    s = cm.Solver.from_host_csr(ctx, A.rowptr, A.colidx, A.val)
    s.ilu0()
    want = oracle.ilu0(A)
    np.testing.assert_allclose(s.ilu0_values(), want, rtol=1e-12, atol=1e-14)
    rng = np.random.default_rng(0)
    for rep in range(2):                       # twice: the far buffer and the product stream are reused
        rhs = rng.standard_normal(A.n)
        dr, do = ctx.array(rhs), ctx.empty(A.n)
        s.precond_apply(dr, do)
        ref = oracle.trsv_upper(A, want, oracle.trsv_lower_unit(A, want, rhs))
        np.testing.assert_allclose(do.download(), ref, rtol=1e-10, atol=1e-12)
    s.close()
    xs = 1.0 + np.sin(np.arange(A.n))
    b = oracle.spmv(A, xs)
    xo, so = oracle.pbicgstab(A, b, vm=want, maxit=500, tol=1e-8)
    x, st, h = _solve_dev(cm, ctx, A, b, precond=cm.PRECOND_ILU0, loop=cm.LOOP_PBICGSTAB, maxit=500, tol=1e-8)
    assert st.converged and abs(st.iters - so.iters) <= max(2, 0.1 * so.iters)
    assert np.linalg.norm(x - xo) / np.linalg.norm(xo) <= 1e-5


@pytest.mark.parametrize("name", ["rand20000x50", "real3000", "mat10000"])
def test_loop_in_level_major_spaces_matches_the_permuting_loop(cm, ctx, oracle, golden_dir, name, sw):
    """hybrid factors live in level-major index spaces; the reference loop then runs with its residual-side vectors in
    L's order, its solution-side vectors in U's, and A stored with rows in L's order and columns in U's positions (no
    vector is permuted inside the loop).  Same mathematics as the loop that permutes around every M^-1 application
    (CUDAMAT_TRSV_PERM=0): same iteration count (+-1: the dot products are summed in another order), solutions equal to
    1e-9, histories to 1e-8 over the first iterations; both agree with the oracle (solution 1e-5, count +-10 %)."""
    sw("TRSV_HYBRID", "1")
    if name == "rand20000x50":
        A = oracle.rand_rows(20000, 50, 0x5EED)
    elif name == "real3000":
        A = _real_sparse(oracle, 3000, 0.004, 11, base=1)
    else:
        A = _load(oracle, golden_dir, name)
    xs = 1.0 + np.sin(np.arange(A.n))
    b = oracle.spmv(A, xs)
    x0 = 1.0 + 0.25 * np.cos(np.arange(A.n))
    xo, so, ho = oracle.pbicgstab(A, b, x0=x0, vm=oracle.ilu0(A), maxit=500, tol=1e-8, want_hist=True)
    res = {}
    for perm in ("1", "0"):
        sw("TRSV_PERM", perm)
        res[perm] = _solve_dev(cm, ctx, A, b, x0=x0, precond=cm.PRECOND_ILU0, loop=cm.LOOP_PBICGSTAB, maxit=500, tol=1e-8)
    (x1, st1, h1), (x0_, st0, h0) = res["1"], res["0"]
    assert st1.converged and st0.converged and abs(st1.iters - st0.iters) <= 1
    assert np.linalg.norm(x1 - x0_) / np.linalg.norm(x0_) <= 1e-9
    k = min(len(h1), len(h0), 6)
    np.testing.assert_allclose(h1[:k], h0[:k], rtol=1e-8)
    np.testing.assert_allclose(h1[:k], ho[:k], rtol=1e-8)
    assert abs(st1.iters - so.iters) <= max(2, 0.1 * so.iters)
    assert np.linalg.norm(x1 - xo) / np.linalg.norm(xo) <= 1e-5
    assert np.linalg.norm(b - oracle.spmv(A, x1)) <= 1e-7 * st1.nrm0
    # the pipelined loop on the same level-major factors (it permutes around every application of M^-1)
    xp, sp, hp = oracle.pipelined_bicgstab(A, b, x0=x0, vm=oracle.ilu0(A), maxit=500, tol=1e-8, want_hist=True)
    x2, st2, h2 = _solve_dev(cm, ctx, A, b, x0=x0, precond=cm.PRECOND_ILU0, loop=cm.LOOP_PIPELINED, maxit=500, tol=1e-8)
    assert st2.converged and st2.restarts == 0 and abs(st2.iters - sp.iters) <= max(2, 0.1 * sp.iters)
    assert np.linalg.norm(x2 - xp) / np.linalg.norm(xp) <= 1e-6 and np.linalg.norm(x2 - x1) / np.linalg.norm(x1) <= 1e-5


def _chain_matrix(oracle, n, width, seed):
    """banded lower+upper coupling: row i depends on rows i-1 .. i-width -> n levels of one row each"""
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    diags = [rng.integers(1, 4, n - k).astype(np.float64) * 0.25 for k in range(1, width + 1)]
    S = sp.diags(diags, [-k for k in range(1, width + 1)]) + sp.diags(diags, list(range(1, width + 1)))
    S = (S + sp.diags(np.full(n, 2.0 * width + 1.0))).tocsr()
    S.sort_indices()
    return oracle.Csr(n, S.indptr.astype(np.int32), S.indices.astype(np.int32), S.data.copy(), n)


@pytest.mark.parametrize("name, lanes", [
    pytest.param(name, None, id=name)
    for name in ("chain3000", "poisson160x90", "rand20000x50", "rand20000x50_hybrid", "longrows", "mat10000")
] + [
    pytest.param("poisson160x90", 2, id="poisson160x90-lanes2"),
    pytest.param("longrows", 64, id="longrows-lanes64"),
    pytest.param("wide", None, id="wide"),
])
def test_dependency_driven_trsv_equals_level_solve(cm, ctx, oracle, golden_dir, name, lanes, sw):
    """k_trsv_syncfree (one launch per group, rows wait for their dependencies' values) against the
    level-by-level kernels (the K = 1 instantiations of k_trsm_level / k_trsm_small_levels / k_trsm_lds) on the same
    factors: every row is summed by the same lanes in the same order,
    so L^-1 U^-1 must be BIT-identical -- deep chains inside one wavefront (chain3000: every row waits for
    the previous one), wavefront-shaped levels (Poisson), scattered rows, the hybrid far/near split, the lane
    counts at both ends pinned with TRSV_LANES (2 on Poisson, 64 on the 60 % dense rows, whatever the row-length rule
    picks), and levels of 3000 rows ("wide": k_trsm_level<L, 1> on several workgroups, then a run of narrow levels)."""
    if lanes:
        sw("TRSV_LANES", str(lanes))
    if name == "chain3000":
        A = _chain_matrix(oracle, 3000, 2, 3)
    elif name == "poisson160x90":
        A = oracle.poisson5(160, 90)
    elif name.startswith("rand20000x50"):
        A = oracle.rand_rows(20000, 50, 0x5EED)
    elif name == "longrows":
        A = _real_sparse(oracle, 400, 0.6, 5)
    elif name == "wide":
        from tests.test_gpu_many_precond import _wide_levels
        A = _wide_levels(oracle)
    else:
        A = _load(oracle, golden_dir, name)
    sw("TRSV_HYBRID", "1" if name.endswith("hybrid") else "0")
    if name.endswith("hybrid"):
        sw("TRSV_GROUPS", "5")
    rng = np.random.default_rng(4)
    rhs = [rng.standard_normal(A.n) for _ in range(3)]
    got = {}
    for form in ("0", "1"):
        sw("TRSV_SYNCFREE", form)
        s = cm.Solver.from_host_csr(ctx, A.rowptr, A.colidx, A.val)
        s.ilu0()
        outs = []
        for b in rhs:
            dr, do = ctx.array(b), ctx.empty(A.n)
            s.precond_apply(dr, do)
            outs.append(do.download())
        got[form] = outs
        if form == "1":       # and through the solver loop, where a timed-out wait would be reported
            xs = 1.0 + np.sin(np.arange(A.n))
            st = s.solve(ctx.array(oracle.spmv(A, xs)), ctx.empty(A.n), precond=cm.PRECOND_ILU0, maxit=50, tol=1e-8,
                         flags=cm.FLAG_X0_ONES)
            assert st.converged
        s.close()
    for a, b in zip(got["0"], got["1"]):
        assert np.isfinite(b).all()
        np.testing.assert_array_equal(a, b)
    want = oracle.ilu0(A)
    ref = oracle.trsv_upper(A, want, oracle.trsv_lower_unit(A, want, rhs[0]))
    np.testing.assert_allclose(got["1"][0], ref, rtol=1e-10, atol=1e-12)


def test_spmv_skewed_rows(cm, ctx, oracle, sw):
    """a few rows with tens of thousands of entries among short ones: the lanes-per-row
    kernel hands them to the whole workgroup; results stay exact, the fused dots stay right"""
    import scipy.sparse as sp
    rng = np.random.default_rng(21)
    n = 70000
    ri = np.repeat(np.arange(n), 8)
    cj = rng.integers(0, n, ri.size)
    for r in (3, 4, 5000, 69999):                  # two adjacent long rows, one mid, the last row
        cols = rng.choice(n, size=30000 if r != 4 else 5000, replace=False)
        ri = np.concatenate([ri, np.full(cols.size, r)])
        cj = np.concatenate([cj, cols])
    S = sp.csr_matrix((np.ones(ri.size), (ri, cj)), shape=(n, n))
    S.sum_duplicates()
    S.data[:] = rng.integers(1, 4, S.nnz)
    S.sort_indices()
    A = oracle.Csr(n, S.indptr.astype(np.int32), S.indices.astype(np.int32), S.data.astype(np.float64), n)
    x = rng.integers(-3, 4, n).astype(np.float64)
    want = oracle.spmv(A, x)
    rp, ci, v = _dev_csr(ctx, A)
    dx, dy = ctx.array(x), ctx.empty(n)
    for lanes in (None, "4", "64"):
        if lanes:
            sw("SPMV_LANES", lanes)
        dy.zero()
        ctx.spmv(n, rp, ci, v, 0, dx, dy)
        np.testing.assert_array_equal(dy.download(), want)
    sw("SPMV_LANES", None)
    for mode in ("csr", "pb"):
        sw("SPMV_MODE", mode)
        np.testing.assert_array_equal(_spmv_via_solver(cm, ctx, A, x), want)
    # inside a solve (fused dot partials include the long rows): make the system dominant and solve it
    sw("SPMV_MODE", "csr")
    S2 = (S + sp.diags(np.asarray(abs(S).sum(axis=1)).ravel() + 1.0)).tocsr()
    S2.sort_indices()
    A2 = oracle.Csr(n, S2.indptr.astype(np.int32), S2.indices.astype(np.int32), S2.data.astype(np.float64), n)
    xs = oracle.xstar(n, 5)
    b = oracle.spmv(A2, xs)
    xg, st, h = _solve_dev(cm, ctx, A2, b, loop=cm.LOOP_PBICGSTAB, maxit=200, tol=1e-10)
    xo, so = oracle.pbicgstab(A2, b, maxit=200, tol=1e-10)
    # (diagonals of 6e4 next to 17: erratic BiCGSTAB convergence, histories agree to 1e-9 for five
    #  iterations and then drift with the rounding order of the 30000-term dots -- both converge)
    assert st.converged and so.converged and abs(st.iters - so.iters) <= max(3, 0.3 * so.iters)
    np.testing.assert_allclose(h[:8], oracle.pbicgstab(A2, b, maxit=4, tol=1e-30, want_hist=True)[2][:8], rtol=1e-7)
    np.testing.assert_allclose(xg, xs, rtol=1e-6)


def test_trsv_timeout_redoes_the_solve_with_level_kernels(cm, ctx, oracle, sw):
    """a dependency-driven triangular solve whose wait times out (here: an absurdly small spin limit on a matrix
    whose rows form one long chain) must not produce an answer: the solve is redone from x0 with the
    level-by-level kernels, which then stay selected; results equal the level-only run bit for bit"""
    A = _chain_matrix(oracle, 6000, 2, 7)
    xs = 1.0 + np.cos(np.arange(A.n))
    b = oracle.spmv(A, xs)
    x0 = np.full(A.n, 0.5)
    res = {}
    for form, limit in (("0", None), ("1", "1")):
        sw("TRSV_SYNCFREE", form)
        if limit:
            sw("TRSV_SPIN_LIMIT", limit)
        s = cm.Solver.from_host_csr(ctx, A.rowptr, A.colidx, A.val)
        s.ilu0()
        assert s.trsv_form() == int(form)
        db, dx = ctx.array(b), ctx.array(x0)
        st = s.solve(db, dx, precond=cm.PRECOND_ILU0, maxit=100, tol=1e-10)       # caller's x0 (no X0_ONES flag)
        res[form] = (dx.download(), st.iters, st.converged, s.trsv_form(), st.trsv_fallbacks, st.trsv_form)
        s.close()
    sw("TRSV_SPIN_LIMIT", None)
    assert res["1"][3] == 0, "the timeout should have switched the solver to the level kernels"
    # the redo is reported, not hidden: one fallback, and the stats name the form the solve ended with
    assert res["0"][4] == 0 and res["1"][4] == 1
    assert res["0"][5] == res["1"][5] and res["1"][5] in (0, 2)      # (2: single-workgroup LDS form, n <= 16384)
    assert res["0"][2] and res["1"][2] and res["0"][1] == res["1"][1]
    np.testing.assert_array_equal(res["0"][0], res["1"][0])
    np.testing.assert_allclose(res["1"][0], xs, atol=1e-7)


def _skewed_matrix(oracle, kind, rng):
    """integer-valued CSR with a nasty row-length distribution"""
    import scipy.sparse as sp
    if kind == "pareto":
        n = 150000
        lens = np.minimum(1 + (rng.pareto(1.3, n) * 4).astype(np.int64), 60000)
    elif kind == "hubs":                       # rows of 8 + a few rows spanning tens of 2048-entry tiles
        n = 120000
        lens = np.full(n, 8, np.int64)
        lens[[0, 1, 777, 60000, n - 2, n - 1]] = [50000, 4097, 2048, 100000, 2049, 30000]
    elif kind == "empties":                    # runs of empty rows, also first / last, around tile boundaries
        n = 90000
        lens = rng.integers(0, 3, n).astype(np.int64) * rng.integers(0, 2, n)
        lens[:300] = 0
        lens[-500:] = 0
        lens[40000:41000] = 0
        lens[5000] = 7000
    else:                                      # "mixed": a 1500-entry row among one-entry rows inside one tile
        n = 70000
        lens = np.ones(n, np.int64)
        lens[::997] = 1500
        lens[::13] = 40
    rp = np.zeros(n + 1, np.int64)
    np.cumsum(lens, out=rp[1:])
    nnz = int(rp[-1])
    rows = np.repeat(np.arange(n), lens)
    cols = rng.integers(0, n, nnz)
    S = sp.csr_matrix((np.ones(nnz), (rows, cols)), shape=(n, n))
    S.sum_duplicates()
    S.sort_indices()
    S.data[:] = rng.integers(1, 5, S.nnz)
    return oracle.Csr(n, S.indptr.astype(np.int32), S.indices.astype(np.int32), S.data.astype(np.float64), n)


@pytest.mark.parametrize("kind", ["pareto", "hubs", "empties", "mixed"])
def test_spmv_nnz_balanced_tiles(cm, ctx, oracle, kind, sw):
    """k_spmv_tiles / k_spmv_tiles_fix (tiles of 2048 ENTRIES; rows spanning tiles finished from head / tail
    partials): exact on integer data for every row-length pathology -- standalone entry point with alpha, beta
    and the diagonal term, solver entry point, base 0 and 1, auto-selected and forced"""
    rng = np.random.default_rng({"pareto": 1, "hubs": 2, "empties": 3, "mixed": 4}[kind])
    A = _skewed_matrix(oracle, kind, rng)
    n = A.n
    x = rng.integers(-3, 4, n).astype(np.float64)
    y0 = rng.integers(-2, 3, n).astype(np.float64)
    d = rng.integers(-2, 3, n).astype(np.float64)
    want = oracle.spmv(A, x)
    want_full = oracle.csrmv(A, 2.0, x, -1.0, y0.copy() * 1.0)          # y = 2 A x - y0
    for form in (None, "tiles", "lanes"):
        if form:
            sw("SPMV_FORM", form)
        for base in (0, 1):
            rp, ci, v = ctx.array((A.rowptr + base).astype(np.int32)), ctx.array((A.colidx + base).astype(np.int32)), ctx.array(A.val)
            dx, dy = ctx.array(x), ctx.array(y0)
            ctx.spmv(n, rp, ci, v, base, dx, dy, alpha=2.0, beta=-1.0)
            np.testing.assert_array_equal(dy.download(), want_full)
            dy.zero()
            ctx.spmv(n, rp, ci, v, base, dx, dy, d=ctx.array(d))
            np.testing.assert_array_equal(dy.download(), want + d * x)
        sw("SPMV_MODE", "csr")
        np.testing.assert_array_equal(_spmv_via_solver(cm, ctx, A, x), want)
        sw("SPMV_MODE", None)
    sw("SPMV_FORM", None)


def test_solve_with_tile_spmv(cm, ctx, oracle, sw):
    """the fused dot partials of the tile kernels (main launch + the launch that finishes spanning rows) inside
    the BiCGSTAB loop: same iterates as the oracle"""
    import scipy.sparse as sp
    rng = np.random.default_rng(12)
    A = _skewed_matrix(oracle, "hubs", rng)
    S = sp.csr_matrix((A.val, A.colidx, A.rowptr), shape=(A.n, A.n))
    S = (S + sp.diags(np.asarray(abs(S).sum(axis=1)).ravel() + 1.0)).tocsr()
    S.sort_indices()
    A2 = oracle.Csr(A.n, S.indptr.astype(np.int32), S.indices.astype(np.int32), S.data.astype(np.float64), A.n)
    xs = oracle.xstar(A.n, 5)
    b = oracle.spmv(A2, xs)
    sw("SPMV_MODE", "csr")
    sw("SPMV_FORM", "tiles")
    xg, st, h = _solve_dev(cm, ctx, A2, b, loop=cm.LOOP_PBICGSTAB, maxit=200, tol=1e-10)
    xo, so, ho = oracle.pbicgstab(A2, b, maxit=200, tol=1e-10, want_hist=True)
    assert st.converged and so.converged and abs(st.iters - so.iters) <= max(3, 0.3 * so.iters)
    np.testing.assert_allclose(h[:6], ho[:6], rtol=1e-7)
    np.testing.assert_allclose(xg, xs, rtol=1e-6)


def test_solver_validates_its_csr(cm, ctx, oracle, sw):
    """malformed inputs become CUDAMAT_ERR_ARG at creation (never a stray device access); rows with unsorted
    columns are accepted by the un-preconditioned path and refused by ILU(0) and by the blocked SpMV"""
    A = oracle.rand_rows(5000, 12, 3)
    n = A.n
    bad_rp = A.rowptr.copy()
    bad_rp[100] = bad_rp[101] + 5                       # decreasing
    with pytest.raises(cm.CudamatError) as e:
        cm.Solver.from_host_csr(ctx, bad_rp, A.colidx, A.val)
    assert e.value.code == 2
    for bad in (n, -1, 2 ** 30):
        ci = A.colidx.copy()
        ci[12345] = bad
        with pytest.raises(cm.CudamatError) as e:
            cm.Solver.from_host_csr(ctx, A.rowptr, ci, A.val)
        assert e.value.code == 2
    # unsorted row (swap two entries of row 7): SpMV still right, ILU(0) and the blocked form refuse
    ci, v = A.colidx.copy(), A.val.copy()
    k = A.rowptr[7]
    ci[[k, k + 3]] = ci[[k + 3, k]]
    v[[k, k + 3]] = v[[k + 3, k]]
    x = np.arange(n, dtype=np.float64) % 7 - 3
    s = cm.Solver.from_host_csr(ctx, A.rowptr, ci, v)
    dx, dy = ctx.array(x), ctx.empty(n)
    s.spmv(dx, dy)
    np.testing.assert_array_equal(dy.download(), oracle.spmv(A, x))
    with pytest.raises(cm.CudamatError) as e:
        s.ilu0()
    assert e.value.code == 2
    s.close()
    sw("SPMV_MODE", "pb")
    s = cm.Solver.from_host_csr(ctx, A.rowptr, ci, v)
    with pytest.raises(cm.CudamatError) as e:
        s.spmv(dx, dy)
    assert e.value.code == 2
    s.close()


@pytest.mark.parametrize("name", ["mat10000", "rand20000x50", "longrows"])
def test_ilu0_prefetching_kernel_equals_simple_kernel(cm, ctx, oracle, golden_dir, name, sw):
    """k_ilu0_level_fast (columns, pivot table and next pivot row staged / prefetched) performs the same
    updates in the same order as k_ilu0_level_simple: bit-identical factors; both within 1e-12 of the oracle"""
    if name == "rand20000x50":
        A = oracle.rand_rows(20000, 50, 0x5EED)
    elif name == "longrows":
        A = _real_sparse(oracle, 400, 0.6, 5)
    else:
        A = _load(oracle, golden_dir, name)
    got = []
    for simple in ("0", "1"):
        sw("ILU0_SIMPLE", simple)
        s = cm.Solver.from_host_csr(ctx, A.rowptr, A.colidx, A.val)
        s.ilu0()
        got.append(s.ilu0_values())
        s.close()
    np.testing.assert_array_equal(got[0], got[1])
    np.testing.assert_allclose(got[0], oracle.ilu0(A), rtol=1e-12, atol=1e-14)


@pytest.mark.parametrize("name", ["mat900", "mat10000", "chain3000", "longrows", "rand9000x30"])
def test_lds_resident_trsv_equals_level_kernels(cm, ctx, oracle, golden_dir, name, sw):
    """k_trsm_lds<L, 1> (n <= 16384: one workgroup, solution vector in LDS, next level's operands prefetched across the
    barrier) against the level kernels (k_trsm_level / k_trsm_small_levels at K = 1) with the vector in global memory: bit-identical L^-1 U^-1, and both within
    1e-10 of the oracle's substitutions"""
    if name == "chain3000":
        A = _chain_matrix(oracle, 3000, 2, 3)
    elif name == "longrows":
        A = _real_sparse(oracle, 400, 0.6, 5)
    elif name == "rand9000x30":
        A = oracle.rand_rows(9000, 30, 77)          # levels of ~100-300 rows: several rows per team and level
    else:
        A = _load(oracle, golden_dir, name)
    sw("TRSV_SYNCFREE", "0")
    rng = np.random.default_rng(8)
    rhs = [rng.standard_normal(A.n) for _ in range(2)]
    got = {}
    for lds in ("0", "1"):
        sw("TRSV_LDS", lds)
        s = cm.Solver.from_host_csr(ctx, A.rowptr, A.colidx, A.val)
        s.ilu0()
        outs = []
        for b in rhs:
            dr, do = ctx.array(b), ctx.empty(A.n)
            s.precond_apply(dr, do)
            outs.append(do.download())
        got[lds] = outs
        s.close()
    for a, b in zip(got["0"], got["1"]):
        np.testing.assert_array_equal(a, b)
    want = oracle.ilu0(A)
    ref = oracle.trsv_upper(A, want, oracle.trsv_lower_unit(A, want, rhs[0]))
    np.testing.assert_allclose(got["1"][0], ref, rtol=1e-10, atol=1e-12)


@pytest.mark.parametrize("case", ["poisson300x210", "banded_ragged", "too_wide", "long_row_255", "base1"])
def test_stream_spmv_with_compressed_indices(cm, ctx, oracle, case, sw):
    """k_spmv_stream_c (16-bit column offsets from the tile's first row, 8-bit row lengths) = k_spmv_stream bit for
    bit, and exact against the oracle on integer data; matrices whose offsets do not fit keep the plain kernel"""
    import scipy.sparse as sp
    rng = np.random.default_rng(31)
    base = 0
    if case == "poisson300x210":
        A = oracle.poisson5(300, 210)
    else:
        n = 40000
        if case == "banded_ragged":          # 0..9 entries per row (empty rows too) within +-3000 of the diagonal
            lens = rng.integers(0, 10, n)
            width = 3000
        elif case == "too_wide":             # short rows, columns anywhere: offsets do not fit 16 bits
            lens = rng.integers(1, 8, n)
            width = n
        elif case == "long_row_255":         # one row of exactly 255 entries among rows of 3
            lens = np.full(n, 3)
            lens[777] = 255
            width = 2000
        else:
            lens = rng.integers(1, 6, n)
            width = 500
            base = 1
        rows = np.repeat(np.arange(n), lens)
        cols = np.clip(rows + rng.integers(-width, width + 1, rows.size), 0, n - 1)
        S = sp.csr_matrix((np.ones(rows.size), (rows, cols)), shape=(n, n))
        S.sum_duplicates()
        S.sort_indices()
        S.data[:] = rng.integers(-3, 4, S.nnz)
        A = oracle.Csr(n, (S.indptr + base).astype(np.int32), (S.indices + base).astype(np.int32),
                       S.data.astype(np.float64), n)
    x = rng.integers(-4, 5, A.n).astype(np.float64)
    d = rng.integers(-2, 3, A.n).astype(np.float64)
    want = oracle.spmv(A, x)
    got = {}
    # plain stream kernel; compressed indices + value dictionary (k_spmv_stream_d); compressed indices on the fp64 values
    # with the line-aligned copies of the two entry streams (k_spmv_stream_c, plan_spmv_align) and with the packed arrays
    for comp, vdict, align in (("0", "1", "1"), ("1", "1", "1"), ("1", "0", "1"), ("1", "0", "0")):
        sw("SPMV_COMPRESS", comp)
        sw("VALUE_DICT", vdict)
        sw("SPMV_ALIGN", align)
        sw("SPMV_MODE", "csr")
        got[comp + vdict + align] = (_spmv_via_solver(cm, ctx, A, x), _spmv_via_solver(cm, ctx, A, x, d=d))
    sw("VALUE_DICT", None)
    sw("SPMV_ALIGN", None)
    for comp in got:
        np.testing.assert_array_equal(got[comp][0], want)
        np.testing.assert_array_equal(got[comp][1], want + d * x)
    # inside a solve (fused dots): identical histories with and without the compressed copy
    if case == "poisson300x210":
        b = oracle.spmv(A, 1.0 + np.sin(np.arange(A.n)))
        hist = []
        for comp in ("0", "1"):
            sw("SPMV_COMPRESS", comp)
            xg, st, h = _solve_dev(cm, ctx, A, b, loop=cm.LOOP_PBICGSTAB, maxit=400, tol=1e-8)
            assert st.converged
            hist.append((xg, h))
        np.testing.assert_array_equal(hist[0][0], hist[1][0])
        np.testing.assert_array_equal(hist[0][1], hist[1][1])


@pytest.mark.parametrize("n,longest", [(3000, 1300), (3000, 2500)])
def test_ilu0_very_long_rows(cm, ctx, oracle, n, longest):
    """a maximum row length above 1024 entries selects k_ilu0_level_simple<4> (LDS slice per wave), above 2048 the
    one-wave-per-workgroup launch; factors and L^-1 U^-1 against the oracle.  (A few dense rows among sparse
    ones keep the oracle's O(sum len^2) factorisation cheap.)"""
    import scipy.sparse as sp
    rng = np.random.default_rng(17)
    S = sp.random(n, n, 0.003, random_state=5, format="lil")
    for r in (n - 1, n - 7, n // 2):
        cols = rng.choice(n, size=longest, replace=False)
        S[r, cols] = rng.uniform(-1, 1, longest)
    S = S.tocsr()
    S.setdiag(0)
    S.eliminate_zeros()
    S = (S + sp.diags(1.0 + np.asarray(abs(S).sum(axis=1)).ravel())).tocsr()
    S.sort_indices()
    A = oracle.Csr(n, S.indptr.astype(np.int32), S.indices.astype(np.int32), S.data.copy(), n)
    assert np.diff(A.rowptr).max() > (1024 if longest < 2048 else 2048)
    s = cm.Solver.from_host_csr(ctx, A.rowptr, A.colidx, A.val)
    s.ilu0()
    want = oracle.ilu0(A)
    np.testing.assert_allclose(s.ilu0_values(), want, rtol=1e-11, atol=1e-13)
    rhs = rng.standard_normal(n)
    dr, do = ctx.array(rhs), ctx.empty(n)
    s.precond_apply(dr, do)
    ref = oracle.trsv_upper(A, want, oracle.trsv_lower_unit(A, want, rhs))
    np.testing.assert_allclose(do.download(), ref, rtol=1e-9, atol=1e-11)
    s.close()


@pytest.mark.parametrize("name", ["mat900", "mat10000", "rand3000x40", "tiny5"])
@pytest.mark.parametrize("loop", ["pbicgstab", "pbicgstab2_d"])
def test_fused_small_system_loop_equals_five_launch_loop(cm, ctx, oracle, golden_dir, name, loop, sw):
    """three launches per iteration (vector updates folded into the SpMVs, csrc/small_loops.hip) against
    the five-launch loop: same expressions element by element, only ||s||^2 is summed per SpMV workgroup instead of
    per vector chunk; both forms (stream tiles / lanes per row), both loops, with and without the diagonal shift"""
    if name == "rand3000x40":
        A = oracle.rand_rows(3000, 40, 9)
    elif name == "tiny5":
        A = oracle.rand_rows(5, 3, 2)
    else:
        A = _load(oracle, golden_dir, name)
    rng = np.random.default_rng(3)
    xs = 1.0 + rng.random(A.n)
    d = None
    kw = dict(loop=cm.LOOP_PBICGSTAB, maxit=400, tol=1e-9)
    if loop == "pbicgstab2_d":
        d = 0.5 + rng.random(A.n)
        kw = dict(loop=cm.LOOP_PBICGSTAB2, maxit=400, tol=1e-9)
    b = oracle.spmv(A, xs) + (d * xs if d is not None else 0.0)
    res = {}
    sw("RESIDENT", "0")      # (the single-launch form of the same loop has its own test below)
    for fused in ("0", "1000000"):
        sw("FUSED", fused)
        sw("SPMV_MODE", "csr")
        x, st, h = _solve_dev(cm, ctx, A, b, d=d, **kw)
        res[fused] = (x, st, h)
    (x0, st0, h0), (x1, st1, h1) = res["0"], res["1000000"]
    assert st0.converged and st1.converged and (st0.loop_form, st1.loop_form) == (0, 1)
    # the summation order of ||s||^2 differs in the last bit; BiCGSTAB amplifies that over hundreds of iterations,
    # so: the first 20 residuals agree to 1e-9, short solves agree throughout, long ones within 10 % of iterations
    k = min(20, len(h0), len(h1))
    np.testing.assert_allclose(h1[:k], h0[:k], rtol=1e-9)
    if st0.iters <= 40:
        assert (st0.iters, st0.half_exit) == (st1.iters, st1.half_exit)
        np.testing.assert_allclose(x1, x0, rtol=1e-10, atol=1e-12)
    else:
        assert abs(st0.iters - st1.iters) <= max(2, st0.iters // 10)
    np.testing.assert_allclose(x1, xs, rtol=1e-6)


@pytest.mark.parametrize("layout", ["aligned", "offset8"])
def test_loop_bits_single_solve(cm, ctx, sw, layout):
    """three iterations of the five-launch loop on the diagonal system of test_loop_rounding.py: x and the residual history
    equal the CPU mirror of csrc/steps.h and the kernels' reduction orders bit for bit -- with b and x 16-byte aligned (the
    pair kernels) and both 8 bytes off (k_init<0> and k_full<0>: a row per thread; k_update_p and k_half see the solver's
    own vectors and keep pairs).  The mirror tells the two-rounding p-update from the reference's three, fma dot terms from
    fl(a b) + acc and the order of the two x steps apart on these inputs (test_the_loop_mirror_tells_its_neighbours_apart)."""
    import test_loop_rounding as L
    col = {"aligned": 2, "offset8": 0}[layout]
    assert (layout, col) in L.TELLING
    a, b, x0 = L.system(col)
    for name, value in (("SPMV_MODE", "csr"), ("SPMV_LANES", L.LANES), ("FUSED", 0), ("RESIDENT", 0)):
        sw(name, value)
    off = 1 if layout == "offset8" else 0
    s = cm.Solver.from_host_csr(ctx, np.arange(L.N + 1), np.arange(L.N), a)
    db, dx = ctx.array(np.concatenate([np.zeros(off), b])), ctx.array(np.concatenate([np.zeros(off), x0]))
    st = s.solve(db.ptr + 8 * off, dx.ptr + 8 * off, loop=cm.LOOP_PBICGSTAB, maxit=L.ITERS, tol=1e-8, flags=cm.FLAG_NO_EXIT)
    x, h = dx.download()[off:], s.history()
    s.close()
    assert (st.iters, st.loop_form) == (L.ITERS, 0)
    want_x, want_h = L.pinned(layout, col)
    print(layout, "entries of x that differ:", L.differing(x, want_x), "residuals:", L.differing(h, want_h), h, want_h)
    np.testing.assert_array_equal(h, want_h)
    np.testing.assert_array_equal(x, want_x)


# ---- the other loop forms, the shifted loop, the ILU(0) loop, exits and solver reuse against the same mirror (test_loop_rounding.py:
# FORMS, inputs, pinned_form; what each comparison can tell apart is checked there, without a GPU)
_LOOP_SWITCHES = {            # SPMV_LANES, FUSED, RESIDENT
    "five/lanes": (64, 0, 0), "five/stream": (None, 0, 0), "fused/lanes": (64, 1000000, 0), "fused/stream": (None, 1000000, 0),
    "single": (None, 1000000, 1),
}
_LOOP_CASES = [("pbicgstab", False), ("pbicgstab2", False), ("pbicgstab2", True)]


def _loop_solver(cm, ctx, sw, form, A, d):
    """a solver on A (a diagonal as a vector, or test_loop_rounding.Csr) with the switches that select `form`"""
    import test_loop_rounding as L
    lanes, fused, resident = _LOOP_SWITCHES[form]
    for name, value in (("SPMV_MODE", "csr"), ("SPMV_LANES", lanes), ("FUSED", fused), ("RESIDENT", resident)):
        sw(name, value)
    if isinstance(A, L.Csr):
        s = cm.Solver.from_host_csr(ctx, A.rp, A.ci, A.val)
    else:
        s = cm.Solver.from_host_csr(ctx, np.arange(len(A) + 1), np.arange(len(A)), A)
    want = "k_spmv<64>" if lanes else "k_spmv_stream"
    assert s.spmv_kernel().startswith(want), (form, s.spmv_kernel())       # the plan whose dealing the mirror restates
    if d is not None:
        s.set_shift(ctx.array(d))
    return s


def _loop_solve(cm, ctx, s, b, x0, kind, **kw):
    db, dx = ctx.array(b), ctx.array(x0)          # 16-byte aligned: the pair kernels
    st = s.solve(db, dx, loop=cm.LOOP_PBICGSTAB if kind == "pbicgstab" else cm.LOOP_PBICGSTAB2, **kw)
    x, h = dx.download(), s.history()
    db.free()
    dx.free()
    return st, x, h


def _assert_loop_bits(tag, got, want, form, iters):
    import test_loop_rounding as L
    (st, x, h), (want_x, want_h) = got, want
    print(tag, "entries of x that differ:", L.differing(x, want_x), "of", len(x), "residuals:",
          L.differing(h, want_h) if len(h) == len(want_h) else (len(h), len(want_h)), h, want_h)
    assert (st.loop_form, st.loop_fallbacks, st.iters) == (L.FORMS[form]["loop_form"], 0, iters)
    np.testing.assert_array_equal(h, want_h)
    np.testing.assert_array_equal(x, want_x)


def _loop_bits_case(cm, ctx, sw, form, which, kind, shifted, iters):
    import test_loop_rounding as L
    A, b, x0, d = L.inputs(which, form, shifted)
    s = _loop_solver(cm, ctx, sw, form, A, d)
    got = _loop_solve(cm, ctx, s, b, x0, kind, maxit=iters, tol=1e-8, flags=cm.FLAG_NO_EXIT)
    s.close()
    _assert_loop_bits("%s %s %s%s %d:" % (form, which, kind, " shifted" if shifted else "", iters), got,
                      L.pinned_form(which, form, kind, shifted, iters), form, iters)


def test_loop_bits_fused_lanes(cm, ctx, sw):
    """three iterations of the three-launch loop on the lanes-per-row plan (k_fspmv_lanes<64, .> + k_full), diagonal system:
    x and the history equal the mirror bit for bit.  x is also the five-launch loop's by construction; the history is not
    (||s||^2 per SpMV workgroup)."""
    _loop_bits_case(cm, ctx, sw, "fused/lanes", "diagonal", "pbicgstab", False, 3)


@pytest.mark.parametrize("iters", [3, 4])
@pytest.mark.parametrize("kind,shifted", _LOOP_CASES)
@pytest.mark.parametrize("which", ["diagonal", "banded"])
def test_loop_bits_fused_stream(cm, ctx, sw, which, kind, shifted, iters):
    """the three-launch loop on stream tiles (k_fspmv_stream<256, .> + k_full): both loops, the second also as (A + I d), on
    the diagonal system (3 tiles) and the banded one (4 tiles, every workgroup gathers p' and s at rows another one stored:
    the double buffers), after an odd and an even number of buffer swaps -- x and the history equal the mirror bit for bit"""
    _loop_bits_case(cm, ctx, sw, "fused/stream", which, kind, shifted, iters)


@pytest.mark.parametrize("iters", [3, 4])
@pytest.mark.parametrize("kind,shifted", _LOOP_CASES)
@pytest.mark.parametrize("which", ["diagonal", "banded"])
def test_loop_bits_single_launch(cm, ctx, sw, which, kind, shifted, iters):
    """the same cases in the single-launch loop (k_resident_loop<256>): its hand-written dot terms, its third phase's scalar
    sums and its restated stopping-test stores give the mirror's x and history bit for bit"""
    _loop_bits_case(cm, ctx, sw, "single", which, kind, shifted, iters)


@pytest.mark.parametrize("iters", [3, 4])
@pytest.mark.parametrize("kind,shifted", _LOOP_CASES)
def test_loop_bits_five_launches_stream(cm, ctx, sw, kind, shifted, iters):
    """the five-launch loop on the stream plan, banded system (test_loop_bits_single_solve pins it on the diagonal one, lanes
    per row): column-order row sums, the tile dealing of the SpMV's dots, the shift in r0 and in every product"""
    _loop_bits_case(cm, ctx, sw, "five/stream", "banded", kind, shifted, iters)


def test_loop_bits_ilu0(cm, ctx, sw):
    """three iterations of the ILU(0) loop on the diagonal system (L = I, U = diag(a)): the factors are a itself, one
    application is rhs fl(1 / a_i) bitwise (tri_rows on empty rows), and x += alpha M^-1 p, then x += omega M^-1 r in k_full give
    the mirror's x and history bit for bit"""
    import test_loop_rounding as L
    a, b, x0, _ = L.inputs("diagonal", "five/lanes")
    s = _loop_solver(cm, ctx, sw, "five/lanes", a, None)
    s.ilu0()
    np.testing.assert_array_equal(s.ilu0_values(), a)
    dr, do = ctx.array(b), ctx.empty(L.N)
    s.precond_apply(dr, do)
    np.testing.assert_array_equal(do.download(), b * (1.0 / a))
    assert L.differing(b * (1.0 / a), b / a) >= L.MIN_DIFFERING_ROWS
    got = _loop_solve(cm, ctx, s, b, x0, "pbicgstab", precond=cm.PRECOND_ILU0, maxit=L.ITERS, tol=1e-8, flags=cm.FLAG_NO_EXIT)
    s.close()
    _assert_loop_bits("ILU(0):", got, L.pinned_ilu0(), "five/lanes", L.ITERS)


@pytest.mark.parametrize("exit_at", ["half", "full"])
@pytest.mark.parametrize("form", ["five/stream", "fused/stream", "single"])
def test_loop_bits_exits(cm, ctx, sw, form, exit_at):
    """the banded system solved to a tolerance at which the loop leaves at the half step of iteration 3 / at the full step of
    iteration 3 (the deciding residual >= 1 % off the tolerance: test_the_exit_cases_end_where_intended): the x the caller
    receives -- finish() applying x += alpha p in form 0, FUSE_HALF's unconditional store in form 1, x_cur = x_half in form 2 --
    and the history equal the mirror's bit for bit"""
    import test_loop_rounding as L
    A, b, x0, _ = L.inputs("banded", form)
    tol = L.TOL_HALF if exit_at == "half" else L.TOL_FULL
    want = L.pinned_exit(form, tol)
    s = _loop_solver(cm, ctx, sw, form, A, None)
    got = _loop_solve(cm, ctx, s, b, x0, "pbicgstab", maxit=20, tol=tol)
    s.close()
    st = got[0]
    assert (bool(st.half_exit), bool(st.converged), bool(st.breakdown)) == (want.half_exit, True, False) and want.half_exit == (exit_at == "half")
    _assert_loop_bits("%s exit at the %s step:" % (form, exit_at), got, (want.x, want.history), form, want.iters)


@pytest.mark.parametrize("which", ["diagonal", "banded"])
@pytest.mark.parametrize("form", ["fused/stream", "single"])
def test_loop_bits_second_solve_on_one_solver(cm, ctx, sw, form, which):
    """one solver object, 3 iterations and then 4 from a fresh copy of the same x0: the host has swapped p_a / p_b, v_a / v_b
    and r / s an odd number of times by then (after every iteration of form 1, after an odd chunk of form 2), and nothing of
    that leaks into the second solve -- each equals its mirror bit for bit"""
    import test_loop_rounding as L
    A, b, x0, d = L.inputs(which, form)
    s = _loop_solver(cm, ctx, sw, form, A, d)
    for iters in (3, 4):
        got = _loop_solve(cm, ctx, s, b, x0, "pbicgstab", maxit=iters, tol=1e-8, flags=cm.FLAG_NO_EXIT)
        _assert_loop_bits("%s %s, solve of %d iterations:" % (form, which, iters), got, L.pinned_form(which, form, iters=iters), form, iters)
    s.close()


def test_huge_maxit_does_not_allocate_a_huge_history(cm, ctx, oracle, golden_dir):
    """maxit = 2^30 (a caller's 'no limit'): the residual history is capped at 2^20 entries instead of 16 GB"""
    A = _load(oracle, golden_dir, "mat900")
    b = oracle.spmv(A, 1.0 + np.sin(np.arange(A.n)))
    x, st, h = _solve_dev(cm, ctx, A, b, loop=cm.LOOP_PBICGSTAB, maxit=2 ** 30, tol=1e-8)
    assert st.converged and st.iters < 100 and len(h) <= 2 * st.iters + 1
    xo, so = oracle.pbicgstab(A, b, maxit=2000, tol=1e-8)
    assert np.linalg.norm(x - xo) / np.linalg.norm(xo) <= 1e-5


@pytest.mark.parametrize("precond", [0, 1])
def test_exact_initial_guess_returns_at_once(cm, ctx, oracle, precond):
    """r0 = 0 (x0 already solves the system): converged, 0 iterations, x0 untouched -- where the reference's loop
    (and the oracle's restatement of it) divides 0 by 0 and returns NaNs; a deliberate difference"""
    A = oracle.rand_rows(500, 10, 3)
    b = oracle.spmv(A, np.ones(A.n))
    for loop in (cm.LOOP_PBICGSTAB, cm.LOOP_PBICGSTAB2):
        if precond and loop == cm.LOOP_PBICGSTAB2:
            continue
        x, st, h = _solve_dev(cm, ctx, A, b, precond=precond, loop=loop, maxit=50, tol=1e-8)
        assert st.converged and st.iters == 0 and not st.breakdown and st.nrm0 == 0.0
        np.testing.assert_array_equal(x, np.ones(A.n))


# ------------------------------------------------------------- pipelined BiCGStab
@pytest.mark.parametrize("name,tol", [("mat900", 1e-8), ("mat10000", 1e-8), ("rand20000", 1e-8), ("poisson", 1e-8)])
def test_pipelined_bicgstab_vs_oracle(cm, ctx, oracle, golden_dir, name, tol):
    """CUDAMAT_LOOP_PIPELINED (Cools & Vanroose 2017, Alg. 4) is NOT a reference algorithm: its parity statement is
    (a) the oracle's restatement of the published recurrences (oracle_solvers.c orc_pipelined_bicgstab): residual
    history 1e-8 relative over the first iterations, iteration count +-15 % (>= +-2: the longer recurrences carry
    rounding differences forward, so late iterations of a 60-70 iteration solve wander by a few), solution 1e-6;
    (b) the reference loop it re-arranges (pbicgstab.cu:45-154, M = I): same solution to 1e-5, iteration count
    within +-15 %; (c) the true residual under 10 tol ||r0||."""
    if name == "rand20000":
        A = oracle.rand_rows(20000, 50, 0x5EED)
    elif name == "poisson":
        A = oracle.poisson5(300, 200)
    else:
        A = _load(oracle, golden_dir, name)
    xs = 1.0 + np.sin(np.arange(A.n))
    b = oracle.spmv(A, xs)
    before = oracle.num_threads()
    oracle.set_num_threads(1)                # fixed summation order in the checker
    try:
        xo, so, ho = oracle.pipelined_bicgstab(A, b, maxit=2000, tol=tol, want_hist=True)
        xr, sr = oracle.pbicgstab(A, b, maxit=2000, tol=tol)
    finally:
        oracle.set_num_threads(before)
    x, st, h = _solve_dev(cm, ctx, A, b, loop=cm.LOOP_PIPELINED, maxit=2000, tol=tol)
    assert st.converged and so.converged
    assert abs(st.iters - so.iters) <= max(2, 0.15 * so.iters)
    assert abs(st.iters - sr.iters) <= max(2, 0.15 * sr.iters)
    k = min(len(h), 8, 2 * so.iters)
    np.testing.assert_allclose(h[:k], ho[:k], rtol=1e-8)
    assert len(h) == 2 * st.iters + (1 if st.half_exit else 0)
    assert np.linalg.norm(x - xo) / np.linalg.norm(xo) <= 1e-6
    assert np.linalg.norm(x - xr) / np.linalg.norm(xr) <= 1e-5
    r0 = np.linalg.norm(b - oracle.spmv(A, np.ones(A.n)))
    assert np.linalg.norm(b - oracle.spmv(A, x)) <= 10 * tol * r0
    # the standard loop on the GPU agrees too
    x2, st2, h2 = _solve_dev(cm, ctx, A, b, loop=cm.LOOP_PBICGSTAB, maxit=2000, tol=tol)
    assert np.linalg.norm(x - x2) / np.linalg.norm(x2) <= 1e-5


def test_half_step_update_of_x_rides_in_the_full_step_kernel(cm, ctx, oracle, golden_dir, sw):
    """the five-launch reference loop leaves pbicgstab.cu:110 (x += alpha p) to k_full of the same iteration, and to one
    axpy after the loop when the solve leaves through the half-step test (x is then streamed once per iteration).  Same
    operations on the same operands as the reference's two updates: through both exits, with and without ILU(0), the
    iterate must be the oracle's (same iteration count, same exit, x to 1e-9) and the residual the loop reports must be
    the TRUE residual of the x it returns -- an update of x that was dropped or applied twice on either exit would show
    there at once.  (Round 3 kept the two-pass form as a switch and compared the two bit for bit; it was removed in
    round 4.)"""
    sw("FUSED", "0")                # the five-launch form also on small systems
    sw("RESIDENT", "0")
    A = oracle.rand_rows(5000, 12, 7)
    xs = oracle.xstar(A.n, 3)
    b = oracle.spmv(A, xs)
    seen_half = seen_full = False
    for precond in (cm.PRECOND_NONE, cm.PRECOND_ILU0):
        for tol in (1e-3, 1e-5, 1e-7, 1e-8, 1e-11):
            x1, st1, h1 = _solve_dev(cm, ctx, A, b, precond=precond, loop=cm.LOOP_PBICGSTAB, maxit=100, tol=tol)
            assert st1.converged and st1.loop_form == 0
            r_true = np.linalg.norm(b - oracle.spmv(A, x1))
            assert abs(r_true - st1.nrm) <= 1e-10 * st1.nrm0, (tol, r_true, st1.nrm)
            assert st1.nrm == h1[-1]
            xo, so = oracle.pbicgstab(A, b, vm=oracle.ilu0(A) if precond else None, maxit=100, tol=tol)
            assert (st1.iters, st1.half_exit) == (so.iters, so.half_exit), (tol, st1.iters, so.iters)
            np.testing.assert_allclose(x1, xo, rtol=1e-9, atol=1e-12)
            seen_half |= bool(st1.half_exit)
            seen_full |= not st1.half_exit
    assert seen_half and seen_full, "the tolerances above were chosen to leave through both tests"


def test_pipelined_bicgstab_exits_and_limits(cm, ctx, oracle):
    """half-step exit returns x + alpha p (kept in a side buffer), maxit stops without convergence, an exact initial
    guess converges in 0 iterations, NO_EXIT runs the full window"""
    A = oracle.rand_rows(5000, 12, 7)
    xs = oracle.xstar(A.n, 3)
    b = oracle.spmv(A, xs)
    seen_half = seen_full = False
    for tol in (1e-3, 1e-5, 1e-8, 1e-11):
        x, st, h = _solve_dev(cm, ctx, A, b, loop=cm.LOOP_PIPELINED, maxit=100, tol=tol)
        xo, so = oracle.pipelined_bicgstab(A, b, maxit=100, tol=tol)
        assert st.converged and (st.iters, st.half_exit) == (so.iters, so.half_exit), (tol, st.iters, so.iters)
        np.testing.assert_allclose(x, xo, rtol=1e-9, atol=1e-12)
        seen_half |= bool(st.half_exit)
        seen_full |= not st.half_exit
    assert seen_half and seen_full, "the tolerances above were chosen to leave through both tests"
    x, st, h = _solve_dev(cm, ctx, A, b, loop=cm.LOOP_PIPELINED, maxit=2, tol=1e-14)
    assert st.iters == 2 and not st.converged and len(h) == 4
    x, st, h = _solve_dev(cm, ctx, A, b, x0=xs, loop=cm.LOOP_PIPELINED, maxit=50, tol=1e-8)
    assert st.converged and st.iters == 0 and np.array_equal(x, xs)
    x, st, h = _solve_dev(cm, ctx, A, b, loop=cm.LOOP_PIPELINED, maxit=4, tol=1e-2, flags=cm.FLAG_NO_EXIT)
    assert st.iters == 4 and len(h) == 8


@pytest.mark.parametrize("name,tol", [("mat900", 1e-8), ("mat10000", 1e-8), ("rand20000", 1e-8), ("poisson", 1e-10)])
def test_preconditioned_pipelined_bicgstab_vs_oracle(cm, ctx, oracle, golden_dir, name, tol):
    """SURVEY 8 f4 finished: CUDAMAT_LOOP_PIPELINED with ILU(0) (Cools & Vanroose's preconditioned p-BiCGStab: M^-1 where
    pbicgstab.cu:92-98,121-127 apply it, the M^-1-applied vectors carried by recurrences, still two reduction phases per
    iteration) and residual replacement every 32 iterations.  Not a reference algorithm; parity statement:
    (a) the oracle's restatement of the same recurrences (orc_ppipelined_bicgstab): history 1e-7 over the first
    iterations, iteration count +-10 % (>= +-2), solution 1e-6; (b) the reference's preconditioned loop
    (orc_pbicgstab with the same ILU(0), pbicgstab.cu:45-154): solution 1e-5, iteration count +-10 % (>= +-2);
    (c) true residual within 10 tol ||r0||, no restart of the verified iterate."""
    if name == "rand20000":
        A = oracle.rand_rows(20000, 50, 0x5EED)
    elif name == "poisson":
        A = oracle.poisson5(300, 200)
    else:
        A = _load(oracle, golden_dir, name)
    xs = 1.0 + np.sin(np.arange(A.n))
    b = oracle.spmv(A, xs)
    before = oracle.num_threads()
    oracle.set_num_threads(1)
    try:
        vm = oracle.ilu0(A)
        xo, so, ho = oracle.pipelined_bicgstab(A, b, maxit=2000, tol=tol, want_hist=True, vm=vm)
        xr, sr = oracle.pbicgstab(A, b, vm=vm, maxit=2000, tol=tol)
    finally:
        oracle.set_num_threads(before)
    x, st, h = _solve_dev(cm, ctx, A, b, loop=cm.LOOP_PIPELINED, precond=cm.PRECOND_ILU0, maxit=2000, tol=tol)
    assert st.converged and so.converged and sr.converged and st.restarts == 0 and so.restarts == 0
    assert abs(st.iters - so.iters) <= max(2, 0.1 * so.iters), (st.iters, so.iters)
    assert abs(st.iters - sr.iters) <= max(2, 0.1 * sr.iters), (st.iters, sr.iters)
    k = min(len(h), 6, 2 * so.iters)
    np.testing.assert_allclose(h[:k], ho[:k], rtol=1e-7)
    assert len(h) == 2 * st.iters + (1 if st.half_exit else 0)
    assert np.linalg.norm(x - xo) / np.linalg.norm(xo) <= 1e-6
    assert np.linalg.norm(x - xr) / np.linalg.norm(xr) <= 1e-5
    r0 = np.linalg.norm(b - oracle.spmv(A, np.ones(A.n)))
    assert np.linalg.norm(b - oracle.spmv(A, x)) <= 10 * tol * r0
    # the reference's preconditioned loop on the GPU returns the same solution
    x2, st2, h2 = _solve_dev(cm, ctx, A, b, loop=cm.LOOP_PBICGSTAB, precond=cm.PRECOND_ILU0, maxit=2000, tol=tol)
    assert st2.converged and np.linalg.norm(x - x2) / np.linalg.norm(x2) <= 1e-5


def test_residual_replacement_keeps_the_pipelined_loop_on_the_true_residual(cm, ctx, oracle):
    """a 300 x 200 Laplacian at tol 1e-10, where pipelined recurrences without replacement can stagnate near 1e-9 ||r0||
    (whether they do depends on the rounding path: a numpy restatement needed 576 iterations and still missed the target
    by 60x, the C oracle and the kernels happen to get through).  With residual replacement every 32 iterations (the
    default) the loop converges like the reference's on every path tried: same iteration count +-15 %, no restart, true
    residual under 2 tol ||r0|| -- on the kernels and in the oracle's restatement."""
    A = oracle.poisson5(300, 200)
    xs = 1.0 + np.sin(np.arange(A.n))
    b = oracle.spmv(A, xs)
    tol = 1e-10
    xr, sr = oracle.pbicgstab(A, b, maxit=3000, tol=tol)
    xo, so = oracle.pipelined_bicgstab(A, b, maxit=3000, tol=tol)
    x, st, h = _solve_dev(cm, ctx, A, b, loop=cm.LOOP_PIPELINED, maxit=3000, tol=tol)
    assert st.converged and so.converged and st.restarts == 0 and so.restarts == 0
    assert abs(st.iters - sr.iters) <= max(2, 0.15 * sr.iters) and abs(so.iters - sr.iters) <= max(2, 0.15 * sr.iters)
    assert np.linalg.norm(b - oracle.spmv(A, x)) <= 2 * tol * st.nrm0
    assert st.iters > 64       # (the solve is long enough to contain replacements)


# ------------------------------------------------------------- SELL-C-sigma
@pytest.mark.parametrize("case", ["rand_real", "poisson_real", "pareto", "hubs", "empties", "mixed", "tiny", "window_edge"])
def test_sell_spmv_is_bit_exact(cm, ctx, oracle, case, sw):
    """SELL-64-1024 (csrc/spmv_sell.hip): one lane per row, products added in column order with one rounding each =
    the rounding sequence of bicstab.cpp:72-77 => bit-exact vs the oracle on REAL-valued data, whatever the row
    lengths; padding slots are never multiplied, so an Inf in x only reaches the rows that reference it"""
    sw("SPMV_MODE", "sell")
    rng = np.random.default_rng(21)
    if case == "rand_real":
        A = oracle.rand_rows(20000, 50, 0x5EED)
    elif case == "poisson_real":
        A = oracle.poisson5(173, 59)
    elif case == "tiny":
        A = oracle.rand_rows(7, 50, 1)
    elif case == "window_edge":                 # n just past a 1024-row window and a 64-row chunk
        A = oracle.rand_rows(1024 * 3 + 65, 9, 4)
    else:
        A = _skewed_matrix(oracle, case, rng)
    A.val[:] = rng.standard_normal(A.nnz)
    x = rng.standard_normal(A.n)
    # default: one ds_add_f64 instruction per segment step, relying on the observed lane order of equal addresses;
    # CUDAMAT_PB_STRICT=1: every rank of a run of equal rows is its own instruction -- the order of a row's additions is
    # architected.  Both must reproduce the reference loop bit for bit (the 20000-column cases have runs of ~25 equal rows
    # per step, the dense row of `ragged` runs that cross the 64-entry cut): this is the guard of the observed property.
    for strict in ("0", "1"):
        sw("PB_STRICT", strict)
        np.testing.assert_array_equal(_spmv_via_solver(cm, ctx, A, x), oracle.spmv(A, x))
        d = rng.standard_normal(A.n)
        np.testing.assert_array_equal(_spmv_via_solver(cm, ctx, A, x, d=d), oracle.csrmv(A, 1.0, x, 1.0, x * d))
    # non-finite input: only the rows that hold column 3 see it
    x2 = x.copy()
    x2[3] = np.inf
    y2 = _spmv_via_solver(cm, ctx, A, x2)
    base = int(A.rowptr[0])
    rows = np.repeat(np.arange(A.n), np.diff(A.rowptr))[(A.colidx - base) == 3]
    untouched = np.setdiff1d(np.arange(A.n), rows)
    assert np.all(np.isfinite(y2[untouched])) and not np.any(np.isfinite(y2[rows]))


def test_sell_in_the_solver_loop_and_auto_selection(cm, ctx, oracle, sw):
    """(a) forced: the BiCGSTAB loop on the SELL form (fused dot partials, half-step test launch) reproduces the CSR
    run's iterates to rounding and the oracle's solution; (b) not forced: on a matrix with varying row lengths
    the tuner times SELL against the CSR forms and keeps the faster one -- either way the result is the oracle's."""
    rng = np.random.default_rng(5)
    import scipy.sparse as sp
    n = 60000
    lens = rng.integers(14, 70, n)                                  # row lengths vary by 5x around a mean of ~40
    rows = np.repeat(np.arange(n), lens)
    cols = (rows + rng.integers(-2000, 2000, rows.size)) % n
    S = sp.csr_matrix((np.ones(rows.size), (rows, cols)), shape=(n, n))
    S.sum_duplicates()
    S.data[:] = rng.integers(-2, 3, S.nnz)
    S.setdiag(np.abs(S).sum(axis=1).A1 + 1.0)
    S.eliminate_zeros()
    S.sort_indices()
    A = oracle.Csr(n, S.indptr.astype(np.int32), S.indices.astype(np.int32), S.data.astype(np.float64), n)
    xs = 1.0 + np.sin(np.arange(n))
    b = oracle.spmv(A, xs)
    xo, so = oracle.pbicgstab(A, b, maxit=200, tol=1e-8)
    res = {}
    for mode in ("sell", "csr", None):
        if mode:
            sw("SPMV_MODE", mode)
        else:
            sw("SPMV_MODE", None)
        s = cm.Solver.from_host_csr(ctx, A.rowptr, A.colidx, A.val)
        chosen = s.spmv_mode()
        assert s.spmv_kernel() == "k_spmv_sell" if chosen == 2 else s.spmv_kernel().startswith("k_spmv")
        db, dx = ctx.array(b), ctx.array(np.ones(n))
        st = s.solve(db, dx, loop=cm.LOOP_PBICGSTAB, maxit=200, tol=1e-8)
        res[mode] = (dx.download(), st.iters, chosen)
        assert st.converged and abs(st.iters - so.iters) <= 1
        assert np.linalg.norm(res[mode][0] - xo) / np.linalg.norm(xo) <= 1e-8
        s.close()
    assert res["sell"][2] == 2 and res["csr"][2] == 0 and res[None][2] in (0, 2)
    assert np.linalg.norm(res["sell"][0] - res["csr"][0]) / np.linalg.norm(xo) <= 1e-10


def test_drop_in_entry_points_over_several_ranks(cm, oracle, golden_dir, monkeypatch):
    """cm.use_gpus(n) (= cudamat_use_gpus of pbicgstab.h): the three drop-in solves row-sharded by cudamat_solve_sharded.
    On a one-GPU box the ranks share device 0 (CUDAMAT_SHARDED_ONE_DEVICE: host-synchronised copies stand in for RCCL)."""
    if cm.device_count() < 3:
        monkeypatch.setenv("CUDAMAT_SHARDED_ONE_DEVICE", "1")
    A = _load(oracle, golden_dir, "mat10000")
    xs = 1.0 + np.sin(np.arange(A.n))
    b = oracle.spmv(A, xs)
    ok1, x1, dt1, st1 = cm.bicgstab(A.n, A.nnz, A.val, A.rowptr, A.colidx, b, 2000, 1e-8)
    try:
        cm.use_gpus(3)
        ok3, x3, dt3, st3 = cm.bicgstab(A.n, A.nnz, A.val, A.rowptr, A.colidx, b, 2000, 1e-8)
        assert ok1 and ok3 and abs(st1.iters - st3.iters) <= max(2, st1.iters // 10)
        assert np.linalg.norm(x3 - x1) / np.linalg.norm(x1) <= 1e-5
        assert np.linalg.norm(b - oracle.spmv(A, x3)) <= 1e-7 * st3.nrm0
        # the preconditioned entry point: block-Jacobi ILU(0) over 3 ranks, same solution
        okp, xp, dtp, stp = cm.bicgstab_lu_precond(A.n, A.nnz, A.val, A.rowptr, A.colidx, b, 2000, 1e-8)
        assert okp and stp.converged and stp.iters < st3.iters
        assert np.linalg.norm(xp - x1) / np.linalg.norm(x1) <= 1e-5
        # (A0 + I d) with a caller's x0
        A0 = _load(oracle, golden_dir, "mat3_A0")
        d = oracle.to_dense_vector(_load(oracle, golden_dir, "vec3_d"))
        b3 = oracle.to_dense_vector(_load(oracle, golden_dir, "vec3"))
        ok, x, dt, st = cm.bicgstab_d(3, A0.nnz, A0.val, A0.rowptr, A0.colidx, d, np.ones(3), b3, 2000, 1e-5)
        assert ok
        np.testing.assert_allclose(x, [7 / 6, 17 / 3, -23 / 6], rtol=1e-7)
    finally:
        cm.use_gpus(1)


def test_drop_in_call_reuses_the_plan_of_the_previous_call(cm, oracle, monkeypatch):
    """cudamat_solve keeps the solver of its last call: the same matrix again (compared on the device after the upload)
    costs upload + loop, no analysis (plan_reused = 1, t_setup = 0, same SpMV form, ILU(0) factors kept); a changed value
    or another matrix builds anew.  And the tuner no longer times forms that cannot win: a matrix whose rows span far more
    than the L2s goes to the blocked form with nothing timed -- the same form the full timing picks."""
    cm.lib().cudamat_plan_cache_clear()
    A = oracle.rand_rows(200000, 20, 0xABCD)
    xs = oracle.xstar(A.n, 5)
    b = oracle.spmv(A, xs)
    ok, x, dt, st = cm.bicgstab(A.n, A.nnz, A.val, A.rowptr, A.colidx, b, 200, 1e-8)
    assert ok and st.plan_reused == 0 and st.t_setup > 0 and st.t_upload > 0
    b2 = oracle.spmv(A, 2.0 * xs)
    ok2, x2, dt2, st2 = cm.bicgstab(A.n, A.nnz, A.val, A.rowptr, A.colidx, b2, 200, 1e-8)
    assert ok2 and st2.plan_reused == 1 and st2.t_setup == 0 and st2.t_tune == 0 and st2.spmv_mode == st.spmv_mode
    np.testing.assert_allclose(x2, 2.0 * xs, rtol=1e-6)
    # the preconditioned entry point on the same matrix: reuses the solver, adds the factors; once more: keeps them
    okp, xp, dtp, stp = cm.bicgstab_lu_precond(A.n, A.nnz, A.val, A.rowptr, A.colidx, b, 200, 1e-8)
    assert okp and stp.converged and stp.plan_reused == 1 and stp.t_factor > 0
    okq, xq, dtq, stq = cm.bicgstab_lu_precond(A.n, A.nnz, A.val, A.rowptr, A.colidx, b2, 200, 1e-8)
    assert stq.converged and stq.plan_reused == 1 and stq.t_factor == 0 and stq.t_analysis == 0
    np.testing.assert_allclose(xq, 2.0 * xs, rtol=1e-6)
    # one value changed: not the same matrix
    v2 = A.val.copy()
    v2[12345] *= 1.5
    A2 = oracle.Csr(A.n, A.rowptr, A.colidx, v2, A.n)
    ok3, x3, dt3, st3 = cm.bicgstab(A.n, A.nnz, v2, A.rowptr, A.colidx, oracle.spmv(A2, xs), 200, 1e-8)
    assert ok3 and st3.plan_reused == 0 and st3.t_setup > 0
    np.testing.assert_allclose(x3, xs, rtol=1e-6)
    # CUDAMAT_PLAN_CACHE=0: every call builds anew
    monkeypatch.setenv("CUDAMAT_PLAN_CACHE", "0")
    ok4, x4, dt4, st4 = cm.bicgstab(A.n, A.nnz, v2, A.rowptr, A.colidx, oracle.spmv(A2, xs), 200, 1e-8)
    assert ok4 and st4.plan_reused == 0
    monkeypatch.delenv("CUDAMAT_PLAN_CACHE")
    # scattered columns: nothing is timed, and the full timing agrees with the shortcut
    S = oracle.rand_rows(4_000_000, 9, 0x77)       # mean column span 0.8 x 32 MB of x
    bs = oracle.spmv(S, oracle.xstar(S.n, 6))
    oks, xs_, dts, sts = cm.bicgstab(S.n, S.nnz, S.val, S.rowptr, S.colidx, bs, 200, 1e-8)
    assert oks and sts.plan_reused == 0 and sts.spmv_mode == 1 and sts.t_tune == 0
    monkeypatch.setenv("CUDAMAT_SPMV_TUNE", "full")
    monkeypatch.setenv("CUDAMAT_PLAN_CACHE", "0")
    okf, xf, dtf, stf = cm.bicgstab(S.n, S.nnz, S.val, S.rowptr, S.colidx, bs, 200, 1e-8)
    assert okf and stf.spmv_mode == 1 and stf.t_tune > 0
    np.testing.assert_array_equal(xf, xs_)
    # The first call above built its blocked copy BESIDE the upload (csrc/dropin.hip) -- behind the value dictionary, in one
    # fill pass after the last byte; the full timing built it the ordinary way: same bits.  With fp64 values the copy is
    # filled PIECE BY PIECE behind the value milestones (36 M entries: three pieces): same bits again, and nearly all of the
    # set-up hidden behind the upload.
    monkeypatch.delenv("CUDAMAT_SPMV_TUNE")
    monkeypatch.setenv("CUDAMAT_VALUE_DICT", "0")
    okv, xv, dtv, stv = cm.bicgstab(S.n, S.nnz, S.val, S.rowptr, S.colidx, bs, 200, 1e-8)
    assert okv and stv.spmv_mode == 1 and stv.t_tune == 0 and stv.plan_reused == 0
    np.testing.assert_array_equal(xv, xs_)
    # index base 1 through the same path (rebased in place once the pattern has landed)
    okb, xb, dtb, stb = cm.bicgstab(S.n, S.nnz, S.val, S.rowptr + 1, S.colidx + 1, bs, 200, 1e-8)
    assert okb and stb.spmv_mode == 1
    np.testing.assert_array_equal(xb, xs_)
    # The count pass of the blocked copy walks the column indices piece by piece WHILE they arrive, before they have been
    # validated (only the row pointers have): a column outside the matrix or row pointers that decrease must still end in
    # the validation's error, never in a stray access.
    bad_c = S.colidx.copy()
    bad_c[20_000_000] = S.n + 7
    bad_c[30_000_001] = -3
    with pytest.raises(cm.CudamatError, match="column index"):
        cm.bicgstab(S.n, S.nnz, S.val, S.rowptr, bad_c, bs, 200, 1e-8)
    bad_r = S.rowptr.copy()
    bad_r[1000] = bad_r[1001] + 5
    with pytest.raises(cm.CudamatError, match="row pointers"):
        cm.bicgstab(S.n, S.nnz, S.val, bad_r, S.colidx, bs, 200, 1e-8)
    oka, xa, dta, sta = cm.bicgstab(S.n, S.nnz, S.val, S.rowptr, S.colidx, bs, 200, 1e-8)       # and the library is fine afterwards
    assert oka and sta.spmv_mode == 1
    np.testing.assert_array_equal(xa, xs_)
    cm.lib().cudamat_plan_cache_clear()


def test_a_failing_rank_does_not_strand_its_peers(cm, oracle, golden_dir, monkeypatch):
    """cudamat_solve_sharded with one rank whose k-th all-reduce fails (injected): that rank leaves the solve while its
    peers are inside the next collective -- the call must RETURN (an error naming the rank), not hang: the failing rank
    breaks the emulated barriers / aborts every rank's RCCL communicator before anything waits for a stream."""
    import threading
    if cm.device_count() < 3:
        monkeypatch.setenv("CUDAMAT_SHARDED_ONE_DEVICE", "1")
    A = _load(oracle, golden_dir, "mat10000")
    b = oracle.spmv(A, 1.0 + np.sin(np.arange(A.n)))
    for inj in ("1:7", "0:3", "2:12"):           # in the loop, right after the setup agreement, some iterations in
        monkeypatch.setenv("CUDAMAT_TEST_COMM_FAIL", inj)
        box = {}

        def call():
            try:
                cm.use_gpus(3)
                box["res"] = cm.bicgstab(A.n, A.nnz, A.val, A.rowptr, A.colidx, b, 2000, 1e-8)
            except Exception as e:  # noqa: BLE001
                box["err"] = e
            finally:
                cm.use_gpus(1)

        t = threading.Thread(target=call, daemon=True)
        t.start()
        t.join(120)
        assert not t.is_alive(), "cudamat_solve_sharded did not return after rank %s failed" % inj.split(":")[0]
        assert "err" in box and "rank %s of 3" % inj.split(":")[0] in str(box["err"]) and "injected" in str(box["err"]), box
    monkeypatch.delenv("CUDAMAT_TEST_COMM_FAIL")
    ok, x, dt, st = cm.bicgstab(A.n, A.nnz, A.val, A.rowptr, A.colidx, b, 2000, 1e-8)      # and the library still works
    assert ok


def test_single_launch_loop_matches_the_three_launch_loop(cm, ctx, oracle, golden_dir, sw):
    """systems of at most one stream tile per compute unit run the whole loop in ONE launch (grid barriers between
    the phases, cudamat_stats.loop_form == 2): same stopping decisions and iterates as one launch per phase"""
    for name, loop, tol in (("mat10000", cm.LOOP_PBICGSTAB, 1e-8), ("mat900", cm.LOOP_PBICGSTAB, 1e-8),
                            ("mat10000", cm.LOOP_PBICGSTAB2, 1e-8)):
        A = _load(oracle, golden_dir, name)
        xs = 1.0 + np.sin(np.arange(A.n))
        b = oracle.spmv(A, xs)
        res = {}
        for resident in ("1", "0"):
            sw("RESIDENT", resident)
            s = cm.Solver.from_host_csr(ctx, A.rowptr, A.colidx, A.val)
            db, dx = ctx.array(b), ctx.empty(A.n)
            st = s.solve(db, dx, loop=loop, maxit=2000, tol=tol, flags=cm.FLAG_X0_ONES)
            res[resident] = (dx.download(), st, s.history())
            for a in (db, dx):
                a.free()
            s.close()
        (x1, st1, h1), (x0, st0, h0) = res["1"], res["0"]
        assert st1.loop_form == 2 and st0.loop_form == 1 and st1.loop_fallbacks == 0
        assert st1.converged and st0.converged
        # the only difference is the grouping of the last phase's partial sums (per tile / per vector chunk): the
        # residual histories start out equal to rounding and then drift apart as any two BiCGSTAB runs with different
        # summation orders do (an un-preconditioned 70-iteration run amplifies 1e-16 to tens of percent)
        assert abs(st1.iters - st0.iters) <= max(2, st0.iters // 10)
        np.testing.assert_allclose(h1[:8], h0[:8], rtol=1e-12)
        assert np.linalg.norm(x1 - x0) <= 1e-5 * np.linalg.norm(x0)
        assert np.linalg.norm(x1 - xs) <= 1e-5 * np.linalg.norm(xs)
        assert np.linalg.norm(b - oracle.spmv(A, x1)) <= 1.5 * tol * st1.nrm0
    # the (A0 + I d) variant with a caller's x0
    A = _load(oracle, golden_dir, "mat900")
    rng = np.random.default_rng(5)
    d = 0.5 + rng.random(A.n)
    xs = 1.0 + rng.random(A.n)
    b = oracle.spmv(A, xs) + d * xs
    out = {}
    for resident in ("1", "0"):
        sw("RESIDENT", resident)
        x, st, h = _solve_dev(cm, ctx, A, b, d=d, loop=cm.LOOP_PBICGSTAB2, maxit=400, tol=1e-9)
        out[resident] = (x, st, h)
    assert (out["1"][1].loop_form, out["0"][1].loop_form) == (2, 1)
    assert out["1"][1].converged and abs(out["1"][1].iters - out["0"][1].iters) <= 2
    np.testing.assert_allclose(out["1"][2][:8], out["0"][2][:8], rtol=1e-12)
    np.testing.assert_allclose(out["1"][0], xs, rtol=1e-6)
    # fixed iteration windows (the bench's mode): exactly maxit iterations, odd and even, also across launch chunks
    A = _load(oracle, golden_dir, "mat10000")
    b = oracle.spmv(A, 1.0 + np.sin(np.arange(A.n)))
    sw("RESIDENT", "1")
    s = cm.Solver.from_host_csr(ctx, A.rowptr, A.colidx, A.val)
    db, dx = ctx.array(b), ctx.empty(A.n)
    for maxit in (1, 2, 7, 8193):
        st = s.solve(db, dx, maxit=maxit, tol=1e-8, flags=cm.FLAG_X0_ONES | cm.FLAG_NO_EXIT)
        assert st.iters == maxit and st.loop_form == 2
    s.close()


def test_single_launch_loop_timeout_redoes_the_solve(cm, ctx, oracle, golden_dir, sw):
    """a grid barrier whose wait runs into its bound (forced here: a bound of one poll) voids the attempt: the solve
    is redone from the caller's x0 with one launch per phase, the solver stays with that form, the stats say so"""
    A = _load(oracle, golden_dir, "mat10000")
    xs = 1.0 + np.sin(np.arange(A.n))
    b = oracle.spmv(A, xs)
    x0 = np.full(A.n, 0.25)
    sw("RESIDENT", "0")
    s = cm.Solver.from_host_csr(ctx, A.rowptr, A.colidx, A.val)
    db, dx = ctx.array(b), ctx.array(x0)
    ref = s.solve(db, dx, maxit=2000, tol=1e-8)
    xref = dx.download()
    s.close()
    sw("RESIDENT", "1")
    sw("RESIDENT_SPIN_LIMIT", "0")
    s = cm.Solver.from_host_csr(ctx, A.rowptr, A.colidx, A.val)
    dx2 = ctx.array(x0)
    st = s.solve(db, dx2, maxit=2000, tol=1e-8)
    assert st.loop_fallbacks == 1 and st.loop_form == 1 and st.converged and st.iters == ref.iters
    np.testing.assert_array_equal(dx2.download(), xref)
    sw("RESIDENT_SPIN_LIMIT", None)
    dx3 = ctx.array(x0)
    st = s.solve(db, dx3, maxit=2000, tol=1e-8)          # the solver keeps to the three-launch loop
    assert st.loop_fallbacks == 1 and st.loop_form == 1
    np.testing.assert_array_equal(dx3.download(), xref)
    s.close()


def test_value_dictionary_is_bit_exact(cm, ctx, oracle, sw):
    """matrices with at most 256 distinct values: the blocked kernels and the compressed stream kernel read 8-bit
    indices into a dictionary of the distinct bit patterns (csrc/valdict.hip) -- same doubles, same order, so the
    products are bit-identical to the run on the fp64 values and to the oracle; 257 distinct values: no dictionary"""
    import scipy.sparse as sp
    rng = np.random.default_rng(17)
    n = 300_000
    cases = []
    # scattered columns, 12 per row, values from a small set with -0.0 and a denormal among them -> blocked kernels
    nnz = n * 12
    S = sp.csr_matrix((np.ones(nnz), (np.repeat(np.arange(n), 12), rng.integers(0, n, nnz))), shape=(n, n))
    S.sum_duplicates(); S.sort_indices()
    few = np.array([-2.0, -1.0, 1.0, 2.0, 0.5, -0.0, 5e-324, 1e300, np.pi])
    cases.append(("pb", S, few))
    # banded short rows -> compressed stream kernel
    B = sp.diags([1.0, 1.0, 1.0, 1.0, 1.0], [-700, -1, 0, 1, 700], shape=(n, n), format="csr")
    B.sort_indices()
    cases.append(("csr", B, np.array([4.0, -1.0, -1.0000000000000002])))
    cases.append(("pb", S, rng.standard_normal(257)))              # one value too many
    for k, (mode, M, vals) in enumerate(cases):
        data = vals[rng.integers(0, len(vals), M.nnz)]
        data[:len(vals)] = vals                                    # every value occurs
        A = oracle.Csr(n, (M.indptr + 1).astype(np.int32), (M.indices + 1).astype(np.int32), data, n)
        x = rng.standard_normal(n)
        want = oracle.spmv(A, x)
        got = {}
        for vd in ("1", "0"):
            sw("VALUE_DICT", vd)
            sw("SPMV_MODE", mode)
            s = cm.Solver.from_host_csr(ctx, A.rowptr, A.colidx, A.val)
            dx, dy = ctx.array(x), ctx.empty(n)
            s.spmv(dx, dy)
            got[vd] = (dy.download(), s.value_dict(), s.spmv_mode())
            for a in (dx, dy):
                a.free()
            s.close()
        assert got["0"][1] == 0
        assert got["1"][1] == (len(np.unique(vals.view(np.uint64))) if len(vals) <= 256 else 0), (k, got["1"][1])
        assert got["1"][2] == (1 if mode == "pb" else 0)
        np.testing.assert_array_equal(got["1"][0].view(np.uint64), got["0"][0].view(np.uint64))
        if mode == "pb":
            np.testing.assert_array_equal(got["1"][0], want)       # the blocked form is bit-exact against the oracle
        else:
            np.testing.assert_allclose(got["1"][0], want, rtol=1e-13, atol=1e-300)


def _soak_case(oracle, seed, want):
    """the system tests/soak.py builds as case `want` of seed `seed` (the generator's draws are replayed)"""
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    for case in range(want + 1):
        n = int(rng.integers(1, 40000))
        per = float(rng.choice([1.5, 4, 9, 30, 80]))
        nnz_t = int(min(n * per, 3e6))
        if case % 3 == 2:
            lens = np.minimum(1 + (rng.pareto(1.2, n) * per / 4).astype(np.int64), max(n // 2, 1))
            lens[rng.integers(0, n, 3)] = max(n // 3, 1)
            ri = np.repeat(np.arange(n), lens)[:int(3e6)]
            nnz_t = ri.size
        else:
            ri = rng.integers(0, n, nnz_t)
        cj = rng.integers(0, n, nnz_t)
        vals = rng.uniform(-1, 1, nnz_t)
        if case % 4 == 1:
            vals = rng.choice(np.array([-1.0, -0.5, 0.25, 2.0]), nnz_t)
        dshift = np.full(n, 1.5) if case % 4 == 1 else 1.0 + rng.random(n)
        base = int(rng.integers(0, 2))
        rng.standard_normal(n)
        xs = 1.0 + rng.random(n)
        rng.standard_normal(n)
    S = sp.csr_matrix((vals, (ri, cj)), shape=(n, n)); S.sum_duplicates(); S.setdiag(0); S.eliminate_zeros()
    S = (S + sp.diags(dshift + np.asarray(abs(S).sum(axis=1)).ravel())).tocsr(); S.sort_indices()
    A = oracle.Csr(n, (S.indptr + base).astype(np.int32), (S.indices + base).astype(np.int32), S.data.copy(), n)
    return A, xs, oracle.spmv(A, xs)


def test_pipelined_loop_verifies_its_iterate(cm, ctx, oracle, sw):
    """the pipelined loop's recurrences drift: on this system (case 41 of `tests/soak.py 21`: 11 881 rows of Pareto
    lengths with three hub rows) the recursive residual of the loop WITHOUT residual replacement passes a 1e-9 test after
    319 iterations while the true one is 5.6e-3.  Two defences: (1) residual replacement every 32 iterations (the
    default): the loop converges like the reference's, restarts == 0 on both sides; (2) an iterate that loop calls
    converged is checked against its TRUE residual (one SpMV) and the loop restarted from it when it is off -- seen with
    replacement switched off; the oracle's restatement applies the same rules"""
    A, xs, b = _soak_case(oracle, 21, 41)
    tol = 1e-9
    xo_raw, so_raw = oracle.pipelined_bicgstab(A, b, maxit=1000, tol=tol, verify=False, rr=0)
    assert so_raw.converged and np.linalg.norm(b - oracle.spmv(A, xo_raw)) > 1e3 * tol * so_raw.nrm0      # the drift is real
    xr, sr = oracle.pbicgstab(A, b, maxit=1000, tol=tol)
    # (1) with replacement
    xo, so = oracle.pipelined_bicgstab(A, b, maxit=1000, tol=tol)
    x, st, h = _solve_dev(cm, ctx, A, b, loop=cm.LOOP_PIPELINED, maxit=1000, tol=tol)
    assert st.converged and so.converged and st.restarts == 0 and so.restarts == 0
    assert abs(st.iters - sr.iters) <= 0.15 * sr.iters and abs(so.iters - sr.iters) <= 0.15 * sr.iters, (st.iters, so.iters, sr.iters)
    assert np.linalg.norm(b - oracle.spmv(A, x)) <= 2.5 * tol * st.nrm0
    np.testing.assert_allclose(x, xs, rtol=1e-6)
    # (2) without: the verify-and-restart rule still makes 'converged' mean what it means for the other loops
    sw("PIPE_RR", "0")
    xo, so = oracle.pipelined_bicgstab(A, b, maxit=1000, tol=tol, rr=0)
    x, st, h = _solve_dev(cm, ctx, A, b, loop=cm.LOOP_PIPELINED, maxit=1000, tol=tol)
    sw("PIPE_RR", None)
    assert st.converged and so.converged
    assert np.linalg.norm(b - oracle.spmv(A, x)) <= 2.5 * tol * st.nrm0          # twice the target is the acceptance bound
    assert np.linalg.norm(b - oracle.spmv(A, xo)) <= 2.5 * tol * so.nrm0
    np.testing.assert_allclose(x, xs, rtol=1e-6)
    # (whether the GPU's rounding drifts on this very system too is not guaranteed; when it restarts, the stats say so)
    assert so.restarts >= 1 and 0 <= st.restarts <= 3
    assert st.iters <= 2 * so.iters
    # the standard loop on the same system needs no such help
    x1, st1, _ = _solve_dev(cm, ctx, A, b, loop=cm.LOOP_PBICGSTAB, maxit=1000, tol=tol)
    assert st1.converged and st1.restarts == 0 and np.linalg.norm(b - oracle.spmv(A, x1)) <= 2.5 * tol * st1.nrm0


def test_context_options(cm, oracle):
    """csrc/config.h: a context reads CUDAMAT_* once, when it is created; afterwards a switch changes only through
    cudamat_ctx_set_option, and whatever runs on the context next sees it.  Unknown names and values outside an option's
    range are errors, not silently ignored."""
    import os
    A = oracle.rand_rows(70000, 20, 3)
    x = np.arange(A.n) % 7 + 1.0
    want = oracle.spmv(A, x)
    os.environ["CUDAMAT_SPMV_MODE"] = "pb"
    try:
        c = cm.Context(0)                      # reads the environment here ...
    finally:
        del os.environ["CUDAMAT_SPMV_MODE"]
    s = cm.Solver.from_host_csr(c, A.rowptr, A.colidx, A.val)
    assert s.spmv_mode() == 1                  # ... so the switch holds although the variable is gone
    s.close()
    os.environ["CUDAMAT_SPMV_MODE"] = "csr"    # a later change of the environment does not reach the context
    try:
        s = cm.Solver.from_host_csr(c, A.rowptr, A.colidx, A.val)
        assert s.spmv_mode() == 1
        s.close()
        c.reset_options()                      # ... unless the host asks for it
        s = cm.Solver.from_host_csr(c, A.rowptr, A.colidx, A.val)
        assert s.spmv_mode() == 0
        s.close()
    finally:
        del os.environ["CUDAMAT_SPMV_MODE"]
    c.set_option("CUDAMAT_SPMV_MODE", "sell").set_option("SPMV_SELL", 1)
    s = cm.Solver.from_host_csr(c, A.rowptr, A.colidx, A.val)
    assert s.spmv_mode() == 2
    dx, dy = c.array(x), c.empty(A.n)
    s.spmv(dx, dy)
    np.testing.assert_array_equal(dy.download(), want)
    s.close()
    for name, value in (("NO_SUCH_SWITCH", "1"), ("SPMV_MODE", "ell"), ("SPMV_LANES", "3"), ("PB_DEPTH", "5"), ("VERBOSE", "yes"),
                        ("TEST_COMM_FAIL", "1"), ("TRSV_GROUPS", "1")):
        with pytest.raises(cm.CudamatError):
            c.set_option(name, value)
    c.close()


def _stencil9(oracle, nx, ny, rng):
    """9-point stencil on an nx x ny grid with real values: rows of 4 / 6 / 9 entries, 9 row shapes"""
    import scipy.sparse as sp
    ex, ey = np.ones(nx), np.ones(ny)
    Tx = sp.diags([ex[:-1], ex, ex[:-1]], [-1, 0, 1])
    Ty = sp.diags([ey[:-1], ey, ey[:-1]], [-1, 0, 1])
    S = sp.kron(Ty, Tx).tocsr()
    S.sort_indices()
    S.data[:] = rng.standard_normal(S.nnz)
    return oracle.Csr(S.shape[0], S.indptr.astype(np.int32), S.indices.astype(np.int32), S.data.astype(np.float64), S.shape[0])


@pytest.mark.parametrize("case", ["poisson_real", "nine_point", "empty_rows_base1", "tiny", "poisson_dict", "nine_point_dict"])
def test_row_pattern_spmv_is_bit_exact(cm, ctx, oracle, case, sw):
    """the row-pattern dictionary form (csrc/spmv_pat.hip: one byte per row instead of column indices) adds a row's
    products in column order with one rounding each -- the rounding sequence of `b[i] += A.Value[j] * x[A.Col[j]]`
    (bicstab.cpp:72-77): bit for bit the oracle's result on real-valued data, with the diagonal term, with rows of
    different lengths, empty rows, a row count that is no multiple of the 64-row chunks, index base 1; and with a value
    dictionary (few distinct values: one byte per entry packed into an 8- or 16-byte word per row, k_spmv_pat_d)"""
    sw("SPMV_MODE", "pat")
    rng = np.random.default_rng(12)
    if case == "poisson_dict":
        A = oracle.poisson5(733, 417)                    # values 4 / -1: two distinct, 1.5 M entries
    elif case == "nine_point_dict":
        A = _stencil9(oracle, 700, 401, rng)             # rows of up to 9 entries: 16-byte index words
        A.val[:] = rng.choice(np.array([-2.5, -1.0, 0.125, 3.0, 7.75]), A.nnz)
    elif case == "poisson_real":
        A = oracle.poisson5(733, 417)
        A.val[:] = rng.standard_normal(A.nnz)
    elif case == "nine_point":
        A = _stencil9(oracle, 211, 97, rng)
    elif case == "tiny":
        A = oracle.poisson5(3, 2)
    else:
        import scipy.sparse as sp
        n = 10007
        S = sp.diags([rng.standard_normal(n - 7), rng.standard_normal(n), rng.standard_normal(n - 3)], [-7, 0, 3]).tolil()
        for r in (0, 5, 64, 4099, n - 1):
            S[r, :] = 0                     # empty rows
        S = S.tocsr()
        S.eliminate_zeros()
        S.sort_indices()
        A = oracle.Csr(n, (S.indptr + 1).astype(np.int32), (S.indices + 1).astype(np.int32), S.data.astype(np.float64), n)
    x = rng.standard_normal(A.n)
    s = cm.Solver.from_host_csr(ctx, A.rowptr, A.colidx, A.val, n_cols=A.m)
    assert s.spmv_mode() == 3
    if case.endswith("_dict"):
        assert s.spmv_kernel() == ("k_spmv_pat_d<1>" if case == "poisson_dict" else "k_spmv_pat_d<2>") and s.value_dict() == (2 if case == "poisson_dict" else 5)
    else:
        assert s.spmv_kernel().startswith("k_spmv_pat<") and s.value_dict() == 0
    s.close()
    np.testing.assert_array_equal(_spmv_via_solver(cm, ctx, A, x), oracle.spmv(A, x))
    d = rng.standard_normal(A.n)
    np.testing.assert_array_equal(_spmv_via_solver(cm, ctx, A, x, d=d), oracle.csrmv(A, 1.0, x, 1.0, x * d))


def test_row_pattern_form_refuses_what_it_cannot_describe(cm, ctx, oracle, sw):
    """more than 255 row shapes, or a row longer than 15 entries: forced, the builder reports it; left to the tuner, the
    matrix simply keeps its column indices"""
    rng = np.random.default_rng(13)
    A = oracle.rand_rows(5000, 6, 21)              # random columns: every row its own shape
    B = oracle.rand_rows(400, 40, 22)              # rows of 40 entries
    for M in (A, B):
        sw("SPMV_MODE", "pat")
        s = cm.Solver.from_host_csr(ctx, M.rowptr, M.colidx, M.val, n_cols=M.m)
        with pytest.raises(cm.CudamatError):
            s.spmv_mode()
        s.close()
        sw("SPMV_MODE", None)
        x = rng.standard_normal(M.n)
        s = cm.Solver.from_host_csr(ctx, M.rowptr, M.colidx, M.val, n_cols=M.m)
        assert s.spmv_mode() != 3
        s.close()


def test_row_pattern_form_in_the_solver_loop_and_auto_selection(cm, ctx, oracle, sw):
    """a Poisson system beyond the fused small-system loops (400 000 rows): the tuner TIMES the row-pattern form against
    the compressed stream kernel and keeps the faster; whichever it is, and with the pattern form forced, the
    reference loop converges like the oracle's and returns its solution (fused dots, half-step test in the prologue)"""
    A = oracle.poisson5(1000, 400)
    xs = oracle.xstar(A.n, 5)
    b = oracle.spmv(A, xs)
    sw("VALUE_DICT", "0")
    s = cm.Solver.from_host_csr(ctx, A.rowptr, A.colidx, A.val)
    auto = s.spmv_kernel()
    assert auto.startswith("k_spmv_pat<") or auto.startswith("k_spmv_stream_c<"), auto
    s.close()
    ref = None
    for mode in ("csr", "pat"):
        sw("SPMV_MODE", mode)
        x, st, h = _solve_dev(cm, ctx, A, b, loop=cm.LOOP_PBICGSTAB, maxit=60, tol=0.0)
        assert st.iters == 60 and np.all(np.isfinite(h))
        # the residual the loop carries is the true residual of the iterate it returns (fused dots and the half-step test in
        # this form's prologue included)
        assert abs(np.linalg.norm(b - oracle.spmv(A, x)) - st.nrm) <= 1e-9 * st.nrm0
        if ref is None:
            ref = h
        else:
            # same products, same order inside every row; the dot partials are summed per workgroup in another grouping, and
            # BiCGSTAB amplifies that over the iterations: the first 20 residuals agree to 1e-9
            np.testing.assert_allclose(h[:20], ref[:20], rtol=1e-9)
    xo, so, ho = oracle.pbicgstab(A, b, maxit=60, tol=0.0, want_hist=True)
    np.testing.assert_allclose(h[:20], ho[:20], rtol=1e-8)


def test_device_memory_pool_recycles_and_trims():
    """csrc/pool.cpp: a freed block stays with the library and serves the next request of that size (no driver call: the
    device's free memory does not move, the address is the same); a larger request splits a free block; neighbours merge
    when freed; cudamat_pool_trim() hands everything back to the driver.  In a process of its own (tests/pool_check.py): what
    earlier tests left in this process's pool is not this test's business.  (Why a pool: DESIGN 6a -- a fresh hipMalloc costs
    up to 26 ms/GB on this platform once a process has allocated tens of GB.)"""
    import subprocess
    import sys
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "pool_check.py")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "pool_check ok" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])


def test_placed_blocked_copy_is_the_same_copy():
    """PB_PLACE (csrc/spmv_pb.hip, round 5): the product stream of a large blocked copy is cut out of a slab of device memory
    in a memory class of its own, values and indices out of another.  tests/place_check.py, in its own process: the placed copy
    gives bit-identical SpMV results to the unplaced one, the placement is reported, and close + trim return every byte."""
    import subprocess
    import sys
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "place_check.py")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "place_check ok" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
    lines = [l for l in r.stderr.splitlines() if "pb placement:" in l]
    assert len(lines) == 2 and all("slab" in l for l in lines), r.stderr[-3000:]          # the two PB_PLACE=1 builds, not the PB_PLACE=0 one
