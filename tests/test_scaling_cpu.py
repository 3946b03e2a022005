"""Power-of-two scale equivariance of the CPU oracle: what tests/test_gpu_scaling.py asks of the HIP loops, the reference's
restatement satisfies first.

BiCGSTAB is exactly equivariant under c = 2^k: with (b, x0) -> (c b, c x0) every vector of the loop is c times what it
was and every dot product c^2 times, so alpha, omega and beta keep their bits (a power of two commutes with rounding
while nothing overflows or goes subnormal); with A -> c A, x0 -> x0 / c and b unchanged the residual-side vectors keep
their bits and the solution-side ones are divided by c.  So x and the written part of the residual history are c (or
1 / c) times the unscaled ones BITWISE, after the same number of iterations through the same exit.  The exponents are the
ones the GPU tests use; the systems are theirs too.  No GPU."""
import os

import numpy as np
import pytest

RHS_EXPONENTS = (-440, -200, -40, 40, 200, 440)
MAT_EXPONENTS = (-200, -40, 40, 200)


@pytest.fixture(autouse=True)
def _serial_oracle(oracle):
    before = oracle.num_threads()
    oracle.set_num_threads(1)          # one fixed summation order (the property does not need it; the comparison of runs does)
    yield
    oracle.set_num_threads(before)


@pytest.fixture(scope="module")
def systems(oracle, golden_dir):
    """name -> (A, b = A (1 + sin i), x0 = 1): built once, read-only"""
    out = {}
    for name in ("mat900", "mat10000", "rand20000x50", "poisson40x30", "poisson459x459"):
        if name == "rand20000x50":
            A = oracle.rand_rows(20000, 50, 0x5EED)
        elif name.startswith("poisson"):
            A = oracle.poisson5(*[int(t) for t in name[7:].split("x")])
        else:
            A = oracle.mtx_load(os.path.join(golden_dir, name + ".mtx"))
        out[name] = (A, oracle.spmv(A, 1.0 + np.sin(np.arange(A.n))), np.ones(A.n))
    from tests.test_gpu_parity import _soak_case          # (the system on which the pipelined loop drifts without replacement)
    A, _, b = _soak_case(oracle, 21, 41)
    out["soak21_41"] = (A, b, np.ones(A.n))
    return out


def _scaled_matrix(oracle, A, c):
    return oracle.Csr(A.n, A.rowptr, A.colidx, A.val * c, A.m)


def _same_up_to(c, got, ref):
    """(x, stats, history) of the scaled run against the unscaled one: bitwise c times it"""
    (xc, stc, hc), (x, st, h) = got, ref
    assert (stc.iters, bool(stc.half_exit), bool(stc.converged), bool(stc.breakdown)) == \
           (st.iters, bool(st.half_exit), bool(st.converged), bool(st.breakdown))
    np.testing.assert_array_equal(xc, c * x)
    written = ~np.isnan(h)
    np.testing.assert_array_equal(np.isnan(hc), ~written)
    np.testing.assert_array_equal(hc[written], c * h[written])
    return written.sum()


def _run(oracle, config, A, b, x0, d=None, vm=None, maxit=2000):
    """one oracle loop, (x, stats, history)"""
    if config in ("pbicgstab", "pbicgstab_ilu0"):
        return oracle.pbicgstab(A, b, x0=x0, vm=vm, maxit=maxit, tol=1e-8, want_hist=True)
    if config in ("pbicgstab2", "pbicgstab2_d"):
        ok, x, st, h = oracle.pbicgstab2(A, b, d=d, x0=x0, maxit=maxit, tol=1e-8, want_hist=True)
        assert ok == bool(st.converged)
        return x, st, h
    # verify=False: the loop alone (the verification wrapper of oracle.py takes numpy's norm of the true residual, a scaled
    # BLAS routine with no claim to equivariance; the product's restart computes its norm with the loop's own kernels)
    rr = {"pipelined": None, "pipelined_ilu0": None, "pipelined_rr4": 4, "pipelined_rr0": 0}[config]
    return oracle.pipelined_bicgstab(A, b, x0=x0, vm=vm, maxit=maxit, tol=1e-8, want_hist=True, verify=False, rr=rr)


# (configuration, system, maxit): the loops the GPU file runs, on the systems it runs them on
CONFIGS = [
    ("pbicgstab", "mat900", 2000),
    ("pbicgstab", "mat10000", 10),
    ("pbicgstab", "poisson40x30", 10),
    ("pbicgstab", "poisson459x459", 10),          # (the grid of the GPU file's value-dictionary forms)
    ("pbicgstab2", "mat900", 2000),
    ("pbicgstab2_d", "mat900", 2000),
    ("pbicgstab_ilu0", "mat900", 2000),
    ("pbicgstab_ilu0", "mat10000", 10),
    ("pbicgstab_ilu0", "rand20000x50", 10),
    ("pipelined", "mat900", 2000),
    ("pipelined_ilu0", "mat900", 2000),
    ("pipelined_rr4", "mat900", 2000),
    ("pipelined_rr0", "soak21_41", 1000),
]


@pytest.mark.parametrize("config,name,maxit", CONFIGS)
def test_oracle_is_equivariant_under_rhs_scaling(oracle, systems, config, name, maxit):
    """(c b, c x0) gives c x and c times the history, bit for bit, at every exponent the GPU tests use"""
    A, b, x0 = systems[name]
    d = 0.5 + np.random.default_rng(5).random(A.n) if config == "pbicgstab2_d" else None
    vm = oracle.ilu0(A) if config.endswith("ilu0") else None
    ref = _run(oracle, config, A, b, x0, d=d, vm=vm, maxit=maxit)
    assert ref[1].iters > 0 and (ref[1].converged or maxit == 10)
    if config == "pipelined_rr4":
        assert ref[1].iters > 4                       # a residual replacement happened within the solve
    for k in RHS_EXPONENTS:
        c = 2.0 ** k
        got = _run(oracle, config, A, c * b, c * x0, d=d, vm=vm, maxit=maxit)
        assert _same_up_to(c, got, ref) > 0
        assert got[1].nrm0 == c * ref[1].nrm0


@pytest.mark.parametrize("config,name,maxit", [c for c in CONFIGS if c[1] in ("mat900", "rand20000x50")])
def test_oracle_is_equivariant_under_matrix_scaling(oracle, systems, config, name, maxit):
    """(2^k A, b, 2^-k x0) gives 2^-k x and the same history, bit for bit; the ILU(0) factors of 2^k A are L and 2^k U"""
    A, b, x0 = systems[name]
    d = 0.5 + np.random.default_rng(5).random(A.n) if config == "pbicgstab2_d" else None
    vm = oracle.ilu0(A) if config.endswith("ilu0") else None
    ref = _run(oracle, config, A, b, x0, d=d, vm=vm, maxit=maxit)
    # gpu_pbicgstab2's guard |omega| < 1e-5 (pbicgstab.cu:735) is absolute in omega, which scales with 1 / A: its loops
    # keep to k = +-10, where omega (of order 1 / ||A||, here 0.1 to 1) stays far above the guard
    exps = (-10, 10) if config.startswith("pbicgstab2") else MAT_EXPONENTS
    for k in exps:
        c = 2.0 ** k
        Ac = _scaled_matrix(oracle, A, c)
        vmc = oracle.ilu0(Ac) if vm is not None else None
        got = _run(oracle, config, Ac, b, x0 / c, d=None if d is None else c * d, vm=vmc, maxit=maxit)
        xc, stc, hc = got
        _same_up_to(1.0, (xc * c, stc, hc), ref)
        assert stc.nrm0 == ref[1].nrm0


@pytest.mark.parametrize("name", ["mat900", "mat10000", "rand20000x50"])
def test_oracle_ilu0_factors_scale_with_the_matrix(oracle, systems, name):
    """ILU(0) of 2^k A: the entries of L (unit lower, l_ij = a_ij / u_jj) keep their bits, those of U are 2^k times U's"""
    A = systems[name][0]
    vm = oracle.ilu0(A)
    base = int(A.rowptr[0])
    rows = np.repeat(np.arange(A.n), np.diff(A.rowptr))
    lower = (A.colidx - base) < rows
    for k in MAT_EXPONENTS:
        c = 2.0 ** k
        vmc = oracle.ilu0(_scaled_matrix(oracle, A, c))
        np.testing.assert_array_equal(vmc[lower], vm[lower])
        np.testing.assert_array_equal(vmc[~lower], c * vm[~lower])


def test_oracle_shares_the_plain_sum_at_the_range_edges(oracle, systems):
    """what the product deliberately does NOT copy: the oracle's norm is a plain sqrt(sum r^2) too (the reference's
    cublasDnrm2 is scaled), so at 2^520 its ||r0|| is inf and it spins to maxit, at 2^-600 its ||r0|| is 0, and at 2^-520
    (squares in the subnormal range) it 'converges' early.  The product refuses these three instead
    (tests/test_gpu_scaling.py)."""
    A, b, x0 = systems["mat900"]
    x, st, h = oracle.pbicgstab(A, b, x0=x0, maxit=2000, tol=1e-8, want_hist=True)
    c = 2.0 ** 520
    xc, stc = oracle.pbicgstab(A, c * b, x0=c * x0, maxit=60, tol=1e-8)
    assert stc.nrm0 == np.inf and not stc.converged and stc.iters == 60
    c = 2.0 ** -600
    xc, stc = oracle.pbicgstab(A, c * b, x0=c * x0, maxit=60, tol=1e-8)
    assert stc.nrm0 == 0.0
    c = 2.0 ** -520
    xc, stc = oracle.pbicgstab(A, c * b, x0=c * x0, maxit=2000, tol=1e-8)
    assert stc.converged and stc.iters < st.iters            # a success it has not computed
