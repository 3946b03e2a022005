"""CUDAMAT_LOOP_BICGSTAB_L2 without a GPU: the numpy restatement of BiCGSTAB(2) (tests/bicgstab_l2_ref.py) that the GPU tests
compare against does what it is there for -- it converges on the two convection-dominated systems of tests/nondominant.py on
which the reference's BiCGSTAB does not, and on mat900 it finds the solution the reference program printed -- and the
constant of the new loop is the same in the C header and in the Python binding."""
import os
import re

import numpy as np
import pytest

from tests import bicgstab_l2_ref as R
from tests import nondominant as ND

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAXIT, TOL = 2000, 1e-8


@pytest.fixture(autouse=True)
def _serial_oracle(oracle):
    before = oracle.num_threads()
    oracle.set_num_threads(1)
    yield
    oracle.set_num_threads(before)


@pytest.mark.parametrize("name", ["convdiff_g8", "convdiff_g40"])
def test_restatement_converges_where_bicgstab_does_not(oracle, name):
    """x0 = 1, tol 1e-8: BiCGSTAB(2) converges with a true residual within 2 tol ||r_init||; the oracle's pbicgstab2 (the
    reference's loop of pbicgstab.cu:581-754) on the same system does not converge within the same 2000 iterations"""
    O = oracle
    A, b = ND.FAMILY[name](O)
    mv, _ = R.oracle_ops(O, A)
    r = R.bicgstab_l2(mv, b, maxit=MAXIT, tol=TOL)
    tr = ND.true_res(O, A, b, r.x)
    ok, xo, so = O.pbicgstab2(A, b, maxit=MAXIT, tol=TOL)
    print(name, "BiCGSTAB(2): sweeps", r.iters, "products", 4 * r.iters + 1, "true residual / ||r_init||", tr / r.nrm0,
          "| pbicgstab2: iters", so.iters, "converged", so.converged, "breakdown", so.breakdown, "nrm / nrm0", so.nrm / so.nrm0)
    assert r.converged and not r.breakdown and len(r.hist) == r.iters
    assert tr <= 2.0 * TOL * r.nrm0
    assert not ok and not so.converged


@pytest.mark.parametrize("rhs", ["sin", "urand"])
def test_restatement_finds_the_reference_programs_solution_on_mat900(oracle, golden_dir, rhs):
    """tests/golden/bicg_mat900_*.npz: the solution the unmodified reference CPU program printed with 6 digits at its eps of
    1e-6 -- the bound tests/test_gpu_parity.py holds the HIP BiCGSTAB solution to (2e-5: print precision + that eps)"""
    O = oracle
    g = np.load(os.path.join(golden_dir, "bicg_mat900_%s.npz" % rhs))
    A = O.mtx_load(os.path.join(golden_dir, "mat900.mtx"))
    mv, _ = R.oracle_ops(O, A)
    r = R.bicgstab_l2(mv, g["b"], maxit=MAXIT, tol=TOL)
    err = np.linalg.norm(r.x - g["x"]) / np.linalg.norm(g["x"])
    print("mat900", rhs, "sweeps", r.iters, "relative distance to the printed solution", err)
    assert r.converged
    assert ND.true_res(O, A, g["b"], r.x) <= 2.0 * TOL * r.nrm0
    assert err <= 2e-5


def test_restatement_preconditioned_and_shifted(oracle, golden_dir):
    """right preconditioning with the oracle's ILU(0) (x = x0 + M^-1 y) and a shift d: the true residual of the operator
    A0 + diag(d) is within 2 tol ||r_init||, in fewer sweeps than without M^-1"""
    O = oracle
    A = O.mtx_load(os.path.join(golden_dir, "mat900.mtx"))
    b = O.spmv(A, 1.0 + np.sin(np.arange(A.n)))
    mv, minv = R.oracle_ops(O, A, O.ilu0(A))
    plain, pc = R.bicgstab_l2(mv, b, maxit=MAXIT, tol=TOL), R.bicgstab_l2(mv, b, minv=minv, maxit=MAXIT, tol=TOL)
    assert plain.converged and pc.converged and pc.iters < plain.iters
    assert ND.true_res(O, A, b, pc.x) <= 2.0 * TOL * pc.nrm0
    d = 0.5 + np.arange(A.n) / A.n
    bd = b + d * (1.0 + np.sin(np.arange(A.n)))
    sh = R.bicgstab_l2(mv, bd, d=d, maxit=MAXIT, tol=TOL)
    assert sh.converged and np.linalg.norm(bd - (O.spmv(A, sh.x) + d * sh.x)) <= 2.0 * TOL * sh.nrm0


def test_restatement_reports_a_breakdown():
    """A = [[0, 1], [1, 0]], b = (1, 0), x0 = 0: gamma = u1.r~ = 0 in the first sweep"""
    A = np.array([[0.0, 1.0], [1.0, 0.0]])
    r = R.bicgstab_l2(lambda v: A @ v, np.array([1.0, 0.0]), x0=np.zeros(2), maxit=10, tol=TOL)
    assert r.breakdown and not r.converged and r.iters == 0 and len(r.hist) == 0


def test_loop_constant_agrees_between_header_and_binding():
    from cuda_mat_amd import _lib
    import cuda_mat_amd as cm
    assert _lib.LOOP_BICGSTAB_L2 == 3 and cm.LOOP_BICGSTAB_L2 == 3
    hdr = open(os.path.join(ROOT, "include", "cudamat.h")).read()
    loops = {name: int(v) for name, v in re.findall(r"^#define\s+CUDAMAT_(LOOP_[A-Z0-9_]+)\s+(\d+)", hdr, re.M)}
    assert loops == {"LOOP_PBICGSTAB": 0, "LOOP_PBICGSTAB2": 1, "LOOP_PIPELINED": 2, "LOOP_BICGSTAB_L2": 3}
    for name, v in loops.items():
        assert getattr(_lib, name) == v, name
    # ... and the C++ and Python entry points of the new loop exist beside the others
    pb = open(os.path.join(ROOT, "include", "pbicgstab.h")).read()
    assert "bool bicgstab_l2(" in pb and "bool bicgstab_l2_lu_precond(" in pb
    assert callable(cm.bicgstab_l2) and callable(cm.bicgstab_l2_lu_precond)
