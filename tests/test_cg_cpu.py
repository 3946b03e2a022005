"""CUDAMAT_LOOP_CG without a GPU: the constants of the new loop are the same in the C headers and in the Python binding, and the
numpy restatement of conjugate gradients (tests/cg_ref.py) that the GPU tests compare against does what it is there for -- on
the two symmetric positive definite fixtures it converges to the solutions the reference's CPU program (BiCG, which on a
symmetric matrix is CG) printed, and on a negative definite matrix it reports the breakdown at once."""
import os
import subprocess

import numpy as np
import pytest

from tests import bicgstab_l2_ref as R2
from tests import cg_ref as R
from tests import nondominant as ND

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAXIT, TOL = 2000, 1e-8


@pytest.fixture(autouse=True)
def _serial_oracle(oracle):
    before = oracle.num_threads()
    oracle.set_num_threads(1)
    yield
    oracle.set_num_threads(before)


def test_constants_agree_between_the_compiled_header_and_the_binding(tmp_path):
    """what the C compiler makes of include/cudamat.h (which includes cudamat_cg.h) against cuda_mat_amd/_lib.py"""
    import cuda_mat_amd as cm
    from cuda_mat_amd import _lib
    names = ["LOOP_PBICGSTAB", "LOOP_PBICGSTAB2", "LOOP_PIPELINED", "LOOP_BICGSTAB_L2", "LOOP_CG", "FLAG_DEBUG", "FLAG_PROFILE",
             "FLAG_NO_EXIT", "FLAG_X0_ONES", "FLAG_GUARD", "FLAG_ASSUME_SYMMETRIC"]
    src = ['#include <stdio.h>', '#include "cudamat.h"', 'int main(void){']
    src += ['printf("%s %%d\\n", CUDAMAT_%s);' % (k, k) for k in names]
    src.append('return 0;}')
    (tmp_path / "c.c").write_text("\n".join(src))
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "c"), str(tmp_path / "c.c")], check=True)
    out = subprocess.run([str(tmp_path / "c")], check=True, capture_output=True, text=True).stdout
    got = {k: int(v) for k, v in (line.split() for line in out.splitlines())}
    assert got["LOOP_CG"] == 8 and got["FLAG_ASSUME_SYMMETRIC"] == 32
    for k in names:
        assert getattr(_lib, k) == got[k], k
        assert getattr(cm, k) == got[k], k
    flags = [v for k, v in got.items() if k.startswith("FLAG_")]
    assert all(v & (v - 1) == 0 for v in flags) and len(set(flags)) == len(flags)
    assert len({v for k, v in got.items() if k.startswith("LOOP_")}) == 5


def test_entry_points_exist_at_every_layer():
    import ctypes as C
    import cuda_mat_amd as cm
    from cuda_mat_amd import _lib
    pb = open(os.path.join(ROOT, "include", "pbicgstab.h")).read()
    assert "bool cg(" in pb and "bool cg_lu_precond(" in pb
    assert callable(cm.cg) and callable(cm.cg_lu_precond) and callable(cm.Solver.symmetry)
    assert _lib._SIGS["cudamat_solver_symmetry"] == (C.c_int, [C.c_void_p, C.POINTER(C.c_longlong), C.POINTER(C.c_double)])
    assert hasattr(cm.lib(), "cudamat_solver_symmetry")


CASES = [("mat900", "sin", "bicg_mat900_sin"), ("mat900", "urand", "bicg_mat900_urand"), ("mat10000", "sin", "bicg_mat10000_sin")]


@pytest.mark.parametrize("mat,rhs,gold", CASES)
@pytest.mark.parametrize("pc", [0, 1])
def test_restatement_finds_the_reference_programs_solution(oracle, golden_dir, mat, rhs, gold, pc):
    """x0 = 1, tol 1e-8, without and with the oracle's ILU(0): converged, true residual <= 2 tol ||r0||, x within 1e-5 of the
    solution the reference CPU program printed"""
    O = oracle
    g = np.load(os.path.join(golden_dir, gold + ".npz"))
    A = O.mtx_load(os.path.join(golden_dir, mat + ".mtx"))
    b = g["b"]
    if rhs == "sin":
        np.testing.assert_array_equal(b, O.spmv(A, 1.0 + np.sin(np.arange(A.n))))
    mv, minv = R2.oracle_ops(O, A, O.ilu0(A) if pc else None)
    r = R.cg(mv, b, minv=minv, maxit=MAXIT, tol=TOL)
    err = np.linalg.norm(r.x - g["x"]) / np.linalg.norm(g["x"])
    tr = ND.true_res(O, A, b, r.x)
    print(mat, rhs, "ILU(0)" if pc else "M = I", "iterations", r.iters, "true residual / ||r0||", tr / r.nrm0,
          "distance to the printed solution", err)
    assert r.converged and not r.breakdown and len(r.hist) == r.iters
    assert r.hist[-1] < TOL * r.nrm0 and np.all(r.hist[:-1] >= TOL * r.nrm0)
    assert tr <= 2.0 * TOL * r.nrm0
    assert err <= 1e-5


def test_restatement_with_ilu0_takes_fewer_iterations(oracle, golden_dir):
    O = oracle
    A = O.mtx_load(os.path.join(golden_dir, "mat10000.mtx"))
    b = O.spmv(A, 1.0 + np.sin(np.arange(A.n)))
    mv, minv = R2.oracle_ops(O, A, O.ilu0(A))
    plain, pc = R.cg(mv, b, maxit=MAXIT, tol=TOL), R.cg(mv, b, minv=minv, maxit=MAXIT, tol=TOL)
    print("mat10000: iterations", plain.iters, "with ILU(0)", pc.iters)
    assert plain.converged and pc.converged and pc.iters < plain.iters


def test_restatement_with_a_shift(oracle, golden_dir):
    O = oracle
    A = O.mtx_load(os.path.join(golden_dir, "mat900.mtx"))
    n = A.n
    d = 0.5 + np.arange(n) / n
    xs = 1.0 + np.sin(np.arange(n))
    b = O.spmv(A, xs) + d * xs
    mv, _ = R2.oracle_ops(O, A)
    r = R.cg(mv, b, d=d, maxit=MAXIT, tol=TOL)
    assert r.converged and np.linalg.norm(b - (O.spmv(A, r.x) + d * r.x)) <= 2.0 * TOL * r.nrm0


def test_restatement_reports_a_matrix_that_is_not_positive_definite(oracle, golden_dir):
    """A - 17 I is negative definite (mat900's spectrum lies in (0.06, 11.96); Gershgorin bound 16): gamma = p.Ap < 0 in
    iteration 0 -- breakdown, no iteration counted, x untouched; under no_exit the same solve runs its 5 iterations"""
    O = oracle
    A = O.mtx_load(os.path.join(golden_dir, "mat900.mtx"))
    S = A.to_scipy()
    assert abs(S).sum(axis=1).max() <= 16.0
    b = O.spmv(A, 1.0 + np.sin(np.arange(A.n)))
    mv, _ = R2.oracle_ops(O, A)
    d = np.full(A.n, -17.0)
    r = R.cg(mv, b, d=d, maxit=5, tol=TOL)
    assert (r.breakdown, r.converged, r.iters, len(r.hist)) == (1, 0, 0, 0)
    np.testing.assert_array_equal(r.x, np.ones(A.n))
    r = R.cg(mv, b, d=d, maxit=5, tol=TOL, no_exit=True)
    assert (r.breakdown, r.converged, r.iters, len(r.hist)) == (0, 0, 5, 5)
