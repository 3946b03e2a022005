"""One set of ILU(0) factors per column, (A0 + I d_j) x_j = b_j with M_j = ILU(0)(A0 + diag d_j), without a GPU: the new entry
points are declared and exported, cudamat_solve_shifts_ilu0 checks its arguments before it touches a device, and
bicgstab_d_lu_precond_many refuses a D of the wrong shape in Python and fails loudly without a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cudamat_solver_solve_shifts_ilu0", "cudamat_solver_precond_apply_shifts", "cudamat_solver_ilu0_shifts_values",
       "cudamat_solve_shifts_ilu0")


@pytest.fixture(scope="module")
def cm():
    import cuda_mat_amd as cm
    cm.lib()
    return cm


def test_new_symbols_declared_and_exported(cm):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cudamat.h")).read(), flags=re.S)
    from cuda_mat_amd import _lib
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib._SIGS and hasattr(cm.lib(), name), name
    assert callable(cm.bicgstab_d_lu_precond_many)
    for method in ("solve_shifts_ilu0", "precond_apply_shifts", "ilu0_shifts_values"):
        assert hasattr(cm.Solver, method), method


def _call(cm, nrhs, D, ldd, B, ldb, X, ldx, n=2):
    val = np.array([2.0, 3.0])
    rp = np.array([0, 1, 2], np.int32)
    ci = np.array([0, 1], np.int32)
    st = (cm.Stats * 4)()
    form = C.c_int(-1)
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)   # noqa: E731
    rc = cm.lib().cudamat_solve_shifts_ilu0(n, 2, vp(val), vp(rp), vp(ci), nrhs, vp(D), ldd, vp(B), ldb, None, vp(X), ldx, 10, 1e-8,
                                            st, C.byref(form))
    return rc, form.value


def test_solve_shifts_ilu0_checks_arguments_before_the_device(cm):
    """CUDAMAT_ERR_ARG (2) for every malformed call, also on a machine without a GPU (where any device work would fail with
    CUDAMAT_ERR_HIP = 1); nrhs = 0 is a successful no-op with form 0"""
    D, B, X = np.ones(8), np.ones(8), np.zeros(8)
    assert _call(cm, -1, D, 2, B, 2, X, 2)[0] == 2
    assert _call(cm, 2, D, 1, B, 2, X, 2)[0] == 2          # ldd < n
    assert _call(cm, 2, D, 2, B, 1, X, 2)[0] == 2          # ldb < n
    assert _call(cm, 2, D, 2, B, 2, X, 1)[0] == 2          # ldx < n
    assert _call(cm, 2, D, 2, None, 2, X, 2)[0] == 2
    assert _call(cm, 2, D, 2, B, 2, None, 2)[0] == 2
    assert _call(cm, 2, None, 2, B, 2, X, 2)[0] == 2       # the shifts are not optional here
    np.testing.assert_array_equal(X, np.zeros(8))
    assert _call(cm, 0, None, 2, None, 2, None, 2) == (0, 0)


def test_bicgstab_d_lu_precond_many_refuses_a_d_of_the_wrong_shape(cm):
    """D is (n, k) or k scalars; anything else is a ValueError raised in Python, before the library is called"""
    A = np.array([2.0, 3.0]), np.array([0, 1, 2], np.int32), np.array([0, 1], np.int32)
    B = np.ones((2, 3))
    for D in (np.ones((2, 2)), np.ones((3, 3)), np.ones(4), np.ones((2, 3, 1)), 1.0):
        with pytest.raises(ValueError):
            cm.bicgstab_d_lu_precond_many(2, 2, A[0], A[1], A[2], D, None, B, 10, 1e-8)
    with pytest.raises(ValueError):                        # x0 of the wrong size
        cm.bicgstab_d_lu_precond_many(2, 2, A[0], A[1], A[2], np.ones((2, 3)), np.ones(5), B, 10, 1e-8)


def test_bicgstab_d_lu_precond_many_fails_loudly_without_gpu(cm):
    if cm.device_count() > 0:
        pytest.skip("a GPU is present")
    A = np.array([2.0]), np.array([0, 1], np.int32), np.array([0], np.int32)
    with pytest.raises(cm.CudamatError):
        cm.bicgstab_d_lu_precond_many(1, 1, A[0], A[1], A[2], np.ones((1, 3)), None, np.ones((1, 3)), 10, 1e-8)
    with pytest.raises(cm.CudamatError):
        cm.bicgstab_d_lu_precond_many(1, 1, A[0], A[1], A[2], np.array([1.0, 2.0, 3.0]), None, np.ones((1, 3)), 10, 1e-8)
