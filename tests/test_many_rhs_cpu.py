"""Several right-hand sides, without a GPU: the new entry points are declared and exported, the MANY_FORM switch is in the
table, cudamat_solve_many checks its arguments before it touches a device, and bicgstab_many fails loudly without one."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cudamat_solver_spmm", "cudamat_solver_solve_many", "cudamat_solver_history_col", "cudamat_solve_many")


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
    assert cm.lib().cudamat_version() == 1


def test_many_form_switch(cm):
    L = cm.lib()
    for v in ("auto", "batched", "columns"):
        assert L.cudamat_option_check(b"MANY_FORM", v.encode()) == 0, v
    for v in ("", "batch", "1", "AUTO"):
        assert L.cudamat_option_check(b"MANY_FORM", v.encode()) == 2, v
    assert "CUDAMAT_MANY_FORM = auto | batched | columns" in L.cudamat_options_help().decode()


def _call(cm, nrhs, B, ldb, X, ldx, n=2):
    val = np.array([2.0, 3.0])
    rp = np.array([0, 1, 2], np.int32)
    ci = np.array([0, 1], np.int32)
    st = (cm.Stats * 4)()
    form = C.c_int(-1)
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)   # noqa: E731
    rc = cm.lib().cudamat_solve_many(n, 2, vp(val), vp(rp), vp(ci), None, nrhs, vp(B), ldb, None, vp(X), ldx, 0, 1, 10, 1e-8,
                                     st, C.byref(form))
    return rc, form.value


def test_solve_many_checks_arguments_before_the_device(cm):
    """CUDAMAT_ERR_ARG (2) for every malformed call, also on a machine without a GPU (where any device work would fail with
    CUDAMAT_ERR_HIP = 1); nrhs = 0 is a successful no-op"""
    B, X = np.ones(8), np.zeros(8)
    assert _call(cm, -1, B, 2, X, 2)[0] == 2
    assert _call(cm, 2, B, 1, X, 2)[0] == 2
    assert _call(cm, 2, B, 2, X, 1)[0] == 2
    assert _call(cm, 2, None, 2, X, 2)[0] == 2
    assert _call(cm, 2, B, 2, None, 2)[0] == 2
    assert _call(cm, 0, None, 2, None, 2) == (0, 0)


def test_bicgstab_many_fails_loudly_without_gpu(cm):
    if cm.device_count() > 0:
        pytest.skip("a GPU is present")
    A = np.array([2.0]), np.array([0, 1], np.int32), np.array([0], np.int32)
    with pytest.raises(cm.CudamatError):
        cm.bicgstab_many(1, 1, A[0], A[1], A[2], np.ones((1, 3)), 10, 1e-8)
