"""Several right-hand sides with ILU(0), without a GPU: the new entry points are declared and exported, the MANY_PRECOND switch
is in the table with `columns` as its default, and bicgstab_lu_precond_many checks its arrays before it touches a device."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cudamat_solver_precond_apply_many", "cudamat_solver_trsm_kernel")


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
    # the calls that carry `precond` keep their signatures
    assert re.search(r"cudamat_solver_solve_many\s*\(cudamat_solver \*s, int nrhs, const double \*B, int ldb, double \*X, "
                     r"int ldx, int precond,\s*int loop, int maxit, double tol, int flags, cudamat_stats \*st, int \*form\)", hdr)
    assert cm.lib().cudamat_version() == 1


def test_many_precond_switch(cm):
    L = cm.lib()
    for v in ("columns", "auto", "batched"):
        assert L.cudamat_option_check(b"MANY_PRECOND", v.encode()) == 0, v
        assert L.cudamat_option_check(b"CUDAMAT_MANY_PRECOND", v.encode()) == 0, v
    for v in ("", "batch", "1", "0", "COLUMNS", "column"):
        assert L.cudamat_option_check(b"MANY_PRECOND", v.encode()) == 2, v
    text = L.cudamat_options_help().decode()
    assert "CUDAMAT_MANY_PRECOND = columns | auto | batched" in text
    line = [t for t in text.splitlines() if t.startswith("CUDAMAT_MANY_PRECOND")][0]
    assert "default" in line and "MANY_FORM = columns" in line
    # the switch beside it is unchanged
    assert "CUDAMAT_MANY_FORM = auto | batched | columns" in text


def test_python_interface_is_there(cm):
    assert callable(cm.bicgstab_lu_precond_many)
    assert callable(cm.Solver.precond_apply_many) and callable(cm.Solver.trsm_kernel)


@pytest.mark.parametrize("bad", ["rowptr", "values", "colidx", "rows_of_B", "B_3d"])
def test_bicgstab_lu_precond_many_rejects_mismatched_sizes(cm, bad):
    """ValueError from the size checks -- raised before the library is asked for anything, so the same on a machine
    without a GPU (where a call that reached a device would raise CudamatError instead)"""
    n, nnz = 3, 3
    A, iA, jA = np.array([2.0, 3.0, 4.0]), np.array([0, 1, 2, 3], np.int32), np.array([0, 1, 2], np.int32)
    B = np.ones((n, 2))
    if bad == "rowptr":
        iA = iA[:-1]
    elif bad == "values":
        A = A[:-1]
    elif bad == "colidx":
        jA = jA[:-1]
    elif bad == "rows_of_B":
        B = np.ones((n + 1, 2))
    else:
        B = np.ones((n, 2, 1))
    with pytest.raises(ValueError):
        cm.bicgstab_lu_precond_many(n, nnz, A, iA, jA, B, 10, 1e-8)


def test_precond_apply_many_checks_arguments(cm):
    """CUDAMAT_ERR_ARG (2) for a NULL solver, on any machine"""
    L = cm.lib()
    assert L.cudamat_solver_precond_apply_many(None, 1, None, 1, None, 1) == 2
    assert L.cudamat_solver_trsm_kernel(None, 1, None, 0) == 2
