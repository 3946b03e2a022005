"""New values on the kept structure without a GPU: the two entry points are in the built library, in the header and in the
binding; they refuse a missing solver before they look for a device; the drop-in call's switch VALUES_REFRESH is in the one
table; Solver has both methods.  The GPU side is tests/test_gpu_set_values.py."""
import ctypes as C
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = 2


@pytest.fixture(scope="module")
def L():
    import cuda_mat_amd as cm
    return cm.lib()


def test_the_two_symbols_exist(L):
    from cuda_mat_amd import _lib
    raw = C.CDLL(_lib.LIB_PATH)
    for name in ("cudamat_solver_set_values", "cudamat_solver_set_values_info"):
        assert hasattr(raw, name), name
    hdr = open(os.path.join(ROOT, "include", "cudamat.h")).read()
    assert re.search(r"int\s+cudamat_solver_set_values\s*\(\s*cudamat_solver\s*\*\s*s\s*,\s*const\s+double\s*\*\s*val\s*\)\s*;", hdr)
    assert re.search(r"int\s+cudamat_solver_set_values_info\s*\(\s*cudamat_solver\s*\*\s*s\s*,\s*int\s*\*\s*count\s*,\s*double\s*\*\s*seconds_last\s*,"
                     r"\s*size_t\s*\*\s*map_bytes\s*,\s*int\s*\*\s*rebuilt_last\s*\)\s*;", hdr)
    assert _lib._SIGS["cudamat_solver_set_values"] == (C.c_int, [C.c_void_p, C.c_void_p])
    assert _lib._SIGS["cudamat_solver_set_values_info"] == (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_double),
                                                                      C.POINTER(C.c_size_t), C.POINTER(C.c_int)])


def test_a_missing_solver_is_refused_without_a_device(L):
    assert L.cudamat_solver_set_values(None, None) == ERR_ARG
    assert "solver is NULL" in L.cudamat_last_error().decode()
    cnt, sec, nb, reb = C.c_int(7), C.c_double(7.0), C.c_size_t(7), C.c_int(7)
    assert L.cudamat_solver_set_values_info(None, C.byref(cnt), C.byref(sec), C.byref(nb), C.byref(reb)) == ERR_ARG
    assert "solver is NULL" in L.cudamat_last_error().decode()
    assert (cnt.value, sec.value, nb.value, reb.value) == (7, 7.0, 7, 7)          # nothing was written


def test_the_switch_is_in_the_table(L):
    assert L.cudamat_option_check(b"VALUES_REFRESH", b"0") == 0
    assert L.cudamat_option_check(b"VALUES_REFRESH", b"1") == 0
    assert L.cudamat_option_check(b"CUDAMAT_VALUES_REFRESH", b"1") == 0
    assert L.cudamat_option_check(b"VALUES_REFRESH", b"2") != 0
    assert "VALUES_REFRESH" in L.cudamat_last_error().decode()
    text = L.cudamat_options_help().decode()
    assert re.search(r"^CUDAMAT_VALUES_REFRESH = 0 \| 1 ", text, re.M)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "VALUES_REFRESH" in design


def test_python_layer_has_both_methods():
    from cuda_mat_amd import api
    assert list(inspect.signature(api.Solver.set_values).parameters) == ["self", "val"]
    assert list(inspect.signature(api.Solver.set_values_info).parameters) == ["self"]
