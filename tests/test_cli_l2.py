"""The `example` CLI's -L switch: BiCGSTAB(2) (CUDAMAT_LOOP_BICGSTAB_L2) through bicgstab_l2_lu_precond / bicgstab_l2 of
include/pbicgstab.h."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "cuda_mat_amd", "host")
GOLD = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def built():
    import cuda_mat_amd
    cuda_mat_amd.lib()
    subprocess.run(["make", "-C", HOST], check=True, capture_output=True)
    return os.path.join(HOST, "example")


def test_host_library_exports_the_l2_entry_points(built):
    syms = subprocess.run(["nm", "-DC", os.path.join(HOST, "libcuda_mat.so")], capture_output=True, text=True, check=True).stdout
    for want in ["bicgstab_l2(int, int, double*, int*, int*, double*, double*, double*, int, double, bool, double*, double*)",
                 "bicgstab_l2_lu_precond(int, int, double*, int*, int*, double*, double*, double*, int, double, bool, double*, double*)"]:
        assert " T " + want in syms, want


@pytest.mark.gpu
def test_cli_l2_solves_mat10000(built):
    """-L on the reference's own usage line: ILU(0)-preconditioned BiCGSTAB(2) (the default -C2), then without a
    preconditioner (-C0) with the trace of -D: exit status 0, "success", one trace line per sweep"""
    mat = "-M" + os.path.join(GOLD, "mat10000.mtx")
    r = subprocess.run([built, mat, "-L"], capture_output=True, text=True)
    assert r.returncode == 0 and "nnz=49600" in r.stdout and "success" in r.stdout, r.stdout[-500:] + r.stderr[-500:]
    sweeps_pc = int(re.search(r"iterations = (\d+)", r.stdout).group(1))
    r = subprocess.run([built, mat, "-L", "-C0", "-T1e-8", "-D"], capture_output=True, text=True)
    assert r.returncode == 0 and "success" in r.stdout and "method failed" not in r.stderr, r.stdout[-500:] + r.stderr[-500:]
    sweeps = int(re.search(r"iterations = (\d+)", r.stdout).group(1))
    assert "initial norm = " in r.stdout and "sweep = %d, norm = " % (sweeps - 1) in r.stdout and "sweep = %d," % sweeps not in r.stdout
    assert 0 < sweeps_pc < sweeps
