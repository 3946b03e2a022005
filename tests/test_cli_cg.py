"""The `example` CLI's -K switch: conjugate gradients (CUDAMAT_LOOP_CG) through cg_lu_precond / cg of include/pbicgstab.h."""
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


def test_host_library_exports_the_cg_entry_points(built):
    syms = subprocess.run(["nm", "-DC", os.path.join(HOST, "libcuda_mat.so")], capture_output=True, text=True, check=True).stdout
    for want in ["cg(int, int, double*, int*, int*, double*, double*, double*, int, double, bool, double*, double*)",
                 "cg_lu_precond(int, int, double*, int*, int*, double*, double*, double*, int, double, bool, double*, double*)"]:
        assert " T " + want in syms, want


@pytest.mark.gpu
def test_cli_cg_solves_mat900(built):
    """-K on the reference's own usage line: ILU(0)-preconditioned CG (the default -C2), then without a preconditioner (-C1)
    with the trace of -D: exit status 0, "success", one trace line per iteration"""
    mat = "-M" + os.path.join(GOLD, "mat900.mtx")
    r = subprocess.run([built, mat, "-K", "-T1e-8", "-D"], capture_output=True, text=True)
    assert r.returncode == 0 and "nnz=7744" in r.stdout and "success" in r.stdout, r.stdout[-500:] + r.stderr[-500:]
    its_pc = int(re.search(r"iterations = (\d+)", r.stdout).group(1))
    assert "initial norm = " in r.stdout and "k = %d, norm = " % (its_pc - 1) in r.stdout and "k = %d," % its_pc not in r.stdout
    r = subprocess.run([built, mat, "-K", "-C1", "-T1e-8", "-D"], capture_output=True, text=True)
    assert r.returncode == 0 and "success" in r.stdout and "method failed" not in r.stderr, r.stdout[-500:] + r.stderr[-500:]
    its = int(re.search(r"iterations = (\d+)", r.stdout).group(1))
    assert "initial norm = " in r.stdout and "k = %d, norm = " % (its - 1) in r.stdout and "k = %d," % its not in r.stdout
    assert 0 < its_pc < its
