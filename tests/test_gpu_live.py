"""Every struct of the library frees what it owns (csrc/owned.h): after a walk through the allocating paths, with every
solver destroyed and the plan cache cleared, cudamat_mem_live reads what it read before."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.gpu
@pytest.mark.parametrize("pool", ["1", "0"])
def test_every_allocation_is_freed_with_its_owner(pool):
    """tests/live_check.py in a process of its own (the pool's switch is read once per process): SpMV forms, loop forms,
    ILU(0) three ways, batched solves that regrow, the collective path at world size 1, the host-pointer entry point and
    three failing set-ups; then the count of live allocations is EQUAL to the one before, and a trimmed pool is empty."""
    env = dict(os.environ, CUDAMAT_POOL=pool)
    r = subprocess.run([sys.executable, os.path.join(HERE, "live_check.py")], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "live_check ok" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
