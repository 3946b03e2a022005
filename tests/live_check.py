"""Run by tests/test_gpu_live.py in a process of its own: every path that allocates device memory is walked, every solver
is destroyed, and cudamat_mem_live must read exactly what it read before the walk -- each struct frees what it owns
(csrc/owned.h, csrc/devmem.h).  The pool is on or off (CUDAMAT_POOL=0) as the parent's environment says."""
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cuda_mat_amd as cm  # noqa: E402

ERR_ARG, ERR_ZERO_PIVOT = 2, 3
NX = 64
N = NX * NX


def stencil(drop_diag_of=None):
    """5-point stencil on an NX x NX grid, 0-based CSR with increasing columns; drop_diag_of: that row loses its diagonal"""
    rp, ci, va = [0], [], []
    for i in range(N):
        x, y = i % NX, i // NX
        for j, v, ok in ((i - NX, -1.0, y > 0), (i - 1, -1.0, x > 0), (i, 4.0, i != drop_diag_of), (i + 1, -1.0, x < NX - 1),
                         (i + NX, -1.0, y < NX - 1)):
            if ok:
                ci.append(j)
                va.append(v)
        rp.append(len(ci))
    return np.array(rp, np.int32), np.array(ci, np.int32), np.array(va)


def scattered():
    """16 distinct columns per row, the diagonal among them: mean row length above 12, where SPMV_FORM=tiles applies"""
    rng = np.random.default_rng(7)
    ci = np.empty((N, 16), np.int32)
    for i in range(N):
        c = rng.choice(N - 1, 15, replace=False)
        c[c >= i] += 1
        ci[i] = np.sort(np.append(c, i))
    va = np.where(ci == np.arange(N)[:, None], 20.0, rng.uniform(-1.0, 1.0, (N, 16)))
    return np.arange(0, 16 * N + 1, 16, dtype=np.int32), ci.ravel(), va.ravel()


def live():
    v = C.c_size_t()
    assert cm.lib().cudamat_mem_live(C.byref(v)) == 0
    return v.value


def raises(code, fn):
    try:
        fn()
    except cm.CudamatError as e:
        assert e.code == code, (e.code, str(e))
        return
    raise AssertionError("expected error code %d" % code)


def main():
    t_last = [time.time()]

    def lap(what):
        now = time.time()
        print("live_check %-28s %6.2f s" % (what, now - t_last[0]))
        t_last[0] = now

    ctx = cm.Context(0)
    lib = cm.lib()
    rp, ci, va = stencil()
    b_host = np.ones(N)
    K = 11
    b, x = ctx.array(b_host), ctx.empty(N)
    B, X, D = ctx.array(np.ones(N * K)), ctx.empty(N * K), ctx.array(np.full(N * K, 0.5))
    shift = ctx.array(np.full(N, 0.25))
    ctx.sync()
    live0 = live()
    lap("context and inputs")

    def options(**kw):
        ctx.reset_options()
        for k, v in kw.items():
            ctx.set_option(k, v)

    def solver(m=(rp, ci, va)):
        return cm.Solver.from_host_csr(ctx, *m)

    def solve(s, expect_form=None, **kw):
        x.upload(np.ones(N))
        st = s.solve(b, x, maxit=kw.pop("maxit", 20), tol=1e-10, **kw)
        assert expect_form is None or st.loop_form == expect_form, (st.loop_form, expect_form)
        return st

    # ---- the SpMV forms: compressed, aligned and dictionary stream plans, then every forced form
    for opts, m in (({}, None), ({"VALUE_DICT": 0}, None), ({"SPMV_MODE": "pb"}, None), ({"SPMV_MODE": "sell"}, None),
                    ({"SPMV_MODE": "pat"}, None), ({"SPMV_MODE": "csr", "SPMV_FORM": "tiles"}, scattered())):
        options(**opts)
        s = solver(*(() if m is None else (m,)))
        s.spmv(b, x)
        ctx.sync()
        if "SPMV_MODE" in opts:
            assert s.spmv_mode() == {"csr": 0, "pb": 1, "sell": 2, "pat": 3}[opts["SPMV_MODE"]]
        if "SPMV_FORM" in opts:
            assert "tiles" in s.spmv_kernel(), s.spmv_kernel()
        s.close()
    lap("SpMV forms")
    # ---- M = I in every loop form; residual history, guarded once
    for opts, form, kw in (({"FUSED": 0, "RESIDENT": 0}, 0, {}), ({"RESIDENT": 0}, 1, {}), ({}, 2, {}),
                           ({}, None, {"loop": cm.LOOP_PIPELINED}), ({}, 0, {"flags": cm.FLAG_GUARD})):
        options(**opts)
        s = solver()
        solve(s, form, **kw)
        assert len(s.history()) > 0
        solve(s, form, maxit=60, **kw)           # a longer history: regrown
        s.close()
    lap("loop forms")
    # ---- ILU(0) three ways (the last one: split factors, far plans, the permuted copy), the preconditioned pipelined loop
    for opts in ({}, {"LEVELS_SWEEP": 1}, {"TRSV_HYBRID": 1, "TRSV_GROUPS": 2}):
        options(**opts)
        s = solver()
        s.ilu0()
        solve(s, precond=cm.PRECOND_ILU0)
        solve(s, precond=cm.PRECOND_ILU0, loop=cm.LOOP_PIPELINED)
        s.ilu0()                                 # a second set-up releases the first
        s.close()
    lap("ILU(0)")
    # ---- several right-hand sides: the groups regrow (3, then 11 columns), per-column shifts, batched preconditioner
    options(MANY_FORM="batched", MANY_PRECOND="batched")
    s = solver()
    for k in (3, K):
        X.upload(np.ones(N * K))
        st, form = s.solve_many(k, B, N, X, N, maxit=20, tol=1e-10)
        assert form == 1, form
    X.upload(np.ones(N * K))
    st, form = s.solve_shifts(K, D, N, B, N, X, N, maxit=20, tol=1e-10)
    assert form == 1, form
    s.ilu0()
    X.upload(np.ones(N * K))
    s.solve_many(K, B, N, X, N, precond=cm.PRECOND_ILU0, maxit=20, tol=1e-10)
    s.close()
    lap("several right-hand sides")
    # ---- the collective path at world size 1 with the block ILU(0): set_comm releases and rebuilds; then set_comm(NULL)
    # (the dry communicator: one rank has nothing to exchange with, and RCCL takes seconds to start; every buffer, stream and
    # event of the collective path is created all the same -- the iterates are not looked at)
    options(FORCE_SHARDED=1)
    comm = cm.Comm()
    cm._lib.check(lib.cudamat_comm_dry_create(ctx.h, 0, 1, C.byref(comm)))
    s = solver()
    solve(s)                                     # work vectors of the unsharded partition: set_comm releases them
    s.set_comm(comm)
    s.block_ilu0()
    solve(s, precond=cm.PRECOND_BLOCK_ILU0, maxit=5, flags=cm.FLAG_NO_EXIT)
    s.set_comm(None)
    solve(s)
    s.close()
    lib.cudamat_comm_dry_destroy(C.byref(comm))
    lap("world size 1")
    # ---- the host-pointer entry point, two different matrices: the plan cache is replaced
    options()
    rp1 = rp + 1
    for scale in (1.0, 2.0):
        ok, xs, dt, st = cm.bicgstab(N, len(va), va * scale, rp1, ci + 1, b_host, 20, 1e-10)
    lap("host-pointer calls")
    # ---- three set-ups that fail, and leave nothing behind
    bad = ci.copy()
    bad[7] = N + 3
    d_rp, d_ci, d_va = ctx.array(rp), ctx.array(bad), ctx.array(va)
    raises(ERR_ARG, lambda: cm.Solver(ctx, N, N, len(va), d_rp, d_ci, d_va, 0))
    for a in (d_rp, d_ci, d_va):
        a.free()
    s = solver(stencil(drop_diag_of=N // 2))
    raises(ERR_ZERO_PIVOT, s.ilu0)
    s.close()
    s = solver()
    s.ilu0()
    s.set_shift(shift)
    raises(ERR_ARG, lambda: solve(s, precond=cm.PRECOND_ILU0))
    s.close()
    lap("failing set-ups")
    # ---- everything that was created is destroyed: not one allocation more than before the walk
    assert lib.cudamat_plan_cache_clear() == 0
    ctx.sync()
    live1 = live()
    assert live1 == live0, "device allocations in use: %d before the walk, %d after it" % (live0, live1)
    assert lib.cudamat_pool_trim() == 0
    pf = C.c_size_t()
    assert lib.cudamat_mem_info(0, None, None, C.byref(pf)) == 0
    assert pf.value == 0, pf.value
    for a in (b, x, B, X, D, shift):
        a.free()
    ctx.close()
    print("live_check ok: %d allocations in use before and after (pool %s)" % (live0, os.environ.get("CUDAMAT_POOL", "1")))


if __name__ == "__main__":
    main()
