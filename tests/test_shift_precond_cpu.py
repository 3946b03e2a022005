"""ILU(0)-preconditioned solves of (A0 + I d) without a GPU: the two new entry points in the header and the binding, the drop-in
function's signature, and the five-launch preconditioned loop WITH a shift restated on the CPU bit for bit from the pieces of
test_loop_rounding.py (the way test_guard_cpu.segment restates the guarded loop).

The loop is the ILU(0) loop of that file (form "five/lanes", diagonal system) with two additions:
  the shift     every product is (A + diag d) z with the shift as fma(d_i, z_i, sum) after the row sum (spmv_finish_row_fused),
                in r0 too -- `product` with shift_fused, as the un-preconditioned shifted loop has it;
  the factors   those of A0 + diag(d_f) (cudamat_solver_ilu0_shift): k_shift_diag adds d_f to the copied diagonal in one plain
                add, one rounding, so on the diagonal system U = diag(fl(a_i + d_f_i)), L = I and one application is
                minv_dinv(a + d_f, .) with `a + d_f` ONE numpy add.  d_f and d are independent.
With d = None and d_f = 0 this is the existing mirror (a + 0.0 is a bitwise): asserted below for every layout, both loops, with and
without a stopping test, and for the neighbours the existing mirror defines.
The GPU tests that pin the kernels to this mirror are test_shift_precond_bits in test_gpu_shift_precond.py; the cases they pin are
found here, by running the mirror -- never from GPU output."""
import functools
import inspect
import math
import os
import re

import numpy as np

import test_loop_rounding as L
from test_loop_rounding import Run, dot_parts, dot_step, each, load_scalars

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORM = "five/lanes"
TOL = 1e-8
LAYOUT_COL = {"aligned": 2, "offset8": 0}        # the columns of test_guard_cpu.py: pairs / rows tell their neighbours apart there


def ploop(a, b, x0, d_f, vec=(1, 1, 1), kind="pbicgstab", d=None, iters=L.ITERS, tol=None, p_update=L.step_p, term=dot_step,
          swap_x=False, minv=L.minv_dinv, shift=L.shift_fused):
    """At most `iters` iterations of iterate_reference with CUDAMAT_PRECOND_ILU0 on the diagonal system diag(a), the solver's
    shift d (None: none) and factors built from a + d_f.  tol = None: FLAG_NO_EXIT.  Returns test_loop_rounding.Run."""
    assert kind in ("pbicgstab", "pbicgstab2")
    two = kind == "pbicgstab2"
    n = len(b)
    d_init, d_spmv, d_half, d_full = L.dealings(a, FORM, vec)
    u = a + d_f                                                  # k_shift_diag: lu[diag] + d_f, one rounding
    def mv(z): return L.product(a, z, d, L.row_sum_products, shift)
    x = np.array(x0, np.float64)
    r = each(L.step_r0, b, mv(x))
    rw, p, v = r.copy(), r.copy(), np.zeros(n)
    full = [dot_parts(d_init, r, r, term)] * 2
    tolabs = None if tol is None else tol * math.sqrt(load_scalars(full[1]))
    rho_s, alpha, omega, hist, it = [1.0, 1.0], 1.0, 1.0, [], 0
    while True:
        rho, rr = load_scalars(full[0]), load_scalars(full[1])
        if it:
            hist.append(math.sqrt(rr))
            if tolabs is not None and hist[-1] < tolabs:
                return Run(it, False, x, np.array(hist))
            assert tolabs is None or not two or abs(omega) >= L.OMEGA_MIN, "breakdown: not restated"
        if it == iters:
            return Run(it, False, x, np.array(hist))
        rho_prev, rho_s[it & 1] = rho_s[(it + 1) & 1], rho
        if it:
            beta = L.step_beta(rho, rho_prev, alpha, omega)
            p = each(lambda ri, pi, vi: p_update(ri, pi, vi, beta, omega), r, p, v)
        pw = minv(u, p)
        v = mv(pw)
        alpha = L.step_alpha(rho, load_scalars(dot_parts(d_spmv, v, rw, term)))
        r = each(lambda ri, vi: L.step_r_half(ri, vi, alpha), r, v)
        nrm_half = math.sqrt(load_scalars(dot_parts(d_half, r, r, term)))
        if not two:
            hist.append(nrm_half)
            if tolabs is not None and nrm_half < tolabs:
                return Run(it, True, each(lambda xi, pi: L.step_x_half(xi, pi, alpha), x, pw), np.array(hist))
        s = minv(u, r)
        t = mv(s)
        omega = L.step_omega(load_scalars(dot_parts(d_spmv, t, r, term)), load_scalars(dot_parts(d_spmv, t, t, term)))
        if swap_x:
            x = each(lambda xi, pi, si: L.step_x_half(L.step_x_full(xi, si, omega), pi, alpha), x, pw, s)
        else:
            x = each(lambda xi, pi, si: L.step_x_full(L.step_x_half(xi, pi, alpha), si, omega), x, pw, s)
        r = each(lambda ri, ti: L.step_r_full(ri, ti, omega), r, t)
        full = [dot_parts(d_full, rw, r, term), dot_parts(d_full, r, r, term)]
        it += 1


# ------------------------------------------------------------------ the cases the GPU test pins
@functools.lru_cache(maxsize=None)
def pinned_exact(layout):
    """(a) factor shift = solver shift = shift_of(N), solved to TOL: M is A up to the rounding of 1 / (a_i + d_i)"""
    a, b, x0 = L.system(LAYOUT_COL[layout])
    d = L.shift_of(L.N)
    run = ploop(a, b, x0, d, vec=L.LAYOUTS[layout], d=d, iters=20, tol=TOL)
    L.frozen(run.x, run.history)
    return run


@functools.lru_cache(maxsize=None)
def pinned_stale(layout):
    """(b) factors built from half the solver's shift, ITERS iterations without a stopping test"""
    a, b, x0 = L.system(LAYOUT_COL[layout])
    d = L.shift_of(L.N)
    run = ploop(a, b, x0, 0.5 * d, vec=L.LAYOUTS[layout], d=d, iters=L.ITERS, tol=None)
    L.frozen(run.x, run.history)
    return run


# ------------------------------------------------------------------ interface
def test_header_declares_and_lib_binds_the_two_functions():
    import ctypes as C
    from cuda_mat_amd import _lib
    text = open(os.path.join(ROOT, "include", "cudamat.h")).read()
    assert re.search(r"int\s+cudamat_solver_ilu0_shift\s*\(\s*cudamat_solver\s*\*\s*s\s*,\s*const\s+double\s*\*\s*d_factor\s*\)\s*;", text)
    assert re.search(r"int\s+cudamat_solver_ilu0_shifted\s*\(\s*cudamat_solver\s*\*\s*s\s*,\s*int\s*\*\s*yes\s*\)\s*;", text)
    table = next(v for v in vars(_lib).values() if isinstance(v, dict) and "cudamat_solver_ilu0" in v)
    assert table["cudamat_solver_ilu0_shift"] == (C.c_int, [C.c_void_p, C.c_void_p])
    assert table["cudamat_solver_ilu0_shifted"] == (C.c_int, [C.c_void_p, C.POINTER(C.c_int)])
    # the C++ shim's overload, marked as an extension of this library
    hdr = open(os.path.join(ROOT, "include", "pbicgstab.h")).read()
    overloads = re.findall(r"bool\s+bicgstab_lu_precond\s*\(([^;]*?)\)\s*;", hdr, re.S)
    assert len(overloads) == 2 and sum("IN(*d)" in o and "IN(*x0)" in o for o in overloads) == 1
    assert re.search(r"EXTENSION[^;]*bicgstab_lu_precond", hdr, re.S)


def test_python_layer_has_the_documented_signatures():
    import cuda_mat_amd as cm
    from cuda_mat_amd import api
    sig = inspect.signature(api.bicgstab_d_lu_precond)
    assert list(sig.parameters) == ["n", "nnz", "A0", "iA0", "jA0", "d", "x0", "b", "maxit", "tol", "debug"]
    assert sig.parameters["debug"].default is False
    assert cm.bicgstab_d_lu_precond is api.bicgstab_d_lu_precond
    sig = inspect.signature(api.Solver.ilu0)
    assert list(sig.parameters) == ["self", "shift"] and sig.parameters["shift"].default is None
    assert list(inspect.signature(api.Solver.ilu0_shifted).parameters) == ["self"]


def test_the_drop_in_function_is_one_gpu_only(monkeypatch):
    """with use_gpus(k > 1) the other drop-in functions shard and ILU(0) becomes block-Jacobi, which takes no shift: this one says
    so before anything is uploaded"""
    import pytest
    from cuda_mat_amd import api
    monkeypatch.setattr(api, "_GPUS", 2)
    with pytest.raises(ValueError, match="one-GPU only"):
        api.bicgstab_d_lu_precond(2, 2, [1.0, 1.0], [0, 1, 2], [0, 1], [0.5, 0.5], [1.0, 1.0], [1.0, 1.0], 5, 1e-8)


def test_no_new_flag_and_no_new_statistic():
    """everything new is a function or an argument"""
    text = open(os.path.join(ROOT, "include", "cudamat.h")).read()
    assert len(set(re.findall(r"\bCUDAMAT_FLAG_[A-Z0-9_]+\b", text))) == 5


# ------------------------------------------------------------------ the mirror
def test_without_a_shift_the_mirror_is_the_existing_one():
    """d = None and d_f = 0: bit for bit the ILU(0) loop of test_loop_rounding.py -- every layout, both loops, without and with
    a stopping test, and under each neighbour that mirror defines"""
    zero = np.zeros(L.N)
    for col in (4, 2, 0):
        a, b, x0 = L.system(col)
        for layout, vec in L.LAYOUTS.items():
            for kind in ("pbicgstab", "pbicgstab2"):
                for tol, iters in ((None, L.ITERS), (TOL, 12)):
                    if col != 4 and (kind == "pbicgstab2" or layout == "rows"):
                        continue
                    want = L.loop(a, b, x0, vec=vec, kind=kind, precond=True, iters=iters, tol=tol)
                    got = ploop(a, b, x0, zero, vec=vec, kind=kind, iters=iters, tol=tol)
                    assert (got.iters, got.half_exit) == (want.iters, want.half_exit), (col, layout, kind, tol)
                    np.testing.assert_array_equal(got.x, want.x)
                    np.testing.assert_array_equal(got.history, want.history)
    a, b, x0, _ = L.inputs("diagonal", FORM)
    for kw in (dict(minv=L.minv_divide), dict(term=L.dot_step_two_roundings), dict(swap_x=True), dict(p_update=L.step_p_three_roundings)):
        want = L.pinned_ilu0(**kw)
        got = ploop(a, b, x0, zero, **kw)
        np.testing.assert_array_equal(got.x, want[0])
        np.testing.assert_array_equal(got.history, want[1])


def test_the_pinned_cases_are_what_the_gpu_test_says_they_are():
    """(a) the exact preconditioner leaves at the half step of iteration 0 with a margin, and x solves the shifted system;
    (b) stale factors: a real iteration (the residual falls by orders of magnitude, every value finite), which the mirror can
    tell from its neighbours: M^-1 as a division, the shift of the product in two roundings, and factors of another matrix
    (of A0 alone; of A0 + d, the solver's shift in place of the factor's)."""
    d = L.shift_of(L.N)
    for layout, col in LAYOUT_COL.items():
        a, b, x0 = L.system(col)
        vec = L.LAYOUTS[layout]
        run = pinned_exact(layout)
        r0 = b - (a + d) * x0
        print(layout, "(a) iters", run.iters, "half", run.half_exit, "history / (tol nrm0)", run.history / (TOL * np.linalg.norm(r0)))
        assert (run.iters, run.half_exit, len(run.history)) == (0, True, 1)
        assert run.history[0] <= 0.01 * TOL * np.linalg.norm(r0)
        assert np.linalg.norm(b - (a + d) * run.x) <= 1e-12 * np.linalg.norm(r0)
        st = pinned_stale(layout)
        assert st.iters == L.ITERS and len(st.history) == 2 * L.ITERS and np.all(np.isfinite(st.x)) and np.all(np.isfinite(st.history))
        print(layout, "(b) history / nrm0", st.history / np.linalg.norm(r0))
        assert st.history[-1] < 1e-3 * st.history[0] and np.all(st.history > 0.0)
        # (the dot terms and the p-update are the unshifted loop's kernels, pinned on inputs picked for them in test_loop_rounding.py)
        for name, kw in (("M^-1 as a division", dict(minv=L.minv_divide)), ("shift in two roundings", dict(shift=L.shift_two_roundings))):
            other = ploop(a, b, x0, 0.5 * d, vec=vec, d=d, **kw)
            print(layout, name, "differs in", L.differing(other.x, st.x), "entries of x")
            assert L.differing(other.x, st.x) >= L.MIN_DIFFERING_ROWS, (layout, name)
        # factors of the wrong matrix: of A0 alone, and of A0 + d
        for name, d_f in (("factors of A0", np.zeros(L.N)), ("factors of A0 + d", d)):
            other = ploop(a, b, x0, d_f, vec=vec, d=d)
            assert L.differing(other.x, st.x) >= L.MIN_DIFFERING_ROWS, (layout, name)
