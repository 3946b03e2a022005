"""Host-side mirror of the reference's interface for the BiCGSTAB path, over the C ABI.

Names and argument meaning follow pbicgstab.h / mmio_wrapper.h of the reference:
  bicgstab(n, nnz, A, iA, jA, b, maxit, tol, debug)                  pbicgstab.h:113
  bicgstab_d(n, nnz, A0, iA0, jA0, d, x0, b, maxit, tol, debug)      pbicgstab.h:116 (overload)
  bicgstab_lu_precond(n, nnz, A, iA, jA, b, maxit, tol, debug)       pbicgstab.h:119
  bicgstab_d_lu_precond(n, nnz, A0, iA0, jA0, d, x0, b, maxit, tol, debug)   ILU(0) of A0 + diag(d), the loop with d (new)
  bicgstab_l2(n, nnz, A0, iA0, jA0, d, x0, b, maxit, tol, debug)     BiCGSTAB(2), no preconditioner; d, x0 may be None (new)
  bicgstab_l2_lu_precond(n, nnz, A0, iA0, jA0, d, x0, b, maxit, tol, debug)   BiCGSTAB(2) with ILU(0) of A0 + diag(d) (new)
  cg(n, nnz, A0, iA0, jA0, d, x0, b, maxit, tol, debug)              conjugate gradients for symmetric positive definite systems (new)
  cg_lu_precond(n, nnz, A0, iA0, jA0, d, x0, b, maxit, tol, debug)   ... with ILU(0) of A0 + diag(d) (new)
  bicgstab_many(n, nnz, A, iA, jA, B, maxit, tol, d, x0)             bicgstab / bicgstab_d for the columns of B (new)
  bicgstab_lu_precond_many(n, nnz, A, iA, jA, B, maxit, tol)         bicgstab_lu_precond for the columns of B (new)
  bicgstab_d_many(n, nnz, A0, iA0, jA0, D, x0, B, maxit, tol)        bicgstab_d with shift D[:, j] for column j of B (new)
  bicgstab_d_lu_precond_many(n, nnz, A0, iA0, jA0, D, x0, B, maxit, tol)   bicgstab_d_lu_precond with shift D[:, j], and the
                                                                     ILU(0) of A0 + diag(D[:, j]), for column j of B (new)
  loadMMSparseMatrix(filename, elem_type, csrFormat)                 mmio_wrapper.h:133
  toDenseVector(n, nnz, A, IA)                                       pbicgstab.cu:1101
Each solver returns (ok, x, dtAlg, stats): `ok` is the reference's bool, x the
solution (written even when not converged), dtAlg the loop's wall seconds.

Context / DeviceArray / Solver expose the HBM-resident operation used by the parity
tests and bench.py.  All compute goes through libcudamat_hip.so; there is no fallback.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import (FLAG_ASSUME_SYMMETRIC, FLAG_DEBUG, FLAG_GUARD, FLAG_NO_EXIT, FLAG_PROFILE, FLAG_X0_ONES, LOOP_BICGSTAB_L2, LOOP_CG, LOOP_PBICGSTAB,
                   LOOP_PBICGSTAB2, LOOP_PIPELINED, PRECOND_BLOCK_ILU0, PRECOND_ILU0, PRECOND_NONE, Comm, CudamatError, Stats, check)


def _np(a, dtype):
    return np.ascontiguousarray(a, dtype=dtype)


def _vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


# ----------------------------------------------------------------- drop-in functions
_GPUS = 1


def use_gpus(ngpu):
    """spread the three drop-in solves below over `ngpu` GPUs of the node (uniform row blocks, one host thread and
    one RCCL rank per device: cudamat_solve_sharded); the ILU(0) entry point then factors every GPU's diagonal block
    (block-Jacobi).  Mirrors cudamat_use_gpus of include/pbicgstab.h.  Default 1 = the reference's behaviour."""
    global _GPUS
    _GPUS = max(1, int(ngpu))


def _solve(n, nnz, A, iA, jA, d, x0, b, precond, loop, maxit, tol, debug):
    A, iA, jA, b = _np(A, np.float64), _np(iA, np.int32), _np(jA, np.int32), _np(b, np.float64)
    d = None if d is None else _np(d, np.float64)
    x0 = None if x0 is None else _np(x0, np.float64)
    if len(iA) != n + 1 or len(A) < nnz or len(jA) < nnz or len(b) != n:
        raise ValueError("array sizes do not match n / nnz")
    x = np.zeros(n)
    st = Stats()
    if _GPUS > 1:
        if precond == PRECOND_ILU0:
            precond = PRECOND_BLOCK_ILU0      # ILU(0) of the whole matrix does not shard
        check(_lib.lib().cudamat_solve_sharded(_GPUS, n, nnz, _vp(A), _vp(iA), _vp(jA), _vp(d), _vp(x0), _vp(b), precond,
                                               loop, maxit, tol, int(bool(debug)), _vp(x), C.byref(st)))
    else:
        check(_lib.lib().cudamat_solve(n, nnz, _vp(A), _vp(iA), _vp(jA), _vp(d), _vp(x0), _vp(b), precond,
                                       loop, maxit, tol, int(bool(debug)), _vp(x), C.byref(st)))
    return x, st


def bicgstab(n, nnz, A, iA, jA, b, maxit, tol, debug=False):
    """solve Ax = b, no preconditioner (pbicgstab.h:113).  The reference implementation is
    broken (its `r += b; r0 = r` lines are commented out, pbicgstab.cu:471-478); this is the
    intended maths: the d-variant loop with d = 0 and x0 = 1 (pbicgstab.cu:827-831)."""
    x, st = _solve(n, nnz, A, iA, jA, None, None, b, PRECOND_NONE, LOOP_PBICGSTAB2, maxit, tol, debug)
    return bool(st.converged), x, st.t_solve, st


def bicgstab_d(n, nnz, A0, iA0, jA0, d, x0, b, maxit, tol, debug=False):
    """solve (A0 + I*d) x = b from x0, no preconditioner (pbicgstab.h:116)."""
    x, st = _solve(n, nnz, A0, iA0, jA0, d, x0, b, PRECOND_NONE, LOOP_PBICGSTAB2, maxit, tol, debug)
    return bool(st.converged), x, st.t_solve, st


def bicgstab_lu_precond(n, nnz, A, iA, jA, b, maxit, tol, debug=False):
    """solve Ax = b with the ILU(0) preconditioner; A[i,i] != 0 required (pbicgstab.h:118-119).
    Like the reference (pbicgstab.cu:408) `ok` is True whenever the solve ran; convergence is
    in stats.converged."""
    x, st = _solve(n, nnz, A, iA, jA, None, None, b, PRECOND_ILU0, LOOP_PBICGSTAB, maxit, tol, debug)
    return True, x, st.t_solve, st


def bicgstab_d_lu_precond(n, nnz, A0, iA0, jA0, d, x0, b, maxit, tol, debug=False):
    """solve (A0 + I*d) x = b from x0 with the ILU(0) preconditioner of A0 + diag(d) (not in the reference: the overload
    bicgstab_lu_precond(..., d, x0, ...) of include/pbicgstab.h).  Returns what bicgstab_lu_precond returns.  A repeated call
    with the same matrix reuses the factors only when d is byte-identical to the one they were built from."""
    if d is None:
        raise ValueError("d is required (bicgstab_lu_precond is the call without a shift)")
    if _GPUS > 1:
        raise ValueError("ILU(0) of the shifted matrix is one-GPU only: use_gpus(%d) is set (block-Jacobi takes no shift)" % _GPUS)
    x, st = _solve(n, nnz, A0, iA0, jA0, d, x0, b, PRECOND_ILU0, LOOP_PBICGSTAB, maxit, tol, debug)
    return True, x, st.t_solve, st


def bicgstab_l2(n, nnz, A0, iA0, jA0, d, x0, b, maxit, tol, debug=False):
    """solve (A0 + I*d) x = b from x0 with BiCGSTAB(2) (LOOP_BICGSTAB_L2: for the systems on which BiCGSTAB stalls), no
    preconditioner; d None: no shift, x0 None: ones.  maxit and stats.iters count sweeps of four products each.  Mirrors
    bicgstab_l2 of include/pbicgstab.h: `ok` is stats.converged.  One GPU only (use_gpus(k > 1): CudamatError)."""
    x, st = _solve(n, nnz, A0, iA0, jA0, d, x0, b, PRECOND_NONE, LOOP_BICGSTAB_L2, maxit, tol, debug)
    return bool(st.converged), x, st.t_solve, st


def bicgstab_l2_lu_precond(n, nnz, A0, iA0, jA0, d, x0, b, maxit, tol, debug=False):
    """bicgstab_l2 with the ILU(0) preconditioner of A0 + diag(d) (of A0 when d is None), applied from the right.  Like
    bicgstab_lu_precond `ok` is True whenever the solve ran; convergence is in stats.converged."""
    x, st = _solve(n, nnz, A0, iA0, jA0, d, x0, b, PRECOND_ILU0, LOOP_BICGSTAB_L2, maxit, tol, debug)
    return True, x, st.t_solve, st


def cg(n, nnz, A0, iA0, jA0, d, x0, b, maxit, tol, debug=False):
    """solve (A0 + I*d) x = b from x0 by conjugate gradients (LOOP_CG: A0 + I*d symmetric positive definite), no preconditioner;
    d None: no shift, x0 None: ones.  One product per iteration.  Mirrors cg of include/pbicgstab.h: `ok` is stats.converged;
    a matrix that is not symmetric raises CudamatError, one that is not positive definite returns stats.breakdown = 1.  One GPU
    only (use_gpus(k > 1): CudamatError)."""
    x, st = _solve(n, nnz, A0, iA0, jA0, d, x0, b, PRECOND_NONE, LOOP_CG, maxit, tol, debug)
    return bool(st.converged), x, st.t_solve, st


def cg_lu_precond(n, nnz, A0, iA0, jA0, d, x0, b, maxit, tol, debug=False):
    """cg with the ILU(0) preconditioner of A0 + diag(d) (of A0 when d is None).  `ok` is stats.converged."""
    x, st = _solve(n, nnz, A0, iA0, jA0, d, x0, b, PRECOND_ILU0, LOOP_CG, maxit, tol, debug)
    return bool(st.converged), x, st.t_solve, st


def bicgstab_many(n, nnz, A, iA, jA, B, maxit, tol, d=None, x0=None):
    """bicgstab (d None) / bicgstab_d for every column of B, shape (n, k), in one call (cudamat_solve_many): the same loop
    (LOOP_PBICGSTAB2, x0 = ones unless given, shape (n, k)), the same plan cache.  Returns (ok, X, dtAlg, stats, form):
    ok a list of k bools, X of shape (n, k), dtAlg the whole call's loop seconds, stats a list of k Stats, form 1 when the
    columns ran batched (several per launch) and 0 when column by column."""
    A, iA, jA = _np(A, np.float64), _np(iA, np.int32), _np(jA, np.int32)
    B = np.asarray(B, dtype=np.float64)
    if B.ndim == 1:
        B = B[:, None]
    if len(iA) != n + 1 or len(A) < nnz or len(jA) < nnz or B.shape[0] != n:
        raise ValueError("array sizes do not match n / nnz")
    k = B.shape[1]
    Bf = np.asfortranarray(B)
    d = None if d is None else _np(d, np.float64)
    x0f = None
    if x0 is not None:
        x0f = np.asfortranarray(np.asarray(x0, dtype=np.float64).reshape(n, k))
    X = np.zeros((n, k), order="F")
    st = (Stats * max(k, 1))()
    form = C.c_int(0)
    check(_lib.lib().cudamat_solve_many(n, nnz, _vp(A), _vp(iA), _vp(jA), _vp(d), k, _vp(Bf), n, _vp(x0f), _vp(X), n,
                                        PRECOND_NONE, LOOP_PBICGSTAB2, maxit, tol, st, C.byref(form)))
    stats = [st[j] for j in range(k)]
    return [bool(s.converged) for s in stats], np.ascontiguousarray(X), (stats[0].t_solve if k else 0.0), stats, form.value


def _shift_block(D, n, k):
    """D as an (n, k) block: given as one, or as k scalars sigma_j meaning d_j = sigma_j * 1"""
    D = np.asarray(D, dtype=np.float64)
    if D.ndim == 1 and D.shape[0] == k:
        D = np.broadcast_to(D[None, :], (n, k))
    if D.shape != (n, k):
        raise ValueError("D must have shape (n, k) = (%d, %d), or hold k scalars; got %s" % (n, k, D.shape))
    return D


def bicgstab_d_many(n, nnz, A0, iA0, jA0, D, x0, B, maxit, tol):
    """bicgstab_d for a family of shifted systems (A0 + I*d_j) x_j = b_j in one call (cudamat_solve_shifts): the matrix is
    shared, column j of B is solved with the shift D[:, j].  D: shape (n, k), or k scalars sigma_j meaning d_j = sigma_j * 1
    (broadcast here; the library sees a block).  x0: shape (n, k), or None for ones.  The same loop (LOOP_PBICGSTAB2) and plan
    cache as bicgstab_many -- the cache compares the matrix, not the shifts, so a call with the same A0 and other shifts reuses
    the plan.  Returns what bicgstab_many returns: (ok, X, dtAlg, stats, form)."""
    A0, iA0, jA0 = _np(A0, np.float64), _np(iA0, np.int32), _np(jA0, np.int32)
    B = np.asarray(B, dtype=np.float64)
    if B.ndim == 1:
        B = B[:, None]
    if len(iA0) != n + 1 or len(A0) < nnz or len(jA0) < nnz or B.ndim != 2 or B.shape[0] != n:
        raise ValueError("array sizes do not match n / nnz")
    k = B.shape[1]
    Df, Bf = np.asfortranarray(_shift_block(D, n, k)), np.asfortranarray(B)
    x0f = None
    if x0 is not None:
        x0f = np.asarray(x0, dtype=np.float64)
        if x0f.size != n * k:
            raise ValueError("x0 must have shape (n, k)")
        x0f = np.asfortranarray(x0f.reshape(n, k))
    X = np.zeros((n, k), order="F")
    st = (Stats * max(k, 1))()
    form = C.c_int(0)
    check(_lib.lib().cudamat_solve_shifts(n, nnz, _vp(A0), _vp(iA0), _vp(jA0), k, _vp(Df), n, _vp(Bf), n, _vp(x0f), _vp(X), n,
                                          LOOP_PBICGSTAB2, maxit, tol, st, C.byref(form)))
    stats = [st[j] for j in range(k)]
    return [bool(s.converged) for s in stats], np.ascontiguousarray(X), (stats[0].t_solve if k else 0.0), stats, form.value


def bicgstab_d_lu_precond_many(n, nnz, A0, iA0, jA0, D, x0, B, maxit, tol):
    """bicgstab_d_lu_precond for a family of shifted systems (A0 + I*d_j) x_j = b_j in one call (cudamat_solve_shifts_ilu0):
    column j of B is solved with the shift D[:, j] and preconditioned with the ILU(0) of A0 + diag(D[:, j]) -- one set of
    factors per column.  D: shape (n, k), or k scalars, as in bicgstab_d_many; x0: shape (n, k), or None for ones.  The loop is
    LOOP_PBICGSTAB; the columns run one factorisation and one solve each unless CUDAMAT_MANY_PRECOND = batched | auto sends
    them through the K-wide factorisation and the multi-column triangular solves.  The plan cache compares the matrix, not
    the shifts.  Returns (ok, X, dtAlg, stats, form) as bicgstab_lu_precond_many does: ok[j] True whenever the solve ran."""
    A0, iA0, jA0 = _np(A0, np.float64), _np(iA0, np.int32), _np(jA0, np.int32)
    B = np.asarray(B, dtype=np.float64)
    if B.ndim == 1:
        B = B[:, None]
    if len(iA0) != n + 1 or len(A0) < nnz or len(jA0) < nnz or B.ndim != 2 or B.shape[0] != n:
        raise ValueError("array sizes do not match n / nnz")
    k = B.shape[1]
    Df, Bf = np.asfortranarray(_shift_block(D, n, k)), np.asfortranarray(B)
    x0f = None
    if x0 is not None:
        x0f = np.asarray(x0, dtype=np.float64)
        if x0f.size != n * k:
            raise ValueError("x0 must have shape (n, k)")
        x0f = np.asfortranarray(x0f.reshape(n, k))
    X = np.zeros((n, k), order="F")
    st = (Stats * max(k, 1))()
    form = C.c_int(0)
    check(_lib.lib().cudamat_solve_shifts_ilu0(n, nnz, _vp(A0), _vp(iA0), _vp(jA0), k, _vp(Df), n, _vp(Bf), n, _vp(x0f), _vp(X), n,
                                               maxit, tol, st, C.byref(form)))
    stats = [st[j] for j in range(k)]
    return [True] * k, np.ascontiguousarray(X), (stats[0].t_solve if k else 0.0), stats, form.value


def bicgstab_lu_precond_many(n, nnz, A, iA, jA, B, maxit, tol):
    """bicgstab_lu_precond for every column of B, shape (n, k), in one call (cudamat_solve_many with ILU(0)): the same loop
    (LOOP_PBICGSTAB, x0 = ones), the same plan cache, the factors computed once.  The columns run one solve each unless the
    switch CUDAMAT_MANY_PRECOND = batched | auto sends them through the multi-column triangular solves.  Returns
    (ok, X, dtAlg, stats, form) as bicgstab_many does, with ok[j] True whenever the solve ran (bicgstab_lu_precond's
    convention; convergence is in stats[j].converged)."""
    A, iA, jA = _np(A, np.float64), _np(iA, np.int32), _np(jA, np.int32)
    B = np.asarray(B, dtype=np.float64)
    if B.ndim == 1:
        B = B[:, None]
    if len(iA) != n + 1 or len(A) < nnz or len(jA) < nnz or B.ndim != 2 or B.shape[0] != n:
        raise ValueError("array sizes do not match n / nnz")
    k = B.shape[1]
    Bf = np.asfortranarray(B)
    X = np.zeros((n, k), order="F")
    st = (Stats * max(k, 1))()
    form = C.c_int(0)
    check(_lib.lib().cudamat_solve_many(n, nnz, _vp(A), _vp(iA), _vp(jA), None, k, _vp(Bf), n, None, _vp(X), n,
                                        PRECOND_ILU0, LOOP_PBICGSTAB, maxit, tol, st, C.byref(form)))
    stats = [st[j] for j in range(k)]
    return [True] * k, np.ascontiguousarray(X), (stats[0].t_solve if k else 0.0), stats, form.value


def loadMMSparseMatrix(filename, elem_type="d", csrFormat=True):
    """mmio_wrapper.h:133-142: returns (err, m, n, nnz, aVal, aRowInd, aColInd); err 0 ok / 1."""
    if elem_type != "d":
        raise ValueError("only elem_type 'd' is supported on this path")
    m, n, nnz = C.c_int(), C.c_int(), C.c_int()
    v, r, c = C.POINTER(C.c_double)(), C.POINTER(C.c_int)(), C.POINTER(C.c_int)()
    L = _lib.lib()
    err = L.cudamat_load_mtx(str(filename).encode(), int(bool(csrFormat)), C.byref(m), C.byref(n),
                             C.byref(nnz), C.byref(v), C.byref(r), C.byref(c))
    if err:
        return 1, 0, 0, 0, None, None, None
    nr = m.value + 1 if csrFormat else nnz.value
    nc = nnz.value if csrFormat else n.value + 1
    row = np.ctypeslib.as_array(r, shape=(nr,)).astype(np.int32, copy=True)
    col = np.ctypeslib.as_array(c, shape=(nc,)).astype(np.int32, copy=True) if nc else np.zeros(0, np.int32)
    val = (np.ctypeslib.as_array(v, shape=(nnz.value,)).astype(np.float64, copy=True)
           if nnz.value else np.zeros(0))
    for p in (v, r, c):
        L.cudamat_host_free(p)
    return 0, m.value, n.value, nnz.value, val, row, col


def toDenseVector(n, nnz, A, IA):
    A, IA = _np(A, np.float64), _np(IA, np.int32)
    out = np.empty(n)
    _lib.lib().cudamat_to_dense_vector(n, nnz, _vp(A), _vp(IA), _vp(out))
    return out


# ----------------------------------------------------------------- HBM-resident operation
class DeviceArray:
    """a typed allocation in HBM owned by a Context"""

    def __init__(self, ctx, n, dtype):
        self.ctx, self.n, self.dtype = ctx, int(n), np.dtype(dtype)
        p = C.c_void_p()
        check(_lib.lib().cudamat_malloc(ctx.h, self.n * self.dtype.itemsize, C.byref(p)))
        self.ptr = p.value

    @property
    def nbytes(self):
        return self.n * self.dtype.itemsize

    def upload(self, a):
        a = _np(a, self.dtype)
        assert a.size == self.n
        check(_lib.lib().cudamat_h2d(self.ctx.h, self.ptr, _vp(a), self.nbytes))
        return self

    def download(self):
        out = np.empty(self.n, self.dtype)
        check(_lib.lib().cudamat_d2h(self.ctx.h, _vp(out), self.ptr, self.nbytes))
        return out

    def zero(self):
        check(_lib.lib().cudamat_memset(self.ctx.h, self.ptr, 0, self.nbytes))
        return self

    def free(self):
        if self.ptr:
            _lib.lib().cudamat_free(self.ctx.h, self.ptr)
            self.ptr = None


def _ptr(a):
    """device pointer of a DeviceArray, a torch tensor, or a raw int"""
    if a is None:
        return None
    if isinstance(a, DeviceArray):
        return a.ptr
    if hasattr(a, "data_ptr"):
        return a.data_ptr()
    return int(a)


class Context:
    """device + stream (+ reduction workspace).  stream: raw hipStream_t value (e.g.
    torch.cuda.current_stream().cuda_stream) or None for a private stream."""

    def __init__(self, device=0, stream=None):
        h = C.c_void_p()
        check(_lib.lib().cudamat_ctx_create(device, stream, C.byref(h)))
        self.h = h
        self.device = device

    def close(self):
        if self.h:
            _lib.lib().cudamat_ctx_destroy(self.h)
            self.h = None

    def sync(self):
        check(_lib.lib().cudamat_ctx_sync(self.h))

    def set_option(self, name, value):
        """one switch of this context (csrc/config.h; `name` as in options_help(), with or without the CUDAMAT_ prefix).
        A context reads the CUDAMAT_* environment once, when it is created; afterwards only this call changes a switch.
        Whatever runs on the context after the call sees the new value."""
        check(_lib.lib().cudamat_ctx_set_option(self.h, str(name).encode(), str(value).encode()))
        return self

    def reset_options(self):
        """back to what a context created now would hold: the defaults overridden by the CUDAMAT_* environment"""
        check(_lib.lib().cudamat_ctx_reset_options(self.h))
        return self

    def empty(self, n, dtype=np.float64):
        return DeviceArray(self, n, dtype)

    def array(self, a, dtype=None):
        a = np.asarray(a)
        dtype = a.dtype if dtype is None else dtype
        return DeviceArray(self, a.size, dtype).upload(a)

    # elementary kernels (device pointers)
    def spmv(self, n, rowptr, colidx, val, base, x, y, alpha=1.0, beta=0.0, d=None):
        check(_lib.lib().cudamat_spmv(self.h, n, _ptr(rowptr), _ptr(colidx), _ptr(val), base, alpha,
                                      _ptr(x), _ptr(d), beta, _ptr(y)))

    def dot(self, n, x, y):
        out = self.empty(1)
        check(_lib.lib().cudamat_dot(self.h, n, _ptr(x), _ptr(y), out.ptr))
        v = out.download()[0]
        out.free()
        return v

    def nrm2(self, n, x):
        out = self.empty(1)
        check(_lib.lib().cudamat_nrm2(self.h, n, _ptr(x), out.ptr))
        v = out.download()[0]
        out.free()
        return v

    def axpy(self, n, alpha, x, y):
        check(_lib.lib().cudamat_axpy(self.h, n, alpha, _ptr(x), _ptr(y)))

    def scal(self, n, alpha, x):
        check(_lib.lib().cudamat_scal(self.h, n, alpha, _ptr(x)))

    # synthetic inputs generated in HBM
    def gen_rand_rows(self, n, per_row, seed, row0, row1, base, rowptr, colidx, val):
        check(_lib.lib().cudamat_gen_rand_rows(self.h, n, per_row, seed, row0, row1, base, _ptr(rowptr),
                                               _ptr(colidx), _ptr(val)))

    def gen_poisson5(self, nx, ny, row0, row1, base, rowptr, colidx, val):
        check(_lib.lib().cudamat_gen_poisson5(self.h, nx, ny, row0, row1, base, _ptr(rowptr),
                                              _ptr(colidx), _ptr(val)))

    def gen_xstar(self, i0, i1, seed, x):
        check(_lib.lib().cudamat_gen_xstar(self.h, i0, i1, seed, _ptr(x)))

    def timer(self):
        return Timer(self)


class Timer:
    """HIP events on the context's stream"""

    def __init__(self, ctx):
        self.ctx = ctx
        h = C.c_void_p()
        check(_lib.lib().cudamat_timer_create(ctx.h, C.byref(h)))
        self.h = h

    def start(self):
        check(_lib.lib().cudamat_timer_start(self.ctx.h, self.h))

    def stop(self):
        check(_lib.lib().cudamat_timer_stop(self.ctx.h, self.h))

    def elapsed_ms(self):
        ms = C.c_double()
        check(_lib.lib().cudamat_timer_elapsed_ms(self.ctx.h, self.h, C.byref(ms)))
        return ms.value

    def close(self):
        if self.h:
            _lib.lib().cudamat_timer_destroy(self.ctx.h, self.h)
            self.h = None


class Solver:
    """one HBM-resident (row block of a) linear system: cudamat_solver_* of the C ABI"""

    def __init__(self, ctx, n_local, n_cols, nnz, rowptr, colidx, val, base):
        self.ctx = ctx
        self.n, self.n_cols, self.nnz = int(n_local), int(n_cols), int(nnz)
        h = C.c_void_p()
        check(_lib.lib().cudamat_solver_create(ctx.h, self.n, self.n_cols, self.nnz, _ptr(rowptr),
                                               _ptr(colidx), _ptr(val), base, C.byref(h)))
        self.h = h
        self._keep = []

    @classmethod
    def from_host_csr(cls, ctx, rowptr, colidx, val, n_cols=None):
        """cudamat_solver_create_host: the solver's set-up runs beside the upload of the host arrays"""
        rowptr, colidx, val = _np(rowptr, np.int32), _np(colidx, np.int32), _np(val, np.float64)
        n = len(rowptr) - 1
        base = int(rowptr[0])
        nnz = int(rowptr[-1]) - base
        if nnz == 0:
            colidx, val = np.zeros(1, np.int32), np.zeros(1)
        s = cls.__new__(cls)
        s.ctx = ctx
        s.n, s.n_cols, s.nnz = n, int(n if n_cols is None else n_cols), nnz
        h = C.c_void_p()
        check(_lib.lib().cudamat_solver_create_host(ctx.h, s.n, s.n_cols, s.nnz, _vp(rowptr), _vp(colidx), _vp(val), base, C.byref(h)))
        s.h = h
        s._keep = []
        return s

    def close(self):
        if self.h:
            _lib.lib().cudamat_solver_destroy(self.h)
            self.h = None

    def set_shift(self, d):
        self._keep.append(d)
        check(_lib.lib().cudamat_solver_set_shift(self.h, _ptr(d)))

    def set_comm(self, comm):
        """comm: a _lib.Comm (kept alive here) or None"""
        self._keep.append(comm)
        check(_lib.lib().cudamat_solver_set_comm(self.h, None if comm is None else C.byref(comm)))

    def ilu0(self, shift=None):
        """ILU(0) of the matrix, or -- shift: a device vector of n doubles, read during the call only and independent of
        set_shift -- of A0 + diag(shift) (cudamat_solver_ilu0_shift: one GPU, whole matrix)"""
        if shift is None:
            check(_lib.lib().cudamat_solver_ilu0(self.h))
        else:
            check(_lib.lib().cudamat_solver_ilu0_shift(self.h, _ptr(shift)))

    def ilu0_shifted(self):
        """True when the factors are those of a shifted matrix (ilu0(shift=...)): a solver shift may then be preconditioned"""
        y = C.c_int()
        check(_lib.lib().cudamat_solver_ilu0_shifted(self.h, C.byref(y)))
        return bool(y.value)

    def ilu0_refactor(self, shift=None):
        """numeric-only refactorisation (cudamat_solver_ilu0_refactor): the values of the factors the solver holds become those of
        A0 + diag(shift) (a device vector of n doubles, read during the call only; None: of A0); the level analysis, the split,
        the maps and the permuted matrix are kept.  Bit-identical to a fresh ilu0(shift)."""
        check(_lib.lib().cudamat_solver_ilu0_refactor(self.h, None if shift is None else _ptr(shift)))

    def ilu0_refactor_info(self):
        """(refactorisations since the set-up of the current factors, wall seconds of the last one, device bytes of the value maps)"""
        cnt, sec, nb = C.c_int(), C.c_double(), C.c_size_t()
        check(_lib.lib().cudamat_solver_ilu0_refactor_info(self.h, C.byref(cnt), C.byref(sec), C.byref(nb)))
        return cnt.value, sec.value, nb.value

    def set_values(self, val):
        """new values on the kept structure (cudamat_solver_set_values): val holds nnz doubles in the CSR order of the creation --
        a DeviceArray, a torch tensor or a raw device pointer, read during the call only, or a host numpy array, which is
        uploaded to a temporary that is freed after the call.  Bit-identical to a solver created from the new values; the
        ILU(0) factors stay those of the old ones until ilu0_refactor()."""
        if isinstance(val, np.ndarray):
            a = _np(val, np.float64)
            assert a.size == self.nnz, "set_values: %d values for %d entries" % (a.size, self.nnz)
            tmp = self.ctx.array(a if self.nnz else np.zeros(1))
            try:
                check(_lib.lib().cudamat_solver_set_values(self.h, tmp.ptr))
            finally:
                tmp.free()
        else:
            check(_lib.lib().cudamat_solver_set_values(self.h, _ptr(val)))

    def symmetry(self):
        """(unmatched, max_abs_diff) of the matrix held (cudamat_solver_symmetry): stored off-diagonal entries without a
        transposed partner, and max |a_ij - a_ji| over the others.  (0, 0.0): symmetric.  Kept until set_values()."""
        lone, diff = C.c_longlong(), C.c_double()
        check(_lib.lib().cudamat_solver_symmetry(self.h, C.byref(lone), C.byref(diff)))
        return lone.value, diff.value

    def set_values_info(self):
        """(calls since the creation, wall seconds of the last one, device bytes of the value maps, 1 when the last call changed
        the storage class and the SpMV form is chosen again)"""
        cnt, sec, nb, reb = C.c_int(), C.c_double(), C.c_size_t(), C.c_int()
        check(_lib.lib().cudamat_solver_set_values_info(self.h, C.byref(cnt), C.byref(sec), C.byref(nb), C.byref(reb)))
        return cnt.value, sec.value, nb.value, reb.value

    def trsv_form(self):
        """1: dependency-driven triangular solves, 0: one launch per level"""
        f = C.c_int()
        check(_lib.lib().cudamat_solver_trsv_form(self.h, C.byref(f)))
        return f.value

    def block_ilu0(self):
        """ILU(0) of this rank's diagonal block (block-Jacobi; the only preconditioner of a sharded solver)"""
        check(_lib.lib().cudamat_solver_block_ilu0(self.h))

    def ilu0_values(self):
        cnt = C.c_int64()
        check(_lib.lib().cudamat_solver_ilu0_nnz(self.h, C.byref(cnt)))
        out = self.ctx.empty(max(cnt.value, 1))
        check(_lib.lib().cudamat_solver_ilu0_values(self.h, out.ptr))
        v = out.download()[:cnt.value]
        out.free()
        return v

    def precond_apply(self, vin, vout):
        check(_lib.lib().cudamat_solver_precond_apply(self.h, _ptr(vin), _ptr(vout)))

    def precond_apply_many(self, nrhs, In, ldin, Out, ldout):
        """Out_j = U^-1 L^-1 In_j for nrhs column-major device blocks (leading dimensions ldin, ldout): up to 8 columns per
        pass over the factors; column j is bit-identical to precond_apply of column j"""
        check(_lib.lib().cudamat_solver_precond_apply_many(self.h, int(nrhs), _ptr(In), int(ldin), _ptr(Out), int(ldout)))

    def trsm_kernel(self, nrhs):
        """name(s) of the kernel(s) precond_apply_many launches per factor for a batch of nrhs columns, e.g.
        "L: k_trsm_lds<8, 4>; U: k_trsm_level<8, 4> + k_trsm_small_levels<8, 4>"; "" when the factors are not covered and
        run column by column"""
        buf = C.create_string_buffer(160)
        check(_lib.lib().cudamat_solver_trsm_kernel(self.h, int(nrhs), buf, 160))
        return buf.value.decode()

    def spmv(self, x, y):
        check(_lib.lib().cudamat_solver_spmv(self.h, _ptr(x), _ptr(y)))

    def spmv_mode(self):
        """0: lanes-per-row CSR kernel, 1: blocked two-phase kernels (chosen by the analysis)"""
        m = C.c_int()
        check(_lib.lib().cudamat_solver_spmv_mode(self.h, C.byref(m)))
        return m.value

    def spmv_kernel(self):
        """name(s) of the kernel(s) one SpMV launch runs, as a kernel trace shows them"""
        buf = C.create_string_buffer(96)
        check(_lib.lib().cudamat_solver_spmv_kernel(self.h, buf, 96))
        return buf.value.decode()

    def placement(self):
        """where the blocked copy's arrays went: {"placed": 1 / 0 / -1 (not tried), "slabs", "seconds", "classes"} (include/cudamat.h)"""
        placed, slabs, sec = C.c_int(), C.c_int(), C.c_double()
        buf = C.create_string_buffer(256)
        check(_lib.lib().cudamat_solver_placement(self.h, C.byref(placed), C.byref(slabs), C.byref(sec), buf, 256))
        return {"placed": placed.value, "slabs": slabs.value, "seconds": sec.value, "blocks_by_class": buf.value.decode().strip()}

    def value_dict(self):
        """distinct values when the selected SpMV form reads 8-bit indices into a value dictionary, else 0"""
        m = C.c_int()
        check(_lib.lib().cudamat_solver_value_dict(self.h, C.byref(m)))
        return m.value

    def solve(self, b, x, precond=PRECOND_NONE, loop=LOOP_PBICGSTAB, maxit=2000, tol=1e-8, flags=0):
        st = Stats()
        check(_lib.lib().cudamat_solver_solve(self.h, _ptr(b), _ptr(x), precond, loop, maxit, tol, flags,
                                              C.byref(st)))
        return st

    def history(self, cap=1 << 16, col=None):
        """residual history of the last solve; col=j: of column j of the last solve_many"""
        if col is not None:
            return self.history_col(col, cap)
        buf = np.empty(cap)
        cnt = C.c_int()
        check(_lib.lib().cudamat_solver_history(self.h, _vp(buf), cap, C.byref(cnt)))
        return buf[:cnt.value].copy()

    def history_col(self, col, cap=1 << 16):
        buf = np.empty(cap)
        cnt = C.c_int()
        check(_lib.lib().cudamat_solver_history_col(self.h, int(col), _vp(buf), cap, C.byref(cnt)))
        return buf[:cnt.value].copy()

    def spmm(self, nrhs, X, ldx, Y, ldy):
        """Y = (A + diag d) X for nrhs column-major device blocks (leading dimensions ldx, ldy)"""
        check(_lib.lib().cudamat_solver_spmm(self.h, int(nrhs), _ptr(X), int(ldx), _ptr(Y), int(ldy)))

    def solve_many(self, nrhs, B, ldb, X, ldx, precond=PRECOND_NONE, loop=LOOP_PBICGSTAB, maxit=2000, tol=1e-8, flags=0):
        """nrhs right-hand sides (column-major device blocks): returns (list of Stats, form) -- form 1 batched, 0 column by
        column"""
        st = (Stats * max(int(nrhs), 1))()
        form = C.c_int(0)
        check(_lib.lib().cudamat_solver_solve_many(self.h, int(nrhs), _ptr(B), int(ldb), _ptr(X), int(ldx), precond, loop,
                                                   maxit, tol, flags, st, C.byref(form)))
        return [st[j] for j in range(int(nrhs))], form.value

    def spmm_shifts(self, nrhs, X, ldx, D, ldd, Y, ldy):
        """Y_j = (A0 + diag D_j) X_j for nrhs column-major device blocks: one shift vector per column, which replaces the
        solver's own shift for this call only"""
        check(_lib.lib().cudamat_solver_spmm_shifts(self.h, int(nrhs), _ptr(X), int(ldx), _ptr(D), int(ldd), _ptr(Y), int(ldy)))

    def solve_shifts(self, nrhs, D, ldd, B, ldb, X, ldx, precond=PRECOND_NONE, loop=LOOP_PBICGSTAB, maxit=2000, tol=1e-8,
                     flags=0):
        """(A0 + diag D_j) x_j = b_j for nrhs column-major device blocks, otherwise as solve_many: returns (list of Stats, form)"""
        st = (Stats * max(int(nrhs), 1))()
        form = C.c_int(0)
        check(_lib.lib().cudamat_solver_solve_shifts(self.h, int(nrhs), _ptr(D), int(ldd), _ptr(B), int(ldb), _ptr(X), int(ldx),
                                                     precond, loop, maxit, tol, flags, st, C.byref(form)))
        return [st[j] for j in range(int(nrhs))], form.value

    def solve_shifts_ilu0(self, nrhs, D, ldd, B, ldb, X, ldx, maxit=2000, tol=1e-8, flags=0):
        """(A0 + diag D_j) x_j = b_j with the ILU(0) of A0 + diag D_j as column j's preconditioner (the reference loop; one set
        of factors per column, K-wide under MANY_PRECOND = batched | auto): returns (list of Stats, form)"""
        st = (Stats * max(int(nrhs), 1))()
        form = C.c_int(0)
        check(_lib.lib().cudamat_solver_solve_shifts_ilu0(self.h, int(nrhs), _ptr(D), int(ldd), _ptr(B), int(ldb), _ptr(X), int(ldx),
                                                          maxit, tol, flags, st, C.byref(form)))
        return [st[j] for j in range(int(nrhs))], form.value

    def precond_apply_shifts(self, nrhs, D, ldd, In, ldin, Out, ldout):
        """Out_j = U_j^-1 L_j^-1 In_j with the factors of A0 + diag D_j: column j is bit-identical to precond_apply after
        ilu0(shift=D_j)"""
        check(_lib.lib().cudamat_solver_precond_apply_shifts(self.h, int(nrhs), _ptr(D), int(ldd), _ptr(In), int(ldin), _ptr(Out),
                                                             int(ldout)))

    def ilu0_shifts_values(self, nrhs, D, ldd):
        """array of shape (entries of the factors, nrhs): column j is what ilu0_values() returns after ilu0(shift=D_j)"""
        nrhs = int(nrhs)
        if nrhs == 0:
            return np.zeros((0, 0))
        cnt = C.c_int64(self.nnz)       # one GPU, whole matrix: the factors share the matrix's pattern
        ld = max(cnt.value, 1)
        out = self.ctx.empty(ld * nrhs)
        try:
            check(_lib.lib().cudamat_solver_ilu0_shifts_values(self.h, nrhs, _ptr(D), int(ldd), out.ptr, ld))
            return out.download().reshape(nrhs, ld)[:, :cnt.value].T.copy()
        finally:
            out.free()
