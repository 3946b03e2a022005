"""The two roundings of the SpMV row epilogue  y = alpha (A x + d .* x) + beta y0  (csrc/device.h), as CPU mirrors.

  fused: fma(beta, y0, fl(alpha * fma(d, x, s)))         spmv_finish_row_fused / spmm_finish_row: every kernel of
                                                         spmv_csr.hip, k_spmm_csr
  exact: fl(fl(alpha * fl(s + fl(d x))) + fl(beta y0))   spmv_finish_row_exact (pattern, SELL) and the blocked form: one
                                                         rounding per product and per sum, the oracle's csrmv

A and x are integer-valued, so the row sum s = (A x)_i is exact in any order and under either rounding: whatever differs
between a kernel and a mirror is the epilogue.  d, y0 (normal, fixed seeds), alpha = 1.7 and beta = -0.3 are real.
The GPU tests that pin every kernel to its mirror are in test_gpu_parity.py (test_epilogue_rounding_*); here, without a
GPU, the check that they can tell the two roundings apart at all."""
import functools
from fractions import Fraction

import numpy as np

ALPHA, BETA = 1.7, -0.3
MIN_DIFFERING_ROWS = 20      # fewer rows than this between the two mirrors: the pinning tests would be vacuous
KMAX = 8                     # columns of the multi-column inputs


def fma(a, b, c):
    """a * b + c with ONE rounding: exact rational arithmetic (what fractions.Fraction does, without reducing the
    fraction at every step), rounded by the int / int true division, which rounds correctly"""
    (na, da), (nb, db), (nc, dc) = float(a).as_integer_ratio(), float(b).as_integer_ratio(), float(c).as_integer_ratio()
    return (na * nb * dc + nc * da * db) / (da * db * dc)


def fma_fraction(a, b, c):
    return float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def fused_dx(d, x, s):
    return np.array([fma(di, xi, si) for di, xi, si in zip(d, x, s)])


def fused(alpha, beta, d, x, s, y0):
    u = alpha * fused_dx(d, x, s)
    return np.array([fma(beta, yi, ui) for yi, ui in zip(y0, u)]) if beta != 0.0 else u


def exact(alpha, beta, d, x, s, y0):
    dx = d * x                   # (numpy rounds every elementwise operation once)
    sum_ = s + dx
    out = alpha * sum_
    return out + beta * y0 if beta != 0.0 else out


@functools.lru_cache(maxsize=None)
def case(which):
    """which: "poisson" (rows of <= 5 entries: stream tiles, row patterns), "poisson_dict" (the same stencil with 2^20
    entries, the fewest for which a solver builds a value dictionary: k_spmv_stream_d, k_spmv_pat_d) or "rand" (rows of 50:
    lanes per row, tiles, SELL, blocked, SpMM; KMAX columns).  Returns a dict; the arrays are shared between tests and must
    not be written."""
    from oracle import oracle as O
    O.build()
    A = {"poisson": lambda: O.poisson5(40, 30), "poisson_dict": lambda: O.poisson5(460, 460),
         "rand": lambda: O.rand_rows(600, 50, 0x5EED)}[which]()
    n, cols = A.n, KMAX if which == "rand" else 1
    assert which != "poisson_dict" or A.nnz >= 1 << 20
    # The two roundings part where d x cancels against s (the sum's exponent drops below the product's, so the product's own
    # rounding error shows); where d x dwarfs s both give s + fl(d x).  That needs |d x| ~ |s|: the row sums are ~370 (rms) in
    # the random matrix and ~20 in the stencil, |x| ~ 5: d and y0 are 100 x standard normal there and 10 x here.
    scale = 100.0 if which == "rand" else 10.0
    X = np.random.default_rng(101).integers(-8, 9, (n, cols)).astype(np.float64)
    D = scale * np.random.default_rng(102).standard_normal((n, cols))
    y0 = scale * np.random.default_rng(103).standard_normal(n)
    S = np.stack([O.spmv(A, np.ascontiguousarray(X[:, j])) for j in range(cols)], axis=1)      # exact: integers
    assert np.all(S == np.rint(S)) and np.all(np.abs(S) < 2.0 ** 40)
    c = {"A": A, "n": n, "cols": cols, "X": X, "D": D, "y0": y0, "S": S, "x": X[:, 0], "d": D[:, 0], "s": S[:, 0]}
    # through a solver: y = (A + diag d) x, alpha = 1, beta = 0; column j of the multi-column products
    c["fused_shift"] = np.stack([fused_dx(c["d"], X[:, j], S[:, j]) for j in range(cols)], axis=1)       # the solver's one shift
    c["fused_shifts"] = np.stack([fused_dx(D[:, j], X[:, j], S[:, j]) for j in range(cols)], axis=1)     # a shift per column
    # standalone SpMV: alpha, beta and d at once (no standalone form reads a dictionary)
    if which != "poisson_dict":
        c["fused"] = fused(ALPHA, BETA, c["d"], c["x"], c["s"], y0)
        c["exact"] = exact(ALPHA, BETA, c["d"], c["x"], c["s"], y0)
    c["exact_shift"] = O.csrmv(A, 1.0, c["x"], 1.0, c["x"] * c["d"])
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def differing(a, b):
    return int(np.count_nonzero(a != b))


def assert_not_vacuous(c, columns=(0,)):
    """the two mirrors must disagree in enough rows for an assert_array_equal against one of them to mean something"""
    assert "fused" not in c or differing(c["fused"], c["exact"]) >= MIN_DIFFERING_ROWS
    assert differing(c["fused_shift"][:, 0], c["exact_shift"]) >= MIN_DIFFERING_ROWS
    for j in columns:
        assert differing(c["fused_shift"][:, j], exact(1.0, 0.0, c["d"], c["X"][:, j], c["S"][:, j], None)) >= MIN_DIFFERING_ROWS
        assert differing(c["fused_shifts"][:, j], exact(1.0, 0.0, c["D"][:, j], c["X"][:, j], c["S"][:, j], None)) >= MIN_DIFFERING_ROWS


def test_the_two_epilogue_mirrors_differ():
    """without a GPU: on the inputs of the pinning tests the fused and the exact epilogue differ in >= 20 rows -- in the
    standalone form (alpha, beta, d), in the solver's shifted product, and in every column of the multi-column products.
    The exact mirror written out here is the oracle's csrmv."""
    for which in ("poisson", "poisson_dict", "rand"):
        c = case(which)
        assert_not_vacuous(c, columns=range(c["cols"]))
        np.testing.assert_array_equal(exact(1.0, 0.0, c["d"], c["x"], c["s"], None), c["exact_shift"])
        print(which, "rows", c["n"], "standalone", differing(c["fused"], c["exact"]) if "fused" in c else "-", "shifted",
              differing(c["fused_shift"][:, 0], c["exact_shift"]))
    c = case("rand")        # the mirror's fma is the textbook one
    for di, xi, si, yi in zip(c["d"], c["x"], c["s"], c["y0"]):
        assert fma(di, xi, si) == fma_fraction(di, xi, si) and fma(BETA, yi, ALPHA * si) == fma_fraction(BETA, yi, ALPHA * si)
