"""No GPU: the dense solve's CPU restatement (tests/dense_ref.py) against LAPACK, what the special
pivot inputs of the GPU tests really do, the measured backward-error constant the GPU test's bound
comes from, and which refusal each entry answers before it asks for a device."""
import ctypes as C

import numpy as np
import pytest

from tests import dense_cases as dc
from tests import dense_ref as dr

i64 = C.c_int64
NO_DEVICE = (5, "no HIP device visible")


# ------------------------------------------------------------------ the restatement itself
@pytest.mark.parametrize("n", dc.SIZES)
def test_restatement_solves_the_system(n):
    A, B = dc.well_conditioned(n, 3, 2, n)
    R = dr.solve_batch(A, B)
    assert not R["status"].any() and (R["fail"] == -1).all()
    assert np.allclose(R["X"], np.linalg.solve(A, B), rtol=1e-12, atol=1e-14)


def test_vectorised_pivot_is_the_literal_scan():
    rng = np.random.default_rng(3)
    for trial in range(200):
        col = rng.integers(-3, 4, rng.integers(1, 9)).astype(np.float64)
        col[rng.random(col.size) < 0.2] = np.nan
        if trial % 7 == 0:
            col[rng.integers(col.size)] = np.inf
        p, best = dr.pivot(col)
        q, want = dr.pivot_scan(col)
        assert p == q and (best == want or (np.isnan(best) and np.isnan(want))), col


@pytest.mark.parametrize("n", dc.SIZES)
def test_the_pivot_inputs_do_what_they_say(n):
    """Off-diagonal: every column with more than one row left swaps.  Tied: all of column 0 has
    one magnitude and row 0 keeps the pivot."""
    A, B = dc.off_diagonal_pivots(n, 1, 2, 100 * n + 11)
    for c in range(2):
        piv = []
        assert dr.solve(A[c], B[c], piv)[1] == 0
        assert all(p != j for j, p in enumerate(piv[:-1])) and piv[-1] == n - 1
    A, B = dc.tied_pivots(n, 1, 2, 100 * n + 11)
    for c in range(2):
        piv = []
        dr.solve(A[c], B[c], piv)
        assert piv[0] == 0 and (np.abs(A[c][:, 0]) == 3).all()


def test_failures_of_the_restatement():
    A, B = dc.random_systems(5, 2, 1, 9)
    A[0][4] = A[0][0]
    X, st, fl = dr.solve(A[0], B[0])
    assert (st, fl) == (1, 4) and np.isnan(X).all()
    A, B = dc.random_systems(5, 2, 1, 9)
    A[0][0, 0] = np.nan
    assert dr.solve(A[0], B[0])[1:] == (1, 0)
    A[0][0, 0] = np.inf
    assert dr.solve(A[0], B[0])[1:] == (1, 0)


def test_the_measured_backward_error_constant():
    """The GPU test's bound is 4 × the largest backward error, in units of n·2⁻⁵², the restatement
    reaches on dense_cases.BACKWARD_CASES: measured 0.07393 (n = 5); LAPACK on the same inputs:
    0.0135.  The recorded constant must cover what is measured here."""
    worst = 0.0
    for n, R, n_c, seed in dc.BACKWARD_CASES:
        A, B = dc.well_conditioned(n, R, n_c, seed)
        X = dr.solve_batch(A, B)["X"]
        for c in range(n_c):
            for q in range(R):
                e = dr.backward_error(A[c], X[c][:, q], B[c][:, q]) / (n * 2.0 ** -52)
                worst = max(worst, e)
    print(f"largest backward error of the restatement: {worst:.5f} n·2⁻⁵²")
    assert 0.9 * dc.BACKWARD_MEASURED <= worst <= dc.BACKWARD_MEASURED
    assert dc.BACKWARD_C == 4 * dc.BACKWARD_MEASURED


# ------------------------------------------------------------------------------ refusals
def _base():
    return dict(C=3, n=4, R=2, A=np.zeros(3 * 16), B=np.zeros(3 * 8), X=np.zeros(3 * 8),
                W=np.zeros(3 * 24), st=np.zeros(3, np.int32), fl=np.zeros(3, np.int32), chunk=0)


DEFECTS = {
    "valid": lambda a: None, "C0": lambda a: a.update(C=0), "n0": lambda a: a.update(n=0),
    "n4097": lambda a: a.update(n=4097), "R0": lambda a: a.update(R=0),
    "big": lambda a: a.update(n=4096, R=2 ** 19), "chunk_neg": lambda a: a.update(chunk=-1),
    "null:A": lambda a: a.update(A=None), "null:B": lambda a: a.update(B=None),
    "null:X": lambda a: a.update(X=None), "null:W": lambda a: a.update(W=None),
    "null:st": lambda a: a.update(st=None), "null:fl": lambda a: a.update(fl=None),
}


def _p(x):
    return None if x is None else x.ctypes.data_as(C.c_void_p)


def _host(L, a):
    return L.aiy_dense_solve_batch(i64(a["C"]), i64(a["n"]), i64(a["R"]), _p(a["A"]), _p(a["B"]),
                                   _p(a["X"]), _p(a["st"]), _p(a["fl"]), i64(a["chunk"]))


def _dev(L, a):
    return L.aiy_dense_solve_batch_dev(i64(a["C"]), i64(a["n"]), i64(a["R"]), _p(a["A"]),
                                       _p(a["B"]), _p(a["X"]), _p(a["W"]), _p(a["st"]),
                                       _p(a["fl"]), None)


CALLERS = {"aiy_dense_solve_batch": _host, "aiy_dense_solve_batch_dev": _dev}
NULL = (6, "NULL argument")
# (entry, defects) -> the answer; a defect pair shows which check comes first
EXPECTED = {
    ("aiy_dense_solve_batch", "null:A"): NULL,
    ("aiy_dense_solve_batch", "null:B+C0"): NULL,
    ("aiy_dense_solve_batch", "null:X"): NULL,
    ("aiy_dense_solve_batch", "null:st"): NULL,
    ("aiy_dense_solve_batch", "null:fl+n0"): NULL,
    ("aiy_dense_solve_batch", "C0"): (1, "need 1 <= C < 2^31"),
    ("aiy_dense_solve_batch", "C0+n0"): (1, "need 1 <= C < 2^31"),
    ("aiy_dense_solve_batch", "n0"): (1, "need 1 <= n <= 4096"),
    ("aiy_dense_solve_batch", "n4097"): (1, "need 1 <= n <= 4096"),
    ("aiy_dense_solve_batch", "n0+R0"): (1, "need 1 <= n <= 4096"),
    ("aiy_dense_solve_batch", "R0"): (1, "need R >= 1"),
    ("aiy_dense_solve_batch", "R0+chunk_neg"): (1, "need R >= 1"),
    ("aiy_dense_solve_batch", "big"): (1, "need n·(n + R) < 2^31"),
    ("aiy_dense_solve_batch", "big+chunk_neg"): (1, "need n·(n + R) < 2^31"),
    ("aiy_dense_solve_batch", "chunk_neg"): (6, "chunk must be >= 0 (0: the default)"),
    ("aiy_dense_solve_batch", "valid"): NO_DEVICE,
    ("aiy_dense_solve_batch_dev", "null:W"): NULL,
    ("aiy_dense_solve_batch_dev", "null:A+C0"): NULL,
    ("aiy_dense_solve_batch_dev", "C0"): (1, "need 1 <= C < 2^31"),
    ("aiy_dense_solve_batch_dev", "n4097"): (1, "need 1 <= n <= 4096"),
    ("aiy_dense_solve_batch_dev", "R0"): (1, "need R >= 1"),
    ("aiy_dense_solve_batch_dev", "big"): (1, "need n·(n + R) < 2^31"),
}


@pytest.mark.parametrize("entry,defects", sorted(EXPECTED))
def test_dense_refusal(pkg, entry, defects):
    want = EXPECTED[(entry, defects)]
    if want == NO_DEVICE:
        import torch
        if torch.cuda.is_available():
            return  # not a refusal: with a device the call would run
    a = _base()
    for x in defects.split("+"):
        DEFECTS[x](a)
    L = pkg.lib()
    rc = CALLERS[entry](L, a)
    assert (rc, L.aiy_last_error().decode()) == want


def test_python_wrapper_refuses_bad_shapes(pkg):
    with pytest.raises(ValueError):
        pkg.dense_solve_batch(np.zeros((2, 3, 4)), np.zeros((2, 3, 1)))
    with pytest.raises(ValueError):
        pkg.dense_solve_batch(np.zeros((2, 3, 3)), np.zeros((2, 4, 1)))
