"""Inputs of the dense-solve tests, shared by the GPU tests and the CPU checks of the reference."""
import numpy as np

SIZES = [1, 2, 5, 33, 70]


def rhs_counts(n):
    return sorted({1, 3, n})


def random_systems(n, R, C, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((C, n, n)), rng.standard_normal((C, n, R))


def off_diagonal_pivots(n, R, C, seed):
    """Small noise plus a large cyclic permutation: the pivot of column j sits in a row other than
    j at every column but (where n > 1) the last, where one row is left."""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((C, n, n)) * 2.0 ** -6
    for j in range(n):
        A[:, (j + 1) % n, j] += 4.0 + rng.random(C)
    return A, rng.standard_normal((C, n, R))


def tied_pivots(n, R, C, seed):
    """Integer entries with every column's candidates ±3: at column 0 all n rows tie and row 0
    must win; the later columns tie or not as the exact integer elimination leaves them."""
    rng = np.random.default_rng(seed)
    A = rng.integers(-2, 3, (C, n, n)).astype(np.float64)
    A[:, :, 0] = np.where(rng.random((C, n)) < 0.5, -3.0, 3.0)
    return A, rng.integers(-4, 5, (C, n, R)).astype(np.float64)


def well_conditioned(n, R, C, seed):
    """Random normal entries with n on the diagonal (cond∞ of a few units)."""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((C, n, n)) + n * np.eye(n)
    return A, rng.standard_normal((C, n, R))


# test 8's inputs: (n, R, C, seed)
BACKWARD_CASES = [(5, 3, 5, 801), (33, 3, 5, 802), (70, 1, 5, 803), (70, 70, 2, 804)]
# The reference's own backward error on BACKWARD_CASES, in units of n·2⁻⁵², measured on the CPU
# (tests/test_dense_solve_cpu.py re-measures it): the largest is BACKWARD_MEASURED; the bound of
# the GPU test is four times that.
BACKWARD_MEASURED = 0.07394  # met at n = 5; LAPACK's on the same inputs: 0.0135
BACKWARD_C = 4 * BACKWARD_MEASURED
