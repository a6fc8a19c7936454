"""GPU parity for the dense solve (dense_kernels.hip): bit for bit against tests/dense_ref.py on
random systems, on systems pivoting off the diagonal at every column and on tied pivot candidates;
a singular and a NaN system among good ones; independence of the batch and of the host entry's
chunking; the normwise backward error against the reference's own."""
import numpy as np
import pytest

from tests import dense_cases as dc
from tests import dense_ref as dr

pytestmark = pytest.mark.gpu


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.int64)


def same(x, y):
    return np.array_equal(bits(x), bits(y))


def same_nan(x, y):
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    nx = np.isnan(x)
    return x.shape == y.shape and np.array_equal(nx, np.isnan(y)) and same(x[~nx], y[~nx])


def agrees(got, want):
    return (same_nan(got["X"], want["X"]) and np.array_equal(got["status"], want["status"])
            and np.array_equal(got["fail"], want["fail"]))


GENERATORS = {"random": dc.random_systems, "off_diagonal": dc.off_diagonal_pivots,
              "tied": dc.tied_pivots}


@pytest.mark.parametrize("kind", sorted(GENERATORS))
@pytest.mark.parametrize("n_c", [1, 5])
@pytest.mark.parametrize("n", dc.SIZES)
def test_solve_is_the_restatement_bit_for_bit(gpu, pkg, n, n_c, kind):
    for R in dc.rhs_counts(n):
        A, B = GENERATORS[kind](n, R, n_c, 100 * n + 10 * n_c + R)
        A0, B0 = A.copy(), B.copy()
        got, want = pkg.dense_solve_batch(A, B), dr.solve_batch(A, B)
        assert got["X"].shape == (n_c, n, R) and agrees(got, want), (kind, n, R, n_c)
        assert same(A, A0) and same(B, B0)  # the inputs are not modified
        if kind != "tied":  # (tied integer systems may be singular: the restatement says which)
            assert not got["status"].any() and (got["fail"] == -1).all()


def test_more_rows_than_threads(gpu, pkg):
    """n = 1030 > 1,024 threads: the pivot scan and the multipliers take a second trip."""
    A, B = dc.random_systems(1030, 1, 1, 1030)
    assert agrees(pkg.dense_solve_batch(A, B), dr.solve_batch(A, B))


def test_vector_right_hand_side_and_a_single_system(gpu, pkg):
    A, B = dc.random_systems(33, 1, 3, 11)
    full = pkg.dense_solve_batch(A, B)
    vec = pkg.dense_solve_batch(A, B[:, :, 0])
    assert vec["X"].shape == (3, 33) and same(vec["X"], full["X"][:, :, 0])
    one = pkg.dense_solve_batch(A[1], B[1])
    assert one["X"].shape == (1, 33, 1) and same(one["X"][0], full["X"][1])


@pytest.mark.parametrize("n,R", [(5, 3), (33, 1), (70, 70)])
def test_a_system_does_not_depend_on_its_batch(gpu, pkg, n, R):
    """The same systems permuted, alone, listed twice and staged 1, 3 or all at a time."""
    A, B = dc.random_systems(n, R, 5, 300 + n)
    base = pkg.dense_solve_batch(A, B)
    perm = np.array([3, 0, 4, 4, 1, 2, 0])
    got = pkg.dense_solve_batch(A[perm], B[perm])
    assert same(got["X"], base["X"][perm])
    for c in range(5):
        solo = pkg.dense_solve_batch(A[c:c + 1], B[c:c + 1])
        assert same(solo["X"][0], base["X"][c]) and solo["status"][0] == 0
    for chunk in (1, 3, 5, 64):
        assert agrees(pkg.dense_solve_batch(A, B, chunk=chunk), base)


@pytest.mark.parametrize("n,R", [(5, 3), (33, 1), (70, 5)])
def test_a_failed_system_stays_where_it_is(gpu, pkg, n, R):
    """Two equal rows (an exact zero pivot), a NaN on the diagonal at its turn and an infinite
    entry: status 1, the reference's `fail`, X NaN; the neighbours keep their solo bits."""
    A, B = dc.random_systems(n, R, 6, 400 + n)
    A[1][n - 1] = A[1][0]  # equal rows stay bit-equal until one is the pivot row: l = 1, zeros
    A[3][0, 0] = np.nan
    A[4][n // 2, n // 2] = np.inf
    got, want = pkg.dense_solve_batch(A, B), dr.solve_batch(A, B)
    assert agrees(got, want)
    assert list(got["status"]) == [0, 1, 0, 1, 1, 0]
    assert got["fail"][3] == 0 and got["fail"][1] == n - 1 and got["fail"][0] == -1
    for c in (1, 3, 4):
        assert np.isnan(got["X"][c]).all()
    for c in (0, 2, 5):
        solo = pkg.dense_solve_batch(A[c:c + 1], B[c:c + 1])
        assert same(solo["X"][0], got["X"][c]) and not np.isnan(got["X"][c]).any()


def test_a_nan_below_the_diagonal_is_never_taken(gpu, pkg):
    """NaNs in column 0 below row 0 are passed over by the scan; they reach later pivots through
    the elimination and stop the system there, as the restatement says."""
    A, B = dc.random_systems(5, 1, 2, 77)
    A[0][2, 0] = np.nan
    got, want = pkg.dense_solve_batch(A, B), dr.solve_batch(A, B)
    assert agrees(got, want) and got["status"][0] == 1 and got["fail"][0] == 2
    assert got["status"][1] == 0


@pytest.mark.parametrize("n,R,n_c,seed", dc.BACKWARD_CASES)
def test_backward_error_against_the_references_own(gpu, pkg, n, R, n_c, seed):
    """‖A·x − b‖∞ / (‖A‖∞·‖x‖∞ + ‖b‖∞) <= c·n·2⁻⁵² with c = 4 × the largest value the restatement
    itself reaches on these inputs (dense_cases.BACKWARD_MEASURED = 0.07394, so c = 0.29576;
    LAPACK's own largest value on them is 0.0135)."""
    A, B = dc.well_conditioned(n, R, n_c, seed)
    got = pkg.dense_solve_batch(A, B)
    assert not got["status"].any()
    worst = 0.0
    for c in range(n_c):
        for q in range(R):
            worst = max(worst, dr.backward_error(A[c], got["X"][c][:, q], B[c][:, q]))
    print(f"n = {n}, R = {R}: backward error {worst / (n * 2.0 ** -52):.5f} n·2⁻⁵²")
    assert worst <= dc.BACKWARD_C * n * 2.0 ** -52


def test_dev_entry_on_torch_tensors(gpu, pkg):
    import torch
    A, B = dc.random_systems(33, 3, 4, 909)
    dA, dB = torch.from_numpy(A).to(gpu), torch.from_numpy(B).to(gpu)
    X = torch.empty_like(dB)
    work = torch.empty((4, 33, 36), dtype=torch.float64, device=gpu)
    st = torch.full((4,), 7, dtype=torch.int32, device=gpu)
    fl = torch.full((4,), 7, dtype=torch.int32, device=gpu)
    pkg.dense_solve_batch_dev(dA, dB, X, work, st, fl)
    torch.cuda.synchronize()
    want = dr.solve_batch(A, B)
    assert same(X.cpu().numpy(), want["X"]) and same(dA.cpu().numpy(), A)
    assert st.cpu().tolist() == [0] * 4 and fl.cpu().tolist() == [-1] * 4
