"""CPU restatement of aiy_dense_solve_batch (include/aiyagari_hip.h, "Dense solve"): Gaussian
elimination with partial pivoting in the header's operation order.  Elementwise numpy rounds every
multiplication, subtraction and division on its own (no fused multiply-add), so the GPU kernel is
compared bit for bit."""
import numpy as np


def pivot_scan(col):
    """The header's scan, literally: p = 0, best = |col[0]|; i ascending: |col[i]| > best takes
    it."""
    p, best = 0, abs(col[0])
    for i in range(1, len(col)):
        if abs(col[i]) > best:
            p, best = i, abs(col[i])
    return p, best


def pivot(col):
    """pivot_scan without the Python loop.  A NaN first entry is never replaced (nothing compares
    larger than a NaN); otherwise a NaN further down never compares larger than the running best,
    so it counts as −1, and argmax returns the first of equal maxima: the lowest index."""
    a = np.abs(col)
    if np.isnan(a[0]):
        return 0, a[0]
    p = int(np.argmax(np.where(np.isnan(a), -1.0, a)))
    return p, a[p]


def solve(A, B, pivots=None):
    """One system: A [n][n], B [n][R] -> (X [n][R], status, fail).  pivots: a list that receives
    the pivot row p of every column reached."""
    A = np.array(A, np.float64)
    B = np.array(B, np.float64)
    n, R = B.shape
    for j in range(n):
        p, best = pivot(A[j:, j])
        p += j
        if pivots is not None:
            pivots.append(p)
        if not (best > 0) or not np.isfinite(best):
            return np.full((n, R), np.nan), 1, j
        if p != j:
            A[[j, p]] = A[[p, j]]
            B[[j, p]] = B[[p, j]]
        with np.errstate(all="ignore"):
            l = A[j + 1:, j] / A[j, j]
            A[j + 1:, j + 1:] = A[j + 1:, j + 1:] - l[:, None] * A[j, j + 1:][None, :]
            B[j + 1:] = B[j + 1:] - l[:, None] * B[j][None, :]
    X = np.empty((n, R))
    with np.errstate(all="ignore"):
        for j in range(n - 1, -1, -1):
            X[j] = B[j] / A[j, j]
            B[:j] = B[:j] - A[:j, j][:, None] * X[j][None, :]
    return X, 0, -1


def solve_batch(A, B):
    """A [C][n][n], B [C][n][R] -> dict(X, status, fail), each system on its own."""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    out = [solve(A[c], B[c]) for c in range(A.shape[0])]
    return dict(X=np.stack([o[0] for o in out]),
                status=np.array([o[1] for o in out], np.int32),
                fail=np.array([o[2] for o in out], np.int32))


def dense_solve_batch(A, B, chunk=0):
    """solve_batch with estimation.dense_solve_batch's signature: B [C][n] gives X [C][n]."""
    B = np.asarray(B, np.float64)
    if B.ndim == 2:
        out = solve_batch(A, B[:, :, None])
        out["X"] = out["X"][:, :, 0]
        return out
    return solve_batch(A, B)


def backward_error(A, x, b):
    """The normwise backward error ‖A·x − b‖∞ / (‖A‖∞·‖x‖∞ + ‖b‖∞) of one right-hand side, the
    residual formed in extended precision."""
    A, x, b = (np.asarray(v, np.longdouble) for v in (A, x, b))
    r = np.max(np.abs(A @ x - b))
    den = np.max(np.sum(np.abs(A), axis=1)) * np.max(np.abs(x)) + np.max(np.abs(b))
    return float(r / den)
