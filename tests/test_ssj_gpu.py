"""GPU parity for the sequence-space Jacobian (ssj_kernels.hip).

Expectation vectors: bit for bit against tests/support/ssj_ref.c, and the adjoint identity against
the GPU's own forward pass.  Fake-news contraction: bit for bit on data whose every product and
partial sum is exact, within the any-order summation bound n·2⁻⁵²·Σ|E·D| of math.fsum on random
data, and run-to-run identical.  jacobian() against tests/ssj_ref.jacobian_cpu, and the Newton
driver on the GPU backend against the CPU backend."""
import math

import numpy as np
import pytest

from oracle import corc
from tests import ssj_ref as sr
from tests import transition_ref as tr
from tests.test_transition_gpu import problem

pytestmark = pytest.mark.gpu


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.int64)


def same(x, y):
    return np.array_equal(bits(x), bits(y))


# ------------------------------------------------------------- expectation vectors
SHAPES = [(3, 37, 5, 3),      # more threads than states
          (7, 400, 6, 2),     # the scripts' grid: several passes of 1,024 threads
          (16, 64, 3, 2),     # N at the cap
          (2, 1024, 2, 1)]    # Na at the cap of the passes that make the policy


def _policies(pkg, N, Na, T, C):
    """Three period policies of test_transition_gpu.py's problem, and its calibration."""
    pr = problem(pkg, N, Na, T, C)
    pks = [pr["ref"][c]["pk"][t] for t in range(T) for c in range(C)]
    return pr["cal"], np.stack([pks[q % len(pks)] for q in range(3)])


def _y0(cal, seed):
    """Per-path outcomes: a_grid in every row, then two non-negative random ones."""
    N, Na = cal["N"], cal["Na"]
    rng = np.random.default_rng(seed)
    return np.stack([np.tile(cal["a_grid"], (N, 1)), rng.random((N, Na)), 3 * rng.random((N, Na))])


@pytest.mark.parametrize("N,Na,T,C", SHAPES)
def test_expectation_is_the_reference_bit_for_bit(gpu, pkg, N, Na, T, C):
    cal, pk = _policies(pkg, N, Na, T, C)
    a, P = cal["a_grid"], cal["P"]
    if (N, Na) in ((3, 37), (7, 400)):  # the clamp binds at both ends of the grid
        assert (pk > a[-1]).any() and (pk <= a[0]).any()
    y0 = _y0(cal, 3)
    G = pkg.expectation_batch(pk, y0, a, P, T)
    assert G.shape == (3, T, N, Na)
    for c in range(3):
        assert same(G[c], sr.expect(pk[c], y0[c], a, P, T)), c
        assert same(pkg.expectation_batch(pk[c:c + 1], y0[c:c + 1], a, P, T)[0], G[c]), c
    S = pkg.expectation_batch(pk, y0[1], a, P, T)  # one y₀ for every policy
    assert same(S[1], G[1])
    for c in (0, 2):
        assert same(S[c], sr.expect(pk[c], y0[1], a, P, T)), c
    assert same(pkg.expectation_batch(pk, y0, a, P, 1)[:, 0], y0)  # T = 1: E is y₀ alone


def test_a_nan_in_one_policy_stays_inside_it(gpu, pkg):
    N, Na, T, C = 7, 400, 6, 2
    cal, pk = _policies(pkg, N, Na, T, C)
    a, P, y0 = cal["a_grid"], cal["P"], _y0(cal, 4)
    good = pkg.expectation_batch(pk, y0, a, P, T)
    pk = pk.copy()
    pk[1, 3, 217] = np.nan
    G = pkg.expectation_batch(pk, y0, a, P, T)
    assert same(G[0], good[0]) and same(G[2], good[2])
    R = sr.expect(pk[1], y0[1], a, P, T)
    assert np.isnan(R[1, 3, 217]) and np.isnan(R[T - 1]).sum() > 1
    assert np.array_equal(np.isnan(G[1]), np.isnan(R))
    assert np.array_equal(G[1], R, equal_nan=True)


@pytest.mark.parametrize("N,Na,T,C", SHAPES[:2])
def test_expectation_is_the_adjoint_of_the_gpu_forward_pass(gpu, pkg, N, Na, T, C):
    """y₀ = a_grid: E_t·λ₀ is K_t of the forward pass under the constant policy, within 1e-12
    relative (every term is non-negative)."""
    cal, pk = _policies(pkg, N, Na, T, C)
    a, P = cal["a_grid"], cal["P"]
    T2 = 9
    lam0 = np.random.default_rng(8).random((3, N, Na))
    lam0 /= lam0.sum((1, 2), keepdims=True)
    E = pkg.expectation_batch(pk, np.tile(a, (N, 1)), a, P, T2 + 1)
    F = pkg.dist_forward_batch(np.repeat(pk[:, None], T2, axis=1), lam0, a, P)
    assert (F["status"] == 0).all()
    for c in range(3):
        for t in range(T2 + 1):
            lhs = float(np.sum(E[c, t] * lam0[c]))
            assert abs(lhs - F["K"][c, t]) <= 1e-12 * abs(F["K"][c, t]), (c, t)


# ------------------------------------------------------------- the contraction
def _exact_data(T, n, n_in, seed):
    """E integers in [-8, 8], Λ1 integer multiples of 2^-20 within 2^-10: with h = 2^-13 every D
    is a multiple of 2^-7 within 2^4, every product and partial sum an exact double."""
    rng = np.random.default_rng(seed)
    E = rng.integers(-8, 9, (T, n)).astype(np.float64)
    L = rng.integers(-1024, 1025, (n_in + 1, T, n)).astype(np.float64) * 2.0 ** -20
    return E, L, 2.0 ** -13


@pytest.mark.parametrize("n_in", [1, 2])
@pytest.mark.parametrize("n", [111, 2800])
@pytest.mark.parametrize("T", [1, 5, 17, 33])
def test_fake_news_on_exact_data_is_numpy_bit_for_bit(gpu, pkg, T, n, n_in):
    E, L, h = _exact_data(T, n, n_in, 100 * T + n_in)
    F, J = pkg.fake_news(E, L, h)
    Fr, Jr = sr.fake_news(E, L, h)
    assert same(F, Fr) and same(J, Jr)
    # one non-zero row of E and one of D: the T-1-s reversal and the (t, s) orientation
    t1, s1, x1 = T // 3, T - 1 - T // 4, n_in - 1
    E0 = np.zeros_like(E)
    E0[t1] = E[t1]
    L0 = np.tile(L[:1], (n_in + 1, 1, 1))
    L0[x1 + 1, T - 1 - s1] = L[x1 + 1, T - 1 - s1]
    F, J = pkg.fake_news(E0, L0, h)
    v = float(np.sum(E[t1] * ((L[x1 + 1, T - 1 - s1] - L[0, T - 1 - s1]) / h)))
    assert v != 0
    Fw, Jw = np.zeros((n_in, T, T)), np.zeros((n_in, T, T))
    Fw[x1, t1, s1] = v
    for q in range(min(T - t1, T - s1)):
        Jw[x1, t1 + q, s1 + q] = v
    assert same(F, Fw) and same(J, Jw)


def _exact_F(E, L, h):
    """(F by math.fsum of the rounded products, Σ_k |E[t][k]·D[s][k]|), each [n_in][T][T]."""
    T = E.shape[0]
    D = sr.news_rows(L, h)
    Er = E.reshape(T, -1)
    F, A = np.empty((D.shape[0], T, T)), np.empty((D.shape[0], T, T))
    for x in range(D.shape[0]):
        for t in range(T):
            for s in range(T):
                p = Er[t] * D[x, s]
                F[x, t, s] = math.fsum(p)
                A[x, t, s] = float(np.sum(np.abs(p)))
    return F, A


def _exact_J(E, L, h):
    """(J by math.fsum over the whole diagonal's products, Σ|products| of the diagonal)."""
    T = E.shape[0]
    D = sr.news_rows(L, h)
    Er = E.reshape(T, -1)
    J, A = np.empty((D.shape[0], T, T)), np.empty((D.shape[0], T, T))
    for x in range(D.shape[0]):
        for t in range(T):
            for s in range(T):
                m = min(t, s)
                p = np.concatenate([Er[t - q] * D[x, s - q] for q in range(m + 1)])
                J[x, t, s] = math.fsum(p)
                A[x, t, s] = float(np.sum(np.abs(p)))
    return J, A


@pytest.mark.parametrize("T,n", [(17, 2800), (33, 111)])
def test_fake_news_on_random_data_is_within_the_summation_bound(gpu, pkg, T, n):
    """|F − F_exact| <= n·2⁻⁵²·Σ_k|E[t][k]·D[s][k]| — the bound of any summation order of n terms,
    fused or not; two runs of the same call are bit-identical."""
    rng = np.random.default_rng(T)
    E = rng.standard_normal((T, n)) * 10
    L = rng.random((3, T, n)) / n
    h = 1e-4
    F, J = pkg.fake_news(E, L, h)
    Fx, A = _exact_F(E, L, h)
    assert (np.abs(F - Fx) <= n * 2.0 ** -52 * A).all()
    assert same(J, sr.jacobian_from_F(F))  # step 5 is sequential along each diagonal
    F2, J2 = pkg.fake_news(E, L, h)
    assert same(F, F2) and same(J, J2)
    # an entry does not depend on the other inputs of the call
    F1, J1 = pkg.fake_news(E, L[[0, 2]], h)
    assert same(F1[0], F[1]) and same(J1[0], J[1])


# ------------------------------------------------------------- the whole Jacobian
def _ss60(pkg):
    cb = pkg.calibration
    cal = cb.aiyagari(Na=60, shocks="rouwenhorst", N=3)
    return tr.steady_state_cpu(cal, 0.03, lambda r: cb.wage(r, cal["alpha"], cal["delta"]))


def _point400(pkg):
    """N = 7, Na = 400: a point to differentiate at in steady_state's form — 60 oracle EGM steps
    and 50 pushes at r = 0.03 (the comparison is arithmetic: it needs no converged point)."""
    cb = pkg.calibration
    cal = cb.aiyagari(Na=400)
    a, s, P, r = cal["a_grid"], cal["s"], cal["P"], 0.03
    w = cb.wage(r, cal["alpha"], cal["delta"])
    R = corc.egm_solve(np.tile((1 + r) * a + w * np.mean(s), (7, 1)), a, s, P, r, w, cal["beta"],
                       cal["sigma"], cal["amin"], max_iter=60)
    lam = np.full((7, 400), 1.0 / 2800)
    for _ in range(50):
        lam = corc.dist_update_lottery(lam, R["policy_k"], a, P)
    return dict(r=r, w=w, K=tr.capital_sum(lam, a), policy_c=R["policy_c"], lam=lam, cal=cal)


@pytest.mark.parametrize("which,T", [("ss60", 12), ("point400", 6)])
def test_jacobian_is_the_cpu_jacobian(gpu, pkg, which, T):
    """E and Λ1 bit for bit; F within the summation bound of the exact contraction of those same
    E and Λ1; J within the bound summed along its diagonal (its (t + 1) or fewer F entries)."""
    ss = _ss60(pkg) if which == "ss60" else _point400(pkg)
    cal, h = ss["cal"], 1e-4
    a, s, P = cal["a_grid"], cal["s"], cal["P"]
    N, Na = cal["N"], cal["Na"]
    n = N * Na
    R = sr.jacobian_cpu(ss, T, h)
    G = pkg.jacobian(ss, T, h)
    assert G["status"] == (0, 0) and set(G) >= {"J_r", "J_w", "F_r", "F_w", "E"}
    assert same(G["E"], R["E"])
    # Λ1 through the public entries that jacobian() chains: steps 1 and 2
    r, w = sr.news_paths(ss, T, h)
    B = pkg.egm_backward_batch(r, w, ss["policy_c"], a, s, P, cal["beta"], cal["sigma"],
                               cal["amin"], want_pc=False)
    assert (B["status"] == 0).all() and same(B["policy_k"], R["pk"])
    Fw = pkg.dist_forward_batch(B["policy_k"].reshape(3 * T, 1, N, Na), ss["lam"], a, P)
    assert (Fw["status"] == 0).all()
    lam1 = Fw["lam_T"].reshape(3, T, N, Na)
    assert same(lam1, R["lam1"])
    # the contraction of those bits is jacobian()'s own, bit for bit (it is deterministic)
    F, J = pkg.fake_news(G["E"], lam1, h)
    assert same(F[0], G["F_r"]) and same(F[1], G["F_w"])
    assert same(J[0], G["J_r"]) and same(J[1], G["J_w"])
    Fx, A = _exact_F(R["E"], R["lam1"], h)
    Jx, AJ = _exact_J(R["E"], R["lam1"], h)
    assert (np.abs(F - Fx) <= n * 2.0 ** -52 * A).all()
    assert (np.abs(J - Jx) <= n * 2.0 ** -52 * AJ).all()
    # and the CPU restatement itself sits inside the same bounds
    assert (np.abs(np.stack([R["F_r"], R["F_w"]]) - Fx) <= n * 2.0 ** -52 * A).all()
    assert (np.abs(np.stack([R["J_r"], R["J_w"]]) - Jx) <= n * 2.0 ** -52 * AJ).all()


def test_newton_driver_on_the_gpu_equals_the_cpu_backend_driver(gpu, pkg):
    """N = 3, Na = 60, T = 12: the Jacobians differ in their last bits, the fixed point does not —
    the same rounds and statuses, K within 1e-10."""
    ss = _ss60(pkg)
    T = 12
    q = np.arange(T)
    Z = np.stack([1 - 0.01 * 0.8 ** q, np.ones(T), 1 + 0.005 * 0.5 ** q])
    A = pkg.aiyagari_transition_newton(ss, Z, T, tol=1e-8)
    B = pkg.aiyagari_transition_newton(ss, Z, T, jac=sr.jacobian_cpu(ss, T, 1e-4), tol=1e-8,
                                       backend=tr.transition_batch)
    print("rounds", A["rounds"], B["rounds"], "max |K_gpu - K_cpu|", np.max(np.abs(A["K"] - B["K"])))
    assert (B["status"] == 0).all() and B["rounds"][1] == 1 and (B["rounds"] <= 6).all()
    assert np.array_equal(A["rounds"], B["rounds"]) and np.array_equal(A["status"], B["status"])
    assert np.max(np.abs(A["K"] - B["K"])) <= 1e-10
    D = pkg.aiyagari_transition(ss, Z, T, damp=0.5, tol=1e-8, max_iter=200)
    assert (D["rounds"][[0, 2]] > A["rounds"][[0, 2]]).all()
    assert np.max(np.abs(A["K"] - D["K"])) <= 1e-7
