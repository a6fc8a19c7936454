"""GPU parity for the estimation kernels (lik_kernels.hip).

MA coefficients: bit for bit against numpy on data whose every product and partial sum is exact,
within the any-order summation bound T·2⁻⁵²·Σ|G·dZ| of math.fsum on random data, independent of
the batch and of the run.  Autocovariances and log-likelihood: bit for bit against
tests/support/estimation_ref.c, a candidate of a batch against its solo call, a singular and a NaN
candidate among good ones.  ar1_loglik and ar1_mle on the GPU against the reference backend."""
import math

import numpy as np
import pytest

from tests import estimation_ref as er
from tests import ssj_ref as sr
from tests import transition_ref as tr

pytestmark = pytest.mark.gpu


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.int64)


def same(x, y):
    return np.array_equal(bits(x), bits(y))


def same_nan(x, y):
    """Equal bits where neither is NaN, NaN in the same places."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    nx = np.isnan(x)
    return x.shape == y.shape and np.array_equal(nx, np.isnan(y)) and same(x[~nx], y[~nx])


# ------------------------------------------------------------- kernel A
def _exact_data(n_o, T, n_c, seed):
    """G integers in [-8, 8], dZ integer multiples of 2^-10 within 1: every product and partial
    sum is an exact double."""
    rng = np.random.default_rng(seed)
    G = rng.integers(-8, 9, (n_o, T, T)).astype(np.float64)
    dZ = rng.integers(-1024, 1025, (n_c, T)).astype(np.float64) * 2.0 ** -10
    return G, dZ


@pytest.mark.parametrize("n_o", [1, 3])
@pytest.mark.parametrize("n_c", [1, 3, 33])
@pytest.mark.parametrize("T", [1, 5, 17, 33, 70])
def test_ma_on_exact_data_is_numpy_bit_for_bit(gpu, pkg, T, n_c, n_o):
    G, dZ = _exact_data(n_o, T, n_c, 1000 * T + 10 * n_c + n_o)
    m = pkg.ma_batch(G, dZ)
    assert m.shape == (n_c, n_o, T) and same(m, er.ma_batch(G, dZ))
    # one non-zero row of G and one of dZ: the (c, o, t) orientation
    o1, t1, c1 = n_o - 1, T // 3, n_c - 1
    G0, Z0 = np.zeros_like(G), np.zeros_like(dZ)
    G0[o1, t1] = np.where(G[o1, t1] == 0, 1.0, G[o1, t1])
    Z0[c1] = np.where(dZ[c1] == 0, 0.5, dZ[c1])
    v = float(np.sum(G0[o1, t1] * Z0[c1]))
    if v == 0:  # (a row whose products cancel: make them all positive)
        G0[o1, t1], Z0[c1] = np.abs(G0[o1, t1]), np.abs(Z0[c1])
        v = float(np.sum(G0[o1, t1] * Z0[c1]))
    want = np.zeros((n_c, n_o, T))
    want[c1, o1, t1] = v
    assert same(pkg.ma_batch(G0, Z0), want)


@pytest.mark.parametrize("T", [1, 5, 17, 33, 70])
def test_ma_on_random_data_is_within_the_summation_bound(gpu, pkg, T):
    """|m − m_exact| <= T·2⁻⁵²·Σ_s|G[o][t][s]·dZ[c][s]| — the bound of any summation order of T
    terms, fused or not; row c of the C = 33 call is the C = 1 call, an observable of the n_o = 3
    call is the n_o = 1 call, and two runs are bit-identical."""
    n_o, n_c = 3, 33
    rng = np.random.default_rng(T)
    G = rng.standard_normal((n_o, T, T)) * 10
    dZ = rng.standard_normal((n_c, T)) * 0.01
    m = pkg.ma_batch(G, dZ)
    for c in range(n_c):
        for o in range(n_o):
            for t in range(T):
                p = G[o, t] * dZ[c]
                assert abs(m[c, o, t] - math.fsum(p)) <= T * 2.0 ** -52 * float(np.sum(np.abs(p)))
    assert same(pkg.ma_batch(G, dZ), m)
    for c in (0, 7, 32):
        assert same(pkg.ma_batch(G, dZ[c:c + 1])[0], m[c]), c
    assert same(pkg.ma_batch(G[1], dZ)[:, 0], m[:, 1])


def test_ma_dev_enqueues_on_torch_tensors(gpu, pkg):
    import torch
    G, dZ = _exact_data(2, 33, 5, 9)
    f = dict(dtype=torch.float64, device=gpu)
    m = torch.empty((5, 2, 33), **f)
    pkg.ma_batch_dev(torch.as_tensor(G, **f), torch.as_tensor(dZ, **f), m)
    torch.cuda.synchronize()
    assert same(m.cpu().numpy(), er.ma_batch(G, dZ))


# ------------------------------------------------------------- kernel B
def _fits(n_o, L, T):
    n = n_o * L
    return 8 * (max(n * (n + 1) // 2, n_o * T) + n * n_o + 3 * n + 2) <= 160 * 1024


def _largest_L(n_o, T):
    L = 1
    while _fits(n_o, L + 1, T):
        L += 1
    return L


LIK_SHAPES = [(1, 1, 1), (1, 2, 5), (1, 9, 4), (3, 7, 17), (2, 33, 40),
              (1, _largest_L(1, 300), 300), (3, _largest_L(3, 300), 300)]


def _lik_problem(n_o, L, T, n_c, shared, seed):
    rng = np.random.default_rng(seed)
    m = rng.standard_normal((n_c, n_o, T))
    y = rng.standard_normal((L, n_o)) * math.sqrt(T)
    me = 0.05 * T * (1 + rng.random(n_o if shared else (n_c, n_o)))
    return m, y, me


def _check(G, R, keys=("loglik", "Gamma", "d")):
    assert np.array_equal(G["status"], R["status"]) and np.array_equal(G["fail"], R["fail"])
    for k in keys:
        assert same_nan(G[k], R[k]), k


@pytest.mark.parametrize("shared", [True, False])
@pytest.mark.parametrize("n_c", [1, 5])
@pytest.mark.parametrize("n_o,L,T", LIK_SHAPES)
def test_loglik_is_the_reference_bit_for_bit(gpu, pkg, n_o, L, T, n_c, shared):
    assert (_largest_L(1, 300), _largest_L(3, 300)) == (197, 65)
    m, y, me = _lik_problem(n_o, L, T, n_c, shared, 100 * L + n_c)
    G = pkg.loglik_batch(m, y, me, want_gamma=True, want_d=True)
    R = er.loglik_batch(m, y, me, want_gamma=True, want_d=True)
    assert (R["status"] == 0).all() and np.isfinite(R["loglik"]).all()
    if L > T:
        assert (R["Gamma"][:, T:] == 0).all()
    _check(G, R)
    plain = pkg.loglik_batch(m, y, me)
    assert set(plain) == {"loglik", "status", "fail"} and same(plain["loglik"], G["loglik"])
    for c in range(n_c if n_c > 1 else 0):  # candidate c of the batch is its solo call
        S = pkg.loglik_batch(m[c], y, me if shared else me[c], want_gamma=True, want_d=True)
        for k in ("loglik", "Gamma", "d", "status", "fail"):
            assert same_nan(np.asarray(S[k][0], np.float64), np.asarray(G[k][c], np.float64)), (c, k)
    # y = None: Γ alone, the Γ of the full call
    assert same(pkg.autocovariance_batch(m, L), G["Gamma"])


def test_a_singular_and_a_nan_candidate_among_good_ones(gpu, pkg):
    """n_o = 2, L = 6, T = 9.  Candidate 1: two equal rows of m, me_var = 0 — L₁₀ = g/g = 1 and
    the second pivot g − 1·g is exactly 0: status 1, fail 1.  Candidate 3: one NaN in the second
    row of m — Γ[0][0][0] is clean, so status 1 at pivot 1, the first the NaN reaches.  The
    others' bits are those of a call without them."""
    n_o, L, T = 2, 6, 9
    m, y, me = _lik_problem(n_o, L, T, 5, False, 77)
    good = pkg.loglik_batch(m, y, me, want_gamma=True, want_d=True)
    assert (good["status"] == 0).all()
    m, me = m.copy(), me.copy()
    m[1, 1] = m[1, 0]
    me[1] = 0.0
    m[3, 1, 4] = np.nan
    G = pkg.loglik_batch(m, y, me, want_gamma=True, want_d=True)
    R = er.loglik_batch(m, y, me, want_gamma=True, want_d=True)
    assert list(R["status"]) == [0, 1, 0, 1, 0] and list(R["fail"]) == [-1, 1, -1, 1, -1]
    assert R["d"][1, 0] > 0 and R["d"][1, 1] == 0 and np.isnan(R["d"][1, 2:]).all()
    assert R["d"][3, 0] > 0 and np.isnan(R["d"][3, 1:]).all()
    _check(G, R)
    assert np.isnan(G["loglik"][[1, 3]]).all()
    for c in (0, 2, 4):
        for k in ("loglik", "Gamma", "d"):
            assert same(G[k][c], good[k][c]), (c, k)


def test_loglik_dev_enqueues_on_torch_tensors(gpu, pkg):
    import torch
    n_o, L, T, n_c = 3, 7, 17, 4
    m, y, me = _lik_problem(n_o, L, T, n_c, True, 5)
    f = dict(dtype=torch.float64, device=gpu)
    i32 = dict(dtype=torch.int32, device=gpu)
    ll, st, fl = torch.empty(n_c, **f), torch.empty(n_c, **i32), torch.empty(n_c, **i32)
    Gam = torch.empty((n_c, L, n_o, n_o), **f)
    pkg.loglik_batch_dev(torch.as_tensor(m, **f), torch.as_tensor(y, **f), torch.as_tensor(me, **f),
                         ll, st, fl, Gamma=Gam)
    Gam2 = torch.empty_like(Gam)
    pkg.loglik_batch_dev(torch.as_tensor(m, **f), None, None, None, None, None, Gamma=Gam2)
    torch.cuda.synchronize()
    R = er.loglik_batch(m, y, me, want_gamma=True)
    assert same(ll.cpu().numpy(), R["loglik"]) and same(Gam.cpu().numpy(), R["Gamma"])
    assert same(Gam2.cpu().numpy(), R["Gamma"])
    assert (st.cpu().numpy() == 0).all() and (fl.cpu().numpy() == -1).all()


# ------------------------------------------------------------- end to end
C_GAP = 0.0131  # test_estimation_cpu.py's constant of the reference's own backward error
T40 = 40


@pytest.fixture(scope="module")
def economy(pkg):
    """G of (Y, C) at N = 3, Na = 60, T = 40 from the CPU Jacobian (host code throughout), and 24
    periods simulated from the MA of ρ = 0.8, σ = 0.01 with a fixed seed."""
    cb = pkg.calibration
    cal = cb.aiyagari(Na=60, shocks="rouwenhorst", N=3)
    ss = tr.steady_state_cpu(cal, 0.03, lambda r: cb.wage(r, cal["alpha"], cal["delta"]))
    G = pkg.ge_jacobians(ss, sr.jacobian_cpu(ss, T40, 1e-4), ("Y", "C"))
    m = er.ma_batch(G, pkg.ar1_ma([0.8], [0.01], T40))[0]
    me = 1e-2 * np.einsum("ot,ot->o", m, m)
    return G, er.simulate(m, 24, me, 11), me


def test_ar1_loglik_on_the_gpu_agrees_with_the_reference_backend(gpu, pkg, economy):
    """The two backends differ in m alone — each within kernel A's any-order bound of the exact
    product, so |δm[o][t]| <= 2·T·2⁻⁵²·Σ_s|G[o][t][s]·dZ[s]| — and run the same factorisation on
    it.  To first order in δm, with n = L·n_o, ‖δV‖₂ <= n·max|δΓ| <= n·2·‖δm‖_F·‖m‖_F,
        |δ logdet| <= n·‖V⁻¹‖₂·‖δV‖₂,   |δ quad| <= ‖y‖²·‖V⁻¹‖₂²·‖δV‖₂,
    and each factorisation carries its own rounding, which the numpy check bounds by
    c·n·2⁻⁵²·cond₂(V) relative on logdet and on quad.  The tolerance on loglik is the sum:
        (n·‖V⁻¹‖·‖δV‖ + ‖y‖²·‖V⁻¹‖²·‖δV‖) + c·n·2⁻⁵²·cond₂(V)·(|logdet| + quad)."""
    G, y, me = economy
    rho = np.array([0.5, 0.8, 0.95, 0.8, 0.3])
    sig = np.array([0.01, 0.01, 0.004, 0.02, 0.03])
    A = pkg.ar1_loglik(G, y, rho, sig, me)
    B = pkg.ar1_loglik(G, y, rho, sig, me, backend=er.BACKEND)
    assert (A["status"] == 0).all() and (B["status"] == 0).all()
    n, u = y.size, 2.0 ** -52
    dZ = pkg.ar1_ma(rho, sig, T40)
    m = er.ma_batch(G, dZ)
    for c in range(rho.size):
        dm = 2 * T40 * u * np.abs(G) @ np.abs(dZ[c])
        dV = n * 2 * np.linalg.norm(dm) * np.linalg.norm(m[c])
        Gam = er.autocovariance_batch(m[c], y.shape[0])[0]
        V = er.dense_V(Gam, me)
        inv = np.linalg.norm(np.linalg.inv(V), 2)
        _, logdet, quad, cond = er.dense_loglik(Gam, y, me)
        tol = (n * inv * dV + float(y.ravel() @ y.ravel()) * inv ** 2 * dV
               + C_GAP * n * u * cond * (abs(logdet) + quad))
        gap = abs(A["loglik"][c] - B["loglik"][c])
        print(f"candidate {c}: loglik {A['loglik'][c]!r} vs {B['loglik'][c]!r}, gap {gap:.3e}, "
              f"tolerance {tol:.3e}")
        assert gap <= tol, c


def test_ar1_mle_picks_the_same_cells_on_both_backends(gpu, pkg, economy):
    G, y, me = economy
    kw = dict(width=8, rounds=4)
    A = pkg.ar1_mle(G, y, me, (0.3, 0.99), (0.002, 0.05), **kw)
    B = pkg.ar1_mle(G, y, me, (0.3, 0.99), (0.002, 0.05), backend=er.BACKEND, **kw)
    assert np.array_equal(A["best"], B["best"]) and (A["best"] >= 0).all()
    assert A["boxes"] == B["boxes"] and list(A["evals"]) == [64] * 4
    assert (A["rho"], A["sigma"]) == (B["rho"], B["sigma"])
    print("ar1_mle:", A["rho"], A["sigma"], A["loglik"], "reference backend", B["loglik"])
