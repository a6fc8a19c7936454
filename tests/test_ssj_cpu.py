"""No GPU: the sequence-space Jacobian's CPU reference (tests/ssj_ref.py) against brute-force
differences of whole reference transitions, the expectation vectors' adjoint identity, the Newton
driver and the linear impulse response on the reference backend, and which refusal each new host
entry answers before it asks for a device (in the manner of test_transition_cpu.py)."""
import ctypes as C

import numpy as np
import pytest

from tests import ssj_ref as sr
from tests import transition_ref as tr


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.int64)


def same(x, y):
    return np.array_equal(bits(x), bits(y))


T40 = 40


@pytest.fixture(scope="module")
def ss60(pkg):
    """N = 3, Na = 60: the stationary point at r = 0.03 (test_transition_cpu.py's)."""
    cb = pkg.calibration
    cal = cb.aiyagari(Na=60, shocks="rouwenhorst", N=3)
    return tr.steady_state_cpu(cal, 0.03, lambda r: cb.wage(r, cal["alpha"], cal["delta"]))


@pytest.fixture(scope="module")
def jac40(ss60):
    """jacobian_cpu at T = 40, h = 1e-4 — the Jacobian the driver tests share."""
    return sr.jacobian_cpu(ss60, T40, 1e-4)


# ------------------------------------------------------------- restatement vs brute force
def test_fake_news_jacobian_is_the_brute_force_jacobian(ss60, jac40):
    """Fake news against one-sided differences of 1 + T whole transitions, the same h in both.
    Measured (relative to max|J|): 1.48e-5 (r) and 9.6e-7 (w) at h = 1e-4, a tenth of that at
    h = 1e-5 — the O(h) nonlinearity of the one-sided difference and nothing else."""
    jac5 = sr.jacobian_cpu(ss60, T40, 1e-5)
    for x in ("r", "w"):
        err = {}
        for h, jac in ((1e-4, jac40), (1e-5, jac5)):
            B = sr.brute_force_cpu(ss60, T40, h, x)
            err[h] = np.max(np.abs(jac["J_" + x] - B)) / np.max(np.abs(B))
        print(f"d K / d {x}: fake news vs brute force {err[1e-4]:.3e} (h = 1e-4), "
              f"{err[1e-5]:.3e} (h = 1e-5)")
        assert err[1e-4] <= 1e-4, (x, err)
        assert err[1e-5] <= 0.2 * err[1e-4], (x, err)


def test_jacobian_steps_4_and_5_restated(ss60, jac40):
    """The numpy restatement's orientation: F[t][s] pairs E[t] with the news of period T-1-s, and J
    sums F down the diagonals, t ascending."""
    E, L, h = jac40["E"], jac40["lam1"], 1e-4
    for (x, t, s) in ((0, 0, 0), (1, 3, 7), (0, T40 - 1, T40 - 1), (1, 11, 2)):
        D = (L[x + 1, T40 - 1 - s] - L[0, T40 - 1 - s]) / h
        F = jac40["F_r" if x == 0 else "F_w"]
        J = jac40["J_r" if x == 0 else "J_w"]
        assert abs(F[t, s] - np.sum(E[t] * D)) <= 1e-12 * np.sum(np.abs(E[t] * D))
        acc = F[t - min(t, s), s - min(t, s)]
        for q in range(min(t, s) - 1, -1, -1):
            acc = F[t - q, s - q] + acc
        assert same(J[t, s], acc)


# ------------------------------------------------------------- expectation vectors
@pytest.mark.parametrize("y_is_grid", [True, False])
def test_expectation_vectors_are_the_adjoint_of_the_push(ss60, jac40, y_is_grid):
    """E_t·λ₀ = y·λ_t under the constant policy g, within 1e-12 relative (every term is
    non-negative), λ_t from the reference forward pass."""
    cal = ss60["cal"]
    a, P, N, Na = cal["a_grid"], cal["P"], cal["N"], cal["Na"]
    g = jac40["pk"][0, 0]
    lam0 = np.random.default_rng(5).random((N, Na))
    lam0 /= lam0.sum()
    y = np.tile(a, (N, 1)) if y_is_grid else np.random.default_rng(6).random((N, Na))
    assert (y >= 0).all()
    E, lo, wl = sr.expect(g, y, a, P, T40, plan=True)
    assert same(E[0], y) and same(lo, tr.lottery_keys(g, a)) and ((0 <= wl) & (wl <= 1)).all()
    if y_is_grid:
        assert same(E, jac40["E"])
    lam = tr.dist_forward(np.tile(g, (T40 - 1, 1, 1)), lam0, a, P)["lam"]
    for t in range(T40):
        lhs, rhs = float(np.sum(E[t] * lam0)), float(np.sum(y * lam[t]))
        assert abs(lhs - rhs) <= 1e-12 * abs(rhs), t


# ------------------------------------------------------------- the Newton driver
def _shocks(T):
    q = np.arange(T)
    return np.stack([1 - 0.01 * 0.8 ** q, 1 + 0.005 * 0.5 ** q])


def test_newton_driver_beats_the_damped_driver(pkg, ss60, jac40):
    """The two shocks at T = 40 to tol = 1e-8: at most 6 Newton rounds (measured 4 and 3) where
    the damped driver needs more than 15 (measured 25 and 23), the same K paths within 1e-7."""
    Z = _shocks(T40)
    A = pkg.aiyagari_transition_newton(ss60, Z, T40, jac=jac40, tol=1e-8,
                                       backend=tr.transition_batch)
    B = pkg.aiyagari_transition(ss60, Z, T40, damp=0.5, tol=1e-8, max_iter=200,
                                backend=tr.transition_batch)
    print("rounds: newton", A["rounds"], "damped", B["rounds"], "max |K_newton - K_damped|",
          np.max(np.abs(A["K"] - B["K"])))
    assert (A["status"] == 0).all() and (B["status"] == 0).all()
    assert (A["resid"] < 1e-8).all() and (B["resid"] < 1e-8).all()
    assert (A["rounds"] <= 6).all() and (B["rounds"] > 15).all()
    assert np.max(np.abs(A["K"] - B["K"])) <= 1e-7
    assert (A["K"][:, 0] == ss60["K"]).all() and set(A) == set(B)


def test_newton_driver_paths_do_not_depend_on_the_batch(pkg, ss60, jac40):
    """Z ≡ 1 stops in round 1; every path of a batch equals its solo run bit for bit."""
    Z = np.stack([_shocks(T40)[0], np.ones(T40), _shocks(T40)[1]])
    run = lambda z: pkg.aiyagari_transition_newton(ss60, z, T40, jac=jac40, tol=1e-8,
                                                   backend=tr.transition_batch)
    A = run(Z)
    assert (A["status"] == 0).all() and A["rounds"][1] == 1 and A["rounds"][0] > 1
    assert (A["K"][1] == ss60["K"]).all()
    for c in range(3):
        S = run(Z[c:c + 1])
        assert S["rounds"][0] == A["rounds"][c] and S["status"][0] == A["status"][c]
        for k in ("K", "r", "w"):
            assert same(S[k][0], A[k][c]), (c, k)


def test_impulse_response_is_the_newton_path_to_first_order(pkg, ss60):
    """K − K_ss of the nonlinear path against the linear response: the difference is second order
    in the shock — it falls by at least 50 when the shock falls by 10.  (The Jacobian at
    h = 1e-6: its own O(h) error is first order in the shock and must stay below the second-order
    term of the smaller shock.)"""
    jac = sr.jacobian_cpu(ss60, T40, 1e-6)
    diff = {}
    for eps in (1e-3, 1e-4):
        dZ = -eps * 0.8 ** np.arange(T40)[None, :]
        R = pkg.aiyagari_transition_newton(ss60, 1 + dZ, T40, jac=jac, tol=1e-11, max_iter=20,
                                           backend=tr.transition_batch)
        assert R["status"][0] == 0 and R["resid"][0] < 1e-11
        dK = pkg.impulse_response(ss60, jac, dZ)
        assert dK.shape == (1, T40 + 1) and dK[0, 0] == 0
        diff[eps] = np.max(np.abs((R["K"][0] - ss60["K"]) - dK[0]))
        assert diff[eps] < 0.05 * np.max(np.abs(dK))
    print("impulse response vs Newton path:", diff)
    assert diff[1e-3] >= 50 * diff[1e-4]


# ------------------------------------------------------------------------------ refusals
N_, NA_, NC_, T_ = 2, 5, 3, 4
i64, d, ci = C.c_int64, C.c_double, C.c_int
NO_DEVICE = (5, "no HIP device visible")
EXP_FIT = ("expectation pass: a steady state's arrays exceed one CU's LDS "
           "(N <= 16, 28·N·Na + 2 KB within 160 KiB)")
JAC_FIT = ("Jacobian: the transition passes' arrays exceed one CU's LDS "
           "(aiy_transition_batch's fit rules)")


def _base():
    n = N_ * NA_
    return dict(C=NC_, T=T_, N=N_, Na=NA_, n_in=2, h=1e-4, r=0.02, w=1.2,
                pk=np.ones(NC_ * n), y0=np.ones(NC_ * n), a=np.arange(NA_, dtype=np.float64),
                s=np.array([0.8, 1.2]), P=np.full(N_ * N_, 0.5), E=np.zeros(NC_ * T_ * n),
                lam1=np.zeros(3 * T_ * n), F=np.zeros(2 * T_ * T_), J=np.zeros(2 * T_ * T_),
                pc=np.ones(n), lam=np.full(n, 1.0 / n), st=np.zeros(2, np.int32))


DEFECTS = {
    "valid": lambda a: None, "C0": lambda a: a.update(C=0), "T0": lambda a: a.update(T=0),
    "N0": lambda a: a.update(N=0), "Na1": lambda a: a.update(Na=1), "N17": lambda a: a.update(N=17),
    "Na500": lambda a: a.update(Na=500, N=16), "Na1025": lambda a: a.update(Na=1025),
    "n0": lambda a: a.update(N=0, Na=0), "nin0": lambda a: a.update(n_in=0),
    "T32769": lambda a: a.update(T=32769),
    "h0": lambda a: a.update(h=0.0), "h_neg": lambda a: a.update(h=-1e-4),
    "h_nan": lambda a: a.update(h=np.nan), "h_inf": lambda a: a.update(h=np.inf),
    "r_m1": lambda a: a.update(r=-1.0), "w_nan": lambda a: a.update(w=np.nan),
    "a_nan": lambda a: a["a"].__setitem__(0, np.nan), "a_dec": lambda a: a["a"].__setitem__(2, 0.5),
    "a_rep": lambda a: a["a"].__setitem__(4, 3.0),
    "null:pk": lambda a: a.update(pk=None), "null:y0": lambda a: a.update(y0=None),
    "null:E": lambda a: a.update(E=None), "null:a": lambda a: a.update(a=None),
    "null:lam1": lambda a: a.update(lam1=None), "null:J": lambda a: a.update(J=None),
    "null:F": lambda a: a.update(F=None), "null:pc": lambda a: a.update(pc=None),
    "null:st": lambda a: a.update(st=None),
}


def _p(x):
    return None if x is None else x.ctypes.data_as(C.c_void_p)


def _expect(L, a):
    return L.aiy_dist_expect_batch(i64(a["C"]), i64(a["T"]), _p(a["pk"]), _p(a["y0"]), ci(0),
                                   _p(a["a"]), _p(a["P"]), i64(a["N"]), i64(a["Na"]), _p(a["E"]))


def _news(L, a):
    return L.aiy_ssj_fake_news(i64(a["T"]), i64(a["n_in"]), i64(a["N"] * a["Na"]), _p(a["E"]),
                               _p(a["lam1"]), d(a["h"]), _p(a["F"]), _p(a["J"]))


def _jacobian(L, a):
    J, F, st = a["J"], a["F"], a["st"]
    tt = a["T"] * a["T"]
    half = lambda x: None if x is None else x[tt:]
    return L.aiy_ssj_jacobian(_p(a["pc"]), _p(a["lam"]), d(a["r"]), d(a["w"]), _p(a["a"]),
                              _p(a["s"]), _p(a["P"]), i64(a["N"]), i64(a["Na"]), d(0.96), d(5.0),
                              d(0.0), i64(a["T"]), d(a["h"]), _p(J), _p(half(J)), _p(F),
                              _p(half(F)), _p(a["E"]), _p(st), _p(None if st is None else st[1:]),
                              None)


CALLERS = {"aiy_dist_expect_batch": _expect, "aiy_ssj_fake_news": _news,
           "aiy_ssj_jacobian": _jacobian}
A_DEC = (6, "a_grid must be non-decreasing (a_grid(3) < a_grid(2))")
A_REP = (6, "grid must be strictly increasing (point 5 repeats point 4)")
H_BAD = (6, "h must be positive and finite")
# (entry, defects) -> the answer; a defect pair shows which check comes first
EXPECTED = {
    ("aiy_dist_expect_batch", "null:pk"): (6, "NULL argument"),
    ("aiy_dist_expect_batch", "null:y0+T0"): (6, "NULL argument"),
    ("aiy_dist_expect_batch", "null:E"): (6, "NULL argument"),
    ("aiy_dist_expect_batch", "C0"): (1, "need 1 <= C < 2^31"),
    ("aiy_dist_expect_batch", "T0"): (1, "T must be in [1, 2^31 - 1)"),
    ("aiy_dist_expect_batch", "T0+N17"): (1, "T must be in [1, 2^31 - 1)"),
    ("aiy_dist_expect_batch", "N0"): (1, "need N >= 1 and Na >= 2"),
    ("aiy_dist_expect_batch", "Na1"): (1, "need N >= 1 and Na >= 2"),
    ("aiy_dist_expect_batch", "N17"): (6, EXP_FIT),
    ("aiy_dist_expect_batch", "Na500"): (6, EXP_FIT),
    ("aiy_dist_expect_batch", "N17+a_nan"): (6, EXP_FIT),
    ("aiy_dist_expect_batch", "null:a"): (6, "a_grid is NULL"),
    ("aiy_dist_expect_batch", "a_nan"): (2, "a_grid(1) is not finite"),
    ("aiy_dist_expect_batch", "a_dec"): A_DEC,
    ("aiy_dist_expect_batch", "a_rep"): A_REP,
    ("aiy_dist_expect_batch", "valid"): NO_DEVICE,
    ("aiy_ssj_fake_news", "null:lam1"): (6, "NULL argument"),
    ("aiy_ssj_fake_news", "null:J+T0"): (6, "NULL argument"),
    ("aiy_ssj_fake_news", "null:F"): (6, "NULL argument"),
    ("aiy_ssj_fake_news", "T0"): (1, "T must be in [1, 32768]"),
    ("aiy_ssj_fake_news", "T32769"): (1, "T must be in [1, 32768]"),
    ("aiy_ssj_fake_news", "T0+h0"): (1, "T must be in [1, 32768]"),
    ("aiy_ssj_fake_news", "nin0"): (1, "need 1 <= n_in <= 65535"),
    ("aiy_ssj_fake_news", "n0"): (1, "need 1 <= n <= 2^28"),
    ("aiy_ssj_fake_news", "h0"): H_BAD,
    ("aiy_ssj_fake_news", "h_neg"): H_BAD,
    ("aiy_ssj_fake_news", "h_nan"): H_BAD,
    ("aiy_ssj_fake_news", "h_inf"): H_BAD,
    ("aiy_ssj_fake_news", "valid"): NO_DEVICE,
    ("aiy_ssj_jacobian", "null:pc"): (6, "NULL argument"),
    ("aiy_ssj_jacobian", "null:J+T0"): (6, "NULL argument"),
    ("aiy_ssj_jacobian", "null:st"): (6, "NULL argument"),
    ("aiy_ssj_jacobian", "N0"): (1, "need N >= 1 and Na >= 2"),
    ("aiy_ssj_jacobian", "N17"): (6, JAC_FIT),
    ("aiy_ssj_jacobian", "Na500"): (6, JAC_FIT),
    ("aiy_ssj_jacobian", "Na1025"): (6, JAC_FIT),
    ("aiy_ssj_jacobian", "N17+T0"): (6, JAC_FIT),
    ("aiy_ssj_jacobian", "T0"): (1, "T must be in [1, 32768]"),
    ("aiy_ssj_jacobian", "T0+h_nan"): (1, "T must be in [1, 32768]"),
    ("aiy_ssj_jacobian", "h0"): H_BAD,
    ("aiy_ssj_jacobian", "h_neg"): H_BAD,
    ("aiy_ssj_jacobian", "h_nan"): H_BAD,
    ("aiy_ssj_jacobian", "h_nan+a_dec"): H_BAD,
    ("aiy_ssj_jacobian", "null:a"): (6, "a_grid is NULL"),
    ("aiy_ssj_jacobian", "a_dec"): A_DEC,
    ("aiy_ssj_jacobian", "a_rep"): A_REP,
    ("aiy_ssj_jacobian", "a_rep+r_m1"): A_REP,
    ("aiy_ssj_jacobian", "r_m1"): (6, "r_ss must be finite with 1 + r_ss > 0"),
    ("aiy_ssj_jacobian", "w_nan"): (6, "w_ss must be finite"),
    ("aiy_ssj_jacobian", "null:F"): NO_DEVICE,
    ("aiy_ssj_jacobian", "null:E"): NO_DEVICE,
    ("aiy_ssj_jacobian", "valid"): NO_DEVICE,
}


def test_the_fit_rule_the_refusals_quote(pkg):
    """E, G and wl (doubles), lo (ints) for N·Na states and P: N = 16, Na = 500 is past 160 KiB,
    N = 2, Na = 1025 and the scripts' N = 7, Na = 400 (80 KB) are inside."""
    fits = lambda N, Na: N <= 16 and 24 * N * Na + 4 * ((N * Na + 1) // 2 * 2) + 2048 <= 160 * 1024
    assert not fits(16, 500) and not fits(17, 5) and fits(2, 1025) and fits(7, 400)
    assert fits(16, 361) and not fits(16, 362)


@pytest.mark.parametrize("entry,defects", sorted(EXPECTED))
def test_ssj_refusal(pkg, entry, defects):
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
