"""No GPU: the labour economy's transition reference against the C oracle, the pricing rule in
κ = K/H, both lockstep drivers on the reference backend (and why the Newton one exists), the
fake-news composition of the hours Jacobian against brute force, and which refusal each new host
entry answers before it asks for a device (in the manner of test_transition_cpu.py)."""
import ctypes as C

import numpy as np
import pytest

from oracle import corc
from tests import labor_transition_ref as lr


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.int64)


def same(x, y):
    return np.array_equal(bits(x), bits(y))


def _cal(pkg, N, Na):
    """The labour script's calibration (rho = .6, sigma_e = .2); Rouwenhorst for N != 7."""
    cb = pkg.calibration
    if N == 7:
        return cb.aiyagari(Na=Na, rho=0.6, sigma_e=0.2)
    return cb.aiyagari(Na=Na, rho=0.6, sigma_e=0.2, shocks="rouwenhorst", N=N)


def _wage(pkg, cal):
    return lambda r: pkg.calibration.wage(r, cal["alpha"], cal["delta"])


# ------------------------------------------------- the reference is the oracle's step, r split
@pytest.mark.parametrize("N,Na,sigma,phi,theta", [(3, 37, 5.0, 1.0, 1.0), (7, 400, 5.0, 1.0, 1.0),
                                                  (3, 37, 1.5, 0.8, 2.0), (7, 100, 2.0, 1.3, 0.5)])
def test_constant_path_is_the_chained_oracle_labor_step(pkg, N, Na, sigma, phi, theta):
    """r_next == r_now == r: T steps of the two-rate reference equal T chained corc.labor_egm_step
    calls bit for bit — pk, pl and pc at every period, integer and fractional sigma, theta = 1
    (no power) and theta != 1."""
    T, r = 4, 0.025
    cal = _cal(pkg, N, Na)
    a, s, P = cal["a_grid"], cal["s"], cal["P"]
    w = _wage(pkg, cal)(r)
    pcT = np.tile((1 + r) * a + w * np.mean(s), (N, 1))
    B = lr.labor_backward(np.full(T + 1, r), np.full(T, w), pcT, a, s, P, cal["beta"], sigma, phi,
                          theta, cal["amin"])
    assert B["status"] == 0 and B["fail_t"] == -1
    cur = pcT
    for t in range(T - 1, -1, -1):
        cur, pk, pl, _ = corc.labor_egm_step(cur, a, s, P, r, w, cal["beta"], sigma, phi, theta,
                                             cal["amin"])
        assert same(cur, B["pc"][t]) and same(pk, B["pk"][t]) and same(pl, B["pl"][t]), t


def test_hours_sum_is_the_capital_sum_order(pkg):
    """hours_sum with pl ≡ 1 and s ≡ 1 weights nothing: it is the device-order sum of λ; and with
    s_j·pl = a it is tests/transition_ref.py's capital_sum bit for bit."""
    from tests import transition_ref as tr
    rng = np.random.default_rng(5)
    for N, Na in ((1, 2), (3, 37), (7, 400)):
        lam = rng.random((N, Na))
        a = np.sort(rng.random(Na))
        assert lr.hours_sum(lam, np.tile(a, (N, 1)), np.ones(N)) == tr.capital_sum(lam, a)


# ------------------------------------------------------------------------------ pricing
def test_prices_from_ratio_at_the_stationary_point_are_exact(pkg):
    cal = _cal(pkg, 7, 20)
    for r_ss, w_ss, K_ss, H_ss in [(0.0371234567, 1.1876543, 5.4321, 0.7531),
                                   (-0.0123, 0.9, 11.0 / 3, 1.0 / 7)]:
        ss = dict(r=r_ss, w=w_ss, K=K_ss, H=H_ss, cal=cal)
        r, w = pkg.prices_from_ratio(np.full((3, 9), K_ss / H_ss), np.ones((3, 9)), ss)
        assert (r == r_ss).all() and (w == w_ss).all()
    # and away from it the anchored Cobb-Douglas rule in capital per effective hour
    k_ss = K_ss / H_ss
    kap, Z = np.array([[0.9 * k_ss, 1.2 * k_ss]]), np.array([[0.99, 1.02]])
    r, w = pkg.prices_from_ratio(kap, Z, ss)
    al, de = cal["alpha"], cal["delta"]
    assert np.allclose(r + de, (r_ss + de) * Z * (kap / k_ss) ** (al - 1), rtol=1e-13, atol=0)
    assert np.allclose(w, w_ss * Z * (kap / k_ss) ** al, rtol=1e-13, atol=0)


# ------------------------------------------------------------------------------ the drivers
T60 = 60


@pytest.fixture(scope="module")
def ss100(pkg):
    """N = 7, Na = 100 on the labour script's calibration, phi = theta = 1."""
    cal = _cal(pkg, 7, 100)
    return lr.steady_state_labor_cpu(cal, 1.0, 1.0, _wage(pkg, cal))


@pytest.fixture(scope="module")
def jac100(ss100):
    return lr.jacobian_labor_cpu(ss100, T60, 1e-4)


def test_reference_steady_state_clears_the_market(pkg, ss100):
    cal = ss100["cal"]
    kd = (cal["alpha"] / (ss100["r"] + cal["delta"])) ** (1 / (1 - cal["alpha"]))
    assert abs(ss100["K"] - ss100["H"] * kd) <= 1e-9
    assert 0 < ss100["r"] < 1 / cal["beta"] - 1 and 0 < ss100["H"] < cal["labor"] * 2
    assert abs(ss100["lam"].sum() - 1) < 1e-10


def test_damped_half_diverges_where_newton_converges(pkg, ss100, jac100):
    """The 1 % AR(0.9) TFP path at T = 60.  M = ∂κ_s/∂κ has spectral radius above 1 (measured
    7.38), so κ ← (κ + κ_s)/2 — the exogenous driver's default — diverges: its gap grows from
    round to round (measured 0.82, 5.8 and 50 after 2, 4 and 6 rounds).
    The Newton update with the steady state's Jacobians converges in 5 rounds, and the damped
    driver at its own default (0.05) reaches the same path in 278."""
    Z = (1 + 0.01 * 0.9 ** np.arange(T60))[None]
    M = pkg.transition._labor_newton_matrix(ss100, jac100) + np.eye(T60)
    rho = np.max(np.abs(np.linalg.eigvals(M)))
    print(f"spectral radius of M: {rho:.3f}")
    assert rho > 3  # (1 + rho)/2 > 1 whatever the sign of the leading eigenvalue: 0.5 cannot work
    gaps = [pkg.aiyagari_labor_transition(ss100, Z, T60, damp=0.5, tol=1e-8, max_iter=k,
                                          backend=lr.labor_transition_batch)["resid"][0]
            for k in (2, 4, 6)]
    print("damp = 0.5 gaps after 2, 4, 6 rounds:", gaps)
    assert gaps[0] < gaps[1] < gaps[2] and gaps[2] > 1.0
    N = pkg.aiyagari_labor_transition_newton(ss100, Z, T60, jac=jac100, tol=1e-8,
                                             backend=lr.labor_transition_batch)
    assert N["status"][0] == 0 and N["resid"][0] < 1e-8 and N["rounds"][0] <= 6
    D = pkg.aiyagari_labor_transition(ss100, Z, T60, tol=1e-8, backend=lr.labor_transition_batch)
    print(f"rounds: Newton {N['rounds'][0]}, damped at its default {D['rounds'][0]}")
    assert D["status"][0] == 0 and D["resid"][0] < 1e-8 and D["rounds"][0] > N["rounds"][0]
    for k in ("K", "H", "kappa"):
        assert np.max(np.abs(D[k] - N[k])) < 1e-7, k
    assert N["K"][0, 0] == ss100["K"]          # K_0 is given ...
    assert abs(N["H"][0, 0] - ss100["H"]) > 1e-4  # ... and hours jump on impact


def test_labor_driver_paths_do_not_depend_on_the_batch(pkg, ss100, jac100):
    """Z ≡ 1 stops in round 1; every path of a batch equals its solo run bit for bit."""
    q = np.arange(T60)
    Z = np.stack([1 + 0.01 * 0.9 ** q, np.ones(T60), 1 - 0.005 * 0.8 ** q])
    run = lambda z: pkg.aiyagari_labor_transition_newton(ss100, z, T60, jac=jac100, tol=1e-8,
                                                         backend=lr.labor_transition_batch)
    A = run(Z)
    assert (A["status"] == 0).all() and A["rounds"][1] == 1 and (A["rounds"][[0, 2]] > 1).all()
    assert (A["r"][1] == ss100["r"]).all() and (A["w"][1] == ss100["w"]).all()
    for c in range(3):
        S = run(Z[c:c + 1])
        assert S["rounds"][0] == A["rounds"][c]
        for k in ("K", "H", "kappa", "r", "w"):
            assert same(S[k][0], A[k][c]), (c, k)


def test_impulse_response_labor_is_the_newton_path_to_first_order(pkg, ss100, jac100):
    """dK and dH of a 0.1 % shock against the nonlinear Newton path: the difference is second
    order in the shock plus the Jacobian's O(h) — below 2 % of the response."""
    dZ = (0.001 * 0.9 ** np.arange(T60))[None]
    N = pkg.aiyagari_labor_transition_newton(ss100, 1 + dZ, T60, jac=jac100, tol=1e-10,
                                             backend=lr.labor_transition_batch)
    dK, dH = pkg.impulse_response_labor(ss100, jac100, dZ)
    assert N["status"][0] == 0 and dK[0, 0] == 0
    eK = np.max(np.abs((N["K"][0] - ss100["K"]) - dK[0])) / np.max(np.abs(dK))
    eH = np.max(np.abs((N["H"][0] - ss100["H"]) - dH[0])) / np.max(np.abs(dH))
    print(f"linear vs nonlinear response: K {eK:.2e}, H {eH:.2e}")
    assert eK < 0.02 and eH < 0.02


# ------------------------------------------------------------- fake news vs brute force
def test_labor_fake_news_is_the_brute_force_jacobian(pkg):
    """N = 3, Na = 60, T = 30: the four Jacobians and the Newton matrix M composed from them
    against one-sided differences of 1 + T whole reference transitions, the same h in both.  The
    two differ by the one-sided difference's O(h) nonlinearity and nothing else, so the error
    must fall tenfold (asserted: to at most a fifth) from h = 1e-4 to h = 1e-5.  Measured on the
    reference, relative to max|·|: J_Kr 1.0e-4, J_Hr 9.0e-5, J_Kw 3.5e-6, J_Hw 2.2e-6 and M
    4.5e-5 at h = 1e-4, a tenth of each at h = 1e-5; the bound at h = 1e-4 is 5e-4, the size of h·|∂²K/∂r²|/|∂K/∂r| for
    a savings response with semi-elasticity of order 5 (J_Kr/K ≈ 3 here)."""
    T = 30
    cal = _cal(pkg, 3, 60)
    ss = lr.steady_state_labor_cpu(cal, 1.0, 1.0, _wage(pkg, cal))
    err = {}
    for h in (1e-4, 1e-5):
        J = lr.jacobian_labor_cpu(ss, T, h)
        B = {}
        for x in ("r", "w"):
            B["J_K" + x], B["J_H" + x] = lr.brute_force_labor_cpu(ss, T, h, x)
        for k in B:
            err[k, h] = np.max(np.abs(J[k] - B[k])) / np.max(np.abs(B[k]))
        M, Mb = (pkg.transition._labor_newton_matrix(ss, X) for X in (J, B))
        err["M", h] = np.max(np.abs(M - Mb)) / np.max(np.abs(Mb + np.eye(T)))
        if h == 1e-4:
            print(f"max |dM| = {np.max(np.abs(M - Mb)):.3e} against max |M| = "
                  f"{np.max(np.abs(Mb + np.eye(T))):.3f}")
    for k in ("J_Kr", "J_Kw", "J_Hr", "J_Hw", "M"):
        print(f"{k}: fake news vs brute force {err[k, 1e-4]:.3e} (h = 1e-4), "
              f"{err[k, 1e-5]:.3e} (h = 1e-5)")
        assert err[k, 1e-4] <= 5e-4, (k, err)
        assert err[k, 1e-5] <= 0.2 * err[k, 1e-4], (k, err)


# ------------------------------------------------------------------------------ refusals
N_, NA_, NC_, T_ = 2, 5, 3, 4
i64, d, ci = C.c_int64, C.c_double, C.c_int
NO_DEVICE = (5, "no HIP device visible")
BACK_FIT = ("backward labour EGM pass: a path's arrays exceed one CU's LDS "
            "(N <= 16, Na <= 1024, 3·N·Na doubles within 160 KiB)")
FWD_FIT = ("forward pass with hours: a path's arrays exceed one CU's LDS "
           "(N <= 16, 8·N·Na·3 + 4·N·(Na+1) + 8·Na + 2.3 KB within 160 KiB)")
JAC_FIT = ("Jacobian: the transition passes' arrays exceed one CU's LDS "
           "(aiy_labor_transition_batch's fit rules)")


def _base():
    n = N_ * NA_
    return dict(C=NC_, T=T_, N=N_, Na=NA_, r=np.full(NC_ * (T_ + 1), 0.02), w=np.full(NC_ * T_, 1.2),
                pcT=np.ones(NC_ * n), lam=np.full(NC_ * n, 1.0 / n), a=np.arange(NA_, dtype=np.float64),
                s=np.array([0.8, 1.2]), P=np.full(N_ * N_, 0.5), pk=np.zeros(NC_ * T_ * n),
                pl=np.zeros(NC_ * T_ * n), pc=np.zeros(NC_ * T_ * n), K=np.zeros(NC_ * (T_ + 1)),
                H=np.zeros(NC_ * T_), lT=np.zeros(NC_ * n), st=np.zeros(NC_, np.int32),
                ft=np.zeros(NC_, np.int32), phi=1.0, theta=1.0, h=1e-4, r_ss=0.03, w_ss=1.2,
                J=np.zeros(4 * T_ * T_), F=np.zeros(4 * T_ * T_), E=np.zeros(2 * T_ * n))


def _set(key, idx, v):
    return lambda a: a[key].__setitem__(idx, v)


DEFECTS = {
    "valid": lambda a: None, "C0": lambda a: a.update(C=0), "T0": lambda a: a.update(T=0),
    "N0": lambda a: a.update(N=0), "Na1": lambda a: a.update(Na=1), "N17": lambda a: a.update(N=17),
    "Na1025": lambda a: a.update(Na=1025), "Na500": lambda a: a.update(Na=500, N=16),
    "Na400": lambda a: a.update(Na=400, N=16),
    "a_nan": _set("a", 0, np.nan), "a_dec": _set("a", 2, 0.5), "a_rep": _set("a", 4, 3.0),
    "r_nan": _set("r", -1, np.nan), "r_m1": _set("r", T_ + 1, -1.0),
    "w_inf": _set("w", T_ + 2, -np.inf),
    "phi0": lambda a: a.update(phi=0.0), "phi_neg": lambda a: a.update(phi=-1.0),
    "phi_nan": lambda a: a.update(phi=np.nan), "phi_inf": lambda a: a.update(phi=np.inf),
    "theta0": lambda a: a.update(theta=0.0), "theta_nan": lambda a: a.update(theta=np.nan),
    "theta_inf": lambda a: a.update(theta=-np.inf),
    "h0": lambda a: a.update(h=0.0), "rss_m1": lambda a: a.update(r_ss=-1.0),
    "wss_nan": lambda a: a.update(w_ss=np.nan),
    "null:pk": lambda a: a.update(pk=None), "null:pl": lambda a: a.update(pl=None),
    "null:r": lambda a: a.update(r=None), "null:K": lambda a: a.update(K=None),
    "null:H": lambda a: a.update(H=None), "null:lam": lambda a: a.update(lam=None),
    "null:pc": lambda a: a.update(pc=None), "null:lT": lambda a: a.update(lT=None),
    "null:a": lambda a: a.update(a=None), "null:s": lambda a: a.update(s=None),
    "null:J": lambda a: a.update(J=None), "null:F": lambda a: a.update(F=None),
    "null:E": lambda a: a.update(E=None), "null:pcT": lambda a: a.update(pcT=None),
}


def _p(x):
    return None if x is None else x.ctypes.data_as(C.c_void_p)


def _backward(L, a):
    return L.aiy_labor_egm_backward_batch(
        i64(a["C"]), i64(a["T"]), _p(a["r"]), _p(a["w"]), _p(a["pcT"]), ci(0), _p(a["a"]),
        _p(a["s"]), _p(a["P"]), i64(a["N"]), i64(a["Na"]), d(0.96), d(5.0), d(a["phi"]),
        d(a["theta"]), d(0.0), _p(a["pk"]), _p(a["pl"]), _p(a["pc"]), _p(a["st"]), _p(a["ft"]))


def _forward(L, a):
    return L.aiy_labor_dist_forward_batch(
        i64(a["C"]), i64(a["T"]), _p(a["pk"]), _p(a["pl"]), _p(a["lam"]), ci(0), _p(a["a"]),
        _p(a["s"]), _p(a["P"]), i64(a["N"]), i64(a["Na"]), _p(a["K"]), _p(a["H"]), _p(a["lT"]),
        _p(a["st"]), _p(a["ft"]))


def _both(L, a):
    return L.aiy_labor_transition_batch(
        i64(a["C"]), i64(a["T"]), _p(a["r"]), _p(a["w"]), _p(a["pcT"]), ci(0), _p(a["lam"]), ci(0),
        _p(a["a"]), _p(a["s"]), _p(a["P"]), i64(a["N"]), i64(a["Na"]), d(0.96), d(5.0), d(a["phi"]),
        d(a["theta"]), d(0.0), _p(a["K"]), _p(a["H"]), _p(a["st"]), _p(a["ft"]))


def _jacobian(L, a):
    tt = a["T"] * a["T"] if a["T"] > 0 else 0
    part = lambda x, q: None if x is None else x[q * tt:]
    J, F, E, st = a["J"], a["F"], a["E"], a["st"]
    return L.aiy_ssj_jacobian_labor(
        _p(a["pcT"]), _p(a["lam"]), d(a["r_ss"]), d(a["w_ss"]), _p(a["a"]), _p(a["s"]), _p(a["P"]),
        i64(a["N"]), i64(a["Na"]), d(0.96), d(5.0), d(a["phi"]), d(a["theta"]), d(0.0),
        i64(a["T"]), d(a["h"]), _p(J), _p(part(J, 1)), _p(part(J, 2)), _p(part(J, 3)), _p(F),
        _p(part(F, 1)), _p(part(F, 2)), _p(part(F, 3)), _p(E),
        _p(None if E is None else E[E.size // 2:]), _p(st), _p(st[1:]), None)


CALLERS = {"aiy_labor_egm_backward_batch": _backward, "aiy_labor_dist_forward_batch": _forward,
           "aiy_labor_transition_batch": _both, "aiy_ssj_jacobian_labor": _jacobian}
A_DEC = (6, "a_grid must be non-decreasing (a_grid(3) < a_grid(2))")
A_REP = (6, "grid must be strictly increasing (point 5 repeats point 4)")
R_LAST = (6, "path 3, period 4: r must be finite with 1 + r > 0")
PHI = (6, "phi must be positive and finite")
THETA = (6, "theta must be finite and not 0")
B_, F_, T2_, J_ = (
    "aiy_labor_egm_backward_batch", "aiy_labor_dist_forward_batch", "aiy_labor_transition_batch",
    "aiy_ssj_jacobian_labor")
# (entry, defects) -> the answer; a defect pair shows which check comes first
EXPECTED = {
    (B_, "null:pk"): (6, "NULL argument"), (B_, "null:pl"): (6, "NULL argument"),
    (B_, "null:r+C0"): (6, "NULL argument"), (B_, "null:s"): (6, "NULL argument"),
    (B_, "C0"): (1, "need 1 <= C < 2^31"), (B_, "C0+T0"): (1, "need 1 <= C < 2^31"),
    (B_, "T0"): (1, "T must be in [1, 2^31 - 1)"), (B_, "T0+N0"): (1, "T must be in [1, 2^31 - 1)"),
    (B_, "N0"): (1, "need N >= 1 and Na >= 2"), (B_, "Na1"): (1, "need N >= 1 and Na >= 2"),
    (B_, "N17"): (6, BACK_FIT), (B_, "Na1025"): (6, BACK_FIT), (B_, "N17+phi0"): (6, BACK_FIT),
    (B_, "phi0"): PHI, (B_, "phi_neg"): PHI, (B_, "phi_nan"): PHI, (B_, "phi_inf"): PHI,
    (B_, "phi0+theta0"): PHI, (B_, "theta0"): THETA, (B_, "theta_nan"): THETA,
    (B_, "theta_inf"): THETA, (B_, "theta0+a_nan"): THETA,
    (B_, "null:a"): (6, "a_grid is NULL"), (B_, "a_nan"): (2, "a_grid(1) is not finite"),
    (B_, "a_dec"): A_DEC, (B_, "a_rep"): A_REP, (B_, "a_rep+r_nan"): A_REP,
    (B_, "r_nan"): R_LAST,
    (B_, "r_m1"): (6, "path 2, period 0: r must be finite with 1 + r > 0"),
    (B_, "w_inf"): (6, "path 2, period 2: w must be finite"),
    (B_, "null:pc"): NO_DEVICE, (B_, "valid"): NO_DEVICE,
    (F_, "null:K"): (6, "NULL argument"), (F_, "null:H"): (6, "NULL argument"),
    (F_, "null:pl"): (6, "NULL argument"), (F_, "null:s"): (6, "NULL argument"),
    (F_, "null:lam+T0"): (6, "NULL argument"),
    (F_, "C0"): (1, "need 1 <= C < 2^31"), (F_, "T0"): (1, "T must be in [1, 2^31 - 1)"),
    (F_, "Na1"): (1, "need N >= 1 and Na >= 2"), (F_, "N17"): (6, FWD_FIT),
    (F_, "Na500"): (6, FWD_FIT), (F_, "a_dec"): A_DEC, (F_, "a_rep"): A_REP,
    (F_, "null:lT"): NO_DEVICE, (F_, "valid"): NO_DEVICE,
    (T2_, "null:K"): (6, "NULL argument"), (T2_, "null:H"): (6, "NULL argument"),
    (T2_, "C0"): (1, "need 1 <= C < 2^31"), (T2_, "T0"): (1, "T must be in [1, 2^31 - 1)"),
    (T2_, "Na1025"): (6, BACK_FIT), (T2_, "Na500"): (6, BACK_FIT),
    (T2_, "Na400"): (6, FWD_FIT), (F_, "Na400"): (6, FWD_FIT), (J_, "Na400"): (6, JAC_FIT),
    (T2_, "phi_nan"): PHI, (T2_, "theta0"): THETA,
    (T2_, "a_nan"): (2, "a_grid(1) is not finite"), (T2_, "a_rep"): A_REP,
    (T2_, "r_nan"): R_LAST, (T2_, "w_inf"): (6, "path 2, period 2: w must be finite"),
    (T2_, "valid"): NO_DEVICE,
    (J_, "null:pcT"): (6, "NULL argument"), (J_, "null:J+T0"): (6, "NULL argument"),
    (J_, "N0"): (1, "need N >= 1 and Na >= 2"), (J_, "N17"): (6, JAC_FIT),
    (J_, "Na500"): (6, JAC_FIT), (J_, "Na1025"): (6, JAC_FIT),
    (J_, "T0"): (1, "T must be in [1, 32768]"), (J_, "h0"): (6, "h must be positive and finite"),
    (J_, "null:a"): (6, "a_grid is NULL"), (J_, "a_dec"): A_DEC, (J_, "a_rep+phi0"): A_REP,
    (J_, "phi0"): PHI, (J_, "phi_inf"): PHI, (J_, "theta0"): THETA, (J_, "theta_nan"): THETA,
    (J_, "theta0+rss_m1"): THETA,
    (J_, "rss_m1"): (6, "r_ss must be finite with 1 + r_ss > 0"),
    (J_, "wss_nan"): (6, "w_ss must be finite"),
    (J_, "null:F"): NO_DEVICE, (J_, "null:E"): NO_DEVICE, (J_, "valid"): NO_DEVICE,
}


def test_the_fit_rules_the_labor_refusals_quote(pkg):
    """Backward: three N·Na arrays and the 2.4 KB scratch.  Forward: the exogenous pass's arrays
    and s [16].  N = 16, Na = 500 fits neither; N = 2, Na = 1025 is past the fused cap; N = 16,
    Na = 400 fits the backward pass only; the scripts' grid fits both.  The forward pass admits every N >= 1, Na >= 2: n = 2 and 3 leave
    the mass array's spare half one double short of two block sums, and the kernel keeps the
    hours' single block sum in the scratch's unused key slot there."""
    back = lambda N, Na: N <= 16 and Na <= 1024 and 8 * 3 * N * Na + 8 * 288 + 64 <= 160 * 1024
    fwd = lambda N, Na: (N <= 16 and 24 * N * Na + 4 * ((N * (Na + 1) + 1) // 2 * 2) + 8 * Na
                         + 8 * 272 + 64 + 128 <= 160 * 1024)
    assert not back(16, 500) and not fwd(16, 500) and not back(2, 1025)
    assert back(7, 400) and fwd(7, 400) and back(16, 400) and not fwd(16, 400)
    assert fwd(1, 2) and back(1, 2)
    for n in (2, 3):
        assert 2 * -(-n // 256) > n // 2
    for n in (4, 5, 256, 257, 513, 16384):
        assert 2 * -(-n // 256) <= n // 2


@pytest.mark.parametrize("entry,defects", sorted(EXPECTED))
def test_labor_transition_refusal(pkg, entry, defects):
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


def test_declared_symbols_list_the_labor_entries(pkg):
    names = set(pkg.declared_symbols())
    want = {"aiy_labor_egm_backward_batch_dev", "aiy_labor_egm_backward_batch",
            "aiy_labor_dist_forward_batch_dev", "aiy_labor_dist_forward_batch",
            "aiy_labor_transition_batch", "aiy_ssj_jacobian_labor"}
    assert want <= names
    assert all(hasattr(pkg.lib(), s) for s in want)
