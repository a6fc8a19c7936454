"""No GPU: the transition's CPU reference against the C oracle, the pricing rule, the lockstep
driver on the reference backend, and which refusal each transition host entry answers before it
asks for a device (in the manner of test_aiy_host_refusals_cpu.py)."""
import ctypes as C

import numpy as np
import pytest

from oracle import corc
from tests import transition_ref as tr


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.int64)


def same(x, y):
    return np.array_equal(bits(x), bits(y))


def _cal(pkg, N, Na):
    cb = pkg.calibration
    return cb.aiyagari(Na=Na) if N == 7 else cb.aiyagari(Na=Na, shocks="rouwenhorst", N=N)


# ------------------------------------------------- the reference is the oracle's step, r split
@pytest.mark.parametrize("N,Na", [(3, 37), (7, 400)])
def test_constant_path_is_the_chained_oracle_step(pkg, N, Na):
    """r_next == r_now == r: T steps of the two-rate reference equal T chained corc.egm_step
    calls bit for bit, pk and pc at every period."""
    cb, T, r = pkg.calibration, 4, 0.025
    cal = _cal(pkg, N, Na)
    a, s, P = cal["a_grid"], cal["s"], cal["P"]
    w = cb.wage(r, cal["alpha"], cal["delta"])
    pcT = np.tile((1 + r) * a + w * np.mean(s), (N, 1))
    B = tr.egm_backward(np.full(T + 1, r), np.full(T, w), pcT, a, s, P, cal["beta"], cal["sigma"],
                        cal["amin"])
    assert B["status"] == 0 and B["fail_t"] == -1
    cur = pcT
    for t in range(T - 1, -1, -1):
        cur, pk, _ = corc.egm_step(cur, a, s, P, r, w, cal["beta"], cal["sigma"], cal["amin"])
        assert same(cur, B["pc"][t]) and same(pk, B["pk"][t]), t


def test_the_golden_path_loses_monotonicity_where_recorded(golden, pkg):
    """tests/golden/transition_nonmonotone.npz: a wage that turns negative in period 3 (sigma = 2,
    so marginal utility stays positive at negative consumption) makes period 2's endogenous grid
    finite and not increasing.  The reference stops there."""
    G = golden("transition_nonmonotone")
    cal = _cal(pkg, int(G["N"]), int(G["Na"]))
    a, s, P = cal["a_grid"], cal["s"], cal["P"]
    B = tr.egm_backward(G["r"], G["w"], G["pc_T"], a, s, P, cal["beta"], float(G["sigma"]),
                        cal["amin"])
    ft = int(G["fail_t"])
    assert (B["status"], B["fail_t"]) == (1, ft) and 0 < ft < len(G["w"]) - 1
    _, _, ah, bad = tr.egm_step2(B["pc"][ft + 1], a, s, P, G["r"][ft + 1], G["r"][ft], G["w"][ft],
                                 cal["beta"], float(G["sigma"]), cal["amin"])
    assert bad == 1 and np.isfinite(ah).all() and (np.diff(ah, axis=1) <= 0).any()
    assert np.isnan(B["pk"][:ft]).all() and np.isfinite(B["pk"][ft + 1:]).all()


# ------------------------------------------------------------------------------ pricing
def test_prices_at_the_stationary_point_are_exact(pkg):
    cal = _cal(pkg, 7, 20)
    for r_ss, w_ss, K_ss in [(0.0371234567, 1.1876543, 5.4321), (-0.0123, 0.9, 11.0 / 3)]:
        ss = dict(r=r_ss, w=w_ss, K=K_ss, cal=cal)
        r, w = pkg.prices_from_K(np.full((3, 9), K_ss), np.ones((3, 9)), ss)
        assert (r == r_ss).all() and (w == w_ss).all()
    # and away from it the anchored Cobb-Douglas rule
    K, Z = np.array([[4.0, 6.0]]), np.array([[0.99, 1.02]])
    r, w = pkg.prices_from_K(K, Z, ss)
    al, de = cal["alpha"], cal["delta"]
    assert np.allclose(r + de, (r_ss + de) * Z * (K / K_ss) ** (al - 1), rtol=1e-13, atol=0)
    assert np.allclose(w, w_ss * Z * (K / K_ss) ** al, rtol=1e-13, atol=0)


# ------------------------------------------------------------------------------ the driver
@pytest.fixture(scope="module")
def ss60(pkg):
    cb = pkg.calibration
    cal = _cal(pkg, 3, 60)
    return tr.steady_state_cpu(cal, 0.03, lambda r: cb.wage(r, cal["alpha"], cal["delta"]))


def test_lockstep_driver_paths_do_not_depend_on_the_batch(pkg, ss60):
    """Three shocks in one batch: each path's K, rounds and status equal its solo run's."""
    T = 12
    q = np.arange(T)
    Z = np.stack([1 - 0.01 * 0.8 ** q, np.ones(T), 1 + 0.005 * 0.5 ** q])
    run = lambda z: pkg.aiyagari_transition(ss60, z, T, damp=0.5, tol=1e-6, max_iter=60,
                                            backend=tr.transition_batch)
    A = run(Z)
    assert (A["status"] == 0).all() and (A["resid"] < 1e-6).all()
    assert A["rounds"][1] == 1 and A["rounds"][0] > 3  # Z ≡ 1 stays put; a shock takes rounds
    assert (A["K"][:, 0] == ss60["K"]).all() and A["K"][0].min() < ss60["K"] - 1e-3
    for c in range(3):
        S = run(Z[c:c + 1])
        assert S["rounds"][0] == A["rounds"][c] and S["status"][0] == A["status"][c]
        for k in ("K", "r", "w"):
            assert same(S[k][0], A[k][c]), (c, k)


# ------------------------------------------------------------------------------ refusals
N_, NA_, NC_, T_ = 2, 5, 3, 4
i64, d, ci = C.c_int64, C.c_double, C.c_int
NO_DEVICE = (5, "no HIP device visible")
BACK_FIT = ("backward EGM pass: a path's arrays exceed one CU's LDS "
            "(N <= 16, Na <= 1024, (2N+1)·Na doubles within 160 KiB)")
FWD_FIT = ("forward histogram pass: a path's arrays exceed one CU's LDS "
           "(N <= 16, 8·N·Na·3 + 4·N·(Na+1) + 8·Na + 2.2 KB within 160 KiB)")


def _base():
    n = N_ * NA_
    return dict(C=NC_, T=T_, N=N_, Na=NA_, r=np.full(NC_ * (T_ + 1), 0.02), w=np.full(NC_ * T_, 1.2),
                pcT=np.ones(NC_ * n), lam=np.full(NC_ * n, 1.0 / n), a=np.arange(NA_, dtype=np.float64),
                s=np.array([0.8, 1.2]), P=np.full(N_ * N_, 0.5), pk=np.zeros(NC_ * T_ * n),
                pc=np.zeros(NC_ * T_ * n), K=np.zeros(NC_ * (T_ + 1)), lT=np.zeros(NC_ * n),
                st=np.zeros(NC_, np.int32), ft=np.zeros(NC_, np.int32))


def _set(key, idx, v):
    return lambda a: a[key].__setitem__(idx, v)


DEFECTS = {
    "valid": lambda a: None, "C0": lambda a: a.update(C=0), "T0": lambda a: a.update(T=0),
    "N0": lambda a: a.update(N=0), "Na1": lambda a: a.update(Na=1), "N17": lambda a: a.update(N=17),
    "Na1025": lambda a: a.update(Na=1025), "Na500": lambda a: a.update(Na=500, N=16),
    "a_nan": _set("a", 0, np.nan), "a_dec": _set("a", 2, 0.5), "a_rep": _set("a", 4, 3.0),
    "r_nan": _set("r", -1, np.nan), "r_inf": _set("r", 0, np.inf), "r_m1": _set("r", T_ + 1, -1.0),
    "w_inf": _set("w", T_ + 2, -np.inf),
    "null:pk": lambda a: a.update(pk=None), "null:r": lambda a: a.update(r=None),
    "null:K": lambda a: a.update(K=None), "null:lam": lambda a: a.update(lam=None),
    "null:pc": lambda a: a.update(pc=None), "null:lT": lambda a: a.update(lT=None),
    "null:a": lambda a: a.update(a=None),
}


def _p(x):
    return None if x is None else x.ctypes.data_as(C.c_void_p)


def _backward(L, a):
    return L.aiy_egm_backward_batch(i64(a["C"]), i64(a["T"]), _p(a["r"]), _p(a["w"]), _p(a["pcT"]),
                                    ci(0), _p(a["a"]), _p(a["s"]), _p(a["P"]), i64(a["N"]),
                                    i64(a["Na"]), d(0.96), d(5.0), d(0.0), _p(a["pk"]), _p(a["pc"]),
                                    _p(a["st"]), _p(a["ft"]))


def _forward(L, a):
    return L.aiy_dist_forward_batch(i64(a["C"]), i64(a["T"]), _p(a["pk"]), _p(a["lam"]), ci(0),
                                    _p(a["a"]), _p(a["P"]), i64(a["N"]), i64(a["Na"]), _p(a["K"]),
                                    _p(a["lT"]), _p(a["st"]), _p(a["ft"]))


def _both(L, a):
    return L.aiy_transition_batch(i64(a["C"]), i64(a["T"]), _p(a["r"]), _p(a["w"]), _p(a["pcT"]),
                                  ci(0), _p(a["lam"]), ci(0), _p(a["a"]), _p(a["s"]), _p(a["P"]),
                                  i64(a["N"]), i64(a["Na"]), d(0.96), d(5.0), d(0.0), _p(a["K"]),
                                  _p(a["st"]), _p(a["ft"]))


CALLERS = {"aiy_egm_backward_batch": _backward, "aiy_dist_forward_batch": _forward,
           "aiy_transition_batch": _both}
A_DEC = (6, "a_grid must be non-decreasing (a_grid(3) < a_grid(2))")
A_REP = (6, "grid must be strictly increasing (point 5 repeats point 4)")
R_LAST = (6, "path 3, period 4: r must be finite with 1 + r > 0")
# (entry, defects) -> the answer; a defect pair shows which check comes first
EXPECTED = {
    ("aiy_egm_backward_batch", "null:pk"): (6, "NULL argument"),
    ("aiy_egm_backward_batch", "null:r+C0"): (6, "NULL argument"),
    ("aiy_egm_backward_batch", "C0"): (1, "need 1 <= C < 2^31"),
    ("aiy_egm_backward_batch", "C0+T0"): (1, "need 1 <= C < 2^31"),
    ("aiy_egm_backward_batch", "T0"): (1, "T must be in [1, 2^31 - 1)"),
    ("aiy_egm_backward_batch", "T0+N0"): (1, "T must be in [1, 2^31 - 1)"),
    ("aiy_egm_backward_batch", "N0"): (1, "need N >= 1 and Na >= 2"),
    ("aiy_egm_backward_batch", "Na1"): (1, "need N >= 1 and Na >= 2"),
    ("aiy_egm_backward_batch", "N17"): (6, BACK_FIT),
    ("aiy_egm_backward_batch", "Na1025"): (6, BACK_FIT),
    ("aiy_egm_backward_batch", "N17+a_nan"): (6, BACK_FIT),
    ("aiy_egm_backward_batch", "null:a"): (6, "a_grid is NULL"),
    ("aiy_egm_backward_batch", "a_nan"): (2, "a_grid(1) is not finite"),
    ("aiy_egm_backward_batch", "a_dec"): A_DEC,
    ("aiy_egm_backward_batch", "a_rep"): A_REP,
    ("aiy_egm_backward_batch", "a_rep+r_nan"): A_REP,
    ("aiy_egm_backward_batch", "r_nan"): R_LAST,
    ("aiy_egm_backward_batch", "r_inf"): (6, "path 1, period 0: r must be finite with 1 + r > 0"),
    ("aiy_egm_backward_batch", "r_m1"): (6, "path 2, period 0: r must be finite with 1 + r > 0"),
    ("aiy_egm_backward_batch", "w_inf"): (6, "path 2, period 2: w must be finite"),
    ("aiy_egm_backward_batch", "r_m1+w_inf"): (6, "path 2, period 0: r must be finite with 1 + r > 0"),
    ("aiy_egm_backward_batch", "null:pc"): NO_DEVICE,
    ("aiy_egm_backward_batch", "valid"): NO_DEVICE,
    ("aiy_dist_forward_batch", "null:K"): (6, "NULL argument"),
    ("aiy_dist_forward_batch", "null:lam+T0"): (6, "NULL argument"),
    ("aiy_dist_forward_batch", "C0"): (1, "need 1 <= C < 2^31"),
    ("aiy_dist_forward_batch", "T0"): (1, "T must be in [1, 2^31 - 1)"),
    ("aiy_dist_forward_batch", "Na1"): (1, "need N >= 1 and Na >= 2"),
    ("aiy_dist_forward_batch", "N17"): (6, FWD_FIT),
    ("aiy_dist_forward_batch", "Na500"): (6, FWD_FIT),
    ("aiy_dist_forward_batch", "a_dec"): A_DEC,
    ("aiy_dist_forward_batch", "a_rep"): A_REP,
    ("aiy_dist_forward_batch", "null:lT"): NO_DEVICE,
    ("aiy_dist_forward_batch", "valid"): NO_DEVICE,
    ("aiy_transition_batch", "null:K"): (6, "NULL argument"),
    ("aiy_transition_batch", "C0"): (1, "need 1 <= C < 2^31"),
    ("aiy_transition_batch", "T0"): (1, "T must be in [1, 2^31 - 1)"),
    ("aiy_transition_batch", "Na1025"): (6, BACK_FIT),
    ("aiy_transition_batch", "Na500"): (6, FWD_FIT),
    ("aiy_transition_batch", "a_nan"): (2, "a_grid(1) is not finite"),
    ("aiy_transition_batch", "a_rep"): A_REP,
    ("aiy_transition_batch", "r_nan"): R_LAST,
    ("aiy_transition_batch", "w_inf"): (6, "path 2, period 2: w must be finite"),
    ("aiy_transition_batch", "valid"): NO_DEVICE,
}


def test_the_fit_rules_the_refusals_quote(pkg):
    """N = 16, Na = 500: (2N+1)·Na doubles fit the backward pass, three N·Na arrays and the
    offsets do not fit the forward pass — so aiy_transition_batch refuses it with the forward
    text.  Na = 1025 is past the fused cap of the backward pass."""
    back = lambda N, Na: N <= 16 and Na <= 1024 and 8 * (2 * N + 1) * Na + 8 * 288 + 64 <= 160 * 1024
    fwd = lambda N, Na: (N <= 16 and 24 * N * Na + 4 * ((N * (Na + 1) + 1) // 2 * 2) + 8 * Na
                         + 8 * 272 + 64 <= 160 * 1024)
    assert back(16, 500) and not fwd(16, 500) and not back(2, 1025) and fwd(7, 400) and back(7, 400)


@pytest.mark.parametrize("entry,defects", sorted(EXPECTED))
def test_transition_refusal(pkg, entry, defects):
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
