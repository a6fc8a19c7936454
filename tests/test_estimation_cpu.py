"""No GPU: the likelihood's CPU reference (tests/estimation_ref.py) against dense numpy, the
general-equilibrium Jacobians against the per-path impulse response and the resource constraint,
the zooming-grid maximiser on the reference backend against brute force, and which refusal each
new host entry answers before it asks for a device (in the manner of test_ssj_cpu.py)."""
import ctypes as C

import numpy as np
import pytest

from tests import estimation_ref as er
from tests import ssj_ref as sr
from tests import transition_ref as tr

T40 = 40


@pytest.fixture(scope="module")
def ss60(pkg):
    """N = 3, Na = 60: the stationary point at r = 0.03 (test_ssj_cpu.py's)."""
    cb = pkg.calibration
    cal = cb.aiyagari(Na=60, shocks="rouwenhorst", N=3)
    return tr.steady_state_cpu(cal, 0.03, lambda r: cb.wage(r, cal["alpha"], cal["delta"]))


@pytest.fixture(scope="module")
def jac40(ss60):
    return sr.jacobian_cpu(ss60, T40, 1e-4)


# ------------------------------------------------------------- the reference vs dense numpy
ME_FRACTION = 1e-3  # me_var[o] = ME_FRACTION·Γ[0][o][o]: cond₂(V) is 2.0e2, 5.9e4 and 4.2e4
C_GAP = 0.0131      # 4 × the largest measured gap, 3.26e-3 units of n·2⁻⁵²·cond₂(V) (case 1, quad)
DENSE_CASES = [(("Y",), 8, 40), (("Y", "C", "K"), 7, 17), (("Y", "C"), 30, 40)]


@pytest.mark.parametrize("outs,L,T", DENSE_CASES)
def test_reference_is_dense_numpy(pkg, ss60, jac40, outs, L, T):
    """logdet and quad of the reference's LDLᵀ against slogdet and solve on the full V, relative,
    within c·n·2⁻⁵²·cond₂(V) — the backward-error form of a Cholesky-type solve — with c = 4 × the
    largest gap measured in those units.  Measured (units): logdet 6.0e-4, 2.2e-6, 5.0e-6; quad
    3.26e-3, 2.6e-5, 9.0e-5.  m: the first T MA coefficients of the observables under an AR(1)
    (ρ = 0.9, σ = 0.01); me_var a stated fraction of the variances, which bounds cond₂(V)."""
    est = pkg.estimation
    G = est.ge_jacobians(ss60, jac40, outs)
    n_o, n = len(outs), len(outs) * L
    m = er.ma_batch(G, est.ar1_ma([0.9], [0.01], T40))[0][:, :T].copy()
    Gam = er.autocovariance_batch(m, L)[0]
    me = ME_FRACTION * np.diagonal(Gam[0])
    y = er.simulate(m, L, me, 7)
    R = er.loglik_batch(m, y, me, want_gamma=True, want_d=True)
    assert R["status"][0] == 0 and R["fail"][0] == -1
    assert np.array_equal(R["Gamma"][0], Gam) and Gam.shape == (L, n_o, n_o)
    # Γ itself: the lag sums against numpy's
    for l in range(L):
        want = m[:, l:] @ m[:, :T - l].T if l < T else np.zeros((n_o, n_o))
        assert np.allclose(Gam[l], want, rtol=1e-12, atol=1e-12 * np.abs(Gam[0]).max()), l
    ll, logdet, quad, cond = er.dense_loglik(Gam, y, me)
    assert cond <= 1e6, cond  # a condition on the inputs
    d = R["d"][0]
    assert (d > 0).all()
    ld_ref = float(np.sum(np.log(d)))
    q_ref = -2 * R["loglik"][0] - n * np.log(2 * np.pi) - ld_ref
    unit = n * 2.0 ** -52 * cond
    g_ld, g_q = abs(ld_ref - logdet) / abs(logdet), abs(q_ref - quad) / abs(quad)
    print(f"{outs} L={L} T={T}: cond {cond:.3e}, gap logdet {g_ld / unit:.3e} quad "
          f"{g_q / unit:.3e} (units of n·2^-52·cond), loglik {R['loglik'][0]!r} vs {ll!r}")
    assert g_ld <= C_GAP * unit and g_q <= C_GAP * unit


def test_reference_flags_a_singular_covariance():
    """Two equal rows of m and no measurement error: L₁₀ = g/g = 1 and the second pivot is
    g − 1·g = 0 exactly — status 1, fail 1, loglik NaN, d = (g, 0, NaN, …)."""
    row = np.random.default_rng(2).standard_normal(9)
    R = er.loglik_batch(np.stack([row, row]), np.ones((3, 2)), np.zeros(2), want_d=True)
    assert R["status"][0] == 1 and R["fail"][0] == 1 and np.isnan(R["loglik"][0])
    d = R["d"][0]
    assert d[0] > 0 and d[1] == 0 and np.isnan(d[2:]).all()


# ------------------------------------------------------------- ge_jacobians
def test_ge_jacobians_are_the_impulse_response(pkg, ss60, jac40):
    """G_K·dZ = impulse_response(ss, jac, dZ)[:, :T] to 1e-12 relative (one multi-right-hand-side
    solve against one solve per path); every output against its definition on the per-path
    responses; C + K′ − (1 − δ)K − Y = 0 to rounding, K′ from the impulse response."""
    est = pkg.estimation
    G = dict(zip(est.OUTPUTS, est.ge_jacobians(ss60, jac40)))
    assert set(G) == {"K", "Y", "C", "r", "w"} and (G["K"][0] == 0).all()
    dZ = np.stack([0.01 * 0.9 ** np.arange(T40), -0.005 * 0.5 ** np.arange(T40),
                   np.eye(T40)[3]])
    dK = pkg.impulse_response(ss60, jac40, dZ)
    scale = np.abs(dK).max(axis=1, keepdims=True)
    assert (np.abs(dZ @ G["K"].T - dK[:, :T40]) <= 1e-12 * scale).all()
    ref = er.ge_jacobians(pkg, ss60, jac40)
    for o in est.OUTPUTS:
        assert np.abs(G[o] - ref[o]).max() <= 1e-12 * np.abs(ref[o]).max(), o
    delta = ss60["cal"]["delta"]
    X = {o: dZ @ G[o].T for o in G}
    resid = X["C"] + dK[:, 1:] - (1 - delta) * X["K"] - X["Y"]
    assert np.abs(resid).max() <= 1e-12 * np.abs(X["Y"]).max()
    assert np.array_equal(est.ge_jacobians(ss60, jac40, ("C", "r")), np.stack([G["C"], G["r"]]))
    with pytest.raises(ValueError):
        est.ge_jacobians(ss60, jac40, ("K", "H"))


def test_ar1_ma_is_a_running_product(pkg):
    est = pkg.estimation
    rho, sig = np.array([0.9, 0.3, 0.977]), np.array([0.01, 2.0, 0.5])
    dZ = est.ar1_ma(rho, sig, 7)
    assert dZ.shape == (3, 7)
    for c in range(3):
        v = sig[c]
        for s in range(7):
            assert dZ[c, s] == v
            v = v * rho[c]
        assert np.array_equal(est.ar1_ma(rho[c:c + 1], sig[c:c + 1], 7)[0], dZ[c])


def test_moments(pkg):
    est = pkg.estimation
    m = np.random.default_rng(4).standard_normal((2, 3, 11))
    Gam = er.autocovariance_batch(m, 4)
    M = est.moments(Gam, lags=(0, 2))
    assert M["sd"].shape == (2, 3) and M["corr"].shape == (2, 2, 3, 3)
    assert np.allclose(M["sd"] ** 2, np.einsum("cot,cot->co", m, m))
    assert np.allclose(np.diagonal(M["corr"][:, 0], axis1=-2, axis2=-1), 1.0)
    assert np.allclose(M["corr"][1, 1, 0, 2],
                       np.dot(m[1, 0, 2:], m[1, 2, :-2]) / (M["sd"][1, 0] * M["sd"][1, 2]))


# ------------------------------------------------------------- the maximiser
def test_ar1_mle_is_the_brute_force_argmax_of_its_grids(pkg, ss60, jac40):
    """On the reference backend: every round's pick is the first maximum of the grid laid over
    that round's box, recomputed here; the boxes nest and shrink by 2/(width − 1)."""
    est = pkg.estimation
    G = est.ge_jacobians(ss60, jac40, ("Y", "C"))
    m = er.ma_batch(G, est.ar1_ma([0.8], [0.01], T40))[0]
    me = 1e-2 * np.einsum("ot,ot->o", m, m)
    y = er.simulate(m, 20, me, 11)
    width, rounds = 5, 4
    R = est.ar1_mle(G, y, me, (0.3, 0.99), (0.002, 0.05), width=width, rounds=rounds,
                    backend=er.BACKEND)
    assert len(R["boxes"]) == rounds + 1 and list(R["evals"]) == [width * width] * rounds
    best = -np.inf
    for q, ((rl, rh), (sl, sh)) in enumerate(R["boxes"][:-1]):
        rr, sg = np.linspace(rl, rh, width), np.linspace(sl, sh, width)
        ll = np.array([[est.ar1_loglik(G, y, [a], [b], me, backend=er.BACKEND)["loglik"][0]
                        for b in sg] for a in rr])
        assert np.isfinite(ll).all()
        pick = int(np.argmax(ll.ravel()))
        assert pick == R["best"][q], q
        best = max(best, ll.ravel()[pick])
        (nrl, nrh), (nsl, nsh) = R["boxes"][q + 1]
        assert rl <= nrl < nrh <= rh and sl <= nsl < nsh <= sh
        assert nrh - nrl <= 2 * (rh - rl) / (width - 1) * (1 + 1e-12)
    assert R["loglik"] == best
    assert 0.3 <= R["rho"] <= 0.99 and 0.002 <= R["sigma"] <= 0.05
    one = est.ar1_loglik(G, y, [R["rho"]], [R["sigma"]], me, backend=er.BACKEND)
    assert one["loglik"][0] == R["loglik"]


def test_ar1_mle_skips_failed_candidates(pkg):
    """A backend whose candidates with sigma below a threshold report status 1 (with a loglik that
    would otherwise win): the pick is the best of the others; none left ends the search."""
    est = pkg.estimation
    G = np.eye(3)[None]

    def lik(m, y, me_var):
        s = m[:, 0, 0]
        return dict(loglik=-s, status=(s < 0.5).astype(np.int32), fail=np.zeros(s.size, np.int32))
    R = est.ar1_mle(G, np.zeros((2, 1)), np.zeros(1), (0.1, 0.9), (0.0, 1.0), width=5, rounds=1,
                    backend=(er.ma_batch, lik))
    assert R["best"][0] == 2 and R["sigma"] == 0.5 and R["rho"] == 0.1 and R["loglik"] == -0.5
    R = est.ar1_mle(G, np.zeros((2, 1)), np.zeros(1), (0.1, 0.9), (0.0, 0.4), width=5, rounds=3,
                    backend=(er.ma_batch, lik))
    assert list(R["best"]) == [-1] and np.isnan(R["loglik"]) and len(R["boxes"]) == 1


# ------------------------------------------------------------------------------ refusals
i64, ci = C.c_int64, C.c_int
NO_DEVICE = (5, "no HIP device visible")
LIK_FIT = ("likelihood batch: a candidate's arrays exceed one CU's LDS (lik_fits: n = L·n_o, "
           "max(n(n+1)/2, n_o·T) + n·n_o + 3n + 2 doubles within 160 KiB)")
NO_, T_, C_, L_ = 2, 5, 3, 4


def _base():
    return dict(n_o=NO_, T=T_, C=C_, L=L_, shared=1, G=np.zeros(NO_ * T_ * T_),
                dZ=np.ones(C_ * T_), m=np.ones(C_ * NO_ * T_), y=np.zeros(L_ * NO_),
                me=np.full(C_ * NO_, 0.1), ll=np.zeros(C_), st=np.zeros(C_, np.int32),
                fl=np.zeros(C_, np.int32), Gam=np.zeros(C_ * L_ * NO_ * NO_),
                d=np.zeros(C_ * L_ * NO_))


DEFECTS = {
    "valid": lambda a: None, "C0": lambda a: a.update(C=0), "T0": lambda a: a.update(T=0),
    "T32769": lambda a: a.update(T=32769), "no0": lambda a: a.update(n_o=0),
    "no65": lambda a: a.update(n_o=65), "L0": lambda a: a.update(L=0),
    "L198": lambda a: a.update(n_o=1, L=198), "L66": lambda a: a.update(n_o=3, L=66, T=300),
    "T30000": lambda a: a.update(T=30000),
    "me_neg": lambda a: a["me"].__setitem__(1, -1e-9),
    "me_nan": lambda a: a["me"].__setitem__(0, np.nan),
    "me_neg_c2": lambda a: (a.update(shared=0), a["me"].__setitem__(5, -1.0)),
    "me_neg_unread": lambda a: a["me"].__setitem__(5, -1.0),
    "null:G": lambda a: a.update(G=None), "null:dZ": lambda a: a.update(dZ=None),
    "null:m": lambda a: a.update(m=None), "null:y": lambda a: a.update(y=None),
    "null:me": lambda a: a.update(me=None), "null:ll": lambda a: a.update(ll=None),
    "null:st": lambda a: a.update(st=None), "null:fl": lambda a: a.update(fl=None),
    "null:Gam": lambda a: a.update(Gam=None), "null:d": lambda a: a.update(d=None),
}


def _p(x):
    return None if x is None else x.ctypes.data_as(C.c_void_p)


def _ma(L, a):
    return L.aiy_ssj_ma_batch(i64(a["n_o"]), i64(a["T"]), i64(a["C"]), _p(a["G"]), _p(a["dZ"]),
                              _p(a["m"]))


def _lik(L, a):
    return L.aiy_ssj_loglik_batch(i64(a["C"]), i64(a["n_o"]), i64(a["T"]), i64(a["L"]), _p(a["m"]),
                                  _p(a["y"]), _p(a["me"]), ci(a["shared"]), _p(a["ll"]),
                                  _p(a["st"]), _p(a["fl"]), _p(a["Gam"]), _p(a["d"]))


CALLERS = {"aiy_ssj_ma_batch": _ma, "aiy_ssj_loglik_batch": _lik}
NULL = (6, "NULL argument")
# (entry, defects) -> the answer; a defect pair shows which check comes first
EXPECTED = {
    ("aiy_ssj_ma_batch", "null:G"): NULL,
    ("aiy_ssj_ma_batch", "null:dZ+T0"): NULL,
    ("aiy_ssj_ma_batch", "null:m"): NULL,
    ("aiy_ssj_ma_batch", "no0"): (1, "need 1 <= n_o <= 64"),
    ("aiy_ssj_ma_batch", "no65"): (1, "need 1 <= n_o <= 64"),
    ("aiy_ssj_ma_batch", "no0+T0"): (1, "need 1 <= n_o <= 64"),
    ("aiy_ssj_ma_batch", "T0"): (1, "T must be in [1, 32768]"),
    ("aiy_ssj_ma_batch", "T32769"): (1, "T must be in [1, 32768]"),
    ("aiy_ssj_ma_batch", "T0+C0"): (1, "T must be in [1, 32768]"),
    ("aiy_ssj_ma_batch", "C0"): (1, "need 1 <= C <= 2^24"),
    ("aiy_ssj_ma_batch", "valid"): NO_DEVICE,
    ("aiy_ssj_loglik_batch", "null:m"): NULL,
    ("aiy_ssj_loglik_batch", "null:me"): NULL,
    ("aiy_ssj_loglik_batch", "null:ll+T0"): NULL,
    ("aiy_ssj_loglik_batch", "null:st"): NULL,
    ("aiy_ssj_loglik_batch", "null:fl"): NULL,
    ("aiy_ssj_loglik_batch", "null:y+null:Gam"): NULL,
    ("aiy_ssj_loglik_batch", "no65"): (1, "need 1 <= n_o <= 64"),
    ("aiy_ssj_loglik_batch", "T0"): (1, "T must be in [1, 32768]"),
    ("aiy_ssj_loglik_batch", "C0"): (1, "need 1 <= C <= 2^24"),
    ("aiy_ssj_loglik_batch", "L0"): (1, "need L >= 1"),
    ("aiy_ssj_loglik_batch", "L0+me_neg"): (1, "need L >= 1"),
    ("aiy_ssj_loglik_batch", "L198"): (6, LIK_FIT),
    ("aiy_ssj_loglik_batch", "L66"): (6, LIK_FIT),
    ("aiy_ssj_loglik_batch", "T30000"): (6, LIK_FIT),
    ("aiy_ssj_loglik_batch", "L198+me_neg"): (6, LIK_FIT),
    ("aiy_ssj_loglik_batch", "null:y+L198"): (6, LIK_FIT),
    ("aiy_ssj_loglik_batch", "me_neg"): (6, "me_var must be finite and >= 0 (entry 2)"),
    ("aiy_ssj_loglik_batch", "me_nan"): (6, "me_var must be finite and >= 0 (entry 1)"),
    ("aiy_ssj_loglik_batch", "me_neg_c2"): (6, "me_var must be finite and >= 0 (entry 6)"),
    ("aiy_ssj_loglik_batch", "me_neg_unread"): NO_DEVICE,  # (shared: entries past n_o are not read)
    ("aiy_ssj_loglik_batch", "null:y+null:me+null:ll+null:st+null:fl"): NO_DEVICE,
    ("aiy_ssj_loglik_batch", "null:Gam"): NO_DEVICE,
    ("aiy_ssj_loglik_batch", "null:d"): NO_DEVICE,
    ("aiy_ssj_loglik_batch", "valid"): NO_DEVICE,
}


def test_the_fit_rule_the_refusals_quote():
    """The packed triangle (or m while Γ is formed), Γ, w, l and z in doubles within 160 KiB:
    n_o = 1 admits L = 197, n_o = 3 with T = 300 admits L = 65 (n = 195); the benchmark's three
    observables at L = 60, T = 300 take 136 KB."""
    def fits(n_o, L, T):
        n = n_o * L
        return 8 * (max(n * (n + 1) // 2, n_o * T) + n * n_o + 3 * n + 2) <= 160 * 1024
    assert fits(1, 197, 300) and not fits(1, 198, 300)
    assert fits(3, 65, 300) and not fits(3, 66, 300)
    assert fits(3, 60, 300) and not fits(2, 4, 30000) and fits(1, 1, 1)


@pytest.mark.parametrize("entry,defects", sorted(EXPECTED))
def test_estimation_refusal(pkg, entry, defects):
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
