"""GPU parity for the labour economy's transition passes (transition_kernels.hip:
labor_egm_backward_batch_kernel and dist_forward_batch_kernel<true>), its sequence-space Jacobian
(aiy_ssj_jacobian_labor) and the lockstep drivers in κ = K/H.

Backward: pk, pl and pc at every period bit for bit against tests/support/labor_transition_ref.c
(the C oracle's labour EGM step with r split in two), and against T calls of aiy_egm_step_dev
(labor = 1) on a constant path.  Forward: λ_T bit for bit against chained
corc.dist_update_lottery; K_t and H_t bit for bit against the reference's restated sums and within
1e-12 relative of a numpy dot product.  The exogenous entries on one fixed problem: unchanged."""
import math

import numpy as np
import pytest

from oracle import corc
from tests import labor_transition_ref as lr
from tests import ssj_ref as sr
from tests import transition_ref as tr
from tests.test_transition_gpu import problem as exo_problem

pytestmark = pytest.mark.gpu


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


_PROB = {}


def problem(pkg, N, Na, T, C, sigma=None, phi=1.0, theta=1.0):
    """test_transition_gpu.problem's price paths on the labour calibration, each path with its own
    terminal policy (40 oracle labour EGM steps at its terminal prices), and the reference's
    backward pass of each."""
    key = (N, Na, T, C, sigma, phi, theta)
    if key not in _PROB:
        cb = pkg.calibration
        cal = dict(_cal(pkg, N, Na))
        if sigma is not None:
            cal["sigma"] = sigma
        a, s, P = cal["a_grid"], cal["s"], cal["P"]
        wage = lambda r: cb.wage(r, cal["alpha"], cal["delta"])
        level = np.linspace(0.012, 0.044, C) if C > 1 else np.array([0.03])
        step = np.array([0.003, -0.002, 0.004, -0.001, 0.002, -0.003, 0.001])
        r = np.stack([level[c] + np.cumsum(np.roll(step, c)[np.arange(T + 1) % 7]) * 0.5
                      for c in range(C)])
        w = wage(r[:, :T])
        pcT = np.stack([corc.labor_egm_solve(
            np.tile((1 + r[c, T]) * a + wage(r[c, T]) * np.mean(s), (N, 1)), a, s, P, r[c, T],
            wage(r[c, T]), cal["beta"], cal["sigma"], phi, theta, cal["amin"],
            max_iter=40)["policy_c"] for c in range(C)])
        ref = [lr.labor_backward(r[c], w[c], pcT[c], a, s, P, cal["beta"], cal["sigma"], phi, theta,
                                 cal["amin"]) for c in range(C)]
        _PROB[key] = dict(cal=cal, r=r, w=w, pcT=pcT, ref=ref, phi=phi, theta=theta)
    return _PROB[key]


def backward(pkg, pr, r=None, w=None, pcT=None):
    cal = pr["cal"]
    return pkg.labor_egm_backward_batch(pr["r"] if r is None else r, pr["w"] if w is None else w,
                                        pr["pcT"] if pcT is None else pcT, cal["a_grid"], cal["s"],
                                        cal["P"], cal["beta"], cal["sigma"], pr["phi"], pr["theta"],
                                        cal["amin"])


SHAPES = [(3, 37, 5, 3),      # one pass; more threads than states
          (7, 400, 6, 2),     # the scripts' grid: three passes of 1,024 threads
          (16, 64, 3, 2),     # N at the cap
          (2, 1024, 2, 1)]    # Na at the fused cap
CASES = [s + (None, 1.0, 1.0) for s in SHAPES] + [
    (3, 37, 5, 3, 1.5, 0.8, 2.0),   # fractional sigma, theta != 1: the pow branches
    (7, 400, 6, 2, 2.0, 1.3, 0.5)]


@pytest.mark.parametrize("N,Na,T,C,sigma,phi,theta", CASES)
def test_backward_is_the_reference_bit_for_bit(gpu, pkg, N, Na, T, C, sigma, phi, theta):
    pr = problem(pkg, N, Na, T, C, sigma, phi, theta)
    # the reference shows the zero clamp of policy_k binding, and hours that differ across states
    assert all(ref["status"] == 0 for ref in pr["ref"])
    assert any((ref["pk"] == 0.0).any() for ref in pr["ref"])
    assert all(np.isfinite(ref["pk"]).all() and np.isfinite(ref["pl"]).all() for ref in pr["ref"])
    G = backward(pkg, pr)
    assert (G["status"] == 0).all() and (G["fail_t"] == -1).all()
    for c in range(C):
        for t in range(T):
            assert same(G["policy_k"][c, t], pr["ref"][c]["pk"][t]), (c, t, "pk")
            assert same(G["policy_l"][c, t], pr["ref"][c]["pl"][t]), (c, t, "pl")
            assert same(G["policy_c"][c, t], pr["ref"][c]["pc"][t]), (c, t, "pc")
    # policy_c is optional; the others do not depend on it
    cal = pr["cal"]
    S = pkg.labor_egm_backward_batch(pr["r"], pr["w"], pr["pcT"], cal["a_grid"], cal["s"], cal["P"],
                                     cal["beta"], cal["sigma"], phi, theta, cal["amin"],
                                     want_pc=False)
    assert S["policy_c"] is None and same(S["policy_k"], G["policy_k"])
    assert same(S["policy_l"], G["policy_l"])


def test_constant_path_equals_chained_labor_egm_step_dev(gpu, pkg):
    """r_next == r_now: the device tier's backward pass equals T calls of aiy_egm_step_dev with
    labor = 1, at two rates."""
    import torch
    N, Na, T = 7, 400, 4
    cb = pkg.calibration
    cal = _cal(pkg, N, Na)
    dev = lambda x: torch.as_tensor(np.ascontiguousarray(x), device=gpu)
    a, s, P = dev(cal["a_grid"]), dev(cal["s"]), dev(cal["P"])
    rates = [0.01, 0.035]
    wages = [cb.wage(r, cal["alpha"], cal["delta"]) for r in rates]
    pcT = np.stack([np.tile((1 + r) * cal["a_grid"] + w * np.mean(cal["s"]), (N, 1))
                    for r, w in zip(rates, wages)])
    ws = pkg.Workspace(N, Na)
    pk, pl, pc = (torch.full((2, T, N, Na), -7.0, dtype=torch.float64, device=gpu)
                  for _ in range(3))
    st, ft = pkg.labor_egm_backward_batch_dev(
        ws, np.repeat(np.array(rates)[:, None], T + 1, 1), np.repeat(np.array(wages)[:, None], T, 1),
        dev(pcT), a, s, P, cal["beta"], cal["sigma"], 1.0, 1.0, cal["amin"], pk, pl, pc)
    assert (st == 0).all() and (ft == -1).all()
    for c in range(2):
        cur = dev(pcT[c])
        for t in range(T - 1, -1, -1):
            nxt, k1, l1 = torch.empty_like(cur), torch.empty_like(cur), torch.empty_like(cur)
            pkg.egm_step_dev(ws, cur, a, s, P, rates[c], wages[c], cal["beta"], cal["sigma"],
                             cal["amin"], nxt, k1, labor=True, phi=1.0, theta=1.0, policy_l=l1)
            torch.cuda.synchronize()
            assert torch.equal(nxt, pc[c, t]) and torch.equal(k1, pk[c, t]), (c, t)
            assert torch.equal(l1, pl[c, t]), (c, t)
            cur = nxt
    ws.close()


def test_a_nan_in_one_terminal_policy_stops_that_path_alone(gpu, pkg):
    N, Na, T, C = 7, 400, 6, 2
    pr = problem(pkg, N, Na, T, C)
    cal = pr["cal"]
    pcT = pr["pcT"].copy()
    pcT[0, 3, 217] = np.nan
    ref_bad = lr.labor_backward(pr["r"][0], pr["w"][0], pcT[0], cal["a_grid"], cal["s"], cal["P"],
                                cal["beta"], cal["sigma"], 1.0, 1.0, cal["amin"])
    assert (ref_bad["status"], ref_bad["fail_t"]) == (1, T - 1)
    G = backward(pkg, pr, pcT=pcT)
    assert G["status"][0] == 1 and G["fail_t"][0] == T - 1
    S = backward(pkg, pr, pr["r"][1:], pr["w"][1:], pr["pcT"][1:])
    assert G["status"][1] == 0 and G["fail_t"][1] == -1 and S["status"][0] == 0
    for k in ("policy_k", "policy_l", "policy_c"):
        assert same(G[k][1], S[k][0]), k
    assert same(G["policy_k"][1], pr["ref"][1]["pk"])
    # through both passes: K and H of the stopped path are NaN, the other path is its solo run
    lam0 = _lam0(C, N, Na, 5)
    args = (cal["a_grid"], cal["s"], cal["P"], cal["beta"], cal["sigma"], 1.0, 1.0, cal["amin"])
    K, H, st, ft = pkg.labor_transition_batch(pr["r"], pr["w"], pcT, lam0, *args)
    K1, H1, st1, _ = pkg.labor_transition_batch(pr["r"][1:], pr["w"][1:], pcT[1:], lam0[1:], *args)
    assert list(st) == [1, 0] and ft[0] == T - 1 and st1[0] == 0
    assert np.isnan(K[0]).all() and np.isnan(H[0]).all()
    assert same(K[1], K1[0]) and same(H[1], H1[0])


def _lam0(C, N, Na, seed):
    lam = np.random.default_rng(seed).random((C, N, Na))
    return lam / lam.sum((1, 2), keepdims=True)


def _tiny():
    """N = 1, Na = 2 — the smallest shape the fit rule admits (n = 2: the mass array's spare half
    holds one double, the hours' block sum sits in the unused key slot): hand-made inputs."""
    rng = np.random.default_rng(12)
    T, C = 3, 2
    cal = dict(a_grid=np.array([0.0, 1.5]), s=np.array([1.3]), P=np.array([[1.0]]), N=1, Na=2)
    pk = np.sort(rng.random((C, T, 1, 2)) * 1.5, axis=-1)
    pk[1, 1] = [[-0.2, 1.7]]  # both ends clamped
    return cal, pk, 0.2 + rng.random((C, T, 1, 2)), T, C


@pytest.mark.parametrize("N,Na,T,C", SHAPES[:2] + [(1, 2, 3, 2)])
def test_forward_is_the_chained_oracle_push_with_hours(gpu, pkg, N, Na, T, C):
    """Input: the reference's backward pass, with one period's row 0 sent to a single node — a
    run of Na > 32 sources, dist_mass's chunked path."""
    if N == 1:
        cal, pk, pl, T, C = _tiny()
    else:
        pr = problem(pkg, N, Na, T, C)
        cal = pr["cal"]
        pk = np.stack([pr["ref"][c]["pk"] for c in range(C)])
        pl = np.stack([pr["ref"][c]["pl"] for c in range(C)])
        pk[C - 1, 1, 0, :] = cal["a_grid"][5]
        assert Na > 32 and (tr.lottery_keys(pk[C - 1, 1], cal["a_grid"])[0] == 5).all()
    a, s, P = cal["a_grid"], cal["s"], cal["P"]
    lam0 = _lam0(C, N, Na, 7)
    G = pkg.labor_dist_forward_batch(pk, pl, lam0, a, s, P)
    assert (G["status"] == 0).all() and (G["fail_t"] == -1).all()
    assert G["K"].shape == (C, T + 1) and G["H"].shape == (C, T)
    for c in range(C):
        R = lr.labor_forward(pk[c], pl[c], lam0[c], a, s, P)
        assert R["status"] == 0
        assert same(G["lam_T"][c], R["lam"][T])
        assert same(G["K"][c], R["K"]) and same(G["H"][c], R["H"])
        dK = np.array([float(np.sum(R["lam"][t] * a[None, :])) for t in range(T + 1)])
        dH = np.array([float(np.sum(R["lam"][t] * (s[:, None] * pl[c, t]))) for t in range(T)])
        assert np.all(np.abs(G["K"][c] - dK) <= 1e-12 * np.abs(dK))
        assert np.all(np.abs(G["H"][c] - dH) <= 1e-12 * np.abs(dH))
    # K, λ_T and the statuses are the exogenous pass's on the same policy_k, bit for bit
    X = pkg.dist_forward_batch(pk, lam0, a, P)
    assert same(X["K"], G["K"]) and same(X["lam_T"], G["lam_T"])
    # one shared λ₀ for every path is path 0's start everywhere
    S = pkg.labor_dist_forward_batch(pk, pl, lam0[0], a, s, P)
    assert same(S["K"][0], G["K"][0]) and same(S["H"][0], G["H"][0])
    assert same(S["lam_T"][0], G["lam_T"][0])


def test_a_nonmonotone_period_policy_stops_the_forward_path_alone(gpu, pkg):
    N, Na, T, C = 3, 37, 5, 3
    pr = problem(pkg, N, Na, T, C)
    cal = pr["cal"]
    a, s, P = cal["a_grid"], cal["s"], cal["P"]
    pk = np.stack([pr["ref"][c]["pk"] for c in range(C)])
    pl = np.stack([pr["ref"][c]["pl"] for c in range(C)])
    lam0 = _lam0(C, N, Na, 3)
    good = pkg.labor_dist_forward_batch(pk, pl, lam0, a, s, P)
    assert (good["status"] == 0).all()
    # the clamp at 0 leaves row 0 flat at its low end: reverse a row that does rise
    assert pk[1, 2, 2, 0] < pk[1, 2, 2, -1]
    pk[1, 2, 2, :] = pk[1, 2, 2, ::-1]
    R = lr.labor_forward(pk[1], pl[1], lam0[1], a, s, P)
    assert (R["status"], R["fail_t"]) == (2, 2)
    G = pkg.labor_dist_forward_batch(pk, pl, lam0, a, s, P)
    assert list(G["status"]) == [0, 2, 0] and list(G["fail_t"]) == [-1, 2, -1]
    assert same(G["K"][1, :3], R["K"][:3]) and np.isnan(G["K"][1, 3:]).all()
    assert same(G["H"][1, :3], R["H"][:3]) and np.isnan(G["H"][1, 3:]).all()
    assert same(G["lam_T"][1], R["lam"][2])
    for c in (0, 2):
        assert same(G["K"][c], good["K"][c]) and same(G["H"][c], good["H"][c])
        assert same(G["lam_T"][c], good["lam_T"][c])


def test_labor_transition_batch_is_order_independent(gpu, pkg):
    """C = 5 in one call equals five C = 1 calls, a permutation of the paths permutes the
    outputs, and every path is the reference's transition."""
    N, Na, T, C = 3, 37, 5, 5
    pr = problem(pkg, N, Na, T, C)
    cal = pr["cal"]
    lam0 = _lam0(C, N, Na, 11)
    args = (cal["a_grid"], cal["s"], cal["P"], cal["beta"], cal["sigma"], 1.0, 1.0, cal["amin"])
    K, H, st, ft = pkg.labor_transition_batch(pr["r"], pr["w"], pr["pcT"], lam0, *args)
    assert (st == 0).all() and (ft == -1).all()
    for c in range(C):
        K1, H1, st1, _ = pkg.labor_transition_batch(pr["r"][c:c + 1], pr["w"][c:c + 1],
                                                    pr["pcT"][c:c + 1], lam0[c:c + 1], *args)
        assert st1[0] == 0 and same(K1[0], K[c]) and same(H1[0], H[c]), c
        R = lr.labor_transition(pr["r"][c], pr["w"][c], pr["pcT"][c], lam0[c], *args)
        assert R["status"] == 0 and same(R["K"], K[c]) and same(R["H"], H[c]), c
    perm = np.array([3, 0, 4, 2, 1])
    Kp, Hp, stp, _ = pkg.labor_transition_batch(pr["r"][perm], pr["w"][perm], pr["pcT"][perm],
                                                lam0[perm], *args)
    assert same(Kp, K[perm]) and same(Hp, H[perm]) and (stp == 0).all()


def test_the_exogenous_entries_did_not_move(gpu, pkg):
    """egm_backward_batch, dist_forward_batch and jacobian on one fixed problem against their
    existing CPU references, bit for bit (F and J of jacobian: against the public contraction of
    the same E and Λ1, as test_ssj_gpu.py states it)."""
    N, Na, T, C = 3, 37, 5, 3
    pr = exo_problem(pkg, N, Na, T, C)
    cal = pr["cal"]
    a, s, P = cal["a_grid"], cal["s"], cal["P"]
    G = pkg.egm_backward_batch(pr["r"], pr["w"], pr["pcT"], a, s, P, cal["beta"], cal["sigma"],
                               cal["amin"])
    assert (G["status"] == 0).all()
    lam0 = _lam0(C, N, Na, 7)
    F = pkg.dist_forward_batch(G["policy_k"], lam0, a, P)
    assert (F["status"] == 0).all()
    for c in range(C):
        assert same(G["policy_k"][c], pr["ref"][c]["pk"]) and same(G["policy_c"][c], pr["ref"][c]["pc"])
        R = tr.dist_forward(G["policy_k"][c], lam0[c], a, P)
        assert same(F["K"][c], R["K"]) and same(F["lam_T"][c], R["lam"][T])
    cb = pkg.calibration
    cal60 = cb.aiyagari(Na=60, shocks="rouwenhorst", N=3)
    ss = tr.steady_state_cpu(cal60, 0.03, lambda r: cb.wage(r, cal60["alpha"], cal60["delta"]))
    Tj, h = 8, 1e-4
    J = pkg.jacobian(ss, Tj, h)
    R = sr.jacobian_cpu(ss, Tj, h)
    assert J["status"] == (0, 0) and same(J["E"], R["E"])
    Fn, Jn = pkg.fake_news(R["E"], R["lam1"], h)
    assert same(Fn[0], J["F_r"]) and same(Fn[1], J["F_w"])
    assert same(Jn[0], J["J_r"]) and same(Jn[1], J["J_w"])


# ------------------------------------------------------------- the Jacobian and the drivers
_SS = {}


def _ss(pkg, N, Na):
    """steady_state_labor_cpu on the labour calibration, phi = theta = 1 (shared by the tests)."""
    if (N, Na) not in _SS:
        cb = pkg.calibration
        cal = _cal(pkg, N, Na)
        _SS[N, Na] = lr.steady_state_labor_cpu(cal, 1.0, 1.0,
                                               lambda r: cb.wage(r, cal["alpha"], cal["delta"]))
    return _SS[N, Na]


def _exact(E, D):
    """(math.fsum of the rounded products E[t]·D[x][s], Σ|products|), each [n_in][T][T]."""
    T = E.shape[0]
    Er = E.reshape(T, -1)
    F, A = np.empty((D.shape[0], T, T)), np.empty((D.shape[0], T, T))
    for x in range(D.shape[0]):
        for t in range(T):
            for q in range(T):
                p = Er[t] * D[x, q]
                F[x, t, q] = math.fsum(p)
                A[x, t, q] = float(np.sum(np.abs(p)))
    return F, A


def _diag_sum(F):
    """Σ of F down each diagonal up to (t, s), in exact arithmetic order-free form (fsum)."""
    J = np.empty_like(F)
    T = F.shape[-1]
    for x in range(F.shape[0]):
        for t in range(T):
            for q in range(T):
                J[x, t, q] = math.fsum(F[x, t - m, q - m] for m in range(min(t, q) + 1))
    return J


@pytest.mark.parametrize("N,Na,T", [(3, 37, 8), (7, 100, 20)])
def test_jacobian_labor_is_the_cpu_jacobian(gpu, pkg, N, Na, T):
    """E^a, E^h, pk, pl, Λ1 and H1 bit for bit against jacobian_labor_cpu; the four F and J bit for
    bit against the same quantities composed from the public per-stage entries; every entry of F
    within n·2⁻⁵²·Σ|terms| of the exact sums of those same E and Λ1 (the first row of F_H, one
    subtraction and one division of H1's bits, exactly), and J within the bound summed along its
    diagonal."""
    ss = _ss(pkg, N, Na)
    cal, h = ss["cal"], 1e-4
    a, s, P = cal["a_grid"], cal["s"], cal["P"]
    n = N * Na
    R = lr.jacobian_labor_cpu(ss, T, h)
    G = pkg.jacobian_labor(ss, T, h)
    assert G["status"] == (0, 0)
    assert same(G["E_a"], R["E_a"]) and same(G["E_h"], R["E_h"])
    # steps 1 and 2 through the public entries that jacobian_labor() chains
    r, w = sr.news_paths(ss, T, h)
    B = pkg.labor_egm_backward_batch(r, w, ss["policy_c"], a, s, P, cal["beta"], cal["sigma"],
                                     ss["phi"], ss["theta"], cal["amin"], want_pc=False)
    assert (B["status"] == 0).all()
    assert same(B["policy_k"], R["pk"]) and same(B["policy_l"], R["pl"])
    Fw = pkg.labor_dist_forward_batch(B["policy_k"].reshape(3 * T, 1, N, Na),
                                      B["policy_l"].reshape(3 * T, 1, N, Na), ss["lam"], a, s, P)
    assert (Fw["status"] == 0).all()
    lam1, H1 = Fw["lam_T"].reshape(3, T, N, Na), Fw["H"].reshape(3, T)
    assert same(lam1, R["lam1"]) and same(H1, R["H1"])
    # steps 3-5 composed from the public entries are jacobian_labor()'s own bits
    E_a = pkg.expectation_batch(B["policy_k"][0, 0], np.tile(a, (N, 1)), a, P, T)[0]
    E_h = pkg.expectation_batch(B["policy_k"][0, 0], s[:, None] * B["policy_l"][0, 0], a, P, T)[0]
    assert same(E_a, G["E_a"]) and same(E_h, G["E_h"])
    FK, JK = pkg.fake_news(E_a, lam1, h)
    Gh, _ = pkg.fake_news(E_h, lam1, h)
    FH = lr.hours_F(Gh, H1, h)
    JH = sr.jacobian_from_F(FH)
    for x, q in (("r", 0), ("w", 1)):
        assert same(FK[q], G["F_K" + x]) and same(JK[q], G["J_K" + x]), x
        assert same(FH[q], G["F_H" + x]) and same(JH[q], G["J_H" + x]), x
    # against the exact sums
    D = sr.news_rows(R["lam1"], h)
    FKx, AK = _exact(R["E_a"], D)
    Ghx, AG = _exact(R["E_h"], D)
    FHx, AH = lr.hours_F(Ghx, R["H1"], h), lr.hours_F(AG, np.zeros((3, T)), h)
    assert same(FH[:, 0], FHx[:, 0])  # the first row is H1's bits, subtracted and divided
    AH[:, 0] = np.abs(FHx[:, 0])      # (it enters the diagonals' sums)
    u = n * 2.0 ** -52
    assert (np.abs(FK - FKx) <= u * AK).all() and (np.abs(FH - FHx) <= u * AH).all()
    assert (np.abs(JK - _diag_sum(FKx)) <= u * _diag_sum(AK)).all()
    assert (np.abs(JH - _diag_sum(FHx)) <= u * _diag_sum(AH)).all()
    # and the CPU restatement itself sits inside the same bounds
    assert (np.abs(np.stack([R["F_Kr"], R["F_Kw"]]) - FKx) <= u * AK).all()
    assert (np.abs(np.stack([R["F_Hr"], R["F_Hw"]]) - FHx) <= u * AH).all()


def test_labor_drivers_on_the_gpu_equal_the_cpu_backend_drivers(gpu, pkg):
    """N = 7, Na = 100, T = 40, three shocks of which one is Z ≡ 1, tol = 1e-8.  The Jacobians
    differ in their last bits, the fixed point does not: the same rounds and statuses, K and H
    within 1e-10.  The zero shock takes exactly 1 round; the Newton driver takes strictly fewer
    rounds than the damped driver at its default on the other two, and both land within 1e-7 of
    each other.  On the CPU backend the rounds are 5, 1, 4 (Newton) and 278, 1, 262 (damped,
    damp = 0.05)."""
    ss = _ss(pkg, 7, 100)
    T = 40
    q = np.arange(T)
    Z = np.stack([1 + 0.01 * 0.9 ** q, np.ones(T), 1 - 0.005 * 0.8 ** q])
    A = pkg.aiyagari_labor_transition_newton(ss, Z, T, tol=1e-8)
    B = pkg.aiyagari_labor_transition_newton(ss, Z, T, jac=lr.jacobian_labor_cpu(ss, T, 1e-4),
                                             tol=1e-8, backend=lr.labor_transition_batch)
    print("rounds", A["rounds"], B["rounds"], "max |K_gpu - K_cpu|", np.max(np.abs(A["K"] - B["K"])),
          "max |H_gpu - H_cpu|", np.max(np.abs(A["H"] - B["H"])))
    assert (B["status"] == 0).all() and B["rounds"][1] == 1 and (B["rounds"] <= 6).all()
    assert np.array_equal(A["rounds"], B["rounds"]) and np.array_equal(A["status"], B["status"])
    assert np.max(np.abs(A["K"] - B["K"])) <= 1e-10 and np.max(np.abs(A["H"] - B["H"])) <= 1e-10
    D = pkg.aiyagari_labor_transition(ss, Z, T, tol=1e-8)
    print("damped rounds", D["rounds"])
    assert (D["status"] == 0).all() and D["rounds"][1] == 1
    assert (D["rounds"][[0, 2]] > A["rounds"][[0, 2]]).all()
    assert np.max(np.abs(A["K"] - D["K"])) <= 1e-7 and np.max(np.abs(A["H"] - D["H"])) <= 1e-7
    dK, dH = pkg.impulse_response_labor(ss, pkg.jacobian_labor(ss, T), Z - 1)
    assert dK.shape == (3, T + 1) and dH.shape == (3, T) and not dK[1].any() and not dH[1].any()


def test_steady_state_labor_is_a_stationary_point(gpu, pkg):
    """One labour EGM step and one push of λ (under the solve's own policy_k) from
    steady_state_labor's point move nothing beyond the solves' tolerances — tol on policy_c (the
    policy's last move was below tol and the step contracts), ge_batch.HIST_TOL on λ — and
    |K − H·k_d(r)| is within the bisection's k_tol."""
    cb = pkg.calibration
    cal = _cal(pkg, 3, 60)
    tol, k_tol = 1e-11, 1e-8
    ss = pkg.steady_state_labor(cal, 1.0, 1.0, tol=tol, k_tol=k_tol)
    a, s, P = cal["a_grid"], cal["s"], cal["P"]
    assert set(ss) >= {"r", "w", "K", "H", "policy_c", "policy_l", "lam", "cal", "phi", "theta"}
    assert 0 < ss["r"] < 1 / cal["beta"] - 1 and ss["w"] == cb.wage(ss["r"], cal["alpha"], cal["delta"])
    kd = (cal["alpha"] / (ss["r"] + cal["delta"])) ** (1 / (1 - cal["alpha"]))
    print("excess", ss["K"] - ss["H"] * kd)
    assert abs(ss["K"] - ss["H"] * kd) <= k_tol
    assert ss["policy_c"].shape == (3, 60) and abs(ss["lam"].sum() - 1) < 1e-10
    pc1, pk1, pl1, _ = corc.labor_egm_step(ss["policy_c"], a, s, P, ss["r"], ss["w"], cal["beta"],
                                           cal["sigma"], 1.0, 1.0, cal["amin"])
    assert np.max(np.abs(pc1 - ss["policy_c"])) <= tol
    lam1 = corc.dist_update_lottery(ss["lam"], ss["policy_k"], a, P)
    assert np.max(np.abs(lam1 - ss["lam"])) <= pkg.ge_batch.HIST_TOL
    assert abs(lr.hours_sum(ss["lam"], ss["policy_l"], s) - ss["H"]) <= 1e-12 * ss["H"]
    # a transition without a shock from it stays put: one round
    R = pkg.aiyagari_labor_transition_newton(ss, np.ones((1, 8)), 8, tol=1e-6)
    assert R["status"][0] == 0 and R["rounds"][0] == 1 and R["resid"][0] < 1e-6
    assert (R["r"] == ss["r"]).all() and (R["w"] == ss["w"]).all()
