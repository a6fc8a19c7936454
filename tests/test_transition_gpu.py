"""GPU parity for the transition passes (transition_kernels.hip: one workgroup per price path, T
dependent steps with no launch between them) and the lockstep driver built on them.

Backward: pk and pc at every period bit for bit against tests/support/transition_ref.c (the C
oracle's EGM step with r split into r_next and r_now), and against T calls of aiy_egm_step_dev on a
constant path.  Forward: λ_T bit for bit against chained corc.dist_update_lottery; K_t bit for bit
against the existing capital sum (aiy_dist_stationary_dev's k_supply after the one push from λ_t)
and within 1e-12 relative of a numpy dot product, as test_dist_batch_gpu.py compares K."""
import numpy as np
import pytest

from oracle import corc
from tests import transition_ref as tr

pytestmark = pytest.mark.gpu


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.int64)


def same(x, y):
    return np.array_equal(bits(x), bits(y))


def _cal(pkg, N, Na):
    cb = pkg.calibration
    return cb.aiyagari(Na=Na) if N == 7 else cb.aiyagari(Na=Na, shocks="rouwenhorst", N=N)


_PROB = {}


def problem(pkg, N, Na, T, C, sigma=None):
    """C price paths that differ per path — r moves by a few 1e-3 per period from a path-specific
    level (the last one above 1/β − 1), w follows cb.wage — each with its own terminal policy (40
    oracle EGM steps at its terminal prices), and the reference's backward pass of each."""
    key = (N, Na, T, C, sigma)
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
        pcT = np.stack([corc.egm_solve(np.tile((1 + r[c, T]) * a + wage(r[c, T]) * np.mean(s), (N, 1)),
                                       a, s, P, r[c, T], wage(r[c, T]), cal["beta"], cal["sigma"],
                                       cal["amin"], max_iter=40)["policy_c"] for c in range(C)])
        ref = [tr.egm_backward(r[c], w[c], pcT[c], a, s, P, cal["beta"], cal["sigma"], cal["amin"])
               for c in range(C)]
        _PROB[key] = dict(cal=cal, r=r, w=w, pcT=pcT, ref=ref)
    return _PROB[key]


def backward(pkg, pr, r=None, w=None, pcT=None):
    cal = pr["cal"]
    return pkg.egm_backward_batch(pr["r"] if r is None else r, pr["w"] if w is None else w,
                                  pr["pcT"] if pcT is None else pcT, cal["a_grid"], cal["s"],
                                  cal["P"], cal["beta"], cal["sigma"], cal["amin"])


SHAPES = [(3, 37, 5, 3),      # one pass; more threads than states
          (7, 400, 6, 2),     # the scripts' grid: three passes of 1,024 threads
          (16, 64, 3, 2),     # N at the cap
          (2, 1024, 2, 1)]    # Na at the fused cap


@pytest.mark.parametrize("N,Na,T,C", SHAPES)
def test_backward_is_the_reference_bit_for_bit(gpu, pkg, N, Na, T, C):
    pr = problem(pkg, N, Na, T, C)
    cal = pr["cal"]
    a, s, P = cal["a_grid"], cal["s"], cal["P"]
    if (N, Na) in ((3, 37), (7, 400)):
        # the reference shows the borrowing clamp binding on the lowest nodes (â_j(0) above the
        # first node: interp1 extrapolates below amin) and extrapolation above a_grid[-1]
        clamp = extrap = False
        for c in range(C):
            for t in range(T):
                nxt = pr["ref"][c]["pc"][t + 1] if t + 1 < T else pr["pcT"][c]
                _, pk, ah, _ = tr.egm_step2(nxt, a, s, P, pr["r"][c, t + 1], pr["r"][c, t],
                                            pr["w"][c, t], cal["beta"], cal["sigma"], cal["amin"])
                clamp |= bool((ah[:, 0] > a[0]).any() and (pk[:, :2] == cal["amin"]).any())
                extrap |= bool((ah[:, -1] < a[-1]).any() and (pk[:, -1] > a[-1]).any())
        assert clamp and extrap
    G = backward(pkg, pr)
    assert (G["status"] == 0).all() and (G["fail_t"] == -1).all()
    for c in range(C):
        assert pr["ref"][c]["status"] == 0
        for t in range(T):
            assert same(G["policy_k"][c, t], pr["ref"][c]["pk"][t]), (c, t, "pk")
            assert same(G["policy_c"][c, t], pr["ref"][c]["pc"][t]), (c, t, "pc")


def test_constant_path_equals_chained_egm_step_dev(gpu, pkg):
    """r_next == r_now: the device tier's backward pass equals T calls of aiy_egm_step_dev."""
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
    pk = torch.full((2, T, N, Na), -7.0, dtype=torch.float64, device=gpu)
    pc = torch.full((2, T, N, Na), -7.0, dtype=torch.float64, device=gpu)
    st, ft = pkg.transition.egm_backward_batch_dev(
        ws, np.repeat(np.array(rates)[:, None], T + 1, 1), np.repeat(np.array(wages)[:, None], T, 1),
        dev(pcT), a, s, P, cal["beta"], cal["sigma"], cal["amin"], pk, pc)
    assert (st == 0).all() and (ft == -1).all()
    for c in range(2):
        cur = dev(pcT[c])
        for t in range(T - 1, -1, -1):
            nxt, k1 = torch.empty_like(cur), torch.empty_like(cur)
            pkg.egm_step_dev(ws, cur, a, s, P, rates[c], wages[c], cal["beta"], cal["sigma"],
                             cal["amin"], nxt, k1)
            torch.cuda.synchronize()
            assert torch.equal(nxt, pc[c, t]) and torch.equal(k1, pk[c, t]), (c, t)
            cur = nxt
    ws.close()


def _solo(pkg, pr, c, r=None, w=None, pcT=None):
    pick = lambda x, d: (pr[d] if x is None else x)[c:c + 1]
    return backward(pkg, pr, pick(r, "r"), pick(w, "w"), pick(pcT, "pcT"))


def _check_contained(pkg, pr, G, bad, ref_bad, r=None, w=None, pcT=None):
    """Path `bad` reports the reference's stop and matches it above fail_t; every other path is
    its solo run (and the reference) bit for bit."""
    C, T = pr["r"].shape[0], pr["w"].shape[1]
    ft = ref_bad["fail_t"]
    assert ref_bad["status"] == 1
    assert G["status"][bad] == 1 and G["fail_t"][bad] == ft
    for t in range(ft + 1, T):
        assert same(G["policy_k"][bad, t], ref_bad["pk"][t]), t
        assert same(G["policy_c"][bad, t], ref_bad["pc"][t]), t
    for c in range(C):
        if c == bad:
            continue
        S = _solo(pkg, pr, c, r, w, pcT)
        assert G["status"][c] == 0 and G["fail_t"][c] == -1 and S["status"][0] == 0
        assert same(G["policy_k"][c], S["policy_k"][0]) and same(G["policy_c"][c], S["policy_c"][0])
        assert same(G["policy_k"][c], np.stack(pr["ref"][c]["pk"]))


def test_a_nonmonotone_path_stops_alone(gpu, pkg, golden):
    """Path 1 of 3 is tests/golden/transition_nonmonotone.npz (sigma = 2; a negative wage in
    period 3 makes period 2's endogenous grid finite and decreasing in places)."""
    F = golden("transition_nonmonotone")
    N, Na, T, sigma = int(F["N"]), int(F["Na"]), len(F["w"]), float(F["sigma"])
    pr = problem(pkg, N, Na, T, 3, sigma=sigma)
    cal = pr["cal"]
    r, w, pcT = pr["r"].copy(), pr["w"].copy(), pr["pcT"].copy()
    r[1], w[1], pcT[1] = F["r"], F["w"], F["pc_T"]
    ref_bad = tr.egm_backward(r[1], w[1], pcT[1], cal["a_grid"], cal["s"], cal["P"], cal["beta"],
                              sigma, cal["amin"])
    assert ref_bad["fail_t"] == int(F["fail_t"]) and 0 < ref_bad["fail_t"] < T - 1
    G = backward(pkg, pr, r, w, pcT)
    _check_contained(pkg, pr, G, 1, ref_bad, r, w, pcT)


def test_a_nan_in_one_terminal_policy_stops_that_path_alone(gpu, pkg):
    N, Na, T, C = 7, 400, 6, 2
    pr = problem(pkg, N, Na, T, C)
    cal = pr["cal"]
    pcT = pr["pcT"].copy()
    pcT[0, 3, 217] = np.nan
    ref_bad = tr.egm_backward(pr["r"][0], pr["w"][0], pcT[0], cal["a_grid"], cal["s"], cal["P"],
                              cal["beta"], cal["sigma"], cal["amin"])
    assert ref_bad["fail_t"] == T - 1
    G = backward(pkg, pr, pcT=pcT)
    _check_contained(pkg, pr, G, 0, ref_bad, pcT=pcT)


def _lam0(C, N, Na, seed):
    lam = np.random.default_rng(seed).random((C, N, Na))
    return lam / lam.sum((1, 2), keepdims=True)


@pytest.mark.parametrize("N,Na,T,C", SHAPES[:2])
def test_forward_is_the_chained_oracle_push(gpu, pkg, N, Na, T, C):
    """Input: the backward pass's output, with one period's row 0 sent to a single node — a run
    of Na > 32 sources, dist_mass's chunked path."""
    import torch
    pr = problem(pkg, N, Na, T, C)
    cal = pr["cal"]
    a, P = cal["a_grid"], cal["P"]
    pk = backward(pkg, pr)["policy_k"]
    pk[C - 1, 1, 0, :] = a[5]
    assert Na > 32 and (tr.lottery_keys(pk[C - 1, 1], a)[0] == 5).all()
    lam0 = _lam0(C, N, Na, 7)
    G = pkg.dist_forward_batch(pk, lam0, a, P)
    assert (G["status"] == 0).all() and (G["fail_t"] == -1).all()
    ws = pkg.Workspace(N, Na)
    dev = lambda x: torch.as_tensor(np.ascontiguousarray(x), device=gpu)
    da, dP = dev(a), dev(P)
    for c in range(C):
        R = tr.dist_forward(pk[c], lam0[c], a, P)
        assert R["status"] == 0
        assert same(G["lam_T"][c], R["lam"][T])
        assert same(G["K"][c], R["K"])  # the reference's restatement of the device's order
        dots = np.array([float(np.sum(R["lam"][t] * a[None, :])) for t in range(T + 1)])
        assert np.all(np.abs(G["K"][c] - dots) <= 1e-12 * np.abs(dots))
        for t in range(T):  # K[t+1]: the existing capital sum after the one push from λ_t
            out, K1 = torch.empty((N, Na), dtype=torch.float64, device=gpu), dev(np.zeros(1))
            pkg.dist_stationary_dev(ws, dev(R["lam"][t]), da, dP, out, policy_k=dev(pk[c, t]),
                                    tol=0.0, max_iter=1, k_supply=K1)
            assert same(out.cpu().numpy(), R["lam"][t + 1])
            assert same(K1.cpu().numpy()[0], G["K"][c, t + 1]), (c, t)
    ws.close()
    # one shared λ₀ for every path is path 0's start everywhere
    S = pkg.dist_forward_batch(pk, lam0[0], a, P)
    assert same(S["K"][0], G["K"][0]) and same(S["lam_T"][0], G["lam_T"][0])


def test_a_nonmonotone_period_policy_stops_the_forward_path_alone(gpu, pkg):
    N, Na, T, C = 3, 37, 5, 3
    pr = problem(pkg, N, Na, T, C)
    cal = pr["cal"]
    a, P = cal["a_grid"], cal["P"]
    pk = np.stack([np.stack(pr["ref"][c]["pk"]) for c in range(C)])
    good = pkg.dist_forward_batch(pk, _lam0(C, N, Na, 3), a, P)
    pk[1, 2, 0, :] = pk[1, 2, 0, ::-1]
    R = tr.dist_forward(pk[1], _lam0(C, N, Na, 3)[1], a, P)
    assert (R["status"], R["fail_t"]) == (2, 2)
    G = pkg.dist_forward_batch(pk, _lam0(C, N, Na, 3), a, P)
    assert list(G["status"]) == [0, 2, 0] and list(G["fail_t"]) == [-1, 2, -1]
    assert same(G["K"][1, :3], R["K"][:3]) and np.isnan(G["K"][1, 3:]).all()
    assert same(G["lam_T"][1], R["lam"][2])
    for c in (0, 2):
        assert same(G["K"][c], good["K"][c]) and same(G["lam_T"][c], good["lam_T"][c])


def test_transition_batch_is_order_independent(gpu, pkg):
    """C = 5 in one call equals five C = 1 calls, a permutation of the paths permutes the
    outputs, and every path is the reference's transition."""
    N, Na, T, C = 3, 37, 5, 5
    pr = problem(pkg, N, Na, T, C)
    cal = pr["cal"]
    lam0 = _lam0(C, N, Na, 11)
    args = (cal["a_grid"], cal["s"], cal["P"], cal["beta"], cal["sigma"], cal["amin"])
    K, st, ft = pkg.transition_batch(pr["r"], pr["w"], pr["pcT"], lam0, *args)
    assert (st == 0).all() and (ft == -1).all()
    for c in range(C):
        K1, st1, _ = pkg.transition_batch(pr["r"][c:c + 1], pr["w"][c:c + 1], pr["pcT"][c:c + 1],
                                          lam0[c:c + 1], *args)
        assert st1[0] == 0 and same(K1[0], K[c]), c
        R = tr.transition(pr["r"][c], pr["w"][c], pr["pcT"][c], lam0[c], *args)
        assert same(R["K"], K[c]), c
    perm = np.array([3, 0, 4, 2, 1])
    Kp, stp, _ = pkg.transition_batch(pr["r"][perm], pr["w"][perm], pr["pcT"][perm], lam0[perm],
                                      *args)
    assert same(Kp, K[perm]) and (stp == 0).all()
    # a path the backward pass stops: K all NaN, its status and fail_t kept, the others untouched
    pcT = pr["pcT"].copy()
    pcT[2, 1, 5] = np.nan
    Kn, stn, ftn = pkg.transition_batch(pr["r"], pr["w"], pcT, lam0, *args)
    assert list(stn) == [0, 0, 1, 0, 0] and ftn[2] == T - 1 and np.isnan(Kn[2]).all()
    keep = [0, 1, 3, 4]
    assert same(Kn[keep], K[keep])


def test_driver_on_the_gpu_equals_the_cpu_backend_driver(gpu, pkg):
    """N = 3, Na = 60, T = 12: a 1 % TFP drop with persistence 0.8, and Z ≡ 1."""
    cb = pkg.calibration
    cal = _cal(pkg, 3, 60)
    ss = tr.steady_state_cpu(cal, 0.03, lambda r: cb.wage(r, cal["alpha"], cal["delta"]))
    T = 12
    Z = np.stack([1 - 0.01 * 0.8 ** np.arange(T), np.ones(T)])
    kw = dict(damp=0.5, tol=1e-6, max_iter=60)
    A = pkg.aiyagari_transition(ss, Z, T, **kw)
    B = pkg.aiyagari_transition(ss, Z, T, backend=tr.transition_batch, **kw)
    assert (B["status"] == 0).all() and B["rounds"][0] > 3 and B["rounds"][1] == 1
    assert np.array_equal(A["rounds"], B["rounds"]) and np.array_equal(A["status"], B["status"])
    for k in ("K", "r", "w", "resid"):
        assert same(A[k], B[k]), k


def test_steady_state_helper_is_a_stationary_point(gpu, pkg):
    """steady_state clears the capital market at each rate's own wage, and a transition without a
    shock from it stays put: one round, K ≡ K_ss within the solves' tolerances."""
    cb = pkg.calibration
    cal = _cal(pkg, 3, 60)
    ss = pkg.steady_state(cal)
    assert -0.02 < ss["r"] < 1 / cal["beta"] - 1
    assert ss["w"] == cb.wage(ss["r"], cal["alpha"], cal["delta"])
    Kd = cb.capital_demand(ss["r"], cal["labor"], cal["alpha"], cal["delta"])
    assert abs(ss["K"] - Kd) <= 1e-4 * Kd
    assert ss["policy_c"].shape == (3, 60) and abs(ss["lam"].sum() - 1) < 1e-10
    R = pkg.aiyagari_transition(ss, np.ones((1, 8)), 8, tol=1e-3)
    assert R["status"][0] == 0 and R["rounds"][0] == 1 and R["resid"][0] < 1e-3
    assert (R["r"] == ss["r"]).all() and (R["w"] == ss["w"]).all()
