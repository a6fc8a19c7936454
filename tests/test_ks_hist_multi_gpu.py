"""GPU: the histogram simulation with one policy per path (ks_simulate_hist_multi, HistSimMulti)
against ks_simulate_hist with each candidate alone and the numpy restatement tests/ks_hist_ref.py —
K_ts, λ and slow_periods bit for bit."""
import numpy as np
import pytest

from tests import ks_egm_batch_cases as bc
from tests import ks_hist_cases as hc
from tests import ks_hist_ref as ref

pytestmark = pytest.mark.gpu

POL = [0, 1, 2, 2, 1, 0]


def _policies(pkg, which):
    """sweeps3: the economies' policies after three sweeps (all monotone: no slow period);
    round2: their second ALM round's policies, where E2's keys are not monotone in some
    periods while E0's and E1's are — both gather orders in one launch."""
    if which == "sweeps3":
        return bc.sweeps3(pkg)
    return np.stack([r["k_opt"][1] for r in bc.oracle_rounds(pkg, carry=False)])


def _check_paths(pkg, ko, kg, Kg, x, prm, zi, lam0, pol, got):
    """Every path of `got` equals ks_simulate_hist with its candidate alone and the restatement."""
    kp = pkg.ks_panel
    K_ts, lam, slow = got
    for m, c in enumerate(pol):
        one = kp.ks_simulate_hist(ko[c], kg, Kg[c], x, zi[:, m], lam0[m], prm[c])
        want = ref.simulate(ko[c], kg, Kg[c], x, prm[c], zi[:, m], lam0[m])
        for w in (one, want):
            assert np.array_equal(K_ts[:, m], w[0][:, 0]), (m, c)
            assert np.array_equal(lam[m], w[1][0]) and slow[m] == w[2][0], (m, c)


@pytest.mark.parametrize("which", ["sweeps3", "round2"])
def test_multi_equals_single_calls_and_the_restatement(pkg, gpu, which):
    """T = 40, nx = 64, M = 6, policy_of_path = [0, 1, 2, 2, 1, 0], two distinct shock paths
    repeated.  The three-sweep policies take no slow period on any start we tried, so the slow
    path is exercised by the round-2 policies (asserted: E2's paths have slow periods, the
    others none)."""
    I, kp = bc.inputs(pkg), pkg.ks_panel
    ko = _policies(pkg, which)
    zi = I["zi"][:, [0, 1, 0, 1, 0, 1]]
    lam0 = np.stack([kp.hist_start(I["x"], I["K_grid"][c][0], I["prm"][c][5]) for c in POL])
    got = kp.ks_simulate_hist_multi(ko, I["k_grid"], I["K_grid"], I["x"], zi, lam0, I["prm"], POL)
    _check_paths(pkg, ko, I["k_grid"], I["K_grid"], I["x"], I["prm"], zi, lam0, POL, got)
    if which == "round2":
        slow = got[2]
        assert slow[2] > 0 and slow[3] > 0 and not slow[[0, 1, 4, 5]].any()


def _lds_bytes(nx, nk, nK, kopt):
    nd = 8 * nx + nK + 8 + (4 * nK * nk if kopt else 0)
    ni = (5 * nx + 4 + 1) & ~1
    return 8 * nd + 4 * ni


def test_policy_read_through_l2(pkg, gpu):
    """k_size = 700, K_size = 8: the policy (179 KB) does not fit beside the path's state, so
    ks_hist_kopt_in_lds is false and each workgroup reads its candidate's block through L2."""
    nx, nk, nK, T = 64, 700, 8, 6
    assert _lds_bytes(nx, nk, nK, False) <= 160 * 1024 < _lds_bytes(nx, nk, nK, True)
    kg, x = hc.grid7(nk), hc.grid7(nx)
    Kg = np.stack([np.linspace(30.0, 50.0, nK), np.linspace(20.0, 45.0, nK)])
    ko = np.stack([hc.smooth_policy(kg, Kg[0]), 0.97 * hc.smooth_policy(kg, Kg[1])])
    prm = np.stack([hc.PARAMS, bc.inputs(pkg)["prm"][2]])
    pol = [1, 0, 1]
    zi = hc.shock_paths(T, 3, seed=8)
    lam0 = hc.start(x, 3)
    got = pkg.ks_panel.ks_simulate_hist_multi(ko, kg, Kg, x, zi, lam0, prm, pol)
    _check_paths(pkg, ko, kg, Kg, x, prm, zi, lam0, pol, got)


def _dev_policies(ko, gpu):
    import torch
    return torch.as_tensor(np.ascontiguousarray(ko.transpose(0, 3, 2, 1)), device=gpu)


def test_one_candidate_equals_the_single_policy_device_tier(pkg, gpu):
    import torch
    I, kp = bc.inputs(pkg), pkg.ks_panel
    ko = bc.sweeps3(pkg)[2]
    zi = I["zi"][:, [0, 1, 1]]
    lam0 = hc.start(I["x"], 3)
    single = kp.HistSim(I["k_grid"], I["K_grid"][2], I["x"], zi, lam0, I["prm"][2])
    Ks = single(_dev_policies(ko[None], gpu)[0])
    multi = kp.HistSimMulti(I["k_grid"], I["x"], zi, lam0)
    Km = multi(_dev_policies(ko[None], gpu), I["K_grid"][2], I["prm"][2], [0, 0, 0])
    torch.cuda.synchronize()
    assert torch.equal(Ks, Km) and torch.equal(single.lam, multi.lam)
    assert torch.equal(single.slow, multi.slow)


def test_hist_sim_multi_reuse_continues_from_the_last_distribution(pkg, gpu):
    """Two calls with persisting λ equal the restatement run twice, the second from the first's
    last distribution."""
    import torch
    I, kp = bc.inputs(pkg), pkg.ks_panel
    ko = _policies(pkg, "round2")
    zi = I["zi"][:, [0, 1, 0, 1, 0, 1]]
    lam0 = np.stack([kp.hist_start(I["x"], I["K_grid"][c][0], I["prm"][c][5]) for c in POL])
    sim = kp.HistSimMulti(I["k_grid"], I["x"], zi, lam0)
    kd = _dev_policies(ko, gpu)
    lam = lam0
    for _ in range(2):
        K = sim(kd, I["K_grid"], I["prm"], POL)
        torch.cuda.synchronize()
        got = (K.cpu().numpy().T, sim.lam.cpu().numpy(), sim.slow.cpu().numpy())
        for m, c in enumerate(POL):
            w = ref.simulate(ko[c], I["k_grid"], I["K_grid"][c], I["x"], I["prm"][c], zi[:, m],
                             lam[m])
            assert np.array_equal(got[0][:, m], w[0][:, 0]) and np.array_equal(got[1][m], w[1][0])
            assert got[2][m] == w[2][0]
        lam = got[1]
