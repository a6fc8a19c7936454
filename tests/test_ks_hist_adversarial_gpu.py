"""GPU: the histogram simulation (csrc/ks_hist_kernels.hip) on the adversarial cases of
tests/ks_hist_adv_cases.py — both instantiations of the kernel (k_opt in LDS, k_opt through L2),
every branch of the thread-to-element walk, whole-row runs, the edges of the monotonicity vote,
exact ties and the shock paths the first tests left out.  K_ts, λ and slow_periods are compared
bit for bit with the restatement tests/ks_hist_ref.py, and the same GPU outputs then with the
independent long-double reference within the recorded tolerance.  The census
tests/test_ks_hist_adv_cases_cpu.py states what each case reaches."""
import numpy as np
import pytest

from tests import ks_hist_adv_cases as cases

pytestmark = pytest.mark.gpu


def _host(pkg, c):
    return pkg.ks_panel.ks_simulate_hist(c["k_opt"], c["k_grid"], c["K_grid"], c["x"], c["zi"],
                                         c["lam0"], c["params"])


def _dev_sim(pkg, c):
    kg, Kg, x = (np.array(c[q]) for q in ("k_grid", "K_grid", "x"))   # (read-only originals)
    return pkg.ks_panel.HistSim(kg, Kg, x, c["zi"], c["lam0"], c["params"])


def _dev_run(sim, k_opt):
    import torch
    ko = torch.as_tensor(np.ascontiguousarray(k_opt.transpose(2, 1, 0)), device=sim.lam.device)
    K = sim(ko)
    torch.cuda.synchronize()
    return K.cpu().numpy().T, sim.lam.cpu().numpy(), sim.slow.cpu().numpy()


def _same(got, want):
    for g, w, name in zip(got, want, ("K_ts", "lam", "slow_periods")):
        assert np.array_equal(np.asarray(g), np.asarray(w)), name


def _check(got, name):
    """Bit for bit against the restatement, then against the independent reference."""
    dK, dl = cases.differences(got, cases.independent(name))
    print(name, cases.instantiation(cases.get(name)), "max rel dK", dK, "max abs dlam", dl)
    _same(got, cases.restatement(name))
    assert dK <= cases.TOL_REL_K and dl <= cases.TOL_ABS_LAM


@pytest.mark.parametrize("name", cases.names())
def test_host_tier(pkg, gpu, name):
    _check(_host(pkg, cases.get(name)), name)


@pytest.mark.parametrize("name", cases.names("lds", "vote", "tie"))
def test_device_tier(pkg, gpu, name):
    c = cases.get(name)
    _check(_dev_run(_dev_sim(pkg, c), c["k_opt"]), name)


def test_vote_cases_count_their_good_periods(pkg, gpu):
    """slow_periods from the GPU itself: the number of zeros among zi[:T-1], per path."""
    for name in ("vote-last1-1100", "vote-first0-64", "vote-long-600"):
        c = cases.get(name)
        assert np.array_equal(_host(pkg, c)[2], cases.expected_slow(c))


@pytest.mark.parametrize("a,b", [("vote-both-129", "vote-long-129"),
                                 ("vote-last1-1100", "vote-first0-1100"),
                                 ("tie-w0", "tie-top")])
def test_histsim_reuse_with_a_different_policy(pkg, gpu, a, b):
    """Policy A, set_lam, policy B on the same object: what a fresh run of B gives."""
    ca, cb = cases.get(a), cases.get(b)
    for q in ("k_grid", "K_grid", "x", "zi", "lam0"):
        assert np.array_equal(ca[q], cb[q]), q
    assert not np.array_equal(ca["k_opt"], cb["k_opt"])
    sim = _dev_sim(pkg, ca)
    _same(_dev_run(sim, ca["k_opt"]), cases.restatement(a))
    sim.set_lam(cb["lam0"])
    _same(_dev_run(sim, cb["k_opt"]), cases.restatement(b))
    _same(_dev_run(_dev_sim(pkg, cb), cb["k_opt"]), cases.restatement(b))


def test_both_instantiations_in_one_process_and_reuse_at_the_unstaged_size(pkg, gpu):
    """An object whose k_opt is staged in LDS runs, then one an nk further, where it is not; the
    second then runs another policy after set_lam and gives what a fresh run of it gives."""
    top = cases.largest_staged_nk(65, 4)
    ca, cb = cases.get(f"lds-nk{top}"), cases.get(f"lds-nk{top + 1}")
    assert cases.instantiation(ca)[0] == "<true>" and cases.instantiation(cb)[0] == "<false>"
    _same(_dev_run(_dev_sim(pkg, ca), ca["k_opt"]), cases.restatement(ca["name"]))
    sim = _dev_sim(pkg, cb)
    _same(_dev_run(sim, cb["k_opt"]), cases.restatement(cb["name"]))
    other = dict(cb, k_opt=0.97 * cb["k_opt"] + 0.2)
    want = cases.restatement_of(other)
    assert not np.array_equal(want[0], cases.restatement(cb["name"])[0])
    sim.set_lam(cb["lam0"])
    _same(_dev_run(sim, other["k_opt"]), want)
    _same(_dev_run(_dev_sim(pkg, other), other["k_opt"]), want)
    # ... and back at the staged size in the same process
    _same(_dev_run(_dev_sim(pkg, ca), ca["k_opt"]), cases.restatement(ca["name"]))


def test_paths_of_the_300_batch_equal_the_same_paths_alone(pkg, gpu):
    c = cases.get("shock-many")
    K_ts, lam, slow = _host(pkg, c)
    for m in (0, 1, 150, 255, 256, 299):
        one = dict(c, zi=c["zi"][:, m:m + 1], lam0=c["lam0"][m:m + 1])
        K1, l1, s1 = _host(pkg, one)
        assert np.array_equal(K1[:, 0], K_ts[:, m]) and np.array_equal(l1[0], lam[m]), m
        assert s1[0] == slow[m]
