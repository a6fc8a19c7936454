"""GPU: the Krusell-Smith VFI drivers — krusell_smith_vfi_batch (economies in lockstep, two
launches per ALM round, value and policy warm on the device) against solo
krusell_smith_vfi(simulate="histogram", **economy) runs and against rounds composed from the
oracles — bit for bit."""
import numpy as np
import pytest

from tests import ks_vfi_batch_cases as vc

pytestmark = pytest.mark.gpu

SIM = dict(T=vc.T, T_discard=vc.T_DISCARD, n_paths=vc.N_PATHS, nx=vc.NX)
LOCKSTEP = dict(k_size=20, K_size=12, update_B=0.5, max_iter_B=4)
LEAVES = dict(k_size=24, K_size=8, update_B=1.0, tol_B=2e-4, max_iter_B=5)


def _same_run(got, want):
    assert got["failed"] is None
    assert len(got["B_history"]) == len(want["B_history"])
    for a, b in zip(got["B_history"], want["B_history"]):
        assert np.array_equal(a, b)
    for key in ("B", "K_ts", "value", "k_opt", "slow_periods", "zi", "x_grid"):
        assert np.array_equal(got[key], want[key]), key
    assert got["vfi_iters"] == want["vfi_iters"]
    assert got["R2"] == want["R2"]


def _solo_runs(pkg, kw):
    return [pkg.ks_panel.krusell_smith_vfi(simulate="histogram", **SIM, **kw, **eco)
            for eco in vc.ECONOMIES]


def test_lockstep_equals_solo_runs_and_the_composed_oracles(pkg, gpu):
    """Four rounds at k = 20, K = 12 with damping 0.5: the forecast indices move between rounds,
    so the warm solves of rounds 2-4 run different numbers of iterations per economy."""
    want = vc.oracle_rounds(pkg, 20, 12, 4, 0.5)
    assert [w["iters"] for w in want] == [[39, 1, 10, 2], [30, 1, 1, 2], [42, 1, 9, 9]]
    solo = _solo_runs(pkg, LOCKSTEP)
    got = pkg.ks_panel.krusell_smith_vfi_batch(list(vc.ECONOMIES), **SIM, **LOCKSTEP)
    assert len(got) == 3
    for g, s, w in zip(got, solo, want):
        _same_run(g, s)
        assert g["vfi_iters"] == w["iters"]
        assert len(g["B_history"]) == 4
        for a, b in zip(g["B_history"], w["B_history"]):
            assert np.array_equal(a, b)
        assert np.array_equal(g["K_ts"], w["K_ts"][-1])
        assert np.array_equal(g["slow_periods"], w["slow"][-1])
        assert np.array_equal(g["B"], w["B"])
        assert np.array_equal(g["value"], w["value"]) and np.array_equal(g["k_opt"], w["k_opt"])


def test_an_economy_leaves_early_and_the_rest_continue_unchanged(pkg, gpu):
    """k = 24, K = 8, undamped, tol_B = 2e-4: economy 1's diff_B falls below it at round 4 and
    it leaves; the others run their fifth round as if alone."""
    want = vc.oracle_rounds(pkg, 24, 8, 5, 1.0, tol_B=2e-4)
    assert [len(w["B_history"]) for w in want] == [5, 4, 5]
    got = pkg.ks_panel.krusell_smith_vfi_batch(list(vc.ECONOMIES), **SIM, **LEAVES)
    solo = _solo_runs(pkg, LEAVES)
    for e, (g, s, w) in enumerate(zip(got, solo, want)):
        _same_run(g, s)
        assert len(g["B_history"]) == (4 if e == 1 else 5)
        assert g["vfi_iters"] == w["iters"]
        assert np.array_equal(g["B"], w["B"]) and np.array_equal(g["K_ts"], w["K_ts"][-1])
        assert np.array_equal(g["value"], w["value"]) and np.array_equal(g["k_opt"], w["k_opt"])


def test_default_economy_is_the_driver_without_keywords(pkg, gpu):
    """krusell_smith_vfi() with no economy keywords and with the defaults spelled out."""
    kw = dict(k_size=12, K_size=2, max_iter_B=2, simulate="histogram", **SIM)
    a = pkg.ks_panel.krusell_smith_vfi(**kw)
    b = pkg.ks_panel.krusell_smith_vfi(beta=0.99, K_min=30.0, K_max=50.0, **kw)
    for key in ("B", "K_ts", "value", "k_opt"):
        assert np.array_equal(a[key], b[key])
    assert a["vfi_iters"] == b["vfi_iters"]
