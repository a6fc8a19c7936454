"""GPU: the Krusell-Smith EGM drivers — krusell_smith_egm against the composed oracles, and
krusell_smith_egm_batch (economies in lockstep, two launches per ALM round) against solo
krusell_smith_egm(simulate="histogram") runs — bit for bit."""
import numpy as np
import pytest

from oracle import np_oracle as no
from tests import ks_egm_batch_cases as bc

pytestmark = pytest.mark.gpu

KW = dict(k_size=bc.K_SIZE, K_size=bc.KK_SIZE, T=bc.T, T_discard=bc.T_DISCARD,
          max_egm=bc.MAX_EGM)


def test_panel_driver_equals_the_composed_oracles(pkg, gpu):
    kp = pkg.ks_panel
    pop = 512
    R = kp.krusell_smith_egm(simulate="panel", population=pop, max_iter_B=2, **KW)
    I = bc.inputs(pkg)
    prm, kg, Kg, P = I["prm"][0], I["k_grid"], I["K_grid"][0], I["P"][0]
    U = kp.matlab_rand(kp.shock_draws(bc.T, pop))
    zi, e = no.ks_shocks(dict(ug=prm[5], ub=prm[6]), bc.T, pop, U)
    k_opt, B, k_pop, hist = I["k0"], np.array(bc.B_IDENTITY), np.full(pop, Kg[0]), []
    for _ in range(2):
        S = bc.oracle_solve(I, 0, k_opt, B)
        k_opt = S["k_opt"]
        K_ts, k_pop = no.ks_panel_simulate(kg, Kg, k_opt, zi, e, k_pop)
        B_new, _, _ = kp.alm_regress(K_ts, zi, bc.T_DISCARD)
        hist.append(B_new)
        B = 0.3 * B_new + 0.7 * B
    assert len(R["B_history"]) == 2 and len(R["egm_iters"]) == 2
    for a, b in zip(R["B_history"], hist):
        assert np.array_equal(a, b)
    assert np.array_equal(R["K_ts"], K_ts) and np.array_equal(R["k_opt"], k_opt)
    assert np.array_equal(R["B"], B) and np.array_equal(R["zi"], zi)


@pytest.fixture(scope="module")
def solo_runs(pkg, gpu):
    kp = pkg.ks_panel
    return [kp.krusell_smith_egm(simulate="histogram", n_paths=bc.N_PATHS, nx=bc.NX,
                                 max_iter_B=bc.ROUNDS, **KW, **eco) for eco in bc.ECONOMIES]


def _same_run(got, want):
    assert got["failed"] is None
    assert len(got["B_history"]) == len(want["B_history"])
    for a, b in zip(got["B_history"], want["B_history"]):
        assert np.array_equal(a, b)
    for key in ("B", "K_ts", "k_opt", "slow_periods", "zi", "x_grid"):
        assert np.array_equal(got[key], want[key]), key
    assert got["egm_iters"] == want["egm_iters"]


def test_solo_histogram_driver_equals_the_composed_oracles(pkg, gpu, solo_runs):
    """The yardstick of the batch comparison is itself the oracles' composition, carried λ
    included; its sweep counts and slow periods are the ones test_ks_egm_batch_cpu.py asserts."""
    want = bc.oracle_rounds(pkg, carry=True)
    for R, w in zip(solo_runs, want):
        assert R["egm_iters"] == w["iters"]
        for a, b in zip(R["B_history"], w["B_history"]):
            assert np.array_equal(a, b)
        assert np.array_equal(R["K_ts"], w["K_ts"][-1]) and np.array_equal(R["k_opt"], w["k_opt"][-1])
        assert np.array_equal(R["slow_periods"], w["slow"][-1])


def test_batch_driver_equals_solo_runs(pkg, gpu, solo_runs):
    got = pkg.ks_panel.krusell_smith_egm_batch(list(bc.ECONOMIES), n_paths=bc.N_PATHS, nx=bc.NX,
                                               max_iter_B=bc.ROUNDS, **KW)
    assert len(got) == 3
    for g, w in zip(got, solo_runs):
        _same_run(g, w)
        assert len(g["B_history"]) == bc.ROUNDS
    assert got[2]["slow_periods"].any() and not got[0]["slow_periods"].any()


def test_converged_economy_leaves_and_the_rest_continue_unchanged(pkg, gpu, solo_runs):
    """tol_B between the economies' round-2 changes of B: the one below it converges there and
    leaves, the others run their third round as if alone."""
    kp = pkg.ks_panel
    want = bc.oracle_rounds(pkg, carry=True)
    d2 = []
    for w in want:                                 # max|B_new - B| of round 2 per economy
        B1 = 0.3 * w["B_history"][0] + 0.7 * np.array(bc.B_IDENTITY)
        d2.append(float(np.max(np.abs(w["B_history"][1] - B1))))
    first = int(np.argmin(d2))
    tol_B = 0.5 * (sorted(d2)[0] + sorted(d2)[1])
    assert sorted(d2)[0] < tol_B < sorted(d2)[1]
    d1 = [float(np.max(np.abs(w["B_history"][0] - np.array(bc.B_IDENTITY)))) for w in want]
    assert min(d1) > tol_B
    got = kp.krusell_smith_egm_batch(list(bc.ECONOMIES), n_paths=bc.N_PATHS, nx=bc.NX,
                                     max_iter_B=bc.ROUNDS, tol_B=tol_B, **KW)
    for e, (g, eco) in enumerate(zip(got, bc.ECONOMIES)):
        assert len(g["B_history"]) == (2 if e == first else 3)
        solo = kp.krusell_smith_egm(simulate="histogram", n_paths=bc.N_PATHS, nx=bc.NX,
                                    max_iter_B=bc.ROUNDS, tol_B=tol_B, **KW, **eco)
        _same_run(g, solo)
        if e != first:      # and its rounds are the ones it runs when nobody leaves
            for a, b in zip(g["B_history"], solo_runs[e]["B_history"]):
                assert np.array_equal(a, b)
            assert np.array_equal(g["K_ts"], solo_runs[e]["K_ts"])
            assert np.array_equal(g["k_opt"], solo_runs[e]["k_opt"])
