"""CPU: the Krusell-Smith histogram simulation's restatement (tests/ks_hist_ref.py) against a
dense formulation, an affine policy with a closed-form capital path, the panel oracle and the
employment chain; the host helpers of ks_panel; and everything the C ABI and the gateway decide
before any device work."""
import ctypes as C

import numpy as np
import pytest

from oracle import np_oracle as no
from tests import ks_hist_cases as cases
from tests import ks_hist_ref as ref
from tests import mexstub


# ------------------------------------------------------------------ the restatement


def test_restatement_matches_dense_transition_matrices():
    """λ' = Mat·λ with the period's dense 2nx x 2nx matrix differs from the restatement only in
    summation order: at most about T·nx·eps ~ 1e-12, checked at 1e-11 (a factor 10)."""
    T, nx = 40, 200
    c = cases.case(nx, 100, 4, T, 1, seed=1)
    zi = c["zi"][:, 0]
    K_ts, lam, slow = ref.simulate_path(c["k_opt"], c["k_grid"], c["K_grid"], c["x"], c["params"],
                                        zi, c["lam0"][0])
    assert slow == 0
    ld = c["lam0"][0].reshape(-1).copy()
    Kd = np.zeros(T)
    for t in range(T - 1):
        Kd[t] = ld @ np.tile(c["x"], 2)
        Mat = ref.transition_matrix(c["k_opt"], c["k_grid"], c["K_grid"], c["x"], c["params"],
                                    Kd[t], int(zi[t]), int(zi[t + 1]))
        ld = Mat @ ld
    Kd[T - 1] = ld @ np.tile(c["x"], 2)
    print("max |dlam|", np.abs(ld - lam.reshape(-1)).max(), "max rel dK",
          np.abs(Kd / K_ts - 1).max())
    assert np.abs(ld - lam.reshape(-1)).max() <= 1e-11
    assert np.abs(Kd / K_ts - 1).max() <= 1e-11


def _affine(nk=40, nK=4):
    a, b, cK = 1.5, 0.9, 0.06
    kg = np.linspace(0.0, 100.0, nk)
    Kg = np.linspace(30.0, 50.0, nK)
    ko = np.repeat((a + b * kg[:, None] + cK * Kg[None, :])[:, :, None], 4, 2)
    return a, b, cK, kg, Kg, ko


def test_affine_policy_follows_the_closed_form_and_the_panel_oracle():
    """k' = a + b·k + c·K in all four states, every kn inside the grid: the lottery preserves the
    mean, so K_{t+1} = a + (b + c)·K_t, which is also the panel oracle's path for any population
    started at K0.  Rounding grows by at most T·nx·eps ~ 1e-12 (b + c < 1); 1e-10 is that with a
    factor 100."""
    T, nx = 60, 150
    a, b, cK, kg, Kg, ko = _affine()
    x = np.linspace(0.0, 100.0, nx)          # kn in [1.5 + 1.8, 1.5 + 90 + 3] for K in [30, 50]
    K0 = 33.0
    pkg_lam0 = np.zeros((2, nx))
    j = int(np.searchsorted(x, K0, side="right") - 1)
    w = (K0 - x[j]) / (x[j + 1] - x[j])
    pkg_lam0[:, j] = np.array([0.96, 0.04]) * (1 - w)
    pkg_lam0[:, j + 1] = np.array([0.96, 0.04]) * w
    zi = cases.shock_paths(T, 1, 2)[:, 0]
    K_ts, lam, slow = ref.simulate_path(ko, kg, Kg, x, cases.PARAMS, zi, pkg_lam0)
    assert slow == 0
    Kc = np.zeros(T)
    Kc[0] = K0
    for t in range(T - 1):
        Kc[t + 1] = a + (b + cK) * Kc[t]
    pop = 64
    e = np.random.RandomState(0).randint(0, 2, size=(T, pop)).astype(np.int8)
    Kp, _ = no.ks_panel_simulate(kg, Kg, ko, zi, e, np.full(pop, K0))
    print("max rel vs closed form", np.abs(K_ts / Kc - 1).max(), "vs panel",
          np.abs(K_ts / Kp - 1).max())
    assert np.abs(K_ts / Kc - 1).max() <= 1e-10
    assert np.abs(K_ts / Kp - 1).max() <= 1e-10


def test_unemployment_mass_follows_the_two_state_chain():
    T = 50
    c = cases.case(65, 100, 4, T, 1, seed=4)
    zi = c["zi"][:, 0]
    thr = ref.thr_table(c["params"])
    lam = c["lam0"][0]
    u = lam[1].sum()
    tot = lam.sum()
    for t in range(1, T):
        K_ts, lam, _ = ref.simulate_path(c["k_opt"], c["k_grid"], c["K_grid"], c["x"],
                                         c["params"], zi[t - 1:t + 1], lam)
        p = thr[zi[t], zi[t - 1]]
        u = (tot - u) * (1 - p[0]) + u * (1 - p[1])
        assert abs(lam[1].sum() - u) <= 1e-12
        assert abs(lam.sum() - tot) <= 1e-12


def test_plateau_case_has_runs_at_every_chunk_boundary():
    c = cases.plateau_case()
    K_ts, _, slow = ref.simulate(c["k_opt"], c["k_grid"], c["K_grid"], c["x"], c["params"],
                                 c["zi"], c["lam0"])
    assert not slow.any()
    seen = set()
    for m in range(c["zi"].shape[1]):
        for t in range(c["zi"].shape[0] - 1):
            seen |= cases.run_lengths(c, K_ts[t, m], int(c["zi"][t, m]))
    assert {32, 33, 64, 65, 130} <= seen


def test_slow_case_mixes_slow_and_fast_periods_and_the_rest_take_none():
    c = cases.slow_case()
    T = c["zi"].shape[0]
    _, _, slow = ref.simulate(c["k_opt"], c["k_grid"], c["K_grid"], c["x"], c["params"], c["zi"],
                              c["lam0"])
    assert np.all((0 < slow) & (slow < T - 1)), slow


def test_slow_and_fast_orders_agree_to_rounding():
    rng = np.random.RandomState(7)
    nx = 120
    lam, w = rng.rand(nx), rng.rand(nx)
    key = np.sort(rng.randint(0, 6, nx)) * 20   # long runs: the chunked order is exercised
    key = np.minimum(key, nx - 2)
    f, s = ref.push_fast(lam, w, key), ref.push_slow(lam, w, key)
    assert np.abs(f - s).max() <= 1e-13 and abs(f.sum() - lam.sum()) <= 1e-12


# ------------------------------------------------------------------ ks_panel's host helpers


def test_zi_paths_path_zero_is_the_oracle_chain(pkg):
    T, pop, M = 200, 3, 4
    p, *_ = no.ks_setup()
    U = pkg.ks_panel.matlab_rand(no.ks_shock_draws(T, pop))
    zi_o, _ = no.ks_shocks(p, T, pop, U)
    zi = pkg.ks_panel.zi_paths(T, M, U, pkg.ks_params())
    assert zi.shape == (T, M) and np.array_equal(zi[:, 0], zi_o)
    assert np.array_equal(zi[:, 1], pkg.ks_panel.zi_paths(T, 1, U[T - 1:], pkg.ks_params())[:, 0])
    with pytest.raises(ValueError):
        pkg.ks_panel.zi_paths(T, 2, U[:T], pkg.ks_params())


def test_alm_regress_paths_single_path_is_alm_regress(pkg):
    rng = np.random.RandomState(3)
    T = 300
    K = 40 + np.cumsum(rng.randn(T)) * 0.05
    zi = rng.randint(0, 2, T)
    B1, g1, b1 = pkg.ks_panel.alm_regress(K, zi, 100)
    B2, g2, b2 = pkg.ks_panel.alm_regress_paths(K[:, None], zi[:, None], 100)
    assert np.array_equal(B1, B2) and g1 == g2 and b1 == b2
    K2 = np.stack([K, K[::-1]], 1)
    z2 = np.stack([zi, zi[::-1]], 1)
    B3, _, _ = pkg.ks_panel.alm_regress_paths(K2, z2, 100)
    assert np.all(np.isfinite(B3)) and not np.array_equal(B3, B1)


def test_hist_grid_and_start(pkg):
    x = pkg.ks_panel.hist_grid(1000, 0.0001, 1000.0)
    assert x.size == 1000 and x[0] == 0.0001 and x[-1] == 1000.0 and np.all(np.diff(x) > 0)
    assert np.array_equal(x, cases.grid7(1000))
    lam = pkg.ks_panel.hist_start(x, 30.0, 0.04)
    assert lam.shape == (2, 1000) and np.count_nonzero(lam) == 4
    assert abs(lam.sum() - 1) <= 1e-15 and abs(lam[1].sum() - 0.04) <= 1e-15
    assert abs((lam * x).sum() - 30.0) <= 1e-12
    car = pkg.ks_panel.hist_carry(np.stack([lam, lam]), 0.1)
    assert np.allclose(car[:, 1].sum(1), 0.1) and np.allclose(car.sum((1, 2)), 1.0)


def test_driver_rejects_unknown_simulation(pkg):
    with pytest.raises(ValueError):
        pkg.ks_panel.krusell_smith_vfi(simulate="young")


# ------------------------------------------------------------------ C ABI validation


def _call(pkg, c, **over):
    a = dict(c)
    a.update(over)
    return pkg.ks_panel.ks_simulate_hist(a["k_opt"], a["k_grid"], a["K_grid"], a["x"], a["zi"],
                                         a["lam0"], a["params"])


@pytest.fixture(scope="module")
def small():
    return cases.case(5, 5, 2, 4, 2)


def test_abi_validation_needs_no_device(pkg, small):
    c = small

    def status(**over):
        with pytest.raises(pkg.AiyError) as e:
            _call(pkg, c, **over)
        return e.value.status

    assert status(zi=c["zi"][:1]) == "AIY_BAD_SHAPE"                      # T >= 2
    for name in ("k_grid", "K_grid", "x"):                                 # strictly increasing
        g = c[name].copy()
        g[1] = g[0]
        assert status(**{name: g}) == "AIY_BAD_ARG", name
        g[1] = np.nan
        assert status(**{name: g}) == "AIY_NON_FINITE", name
    ko = c["k_opt"].copy()
    ko[1, 1, 2] = np.inf
    assert status(k_opt=ko) == "AIY_NON_FINITE"
    lam = c["lam0"].copy()
    lam[1, 0, 3] = np.nan
    assert status(lam0=lam) == "AIY_NON_FINITE"
    prm = c["params"].copy()
    prm[0] = np.nan
    assert status(params=prm) == "AIY_NON_FINITE"
    prm = c["params"].copy()
    prm[5] = 1.5
    assert status(params=prm) == "AIY_BAD_ARG"
    zi = c["zi"].astype(np.float64)
    zi[2, 1] = 2.0
    assert status(zi=zi) == "AIY_BAD_ARG"
    zi[2, 1] = 0.5
    assert status(zi=zi) == "AIY_BAD_ARG"


def test_abi_path_count_and_null_pointers(pkg, small):
    c = small
    L = pkg.lib()
    ko = np.asfortranarray(c["k_opt"])
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    lam = np.ascontiguousarray(c["lam0"])
    zi = np.asfortranarray(c["zi"].astype(np.float64))
    K_ts = np.zeros((4, 2), order="F")

    def rc(M=2, T=4, **null):
        a = dict(ko=p(ko), kg=p(c["k_grid"]), Kg=p(c["K_grid"]), x=p(c["x"]), prm=p(c["params"]),
                 zi=p(zi), lam=p(lam), K=p(K_ts))
        a.update({k: None for k in null})
        return L.ks_simulate_hist(a["ko"], a["kg"], a["Kg"], C.c_int64(5), C.c_int64(2), a["x"],
                                  C.c_int64(5), a["prm"], a["zi"], C.c_int64(T), C.c_int64(M),
                                  a["lam"], a["K"], None)

    for name in ("ko", "kg", "Kg", "x", "prm", "zi", "lam", "K"):
        assert rc(**{name: 1}) == 6, name                                  # AIY_BAD_ARG
    assert rc(M=0) == 1 and rc(M=65536) == 1 and rc(T=1) == 1            # AIY_BAD_SHAPE
    # the device tier validates shapes and params before it looks for a device
    args = [C.c_int64(5), C.c_int64(2), p(c["k_grid"]), p(c["K_grid"]), p(ko), p(c["x"])]
    tail = [p(zi), C.c_int64(4), C.c_int64(2), p(lam), p(K_ts), None, None]
    assert L.ks_simulate_hist_dev(*args, C.c_int64(1), p(c["params"]), *tail) == 1
    assert L.ks_simulate_hist_dev(*args, C.c_int64(5), None, *tail) == 6


def test_fit_rule_admits_the_reference_size_and_names_itself(pkg):
    import torch
    for nx, fits in ((1000, True), (1900, True), (2000, False)):
        c = cases.case(nx, 100, 4, 2, 1)
        if fits:
            if not torch.cuda.is_available():
                with pytest.raises(pkg.AiyError) as e:
                    _call(pkg, c)
                assert e.value.status == "AIY_NO_DEVICE"
        else:
            with pytest.raises(pkg.AiyError) as e:
                _call(pkg, c)
            assert e.value.status == "AIY_BAD_SHAPE" and "160 KiB" in str(e.value)


def test_valid_call_needs_a_device(pkg, small):
    import torch
    if torch.cuda.is_available():
        K_ts, lam, slow = _call(pkg, small)      # with a device the same call runs
        assert np.all(np.isfinite(K_ts)) and lam.shape == (2, 2, 5) and not slow.any()
        return
    with pytest.raises(pkg.AiyError) as e:
        _call(pkg, small)
    assert e.value.status == "AIY_NO_DEVICE"


# ------------------------------------------------------------------ gateway


def _mex_args(c):
    lam = np.asfortranarray(c["lam0"].transpose(2, 1, 0))     # nx x 2 x M
    return [c["k_opt"], c["k_grid"], c["K_grid"], c["x"], c["params"],
            c["zi"].astype(np.float64), lam]


def test_gateway_validates_and_balances_its_lock(small):
    if not mexstub.LIB.exists():
        pytest.skip("libmexstub.so not built")
    import torch
    L = mexstub.lib()
    d0 = L.stub_lock_depth()
    args = _mex_args(small)
    with pytest.raises(mexstub.MexError) as e:
        mexstub.call("ks_simulate_hist_mex", 3, *args[:6])
    assert e.value.id == "aiy:usage"
    with pytest.raises(mexstub.MexError) as e:
        mexstub.call("ks_simulate_hist_mex", 4, *args)
    assert e.value.id == "aiy:usage"
    bad = list(args)
    bad[0] = np.zeros((5, 3, 4))                              # k_opt vs the grids
    with pytest.raises(mexstub.MexError) as e:
        mexstub.call("ks_simulate_hist_mex", 3, *bad)
    assert e.value.id == "aiy:shape"
    bad = list(args)
    bad[6] = args[6][:, :, :1]                                # one start for two paths
    with pytest.raises(mexstub.MexError) as e:
        mexstub.call("ks_simulate_hist_mex", 3, *bad)
    assert e.value.id == "aiy:shape"
    bad = list(args)
    bad[4] = np.zeros(12)                                     # params: 13 doubles
    with pytest.raises(mexstub.MexError) as e:
        mexstub.call("ks_simulate_hist_mex", 3, *bad)
    assert e.value.id == "aiy:shape"
    bad = list(args)
    bad[5] = np.full((4, 2), 3.0)                             # library status: zi codes
    with pytest.raises(mexstub.MexError) as e:
        mexstub.call("ks_simulate_hist_mex", 3, *bad)
    assert e.value.id == "aiy:BAD_ARG"
    if not torch.cuda.is_available():
        with pytest.raises(mexstub.MexError) as e:
            mexstub.call("ks_simulate_hist_mex", 3, *args)
        assert e.value.id == "aiy:NO_DEVICE"
    assert L.stub_lock_depth() == d0
