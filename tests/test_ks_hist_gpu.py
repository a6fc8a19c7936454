"""GPU: the Krusell-Smith histogram simulation (csrc/ks_hist_kernels.hip) through the C ABI, the
device tier, the gateway and the ALM driver, against the numpy restatement tests/ks_hist_ref.py —
λ, K_ts and slow_periods bit for bit (the kernel and the restatement perform the same IEEE
operations in the same order)."""
import numpy as np
import pytest

from tests import ks_hist_cases as cases
from tests import ks_hist_ref as ref
from tests import mexstub

pytestmark = pytest.mark.gpu


def _ref(c):
    return ref.simulate(c["k_opt"], c["k_grid"], c["K_grid"], c["x"], c["params"], c["zi"],
                        c["lam0"])


def _host(pkg, c):
    return pkg.ks_panel.ks_simulate_hist(c["k_opt"], c["k_grid"], c["K_grid"], c["x"], c["zi"],
                                         c["lam0"], c["params"])


def _same(got, want):
    for g, w, name in zip(got, want, ("K_ts", "lam", "slow_periods")):
        assert np.array_equal(np.asarray(g), np.asarray(w)), name


def _dev_sim(pkg, c):
    return pkg.ks_panel.HistSim(c["k_grid"], c["K_grid"], c["x"], c["zi"], c["lam0"],
                                c["params"])


def _dev_run(sim, c):
    import torch
    ko = torch.as_tensor(np.ascontiguousarray(c["k_opt"].transpose(2, 1, 0)),
                         device=sim.lam.device)
    K = sim(ko)
    torch.cuda.synchronize()
    return K.cpu().numpy().T, sim.lam.cpu().numpy(), sim.slow.cpu().numpy()


@pytest.mark.parametrize("nx,nk,nK,T,M", cases.SHAPES)
def test_shapes_match_the_restatement(pkg, gpu, nx, nk, nK, T, M):
    """Every listed nx, nk, nK, T and M; kn clamped at both ends of x; K_t below K_grid[0] and
    above K_grid[-1] (the paths start at 25, 40 and 62); monotone policies: no slow period."""
    c = cases.case(nx, nk, nK, T, M, seed=nx + T + M)
    want = _ref(c)
    assert not want[2].any()
    if T > 3 and M >= 3:
        assert want[0].min() < c["K_grid"][0] and want[0].max() > c["K_grid"][-1]
    _same(_host(pkg, c), want)


@pytest.fixture(scope="module")
def reference_size():
    c = cases.case(1000, 100, 4, 1100, 2, seed=11)
    c30 = dict(c, zi=c["zi"][:30])
    return c, c30, _ref(c30)


def test_reference_size_first_30_periods(pkg, gpu, reference_size):
    """nx = 1,000, nk = 100, nK = 4, M = 2: T = 1,100 on the GPU agrees with the restatement on
    the first 30 periods, and the T = 30 run of the same inputs agrees in full."""
    c, c30, want = reference_size
    K_ts, lam, slow = _host(pkg, c)
    assert np.array_equal(K_ts[:30], want[0]) and np.all(np.isfinite(K_ts))
    assert abs(lam.sum() - 2.0) <= 1e-9 and not slow.any()
    _same(_host(pkg, c30), want)


def test_runs_at_the_chunk_boundaries(pkg, gpu):
    """Runs of exactly 32, 33, 64, 65 and 130 sources (test_ks_hist_cpu.py checks the input has
    them): the chunked order of dist_mass at and past kDistChunk and two chunks."""
    c = cases.plateau_case()
    want = _ref(c)
    assert not want[2].any()
    _same(_host(pkg, c), want)


def test_non_monotone_column_takes_the_slow_path_in_some_periods(pkg, gpu):
    c = cases.slow_case()
    want = _ref(c)
    T = c["zi"].shape[0]
    assert np.all((0 < want[2]) & (want[2] < T - 1))
    _same(_host(pkg, c), want)
    _same(_dev_run(_dev_sim(pkg, c), c), want)


@pytest.fixture(scope="module")
def batch_case():
    return cases.case(65, 100, 4, 60, 5, seed=21)


def test_batch_equals_separate_calls(pkg, gpu, batch_case):
    c = batch_case
    K_ts, lam, slow = _host(pkg, c)
    for m in range(c["zi"].shape[1]):
        one = dict(c, zi=c["zi"][:, m:m + 1], lam0=c["lam0"][m:m + 1])
        K1, l1, s1 = _host(pkg, one)
        assert np.array_equal(K1[:, 0], K_ts[:, m]) and np.array_equal(l1[0], lam[m])
        assert s1[0] == slow[m]


def test_device_tier_equals_host_tier_and_reuse_equals_fresh(pkg, gpu, batch_case):
    c = batch_case
    host = _host(pkg, c)
    sim = _dev_sim(pkg, c)
    first = _dev_run(sim, c)
    _same(first, host)
    sim.set_lam(c["lam0"])
    _same(_dev_run(sim, c), host)
    # without the restart the distributions persist: the run continues from the last λ
    cont = dict(c, lam0=host[1])
    _same(_dev_run(sim, c), _host(pkg, cont))


def test_gateway_equals_library(pkg, gpu, batch_case):
    if not mexstub.LIB.exists():
        pytest.skip("libmexstub.so not built")
    c = batch_case
    K_ts, lam, slow = _host(pkg, c)
    M, nx = c["zi"].shape[1], c["x"].size
    lam_m = np.asfortranarray(c["lam0"].transpose(2, 1, 0))
    Kg, lg, sg = mexstub.call("ks_simulate_hist_mex", 3, c["k_opt"], c["k_grid"], c["K_grid"],
                              c["x"], c["params"], c["zi"].astype(np.float64), lam_m)
    assert np.array_equal(Kg, K_ts) and np.array_equal(sg[:, 0], slow)
    assert np.array_equal(lg.reshape((nx, 2, M), order="F").transpose(2, 1, 0), lam)


def test_histogram_alm_loop_equals_its_composition(pkg, gpu):
    """krusell_smith_vfi(simulate="histogram") = ks_vfi_solve + the restatement + the pooled
    regression, iteration by iteration: B_history bit for bit."""
    kp = pkg.ks_panel
    k_size, nx, T, M = 30, 150, 200, 2
    R = kp.krusell_smith_vfi(k_size=k_size, T=T, max_iter_B=2, max_vfi=20, simulate="histogram",
                             n_paths=M, nx=nx)
    prm = pkg.ks_params()
    kg, Kg, P, V0 = pkg.calibration.krusell_smith(k_size=k_size, K_size=4)
    zi = kp.zi_paths(T, M, kp.matlab_rand(M * (T - 1)), prm)
    x = kp.hist_grid(nx, prm[3], prm[4])
    lam = kp.hist_start(x, Kg[0], prm[5])
    value = V0
    k_opt = 0.9 * np.repeat(np.repeat(kg[:, None, None], 4, 1), 4, 2)
    B = np.array([0.0, 1.0, 0.0, 1.0])
    hist = []
    for _ in range(2):
        S = pkg.ks_vfi_solve(value, k_opt, kg, Kg, B, P, prm, howard_steps=50, tol=1e-6,
                             max_vfi=20)
        value, k_opt = S["value"], S["k_opt"]
        K_ts, lam_T, _ = ref.simulate(k_opt, kg, Kg, x, prm, zi, lam)
        lam = kp.hist_carry(lam_T, prm[5])
        B_new, _, _ = kp.alm_regress_paths(K_ts, zi, 100)
        hist.append(B_new)
        B = 0.3 * B_new + 0.7 * B
    assert len(R["B_history"]) == 2
    for a, b in zip(R["B_history"], hist):
        assert np.array_equal(a, b)
    assert np.array_equal(R["K_ts"], K_ts) and R["K_ts"].shape == (T, M)


def test_panel_loop_is_what_it_was(pkg, gpu):
    """The default simulate="panel" equals the direct composition of the existing calls."""
    kp = pkg.ks_panel
    k_size, T, pop = 30, 60, 300
    R = kp.krusell_smith_vfi(k_size=k_size, T=T, population=pop, max_iter_B=2, max_vfi=10,
                             T_discard=10)
    R2 = kp.krusell_smith_vfi(k_size=k_size, T=T, population=pop, max_iter_B=2, max_vfi=10,
                              T_discard=10, simulate="panel")
    prm = pkg.ks_params()
    kg, Kg, P, V0 = pkg.calibration.krusell_smith(k_size=k_size, K_size=4)
    zi, eps = kp.ks_shocks(T, pop, kp.matlab_rand(kp.shock_draws(T, pop)), prm)
    value = V0
    k_opt = 0.9 * np.repeat(np.repeat(kg[:, None, None], 4, 1), 4, 2)
    B = np.array([0.0, 1.0, 0.0, 1.0])
    k_pop = np.full(pop, Kg[0])
    hist = []
    for _ in range(2):
        S = pkg.ks_vfi_solve(value, k_opt, kg, Kg, B, P, prm, howard_steps=50, tol=1e-6,
                             max_vfi=10)
        value, k_opt = S["value"], S["k_opt"]
        K_ts, k_pop = kp.ks_simulate_capital(k_opt, kg, Kg, zi, eps, k_pop)
        B_new, _, _ = kp.alm_regress(K_ts, zi, 10)
        hist.append(B_new)
        B = 0.3 * B_new + 0.7 * B
    for Rq in (R, R2):
        assert len(Rq["B_history"]) == 2
        for a, b in zip(Rq["B_history"], hist):
            assert np.array_equal(a, b)
        assert np.array_equal(Rq["K_ts"], K_ts) and np.array_equal(Rq["k_opt"], k_opt)
