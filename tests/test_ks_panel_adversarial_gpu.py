"""GPU parity of the Krusell-Smith shock panel (F3) and the agent-panel capital simulation (F2),
csrc/ks_panel_kernels.hip, on the adversarial cases of tests/ks_panel_cases.py: the device tier
(ks_shocks_dev, PanelSim), the host tier (ks_shocks, ks_simulate_capital: MATLAB layouts, the
transposed shock strides) and the gateway against oracle/np_oracle.py, bit for bit — integer
shocks, and the interpolation and the mean use IEEE basic operations only, in the kernel's
order.  tests/test_ks_panel_cases_cpu.py holds the conditions under which these comparisons say
something (which branches the cases reach, which defects they would show)."""
import numpy as np
import pytest

from oracle import np_oracle as no
from tests import ks_panel_cases as cases
from tests import mexstub

pytestmark = pytest.mark.gpu


def _t(x, dev):
    import torch
    return torch.tensor(np.ascontiguousarray(x), device=dev)


def _sim(pkg, dev, c, k0=None):
    return pkg.ks_panel.PanelSim(_t(c["k_grid"], dev), _t(c["K_grid"], dev), _t(c["zi"], dev),
                                 _t(c["e"], dev), _t(c["k0"] if k0 is None else k0, dev))


def _call(sim, k_opt, dev):
    import torch
    K_ts = sim(_t(k_opt.transpose(2, 1, 0), dev))
    torch.cuda.synchronize()
    return K_ts.cpu().numpy(), sim.k_pop.cpu().numpy()


def _dev_run(pkg, dev, c):
    return _call(_sim(pkg, dev, c), c["k_opt"], dev)


def _host_run(pkg, c):
    return pkg.ks_panel.ks_simulate_capital(c["k_opt"], c["k_grid"], c["K_grid"],
                                            c["zi"].astype(np.float64),
                                            c["e"].astype(np.float64) + 1.0, c["k0"])


def _same(got, want, name, equal_nan=False):
    assert got[0].shape == want[0].shape and got[1].shape == want[1].shape, name
    assert np.array_equal(got[0], want[0], equal_nan=equal_nan), f"{name}: K_ts"
    assert np.array_equal(got[1], want[1], equal_nan=equal_nan), f"{name}: k_population"


@pytest.mark.parametrize("nk,nK", cases.PANEL_SHAPES)
def test_device_tier_two_sided(pkg, gpu, nk, nK):
    """Every (nk, nK) — the three grid stagings of the step kernel and their boundaries, nk + nK
    = 8192 included — from the three starts: agents below, above and on the nodes of k_grid,
    K_t below, inside and above K_grid."""
    for K0 in cases.STARTS:
        c = cases.panel_case(nk, nK, K0)
        _same(_dev_run(pkg, gpu, c), cases.oracle(c), c["name"])


@pytest.mark.parametrize("c", cases.special_cases(), ids=lambda c: c["name"])
def test_device_tier_ties(pkg, gpu, c):
    """Every agent on a node in every period (each search a tie, tk = 0, and 1 at the last
    node), and K_ts[0] exactly on the last and on an interior node of K_grid."""
    _same(_dev_run(pkg, gpu, c), cases.oracle(c), c["name"])


@pytest.mark.parametrize("T", [2, 3])
def test_device_tier_non_finite_cells(pkg, gpu, T):
    """A NaN and a +inf cell of k_opt read by some agents at t = 0: the same agents, and from
    t = 1 on K_ts, are non-finite in the kernel and in the oracle."""
    c = cases.nonfinite_case(T)
    with np.errstate(all="ignore"):
        want = cases.oracle(c)
    got = _dev_run(pkg, gpu, c)
    _same(got, want, c["name"], equal_nan=True)
    assert np.isfinite(got[0][0]) and np.all(np.isnan(got[0][1:]))


@pytest.mark.parametrize("nk,nK", cases.HOST_SHAPES)
def test_host_tier_two_sided(pkg, gpu, nk, nK):
    """k_opt k x K x 4 column-major, epsi_shock T x population column-major in {1, 2} (the
    kernel's ts = 1, is = T), zi_shock in {0, 1}."""
    for K0 in cases.STARTS:
        c = cases.panel_case(nk, nK, K0)
        _same(_host_run(pkg, c), cases.oracle(c), c["name"])


def test_host_tier_ties(pkg, gpu):
    for c in (cases.node_case(257, 4, "scatter"), cases.node_K_case(4)):
        _same(_host_run(pkg, c), cases.oracle(c), c["name"])


def test_gateway_ragged(pkg, gpu):
    nk, nK, pop, T = 5, 4, 257, 7
    c = cases.panel_case(nk, nK, 40.0, T, pop)
    K_ts, kf = mexstub.call("ks_simulate_capital_mex", 2, c["k_opt"], c["k_grid"], c["K_grid"],
                            c["zi"].astype(np.float64), c["e"].astype(np.float64) + 1.0, c["k0"])
    assert K_ts.shape == (T, 1) and kf.shape == (pop, 1)
    _same((K_ts.ravel(), kf.ravel()), cases.oracle(c), c["name"])


@pytest.mark.parametrize("pop,G", list(zip(cases.REDUCTION_POPS, cases.REDUCTION_G)))
def test_reduction_geometry(pkg, gpu, pop, G):
    """The mean's fold at G = 1 (nothing to fold), shuffles only (G <= 64), partial and full
    register stages with zero padding (65 ... 1023), and G = 1024 with exactly one agent per
    lane, one lane holding two, and every lane holding two and one three."""
    c = cases.reduction_case(pop)
    assert no.ks_panel_blocks(pop) == G
    got, want = _dev_run(pkg, gpu, c), cases.oracle(c)
    assert got[0].shape == (3,)
    _same(got, want, c["name"])


@pytest.mark.parametrize("T,pop", [(6, 600), (7, 600), (6, 16385), (7, 16385)])
def test_reuse_carries_the_population(pkg, gpu, T, pop):
    """One PanelSim called twice with two policies (the ALM loop's use): the second call starts
    from the first call's k_final — after an even and an odd number of periods, so the ping-pong
    of the block partials restarts from either half — and a third call from a population written
    into sim.k_pop in place."""
    kg, Kg = cases.grid_p(100), cases.K_grid(4)
    zi, e = cases.direct_shocks(T, pop, 90 + T)
    rs = np.random.RandomState(pop + T)
    c = dict(k_grid=kg, K_grid=Kg, zi=zi, e=e, k0=rs.uniform(-5.0, 400.0, pop))
    ko_a = cases.two_sided_policy(kg, Kg)
    ko_b = 0.97 * ko_a + 0.2
    sim = _sim(pkg, gpu, c)
    k = c["k0"]
    for ko in (ko_a, ko_b):
        want = no.ks_panel_simulate(kg, Kg, ko, zi, e, k)
        _same(_call(sim, ko, gpu), want, "call")
        k = want[1]
    k_new = rs.uniform(0.0, 300.0, pop)
    sim.k_pop.copy_(_t(k_new, gpu))
    _same(_call(sim, ko_a, gpu), no.ks_panel_simulate(kg, Kg, ko_a, zi, e, k_new), "restart")


# ------------------------------------------------------------------ shocks


@pytest.mark.parametrize("T,pop", cases.SHOCK_SHAPES)
def test_shocks_both_tiers(pkg, gpu, T, pop):
    """The loop edges of both chains (T = 1, the 32-step unroll and the 64-step rounds one short,
    exact and one over; one agent, one block short, exact, one over), three (ug, ub), and
    MATLAB's stream and one in which draws equal the thresholds and their neighbours: zi and
    eps through the device tier and through the host tier's transposed strides."""
    import torch
    for ug, ub in cases.UG_UB:
        for stream in cases.STREAMS:
            c = cases.shock_case(T, pop, ug, ub, stream)
            zi_o, e_o = cases.shock_oracle(c)
            zi, eps = pkg.ks_panel.ks_shocks_dev(_t(c["U"], gpu), c["params"], T, pop)
            torch.cuda.synchronize()
            zi, eps = zi.cpu().numpy(), eps.cpu().numpy()
            assert zi.shape == (T,) and eps.shape == (T, pop), c["name"]
            assert np.array_equal(zi, zi_o) and np.array_equal(eps, e_o), c["name"]
            zh, eh = pkg.ks_panel.ks_shocks(T, pop, c["U"], c["params"])
            assert zh.shape == (T,) and eh.shape == (T, pop), c["name"]
            assert np.array_equal(zh, zi_o) and np.array_equal(eh, e_o + 1), c["name"]


# ------------------------------------------------------------------ refusals


def _host_refused(pkg, status, nk=5, nK=2, T=2, pop=3, kg=None, Kg=None, zi=None, eps=None,
                  kp=None):
    """ks_simulate_capital through the C ABI (the Python wrapper copies k_population): refused
    with `status`, k_population as it was."""
    capi = pkg._capi
    n = lambda q: max(q, 1)
    ko = np.zeros(n(nk) * n(nK) * 4)
    kg = np.linspace(0.0, 1.0, n(nk)) if kg is None else np.asarray(kg, np.float64)
    Kg = np.linspace(30.0, 50.0, n(nK)) if Kg is None else np.asarray(Kg, np.float64)
    zi = np.zeros(n(T)) if zi is None else np.asarray(zi, np.float64)
    eps = np.ones(n(T) * n(pop)) if eps is None else np.asarray(eps, np.float64)
    kp = np.arange(1.0, n(pop) + 1.0) if kp is None else np.asarray(kp, np.float64)
    before = kp.copy()
    K_ts = np.zeros(n(T))
    i64, ptr = capi.i64, capi.ptr
    with pytest.raises(pkg.AiyError) as err:
        capi.check(pkg.lib().ks_simulate_capital(ptr(ko), ptr(kg), ptr(Kg), i64(nk), i64(nK),
                                                 ptr(zi), ptr(eps), i64(T), i64(pop), ptr(kp),
                                                 ptr(K_ts)))
    assert err.value.status == status
    assert np.array_equal(kp, before, equal_nan=True)


def test_host_tier_refusals_by_status(pkg, gpu):
    _host_refused(pkg, "AIY_BAD_SHAPE", nk=1)
    _host_refused(pkg, "AIY_BAD_SHAPE", nK=1)
    _host_refused(pkg, "AIY_BAD_SHAPE", T=0)
    _host_refused(pkg, "AIY_BAD_SHAPE", pop=0)
    _host_refused(pkg, "AIY_BAD_ARG", kg=[0.0, 0.25, 0.25, 0.75, 1.0])
    _host_refused(pkg, "AIY_BAD_ARG", kg=[0.0, 0.5, 0.25, 0.75, 1.0])
    _host_refused(pkg, "AIY_BAD_ARG", Kg=[30.0, 30.0])
    _host_refused(pkg, "AIY_BAD_ARG", Kg=[50.0, 30.0])
    _host_refused(pkg, "AIY_BAD_ARG", zi=[0.0, 2.0])
    _host_refused(pkg, "AIY_BAD_ARG", eps=[1.0, 1.0, 0.0, 1.0, 1.0, 1.0])
    _host_refused(pkg, "AIY_BAD_ARG", eps=[1.0, 1.0, 1.0, 1.0, 3.0, 1.0])
    _host_refused(pkg, "AIY_NON_FINITE", kp=[1.0, np.nan, 2.0])
    _host_refused(pkg, "AIY_NON_FINITE", kp=[1.0, 2.0, np.inf])
    # the Python wrapper reports the same status
    with pytest.raises(pkg.AiyError) as err:
        pkg.ks_panel.ks_simulate_capital(np.zeros((5, 2, 4)), np.linspace(0, 1, 5),
                                         np.array([30.0, 50.0]), np.array([0.0, 1.0]),
                                         np.full((2, 3), 3.0), np.ones(3))
    assert err.value.status == "AIY_BAD_ARG"


@pytest.mark.parametrize("bad", ["nk", "nK", "T", "pop"])
def test_device_tier_refuses_bad_shapes(pkg, gpu, bad):
    """ks_simulate_capital_dev with valid buffers and one size out of range: AIY_BAD_SHAPE
    before any launch (k_population as it was)."""
    import torch
    capi = pkg._capi
    size = dict(nk=5, nK=2, T=2, pop=3)
    size[bad] = 1 if bad in ("nk", "nK") else 0
    f64 = dict(dtype=torch.float64, device=gpu)
    kg, Kg = torch.linspace(0, 1, 5, **f64), torch.linspace(30, 50, 2, **f64)
    ko = torch.zeros(40, **f64)
    zi = torch.zeros(2, dtype=torch.int8, device=gpu)
    eps = torch.zeros(6, dtype=torch.int8, device=gpu)
    kp, K_ts, scratch = torch.arange(1, 4, **f64), torch.zeros(2, **f64), torch.zeros(2, **f64)
    i64, ptr = capi.i64, capi.ptr
    with pytest.raises(pkg.AiyError) as err:
        capi.check(pkg.lib().ks_simulate_capital_dev(
            i64(size["nk"]), i64(size["nK"]), ptr(kg), ptr(Kg), ptr(ko), i64(size["T"]),
            i64(size["pop"]), ptr(zi), ptr(eps), ptr(kp), ptr(K_ts), ptr(scratch),
            capi.stream_handle(None)))
    assert err.value.status == "AIY_BAD_SHAPE"
    torch.cuda.synchronize()
    assert kp.cpu().tolist() == [1.0, 2.0, 3.0]


@pytest.mark.parametrize("ug,ub", [(0.0, 0.1), (1.0, 0.1), (0.04, 0.0), (0.04, 1.0), (-0.1, 0.1),
                                   (0.04, 1.5), (np.nan, 0.1)])
def test_shock_tiers_refuse_ug_ub_outside_the_unit_interval(pkg, gpu, ug, ub):
    T, pop = 3, 4
    _, prm = cases.shock_params(ug, ub)
    U = no.matlab_rand_stream(no.ks_shock_draws(T, pop))
    with pytest.raises(pkg.AiyError) as err:
        pkg.ks_panel.ks_shocks(T, pop, U, prm)
    assert err.value.status == "AIY_BAD_ARG"
    with pytest.raises(pkg.AiyError) as err:
        pkg.ks_panel.ks_shocks_dev(_t(U, gpu), prm, T, pop)
    assert err.value.status == "AIY_BAD_ARG"


def test_shock_tiers_refuse_empty_panels(pkg, gpu):
    prm = cases.shock_params(0.04, 0.10)[1]
    for T, pop in ((0, 4), (3, 0)):
        with pytest.raises(pkg.AiyError) as err:
            capi = pkg._capi
            zi, eps = np.zeros(4), np.zeros(16)
            capi.check(pkg.lib().ks_shocks(capi.i64(T), capi.i64(pop), capi.ptr(np.zeros(16)),
                                           capi.ptr(prm), capi.ptr(zi), capi.ptr(eps)))
        assert err.value.status == "AIY_BAD_SHAPE"
