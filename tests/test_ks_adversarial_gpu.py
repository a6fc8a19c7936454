"""GPU: the Krusell-Smith VFI kernels against the C oracle, bit for bit, on inputs built to break
their shortcuts (tests/ks_cases.py; tests/test_ks_cases_cpu.py shows the oracle alone reaches the
branches): grids whose spacing varies by 10^4 (the tabled-reciprocal division and the tabled
slope weights), noisy / flat / decreasing / NaN values and hand-built end-rule columns (every
branch of both slope routines), policies on nodes, outside the grid and at its last point with
stale or foreign segment hints, the fused Howard sweep's one- and two-node last tiles and its
one-block/halo switch, and both sides of the one-workgroup/tiled dispatch."""
import functools

import numpy as np
import pytest

from oracle import corc
from oracle import np_oracle as no
from tests import ks_cases as kc

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _cases():
    return kc.vfi_cases()


def _of_size(nk, nK):
    return [c for c in _cases() if c["V"].shape[:2] == (nk, nK)]


def _grids(c):
    return c["k_grid"], c["K_grid"], c["B"], c["P"], kc.prm(c["p"])


def _ogrids(c):
    return kc.cparams(c["p"]), c["k_grid"], c["K_grid"]


def _nan(c):
    return bool(np.isnan(c["V"]).any())


@pytest.mark.parametrize("nk,nK", kc.VFI_SIZES)
def test_improve_matches_oracle(pkg, gpu, nk, nK):
    """ks_policy_improve (tiled: tabled slopes, bracketed segment search): k_opt and nfev."""
    for c in _of_size(nk, nK):
        ko, nf = pkg.ks_policy_improve(c["V"], *_grids(c))
        koO, nfO = corc.ks_policy_improve(*_ogrids(c), c["V"], c["B"], c["P"])
        assert np.array_equal(nf, nfO), c["name"]
        assert np.array_equal(ko, koO, equal_nan=_nan(c)), c["name"]


@pytest.mark.parametrize("steps", [1, 3])
@pytest.mark.parametrize("nk,nK", kc.VFI_SIZES)
def test_howard_with_stale_hints_matches_oracle(pkg, gpu, nk, nK, steps):
    """ks_howard right after an improvement of ANOTHER case of the same shape (the context's
    hint buffer then holds that case's segments), with a policy on nodes, outside
    [k_min, k_max] and at k_grid(end)."""
    cs = _of_size(nk, nK)
    for i, c in enumerate(cs):
        other = cs[(i + 1) % len(cs)]
        pkg.ks_policy_improve(other["V"], *_grids(other))
        ko = kc.howard_kopt(c, 40 + i)
        V = pkg.ks_howard(c["V"], ko, *_grids(c), steps=steps)
        VO = corc.ks_howard(*_ogrids(c), c["V"], ko, c["B"], c["P"], steps)
        assert np.array_equal(V, VO, equal_nan=_nan(c)), c["name"]


def test_howard_after_a_larger_shape(pkg, gpu):
    """A larger problem first, then small ones: whatever the hint buffers hold is foreign."""
    big = _of_size(506, 5)[1]
    pkg.ks_policy_improve(big["V"], *_grids(big))
    for nk, nK in ((253, 2), (64, 5), (4, 2)):
        c = _of_size(nk, nK)[2]
        ko = kc.howard_kopt(c, 3)
        V = pkg.ks_howard(c["V"], ko, *_grids(c), steps=2)
        assert np.array_equal(V, corc.ks_howard(*_ogrids(c), c["V"], ko, c["B"], c["P"], 2))


@pytest.mark.parametrize("nk,nK", kc.SOLVE_SIZES)
def test_vfi_solve_both_sides_of_the_fused_edge(pkg, gpu, nk, nK):
    """ks_vfi_solve, 6 iterations (improvements at 1 and 6) of 3 sweeps, tol = 0, from a noisy
    value and a random policy: 4,096 nodes run in the one-workgroup kernel (its own slope
    routine), 4,112 in the tiled kernels."""
    c = kc.solve_case(nk, nK, 300 + nk)
    R = pkg.ks_vfi_solve(c["V"], c["k0"], *_grids(c), howard_steps=3, tol=0.0, max_vfi=6)
    Ro = corc.ks_vfi_solve(*_ogrids(c), c["V"], c["k0"], c["B"], c["P"], howard=3, tol=0.0,
                           max_vfi=6)
    assert R["iters"] == Ro["iters"] == 6
    assert np.array_equal(R["value"], Ro["value"])
    assert np.array_equal(R["k_opt"], Ro["k_opt"])
    assert R["rel_diff"] == Ro["rel_diff"]


# ------------------------------------------------------------------------------ device tier
SENT = -7.25e9  # no kernel result: the marker of a node that must stay unwritten


def _dev(x):
    import torch
    return torch.as_tensor(np.ascontiguousarray(np.asarray(x).transpose(2, 1, 0)), device="cuda:0")


def _host(t):
    return t.cpu().numpy().transpose(2, 1, 0)


@pytest.mark.parametrize("family", ["noise005", "nan"])
def test_shard_sub_rectangle_matches_oracle(pkg, gpu, family):
    """HipShard on K in [1, 4), s in [1, 3) of a 506 x 5 problem (irregular grid; a last tile
    of two own nodes): improve, howard, and slopes + howard_fused equal the ORACLE on the own
    nodes; every other node of the outputs keeps a sentinel, and so do the slopes of every
    column the shard does not read."""
    import torch
    nk, nK, K0, K1, s0, s1 = 506, 5, 1, 4, 1, 3
    c = [x for x in _of_size(nk, nK) if x["family"] == family][0]
    nan = _nan(c)
    kg = c["k_grid"]
    sh = pkg.ks_dist.HipShard(*_grids(c), K0, K1, s0, s1)
    own = np.zeros((nk, nK, 4), bool)
    own[:, K0:K1, s0:s1] = True
    V = _dev(c["V"])

    def check(out, ref, what):
        assert np.array_equal(out[own], ref[own], equal_nan=nan), what
        assert np.all(out[~own] == SENT), what

    ko = torch.full_like(V, SENT)
    sh.improve(V, ko)
    koO, _ = corc.ks_policy_improve(*_ogrids(c), c["V"], c["B"], c["P"])
    check(_host(ko), koO, "improve")

    kadv = kc.howard_kopt(c, 11)
    sh.hints(_dev(kc.howard_kopt(c, 12)))            # hints of another policy: all stale
    Vout = torch.full_like(V, SENT)
    sh.howard(V, _dev(kadv), Vout)
    V1 = corc.ks_howard(*_ogrids(c), c["V"], kadv, c["B"], c["P"], 1)
    check(_host(Vout), V1, "howard")

    dV = torch.full_like(V, SENT)
    sh.slopes(V, dV)
    kp = np.asarray(sh.kp_idx).reshape(4, nK)
    read = np.zeros((nK, 4), bool)
    for s in range(s0, s1):
        for K in range(K0, K1):
            read[K, s] = True
            read[kp[s, K], :] = True
    assert not read.all()                             # some column stays unread
    d = _host(dV)
    with np.errstate(all="ignore"):
        for K in range(nK):
            for s in range(4):
                if read[K, s]:
                    ref = no.pchip_slopes(kg, c["V"][:, K, s])
                    assert np.array_equal(d[:, K, s], ref, equal_nan=nan), (K, s)
                else:
                    assert np.all(d[:, K, s] == SENT), (K, s)

    Vf, dVf = torch.full_like(V, SENT), torch.full_like(V, SENT)
    sh.howard_fused(V, dV, _dev(kadv), Vf, dVf)
    torch.cuda.synchronize()
    check(_host(Vf), V1, "howard_fused value")
    d1 = np.full((nk, nK, 4), SENT)
    with np.errstate(all="ignore"):
        for K in range(K0, K1):
            for s in range(s0, s1):
                d1[:, K, s] = no.pchip_slopes(kg, V1[:, K, s])
    check(_host(dVf), d1, "howard_fused slopes")
    sh.close()


def test_shard_reldiff_matches_nanmax(pkg, gpu):
    """ks_dev_reldiff = nanmax(|V - Vold| / (|Vold| + 1e-10)) over the own nodes: zeros in Vold,
    NaN in either array, and own nodes that are all NaN (-> NaN)."""
    nk, nK = 257, 2
    c = _of_size(nk, nK)[1]
    rng = np.random.default_rng(5)
    sh = pkg.ks_dist.HipShard(*_grids(c), 1, 2, 0, 4)
    own = np.zeros((nk, nK, 4), bool)
    own[:, 1:2, :] = True
    Vold = rng.standard_normal((nk, nK, 4))
    V = Vold + 1e-3 * rng.standard_normal((nk, nK, 4))
    Vold[rng.random(Vold.shape) < 0.05] = 0.0
    V[rng.random(V.shape) < 0.05] = np.nan
    Vold[rng.random(Vold.shape) < 0.05] = np.nan
    V[:, 0, :] = 1e6                                  # a foreign column must not count
    got = sh.reldiff(_dev(V), _dev(Vold))
    assert got == kc.rel_diff(V[own], Vold[own])
    assert (Vold[own] == 0).any() and np.isnan(V[own]).any() and np.isnan(Vold[own]).any()
    Vn = V.copy()
    Vn[own] = np.nan
    assert np.isnan(sh.reldiff(_dev(Vn), _dev(Vold)))
    sh.close()


# ------------------------------------------------------------------------------ validation
def _code(pkg, fn, *a, **kw):
    with pytest.raises(pkg.AiyError) as e:
        fn(*a, **kw)
    return e.value.status


def test_repeated_grid_point_is_refused(pkg, gpu):
    """A repeated k_grid point (MATLAB's interpolants raise): AIY_BAD_ARG from every KS VFI
    entry point, host tier and device tier."""
    c = _of_size(64, 5)[1]
    kg = c["k_grid"].copy()
    kg[20] = kg[19]
    g = (kg,) + _grids(c)[1:]
    ko = kc.howard_kopt(c, 1)
    assert _code(pkg, pkg.ks_policy_improve, c["V"], *g) == "AIY_BAD_ARG"
    assert _code(pkg, pkg.ks_howard, c["V"], ko, *g, steps=1) == "AIY_BAD_ARG"
    assert _code(pkg, pkg.ks_vfi_solve, c["V"], ko, *g, max_vfi=1) == "AIY_BAD_ARG"
    assert _code(pkg, pkg.ks_vfi_solve, c["V"], ko, *g, max_vfi=1, n_devices=2) == "AIY_BAD_ARG"
    assert _code(pkg, pkg.ks_vfi_solve, c["V"], ko, *g, max_vfi=1, n_devices=2,
                 depth=0) == "AIY_BAD_ARG"
    assert _code(pkg, pkg.ks_dist.HipShard, *g, 0, 5) == "AIY_BAD_ARG"
    assert _code(pkg, pkg.ks_dist.HipShard, *g, 1, 3, 0, 2) == "AIY_BAD_ARG"


@pytest.mark.parametrize("bad", [np.inf, -np.inf])
def test_infinite_value_is_refused(pkg, gpu, bad):
    """±inf in value: AIY_NON_FINITE from the host-tier VFI entry points (the tabled-reciprocal
    division is the IEEE quotient for finite and NaN numerators only); NaN stays accepted."""
    c = _of_size(64, 5)[1]
    V = c["V"].copy()
    V[7, 2, 1] = bad
    g = _grids(c)
    ko = kc.howard_kopt(c, 1)
    assert _code(pkg, pkg.ks_policy_improve, V, *g) == "AIY_NON_FINITE"
    assert _code(pkg, pkg.ks_howard, V, ko, *g, steps=1) == "AIY_NON_FINITE"
    assert _code(pkg, pkg.ks_vfi_solve, V, ko, *g, max_vfi=1) == "AIY_NON_FINITE"
    assert _code(pkg, pkg.ks_vfi_solve, V, ko, *g, max_vfi=1, n_devices=2) == "AIY_NON_FINITE"
    assert _code(pkg, pkg.ks_vfi_solve, V, ko, *g, max_vfi=1, n_devices=2,
                 depth=0) == "AIY_NON_FINITE"
    V[7, 2, 1] = np.nan
    pkg.ks_policy_improve(V, *g)
