"""The tree kernel's wave-level superblock bound: one test of each 512-candidate
superblock per wave, against the wave's lowest bar and its largest cash on hand, instead of one
per lane.  GPU cases: the tree path (an explicit variant, so the small-grid one-launch sweep is
not picked) against the C oracle bit for bit — v_new, idx and the policies — on inputs where a
wave's lanes disagree most: ragged tiles, bars that are not monotone along the tile, −inf / NaN
values, tiles without a feasible candidate, shrinking feasible prefixes, labour groups, and a
bar raised during the walk.  CPU case: the bound has no false negatives, in the kernel's own
operation order."""
import numpy as np
import pytest

from oracle import corc
from oracle import np_oracle as no

W1 = 0                                                      # one wave per tile (tree defaults)
W2 = 2                                                      # two cooperating waves per tile
HL = 16 | 2048 | 1 << 16 | 1 << 21 | 1 << 23 | 1 << 24      # the large-grid default (packed)


def _device_sweep(pkg, V, a, s, P, r, w, hint=None, variant=0, ws=None):
    import torch
    dev = torch.device("cuda:0")
    N, Na = V.shape
    ws = ws or pkg.Workspace(N, Na)
    ws.set_variant(variant)
    t = lambda x: torch.as_tensor(np.ascontiguousarray(x), device=dev)
    vo, at, st, Pt = t(V), t(a), t(s), t(P)
    vn = torch.empty_like(vo); pk = torch.empty_like(vo); pc = torch.empty_like(vo)
    idx = torch.empty((N, Na), dtype=torch.int32, device=dev)
    ht = None if hint is None else t(hint.astype(np.int32))
    ws.vfi_sweep(vo, at, st, Pt, r, w, 0.96, 5.0, vn, idx, pk, pc, hint=ht, mode=1)
    torch.cuda.synchronize()
    return vn.cpu().numpy(), idx.cpu().numpy(), pk.cpu().numpy(), pc.cpu().numpy()


def _same(out, ref):
    for name, x, y in zip(("v_new", "idx", "policy_k", "policy_c"), out, ref):
        assert np.array_equal(x, y, equal_nan=x.dtype.kind == "f"), name


_cache = {}


def _warm(Na, r, sweeps):
    """(a, s, P, w, V after `sweeps` oracle sweeps from v = 0), computed once per key."""
    key = (Na, r, sweeps)
    if key not in _cache:
        cal = no.calib_aiyagari(Na=Na, shocks="rouwenhorst")
        a, s, P = cal["a_grid"], cal["s"], cal["P"]
        w = no.wage(r, 0.36, 0.08)
        V = corc.vfi_solve(np.zeros((7, Na)), a, s, P, r, w, 0.96, 5.0, 1e-5, sweeps)["v_new"]
        _cache[key] = (a, s, P, w, V)
    return _cache[key]


@pytest.mark.gpu
@pytest.mark.parametrize("Na", [1601, 2111])
@pytest.mark.parametrize("variant", [W1, W2])
def test_ragged_last_tile(pkg, gpu, Na, variant):
    """Na not a multiple of 64: the last tile's invalid lanes hold NaN bars and no cash, and
    must drop out of the wave's minimum and maximum.  Cold and hinted."""
    a, s, P, w, V = _warm(Na, 0.03, 12)
    ref = corc.vfi_sweep(V, a, s, P, 0.03, w, 0.96, 5.0)
    for hint in (None, np.clip(ref[1] - 5, 0, Na - 1)):
        _same(_device_sweep(pkg, V, a, s, P, 0.03, w, hint=hint, variant=variant), ref)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [W1, W2, HL])
def test_noisy_value(pkg, gpu, variant):
    """v not monotone in a: the lowest bar of a wave sits at any lane.  Hinted (random hints)
    and cold (idx < 0 lanes: the bar is −inf)."""
    rng = np.random.default_rng(23)
    for Na, scale in ((2001, 1e-3), (1601, 1.0)):
        a, s, P, w, V = _warm(Na, 0.03, 25)
        V = V + scale * rng.standard_normal(V.shape)
        ref = corc.vfi_sweep(V, a, s, P, 0.03, w, 0.96, 5.0)
        for hint in (None, rng.integers(0, Na, (7, Na)), np.full((7, Na), -1)):
            _same(_device_sweep(pkg, V, a, s, P, 0.03, w, hint=hint, variant=variant), ref)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [W1, W2])
def test_special_values_and_infeasible_tiles(pkg, gpu, variant):
    """−inf and NaN entries in v (NaN and −inf candidates in every row), on a grid that starts
    at a = 10 with r = −0.5: the low-income rows' first tiles have no feasible candidate at all
    (the oracle gives NaN at index 1 there), later tiles a short feasible prefix."""
    Na = 1700
    cal = no.calib_aiyagari(Na=Na, shocks="rouwenhorst")
    s, P = cal["s"], cal["P"]
    a = np.linspace(10.0, 60.0, Na)
    r, w = -0.5, 1.0
    coh = (1 + r) * a[None, :] + w * s[:, None]
    assert (coh[0, :128] <= a[0]).all() and (coh[0, -1] > a[0])  # two whole tiles, then some
    # smooth, increasing, concave: interior optima up to a' ≈ a_700, over two superblocks
    V = 0.01 * np.log(a)[None, :] * (1 + 0.1 * np.arange(7))[:, None]
    V[3, [3, 700]] = np.nan
    V[2, 40:45] = -np.inf
    V[5, 1200] = -np.inf
    ref = corc.vfi_sweep(V, a, s, P, r, w, 0.96, 5.0)
    assert np.isnan(ref[0]).any() and np.isfinite(ref[0]).any() and ref[1].max() > 512
    for hint in (None, np.clip(ref[1] + 2, 0, Na - 1)):
        _same(_device_sweep(pkg, V, a, s, P, r, w, hint=hint, variant=variant), ref)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [W1, W2])
def test_negative_interest_rate(pkg, gpu, variant):
    """r = −0.05: cash on hand grows slower than a, so the feasible prefixes shrink."""
    Na = 1800
    a, s, P, w, V = _warm(Na, -0.05, 12)
    ref = corc.vfi_sweep(V, a, s, P, -0.05, w, 0.96, 5.0)
    for hint in (None, np.clip(ref[1] + 1, 0, Na - 1)):
        _same(_device_sweep(pkg, V, a, s, P, -0.05, w, hint=hint, variant=variant), ref)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [16, 4100])
def test_labour_hinted_after_cold(pkg, gpu, variant):
    """A3 (five labour sub-states per lane, two groups): two cold sweeps from v = 0, then one
    hinted sweep compared with the oracle.  Variants: one wave per tile, and the small-grid
    tree default (four cooperating waves, dealt blocks)."""
    import torch
    Na = 1700
    cal = no.calib_aiyagari(Na=Na, rho=0.6, sigma_e=0.2)
    a, s, P = cal["a_grid"], cal["s"], cal["P"]
    L = 0.01 + (1.5 - 0.01) * no.matlab_linspace01(10)
    r = 0.04
    w = no.wage(r, 0.36, 0.08)
    dev = torch.device("cuda", 0)
    t = lambda x: torch.as_tensor(np.ascontiguousarray(x), device=dev)
    a_t, s_t, P_t, L_t = t(a), t(s), t(P), t(L)
    ws = pkg.Workspace(7, Na, 10)
    ws.set_variant(variant)
    v = [torch.zeros((7, Na), dtype=torch.float64, device=dev) for _ in range(2)]
    lin = torch.zeros((7, Na), dtype=torch.int32, device=dev)
    pk, pl, pc = (torch.zeros((7, Na), dtype=torch.float64, device=dev) for _ in range(3))
    cur = 0
    for q in range(3):
        if q == 2:
            V = v[cur].cpu().numpy()
        ws.labor_vfi_sweep(v[cur], a_t, s_t, P_t, L_t, r, w, 0.96, 5.0, 1.0, 2.0, v[1 - cur], lin,
                           pk, pl, pc, hint=None if q < 2 else lin)
        cur = 1 - cur
    torch.cuda.synchronize()
    vo, (pko, plo, pco, lino) = corc.labor_vfi_sweep(V, a, s, P, L, r, w, 0.96, 5.0, 1.0, 2.0)
    assert np.array_equal(v[cur].cpu().numpy(), vo)
    assert np.array_equal(lin.cpu().numpy(), lino)
    assert np.array_equal(pk.cpu().numpy(), pko) and np.array_equal(pl.cpu().numpy(), plo)
    assert np.array_equal(pc.cpu().numpy(), pco)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [W1, HL])
def test_chained_hinted_sweeps(pkg, gpu, variant):
    """Five chained hinted sweeps from v = 0 at Na = 2,048 (after the cold first one): early in
    a solve the optimum drifts, so the walk's exact paths raise lanes' bars above the wave's
    older minimum.  Every sweep's output equals the oracle's for the same input."""
    Na = 2048
    cal = no.calib_aiyagari(Na=Na, shocks="rouwenhorst")
    a, s, P = cal["a_grid"], cal["s"], cal["P"]
    w = no.wage(0.04, 0.36, 0.08)
    ws = pkg.Workspace(7, Na)
    V, hint = np.zeros((7, Na)), None
    for _ in range(6):
        out = _device_sweep(pkg, V, a, s, P, 0.04, w, hint=hint, variant=variant, ws=ws)
        _same(out, corc.vfi_sweep(V, a, s, P, 0.04, w, 0.96, 5.0))
        V, hint = out[0], out[1]


# ------------------------------------------------------------------ CPU: no false negatives
K_TAU = 2.0 ** -46
K_THR = 1.0 - 2.0 ** -48


def _screen_B(best, idx, dis, n):
    """bell_dev.hpp screen_B, operation for operation."""
    nd = float(n)
    with np.errstate(all="ignore"):
        B = nd * (best + dis) - (K_TAU * nd) * (np.abs(best) + np.abs(dis))
    return np.where(idx < 0, -np.inf, B)


def _screen_t(cx, dd, n):
    """bell_dev.hpp screen_t: t = dd · max(cx, 0)^n by square-and-multiply from the top bit."""
    with np.errstate(all="ignore"):
        c = np.fmax(cx, 0.0)
        p = c.copy()
        for b in range(n.bit_length() - 2, -1, -1):
            p = p * p
            if (n >> b) & 1:
                p = p * c
        return dd * p


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6, 7, 8])
def test_wave_bound_has_no_false_negative(n):
    """On random (D, a0, coh, best) with NaN and ±inf mixed in, idx < 0 lanes (bar −inf) and
    invalid sub-states (NaN bar, no cash), the wave-level test — (D − min B)·max(max coh − a0,
    0)^n ≥ 1 − 2^-48 — is true whenever some lane's own test is."""
    rng = np.random.default_rng(100 + n)
    nw, LB = 1000, 5                      # waves; sub-states per lane (labour groups)
    special = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0])

    def mix(x, frac):
        m = rng.random(x.shape) < frac
        return np.where(m, rng.choice(special, x.shape), x)

    # bars around the bounds' own scale, so that tests pass and fail in comparable numbers
    best = mix(-rng.lognormal(0.0, 2.0, (nw, 64, 1)) * np.ones((1, 1, LB)), 0.03)
    dis = rng.random((1, 1, LB)) * (LB > 1)
    idx = np.where(rng.random((nw, 64, 1)) < 0.05, -1, 7)
    valid = rng.random((nw, 64, LB)) < 0.9
    valid[: nw // 8] &= rng.random((nw // 8, 64, 1)) < 0.05   # nearly empty waves
    valid[:8] = False                                          # and wholly empty ones
    coh = mix(rng.lognormal(0.0, 1.5, (nw, 64, LB)) - 0.5, 0.02)
    B = np.where(valid, _screen_B(best, idx, dis, n), np.nan)
    nblk = 16                                                  # block bounds per wave
    with np.errstate(all="ignore"):
        D = mix(n * -rng.lognormal(0.0, 2.0, (nw, nblk)) + 1.0, 0.03)
    a0 = mix(rng.lognormal(0.0, 1.5, (nw, nblk)) - 0.5, 0.02)

    with np.errstate(all="ignore"):
        t_lane = _screen_t(coh[:, None] - a0[:, :, None, None], D[:, :, None, None] - B[:, None], n)
        lane_pass = (t_lane >= K_THR).any(axis=(2, 3))
        bmin = np.fmin.reduce(B.reshape(nw, -1), axis=1)
        cmax = np.fmax.reduce(np.where(valid, coh, -np.inf).reshape(nw, -1), axis=1)
        wave_pass = _screen_t(cmax[:, None] - a0, D - bmin[:, None], n) >= K_THR
    assert lane_pass.any() and (~lane_pass).any() and (wave_pass & ~lane_pass).any()
    empty = ~valid.reshape(nw, -1).any(axis=1)
    assert empty.any() and not wave_pass[empty].any()          # every bar NaN: false
    assert not (lane_pass & ~wave_pass).any()
