"""The tree kernel's group-level 8-block bound: the 64 sub-block bounds of a
superblock are tested in place, one per lane, against the lowest bar and the largest cash on
hand of each group of consecutive lanes, instead of eight at a time per lane.  The tree path
(an explicit variant, so the small-grid one-launch sweep is not picked) against the C oracle bit
for bit — v_new, idx and the policies — where the groups of a wave differ most or are degenerate:
last tiles that leave whole groups without a valid lane, bars that are not monotone inside and
across groups, −inf / NaN values, tiles without a feasible candidate, feasible ranges that end
inside a 64-block and inside an 8-block, every wave split of the group path (one wave, two
waves by 64-block, two and four waves with dealt 8-blocks, packed one-wave tiles), and stale
group bars.  The labour cases run the per-lane cascade, which labour keeps."""
import numpy as np
import pytest

from oracle import corc
from oracle import np_oracle as no

W1 = 0                                                      # one wave per tile (tree defaults)
W2 = 2                                                      # two cooperating waves per tile
HL = 16 | 2048 | 1 << 16 | 1 << 21 | 1 << 23 | 1 << 24      # the large-grid default (packed)
D2 = 2 | 4096                                               # two waves, dealt 8-blocks
D4 = 4 | 4096                                               # four waves, dealt 8-blocks
GEN = 1 << 7                                                # hint window of 2: the generic body
LAB1 = 16                                                   # labour: one wave per tile
LAB4 = 4 | 4096                                             # labour small-grid default: 4 waves, dealt


def _device_sweep(pkg, V, a, s, P, r, w, hint=None, variant=0, ws=None, sigma=5.0):
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
    ws.vfi_sweep(vo, at, st, Pt, r, w, 0.96, sigma, vn, idx, pk, pc, hint=ht, mode=1)
    torch.cuda.synchronize()
    return vn.cpu().numpy(), idx.cpu().numpy(), pk.cpu().numpy(), pc.cpu().numpy()


def _same(out, ref):
    for name, x, y in zip(("v_new", "idx", "policy_k", "policy_c"), out, ref):
        assert np.array_equal(x, y, equal_nan=x.dtype.kind == "f"), name


_cache = {}


def _warm(Na, r, sweeps, sigma=5.0, N=7):
    """(a, s, P, w, V after `sweeps` oracle sweeps from v = 0, the oracle's next sweep), computed
    once per key and left unchanged."""
    key = (Na, r, sweeps, sigma, N)
    if key not in _cache:
        cal = no.calib_aiyagari(Na=Na, shocks="rouwenhorst", N=N)
        a, s, P = cal["a_grid"], cal["s"], cal["P"]
        w = no.wage(r, 0.36, 0.08)
        V = corc.vfi_solve(np.zeros((N, Na)), a, s, P, r, w, 0.96, sigma, 1e-5, sweeps)["v_new"]
        ref = corc.vfi_sweep(V, a, s, P, r, w, 0.96, sigma)
        _cache[key] = (a, s, P, w, V, ref)
    return _cache[key]


@pytest.mark.gpu
@pytest.mark.parametrize("Na", [1601, 1609, 2111])
@pytest.mark.parametrize("variant", [W1, W2, D2, D4, HL])
def test_ragged_last_tile(pkg, gpu, Na, variant):
    """The last tile holds 1 valid lane (Na = 1601: every other group has only NaN bars and no
    cash), 9 (Na = 1609: one valid lane in the second group) or 63 (Na = 2111).  Cold and
    hinted."""
    a, s, P, w, V, ref = _warm(Na, 0.03, 12)
    for hint in (None, np.clip(ref[1] - 5, 0, Na - 1)):
        _same(_device_sweep(pkg, V, a, s, P, 0.03, w, hint=hint, variant=variant), ref)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [W1, W2, D2, D4, HL])
def test_noisy_value(pkg, gpu, variant):
    """v not monotone in a: bars are non-monotone inside and across groups, and near-ties are
    everywhere.  Hinted (random hints) and cold (idx < 0 lanes: the bar is −inf)."""
    rng = np.random.default_rng(29)
    for Na, scale in ((2001, 1e-3), (1601, 1.0)):
        a, s, P, w, V, _ = _warm(Na, 0.03, 25 if Na == 2001 else 12)
        V = V + scale * rng.standard_normal(V.shape)
        ref = corc.vfi_sweep(V, a, s, P, 0.03, w, 0.96, 5.0)
        for hint in (None, rng.integers(0, Na, (7, Na)), np.full((7, Na), -1)):
            _same(_device_sweep(pkg, V, a, s, P, 0.03, w, hint=hint, variant=variant), ref)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [W1, W2, D2, D4, HL])
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
    V[6, 512:520] = -np.inf            # a whole 8-block of −inf bounds inside a superblock
    ref = corc.vfi_sweep(V, a, s, P, r, w, 0.96, 5.0)
    assert np.isnan(ref[0]).any() and np.isfinite(ref[0]).any() and ref[1].max() > 512
    for hint in (None, np.clip(ref[1] + 2, 0, Na - 1)):
        _same(_device_sweep(pkg, V, a, s, P, r, w, hint=hint, variant=variant), ref)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [W1, W2, D2, D4, HL])
def test_negative_interest_rate(pkg, gpu, variant):
    """r = −0.05: cash on hand grows slower than a, so the feasible prefixes shrink and the
    tiles' feasible ranges end inside a 64-block and inside an 8-block of a superblock."""
    Na = 1800
    a, s, P, w, V, ref = _warm(Na, -0.05, 12)
    coh = (1 - 0.05) * a[None, :] + w * s[:, None]
    kf = (a[None, None, :] < coh[:, :, None]).sum(axis=2)          # feasible prefix per state
    kg = np.array([kf[:, j:j + 64].max(axis=1) for j in range(0, Na, 64)])
    assert (kg % 64 != 0).any() and (kg % 8 != 0).any() and (kg < Na).any()
    for hint in (None, np.clip(ref[1] + 1, 0, Na - 1)):
        _same(_device_sweep(pkg, V, a, s, P, -0.05, w, hint=hint, variant=variant), ref)


@pytest.mark.gpu
@pytest.mark.parametrize("N", [2, 7])
@pytest.mark.parametrize("variant", [W1, W2, D4, HL])
def test_number_of_shocks(pkg, gpu, N, variant):
    """N = 2 and N = 7 income states, Na = 1609.  Cold and hinted."""
    Na = 1609
    a, s, P, w, V, ref = _warm(Na, 0.03, 12, N=N)
    for hint in (None, np.clip(ref[1] - 3, 0, Na - 1)):
        _same(_device_sweep(pkg, V, a, s, P, 0.03, w, hint=hint, variant=variant), ref)


@pytest.mark.gpu
@pytest.mark.parametrize("sigma,variant", [(2.0, W1), (2.0, W2), (2.0, HL), (3.0, W1),
                                           (3.0, W2), (3.0, HL), (5.0, W1), (5.0, HL),
                                           (5.0, GEN), (5.0, GEN | W2), (5.0, GEN | D4)])
def test_sigmas_and_bodies(pkg, gpu, sigma, variant):
    """σ = 2, 3, 5 (screen exponents 1, 2, 4); σ = 5 through the three-slot body (the default
    hint window) and the generic one (window of 2), the other σ through the generic body (the
    wave splits and the packed launch are instantiated for σ = 5 only: at σ = 2, 3 the variant's
    geometry bits select nothing, and the run pins that they are harmless)."""
    Na = 1609
    a, s, P, w, V, ref = _warm(Na, 0.03, 12, sigma=sigma)
    for hint in (None, np.clip(ref[1] - 4, 0, Na - 1)):
        _same(_device_sweep(pkg, V, a, s, P, 0.03, w, hint=hint, variant=variant, sigma=sigma),
              ref)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [LAB1, LAB4])
def test_labour_hinted_after_cold(pkg, gpu, variant):
    """Labour at Na = 509, Nl = 10 (five sub-states per lane, two labour groups; the last tile
    holds 61 lanes): two cold sweeps from v = 0, then one hinted sweep compared with the oracle.
    One wave per tile, and the small-grid default (four cooperating waves, dealt 8-blocks).
    The labour instantiations keep the per-lane cascade inside the same `prep` (the group pair
    is too loose across labour levels), with the group reductions feeding the wave's bar."""
    import torch
    Na = 509
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
@pytest.mark.parametrize("variant", [W1, W2, D2, D4, HL])
def test_chained_hinted_sweeps(pkg, gpu, variant):
    """Five chained hinted sweeps from v = 0 at Na = 2,048 on one workspace (after the cold first
    one): early in a solve the optimum drifts, so the walk's exact paths raise lanes' bars above
    the groups' older minima.  Every sweep's output equals the oracle's for the same input."""
    Na = 2048
    cal = no.calib_aiyagari(Na=Na, shocks="rouwenhorst")
    a, s, P = cal["a_grid"], cal["s"], cal["P"]
    w = no.wage(0.04, 0.36, 0.08)
    ws = pkg.Workspace(7, Na)
    V, hint = np.zeros((7, Na)), None
    for q in range(6):
        out = _device_sweep(pkg, V, a, s, P, 0.04, w, hint=hint, variant=variant, ws=ws)
        if ("chain", q) not in _cache:     # (the oracle's sweeps do not depend on the variant)
            _cache[("chain", q)] = corc.vfi_sweep(V, a, s, P, 0.04, w, 0.96, 5.0)
        _same(out, _cache[("chain", q)])
        V, hint = out[0], out[1]
