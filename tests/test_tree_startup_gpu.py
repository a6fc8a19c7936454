"""The tree kernel's start-up: the hint, the momentum and the feasible
prefix loaded in one round at clamped indices, the hint window compiled for its width (variant
bits 7-8 clear: three slots; set: the generic seventeen), and the climb that follows.  The
start-up only sets the screening bar, so whatever the hints are the tree path (an explicit
variant, so the small-grid one-launch sweep is not picked) must equal the C oracle bit for bit:
v_new, idx and both policies.  The cases put the hints where the start-up's index arithmetic is
most exposed: spread over the whole row, one lane of a tile far from the others, at and past
both ends of the feasible prefix, absent in some or all lanes, tiles without a feasible
candidate, ragged last tiles, a drift of thousands of candidates recorded in the momentum, the
early sweeps of a solve, NaN / −inf candidates around the hint, and the batched launch."""
import numpy as np
import pytest

from oracle import corc
from oracle import np_oracle as no

HL = 16 | 2048 | 1 << 16 | 1 << 21 | 1 << 23 | 1 << 24      # the large-grid default (packed)
VARIANTS = [0, 2, HL, HL | 3 << 7]                          # ..., and HL with the generic window
BETA, SIGMA = 0.96, 5.0


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
    ws.vfi_sweep(vo, at, st, Pt, r, w, BETA, SIGMA, vn, idx, pk, pc, hint=ht, mode=1)
    torch.cuda.synchronize()
    return vn.cpu().numpy(), idx.cpu().numpy(), pk.cpu().numpy(), pc.cpu().numpy()


def _same(out, ref, what=""):
    for name, x, y in zip(("v_new", "idx", "policy_k", "policy_c"), out, ref):
        assert np.array_equal(x, y, equal_nan=x.dtype.kind == "f"), (name, what)


_cache = {}


def _warm(Na, r, sweeps, N=7):
    """(a, s, P, w, V after `sweeps` oracle sweeps from v = 0, the oracle's sweep of V), computed
    once per key and never modified."""
    key = (Na, r, sweeps, N)
    if key not in _cache:
        cal = no.calib_aiyagari(Na=Na, N=N, shocks="rouwenhorst")
        a, s, P = cal["a_grid"], cal["s"], cal["P"]
        w = no.wage(r, 0.36, 0.08)
        V = corc.vfi_solve(np.zeros((N, Na)), a, s, P, r, w, BETA, SIGMA, 1e-5, sweeps)["v_new"]
        _cache[key] = (a, s, P, w, V, corc.vfi_sweep(V, a, s, P, r, w, BETA, SIGMA))
    return _cache[key]


def _prefix(a, s, r, w):
    """The feasible prefix per state (candidates with a_k below cash on hand), as the CPU sees
    it; used only to describe the hints the cases build."""
    coh = (1 + r) * a[None, :] + w * s[:, None]
    return np.searchsorted(a, coh.ravel(), side="left").reshape(coh.shape)


def _tile_spans(h, Na):
    """Per 64-state tile of every row: (max − min) of the hints h, and the same without the
    tile's farthest-out lane."""
    N = h.shape[0]
    nt = (Na + 63) // 64
    hp = np.full((N, nt * 64), -1)
    hp[:, :Na] = h
    hp = hp.reshape(N, nt, 64)
    full = hp[:, :-1] if Na % 64 else hp           # whole tiles only
    srt = np.sort(full, axis=2)
    span = srt[:, :, -1] - srt[:, :, 0]
    span_but_one = np.minimum(srt[:, :, -2] - srt[:, :, 0], srt[:, :, -1] - srt[:, :, 1])
    return span, span_but_one


@pytest.mark.gpu
@pytest.mark.parametrize("variant", VARIANTS)
def test_hints_spread_over_the_row(pkg, gpu, variant):
    """Random hints over the whole row: the lanes of a tile start thousands of candidates
    apart, so no 512-candidate range holds them."""
    Na, r = 2111, 0.03
    a, s, P, w, V, ref = _warm(Na, r, 12)
    rng = np.random.default_rng(5)
    hint = rng.integers(0, Na, (7, Na))
    span, _ = _tile_spans(np.minimum(hint, _prefix(a, s, r, w) - 1), Na)
    # most tiles have lanes outside any 512-candidate range (the poorest states' tiles have a
    # short feasible prefix, which the clamped hints cannot leave)
    assert (span > 512).mean() > 0.5
    _same(_device_sweep(pkg, V, a, s, P, r, w, hint=hint, variant=variant), ref)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", VARIANTS)
def test_one_lane_far_from_its_tile(pkg, gpu, variant):
    """The last argmax as the hint, except one lane per tile (a different lane in each) whose
    hint sits 700 candidates away: 63 lanes fit one 512-candidate range, one does not."""
    Na, r = 2111, 0.03
    a, s, P, w, V, ref = _warm(Na, r, 12)
    hint = ref[1].copy()
    kf = _prefix(a, s, r, w)
    j = np.arange(Na)
    odd = (j % 64) == (j // 64 * 7 + 3) % 64
    far = np.where(hint + 700 < kf, hint + 700, np.maximum(hint - 700, 0))
    hint[:, odd] = far[:, odd]
    assert (hint >= 0).all() and (hint < kf).all()
    span, span_but_one = _tile_spans(hint, Na)
    assert ((span > 512) & (span_but_one < 512)).any()
    _same(_device_sweep(pkg, V, a, s, P, r, w, hint=hint, variant=variant), ref)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("Na,N", [(1601, 7), (2048, 3)])
def test_hints_at_the_ends_and_absent(pkg, gpu, variant, Na, N):
    """Hints of 0, of kf − 1 and past kf (clamped) for every state, −1 in some lanes and in all
    of them; Na = 1,601 leaves a ragged last tile."""
    r = 0.03
    a, s, P, w, V, ref = _warm(Na, r, 12, N)
    kf = _prefix(a, s, r, w)
    rng = np.random.default_rng(Na)
    some = np.where(rng.random((N, Na)) < 0.3, -1, ref[1])
    lanes = ref[1].copy()
    lanes[:, 64:128] = -1                          # a whole tile without hints among hinted ones
    for what, hint in (("zero", np.zeros((N, Na), int)), ("kf-1", np.maximum(kf - 1, 0)),
                       ("past kf", np.full((N, Na), Na - 1)), ("past Na", np.full((N, Na), Na + 50)),
                       ("some -1", some), ("tile -1", lanes), ("all -1", np.full((N, Na), -1))):
        _same(_device_sweep(pkg, V, a, s, P, r, w, hint=hint, variant=variant), ref, what)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", VARIANTS)
def test_tiles_without_a_feasible_candidate(pkg, gpu, variant):
    """r = −0.5 on a grid that starts at a = 10: the low-income rows' first tiles have kf = 0
    (nothing to evaluate, whatever the hint), later tiles a short prefix the hints overshoot."""
    Na = 1700
    cal = no.calib_aiyagari(Na=Na, shocks="rouwenhorst")
    s, P = cal["s"], cal["P"]
    a = np.linspace(10.0, 60.0, Na)
    r, w = -0.5, 1.0
    coh = (1 + r) * a[None, :] + w * s[:, None]
    assert (coh[0, :128] <= a[0]).all() and (coh[0, -1] > a[0])
    V = 0.01 * np.log(a)[None, :] * (1 + 0.1 * np.arange(7))[:, None]
    ref = corc.vfi_sweep(V, a, s, P, r, w, BETA, SIGMA)
    assert np.isnan(ref[0]).any() and np.isfinite(ref[0]).any()
    for what, hint in (("argmax+2", np.clip(ref[1] + 2, 0, Na - 1)), ("zero", np.zeros((7, Na), int)),
                       ("last", np.full((7, Na), Na - 1))):
        _same(_device_sweep(pkg, V, a, s, P, r, w, hint=hint, variant=variant), ref, what)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", VARIANTS)
def test_large_drift_then_two_hinted_sweeps(pkg, gpu, variant):
    """Three sweeps on one workspace at Na = 4,100.  Sweep 1 is hinted with the mirror image of
    its argmax, so the momentum records shifts of both signs up to ≈ ±4,000 (the largest an
    Na = 4,100 row can hold; ±32,767 is out of reach); sweeps 2 and 3 are hinted by the
    previous argmax and extrapolate from those shifts.  Every sweep equals the oracle."""
    Na, r = 4100, 0.04
    a, s, P, w, V, ref = _warm(Na, r, 3)
    hint = (Na - 1) - ref[1]
    assert np.abs(ref[1] - np.minimum(hint, _prefix(a, s, r, w) - 1)).max() > 3000
    ws = pkg.Workspace(7, Na)
    for q in range(3):
        key = ("drift", q)
        if key not in _cache:
            _cache[key] = corc.vfi_sweep(V, a, s, P, r, w, BETA, SIGMA)
        out = _device_sweep(pkg, V, a, s, P, r, w, hint=hint, variant=variant, ws=ws)
        _same(out, _cache[key], f"sweep {q + 1}")
        V, hint = out[0], out[1]


@pytest.mark.gpu
@pytest.mark.parametrize("variant", VARIANTS)
def test_early_sweeps_of_a_solve(pkg, gpu, variant):
    """12 sweeps from v = 0 at Na = 4,100, each hinted by the previous argmax (the first one
    cold): the optimum drifts by tens to thousands of candidates per sweep."""
    Na, r = 4100, 0.04
    cal = no.calib_aiyagari(Na=Na, shocks="rouwenhorst")
    a, s, P = cal["a_grid"], cal["s"], cal["P"]
    w = no.wage(r, 0.36, 0.08)
    ws = pkg.Workspace(7, Na)
    V, hint = np.zeros((7, Na)), None
    for q in range(12):
        key = ("early", q)
        if key not in _cache:
            _cache[key] = corc.vfi_sweep(V, a, s, P, r, w, BETA, SIGMA)
        out = _device_sweep(pkg, V, a, s, P, r, w, hint=hint, variant=variant, ws=ws)
        _same(out, _cache[key], f"sweep {q + 1}")
        V, hint = out[0], out[1]


@pytest.mark.gpu
@pytest.mark.parametrize("variant", VARIANTS)
def test_noisy_value_with_nan_and_inf(pkg, gpu, variant):
    """v not monotone, with NaN and −inf entries, hinted: the climb stops anywhere, and NaN /
    −inf candidates next to the hints merge as in the plain scan."""
    Na, r = 2001, 0.03
    a, s, P, w, V0, ref0 = _warm(Na, r, 25)
    key = ("noisy", Na)
    if key not in _cache:
        rng = np.random.default_rng(41)
        V = V0 + 1e-3 * rng.standard_normal(V0.shape)
        V[rng.random(V.shape) < 0.01] = np.nan
        V[rng.random(V.shape) < 0.01] = -np.inf
        V[2, 300:420] = np.nan                     # a run of NaN candidates across the optima
        _cache[key] = (V, corc.vfi_sweep(V, a, s, P, r, w, BETA, SIGMA))
    V, ref = _cache[key]
    rng = np.random.default_rng(43)
    for what, hint in (("clean argmax", ref0[1]), ("argmax-3", np.clip(ref[1] - 3, 0, Na - 1)),
                       ("random", rng.integers(0, Na, (7, Na)))):
        _same(_device_sweep(pkg, V, a, s, P, r, w, hint=hint, variant=variant), ref, what)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", VARIANTS)
def test_batched_two_rates_hinted(pkg, gpu, variant):
    """One batched sweep of C = 2 rates with a starting hint equals the two single-rate sweeps
    (the oracle's) of the same value function."""
    import torch
    Na = 1601
    a, s, P, w3, V, ref3 = _warm(Na, 0.03, 12)
    rs = [0.03, 0.01]
    w = [w3, no.wage(0.01, 0.36, 0.08)]
    key = ("batch", Na)
    if key not in _cache:
        _cache[key] = [ref3, corc.vfi_sweep(V, a, s, P, rs[1], w[1], BETA, SIGMA)]
    refs = _cache[key]
    dev = torch.device("cuda:0")
    t = lambda x: torch.as_tensor(np.ascontiguousarray(x), device=dev)
    ws = pkg.Workspace(7, Na)
    ws.set_variant(variant)
    va = t(np.broadcast_to(V, (2, 7, Na)).copy())
    vb = torch.zeros_like(va)
    hint = np.stack([np.clip(refs[0][1] + 40, 0, Na - 1), np.clip(refs[1][1] - 40, 0, Na - 1)])
    idx = t(hint.astype(np.int32))
    pk, pc = torch.zeros_like(va), torch.zeros_like(va)
    it, which = pkg.vfi.solve_batch_dev(ws, rs, w, va, vb, t(a), t(s), t(P), BETA, SIGMA, 1e-5, 1,
                                        idx, pk, pc, use_hint=True)
    torch.cuda.synchronize()
    assert it == [1, 1]
    for c in range(2):
        vn = (vb if which[c] else va)[c].cpu().numpy()
        _same((vn, idx[c].cpu().numpy(), pk[c].cpu().numpy(), pc[c].cpu().numpy()), refs[c], c)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [16, 16 | 3 << 7, 4100])
def test_labour_hints_on_every_level(pkg, gpu, variant):
    """A3 (Nl = 10): the hint's labour level picks the feasible prefix the start-up clamps into.
    Two cold sweeps from v = 0, then a sweep hinted by the last argmax — whose levels cover the
    whole labour grid — against the oracle; with the three-slot and the generic window, and the
    small-grid tree default (four cooperating waves)."""
    import torch
    Na = 1601
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
            levels = np.unique((lin.cpu().numpy() - 1) % 10)
            assert len(levels) >= 3 and levels.max() > 0   # hints on levels other than 0
        ws.labor_vfi_sweep(v[cur], a_t, s_t, P_t, L_t, r, w, BETA, SIGMA, 1.0, 2.0, v[1 - cur], lin,
                           pk, pl, pc, hint=None if q < 2 else lin)
        cur = 1 - cur
    torch.cuda.synchronize()
    key = ("labour", Na)
    if key not in _cache:
        _cache[key] = corc.labor_vfi_sweep(V, a, s, P, L, r, w, BETA, SIGMA, 1.0, 2.0)
    vo, (pko, plo, pco, lino) = _cache[key]
    assert np.array_equal(v[cur].cpu().numpy(), vo)
    assert np.array_equal(lin.cpu().numpy(), lino)
    assert np.array_equal(pk.cpu().numpy(), pko) and np.array_equal(pl.cpu().numpy(), plo)
    assert np.array_equal(pc.cpu().numpy(), pco)
