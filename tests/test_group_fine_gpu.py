"""The tree kernel's fine screens walked per 8-lane group: each group
of eight consecutive lanes walks the 8-blocks its own lanes passed in the confirmation, the
groups in lockstep, instead of every lane walking the wave's union.  The tree path (an explicit
variant, so the small-grid one-launch sweep is not picked) against the C oracle bit for bit —
v_new, idx and both policies — at the smallest shapes where the walk can go wrong: groups without
a valid lane beside a group with one, groups on far-apart blocks and in different superblocks in
one trip, special values and infeasible tiles, trips whose groups screen blocks on both sides
of the smallest feasible prefix, the other σ and N, chained sweeps, the batched sweep, and the
work counters (exact evaluations, superblock tests and block tests equal to the union walk's
recorded counts, candidates screened strictly fewer; exact evaluations equal to the one-wave
two-states-per-lane union walk's)."""
import numpy as np
import pytest

from oracle import corc
from oracle import np_oracle as no

W1 = 0                                                      # one wave per tile: the group walk
R2 = 1                                                      # two states per lane: the union walk
HL = 16 | 2048 | 1 << 16 | 1 << 21 | 1 << 23 | 1 << 24      # the large-grid default (packed)
PLAIN = 1 << 22                                             # every screen keeps the clamp
BETA = 0.96


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
    ws.vfi_sweep(vo, at, st, Pt, r, w, BETA, sigma, vn, idx, pk, pc, hint=ht, mode=1)
    torch.cuda.synchronize()
    return vn.cpu().numpy(), idx.cpu().numpy(), pk.cpu().numpy(), pc.cpu().numpy()


def _same(out, ref, what=""):
    for name, x, y in zip(("v_new", "idx", "policy_k", "policy_c"), out, ref):
        assert np.array_equal(x, y, equal_nan=x.dtype.kind == "f"), (what, name)


_cache = {}


def _warm(Na, r, sweeps, sigma=5.0, N=7, w=None):
    """(a, s, P, w, V after `sweeps` oracle sweeps from v = 0, the oracle's next sweep), computed
    once per key and left unchanged."""
    key = (Na, r, sweeps, sigma, N, w)
    if key not in _cache:
        cal = no.calib_aiyagari(Na=Na, shocks="rouwenhorst", N=N)
        a, s, P = cal["a_grid"], cal["s"], cal["P"]
        w_ = no.wage(r, 0.36, 0.08) if w is None else w
        V = corc.vfi_solve(np.zeros((N, Na)), a, s, P, r, w_, BETA, sigma, 1e-5, sweeps)["v_new"]
        ref = corc.vfi_sweep(V, a, s, P, r, w_, BETA, sigma)
        _cache[key] = (a, s, P, w_, V, ref)
    return _cache[key]


@pytest.mark.gpu
@pytest.mark.parametrize("Na", [1601, 1609, 2111])
@pytest.mark.parametrize("variant", [W1, HL])
def test_ragged_last_tile(pkg, gpu, Na, variant):
    """The last tile holds 1 valid lane (Na = 1601: seven groups with an empty mask and NaN bars
    beside a group with one lane), 9 (Na = 1609) or 63 (Na = 2111).  Cold and hinted."""
    a, s, P, w, V, ref = _warm(Na, 0.03, 12)
    for hint in (None, np.clip(ref[1] - 5, 0, Na - 1)):
        _same(_device_sweep(pkg, V, a, s, P, 0.03, w, hint=hint, variant=variant), ref)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [W1, HL])
def test_groups_on_far_apart_blocks(pkg, gpu, variant):
    """v plus noise: the optima of one wave's groups lie in different 64-blocks and different
    superblocks, so one trip screens far-apart blocks, and a group has no block in a superblock
    where another has many.  Random hints, hint = −1 everywhere and cold."""
    rng = np.random.default_rng(41)
    for Na, scale in ((2001, 1e-3), (2001, 1.0), (1601, 1e-3), (1601, 1.0)):
        a, s, P, w, V, _ = _warm(Na, 0.03, 25 if Na == 2001 else 12)
        V = V + scale * rng.standard_normal(V.shape)
        ref = corc.vfi_sweep(V, a, s, P, 0.03, w, BETA, 5.0)
        for hint in (rng.integers(0, Na, (7, Na)), np.full((7, Na), -1), None):
            _same(_device_sweep(pkg, V, a, s, P, 0.03, w, hint=hint, variant=variant), ref,
                  (Na, scale))


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [W1, HL])
def test_special_values_and_infeasible_tiles(pkg, gpu, variant):
    """NaN and −inf entries in v and a whole 8-block of −inf, on the grid from a = 10 with
    r = −0.5: tiles without a feasible candidate, feasible ranges that end inside an 8-block
    and inside a 64-block (the per-lane cut to the range)."""
    Na = 1700
    cal = no.calib_aiyagari(Na=Na, shocks="rouwenhorst")
    s, P = cal["s"], cal["P"]
    a = np.linspace(10.0, 60.0, Na)
    r, w = -0.5, 1.0
    coh = (1 + r) * a[None, :] + w * s[:, None]
    kf = (a[None, None, :] < coh[:, :, None]).sum(axis=2)
    kg = np.array([kf[:, j:j + 64].max(axis=1) for j in range(0, Na, 64)])
    assert (kg == 0).any() and (kg % 8 != 0).any() and (kg % 64 != 0).any()
    V = 0.01 * np.log(a)[None, :] * (1 + 0.1 * np.arange(7))[:, None]
    V[3, [3, 700]] = np.nan
    V[2, 40:45] = -np.inf
    V[5, 1200] = -np.inf
    V[6, 512:520] = -np.inf
    ref = corc.vfi_sweep(V, a, s, P, r, w, BETA, 5.0)
    assert np.isnan(ref[0]).any() and np.isfinite(ref[0]).any() and ref[1].max() > 512
    for hint in (None, np.clip(ref[1] + 2, 0, Na - 1)):
        _same(_device_sweep(pkg, V, a, s, P, r, w, hint=hint, variant=variant), ref)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [W1, HL])
def test_mixed_fast_path_trips(pkg, gpu, variant):
    """Small income (w = 0.02), cold and hinted: the optimum sits next to the feasibility edge, so
    the groups of one trip screen blocks on both sides of the wave's smallest prefix.  The body
    is chosen once per superblock (from its highest passing block), so such a trip runs the
    clamped body as a whole; superblocks that end below the prefix run the unclamped one.  The
    test shows that both bodies ran in the sweep, and that the outputs equal the oracle's with
    and without the forcing bit."""
    Na = 1700
    a, s, P, w, V, ref = _warm(Na, 0.04, 8, w=0.02)
    ws = pkg.Workspace(7, Na)
    ws.set_timing(False, count=True)
    before = ws.screen_paths()
    for hint in (None, np.clip(ref[1] + 1, 0, Na - 1)):
        _same(_device_sweep(pkg, V, a, s, P, 0.04, w, hint=hint, variant=variant, ws=ws), ref)
    paths = tuple(x - y for x, y in zip(ws.screen_paths(), before))
    print("trips (with the clamp, without it):", paths)
    assert paths[0] > 0 and paths[1] > 0
    for hint in (None, np.clip(ref[1] + 1, 0, Na - 1)):
        _same(_device_sweep(pkg, V, a, s, P, 0.04, w, hint=hint, variant=variant | PLAIN), ref)


@pytest.mark.gpu
@pytest.mark.parametrize("sigma,N", [(2.0, 7), (3.0, 7), (5.0, 7), (5.0, 2)])
@pytest.mark.parametrize("variant", [W1, HL])
def test_sigmas_and_shocks(pkg, gpu, sigma, N, variant):
    """σ = 2, 3 (the generic body) and 5; N = 2.  Cold and hinted."""
    Na = 1609
    a, s, P, w, V, ref = _warm(Na, 0.03, 12, sigma=sigma, N=N)
    for hint in (None, np.clip(ref[1] - 4, 0, Na - 1)):
        _same(_device_sweep(pkg, V, a, s, P, 0.03, w, hint=hint, variant=variant, sigma=sigma),
              ref)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [W1, HL])
def test_chained_hinted_sweeps(pkg, gpu, variant):
    """A cold sweep from v = 0 and five chained hinted sweeps on one workspace at Na = 1601:
    stale group bars, the drift predictor, bars raised inside a trip."""
    Na = 1601
    cal = no.calib_aiyagari(Na=Na, shocks="rouwenhorst")
    a, s, P = cal["a_grid"], cal["s"], cal["P"]
    w = no.wage(0.04, 0.36, 0.08)
    ws = pkg.Workspace(7, Na)
    V, hint = np.zeros((7, Na)), None
    for q in range(6):
        if ("chain", q) not in _cache:     # (the oracle's sweeps do not depend on the variant)
            _cache[("chain", q)] = corc.vfi_sweep(V, a, s, P, 0.04, w, BETA, 5.0)
        out = _device_sweep(pkg, V, a, s, P, 0.04, w, hint=hint, variant=variant, ws=ws)
        _same(out, _cache[("chain", q)], q)
        V, hint = out[0], out[1]


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [W1, HL])
def test_batched_two_rates(pkg, gpu, variant):
    """One batched sweep of two rates at Na = 1700 through the multi-rate entry point, against
    the oracle per rate."""
    import torch
    Na = 1700
    a, s, P, w3, V, ref3 = _warm(Na, 0.03, 12)
    rs = [0.03, 0.01]
    w = [w3, no.wage(0.01, 0.36, 0.08)]
    if ("batch", Na) not in _cache:
        _cache["batch", Na] = [ref3, corc.vfi_sweep(V, a, s, P, rs[1], w[1], BETA, 5.0)]
    refs = _cache["batch", Na]
    dev = torch.device("cuda:0")
    t = lambda x: torch.as_tensor(np.ascontiguousarray(x), device=dev)
    ws = pkg.Workspace(7, Na)
    ws.set_variant(variant)
    va = t(np.broadcast_to(V, (2, 7, Na)).copy())
    vb = torch.zeros_like(va)
    hint = np.stack([np.clip(refs[0][1] + 40, 0, Na - 1), np.clip(refs[1][1] - 40, 0, Na - 1)])
    idx = t(hint.astype(np.int32))
    pk, pc = torch.zeros_like(va), torch.zeros_like(va)
    it, which = pkg.vfi.solve_batch_dev(ws, rs, w, va, vb, t(a), t(s), t(P), BETA, 5.0, 1e-5, 1,
                                        idx, pk, pc, use_hint=True)
    torch.cuda.synchronize()
    assert it == [1, 1]
    for c in range(2):
        vn = (vb if which[c] else va)[c].cpu().numpy()
        _same((vn, idx[c].cpu().numpy(), pk[c].cpu().numpy(), pc[c].cpu().numpy()), refs[c], c)


@pytest.mark.gpu
def test_work_counters(pkg, gpu):
    """Na = 2111 on the instrumented build, hint = −1 everywhere (no start-up, so every exact
    evaluation is the walk's, and every tile takes its superblocks in ascending order whatever
    its shape): the
    group walk (one state per lane) and the union walk on one wave (two states per lane, 128-
    state tiles) make the same exact evaluations — a state's sequence of evaluations depends
    only on its own passing blocks and its own bar, not on the tile it shares — and the group
    walk screens no more candidates per state.  The superblock and block counters are per tile
    and differ with the tile width, so they are not compared here (two cooperating waves repeat
    the start-up and count it twice, so that geometry does not run the same set either)."""
    Na = 2111
    a, s, P, w, V, ref = _warm(Na, 0.03, 12)
    got = {}
    for variant in (W1, R2):
        ws = pkg.Workspace(7, Na)
        ws.set_timing(False, count=True)
        before = ws.counters()
        _same(_device_sweep(pkg, V, a, s, P, 0.03, w, hint=np.full((7, Na), -1), variant=variant,
                            ws=ws), ref)
        got[variant] = tuple(x - y for x, y in zip(ws.counters(), before))
    print("(exact, superblock, block, candidate): group walk", got[W1], "union walk", got[R2])
    assert got[W1][0] > 7 * Na
    assert got[W1][0] == got[R2][0], "exact evaluations differ: the walk dropped or reordered one"
    assert 0 < got[W1][3] <= got[R2][3], "the group walk screened more candidates than the union"


# (exact, superblock, block, candidate) of the sweep below as the union walk made it: recorded
# from the build before the group walk (the same sources with the 64-lane union walked by
# every lane), variant 0, on the instrumented build
UNION_WALK_COUNTS = (153267, 14784, 320128, 1284032)


@pytest.mark.gpu
def test_work_counters_against_the_union_walk(pkg, gpu):
    """Na = 2111, hinted (hint = the oracle's argmax − 5: finite bars at the confirmation, so the
    groups' masks differ), variant 0, on the instrumented build, against the counts recorded
    from the union walk on the same tiles: the exact evaluations, the superblock tests and the
    block tests have not moved at all, and the candidates screened are strictly fewer."""
    Na = 2111
    a, s, P, w, V, ref = _warm(Na, 0.03, 12)
    ws = pkg.Workspace(7, Na)
    ws.set_timing(False, count=True)
    before = ws.counters()
    _same(_device_sweep(pkg, V, a, s, P, 0.03, w, hint=np.clip(ref[1] - 5, 0, Na - 1), variant=W1,
                        ws=ws), ref)
    got = tuple(x - y for x, y in zip(ws.counters(), before))
    print("(exact, superblock, block, candidate): hinted", got, "union walk", UNION_WALK_COUNTS)
    assert got[:3] == UNION_WALK_COUNTS[:3], "exact, superblock or block tests moved"
    assert 0 < got[3] < UNION_WALK_COUNTS[3], "the group walk screened no fewer candidates"
