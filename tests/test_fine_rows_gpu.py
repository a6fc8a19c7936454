"""The tree kernel's group walk in 32-bit windows: the passing blocks of
a superblock are walked in windows of 32 from the lowest one left, every group's mask one word
per window — work order and address arithmetic only.  The tree path (an explicit variant, so the
small-grid one-launch sweep is not picked) against the C oracle bit for bit — v_new, idx and
both policies — through the one-wave tree, the packed launch and a two-wave geometry (which
keeps the union walk: the same inputs through the neighbouring body), at shapes where an address
or a walk can go wrong: a ragged last tile with seven all-invalid groups, more than eight
superblocks (windows that start in either half of the mask), passing blocks far apart (two
windows, groups that have a block in only one of them), whole superblocks passing; and the four
work counters against the parent's."""
import numpy as np
import pytest

from oracle import corc
from oracle import np_oracle as no

W1 = 0                                                      # one wave per tile: the group walk
HL = 16 | 2048 | 1 << 16 | 1 << 21 | 1 << 23 | 1 << 24      # the large-grid default (packed)
W2 = 2                                                      # two cooperating waves per tile
GEOS = [W1, HL, W2]
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


def _calib(Na, N):
    if ("cal", Na, N) not in _cache:
        cal = no.calib_aiyagari(Na=Na, shocks="rouwenhorst", N=N)
        _cache["cal", Na, N] = (cal["a_grid"], cal["s"], cal["P"])
    return _cache["cal", Na, N]


def _chain(Na, r, sigma=5.0, N=7, sweeps=6):
    """The oracle's sweeps from v = 0 (sweep q + 1 from sweep q's v_new), computed once per key
    and left unchanged."""
    key = ("chain", Na, r, sigma, N)
    if key not in _cache:
        a, s, P = _calib(Na, N)
        w = no.wage(r, 0.36, 0.08)
        V, refs = np.zeros((N, Na)), []
        for _ in range(sweeps):
            refs.append(corc.vfi_sweep(V, a, s, P, r, w, BETA, sigma))
            V = refs[-1][0]
        _cache[key] = (a, s, P, w, refs)
    return _cache[key]


def _run_chain(pkg, variant, Na, r, sigma=5.0, N=7):
    """A cold sweep from v = 0 and five chained hinted sweeps on one workspace."""
    a, s, P, w, refs = _chain(Na, r, sigma, N)
    ws = pkg.Workspace(N, Na)
    V, hint = np.zeros((N, Na)), None
    for q, ref in enumerate(refs):
        out = _device_sweep(pkg, V, a, s, P, r, w, hint=hint, variant=variant, ws=ws, sigma=sigma)
        _same(out, ref, (Na, r, sigma, N, variant, q))
        V, hint = out[0], out[1]


@pytest.mark.gpu
@pytest.mark.parametrize("Na", [1601, 2111, 4100])
@pytest.mark.parametrize("variant", GEOS)
def test_chained_sweeps(pkg, gpu, Na, variant):
    """Na = 1601: the last tile holds one valid lane (seven groups without one); 2111: 63; 4100:
    nine superblocks of 64 blocks, so a window starts at any block of the mask, in either half,
    and the cold sweep walks whole superblocks in two windows."""
    _run_chain(pkg, variant, Na, 0.03)


@pytest.mark.gpu
@pytest.mark.parametrize("sigma,N", [(2.0, 7), (3.0, 7), (5.0, 2), (2.0, 2)])
@pytest.mark.parametrize("variant", GEOS)
def test_sigmas_and_shocks(pkg, gpu, sigma, N, variant):
    """σ = 2, 3 (the generic body; σ = 5 is every other test here) and N = 2."""
    _run_chain(pkg, variant, 1601, 0.03, sigma=sigma, N=N)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", GEOS)
def test_negative_rate(pkg, gpu, variant):
    _run_chain(pkg, variant, 2111, -0.02)


def _noisy(Na, scale):
    """The oracle's v after five sweeps plus seeded noise: near ties and rows that are no longer
    monotone, so a state's passing blocks lie far apart."""
    if ("noisy", Na, scale) not in _cache:
        a, s, P, w, refs = _chain(Na, 0.03)
        rng = np.random.default_rng(1609)
        V = refs[4][0] + scale * rng.standard_normal(refs[4][0].shape)
        _cache["noisy", Na, scale] = (V, corc.vfi_sweep(V, a, s, P, 0.03, w, BETA, 5.0))
    return _cache["noisy", Na, scale]


@pytest.mark.gpu
@pytest.mark.parametrize("scale", [1e-9, 1e-3, 1.0])
@pytest.mark.parametrize("variant", GEOS)
def test_noisy_value_function(pkg, gpu, variant, scale):
    """Noise of 1e-9 (near ties), and of 1e-3 and 1 (optima and passing blocks scattered over the
    whole feasible range: both halves of a superblock, so two windows, groups with blocks in
    only one of them, and groups on different blocks in every trip): hinted by the argmax of
    the smooth v, by −1 everywhere and cold."""
    Na = 4100
    a, s, P, w, refs = _chain(Na, 0.03)
    V, ref = _noisy(Na, scale)
    for hint in (refs[4][1], np.full((7, Na), -1), None):
        _same(_device_sweep(pkg, V, a, s, P, 0.03, w, hint=hint, variant=variant), ref)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", GEOS)
def test_cold_sweeps(pkg, gpu, variant):
    """No hint (the init kernel's bar) and hint = −1 everywhere (every bar −inf at the
    confirmation: whole superblocks pass, two windows of 32 trips each)."""
    Na = 4100
    a, s, P, w, refs = _chain(Na, 0.03)
    V, ref = refs[4][0], refs[5]
    for hint in (None, np.full((7, Na), -1)):
        _same(_device_sweep(pkg, V, a, s, P, 0.03, w, hint=hint, variant=variant), ref)


# (exact, superblock, block, candidate) of the sweep below on the parent build (the group walk
# with the 64-bit bit walk), variant 0, instrumented build: the figures
# recorded from that build's run of the same sweep (profiles/r15_group_fine_ab.txt, "G=8")
PARENT_COUNTS = (153267, 14784, 320128, 667072)


@pytest.mark.gpu
def test_work_counters_equal_the_parents(pkg, gpu):
    """Na = 2111, one hinted sweep (hint = the oracle's argmax − 5) of v after twelve oracle
    sweeps, variant 0 on the instrumented build: the walk is address arithmetic and work order
    only, and every superblock of this sweep fits one window, so exact evaluations, superblock
    tests, block tests and candidates screened are the parent's to the last one."""
    Na = 2111
    a, s, P = _calib(Na, 7)
    w = no.wage(0.03, 0.36, 0.08)
    V = corc.vfi_solve(np.zeros((7, Na)), a, s, P, 0.03, w, BETA, 5.0, 1e-5, 12)["v_new"]
    ref = corc.vfi_sweep(V, a, s, P, 0.03, w, BETA, 5.0)
    ws = pkg.Workspace(7, Na)
    ws.set_timing(False, count=True)
    before = ws.counters()
    _same(_device_sweep(pkg, V, a, s, P, 0.03, w, hint=np.clip(ref[1] - 5, 0, Na - 1), variant=W1,
                        ws=ws), ref)
    got = tuple(x - y for x, y in zip(ws.counters(), before))
    print("(exact, superblock, block, candidate):", got, "parent", PARENT_COUNTS)
    assert got == PARENT_COUNTS
