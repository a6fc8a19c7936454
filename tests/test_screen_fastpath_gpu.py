"""The tree screen's clamp fast path: a block of eight candidates that
lies below the wave's smallest feasible prefix is screened without the clamp max(c, 0), which is
the identity there.  Nothing here is a new bound: with the fast path on (the default) and off
(variant bit 22) the sweep must give the same outputs AND the same work counters — the same
passes block by block — and both must equal the exhaustive scan (mode 2) and the C oracle bit
for bit.  The shapes are the smallest at which the path can go wrong: ragged last tiles, blocks
and superblocks that straddle the smallest prefix and the feasible range, one and several
superblocks; the inputs put feasibility edges inside the searched blocks (small income), make
passes occur in many blocks (noisy v, cold starts) and move the bars between sweeps (chains).
Each test asserts on the instrumented build that both bodies ran."""
import numpy as np
import pytest

from oracle import corc
from oracle import np_oracle as no

PLAIN = 1 << 22                                             # every screen keeps the clamp
W1 = 0                                                      # one wave per tile (tree defaults)
HL = 16 | 2048 | 1 << 16 | 1 << 21 | 1 << 23 | 1 << 24      # the large-grid default (packed)
D2 = 2 | 4096                                               # two waves, dealt 8-blocks
NAS = (65, 100, 513, 577, 1601)


class _Runner:
    """One workspace per (fast path on / off) × (production / instrumented build), so that a
    chain's momentum history is the same in all four."""

    def __init__(self, pkg, N, Na, variant):
        self.pkg, self.N, self.Na = pkg, N, Na
        self.ws = {}
        for plain in (False, True):
            for count in (False, True):
                ws = pkg.Workspace(N, Na)
                ws.set_variant(variant | (PLAIN if plain else 0))
                if count:
                    ws.set_timing(False, count=True)
                self.ws[plain, count] = ws
        self.ex = pkg.Workspace(N, Na)

    def sweep(self, ws, V, a, s, P, r, w, sigma, hint, mode=1):
        import torch
        dev = torch.device("cuda:0")
        t = lambda x: torch.as_tensor(np.ascontiguousarray(x), device=dev)
        vo, at, st, Pt = t(V), t(a), t(s), t(P)
        vn = torch.empty_like(vo); pk = torch.empty_like(vo); pc = torch.empty_like(vo)
        idx = torch.empty(V.shape, dtype=torch.int32, device=dev)
        ht = None if hint is None else t(hint.astype(np.int32))
        ws.vfi_sweep(vo, at, st, Pt, r, w, 0.96, sigma, vn, idx, pk, pc, hint=ht, mode=mode)
        torch.cuda.synchronize()
        return vn.cpu().numpy(), idx.cpu().numpy(), pk.cpu().numpy(), pc.cpu().numpy()

    def check(self, V, a, s, P, r, w, sigma, hint, ref):
        """All four builds against `ref`; returns the fast build's per-body block counts."""
        args = (V, a, s, P, r, w, sigma, hint)
        before = {p: (self.ws[p, True].counters(), self.ws[p, True].screen_paths())
                  for p in (False, True)}
        out = {k: self.sweep(ws, *args) for k, ws in self.ws.items()}
        for k, o in out.items():
            _same(o, ref, f"plain={k[0]} counted={k[1]}")
        delta = {}
        for p in (False, True):
            c, q = self.ws[p, True].counters(), self.ws[p, True].screen_paths()
            delta[p] = (tuple(x - y for x, y in zip(c, before[p][0])),
                        tuple(x - y for x, y in zip(q, before[p][1])))
        print("counters", delta[False][0], "paths", delta[False][1])
        assert delta[False][0] == delta[True][0], "work counters differ between the bodies"
        assert sum(delta[False][1]) == sum(delta[True][1]), "fine-screen blocks differ"
        assert delta[True][1][1] == 0, "the forcing bit left the fast body on"
        return np.array(delta[False][1])

    def exhaustive(self, V, a, s, P, r, w, sigma, ref):
        _same(self.sweep(self.ex, V, a, s, P, r, w, sigma, None, mode=2), ref, "mode 2")


def _same(out, ref, what):
    for name, x, y in zip(("v_new", "idx", "policy_k", "policy_c"), out, ref):
        assert np.array_equal(x, y, equal_nan=x.dtype.kind == "f"), (what, name)


def _covered(paths):
    """Both the unclamped and the clamped body screened blocks."""
    print("blocks (with the clamp, without it):", paths)
    assert paths[1] > 0, "the unclamped body never ran"
    assert paths[0] > 0, "the clamped body never ran"


_cache = {}


def _warm(Na, r, sweeps, sigma=5.0, N=7, w=None):
    """(a, s, P, w, V after `sweeps` oracle sweeps from v = 0), computed once per key and left
    unchanged."""
    key = (Na, r, sweeps, sigma, N, w)
    if key not in _cache:
        cal = no.calib_aiyagari(Na=Na, shocks="rouwenhorst", N=N)
        a, s, P = cal["a_grid"], cal["s"], cal["P"]
        w_ = no.wage(r, 0.36, 0.08) if w is None else w
        V = corc.vfi_solve(np.zeros((N, Na)), a, s, P, r, w_, 0.96, sigma, 1e-5, sweeps)["v_new"]
        _cache[key] = (a, s, P, w_, V)
    return _cache[key]


def _cold_and_hinted(run, V, a, s, P, r, w, sigma, shift):
    ref = corc.vfi_sweep(V, a, s, P, r, w, 0.96, sigma)
    run.exhaustive(V, a, s, P, r, w, sigma, ref)
    Na = V.shape[1]
    paths = np.zeros(2, dtype=np.int64)
    for hint in (None, np.clip(ref[1] + shift, 0, Na - 1)):
        paths += run.check(V, a, s, P, r, w, sigma, hint, ref)
    return paths


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [W1, HL, D2])
@pytest.mark.parametrize("N", [2, 7])
def test_shapes(pkg, gpu, N, variant):
    """Na = 65 … 1601 (one valid lane in the last tile at 65, 513, 577 and 1601; one, two and
    four superblocks), r = 0.04 and r = −0.05 (the smallest prefix is not in lane 0's state
    order by construction there: kfmin is a reduction).  Smooth v, cold and hinted."""
    paths = np.zeros(2, dtype=np.int64)
    for Na in NAS:
        run = _Runner(pkg, N, Na, variant)
        for r in (0.04, -0.05):
            a, s, P, w, V = _warm(Na, r, 8, N=N)
            paths += _cold_and_hinted(run, V, a, s, P, r, w, 5.0, -3)
    _covered(paths)


@pytest.mark.gpu
@pytest.mark.parametrize("sigma", [2.0, 3.0, 5.0])
@pytest.mark.parametrize("variant", [W1, HL, D2])
def test_sigmas(pkg, gpu, sigma, variant):
    """σ = 2, 3, 5: screen exponents n = 1, 2, 4 (odd and even; for even n the unclamped power
    of a negative difference is positive, so a wrong fast-path condition shows as extra passes —
    in the counters even where the exact re-test hides it from the outputs)."""
    paths = np.zeros(2, dtype=np.int64)
    for Na in (100, 577, 1601):
        run = _Runner(pkg, 7, Na, variant)
        for r in (0.04, -0.05):
            a, s, P, w, V = _warm(Na, r, 8, sigma=sigma)
            paths += _cold_and_hinted(run, V, a, s, P, r, w, sigma, 4)
    _covered(paths)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [W1, HL, D2])
def test_small_income(pkg, gpu, variant):
    """w·s small (w = 0.02): consumption is a few grid steps, so the optimum sits next to the
    feasibility edge and the searched blocks hold it — the clamped body is taken, and blocks
    and superblocks straddle kfmin."""
    paths = np.zeros(2, dtype=np.int64)
    for Na in NAS:
        run = _Runner(pkg, 7, Na, variant)
        for r in (0.04, -0.05):
            a, s, P, w, V = _warm(Na, r, 8, w=0.02)
            paths += _cold_and_hinted(run, V, a, s, P, r, w, 5.0, 1)
    _covered(paths)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [W1, HL, D2])
def test_noisy_value(pkg, gpu, variant):
    """v not monotone in a: passes in many blocks, bars that differ from lane to lane, argmaxes
    scattered over the blocks.  Random hints, hints of −1 and a cold start."""
    rng = np.random.default_rng(31)
    paths = np.zeros(2, dtype=np.int64)
    for Na, scale in ((577, 1.0), (1601, 1e-3), (1601, 1.0)):
        run = _Runner(pkg, 7, Na, variant)
        a, s, P, w, V = _warm(Na, 0.04, 8)
        V = V + scale * rng.standard_normal(V.shape)
        ref = corc.vfi_sweep(V, a, s, P, 0.04, w, 0.96, 5.0)
        run.exhaustive(V, a, s, P, 0.04, w, 5.0, ref)
        for hint in (None, rng.integers(0, Na, (7, Na)), np.full((7, Na), -1)):
            paths += run.check(V, a, s, P, 0.04, w, 5.0, hint, ref)
    _covered(paths)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [W1, HL, D2])
def test_chained_hinted_sweeps(pkg, gpu, variant):
    """A cold sweep from v = 0, then five chained hinted sweeps on the same workspaces: the
    optimum drifts, the exact paths raise bars inside a block after its body was chosen, and
    the argmax moves between blocks from sweep to sweep."""
    paths = np.zeros(2, dtype=np.int64)
    for Na in (577, 1601):
        cal = no.calib_aiyagari(Na=Na, shocks="rouwenhorst")
        a, s, P = cal["a_grid"], cal["s"], cal["P"]
        w = no.wage(0.04, 0.36, 0.08)
        run = _Runner(pkg, 7, Na, variant)
        V, hint = np.zeros((7, Na)), None
        for q in range(6):
            if ("chain", Na, q) not in _cache:  # (the oracle's sweeps do not depend on the variant)
                _cache["chain", Na, q] = corc.vfi_sweep(V, a, s, P, 0.04, w, 0.96, 5.0)
            ref = _cache["chain", Na, q]
            paths += run.check(V, a, s, P, 0.04, w, 5.0, hint, ref)
            V, hint = ref[0], ref[1]
    _covered(paths)
