"""GPU: the batched Krusell-Smith VFI solve (ks_vfi_solve_batch, one workgroup per economy)
against ks_vfi_solve called alone and the C oracle — value, k_opt, iters and rel_diff bit for bit
— under every thread-count instantiation, through the host tier and the device tier."""
import numpy as np
import pytest

from tests import ks_vfi_batch_cases as vc

pytestmark = pytest.mark.gpu

KNOB = "AIY_KS_VFI_BATCH_THREADS"      # the A/B tool's geometry knob (csrc/ks_vfi_batch_host.cpp)
SOLVES = [(50, 1e-6, 200),             # full convergence, the candidates stop at different times
          (3, 0.0, 1),                 # a single iteration
          (2, 0.0, 6)]                 # the cap reached on the second improvement iteration


def _eq(a, b):
    return a == b or (np.isnan(a) and np.isnan(b))


def _kw(howard, tol, max_vfi):
    return dict(howard_steps=howard, tol=tol, max_vfi=max_vfi)


def _batch(pkg, I, order, V0s, k0s, B, **kw):
    return pkg.ks_vfi_solve_batch(np.stack(V0s), np.stack(k0s), I["k_grid"], I["K_grid"][order],
                                  B, I["P"][order], I["prm"][order], **kw)


def _solo(pkg, I, e, V0, k0, B, **kw):
    return pkg.ks_vfi_solve(V0, k0, I["k_grid"], I["K_grid"][e], B, I["P"][e], I["prm"][e], **kw)


def _same(R, c, S):
    assert R["iters"][c] == S["iters"], (c, R["iters"][c], S["iters"])
    assert _eq(R["rel_diff"][c], S["rel_diff"]), (c, R["rel_diff"][c], S["rel_diff"])
    assert np.array_equal(R["value"][c], S["value"], equal_nan=True), c
    assert np.array_equal(R["k_opt"][c], S["k_opt"], equal_nan=True), c


def _same_batch(R, Q):
    assert np.array_equal(R["iters"], Q["iters"])
    assert np.array_equal(R["rel_diff"], Q["rel_diff"], equal_nan=True)
    assert np.array_equal(R["value"], Q["value"], equal_nan=True)
    assert np.array_equal(R["k_opt"], Q["k_opt"], equal_nan=True)


def _cold(pkg, I, order, B, **kw):
    return _batch(pkg, I, order, [I["V0"][e] for e in order], [I["k0"]] * len(order), B, **kw)


@pytest.mark.parametrize("howard,tol,max_vfi", SOLVES)
@pytest.mark.parametrize("B", [vc.B_IDENTITY, vc.B_SHIFT])
def test_batch_equals_single_calls_and_the_oracle(pkg, gpu, B, howard, tol, max_vfi):
    I = vc.inputs(pkg)
    R = _cold(pkg, I, [0, 1, 2], B, **_kw(howard, tol, max_vfi))
    for e in range(3):
        _same(R, e, _solo(pkg, I, e, I["V0"][e], I["k0"], B, **_kw(howard, tol, max_vfi)))
        _same(R, e, vc.oracle_cold(pkg, e, B, howard, tol, max_vfi))
    if max_vfi == 200:
        assert len(set(R["iters"].tolist())) == 3 and R["iters"].max() < 200
    else:
        assert R["iters"].tolist() == [max_vfi] * 3


@pytest.mark.parametrize("e", [0, 1, 2])
def test_one_candidate(pkg, gpu, e):
    I = vc.inputs(pkg)
    R = _cold(pkg, I, [e], vc.B_SHIFT, **_kw(50, 1e-6, 200))
    assert R["value"].shape == (1,) + I["k0"].shape
    _same(R, 0, vc.oracle_cold(pkg, e, vc.B_SHIFT))
    _same(R, 0, _solo(pkg, I, e, I["V0"][e], I["k0"], vc.B_SHIFT, **_kw(50, 1e-6, 200)))


def test_permuted_candidates_give_permuted_results(pkg, gpu):
    I = vc.inputs(pkg)
    perm = [2, 0, 1]
    Rp = _cold(pkg, I, perm, vc.B_SHIFT, **_kw(50, 1e-6, 200))
    for c, e in enumerate(perm):
        _same(Rp, c, vc.oracle_cold(pkg, e, vc.B_SHIFT))


@pytest.mark.parametrize("threads", [1024, 512, 256])
def test_every_geometry_gives_the_same_results(pkg, gpu, monkeypatch, threads):
    """The first case (identity ALM, full convergence) under each thread-count instantiation:
    the oracle's results, hence identical across geometries and to the default's."""
    I = vc.inputs(pkg)
    default = _cold(pkg, I, [0, 1, 2], vc.B_IDENTITY, **_kw(50, 1e-6, 200))
    monkeypatch.setenv(KNOB, str(threads))
    R = _cold(pkg, I, [0, 1, 2], vc.B_IDENTITY, **_kw(50, 1e-6, 200))
    _same_batch(R, default)
    for e in range(3):
        _same(R, e, vc.oracle_cold(pkg, e, vc.B_IDENTITY))


def test_unknown_geometry_is_refused(pkg, gpu, monkeypatch):
    I = vc.inputs(pkg)
    monkeypatch.setenv(KNOB, "128")
    with pytest.raises(pkg.AiyError) as err:
        _cold(pkg, I, [0, 1, 2], vc.B_IDENTITY, **_kw(2, 0.0, 1))
    assert err.value.status == "AIY_BAD_ARG"


@pytest.mark.parametrize("threads", [None, 512, 256])
def test_nan_candidate_leaves_its_neighbours_alone(pkg, gpu, monkeypatch, threads):
    """A candidate whose value is all NaN between two ordinary ones, max_vfi = 6: every
    relative difference is NaN, so it never stops early (iters == max_vfi, rel_diff NaN), its
    outputs are the oracle's, and the neighbours' equal the batch without it."""
    if threads:
        monkeypatch.setenv(KNOB, str(threads))
    I = vc.inputs(pkg)
    kw = _kw(50, 1e-6, 6)
    nanV = np.full_like(I["V0"][1], np.nan)
    R = _batch(pkg, I, [0, 1, 2], [I["V0"][0], nanV, I["V0"][2]], [I["k0"]] * 3, vc.B_SHIFT, **kw)
    want = vc.oracle_solve(I, 1, nanV, I["k0"], vc.B_SHIFT, 50, 1e-6, 6, key=("nan", 1))
    assert want["iters"] == 6 and np.isnan(want["rel_diff"])
    _same(R, 1, want)
    assert R["iters"][1] == 6 and np.isnan(R["rel_diff"][1])
    for e in (0, 2):
        _same(R, e, vc.oracle_cold(pkg, e, vc.B_SHIFT, 50, 1e-6, 6))
    plain = _cold(pkg, I, [0, 2], vc.B_SHIFT, **kw)
    for c, e in enumerate((0, 2)):
        for key in ("value", "k_opt", "iters", "rel_diff"):
            assert np.array_equal(plain[key][c], R[key][e])


@pytest.mark.parametrize("threads", [1024, 512, 256])
@pytest.mark.parametrize("nk", [64, 65, 256])
def test_edges_of_the_nodes_per_thread_loops(pkg, gpu, monkeypatch, nk, threads):
    """k x 4 x 4 = 1,024 nodes (every lane of the widest geometry holds one node), 1,040 (16
    lanes hold a second one) and 4,096 (the largest that fits: every lane full, ~100 KB of
    LDS), two economies, against single calls."""
    monkeypatch.setenv(KNOB, str(threads))
    I = vc.inputs(pkg, nk, 4)
    kw = _kw(2, 1e-6, 2)
    R = _cold(pkg, I, [0, 1], vc.B_SHIFT, **kw)
    assert R["iters"].tolist() == [2, 2]
    for e in (0, 1):
        _same(R, e, _solo(pkg, I, e, I["V0"][e], I["k0"], vc.B_SHIFT, **kw))


def test_too_large_is_refused(pkg, gpu):
    I = vc.inputs(pkg, 257, 4)
    with pytest.raises(pkg.AiyError) as err:
        _cold(pkg, I, [0, 1], vc.B_IDENTITY, **_kw(2, 1e-6, 2))
    assert err.value.status == "AIY_BAD_SHAPE" and "no tiled" in str(err.value)


def test_more_workgroups_than_the_chip_holds(pkg, gpu):
    """C = 600 at 12 x 2, the candidates cycling over the three economies: each equals its
    economy's single result."""
    I = vc.inputs(pkg, 12, 2)
    kw = _kw(2, 1e-6, 6)
    order = [c % 3 for c in range(600)]
    R = _cold(pkg, I, order, vc.B_SHIFT, **kw)
    solo = [_solo(pkg, I, e, I["V0"][e], I["k0"], vc.B_SHIFT, **kw) for e in range(3)]
    for e in range(3):                                     # the yardstick is the oracle's
        want = vc.oracle_cold(pkg, e, vc.B_SHIFT, 2, 1e-6, 6, 12, 2)
        assert solo[e]["iters"] == want["iters"] == 6
        assert np.array_equal(solo[e]["value"], want["value"])
        assert np.array_equal(solo[e]["k_opt"], want["k_opt"])
    for c, e in enumerate(order):
        _same(R, c, solo[e])


def test_reference_size(pkg, gpu):
    """k_size = 100, K_size = 4 (the script's size), identity ALM, to convergence."""
    I = vc.inputs(pkg, 100, 4)
    kw = _kw(50, 1e-6, 200)
    R = _cold(pkg, I, [0, 1, 2], vc.B_IDENTITY, **kw)
    assert R["iters"].tolist() == [44, 40, 45]
    for e in range(3):
        _same(R, e, vc.oracle_cold(pkg, e, vc.B_IDENTITY, 50, 1e-6, 200, 100, 4))
        _same(R, e, _solo(pkg, I, e, I["V0"][e], I["k0"], vc.B_IDENTITY, **kw))


def test_device_tier_equals_host_tier_and_scratch_is_reused(pkg, gpu):
    """Two device-tier calls back to back on one stream with one scratch and different C: both
    results equal the host tier's; a scratch that is too small is refused in Python."""
    import torch
    I = vc.inputs(pkg)
    kw3, kw2 = _kw(50, 1e-6, 200), _kw(2, 0.0, 6)
    o3, o2 = [0, 1, 2], [2, 0]
    host3 = _cold(pkg, I, o3, vc.B_SHIFT, **kw3)
    host2 = _cold(pkg, I, o2, vc.B_IDENTITY, **kw2)
    kg = torch.as_tensor(I["k_grid"], device=gpu)

    def rows(blocks):                                                      # [C][4][nK][nk]
        return torch.as_tensor(np.ascontiguousarray(np.stack(blocks).transpose(0, 3, 2, 1)),
                               device=gpu)
    V3, k3 = rows([I["V0"][e] for e in o3]), rows([I["k0"]] * 3)
    V2, k2 = rows([I["V0"][e] for e in o2]), rows([I["k0"]] * 2)
    it3, r3, scratch = pkg.ks_vfi_solve_batch_dev(V3, k3, kg, I["K_grid"][o3], vc.B_SHIFT,
                                                  I["P"][o3], I["prm"][o3], **kw3)
    it2, r2, again = pkg.ks_vfi_solve_batch_dev(V2, k2, kg, I["K_grid"][o2], vc.B_IDENTITY,
                                                I["P"][o2], I["prm"][o2], scratch=scratch, **kw2)
    torch.cuda.synchronize()
    assert again is scratch
    for host, V, k, it, rel in ((host3, V3, k3, it3, r3), (host2, V2, k2, it2, r2)):
        assert np.array_equal(V.cpu().numpy().transpose(0, 3, 2, 1), host["value"])
        assert np.array_equal(k.cpu().numpy().transpose(0, 3, 2, 1), host["k_opt"])
        assert np.array_equal(it.cpu().numpy(), host["iters"])
        assert np.array_equal(rel.cpu().numpy(), host["rel_diff"], equal_nan=True)
    with pytest.raises(ValueError):
        pkg.ks_vfi_solve_batch_dev(V3, k3, kg, I["K_grid"][o3], vc.B_SHIFT, I["P"][o3],
                                   I["prm"][o3], scratch=scratch[:16], **kw3)
    with pytest.raises(ValueError):
        pkg.ks_vfi_solve_batch_dev(V3, k3[:2], kg, I["K_grid"][o3], vc.B_SHIFT, I["P"][o3],
                                   I["prm"][o3], **kw3)
