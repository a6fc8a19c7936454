"""GPU: the batched Gauss-Seidel Krusell-Smith EGM solve (ks_egm_solve_batch, one workgroup per
economy) against ks_egm_solve called alone and the C oracle — k_opt, iters and diff bit for bit —
through the host tier and the device tier."""
import numpy as np
import pytest

from tests import ks_egm_batch_cases as bc

pytestmark = pytest.mark.gpu


def _eq(a, b):
    return a == b or (np.isnan(a) and np.isnan(b))


def _batch(pkg, I, order, k0s, B, **kw):
    return pkg.ks_egm_solve_batch(np.stack(k0s), I["k_grid"], I["K_grid"][order], B,
                                  I["P"][order], I["prm"][order], **kw)


def _solo(pkg, I, e, k0, B, **kw):
    return pkg.ks_egm_solve(k0, I["k_grid"], I["K_grid"][e], B, I["P"][e], I["prm"][e], **kw)


def _same(R, c, S):
    assert R["status"][c] == 0
    assert R["iters"][c] == S["iters"] and _eq(R["diff"][c], S["diff"])
    assert np.array_equal(R["k_opt"][c], S["k_opt"])


@pytest.mark.parametrize("max_iter", [1, 3, 400])
@pytest.mark.parametrize("B", [bc.B_IDENTITY, bc.B_OTHER])
def test_batch_equals_single_calls_and_the_oracle(pkg, gpu, B, max_iter):
    I = bc.inputs(pkg)
    order = [0, 1, 2]
    R = _batch(pkg, I, order, [I["k0"]] * 3, B, max_iter=max_iter)
    for c, e in enumerate(order):
        _same(R, c, _solo(pkg, I, e, I["k0"], B, max_iter=max_iter))
        _same(R, c, bc.oracle_solve(I, e, I["k0"], B, max_iter=max_iter))


@pytest.mark.parametrize("e,max_iter", [(0, 3), (1, 3), (2, 3), (2, 400)])
def test_one_candidate(pkg, gpu, e, max_iter):
    I = bc.inputs(pkg)
    R = _batch(pkg, I, [e], [I["k0"]], bc.B_OTHER, max_iter=max_iter)
    assert R["k_opt"].shape == (1,) + I["k0"].shape
    _same(R, 0, _solo(pkg, I, e, I["k0"], bc.B_OTHER, max_iter=max_iter))
    _same(R, 0, bc.oracle_solve(I, e, I["k0"], bc.B_OTHER, max_iter=max_iter))


def test_permuted_candidates_give_permuted_results(pkg, gpu):
    I = bc.inputs(pkg)
    R = _batch(pkg, I, [0, 1, 2], [I["k0"]] * 3, bc.B_OTHER, max_iter=400)
    perm = [2, 0, 1]
    Rp = _batch(pkg, I, perm, [I["k0"]] * 3, bc.B_OTHER, max_iter=400)
    for c, e in enumerate(perm):
        assert Rp["iters"][c] == R["iters"][e] and _eq(Rp["diff"][c], R["diff"][e])
        assert np.array_equal(Rp["k_opt"][c], R["k_opt"][e])


def test_mixed_stopping(pkg, gpu):
    I = bc.inputs(pkg)
    k0s = [I["k0"]] * 3
    # the first sweep from 0.9 k_grid moves the policy by far more than 1.0 (k reaches 1,000), so
    # tol = 1.0 stops nobody at sweep 1 here; tol = inf does, and both must follow the oracle
    for tol in (1.0, np.inf):
        R = _batch(pkg, I, [0, 1, 2], k0s, bc.B_IDENTITY, tol=tol, max_iter=7)
        for c in range(3):
            _same(R, c, bc.oracle_solve(I, c, I["k0"], bc.B_IDENTITY, tol=tol, max_iter=7))
    assert R["iters"].tolist() == [1, 1, 1]
    R = _batch(pkg, I, [0, 1, 2], k0s, bc.B_IDENTITY, tol=0.0, max_iter=7)
    assert R["iters"].tolist() == [7, 7, 7]
    for c in range(3):
        _same(R, c, bc.oracle_solve(I, c, I["k0"], bc.B_IDENTITY, tol=0.0, max_iter=7))
    # a warm candidate (its converged policy: stops at sweep 1) between two cold ones
    conv = _solo(pkg, I, 1, I["k0"], bc.B_IDENTITY, max_iter=5000)
    assert conv["iters"] < 5000
    starts = [I["k0"], conv["k_opt"], I["k0"]]
    order = [0, 1, 1]
    R = _batch(pkg, I, order, starts, bc.B_IDENTITY, max_iter=50)
    assert R["iters"].tolist() == [50, 1, 50]
    for c, e in enumerate(order):
        _same(R, c, _solo(pkg, I, e, starts[c], bc.B_IDENTITY, max_iter=50))
        _same(R, c, bc.oracle_solve(I, e, starts[c], bc.B_IDENTITY, max_iter=50))


def test_failing_candidate_leaves_its_neighbours_alone(pkg, gpu):
    """Candidate 1 has no valid EGM point (ks_cases' nanP construction: the oracle returns
    rc != 0, ks_egm_solve AIY_NON_FINITE): status 1, the call returns OK, and the healthy
    candidates on both sides equal their solo runs.  An all-NaN k_opt start, in contrast, is
    run by the oracle (the c_next floor turns NaN into 1e-8), and by the batch alike."""
    I = bc.inputs(pkg)
    J = dict(I, P=np.stack([I["P"][0], bc.nan_row_P(I["P"][1]), I["P"][2]]))
    with pytest.raises(ValueError):
        bc.oracle_solve(J, 1, I["k0"], bc.B_OTHER, max_iter=6)
    with pytest.raises(pkg.AiyError) as err:
        _solo(pkg, J, 1, I["k0"], bc.B_OTHER, max_iter=6)
    assert err.value.status == "AIY_NON_FINITE"
    R = _batch(pkg, J, [0, 1, 2], [I["k0"]] * 3, bc.B_OTHER, max_iter=6)
    assert R["status"].tolist() == [0, 1, 0]
    for c in (0, 2):
        _same(R, c, _solo(pkg, I, c, I["k0"], bc.B_OTHER, max_iter=6))
        _same(R, c, bc.oracle_solve(I, c, I["k0"], bc.B_OTHER, max_iter=6))
    nan0 = np.full_like(I["k0"], np.nan)
    starts = [I["k0"], nan0, I["k0"]]
    R = _batch(pkg, I, [0, 1, 2], starts, bc.B_OTHER, max_iter=6)
    for c in range(3):
        _same(R, c, bc.oracle_solve(I, c, starts[c], bc.B_OTHER, max_iter=6))


def test_reference_size(pkg, gpu, golden):
    """k_size = 100, K_size = 4 (the reference LDS geometry), C = 5, three sweeps: the reference
    economy's candidates equal the golden fixture, the others their solo runs."""
    g = golden("ks_egm_defaults")
    I = bc.inputs(pkg, 100, 4)
    assert np.array_equal(I["k_grid"], g["k_grid"]) and np.array_equal(I["K_grid"][0], g["K_grid"])
    order = [0, 1, 0, 2, 0]
    R = _batch(pkg, I, order, [g["k_opt0"]] * 5, g["B"], max_iter=3)
    assert R["status"].tolist() == [0] * 5 and R["iters"].tolist() == [3] * 5
    for c, e in enumerate(order):
        if e == 0:
            assert np.array_equal(R["k_opt"][c], g["k_opt3"]) and R["diff"][c] == float(g["diff3"])
        else:
            _same(R, c, _solo(pkg, I, e, g["k_opt0"], g["B"], max_iter=3))


def test_device_tier_equals_host_tier_and_scratch_is_reused(pkg, gpu):
    """Two device-tier calls back to back on one stream with one scratch and different C: both
    results equal the host tier's."""
    import torch
    I = bc.inputs(pkg)
    host3 = _batch(pkg, I, [0, 1, 2], [I["k0"]] * 3, bc.B_OTHER, max_iter=400)
    host2 = _batch(pkg, I, [2, 0], [I["k0"]] * 2, bc.B_IDENTITY, max_iter=40)
    kg = torch.as_tensor(I["k_grid"], device=gpu)
    k0 = np.ascontiguousarray(I["k0"].transpose(2, 1, 0))                  # [4][nK][nk]
    ko3 = torch.as_tensor(np.stack([k0] * 3), device=gpu)
    ko2 = torch.as_tensor(np.stack([k0] * 2), device=gpu)
    o3 = [0, 1, 2]
    it3, d3, s3, scratch = pkg.ks_egm_solve_batch_dev(ko3, kg, I["K_grid"][o3], bc.B_OTHER,
                                                      I["P"][o3], I["prm"][o3], max_iter=400)
    o2 = [2, 0]
    it2, d2, s2, _ = pkg.ks_egm_solve_batch_dev(ko2, kg, I["K_grid"][o2], bc.B_IDENTITY,
                                                I["P"][o2], I["prm"][o2], max_iter=40,
                                                scratch=scratch)
    torch.cuda.synchronize()
    for host, ko, it, dd, st in ((host3, ko3, it3, d3, s3), (host2, ko2, it2, d2, s2)):
        assert np.array_equal(ko.cpu().numpy().transpose(0, 3, 2, 1), host["k_opt"])
        assert np.array_equal(it.cpu().numpy(), host["iters"])
        assert np.array_equal(dd.cpu().numpy(), host["diff"], equal_nan=True)
        assert np.array_equal(st.cpu().numpy(), host["status"])
