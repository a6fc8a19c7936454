"""GPU parity for the batched Jacobian (aiy_ssj_jacobian_batch): every economy of a batch bit for
bit against jacobian() on it alone and against tests/ssj_ref.jacobian_cpu (E exactly, F and J
within test_ssj_gpu.py's summation bound); independence of the batch's size, order and chunking;
the scripts' grid, where every strided loop takes several trips; an economy with a NaN policy
among good ones; and the solo entry, whose kernels gained the per-economy fields, against the
public entries it chains."""
import numpy as np
import pytest

from oracle import corc
from tests import ssj_ref as sr
from tests import transition_ref as tr
from tests.ssj_batch_cases import H, KEYS, SHAPES, economies, same, same_nan
from tests.test_ssj_gpu import _exact_F, _exact_J

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def solo(gpu, pkg):
    """(Na, T) -> the four jacobian() results, computed once."""
    memo = {}

    def get(Na, T):
        if (Na, T) not in memo:
            memo[(Na, T)] = [pkg.jacobian(ss, T, H) for ss in economies(Na)]
        return memo[(Na, T)]
    return get


def agrees(B, e, S):
    """Economy e of the batch B is the solo result S."""
    return (all(same_nan(B[k][e], S[k]) for k in KEYS)
            and tuple(int(v) for v in B["status"][e]) == tuple(S["status"]))


@pytest.mark.parametrize("Na,T", SHAPES)
def test_the_batch_is_the_solo_call_and_the_cpu_jacobian(gpu, pkg, solo, Na, T):
    eco = economies(Na)
    B = pkg.jacobian_batch(eco, T, H)
    assert B["J_r"].shape == (4, T, T) and B["E"].shape == (4, T, 3, Na)
    assert B["status"].shape == (4, 2) and not B["status"].any()
    n = 3 * Na
    for e, ss in enumerate(eco):
        S = solo(Na, T)[e]
        assert S["status"] == (0, 0)
        for k in KEYS:
            assert same(B[k][e], S[k]), (e, k)
        R = sr.jacobian_cpu(ss, T, H)
        assert same(B["E"][e], R["E"]), e
        Fx, A = _exact_F(R["E"], R["lam1"], H)
        Jx, AJ = _exact_J(R["E"], R["lam1"], H)
        F = np.stack([B["F_r"][e], B["F_w"][e]])
        J = np.stack([B["J_r"][e], B["J_w"][e]])
        assert np.isfinite(J).all()
        assert (np.abs(F - Fx) <= n * 2.0 ** -52 * A).all(), e
        assert (np.abs(J - Jx) <= n * 2.0 ** -52 * AJ).all(), e
    # the economies really differ: no two share a Jacobian
    assert all(not same(B["J_r"][e], B["J_r"][f]) for e in range(4) for f in range(e))


@pytest.mark.parametrize("Na,T", SHAPES)
def test_an_economy_does_not_depend_on_its_batch(gpu, pkg, solo, Na, T):
    """Permuted, alone, listed twice, and staged 1, 3 or all at a time: the same bits."""
    eco, S = economies(Na), solo(Na, T)
    for order in ([2, 0, 3, 1], [1], [3, 3, 0], [0, 1, 2, 3, 0]):
        B = pkg.jacobian_batch([eco[e] for e in order], T, H)
        for q, e in enumerate(order):
            assert agrees(B, q, S[e]), (order, q)
    for chunk in (0, 1, 3):
        B = pkg.jacobian_batch(eco, T, H, chunk=chunk)
        for e in range(4):
            assert agrees(B, e, S[e]), (chunk, e)
    ms = np.full(4, -1.0)
    B = pkg.jacobian_batch(eco, T, H, stage_ms=ms, chunk=3)
    assert (ms > 0).all() and all(agrees(B, e, S[e]) for e in range(4))


def _point400(pkg, beta):
    """test_ssj_gpu._point400 with this β: N = 7, Na = 400, 60 oracle EGM steps and 50 pushes."""
    cb = pkg.calibration
    cal = cb.aiyagari(Na=400, beta=beta)
    a, s, P, r = cal["a_grid"], cal["s"], cal["P"], 0.03
    w = cb.wage(r, cal["alpha"], cal["delta"])
    R = corc.egm_solve(np.tile((1 + r) * a + w * np.mean(s), (7, 1)), a, s, P, r, w, cal["beta"],
                       cal["sigma"], cal["amin"], max_iter=60)
    lam = np.full((7, 400), 1.0 / 2800)
    for _ in range(50):
        lam = corc.dist_update_lottery(lam, R["policy_k"], a, P)
    return dict(r=r, w=w, K=tr.capital_sum(lam, a), policy_c=R["policy_c"], lam=lam, cal=cal)


def test_the_full_width_case(gpu, pkg):
    """N·Na = 2,800 states and 1,024 threads: every strided loop walks several elements a
    thread."""
    T = 6
    eco = [_point400(pkg, beta) for beta in (0.96, 0.94)]
    B = pkg.jacobian_batch(eco, T, H)
    for e, ss in enumerate(eco):
        S = pkg.jacobian(ss, T, H)
        assert agrees(B, e, S), e
        assert np.array_equal(B["J_r"][e], S["J_r"], equal_nan=True)
    assert not same(B["J_r"][0], B["J_r"][1]) and not B["status"].any()


@pytest.mark.parametrize("bad", [0, 2])
def test_a_nan_policy_stays_in_its_economy(gpu, pkg, solo, bad):
    Na, T = SHAPES[0]
    eco, S = list(economies(Na)), solo(Na, T)
    sick = dict(eco[bad])
    sick["policy_c"] = sick["policy_c"].copy()
    sick["policy_c"][1, 17] = np.nan
    eco[bad] = sick
    B = pkg.jacobian_batch(eco, T, H)
    assert B["status"][bad][0] != 0
    assert np.isnan(B["J_r"][bad]).all() and np.isnan(B["J_w"][bad]).all()
    for e in range(4):
        if e != bad:
            assert agrees(B, e, S[e]), e


def test_the_solo_entry_did_not_move(gpu, pkg, solo):
    """test_ssj_gpu.test_jacobian_is_the_cpu_jacobian's chain on the first economy: jacobian()
    against the public entries it chains, whose kernels now carry the per-economy fields, all
    zero here."""
    Na, T = SHAPES[0]
    ss, G = economies(Na)[0], solo(Na, T)[0]
    cal = ss["cal"]
    a, s, P, N = cal["a_grid"], cal["s"], cal["P"], cal["N"]
    R = sr.jacobian_cpu(ss, T, H)
    assert G["status"] == (0, 0) and same(G["E"], R["E"])
    r, w = sr.news_paths(ss, T, H)
    Bk = pkg.egm_backward_batch(r, w, ss["policy_c"], a, s, P, cal["beta"], cal["sigma"],
                                cal["amin"], want_pc=False)
    assert (Bk["status"] == 0).all() and same(Bk["policy_k"], R["pk"])
    Fw = pkg.dist_forward_batch(Bk["policy_k"].reshape(3 * T, 1, N, Na), ss["lam"], a, P)
    assert (Fw["status"] == 0).all()
    lam1 = Fw["lam_T"].reshape(3, T, N, Na)
    assert same(lam1, R["lam1"])
    F, J = pkg.fake_news(G["E"], lam1, H)
    assert same(F[0], G["F_r"]) and same(F[1], G["F_w"])
    assert same(J[0], G["J_r"]) and same(J[1], G["J_w"])
    assert same(pkg.expectation_batch(R["pk"][0, :1], np.tile(a, (N, 1)), a, P, T)[0], G["E"])
