"""GPU: failed candidates strictly between runs of good ones in aiy_egm_ge_batch and
aiy_egm_ge_hist_batch.  The supply step then runs once per run of candidates that solved, each
launch at its offset into the share's policies, uniforms and outputs (here three runs of one).

Every candidate of these entries starts from one policy_c, so what makes a candidate fail is its
rate: from c(a) = 12 - 0.99 a the first step's endogenous grid has slope
1 - 0.99 (beta (1 + r))^(-1/sigma), which is negative at r = -0.04 and -0.02 (the folding grid of
test_folding_candidate_among_good_ones, by the rate) and positive at r = 0, 0.02, 0.04.  The good
candidates equal their own single calls bit for bit."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, NA, C, T = 2, 40, 5, 50
BETA, SIGMA, AMIN, ALPHA, DELTA, LABOR = 0.96, 5.0, 0.0, 0.36, 0.08, 1.0
TOL, MAX_ITER, DIST_TOL, DIST_MAX_ITER = 1e-3, 50, 1e-10, 2000
FAILS = (1, 3)  # positions 2 and 4


@pytest.fixture(scope="module")
def case(pkg, gpu):
    a = np.linspace(0, 10, NA)
    s, P = np.array([1.0, 1.2]), np.full((N, N), 0.5)
    cal = dict(N=N, Na=NA, a_grid=a, s=s, P=P, alpha=ALPHA, delta=DELTA, beta=BETA, sigma=SIGMA,
               amin=AMIN, labor=LABOR)
    pc = np.tile((12 - 0.99 * a)[None, :], (N, 1))  # [N][Na]
    r = np.array([0.0, -0.04, 0.02, -0.02, 0.04])
    w = np.array([1.0, 1.0, 1.05, 1.0, 0.95])
    rng = np.random.RandomState(7)
    blocks = [rng.random_sample(T - 1) for _ in range(C)]
    single = {}
    for q in range(C):
        if q in FAILS:
            with pytest.raises(pkg.AiyError, match="not increasing"):
                pkg.egm_solve(pc.T, a, s, P, r[q], w[q], BETA, SIGMA, AMIN, TOL, MAX_ITER)
        else:
            single[q] = pkg.egm_solve(pc.T, a, s, P, r[q], w[q], BETA, SIGMA, AMIN, TOL, MAX_ITER)
    return dict(cal=cal, pc=pc, r=r, w=w, blocks=blocks, z1=2, k1=a[7], single=single)


def _check_common(pkg, g, Ks, Kd, it, st):
    assert list(st) == [1 if q in FAILS else 0 for q in range(C)]
    for q in range(C):
        assert Kd[q] == pkg.calibration.capital_demand(g["r"][q], LABOR, ALPHA, DELTA), q
        if q in FAILS:
            assert math.isnan(Ks[q]), q
        else:
            assert it[q] == g["single"][q]["iters"], q


def test_chains_run_per_run_of_solved_candidates(pkg, case):
    g, a, P = case, case["cal"]["a_grid"], case["cal"]["P"]
    Ks, Kd, it, st = pkg.ge_batch.egm_ge_batch_call(g["r"], g["w"], g["pc"], g["cal"], g["z1"],
                                                    g["k1"], g["blocks"], tol=TOL,
                                                    max_iter=MAX_ITER)
    _check_common(pkg, g, Ks, Kd, it, st)
    for q, R in g["single"].items():
        K1 = pkg.sim_capital(R["policy_k"], a, P, g["z1"], g["k1"], g["blocks"][q],
                             vfi_layout=False)
        assert Ks[q] == K1, (q, Ks[q], K1)
    assert len({float(Ks[q]) for q in g["single"]}) == 3  # (an offset error could not hide)


def test_histograms_run_per_run_of_solved_candidates(pkg, case):
    g, a, P = case, case["cal"]["a_grid"], case["cal"]["P"]
    Ks, Kd, it, dit, st = pkg.ge_batch.egm_ge_hist_batch_call(
        g["r"], g["w"], g["pc"], g["cal"], tol=TOL, max_iter=MAX_ITER, dist_tol=DIST_TOL,
        dist_max_iter=DIST_MAX_ITER)
    _check_common(pkg, g, Ks, Kd, it, st)
    for q in FAILS:
        assert dit[q] == 0, q
    for q, R in g["single"].items():
        _, K1, it1, _ = pkg.dist_stationary(a, P, policy_k=R["policy_k"], tol=DIST_TOL,
                                            max_iter=DIST_MAX_ITER, vfi_layout=False)
        assert Ks[q] == K1 and dit[q] == it1, (q, Ks[q], K1, dit[q], it1)
    assert len({float(Ks[q]) for q in g["single"]}) == 3
