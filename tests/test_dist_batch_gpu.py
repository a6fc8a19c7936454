"""GPU parity for the batched stationary-distribution solve (aiy_dist_stationary_batch_dev: one
workgroup per candidate policy, the whole fixed point in LDS) and the histogram GE batches built
on it (aiy_ge_hist_batch, aiy_egm_ge_hist_batch, their gateways, ge_batch.py).  The oracle is the
C restatement: corc.dist_stationary on policies from corc.vfi_solve / corc.egm_solve.  λ, iters
and dist are compared bit for bit; K within 1e-12 relative (the device's fixed-order tree sum
against the oracle's sequential sum, as in test_dist_gpu.py)."""
import numpy as np
import pytest

from oracle import corc

pytestmark = pytest.mark.gpu

TOL, CAP = 1e-13, 5000
RATES = [-0.03, -0.012, 0.004, 0.021, 0.036]  # five distinct rates inside the GE bracket
# the dispatch threshold recorded in DESIGN.md §5 (profiles/r12_dist_batch_ab.txt)
RECORDED_MIN_C = 2


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.int64)


def same(x, y):
    return np.array_equal(bits(x), bits(y))


def _random_problem(N, Na, rng):
    a = np.linspace(0.0, 30.0, Na) ** 2 / 30.0
    P = rng.random((N, N)) + 0.05
    P /= P.sum(1, keepdims=True)
    return a, P


def _sorted_idx(C, N, Na, rng):
    steps = rng.choice([0, 1, 1, 1, 2, 0, 0], size=(C, N, Na))
    return np.minimum(np.cumsum(steps, 2), Na - 1).astype(np.int32)


def _sorted_kp(C, N, Na, a, rng):
    return np.sort(rng.uniform(-1.0, a[-1] * 0.9, (C, N, Na)), 2)


def _lam0(C, N, Na, rng):
    lam = rng.random((C, N, Na))
    return lam / lam.sum((1, 2), keepdims=True)


_POL = {}


def solved_policies(pkg, Na):
    """(a, P, idx [5][7][Na] 0-based, kp [5][7][Na]) — oracle VFI / EGM solves at RATES."""
    if Na not in _POL:
        gb, cb = pkg.ge_batch, pkg.calibration
        cal = cb.aiyagari(Na=Na)
        a, s, P = cal["a_grid"], cal["s"], cal["P"]
        idx = np.stack([corc.vfi_solve(np.zeros((7, Na)), a, s, P, r,
                                       cb.wage(r, cal["alpha"], cal["delta"]), cal["beta"],
                                       cal["sigma"])["idx"] for r in RATES]).astype(np.int32)
        _, r0, w, guess = gb.egm_calibration(Na, False)
        kp = np.stack([corc.egm_solve(guess, a, s, P, r, w, cal["beta"], cal["sigma"],
                                      cal["amin"])["policy_k"] for r in RATES])
        _POL[Na] = (a, P, idx, kp)
    return _POL[Na]


class Dev:
    """The device tier on numpy inputs: [C][N][Na] policies and starts."""

    def __init__(self, pkg, a, P):
        import torch
        self.pkg, self.torch = pkg, torch
        self.dev = torch.device("cuda:0")
        self.a, self.P = self.t(a), self.t(P)

    def t(self, x):
        return None if x is None else self.torch.as_tensor(np.ascontiguousarray(x), device=self.dev)

    def batch(self, ws, lam0, idx=None, kp=None, tol=TOL, max_iter=CAP):
        torch = self.torch
        C = lam0.shape[0]
        out = torch.full(lam0.shape, -7.0, dtype=torch.float64, device=self.dev)
        K = torch.full((C,), -7.0, dtype=torch.float64, device=self.dev)
        it, dist = self.pkg.dist_stationary_batch_dev(ws, self.t(lam0), self.a, self.P, out,
                                                      policy_idx=self.t(idx), policy_k=self.t(kp),
                                                      tol=tol, max_iter=max_iter, k_supply=K)
        return dict(lam=out.cpu().numpy(), K=K.cpu().numpy(), it=it, dist=dist)

    def separate(self, ws, lam0, idx=None, kp=None, tol=TOL, max_iter=CAP):
        torch = self.torch
        C = lam0.shape[0]
        out = torch.empty(lam0.shape, dtype=torch.float64, device=self.dev)
        K = torch.empty((C,), dtype=torch.float64, device=self.dev)
        it, dist = np.empty(C, np.int64), np.empty(C)
        for c in range(C):
            it[c], dist[c] = self.pkg.dist_stationary_dev(
                ws, self.t(lam0[c]), self.a, self.P, out[c],
                policy_idx=None if idx is None else self.t(idx[c]),
                policy_k=None if kp is None else self.t(kp[c]), tol=tol, max_iter=max_iter,
                k_supply=K[c:c + 1])
        return dict(lam=out.cpu().numpy(), K=K.cpu().numpy(), it=it, dist=dist)


def oracle(lam0, a, P, idx=None, kp=None, tol=TOL, max_iter=CAP):
    C = lam0.shape[0]
    res = [corc.dist_stationary(lam0[c], a, P, idx=None if idx is None else idx[c],
                                kp=None if kp is None else kp[c], tol=tol, max_iter=max_iter)
           for c in range(C)]
    return dict(lam=np.stack([x[0] for x in res]), K=np.array([x[1] for x in res]),
                it=np.array([x[2] for x in res], np.int64), dist=np.array([x[3] for x in res]))


def assert_same(got, ref, what=("lam", "K", "it", "dist")):
    for k in what:
        assert same(got[k], ref[k]) if k != "it" else np.array_equal(got[k], ref[k]), k


def assert_oracle(got, ref):
    assert_same(got, ref, ("lam", "it", "dist"))
    assert np.all(np.abs(got["K"] - ref["K"]) <= 1e-12 * np.abs(ref["K"]))


def forced(pkg, N, Na):
    ws = pkg.Workspace(N, Na)
    ws.set_dist_batch(1)
    return ws


def problem(pkg, N, Na, lottery, C=5):
    """The issue's cases: oracle solves at distinct rates where N = 7 (C = 5), sorted random
    policies elsewhere; a distinct random normalised λ₀ per candidate."""
    rng = np.random.default_rng(1000 * N + Na + (7 if lottery else 0))
    if N == 7 and C == 5:
        a, P, idx, kp = solved_policies(pkg, Na)
    else:
        a, P = _random_problem(N, Na, rng)
        idx, kp = _sorted_idx(C, N, Na, rng), _sorted_kp(C, N, Na, a, rng)
    return a, P, (None if lottery else idx), (kp if lottery else None), _lam0(C, N, Na, rng)


# ------------------------------------------------------------------ 1. batched == separate == oracle
@pytest.mark.parametrize("lottery", [False, True], ids=["ongrid", "lottery"])
@pytest.mark.parametrize("N,Na", [(1, 2), (2, 3), (3, 33), (7, 40), (7, 64), (7, 65), (16, 70),
                                  (7, 400)])
def test_batched_equals_separate_equals_oracle(pkg, gpu, N, Na, lottery):
    a, P, idx, kp, lam0 = problem(pkg, N, Na, lottery)
    D = Dev(pkg, a, P)
    ws = forced(pkg, N, Na)
    got = D.batch(ws, lam0, idx, kp)
    assert ws.dist_batch_counts() == (1, 0)  # the batched path ran: one solve launch
    assert_same(got, D.separate(pkg.Workspace(N, Na), lam0, idx, kp))
    assert_oracle(got, oracle(lam0, a, P, idx, kp))
    if N == 7:  # policies of distinct rates: the workgroups stop at different pushes
        assert len(set(got["it"].tolist())) > 1, got["it"]


# ------------------------------------------------------------------ 2. stop kinds
@pytest.mark.parametrize("lottery", [False, True], ids=["ongrid", "lottery"])
@pytest.mark.parametrize("tol,max_iter", [(0.0, 45), (1e-9, 5000), (2.0, 5000), (1e-13, 1),
                                          (1e-13, 70)])
def test_stop_kinds(pkg, gpu, tol, max_iter, lottery):
    a, P, idx, kp, lam0 = problem(pkg, 7, 40, lottery)
    D = Dev(pkg, a, P)
    ws = forced(pkg, 7, 40)
    got = D.batch(ws, lam0, idx, kp, tol, max_iter)
    assert ws.dist_batch_counts() == (1, 0)
    ref = oracle(lam0, a, P, idx, kp, tol, max_iter)
    assert_oracle(got, ref)
    assert_same(got, D.separate(pkg.Workspace(7, 40), lam0, idx, kp, tol, max_iter))
    if tol == 2.0:
        assert got["it"].tolist() == [1] * 5
    if tol == 0.0 or max_iter == 1:
        assert got["it"].tolist() == [max_iter] * 5


# ------------------------------------------------------------------ 3. long runs
def _long_run_rows(Na=600):
    """Three monotone rows of 600 sources: a borrowing-constraint run of 300 (ten chunks of 32,
    the last partial), a top-of-grid run of 130, runs of exactly 32, 33, 64 and 65 among them,
    single-source destinations in between."""
    def row(mid):
        keys, k = [0] * 300, 1
        n_single = Na - 300 - 130 - sum(mid)
        assert n_single >= len(mid)
        for q, L in enumerate(mid):
            keys += [k] * L
            k += 2  # (a gap: an empty destination)
            keys += list(range(k, k + n_single // len(mid) + (q < n_single % len(mid))))
            k = keys[-1] + 1
        keys += [Na - 1] * 130
        assert len(keys) == Na and keys == sorted(keys) and keys[-131] < Na - 2
        return keys
    return np.array([row([32, 33]), row([64, 65]), row([65, 33, 32])], np.int32)


@pytest.mark.parametrize("lottery", [False, True], ids=["ongrid", "lottery"])
def test_long_runs_chunked_order_bitwise(pkg, gpu, lottery):
    N, Na, C = 3, 600, 5
    rng = np.random.default_rng(11)
    a, P = _random_problem(N, Na, rng)
    rows = _long_run_rows(Na)
    idx = np.stack([np.roll(rows, c, 0) for c in range(C)])
    kp = None
    if lottery:  # the same runs as lottery keys; policy_k below and above the grid at the ends
        up = np.minimum(idx + 1, Na - 1)
        kp = a[idx] + rng.uniform(0.05, 0.95, idx.shape) * (a[up] - a[idx])
        kp[:, :, :300] = a[0] - 1.0
        kp[:, :, -130:] = a[-1] + 1.0
        idx = None
    lam0 = _lam0(C, N, Na, rng)
    D = Dev(pkg, a, P)
    ws = forced(pkg, N, Na)
    got = D.batch(ws, lam0, idx, kp, 0.0, 3)
    assert ws.dist_batch_counts() == (1, 0)
    assert_oracle(got, oracle(lam0, a, P, idx, kp, 0.0, 3))
    assert got["it"].tolist() == [3] * C


# ------------------------------------------------------------------ 4. mixed batch
@pytest.mark.parametrize("lottery", [False, True], ids=["ongrid", "lottery"])
def test_non_monotone_candidate_among_monotone(pkg, gpu, lottery):
    a, P, idx, kp, lam0 = problem(pkg, 7, 40, lottery)
    rng = np.random.default_rng(5)
    if lottery:
        kp = kp.copy()
        kp[2] = rng.uniform(-1.0, a[-1] + 1.0, (7, 40))
    else:
        idx = idx.copy()
        idx[2] = rng.integers(0, 40, (7, 40))
    D = Dev(pkg, a, P)
    ws = forced(pkg, 7, 40)
    got = D.batch(ws, lam0, idx, kp, TOL, 300)
    assert ws.dist_batch_counts() == (1, 1)
    assert_same(got, D.separate(pkg.Workspace(7, 40), lam0, idx, kp, TOL, 300))
    assert_oracle(got, oracle(lam0, a, P, idx, kp, TOL, 300))


@pytest.mark.parametrize("force", [1, 0])
def test_out_of_range_index_names_the_candidate(pkg, gpu, force):
    a, P, idx, _, lam0 = problem(pkg, 7, 40, False)
    idx = idx.copy()
    idx[3, 2, 5] = 40  # 0-based: one past the grid, in the fourth candidate
    D = Dev(pkg, a, P)
    ws = pkg.Workspace(7, 40)
    ws.set_dist_batch(force)
    with pytest.raises(pkg.AiyError) as e:
        D.batch(ws, lam0, idx)
    assert e.value.status == "AIY_BAD_ARG" and "candidate 4" in str(e.value)  # (1-based)
    assert ws.dist_batch_counts() == (0, 0)  # before any solve


# ------------------------------------------------------------------ 5. NaN
@pytest.mark.parametrize("lottery", [False, True], ids=["ongrid", "lottery"])
def test_nan_in_one_candidate(pkg, gpu, lottery):
    a, P, idx, kp, lam0 = problem(pkg, 7, 40, lottery)
    bad = lam0.copy()
    bad[1, 0, 3] = np.nan
    D = Dev(pkg, a, P)
    ws = forced(pkg, 7, 40)
    got = D.batch(ws, bad, idx, kp, TOL, 40)
    assert ws.dist_batch_counts() == (1, 0)
    sep = D.separate(pkg.Workspace(7, 40), bad, idx, kp, TOL, 40)
    assert got["it"][1] == sep["it"][1] == 40 and same(got["dist"][1], sep["dist"][1])
    assert_same(got, sep)
    assert_same(got, oracle(bad, a, P, idx, kp, TOL, 40), ("lam", "it", "dist"))
    clean = D.batch(forced(pkg, 7, 40), lam0, idx, kp, TOL, 40)
    for c in (0, 2, 3, 4):
        for k in ("lam", "K", "it", "dist"):
            assert same(got[k][c], clean[k][c]), (k, c)


# ------------------------------------------------------------------ 6. shapes that do not fit
@pytest.mark.parametrize("lottery", [False, True], ids=["ongrid", "lottery"])
@pytest.mark.parametrize("N,Na,C", [(7, 4000, 3), (17, 900, 2)])
def test_shapes_that_do_not_fit_run_per_candidate(pkg, gpu, N, Na, C, lottery):
    a, P, idx, kp, lam0 = problem(pkg, N, Na, lottery, C)
    D = Dev(pkg, a, P)
    ws = forced(pkg, N, Na)
    got = D.batch(ws, lam0, idx, kp, 1e-9, 12)
    assert ws.dist_batch_counts() == (0, C)
    assert_same(got, D.separate(pkg.Workspace(N, Na), lam0, idx, kp, 1e-9, 12))
    assert_oracle(got, oracle(lam0, a, P, idx, kp, 1e-9, 12))


# ------------------------------------------------------------------ 7. dispatch and workspace
def test_dispatch_setting_does_not_change_results(pkg, gpu):
    a, P, idx, _, lam0 = problem(pkg, 7, 40, False)
    D = Dev(pkg, a, P)
    never = pkg.Workspace(7, 40)
    never.set_dist_batch(0)
    A, B = D.batch(never, lam0, idx), D.batch(forced(pkg, 7, 40), lam0, idx)
    assert never.dist_batch_counts() == (0, 5)
    assert_same(A, B)
    with pytest.raises(pkg.AiyError):
        never.set_dist_batch(-2)


def test_default_dispatch_threshold(pkg, gpu):
    a, P, idx, _, lam0 = problem(pkg, 7, 40, False)
    D = Dev(pkg, a, P)
    ws = pkg.Workspace(7, 40)
    below = RECORDED_MIN_C - 1
    D.batch(ws, lam0[:below], idx[:below])
    assert ws.dist_batch_counts() == (0, below)
    D.batch(ws, lam0[:RECORDED_MIN_C], idx[:RECORDED_MIN_C])
    assert ws.dist_batch_counts() == (1, below)


@pytest.fixture(scope="module")
def seventy(pkg, gpu):
    """70 candidates at (7, 40): the five solved policies and sorted random ones, on-grid."""
    rng = np.random.default_rng(70)
    a, P, idx, _ = solved_policies(pkg, 40)
    idx = np.concatenate([idx, _sorted_idx(65, 7, 40, rng)])
    lam0 = _lam0(70, 7, 40, rng)
    return a, P, idx, lam0, oracle(lam0, a, P, idx, None, TOL, 400)


def test_seventy_candidates(pkg, gpu, seventy):
    a, P, idx, lam0, ref = seventy
    ws = forced(pkg, 7, 40)
    got = Dev(pkg, a, P).batch(ws, lam0, idx, None, TOL, 400)
    assert ws.dist_batch_counts() == (1, 0)
    assert_oracle(got, ref)


def test_used_workspace_equals_fresh(pkg, gpu, seventy):
    """C = 5, 70, 3 on ONE workspace give what fresh workspaces give (the blocks grow to the
    largest C seen; nothing cached leaks between calls)."""
    a, P, idx, lam0, ref = seventy
    D = Dev(pkg, a, P)
    used = forced(pkg, 7, 40)
    for sel in (slice(0, 5), slice(0, 70), slice(10, 13)):
        got = D.batch(used, lam0[sel], idx[sel], None, TOL, 400)
        assert_same(got, D.batch(forced(pkg, 7, 40), lam0[sel], idx[sel], None, TOL, 400))
        assert_same(got, {k: v[sel] for k, v in ref.items()}, ("lam", "it", "dist"))
    assert used.dist_batch_counts() == (3, 0)


# ------------------------------------------------------------------ 8. host tier
@pytest.mark.parametrize("lottery", [False, True], ids=["ongrid", "lottery"])
@pytest.mark.parametrize("vfi_layout", [True, False])
def test_host_tier_equals_single_calls(pkg, gpu, lottery, vfi_layout):
    a, P, idx, kp, lam0 = problem(pkg, 7, 40, lottery)
    lay = (lambda x: x) if vfi_layout else (lambda x: np.swapaxes(x, -1, -2))
    kw = dict(policy_k=lay(kp)) if lottery else dict(policy_idx=lay(idx + 1))
    lam, K, it, dist = pkg.dist_stationary_batch(a, P, lam0=lay(lam0), tol=TOL, max_iter=CAP,
                                                 vfi_layout=vfi_layout, **kw)
    for c in range(5):
        one = {k: v[c] for k, v in kw.items()}
        l1, K1, it1, d1 = pkg.dist_stationary(a, P, lam0=lay(lam0)[c], tol=TOL, max_iter=CAP,
                                              vfi_layout=vfi_layout, **one)
        assert same(lam[c], l1) and same(K[c], K1) and it[c] == it1 and same(dist[c], d1)
    assert len(set(it.tolist())) > 1


# ------------------------------------------------------------------ 9. GE
DT, DCAP = 1e-13, 100000


def _oracle_vfi_callables(pkg, cal):
    cb = pkg.calibration
    a, s, P = cal["a_grid"], cal["s"], cal["P"]
    uni = np.full((cal["N"], cal["Na"]), 1.0 / (cal["N"] * cal["Na"]))

    def solve(v, r):
        return corc.vfi_solve(v, a, s, P, r, cb.wage(r, cal["alpha"], cal["delta"]), cal["beta"],
                              cal["sigma"])

    def supply(R):
        _, K, it, _ = corc.dist_stationary(uni, a, P, idx=R["idx"], tol=DT, max_iter=DCAP)
        return K, it
    return solve, supply


def _oracle_egm_callables(cal, w, labor):
    a, s, P = cal["a_grid"], cal["s"], cal["P"]
    uni = np.full((cal["N"], cal["Na"]), 1.0 / (cal["N"] * cal["Na"]))

    def solve(pc, r):
        if labor:
            return corc.labor_egm_solve(pc, a, s, P, r, w, cal["beta"], cal["sigma"], 1.0, 1.0,
                                        cal["amin"])
        return corc.egm_solve(pc, a, s, P, r, w, cal["beta"], cal["sigma"], cal["amin"])

    def supply(R):
        _, K, it, _ = corc.dist_stationary(uni, a, P, kp=R["policy_k"], tol=DT, max_iter=DCAP)
        return K, it
    return solve, supply


def _vfi_setup(pkg, Na):
    cb = pkg.calibration
    cal = cb.aiyagari(Na=Na)
    solve, supply = _oracle_vfi_callables(pkg, cal)
    v0 = corc.vfi_solve(np.zeros((7, Na)), cal["a_grid"], cal["s"], cal["P"], 0.04,
                        cb.wage(0.04, cal["alpha"], cal["delta"]), cal["beta"],
                        cal["sigma"])["v_old"]
    return cal, v0, pkg.ge_batch.hist_evaluator(cal, solve, supply, v0)


def _egm_setup(pkg, Na, labor):
    cal, r0, w, guess = pkg.ge_batch.egm_calibration(Na, labor)
    solve, supply = _oracle_egm_callables(cal, w, labor)
    pc0 = solve(guess, r0)["policy_c"]
    return cal, w, pc0, pkg.ge_batch.hist_evaluator(cal, solve, supply, pc0)


@pytest.fixture(scope="module")
def ge40(pkg, gpu):
    """Na = 40: per script the calibration, the r0 start and the 7 nodes of a 3-level tree with
    their oracle results (shared by the GE-batch and the gateway tests)."""
    out = {}
    cal, v0, ev = _vfi_setup(pkg, 40)
    nodes = pkg.ge_batch.subtree(-0.05, 1 / cal["beta"] - 1, 1, 3)
    out["vfi"] = dict(cal=cal, v0=v0, nodes=nodes, ref=[ev(n) for n in nodes])
    for labor in (False, True):
        cal, w, pc0, ev = _egm_setup(pkg, 40, labor)
        out[labor] = dict(cal=cal, w=w, pc0=pc0, nodes=nodes, ref=[ev(n) for n in nodes])
    return out


def _check_nodes(Ks, Kd, it, dit, st, ref):
    for q, v in enumerate(ref):  # v = (K_s, K_d, iters, status, dist_iters)
        assert abs(Ks[q] - v[0]) <= 1e-12 * abs(v[0]), q
        assert Kd[q] == v[1] and it[q] == v[2] and st[q] == v[3] and dit[q] == v[4], q


def test_ge_hist_batch_equals_oracle_per_node(pkg, gpu, ge40):
    g = ge40["vfi"]
    r = [n.r for n in g["nodes"]]
    for nd in (1, 2):  # one GPU: the library clamps n_devices, the result is identical
        Ks, Kd, it, dit = pkg.ge_batch.ge_hist_batch_call(r, g["v0"], g["cal"], n_devices=nd)
        _check_nodes(Ks, Kd, it, dit, [0] * 7, g["ref"])
    assert len(set(dit.tolist())) > 1
    # a start of the caller's: from the first node's converged λ that node stops at once, and
    # every K_s moves by no more than the stopping rule allows (max|Δλ| < 1e-13 at a contraction
    # rate below 0.99 over 280 states of a <= 20: well within 1e-7 relative)
    cal = g["cal"]
    R = corc.vfi_solve(g["v0"], cal["a_grid"], cal["s"], cal["P"], r[0],
                       pkg.calibration.wage(r[0], cal["alpha"], cal["delta"]), cal["beta"],
                       cal["sigma"])
    lam = corc.dist_stationary(np.full((7, 40), 1 / 280), cal["a_grid"], cal["P"], idx=R["idx"],
                               tol=DT, max_iter=DCAP)[0]
    Ks2, _, it2, dit2 = pkg.ge_batch.ge_hist_batch_call(r, g["v0"], g["cal"], lam_start=lam)
    assert np.array_equal(it2, it) and dit2[0] <= 2 and np.allclose(Ks2, Ks, rtol=1e-7, atol=0)


@pytest.mark.parametrize("labor", [False, True])
def test_egm_ge_hist_batch_equals_oracle_per_node(pkg, gpu, ge40, labor):
    g = ge40[labor]
    r = [n.r for n in g["nodes"]]
    Ks, Kd, it, dit, st = pkg.ge_batch.egm_ge_hist_batch_call(r, g["w"], g["pc0"], g["cal"],
                                                              labor=labor)
    _check_nodes(Ks, Kd, it, dit, st, g["ref"])


def test_gateways_equal_library_calls(pkg, gpu, ge40):
    from tests import mexstub
    gb = pkg.ge_batch
    g = ge40["vfi"]
    cal = g["cal"]
    r = np.array([n.r for n in g["nodes"]])
    lam = _lam0(1, 7, 40, np.random.default_rng(3))[0]
    for start, tail in ((None, ()), (lam, (lam,))):
        Ks, Kd, it, dit = gb.ge_hist_batch_call(r, g["v0"], cal, lam_start=start)
        out = mexstub.call("aiy_ge_hist_batch_mex", 4, r, g["v0"], cal["a_grid"], cal["s"], cal["P"],
                           cal["alpha"], cal["delta"], cal["beta"], cal["sigma"], cal["labor"], 1e-5,
                           1000.0, DT, float(DCAP), 1.0, *tail)
        assert len(out) == 4 and all(o.shape == (7, 1) for o in out)
        for o, x in zip(out, (Ks, Kd, it, dit)):
            assert same(o.ravel(), np.asarray(x, np.float64))
    for labor in (False, True):
        g = ge40[labor]
        cal = g["cal"]
        for start, mx in ((None, np.zeros((0, 0))), (lam, lam.T)):
            res = gb.egm_ge_hist_batch_call(r, g["w"], g["pc0"], cal, labor=labor, lam_start=start)
            out = mexstub.call("aiy_egm_ge_hist_batch_mex", 5, r, g["pc0"].T, cal["a_grid"],
                               cal["s"], cal["P"], g["w"], cal["alpha"], cal["delta"], cal["beta"],
                               cal["sigma"], cal["amin"], cal["labor"], 1e-5, 1000.0, DT,
                               float(DCAP), 1.0, mx, *((1.0, 1.0) if labor else ()))
            Ks, Kd, it, dit, st = res
            for o, x in zip(out, (Ks, Kd, it, st, dit)):
                assert o.shape == (7, 1) and same(o.ravel(), np.asarray(x, np.float64))


@pytest.mark.parametrize("Na", [40, 400])
def test_vfi_multisection_histogram_equals_oracle_bisection(pkg, gpu, Na):
    """No sampling noise and |K_s − K_d| on the path far above the K tolerance (1e-12 relative):
    the batched GPU rounds take the oracle bisection's decisions exactly."""
    gb = pkg.ge_batch
    A = gb.aiyagari_vfi_multisection(Na=Na, levels=6, supply="histogram")
    assert A.rounds == 2 and A.candidates == 63 + 15
    cal, v0, ev = _vfi_setup(pkg, Na)
    S = gb.bisection(ev, -0.05, 1 / cal["beta"] - 1)
    assert A.r_history == S.r_history and A.r == S.r and A.iters == S.iters
    assert min(abs(x - y) for x, y in zip(S.k_supply, S.k_demand)) > 1e-3
    assert np.allclose(A.k_supply, S.k_supply, rtol=1e-12, atol=0)
    if Na == 400:  # the unbatched GPU evaluator: the same trace
        U = gb.aiyagari_vfi_multisection(Na=Na, levels=6, supply="histogram", batched=False)
        assert U.r_history == A.r_history and U.k_supply == A.k_supply and U.iters == A.iters


@pytest.mark.parametrize("Na", [40, 400])
def test_egm_multisection_histogram_equals_oracle_bisection(pkg, gpu, Na):
    gb = pkg.ge_batch
    A = gb.aiyagari_egm_multisection(Na=Na, levels=6, supply="histogram")
    assert A.rounds == 2 and A.candidates == 63 + 15
    cal, w, pc0, ev = _egm_setup(pkg, Na, False)
    S = gb.bisection(ev, -0.05, 1 / cal["beta"] - 1)
    assert A.r_history == S.r_history and A.r == S.r and A.iters[1:] == S.iters
    assert min(abs(x - y) for x, y in zip(S.k_supply, S.k_demand)) > 1e-3
    assert np.allclose(A.k_supply, S.k_supply, rtol=1e-12, atol=0)
    if Na == 400:
        U = gb.aiyagari_egm_multisection(Na=Na, levels=6, supply="histogram", batched=False)
        assert U.r_history == A.r_history and U.k_supply == A.k_supply and U.iters == A.iters
