"""GPU: the batched multi-rate EGM solve (aiy_egm_solve_batch_dev: one workgroup per candidate
rate, the whole loop in LDS) and its GE entry points (aiy_egm_ge_batch, the gateway, the
multisection driver).  Every comparison is bit for bit: against separate aiy_egm_solve_dev
calls and against the C restatement (oracle/)."""
import math

import numpy as np
import pytest

from oracle import corc
from oracle import np_oracle as no

pytestmark = pytest.mark.gpu

BETA, ALPHA, DELTA = 0.96, 0.36, 0.08
SHAPES = [(1, 2), (2, 3), (7, 63), (7, 65), (7, 400), (16, 128)]
# (labor, sigma, theta): A4 and A5, an integer and a non-integer sigma, theta = 1 and not
CONFIGS = [(False, 5.0, 1.0), (False, 2.5, 1.0), (True, 5.0, 1.0), (True, 2.5, 1.7)]
# one call holds both stop kinds (asserted below): at tol = 1e-2 the C loop needs 42-77 steps on
# these problems, or never gets there (some A5 candidates); the cap that splits every
# configuration's 70 candidates is 56 steps for the N <= 7 shapes and 60 for N = 16
TOL = 1e-2


def cap_of(N):
    return 60 if N == 16 else 56


def problem(N, Na, C, labor, sigma, theta):
    """C candidates on an (N, Na) model: distinct r over [-0.045, 0.04], distinct w and
    distinct starting policies (the scripts' r0 guess scaled per candidate), all [C][N][Na]."""
    if N == 7:
        cal = no.calib_aiyagari(Na=Na)
    elif N == 1:
        cal = dict(no.calib_aiyagari(Na=Na), s=np.array([1.0]), P=np.array([[1.0]]))
    elif N == 2:
        cal = dict(no.calib_aiyagari(Na=Na), s=np.array([0.6, 1.4]),
                   P=np.array([[0.8, 0.2], [0.3, 0.7]]))
    else:
        cal = no.calib_aiyagari(Na=Na, shocks="rouwenhorst", N=N)
    a, s, P = cal["a_grid"], np.asarray(cal["s"], float), np.asarray(cal["P"], float)
    f = np.arange(C) / max(C - 1, 1)
    r = -0.045 + 0.085 * f
    w0 = no.wage(0.04, ALPHA, DELTA)
    w = w0 * (0.9 + 0.2 * f[::-1])
    guess = np.tile((1.04 * a + w0 * np.mean(s))[None, :], (N, 1))
    pc = np.stack([guess * (0.8 + 0.4 * ((7 * c) % C) / C) for c in range(C)])
    return dict(N=N, Na=Na, C=C, a=a, s=s, P=P, r=r, w=w, pc=pc, amin=float(cal["amin"]),
                labor=labor, sigma=sigma, phi=1.0, theta=theta)


def oracle_solve(p, c, tol, max_iter):
    if p["labor"]:
        return corc.labor_egm_solve(p["pc"][c], p["a"], p["s"], p["P"], p["r"][c], p["w"][c], BETA,
                                    p["sigma"], p["phi"], p["theta"], p["amin"], tol, max_iter)
    return corc.egm_solve(p["pc"][c], p["a"], p["s"], p["P"], p["r"][c], p["w"][c], BETA,
                          p["sigma"], p["amin"], tol, max_iter)


class Dev:
    def __init__(self, pkg, p):
        import torch
        self.pkg, self.p, self.torch = pkg, p, torch
        self.dev = torch.device("cuda", 0)
        self.a, self.s, self.P = self.t(p["a"]), self.t(p["s"]), self.t(p["P"])

    def t(self, x):
        return self.torch.as_tensor(np.ascontiguousarray(x, dtype=np.float64), device=self.dev)

    def batch(self, ws, sel, tol, max_iter, fill=np.nan):
        """The candidates `sel` in one call -> dict of numpy results."""
        p = self.p
        c = self.t(p["pc"][sel])
        pk = self.torch.full_like(c, fill)
        pl = self.torch.full_like(c, fill) if p["labor"] else None
        it, dist, st = self.pkg.egm_solve_batch_dev(
            ws, p["r"][sel], p["w"][sel], c, self.a, self.s, self.P, BETA, p["sigma"], p["amin"],
            tol, max_iter, pk, labor=p["labor"], phi=p["phi"], theta=p["theta"], policy_l=pl)
        return dict(c=c.cpu().numpy(), pk=pk.cpu().numpy(),
                    pl=pl.cpu().numpy() if p["labor"] else None, it=it, dist=dist, st=st)

    def separate(self, ws, c, tol, max_iter, fill=np.nan):
        """Candidate c through aiy_egm_solve_dev (None where it reports a folding grid)."""
        p = self.p
        pc = self.t(p["pc"][c])
        pk = self.torch.full_like(pc, fill)
        pl = self.torch.full_like(pc, fill) if p["labor"] else None
        try:
            it, dist = self.pkg.egm_solve_dev(ws, pc, self.a, self.s, self.P, p["r"][c], p["w"][c],
                                              BETA, p["sigma"], p["amin"], tol, max_iter, pk,
                                              labor=p["labor"], phi=p["phi"], theta=p["theta"],
                                              policy_l=pl)
        except self.pkg.AiyError as e:
            assert "not increasing" in str(e)
            return None
        return dict(c=pc.cpu().numpy(), pk=pk.cpu().numpy(),
                    pl=pl.cpu().numpy() if p["labor"] else None, it=it, dist=dist)


def same(x, y):
    """bit-for-bit equality that also holds where both are NaN (an untouched output)."""
    return np.array_equal(np.asarray(x), np.asarray(y), equal_nan=True)


def check_against(B, sel, refs, labor):
    for q, c in enumerate(sel):
        R = refs[c]
        if R is None:
            assert B["st"][q] == 1, (c, B["st"][q])
            continue
        assert B["st"][q] == 0, (c, B["st"][q])
        assert B["it"][q] == R["it"], (c, B["it"][q], R["it"])
        assert same(B["dist"][q], R["dist"]), (c, B["dist"][q], R["dist"])
        assert same(B["c"][q], R["c"]) and same(B["pk"][q], R["pk"]), c
        if labor:
            assert same(B["pl"][q], R["pl"]), c


@pytest.mark.parametrize("labor,sigma,theta", CONFIGS)
@pytest.mark.parametrize("N,Na", SHAPES)
def test_batched_equals_separate_equals_oracle(pkg, gpu, N, Na, labor, sigma, theta):
    """C in {1, 2, 7, 70} candidates (70: more workgroup indices than one wave's lanes) on the
    one-launch path == separate aiy_egm_solve_dev calls == the C loop: policy_c, policy_k,
    policy_l, iters, dist; with tol = 1e-2 and max_iter = 56 (60) one call holds candidates that
    stop on tol and candidates that stop at the cap.  Also max_iter = 0 and tol >= 1 (no step:
    the outputs stay untouched) and the default dispatch."""
    p = problem(N, Na, 70, labor, sigma, theta)
    CAP = cap_of(N)
    D = Dev(pkg, p)
    ws1 = pkg.Workspace(N, Na)
    refs = [D.separate(ws1, c, TOL, CAP) for c in range(70)]
    ws = pkg.Workspace(N, Na)
    ws.set_egm_batch(1)  # the one-launch path whatever C
    for c in range(70):  # separate == oracle
        if refs[c] is None:
            continue
        O = oracle_solve(p, c, TOL, CAP)
        assert refs[c]["it"] == O["iters"] and same(refs[c]["dist"], O["dist"]), c
        assert same(refs[c]["c"], O["policy_c"]) and same(refs[c]["pk"], O["policy_k"]), c
        if labor:
            assert same(refs[c]["pl"], O["policy_l"]), c
    n_launch = 0
    for C in (1, 2, 7, 70):
        sel = np.unique(np.round(np.linspace(0, 69, C)).astype(int)) if C > 1 else np.array([35])
        B = D.batch(ws, sel, TOL, CAP)
        n_launch += 1
        check_against(B, sel, refs, labor)
    assert ws.egm_batch_counts() == (n_launch, 0)
    ok = [R for R in refs if R is not None]
    assert len(ok) == 70  # every candidate solves; both stop kinds; several counts
    its = [R["it"] for R in ok]
    assert any(i == CAP and R["dist"] > TOL for i, R in zip(its, ok))
    assert any(i < CAP and not R["dist"] > TOL for i, R in zip(its, ok))
    assert len(set(its)) >= 3, sorted(set(its))
    # no step: max_iter = 0, and tol >= 1 (dist = 1 is tested first)
    sel = np.array([0, 33, 69])
    for tol, mi in ((TOL, 0), (1.0, 50), (2.5, 50)):
        B = D.batch(ws, sel, tol, mi)
        for q, c in enumerate(sel):
            R = D.separate(ws1, c, tol, mi)
            assert B["it"][q] == R["it"] == 0 and B["dist"][q] == R["dist"] == 1.0
            assert B["st"][q] == 0 and same(B["c"][q], R["c"]) and same(B["pk"][q], R["pk"])
            assert same(B["c"][q], p["pc"][c]) and np.isnan(B["pk"][q]).all()
    # the default dispatch (whatever the threshold) gives the same
    wd = pkg.Workspace(N, Na)
    for C in (1, 7):
        sel = np.arange(C) * 9
        check_against(D.batch(wd, sel, TOL, CAP), sel, refs, labor)
    for x in (ws, ws1, wd):
        x.close()


@pytest.mark.parametrize("N,Na,C,labor", [(7, 1025, 3, False), (7, 2000, 3, False),
                                          (7, 2000, 3, True), (16, 512, 2, True)])
def test_shapes_that_do_not_fit_take_the_per_candidate_path(pkg, gpu, N, Na, C, labor):
    """Na > 1,024, or A5's 3·N·Na doubles past a CU's LDS: the same contract through the
    existing solve, candidate after candidate — and the counters say which path ran."""
    p = problem(N, Na, C, labor, 5.0, 1.0)
    CAP = cap_of(N)
    D = Dev(pkg, p)
    ws = pkg.Workspace(N, Na)
    ws.set_egm_batch(1)
    B = D.batch(ws, np.arange(C), TOL, CAP)
    assert ws.egm_batch_counts() == (0, C)
    ws1 = pkg.Workspace(N, Na)
    refs = [D.separate(ws1, c, TOL, CAP) for c in range(C)]
    assert all(R is not None for R in refs)
    check_against(B, np.arange(C), refs, labor)
    for c in range(C):
        O = oracle_solve(p, c, TOL, CAP)
        assert B["it"][c] == O["iters"] and same(B["c"][c], O["policy_c"])
        assert same(B["pk"][c], O["policy_k"])
    # the scripts' shape at the same setting takes the one-launch path; A4 at N = 16 fits where
    # A5 does not
    for (n2, na2, lab2) in ((7, 400, labor), (16, 512, False)):
        p2 = problem(n2, na2, C, lab2, 5.0, 1.0)
        w2 = pkg.Workspace(n2, na2)
        w2.set_egm_batch(1)
        Dev(pkg, p2).batch(w2, np.arange(C), TOL, 5)
        assert w2.egm_batch_counts() == (1, 0)
        w2.close()
    ws.close()
    ws1.close()


@pytest.mark.parametrize("min_c", [1, 0])
def test_folding_candidate_among_good_ones(pkg, gpu, min_c):
    """A candidate whose endogenous grid folds (the recipe of
    test_egm_nonmonotone_grid_is_reported) gets status 1; the call returns OK and its
    neighbours equal their separate solves — on the one-launch path and on the other."""
    import torch
    dev = torch.device("cuda", 0)
    t = lambda x: torch.as_tensor(np.ascontiguousarray(x, dtype=np.float64), device=dev)
    a = np.linspace(0, 10, 50)
    s, P = np.array([1.0, 1.2]), np.full((2, 2), 0.5)
    good = np.tile((1.02 * a + 1.0 * np.mean(s))[None, :], (2, 1))
    fold = np.tile(np.linspace(50, 0.01, 50)[None, :], (2, 1))
    pc = np.stack([good, fold, good * 1.1])
    r, w = np.array([0.02, 0.02, 0.03]), np.array([1.0, 1.0, 1.05])
    ws = pkg.Workspace(2, 50)
    ws.set_egm_batch(min_c)
    c, pk = t(pc), t(np.zeros_like(pc))
    it, dist, st = pkg.egm_solve_batch_dev(ws, r, w, c, t(a), t(s), t(P), 0.96, 5.0, 0.0, 1e-6, 50,
                                           pk)
    assert list(st) == [0, 1, 0]
    assert ws.egm_batch_counts() == ((1, 0) if min_c else (0, 3))
    for q in (0, 2):
        c1, k1 = t(pc[q]), t(np.zeros_like(pc[q]))
        i1, d1 = pkg.egm_solve_dev(ws, c1, t(a), t(s), t(P), r[q], w[q], 0.96, 5.0, 0.0, 1e-6, 50, k1)
        assert it[q] == i1 and dist[q] == d1
        assert np.array_equal(c[q].cpu().numpy(), c1.cpu().numpy())
        assert np.array_equal(pk[q].cpu().numpy(), k1.cpu().numpy())
    with pytest.raises(pkg.AiyError):
        pkg.egm_solve_dev(ws, t(pc[1]), t(a), t(s), t(P), r[1], w[1], 0.96, 5.0, 0.0, 1e-6, 50,
                          t(np.zeros_like(pc[1])))
    ws.close()


# ------------------------------------------------------------------ GE entry points
def _oracle_callables(cal, labor, tol=1e-5, max_iter=1000):
    a, s, P = cal["a_grid"], cal["s"], cal["P"]

    def solve(pc, r, w):
        if labor:
            return corc.labor_egm_solve(pc, a, s, P, r, w, cal["beta"], cal["sigma"], 1.0, 1.0,
                                        cal["amin"], tol, max_iter)
        return corc.egm_solve(pc, a, s, P, r, w, cal["beta"], cal["sigma"], cal["amin"], tol,
                              max_iter)

    def simulate(pk, z1, k1, u):
        return corc.sim_capital(pk, a, P, z1 - 1, k1, u)
    return solve, simulate


@pytest.fixture(scope="module")
def ge40(pkg, gpu):
    """Na = 40, T = 2,000: per script the calibration, the r0 policy and the 7 nodes of a 3-level
    tree with their oracle results (shared by the GE-batch and the gateway tests)."""
    gb = pkg.ge_batch
    out = {}
    for labor in (False, True):
        cal, r0, w, guess = gb.egm_calibration(40, labor)
        solve, simulate = _oracle_callables(cal, labor)
        pc0 = solve(guess, r0, w)["policy_c"]
        nodes = gb.subtree(-0.05, 1 / cal["beta"] - 1, 1, 3)
        ev = gb.egm_evaluator(cal, solve, simulate, pc0, w, labor, T=2000)
        head, blocks = gb.mc_stream(2000)
        z1 = int(math.ceil(cal["N"] * head[0]))
        k1 = cal["a_grid"][int(math.ceil(40 * head[1])) - 1]
        out[labor] = dict(cal=cal, w=w, pc0=pc0, nodes=nodes, ref=[ev(n) for n in nodes], z1=z1,
                          k1=k1, blocks=[blocks[n.depth] for n in nodes])
    return out


@pytest.mark.parametrize("labor", [False, True])
def test_egm_ge_batch_equals_oracle_per_node(pkg, gpu, ge40, labor):
    g = ge40[labor]
    r = [n.r for n in g["nodes"]]
    for nd in (1, 2):  # one GPU: the library clamps n_devices, the result is identical
        Ks, Kd, it, st = pkg.ge_batch.egm_ge_batch_call(r, g["w"], g["pc0"], g["cal"], g["z1"],
                                                        g["k1"], g["blocks"], labor=labor,
                                                        n_devices=nd)
        assert list(st) == [0] * 7
        assert [float(x) for x in Ks] == [v[0] for v in g["ref"]]
        assert [float(x) for x in Kd] == [v[1] for v in g["ref"]]
        assert [int(x) for x in it] == [v[2] for v in g["ref"]]


@pytest.mark.parametrize("labor", [False, True])
def test_gateway_equals_library_call(pkg, gpu, ge40, labor):
    from tests import mexstub
    g = ge40[labor]
    cal = g["cal"]
    r = np.array([n.r for n in g["nodes"]])
    U = np.stack(g["blocks"], axis=1)
    tail = (1.0, 1.0) if labor else ()
    wv = g["w"] * (1 + 0.01 * np.arange(7))
    for w in (g["w"], wv):
        Ks, Kd, it, st = pkg.ge_batch.egm_ge_batch_call(r, w, g["pc0"], cal, g["z1"], g["k1"],
                                                        g["blocks"], labor=labor)
        out = mexstub.call("aiy_egm_ge_batch_mex", 4, r, g["pc0"].T, cal["a_grid"], cal["s"],
                           cal["P"], w, cal["alpha"], cal["delta"], cal["beta"], cal["sigma"],
                           cal["amin"], cal["labor"], 1e-5, 1000.0, float(g["z1"]), g["k1"], U, 1.0,
                           *tail)
        assert len(out) == 4 and all(o.shape == (7, 1) for o in out)
        assert np.array_equal(out[0].ravel(), Ks) and np.array_equal(out[1].ravel(), Kd)
        assert np.array_equal(out[2].ravel(), it) and np.array_equal(out[3].ravel(), st)
    assert not np.array_equal(Ks, [v[0] for v in g["ref"]])  # (the vector w was used)


def test_multisection_at_the_script_defaults(pkg, gpu):
    """Aiyagari_EGM.m's GE at its defaults (Na = 400, T = 10,000) in two batched rounds: the
    trace of the sequential bisection over the one-after-another evaluator, and the r path of
    the script's own chained warm start (ge.aiyagari_egm)."""
    gb = pkg.ge_batch
    A = gb.aiyagari_egm_multisection(Na=400, levels=6)
    assert A.rounds == 2 and A.candidates == 63 + 15
    cal, r0, w, guess = gb.egm_calibration(400, False)
    R0 = pkg.egm_solve(guess.T, cal["a_grid"], cal["s"], cal["P"], r0, w, cal["beta"],
                       cal["sigma"], cal["amin"])
    ev = gb.hip_egm_evaluator(cal, np.ascontiguousarray(R0["policy_c"].T), w)
    S = gb.bisection(ev, -0.05, 1 / cal["beta"] - 1)
    assert A.r_history == S.r_history and A.k_supply == S.k_supply
    assert A.k_demand == S.k_demand and A.iters[1:] == S.iters and A.iters[0] == R0["iters"]
    G = pkg.ge.aiyagari_egm()
    assert A.r_history == G["r_history"]
    assert A.r == -0.010880533854166636
    assert np.max(np.abs(np.array(A.k_supply) - np.array(G["k_supply"]))) < 7e-3


def test_multisection_labor_at_na_40(pkg, gpu):
    """A5 at Na = 40: the same assertions; many of its 63 first-round candidates run to
    max_iter = 1000 (the script's stale w) without disturbing the others."""
    gb = pkg.ge_batch
    A = gb.aiyagari_egm_multisection(Na=40, labor=True, levels=6)
    assert A.rounds == 2 and A.candidates == 63 + 15
    cal, r0, w, guess = gb.egm_calibration(40, True)
    R0 = pkg.labor_egm_solve(guess.T, cal["a_grid"], cal["s"], cal["P"], r0, w, cal["beta"],
                             cal["sigma"], 1.0, 1.0, cal["amin"])
    pc0 = np.ascontiguousarray(R0["policy_c"].T)
    S = gb.bisection(gb.hip_egm_evaluator(cal, pc0, w, labor=True), -0.05, 1 / cal["beta"] - 1)
    assert A.r_history == S.r_history and A.k_supply == S.k_supply and A.iters[1:] == S.iters
    G = pkg.ge.aiyagari_labor_egm(Na=40)
    assert A.r_history == G["r_history"]
    assert A.r == 0.03924967447916673
    # the whole first round against the C loop: capped candidates among converged ones
    solve, simulate = _oracle_callables(cal, True)
    nodes = gb.subtree(-0.05, 1 / cal["beta"] - 1, 1, 6)
    got = gb.hip_egm_batch_evaluator(cal, pc0, w, labor=True).many(nodes)
    evo = gb.egm_evaluator(cal, solve, simulate, pc0, w, True)
    its = [v[2] for v in got]
    assert 1000 in its and min(its) < 1000
    assert got == [evo(n) for n in nodes]


def test_used_workspace_equals_fresh(pkg, gpu):
    """A batch, an ordinary solve, then a batch with another C on ONE workspace give what fresh
    workspaces give (the blocks grow; nothing cached leaks between calls)."""
    p = problem(7, 400, 9, False, 5.0, 1.0)
    CAP = cap_of(7)
    D = Dev(pkg, p)

    def fresh():
        ws = pkg.Workspace(7, 400)
        ws.set_egm_batch(1)
        return ws
    used = fresh()
    b1 = D.batch(used, np.arange(3), TOL, CAP)
    s1 = D.separate(used, 4, TOL, CAP)
    b2 = D.batch(used, np.arange(9), TOL, CAP)
    b3 = D.batch(used, np.arange(2), TOL, CAP)
    for got, args in ((b1, np.arange(3)), (b2, np.arange(9)), (b3, np.arange(2))):
        ref = D.batch(fresh(), args, TOL, CAP)
        for k in ("c", "pk", "it", "dist", "st"):
            assert same(got[k], ref[k]), k
    r1 = D.separate(fresh(), 4, TOL, CAP)
    assert s1["it"] == r1["it"] and same(s1["c"], r1["c"]) and same(s1["pk"], r1["pk"])


def test_default_dispatch_threshold(pkg, gpu):
    """The default threshold follows the measured cost model: the one-launch path
    from 2 candidates at the scripts' grid and from 4 at Na = 1,000; never for a single solve."""
    for Na, first in ((400, 2), (1000, 4)):
        p = problem(7, Na, first, False, 5.0, 1.0)
        D = Dev(pkg, p)
        ws = pkg.Workspace(7, Na)
        D.batch(ws, np.arange(first - 1), TOL, 3)
        assert ws.egm_batch_counts() == (0, first - 1)
        D.batch(ws, np.arange(first), TOL, 3)
        assert ws.egm_batch_counts() == (1, first - 1)
        ws.close()
