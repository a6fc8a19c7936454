"""GPU: the batched multi-rate labour VFI solve (aiy_labor_vfi_solve_batch_dev: one small-grid
launch per sweep over all candidates still running, each candidate stopped on the device) and its
GE entry points (aiy_labor_ge_batch, the gateway, the multisection driver).  Every comparison is
bit for bit: against the host-tier solve, candidate by candidate, and against the C restatement
(oracle/)."""
import math

import numpy as np
import pytest

from oracle import corc
from oracle import np_oracle as no

pytestmark = pytest.mark.gpu

BETA, ALPHA, DELTA, SIGMA, PSI, ETA = 0.96, 0.36, 0.08, 5.0, 1.0, 2.0
TOL = 0.1
# (N, Na, Nl, candidates, cap): the cap is the median of the C loop's iteration counts at
# max_iter = 400 (47-51, 8-44, 12-21, 12-21, 14-24, 12-22), so each call holds candidates that
# stop on tol and candidates that stop at the cap (asserted below, not trusted)
SHAPES = [(1, 2, 2, 70, 49), (2, 3, 3, 70, 36), (7, 63, 10, 70, 15), (7, 65, 16, 70, 15),
          (16, 128, 7, 70, 16), (7, 400, 10, 9, 15)]


def model(N, Na):
    if N == 7:
        cal = no.calib_aiyagari(Na=Na, rho=0.6, sigma_e=0.2)  # (the labour script's)
    elif N == 1:
        cal = dict(no.calib_aiyagari(Na=Na), s=np.array([1.0]), P=np.array([[1.0]]))
    elif N == 2:
        cal = dict(no.calib_aiyagari(Na=Na), s=np.array([0.6, 1.4]),
                   P=np.array([[0.8, 0.2], [0.3, 0.7]]))
    else:
        cal = no.calib_aiyagari(Na=Na, shocks="rouwenhorst", N=N)
    return cal["a_grid"], np.asarray(cal["s"], float), np.asarray(cal["P"], float)


def problem(N, Na, Nl, C, sigma=SIGMA):
    """C candidates on an (N, Na, Nl) model: r = -0.045 + 0.085 c/(C-1), w = wage(r) scaled by
    0.9 + 0.2 (C-1-c)/(C-1), start v = V0 scaled by 0.8 + 0.4 ((7c) mod C)/C, V0 = 6 oracle
    sweeps from 0 at r = 0.04."""
    a, s, P = model(N, Na)
    L = 0.01 + (1.5 - 0.01) * no.matlab_linspace01(Nl)
    f = np.arange(C) / max(C - 1, 1)
    r = -0.045 + 0.085 * f
    w = np.array([no.wage(x, ALPHA, DELTA) for x in r]) * (0.9 + 0.2 * f[::-1])
    V0 = corc.labor_vfi_solve(np.zeros((N, Na)), a, s, P, L, 0.04, no.wage(0.04, ALPHA, DELTA),
                              BETA, sigma, PSI, ETA, 1e-300, 6)["v_new"]
    v = np.stack([V0 * (0.8 + 0.4 * ((7 * c) % C) / C) for c in range(C)])
    return dict(N=N, Na=Na, Nl=Nl, C=C, a=a, s=s, P=P, L=L, r=r, w=w, v=v, sigma=sigma, beta=BETA)


def oracle_solve(p, c, tol, max_iter):
    return corc.labor_vfi_solve(p["v"][c], p["a"], p["s"], p["P"], p["L"], p["r"][c], p["w"][c],
                                p["beta"], p["sigma"], PSI, ETA, tol, max_iter)


KEYS = ("v_new", "v_old", "policy_k", "policy_l", "policy_c", "lin", "iters")


class Dev:
    def __init__(self, pkg, p):
        import torch
        self.pkg, self.p, self.torch = pkg, p, torch
        self.dev = torch.device("cuda", 0)
        self.a, self.s, self.P, self.L = (self.t(p[k]) for k in ("a", "s", "P", "L"))

    def t(self, x, dtype=np.float64):
        return self.torch.as_tensor(np.ascontiguousarray(x, dtype=dtype), device=self.dev)

    def batch(self, ws, sel, tol, max_iter, v_new=0.0, pol=(0.0, 0.0, 0.0), lin=0):
        """The candidates `sel` in one call -> list of per-candidate dicts (lin 0-based)."""
        p, n = self.p, len(sel)
        shape = (n, p["N"], p["Na"])
        va = self.t(p["v"][sel])
        vb = self.t(np.full(shape, v_new))
        pk, pl, pc = (self.t(np.full(shape, x)) for x in pol)
        li = self.t(np.full(shape, lin), np.int32)
        it, which = self.pkg.labor_solve_batch_dev(
            ws, p["r"][sel], p["w"][sel], va, vb, self.a, self.s, self.P, self.L, p["beta"],
            p["sigma"], PSI, ETA, tol, max_iter, li, pk, pl, pc)
        va, vb, pk, pl, pc, li = (x.cpu().numpy() for x in (va, vb, pk, pl, pc, li))
        return [dict(v_new=(vb if which[q] else va)[q], v_old=(va if which[q] else vb)[q],
                     policy_k=pk[q], policy_l=pl[q], policy_c=pc[q], lin=li[q], iters=it[q])
                for q in range(n)]

    def host(self, c, tol, max_iter):
        """Candidate c through the host-tier aiy_labor_vfi_solve (lin made 0-based)."""
        p = self.p
        R = self.pkg.labor_vfi_solve(p["v"][c], p["a"], p["s"], p["P"], p["L"], p["r"][c],
                                     p["w"][c], p["beta"], p["sigma"], PSI, ETA, tol, max_iter)
        return dict(R, lin=R["lin"] - 1)


def same(x, y):
    return np.array_equal(np.asarray(x), np.asarray(y))


def check_against(B, sel, refs):
    for q, c in enumerate(sel):
        for k in KEYS:
            assert same(B[q][k], refs[c][k]), (c, k)


@pytest.fixture(scope="module")
def oracle_runs():
    """Per shape, computed once: the problem, the C loop's iteration counts at max_iter = 400 and
    its results at the shape's cap (the uncapped run's where it stops within the cap: the loop is
    deterministic)."""
    cache = {}

    def get(shape):
        if shape not in cache:
            N, Na, Nl, C, cap = shape
            p = problem(N, Na, Nl, C)
            full = [oracle_solve(p, c, TOL, 400) for c in range(C)]
            refs = [R if R["iters"] <= cap else oracle_solve(p, c, TOL, cap)
                    for c, R in enumerate(full)]
            cache[shape] = (p, [R["iters"] for R in full], refs)
        return cache[shape]
    return get


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s[:3])))
def test_batched_equals_host_equals_oracle(pkg, gpu, oracle_runs, shape):
    """C in {1, 2, 7, all} candidates on the forced batched path == the host-tier solve == the C
    loop, candidate by candidate: v_new, v_old, lin, the policies, iters; one call holds
    candidates that stop on tol and candidates that stop at the cap.  Also max_iter = 1 and the
    default dispatch."""
    N, Na, Nl, C, CAP = shape
    p, full, refs = oracle_runs(shape)
    D = Dev(pkg, p)
    for c in range(C):  # host tier == oracle
        H = D.host(c, TOL, CAP)
        for k in KEYS:
            assert same(H[k], refs[c][k]), (c, k)
    # both stop kinds in one call, several counts.  A candidate that stops below the cap has
    # d < tol between its v_new and v_old; one that needs more than the cap uncapped had d >= tol
    # at the cap (an exhausted loop leaves v_old = v_new, so d is not read off its result)
    its = [R["iters"] for R in refs]
    dlast = [np.nanmax(np.abs(R["v_new"] - R["v_old"])) for R in refs]
    print("iteration counts at max_iter = 400:", sorted(set(full)))
    assert any(i < CAP and d < TOL for i, d in zip(its, dlast))
    assert any(i == CAP and f > CAP and d == 0.0 for i, f, d in zip(its, full, dlast))
    assert len(set(full)) >= 3, sorted(set(full))
    ws = pkg.Workspace(N, Na, Nl)
    ws.set_labor_batch(1)  # the batched path whatever C
    calls = 0
    for n in (1, 2, 7, C):
        sel = np.unique(np.round(np.linspace(0, C - 1, n)).astype(int)) if n > 1 \
            else np.array([C // 2])
        check_against(D.batch(ws, sel, TOL, CAP), sel, refs)
        calls += 1
    # max_iter = 1: every candidate exhausted after one sweep (or below tol at once)
    sel = np.array([0, C // 2, C - 1])
    one = {c: oracle_solve(p, c, TOL, 1) for c in sel}
    check_against(D.batch(ws, sel, TOL, 1), sel, one)
    calls += 1
    assert ws.labor_batch_counts() == (calls, 0)
    # the default dispatch (whatever the threshold) gives the same
    wd = pkg.Workspace(N, Na, Nl)
    for n in (1, 7):
        sel = (np.arange(n) * (C // 8 if C >= 56 else 1)) % C
        check_against(D.batch(wd, sel, TOL, CAP), sel, refs)
    ws.close()
    wd.close()


def _literal_loop(a, s, P, L, r, w, beta, v0, v_in, pol, tol, max_iter):
    """The script's loop over the C oracle's sweep (lin 0-based): sweep, stop test, v_old = v_new;
    exhausted: v_old = v_new after the last sweep."""
    v_old, v_new, p = v0.copy(), v_in.copy(), pol
    it, stopped = 0, False
    for it in range(1, max_iter + 1):
        v_new, p = corc.labor_vfi_sweep(v_old, a, s, P, L, r, w, beta, SIGMA, PSI, ETA,
                                        v_new=v_new, pol=p)
        if np.nanmax(np.abs(v_new - v_old)) < tol:
            stopped = True
            break
        v_old = v_new.copy()
    return dict(v_new=v_new, v_old=v_old, policy_k=p[0], policy_l=p[1], policy_c=p[2], lin=p[3],
                iters=it, stopped=stopped)


def test_infeasible_states_differ_per_candidate(pkg, gpu):
    """States with no feasible (l, a') (:85) keep the incoming v_new = 42 and policies, per
    candidate: the four candidates have 1, 2, 0 and 0 such states of 14; the literal loop needs
    13, 15, 114 and 76 sweeps at tol = 1e-2, so max_iter = 80 caps one of them."""
    a = np.array([0.5, 1.0, 2.0, 3.0, 4.5, 6.0, 8.0])
    s = np.array([0.2, 0.6])
    P = np.array([[0.7, 0.3], [0.4, 0.6]])
    L = np.array([0.4, 1.0])
    r = np.array([-0.5, -0.7, -0.2, 0.02])
    w = np.array([1.0, 1.0, 1.0, 1.3])
    beta, tol, max_iter = 0.9, 1e-2, 80
    v0 = np.zeros((2, 7))
    p = dict(N=2, Na=7, Nl=2, C=4, a=a, s=s, P=P, L=L, r=r, w=w, v=np.stack([v0] * 4), sigma=SIGMA,
             beta=beta)
    D = Dev(pkg, p)
    ws = pkg.Workspace(2, 7, 2)
    ws.set_labor_batch(1)
    B = D.batch(ws, np.arange(4), tol, max_iter, v_new=42.0, pol=(1.5, 2.5, 3.5), lin=2)
    assert ws.labor_batch_counts() == (1, 0)
    pol = (np.full((2, 7), 1.5), np.full((2, 7), 2.5), np.full((2, 7), 3.5),
           np.full((2, 7), 2, np.int32))
    n_inf, capped = [], []
    for c in range(4):
        R = _literal_loop(a, s, P, L, r[c], w[c], beta, v0, np.full((2, 7), 42.0), pol, tol,
                          max_iter)
        for k in KEYS:
            assert same(B[c][k], R[k]), (c, k)
        feasible = (1 + r[c]) * a[None, :] + w[c] * s[:, None] * L.max() > a[0]
        n_inf.append(int((~feasible).sum()))
        capped.append(not R["stopped"])
        assert np.all(B[c]["v_new"][~feasible] == 42.0) and np.all(B[c]["lin"][~feasible] == 2)
        assert np.all(B[c]["policy_k"][~feasible] == 1.5)
        assert np.all(B[c]["policy_l"][~feasible] == 2.5)
        assert np.all(B[c]["policy_c"][~feasible] == 3.5)
    assert n_inf == [1, 2, 0, 0]
    assert [B[c]["iters"] for c in range(4)] == [13, 15, 80, 76] and capped == [False, False, True, False]
    ws.close()


@pytest.mark.parametrize("N,Na,Nl,sigma", [(7, 2100, 10, 5.0), (7, 64, 17, 5.0), (7, 63, 10, 2.5)])
def test_fallback_shapes_take_the_per_candidate_path(pkg, gpu, N, Na, Nl, sigma):
    """Na above the one-launch sweep's bound, more labour levels than it holds in registers, a
    non-integer sigma: the same contract through the single-rate solve, candidate after candidate —
    and the counters say which path ran."""
    p = problem(N, Na, Nl, 2, sigma)
    D = Dev(pkg, p)
    ws = pkg.Workspace(N, Na, Nl)
    ws.set_labor_batch(1)
    B = D.batch(ws, np.arange(2), TOL, 3)
    assert ws.labor_batch_counts() == (0, 2)
    check_against(B, np.arange(2), [oracle_solve(p, c, TOL, 3) for c in range(2)])
    ws.close()


# ------------------------------------------------------------------ GE entry points
def _oracle_callables(cal, L, tol=1e-5, max_iter=1000):
    a, s, P = cal["a_grid"], cal["s"], cal["P"]

    def solve(st, r, w):  # (every state is feasible at these rates: the start's v_new is unread)
        return corc.labor_vfi_solve(st["v_old"], a, s, P, L, r, w, cal["beta"], cal["sigma"], PSI,
                                    ETA, tol, max_iter)

    def simulate(pk, z1, k1, u):
        return corc.sim_capital(pk, a, P, z1 - 1, k1, u)
    return solve, simulate


@pytest.fixture(scope="module")
def ge40(pkg, gpu):
    """Na = 40, T = 2,000: the calibration, the r0 solution and the 7 nodes of a 3-level tree with
    their oracle results (shared by the GE-batch and the gateway tests)."""
    gb = pkg.ge_batch
    cal, L = gb.labor_calibration(40)
    solve, simulate = _oracle_callables(cal, L)
    R0 = solve(dict(v_old=np.zeros((cal["N"], 40))), 0.04, no.wage(0.04, ALPHA, DELTA))
    start = gb.labor_start(dict(R0, lin=R0["lin"] + 1))
    nodes = gb.subtree(-0.05, 1 / cal["beta"] - 1, 1, 3)
    ev = gb.labor_vfi_evaluator(cal, solve, simulate, start, T=2000)
    head, blocks = gb.mc_stream(2000)
    z1 = int(math.ceil(cal["N"] * head[0]))
    k1 = cal["a_grid"][int(math.ceil(40 * head[1])) - 1]
    return dict(cal=cal, L=L, start=start, nodes=nodes, ref=[ev(n) for n in nodes], z1=z1, k1=k1,
                blocks=[blocks[n.depth] for n in nodes])


def test_labor_ge_batch_equals_oracle_per_node(pkg, gpu, ge40):
    g = ge40
    r = [n.r for n in g["nodes"]]
    for nd in (1, 2):  # one GPU: the library clamps n_devices, the result is identical
        Ks, Kd, it = pkg.ge_batch.labor_ge_batch_call(r, g["start"], g["cal"], g["L"], g["z1"],
                                                      g["k1"], g["blocks"], n_devices=nd)
        assert [float(x) for x in Ks] == [v[0] for v in g["ref"]]
        assert [float(x) for x in Kd] == [v[1] for v in g["ref"]]
        assert [int(x) for x in it] == [v[2] for v in g["ref"]]


def test_gateway_equals_library_call(pkg, gpu, ge40):
    from tests import mexstub
    g = ge40
    cal, st = g["cal"], g["start"]
    r = np.array([n.r for n in g["nodes"]])
    U = np.stack(g["blocks"], axis=1)
    Ks, Kd, it = pkg.ge_batch.labor_ge_batch_call(r, st, cal, g["L"], g["z1"], g["k1"], g["blocks"])
    pk, pl, pc, lin = st["policies"]
    out = mexstub.call("aiy_labor_ge_batch_mex", 3, r, st["v_old"], st["v_new"], pk, pl, pc,
                       lin.astype(np.float64), cal["a_grid"], cal["s"], cal["P"], g["L"],
                       cal["alpha"], cal["delta"], cal["beta"], cal["sigma"], PSI, ETA, cal["labor"],
                       1e-5, 1000.0, float(g["z1"]), g["k1"], U, 1.0)
    assert len(out) == 3 and all(o.shape == (7, 1) for o in out)
    assert np.array_equal(out[0].ravel(), Ks) and np.array_equal(out[1].ravel(), Kd)
    assert np.array_equal(out[2].ravel(), it)


def _multisection_checks(pkg, Na):
    gb = pkg.ge_batch
    A = gb.aiyagari_labor_vfi_multisection(Na=Na, levels=6)
    assert A.rounds == 2 and A.candidates == 63 + 15
    cal, L = gb.labor_calibration(Na)
    R0 = pkg.labor_vfi_solve(np.zeros((cal["N"], Na)), cal["a_grid"], cal["s"], cal["P"], L, 0.04,
                             no.wage(0.04, ALPHA, DELTA), cal["beta"], cal["sigma"], PSI, ETA)
    S = gb.bisection(gb.hip_labor_vfi_evaluator(cal, L, gb.labor_start(R0)), -0.05,
                     1 / cal["beta"] - 1)
    assert A.r_history == S.r_history and A.k_supply == S.k_supply
    assert A.k_demand == S.k_demand and A.iters[1:] == S.iters and A.iters[0] == R0["iters"]
    G = pkg.ge.aiyagari_labor_vfi(Na=Na)
    assert A.r_history == G["r_history"]
    return A


def test_multisection_at_na_40(pkg, gpu):
    """The script's GE at Na = 40, T = 10,000 in two batched rounds (63 + 15 candidates): the
    trace of the sequential bisection over the one-after-another evaluator, and the r path of the
    script's own chained warm start (ge.aiyagari_labor_vfi)."""
    A = _multisection_checks(pkg, 40)
    assert A.r == 0.01758626302083339


def test_multisection_at_the_script_defaults(pkg, gpu):
    """The same three assertions at Na = 400, GPU against GPU."""
    _multisection_checks(pkg, 400)


def test_default_levels_on_one_gpu(pkg, gpu):
    """The driver's single-GPU default is the measured LABOR_LEVELS_ONE_GPU; any levels give the
    same path."""
    gb = pkg.ge_batch
    A = gb.aiyagari_labor_vfi_multisection(Na=40)
    B = gb.aiyagari_labor_vfi_multisection(Na=40, levels=6)
    assert A.r_history == B.r_history and A.k_supply == B.k_supply and A.iters == B.iters
    assert A.rounds == -(-10 // gb.LABOR_LEVELS_ONE_GPU)


def test_used_workspace_equals_fresh(pkg, gpu):
    """A batch, a single labour sweep, a batch with another C, then an A1 batched solve, all on
    ONE workspace, give what fresh workspaces give."""
    import torch
    shape = SHAPES[2]
    N, Na, Nl, C, CAP = shape
    p = problem(N, Na, Nl, C)
    D = Dev(pkg, p)

    def fresh():
        ws = pkg.Workspace(N, Na, Nl)
        ws.set_labor_batch(1)
        return ws

    def sweep(ws):
        v = D.t(p["v"][3])
        out = [torch.zeros_like(v) for _ in range(4)]
        lin = torch.zeros((N, Na), dtype=torch.int32, device=D.dev)
        ws.labor_vfi_sweep(v, D.a, D.s, D.P, D.L, p["r"][3], p["w"][3], BETA, SIGMA, PSI, ETA,
                           out[0], lin, out[1], out[2], out[3])
        return [x.cpu().numpy() for x in out] + [lin.cpu().numpy()]

    def a1(ws):
        sel = np.arange(3)
        va, vb = D.t(p["v"][sel]), D.t(np.zeros((3, N, Na)))
        idx = torch.zeros((3, N, Na), dtype=torch.int32, device=D.dev)
        pk = torch.zeros_like(va)
        it, which = pkg.solve_batch_dev(ws, p["r"][sel], p["w"][sel], va, vb, D.a, D.s, D.P, BETA,
                                        SIGMA, TOL, CAP, idx, pk)
        return [va.cpu().numpy(), vb.cpu().numpy(), idx.cpu().numpy(), pk.cpu().numpy(), it, which]
    used = fresh()
    got = [D.batch(used, np.arange(3), TOL, CAP), sweep(used), D.batch(used, np.arange(9), TOL, CAP),
           a1(used)]
    ref = [D.batch(fresh(), np.arange(3), TOL, CAP), sweep(fresh()),
           D.batch(fresh(), np.arange(9), TOL, CAP), a1(fresh())]
    for q in (0, 2):
        for x, y in zip(got[q], ref[q]):
            for k in KEYS:
                assert same(x[k], y[k]), (q, k)
    for q in (1, 3):
        for x, y in zip(got[q], ref[q]):
            assert same(x, y), q


def test_default_dispatch_threshold(pkg, gpu):
    """The default threshold is the measured one: the batched path from
    2 candidates at the script's grid; never for a single solve."""
    p = problem(7, 400, 10, 2)
    D = Dev(pkg, p)
    ws = pkg.Workspace(7, 400, 10)
    D.batch(ws, np.arange(1), TOL, 3)
    assert ws.labor_batch_counts() == (0, 1)
    D.batch(ws, np.arange(2), TOL, 3)
    assert ws.labor_batch_counts() == (1, 1)
    ws.close()
