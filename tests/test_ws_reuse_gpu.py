"""Workspace ownership (csrc/ws.hpp, devbuf.hpp): one workspace driven through an order of calls
that makes every growable buffer (re)allocate at least once — the small-grid sweep, the tree, a
labour sweep (kf grows), the chunked screen (partial), another k_chunk (partial refilled),
tracing, speculative solves at batch 4 then 8 (rings released), rate batches with C = 3 then 2
(blocks released), an EGM step and solve, histogram pushes, capital simulations of growing T —
must give, call by call and bit for bit, what a freshly created workspace gives for the same call.
And the dynamic-LDS limit of the simulation kernels holds on every device, not only the first."""
import numpy as np
import pytest

from oracle import np_oracle as no

pytestmark = pytest.mark.gpu

R, BETA, SIGMA = 0.04, 0.96, 5.0
W = no.wage(R, 0.36, 0.08)


class _Case:
    def __init__(self, pkg, torch, N, Na, Nl):
        self.pkg, self.torch, self.N, self.Na, self.Nl = pkg, torch, N, Na, Nl
        self.dev = torch.device("cuda:0")
        cal = no.calib_aiyagari(Na=Na, N=N, shocks="rouwenhorst")
        a, s = cal["a_grid"], cal["s"]
        self.amin = cal["amin"]
        self.a, self.s, self.P = self.t(a), self.t(s), self.t(cal["P"])
        self.L = self.t(0.01 + (1.5 - 0.01) * no.matlab_linspace01(Nl))
        self.V0 = self.t(np.log1p(a - a[0])[None, :] * (1.0 + 0.1 * np.arange(N))[:, None] - 5.0)
        self.c0 = self.t(np.tile(((1 + R) * a + W * np.mean(s))[None, :], (N, 1)))
        self.lam0 = self.t(np.full((N, Na), 1.0 / (N * Na)))
        self.U = self.t(np.random.default_rng(7).uniform(size=8191))
        # a policy for the histogram and the simulation: the first sweep's, computed once
        ws = pkg.Workspace(N, Na, Nl)
        out = self.sweep(ws)
        ws.close()
        self.pol_idx, self.pol_k = self.t(out["idx"]), self.t(out["pk"])

    def t(self, x):
        return self.torch.as_tensor(np.ascontiguousarray(x), device=self.dev)

    def new(self, shape=None, dtype=None):
        shape = (self.N, self.Na) if shape is None else shape
        return self.torch.zeros(shape, dtype=dtype or self.torch.float64, device=self.dev)

    def get(self, **kw):
        self.torch.cuda.synchronize()
        return {k: (v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)) for k, v in kw.items()}

    # ------------------------------------------------------------------ the calls
    def sweep(self, ws):
        i32 = self.torch.int32
        v, pk, pc, idx, d = self.new(), self.new(), self.new(), self.new(dtype=i32), self.new((2,))
        ws.vfi_sweep(self.V0, self.a, self.s, self.P, R, W, BETA, SIGMA, v, idx, pk, pc, diff=d)
        return self.get(v=v, idx=idx, pk=pk, pc=pc, d=d)

    def labor(self, ws):
        v, pk, pl, pc, d = self.new(), self.new(), self.new(), self.new(), self.new((2,))
        lin = self.new(dtype=self.torch.int32)
        ws.labor_vfi_sweep(self.V0, self.a, self.s, self.P, self.L, R, W, BETA, SIGMA, 1.0, 2.0, v,
                           lin, pk, pl, pc, diff=d)
        return self.get(v=v, lin=lin, pk=pk, pl=pl, pc=pc, d=d)

    def solve(self, ws):
        va, vb, pk, pc = self.V0.clone(), self.new(), self.new(), self.new()
        idx = self.new(dtype=self.torch.int32)
        it, which = ws.vfi_solve(va, vb, self.a, self.s, self.P, R, W, BETA, SIGMA, 1e-5, 40, idx,
                                 pk, pc)
        return self.get(va=va, vb=vb, idx=idx, pk=pk, pc=pc, it=it, which=which)

    def batch(self, ws, C):
        r = R + 0.002 * np.arange(C)
        w = np.array([no.wage(x, 0.36, 0.08) for x in r])
        sh = (C, self.N, self.Na)
        va, vb, pk, pc = self.V0.repeat(C, 1, 1).contiguous(), self.new(sh), self.new(sh), self.new(sh)
        idx = self.new(sh, self.torch.int32)
        it, which = self.pkg.solve_batch_dev(ws, r, w, va, vb, self.a, self.s, self.P, BETA, SIGMA,
                                             1e-5, 30, idx, pk, pc)
        return self.get(va=va, vb=vb, idx=idx, pk=pk, pc=pc, it=it, which=which)

    def egm_step(self, ws):
        out, pk, d = self.new(), self.new(), self.new((2,))
        self.pkg.egm_step_dev(ws, self.c0, self.a, self.s, self.P, R, W, BETA, SIGMA, self.amin,
                              out, pk, diff=d)
        return self.get(out=out, pk=pk, d=d)

    def egm_solve(self, ws):
        c, pk = self.c0.clone(), self.new()
        it, dist = self.pkg.egm_solve_dev(ws, c, self.a, self.s, self.P, R, W, BETA, SIGMA,
                                          self.amin, 1e-5, 60, pk)
        return self.get(c=c, pk=pk, it=it, dist=dist)

    def dist(self, ws):
        out, out2, K, d = self.new(), self.new(), self.new((1,)), self.new((2,))
        it, dist = self.pkg.dist_stationary_dev(ws, self.lam0, self.a, self.P, out,
                                                policy_idx=self.pol_idx, tol=1e-10, max_iter=100,
                                                k_supply=K)
        self.pkg.dist_update_dev(ws, out, self.a, self.P, out2, policy_k=self.pol_k, diff=d)
        return self.get(out=out, out2=out2, K=K, d=d, it=it, dist=dist)

    def sim(self, ws, T):
        i32 = self.torch.int32
        K, st, sk, sz = self.new((1,)), self.new((4,), i32), self.new((T,)), self.new((T,), i32)
        self.pkg.sim_capital_dev(ws, self.pol_k, self.a, self.P, 0, float(self.a[self.Na // 2]),
                                 self.U[:T - 1], K, st, sim_k=sk, sim_z=sz)
        return self.get(K=K, st=st[:1], sk=sk, sz=sz)


def _apply(ws, state):
    ws.set_variant(state["variant"])
    ws.set_search(0, state["k_chunk"])
    ws.set_speculation(state["spec"])
    ws.set_timing(False, trace=state["trace"])


def _steps(c):
    """(name, settings that change before the call, the call)."""
    return [
        ("A1 default (wide)", {}, c.sweep),
        ("A1 tree", dict(variant=0), c.sweep),
        ("labour (kf grows)", {}, c.labor),
        ("chunked screen", dict(variant=8), c.sweep),
        ("another k_chunk", dict(k_chunk=64), c.sweep),
        ("tracing, chunked", dict(trace=True), c.sweep),
        ("tracing, tree", dict(variant=0), c.sweep),
        ("tracing, wide", dict(variant=-1), c.sweep),
        ("tracing, labour", {}, c.labor),
        ("speculative solve, batch 4", dict(trace=False, spec=4), c.solve),
        ("speculative solve, batch 8", dict(spec=8), c.solve),
        ("rate batch, C = 3", {}, lambda ws: c.batch(ws, 3)),
        ("rate batch, C = 2", {}, lambda ws: c.batch(ws, 2)),
        ("A1 after the batch", {}, c.sweep),
        ("EGM step", {}, c.egm_step),
        ("EGM solve", {}, c.egm_solve),
        ("EGM solve, traced", dict(trace=True), c.egm_solve),
        ("histogram", dict(trace=False), c.dist),
        ("histogram, traced", dict(trace=True), c.dist),
        ("simulation, T = 3000", dict(trace=False), lambda ws: c.sim(ws, 3000)),
        ("simulation, T = 8192", {}, lambda ws: c.sim(ws, 8192)),
        ("A1 at the end", {}, c.sweep),
    ]


def _used_equals_fresh(pkg, N, Na, Nl, steps=_steps):
    import torch
    c = _Case(pkg, torch, N, Na, Nl)
    state = dict(variant=-1, k_chunk=1024, spec=16, trace=False)
    used = pkg.Workspace(N, Na, Nl)
    for name, change, call in steps(c):
        state.update(change)
        _apply(used, state)
        got = call(used)
        fresh = pkg.Workspace(N, Na, Nl)
        _apply(fresh, state)
        want = call(fresh)
        fresh.close()
        assert got.keys() == want.keys()
        for k in want:
            assert np.array_equal(got[k], want[k], equal_nan=True), (name, k)
    used.close()


def test_used_workspace_equals_fresh_small(pkg, gpu):
    _used_equals_fresh(pkg, 3, 200, 4)


def test_used_workspace_equals_fresh_chained_egm(pkg, gpu):
    """Na = 1,100: the chained EGM solve (its second â / c̃ pair) and the tree labour sweep."""
    _used_equals_fresh(pkg, 3, 1100, 4)


def test_used_workspace_equals_fresh_sim_1024_tables(pkg, gpu):
    """Na = 900: the speculative-segment chain with its 1,024-entry tables, scratch growing."""
    _used_equals_fresh(pkg, 3, 900, 1, lambda c: [
        ("simulation, T = 2048", {}, lambda ws: c.sim(ws, 2048)),
        ("simulation, T = 4096", {}, lambda ws: c.sim(ws, 4096)),
        ("simulation, T = 2500", {}, lambda ws: c.sim(ws, 2500))])


def test_sim_capital_lds_limit_per_device(pkg, gpu):
    """The same chain on device 0 and then device 1 of one process, at a shape that needs more
    than 64 KiB of dynamic LDS (N = 7, Na = 900: 128 KiB of tables): the limit is per device, so
    it must be raised on each."""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two devices")
    N, Na, T = 7, 900, 4096
    cal = no.calib_aiyagari(Na=Na)
    a = cal["a_grid"]
    j = np.clip((0.97 * np.arange(Na)).astype(int)[None, :] + 4 * np.arange(N)[:, None], 0, Na - 1)
    U = np.random.default_rng(11).uniform(size=T - 1)
    res = []
    for d in (0, 1):
        with torch.cuda.device(d):
            dev = torch.device("cuda", d)
            t = lambda x: torch.as_tensor(np.ascontiguousarray(x), device=dev)
            ws = pkg.Workspace(N, Na)
            K = torch.zeros(1, dtype=torch.float64, device=dev)
            st = torch.zeros(4, dtype=torch.int32, device=dev)
            sk = torch.zeros(T, dtype=torch.float64, device=dev)
            sz = torch.zeros(T, dtype=torch.int32, device=dev)
            pkg.sim_capital_dev(ws, t(a[j]), t(a), t(cal["P"]), 3, float(a[Na // 2]), t(U), K, st,
                                sim_k=sk, sim_z=sz)
            torch.cuda.synchronize(dev)
            res.append((K.cpu().numpy(), int(st[0]), sk.cpu().numpy(), sz.cpu().numpy()))
            ws.close()
    assert res[0][1] == 0 and res[1][1] == 0
    assert np.array_equal(res[0][0], res[1][0]) and res[0][0][0] > 0
    assert np.array_equal(res[0][2], res[1][2]) and np.array_equal(res[0][3], res[1][3])
