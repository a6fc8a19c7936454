"""E2 / BASELINE config 4 — the general-equilibrium r search with many candidate interest
rates solved at once across ranks (one process per GPU, torch.distributed over RCCL).

The reference loop (Aiyagari_VFI.m:131-206) is a 10-step bisection: r = (r_low + r_high)/2,
solve, simulate K_s, compare with K_d, halve the bracket.  Its steps are sequential, but the
points it *may* visit are known in advance: the midpoints of the bisection tree.  A round
evaluates every node of the next L levels of that tree (2^L - 1 candidate rates, each node
computed from its parent bracket exactly as the sequential loop would, bit for bit), spread
round-robin over the ranks; one all-gather of (K_s, K_d) per round (the only collective,
8 bytes x 2 per candidate) lets every rank walk the path the sequential loop would take, with
its early stop |K_s - K_d| < 1e-5.  The all-gather is one float64 tensor collective
(all_gather_into_tensor over RCCL).  Two rounds of L = 6 cover the reference's 10 steps.

Path independence: a node's result must not depend on which nodes were solved before it on
the same rank.  Every candidate therefore starts its VFI from the same value function (the
solution at r0, "warm from r0"), and its Monte-Carlo supply uses the uniforms block of its
tree depth (the block the sequential loop would use at that step).  The sequential twin
`bisection(..., warm="r0")` gives the identical trace (tests/test_ge_batch_*.py); the
reference's own chained warm start (previous step's v_old) differs from it at the
convergence-tolerance level and is reproduced by ge.aiyagari_vfi.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import numpy as np


@dataclass
class Node:
    depth: int        # 1-based bisection step
    r: float
    lo: float
    hi: float


def subtree(lo: float, hi: float, depth0: int, levels: int) -> list[Node]:
    """The 2^levels - 1 midpoints below bracket (lo, hi), breadth-first, each computed as the
    sequential loop computes it: r = (lo + hi)/2 of its own bracket (Aiyagari_VFI.m:143)."""
    out, frontier = [], [(lo, hi)]
    for lev in range(levels):
        nxt = []
        for (a, b) in frontier:
            m = (a + b) / 2
            out.append(Node(depth0 + lev, m, a, b))
            nxt += [(a, m), (m, b)]
        frontier = nxt
    return out


@dataclass
class Trace:
    r_history: list = field(default_factory=list)
    k_supply: list = field(default_factory=list)
    k_demand: list = field(default_factory=list)
    iters: list = field(default_factory=list)
    r: float = math.nan
    rounds: int = 0
    candidates: int = 0


class NodeFailed(RuntimeError):
    """The sequential loop's path visits a candidate whose evaluation failed (status != 0)."""

    def __init__(self, node, status):
        super().__init__(f"bisection step {node.depth} at r = {node.r!r}: candidate status "
                         f"{status} (1: endogenous grid not increasing, 2: find() empty)")
        self.node, self.status = node, status


def _unpack(node, v):
    """(K_s, K_d, iters) of a node's result; a result may carry a fourth field, its status
    (the EGM evaluators): non-zero raises NodeFailed — only where the path reads the node."""
    if len(v) > 3 and v[3] != 0:
        raise NodeFailed(node, int(v[3]))
    return v[0], v[1], v[2]


def walk(nodes: list[Node], res: dict, lo: float, hi: float, steps: int, tr: Trace, tol: float):
    """Follow the sequential loop's path through an evaluated subtree (Aiyagari_VFI.m:195-204).
    Returns (lo, hi, stopped).  Raises NodeFailed when the path visits a node whose result
    carries a non-zero status; failed nodes off the path are ignored."""
    by_key = {(n.lo, n.hi): n for n in nodes}
    for _ in range(steps):
        n = by_key[(lo, hi)]
        Ks, Kd, it = _unpack(n, res[(n.lo, n.hi)])
        tr.r_history.append(n.r); tr.k_supply.append(Ks); tr.k_demand.append(Kd)
        tr.iters.append(it)
        tr.r = n.r
        if abs(Ks - Kd) < tol:
            return lo, hi, True
        if Ks > Kd:
            hi = n.r
        else:
            lo = n.r
    return lo, hi, False


def multisection(evaluate, r_low, r_high, max_steps=10, levels=6, tol=1e-5, rank=0, world=1,
                 allgather=None) -> Trace:
    """evaluate(node) -> (K_s, K_d, iters) for the nodes this rank owns (index % world == rank),
    or, when `evaluate` has an `many` attribute, evaluate.many(nodes) -> list of triples for all
    of them at once (the batched device path); allgather(mine, n_nodes) -> list over ranks of
    lists (None when world == 1; torch_allgather: one tensor all-gather per round)."""
    tr = Trace()
    lo, hi, done, step = r_low, r_high, False, 0
    while not done and step < max_steps:
        L = min(levels, max_steps - step)
        nodes = subtree(lo, hi, step + 1, L)
        own = [q for q in range(len(nodes)) if q % world == rank]
        if hasattr(evaluate, "many"):
            mine = list(zip(own, evaluate.many([nodes[q] for q in own]))) if own else []
        else:
            mine = [(q, evaluate(nodes[q])) for q in own]
        if world > 1:
            parts = allgather(mine, len(nodes))
            allres = [x for part in parts for x in part]
        else:
            allres = mine
        res = {(nodes[q].lo, nodes[q].hi): v for q, v in allres}
        lo, hi, done = walk(nodes, res, lo, hi, L, tr, tol)
        step += L
        tr.rounds += 1
        tr.candidates += len(nodes)
    return tr


def bisection(evaluate, r_low, r_high, max_steps=10, tol=1e-5) -> Trace:
    """The sequential twin (the reference loop's control flow) over the same evaluator."""
    tr = Trace()
    lo, hi = r_low, r_high
    for step in range(max_steps):
        n = Node(step + 1, (lo + hi) / 2, lo, hi)
        Ks, Kd, it = _unpack(n, evaluate(n))
        tr.r_history.append(n.r); tr.k_supply.append(Ks); tr.k_demand.append(Kd)
        tr.iters.append(it)
        tr.r = n.r
        tr.candidates += 1
        if abs(Ks - Kd) < tol:
            break
        if Ks > Kd:
            hi = n.r
        else:
            lo = n.r
    tr.rounds = len(tr.r_history)
    return tr


def torch_allgather(mine, n_nodes, fields=3):
    """The round's one collective (Aiyagari_VFI.m:193-204's decision inputs): every rank's
    (q, K_s, K_d, iters) rows as one float64 tensor [ceil(n_nodes / world), 4] (padding rows
    q = -1), gathered with all_gather_into_tensor — RCCL on GPU ranks (the tensor lives on the
    rank's current device), gloo on CPU.  All four fields are exact in float64 (q, iters are
    small integers).  Returns the list over ranks of [(q, (K_s, K_d, iters)), ...].
    fields=4 (the EGM evaluators): a fifth column carries each result's status."""
    import torch
    import torch.distributed as dist
    world = dist.get_world_size()
    rows = -(-n_nodes // world)
    if len(mine) > rows:
        raise ValueError(f"{len(mine)} results on one rank, at most {rows} expected")
    dev = (torch.device("cuda", torch.cuda.current_device())
           if dist.get_backend() == "nccl" else torch.device("cpu"))
    buf = torch.full((rows, 1 + fields), -1.0, dtype=torch.float64)
    for n, (q, v) in enumerate(mine):
        buf[n] = torch.tensor([q, *v[:fields]], dtype=torch.float64)
    out = torch.empty((world * rows, 1 + fields), dtype=torch.float64, device=dev)
    dist.all_gather_into_tensor(out, buf.to(dev))
    got = out.cpu().view(world, rows, 1 + fields).tolist()
    return [[(int(x[0]), (x[1], x[2], *(int(y) for y in x[3:]))) for x in part if x[0] >= 0]
            for part in got]


# ------------------------------------------------------------------------------ evaluators
def mc_stream(T=10000, steps=10, seed=5489):
    """MATLAB's fresh-session rand stream split as the VFI script consumes it: randi(N),
    randi(Na), then one block of T-1 uniforms per simulation (initial solve, then step d)."""
    u = np.random.RandomState(seed).random_sample(2 + (T - 1) * (steps + 1))
    head = u[:2]
    blocks = [u[2 + b * (T - 1): 2 + (b + 1) * (T - 1)] for b in range(steps + 1)]
    return head, blocks


def _stream_start(cal, T):
    """(z1, k1, blocks) as the scripts draw them from mc_stream(T): z1 = randi(N) (1-based),
    k1 = a_grid(randi(Na)), then one block of uniforms per simulation."""
    head, blocks = mc_stream(T)
    z1 = int(math.ceil(cal["N"] * head[0]))
    k1 = cal["a_grid"][int(math.ceil(cal["Na"] * head[1])) - 1]
    return z1, k1, blocks


def _with_many(many):
    """The evaluator that multisection and bisection take, from many(nodes) -> list of results:
    one node is a batch of one, a round goes through `.many`."""
    def evaluate(node):
        return many([node])[0]
    evaluate.many = many
    return evaluate


def _batch_arrays(r, cal, blocks=None, w=None, ints=(np.int64,)):
    """What every *_batch_call hands the library, in the layouts it reads: the rates, the wage per
    rate (w: a scalar or one per rate; None stays None), a_grid, s, P (column-major), the
    (T-1) x C uniforms matrix of `blocks` (None stays None) and the outputs [K_s, K_d, one array
    per dtype in `ints`].  Returns (r, w, a, s, P, U, outputs)."""
    r = np.ascontiguousarray(r, np.float64)
    n = r.size
    if w is not None:
        w = np.ascontiguousarray(np.broadcast_to(np.asarray(w, np.float64), (n,)))
    U = None
    if blocks is not None:
        U = np.asfortranarray(np.stack([np.asarray(b, np.float64) for b in blocks], axis=1))
    a = np.ascontiguousarray(cal["a_grid"], np.float64)
    s = np.ascontiguousarray(cal["s"], np.float64)
    P = np.asfortranarray(cal["P"], dtype=np.float64)
    return r, w, a, s, P, U, [np.empty(n), np.empty(n)] + [np.empty(n, t) for t in ints]


def vfi_evaluator(cal, solve, simulate, v_start, T=10000, tol=1e-5, max_iter=1000):
    """Node evaluator for Aiyagari_VFI.m: VFI from v_start (path-independent warm start), MC
    supply with the uniforms block of the node's depth, K_d (:195).
    solve(v_old, r, w) -> dict(policy_k, iters); simulate(policy_k, z1, k1, uniforms) -> K_s."""
    from . import calibration as cb
    z1, k1, blocks = _stream_start(cal, T)

    def evaluate(node):
        r = node.r
        R = solve(v_start, r, cb.wage(r, cal["alpha"], cal["delta"]))
        Ks = simulate(R["policy_k"], z1, k1, blocks[node.depth])
        Kd = cb.capital_demand(r, cal["labor"], cal["alpha"], cal["delta"])
        return (float(Ks), float(Kd), int(R["iters"]))
    return evaluate


def hip_vfi_evaluator(cal, v_start, T=10000, tol=1e-5, max_iter=1000):
    """The evaluator on this rank's GPU through the C ABI (host tier)."""
    from .sim import sim_capital
    from .vfi import vfi_solve

    def solve(v, r, w):
        return vfi_solve(v, cal["a_grid"], cal["s"], cal["P"], r, w, cal["beta"], cal["sigma"],
                         tol, max_iter)

    def simulate(pk, z1, k1, u):
        return sim_capital(pk, cal["a_grid"], cal["P"], z1, k1, u)
    return vfi_evaluator(cal, solve, simulate, v_start, T, tol, max_iter)


def ge_batch_call(r, v_start, cal, z1, k1, blocks, tol=1e-5, max_iter=1000, n_devices=1):
    """aiy_ge_batch (C ABI): K_s, K_d and iteration count at every rate in `r`, each
    from v_start, with uniforms blocks[c] (T-1 draws) for candidate c; z1 1-based."""
    from ._capi import check, d, i64, ip, lib, ptr
    r, _, a, s, P, U, (Ks, Kd, it) = _batch_arrays(r, cal, blocks)
    v = np.asfortranarray(v_start, dtype=np.float64)
    check(lib().aiy_ge_batch(ptr(r), i64(r.size), ptr(v), ptr(a), ptr(s), ptr(P), i64(cal["N"]),
                             i64(cal["Na"]), d(cal["alpha"]), d(cal["delta"]), d(cal["beta"]),
                             d(cal["sigma"]), d(cal["labor"]), d(tol), i64(max_iter), i64(z1),
                             d(k1), i64(U.shape[0] + 1), ptr(U), ip(n_devices), ptr(Ks), ptr(Kd),
                             ptr(it)))
    return Ks, Kd, it


def hip_batch_evaluator(cal, v_start, T=10000, tol=1e-5, max_iter=1000, n_devices=1):
    """The node evaluator on the batched device path: all of a round's nodes of this rank in
    one aiy_ge_batch call (one batched solve and one batched launch of the chains per GPU).
    Same per-node arithmetic as vfi_evaluator, so the traces are identical."""
    z1, k1, blocks = _stream_start(cal, T)

    def many(nodes):
        Ks, Kd, it = ge_batch_call([n.r for n in nodes], v_start, cal, z1, k1,
                                   [blocks[n.depth] for n in nodes], tol, max_iter, n_devices)
        return [(float(Ks[q]), float(Kd[q]), int(it[q])) for q in range(len(nodes))]
    return _with_many(many)


def auto_levels(world: int) -> int:
    """Tree levels per round so that one round's 2^L - 1 candidates fit the ranks (one each)."""
    return max(1, int(math.floor(math.log2(world + 1))))


def aiyagari_vfi_multisection(Na=400, levels=None, rank=0, world=1, allgather=None, r0=0.04,
                              shocks="tauchen", batched=True, supply="mc"):
    """Config 4: the GE of Aiyagari_VFI.m with candidate rates spread over `world` ranks.
    Every rank solves r0 once (the common warm start), then the rounds; batched=True evaluates
    each rank's nodes of a round in one batched device call (else one solve after another).
    levels=None picks auto_levels(world); BASELINE's 64-candidate configuration is levels=6.
    supply="histogram": K_s from the stationary histogram (A10) of each candidate's policy, a
    round's histograms in one batched solve (hip_hist_batch_evaluator), in place of the chains."""
    if supply not in ("mc", "histogram"):
        raise ValueError(f"supply must be 'mc' or 'histogram', not {supply!r}")
    levels = auto_levels(world) if levels is None else levels
    from . import calibration as cb
    from .vfi import vfi_solve
    cal = cb.aiyagari(Na=Na, shocks=shocks)
    R0 = vfi_solve(np.zeros((cal["N"], Na)), cal["a_grid"], cal["s"], cal["P"], r0,
                   cb.wage(r0, cal["alpha"], cal["delta"]), cal["beta"], cal["sigma"])
    lo, hi = -0.05, 1 / cal["beta"] - 1
    if supply == "histogram":
        import functools
        ev = (hip_hist_batch_evaluator if batched else hip_hist_evaluator)(cal, R0["v_old"])
        if allgather is None and world > 1:
            allgather = functools.partial(torch_allgather, fields=5)
        return multisection(ev, lo, hi, levels=levels, rank=rank, world=world, allgather=allgather)
    ev = (hip_batch_evaluator if batched else hip_vfi_evaluator)(cal, R0["v_old"])
    return multisection(ev, lo, hi, levels=levels, rank=rank, world=world,
                        allgather=allgather if allgather else (torch_allgather if world > 1 else None))


# ------------------------------------------------------------------- the EGM scripts (E2)
def egm_calibration(Na=400, labor=False):
    """The EGM scripts' calibration (labour: rho = .6, sigma_e = .2), the wage they freeze at
    r0 = 0.04 (Aiyagari_EGM.m:61, labour :55) and the :64 starting policy_c [N][Na]."""
    from . import calibration as cb
    cal = cb.aiyagari(Na=Na, rho=0.6 if labor else 0.75, sigma_e=0.2 if labor else 0.75)
    r0 = 0.04
    w = cb.wage(r0, cal["alpha"], cal["delta"])
    guess = np.tile((1 + r0) * cal["a_grid"] + w * np.mean(cal["s"]), (cal["N"], 1))
    return cal, r0, w, guess


def egm_evaluator(cal, solve, simulate, pc_start, w, labor=False, T=10000):
    """Node evaluator for Aiyagari_EGM.m / Aiyagari_Endogenous_Labor_EGM.m: the EGM solve from
    pc_start (the path-independent warm start) at the node's r and the scripts' stale w, MC
    supply with the uniforms block of the node's depth, K_d.  Generic in the two callables (the
    GPU path or the C oracle): solve(pc_start, r, w) -> dict(policy_k, iters[, status]);
    simulate(policy_k, z1, k1, uniforms) -> K_s.  `labor` only documents which script the
    callables restate.  Results are (K_s, K_d, iters, status); K_s is NaN where status != 0."""
    from . import calibration as cb
    z1, k1, blocks = _stream_start(cal, T)

    def evaluate(node):
        R = solve(pc_start, node.r, w)
        st = int(R.get("status", 0))
        Ks = math.nan if st else simulate(R["policy_k"], z1, k1, blocks[node.depth])
        Kd = cb.capital_demand(node.r, cal["labor"], cal["alpha"], cal["delta"])
        return (float(Ks), float(Kd), int(R["iters"]), st)
    return evaluate


def _hip_egm_solve(cal, labor, tol, max_iter, phi, theta):
    """solve(pc [N][Na], r, w) -> the host tier's EGM solve of the script `labor` names; where it
    refuses an endogenous grid that is not increasing, dict(policy_k=None, iters=0, status=1)."""
    from ._capi import AiyError
    from .egm import egm_solve, labor_egm_solve
    a, s, P = cal["a_grid"], cal["s"], cal["P"]

    def solve(pc, r, w):
        try:
            if labor:
                return labor_egm_solve(pc.T, a, s, P, r, w, cal["beta"], cal["sigma"], phi, theta,
                                       cal["amin"], tol, max_iter)
            return egm_solve(pc.T, a, s, P, r, w, cal["beta"], cal["sigma"], cal["amin"], tol,
                             max_iter)
        except AiyError as e:
            if "not increasing" not in str(e):
                raise
            return dict(policy_k=None, iters=0, status=1)
    return solve


def hip_egm_evaluator(cal, pc_start, w, labor=False, T=10000, tol=1e-5, max_iter=1000, phi=1.0,
                      theta=1.0):
    """The evaluator on this rank's GPU, one solve after another (host tier); pc_start [N][Na]."""
    from .sim import sim_capital
    a, P = cal["a_grid"], cal["P"]
    solve = _hip_egm_solve(cal, labor, tol, max_iter, phi, theta)

    def simulate(pk, z1, k1, u):
        return sim_capital(pk, a, P, z1, k1, u, vfi_layout=False)
    return egm_evaluator(cal, solve, simulate, pc_start, w, labor, T)


def egm_ge_batch_call(r, w, pc_start, cal, z1, k1, blocks, labor=False, phi=1.0, theta=1.0,
                      tol=1e-5, max_iter=1000, n_devices=1):
    """aiy_egm_ge_batch (C ABI): K_s, K_d, iteration count and status at every rate in `r`, each
    from pc_start ([N][Na]) at wage w (a scalar or one per rate), with uniforms blocks[c]
    (T-1 draws) for candidate c; z1 1-based."""
    from ._capi import check, d, i64, ip, lib, ptr
    r, w, a, s, P, U, (Ks, Kd, it, st) = _batch_arrays(r, cal, blocks, w, (np.int64, np.int32))
    n, N, Na, T = r.size, cal["N"], cal["Na"], U.shape[0] + 1
    pc = np.ascontiguousarray(pc_start, np.float64)  # [N][Na] == the script's Na x N
    if pc.shape != (N, Na):
        raise ValueError(f"pc_start must be [N][Na] = {(N, Na)}")
    check(lib().aiy_egm_ge_batch(ptr(r), ptr(w), i64(n), ptr(pc), ptr(a), ptr(s), ptr(P), i64(N),
                                 i64(Na), d(cal["alpha"]), d(cal["delta"]), d(cal["beta"]),
                                 d(cal["sigma"]), d(cal["amin"]), ip(1 if labor else 0), d(phi),
                                 d(theta), d(cal["labor"]), d(tol), i64(max_iter), i64(z1),
                                 d(k1), i64(T), ptr(U), ip(n_devices), ptr(Ks), ptr(Kd), ptr(it),
                                 ptr(st)))
    return Ks, Kd, it, st


def hip_egm_batch_evaluator(cal, pc_start, w, labor=False, T=10000, tol=1e-5, max_iter=1000,
                            n_devices=1, phi=1.0, theta=1.0):
    """The node evaluator on the batched device path: all of a round's nodes of this rank in
    one aiy_egm_ge_batch call (one launch of the solves and one of the chains per GPU).  Same
    per-node arithmetic as hip_egm_evaluator, so the traces are identical."""
    z1, k1, blocks = _stream_start(cal, T)

    def many(nodes):
        Ks, Kd, it, st = egm_ge_batch_call([n.r for n in nodes], w, pc_start, cal, z1, k1,
                                           [blocks[n.depth] for n in nodes], labor, phi, theta,
                                           tol, max_iter, n_devices)
        return [(float(Ks[q]), float(Kd[q]), int(it[q]), int(st[q])) for q in range(len(nodes))]
    return _with_many(many)


def aiyagari_egm_multisection(Na=400, labor=False, levels=None, rank=0, world=1, allgather=None,
                              batched=True, T=10000, tol=1e-5, max_iter=1000, phi=1.0, theta=1.0,
                              supply="mc"):
    """The GE of Aiyagari_EGM.m (labor: Aiyagari_Endogenous_Labor_EGM.m) with the candidate
    rates of the next `levels` bisection steps evaluated at once.  Every rank solves r0 = 0.04
    from the :64 guess, then the rounds, every candidate from that policy at the scripts' stale
    w; batched=True runs a round's nodes of this rank in one aiy_egm_ge_batch call.  The scripts'
    chained warm start takes the same bracket decisions (tests/test_egm_batch_gpu.py).
    supply="histogram": K_s from the lottery histogram (A10) of each candidate's policy_k, a
    round's histograms in one batched solve (hip_egm_hist_batch_evaluator)."""
    import functools
    from .egm import egm_solve, labor_egm_solve
    if supply not in ("mc", "histogram"):
        raise ValueError(f"supply must be 'mc' or 'histogram', not {supply!r}")
    levels = auto_levels(world) if levels is None else levels
    cal, r0, w, guess = egm_calibration(Na, labor)
    a, s, P = cal["a_grid"], cal["s"], cal["P"]
    if labor:
        R0 = labor_egm_solve(guess.T, a, s, P, r0, w, cal["beta"], cal["sigma"], phi, theta,
                             cal["amin"], tol, max_iter)
    else:
        R0 = egm_solve(guess.T, a, s, P, r0, w, cal["beta"], cal["sigma"], cal["amin"], tol,
                       max_iter)
    pc0 = np.ascontiguousarray(R0["policy_c"].T)
    if supply == "histogram":
        ev = (hip_egm_hist_batch_evaluator if batched else hip_egm_hist_evaluator)(
            cal, pc0, w, labor, tol, max_iter, phi=phi, theta=theta)
    elif batched:
        ev = hip_egm_batch_evaluator(cal, pc0, w, labor, T, tol, max_iter, 1, phi, theta)
    else:
        ev = hip_egm_evaluator(cal, pc0, w, labor, T, tol, max_iter, phi, theta)
    if allgather is None and world > 1:
        allgather = functools.partial(torch_allgather, fields=5 if supply == "histogram" else 4)
    tr = multisection(ev, -0.05, 1 / cal["beta"] - 1, levels=levels, rank=rank, world=world,
                      allgather=allgather)
    tr.iters = [int(R0["iters"])] + tr.iters
    return tr


# --------------------------------------------- the histogram supply (A10) in the GE rounds
# the stopping rule ge.py's supply="histogram" uses
HIST_TOL, HIST_MAX_ITER = 1e-13, 100000


def hist_evaluator(cal, solve, supply, start):
    """Node evaluator with the stationary histogram (A10) as the supply estimator: no sampling
    noise, so a node's result depends on its rate alone.  Generic in the two callables (the GPU
    path or the C oracle): solve(start, r) -> dict(iters[, status], the policy) from the
    path-independent warm start (the callable fixes the wage: Aiyagari_VFI.m's follows r, the EGM
    scripts keep theirs); supply(R) -> (K_s, pushes) on that policy.  Results are
    (K_s, K_d, iters, status, dist_iters); K_s is NaN and dist_iters 0 where status != 0."""
    from . import calibration as cb

    def evaluate(node):
        R = solve(start, node.r)
        st = int(R.get("status", 0))
        Ks, pushes = (math.nan, 0) if st else supply(R)
        Kd = cb.capital_demand(node.r, cal["labor"], cal["alpha"], cal["delta"])
        return (float(Ks), float(Kd), int(R["iters"]), st, int(pushes))
    return evaluate


def hip_hist_evaluator(cal, v_start, tol=1e-5, max_iter=1000, dist_tol=HIST_TOL,
                       dist_max_iter=HIST_MAX_ITER, lam_start=None):
    """hist_evaluator on this rank's GPU, one VFI solve and one histogram after another."""
    from . import calibration as cb
    from .dist import dist_stationary
    from .vfi import vfi_solve
    a, s, P = cal["a_grid"], cal["s"], cal["P"]

    def solve(v, r):
        return vfi_solve(v, a, s, P, r, cb.wage(r, cal["alpha"], cal["delta"]), cal["beta"],
                         cal["sigma"], tol, max_iter)

    def supply(R):
        _, K, it, _ = dist_stationary(a, P, policy_idx=R["idx"], lam0=lam_start, tol=dist_tol,
                                      max_iter=dist_max_iter)
        return K, it
    return hist_evaluator(cal, solve, supply, v_start)


def hip_egm_hist_evaluator(cal, pc_start, w, labor=False, tol=1e-5, max_iter=1000,
                           dist_tol=HIST_TOL, dist_max_iter=HIST_MAX_ITER, lam_start=None, phi=1.0,
                           theta=1.0):
    """hist_evaluator on this rank's GPU for the EGM scripts (pc_start, lam_start [N][Na]), one
    solve and one lottery histogram after another."""
    from .dist import dist_stationary
    a, P = cal["a_grid"], cal["P"]
    solve = _hip_egm_solve(cal, labor, tol, max_iter, phi, theta)

    def supply(R):
        _, K, it, _ = dist_stationary(a, P, policy_k=R["policy_k"],
                                      lam0=None if lam_start is None else np.asarray(lam_start).T,
                                      tol=dist_tol, max_iter=dist_max_iter, vfi_layout=False)
        return K, it
    return hist_evaluator(cal, lambda pc, r: solve(pc, r, w), supply, pc_start)


def ge_hist_batch_call(r, v_start, cal, tol=1e-5, max_iter=1000, dist_tol=HIST_TOL,
                       dist_max_iter=HIST_MAX_ITER, lam_start=None, n_devices=1):
    """aiy_ge_hist_batch (C ABI): K_s (histogram), K_d, VFI sweeps and pushes at every rate in
    `r`, each from v_start and lam_start (N x Na; None: uniform)."""
    from ._capi import check, d, i64, ip, lib, ptr
    r, _, a, s, P, _, (Ks, Kd, it, dit) = _batch_arrays(r, cal, ints=(np.int64, np.int64))
    n, N, Na = r.size, cal["N"], cal["Na"]
    v = np.asfortranarray(v_start, dtype=np.float64)
    lam = None if lam_start is None else np.asfortranarray(lam_start, dtype=np.float64)
    if lam is not None and lam.shape != (N, Na):
        raise ValueError(f"lam_start must be (N, Na) = {(N, Na)}")
    check(lib().aiy_ge_hist_batch(ptr(r), i64(n), ptr(v), ptr(a), ptr(s), ptr(P), i64(N), i64(Na),
                                  d(cal["alpha"]), d(cal["delta"]), d(cal["beta"]),
                                  d(cal["sigma"]), d(cal["labor"]), d(tol), i64(max_iter),
                                  d(dist_tol), i64(dist_max_iter), ptr(lam), ip(n_devices),
                                  ptr(Ks), ptr(Kd), ptr(it), ptr(dit)))
    return Ks, Kd, it, dit


def egm_ge_hist_batch_call(r, w, pc_start, cal, labor=False, phi=1.0, theta=1.0, tol=1e-5,
                           max_iter=1000, dist_tol=HIST_TOL, dist_max_iter=HIST_MAX_ITER,
                           lam_start=None, n_devices=1):
    """aiy_egm_ge_hist_batch (C ABI): K_s (lottery histogram), K_d, EGM steps, pushes and status
    at every rate in `r`, each from pc_start and lam_start ([N][Na]; None: uniform) at wage w
    (a scalar or one per rate)."""
    from ._capi import check, d, i64, ip, lib, ptr
    r, w, a, s, P, _, (Ks, Kd, it, dit, st) = _batch_arrays(
        r, cal, w=w, ints=(np.int64, np.int64, np.int32))
    n, N, Na = r.size, cal["N"], cal["Na"]
    pc = np.ascontiguousarray(pc_start, np.float64)  # [N][Na] == the script's Na x N
    lam = None if lam_start is None else np.ascontiguousarray(lam_start, np.float64)
    if pc.shape != (N, Na) or (lam is not None and lam.shape != (N, Na)):
        raise ValueError(f"pc_start and lam_start must be [N][Na] = {(N, Na)}")
    check(lib().aiy_egm_ge_hist_batch(ptr(r), ptr(w), i64(n), ptr(pc), ptr(a), ptr(s), ptr(P),
                                      i64(N), i64(Na), d(cal["alpha"]), d(cal["delta"]),
                                      d(cal["beta"]), d(cal["sigma"]), d(cal["amin"]),
                                      ip(1 if labor else 0), d(phi), d(theta), d(cal["labor"]),
                                      d(tol), i64(max_iter), d(dist_tol), i64(dist_max_iter),
                                      ptr(lam), ip(n_devices), ptr(Ks), ptr(Kd), ptr(it), ptr(dit),
                                      ptr(st)))
    return Ks, Kd, it, dit, st


def hip_hist_batch_evaluator(cal, v_start, tol=1e-5, max_iter=1000, dist_tol=HIST_TOL,
                             dist_max_iter=HIST_MAX_ITER, lam_start=None, n_devices=1):
    """hist_evaluator on the batched device path: all of a round's nodes of this rank in one
    aiy_ge_hist_batch call (one batched VFI solve and one batched histogram solve per GPU).
    Same per-node arithmetic as hip_hist_evaluator, so the traces are identical."""
    def many(nodes):
        Ks, Kd, it, dit = ge_hist_batch_call([n.r for n in nodes], v_start, cal, tol, max_iter,
                                             dist_tol, dist_max_iter, lam_start, n_devices)
        return [(float(Ks[q]), float(Kd[q]), int(it[q]), 0, int(dit[q]))
                for q in range(len(nodes))]
    return _with_many(many)


def hip_egm_hist_batch_evaluator(cal, pc_start, w, labor=False, tol=1e-5, max_iter=1000,
                                 dist_tol=HIST_TOL, dist_max_iter=HIST_MAX_ITER, lam_start=None,
                                 n_devices=1, phi=1.0, theta=1.0):
    """The same for the EGM scripts: one aiy_egm_ge_hist_batch call per round (one launch of the
    solves and one of the lottery histograms per GPU)."""
    def many(nodes):
        Ks, Kd, it, dit, st = egm_ge_hist_batch_call([n.r for n in nodes], w, pc_start, cal, labor,
                                                     phi, theta, tol, max_iter, dist_tol,
                                                     dist_max_iter, lam_start, n_devices)
        return [(float(Ks[q]), float(Kd[q]), int(it[q]), int(st[q]), int(dit[q]))
                for q in range(len(nodes))]
    return _with_many(many)


# ------------------------------------------------------- the labour VFI script (E2)
def labor_calibration(Na=400):
    """Aiyagari_Endogenous_Labor_VFI.m's calibration (rho = .6, sigma_e = .2) and its 10 labour
    levels."""
    from . import calibration as cb
    cal = cb.aiyagari(Na=Na, rho=0.6, sigma_e=0.2)
    return cal, 0.01 + (1.5 - 0.01) * cb.linspace01(10)


def labor_start(R):
    """The state the script carries from one solve into the next (and a state with no feasible
    choice keeps, :85), from a labour solve's result: v_old, v_new and the policies."""
    return dict(v_old=R["v_old"], v_new=R["v_new"],
                policies=(R["policy_k"], R["policy_l"], R["policy_c"], R["lin"]))


def labor_vfi_evaluator(cal, solve, simulate, start, T=10000):
    """Node evaluator for Aiyagari_Endogenous_Labor_VFI.m:166-245: the labour VFI from `start`
    (labor_start: the path-independent warm start) at the node's r and its own wage, MC supply on
    policy_k with the uniforms block of the node's depth, K_d.  Generic in the two callables (the
    GPU path or the C oracle): solve(start, r, w) -> dict(policy_k, iters);
    simulate(policy_k, z1, k1, uniforms) -> K_s.  The steps are vfi_evaluator's, with the
    labour script's state as the start."""
    return vfi_evaluator(cal, solve, simulate, start, T)


def hip_labor_vfi_evaluator(cal, L, start, T=10000, tol=1e-5, max_iter=1000, psi=1.0, eta=2.0):
    """The evaluator on this rank's GPU, one solve after another (host tier)."""
    from .sim import sim_capital
    from .vfi import labor_vfi_solve
    a, s, P = cal["a_grid"], cal["s"], cal["P"]

    def solve(st, r, w):
        return labor_vfi_solve(st["v_old"], a, s, P, L, r, w, cal["beta"], cal["sigma"], psi, eta,
                               tol, max_iter, v_new=st["v_new"], policies=st["policies"])

    def simulate(pk, z1, k1, u):
        return sim_capital(pk, a, P, z1, k1, u)
    return labor_vfi_evaluator(cal, solve, simulate, start, T)


def labor_ge_batch_call(r, start, cal, L, z1, k1, blocks, psi=1.0, eta=2.0, tol=1e-5,
                        max_iter=1000, n_devices=1):
    """aiy_labor_ge_batch (C ABI): K_s, K_d and iteration count at every rate in `r`, each from
    `start` (labor_start; v_new / policies None = zeros), with uniforms blocks[c] (T-1 draws) for
    candidate c; z1 1-based."""
    from ._capi import check, d, i64, ip, lib, ptr
    r, _, a, s, P, U, (Ks, Kd, it) = _batch_arrays(r, cal, blocks)
    n, N, Na, T = r.size, cal["N"], cal["Na"], U.shape[0] + 1
    f = lambda x: None if x is None else np.asfortranarray(x, dtype=np.float64)
    v, vn = f(start["v_old"]), f(start.get("v_new"))
    pol = start.get("policies") or (None, None, None, None)
    pk, pl, pc = f(pol[0]), f(pol[1]), f(pol[2])
    lin = None if pol[3] is None else np.asfortranarray(pol[3], dtype=np.int32)
    for x in (v, vn, pk, pl, pc, lin):
        if x is not None and x.shape != (N, Na):
            raise ValueError(f"start arrays must be (N, Na) = {(N, Na)}")
    L = np.ascontiguousarray(L, np.float64)
    check(lib().aiy_labor_ge_batch(ptr(r), i64(n), ptr(v), ptr(vn), ptr(pk), ptr(pl), ptr(pc),
                                   ptr(lin), ptr(a), ptr(s), ptr(P), ptr(L), i64(N), i64(Na),
                                   i64(L.size), d(cal["alpha"]), d(cal["delta"]), d(cal["beta"]),
                                   d(cal["sigma"]), d(psi), d(eta), d(cal["labor"]), d(tol),
                                   i64(max_iter), i64(z1), d(k1), i64(T), ptr(U), ip(n_devices),
                                   ptr(Ks), ptr(Kd), ptr(it)))
    return Ks, Kd, it


def hip_labor_batch_evaluator(cal, L, start, T=10000, tol=1e-5, max_iter=1000, n_devices=1,
                              psi=1.0, eta=2.0):
    """The node evaluator on the batched device path: all of a round's nodes of this rank in one
    aiy_labor_ge_batch call (one launch per sweep over all of them, one launch of the chains per
    GPU).  Same per-node arithmetic as hip_labor_vfi_evaluator, so the traces are identical."""
    z1, k1, blocks = _stream_start(cal, T)

    def many(nodes):
        Ks, Kd, it = labor_ge_batch_call([n.r for n in nodes], start, cal, L, z1, k1,
                                         [blocks[n.depth] for n in nodes], psi, eta, tol,
                                         max_iter, n_devices)
        return [(float(Ks[q]), float(Kd[q]), int(it[q])) for q in range(len(nodes))]
    return _with_many(many)


# tree levels per round on one GPU (measured: DESIGN.md §5, profiles/r10_labor_batch_ab.txt)
LABOR_LEVELS_ONE_GPU = 2


def aiyagari_labor_vfi_multisection(Na=400, levels=None, rank=0, world=1, allgather=None, r0=0.04,
                                    batched=True, T=10000, tol=1e-5, max_iter=1000, psi=1.0,
                                    eta=2.0):
    """The GE of Aiyagari_Endogenous_Labor_VFI.m with the candidate rates of the next `levels`
    bisection steps evaluated at once.  Every rank solves r0 from v = 0 (the script's first
    solve), then the rounds, every candidate warm from that solution (v_old, v_new and the
    policies: path independence, see the module docstring); batched=True runs a round's nodes of
    this rank in one aiy_labor_ge_batch call.  levels=None: LABOR_LEVELS_ONE_GPU on one rank,
    else auto_levels(world).  The script's chained warm start takes the same bracket decisions
    (tests/test_labor_batch_gpu.py)."""
    from . import calibration as cb
    from .vfi import labor_vfi_solve
    if levels is None:
        levels = LABOR_LEVELS_ONE_GPU if world == 1 else auto_levels(world)
    cal, L = labor_calibration(Na)
    R0 = labor_vfi_solve(np.zeros((cal["N"], Na)), cal["a_grid"], cal["s"], cal["P"], L, r0,
                         cb.wage(r0, cal["alpha"], cal["delta"]), cal["beta"], cal["sigma"], psi,
                         eta, tol, max_iter)
    start = labor_start(R0)
    if batched:
        ev = hip_labor_batch_evaluator(cal, L, start, T, tol, max_iter, 1, psi, eta)
    else:
        ev = hip_labor_vfi_evaluator(cal, L, start, T, tol, max_iter, psi, eta)
    tr = multisection(ev, -0.05, 1 / cal["beta"] - 1, levels=levels, rank=rank, world=world,
                      allgather=allgather if allgather else (torch_allgather if world > 1 else None))
    tr.iters = [int(R0["iters"])] + tr.iters
    return tr
