"""Deterministic adversarial cases for the Krusell-Smith shock panel (F3) and the agent-panel
capital simulation (F2), csrc/ks_panel_kernels.hip, shared by the CPU census
(tests/test_ks_panel_cases_cpu.py) and the GPU parity tests
(tests/test_ks_panel_adversarial_gpu.py).  A plain module: every builder is a pure function of
its arguments (seeded RandomState), so both sides see the same bytes; the builders and the
oracle results are cached and must not be written to.

A panel case is a dict(name, k_grid, K_grid, k_opt [k, K, s], zi (T,) int8, e (T, pop) int8
in {0 employed, 1 unemployed}, k0 (pop,)).  A shock case is a dict(name, p, params, T, pop, U).
"""
from __future__ import annotations

import functools

import numpy as np

from oracle import np_oracle as no
from tests.ks_hist_cases import PARAMS

K_MIN, K_MAX = 1e-4, 1000.0
LDS_GRID = 8192        # kPanelLdsGrid: nk + nK up to this is staged in LDS
ONE_PER_THREAD = 256   # both grids at most this long: one value per thread

# (nk, nK): floor and boundaries of the one-value-per-thread path, nk + nK = 8192 by two splits
# and 8193 by two splits, and a grid well past the LDS
PANEL_SHAPES = ((2, 2), (3, 2), (5, 4), (100, 4), (256, 256), (257, 4), (100, 257),
                (8189, 3), (8190, 2), (8190, 3), (8191, 2), (20000, 5))
PANEL_T, PANEL_POP = 12, 600
STARTS = (22.0, 40.0, 70.0)
# share of a start above k_max: each such agent adds about 1050 / pop to the mean, so the share
# grows with the mean the start aims at (6 + 15 + 30 agents of 600)
ABOVE = {22.0: 0.01, 40.0: 0.025, 70.0: 0.05}
HOST_SHAPES = ((2, 2), (100, 4), (257, 4), (8190, 2), (8190, 3))
NODE_SHAPES = ((100, 4), (257, 4), (8191, 2))
NODE_D = (1, -1, 2, -3)
NODE_KINDS = ("shift", "scatter")

# populations of the reduction cases and the G they give (256 lanes per block, 1,024 blocks at
# most): no fold, shuffles only, one register stage ... all four, then several agents per lane
REDUCTION_POPS = (1, 256, 257, 513, 16384, 16385, 32769, 131073, 261633, 262144, 262145,
                  2 * 262144 + 1)
REDUCTION_G = (1, 1, 2, 3, 64, 65, 129, 513, 1023, 1024, 1024, 1024)

# (T, pop): every T of {1, 2, 32, 33, 34, 64, 65, 66, 129, 130} (the 32-step unroll of the
# idiosyncratic chains and the 64-step rounds of the aggregate chain, one short, exact, one
# over) and every pop of {1, 255, 256, 257}
SHOCK_SHAPES = ((1, 1), (1, 257), (2, 255), (2, 1), (32, 256), (33, 1), (33, 257), (34, 255),
                (64, 256), (65, 257), (65, 1), (66, 255), (129, 256), (130, 257))
UG_UB = ((0.04, 0.10), (0.2, 0.35), (0.5, 0.6))
STREAMS = ("matlab", "adversarial")


def staging_path(nk, nK):
    """Which grid staging of ks_panel_step_kernel a shape takes."""
    if nk + nK > LDS_GRID:
        return "global"
    return "one" if nk <= ONE_PER_THREAD and nK <= ONE_PER_THREAD else "looped"


def grid_p(n, p=None):
    """linspace(0, 1, n)^p * (k_max - k_min) + k_min with exact end points; p = 7 (the script's
    spacing) up to 1,000 nodes and 2 above (x^7 repeats k_min from about 2,043 nodes on)."""
    if p is None:
        p = 7 if n <= 1000 else 2
    x = (np.arange(n) / (n - 1.0)) ** p * (K_MAX - K_MIN) + K_MIN
    x[0], x[-1] = K_MIN, K_MAX
    assert np.all(np.diff(x) > 0)
    return x


def K_grid(nK):
    return np.linspace(30.0, 50.0, nK)


def two_sided_policy(kg, Kg):
    """Increasing in k; the unemployed columns are negative near k_min and the good-employed
    one passes k_max; the slope in k is about 1 at the bottom, so that linear extrapolation
    below the grid stays bounded."""
    a = (0.3, -1.5, 0.1, -2.0)
    b = (1.06, 0.9, 0.93, 0.88)
    ko = np.zeros((kg.size, Kg.size, 4))
    for s in range(4):
        ko[:, :, s] = a[s] + b[s] * kg[:, None] + 0.1 * np.sqrt(kg + 1.0)[:, None] \
            + 0.05 * (Kg[None, :] - 40.0)
    return ko


def node_policy(kg, nK):
    """k_opt[i, :, s] = k_grid[clip(i + d_s)]: an agent on a node moves to a node."""
    nk = kg.size
    ko = np.zeros((nk, nK, 4))
    for s, d in enumerate(NODE_D):
        ko[:, :, s] = kg[np.clip(np.arange(nk) + d, 0, nk - 1)][:, None]
    return ko


def scatter_policy(kg, nK, seed):
    """k_opt[i, :, s] = k_grid[m_s(i)] with random maps m_s (the last two nodes share a target, so
    that tk = 1 at the top is exact too).  Neighbouring values differ by orders of magnitude:
    f(j-1) + 1 * (f(j) - f(j-1)) is then not f(j) bit for bit, so a search that takes a node
    for the end of the segment below it leaves the grid."""
    nk = kg.size
    rs = np.random.RandomState(seed)
    ko = np.zeros((nk, nK, 4))
    for s in range(4):
        m = rs.randint(0, nk, nk)
        m[0], m[-1], m[-2] = nk - 1, 0, 0    # the end nodes send their agents to each other
        ko[:, :, s] = kg[m][:, None]
    return ko


def direct_shocks(T, pop, seed):
    """zi[0] = 0, then fair coin flips; about 30 % unemployed: all four states populated."""
    rs = np.random.RandomState(seed)
    zi = rs.randint(0, 2, size=T).astype(np.int8)
    zi[0] = 0
    e = (rs.random_sample((T, pop)) < 0.3).astype(np.int8)
    return zi, e


def start_population(kg, pop, K0, seed):
    """A lognormal bulk scaled so that the mean is about K0, 5 % below k_min (down to -5),
    ABOVE[K0] above k_max (up to 1100), 10 % in (0, 3), 5 % on randomly chosen nodes up to 150,
    agent 0 on k_grid[0] and the last agent on k_grid[-1]."""
    rs = np.random.RandomState(seed)
    n_below, n_above = int(0.05 * pop), int(round(ABOVE[K0] * pop))
    n_low, n_node = int(0.10 * pop), int(0.05 * pop)
    n_bulk = pop - 2 - n_below - n_above - n_low - n_node
    below = rs.uniform(-5.0, K_MIN, n_below)
    above = rs.uniform(K_MAX + 0.5, 1100.0, n_above)
    low = rs.uniform(0.0, 3.0, n_low)
    small = np.flatnonzero(kg <= 150.0)
    nodes = kg[small[rs.randint(0, small.size, n_node)]]
    bulk = np.exp(0.5 * rs.standard_normal(n_bulk))
    rest = below.sum() + above.sum() + low.sum() + nodes.sum() + kg[0] + kg[-1]
    scale = (K0 * pop - rest) / bulk.sum()
    assert scale > 1.0, (K0, scale)
    k0 = np.concatenate([below, above, low, nodes, scale * bulk])
    rs.shuffle(k0)
    return np.concatenate([[kg[0]], k0, [kg[-1]]])


def _case(key, kg, Kg, ko, zi, e, k0):
    return dict(name="-".join(str(q) for q in key), key=key, k_grid=kg, K_grid=Kg, k_opt=ko,
                zi=zi, e=e, k0=k0)


@functools.lru_cache(maxsize=None)
def panel_case(nk, nK, K0, T=PANEL_T, pop=PANEL_POP):
    kg, Kg = grid_p(nk), K_grid(nK)
    seed = 1000 * nk + 10 * nK + int(K0)
    zi, e = direct_shocks(T, pop, seed)
    return _case(("panel", nk, nK, K0, T, pop), kg, Kg, two_sided_policy(kg, Kg), zi, e,
                 start_population(kg, pop, K0, seed + 1))


@functools.lru_cache(maxsize=None)
def node_case(nk, nK, kind="shift", T=PANEL_T, pop=PANEL_POP):
    """Every agent on a node in every period: every search is a tie, tk is 0 (1 at the top).
    kind "shift": node_policy, "scatter": scatter_policy."""
    kg, Kg = grid_p(nk), K_grid(nK)
    rs = np.random.RandomState(7 * nk + nK)
    zi, e = direct_shocks(T, pop, 7 * nk + nK + 1)
    k0 = kg[rs.randint(0, nk, pop)]
    k0[0], k0[-1] = kg[0], kg[-1]
    ko = node_policy(kg, nK) if kind == "shift" else scatter_policy(kg, nK, 7 * nk + nK + 2)
    return _case(("node", nk, nK, kind), kg, Kg, ko, zi, e, k0)


@functools.lru_cache(maxsize=None)
def node_K_case(j, nk=100, nK=5, T=6, pop=PANEL_POP):
    """Every agent starts at K_grid[j] (30, 35, ..., 50: the blocked sum of 600 equal integers is
    exact), so K_ts[0] is that node: j = nK - 1 is the upper clamp with tK = 1, an interior j
    the tie of the K search."""
    kg, Kg = grid_p(nk), K_grid(nK)
    zi, e = direct_shocks(T, pop, 50 + j)
    return _case(("node_K", j), kg, Kg, two_sided_policy(kg, Kg), zi, e, np.full(pop, Kg[j]))


@functools.lru_cache(maxsize=None)
def nonfinite_case(T):
    """One k_opt entry NaN and one +inf, in cells of the first period's K segment that only
    the agents of two k segments read at t = 0 (device tier only: the host tier's population
    check would refuse the second call, not this one)."""
    c = dict(panel_case(100, 4, 40.0))
    ko = c["k_opt"].copy()
    kg, Kg, k0 = c["k_grid"], c["K_grid"], c["k0"]
    iK = int(no._bilin_seg(Kg, np.array([no.ks_mean_blocked(k0, no.ks_panel_blocks(k0.size))]))[0])
    ik = no._bilin_seg(kg, k0)
    a, b = 5, 17
    assert abs(int(ik[a]) - int(ik[b])) > 1
    ko[ik[a] + 1, iK, 2 * int(c["zi"][0]) + int(c["e"][0, a])] = np.nan
    ko[ik[b], iK + 1, 2 * int(c["zi"][0]) + int(c["e"][0, b])] = np.inf
    c.update(name=f"nonfinite-{T}", key=("nonfinite", T), k_opt=ko, zi=c["zi"][:T], e=c["e"][:T])
    return c


@functools.lru_cache(maxsize=None)
def reduction_case(pop, seed=0):
    kg, Kg = grid_p(100), K_grid(4)
    zi, e = direct_shocks(3, pop, pop % 100003 + seed)
    k0 = np.random.RandomState(pop % 100003 + seed + 1).uniform(0.0, 200.0, pop)
    return _case(("reduction", pop, seed), kg, Kg, two_sided_policy(kg, Kg), zi, e, k0)


def two_sided_cases():
    return [panel_case(nk, nK, K0) for nk, nK in PANEL_SHAPES for K0 in STARTS]


def special_cases():
    return [node_case(nk, nK, kind) for nk, nK in NODE_SHAPES for kind in NODE_KINDS] \
        + [node_K_case(4), node_K_case(2)]


def finite_panel_cases():
    return two_sided_cases() + special_cases()


@functools.lru_cache(maxsize=None)
def _oracle(kind, *key):
    c = {"panel": panel_case, "node": node_case, "node_K": node_K_case,
         "nonfinite": nonfinite_case, "reduction": reduction_case}[kind](*key)
    with np.errstate(all="ignore"):   # the non-finite case
        return no.ks_panel_simulate(c["k_grid"], c["K_grid"], c["k_opt"], c["zi"], c["e"],
                                    c["k0"])


def oracle(c):
    """(K_ts, k_final) of np_oracle.ks_panel_simulate for a case of this module, computed once."""
    return _oracle(*c["key"])


def trace(c):
    """k of every period in which it is searched (T - 1, pop) and K_ts, by one-period runs of the
    oracle (each restarts from the last one's population, so the operations are the same)."""
    T = c["zi"].size
    k = c["k0"]
    ks, Ks = [], []
    for t in range(T - 1):
        ks.append(k)
        K2, k = no.ks_panel_simulate(c["k_grid"], c["K_grid"], c["k_opt"], c["zi"][t:t + 2],
                                     c["e"][t:t + 2], k)
        Ks.append(K2[0])
    Ks.append(K2[1])
    return np.array(ks), np.array(Ks)


# ------------------------------------------------------------------ shock cases


def shock_params(ug, ub):
    """(np_oracle parameter dict, the 13 doubles of the C ABI) for one (ug, ub)."""
    p = dict(no.ks_setup()[0], ug=ug, ub=ub)
    prm = PARAMS.copy()
    prm[5], prm[6] = ug, ub
    return p, prm


def thresholds(p):
    """The eleven numbers a draw is compared with: pgg, pbb, ug and thr[cur_z, prev_z, prev_e]."""
    pr = no.ks_eps_probs(p)
    th = np.concatenate([[pr["pgg"], pr["pbb"], p["ug"]], pr["thr"].ravel()])
    assert np.all((th > 0) & (th < 1))
    return th


def adversarial_stream(p, n, seed):
    """MATLAB's stream with half of the draws replaced: a quarter of all draws is a threshold
    itself, an eighth each its neighbour up and down, and an eighth is 0 or the largest
    double below 1 (rand's range end)."""
    rs = np.random.RandomState(seed)
    U = no.matlab_rand_stream(n).copy()
    th = thresholds(p)
    kind = rs.randint(0, 8, n)
    pick = th[rs.randint(0, th.size, n)]
    U = np.where(kind < 2, pick, U)
    U = np.where(kind == 2, np.nextafter(pick, 1.0), U)
    U = np.where(kind == 3, np.nextafter(pick, 0.0), U)
    U = np.where(kind == 4, np.where(rs.randint(0, 2, n) == 0, 0.0, 1.0 - 2.0 ** -53), U)
    return U


@functools.lru_cache(maxsize=None)
def shock_case(T, pop, ug, ub, stream):
    p, prm = shock_params(ug, ub)
    n = no.ks_shock_draws(T, pop)
    if stream == "matlab":
        U = no.matlab_rand_stream(n)
    else:
        U = adversarial_stream(p, n, 31 * T + pop)
    key = (T, pop, ug, ub, stream)
    return dict(name="-".join(str(q) for q in key), key=key, p=p, params=prm, T=T, pop=pop, U=U)


def shock_cases(shapes=SHOCK_SHAPES):
    return [shock_case(T, pop, ug, ub, s) for T, pop in shapes for ug, ub in UG_UB
            for s in STREAMS]


@functools.lru_cache(maxsize=None)
def _shock_oracle(T, pop, ug, ub, stream):
    c = shock_case(T, pop, ug, ub, stream)
    return no.ks_shocks(c["p"], T, pop, c["U"])


def shock_oracle(c):
    return _shock_oracle(*c["key"])


def shock_hits(c):
    """(comparisons, hits (11,)): how many draws are compared, and how many of them equal the
    threshold they are compared with, by threshold (the order of `thresholds`)."""
    T, pop, U, p = c["T"], c["pop"], c["U"], c["p"]
    zi, e = shock_oracle(c)
    th = thresholds(p)
    hits = np.zeros(11, np.int64)
    for t in range(1, T):
        j = 0 if zi[t - 1] == 0 else 1
        hits[j] += U[t - 1] == th[j]
    hits[2] += np.sum(U[T - 1:T - 1 + pop] == th[2])
    pos = T - 1 + pop
    for t in range(1, T):
        j = 3 + (int(zi[t]) * 2 + int(zi[t - 1])) * 2 + e[t - 1].astype(np.int64)
        np.add.at(hits, j[U[pos:pos + pop] == th[j]], 1)
        pos += pop
    return U.size, hits
