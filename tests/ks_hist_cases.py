"""Inputs shared by the histogram-simulation tests (tests/test_ks_hist_cpu.py, _gpu.py)."""
import numpy as np

PARAMS = np.array([0.99, 0.36, 0.025, 0.0001, 1000.0, 0.04, 0.10, 1 / (1 - 0.10), 0.0, 1.01, 0.99,
                   1.0, 0.0])


def grid7(n, lo=0.0001, hi=1000.0):
    x = (np.arange(n) / (n - 1.0)) ** 7 * (hi - lo) + lo
    x[0], x[-1] = lo, hi
    return x


def shock_paths(T, M, seed):
    zi = np.random.RandomState(seed).randint(0, 2, size=(T, M)).astype(np.int8)
    zi[0] = 0
    return zi


def start(x, M, K0s=(25.0, 40.0, 62.0)):
    """lam0 (M, 2, nx): 98 % of the mass at K0 (below, inside and above K_grid = [30, 50], cycling
    over the paths) by the lottery, 2 % spread over every node, split (0.96, 0.04)."""
    nx = x.size
    lam = np.zeros((M, 2, nx))
    for m in range(M):
        K0 = min(max(K0s[m % len(K0s)], x[0]), x[-1])
        j = int(np.clip(np.searchsorted(x, K0, side="right") - 1, 0, nx - 2))
        w = (K0 - x[j]) / (x[j + 1] - x[j])
        marg = np.full(nx, 0.02 / nx)
        marg[j] += 0.98 * (1 - w)
        marg[j + 1] += 0.98 * w
        lam[m, 0], lam[m, 1] = 0.96 * marg, 0.04 * marg
    return lam


def smooth_policy(kg, Kg):
    """Increasing in k in every column; the employed save more; kn leaves [x_0, x_end] at both
    ends (the unemployed columns are negative at k_min, the good employed one passes k_max)."""
    nk, nK = kg.size, Kg.size
    ko = np.zeros((nk, nK, 4))
    a = (0.3, -0.5, 0.1, -0.8)
    b = (1.06, 0.9, 0.93, 0.88)
    for s in range(4):
        ko[:, :, s] = a[s] + b[s] * kg[:, None] + 0.4 * np.sqrt(kg)[:, None] \
            + 0.05 * (Kg[None, :] - 40.0)
    return ko


def case(nx, nk, nK, T, M, seed=0):
    kg, Kg, x = grid7(nk), np.linspace(30.0, 50.0, nK), grid7(nx)
    return dict(k_opt=smooth_policy(kg, Kg), k_grid=kg, K_grid=Kg, x=x, params=PARAMS,
                zi=shock_paths(T, M, seed), lam0=start(x, M))


# one case per listed value of nx, nk, nK, T and M (every value appears at least once)
SHAPES = [(2, 2, 2, 2, 1), (3, 5, 4, 3, 3), (65, 100, 4, 60, 3), (150, 5, 2, 60, 1),
          (150, 100, 4, 3, 70), (65, 2, 2, 3, 70), (3, 100, 2, 2, 3), (2, 5, 4, 60, 1)]


def plateau_case(T=12, M=2, seed=3):
    """nx = 150, nk = 100: plateau policies, so that whole stretches of sources share one lottery
    key and the runs of dist_mass hold exactly 32, 33, 64, 65 and 130 sources (its chunk
    boundaries).  k_grid is a subset of x holding both end nodes of every plateau, so every
    source's kn is its plateau's value exactly."""
    nx, nk, nK = 150, 100, 4
    x, Kg = grid7(nx), np.linspace(30.0, 50.0, nK)
    groups = {0: [(0, 31), (32, 64), (65, 128), (129, 149)],    # 32, 33, 64, 21 sources
              1: [(0, 64), (65, 149)],                           # 65, 85
              2: [(0, 129), (130, 149)]}                         # 130, 20
    need = sorted({q for g in groups.values() for ab in g for q in ab})
    rest = [q for q in range(nx) if q not in need]
    pick = np.round(np.linspace(0, len(rest) - 1, nk - len(need))).astype(int)
    keep = sorted(need + [rest[q] for q in pick])
    assert len(keep) == nk
    kg = x[keep]
    ko = smooth_policy(kg, Kg)
    targets = (100, 108, 116, 124)   # plateau g sits mid-segment targets[g] of x: keys >= 2 apart
    for s, gs in groups.items():
        for g, (a, b) in enumerate(gs):
            sel = (kg >= x[a]) & (kg <= x[b])
            v = 0.5 * (x[targets[g]] + x[targets[g] + 1])
            ko[sel, :, s] = v + 0.02 * (Kg[None, :] - 40.0)
    return dict(k_opt=ko, k_grid=kg, K_grid=Kg, x=x, params=PARAMS, zi=shock_paths(T, M, seed),
                lam0=start(x, M))


def run_lengths(c, K, z):
    """The run lengths je - jb of every destination at period policy (K, z)."""
    from oracle import np_oracle as no
    from tests import ks_hist_ref as ref
    x, kg = c["x"], c["k_grid"]
    ik = no._bilin_seg(kg, x)
    tk = (x - kg[ik]) / (kg[ik + 1] - kg[ik])
    key, _ = ref.keys_weights(c["k_opt"], kg, c["K_grid"], x, ik, tk, K, z)
    out = set()
    for e in (0, 1):
        off = np.searchsorted(key[e], np.arange(x.size + 1), side="left")
        for k in range(x.size):
            out.add(int(off[k + 1] - (off[k - 1] if k else off[k])))
    return out


def slow_case(T=40, M=2, seed=5):
    """nx = 65, nk = 100: column (K_grid[3], good employed) of k_opt decreases over a stretch of
    k.  Periods in the good state whose K_t lies in K_grid's last segment (or above it) read that
    column and have non-monotone keys; the bad state's never do."""
    c = case(65, 100, 4, T, M, seed)
    kg = c["k_grid"]
    ko = c["k_opt"]
    sel = (kg > 20.0) & (kg < 200.0)
    ko[sel, 3, 0] = ko[sel, 3, 0][::-1]
    return c
