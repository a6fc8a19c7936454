"""Adversarial inputs of the histogram simulation (csrc/ks_hist_kernels.hip) and an independent
reference of it, shared by tests/test_ks_hist_adv_cases_cpu.py (the census) and
tests/test_ks_hist_adversarial_gpu.py (the parity tests).

The GPU is compared bit for bit with tests/ks_hist_ref.py, which restates the kernel's own
operation order.  `independent` below states Young's recursion without any order: long double,
scattered lottery halves, a plain sum for K_t.  It shares the probability table with the
restatement and nothing else, so a mistake the kernel and its restatement have in common (the
lottery's side, a transposed employment probability) shows against it.

Every case is a dict like ks_hist_cases.case's plus `name` and `group`; T is 6 to 12 unless the
case is about T."""
import functools

import numpy as np

from tests import ks_hist_cases as base
from tests import ks_hist_ref as ref

LD = np.longdouble
PARAMS = base.PARAMS

# Restatement (fp64, the kernel's order) against `independent` (long double, no order) over
# all_cases(): the largest relative difference in K_ts and the largest absolute difference in λ.
# Measured 2026-10-20 on x86-64 (80-bit long double); the differences are sized by summation
# order.  Both the restatement and the GPU are held to 8 x these (TOL_*), the margin covering
# platforms whose long double is narrower; the bound may not pass 1e-11, the figure
# test_ks_hist_cpu.py grants the dense formulation — a case that needs more is ill-conditioned
# and must change.
MEASURED_MAX_REL_K = 1.11e-14     # shock-T1100
MEASURED_MAX_ABS_LAM = 1.05e-13   # lam-tiny (a start whose total is 2.25)
TOL_REL_K = 8 * MEASURED_MAX_REL_K
TOL_ABS_LAM = 8 * MEASURED_MAX_ABS_LAM
TOL_CEILING = 1e-11


# ------------------------------------------------------------------ the fit rule (ks_hist.hpp)

MAX_LDS = 160 * 1024
FOLD = 256


def lds_bytes(nx, nk, nK, kopt):
    nd = 8 * nx + nK + 8 + (4 * nK * nk if kopt else 0)
    ni = (5 * nx + 4 + 1) & ~1
    return 8 * nd + 4 * ni


def fits(nx, nk, nK):
    return (2 <= nx <= 1 << 20 and 2 <= nk <= 1 << 24 and 2 <= nK <= 1 << 24
            and lds_bytes(nx, nk, nK, False) <= MAX_LDS)


def kopt_in_lds(nx, nk, nK):
    return nk * nK <= 1 << 16 and lds_bytes(nx, nk, nK, True) <= MAX_LDS


def shape(c):
    return c["x"].size, c["k_grid"].size, c["K_grid"].size


def instantiation(c):
    """The kernel instantiation launch_ks_hist chooses and its dynamic LDS in bytes."""
    nx, nk, nK = shape(c)
    staged = kopt_in_lds(nx, nk, nK)
    return ("<true>" if staged else "<false>"), lds_bytes(nx, nk, nK, staged)


def largest_staged_nk(nx, nK):
    nk = 2
    while kopt_in_lds(nx, nk + 1, nK):
        nk += 1
    return nk


# ------------------------------------------------------------------ the independent reference


def _seg(g, q):
    return np.clip(np.searchsorted(g, q, "right") - 1, 0, g.size - 2)


def independent_path(k_opt, k_grid, K_grid, x, params, zi, lam0):
    """Young's recursion for one shock path in long double: K_t = Σ λ x; every source (e, j)
    moves to kn = k_opt(x_j, K_t; z_t, e) (bilinear, clamped to x's range) and its mass is split
    between the two nodes that bracket kn, in proportion to the distances, and between the two
    employment states of t + 1 by P(e' | e; z_t, z_{t+1})."""
    thr = ref.thr_table(params).astype(LD)
    kg, Kg, xs, ko = (np.asarray(a, LD) for a in (k_grid, K_grid, x, k_opt))
    ik = _seg(kg, xs)
    tk = (xs - kg[ik]) / (kg[ik + 1] - kg[ik])
    lam = np.array(lam0, LD)
    T = len(zi)
    K_ts = np.zeros(T, LD)
    for t in range(T - 1):
        z, zn = int(zi[t]), int(zi[t + 1])
        K = (lam * xs).sum()
        K_ts[t] = K
        iK = int(_seg(Kg, np.array([K], LD))[0])
        tK = (K - Kg[iK]) / (Kg[iK + 1] - Kg[iK])
        new = np.zeros_like(lam)
        for e in (0, 1):
            f = ko[:, :, 2 * z + e]
            kn = ((1 - tk) * (1 - tK) * f[ik, iK] + tk * (1 - tK) * f[ik + 1, iK]
                  + (1 - tk) * tK * f[ik, iK + 1] + tk * tK * f[ik + 1, iK + 1])
            kn = np.clip(kn, xs[0], xs[-1])
            key = _seg(xs, kn)
            w = (kn - xs[key]) / (xs[key + 1] - xs[key])
            employed = thr[zn, z, e]
            for en, p in ((0, employed), (1, 1 - employed)):
                np.add.at(new[en], key, p * lam[e] * (1 - w))
                np.add.at(new[en], key + 1, p * lam[e] * w)
        lam = new
    K_ts[T - 1] = (lam * xs).sum()
    return K_ts, lam


def independent_of(c):
    """(K_ts (T, M), lam (M, 2, nx)) in long double."""
    zi = c["zi"]
    T, M = zi.shape
    nx = c["x"].size
    lam0 = np.broadcast_to(c["lam0"], (M, 2, nx))
    K_ts = np.zeros((T, M), LD)
    lam = np.zeros((M, 2, nx), LD)
    for m in range(M):
        K_ts[:, m], lam[m] = independent_path(c["k_opt"], c["k_grid"], c["K_grid"], c["x"],
                                              c["params"], zi[:, m], lam0[m])
    return K_ts, lam


def restatement_of(c):
    return ref.simulate(c["k_opt"], c["k_grid"], c["K_grid"], c["x"], c["params"], c["zi"],
                        c["lam0"])


def differences(got, want):
    """(max relative difference in K_ts, max absolute difference in λ) of (K_ts, lam, ...)
    against the independent reference's (K_ts, lam)."""
    dK = np.abs(np.asarray(got[0], LD) / want[0] - 1).max()
    dl = np.abs(np.asarray(got[1], LD) - want[1]).max()
    return float(dK), float(dl)


# ------------------------------------------------------------------ building blocks


def grid_p(n, p, lo=0.0001, hi=1000.0):
    """ks_hist_cases.grid7 with the power p (x^7 repeats k_min from a few thousand nodes on)."""
    x = (np.arange(n) / (n - 1.0)) ** p * (hi - lo) + lo
    x[0], x[-1] = lo, hi
    assert np.all(np.diff(x) > 0)
    return x


def random_start(nx, M, seed, split=(0.9, 0.1)):
    """lam0 (M, 2, nx): a different positive weight on every node, every path its own, Σ = 1."""
    r = np.random.RandomState(seed).rand(M, nx) + 0.05
    r /= r.sum(1, keepdims=True)
    return np.stack([split[0] * r, split[1] * r], 1)


def patterns(T, *kinds):
    """Shock paths (T, len(kinds)): "01" 0101..., "0011", "0" all good, "1" all bad, "10"."""
    cols = []
    for kind in kinds:
        cols.append([int(kind[t % len(kind)]) for t in range(T)])
    return np.array(cols, np.int8).T.copy()


def _case(name, group, c, **extra):
    d = dict(c, name=name, group=group)
    d.update(extra)
    return d


def smooth_case(name, group, nx, nk, nK, T, M, seed, k_power=7):
    kg, Kg, x = grid_p(nk, k_power), np.linspace(30.0, 50.0, nK), base.grid7(nx)
    assert np.all(np.diff(x) > 0)
    return _case(name, group, dict(k_opt=base.smooth_policy(kg, Kg), k_grid=kg, K_grid=Kg, x=x,
                                   params=PARAMS, zi=base.shock_paths(T, M, seed),
                                   lam0=base.start(x, M)))


def direct_case(name, group, x, keys, ws, zi, lam0, nK=2):
    """k_grid = x and k_opt constant in K: source j of state s lands at
    x[keys[s, j]] + ws[s, j]·(x[keys[s, j] + 1] − x[keys[s, j]]) — on the node itself for a
    weight of exactly 0 or 1.  keys, ws: (4, nx)."""
    keys = np.asarray(keys, np.int64)
    ws = np.asarray(ws, np.float64)
    lo, hi = x[keys], x[keys + 1]
    kn = np.where(ws == 0, lo, np.where(ws == 1, hi, lo + ws * (hi - lo)))
    ko = np.repeat(kn.T[:, None, :], nK, 1)
    return _case(name, group, dict(k_opt=ko, k_grid=x.copy(), K_grid=np.linspace(30.0, 50.0, nK),
                                   x=x, params=PARAMS, zi=zi, lam0=lam0), keys=keys, ws=ws)


# The direct-key cases take x^2 spacing: x^7 has segments of 1e-12 beside x[0] = 1e-4, where one
# rounding of kn moves the lottery weight by 1e-9 and the comparison with the independent
# reference would be ill-conditioned.
DIRECT_POWER = 2


def base_keys(nx):
    """Monotone keys (4, nx) from 3 upwards, a slope per state, and weights in [0.25, 0.75]."""
    j = np.arange(nx)
    keys = np.stack([np.minimum(3 + (j * (7 + s)) // 10, nx - 2) for s in range(4)])
    ws = np.stack([0.25 + 0.5 * np.mod(0.37 * j + 0.11 * s, 1.0) for s in range(4)])
    return keys, ws


# ------------------------------------------------------------------ the groups

SWEEP_NX = (127, 128, 129, 160, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 1900)


def sweep_cases():
    """The thread-to-element walk: 2·nx at, just under and just past the block sizes 256 ... 1024,
    the first strided walk (nx = 513), de == 0 (nx > 1024), and the moment's dj = 1, 0, 256."""
    return [smooth_case(f"sweep-{nx}", "sweep", nx, 100, 4, 8, 2, seed=nx) for nx in SWEEP_NX]


def lds_cases():
    """k_opt staged in LDS up to the last nk that fits, read through L2 from the next one on,
    past nk·nK = 2^16, and at the largest state (more than 64 KiB of dynamic LDS unstaged)."""
    top = largest_staged_nk(65, 4)
    return [smooth_case(f"lds-nk{top}", "lds", 65, top, 4, 8, 2, seed=1),
            smooth_case(f"lds-nk{top + 1}", "lds", 65, top + 1, 4, 8, 2, seed=2),
            smooth_case("lds-nk16400", "lds", 65, 16400, 4, 8, 2, seed=3, k_power=3),
            smooth_case("lds-nx1900", "lds", 1900, 100, 4, 6, 2, seed=4)]


ROW_KINDS = ("low", "high", "mixed", "segment")


def row_case(nx, kind):
    """One run of the whole row: the policy below x[0] everywhere (key 0, w = 0), above x[-1]
    everywhere (key nx−2, w = 1), the employed high and the unemployed low, or everywhere inside
    one interior segment with a weight of its own per source."""
    c = smooth_case(f"row-{kind}-{nx}", "rows", nx, 100, 4, 6, 2, seed=nx + len(kind))
    ko, x = c["k_opt"], c["x"]
    if kind == "low":
        ko[:] = -5.0
    elif kind == "high":
        ko[:] = 2000.0
    elif kind == "mixed":
        ko[:, :, (0, 2)] = 2000.0
        ko[:, :, (1, 3)] = -5.0
    else:
        mid = nx // 2
        frac = 0.1 + 0.8 * np.arange(100)[:, None, None] / 99.0 * np.array([1.0, 0.9, 0.8, 0.7])
        ko[:] = x[mid] + frac * (x[mid + 1] - x[mid])
    c["lam0"] = random_start(nx, 2, seed=nx)
    return c


def row_cases():
    return [row_case(nx, kind) for nx in (1000, 1900) for kind in ROW_KINDS]


VOTE_NX = (64, 129, 600, 1100)
VOTE_KINDS = ("last1", "first0", "both", "long")
VOTE_T = 9


def vote_case(nx, kind, inverted=True):
    """Direct keys with the inversions in the good states (s = 0, 1) only: a period is slow
    exactly when z_t = 0.  last1: key(1, nx−1) < key(1, nx−2) and nothing else; first0:
    key(0, 0) > key(0, 1) and nothing else; both: the two together; long: all four states send
    a stretch of sources (100, or nx − 20 where that is less) to one key, and row 0 has one
    inversion after it.  inverted=False leaves the inversion(s) out."""
    keys, ws = base_keys(nx)
    if kind == "long":
        a, n = 10, min(100, nx - 20)
        keys[:, a:a + n] = keys[:, a:a + 1]
    if inverted:
        if kind in ("last1", "both"):
            keys[1, nx - 1] = keys[1, nx - 2] - 1
        if kind in ("first0", "both"):
            keys[0, 0] = keys[0, 1] + 1
        if kind == "long":
            q = nx - 8
            keys[0, q] = keys[0, q + 1] + 1
    zi = patterns(VOTE_T, "01", "0011", "0")
    return direct_case(f"vote-{kind}-{nx}", "vote", grid_p(nx, DIRECT_POWER), keys, ws, zi,
                       random_start(nx, 3, seed=nx), nK=2)


def vote_cases():
    return [vote_case(nx, kind) for nx in VOTE_NX for kind in VOTE_KINDS]


def expected_slow(c):
    """Per path: the number of good periods among the T − 1 that push mass."""
    return (c["zi"][:-1] == 0).sum(0)


TIE_NX = 129
NODE_K = 32.0


def node_K_case(name, K_grid):
    """All mass on the node x[39] = 32.0 (0.75 employed, 0.25 unemployed): K_0 is 32.0 exactly,
    a node of K_grid."""
    c = smooth_case(name, "tie", 65, 100, 4, 8, 2, seed=9)
    c["x"][39] = NODE_K
    assert np.all(np.diff(c["x"]) > 0)
    c["K_grid"] = np.asarray(K_grid, np.float64)
    c["k_opt"] = base.smooth_policy(c["k_grid"], c["K_grid"])
    lam = np.zeros((2, 65))
    lam[:, 39] = 0.75, 0.25
    c["lam0"] = np.stack([lam, lam])
    return c


def tie_cases():
    nx = TIE_NX
    x = grid_p(nx, DIRECT_POWER)
    keys, ws = base_keys(nx)
    zi = base.shock_paths(8, 2, seed=6)
    zi[0, 1] = 1
    lam0 = random_start(nx, 2, seed=8)
    out = [direct_case("tie-w0", "tie", x, keys, np.zeros_like(ws), zi, lam0)]
    # the identity: every source stays on its node
    ident = np.repeat(np.repeat(x[:, None, None], 2, 1), 4, 2)
    out.append(_case("tie-identity", "tie",
                     dict(k_opt=ident, k_grid=x.copy(), K_grid=np.linspace(30.0, 50.0, 2), x=x,
                          params=PARAMS, zi=patterns(10, "0110", "1"),
                          lam0=random_start(nx, 2, seed=8, split=(0.7, 0.3)))))
    # sources 40 ... 79 land on x[-1] itself (key nx−2, w = 1), the ones after them inside the
    # last segment: without the clamp of the key the row is no longer monotone
    kt, wt = keys.copy(), ws.copy()
    kt[:, 40:] = nx - 2
    wt[:, 40:80] = 1.0
    out.append(direct_case("tie-top", "tie", x, kt, wt, zi, lam0))
    # sources 10 ... 49 land on one node (w = 0) and the 50 after them in the segment above it:
    # the node's sources head the run of the destination above with 40 terms of λ·0, which place
    # the chunk boundaries among the 50 that follow (a search with < would move them a run down)
    # Every other source stays in its own segment, so the mass does not contract onto a few
    # nodes, where the last bit that tells the two apart would be rounded away within T periods.
    kr, wr = np.tile(np.minimum(np.arange(nx), nx - 2), (4, 1)), ws.copy()
    kr[:, 10:50] = 30 + np.arange(4)[:, None]
    kr[:, 50:100] = 31 + np.arange(4)[:, None]
    wr[:, 10:50] = 0.0
    out.append(direct_case("tie-node-run", "tie", x, kr, wr, patterns(6, "10", "01"), lam0))
    out.append(node_K_case("tie-K-interior", (30.0, NODE_K, 40.0, 50.0)))
    out.append(node_K_case("tie-K-last", (20.0, 25.0, 30.0, NODE_K)))
    return out


def shock_cases():
    starts = smooth_case("shock-starts", "shock", 65, 100, 4, 10, 4, seed=12)
    zi = starts["zi"]
    zi[0, 0] = 1                                   # a random path that starts bad
    zi[:, 1:] = patterns(10, "1", "0", "10")       # all bad, all good, alternating from bad
    many = smooth_case("shock-many", "shock", 10, 5, 4, 4, 300, seed=13)
    many["zi"] = np.random.RandomState(14).randint(0, 2, size=(4, 300)).astype(np.int8)
    # a start of its own per path, from nearly all mass at the low nodes (K_0 below K_grid) to
    # even weights (K_0 above it)
    decay = np.exp(-np.linspace(0.0, 3.0, 300)[:, None, None] * np.arange(10))
    r = np.random.RandomState(15).rand(300, 2, 10) * decay
    many["lam0"] = r / r.sum((1, 2), keepdims=True)
    long = smooth_case("shock-T1100", "shock", 65, 100, 4, 1100, 1, seed=16)
    return [starts, many, long]


def lam_cases():
    out = []
    for kind in ("zeros", "tiny", "unnormalised"):
        c = smooth_case(f"lam-{kind}", "lam", 150, 100, 4, 8, 2, seed=17)
        lam = random_start(150, 2, seed=18)
        if kind == "zeros":                        # exact zeros over whole stretches
            lam[:, :, :50] = 0.0
            lam[:, :, 100:] = 0.0
            lam[1, 1, :] = 0.0
        elif kind == "tiny":                       # 1e-300 beside entries of order 1
            lam[:] = 1e-300
            lam[:, 0, 70::7] = 0.125
            lam[:, 1, 71::7] = 0.0625
        else:
            lam *= 3.7
        c["lam0"] = lam
        out.append(c)
    return out


@functools.lru_cache(maxsize=None)
def all_cases():
    cs = (sweep_cases() + lds_cases() + row_cases() + vote_cases() + tie_cases() + shock_cases()
          + lam_cases())
    names = [c["name"] for c in cs]
    assert len(set(names)) == len(names)
    for c in cs:
        for a in c.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)      # shared by every test: left unchanged
    return tuple(cs)


def names(*groups):
    return [c["name"] for c in all_cases() if not groups or c["group"] in groups]


def get(name):
    return next(c for c in all_cases() if c["name"] == name)


@functools.lru_cache(maxsize=None)
def restatement(name):
    """ks_hist_ref.simulate of the case, computed once."""
    out = restatement_of(get(name))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def independent(name):
    out = independent_of(get(name))
    for a in out:
        a.setflags(write=False)
    return out


def keys_weights_at(c, K, z):
    """The restatement's (key, w) (2, nx) of period policy (K, z)."""
    from oracle import np_oracle as no
    x, kg = c["x"], c["k_grid"]
    ik = no._bilin_seg(kg, x)
    tk = (x - kg[ik]) / (kg[ik + 1] - kg[ik])
    return ref.keys_weights(c["k_opt"], kg, c["K_grid"], x, ik, tk, K, z)
