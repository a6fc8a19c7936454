"""Deterministic adversarial cases for the Krusell-Smith VFI and EGM kernels, shared by the CPU
census (tests/test_ks_cases_cpu.py) and the GPU parity tests (tests/test_ks_adversarial_gpu.py,
tests/test_ks_egm_adversarial_gpu.py).  A plain module: every builder is a pure function of its
arguments (np.random.default_rng(seed)), so both sides see the same bytes.

A case is a dict(name, p, k_grid, K_grid, P, B, V | k0): p is the np_oracle-style parameter
dict; prm(p) / cparams(p) turn it into the 13-double block of the C ABI and the C oracle's
struct.  Arrays are k x K x S as in the scripts.
"""
from __future__ import annotations

import math

import numpy as np

from oracle import np_oracle as no

# (nk, nK) of the VFI pieces: the smallest legal grids, the 64-lane block edge, the fused
# Howard+slopes geometry switch (one block per column up to 256, then 252 own nodes + halo:
# 257 -> tiles of 252 + 5, 505 / 506 -> a last tile of 1 / 2 own nodes)
VFI_SIZES = ((3, 1), (4, 2), (64, 5), (65, 1), (253, 2), (256, 1), (257, 2), (505, 1), (506, 5))
# ks_fused_fits switches at 4,096 nodes: (256, 4) is the one-workgroup kernel, (257, 4) tiled
SOLVE_SIZES = ((256, 4), (257, 4), (65, 2))
VFI_FAMILIES = ("smooth", "noise005", "noise5", "decreasing", "endrule", "nan")
NOISE = {"smooth": 0.0, "noise005": 0.05, "noise5": 5.0, "decreasing": 0.0, "endrule": 0.05,
         "nan": 5.0}

_BASE = dict(beta=0.99, alpha=0.36, delta=0.025, ug=0.04, ub=0.10, mu=0.0, z_grid=(1.01, 0.99),
             eps_grid=(1.0, 0.0))

# parameter / ALM variants.  K' = exp(B0 + B1 log K) per z, then clamped to K_grid and snapped
# to the nearest point (first index on a tie):
#   0  defaults, identity ALM, mu = 0 (unemployed at k_min: a degenerate fminbnd interval)
#   1  mu = 0.15, a contracting ALM (K' index moves)
#   2  mu = 0.3, beta = 0.95, delta = 0.06; K' = sqrt(K) clamps at K_grid(1) for one z and
#      K' = e K clamps at K_grid(end) for the other
#   3  mu = 0, K' = exp(0) = 1 exactly, on a K_grid whose points 0.5 and 1.5 are equidistant
VARIANTS = (
    dict(mu=0.0, B=(0.0, 1.0, 0.0, 1.0), K="default"),
    dict(mu=0.15, B=(0.1, 0.97, 0.08, 0.975), K="default"),
    dict(mu=0.3, beta=0.95, delta=0.06, B=(0.0, 0.5, 1.0, 1.0), K="default"),
    dict(mu=0.0, B=(0.0, 0.0, 0.0, 0.0), K="tie"),
)
_K_TIE = {1: (1.0,), 2: (0.5, 1.5), 5: (0.25, 0.5, 1.5, 2.0, 3.0), 4: (0.5, 1.5, 2.0, 3.0)}


def params(k_min, k_max, **kw):
    p = dict(_BASE, k_min=float(k_min), k_max=float(k_max))
    p.update(kw)
    p["l_bar"] = 1 / (1 - p["ub"])
    return p


def prm(p):
    """The 13-double parameter block of the C ABI."""
    return np.array([p["beta"], p["alpha"], p["delta"], p["k_min"], p["k_max"], p["ug"], p["ub"],
                     p["l_bar"], p["mu"], p["z_grid"][0], p["z_grid"][1], p["eps_grid"][0],
                     p["eps_grid"][1]], dtype=np.float64)


def cparams(p):
    from oracle import corc
    return corc.ks_params(**p)


def transition():
    return no.ks_setup(k_size=3, K_size=1)[3]


def irregular_grid(nk, seed, k_min=1e-4):
    """k_min + cumsum(10**U(-3, 1.2)): neighbouring spacings differ by up to 10^4.2."""
    rng = np.random.default_rng(seed)
    return k_min + np.cumsum(10.0 ** rng.uniform(-3.0, 1.2, nk))


def K_grid_of(nK, kind="default"):
    if kind == "tie":
        return np.array(_K_TIE[nK])
    return np.array([40.0]) if nK == 1 else np.linspace(30.0, 50.0, nK)


def _shape3(col_fn, nk, nK):
    V = np.empty((nk, nK, 4))
    for s in range(4):
        for K in range(nK):
            V[:, K, s] = col_fn(K, s)
    return V


def _end_rule_values(x, which, at_end):
    """Three values whose pchip end slope takes branch `which` (0: sign mismatch -> 0,
    1: |d| > 3|e0| -> 3 e0, 2: plain) at the first (or, mirrored, the last) grid point.
    e0 is the end interval's secant, e1 the next one's; d = ((2h0 + h1) e0 - h0 e1)/(h0 + h1)."""
    if at_end:
        h0, h1 = x[-1] - x[-2], x[-2] - x[-3]
    else:
        h0, h1 = x[1] - x[0], x[2] - x[1]
    e0 = 1.0
    if which == 0:
        e1 = 2.0 * (2 * h0 + h1) / h0 + 1.0          # d < 0 < e0
    elif which == 1:
        e1 = -(2.0 * (1.0 + 2.0 * h1 / h0) + 1.0)    # signs differ and d > 3 e0
    else:
        e1 = 0.5                                      # same signs, d > 0
    if at_end:   # y[n-1] - y[n-2] = e0 h0, y[n-2] - y[n-3] = e1 h1
        return np.array([-(e0 * h0 + e1 * h1), -e0 * h0, 0.0])
    return np.array([0.0, e0 * h0, e0 * h0 + e1 * h1])


def end_rule_branch(x, y, at_end):
    """Which end-rule outcome pchip takes for column y: 0, 1 or 2 as in _end_rule_values."""
    if at_end:
        x, y = -np.asarray(x)[::-1], np.asarray(y)[::-1]
    h0, h1 = x[1] - x[0], x[2] - x[1]
    e0, e1 = (y[1] - y[0]) / h0, (y[2] - y[1]) / h1
    d = ((2 * h0 + h1) * e0 - h0 * e1) / (h0 + h1)
    if np.sign(d) != np.sign(e0):
        return 0
    if np.sign(e0) != np.sign(e1) and abs(d) > abs(3 * e0):
        return 1
    return 2


def value_family(family, k_grid, nK, seed):
    """A k x K x 4 start value of one family on k_grid."""
    nk = len(k_grid)
    rng = np.random.default_rng(seed)
    scale = NOISE[family]

    def col(K, s):
        base = 100.0 * np.log(0.1 * (k_grid + 1.0 + 0.5 * K + 0.25 * s))   # smooth, concave
        if family == "decreasing":
            base = -100.0 * np.log(k_grid + 1.0 + 0.5 * K + 0.25 * s)      # optimum at k_min
        y = base + scale * rng.standard_normal(nk)
        if family in ("noise005", "noise5", "nan", "endrule"):
            flat = np.flatnonzero(rng.random(nk) < 0.10)                     # exact flat segments
            for i in flat[flat > 0]:
                y[i] = y[i - 1]
        if family == "endrule":
            c = s * nK + K
            y[:3] = y[3 % nk] + _end_rule_values(k_grid, c % 3, False)
            if nk >= 6:
                y[-3:] = y[-4] + _end_rule_values(k_grid, (c + 1) % 3, True)
        if family == "nan":
            y[rng.choice(nk, size=max(1, nk // 100), replace=False)] = np.nan
        return y

    return _shape3(col, nk, nK)


def vfi_case(nk, nK, family, variant, seed):
    v = VARIANTS[variant]
    kind = v["K"]
    kg = irregular_grid(nk, seed)
    extra = {k: v[k] for k in ("mu", "beta", "delta") if k in v}
    p = params(kg[0], kg[-1], **extra)
    return dict(name=f"{family}-{nk}x{nK}-v{variant}", p=p, k_grid=kg, K_grid=K_grid_of(nK, kind),
                P=transition(), B=np.array(v["B"], dtype=np.float64),
                V=value_family(family, kg, nK, seed + 1), family=family, variant=variant)


def vfi_cases(sizes=VFI_SIZES):
    """Every family at every size; the parameter variant rotates so each family meets each."""
    out = []
    for i, (nk, nK) in enumerate(sizes):
        for j, fam in enumerate(VFI_FAMILIES):
            out.append(vfi_case(nk, nK, fam, (i + j) % len(VARIANTS), 1000 + 17 * i + j))
    return out


def improve_upper_bound(case):
    """fminbnd's upper bound min(res, k_max) per node (Krusell_Smith_VFI.m:152-159), k x K x 4,
    in np_oracle.ks_policy_improve's operation order."""
    p, kg, Kg = case["p"], case["k_grid"], case["K_grid"]
    a = p["alpha"]
    out = np.empty((len(kg), len(Kg), 4))
    for s_i in range(4):
        zt = p["z_grid"][0] if s_i < 2 else p["z_grid"][1]
        eps = p["eps_grid"][0] if s_i % 2 == 0 else p["eps_grid"][1]
        L = p["l_bar"] * (1 - p["ug"] * float(zt == p["z_grid"][0])
                          - p["ub"] * float(zt == p["z_grid"][1]))
        for K_i, K in enumerate(map(float, Kg)):
            wt = (1 - a) * zt * math.pow(K, a) * math.pow(L, -a)
            rt = a * zt * math.pow(K, a - 1) * math.pow(L, 1 - a)
            res = (rt + 1 - p["delta"]) * kg + wt * (eps * p["l_bar"] + (1 - eps) * p["mu"])
            out[:, K_i, s_i] = np.minimum(res, p["k_max"])
    return out


def forecast_ties(case):
    """(s, K) slices whose clamped forecast K' is equidistant from two K_grid points."""
    p, Kg, B = case["p"], case["K_grid"], case["B"]
    n = 0
    for s_i in range(4):
        z = p["z_grid"][1] if (s_i + 1) <= 2 else p["z_grid"][0]     # bellman_value's z (:332)
        b = B[0:2] if z == p["z_grid"][0] else B[2:4]
        for K in map(float, Kg):
            Kp = math.exp(b[0] + b[1] * math.log(max(K, 1e-8)))
            Kp = max(min(Kp, Kg[-1]), Kg[0])
            dist = np.abs(Kg - Kp)
            n += int((dist == dist.min()).sum() > 1)
    return n


def forecast_clamps(case):
    """(low, high): slices whose unclamped forecast lies below K_grid(1) / above K_grid(end)."""
    p, Kg, B = case["p"], case["K_grid"], case["B"]
    lo = hi = 0
    for s_i in range(4):
        z = p["z_grid"][1] if (s_i + 1) <= 2 else p["z_grid"][0]
        b = B[0:2] if z == p["z_grid"][0] else B[2:4]
        for K in map(float, Kg):
            Kp = math.exp(b[0] + b[1] * math.log(max(K, 1e-8)))
            lo += Kp < Kg[0]
            hi += Kp > Kg[-1]
    return lo, hi


def howard_kopt(case, seed):
    """Adversarial Howard policy: uniform on [k_min - 1, k_max + 1] (clamped by bellman_value),
    every third entry exactly on a random node, some exactly k_grid(1), k_grid(end - 1) and
    k_grid(end)."""
    kg = case["k_grid"]
    shape = case["V"].shape
    rng = np.random.default_rng(seed)
    ko = rng.uniform(kg[0] - 1.0, kg[-1] + 1.0, shape).reshape(-1, order="F")
    ko[::3] = kg[rng.integers(0, len(kg), ko[::3].size)]
    n = ko.size
    for j, node in enumerate((kg[0], kg[-2], kg[-1])):
        ko[rng.choice(n, size=max(1, n // 50), replace=False)] = node
    return ko.reshape(shape, order="F")


def solve_case(nk, nK, seed, variant=1):
    """ks_vfi_solve start: a noisy value with flat runs and hand-built end-rule columns (the
    one-workgroup kernel has a slope routine of its own) and a random policy."""
    c = vfi_case(nk, nK, "endrule", variant, seed)
    c["k0"] = howard_kopt(c, seed + 2)
    return c


# ------------------------------------------------------------------------------ EGM
def _egm_base(nk=60, nK=3, k_max=1000.0, B=(0.1, 0.97, 0.08, 0.975)):
    p, kg, Kg, P, _, _ = no.ks_setup(k_size=nk, K_size=max(nK, 2))
    if nK == 1:
        Kg = np.array([40.0])
    if k_max != 1000.0:
        p["k_max"] = k_max
        kg = (no.matlab_linspace01(nk) ** 7) * (k_max - p["k_min"]) + p["k_min"]
        kg[0], kg[-1] = p["k_min"], k_max
    return p, kg, Kg, P, np.array(B, dtype=np.float64)


def egm_cases():
    """The EGM starts: name -> case.  k0 is k x K x 4."""
    out = []

    def add(name, k0_fn, **kw):
        p, kg, Kg, P, B = _egm_base(**kw)
        rng = np.random.default_rng(sum(map(ord, name)))
        full = np.repeat(np.repeat(kg[:, None, None], len(Kg), 1), 4, 2)
        out.append(dict(name=name, p=p, k_grid=kg, K_grid=Kg, P=P, B=B,
                        k0=np.asfortranarray(k0_fn(full, p, rng))))

    add("uniform", lambda k, p, r: r.uniform(p["k_min"], p["k_max"], k.shape))
    add("noisy09", lambda k, p, r: 0.9 * k * (1 + 0.2 * r.standard_normal(k.shape)))
    add("const_kmin", lambda k, p, r: np.full(k.shape, p["k_min"]))
    add("const_kmax", lambda k, p, r: np.full(k.shape, p["k_max"]))
    add("k12", lambda k, p, r: 1.2 * k)
    add("staircase", lambda k, p, r: np.round(0.9 * k, -1))

    def with_nan(k, p, r):
        y = 0.9 * k
        y.reshape(-1)[r.choice(y.size, size=8, replace=False)] = np.nan
        return y
    add("nan8", with_nan)
    add("kmax40", lambda k, p, r: 0.9 * k, k_max=40.0)
    add("nk5", lambda k, p, r: 0.9 * k, nk=5, nK=1)
    add("nk3", lambda k, p, r: 0.9 * k, nk=3, nK=2)
    # Beyond the listed starts.  k_current = ((c + k') - We) / R never ties on a grid whose
    # points are far apart in ulps, and never is NaN for finite inputs (the c_next floor maps
    # NaN to 1e-8), so the sort's tie order and NaN-last rule need inputs of their own:
    #  twins  every third grid point from the 11th on is followed by its next double — the sum
    #         c + k' rounds such pairs together: exact ties among the valid points
    #  nanP   P(4, :) = NaN: every k_current of the s = 4 pairs is NaN, none is valid
    p, kg, Kg, P, B = _egm_base()
    tw = np.sort(np.concatenate([kg, np.nextafter(kg[10::3], np.inf)]))
    full = np.repeat(np.repeat(tw[:, None, None], len(Kg), 1), 4, 2)
    out.append(dict(name="twins", p=p, k_grid=tw, K_grid=Kg, P=P, B=B,
                    k0=np.asfortranarray(np.round(0.9 * full, -1))))
    Pn = P.copy()
    Pn[3, :] = np.nan
    out.append(dict(out[1], name="nanP", P=Pn))
    return out


def egm_k_current(case, k_opt, s_i, K_i):
    """k_current of Krusell_Smith_EGM.m:155-189 for pair (s_i, K_i) reading k_opt — the array
    the pair's rank sort sees (np_oracle.ks_egm_sweep keeps it local)."""
    p, kg, Kg, P, B = case["p"], case["k_grid"], case["K_grid"], case["P"], case["B"]
    nK = len(Kg)
    q = no.ks_egm_pairs(p, Kg, B)[s_i * nK + K_i]
    cols = [np.asarray(k_opt)[:, q["kd"][s_j], s_j] for s_j in range(4)]
    with np.errstate(all="ignore"):
        slopes = [no.pchip_slopes(kg, c) for c in cols]
        kc = np.empty(len(kg))
        for t, kp in enumerate(map(float, kg)):
            em = 0.0
            for s_j in range(4):
                kpn = no.pchip_eval(kg, cols[s_j], slopes[s_j], kp)
                cn = (q["Rn"][s_j] * kp + q["Wn"][s_j]) - kpn
                cn = cn if cn > 1e-8 else 1e-8
                em = em + (P[s_i, s_j] * q["Rn"][s_j]) / cn
            kc[t] = (((1 / (p["beta"] * em)) + kp) - q["We"]) / q["R"]
    return kc


def egm_census(case, k_opt):
    """Over every pair reading k_opt: how many have k_current below k_min, above k_max, NaN,
    exact ties among the valid points, and fewer than two valid points."""
    p = case["p"]
    c = dict(below=0, above=0, nan=0, ties=0, short=0)
    for s_i in range(4):
        for K_i in range(len(case["K_grid"])):
            kc = egm_k_current(case, k_opt, s_i, K_i)
            valid = kc[(kc >= p["k_min"]) & (kc <= p["k_max"])]
            c["below"] += bool((kc < p["k_min"]).any())
            c["above"] += bool((kc > p["k_max"]).any())
            c["nan"] += bool(np.isnan(kc).any())
            c["ties"] += bool(len(np.unique(valid)) < len(valid))
            c["short"] += bool(len(valid) < 2)
    return c


def rel_diff(V, Vold):
    """Krusell_Smith_VFI.m:195: nanmax(|V - Vold| / (|Vold| + 1e-10)); NaN if every entry is."""
    with np.errstate(all="ignore"):
        d = np.abs(V - Vold) / (np.abs(Vold) + 1e-10)
    return math.nan if np.all(np.isnan(d)) else float(np.nanmax(d))
