"""CPU census of tests/ks_panel_cases.py: the oracle alone reaches every branch the GPU parity
tests (tests/test_ks_panel_adversarial_gpu.py) are meant to pin.  These are the conditions that
keep those comparisons from passing vacuously, not measurements: if one fails, the inputs change,
not the condition.  The defect table at the end restates the kernels with one defect at a time
and counts the cases on which the outputs change — the evidence that the bit-for-bit GPU
comparison would notice the same defect in csrc/ks_panel_kernels.hip."""
import numpy as np
import pytest

from oracle import np_oracle as no
from tests import ks_panel_cases as cases
from tests.test_ks_panel_cpu import _literal_shocks


@pytest.fixture(scope="module")
def traces():
    return {c["name"]: cases.trace(c) for c in cases.two_sided_cases() + cases.special_cases()}


def test_listed_geometry():
    assert [no.ks_panel_blocks(n) for n in cases.REDUCTION_POPS] == list(cases.REDUCTION_G)
    assert {cases.staging_path(*s) for s in cases.PANEL_SHAPES} == {"one", "looped", "global"}
    assert [cases.staging_path(*s) for s in ((256, 256), (257, 4), (100, 257), (8189, 3),
                                              (8190, 2), (8190, 3), (8191, 2))] == \
        ["one", "looped", "looped", "looped", "looped", "global", "global"]
    assert set(cases.HOST_SHAPES) <= set(cases.PANEL_SHAPES)
    assert {T for T, _ in cases.SHOCK_SHAPES} == {1, 2, 32, 33, 34, 64, 65, 66, 129, 130}
    assert {n for _, n in cases.SHOCK_SHAPES} == {1, 255, 256, 257}
    with pytest.raises(AssertionError):
        cases.grid_p(2100, 7)   # x^7 repeats k_min: the host tier refuses such a grid
    for ug, ub in cases.UG_UB:
        cases.thresholds(cases.shock_params(ug, ub)[0])   # asserts all eleven inside (0, 1)


@pytest.mark.parametrize("nk,nK", cases.PANEL_SHAPES)
def test_two_sided_cases_leave_the_grid_on_both_sides(traces, nk, nK):
    """Per shape, over the three starts: at least 50 agent-periods each below k_grid[0], above
    k_grid[-1] and exactly on a node; everything stays finite and bounded."""
    below = above = node = 0
    for K0 in cases.STARTS:
        c = cases.panel_case(nk, nK, K0)
        ks, Ks = traces[c["name"]]
        kg = c["k_grid"]
        below += int(np.sum(ks < kg[0]))
        above += int(np.sum(ks > kg[-1]))
        node += int(np.sum(np.isin(ks, kg)))
        K_ts, kf = cases.oracle(c)
        assert np.array_equal(K_ts, Ks)
        assert np.all(np.isfinite(K_ts)) and max(np.abs(ks).max(), np.abs(kf).max()) < 1e5
        assert c["k0"][0] == kg[0] and c["k0"][-1] == kg[-1]
    assert min(below, above, node) >= 50, (below, above, node)


@pytest.mark.parametrize("path", ["one", "looped", "global"])
def test_every_staging_path_sees_K_below_inside_and_above(traces, path):
    lo = mid = hi = 0
    shapes = [s for s in cases.PANEL_SHAPES if cases.staging_path(*s) == path]
    assert len(shapes) >= 3
    for nk, nK in shapes:
        for K0 in cases.STARTS:
            c = cases.panel_case(nk, nK, K0)
            K = traces[c["name"]][1][:-1]      # the periods whose K_t is searched
            Kg = c["K_grid"]
            lo += int(np.sum(K < Kg[0]))
            mid += int(np.sum((K >= Kg[0]) & (K <= Kg[-1])))
            hi += int(np.sum(K > Kg[-1]))
    assert min(lo, mid, hi) >= 2, (lo, mid, hi)


@pytest.mark.parametrize("kind", cases.NODE_KINDS)
@pytest.mark.parametrize("nk,nK", cases.NODE_SHAPES)
def test_node_policy_keeps_every_agent_on_a_node(traces, nk, nK, kind):
    c = cases.node_case(nk, nK, kind)
    ks, _ = traces[c["name"]]
    kg = c["k_grid"]
    allk = np.concatenate([ks.ravel(), cases.oracle(c)[1]])
    assert np.all(np.isin(allk, kg))
    # both ends are searched in several periods, not only at the start
    assert np.any(ks[1:] == kg[0]) and np.any(ks[1:] == kg[-1])


@pytest.mark.parametrize("j", [4, 2])
def test_node_K_start_is_exactly_on_the_node(j):
    c = cases.node_K_case(j)
    K_ts, _ = cases.oracle(c)
    assert K_ts[0] == c["K_grid"][j] and np.all(np.isfinite(K_ts))
    assert (j == c["K_grid"].size - 1) or (0 < j < c["K_grid"].size - 1)


def test_nonfinite_cells_are_read_by_some_agents_only():
    c2, c3 = cases.nonfinite_case(2), cases.nonfinite_case(3)
    K2, k2 = cases.oracle(c2)
    n = c2["k0"].size
    assert 0 < np.sum(np.isnan(k2)) < n and 0 < np.sum(np.isposinf(k2)) < n
    assert np.sum(np.isfinite(k2)) > n // 2
    assert np.isfinite(K2[0]) and np.isnan(K2[1])
    K3, k3 = cases.oracle(c3)
    assert np.isfinite(K3[0]) and np.all(np.isnan(K3[1:])) and np.all(np.isnan(k3))


def _left_to_right_mean(x):
    return np.cumsum(x)[-1] / x.size


@pytest.mark.parametrize("pop,G", list(zip(cases.REDUCTION_POPS, cases.REDUCTION_G)))
def test_reduction_cases_tell_the_blocked_mean_from_a_plain_one(pop, G):
    c = cases.reduction_case(pop)
    assert no.ks_panel_blocks(pop) == G
    if G > 1:
        assert no.ks_mean_blocked(c["k0"], G) != _left_to_right_mean(c["k0"])
    K_ts, kf = cases.oracle(c)
    assert K_ts.shape == (3,) and np.all(np.isfinite(K_ts)) and np.all(np.isfinite(kf))


def test_adversarial_uniforms_hit_every_threshold():
    """At least 1 % of all comparisons of the adversarial stream's cases have the draw equal to
    the threshold it is compared with, and each of the eleven thresholds is hit.  pgg == pbb in
    the script (both 1 - 1/8): a kernel that swapped the two cannot be told apart by any input,
    here or on the GPU; they are counted by the aggregate state the comparison is made in."""
    total, hits = 0, np.zeros(11, np.int64)
    for c in cases.shock_cases():
        if c["key"][-1] != "adversarial":
            continue
        assert np.all((c["U"] >= 0) & (c["U"] < 1))
        n, h = cases.shock_hits(c)
        total += n
        hits += h
    assert hits.sum() >= 0.01 * total, (hits.sum(), total)
    assert np.all(hits >= 1), hits
    p = cases.shock_params(*cases.UG_UB[0])[0]
    pr = no.ks_eps_probs(p)
    assert pr["pgg"] == pr["pbb"]


def test_shock_cases_populate_every_state():
    """Over the set, every (cur_z, prev_z, prev_e) threshold is used, in both streams."""
    for stream in cases.STREAMS:
        seen = np.zeros((2, 2, 2), bool)
        for c in cases.shock_cases():
            if c["key"][-1] == stream and c["T"] > 1:
                zi, e = cases.shock_oracle(c)
                for t in range(1, c["T"]):
                    seen[zi[t], zi[t - 1], np.unique(e[t - 1])] = True
        assert seen.all(), stream


# ------------------------------------------------------------------ literal transcriptions


def _pairwise(v):
    n = 1
    while n < len(v):
        n *= 2
    v = list(v) + [0.0] * (n - len(v))
    h = n // 2
    while h >= 1:
        v = [v[l] + v[l + h] if l < h else v[l] for l in range(len(v))]
        h //= 2
    return v[0]


def _literal_panel(kg, Kg, k_opt, zi, e, k0):
    """:206-248 agent by agent (scalar search, edge extrapolation) with the literal mean: lane
    sums in agent order, pairwise fold per block, pairwise fold of the zero-padded block sums
    (tests/test_ks_panel_cpu.py's transcription for any G)."""
    pop, T = len(k0), len(zi)
    G = no.ks_panel_blocks(pop)

    def mean(k):
        lanes = [0.0] * (G * 256)
        for i in range(pop):
            lanes[i % (G * 256)] += k[i]
        return _pairwise([_pairwise(lanes[b * 256:(b + 1) * 256]) for b in range(G)]) / pop

    k = [float(v) for v in k0]
    K_ts = [mean(k)]
    for t in range(T - 1):
        K = K_ts[t]
        iK = min(max(int(np.searchsorted(Kg, K, "right")) - 1, 0), len(Kg) - 2)
        tK = (K - Kg[iK]) / (Kg[iK + 1] - Kg[iK])
        new = []
        for i in range(pop):
            s = 2 * zi[t] + e[t, i]
            ik = min(max(int(np.searchsorted(kg, k[i], "right")) - 1, 0), len(kg) - 2)
            tk = (k[i] - kg[ik]) / (kg[ik + 1] - kg[ik])
            f0 = k_opt[ik, iK, s] + tk * (k_opt[ik + 1, iK, s] - k_opt[ik, iK, s])
            f1 = k_opt[ik, iK + 1, s] + tk * (k_opt[ik + 1, iK + 1, s] - k_opt[ik, iK + 1, s])
            new.append(f0 + tK * (f1 - f0))
        k = new
        K_ts.append(mean(k))
    return np.array(K_ts), np.array(k)


def test_vectorised_oracle_equals_the_literal_loops():
    c = cases.panel_case(5, 4, 22.0)
    K_l, k_l = _literal_panel(c["k_grid"], c["K_grid"], c["k_opt"], c["zi"][:6], c["e"][:6],
                              c["k0"])
    K_o, k_o = no.ks_panel_simulate(c["k_grid"], c["K_grid"], c["k_opt"], c["zi"][:6],
                                    c["e"][:6], c["k0"])
    assert np.array_equal(K_l, K_o) and np.array_equal(k_l, k_o)
    assert np.any(c["k0"] < c["k_grid"][0]) and np.any(c["k0"] > c["k_grid"][-1])
    s = cases.shock_case(34, 255, 0.2, 0.35, "adversarial")
    assert cases.shock_hits(s)[1].sum() > 50
    zl, el = _literal_shocks(s["p"], s["T"], s["pop"], s["U"])
    zi, e = cases.shock_oracle(s)
    assert np.array_equal(zi, zl) and np.array_equal(e + 1, el)


# ------------------------------------------------------------------ defect table

PANEL_DEFECTS = ("search_lt", "no_upper_clamp", "no_lower_clamp", "tK_unclamped",
                 "state_swapped", "strides_swapped")
MEAN_DEFECTS = ("blocks_left_to_right", "first_64_first")
SHOCK_DEFECTS = ("ge_aggregate", "ge_initial", "ge_idiosyncratic", "thr_transposed",
                 "prev_e_from_t_minus_2")


def _fold(v):
    """Pairwise fold of v zero-padded to a power of two (h = n/2 ... 1: s[l] + s[l+h])."""
    n = 1
    while n < v.size:
        n *= 2
    q = np.zeros(n)
    q[:v.size] = v
    h = n // 2
    while h >= 1:
        q = q.copy()
        q[:h] = q[:h] + q[h:2 * h]
        h //= 2
    return q[0]


def _mean(x, G, defect):
    n, L = x.size, G * 256
    lanes = np.zeros(L)
    for m in range(0, n, L):
        seg = x[m:m + L]
        lanes[:seg.size] = lanes[:seg.size] + seg
    s = lanes.reshape(G, 256)
    h = 128
    while h >= 1:
        s = s.copy()
        s[:, :h] = s[:, :h] + s[:, h:2 * h]
        h //= 2
    b = s[:, 0]
    if defect == "blocks_left_to_right":
        tot = np.cumsum(b)[-1]
    elif defect == "first_64_first":     # each run of 64 partials folded on its own, then the runs
        tot = _fold(np.array([_fold(b[i:i + 64]) for i in range(0, G, 64)]))
    else:
        tot = _fold(b)
    return tot / n


def _seg(x, q, defect):
    """(segment the values are read from, segment the weight is taken from)."""
    n = x.size
    raw = np.searchsorted(x, q, side="left" if defect == "search_lt" else "right") - 1
    lo = -1 if defect == "no_lower_clamp" else 0
    hi = n - 1 if defect == "no_upper_clamp" else n - 2
    return np.clip(raw, lo, hi), raw


def _panel_variant(c, defect):
    """np_oracle.ks_panel_simulate restated with one defect (reads past an end wrap round)."""
    kg, Kg, ko, zi, e = c["k_grid"], c["K_grid"], c["k_opt"], c["zi"], c["e"]
    nk, nK = kg.size, Kg.size
    flat = np.ascontiguousarray(ko.transpose(2, 1, 0)).ravel()   # (s*nK + iK)*nk + ik
    k = c["k0"].copy()
    T = zi.size
    G = no.ks_panel_blocks(k.size)
    K_ts = np.zeros(T)
    K_ts[0] = _mean(k, G, defect)
    for t in range(T - 1):
        K = K_ts[t]
        iK, rawK = _seg(Kg, np.array([K]), defect)
        iK, iw = int(iK[0]), int(rawK[0]) if defect == "tK_unclamped" else int(iK[0])
        tK = (K - Kg[iw % nK]) / (Kg[(iw + 1) % nK] - Kg[iw % nK])
        s = e[t].astype(np.int64) * 2 + int(zi[t]) if defect == "state_swapped" \
            else 2 * int(zi[t]) + e[t].astype(np.int64)
        ik, _ = _seg(kg, k, defect)
        tk = (k - kg[ik % nk]) / (kg[(ik + 1) % nk] - kg[ik % nk])

        def rd(a, b):
            if defect == "strides_swapped":
                return flat[(s * nk + a % nk) * nK + b % nK]
            return flat[(s * nK + b % nK) * nk + a % nk]
        f00, f10, f01, f11 = rd(ik, iK), rd(ik + 1, iK), rd(ik, iK + 1), rd(ik + 1, iK + 1)
        f0 = f00 + tk * (f10 - f00)
        f1 = f01 + tk * (f11 - f01)
        k = f0 + tK * (f1 - f0)
        K_ts[t + 1] = _mean(k, G, defect)
    return K_ts, k


def _shocks_variant(c, defect):
    p, T, pop, U = c["p"], c["T"], c["pop"], c["U"]
    pr = no.ks_eps_probs(p)

    def gt(u, th, which):
        return u >= th if defect == "ge_" + which else u > th
    zi = np.zeros(T, np.int8)
    z = 0
    for t in range(1, T):
        z = int(gt(U[t - 1], pr["pbb"] if z else pr["pgg"], "aggregate"))
        zi[t] = z
    pos = T - 1
    e = np.zeros((T, pop), np.int8)
    e[0] = gt(U[pos:pos + pop], p["ug"], "initial")
    pos += pop
    for t in range(1, T):
        th = pr["thr"][zi[t - 1], zi[t]] if defect == "thr_transposed" \
            else pr["thr"][zi[t], zi[t - 1]]
        ep = e[t - 2] if defect == "prev_e_from_t_minus_2" and t >= 2 else e[t - 1]
        e[t] = gt(U[pos:pos + pop], th[ep], "idiosyncratic")
        pos += pop
    return zi, e


def _differs(got, want):
    return not all(np.array_equal(g, w) for g, w in zip(got, want))


def test_defect_table():
    """Every defect changes K_ts, k_final, zi or eps on at least one case; without a defect the
    restatements equal the oracle on every case.  Cases that differ, of the 44 finite panel
    cases (36 two-sided, 6 node-policy, 2 node-K), those and the 12 reduction cases for the
    mean's order, and the 84 shock cases:

        x[mid] < q instead of <= in the search            4 of 44
        no upper clamp to n - 2 (n - 1, wrapped read)     36 of 44
        no lower clamp                                    36 of 44
        tK taken from the unclamped segment               36 of 44
        state index 2 e + z instead of 2 z + e            44 of 44
        k_opt indexed with nK and nk strides swapped      44 of 44
        block sums folded left to right                   52 of 56
        the first 64 partials folded first                7 of 56 (all seven with G > 64)
        >= in the aggregate comparison                    30 of 84
        >= in the initial comparison                      30 of 84
        >= in the idiosyncratic comparison                31 of 84
        thr indexed [prev_z][cur_z]                       59 of 84
        previous employment taken from t - 2              58 of 84

    (counted when the cases were written; the assertion is one case at least per defect).  The
    tie rule shows only where f(j-1) + 1 * (f(j) - f(j-1)) is not f(j) bit for bit: the three
    scatter node policies and one two-sided case.
    """
    panel = cases.finite_panel_cases()
    reduction = [cases.reduction_case(n) for n in cases.REDUCTION_POPS]
    shocks = cases.shock_cases()
    for c in panel + reduction:
        assert not _differs(_panel_variant(c, None), cases.oracle(c)), c["name"]
    for c in shocks:
        assert not _differs(_shocks_variant(c, None), cases.shock_oracle(c)), c["name"]
    counts = {}
    with np.errstate(all="ignore"):   # wrapped reads and unclamped weights overflow
        for d in PANEL_DEFECTS:
            counts[d] = sum(_differs(_panel_variant(c, d), cases.oracle(c)) for c in panel)
        for d in MEAN_DEFECTS:
            counts[d] = sum(_differs(_panel_variant(c, d), cases.oracle(c))
                            for c in panel + reduction)
    for d in SHOCK_DEFECTS:
        counts[d] = sum(_differs(_shocks_variant(c, d), cases.shock_oracle(c)) for c in shocks)
    print(counts)
    assert all(n >= 1 for n in counts.values()), counts
    # the register stage of the fold is pinned by the G > 64 cases alone
    big = [c for c in reduction if no.ks_panel_blocks(c["k0"].size) > 64]
    assert all(_differs(_panel_variant(c, "first_64_first"), cases.oracle(c)) for c in big)
