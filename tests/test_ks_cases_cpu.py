"""CPU: the adversarial Krusell-Smith cases of tests/ks_cases.py do reach the branches the GPU
parity tests are meant to break (a census with the oracles alone — conditions, not
measurements), and the C oracle equals the numpy restatement bit for bit off the defaults."""
import functools

import numpy as np
import pytest

from oracle import corc
from oracle import np_oracle as no
from tests import ks_cases as kc


@functools.lru_cache(maxsize=None)
def _vfi():
    """Every VFI case with the C oracle's improvement: [(case, k_opt, nfev)]."""
    out = []
    for c in kc.vfi_cases():
        ko, nf = corc.ks_policy_improve(kc.cparams(c["p"]), c["k_grid"], c["K_grid"], c["V"],
                                        c["B"], c["P"])
        out.append((c, ko, nf))
    return out


def _columns(c):
    V = c["V"]
    for K in range(V.shape[1]):
        for s in range(4):
            yield V[:, K, s]


def test_slope_branch_census():
    """Interior slopes: the harmonic-mean branch and the 0.0 branch, each >= 20 times in every
    noisy case with nk >= 64.  End rule: each of the three outcomes at each end, overall — and
    the classification agrees with the slopes np_oracle.pchip_slopes returns."""
    ends = [set(), set()]
    noisy = 0
    for c, _, _ in _vfi():
        kg = c["k_grid"]
        zero = prod = 0
        for y in _columns(c):
            with np.errstate(all="ignore"):
                d = no.pchip_slopes(kg, y)
                sec = np.diff(y) / np.diff(kg)
            taken = np.sign(sec[:-1]) * np.sign(sec[1:]) > 0
            prod += int(taken.sum())
            zero += int((~taken).sum())
            assert np.all(d[1:-1][~taken] == 0.0)
            if np.isnan(y[:3]).any() or np.isnan(y[-3:]).any():
                continue
            for end, (dd, e0) in enumerate(((d[0], sec[0]), (d[-1], sec[-1]))):
                b = kc.end_rule_branch(kg, y, bool(end))
                ends[end].add(b)
                assert (b == 0 and dd == 0.0) or (b == 1 and dd == 3 * e0) or b == 2, c["name"]
        if c["family"] in ("noise005", "noise5") and len(kg) >= 64:
            noisy += 1
            assert prod >= 20 and zero >= 20, (c["name"], prod, zero)
    assert noisy >= 10
    assert ends[0] == {0, 1, 2} and ends[1] == {0, 1, 2}, ends


@pytest.mark.parametrize("nk,nK", kc.SOLVE_SIZES)
def test_solve_starts_reach_every_slope_branch(nk, nK):
    """The ks_vfi_solve starts (4,096 nodes: the one-workgroup kernel's own slope routine) take
    both interior branches >= 20 times and every end-rule outcome at each end."""
    c = kc.solve_case(nk, nK, 300 + nk)
    kg = c["k_grid"]
    ends = [set(), set()]
    prod = zero = 0
    for y in _columns(c):
        sec = np.diff(y) / np.diff(kg)
        taken = np.sign(sec[:-1]) * np.sign(sec[1:]) > 0
        prod, zero = prod + int(taken.sum()), zero + int((~taken).sum())
        for end in (0, 1):
            ends[end].add(kc.end_rule_branch(kg, y, bool(end)))
    assert prod >= 20 and zero >= 20
    assert ends[0] == {0, 1, 2} and ends[1] == {0, 1, 2}
    assert (c["k0"] < kg[0]).any() and (c["k0"] > kg[-1]).any()


def test_flat_segments_and_nan_entries_present():
    for c, _, _ in _vfi():
        if len(c["k_grid"]) < 64:
            continue
        if c["family"] in ("noise005", "noise5"):
            assert sum(int((np.diff(y) == 0).sum()) for y in _columns(c)) >= 4, c["name"]
        if c["family"] == "nan":
            assert np.isnan(c["V"]).any() and not np.isinf(c["V"]).any()
        if c["family"] == "decreasing":
            assert all((np.diff(y) < 0).all() for y in _columns(c))


def test_grid_spacing_varies_by_four_decades():
    for nk, _ in kc.VFI_SIZES:
        h = np.diff(kc.irregular_grid(nk, 1000))
        assert (h > 0).all()
        if nk >= 64:
            assert h.max() / h.min() > 1e3


def test_calibration_grids_are_strictly_increasing(pkg):
    """The x^7 grid rounds its first points onto k_min from k_size = 2,043 on; the calibration
    moves each repeat to the next double (the KS entry points refuse repeated points) and
    leaves every grid the formula already separates untouched."""
    cal = pkg.calibration
    for nk in (100, 300, 1000, 2042):
        kg = cal.krusell_smith(k_size=nk)[0]
        x = cal.linspace01(nk)
        raw = (x ** 7) * (1000.0 - 0.0001) + 0.0001
        raw[0], raw[-1] = 0.0001, 1000.0
        assert np.array_equal(kg, raw) and (np.diff(kg) > 0).all()
    for nk in (4096, 4099, 32768):
        kg, _, _, V0 = cal.krusell_smith(k_size=nk, K_size=1)
        assert (np.diff(kg) > 0).all() and kg[0] == 0.0001 and kg[-1] == 1000.0
        x = cal.linspace01(nk)
        raw = (x ** 7) * (1000.0 - 0.0001) + 0.0001
        moved = np.flatnonzero(kg[1:-1] != raw[1:-1])
        assert 0 < moved.size < 64 and moved.max() < 64       # only the first few points
        assert np.all(kg[1:-1][moved] - raw[1:-1][moved] < 64 * np.spacing(0.0001))
        assert np.isfinite(V0).all()


def test_fminbnd_census():
    """nfev == 1 (mu = 0, unemployed, k = k_min: a degenerate interval); >= 20 distinct nfev on
    a noisy case with nk >= 257; an optimum within 1e-3 of k_min and one within 1e-3 of the
    upper bound min(res, k_max)."""
    degenerate = distinct = at_min = at_max = 0
    for c, ko, nf in _vfi():
        if c["p"]["mu"] == 0.0:
            degenerate += int((nf[0, :, 1::2] == 1).sum())
        if c["family"] in ("noise005", "noise5") and len(c["k_grid"]) >= 257:
            distinct = max(distinct, len(np.unique(nf)))
        ub = kc.improve_upper_bound(c)
        ok = ~np.isnan(ko)
        at_min += int((np.abs(ko - c["p"]["k_min"]) < 1e-3)[ok].sum())
        at_max += int(((np.abs(ko - ub) < 1e-3) & (ub - c["p"]["k_min"] > 1.0))[ok].sum())
        assert nf.min() >= 1 and nf.max() <= 500
    assert degenerate >= 1
    assert distinct >= 20
    assert at_min >= 1 and at_max >= 1


def test_alm_variants_clamp_and_tie():
    """The B sets clamp K' at both ends of K_grid, and one forecast is equidistant from two K
    points (the first index wins in every implementation: strict < in the scan)."""
    lo = hi = ties = 0
    mus = set()
    for c, _, _ in _vfi():
        a, b = kc.forecast_clamps(c)
        lo, hi, ties = lo + a, hi + b, ties + kc.forecast_ties(c)
        mus.add(c["p"]["mu"])
    assert lo >= 1 and hi >= 1 and ties >= 1
    assert mus == {0.0, 0.15, 0.3}


def test_howard_policy_hits_nodes_and_leaves_the_grid():
    c = kc.vfi_case(506, 5, "noise5", 1, 7)
    ko, kg = kc.howard_kopt(c, 8), c["k_grid"]
    assert (ko < kg[0]).any() and (ko > kg[-1]).any()
    assert np.isin(ko, kg).mean() > 0.3
    for node in (kg[0], kg[-2], kg[-1]):
        assert (ko == node).any()


# ------------------------------------------------------------------------------ EGM
@functools.lru_cache(maxsize=None)
def _egm_census():
    """name -> list of censuses: of the start, and of the C oracle's Jacobi iterates after 1
    and 3 sweeps (what the pairs of sweeps 1, 2 and 4 read)."""
    out = {}
    for c in kc.egm_cases():
        cen = [kc.egm_census(c, c["k0"])]
        for sweeps in (1, 3):
            try:
                R = corc.ks_egm_solve(kc.cparams(c["p"]), c["k_grid"], c["K_grid"], c["B"],
                                      c["P"], c["k0"], tol=0.0, max_iter=sweeps, jacobi=True)
            except ValueError:
                break
            cen.append(kc.egm_census(c, R["k_opt"]))
        out[c["name"]] = cen
    return out


def test_egm_census():
    cen = _egm_census()
    total = {k: sum(x[k] for v in cen.values() for x in v) for k in ("below", "above", "nan",
                                                                     "ties", "short")}
    assert total["below"] >= 1      # lo > 0: the valid run does not start at rank 0
    assert total["above"] >= 1
    assert total["nan"] >= 1        # NaN sorts last and is neither below nor valid
    assert total["ties"] >= 1       # equal k_current: index order decides the rank
    assert cen["nk3"][0]["short"] >= 1 and cen["nanP"][0]["short"] >= 1
    assert sum(x["ties"] for x in cen["twins"]) >= 1
    # the c_next floor turns a NaN policy into 1e-8, never into a NaN k_current
    assert all(x["nan"] == 0 for x in cen["nan8"])
    for name, v in cen.items():
        if name not in ("nk3", "nanP"):
            assert all(x["short"] == 0 for x in v), name


def test_egm_oracles_refuse_the_same_starts():
    """nk = 3 on the default grid and the NaN row of P leave a pair with < 2 valid points: the
    C oracle returns rc = -2 and the numpy restatement raises; every other start runs 6 sweeps,
    Gauss-Seidel and Jacobi."""
    for c in kc.egm_cases():
        for jacobi in (False, True):
            args = (kc.cparams(c["p"]), c["k_grid"], c["K_grid"], c["B"], c["P"], c["k0"])
            if c["name"] in ("nk3", "nanP"):
                with pytest.raises(ValueError):
                    corc.ks_egm_solve(*args, tol=0.0, max_iter=6, jacobi=jacobi)
            else:
                assert corc.ks_egm_solve(*args, tol=0.0, max_iter=6, jacobi=jacobi)["iters"] == 6
    c = [x for x in kc.egm_cases() if x["name"] == "nk3"][0]
    with pytest.raises(ValueError):
        no.ks_egm_sweep(c["p"], c["k_grid"], c["K_grid"], c["B"], c["P"], c["k0"].copy())


# ------------------------------------------------------------------------------ C vs numpy
def _eq(a, b, nan):
    return np.array_equal(a, b, equal_nan=nan)


SMALL = [(nk, nK, f) for nk, nK in kc.VFI_SIZES if nk <= 64 for f in kc.VFI_FAMILIES]


@pytest.mark.parametrize("nk,nK,family", SMALL)
def test_c_oracle_equals_numpy_vfi(nk, nK, family):
    """Improvement (k_opt and nfev) and 2 Howard sweeps from an adversarial policy."""
    i = [s[:2] for s in kc.VFI_SIZES].index((nk, nK))
    j = kc.VFI_FAMILIES.index(family)
    c = kc.vfi_case(nk, nK, family, (i + j) % len(kc.VARIANTS), 1000 + 17 * i + j)
    nan = bool(np.isnan(c["V"]).any())
    args = (c["k_grid"], c["K_grid"], c["V"])
    with np.errstate(all="ignore"):
        kn, nn = no.ks_policy_improve(c["p"], *args, c["B"], c["P"])
    kC, nC = corc.ks_policy_improve(kc.cparams(c["p"]), *args, c["B"], c["P"])
    assert _eq(kn, kC, nan) and np.array_equal(nn, nC)
    ko = kc.howard_kopt(c, 5)
    with np.errstate(all="ignore"):
        Vn = no.ks_howard(c["p"], *args, ko, c["B"], c["P"], 2)
    VC = corc.ks_howard(kc.cparams(c["p"]), *args, ko, c["B"], c["P"], 2)
    assert _eq(Vn, VC, nan)


@pytest.mark.parametrize("name", [c["name"] for c in kc.egm_cases()
                                  if c["name"] not in ("nk3", "nanP")])
@pytest.mark.parametrize("jacobi", [False, True])
def test_c_oracle_equals_numpy_egm(name, jacobi):
    c = [x for x in kc.egm_cases() if x["name"] == name][0]
    with np.errstate(all="ignore"):
        Rn = no.ks_egm_solve(c["p"], c["k_grid"], c["K_grid"], c["B"], c["P"], c["k0"], tol=0.0,
                             max_iter=2, jacobi=jacobi)
    RC = corc.ks_egm_solve(kc.cparams(c["p"]), c["k_grid"], c["K_grid"], c["B"], c["P"], c["k0"],
                           tol=0.0, max_iter=2, jacobi=jacobi)
    assert Rn["iters"] == RC["iters"] == 2
    assert _eq(Rn["k_opt"], RC["k_opt"], True)
    assert Rn["diff"] == RC["diff"]
