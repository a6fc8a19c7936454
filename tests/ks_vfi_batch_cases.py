"""Inputs shared by the batched Krusell-Smith VFI tests (tests/test_ks_vfi_batch_cpu.py and the
GPU files test_ks_vfi_batch_gpu.py, test_ks_vfi_driver_gpu.py): the three economies of
tests/ks_egm_batch_cases.py with the VFI script's start (V0 from calibration.krusell_smith,
k0 = 0.9 k), the C oracle's solves (corc.ks_vfi_solve, cached: a reference is computed once and
shared) and the ALM rounds composed from the oracles.  A plain module; `pkg` is the host package."""
import numpy as np

from oracle import corc
from tests import ks_egm_batch_cases as bc
from tests import ks_hist_ref as ref

ECONOMIES = bc.ECONOMIES
K_SIZE, KK_SIZE = bc.K_SIZE, bc.KK_SIZE
T, T_DISCARD, NX, N_PATHS = bc.T, bc.T_DISCARD, bc.NX, bc.N_PATHS
B_IDENTITY = bc.B_IDENTITY
# moves the forecast index in both aggregate states on K in [30, 50] and [15, 35]
# (ks_egm_batch_cases.B_OTHER moves none on these grids)
B_SHIFT = (0.0, 1.08, 0.9, 0.7)

_cache = {}


def inputs(pkg, k_size=K_SIZE, K_size=KK_SIZE):
    """ks_egm_batch_cases.inputs plus V0 (3, nk, nK, 4), each economy's own VFI start."""
    key = ("inputs", k_size, K_size)
    if key not in _cache:
        I = dict(bc.inputs(pkg, k_size, K_size))
        V0 = []
        for e, eco in enumerate(ECONOMIES):
            eco = dict(eco)
            K_min, K_max = eco.pop("K_min", 30.0), eco.pop("K_max", 50.0)
            p = I["prm"][e]
            V0.append(pkg.calibration.krusell_smith(k_size=k_size, K_size=K_size, K_min=K_min,
                                                    K_max=K_max, beta=p[0], k_min=p[3],
                                                    k_max=p[4], ug=p[5], ub=p[6])[3])
        I["V0"] = np.stack(V0)
        _cache[key] = I
    return _cache[key]


def forecast_index(K_grid, B):
    """The nearest-index rule of Krusell_Smith_VFI.m:335-343 restated in numpy: per aggregate
    state (good, bad) and K_i the index of the K_grid point nearest the ALM forecast (first on
    ties).  Returns (2, nK) integers."""
    Kg = np.asarray(K_grid, np.float64)
    out = np.zeros((2, Kg.size), np.int64)
    for z in (0, 1):
        Kp = np.exp(B[2 * z] + B[2 * z + 1] * np.log(np.maximum(Kg, 1e-8)))
        Kp = np.maximum(np.minimum(Kp, Kg[-1]), Kg[0])
        out[z] = np.argmin(np.abs(Kg[None, :] - Kp[:, None]), axis=1)
    return out


def oracle_solve(I, e, V, k_opt, B, howard=50, tol=1e-6, max_vfi=200, key=None):
    """corc.ks_vfi_solve of economy e; cached under `key` (hashable) when given."""
    if key is not None and ("solve", key) in _cache:
        return _cache[("solve", key)]
    R = corc.ks_vfi_solve(bc.cparams(I["prm"][e]), I["k_grid"], I["K_grid"][e], V, k_opt,
                          np.asarray(B, np.float64), I["P"][e], howard=howard, tol=tol,
                          max_vfi=max_vfi)
    if key is not None:
        _cache[("solve", key)] = R
    return R


def oracle_cold(pkg, e, B, howard=50, tol=1e-6, max_vfi=200, k_size=K_SIZE, K_size=KK_SIZE):
    """The oracle's solve of economy e from the script's start (V0, 0.9 k); cached."""
    I = inputs(pkg, k_size, K_size)
    return oracle_solve(I, e, I["V0"][e], I["k0"], B, howard, tol, max_vfi,
                        key=("cold", e, tuple(B), howard, tol, max_vfi, k_size, K_size))


def oracle_rounds(pkg, k_size, K_size, rounds, update_B, tol_B=1e-6, howard=50, tol=1e-6,
                  max_vfi=10000):
    """The histogram ALM loop of every economy composed from the oracles (corc.ks_vfi_solve warm
    from the previous round, ks_hist_ref.simulate with the carried capital marginal,
    alm_regress_paths).  Per economy: dict(iters, K_ts, slow, B_history, diff_B, B, value,
    k_opt); an economy stops at diff_B < tol_B as the drivers do."""
    key = ("rounds", k_size, K_size, rounds, update_B, tol_B, howard, tol, max_vfi)
    if key in _cache:
        return _cache[key]
    I, kp = inputs(pkg, k_size, K_size), pkg.ks_panel
    out = []
    for e in range(len(ECONOMIES)):
        prm, Kg = I["prm"][e], I["K_grid"][e]
        lam = kp.hist_start(I["x"], Kg[0], prm[5])
        V, k_opt, B = I["V0"][e], I["k0"], np.array(B_IDENTITY)
        r = dict(iters=[], K_ts=[], slow=[], B_history=[], diff_B=[])
        for _ in range(rounds):
            S = oracle_solve(I, e, V, k_opt, B, howard, tol, max_vfi)
            V, k_opt = S["value"], S["k_opt"]
            K_ts, lam_T, slow = ref.simulate(k_opt, I["k_grid"], Kg, I["x"], prm, I["zi"], lam)
            lam = kp.hist_carry(lam_T, prm[5])
            B_new, _, _ = kp.alm_regress_paths(K_ts, I["zi"], T_DISCARD)
            d = float(np.max(np.abs(B_new - B)))
            r["iters"].append(S["iters"])
            r["K_ts"].append(K_ts)
            r["slow"].append(slow)
            r["B_history"].append(B_new)
            r["diff_B"].append(d)
            if d < tol_B:
                break
            B = update_B * B_new + (1 - update_B) * B
        r.update(B=B, value=V, k_opt=k_opt)
        out.append(r)
    _cache[key] = out
    return out
