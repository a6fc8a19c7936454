"""Inputs shared by the batched Krusell-Smith EGM tests (tests/test_ks_egm_batch_cpu.py and the
GPU files test_ks_egm_batch_gpu.py, test_ks_hist_multi_gpu.py, test_ks_egm_driver_gpu.py): three
economies on one k_grid, and their ALM rounds composed from the C oracle (corc.ks_egm_solve) and
the numpy restatement of the histogram simulation (tests/ks_hist_ref.py).  A plain module; `pkg`
is the host package (its calibration and regression helpers are plain numpy)."""
import numpy as np

from oracle import corc
from tests import ks_hist_ref as ref

# E0 the reference economy, E1 more impatient with faster depreciation on a lower K_grid, E2
# higher unemployment rates (its own P, l_bar and employment transitions)
ECONOMIES = (dict(),
             dict(beta=0.98, delta=0.03, K_min=15.0, K_max=35.0),
             dict(ug=0.05, ub=0.12))
K_SIZE, KK_SIZE, T, T_DISCARD, NX, N_PATHS, MAX_EGM, ROUNDS = 24, 3, 40, 10, 64, 2, 400, 3
B_IDENTITY = (0.0, 1.0, 0.0, 1.0)
B_OTHER = (0.1, 0.97, 0.08, 0.975)

_cache = {}


def economy(pkg, eco, k_size=K_SIZE, K_size=KK_SIZE):
    """(params, k_grid, K_grid, P) of one economy dict."""
    eco = dict(eco)
    K_min, K_max = eco.pop("K_min", 30.0), eco.pop("K_max", 50.0)
    p = pkg.ks_params(**eco)
    kg, Kg, P, _ = pkg.calibration.krusell_smith(k_size=k_size, K_size=K_size, K_min=K_min,
                                                 K_max=K_max, beta=p[0], k_min=p[3], k_max=p[4],
                                                 ug=p[5], ub=p[6])
    return p, kg, Kg, P


def inputs(pkg, k_size=K_SIZE, K_size=KK_SIZE):
    """dict(prm (3, 13), k_grid, K_grid (3, nK), P (3, 4, 4), k0 (nk, nK, 4), zi (T, 2), x)."""
    key = ("inputs", k_size, K_size)
    if key not in _cache:
        es = [economy(pkg, e, k_size, K_size) for e in ECONOMIES]
        kg = es[0][1]
        kp = pkg.ks_panel
        _cache[key] = dict(
            prm=np.stack([e[0] for e in es]), k_grid=kg, K_grid=np.stack([e[2] for e in es]),
            P=np.stack([e[3] for e in es]),
            k0=0.9 * np.repeat(np.repeat(kg[:, None, None], K_size, 1), 4, 2),
            zi=kp.zi_paths(T, N_PATHS, kp.matlab_rand(N_PATHS * (T - 1)), es[0][0]),
            x=kp.hist_grid(NX, float(es[0][0][3]), float(es[0][0][4])))
    return _cache[key]


def cparams(prm):
    return corc.ks_params(beta=prm[0], alpha=prm[1], delta=prm[2], k_min=prm[3], k_max=prm[4],
                          ug=prm[5], ub=prm[6], l_bar=prm[7], mu=prm[8], z_grid=(prm[9], prm[10]),
                          eps_grid=(prm[11], prm[12]))


def nan_row_P(P):
    """tests/ks_cases.egm_cases' `nanP`: P(4, :) = NaN, so the s = 4 pairs have no valid point."""
    Pn = np.array(P, dtype=np.float64, copy=True)
    Pn[3, :] = np.nan
    return Pn


def oracle_solve(I, e, k_opt, B, tol=1e-6, max_iter=MAX_EGM):
    return corc.ks_egm_solve(cparams(I["prm"][e]), I["k_grid"], I["K_grid"][e], np.asarray(B),
                             I["P"][e], k_opt, tol=tol, max_iter=max_iter)


def oracle_rounds(pkg, carry, rounds=ROUNDS, tol_B=1e-6, update_B=0.3):
    """The histogram ALM loop of every economy from the oracles.  carry: the capital marginal of
    the last distribution starts the next round (the drivers' rule), else every round restarts
    at hist_start.  Per economy: dict(iters, slow (rounds, 2), K_ts, k_opt, lam (per round),
    B_history, B)."""
    key = ("rounds", carry, rounds, tol_B, update_B)
    if key in _cache:
        return _cache[key]
    I, kp = inputs(pkg), pkg.ks_panel
    out = []
    for e in range(len(ECONOMIES)):
        prm, Kg = I["prm"][e], I["K_grid"][e]
        lam0 = kp.hist_start(I["x"], Kg[0], prm[5])
        lam, k_opt, B = lam0, I["k0"], np.array(B_IDENTITY)
        r = dict(iters=[], slow=[], K_ts=[], k_opt=[], lam=[], B_history=[])
        for _ in range(rounds):
            S = oracle_solve(I, e, k_opt, B)
            k_opt = S["k_opt"]
            K_ts, lam_T, slow = ref.simulate(k_opt, I["k_grid"], Kg, I["x"], prm, I["zi"], lam)
            lam = kp.hist_carry(lam_T, prm[5]) if carry else lam0
            B_new, _, _ = kp.alm_regress_paths(K_ts, I["zi"], T_DISCARD)
            r["iters"].append(S["iters"])
            r["slow"].append(slow)
            r["K_ts"].append(K_ts)
            r["k_opt"].append(k_opt)
            r["lam"].append(lam_T)
            r["B_history"].append(B_new)
            if float(np.max(np.abs(B_new - B))) < tol_B:
                break
            B = update_B * B_new + (1 - update_B) * B
        r["B"] = B
        out.append(r)
    _cache[key] = out
    return out


def sweeps3(pkg):
    """The three economies' policies after three oracle sweeps from 0.9 k_grid at the identity
    ALM: (3, nk, nK, 4)."""
    if "sweeps3" not in _cache:
        I = inputs(pkg)
        _cache["sweeps3"] = np.stack([oracle_solve(I, e, I["k0"], B_IDENTITY, tol=0.0,
                                                   max_iter=3)["k_opt"] for e in range(3)])
    return _cache["sweeps3"]
