"""Second moments and the Gaussian likelihood of the aggregates from the sequence-space Jacobian
(Auclert, Bardóczy, Rognlie, Straub 2021, §5), many candidate shock processes per launch.

The linearised economy maps a TFP path dZ to the paths of the observables through the
general-equilibrium Jacobians G (ge_jacobians, host numpy: they do not depend on the shock
process).  A candidate process c with MA coefficients dZ[c] then has the observables' MA
coefficients m[c] = G·dZ[c] (ma_batch: one launch on the fp64 matrix cores), autocovariances
Γ[c] and a Gaussian log-likelihood of an observed panel (loglik_batch: one workgroup per
candidate) — include/aiyagari_hip.h, "Second moments and the Gaussian likelihood".  A candidate's
bits do not depend on its batch.

Timing: row t of every Jacobian is date t, t = 0 … T−1; column s is the date of the shock.  K_t
is the capital in place at date t (chosen at t − 1), so K's row 0 is zero."""
from __future__ import annotations

import numpy as np

from ._capi import check, i64, ip, lib, ptr
from .transition import (_f, _labor_newton_matrix, _labor_response, _newton_matrix,
                         _price_slopes, _ratio_slopes, jacobian_batch)

OUTPUTS = ("K", "Y", "C", "r", "w")
OUTPUTS_LABOR = ("K", "Y", "C", "r", "w", "H")


def _pick(G, outputs):
    bad = [o for o in outputs if o not in G]
    if bad:
        raise ValueError(f"unknown outputs {bad}: choose from {sorted(G)}")
    return np.stack([G[o] for o in outputs])


def ge_jacobians(ss, jac, outputs=OUTPUTS):
    """G [n_o][T][T], G[o][t][s] = ∂X_{o,t}/∂Z_s in levels, of the exogenous-labour economy around
    the steady state ss (steady_state's dict), jac = jacobian(ss, T)'s dict.

    K: row t is K_t, the capital in place at date t.  Row 0 is zero (K_0 is given); rows 1 … T−1
       are rows 0 … T−2 of X, the ONE multi-right-hand-side solve (I − M)·X = J_r·r_Z + J_w·w_Z
       (impulse_response's system, all T unit shocks at once), whose row t is K_{t+1}.
    r, w: prices_from_K's slopes, dr_t = r_K·dK_t + r_Z·dZ_t and dw_t likewise.
    Y: Y_t = Y_ss·Z_t·(K_t/K_ss)^α anchored as prices_from_K anchors prices, Y_ss = (r_ss + δ)·
       K_ss/α, so dY_t = Y_ss·dZ_t + (r_ss + δ)·dK_t.
    C: the resource constraint C_t = Y_t − K_{t+1} + (1 − δ)·K_t; X's last row supplies K_T."""
    J_r, J_w = _f(jac["J_r"]), _f(jac["J_w"])
    T = J_r.shape[0]
    r_K, w_K, r_Z, w_Z = _price_slopes(ss)
    alpha, delta = ss["cal"]["alpha"], ss["cal"]["delta"]
    X = np.linalg.solve(-_newton_matrix(ss, jac), J_r * r_Z + J_w * w_Z)
    I = np.eye(T)
    G = {"K": np.zeros((T, T))}
    G["K"][1:] = X[:-1]
    G["r"] = r_K * G["K"] + r_Z * I
    G["w"] = w_K * G["K"] + w_Z * I
    Y_ss = (ss["r"] + delta) * ss["K"] / alpha
    G["Y"] = Y_ss * I + (ss["r"] + delta) * G["K"]
    G["C"] = G["Y"] - X + (1 - delta) * G["K"]
    return _pick(G, outputs)


def ge_jacobians_labor(ss, jac, outputs=OUTPUTS_LABOR):
    """ge_jacobians for the endogenous-labour economy (ss: steady_state_labor's dict, jac:
    jacobian_labor's).  The unknown is κ_t = K_t/H_t, t = 0 … T−1: ONE solve (I − M)·dκ = N_Z
    (impulse_response_labor's system, all T unit shocks at once), then dr = r_κ·dκ + r_Z·I, dw
    likewise, X = J_Kr·dr + J_Kw·dw (row t is K_{t+1}) and H = J_Hr·dr + J_Hw·dw (row t is H_t:
    hours move on impact).  K's row t is K_t (row 0 zero, rows 1 … from X), Y_t = Y_ss·Z_t·
    (K_t/K_ss)^α·(H_t/H_ss)^(1−α) with Y_ss = (r_ss + δ)·K_ss/α, C_t = Y_t − K_{t+1} + (1 − δ)·K_t."""
    r_k, w_k, r_Z, w_Z = _ratio_slopes(ss)
    alpha, delta = ss["cal"]["alpha"], ss["cal"]["delta"]
    dk = np.linalg.solve(-_labor_newton_matrix(ss, jac), _labor_response(ss, jac, r_Z, w_Z))
    T = dk.shape[0]
    I = np.eye(T)
    G = {"r": r_k * dk + r_Z * I, "w": w_k * dk + w_Z * I}
    X = _f(jac["J_Kr"]) @ G["r"] + _f(jac["J_Kw"]) @ G["w"]
    G["H"] = _f(jac["J_Hr"]) @ G["r"] + _f(jac["J_Hw"]) @ G["w"]
    G["K"] = np.zeros((T, T))
    G["K"][1:] = X[:-1]
    Y_ss = (ss["r"] + delta) * ss["K"] / alpha
    G["Y"] = Y_ss * I + (ss["r"] + delta) * G["K"] + (Y_ss * (1 - alpha) / ss["H"]) * G["H"]
    G["C"] = G["Y"] - X + (1 - delta) * G["K"]
    return _pick(G, outputs)


def ar1_ma(rho, sigma, T):
    """dZ [C][T], the MA coefficients of C AR(1) processes: dZ[c][0] = σ_c and dZ[c][s] =
    dZ[c][s−1]·ρ_c — a running product, so an element's bits do not depend on the batch."""
    rho, sigma = np.atleast_1d(_f(rho)), np.atleast_1d(_f(sigma))
    if rho.ndim != 1 or rho.shape != sigma.shape or T < 1:
        raise ValueError("rho and sigma must be [C] and T >= 1")
    dZ = np.empty((rho.size, T))
    dZ[:, 0] = sigma
    for s in range(1, T):
        dZ[:, s] = dZ[:, s - 1] * rho
    return dZ


def _G3(G):
    G = _f(G)
    if G.ndim == 2:
        G = G[None]
    if G.ndim != 3 or G.shape[1] != G.shape[2]:
        raise ValueError("G must be [n_o][T][T]")
    return G


def ma_batch(G, dZ):
    """aiy_ssj_ma_batch: G [n_o][T][T], dZ [C][T] -> m [C][n_o][T], m[c][o][t] = Σ_s G[o][t][s]·
    dZ[c][s]."""
    G, dZ = _G3(G), np.atleast_2d(_f(dZ))
    n_o, T = G.shape[0], G.shape[1]
    if dZ.ndim != 2 or dZ.shape[1] != T:
        raise ValueError("dZ must be [C][T] with G's T")
    m = np.empty((dZ.shape[0], n_o, T))
    check(lib().aiy_ssj_ma_batch(i64(n_o), i64(T), i64(dZ.shape[0]), ptr(G), ptr(dZ), ptr(m)))
    return m


def ma_batch_dev(G, dZ, m, stream=None):
    """aiy_ssj_ma_batch_dev (torch tensors): G [n_o][T][T], dZ [C][T], m [C][n_o][T] (out).
    Enqueues only."""
    from ._capi import stream_handle
    check(lib().aiy_ssj_ma_batch_dev(i64(G.shape[0]), i64(G.shape[1]), i64(dZ.shape[0]), ptr(G),
                                     ptr(dZ), ptr(m), stream_handle(stream)))


def _m3(m):
    m = _f(m)
    if m.ndim == 2:
        m = m[None]
    if m.ndim != 3:
        raise ValueError("m must be [C][n_o][T]")
    return m


def loglik_batch(m, y, me_var, want_gamma=False, want_d=False):
    """aiy_ssj_loglik_batch: m [C][n_o][T], y [L][n_o] (the observed deviations from the steady
    state, shared by the candidates), me_var [n_o] (shared) or [C][n_o], >= 0.  Returns
    dict(loglik [C], status [C], fail [C][, Gamma [C][L][n_o][n_o]][, d [C][L·n_o]]); status 1:
    pivot `fail` of the covariance's LDLᵀ was not positive (loglik NaN) — that candidate only."""
    m = _m3(m)
    n_c, n_o, T = m.shape
    y = _f(y)
    if y.ndim == 1:
        y = y[:, None]
    if y.ndim != 2 or y.shape[1] != n_o:
        raise ValueError("y must be [L][n_o]")
    L = y.shape[0]
    me = _f(me_var)
    if me.shape == (n_o,):
        shared = 1
    elif me.shape == (n_c, n_o):
        shared = 0
    else:
        raise ValueError("me_var must be [n_o] or [C][n_o]")
    ll = np.empty(n_c)
    st, fl = np.zeros(n_c, np.int32), np.zeros(n_c, np.int32)
    Gam = np.empty((n_c, L, n_o, n_o)) if want_gamma else None
    dd = np.empty((n_c, L * n_o)) if want_d else None
    check(lib().aiy_ssj_loglik_batch(i64(n_c), i64(n_o), i64(T), i64(L), ptr(m), ptr(y), ptr(me),
                                     ip(shared), ptr(ll), ptr(st), ptr(fl), ptr(Gam), ptr(dd)))
    out = dict(loglik=ll, status=st, fail=fl)
    if want_gamma:
        out["Gamma"] = Gam
    if want_d:
        out["d"] = dd
    return out


def loglik_batch_dev(m, y, me_var, loglik, status, fail, Gamma=None, d=None, stream=None):
    """aiy_ssj_loglik_batch_dev (torch tensors): m [C][n_o][T], y [L][n_o] or None, me_var [n_o] or
    [C][n_o]; loglik (float64), status, fail (int32) [C], Gamma [C][L][n_o][n_o] and d [C][L·n_o]
    (optional) are written.  With y None, Gamma [C][L][n_o][n_o] fixes L.  Enqueues only."""
    from ._capi import stream_handle
    L = int(y.shape[0]) if y is not None else int(Gamma.shape[1])
    shared = 1 if me_var is None or me_var.dim() == 1 else 0
    check(lib().aiy_ssj_loglik_batch_dev(i64(m.shape[0]), i64(m.shape[1]), i64(m.shape[2]), i64(L),
                                         ptr(m), ptr(y), ptr(me_var), ip(shared), ptr(loglik),
                                         ptr(status), ptr(fail), ptr(Gamma), ptr(d),
                                         stream_handle(stream)))


def autocovariance_batch(m, L):
    """The second-moment path of aiy_ssj_loglik_batch (y NULL): Γ [C][L][n_o][n_o], Γ[c][l][o][p] =
    Σ_u m[c][o][u+l]·m[c][p][u] = cov(X_{o,t+l}, X_{p,t}) under unit-variance innovations."""
    m = _m3(m)
    n_c, n_o, T = m.shape
    Gam = np.empty((n_c, max(int(L), 0), n_o, n_o))
    check(lib().aiy_ssj_loglik_batch(i64(n_c), i64(n_o), i64(T), i64(L), ptr(m), None, None, ip(1),
                                     None, None, None, ptr(Gam), None))
    return Gam


def dense_solve_batch(A, B, chunk=0):
    """aiy_dense_solve_batch: A [C][n][n], B [C][n][R] (or [C][n]: R = 1) -> dict(X (B's shape),
    status [C], fail [C]).  Gaussian elimination with partial pivoting, one workgroup per system,
    in the header's operation order; status 1: column `fail` had no finite non-zero pivot (X NaN)
    — that system only.  chunk: systems staged at a time (0: the 4 GiB default)."""
    A, B = _f(A), _f(B)
    if A.ndim == 2:
        A, B = A[None], B[None]
    vec = B.ndim == 2
    B3 = B[:, :, None] if vec else B
    if A.ndim != 3 or A.shape[1] != A.shape[2] or B3.ndim != 3 or B3.shape[:2] != A.shape[:2]:
        raise ValueError("A must be [C][n][n] and B [C][n][R] or [C][n]")
    B3 = np.ascontiguousarray(B3)
    n_c, n, R = B3.shape
    X = np.empty((n_c, n, R))
    st, fl = np.zeros(n_c, np.int32), np.zeros(n_c, np.int32)
    check(lib().aiy_dense_solve_batch(i64(n_c), i64(n), i64(R), ptr(A), ptr(B3), ptr(X), ptr(st),
                                      ptr(fl), i64(chunk)))
    return dict(X=X[:, :, 0] if vec else X, status=st, fail=fl)


def dense_solve_batch_dev(A, B, X, work, status, fail, stream=None):
    """aiy_dense_solve_batch_dev (torch tensors): A [C][n][n], B [C][n][R], X [C][n][R] (out), work
    [C][n][n+R] (float64 scratch), status, fail (int32) [C].  Enqueues only."""
    from ._capi import stream_handle
    check(lib().aiy_dense_solve_batch_dev(i64(A.shape[0]), i64(A.shape[1]), i64(B.shape[2]),
                                          ptr(A), ptr(B), ptr(X), ptr(work), ptr(status),
                                          ptr(fail), stream_handle(stream)))


def _ge_system(ss, J_r, J_w, dZ):
    """Economy's GE system for one shock path dZ [T]: (I − M, b) with M of _newton_matrix and
    b = J_r·(r_Z·dZ) + J_w·(w_Z·dZ)."""
    _, _, r_Z, w_Z = _price_slopes(ss)
    A = -_newton_matrix(ss, dict(J_r=J_r, J_w=J_w))
    return A, J_r @ (r_Z * dZ) + J_w @ (w_Z * dZ)


def _ge_outputs(ss, x, dZ, outputs):
    """ge_jacobians' formulas on the vector x (row t is K_{t+1}) rather than on the matrix X."""
    r_K, w_K, r_Z, w_Z = _price_slopes(ss)
    alpha, delta = ss["cal"]["alpha"], ss["cal"]["delta"]
    G = {"K": np.zeros_like(x)}
    G["K"][1:] = x[:-1]
    G["r"] = r_K * G["K"] + r_Z * dZ
    G["w"] = w_K * G["K"] + w_Z * dZ
    Y_ss = (ss["r"] + delta) * ss["K"] / alpha
    G["Y"] = Y_ss * dZ + (ss["r"] + delta) * G["K"]
    G["C"] = G["Y"] - x + (1 - delta) * G["K"]
    return _pick(G, outputs)


def ge_ma_batch(ss_list, jac_batch, dZ, outputs=OUTPUTS, solve=None, chunk=0):
    """m [C][n_o][T], the observables' MA coefficients of C economies, economy c under its own
    shock path dZ[c] [T]: m[c] = ge_jacobians(ss_c, jac_c, outputs) @ dZ[c] without forming G —
    one right-hand side per economy instead of T.  The host forms b_c = J_r[c]·(r_Z·dZ_c) +
    J_w[c]·(w_Z·dZ_c) and I − M_c (_newton_matrix); ONE dense_solve_batch call with R = 1 gives
    x_c, whose row t is K_{t+1}; K, r, w, Y and C follow by ge_jacobians' formulas.  jac_batch:
    jacobian_batch's dict (J_r, J_w [C][T][T]).  An economy whose solve stops (status 1) has NaN
    rows.  solve: dense_solve_batch's signature (the tests' CPU reference)."""
    ss_list = list(ss_list)
    J_r, J_w, dZ = _f(jac_batch["J_r"]), _f(jac_batch["J_w"]), np.atleast_2d(_f(dZ))
    n_c = len(ss_list)
    if J_r.ndim != 3 or J_r.shape != J_w.shape or J_r.shape[0] != n_c or \
            dZ.shape != (n_c, J_r.shape[1]):
        raise ValueError("jac_batch must hold J_r, J_w [C][T][T] and dZ must be [C][T]")
    sys_ = [_ge_system(ss_list[c], J_r[c], J_w[c], dZ[c]) for c in range(n_c)]
    A, b = np.stack([q[0] for q in sys_]), np.stack([q[1] for q in sys_])
    out = (solve or dense_solve_batch)(A, b, chunk=chunk)
    m = np.stack([_ge_outputs(ss_list[c], out["X"][c], dZ[c], outputs) for c in range(n_c)])
    m[out["status"] != 0] = np.nan  # (K_0 = 0 and the impact terms would survive a NaN x)
    return m


def structural_loglik(ss_list, y, rho, sigma_e, me_var, T, outputs=("Y", "C", "K"), h=1e-4,
                      split_ms=None):
    """The log-likelihoods of C structural candidates, candidate c = (the economy ss_list[c], the
    AR(1) shock (rho[c], sigma_e[c])), against one observed panel y [L][n_o]: jacobian_batch,
    ar1_ma, ge_ma_batch and loglik_batch chained — four launches' worth of device work for the
    whole batch.  Returns dict(loglik, status, fail [C], jac_status [C][2]); a candidate's bits do
    not depend on the batch.  split_ms: an optional float64 [4] array that receives the host
    clock's split in ms: Jacobians, host assembly, solve, likelihood."""
    import time
    ss_list = list(ss_list)
    t0 = time.perf_counter()
    jac = jacobian_batch(ss_list, T, h, want_F=False, want_E=False)
    t1 = time.perf_counter()
    dZ = ar1_ma(rho, sigma_e, T)
    took = {}

    def timed_solve(A, b, chunk=0):
        ts = time.perf_counter()
        out = dense_solve_batch(A, b, chunk=chunk)
        took["solve"] = time.perf_counter() - ts
        return out

    m = ge_ma_batch(ss_list, jac, dZ, outputs, solve=timed_solve)
    t2 = time.perf_counter()
    out = loglik_batch(m, y, me_var)
    t3 = time.perf_counter()
    if split_ms is not None:
        split_ms[:] = [1e3 * (t1 - t0), 1e3 * (t2 - t1 - took["solve"]), 1e3 * took["solve"],
                       1e3 * (t3 - t2)]
    out["jac_status"] = jac["status"]
    return out


def moments(Gamma, lags=(0, 1)):
    """Business-cycle moments of autocovariances Γ [...][L][n_o][n_o] (host code): dict(sd
    [...][n_o], the standard deviations, and corr [...][len(lags)][n_o][n_o], corr[l][o][p] =
    corr(X_{o,t+l}, X_{p,t}) at the given lags)."""
    Gamma = _f(Gamma)
    sd = np.sqrt(np.diagonal(Gamma[..., 0, :, :], axis1=-2, axis2=-1))
    corr = Gamma[..., list(lags), :, :] / (sd[..., None, :, None] * sd[..., None, None, :])
    return dict(sd=sd, corr=corr)


def ar1_loglik(G, y, rho, sigma, me_var, backend=None):
    """The log-likelihoods of C AR(1) parameter pairs (rho [C], sigma [C]) in two launches:
    dZ = ar1_ma(rho, sigma, T), m = ma(G, dZ), lik(m, y, me_var) -> dict(loglik, status, fail).
    backend: the pair (ma, lik) with ma_batch's and loglik_batch's signatures — the GPU's by
    default, the CPU reference's in the tests."""
    ma, lik = (ma_batch, loglik_batch) if backend is None else backend
    G = _G3(G)
    return lik(ma(G, ar1_ma(rho, sigma, G.shape[1])), y, me_var)


def ar1_mle(G, y, me_var, rho_bounds, sigma_bounds, width=16, rounds=6, backend=None):
    """The AR(1) parameters that maximise the likelihood, by a lockstep zooming grid.  A round
    lays width equally spaced values (end points included) over each side of the box, evaluates
    the width × width pairs — candidate q = i·width + k is (rho_i, sigma_k) — in ONE ar1_loglik
    call, takes the argmax over the candidates with status 0 (ties: the lowest q) and shrinks the
    box to one grid step either side of it, clipped to the box it came from: each side by
    2/(width − 1) a round.  A round without a status-0 candidate ends the search.
    Returns dict(rho, sigma, loglik (the best candidate met; NaN when there was none), boxes (the
    path of boxes ((rho_lo, rho_hi), (sigma_lo, sigma_hi)), the first included), evals [rounds
    run], best [rounds run] (each round's argmax q, −1: none))."""
    if width < 3 or rounds < 1:
        raise ValueError("need width >= 3 and rounds >= 1")
    box = (tuple(map(float, rho_bounds)), tuple(map(float, sigma_bounds)))
    boxes, evals, picks = [box], [], []
    best = (np.nan, np.nan, np.nan)
    for _ in range(rounds):
        rr = np.linspace(box[0][0], box[0][1], width)
        sg = np.linspace(box[1][0], box[1][1], width)
        R = ar1_loglik(G, y, np.repeat(rr, width), np.tile(sg, width), me_var, backend)
        evals.append(width * width)
        ll = np.where((R["status"] == 0) & ~np.isnan(R["loglik"]), R["loglik"], -np.inf)
        q = int(np.argmax(ll))
        if ll[q] == -np.inf:
            picks.append(-1)
            break
        picks.append(q)
        i, k = divmod(q, width)
        if not ll[q] < best[2]:
            best = (float(rr[i]), float(sg[k]), float(ll[q]))
        hr, hs = rr[1] - rr[0], sg[1] - sg[0]
        box = ((max(box[0][0], rr[i] - hr), min(box[0][1], rr[i] + hr)),
               (max(box[1][0], sg[k] - hs), min(box[1][1], sg[k] + hs)))
        boxes.append(box)
    return dict(rho=best[0], sigma=best[1], loglik=best[2], boxes=boxes,
                evals=np.array(evals), best=np.array(picks))
