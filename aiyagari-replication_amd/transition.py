"""Perfect-foresight transition paths of the Aiyagari EGM economy (MIT shocks) on the GPU.

A transition is two passes over T periods.  The backward pass takes a price path (r_t, w_t) and
iterates the two-rate EGM step back from the terminal steady-state policy; the forward pass
pushes the initial distribution through the period policies and yields the capital path K_t.
C paths run per call, one workgroup per path and pass (include/aiyagari_hip.h, "Transition
paths").  Arrays are [N][Na] rows per (path, period), C-contiguous: policy_k [C][T][N][Na]."""
from __future__ import annotations

import ctypes
import math

import numpy as np

from ._capi import check, d, i64, ip, lib, ptr


def _f(x):
    return np.ascontiguousarray(x, np.float64)


def _paths(r, w):
    r, w = np.atleast_2d(_f(r)), np.atleast_2d(_f(w))
    if r.ndim != 2 or w.ndim != 2 or r.shape != (w.shape[0], w.shape[1] + 1):
        raise ValueError("r must be [C][T+1] and w [C][T]")
    return r, w, w.shape[0], w.shape[1]


def _start(x, n_c, N, Na, name):
    """A start array shared by all paths ([N][Na]) or one per path ([C][N][Na]) -> (array, flag)."""
    x = _f(x)
    if x.shape == (N, Na):
        return x, 1
    if x.shape == (n_c, N, Na):
        return x, 0
    raise ValueError(f"{name} must be [N][Na] = {(N, Na)} or [C][N][Na]")


def egm_backward_batch(r, w, pc_T, a_grid, s, P, beta, sigma, amin, want_pc=True):
    """aiy_egm_backward_batch: r [C][T+1] (r[c][T]: the terminal rate), w [C][T], pc_T [N][Na]
    (shared) or [C][N][Na].  Returns dict(policy_k, policy_c [C][T][N][Na] (None unless want_pc),
    status [C], fail_t [C]); status 1: the endogenous grid of period fail_t was not increasing
    (that path's periods <= fail_t are undefined, the other paths are unaffected)."""
    r, w, n_c, T = _paths(r, w)
    a, s, P = _f(a_grid), _f(s), np.asfortranarray(P, dtype=np.float64)
    N, Na = s.size, a.size
    pcT, shared = _start(pc_T, n_c, N, Na, "pc_T")
    pk = np.empty((n_c, T, N, Na))
    pc = np.empty((n_c, T, N, Na)) if want_pc else None
    st, ft = np.zeros(n_c, np.int32), np.zeros(n_c, np.int32)
    check(lib().aiy_egm_backward_batch(i64(n_c), i64(T), ptr(r), ptr(w), ptr(pcT), ip(shared),
                                       ptr(a), ptr(s), ptr(P), i64(N), i64(Na), d(beta), d(sigma),
                                       d(amin), ptr(pk), ptr(pc), ptr(st), ptr(ft)))
    return dict(policy_k=pk, policy_c=pc, status=st, fail_t=ft)


def dist_forward_batch(policy_k, lam0, a_grid, P, want_lam=True):
    """aiy_dist_forward_batch: policy_k [C][T][N][Na], lam0 [N][Na] (shared) or [C][N][Na].
    Returns dict(K [C][T+1], lam_T [C][N][Na] (None unless want_lam), status [C], fail_t [C]);
    status 2: the keys of policy_k[c][fail_t] are not monotone (K beyond fail_t is NaN)."""
    pk = _f(policy_k)
    if pk.ndim != 4:
        raise ValueError("policy_k must be [C][T][N][Na]")
    n_c, T, N, Na = pk.shape
    a, P = _f(a_grid), np.asfortranarray(P, dtype=np.float64)
    l0, shared = _start(lam0, n_c, N, Na, "lam0")
    K = np.empty((n_c, T + 1))
    lT = np.empty((n_c, N, Na)) if want_lam else None
    st, ft = np.zeros(n_c, np.int32), np.zeros(n_c, np.int32)
    check(lib().aiy_dist_forward_batch(i64(n_c), i64(T), ptr(pk), ptr(l0), ip(shared), ptr(a),
                                       ptr(P), i64(N), i64(Na), ptr(K), ptr(lT), ptr(st), ptr(ft)))
    return dict(K=K, lam_T=lT, status=st, fail_t=ft)


def transition_batch(r, w, pc_T, lam0, a_grid, s, P, beta, sigma, amin):
    """aiy_transition_batch: both passes on one stream, the period policies staying on the device.
    Returns (K [C][T+1], status [C], fail_t [C]); a path with status 1 has K all NaN."""
    r, w, n_c, T = _paths(r, w)
    a, s, P = _f(a_grid), _f(s), np.asfortranarray(P, dtype=np.float64)
    N, Na = s.size, a.size
    pcT, pshared = _start(pc_T, n_c, N, Na, "pc_T")
    l0, lshared = _start(lam0, n_c, N, Na, "lam0")
    K = np.empty((n_c, T + 1))
    st, ft = np.zeros(n_c, np.int32), np.zeros(n_c, np.int32)
    check(lib().aiy_transition_batch(i64(n_c), i64(T), ptr(r), ptr(w), ptr(pcT), ip(pshared),
                                     ptr(l0), ip(lshared), ptr(a), ptr(s), ptr(P), i64(N), i64(Na),
                                     d(beta), d(sigma), d(amin), ptr(K), ptr(st), ptr(ft)))
    return K, st, ft


def egm_backward_batch_dev(ws, r, w, pc_T, a_grid, s, P, beta, sigma, amin, policy_k,
                           policy_c=None, stream=None):
    """aiy_egm_backward_batch_dev (torch tensors; r [C][T+1] and w [C][T] numpy): pc_T [N][Na]
    (shared) or [C][N][Na]; policy_k, policy_c (optional): [C][T][N][Na]; P row-major.
    Returns (status [C], fail_t [C]) as numpy arrays."""
    from ._capi import stream_handle
    r, w, n_c, T = _paths(r, w)
    st, ft = np.zeros(n_c, np.int32), np.zeros(n_c, np.int32)
    check(lib().aiy_egm_backward_batch_dev(ws.handle, i64(n_c), i64(T), ptr(r), ptr(w), ptr(pc_T),
                                           ip(1 if pc_T.dim() == 2 else 0), ptr(a_grid), ptr(s),
                                           ptr(P), d(beta), d(sigma), d(amin), ptr(policy_k),
                                           ptr(policy_c), ptr(st), ptr(ft), stream_handle(stream)))
    return st, ft


def dist_forward_batch_dev(ws, policy_k, lam0, a_grid, P, K, lam_T=None, stream=None):
    """aiy_dist_forward_batch_dev (torch tensors): policy_k [C][T][N][Na], lam0 [N][Na] (shared)
    or [C][N][Na], K [C][T+1], lam_T (optional) [C][N][Na]; P row-major.
    Returns (status [C], fail_t [C]) as numpy arrays."""
    from ._capi import stream_handle
    n_c, T = int(policy_k.shape[0]), int(policy_k.shape[1])
    st, ft = np.zeros(n_c, np.int32), np.zeros(n_c, np.int32)
    check(lib().aiy_dist_forward_batch_dev(ws.handle, i64(n_c), i64(T), ptr(policy_k), ptr(lam0),
                                           ip(1 if lam0.dim() == 2 else 0), ptr(a_grid), ptr(P),
                                           ptr(K), ptr(lam_T), ptr(st), ptr(ft),
                                           stream_handle(stream)))
    return st, ft


def prices_from_K(K, Z, ss):
    """The price paths of capital paths K and TFP paths Z (same shape), anchored to the steady
    state ss (r, w, K; alpha, delta in ss["cal"]):
        r_t + δ = (r_ss + δ)·Z_t·(K_t/K_ss)^(α−1),   w_t = w_ss·Z_t·(K_t/K_ss)^α.
    At K = K_ss, Z = 1 this returns r_ss and w_ss exactly, whatever residual the steady state's
    bisection left between K_ss and the capital demand at r_ss."""
    K, Z = np.asarray(K, np.float64), np.asarray(Z, np.float64)
    alpha, delta = ss["cal"]["alpha"], ss["cal"]["delta"]
    x = K / ss["K"]
    # r_ss + (r_ss + δ)·(Z·x^(α−1) − 1): the same rate, and exactly r_ss at the stationary point
    r = ss["r"] + (ss["r"] + delta) * (Z * _pow(x, alpha - 1) - 1.0)
    return r, ss["w"] * Z * _pow(x, alpha)


def _pow(x, p):
    """x ** p element by element through math.pow: an element's result does not depend on its
    place in the array (a vectorised power may treat a block's tail differently), which keeps a
    path's arithmetic independent of its batch."""
    return np.array([math.pow(v, p) for v in x.ravel()]).reshape(x.shape)


def steady_state(cal, r_low=-0.02, r_high=None, steps=40, levels=3, tol=1e-5, max_iter=1000,
                 k_tol=1e-8):
    """The stationary equilibrium a transition starts from and returns to: dict(r, w, K,
    policy_c, lam ([N][Na]), cal).  r by bisection on the lottery-histogram capital supply, a
    round's candidates in one aiy_egm_ge_hist_batch call (ge_batch.egm_ge_hist_batch_call), each
    at its own wage cb.wage(r) — not the EGM script's frozen wage; then policy_c from egm_solve
    and λ, K from dist_stationary at that r."""
    from . import calibration as cb
    from . import ge_batch as gb
    from .dist import dist_stationary
    from .egm import egm_solve
    a, s, P = cal["a_grid"], cal["s"], cal["P"]
    wage = lambda r: cb.wage(r, cal["alpha"], cal["delta"])
    r0 = 0.04
    guess = np.tile((1 + r0) * a + wage(r0) * np.mean(s), (cal["N"], 1))

    def many(nodes):
        rr = np.array([n.r for n in nodes])
        Ks, Kd, it, dit, st = gb.egm_ge_hist_batch_call(rr, wage(rr), guess, cal, tol=tol,
                                                        max_iter=max_iter)
        return [(float(Ks[q]), float(Kd[q]), int(it[q]), int(st[q]), int(dit[q]))
                for q in range(len(nodes))]
    hi = 1 / cal["beta"] - 1 if r_high is None else r_high
    tr = gb.multisection(gb._with_many(many), r_low, hi, max_steps=steps, levels=levels, tol=k_tol)
    r = tr.r
    R = egm_solve(guess.T, a, s, P, r, wage(r), cal["beta"], cal["sigma"], cal["amin"], tol,
                  max_iter)
    lam, K, _, _ = dist_stationary(a, P, policy_k=R["policy_k"], tol=gb.HIST_TOL,
                                   max_iter=gb.HIST_MAX_ITER, vfi_layout=False)
    return dict(r=r, w=wage(r), K=K, policy_c=np.ascontiguousarray(R["policy_c"].T),
                lam=np.ascontiguousarray(lam.T), cal=cal)


def aiyagari_transition(ss, Z, T=None, damp=0.5, tol=1e-6, max_iter=200, backend=None):
    """The transitions after C unexpected TFP paths Z [C][T] from the steady state ss
    (steady_state's dict), by a lockstep damped fixed point on the capital paths.  Every path
    starts at K ≡ K_ss; a round prices the paths still running (prices_from_K; the terminal rate
    is r_ss), runs them through ONE transition_batch call — backend(r, w, pc_T, lam0, a_grid, s,
    P, beta, sigma, amin) -> (K_supply, status, fail_t), the GPU's by default — and updates
    K ← (1 − damp)·K + damp·K_supply with K_0 held at K_ss.  A path stops when
    max_t |K_supply − K| < tol (measured before the update), when its backend status is not 0,
    or after max_iter rounds.  A path's arithmetic does not depend on the others in its batch.
    Returns dict(K [C][T+1], r [C][T+1], w [C][T], rounds [C], status [C], resid [C])."""
    Z = np.atleast_2d(np.asarray(Z, np.float64))
    if T is None:
        T = Z.shape[1]
    if Z.shape[1] != T or T < 1:
        raise ValueError("Z must be [C][T] with T >= 1")
    run = transition_batch if backend is None else backend
    cal = ss["cal"]
    n_c = Z.shape[0]
    K = np.full((n_c, T + 1), float(ss["K"]))
    rounds, status = np.zeros(n_c, np.int64), np.zeros(n_c, np.int32)
    resid = np.full(n_c, np.nan)
    live = np.arange(n_c)

    def price(Kc, Zc):
        r, w = prices_from_K(Kc[:, :T], Zc, ss)
        return np.concatenate([r, np.full((len(Kc), 1), float(ss["r"]))], axis=1), w
    for _ in range(max_iter):
        if live.size == 0:
            break
        r, w = price(K[live], Z[live])
        Ks, st, _ = run(r, w, ss["policy_c"], ss["lam"], cal["a_grid"], cal["s"], cal["P"],
                        cal["beta"], cal["sigma"], cal["amin"])
        rounds[live] += 1
        status[live] = st
        ok = st == 0
        gap = np.full(live.size, np.nan)
        gap[ok] = np.max(np.abs(Ks[ok] - K[live[ok]]), axis=1)
        resid[live] = gap
        upd = live[ok]
        new = (1 - damp) * K[upd] + damp * Ks[ok]
        new[:, 0] = float(ss["K"])
        done = gap[ok] < tol
        K[upd[~done]] = new[~done]
        live = upd[~done]
    r, w = price(K, Z)
    return dict(K=K, r=r, w=w, rounds=rounds, status=status, resid=resid)


# ------------------------------------------------------------- sequence-space Jacobian
def expectation_batch(policy_k, y0, a_grid, P, T):
    """aiy_dist_expect_batch: the expectation vectors of C constant policies, policy_k [C][N][Na]
    (or one [N][Na]), y0 [N][Na] (shared) or [C][N][Na].  Returns E [C][T][N][Na]: E[c][t]·λ₀ is
    the mean of y0 t periods after λ₀ under policy_k[c]."""
    pk = _f(policy_k)
    if pk.ndim == 2:
        pk = pk[None]
    if pk.ndim != 3:
        raise ValueError("policy_k must be [C][N][Na]")
    n_c, N, Na = pk.shape
    a, P = _f(a_grid), np.asfortranarray(P, dtype=np.float64)
    y, shared = _start(y0, n_c, N, Na, "y0")
    E = np.empty((n_c, max(int(T), 0), N, Na))
    check(lib().aiy_dist_expect_batch(i64(n_c), i64(T), ptr(pk), ptr(y), ip(shared), ptr(a),
                                      ptr(P), i64(N), i64(Na), ptr(E)))
    return E


def expectation_batch_dev(ws, policy_k, y0, a_grid, P, E, stream=None):
    """aiy_dist_expect_batch_dev (torch tensors): policy_k [C][N][Na], y0 [N][Na] (shared) or
    [C][N][Na], E [C][T][N][Na] (out); P row-major.  Enqueues only."""
    from ._capi import stream_handle
    check(lib().aiy_dist_expect_batch_dev(ws.handle, i64(E.shape[0]), i64(E.shape[1]),
                                          ptr(policy_k), ptr(y0), ip(1 if y0.dim() == 2 else 0),
                                          ptr(a_grid), ptr(P), ptr(E), stream_handle(stream)))


def fake_news(E, lam1, h):
    """aiy_ssj_fake_news: E [T][...n], lam1 [n_in+1][T][...n] (block 0 the base path's one-step
    distributions).  Returns (F, J), each [n_in][T][T]: F[x][t][s] = E[t]·(lam1[x+1][T−1−s] −
    lam1[0][T−1−s])/h and J its sum down each diagonal."""
    E, L = _f(E), _f(lam1)
    T = E.shape[0]
    if E.ndim < 2 or L.ndim != E.ndim + 1 or L.shape[1:] != E.shape or L.shape[0] < 2:
        raise ValueError("E must be [T][...] and lam1 [n_in+1][T][...] over the same states")
    n_in, n = L.shape[0] - 1, E.size // max(T, 1)
    F, J = np.empty((n_in, T, T)), np.empty((n_in, T, T))
    check(lib().aiy_ssj_fake_news(i64(T), i64(n_in), i64(n), ptr(E), ptr(L), d(h), ptr(F), ptr(J)))
    return F, J


def fake_news_dev(E, lam1, h, F, J, stream=None):
    """aiy_ssj_fake_news_dev (torch tensors): E [T][n], lam1 [n_in+1][T][n], F, J [n_in][T][T]
    (out).  Enqueues only."""
    from ._capi import stream_handle
    check(lib().aiy_ssj_fake_news_dev(i64(E.shape[0]), i64(lam1.shape[0] - 1), i64(E.shape[1]),
                                      ptr(E), ptr(lam1), d(h), ptr(F), ptr(J),
                                      stream_handle(stream)))


def jacobian(ss, T, h=1e-4, stage_ms=None):
    """aiy_ssj_jacobian: the sequence-space Jacobians of the capital path around the steady state
    ss (steady_state's dict) by the fake-news algorithm — one backward pass of three price paths,
    one push of each of their 3T period policies, T − 1 transposed pushes and one T × T × N·Na
    contraction.  Returns dict(J_r, J_w, F_r, F_w [T][T], E [T][N][Na], status (backward,
    forward)); J_x[t][s] = ∂K_{t+1}/∂x_s.  A non-zero status: J_r and J_w are NaN.
    stage_ms: an optional float64 [4] array that receives the four stages' device times."""
    cal = ss["cal"]
    a, s, P = _f(cal["a_grid"]), _f(cal["s"]), np.asfortranarray(cal["P"], dtype=np.float64)
    N, Na = s.size, a.size
    pc, lam = _f(ss["policy_c"]), _f(ss["lam"])
    if pc.shape != (N, Na) or lam.shape != (N, Na):
        raise ValueError("ss['policy_c'] and ss['lam'] must be [N][Na]")
    Tn = max(int(T), 0)
    J_r, J_w, F_r, F_w = (np.empty((Tn, Tn)) for _ in range(4))
    E = np.empty((Tn, N, Na))
    sb, sf = ip(0), ip(0)
    check(lib().aiy_ssj_jacobian(ptr(pc), ptr(lam), d(ss["r"]), d(ss["w"]), ptr(a), ptr(s), ptr(P),
                                 i64(N), i64(Na), d(cal["beta"]), d(cal["sigma"]), d(cal["amin"]),
                                 i64(T), d(h), ptr(J_r), ptr(J_w), ptr(F_r), ptr(F_w), ptr(E),
                                 ctypes.byref(sb), ctypes.byref(sf), ptr(stage_ms)))
    return dict(J_r=J_r, J_w=J_w, F_r=F_r, F_w=F_w, E=E, status=(sb.value, sf.value))


def jacobian_batch(ss_list, T, h=1e-4, stage_ms=None, chunk=0, want_F=True, want_E=True):
    """aiy_ssj_jacobian_batch: jacobian() of C steady states (a list of steady_state's dicts with
    one N and one Na; everything else — β, σ, amin, the grid, the shocks, r, w — is the
    economy's own) in one call, each stage one launch over a chunk of economies.  Returns
    dict(J_r, J_w, F_r, F_w [C][T][T], E [C][T][N][Na], status [C][2] (backward, forward));
    economy e's arrays are jacobian(ss_list[e], T, h)'s bit for bit, whatever the batch.
    stage_ms: an optional float64 [4] array that receives the four stages' device times;
    chunk: economies staged at a time (0: as many as fit the 4 GiB cap); want_F, want_E: False
    leaves F_r, F_w or E out of the dict and on the device (E is T·N·Na doubles an economy)."""
    ss_list = list(ss_list)
    if not ss_list:
        raise ValueError("jacobian_batch needs at least one steady state")
    N, Na = _f(ss_list[0]["cal"]["s"]).size, _f(ss_list[0]["cal"]["a_grid"]).size
    for e, ss in enumerate(ss_list):
        cal = ss["cal"]
        if _f(cal["s"]).size != N or _f(cal["a_grid"]).size != Na:
            raise ValueError(f"economy {e} has another N or Na than economy 0")
        if _f(ss["policy_c"]).shape != (N, Na) or _f(ss["lam"]).shape != (N, Na):
            raise ValueError(f"economy {e}: ss['policy_c'] and ss['lam'] must be [N][Na]")
    n_c = len(ss_list)
    col = lambda f: np.ascontiguousarray(np.stack([_f(f(ss)) for ss in ss_list]))
    pc, lam = col(lambda ss: ss["policy_c"]), col(lambda ss: ss["lam"])
    a, s = col(lambda ss: ss["cal"]["a_grid"]), col(lambda ss: ss["cal"]["s"])
    P = col(lambda ss: _f(ss["cal"]["P"]).T)  # each block column-major
    r, w = col(lambda ss: ss["r"]), col(lambda ss: ss["w"])
    beta, sigma, amin = (col(lambda ss, k=k: ss["cal"][k]) for k in ("beta", "sigma", "amin"))
    Tn = max(int(T), 0)
    J_r, J_w = np.empty((n_c, Tn, Tn)), np.empty((n_c, Tn, Tn))
    F_r, F_w = (np.empty((n_c, Tn, Tn)), np.empty((n_c, Tn, Tn))) if want_F else (None, None)
    E = np.empty((n_c, Tn, N, Na)) if want_E else None
    sb, sf = np.zeros(n_c, np.int32), np.zeros(n_c, np.int32)
    check(lib().aiy_ssj_jacobian_batch(i64(n_c), ptr(pc), ptr(lam), ptr(r), ptr(w), ptr(a), ptr(s),
                                       ptr(P), i64(N), i64(Na), ptr(beta), ptr(sigma), ptr(amin),
                                       i64(T), d(h), ptr(J_r), ptr(J_w), ptr(F_r), ptr(F_w),
                                       ptr(E), ptr(sb), ptr(sf), ptr(stage_ms), i64(chunk)))
    out = dict(J_r=J_r, J_w=J_w, status=np.stack([sb, sf], axis=1))
    if want_F:
        out.update(F_r=F_r, F_w=F_w)
    if want_E:
        out["E"] = E
    return out


def _price_slopes(ss):
    """∂r/∂K, ∂w/∂K, ∂r/∂Z, ∂w/∂Z of prices_from_K at the steady state."""
    alpha, delta = ss["cal"]["alpha"], ss["cal"]["delta"]
    r_K = (ss["r"] + delta) * (alpha - 1) / ss["K"]
    w_K = ss["w"] * alpha / ss["K"]
    return r_K, w_K, ss["r"] + delta, ss["w"]


def _newton_matrix(ss, jac):
    """M − I, M = ∂K_supply[1:]/∂K[1:]: K_j moves r_j and w_j, j = 1 … T−1 (K_T moves no price
    inside the horizon: M's last column is zero)."""
    J_r, J_w = _f(jac["J_r"]), _f(jac["J_w"])
    r_K, w_K, _, _ = _price_slopes(ss)
    T = J_r.shape[0]
    M = np.zeros((T, T))
    M[:, :T - 1] = J_r[:, 1:] * r_K + J_w[:, 1:] * w_K
    return M - np.eye(T)


def impulse_response(ss, jac, dZ):
    """The linear response dK [C][T+1] (dK_0 = 0) of the capital path to the TFP paths 1 + dZ,
    dZ [C][T]: (I − M)·dK[1:] = J_r·(∂r/∂Z·dZ) + J_w·(∂w/∂Z·dZ) with M of
    aiyagari_transition_newton and the slopes of prices_from_K at the steady state.  Each path
    is its own solve."""
    dZ = np.atleast_2d(np.asarray(dZ, np.float64))
    A = -_newton_matrix(ss, jac)
    _, _, r_Z, w_Z = _price_slopes(ss)
    J_r, J_w = _f(jac["J_r"]), _f(jac["J_w"])
    if dZ.shape[1] != J_r.shape[0]:
        raise ValueError("dZ must be [C][T] with the Jacobian's T")
    out = np.zeros((dZ.shape[0], dZ.shape[1] + 1))
    for c in range(dZ.shape[0]):
        out[c, 1:] = np.linalg.solve(A, J_r @ (r_Z * dZ[c]) + J_w @ (w_Z * dZ[c]))
    return out


def aiyagari_transition_newton(ss, Z, T=None, jac=None, tol=1e-6, max_iter=50, backend=None):
    """aiyagari_transition with a Newton update from the steady state's sequence-space Jacobian:
    the same arguments, lockstep rounds, stopping rule (max_t |K_supply − K| < tol, measured
    before the update), statuses and return dict; the update is
        K[1:] ← K[1:] − (M − I)⁻¹·(K_supply − K)[1:],   K_0 held at K_ss,
    M[:, j−1] = J_r[:, j]·r_K + J_w[:, j]·w_K (j = 1 … T−1, last column zero), r_K = (r_ss + δ)
    (α − 1)/K_ss, w_K = w_ss·α/K_ss.  The same (M − I) serves every round and path; a path's update
    is its own single-right-hand-side solve, so its arithmetic does not depend on its batch.
    jac: jacobian(ss, T)'s dict (computed once when None)."""
    Z = np.atleast_2d(np.asarray(Z, np.float64))
    if T is None:
        T = Z.shape[1]
    if Z.shape[1] != T or T < 1:
        raise ValueError("Z must be [C][T] with T >= 1")
    run = transition_batch if backend is None else backend
    if jac is None:
        jac = jacobian(ss, T)
    if np.shape(jac["J_r"]) != (T, T) or np.shape(jac["J_w"]) != (T, T):
        raise ValueError("jac must hold J_r and J_w [T][T]")
    A = _newton_matrix(ss, jac)
    if not np.isfinite(A).all():
        raise ValueError(f"the Jacobian is not finite (jacobian()'s status: {jac.get('status')})")
    cal = ss["cal"]
    n_c = Z.shape[0]
    K = np.full((n_c, T + 1), float(ss["K"]))
    rounds, status = np.zeros(n_c, np.int64), np.zeros(n_c, np.int32)
    resid = np.full(n_c, np.nan)
    live = np.arange(n_c)

    def price(Kc, Zc):
        r, w = prices_from_K(Kc[:, :T], Zc, ss)
        return np.concatenate([r, np.full((len(Kc), 1), float(ss["r"]))], axis=1), w
    for _ in range(max_iter):
        if live.size == 0:
            break
        r, w = price(K[live], Z[live])
        Ks, st, _ = run(r, w, ss["policy_c"], ss["lam"], cal["a_grid"], cal["s"], cal["P"],
                        cal["beta"], cal["sigma"], cal["amin"])
        rounds[live] += 1
        status[live] = st
        ok = st == 0
        gap = np.full(live.size, np.nan)
        gap[ok] = np.max(np.abs(Ks[ok] - K[live[ok]]), axis=1)
        resid[live] = gap
        upd = live[ok]
        done = gap[ok] < tol
        Kok = Ks[ok]
        for q in np.flatnonzero(~done):
            c = upd[q]
            K[c, 1:] = K[c, 1:] - np.linalg.solve(A, (Kok[q] - K[c])[1:])
        live = upd[~done]
    r, w = price(K, Z)
    return dict(K=K, r=r, w=w, rounds=rounds, status=status, resid=resid)


# ------------------------------------------------------------- the endogenous-labour economy
def labor_egm_backward_batch(r, w, pc_T, a_grid, s, P, beta, sigma, phi, theta, amin,
                             want_pc=True):
    """aiy_labor_egm_backward_batch: egm_backward_batch for the labour economy (A5).  Returns
    dict(policy_k, policy_l, policy_c [C][T][N][Na] (policy_c None unless want_pc), status [C],
    fail_t [C])."""
    r, w, n_c, T = _paths(r, w)
    a, s, P = _f(a_grid), _f(s), np.asfortranarray(P, dtype=np.float64)
    N, Na = s.size, a.size
    pcT, shared = _start(pc_T, n_c, N, Na, "pc_T")
    pk, pl = np.empty((n_c, T, N, Na)), np.empty((n_c, T, N, Na))
    pc = np.empty((n_c, T, N, Na)) if want_pc else None
    st, ft = np.zeros(n_c, np.int32), np.zeros(n_c, np.int32)
    check(lib().aiy_labor_egm_backward_batch(i64(n_c), i64(T), ptr(r), ptr(w), ptr(pcT), ip(shared),
                                             ptr(a), ptr(s), ptr(P), i64(N), i64(Na), d(beta),
                                             d(sigma), d(phi), d(theta), d(amin), ptr(pk), ptr(pl),
                                             ptr(pc), ptr(st), ptr(ft)))
    return dict(policy_k=pk, policy_l=pl, policy_c=pc, status=st, fail_t=ft)


def labor_dist_forward_batch(policy_k, policy_l, lam0, a_grid, s, P, want_lam=True):
    """aiy_labor_dist_forward_batch: dist_forward_batch and the hours in efficiency units,
    H[c][t] = Σ λ_t·(s_j·policy_l[c][t]).  Returns dict(K [C][T+1], H [C][T], lam_T, status,
    fail_t); on status 2, K and H beyond fail_t are NaN."""
    pk, pl = _f(policy_k), _f(policy_l)
    if pk.ndim != 4 or pl.shape != pk.shape:
        raise ValueError("policy_k and policy_l must be [C][T][N][Na]")
    n_c, T, N, Na = pk.shape
    a, s, P = _f(a_grid), _f(s), np.asfortranarray(P, dtype=np.float64)
    l0, shared = _start(lam0, n_c, N, Na, "lam0")
    K, H = np.empty((n_c, T + 1)), np.empty((n_c, T))
    lT = np.empty((n_c, N, Na)) if want_lam else None
    st, ft = np.zeros(n_c, np.int32), np.zeros(n_c, np.int32)
    check(lib().aiy_labor_dist_forward_batch(i64(n_c), i64(T), ptr(pk), ptr(pl), ptr(l0),
                                             ip(shared), ptr(a), ptr(s), ptr(P), i64(N), i64(Na),
                                             ptr(K), ptr(H), ptr(lT), ptr(st), ptr(ft)))
    return dict(K=K, H=H, lam_T=lT, status=st, fail_t=ft)


def labor_transition_batch(r, w, pc_T, lam0, a_grid, s, P, beta, sigma, phi, theta, amin):
    """aiy_labor_transition_batch: both passes on one stream, the period policies staying on the
    device.  Returns (K [C][T+1], H [C][T], status [C], fail_t [C]); a path with status 1 has K
    and H all NaN."""
    r, w, n_c, T = _paths(r, w)
    a, s, P = _f(a_grid), _f(s), np.asfortranarray(P, dtype=np.float64)
    N, Na = s.size, a.size
    pcT, pshared = _start(pc_T, n_c, N, Na, "pc_T")
    l0, lshared = _start(lam0, n_c, N, Na, "lam0")
    K, H = np.empty((n_c, T + 1)), np.empty((n_c, T))
    st, ft = np.zeros(n_c, np.int32), np.zeros(n_c, np.int32)
    check(lib().aiy_labor_transition_batch(i64(n_c), i64(T), ptr(r), ptr(w), ptr(pcT),
                                           ip(pshared), ptr(l0), ip(lshared), ptr(a), ptr(s),
                                           ptr(P), i64(N), i64(Na), d(beta), d(sigma), d(phi),
                                           d(theta), d(amin), ptr(K), ptr(H), ptr(st), ptr(ft)))
    return K, H, st, ft


def labor_egm_backward_batch_dev(ws, r, w, pc_T, a_grid, s, P, beta, sigma, phi, theta, amin,
                                 policy_k, policy_l, policy_c=None, stream=None):
    """aiy_labor_egm_backward_batch_dev (torch tensors; r [C][T+1] and w [C][T] numpy): as
    egm_backward_batch_dev, with policy_l [C][T][N][Na].  Returns (status [C], fail_t [C])."""
    from ._capi import stream_handle
    r, w, n_c, T = _paths(r, w)
    st, ft = np.zeros(n_c, np.int32), np.zeros(n_c, np.int32)
    check(lib().aiy_labor_egm_backward_batch_dev(
        ws.handle, i64(n_c), i64(T), ptr(r), ptr(w), ptr(pc_T), ip(1 if pc_T.dim() == 2 else 0),
        ptr(a_grid), ptr(s), ptr(P), d(beta), d(sigma), d(phi), d(theta), d(amin), ptr(policy_k),
        ptr(policy_l), ptr(policy_c), ptr(st), ptr(ft), stream_handle(stream)))
    return st, ft


def labor_dist_forward_batch_dev(ws, policy_k, policy_l, lam0, a_grid, s, P, K, H, lam_T=None,
                                 stream=None):
    """aiy_labor_dist_forward_batch_dev (torch tensors): as dist_forward_batch_dev, with policy_l
    [C][T][N][Na], s [N] and H [C][T].  Returns (status [C], fail_t [C])."""
    from ._capi import stream_handle
    n_c, T = int(policy_k.shape[0]), int(policy_k.shape[1])
    st, ft = np.zeros(n_c, np.int32), np.zeros(n_c, np.int32)
    check(lib().aiy_labor_dist_forward_batch_dev(
        ws.handle, i64(n_c), i64(T), ptr(policy_k), ptr(policy_l), ptr(lam0),
        ip(1 if lam0.dim() == 2 else 0), ptr(a_grid), ptr(s), ptr(P), ptr(K), ptr(H), ptr(lam_T),
        ptr(st), ptr(ft), stream_handle(stream)))
    return st, ft


def prices_from_ratio(kappa, Z, ss):
    """The price paths of capital per effective hour κ = K/H and TFP paths Z (same shape),
    anchored to the steady state ss (r, w, K, H), x = κ/κ_ss, κ_ss = K_ss/H_ss:
        r_t = r_ss + (r_ss + δ)·(Z_t·x_t^(α−1) − 1),   w_t = w_ss·Z_t·x_t^α.
    At κ = κ_ss, Z = 1 this returns r_ss and w_ss exactly."""
    kappa, Z = np.asarray(kappa, np.float64), np.asarray(Z, np.float64)
    alpha, delta = ss["cal"]["alpha"], ss["cal"]["delta"]
    x = kappa / (ss["K"] / ss["H"])
    r = ss["r"] + (ss["r"] + delta) * (Z * _pow(x, alpha - 1) - 1.0)
    return r, ss["w"] * Z * _pow(x, alpha)


def hours_sum(lam, policy_l, s):
    """H = Σ λ·(s_j·policy_l) of [N][Na] arrays, on the host."""
    return float(np.sum(_f(lam) * (_f(s)[:, None] * _f(policy_l))))


def labor_excess(K, H, r, alpha, delta):
    """K − H·(α/(r+δ))^(1/(1−α)): the capital market's excess supply at hours H."""
    return K - H * (alpha / (r + delta)) ** (1 / (1 - alpha))


def steady_state_labor(cal, phi=1.0, theta=1.0, r_low=0.0, r_high=None, rounds=12, width=7,
                       tol=1e-11, max_iter=5000, k_tol=1e-8, device="cuda"):
    """The stationary equilibrium of the labour economy (A5): dict(r, w, K, H, policy_c, policy_l,
    policy_k, lam ([N][Na]), cal, phi, theta).  r by bisection on K_s(r) − H(r)·(α/(r+δ))^(1/(1−α)) at
    w = cb.wage(r): a round's `width` equally spaced candidates go through ONE batched labour EGM
    solve (egm_solve_batch_dev, labor=True) and ONE batched stationary-distribution solve
    (dist_stationary_batch_dev); H is summed on the host from the returned λ and policy_l.  The
    bracket shrinks to the sub-interval where the excess changes sign (× 1/(width+1) per round)
    and the search stops once a candidate's |excess| <= k_tol.  Not the script's K_d, which uses
    the exogenous aggregate cal["labor"]: here labour demand is the hours households supply."""
    import torch
    from . import calibration as cb
    from . import ge_batch as gb
    from .dist import dist_stationary_batch_dev
    from .egm import egm_solve_batch_dev
    from .vfi import Workspace
    a, s, P = _f(cal["a_grid"]), _f(cal["s"]), _f(cal["P"])
    N, Na = s.size, a.size
    alpha, delta = cal["alpha"], cal["delta"]
    wage = lambda r: cb.wage(r, alpha, delta)
    f64 = dict(dtype=torch.float64, device=device)
    da, ds, dP = (torch.as_tensor(x, **f64) for x in (a, s, P))
    ws = Workspace(N, Na)
    r0 = 0.04  # the labour script's starting policy_c (Aiyagari_Endogenous_Labor_EGM.m:58)
    guess = np.tile((1 + r0) * a + wage(r0) * np.mean(s), (N, 1))
    uni = np.full((N, Na), 1.0 / (N * Na))

    def many(rr):
        rr = np.ascontiguousarray(rr, np.float64)
        n_c = rr.size
        pc = torch.as_tensor(np.tile(guess, (n_c, 1, 1)), **f64)
        pk, pl = torch.empty_like(pc), torch.empty_like(pc)
        _, _, st = egm_solve_batch_dev(ws, rr, wage(rr), pc, da, ds, dP, cal["beta"], cal["sigma"],
                                       cal["amin"], tol, max_iter, pk, labor=True, phi=phi,
                                       theta=theta, policy_l=pl)
        if st.any():
            raise RuntimeError(f"labour EGM solve: status {st} at r = {rr}")
        lam = torch.empty_like(pc)
        Ks = torch.empty(n_c, **f64)
        dist_stationary_batch_dev(ws, torch.as_tensor(np.tile(uni, (n_c, 1, 1)), **f64), da, dP,
                                  lam, policy_k=pk, tol=gb.HIST_TOL, max_iter=gb.HIST_MAX_ITER,
                                  k_supply=Ks)
        torch.cuda.synchronize()
        lam, pl, pc, pk, Ks = (x.cpu().numpy() for x in (lam, pl, pc, pk, Ks))
        H = np.array([hours_sum(lam[q], pl[q], s) for q in range(n_c)])
        ex = np.array([labor_excess(Ks[q], H[q], rr[q], alpha, delta) for q in range(n_c)])
        return ex, Ks, H, pc, pl, pk, lam
    try:
        lo, hi = r_low, (1 / cal["beta"] - 1 if r_high is None else r_high)
        best = None
        for _ in range(rounds):
            rr = lo + (hi - lo) * np.arange(1, width + 1) / (width + 1)
            ex, Ks, H, pc, pl, pk, lam = many(rr)
            q = int(np.argmin(np.abs(ex)))
            if best is None or abs(ex[q]) < abs(best[0]):
                best = (ex[q], rr[q], Ks[q], H[q], pc[q], pl[q], pk[q], lam[q])
            if abs(best[0]) <= k_tol:
                break
            up = np.flatnonzero(ex > 0)  # the excess supply rises with r
            j = int(up[0]) if up.size else width
            lo, hi = (rr[j - 1] if j > 0 else lo), (rr[j] if j < width else hi)
    finally:
        ws.close()
    _, r, K, H, pc, pl, pk, lam = best
    return dict(r=float(r), w=float(wage(r)), K=float(K), H=float(H), policy_c=pc, policy_l=pl,
                policy_k=pk, lam=lam, cal=cal, phi=phi, theta=theta)


def jacobian_labor(ss, T, h=1e-4, stage_ms=None):
    """aiy_ssj_jacobian_labor: the sequence-space Jacobians of the labour economy's capital and
    hours paths around the steady state ss (steady_state_labor's dict).  Returns dict(J_Kr, J_Kw
    (J[t][s] = ∂K_{t+1}/∂x_s), J_Hr, J_Hw (J[t][s] = ∂H_t/∂x_s), F_Kr, F_Kw, F_Hr, F_Hw [T][T],
    E_a, E_h [T][N][Na], status (backward, forward)).  A non-zero status: the J are NaN."""
    cal = ss["cal"]
    a, s, P = _f(cal["a_grid"]), _f(cal["s"]), np.asfortranarray(cal["P"], dtype=np.float64)
    N, Na = s.size, a.size
    pc, lam = _f(ss["policy_c"]), _f(ss["lam"])
    if pc.shape != (N, Na) or lam.shape != (N, Na):
        raise ValueError("ss['policy_c'] and ss['lam'] must be [N][Na]")
    Tn = max(int(T), 0)
    M = {k: np.empty((Tn, Tn)) for k in ("J_Kr", "J_Kw", "J_Hr", "J_Hw", "F_Kr", "F_Kw", "F_Hr",
                                         "F_Hw")}
    E_a, E_h = np.empty((Tn, N, Na)), np.empty((Tn, N, Na))
    sb, sf = ip(0), ip(0)
    check(lib().aiy_ssj_jacobian_labor(
        ptr(pc), ptr(lam), d(ss["r"]), d(ss["w"]), ptr(a), ptr(s), ptr(P), i64(N), i64(Na),
        d(cal["beta"]), d(cal["sigma"]), d(ss["phi"]), d(ss["theta"]), d(cal["amin"]), i64(T), d(h),
        ptr(M["J_Kr"]), ptr(M["J_Kw"]), ptr(M["J_Hr"]), ptr(M["J_Hw"]), ptr(M["F_Kr"]),
        ptr(M["F_Kw"]), ptr(M["F_Hr"]), ptr(M["F_Hw"]), ptr(E_a), ptr(E_h), ctypes.byref(sb),
        ctypes.byref(sf), ptr(stage_ms)))
    return dict(M, E_a=E_a, E_h=E_h, status=(sb.value, sf.value))


def _ratio_slopes(ss):
    """∂r/∂κ, ∂w/∂κ, ∂r/∂Z, ∂w/∂Z of prices_from_ratio at the steady state."""
    alpha, delta = ss["cal"]["alpha"], ss["cal"]["delta"]
    k_ss = ss["K"] / ss["H"]
    return ((ss["r"] + delta) * (alpha - 1) / k_ss, ss["w"] * alpha / k_ss, ss["r"] + delta,
            ss["w"])


def _labor_response(ss, jac, r_x, w_x):
    """∂κ_supply/∂x for prices moving with slopes (r_x, w_x): κ_s,t = K_t/H_t, K_t the
    Jacobian's row t − 1 (K_0 is given), so
    ((J′_Kr·r_x + J′_Kw·w_x) − κ_ss·(J_Hr·r_x + J_Hw·w_x))/H_ss with J′_K = J_K shifted a row."""
    JK = _f(jac["J_Kr"]) * r_x + _f(jac["J_Kw"]) * w_x
    JH = _f(jac["J_Hr"]) * r_x + _f(jac["J_Hw"]) * w_x
    JKs = np.zeros_like(JK)
    JKs[1:] = JK[:-1]
    return (JKs - (ss["K"] / ss["H"]) * JH) / ss["H"]


def _labor_newton_matrix(ss, jac):
    """M − I, M = ∂κ_supply/∂κ at the steady state."""
    r_k, w_k, _, _ = _ratio_slopes(ss)
    M = _labor_response(ss, jac, r_k, w_k)
    return M - np.eye(M.shape[0])


def impulse_response_labor(ss, jac, dZ):
    """The linear responses (dK [C][T+1], dH [C][T]) to the TFP paths 1 + dZ, dZ [C][T]:
    (I − M)·dκ = N_Z·dZ with M of aiyagari_labor_transition_newton and N_Z = ∂κ_supply/∂Z, then
    dr = r_κ·dκ + r_Z·dZ, dw likewise, dK[1:] = J_Kr·dr + J_Kw·dw, dH = J_Hr·dr + J_Hw·dw.  Each
    path is its own solve."""
    dZ = np.atleast_2d(np.asarray(dZ, np.float64))
    r_k, w_k, r_Z, w_Z = _ratio_slopes(ss)
    A = -_labor_newton_matrix(ss, jac)
    NZ = _labor_response(ss, jac, r_Z, w_Z)
    if dZ.shape[1] != A.shape[0]:
        raise ValueError("dZ must be [C][T] with the Jacobian's T")
    dK, dH = np.zeros((dZ.shape[0], dZ.shape[1] + 1)), np.zeros(dZ.shape)
    for c in range(dZ.shape[0]):
        dk = np.linalg.solve(A, NZ @ dZ[c])
        dr, dw = r_k * dk + r_Z * dZ[c], w_k * dk + w_Z * dZ[c]
        dK[c, 1:] = _f(jac["J_Kr"]) @ dr + _f(jac["J_Kw"]) @ dw
        dH[c] = _f(jac["J_Hr"]) @ dr + _f(jac["J_Hw"]) @ dw
    return dK, dH


def _labor_driver(ss, Z, T, tol, max_iter, backend, update):
    """The lockstep loop both labour drivers share; update(κ_c, κ_supply_c) -> the next κ_c."""
    Z = np.atleast_2d(np.asarray(Z, np.float64))
    if T is None:
        T = Z.shape[1]
    if Z.shape[1] != T or T < 1:
        raise ValueError("Z must be [C][T] with T >= 1")
    run = labor_transition_batch if backend is None else backend
    cal = ss["cal"]
    n_c = Z.shape[0]
    kap = np.full((n_c, T), float(ss["K"]) / float(ss["H"]))
    K, H = np.full((n_c, T + 1), np.nan), np.full((n_c, T), np.nan)
    rounds, status = np.zeros(n_c, np.int64), np.zeros(n_c, np.int32)
    resid = np.full(n_c, np.nan)
    live = np.arange(n_c)

    def price(kc, Zc):
        r, w = prices_from_ratio(kc, Zc, ss)
        return np.concatenate([r, np.full((len(kc), 1), float(ss["r"]))], axis=1), w
    for _ in range(max_iter):
        if live.size == 0:
            break
        r, w = price(kap[live], Z[live])
        Ks, Hs, st, _ = run(r, w, ss["policy_c"], ss["lam"], cal["a_grid"], cal["s"], cal["P"],
                            cal["beta"], cal["sigma"], ss["phi"], ss["theta"], cal["amin"])
        rounds[live] += 1
        status[live] = st
        K[live], H[live] = Ks, Hs
        ok = st == 0
        ks = Ks[ok][:, :T] / Hs[ok]
        gap = np.full(live.size, np.nan)
        gap[ok] = np.max(np.abs(ks - kap[live[ok]]), axis=1)
        resid[live] = gap
        upd = live[ok]
        done = gap[ok] < tol
        for q in np.flatnonzero(~done):
            kap[upd[q]] = update(kap[upd[q]], ks[q])
        live = upd[~done]
    r, w = price(kap, Z)
    return dict(K=K, H=H, kappa=kap, r=r, w=w, rounds=rounds, status=status, resid=resid)


def aiyagari_labor_transition(ss, Z, T=None, damp=0.05, tol=1e-6, max_iter=1000, backend=None):
    """The labour economy's transitions after C unexpected TFP paths Z [C][T] from the steady
    state ss (steady_state_labor's dict), by a lockstep damped fixed point.  The unknown is
    capital per effective hour κ_t = K_t/H_t, t = 0 … T−1 — hours jump on impact, so K_0 being
    given does not pin the date-0 prices, and prices depend on K and H through κ alone.  Every
    path starts at κ ≡ κ_ss; a round prices the paths still running (prices_from_ratio; the
    terminal rate is r_ss), runs them through ONE labor_transition_batch call — backend(r, w,
    pc_T, lam0, a_grid, s, P, beta, sigma, phi, theta, amin) -> (K, H, status, fail_t), the GPU's
    by default — sets κ_s = K[:T]/H and updates κ ← (1 − damp)·κ + damp·κ_s.  A path stops when
    max_t |κ_s − κ| < tol (measured before the update), on a non-zero status, or after max_iter
    rounds.  A path's arithmetic does not depend on the others in its batch.
    damp defaults to 0.05, not the exogenous driver's 0.5: with elastic hours the map κ → κ_s
    overshoots — the leading eigenvalue of M = ∂κ_s/∂κ is real and negative — and the damped
    update contracts only for damp < 2/(1 + ρ(M)).  ρ(M) grows with the horizon: measured on the
    labour script's calibration 2.9, 7.5, 14.4 and 20.4 at T = 30, 60, 120 and 240 (N = 3,
    Na = 60), 7.4 at T = 60 (N = 7, Na = 100).  So 0.5 diverges from T ≈ 30 on (gaps 0.82, 5.8, 50
    after 2, 4, 6 rounds at T = 60), 0.1 from T ≈ 240 on; 0.05 covers ρ < 39 and takes about 270
    rounds to 1e-8 on a 1 % AR(0.9) TFP path, where the Newton driver takes 5.
    Returns dict(K [C][T+1], H [C][T] (the last round's supply), kappa [C][T], r [C][T+1],
    w [C][T], rounds [C], status [C], resid [C])."""
    return _labor_driver(ss, Z, T, tol, max_iter, backend,
                         lambda k, ks: (1 - damp) * k + damp * ks)


def aiyagari_labor_transition_newton(ss, Z, T=None, jac=None, tol=1e-6, max_iter=50,
                                     backend=None):
    """aiyagari_labor_transition with a Newton update from the steady state's sequence-space
    Jacobians: the same arguments, rounds, stopping rule and return dict; the update is
        κ ← κ − (M − I)⁻¹·(κ_s − κ),
    M = ((J′_Kr·r_κ + J′_Kw·w_κ) − κ_ss·(J_Hr·r_κ + J_Hw·w_κ))/H_ss, J′_K[0] = 0 and J′_K[t] =
    J_K[t−1], r_κ = (r_ss + δ)(α − 1)/κ_ss, w_κ = w_ss·α/κ_ss.  The same (M − I) serves every
    round and path; a path's update is its own single-right-hand-side solve.
    jac: jacobian_labor(ss, T)'s dict (computed once when None)."""
    Tn = np.atleast_2d(np.asarray(Z)).shape[1] if T is None else T
    if jac is None:
        jac = jacobian_labor(ss, Tn)
    if any(np.shape(jac[k]) != (Tn, Tn) for k in ("J_Kr", "J_Kw", "J_Hr", "J_Hw")):
        raise ValueError("jac must hold J_Kr, J_Kw, J_Hr and J_Hw [T][T]")
    A = _labor_newton_matrix(ss, jac)
    if not np.isfinite(A).all():
        raise ValueError(f"the Jacobian is not finite (jacobian_labor()'s status: "
                         f"{jac.get('status')})")
    return _labor_driver(ss, Z, T, tol, max_iter, backend,
                         lambda k, ks: k - np.linalg.solve(A, ks - k))
