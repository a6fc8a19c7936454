"""CPU reference of the labour economy's transition passes, steady state and sequence-space
Jacobian (TEST INFRASTRUCTURE ONLY; not a test module).

Backward: tests/support/labor_transition_ref.c — orc_labor_egm_step's operations with r split
into r_next and r_now — built into tests/support/liblabor_transition_ref.so by
__graft_entry__.build(), or here with gcc when it is missing.  Forward: corc.dist_update_lottery
chained in Python, K = Σ λ·a by tests/transition_ref.py's capital_sum and H = Σ λ·(s_j·pl)
restated in the same (the device's) summation order, the inner product rounded first.
labor_transition_batch is the CPU stand-in for transition.labor_transition_batch (backend=).
Arrays are [N][Na] rows per (path, period), C-contiguous."""
from __future__ import annotations

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

from oracle import corc
from tests import ssj_ref as sr
from tests import transition_ref as tr

_HERE = Path(__file__).resolve().parent / "support"
SRC, LIB = _HERE / "labor_transition_ref.c", _HERE / "liblabor_transition_ref.so"
_LIB = None

_d, _i64, _P = C.c_double, C.c_int64, C.c_void_p
f64 = corc.f64


def build(force=False):
    if force or not LIB.exists() or LIB.stat().st_mtime < SRC.stat().st_mtime:
        subprocess.run(["gcc", *tr.CFLAGS, "-shared", "-o", str(LIB), str(SRC), "-lm"], check=True)
    return LIB


def lib():
    global _LIB
    if _LIB is None:
        L = C.CDLL(str(build()))
        L.lref_labor_step2.restype = C.c_int
        L.lref_labor_backward.restype = C.c_int
        _LIB = L
    return _LIB


def _p(x):
    return None if x is None else x.ctypes.data_as(_P)


def labor_step2(pc_next, a, s, P, r_next, r_now, w_now, beta, sigma, phi, theta, amin):
    """One two-rate labour step -> (pc_now, pk_now, pl_now, ahat, bad)."""
    pc_next, a, s, P = map(f64, (pc_next, a, s, P))
    N, Na = pc_next.shape
    pc, pk, pl, ah = (np.empty((N, Na)) for _ in range(4))
    bad = lib().lref_labor_step2(_i64(N), _i64(Na), _p(pc_next), _p(a), _p(s), _p(P), _d(r_next),
                                 _d(r_now), _d(w_now), _d(beta), _d(sigma), _d(phi), _d(theta),
                                 _d(amin), _p(pc), _p(pk), _p(pl), _p(ah))
    assert bad in (0, 1)
    return pc, pk, pl, ah, bad


def labor_backward(r, w, pc_T, a, s, P, beta, sigma, phi, theta, amin):
    """One path: r [T+1], w [T], pc_T [N][Na] -> dict(pk, pl, pc [T][N][Na], status, fail_t).
    Periods below fail_t are NaN."""
    r, w, pc_T, a, s, P = map(f64, (r, w, pc_T, a, s, P))
    T = w.size
    assert r.size == T + 1
    N, Na = pc_T.shape
    pk, pl, pc = (np.full((T, N, Na), np.nan) for _ in range(3))
    st, ft = C.c_int32(), C.c_int32()
    rc = lib().lref_labor_backward(_i64(N), _i64(Na), _i64(T), _p(r), _p(w), _p(pc_T), _p(a),
                                   _p(s), _p(P), _d(beta), _d(sigma), _d(phi), _d(theta),
                                   _d(amin), _p(pk), _p(pl), _p(pc), C.byref(st), C.byref(ft))
    assert rc == 0 and st.value in (0, 1)
    return dict(pk=pk, pl=pl, pc=pc, status=st.value, fail_t=ft.value)


def hours_sum(lam, pl, s):
    """Σ λ·(s_j·pl) in launch_dist_capital's order (N·Na <= 65,536: one term per thread), the
    inner product rounded first."""
    lam, pl, s = f64(lam), f64(pl), f64(s)
    n = lam.size
    assert n <= 65536
    x = 0.0 + lam.ravel() * (s[:, None] * pl).ravel()
    nb = -(-n // 256)
    blk = np.zeros(nb * 256)
    blk[:n] = x
    blk = blk.reshape(nb, 256)
    q = 128
    while q > 0:
        blk[:, :q] = blk[:, :q] + blk[:, q:2 * q]
        q >>= 1
    acc = 0.0
    for b in range(nb):
        acc = acc + blk[b, 0]
    return float(acc)


def labor_forward(pk, pl, lam0, a, s, P):
    """One path: pk, pl [T][N][Na], lam0 [N][Na] -> dict(lam [T+1][N][Na], K [T+1], H [T],
    status, fail_t).  K[t] and H[t] are formed before period t's monotonicity check; a period
    whose keys are not monotone stops the path (status 2): K and H beyond it are NaN."""
    pk, pl, lam0, a, s, P = map(f64, (pk, pl, lam0, a, s, P))
    T = pk.shape[0]
    lam = [lam0]
    K, H = np.full(T + 1, np.nan), np.full(T, np.nan)
    status, fail_t = 0, -1
    for t in range(T):
        K[t] = tr.capital_sum(lam[-1], a)
        H[t] = hours_sum(lam[-1], pl[t], s)
        if (np.diff(tr.lottery_keys(pk[t], a), axis=1) < 0).any():
            status, fail_t = 2, t
            break
        lam.append(corc.dist_update_lottery(lam[-1], pk[t], a, P))
    if status == 0:
        K[T] = tr.capital_sum(lam[-1], a)
    return dict(lam=np.stack(lam), K=K, H=H, status=status, fail_t=fail_t)


def labor_transition(r, w, pc_T, lam0, a, s, P, beta, sigma, phi, theta, amin):
    """One path through both passes -> dict(K [T+1], H [T], status, fail_t, pk, pl, lam)."""
    B = labor_backward(r, w, pc_T, a, s, P, beta, sigma, phi, theta, amin)
    if B["status"]:
        T = len(w)
        return dict(K=np.full(T + 1, np.nan), H=np.full(T, np.nan), status=B["status"],
                    fail_t=B["fail_t"], pk=B["pk"], pl=B["pl"], lam=None)
    F = labor_forward(B["pk"], B["pl"], lam0, a, s, P)
    return dict(K=F["K"], H=F["H"], status=F["status"], fail_t=F["fail_t"], pk=B["pk"],
                pl=B["pl"], lam=F["lam"])


def labor_transition_batch(r, w, pc_T, lam0, a_grid, s, P, beta, sigma, phi, theta, amin):
    """The CPU stand-in for transition.labor_transition_batch (same arguments and results)."""
    r, w = np.atleast_2d(f64(r)), np.atleast_2d(f64(w))
    n_c = r.shape[0]
    pc_T, lam0 = f64(pc_T), f64(lam0)
    pick = lambda x, c: x if x.ndim == 2 else x[c]
    res = [labor_transition(r[c], w[c], pick(pc_T, c), pick(lam0, c), a_grid, s, P, beta, sigma,
                            phi, theta, amin) for c in range(n_c)]
    return (np.stack([x["K"] for x in res]), np.stack([x["H"] for x in res]),
            np.array([x["status"] for x in res], np.int32),
            np.array([x["fail_t"] for x in res], np.int32))


def _solve_at(cal, phi, theta, r, wage, guess, egm_tol, max_iter):
    a, s, P = cal["a_grid"], cal["s"], cal["P"]
    R = corc.labor_egm_solve(guess, a, s, P, r, wage(r), cal["beta"], cal["sigma"], phi, theta,
                             cal["amin"], egm_tol, max_iter)
    uni = np.full((cal["N"], cal["Na"]), 1.0 / (cal["N"] * cal["Na"]))
    lam, _, _, _ = corc.dist_stationary(uni, a, P, kp=R["policy_k"], tol=1e-14, max_iter=100000)
    return R, lam, tr.capital_sum(lam, a), hours_sum(lam, R["policy_l"], s)


def steady_state_labor_cpu(cal, phi, theta, wage, r_low=0.02, r_high=0.041, steps=60,
                           egm_tol=1e-11, max_iter=5000, k_tol=1e-9):
    """The labour economy's stationary equilibrium from the C oracle, in
    transition.steady_state_labor's form: the root in r of K_s(r) − H(r)·(α/(r+δ))^(1/(1−α)) at
    w = wage(r), each rate's labour EGM solve and lottery histogram from the oracle.  The root is
    bracketed in [r_low, r_high] and found by false position with the Illinois halving (the excess
    is smooth and increasing: a handful of solves where bisection takes thirty)."""
    a, s = cal["a_grid"], cal["s"]
    alpha, delta = cal["alpha"], cal["delta"]
    r0 = 0.04
    guess = np.tile((1 + r0) * a + wage(r0) * np.mean(s), (cal["N"], 1))

    def excess(r):
        R, lam, K, H = _solve_at(cal, phi, theta, r, wage, guess, egm_tol, max_iter)
        return K - H * (alpha / (r + delta)) ** (1 / (1 - alpha)), (R, lam, K, H)
    lo, hi = r_low, r_high
    (flo, _), (fhi, _) = excess(lo), excess(hi)
    assert flo < 0 < fhi, (flo, fhi)
    side = 0
    for _ in range(steps):
        r = (lo * fhi - hi * flo) / (fhi - flo)
        ex, (R, lam, K, H) = excess(r)
        if abs(ex) <= k_tol:
            break
        if ex > 0:
            hi, fhi = r, ex
            flo = flo / 2 if side == 1 else flo
            side = 1
        else:
            lo, flo = r, ex
            fhi = fhi / 2 if side == -1 else fhi
            side = -1
    return dict(r=r, w=wage(r), K=K, H=H, policy_c=R["policy_c"], policy_l=R["policy_l"],
                policy_k=R["policy_k"], lam=lam, cal=cal, phi=phi, theta=theta)


def hours_news(H1, h):
    """F_H's first row: [n_in][T], (H1[x+1][T-1-s] - H1[0][T-1-s]) / h."""
    H1 = f64(H1)
    return (H1[1:, ::-1] - H1[:1, ::-1]) / h


def hours_F(G, H1, h):
    """F_H [n_in][T][T] from G = E^h·D^T [n_in][T][T] and H1 [n_in+1][T]: row 0 the one-step
    hours' differences, row t >= 1 = G's row t - 1."""
    G = f64(G)
    F = np.empty_like(G)
    F[:, 0, :] = hours_news(H1, h)
    F[:, 1:, :] = G[:, :-1, :]
    return F


def jacobian_labor_cpu(ss, T, h):
    """Steps 1-5 on the reference passes -> dict(J_Kr, J_Kw, J_Hr, J_Hw, F_Kr, F_Kw, F_Hr, F_Hw
    [T][T], E_a, E_h [T][N][Na], lam1, pk, pl [3][T][N][Na], H1 [3][T])."""
    cal = ss["cal"]
    a, s, P = cal["a_grid"], cal["s"], cal["P"]
    r, w = sr.news_paths(ss, T, h)
    B = [labor_backward(r[c], w[c], ss["policy_c"], a, s, P, cal["beta"], cal["sigma"], ss["phi"],
                        ss["theta"], cal["amin"]) for c in range(3)]
    assert all(b["status"] == 0 for b in B)
    pk, pl = np.stack([b["pk"] for b in B]), np.stack([b["pl"] for b in B])
    lam_ss = f64(ss["lam"])
    lam1 = np.stack([np.stack([corc.dist_update_lottery(lam_ss, pk[c, t], a, P) for t in range(T)])
                     for c in range(3)])
    H1 = np.array([[hours_sum(lam_ss, pl[c, t], s) for t in range(T)] for c in range(3)])
    E_a = sr.expect(pk[0, 0], np.tile(a, (cal["N"], 1)), a, P, T)
    E_h = sr.expect(pk[0, 0], f64(s)[:, None] * pl[0, 0], a, P, T)
    FK, JK = sr.fake_news(E_a, lam1, h)
    G, _ = sr.fake_news(E_h, lam1, h)
    FH = hours_F(G, H1, h)
    JH = sr.jacobian_from_F(FH)
    return dict(J_Kr=JK[0], J_Kw=JK[1], J_Hr=JH[0], J_Hw=JH[1], F_Kr=FK[0], F_Kw=FK[1],
                F_Hr=FH[0], F_Hw=FH[1], E_a=E_a, E_h=E_h, lam1=lam1, pk=pk, pl=pl, H1=H1)


def brute_force_labor_cpu(ss, T, h, which):
    """(J_K, J_H): J_K[t][s] = (K_{t+1}(x_s + h) − K_{t+1}(x))/h and J_H[t][s] = (H_t(x_s + h) −
    H_t(x))/h from 1 + T whole reference transitions; which: "r" or "w"."""
    cal = ss["cal"]
    args = (ss["policy_c"], ss["lam"], cal["a_grid"], cal["s"], cal["P"], cal["beta"], cal["sigma"],
            ss["phi"], ss["theta"], cal["amin"])
    r0, w0 = np.full(T + 1, float(ss["r"])), np.full(T, float(ss["w"]))
    base = labor_transition(r0, w0, *args)
    assert base["status"] == 0
    JK, JH = np.empty((T, T)), np.empty((T, T))
    for q in range(T):
        r, w = r0.copy(), w0.copy()
        (r if which == "r" else w)[q] += h
        R = labor_transition(r, w, *args)
        assert R["status"] == 0
        JK[:, q] = (R["K"][1:] - base["K"][1:]) / h
        JH[:, q] = (R["H"] - base["H"]) / h
    return JK, JH
