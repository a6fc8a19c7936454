"""CPU reference of the transition passes (TEST INFRASTRUCTURE ONLY; not a test module).

Backward: tests/support/transition_ref.c — orc_egm_step's operations with r split into r_next
and r_now — built into tests/support/libtransition_ref.so by __graft_entry__.build(), or here
with gcc when it is missing.  Forward: corc.dist_update_lottery chained in Python, with K = Σ λ·a
restated in the device's summation order (launch_dist_capital: 256 strided sums of 256 threads,
pairwise block fold, sequential fold of the block sums) so that drivers built on either backend
see the same bits.  Arrays are [N][Na] rows per (path, period), C-contiguous."""
from __future__ import annotations

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

from oracle import corc

_HERE = Path(__file__).resolve().parent / "support"
SRC, LIB = _HERE / "transition_ref.c", _HERE / "libtransition_ref.so"
# oracle/Makefile's floating-point flags
CFLAGS = ["-O2", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wextra"]
_LIB = None

_d, _i64, _P = C.c_double, C.c_int64, C.c_void_p


def build(force=False):
    if force or not LIB.exists() or LIB.stat().st_mtime < SRC.stat().st_mtime:
        subprocess.run(["gcc", *CFLAGS, "-shared", "-o", str(LIB), str(SRC), "-lm"], check=True)
    return LIB


def lib():
    global _LIB
    if _LIB is None:
        L = C.CDLL(str(build()))
        L.tref_egm_step2.restype = C.c_int
        L.tref_egm_backward.restype = C.c_int
        _LIB = L
    return _LIB


def _p(x):
    return None if x is None else x.ctypes.data_as(_P)


f64 = corc.f64


def egm_step2(pc_next, a, s, P, r_next, r_now, w_now, beta, sigma, amin):
    """One two-rate step -> (pc_now, pk_now, ahat, bad)."""
    pc_next, a, s, P = map(f64, (pc_next, a, s, P))
    N, Na = pc_next.shape
    pc, pk, ah = np.empty((N, Na)), np.empty((N, Na)), np.empty((N, Na))
    bad = lib().tref_egm_step2(_i64(N), _i64(Na), _p(pc_next), _p(a), _p(s), _p(P), _d(r_next),
                               _d(r_now), _d(w_now), _d(beta), _d(sigma), _d(amin), _p(pc), _p(pk),
                               _p(ah))
    assert bad in (0, 1)
    return pc, pk, ah, bad


def egm_backward(r, w, pc_T, a, s, P, beta, sigma, amin):
    """One path: r [T+1], w [T], pc_T [N][Na] -> dict(pk, pc [T][N][Na], status, fail_t).
    Periods below fail_t are NaN."""
    r, w, pc_T, a, s, P = map(f64, (r, w, pc_T, a, s, P))
    T = w.size
    assert r.size == T + 1
    N, Na = pc_T.shape
    pk, pc = np.full((T, N, Na), np.nan), np.full((T, N, Na), np.nan)
    st, ft = C.c_int32(), C.c_int32()
    rc = lib().tref_egm_backward(_i64(N), _i64(Na), _i64(T), _p(r), _p(w), _p(pc_T), _p(a), _p(s),
                                 _p(P), _d(beta), _d(sigma), _d(amin), _p(pk), _p(pc),
                                 C.byref(st), C.byref(ft))
    assert rc == 0
    return dict(pk=pk, pc=pc, status=st.value, fail_t=ft.value)


def capital_sum(lam, a):
    """Σ λ·a in launch_dist_capital's order (N·Na <= 65,536: one term per thread)."""
    lam, a = f64(lam), f64(a)
    n = lam.size
    assert n <= 65536
    x = 0.0 + lam.ravel() * np.tile(a, lam.shape[0])
    nb = -(-n // 256)
    blk = np.zeros(nb * 256)
    blk[:n] = x
    blk = blk.reshape(nb, 256)
    s = 128
    while s > 0:
        blk[:, :s] = blk[:, :s] + blk[:, s:2 * s]
        s >>= 1
    acc = 0.0
    for q in range(nb):
        acc = acc + blk[q, 0]
    return float(acc)


def lottery_keys(kp, a):
    """dist_keys_kernel's keys of an off-grid policy [N][Na]."""
    x = np.minimum(np.maximum(f64(kp), a[0]), a[-1])
    return np.clip(np.searchsorted(a, x, side="right") - 1, 0, a.size - 2)


def dist_forward(pk, lam0, a, P):
    """One path: pk [T][N][Na], lam0 [N][Na] -> dict(lam [T+1][N][Na], K [T+1], status, fail_t).
    A period whose keys are not monotone stops the path (status 2): K beyond it is NaN."""
    pk, lam0, a, P = map(f64, (pk, lam0, a, P))
    T = pk.shape[0]
    lam = [lam0]
    K = np.full(T + 1, np.nan)
    status, fail_t = 0, -1
    for t in range(T):
        K[t] = capital_sum(lam[-1], a)
        if (np.diff(lottery_keys(pk[t], a), axis=1) < 0).any():
            status, fail_t = 2, t
            break
        lam.append(corc.dist_update_lottery(lam[-1], pk[t], a, P))
    if status == 0:
        K[T] = capital_sum(lam[-1], a)
    return dict(lam=np.stack(lam), K=K, status=status, fail_t=fail_t)


def transition(r, w, pc_T, lam0, a, s, P, beta, sigma, amin):
    """One path through both passes -> dict(K [T+1], status, fail_t, pk, lam)."""
    B = egm_backward(r, w, pc_T, a, s, P, beta, sigma, amin)
    if B["status"]:
        return dict(K=np.full(len(w) + 1, np.nan), status=B["status"], fail_t=B["fail_t"],
                    pk=B["pk"], lam=None)
    F = dist_forward(B["pk"], lam0, a, P)
    return dict(K=F["K"], status=F["status"], fail_t=F["fail_t"], pk=B["pk"], lam=F["lam"])


def transition_batch(r, w, pc_T, lam0, a_grid, s, P, beta, sigma, amin):
    """The CPU stand-in for transition.transition_batch (same arguments and results): pc_T and
    lam0 [N][Na] shared or [C][N][Na]."""
    r, w = np.atleast_2d(f64(r)), np.atleast_2d(f64(w))
    n_c = r.shape[0]
    pc_T, lam0 = f64(pc_T), f64(lam0)
    pick = lambda x, c: x if x.ndim == 2 else x[c]
    res = [transition(r[c], w[c], pick(pc_T, c), pick(lam0, c), a_grid, s, P, beta, sigma, amin)
           for c in range(n_c)]
    return (np.stack([x["K"] for x in res]), np.array([x["status"] for x in res], np.int32),
            np.array([x["fail_t"] for x in res], np.int32))


def steady_state_cpu(cal, r, wage, egm_tol=1e-11, max_iter=5000):
    """A stationary point at rate r from the C oracle, in transition.steady_state's form: the
    EGM solve at (r, wage(r)), its lottery histogram and K = the histogram's capital.  (No
    market clearing: prices_from_K anchors the paths to whatever point it is given.)"""
    a, s, P = cal["a_grid"], cal["s"], cal["P"]
    w = wage(r)
    guess = np.tile((1 + r) * a + w * np.mean(s), (cal["N"], 1))
    R = corc.egm_solve(guess, a, s, P, r, w, cal["beta"], cal["sigma"], cal["amin"], egm_tol,
                       max_iter)
    uni = np.full((cal["N"], cal["Na"]), 1.0 / (cal["N"] * cal["Na"]))
    lam, _, _, _ = corc.dist_stationary(uni, a, P, kp=R["policy_k"], tol=1e-14, max_iter=100000)
    return dict(r=r, w=w, K=capital_sum(lam, a), policy_c=R["policy_c"], lam=lam, cal=cal)
