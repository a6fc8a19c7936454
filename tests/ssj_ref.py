"""CPU reference of the sequence-space Jacobian (TEST INFRASTRUCTURE ONLY; not a test module).

Expectation vectors: tests/support/ssj_ref.c — dist_expect_batch_kernel operation for operation —
built into tests/support/libssj_ref.so by __graft_entry__.build(), or here with gcc when it is
missing.  The fake-news matrices and the Jacobians are numpy restatements (the contraction's
summation order is the device's own business: tests bound it, they do not restate it).
jacobian_cpu composes the five steps from tests/transition_ref.py's passes; brute_force_cpu is the
one-sided difference of 1 + T whole transitions.  Arrays are [N][Na] rows per block."""
from __future__ import annotations

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

from oracle import corc
from tests import transition_ref as tr

_HERE = Path(__file__).resolve().parent / "support"
SRC, LIB = _HERE / "ssj_ref.c", _HERE / "libssj_ref.so"
_LIB = None

_i64, _P = C.c_int64, C.c_void_p
f64 = corc.f64


def build(force=False):
    if force or not LIB.exists() or LIB.stat().st_mtime < SRC.stat().st_mtime:
        subprocess.run(["gcc", *tr.CFLAGS, "-shared", "-o", str(LIB), str(SRC), "-lm"], check=True)
    return LIB


def lib():
    global _LIB
    if _LIB is None:
        L = C.CDLL(str(build()))
        L.sref_expect.restype = C.c_int
        _LIB = L
    return _LIB


def _p(x):
    return None if x is None else x.ctypes.data_as(_P)


def expect(policy, y0, a, P, T, plan=False):
    """policy, y0 [N][Na], P [N][N] -> E [T][N][Na] (and lo, wl [N][Na] when plan)."""
    policy, y0, a, P = map(f64, (policy, y0, a, P))
    N, Na = policy.shape
    assert y0.shape == (N, Na) and a.shape == (Na,) and P.shape == (N, N) and T >= 1
    E = np.empty((T, N, Na))
    lo, wl = np.empty((N, Na), np.int64), np.empty((N, Na))
    rc = lib().sref_expect(_i64(N), _i64(Na), _i64(T), _p(policy), _p(y0), _p(a), _p(P), _p(E),
                           _p(lo), _p(wl))
    assert rc == 0
    return (E, lo, wl) if plan else E


def news_rows(lam1, h):
    """D [n_in][T][n]: D[x][s] = (lam1[x+1][T-1-s] - lam1[0][T-1-s]) / h."""
    lam1 = f64(lam1)
    T = lam1.shape[1]
    L = lam1.reshape(lam1.shape[0], T, -1)
    return (L[1:, ::-1] - L[:1, ::-1]) / h


def jacobian_from_F(F):
    """J[t][s] = F[t][s] + J[t-1][s-1], t ascending along each diagonal."""
    J = f64(F).copy()
    for t in range(1, J.shape[-2]):
        J[..., t, 1:] = J[..., t, 1:] + J[..., t - 1, :-1]
    return J


def fake_news(E, lam1, h):
    """E [T][...], lam1 [n_in+1][T][...] -> (F, J) [n_in][T][T], F by numpy's matrix product."""
    E = f64(E)
    T = E.shape[0]
    D = news_rows(lam1, h)
    F = np.stack([E.reshape(T, -1) @ D[x].T for x in range(D.shape[0])])
    return F, jacobian_from_F(F)


def news_paths(ss, T, h):
    """The three price paths of step 1: r [3][T+1], w [3][T]."""
    r, w = np.full((3, T + 1), float(ss["r"])), np.full((3, T), float(ss["w"]))
    r[1, T - 1] = float(ss["r"]) + h
    w[2, T - 1] = float(ss["w"]) + h
    return r, w


def jacobian_cpu(ss, T, h):
    """Steps 1-5 on the reference passes -> dict(J_r, J_w, F_r, F_w [T][T], E [T][N][Na],
    lam1 [3][T][N][Na], pk [3][T][N][Na])."""
    cal = ss["cal"]
    a, s, P = cal["a_grid"], cal["s"], cal["P"]
    r, w = news_paths(ss, T, h)
    B = [tr.egm_backward(r[c], w[c], ss["policy_c"], a, s, P, cal["beta"], cal["sigma"],
                         cal["amin"]) for c in range(3)]
    assert all(b["status"] == 0 for b in B)
    pk = np.stack([b["pk"] for b in B])
    lam1 = np.stack([np.stack([corc.dist_update_lottery(f64(ss["lam"]), pk[c, t], a, P)
                               for t in range(T)]) for c in range(3)])
    E = expect(pk[0, 0], np.tile(a, (cal["N"], 1)), a, P, T)
    F, J = fake_news(E, lam1, h)
    return dict(J_r=J[0], J_w=J[1], F_r=F[0], F_w=F[1], E=E, lam1=lam1, pk=pk)


def brute_force_cpu(ss, T, h, which):
    """J[t][s] = (K_{t+1}(x_s + h) - K_{t+1}(x)) / h from 1 + T whole reference transitions;
    which: "r" or "w"."""
    cal = ss["cal"]
    args = (ss["policy_c"], ss["lam"], cal["a_grid"], cal["s"], cal["P"], cal["beta"], cal["sigma"],
            cal["amin"])
    r0, w0 = np.full(T + 1, float(ss["r"])), np.full(T, float(ss["w"]))
    base = tr.transition(r0, w0, *args)
    assert base["status"] == 0
    J = np.empty((T, T))
    for s in range(T):
        r, w = r0.copy(), w0.copy()
        (r if which == "r" else w)[s] += h
        R = tr.transition(r, w, *args)
        assert R["status"] == 0
        J[:, s] = (R["K"][1:] - base["K"][1:]) / h
    return J
