"""CPU reference of the estimation kernels (TEST INFRASTRUCTURE ONLY; not a test module).

Autocovariances and log-likelihood: tests/support/estimation_ref.c — ssj_loglik_batch_kernel
operation for operation — built into tests/support/libestimation_ref.so by
__graft_entry__.build(), or here with gcc when it is missing.  The MA coefficients and the
general-equilibrium Jacobians are numpy restatements (the product's summation order is the
device's own business: tests bound it, they do not restate it).  ma_batch and loglik_batch have
the package's signatures, so BACKEND drives estimation.ar1_loglik and ar1_mle without a GPU."""
from __future__ import annotations

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

from tests import transition_ref as tr

_HERE = Path(__file__).resolve().parent / "support"
SRC, LIB = _HERE / "estimation_ref.c", _HERE / "libestimation_ref.so"
_LIB = None

_i64, _P = C.c_int64, C.c_void_p


def f64(x):
    return np.ascontiguousarray(x, np.float64)


def build(force=False):
    if force or not LIB.exists() or LIB.stat().st_mtime < SRC.stat().st_mtime:
        subprocess.run(["gcc", *tr.CFLAGS, "-shared", "-o", str(LIB), str(SRC), "-lm"], check=True)
    return LIB


def lib():
    global _LIB
    if _LIB is None:
        L = C.CDLL(str(build()))
        L.eref_loglik.restype = C.c_int
        _LIB = L
    return _LIB


def _p(x):
    return None if x is None else x.ctypes.data_as(_P)


def ma_batch(G, dZ):
    """G [n_o][T][T], dZ [C][T] -> m [C][n_o][T] by numpy's matrix product."""
    G, dZ = f64(G), np.atleast_2d(f64(dZ))
    if G.ndim == 2:
        G = G[None]
    return f64(np.matmul(G[None], dZ[:, None, :, None])[..., 0])


def loglik_batch(m, y, me_var, want_gamma=False, want_d=False):
    """estimation.loglik_batch on the C reference, one candidate after another; y None: Gamma only
    (then me_var is the number of lags L)."""
    m = f64(m)
    if m.ndim == 2:
        m = m[None]
    n_c, n_o, T = m.shape
    if y is None:
        L, me = int(me_var), None
    else:
        y = f64(y).reshape(-1, n_o)
        L = y.shape[0]
        me = np.broadcast_to(f64(me_var), (n_c, n_o))
    ll = np.empty(n_c)
    st, fl = np.zeros(n_c, np.int32), np.zeros(n_c, np.int32)
    Gam = np.empty((n_c, L, n_o, n_o)) if (want_gamma or y is None) else None
    dd = np.empty((n_c, L * n_o)) if want_d else None
    for c in range(n_c):
        mec = None if me is None else f64(me[c])
        rc = lib().eref_loglik(_i64(n_o), _i64(T), _i64(L), _p(m[c]), _p(y), _p(mec),
                               _p(ll[c:c + 1]), _p(st[c:c + 1]), _p(fl[c:c + 1]),
                               _p(None if Gam is None else Gam[c]), _p(None if dd is None else dd[c]))
        assert rc == 0
    if y is None:
        return Gam
    out = dict(loglik=ll, status=st, fail=fl)
    if want_gamma:
        out["Gamma"] = Gam
    if want_d:
        out["d"] = dd
    return out


def autocovariance_batch(m, L):
    return loglik_batch(m, None, L)


BACKEND = (ma_batch, loglik_batch)


def dense_V(Gamma, me_var):
    """The full block-Toeplitz covariance [n][n] of Γ [L][n_o][n_o]: block (t, t') is Γ[t−t'] for
    t >= t' and Γ[t'−t]ᵀ above; me_var on the diagonal."""
    Gamma = f64(Gamma)
    L, n_o, _ = Gamma.shape
    V = np.empty((L * n_o, L * n_o))
    for t in range(L):
        for u in range(L):
            V[t * n_o:(t + 1) * n_o, u * n_o:(u + 1) * n_o] = (Gamma[t - u] if t >= u
                                                               else Gamma[u - t].T)
    return V + np.diag(np.tile(f64(me_var), L))


def dense_loglik(Gamma, y, me_var):
    """(loglik, logdet, quad, cond₂(V)) by numpy's slogdet and solve on the dense V."""
    V = dense_V(Gamma, me_var)
    yv = f64(y).ravel()
    sign, logdet = np.linalg.slogdet(V)
    assert sign > 0
    quad = float(yv @ np.linalg.solve(V, yv))
    n = yv.size
    return -0.5 * (n * np.log(2 * np.pi) + logdet + quad), float(logdet), quad, np.linalg.cond(V)


def ge_jacobians(pkg, ss, jac):
    """estimation.ge_jacobians restated from impulse_response's per-path solves: the T unit shocks
    one after another, then the definitions of r, w, Y and C on the paths.  Returns dict of
    [T][T] arrays, column s the response to a unit dZ_s."""
    T = np.shape(jac["J_r"])[0]
    alpha, delta = ss["cal"]["alpha"], ss["cal"]["delta"]
    I = np.eye(T)
    dK = pkg.impulse_response(ss, jac, I)        # [s][T+1]: dK_0 … dK_T
    r_K = (ss["r"] + delta) * (alpha - 1) / ss["K"]
    w_K = ss["w"] * alpha / ss["K"]
    Y_ss = (ss["r"] + delta) * ss["K"] / alpha
    K, Kn = dK[:, :T].T, dK[:, 1:].T
    Y = Y_ss * (I + alpha * K / ss["K"])
    return dict(K=K, r=r_K * K + (ss["r"] + delta) * I, w=w_K * K + ss["w"] * I, Y=Y,
                C=Y - Kn + (1 - delta) * K, K_next=Kn)


def simulate(m, L, me_var, seed):
    """L periods of the observables [L][n_o] from the MA coefficients m [n_o][T] with unit-variance
    Gaussian innovations, plus measurement error of variance me_var."""
    m = f64(m)
    n_o, T = m.shape
    rng = np.random.default_rng(seed)
    eps = rng.standard_normal(L + T - 1)
    y = np.stack([np.convolve(eps, m[o], mode="valid") for o in range(n_o)], axis=1)
    return y + rng.standard_normal((L, n_o)) * np.sqrt(f64(me_var))
