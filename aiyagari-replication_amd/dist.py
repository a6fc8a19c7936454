"""A10 (new component) — stationary distribution by histogram iteration on the GPU."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._capi import check, d, i64, ip, lib, ptr, stream_handle


def dist_stationary(a_grid, P, policy_idx=None, policy_k=None, lam0=None, tol=1e-12,
                    max_iter=10000, vfi_layout=True):
    """Iterate λ' = Pᵀ·push(λ) to a fixed point.  policy_idx: on-grid (1-based, as idx from
    Aiyagari_VFI.m:79); policy_k: off-grid (EGM) policy, mass split between bracketing nodes.
    Layout N x Na (vfi_layout) or Na x N.  Returns (lambda, K = Σ λ·a, iters, dist)."""
    a = np.ascontiguousarray(a_grid, np.float64)
    P = np.asfortranarray(P, dtype=np.float64)
    pol = policy_idx if policy_idx is not None else policy_k
    shape = np.shape(pol)
    N, Na = shape if vfi_layout else shape[::-1]
    lam = (np.full(shape, 1.0 / (N * Na)) if lam0 is None else np.array(lam0, np.float64))
    lam = np.asfortranarray(lam)
    idx = np.asfortranarray(policy_idx, np.int32) if policy_idx is not None else None
    kp = np.asfortranarray(policy_k, np.float64) if policy_idx is None else None
    K, it, dist = C.c_double(), C.c_int64(), C.c_double()
    check(lib().aiy_dist_stationary(ptr(idx), ptr(kp), ip(1 if vfi_layout else 0), ptr(a), ptr(P),
                                    i64(N), i64(Na), d(tol), i64(max_iter), ptr(lam),
                                    C.byref(K), C.byref(it), C.byref(dist)))
    return lam, K.value, it.value, dist.value


def dist_update_dev(ws, lam, a_grid, P, out, policy_idx=None, policy_k=None, diff=None,
                    stream=None):
    """One histogram push on device ([N][Na] torch tensors; policy_idx 0-based)."""
    check(lib().aiy_dist_update_dev(ws.handle, ptr(lam), ptr(policy_idx), ptr(policy_k),
                                    ptr(a_grid), ptr(P), ptr(out), ptr(diff),
                                    stream_handle(stream)))


def dist_stationary_dev(ws, lam0, a_grid, P, out, policy_idx=None, policy_k=None, tol=1e-12,
                        max_iter=10000, k_supply=None, stream=None):
    """aiy_dist_stationary_dev: the fixed point on device ([N][Na] torch tensors; policy_idx
    0-based).  `out` receives λ; k_supply (optional 1-element device tensor) Σ λ·a.
    Returns (iters, dist)."""
    it, dist = C.c_int64(), C.c_double()
    check(lib().aiy_dist_stationary_dev(ws.handle, ptr(lam0), ptr(policy_idx), ptr(policy_k),
                                        ptr(a_grid), ptr(P), d(tol), i64(max_iter), ptr(out),
                                        ptr(k_supply), C.byref(it), C.byref(dist),
                                        stream_handle(stream)))
    return it.value, dist.value


def dist_stationary_batch(a_grid, P, policy_idx=None, policy_k=None, lam0=None, tol=1e-12,
                          max_iter=10000, vfi_layout=True):
    """aiy_dist_stationary_batch: the fixed points of C policies at once.  policy_idx (1-based)
    or policy_k: [C] stacked arrays, each N x Na (vfi_layout) or Na x N; lam0 likewise (None:
    uniform).  Returns (lambda [C]..., K [C], iters [C], dist [C]), each candidate's equal to
    dist_stationary's."""
    a = np.ascontiguousarray(a_grid, np.float64)
    P = np.asfortranarray(P, dtype=np.float64)
    pol = np.asarray(policy_idx if policy_idx is not None else policy_k)
    if pol.ndim != 3:
        raise ValueError("policies must be stacked [C] x (N x Na | Na x N)")
    n_c, shape = pol.shape[0], pol.shape[1:]
    N, Na = shape if vfi_layout else shape[::-1]
    fo = lambda x, dt: np.ascontiguousarray(np.stack([np.asfortranarray(y, dtype=dt).ravel("F")
                                                      for y in x]))
    lam = (np.full((n_c,) + shape, 1.0 / (N * Na)) if lam0 is None else np.asarray(lam0, np.float64))
    if lam.shape != pol.shape:
        raise ValueError(f"lam0 must have the policies' shape {pol.shape}")
    lam = fo(lam, np.float64)
    idx = fo(pol, np.int32) if policy_idx is not None else None
    kp = fo(pol, np.float64) if policy_idx is None else None
    K, it, dist = np.empty(n_c), np.empty(n_c, np.int64), np.empty(n_c)
    check(lib().aiy_dist_stationary_batch(i64(n_c), ptr(idx), ptr(kp), ip(1 if vfi_layout else 0),
                                          ptr(a), ptr(P), i64(N), i64(Na), d(tol), i64(max_iter),
                                          ptr(lam), ptr(K), ptr(it), ptr(dist)))
    out = np.stack([lam[c].reshape(shape, order="F") for c in range(n_c)])
    return out, K, it, dist


def dist_stationary_batch_dev(ws, lam0, a_grid, P, out, policy_idx=None, policy_k=None, tol=1e-12,
                              max_iter=10000, k_supply=None, stream=None):
    """aiy_dist_stationary_batch_dev: C fixed points on device ([C][N][Na] torch tensors;
    policy_idx 0-based int32).  `out` receives the C lambdas; k_supply (optional [C] device
    tensor) the C sums of lambda * a.  Returns (iters [C], dist [C]) as numpy arrays."""
    n_c = int(lam0.shape[0])
    it, dist = np.empty(n_c, np.int64), np.empty(n_c)
    check(lib().aiy_dist_stationary_batch_dev(ws.handle, i64(n_c), ptr(lam0), ptr(policy_idx),
                                              ptr(policy_k), ptr(a_grid), ptr(P), d(tol),
                                              i64(max_iter), ptr(out), ptr(k_supply), ptr(it),
                                              ptr(dist), stream_handle(stream)))
    return it, dist
