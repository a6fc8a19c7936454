"""A6/A7 — Krusell-Smith VFI pieces through the C ABI (Krusell_Smith_VFI.m:143-204).
value / k_opt are k x K x S arrays exactly as in the script (column-major on the boundary)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._capi import check, d, i64, ip, lib, ptr

PARAM_ORDER = ("beta", "alpha", "delta", "k_min", "k_max", "ug", "ub", "l_bar", "mu")


def ks_params(beta=0.99, alpha=0.36, delta=0.025, k_min=0.0001, k_max=1000.0, ug=0.04, ub=0.10,
              mu=0.0, z_grid=(1.01, 0.99), eps_grid=(1.0, 0.0), l_bar=None):
    """The 13-double parameter block (Krusell_Smith_VFI.m:5-13)."""
    if l_bar is None:
        l_bar = 1 / (1 - ub)
    return np.array([beta, alpha, delta, k_min, k_max, ug, ub, l_bar, mu, z_grid[0], z_grid[1],
                     eps_grid[0], eps_grid[1]], dtype=np.float64)


def _arrs(k_grid, K_grid, B, P, params):
    return (np.ascontiguousarray(k_grid, np.float64), np.ascontiguousarray(K_grid, np.float64),
            np.ascontiguousarray(B, np.float64), np.asfortranarray(P, dtype=np.float64),
            np.ascontiguousarray(params, np.float64))


def ks_policy_improve(value, k_grid, K_grid, B, P, params):
    """Replaces :149-168 → (k_opt, nfev)."""
    V = np.asfortranarray(value, dtype=np.float64)
    nk, nK, nS = V.shape
    kg, Kg, B, P, prm = _arrs(k_grid, K_grid, B, P, params)
    k_opt = np.empty_like(V, order="F")
    nfev = np.empty(V.shape, np.int32, order="F")
    check(lib().ks_policy_improve(ptr(V), ptr(kg), ptr(Kg), ptr(B), ptr(P), ptr(prm), i64(nk),
                                  i64(nK), ptr(k_opt), ptr(nfev)))
    return k_opt, nfev


def ks_howard(value, k_opt, k_grid, K_grid, B, P, params, steps=50):
    """Replaces :172-192 (Jacobi Howard sweeps with pchip refresh)."""
    V = np.array(value, dtype=np.float64, order="F", copy=True)
    nk, nK, nS = V.shape
    kg, Kg, B, P, prm = _arrs(k_grid, K_grid, B, P, params)
    ko = np.asfortranarray(k_opt, dtype=np.float64)
    check(lib().ks_howard(ptr(V), ptr(ko), ptr(kg), ptr(Kg), ptr(B), ptr(P), ptr(prm), i64(nk),
                          i64(nK), i64(steps)))
    return V


def ks_vfi_solve(value, k_opt, k_grid, K_grid, B, P, params, howard_steps=50, tol=1e-6,
                 max_vfi=10000, n_devices=1, depth=None):
    """Replaces the VFI loop :143-204 for one ALM coefficient vector B.  n_devices > 1: the
    in-process (K, Z)-sliced solve (ks_vfi_solve_sharded), `depth` Howard sweeps per exchange
    (default 4)."""
    V = np.array(value, dtype=np.float64, order="F", copy=True)
    ko = np.array(k_opt, dtype=np.float64, order="F", copy=True)
    nk, nK, nS = V.shape
    kg, Kg, B, P, prm = _arrs(k_grid, K_grid, B, P, params)
    it, rel = C.c_int64(), C.c_double()
    if depth is not None:
        check(lib().ks_vfi_solve_sharded(ptr(V), ptr(ko), ptr(kg), ptr(Kg), ptr(B), ptr(P),
                                         ptr(prm), i64(nk), i64(nK), i64(howard_steps), d(tol),
                                         i64(max_vfi), ip(n_devices), ip(depth), C.byref(it),
                                         C.byref(rel)))
    else:
        check(lib().ks_vfi_solve(ptr(V), ptr(ko), ptr(kg), ptr(Kg), ptr(B), ptr(P), ptr(prm),
                                 i64(nk), i64(nK), i64(howard_steps), d(tol), i64(max_vfi),
                                 ip(n_devices), C.byref(it), C.byref(rel)))
    return dict(value=V, k_opt=ko, iters=it.value, rel_diff=rel.value)


def ks_egm_solve(k_opt, k_grid, K_grid, B, P, params, tol=1e-6, max_iter=10000, jacobi=False):
    """A8 — replaces the EGM loop of Krusell_Smith_EGM.m:130-209 for one ALM vector B
    (Gauss-Seidel over (s, K) as the script).  jacobi=True: the F1 Jacobi variant
    (ks_egm_solve_jacobi — NOT the reference's result, all pairs of a sweep in parallel).
    Returns dict(k_opt, iters, diff)."""
    ko = np.array(k_opt, dtype=np.float64, order="F", copy=True)
    nk, nK, nS = ko.shape
    kg, Kg, B, P, prm = _arrs(k_grid, K_grid, B, P, params)
    it, diff = C.c_int64(), C.c_double()
    fn = lib().ks_egm_solve_jacobi if jacobi else lib().ks_egm_solve
    check(fn(ptr(ko), ptr(kg), ptr(Kg), ptr(B), ptr(P), ptr(prm), i64(nk), i64(nK), d(tol),
             i64(max_iter), C.byref(it), C.byref(diff)))
    return dict(k_opt=ko, iters=it.value, diff=diff.value)


def _per_candidate(x, C_, tail, name):
    """x as a C-contiguous (C, *tail) float64 array; a single candidate's block broadcasts."""
    a = np.asarray(x, np.float64)
    if a.shape == tuple(tail):
        a = np.broadcast_to(a, (C_,) + tuple(tail))
    if a.shape != (C_,) + tuple(tail):
        raise ValueError(f"{name} must be {tuple(tail)} or ({C_},) + {tuple(tail)}, "
                         f"got {a.shape}")
    return np.ascontiguousarray(a)


def egm_batch_inputs(C_, nK, K_grid, B, P, params):
    """The candidate-major host arrays of the batched solve: K_grid (C, nK), B (C, 4), P (C, 4, 4)
    with each block in MATLAB's column-major order, params (C, 13).  Shared inputs broadcast."""
    Kg = _per_candidate(K_grid, C_, (nK,), "K_grid")
    Bc = _per_candidate(B, C_, (4,), "B")
    Pc = _per_candidate(P, C_, (4, 4), "P")
    Pc = np.ascontiguousarray(Pc.transpose(0, 2, 1))   # each block column-major
    prm = _per_candidate(params, C_, (13,), "params")
    return Kg, Bc, Pc, prm


def ks_egm_solve_batch(k_opt, k_grid, K_grid, B, P, params, tol=1e-6, max_iter=10000):
    """A8 at C candidate economies in one launch (ks_egm_solve_batch): k_opt (C, nk, nK, 4),
    K_grid (C, nK), B (C, 4), P (C, 4, 4), params (C, 13); a shared K_grid, B, P or params (one
    candidate's shape) broadcasts.  Returns dict(k_opt (C, nk, nK, 4), iters (C,), diff (C,),
    status (C,)): status 1 marks a candidate that met fewer than two valid EGM points (its k_opt
    is unspecified); every other candidate equals its own ks_egm_solve bit for bit."""
    ko = np.asarray(k_opt, np.float64)
    if ko.ndim != 4 or ko.shape[3] != 4:
        raise ValueError("k_opt must be (C, k_size, K_size, 4)")
    C_, nk, nK, _ = ko.shape
    kg = np.ascontiguousarray(k_grid, np.float64)
    if kg.shape != (nk,):
        raise ValueError("k_opt must be (C, numel(k_grid), K_size, 4)")
    Kg, Bc, Pc, prm = egm_batch_inputs(C_, nK, K_grid, B, P, params)
    # candidate-major, each block k x K x 4 column-major = [4][nK][nk] row-major
    kd = np.ascontiguousarray(ko.transpose(0, 3, 2, 1))
    iters = np.zeros(C_, np.int64)
    diff = np.zeros(C_)
    status = np.zeros(C_, np.int32)
    check(lib().ks_egm_solve_batch(i64(C_), ptr(kd), ptr(kg), ptr(Kg), ptr(Bc), ptr(Pc), ptr(prm),
                                   i64(nk), i64(nK), d(tol), i64(max_iter), ptr(iters), ptr(diff),
                                   ptr(status)))
    return dict(k_opt=kd.transpose(0, 3, 2, 1), iters=iters, diff=diff, status=status)


def ks_egm_solve_batch_dev(k_opt, k_grid, K_grid, B, P, params, tol=1e-6, max_iter=10000,
                           out=None, scratch=None, stream=None):
    """Device tier of ks_egm_solve_batch: k_opt a device tensor [C][4][nK][nk] (in/out), k_grid a
    device tensor; K_grid, B, P, params host arrays as in ks_egm_solve_batch.  `out` = (iters
    int64, diff float64, status int32) device tensors [C] and `scratch` a device byte tensor of
    ks_egm_batch_scratch_bytes(C, nK) are allocated when None.  Asynchronous on `stream` after the
    table upload; returns (iters, diff, status, scratch)."""
    import torch
    from ._capi import stream_handle
    C_, nS, nK, nk = k_opt.shape
    if nS != 4 or k_grid.numel() != nk:
        raise ValueError("k_opt must be [C][4][K_size][numel(k_grid)]")
    if not k_opt.is_contiguous():
        raise ValueError("k_opt must be a contiguous tensor")
    Kg, Bc, Pc, prm = egm_batch_inputs(C_, nK, K_grid, B, P, params)
    dev = k_opt.device
    lib().ks_egm_batch_scratch_bytes.restype = C.c_int64
    need = int(lib().ks_egm_batch_scratch_bytes(i64(C_), i64(nK)))
    if scratch is None:
        scratch = torch.empty(need, dtype=torch.uint8, device=dev)
    if scratch.numel() < need:
        raise ValueError(f"scratch holds {scratch.numel()} bytes, the call needs {need}")
    if out is None:
        out = (torch.zeros(C_, dtype=torch.int64, device=dev),
               torch.zeros(C_, dtype=torch.float64, device=dev),
               torch.zeros(C_, dtype=torch.int32, device=dev))
    iters, diff, status = out
    check(lib().ks_egm_solve_batch_dev(i64(C_), ptr(k_opt), ptr(k_grid), ptr(Kg), ptr(Bc), ptr(Pc),
                                       ptr(prm), i64(nk), i64(nK), d(tol), i64(max_iter),
                                       ptr(iters), ptr(diff), ptr(status), ptr(scratch),
                                       stream_handle(stream)))
    return iters, diff, status, scratch


def ks_vfi_solve_batch(value, k_opt, k_grid, K_grid, B, P, params, howard_steps=50, tol=1e-6,
                       max_vfi=10000):
    """A6/A7 at C candidate economies in one launch (ks_vfi_solve_batch): value and k_opt
    (C, nk, nK, 4), K_grid (C, nK), B (C, 4), P (C, 4, 4), params (C, 13); a shared K_grid, B, P
    or params (one candidate's shape) broadcasts.  Returns dict(value, k_opt (C, nk, nK, 4),
    iters (C,), rel_diff (C,)); every candidate equals its own ks_vfi_solve bit for bit.  Sizes
    past the one-workgroup rule (nk * nK * 4 <= 4,096) are refused: there is no tiled batch."""
    V = np.asarray(value, np.float64)
    ko = np.asarray(k_opt, np.float64)
    if V.ndim != 4 or V.shape[3] != 4:
        raise ValueError("value must be (C, k_size, K_size, 4)")
    if ko.shape != V.shape:
        raise ValueError("k_opt must have value's shape (C, k_size, K_size, 4)")
    C_, nk, nK, _ = V.shape
    kg = np.ascontiguousarray(k_grid, np.float64)
    if kg.shape != (nk,):
        raise ValueError("value must be (C, numel(k_grid), K_size, 4)")
    Kg, Bc, Pc, prm = egm_batch_inputs(C_, nK, K_grid, B, P, params)
    # candidate-major, each block k x K x 4 column-major = [4][nK][nk] row-major
    Vd = np.ascontiguousarray(V.transpose(0, 3, 2, 1))
    kd = np.ascontiguousarray(ko.transpose(0, 3, 2, 1))
    iters = np.zeros(C_, np.int64)
    rel = np.zeros(C_)
    check(lib().ks_vfi_solve_batch(i64(C_), ptr(Vd), ptr(kd), ptr(kg), ptr(Kg), ptr(Bc), ptr(Pc),
                                   ptr(prm), i64(nk), i64(nK), i64(howard_steps), d(tol),
                                   i64(max_vfi), ptr(iters), ptr(rel)))
    return dict(value=Vd.transpose(0, 3, 2, 1), k_opt=kd.transpose(0, 3, 2, 1), iters=iters,
                rel_diff=rel)


def ks_vfi_solve_batch_dev(value, k_opt, k_grid, K_grid, B, P, params, howard_steps=50, tol=1e-6,
                           max_vfi=10000, out=None, scratch=None, stream=None):
    """Device tier of ks_vfi_solve_batch: value and k_opt device tensors [C][4][nK][nk] (in/out),
    k_grid a device tensor; K_grid, B, P, params host arrays as in ks_vfi_solve_batch.  `out` =
    (iters int64, rel_diff float64) device tensors [C] and `scratch` a device byte tensor of
    ks_vfi_batch_scratch_bytes(C, nK) are allocated when None.  value must hold no ±inf (NaN is
    accepted) and k_grid must increase strictly: the caller's preconditions.  Asynchronous on
    `stream` after the table upload; returns (iters, rel_diff, scratch)."""
    import torch
    from ._capi import stream_handle
    C_, nS, nK, nk = value.shape
    if nS != 4 or k_grid.numel() != nk:
        raise ValueError("value must be [C][4][K_size][numel(k_grid)]")
    if tuple(k_opt.shape) != tuple(value.shape):
        raise ValueError("k_opt must have value's shape")
    if not (value.is_contiguous() and k_opt.is_contiguous()):
        raise ValueError("value and k_opt must be contiguous tensors")
    Kg, Bc, Pc, prm = egm_batch_inputs(C_, nK, K_grid, B, P, params)
    dev = value.device
    lib().ks_vfi_batch_scratch_bytes.restype = C.c_int64
    need = int(lib().ks_vfi_batch_scratch_bytes(i64(C_), i64(nK)))
    if scratch is None:
        scratch = torch.empty(need, dtype=torch.uint8, device=dev)
    if scratch.numel() < need:
        raise ValueError(f"scratch holds {scratch.numel()} bytes, the call needs {need}")
    if out is None:
        out = (torch.zeros(C_, dtype=torch.int64, device=dev),
               torch.zeros(C_, dtype=torch.float64, device=dev))
    iters, rel = out
    check(lib().ks_vfi_solve_batch_dev(i64(C_), ptr(value), ptr(k_opt), ptr(k_grid), ptr(Kg),
                                       ptr(Bc), ptr(Pc), ptr(prm), i64(nk), i64(nK),
                                       i64(howard_steps), d(tol), i64(max_vfi), ptr(iters),
                                       ptr(rel), ptr(scratch), stream_handle(stream)))
    return iters, rel, scratch
