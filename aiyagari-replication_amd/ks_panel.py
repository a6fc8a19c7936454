"""F3 / F2 — the Krusell-Smith shock panel (Krusell_Smith_VFI.m:57-94) and the agent-panel
capital simulation (:206-248) through the C ABI, plus the script's outer ALM loop
(:138-296) driven from the host: VFI solve (A6/A7 on the GPU) -> panel simulation (GPU) ->
OLS of the law of motion (host, 4 numbers) -> damped B update.

The uniforms are MATLAB's `rand` stream in the script's draw order; `matlab_rand` gives the
fresh-session stream (MT19937 seed 5489, 53-bit doubles — numpy's RandomState implements the
same generator)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import calibration
from ._capi import check, i64, lib, ptr, stream_handle
from .ge import matlab_rand  # noqa: F401  (the fresh-session stream; exported from here too)
from .ks import (_per_candidate, ks_egm_solve, ks_egm_solve_batch_dev, ks_params, ks_vfi_solve,
                 ks_vfi_solve_batch_dev)


def shock_draws(T: int, population: int) -> int:
    """Uniforms consumed by :57-94: T-1 aggregate, `population` initial, (T-1)*population."""
    return (T - 1) + population + (T - 1) * population


def ks_shocks(T, population, uniforms, params):
    """Replaces :57-94.  Returns zi_shock (T,) in {0 good, 1 bad} (after :68) and epsi_shock
    (T, population) in {1 employed, 2 unemployed}, as the script holds them."""
    U = np.ascontiguousarray(uniforms, np.float64)
    if U.size != shock_draws(T, population):
        raise ValueError(f"need {shock_draws(T, population)} uniforms, got {U.size}")
    prm = np.ascontiguousarray(params, np.float64)
    zi = np.empty(T)
    eps = np.empty((T, population), order="F")
    check(lib().ks_shocks(i64(T), i64(population), ptr(U), ptr(prm), ptr(zi), ptr(eps)))
    return zi, eps


def ks_simulate_capital(k_opt, k_grid, K_grid, zi_shock, epsi_shock, k_population):
    """Replaces :206-248.  k_opt k x K x 4; returns (K_ts (T,), k_population (pop,))."""
    ko = np.asfortranarray(k_opt, dtype=np.float64)
    nk, nK, nS = ko.shape
    if nS != 4:
        raise ValueError("k_opt must be k x K x 4")
    kg = np.ascontiguousarray(k_grid, np.float64)
    Kg = np.ascontiguousarray(K_grid, np.float64)
    zi = np.ascontiguousarray(zi_shock, np.float64)
    eps = np.asfortranarray(epsi_shock, dtype=np.float64)
    T, pop = eps.shape
    kp = np.array(k_population, dtype=np.float64, copy=True)
    K_ts = np.empty(T)
    check(lib().ks_simulate_capital(ptr(ko), ptr(kg), ptr(Kg), i64(nk), i64(nK), ptr(zi),
                                    ptr(eps), i64(T), i64(pop), ptr(kp), ptr(K_ts)))
    return K_ts, kp


# ------------------------------------------------------------------ device tier


def ks_shocks_dev(uniforms, params, T, population, stream=None):
    """Device tier: uniforms a cuda float64 tensor; returns (zi int8 [T], eps int8 [T][pop])."""
    import torch
    dev = uniforms.device
    if uniforms.numel() != shock_draws(T, population):
        raise ValueError("uniforms has the wrong length")
    prm = np.ascontiguousarray(params, np.float64)
    zi = torch.empty(T, dtype=torch.int8, device=dev)
    eps = torch.empty((T, population), dtype=torch.int8, device=dev)
    check(lib().ks_shocks_dev(i64(T), i64(population), ptr(uniforms), ptr(prm), ptr(zi),
                              ptr(eps), stream_handle(stream)))
    return zi, eps


class PanelSim:
    """Device-resident panel simulation: k_opt [S][K][k] (k x K x S column-major), grids,
    shocks and the population stay in HBM across calls (the population persists across ALM
    iterations, Krusell_Smith_VFI.m:101)."""

    def __init__(self, k_grid, K_grid, zi, eps, k_population):
        import torch
        self.k_grid, self.K_grid, self.zi, self.eps = k_grid, K_grid, zi, eps
        self.k_pop = k_population
        self.T, self.pop = eps.shape
        lib().ks_panel_scratch_bytes.restype = C.c_int64
        nb = int(lib().ks_panel_scratch_bytes(i64(self.pop)))
        self.scratch = torch.empty(nb // 8, dtype=torch.float64, device=k_population.device)
        self.K_ts = torch.empty(self.T, dtype=torch.float64, device=k_population.device)

    def __call__(self, k_opt, stream=None):
        """One run of :206-248 with policy k_opt (device [S][K][k]); returns K_ts (device)."""
        nS, nK, nk = k_opt.shape
        check(lib().ks_simulate_capital_dev(i64(nk), i64(nK), ptr(self.k_grid), ptr(self.K_grid),
                                            ptr(k_opt), i64(self.T), i64(self.pop), ptr(self.zi),
                                            ptr(self.eps), ptr(self.k_pop), ptr(self.K_ts),
                                            ptr(self.scratch), stream_handle(stream)))
        return self.K_ts


# ------------------------------------------------------------------ histogram simulation


def hist_grid(nx=1000, k_min=0.0001, k_max=1000.0):
    """The histogram grid: linspace(0, 1, nx)^7 * (k_max - k_min) + k_min with the end points
    set exactly (the spacing rule of the script's k_grid, :16-17)."""
    x = (np.arange(nx) / (nx - 1.0)) ** 7 * (k_max - k_min) + k_min
    x[0], x[-1] = k_min, k_max
    return x


def hist_start(x_grid, K0, ug):
    """lam0 (2, nx): all mass at K0 by the lottery between its bracketing nodes, split
    (1 - ug, ug) over employment (row 0 employed, row 1 unemployed)."""
    x = np.asarray(x_grid, np.float64)
    K0 = min(max(float(K0), x[0]), x[-1])
    j = int(np.clip(np.searchsorted(x, K0, side="right") - 1, 0, x.size - 2))
    w = (K0 - x[j]) / (x[j + 1] - x[j])
    lam = np.zeros((2, x.size))
    for e, pe in ((0, 1 - ug), (1, ug)):
        lam[e, j] = pe * (1 - w)
        lam[e, j + 1] = pe * w
    return lam


def zi_paths(T, M, uniforms, params):
    """M aggregate shock paths (T, M) in {0 good, 1 bad}: the chain of :59-68 on M consecutive
    blocks of T-1 draws (path 0 on the stream's first T-1 draws is ks_shocks' zi)."""
    U = np.asarray(uniforms, np.float64).ravel()
    if U.size < M * (T - 1):
        raise ValueError(f"need {M * (T - 1)} uniforms, got {U.size}")
    pgg = 1 - 1 / 8.0
    pbb = 1 - 1 / 8.0
    zi = np.zeros((T, M), np.int8)
    for m in range(M):
        u = U[m * (T - 1):(m + 1) * (T - 1)]
        z = 0
        for t in range(1, T):
            z = int(u[t - 1] > (pbb if z else pgg))
            zi[t, m] = z
    return zi


def _hist_shapes(k_opt, k_grid, K_grid, x_grid):
    nk, nK, nS = k_opt.shape
    if nS != 4:
        raise ValueError("k_opt must be k x K x 4")
    if k_grid.size != nk or K_grid.size != nK:
        raise ValueError("k_opt must be numel(k_grid) x numel(K_grid) x 4")
    return nk, nK, x_grid.size


def _paths_2d(zi_paths, dtype=None):
    zi = np.asarray(zi_paths, dtype)
    return zi[:, None] if zi.ndim == 1 else zi


def _host_paths(zi_paths):
    """The host tier's zi_shock: (T, M) float64 column-major; with T and M."""
    zi = _paths_2d(zi_paths, np.float64)
    return (np.asfortranarray(zi),) + zi.shape


def _host_state(lam0, T, M, nx):
    """The host tier's lam (M, 2, nx) from lam0, and its outputs K_ts (T, M) and slow (M,)."""
    lam = np.array(np.broadcast_to(np.asarray(lam0, np.float64), (M, 2, nx)), order="C")
    return lam, np.empty((T, M), order="F"), np.zeros(M, np.int64)


def ks_simulate_hist(k_opt, k_grid, K_grid, x_grid, zi_paths, lam0, params):
    """The histogram simulation of the capital path through the host tier.  k_opt k x K x 4;
    zi_paths (T, M) in {0, 1}; lam0 (M, 2, nx) or (2, nx) (every path starts from it).
    Returns (K_ts (T, M), lam (M, 2, nx), slow_periods (M,))."""
    ko = np.asfortranarray(k_opt, dtype=np.float64)
    kg = np.ascontiguousarray(k_grid, np.float64)
    Kg = np.ascontiguousarray(K_grid, np.float64)
    x = np.ascontiguousarray(x_grid, np.float64)
    nk, nK, nx = _hist_shapes(ko, kg, Kg, x)
    zi, T, M = _host_paths(zi_paths)
    lam, K_ts, slow = _host_state(lam0, T, M, nx)
    prm = np.ascontiguousarray(params, np.float64)
    if prm.size != 13:
        raise ValueError("params must hold the 13 KS doubles")
    check(lib().ks_simulate_hist(ptr(ko), ptr(kg), ptr(Kg), i64(nk), i64(nK), ptr(x), i64(nx),
                                 ptr(prm), ptr(zi), i64(T), i64(M), ptr(lam), ptr(K_ts),
                                 ptr(slow)))
    return K_ts, lam, slow


class _HistState:
    """What HistSim and HistSimMulti keep in HBM across calls: k_grid, x_grid, the M shock paths
    (int8 [M][T]), the distributions lam [M][2][nx], K_ts [M][T] and the slow-period counts."""

    def __init__(self, k_grid, x_grid, zi_paths, lam0, device, params=None):
        import torch
        dev = torch.device(device)
        self._f64 = dict(dtype=torch.float64, device=dev)
        self.k_grid = self._grid(k_grid)
        self.x_grid = self._grid(x_grid)
        zi = _paths_2d(zi_paths)
        if not np.all((zi == 0) | (zi == 1)):
            raise ValueError("zi_paths must hold 0 (good) or 1 (bad)")
        self.T, self.M = zi.shape
        self.nx = self.x_grid.numel()
        self.zi = torch.as_tensor(np.ascontiguousarray(zi.T.astype(np.int8)), device=dev)
        if params is not None:
            self.params = np.ascontiguousarray(params, np.float64)
            if self.params.size != 13:
                raise ValueError("params must hold the 13 KS doubles")
        self.lam = torch.empty((self.M, 2, self.nx), **self._f64)
        self.set_lam(lam0)
        self.K_ts = torch.empty((self.M, self.T), **self._f64)
        self.slow = torch.zeros(self.M, dtype=torch.int64, device=dev)

    def _grid(self, g):
        import torch
        return torch.as_tensor(np.ascontiguousarray(g, np.float64), **self._f64)


class HistSim(_HistState):
    """Device-resident histogram simulation: grids, the M shock paths and the distributions stay
    in HBM across calls.  zi_paths (T, M) host array in {0, 1}; lam0 (M, 2, nx) or (2, nx).
    `lam` persists across calls like PanelSim's population; set_lam restarts it."""

    def __init__(self, k_grid, K_grid, x_grid, zi_paths, lam0, params, device="cuda"):
        super().__init__(k_grid, x_grid, zi_paths, lam0, device, params)
        self.K_grid = self._grid(K_grid)

    def set_lam(self, lam0):
        import torch
        lam = np.array(np.broadcast_to(np.asarray(lam0, np.float64), (self.M, 2, self.nx)))
        self.lam.copy_(torch.as_tensor(lam))

    def __call__(self, k_opt, stream=None):
        """One run with policy k_opt (device [S][K][k] = k x K x S column-major); returns K_ts
        (device [M][T]); self.lam holds the last period's distribution, self.slow the counts."""
        nS, nK, nk = k_opt.shape
        if nS != 4 or nK != self.K_grid.numel() or nk != self.k_grid.numel():
            raise ValueError("k_opt must be [4][numel(K_grid)][numel(k_grid)]")
        check(lib().ks_simulate_hist_dev(i64(nk), i64(nK), ptr(self.k_grid), ptr(self.K_grid),
                                         ptr(k_opt), ptr(self.x_grid), i64(self.nx),
                                         ptr(self.params), ptr(self.zi), i64(self.T),
                                         i64(self.M), ptr(self.lam), ptr(self.K_ts),
                                         ptr(self.slow), stream_handle(stream)))
        return self.K_ts


def _multi_shapes(k_opt, k_grid, K_grid, params, policy_of_path, M):
    """Candidate-major host inputs of the one-policy-per-path simulation: k_opt (C, nk, nK, 4),
    K_grid (C, nK) and params (C, 13) (one candidate's shape broadcasts), policy_of_path (M,)."""
    ko = np.asarray(k_opt, np.float64)
    if ko.ndim != 4 or ko.shape[3] != 4:
        raise ValueError("k_opt must be (C, k_size, K_size, 4)")
    C_, nk, nK, _ = ko.shape
    if k_grid.size != nk:
        raise ValueError("k_opt must be (C, numel(k_grid), K_size, 4)")
    Kg = _per_candidate(K_grid, C_, (nK,), "K_grid")
    prm = _per_candidate(params, C_, (13,), "params")
    pol = np.asarray(policy_of_path)
    if pol.shape != (M,) or not np.issubdtype(pol.dtype, np.integer):
        raise ValueError(f"policy_of_path must hold {M} integers, one per path")
    return ko, Kg, prm, np.ascontiguousarray(pol, np.int32), C_, nk, nK


def ks_simulate_hist_multi(k_opt, k_grid, K_grid, x_grid, zi_paths, lam0, params,
                           policy_of_path):
    """ks_simulate_hist with one policy per path (host tier): k_opt (C, nk, nK, 4), K_grid
    (C, nK), params (C, 13), policy_of_path (M,) integers in [0, C): path m runs candidate
    policy_of_path[m].  Returns (K_ts (T, M), lam (M, 2, nx), slow_periods (M,))."""
    kg = np.ascontiguousarray(k_grid, np.float64)
    x = np.ascontiguousarray(x_grid, np.float64)
    zi, T, M = _host_paths(zi_paths)
    ko, Kg, prm, pol, C_, nk, nK = _multi_shapes(k_opt, kg, K_grid, params, policy_of_path, M)
    kd = np.ascontiguousarray(ko.transpose(0, 3, 2, 1))    # each block k x K x 4 column-major
    nx = x.size
    lam, K_ts, slow = _host_state(lam0, T, M, nx)
    check(lib().ks_simulate_hist_multi(i64(C_), ptr(kd), ptr(kg), ptr(Kg), i64(nk), i64(nK),
                                       ptr(x), i64(nx), ptr(prm), ptr(pol), ptr(zi), i64(T),
                                       i64(M), ptr(lam), ptr(K_ts), ptr(slow)))
    return K_ts, lam, slow


class HistSimMulti(_HistState):
    """Device-resident histogram simulation with one policy per path: k_grid, x_grid, the M
    shock paths and the distributions stay in HBM across calls; the candidates (policies, their
    K_grid rows and params) and policy_of_path come with each call.  zi_paths (T, M) host array
    in {0, 1}; lam0 (M, 2, nx) or (2, nx).  `lam` persists across calls; set_lam restarts it.  A
    call with fewer than M entries in policy_of_path runs the first len(policy_of_path) paths."""

    def __init__(self, k_grid, x_grid, zi_paths, lam0, device="cuda"):
        super().__init__(k_grid, x_grid, zi_paths, lam0, device)
        self.scratch = None

    def set_lam(self, lam0):
        """lam0 (m, 2, nx), m <= M: the start of the first m paths; (2, nx): of every path."""
        import torch
        lam = np.asarray(lam0, np.float64)
        if lam.ndim == 2:
            lam = np.broadcast_to(lam, (self.M, 2, self.nx))
        if lam.ndim != 3 or lam.shape[0] > self.M or lam.shape[1:] != (2, self.nx):
            raise ValueError("lam0 must be (2, nx) or (m, 2, nx) with m <= M")
        self.lam[:lam.shape[0]].copy_(torch.as_tensor(np.ascontiguousarray(lam)))

    def __call__(self, k_opt, K_grid, params, policy_of_path, stream=None):
        """One run.  k_opt: device [C][4][nK][nk]; K_grid: (C, nK) host array or device tensor;
        params (C, 13) and policy_of_path (m,), m <= M, host.  Returns K_ts (device [m][T]);
        self.lam[:m] holds the last period's distributions, self.slow[:m] the counts."""
        import torch
        C_, nS, nK, nk = k_opt.shape
        if nS != 4 or nk != self.k_grid.numel():
            raise ValueError("k_opt must be [C][4][K_size][numel(k_grid)]")
        if not hasattr(K_grid, "data_ptr"):
            K_grid = torch.as_tensor(np.array(_per_candidate(K_grid, C_, (nK,), "K_grid"),
                                              order="C"), device=self.lam.device)
        if tuple(K_grid.shape) != (C_, nK):
            raise ValueError("K_grid must be (C, K_size)")
        if not (k_opt.is_contiguous() and K_grid.is_contiguous()):
            raise ValueError("k_opt and K_grid must be contiguous tensors")
        prm = _per_candidate(params, C_, (13,), "params")
        pol = np.asarray(policy_of_path)
        m = pol.size
        if pol.ndim != 1 or not 1 <= m <= self.M or not np.issubdtype(pol.dtype, np.integer):
            raise ValueError(f"policy_of_path must hold 1..{self.M} integers, one per path")
        pol = np.ascontiguousarray(pol, np.int32)
        lib().ks_hist_multi_scratch_bytes.restype = C.c_int64
        need = int(lib().ks_hist_multi_scratch_bytes(i64(C_), i64(m)))
        if self.scratch is None or self.scratch.numel() < need:
            self.scratch = torch.empty(need, dtype=torch.uint8, device=self.lam.device)
        check(lib().ks_simulate_hist_multi_dev(i64(C_), i64(nk), i64(nK), ptr(self.k_grid),
                                               ptr(K_grid), ptr(k_opt), ptr(self.x_grid),
                                               i64(self.nx), ptr(prm), ptr(pol), ptr(self.zi),
                                               i64(self.T), i64(m), ptr(self.lam),
                                               ptr(self.K_ts), ptr(self.slow),
                                               ptr(self.scratch), stream_handle(stream)))
        return self.K_ts[:m]


# ------------------------------------------------------------------ ALM loop (host)


def alm_regress(K_ts, zi_shock, T_discard=100):
    """Krusell_Smith_VFI.m:252-285: OLS of log K(t+1) on [1, log K(t)] per aggregate state,
    t = T_discard..T-1.  Host-side (4 coefficients; SURVEY C13 is out of the kernel scope).
    Returns (B_new, R2_good, R2_bad).  It is alm_regress_paths on the one path."""
    return alm_regress_paths(np.asarray(K_ts, np.float64).ravel(), np.asarray(zi_shock).ravel(),
                             T_discard)


def alm_regress_paths(K_ts, zi, T_discard=100):
    """The regression of :252-285 pooled over M shock paths: K_ts and zi are (T, M); the
    observations (t, m), t = T_discard..T-1, are stacked path after path.  For M = 1 this is
    alm_regress.  Returns (B_new, R2_good, R2_bad)."""
    K_ts = np.asarray(K_ts, np.float64)
    zi = np.asarray(zi)
    if K_ts.ndim == 1:
        K_ts, zi = K_ts[:, None], zi.reshape(-1, 1)
    T, M = K_ts.shape
    ts = np.arange(T_discard - 1, T - 1)
    B = np.zeros(4)
    R2 = [0.0, 0.0]
    for g in (0, 1):
        lk, lkn = [], []
        for m in range(M):
            sel = ts[zi[ts, m] == g]
            lk.append(np.log(K_ts[sel, m]))
            lkn.append(np.log(K_ts[sel + 1, m]))
        lk, Y = np.concatenate(lk), np.concatenate(lkn)
        if lk.size == 0:
            continue
        X = np.stack([np.ones(lk.size), lk], 1)
        Q, R = np.linalg.qr(X)
        b = np.linalg.solve(R, Q.T @ Y)
        B[2 * g:2 * g + 2] = b
        res = Y - X @ b
        R2[g] = 1 - np.sum(res ** 2) / np.sum((Y - Y.mean()) ** 2)
    return B, R2[0], R2[1]


def _alm_step(B, B_new, tol_B, update_B):
    """One economy's stop test and damped update (:286-295): (diff_B, done, the next B)."""
    diff_B = float(np.max(np.abs(B_new - B)))                                  # :286
    if diff_B < tol_B:
        return diff_B, True, B
    return diff_B, False, update_B * B_new + (1 - update_B) * B                 # :295


def _alm_loop(solve, simulate, regress, B0, max_iter_B, tol_B, update_B, log):
    """The outer loop of :138-296: solve(B) -> k_opt, simulate(k_opt) -> K_ts, regress(K_ts) ->
    (B_new, R2_good, R2_bad), until max |B_new - B| < tol_B.  Returns (B, B_history, R2, K_ts)."""
    B, hist, R2, K_ts = B0, [], (0.0, 0.0), None
    for it in range(max_iter_B):
        K_ts = simulate(solve(B))
        B_new, r2g, r2b = regress(K_ts)
        R2 = (r2g, r2b)
        diff_B, done, B = _alm_step(B, B_new, tol_B, update_B)
        hist.append(B_new.copy())
        if log:
            log(f"ALM {it + 1}: B_new={B_new} diff={diff_B:.2e} R2={R2}")
        if done:
            break
    return B, hist, R2, K_ts


def _check_simulate(simulate):
    if simulate not in ("panel", "histogram"):
        raise ValueError(f'simulate must be "panel" or "histogram", got {simulate!r}')


def _alm_simulation(simulate, prm, kg, Kg, T, population, uniforms, n_paths, nx):
    """The simulation step of an ALM loop: (run(k_opt) -> K_ts, zi, extra).  "panel": the agent
    panel, the population persisting across calls (:101).  "histogram": HistSim on n_paths
    paths; between calls the capital marginal of the last distribution is carried and re-split
    (1 - ug, ug) over employment, the analogue of k_population persisting while epsi_shock
    restarts at its first row.  `extra` holds what only the histogram returns (slow_periods,
    filled by each run, and x_grid)."""
    if simulate == "histogram":
        import torch
        ug = float(prm[5])
        U = matlab_rand(n_paths * (T - 1)) if uniforms is None else uniforms
        zi = zi_paths(T, n_paths, U, prm)
        x = hist_grid(nx, float(prm[3]), float(prm[4]))
        sim = HistSim(kg, Kg, x, zi, hist_start(x, Kg[0], ug), prm)
        extra = dict(slow_periods=None, x_grid=x)

        def run(k_opt):
            ko_dev = torch.as_tensor(np.ascontiguousarray(k_opt.transpose(2, 1, 0)),
                                     device=sim.lam.device)
            K_ts = sim(ko_dev).cpu().numpy().T
            extra["slow_periods"] = sim.slow.cpu().numpy()
            sim.set_lam(hist_carry(sim.lam.cpu().numpy(), ug))
            return K_ts
    else:
        U = matlab_rand(shock_draws(T, population)) if uniforms is None else uniforms
        zi, eps = ks_shocks(T, population, U, prm)
        pop = [np.full(population, Kg[0])]                                      # :101
        extra = {}

        def run(k_opt):
            K_ts, pop[0] = ks_simulate_capital(k_opt, kg, Kg, zi, eps, pop[0])
            return K_ts
    return run, zi, extra


def _alm_start(kg, K_size):
    """k_opt = 0.9 k (:97) and the identity law of motion (:99)."""
    return (0.9 * np.repeat(np.repeat(kg[:, None, None], K_size, 1), 4, 2),
            np.array([0.0, 1.0, 0.0, 1.0]))


def krusell_smith_vfi(k_size=100, K_size=4, T=1100, population=10000, max_iter_B=100, tol_B=1e-6,
                      update_B=0.3, howard_steps=50, tol_vfi=1e-6, max_vfi=10000, T_discard=100,
                      uniforms=None, n_devices=1, log=None, simulate="panel", n_paths=1,
                      nx=1000, **economy):
    """Krusell_Smith_VFI.m:4-296 end to end on the GPU kernels: shocks (F3), then per ALM
    iteration the VFI solve (A6/A7), the panel simulation (F2) and the host regression/update.
    Returns dict(B, B_history, R2, K_ts, value, k_opt, vfi_iters).
    simulate="histogram": the capital path comes from the histogram simulation (HistSim) on
    n_paths shock paths over an nx-point grid instead of the agent panel, and the regression is
    pooled over the paths (alm_regress_paths); K_ts and zi are then (T, n_paths).  `uniforms`
    then holds n_paths * (T - 1) aggregate draws.  `economy`: ks_params keywords plus K_min and
    K_max (defaults: the script's), as krusell_smith_egm's."""
    _check_simulate(simulate)
    prm, kg, Kg, P, V0 = _economy(k_size, K_size, economy)
    run, zi, extra = _alm_simulation(simulate, prm, kg, Kg, T, population, uniforms, n_paths, nx)
    k_opt, B0 = _alm_start(kg, K_size)
    st = dict(value=V0, k_opt=k_opt, vfi_iters=[])

    def solve(B):
        R = ks_vfi_solve(st["value"], st["k_opt"], kg, Kg, B, P, prm, howard_steps=howard_steps,
                         tol=tol_vfi, max_vfi=max_vfi, n_devices=n_devices)
        st.update(value=R["value"], k_opt=R["k_opt"])
        st["vfi_iters"].append(R["iters"])
        return R["k_opt"]
    B, hist, R2, K_ts = _alm_loop(solve, run, lambda K: alm_regress_paths(K, zi, T_discard), B0,
                                  max_iter_B, tol_B, update_B, log)
    return dict(B=B, B_history=hist, R2=R2, K_ts=K_ts, **st, zi=zi, **extra)


def _economy(k_size, K_size, economy):
    """(params, k_grid, K_grid, P, V0) of one economy: ks_params keywords plus K_min and K_max;
    V0 is the VFI script's start (Krusell_Smith_VFI.m:98)."""
    eco = dict(economy)
    K_min, K_max = eco.pop("K_min", 30.0), eco.pop("K_max", 50.0)
    prm = ks_params(**eco)
    kg, Kg, P, V0 = calibration.krusell_smith(k_size=k_size, K_size=K_size, K_min=K_min,
                                              K_max=K_max, beta=prm[0], k_min=prm[3],
                                              k_max=prm[4], ug=prm[5], ub=prm[6])
    return prm, kg, Kg, P, V0


def krusell_smith_egm(k_size=100, K_size=4, T=1100, population=10000, max_iter_B=100, tol_B=1e-6,
                      update_B=0.3, tol_egm=1e-6, max_egm=10000, T_discard=100, uniforms=None,
                      simulate="panel", n_paths=1, nx=1000, log=None, **economy):
    """Krusell_Smith_EGM.m:95-301 end to end on the GPU kernels: shocks (F3), then per ALM
    iteration the Gauss-Seidel EGM solve (A8, from the previous iteration's k_opt), the panel
    simulation (F2, the population persisting, :99) and the host regression / damped update
    (:255-300).  `economy`: ks_params keywords plus K_min and K_max (defaults: the script's).
    Returns dict(B, B_history, R2, K_ts, k_opt, egm_iters, zi).
    simulate="histogram": the histogram simulation on n_paths shock paths over an nx-point grid
    in place of the panel, as krusell_smith_vfi's; K_ts and zi are then (T, n_paths) and
    `uniforms` holds n_paths * (T - 1) aggregate draws."""
    _check_simulate(simulate)
    prm, kg, Kg, P, _ = _economy(k_size, K_size, economy)
    run, zi, extra = _alm_simulation(simulate, prm, kg, Kg, T, population, uniforms, n_paths, nx)
    k_opt, B0 = _alm_start(kg, K_size)                                         # :96-97
    st = dict(k_opt=k_opt, egm_iters=[])

    def solve(B):
        R = ks_egm_solve(st["k_opt"], kg, Kg, B, P, prm, tol=tol_egm, max_iter=max_egm)
        st["k_opt"] = R["k_opt"]
        st["egm_iters"].append(R["iters"])
        return R["k_opt"]
    B, hist, R2, K_ts = _alm_loop(solve, run, lambda K: alm_regress_paths(K, zi, T_discard), B0,
                                  max_iter_B, tol_B, update_B, log)
    return dict(B=B, B_history=hist, R2=R2, K_ts=K_ts, **st, zi=zi, **extra)


def _policy_rows(x):
    """k x K x 4 (MATLAB) as the device tiers' [4][nK][nk]."""
    return np.ascontiguousarray(np.asarray(x, np.float64).transpose(2, 1, 0))


def _alm_lockstep(economies, make_solver, iters_key, fail_name, k_size, K_size, T, max_iter_B,
                  tol_B, update_B, T_discard, uniforms, n_paths, nx, log):
    """The histogram ALM loop of several economies in lockstep, shared by
    krusell_smith_egm_batch and krusell_smith_vfi_batch.  The economies share k_min and k_max
    (hence k_grid and x_grid), the sizes and the n_paths shock paths; each has its own params, P,
    K_grid and B.  `make_solver(ecos, kg_dev, dev)` returns (solve, finish): solve(idx, Kg, B,
    P, prm) runs one batched solve of the economies idx (a device index tensor) on the solver's
    own device-resident state and returns (k_opt [R][4][nK][nk] on the device, iters (R,),
    status (R,)); finish(res) stores that state into the result dicts.  One round: one solve,
    one histogram launch of (economies with status 0) x n_paths workgroups with one policy per
    path, K_ts back to the host and one pooled regression per economy.  An economy leaves when
    its diff_B < tol_B, or when it fails: status != 0 (`failed` = fail_name; it is not
    simulated) or a non-positive or non-finite K_ts in the regression window (`failed` =
    "K_ts")."""
    import torch
    ecos = [_economy(k_size, K_size, e) for e in economies]
    E = len(ecos)
    if E < 1:
        raise ValueError("need at least one economy")
    prm = np.stack([e[0] for e in ecos])
    kg = ecos[0][1]
    if np.any(prm[:, 3] != prm[0, 3]) or np.any(prm[:, 4] != prm[0, 4]):
        raise ValueError("the economies of a batch share k_min and k_max (one k_grid and x_grid)")
    Kg = np.stack([e[2] for e in ecos])
    P = np.stack([e[3] for e in ecos])
    ug = prm[:, 5]
    U = matlab_rand(n_paths * (T - 1)) if uniforms is None else uniforms
    zi = zi_paths(T, n_paths, U, prm[0])
    x = hist_grid(nx, float(prm[0, 3]), float(prm[0, 4]))
    # path e * n_paths + p of the launch is shock path p: a prefix serves any number of economies
    sim = HistSimMulti(kg, x, np.tile(zi, (1, E)), np.zeros((2, nx)))
    dev = sim.lam.device
    solve, finish = make_solver(ecos, sim.k_grid, dev)
    lam = np.stack([np.broadcast_to(hist_start(x, Kg[e, 0], ug[e]), (n_paths, 2, nx))
                    for e in range(E)])
    B = np.tile(np.array([0.0, 1.0, 0.0, 1.0]), (E, 1))                        # :97
    res = [dict(B=B[e].copy(), B_history=[], R2=(0.0, 0.0), K_ts=None, k_opt=None, zi=zi,
                slow_periods=None, x_grid=x, failed=None, **{iters_key: []}) for e in range(E)]
    run = list(range(E))
    for it in range(max_iter_B):
        if not run:
            break
        idx = torch.as_tensor(run, device=dev)
        ko, iters, status = solve(idx, Kg[run], B[run], P[run], prm[run])
        good = [r for r in range(len(run)) if status[r] == 0]
        for r, e in enumerate(run):
            res[e][iters_key].append(int(iters[r]))
            if status[r] != 0:
                res[e]["failed"] = fail_name
        K_all = slow = lam_new = None
        if good:
            sim.set_lam(np.concatenate([lam[run[r]] for r in good]))
            pol = np.repeat(np.array(good, np.int32), n_paths)
            K_all = sim(ko, Kg[run], prm[run], pol).cpu().numpy()
            slow = sim.slow.cpu().numpy()
            lam_new = sim.lam.cpu().numpy()
        still = []
        for g, r in enumerate(good):
            e = run[r]
            sl = slice(g * n_paths, (g + 1) * n_paths)
            K_ts = K_all[sl].T
            res[e].update(K_ts=K_ts, slow_periods=slow[sl].copy())
            lam[e] = hist_carry(lam_new[sl], ug[e])
            win = K_ts[T_discard - 1:]
            if not (np.all(np.isfinite(win)) and np.all(win > 0)):
                res[e]["failed"] = "K_ts"
                continue
            B_new, r2g, r2b = alm_regress_paths(K_ts, zi, T_discard)
            res[e]["R2"] = (r2g, r2b)
            diff_B, done, B[e] = _alm_step(B[e], B_new, tol_B, update_B)       # :291-300
            res[e]["B_history"].append(B_new.copy())
            if log:
                log(f"ALM {it + 1} economy {e}: B_new={B_new} diff={diff_B:.2e}")
            if not done:
                still.append(e)
        run = still
    for e in range(E):
        res[e]["B"] = B[e].copy()
    finish(res)
    return res


def _store_policies(res, key, dev_blocks):
    """The device blocks [E][4][nK][nk] into res[e][key] as k x K x 4 column-major arrays."""
    host = dev_blocks.cpu().numpy()
    for e, r in enumerate(res):
        r[key] = np.asfortranarray(host[e].transpose(2, 1, 0))


def krusell_smith_egm_batch(economies, k_size=100, K_size=4, T=1100, max_iter_B=100, tol_B=1e-6,
                            update_B=0.3, tol_egm=1e-6, max_egm=10000, T_discard=100,
                            uniforms=None, n_paths=1, nx=1000, log=None):
    """krusell_smith_egm(simulate="histogram") for several economies in lockstep.  `economies`:
    a list of dicts of ks_params keywords plus K_min / K_max; all share k_min and k_max (hence
    k_grid and x_grid), the sizes and the n_paths shock paths, each has its own params, P, K_grid
    and B.  One ALM round is one ks_egm_solve_batch_dev over the economies still running (the
    policies stay on the device), one histogram launch of (running economies) x n_paths
    workgroups with one policy per path, K_ts back to the host and one pooled regression per
    economy.  An economy leaves when its diff_B < tol_B, or when it fails: an EGM status != 0
    (`failed` = "egm"; it is not simulated) or a non-positive or non-finite K_ts in the
    regression window (`failed` = "K_ts").  Returns one dict per economy with
    krusell_smith_egm's keys plus `failed` (None when it ran through); every economy that does
    not fail equals its own krusell_smith_egm(simulate="histogram") run bit for bit."""
    import torch

    def make_solver(ecos, kg_dev, dev):
        k0 = _policy_rows(_alm_start(ecos[0][1], K_size)[0])                   # :96
        k_opt = torch.as_tensor(np.ascontiguousarray(np.broadcast_to(k0, (len(ecos),) + k0.shape)),
                                device=dev)

        def solve(idx, Kg, B, P, prm):
            ko = k_opt[idx]
            iters, _, status, _ = ks_egm_solve_batch_dev(ko, kg_dev, Kg, B, P, prm, tol=tol_egm,
                                                         max_iter=max_egm)
            k_opt[idx] = ko
            return ko, iters.cpu().numpy(), status.cpu().numpy()
        return solve, lambda res: _store_policies(res, "k_opt", k_opt)
    return _alm_lockstep(economies, make_solver, "egm_iters", "egm", k_size, K_size, T,
                         max_iter_B, tol_B, update_B, T_discard, uniforms, n_paths, nx, log)


def krusell_smith_vfi_batch(economies, k_size=100, K_size=4, T=1100, max_iter_B=100, tol_B=1e-6,
                            update_B=0.3, howard_steps=50, tol_vfi=1e-6, max_vfi=10000,
                            T_discard=100, uniforms=None, n_paths=1, nx=1000, log=None):
    """krusell_smith_vfi(simulate="histogram") for several economies in lockstep, the VFI twin
    of krusell_smith_egm_batch (same `economies`, same sharing rules).  One ALM round is one
    ks_vfi_solve_batch_dev over the economies still running (one workgroup each; value and
    policy stay on the device and are warm from the economy's previous round), one histogram
    launch with one policy per path and one pooled regression per economy.  An economy leaves
    when its diff_B < tol_B, or with `failed` = "K_ts" on a non-positive or non-finite K_ts in
    the regression window.  k_size x K_size x 4 must fit the one-workgroup rule (<= 4,096
    nodes).  Returns one dict per economy with krusell_smith_vfi's keys plus `failed`; every
    economy equals its own krusell_smith_vfi(simulate="histogram", **economy) run bit for bit."""
    import torch

    def make_solver(ecos, kg_dev, dev):
        k0 = _policy_rows(_alm_start(ecos[0][1], K_size)[0])                   # :97
        k_opt = torch.as_tensor(np.ascontiguousarray(np.broadcast_to(k0, (len(ecos),) + k0.shape)),
                                device=dev)
        value = torch.as_tensor(np.stack([_policy_rows(e[4]) for e in ecos]), device=dev)  # :98

        def solve(idx, Kg, B, P, prm):
            V, ko = value[idx], k_opt[idx]
            iters, _, _ = ks_vfi_solve_batch_dev(V, ko, kg_dev, Kg, B, P, prm,
                                                 howard_steps=howard_steps, tol=tol_vfi,
                                                 max_vfi=max_vfi)
            value[idx] = V
            k_opt[idx] = ko
            return ko, iters.cpu().numpy(), np.zeros(len(Kg), np.int32)

        def finish(res):
            _store_policies(res, "k_opt", k_opt)
            _store_policies(res, "value", value)
        return solve, finish
    return _alm_lockstep(economies, make_solver, "vfi_iters", None, k_size, K_size, T, max_iter_B,
                         tol_B, update_B, T_discard, uniforms, n_paths, nx, log)


def hist_carry(lam, ug):
    """The start of the next ALM iteration from the last distributions lam (M, 2, nx): the
    capital marginal lam[:, 0] + lam[:, 1], re-split (1 - ug, ug) over employment."""
    marg = lam[:, 0, :] + lam[:, 1, :]
    return np.stack([(1 - ug) * marg, ug * marg], 1)
