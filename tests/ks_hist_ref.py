"""Plain numpy restatement of the Krusell-Smith histogram simulation (csrc/ks_hist_kernels.hip):
the recursion, the kernel's order for K_t = Σ λ·x, and both summation orders of the pushed
mass.  The bilinear and segment arithmetic is np_oracle.ks_panel_simulate's.  Every floating
point operation is written in the order the kernel performs it (fp64, no contraction), so the
GPU tests compare bit for bit."""
import numpy as np

from oracle import np_oracle as no

CHUNK = 32   # kDistChunk
FOLD = 256   # kHistFold


def thr_table(params):
    """thr[z_next, z, e] = P(employed next | e): the panel's table (np_oracle.ks_eps_probs)."""
    return no.ks_eps_probs(dict(ug=float(params[5]), ub=float(params[6])))["thr"]


def moment(lam, x):
    """K = Σ λ[e][j]·x[j]: 256 strided partial sums over the flat index f = e·nx + j, each group
    of 64 folded pairwise (h = 32 ... 1), then (q0 + q2) + (q1 + q3)."""
    nx = x.size
    prod = np.zeros(-(-2 * nx // FOLD) * FOLD)
    prod[:2 * nx] = lam.reshape(-1) * np.tile(x, 2)
    s = np.zeros(FOLD)
    for row in prod.reshape(-1, FOLD):     # (a padded 0.0 leaves the sum unchanged)
        s = s + row
    s = s.reshape(4, 64)
    h = 32
    while h >= 1:
        s = s.copy()
        s[:, :h] = s[:, :h] + s[:, h:2 * h]
        h //= 2
    q = s[:, 0]
    return (q[0] + q[2]) + (q[1] + q[3])


def keys_weights(k_opt, k_grid, K_grid, x, ik, tk, K, z):
    """key[e][j], w[e][j] of period policy (K, z): steps b and c."""
    nx = x.size
    iK = int(no._bilin_seg(K_grid, np.array([K]))[0])
    tK = (K - K_grid[iK]) / (K_grid[iK + 1] - K_grid[iK])
    key = np.zeros((2, nx), np.int64)
    w = np.zeros((2, nx))
    for e in (0, 1):
        s = 2 * z + e
        f00 = k_opt[ik, iK, s]; f10 = k_opt[ik + 1, iK, s]
        f01 = k_opt[ik, iK + 1, s]; f11 = k_opt[ik + 1, iK + 1, s]
        f0 = f00 + tk * (f10 - f00)
        f1 = f01 + tk * (f11 - f01)
        kn = f0 + tK * (f1 - f0)
        kn = np.where(kn < x[0], x[0], kn)
        kn = np.where(kn > x[-1], x[-1], kn)
        key[e] = no._bilin_seg(x, kn)
        w[e] = (kn - x[key[e]]) / (x[key[e] + 1] - x[key[e]])
    return key, w


def _seq_sum(terms, lens):
    """Row r: 0.0 + terms[r, 0] + ... + terms[r, lens[r]-1], sequentially (vectorised over r)."""
    acc = np.zeros(terms.shape[0])
    for u in range(terms.shape[1]):
        live = lens > u
        if not live.any():
            break
        acc = np.where(live, acc + terms[:, u], acc)
    return acc


def push_fast(lam_row, w_row, key_row):
    """dist_mass<true> on a monotone row: destination k's sources are the run
    [off(k-1), off(k+1)) (λ·w below off(k), λ·(1-w) from it), summed sequentially in chunks of
    32 from the run's start, the chunk sums added in chunk order; a run of <= 32 terms is the
    plain sequential sum."""
    nx = lam_row.size
    off = np.searchsorted(key_row, np.arange(nx + 1), side="left")
    up = lam_row * w_row
    dn = lam_row * (1 - w_row)
    k = np.arange(nx)
    js = off[k]
    je = off[k + 1]
    jb = np.where(k > 0, off[np.maximum(k - 1, 0)], js)
    L = je - jb
    out = np.zeros(nx)
    short = np.nonzero(L <= CHUNK)[0]
    if short.size:
        pos = jb[short, None] + np.arange(CHUNK)[None, :]
        posc = np.minimum(pos, nx - 1)
        terms = np.where(pos < js[short, None], up[posc], dn[posc])
        out[short] = _seq_sum(terms, L[short])
    for d in np.nonzero(L > CHUNK)[0]:
        total = 0.0
        for b in range(jb[d], je[d], CHUNK):
            part = 0.0
            for j in range(b, min(b + CHUNK, je[d])):
                part = part + (up[j] if j < js[d] else dn[j])
            total = total + part
        out[d] = total
    return out


def push_slow(lam_row, w_row, key_row):
    """Ordered scan: destination k adds its matching terms in ascending source j, from 0.0."""
    nx = lam_row.size
    up = lam_row * w_row
    dn = lam_row * (1 - w_row)
    out = np.zeros(nx)
    for j in range(nx):
        kk = key_row[j]
        out[kk + 1] = out[kk + 1] + up[j]
        out[kk] = out[kk] + dn[j]
    return out


def simulate_path(k_opt, k_grid, K_grid, x, params, zi, lam0):
    """One shock path.  k_opt [k, K, s]; zi (T,) in {0, 1}; lam0 (2, nx).
    Returns (K_ts (T,), lam (2, nx), slow_periods)."""
    thr = thr_table(params)
    x = np.asarray(x, np.float64)
    ik = no._bilin_seg(k_grid, x)
    tk = (x - k_grid[ik]) / (k_grid[ik + 1] - k_grid[ik])
    lam = np.array(lam0, np.float64, copy=True)
    T = len(zi)
    K_ts = np.zeros(T)
    slow = 0
    for t in range(T - 1):
        z, zn = int(zi[t]), int(zi[t + 1])
        K = moment(lam, x)
        K_ts[t] = K
        key, w = keys_weights(k_opt, k_grid, K_grid, x, ik, tk, K, z)
        mono = all(np.all(key[e][1:] >= key[e][:-1]) for e in (0, 1))
        if not mono:
            slow += 1
        push = push_fast if mono else push_slow
        pushed = [push(lam[e], w[e], key[e]) for e in (0, 1)]
        p = thr[zn, z]
        new = np.zeros_like(lam)
        for en in (0, 1):
            a0 = p[0] if en == 0 else 1 - p[0]
            a1 = p[1] if en == 0 else 1 - p[1]
            acc = np.zeros(x.size)
            acc = acc + a0 * pushed[0]
            acc = acc + a1 * pushed[1]
            new[en] = acc
        lam = new
    K_ts[T - 1] = moment(lam, x)
    return K_ts, lam, slow


def simulate(k_opt, k_grid, K_grid, x, params, zi_paths, lam0):
    """M paths: zi_paths (T, M); lam0 (M, 2, nx) or (2, nx).
    Returns (K_ts (T, M), lam (M, 2, nx), slow_periods (M,))."""
    zi = np.asarray(zi_paths)
    zi = zi[:, None] if zi.ndim == 1 else zi
    T, M = zi.shape
    lam0 = np.broadcast_to(np.asarray(lam0, np.float64), (M, 2, len(x)))
    K_ts = np.zeros((T, M))
    lam = np.zeros((M, 2, len(x)))
    slow = np.zeros(M, np.int64)
    for m in range(M):
        K_ts[:, m], lam[m], slow[m] = simulate_path(k_opt, k_grid, K_grid, x, params, zi[:, m],
                                                    lam0[m])
    return K_ts, lam, slow


def transition_matrix(k_opt, k_grid, K_grid, x, params, K, z, zn):
    """The dense 2nx x 2nx matrix of one period: λ' = Mat @ λ.flat (a different summation order
    of the same recursion)."""
    thr = thr_table(params)
    nx = x.size
    ik = no._bilin_seg(k_grid, x)
    tk = (x - k_grid[ik]) / (k_grid[ik + 1] - k_grid[ik])
    key, w = keys_weights(k_opt, k_grid, K_grid, x, ik, tk, K, z)
    Mat = np.zeros((2 * nx, 2 * nx))
    for e in (0, 1):
        pe = (thr[zn, z, e], 1 - thr[zn, z, e])
        for j in range(nx):
            for en in (0, 1):
                Mat[en * nx + key[e, j], e * nx + j] += pe[en] * (1 - w[e, j])
                Mat[en * nx + key[e, j] + 1, e * nx + j] += pe[en] * w[e, j]
    return Mat
