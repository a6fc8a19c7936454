"""The economies of the batched-Jacobian tests: four calibrations that differ in β, σ, the income
process and the asset grid (integer σ, non-integer σ, σ = 1; three grids), each turned into a
point to differentiate at by tests.transition_ref.steady_state_cpu at r = 0.03."""
import functools

import numpy as np

from tests import transition_ref as tr
from tests.conftest import load_pkg

# (β, σ, ρ, σ_e, scale of a_grid)
PARAMS = [(0.96, 5.0, 0.75, 0.75, 1.0),
          (0.94, 2.0, 0.6, 0.4, 0.75),
          (0.95, 1.5, 0.9, 0.5, 1.0),
          (0.96, 1.0, 0.75, 0.75, 0.5)]
SHAPES = [(60, 12), (24, 9)]  # (Na, T)
H = 1e-4


@functools.lru_cache(maxsize=None)
def economies(Na):
    """The four steady-state dicts at N = 3 and this Na (shared: do not modify)."""
    cb = load_pkg().calibration
    out = []
    for beta, sigma, rho, sigma_e, scale in PARAMS:
        cal = cb.aiyagari(Na=Na, shocks="rouwenhorst", N=3, beta=beta, sigma=sigma, rho=rho,
                          sigma_e=sigma_e)
        cal["a_grid"] = cal["a_grid"] * scale
        out.append(tr.steady_state_cpu(cal, 0.03,
                                       lambda r, c=cal: cb.wage(r, c["alpha"], c["delta"])))
    return tuple(out)


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.int64)


def same(x, y):
    x, y = np.asarray(x), np.asarray(y)
    return x.shape == y.shape and np.array_equal(bits(x), bits(y))


def same_nan(x, y):
    """Equal bits where neither is NaN, NaN in the same places."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    nx = np.isnan(x)
    return x.shape == y.shape and np.array_equal(nx, np.isnan(y)) and same(x[~nx], y[~nx])


KEYS = ("J_r", "J_w", "F_r", "F_w", "E")


# ---- the general-equilibrium chain (tests/test_structural_*.py): economy e under the AR(1) shock
# (RHO[e], SIG[e])
RHO = np.array([0.9, 0.8, 0.7, 0.95])
SIG = np.array([0.01, 0.02, 0.005, 0.01])
# ge_ma_batch through the reference LU (tests/dense_ref.py) against the host route
# ge_jacobians(...) @ dZ (LAPACK), both on tests.ssj_ref.jacobian_cpu's Jacobians of the four
# economies at SHAPES: the largest max|m − m_host| / (cond∞(I − M)·T·2⁻⁵²·max|m_host|) met is
# GE_MEASURED (economy 2 at Na = 24, T = 9; test_structural_cpu.py re-measures it); the GPU test's
# bound is four times that.
GE_MEASURED = 0.2647
GE_C = 4 * GE_MEASURED


def ge_ratio(pkg, ss, jac, m, dZ):
    """max|m − m_host| / (cond∞(I − M)·T·2⁻⁵²·max|m_host|) of one economy, m_host the host route
    ge_jacobians(ss, jac) @ dZ over the default outputs."""
    mh = pkg.ge_jacobians(ss, jac) @ dZ
    T = dZ.size
    cond = np.linalg.cond(-pkg.transition._newton_matrix(ss, jac), np.inf)
    return float(np.max(np.abs(m - mh)) / (cond * T * 2.0 ** -52 * np.max(np.abs(mh))))
