"""No GPU: the general-equilibrium chain of estimation.py on CPU backends — ge_ma_batch through the
reference LU against the host route ge_jacobians(...) @ dZ, which is also where the constant of
the GPU test's bound is measured, and its shape checks."""
import numpy as np
import pytest

from tests import dense_ref as dr
from tests import ssj_ref as sr
from tests.ssj_batch_cases import (GE_C, GE_MEASURED, H, RHO, SHAPES, SIG, economies, ge_ratio,
                                   same)


def _cpu_chain(pkg, Na, T):
    eco = economies(Na)
    jacs = [sr.jacobian_cpu(ss, T, H) for ss in eco]
    jb = dict(J_r=np.stack([j["J_r"] for j in jacs]), J_w=np.stack([j["J_w"] for j in jacs]))
    dZ = pkg.ar1_ma(RHO, SIG, T)
    return eco, jacs, jb, dZ


def test_ge_ma_batch_is_the_host_route_and_the_measured_constant(pkg):
    """m = G·dZ from one right-hand side per economy.  The two solves are different algorithms:
    the difference is measured relative to cond∞(I − M)·T·2⁻⁵²·max|m| — 0.2646 at most (economy 2
    at Na = 24, T = 9) — and the recorded constant must cover it."""
    worst = 0.0
    for Na, T in SHAPES:
        eco, jacs, jb, dZ = _cpu_chain(pkg, Na, T)
        m = pkg.ge_ma_batch(eco, jb, dZ, solve=dr.dense_solve_batch)
        assert m.shape == (4, 5, T)
        for e in range(4):
            worst = max(worst, ge_ratio(pkg, eco[e], jacs[e], m[e], dZ[e]))
            solo = pkg.ge_ma_batch(eco[e:e + 1], dict(J_r=jb["J_r"][e:e + 1],
                                                      J_w=jb["J_w"][e:e + 1]), dZ[e:e + 1],
                                   solve=dr.dense_solve_batch)
            assert same(solo[0], m[e])
            assert (m[e][0][0] == 0)  # K_0 is given
    print(f"reference LU vs LAPACK through the GE chain: {worst:.4f}")
    assert 0.9 * GE_MEASURED <= worst <= GE_MEASURED and GE_C == 4 * GE_MEASURED


def test_ge_ma_batch_outputs_and_shapes(pkg):
    Na, T = SHAPES[1]
    eco, jacs, jb, dZ = _cpu_chain(pkg, Na, T)
    full = pkg.ge_ma_batch(eco, jb, dZ, solve=dr.dense_solve_batch)
    part = pkg.ge_ma_batch(eco, jb, dZ, outputs=("C", "K"), solve=dr.dense_solve_batch)
    assert same(part[:, 0], full[:, 2]) and same(part[:, 1], full[:, 0])
    with pytest.raises(ValueError):
        pkg.ge_ma_batch(eco, jb, dZ[:3], solve=dr.dense_solve_batch)
    with pytest.raises(ValueError):
        pkg.ge_ma_batch(eco, jb, dZ, outputs=("Q",), solve=dr.dense_solve_batch)
    # a singular system (NaN Jacobian) gives that economy NaN rows and leaves the others alone
    jb2 = dict(J_r=jb["J_r"].copy(), J_w=jb["J_w"])
    jb2["J_r"][1] = np.nan
    sick = pkg.ge_ma_batch(eco, jb2, dZ, solve=dr.dense_solve_batch)
    assert np.isnan(sick[1]).all() and same(sick[[0, 2, 3]], full[[0, 2, 3]])
