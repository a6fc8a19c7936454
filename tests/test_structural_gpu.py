"""GPU tests of the structural chain (estimation.py): ge_ma_batch — one dense solve with one
right-hand side per economy — against the host route ge_jacobians(...) @ dZ and against the
reference LU bit for bit, and structural_loglik against the hand-chained calls and against each
candidate alone."""
import numpy as np
import pytest

from tests import dense_ref as dr
from tests.ssj_batch_cases import GE_C, H, RHO, SHAPES, SIG, economies, ge_ratio, same

pytestmark = pytest.mark.gpu


def _one(jac, e):
    return {k: v[e] for k, v in jac.items() if k != "status"}


@pytest.mark.parametrize("Na,T", SHAPES)
def test_ge_ma_batch_is_the_host_route(gpu, pkg, Na, T):
    """|m − ge_jacobians(ss_e, jac_e) @ dZ_e| <= c·cond∞(I − M_e)·T·2⁻⁵²·max|m_e| with c = 4 × the
    value the reference LU reaches against LAPACK on the CPU Jacobians (GE_MEASURED = 0.2647, so
    c = 1.0588); the device solve is the reference LU bit for bit, and an economy's m does not
    depend on its batch."""
    eco = economies(Na)
    jac = pkg.jacobian_batch(eco, T, H)
    assert not jac["status"].any()
    dZ = pkg.ar1_ma(RHO, SIG, T)
    m = pkg.ge_ma_batch(eco, jac, dZ)
    assert m.shape == (4, 5, T) and np.isfinite(m).all()
    assert same(m, pkg.ge_ma_batch(eco, jac, dZ, solve=dr.dense_solve_batch))
    for e in range(4):
        ratio = ge_ratio(pkg, eco[e], _one(jac, e), m[e], dZ[e])
        print(f"Na = {Na}, T = {T}, economy {e}: {ratio:.4f} (bound {GE_C:.4f})")
        assert ratio <= GE_C, e
        solo = pkg.ge_ma_batch(eco[e:e + 1], {k: jac[k][e:e + 1] for k in ("J_r", "J_w")},
                               dZ[e:e + 1])
        assert same(solo[0], m[e]), e
    for chunk in (1, 3):
        assert same(pkg.ge_ma_batch(eco, jac, dZ, chunk=chunk), m)
    part = pkg.ge_ma_batch(eco, jac, dZ, outputs=("Y", "C", "K"))
    assert same(part, m[:, [1, 2, 0]])


def _panel(pkg, Na, T, L, outputs):
    """y [L][n_o] simulated from economy 0's MA coefficients (seeded), and me_var [n_o]."""
    eco = economies(Na)
    jac = pkg.jacobian_batch(eco[:1], T, H)
    m0 = pkg.ge_ma_batch(eco[:1], jac, pkg.ar1_ma(RHO[:1], SIG[:1], T), outputs)[0]
    rng = np.random.default_rng(2024)
    eps = rng.standard_normal(L + T)
    me_var = 0.01 * np.sum(m0 * m0, axis=1)
    y = np.stack([[float(np.sum(m0[o] * eps[T + t - np.arange(T)])) for o in range(len(outputs))]
                  for t in range(L)])
    return y + np.sqrt(me_var) * rng.standard_normal(y.shape), me_var


@pytest.mark.parametrize("Na,T", SHAPES)
def test_structural_loglik_is_the_hand_chained_calls(gpu, pkg, Na, T):
    outputs, L = ("Y", "C", "K"), 8
    eco = economies(Na)
    y, me_var = _panel(pkg, Na, T, L, outputs)
    split = np.full(4, -1.0)
    R = pkg.structural_loglik(eco, y, RHO, SIG, me_var, T, split_ms=split)
    assert set(R) == {"loglik", "status", "fail", "jac_status"} and (split >= 0).all()
    assert R["loglik"].shape == (4,) and not R["status"].any() and not R["jac_status"].any()
    assert np.isfinite(R["loglik"]).all() and (R["fail"] == -1).all()
    jac = pkg.jacobian_batch(eco, T, H)
    m = pkg.ge_ma_batch(eco, jac, pkg.ar1_ma(RHO, SIG, T), outputs)
    W = pkg.loglik_batch(m, y, me_var)
    assert same(R["loglik"], W["loglik"]) and np.array_equal(R["status"], W["status"])
    assert np.array_equal(R["fail"], W["fail"]) and np.array_equal(R["jac_status"], jac["status"])
    for e in range(4):
        S = pkg.structural_loglik(eco[e:e + 1], y, RHO[e:e + 1], SIG[e:e + 1], me_var, T)
        assert same(S["loglik"][0], R["loglik"][e]) and S["status"][0] == R["status"][e], e


def test_a_sick_economy_fails_alone(gpu, pkg):
    """A NaN policy: the Jacobian's status, a stopped solve and a status-1 likelihood for that
    candidate; the others keep their bits."""
    Na, T = SHAPES[1]
    outputs, L = ("Y", "C", "K"), 8
    eco = list(economies(Na))
    y, me_var = _panel(pkg, Na, T, L, outputs)
    good = pkg.structural_loglik(eco, y, RHO, SIG, me_var, T)
    sick = dict(eco[2])
    sick["policy_c"] = sick["policy_c"].copy()
    sick["policy_c"][0, 3] = np.nan
    eco[2] = sick
    R = pkg.structural_loglik(eco, y, RHO, SIG, me_var, T)
    assert R["jac_status"][2][0] != 0 and R["status"][2] == 1 and np.isnan(R["loglik"][2])
    keep = [0, 1, 3]
    assert same(R["loglik"][keep], good["loglik"][keep]) and not R["status"][keep].any()
