"""GPU: the Krusell-Smith EGM kernels (Gauss-Seidel one-workgroup solve and the Jacobi variant)
against the C oracle, bit for bit, from starts that are not the calibration's smooth 0.9 k
(tests/ks_cases.egm_cases; tests/test_ks_cases_cpu.py shows what each reaches): the rank sort
sees k_current below k_min (the valid run starts at lo > 0) and above k_max, exact ties (index
order), all-NaN columns, two valid points (linear pchip), 'nearest' extension on both sides —
and raises exactly where the oracle refuses (fewer than two valid points)."""
import numpy as np
import pytest

from oracle import corc
from tests import ks_cases as kc

pytestmark = pytest.mark.gpu

CASES = {c["name"]: c for c in kc.egm_cases()}


@pytest.mark.parametrize("jacobi", [False, True])
@pytest.mark.parametrize("name", sorted(CASES))
def test_six_sweeps_match_oracle(pkg, gpu, name, jacobi):
    """6 sweeps, tol = 0: iters, k_opt and diff equal the oracle's; where the oracle refuses
    the start (rc = -2), the device raises AIY_NON_FINITE — and nowhere else."""
    c = CASES[name]
    oargs = (kc.cparams(c["p"]), c["k_grid"], c["K_grid"], c["B"], c["P"], c["k0"])
    dargs = (c["k0"], c["k_grid"], c["K_grid"], c["B"], c["P"], kc.prm(c["p"]))
    try:
        Ro = corc.ks_egm_solve(*oargs, tol=0.0, max_iter=6, jacobi=jacobi)
    except ValueError:
        Ro = None
    if Ro is None:
        with pytest.raises(pkg.AiyError) as e:
            pkg.ks_egm_solve(*dargs, tol=0.0, max_iter=6, jacobi=jacobi)
        assert e.value.status == "AIY_NON_FINITE"
        return
    R = pkg.ks_egm_solve(*dargs, tol=0.0, max_iter=6, jacobi=jacobi)
    assert R["iters"] == Ro["iters"] == 6
    assert np.array_equal(R["k_opt"], Ro["k_opt"], equal_nan=bool(np.isnan(c["k0"]).any()))
    assert R["diff"] == Ro["diff"]
