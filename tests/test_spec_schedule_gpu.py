"""The launch schedule of the speculative and lockstep solves: how many timed launches each solve
issues (Workspace.timing() with timing on: a count per sweep / step / push enqueued, the
speculative ones past the stop included) and where it stops.

tests/golden/spec_schedule.json was recorded with `record()` below on an MI355X at the commit
before the three solves' batch loops became csrc/spec_loop.hpp and the two batched Bellman solves'
lockstep loops became one function (bell_host.cpp), i.e. from the three separate loops.  The
counts are a pure function of each solve's distance sequence, which the oracle tests pin bit for
bit, so they do not depend on the machine's speed."""
import json

import numpy as np
import pytest

from oracle import np_oracle as no
from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu

FIXTURE = GOLDEN / "spec_schedule.json"


def _t(torch, x, dtype=np.float64):
    return torch.as_tensor(np.ascontiguousarray(x, dtype=dtype), device=torch.device("cuda:0"))


def _vfi(pkg, torch, Na, max_iter):
    cal = no.calib_aiyagari(Na=Na)
    ws = pkg.Workspace(7, Na)
    ws.set_timing(True)
    va = _t(torch, np.zeros((7, Na)))
    vb = torch.zeros_like(va)
    idx = torch.empty((7, Na), dtype=torch.int32, device=va.device)
    it, which = ws.vfi_solve(va, vb, _t(torch, cal["a_grid"]), _t(torch, cal["s"]),
                             _t(torch, cal["P"]), 0.04, no.wage(0.04, 0.36, 0.08), 0.96, 5.0, 1e-5,
                             max_iter, idx, torch.empty_like(va), torch.empty_like(va))
    out = dict(iters=it, which=which, launches=ws.timing()[1])
    ws.close()
    return out, cal, idx


def _egm(pkg, torch):
    N, Na, r = 7, 1100, 0.03
    cal = no.calib_aiyagari(Na=Na, shocks="rouwenhorst")
    a, s = cal["a_grid"], cal["s"]
    w = no.wage(r, 0.36, 0.08)
    ws = pkg.Workspace(N, Na)
    ws.set_timing(True)
    c = _t(torch, np.tile(((1 + r) * a + w * np.mean(s))[None, :], (N, 1)))
    it, _ = pkg.egm_solve_dev(ws, c, _t(torch, a), _t(torch, s), _t(torch, cal["P"]), r, w, 0.96,
                              5.0, cal["amin"], 1e-6, 400, torch.zeros_like(c))
    out = dict(iters=it, launches=ws.timing()[1])
    ws.close()
    return out


def _dist(pkg, torch, cal, idx):
    """From a uniform λ, under the Na = 400 VFI case's policy."""
    N, Na = 7, 400
    ws = pkg.Workspace(N, Na)
    ws.set_timing(True)
    lam0 = _t(torch, np.full((N, Na), 1.0 / (N * Na)))
    it, _ = pkg.dist_stationary_dev(ws, lam0, _t(torch, cal["a_grid"]), _t(torch, cal["P"]),
                                    torch.empty_like(lam0), policy_idx=idx, tol=1e-12,
                                    max_iter=10000)
    out = dict(iters=it, launches=ws.timing()[1])
    ws.close()
    return out


def _vfi_batch(pkg, torch):
    N, Na, C = 7, 2500, 3
    cal = no.calib_aiyagari(Na=Na)
    r = np.array([0.02, 0.03, 0.04])
    w = np.array([no.wage(x, 0.36, 0.08) for x in r])
    ws = pkg.Workspace(N, Na)
    ws.set_timing(True)
    va = _t(torch, np.zeros((C, N, Na)))
    vb = torch.zeros_like(va)
    idx = torch.zeros((C, N, Na), dtype=torch.int32, device=va.device)
    it, which = pkg.solve_batch_dev(ws, r, w, va, vb, _t(torch, cal["a_grid"]), _t(torch, cal["s"]),
                                    _t(torch, cal["P"]), 0.96, 5.0, 1e-5, 1000, idx,
                                    torch.zeros_like(va), torch.zeros_like(va))
    out = dict(iters=it, which=which, launches=ws.timing()[1])
    ws.close()
    return out


def _labor_batch(pkg, torch):
    N, Na, Nl, C = 7, 400, 5, 3
    cal = no.calib_aiyagari(Na=Na, rho=0.6, sigma_e=0.2)
    L = 0.01 + (1.5 - 0.01) * no.matlab_linspace01(Nl)
    r = np.array([0.01, 0.02, 0.03])
    w = np.array([no.wage(x, 0.36, 0.08) for x in r])
    ws = pkg.Workspace(N, Na, Nl)
    ws.set_timing(True)
    va = _t(torch, np.zeros((C, N, Na)))
    vb = torch.zeros_like(va)
    lin = torch.zeros((C, N, Na), dtype=torch.int32, device=va.device)
    pol = [torch.zeros_like(va) for _ in range(3)]
    it, which = pkg.labor_solve_batch_dev(ws, r, w, va, vb, _t(torch, cal["a_grid"]),
                                          _t(torch, cal["s"]), _t(torch, cal["P"]), _t(torch, L),
                                          0.96, 5.0, 1.0, 2.0, 1e-5, 1000, lin, *pol)
    out = dict(iters=it, which=which, launches=ws.timing()[1],
               batched_solves=ws.labor_batch_counts()[0])
    ws.close()
    return out


def record(pkg):
    """Every case -> {name: {iters, launches, ...}}: what the fixture holds."""
    import torch
    out = {}
    out["vfi_wide_na400"], cal, idx = _vfi(pkg, torch, 400, 1000)
    out["vfi_tree_na2500"] = _vfi(pkg, torch, 2500, 1000)[0]
    out["vfi_na400_max_iter7"] = _vfi(pkg, torch, 400, 7)[0]
    out["egm_chained_na1100"] = _egm(pkg, torch)
    out["dist_na400"] = _dist(pkg, torch, cal, idx)
    out["vfi_batch_c3_na2500"] = _vfi_batch(pkg, torch)
    out["labor_batch_c3_na400_nl5"] = _labor_batch(pkg, torch)
    return out


@pytest.fixture(scope="module")
def schedule(pkg, gpu):
    return record(pkg)


@pytest.mark.parametrize("case", ["vfi_wide_na400", "vfi_tree_na2500", "vfi_na400_max_iter7",
                                  "egm_chained_na1100", "dist_na400", "vfi_batch_c3_na2500",
                                  "labor_batch_c3_na400_nl5"])
def test_schedule_equals_recorded(schedule, case):
    want = json.loads(FIXTURE.read_text())[case]
    print(case, schedule[case])
    assert schedule[case] == want


def test_fixture_shows_a_schedule():
    """The recorded cases do what their names say: speculation past the stop, exhaustion inside
    a batch, the batched labour path taken."""
    fx = json.loads(FIXTURE.read_text())
    for k in ("vfi_wide_na400", "vfi_tree_na2500", "egm_chained_na1100", "dist_na400"):
        assert fx[k]["launches"] >= fx[k]["iters"] > 16, k
    assert fx["vfi_na400_max_iter7"]["iters"] == fx["vfi_na400_max_iter7"]["launches"] == 7
    assert fx["labor_batch_c3_na400_nl5"]["batched_solves"] == 1
    for k in ("vfi_batch_c3_na2500", "labor_batch_c3_na400_nl5"):
        assert fx[k]["launches"] >= max(fx[k]["iters"]) and len(fx[k]["iters"]) == 3, k
