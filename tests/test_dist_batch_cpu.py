"""CPU: the batched histogram solve and its GE entry points without a GPU — argument validation
before any device work (library and gateways), the host driver (ge_batch.py: hist_evaluator over
the C restatement, multisection against bisection) and the batch blocks' memory logic with the
fit rule in a stand-alone program built with AddressSanitizer and UBSan."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from oracle import corc
from tests import mexstub
from tests.conftest import ROOT
from tests.test_host_layer_cpu import ROCM, _build

OK, BAD_SHAPE, NON_FINITE, NO_DEVICE, BAD_ARG = 0, 1, 2, 5, 6
p = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)
d, i64 = C.c_double, C.c_int64


def _has_gpu():
    import torch
    return torch.cuda.is_available()


# ------------------------------------------------------------------ aiy_dist_stationary_batch
def _dist_args(pkg, Cn=2, Na=20, lottery=False, **over):
    cal = pkg.calibration.aiyagari(Na=Na)
    N = cal["N"]
    k = dict(C=Cn, idx=None if lottery else np.ones((Cn, N * Na), np.int32),
             kp=np.zeros((Cn, N * Na)) if lottery else None, lay=1, a=cal["a_grid"].copy(),
             P=np.asfortranarray(cal["P"]), N=N, Na=Na, tol=1e-10, max_iter=50,
             lam=np.full((Cn, N * Na), 1.0 / (N * Na)), K=np.zeros(Cn), it=np.zeros(Cn, np.int64),
             dist=np.zeros(Cn))
    k.update(over)
    return k


def _dist_call(pkg, k):
    return pkg.lib().aiy_dist_stationary_batch(
        i64(k["C"]), p(k["idx"]), p(k["kp"]), C.c_int(k["lay"]), p(k["a"]), p(k["P"]), i64(k["N"]),
        i64(k["Na"]), d(k["tol"]), i64(k["max_iter"]), p(k["lam"]), p(k["K"]), p(k["it"]),
        p(k["dist"]))


def test_dist_batch_validates_before_device_work(pkg):
    rep = _dist_args(pkg)["a"]
    rep[3] = rep[2]
    cases = [(dict(idx=None), BAD_ARG), (dict(P=None), BAD_ARG), (dict(lam=None), BAD_ARG),
             (dict(K=None), BAD_ARG), (dict(it=None), BAD_ARG), (dict(dist=None), BAD_ARG),
             (dict(C=0), BAD_SHAPE), (dict(C=-3), BAD_SHAPE), (dict(N=0), BAD_SHAPE),
             (dict(Na=1), BAD_SHAPE), (dict(max_iter=0), BAD_ARG)]
    for over, code in cases:
        assert _dist_call(pkg, _dist_args(pkg, **over)) == code, over
    # a repeated grid node: refused with a lottery policy (it divides by a(k+1) - a(k)) only
    assert _dist_call(pkg, _dist_args(pkg, lottery=True, a=rep)) == BAD_ARG
    assert b"strictly increasing" in pkg.lib().aiy_last_error()
    assert _dist_call(pkg, _dist_args(pkg, a=rep)) == (OK if _has_gpu() else NO_DEVICE)


def test_dist_batch_dev_validates_before_device_work(pkg):
    """The device tier's argument errors need no workspace contents and no device."""
    L = pkg.lib()
    z, zi = np.zeros(8), np.zeros(8, np.int32)
    one, i1 = np.zeros(1), np.zeros(1, np.int64)

    def call(ws, Cn=1, lam=z, idx=zi, kp=None, max_iter=5, it=i1, out=z):
        return L.aiy_dist_stationary_batch_dev(ws, i64(Cn), p(lam), p(idx), p(kp), p(z), p(z),
                                               d(1e-10), i64(max_iter), p(out), None, p(it), p(one),
                                               None)
    assert call(None) == BAD_ARG
    assert L.aiy_ws_set_dist_batch(None, C.c_int(1)) == BAD_ARG
    assert L.aiy_ws_dist_batch_counts(None, None, None) == BAD_ARG
    h = C.c_void_p()
    rc = L.aiy_ws_create(i64(2), i64(2), i64(1), C.byref(h))
    if rc != OK:  # no device: a workspace cannot be made; the NULL checks above are what runs
        assert rc == NO_DEVICE
        return
    try:
        assert call(h, lam=None) == BAD_ARG and call(h, it=None) == BAD_ARG
        assert call(h, out=None) == BAD_ARG and call(h, idx=None) == BAD_ARG
        assert call(h, Cn=0) == BAD_SHAPE
        assert call(h, max_iter=0) == BAD_ARG
        assert L.aiy_ws_set_dist_batch(h, C.c_int(-2)) == BAD_ARG
        a, b = i64(-1), i64(-1)
        assert L.aiy_ws_dist_batch_counts(h, C.byref(a), C.byref(b)) == OK
        assert (a.value, b.value) == (0, 0)
    finally:
        L.aiy_ws_destroy(h)


# ------------------------------------------------------------------ the GE entry points
def _ge_args(pkg, C_=2, Na=20, **over):
    cal = pkg.calibration.aiyagari(Na=Na)
    N = cal["N"]
    k = dict(r=np.linspace(0.0, 0.02, C_), C=C_, v=np.zeros((N, Na), order="F"),
             a=cal["a_grid"].copy(), s=cal["s"].copy(), P=np.asfortranarray(cal["P"]), N=N, Na=Na,
             tol=1e-5, max_iter=100, dtol=1e-10, dmax=50, lam=None, nd=1, Ks=np.zeros(C_),
             Kd=np.zeros(C_), it=np.zeros(C_, np.int64), dit=np.zeros(C_, np.int64), cal=cal)
    k.update(over)
    return k


def _ge_call(pkg, k):
    cal = k["cal"]
    return pkg.lib().aiy_ge_hist_batch(
        p(k["r"]), i64(k["C"]), p(k["v"]), p(k["a"]), p(k["s"]), p(k["P"]), i64(k["N"]),
        i64(k["Na"]), d(cal["alpha"]), d(cal["delta"]), d(cal["beta"]), d(cal["sigma"]),
        d(cal["labor"]), d(k["tol"]), i64(k["max_iter"]), d(k["dtol"]), i64(k["dmax"]), p(k["lam"]),
        C.c_int(k["nd"]), p(k["Ks"]), p(k["Kd"]), p(k["it"]), p(k["dit"]))


def _egm_args(pkg, C_=2, Na=20, **over):
    cal, r0, w, guess = pkg.ge_batch.egm_calibration(Na, False)
    k = dict(r=np.linspace(0.0, 0.02, C_), w=np.full(C_, w), C=C_, pc=np.ascontiguousarray(guess),
             a=cal["a_grid"].copy(), s=cal["s"].copy(), P=np.asfortranarray(cal["P"]), N=cal["N"],
             Na=Na, labor_flag=0, phi=1.0, theta=1.0, tol=1e-5, max_iter=100, dtol=1e-10, dmax=50,
             lam=None, nd=1, Ks=np.zeros(C_), Kd=np.zeros(C_), it=np.zeros(C_, np.int64),
             dit=np.zeros(C_, np.int64), st=np.zeros(C_, np.int32), cal=cal)
    k.update(over)
    return k


def _egm_call(pkg, k):
    cal = k["cal"]
    return pkg.lib().aiy_egm_ge_hist_batch(
        p(k["r"]), p(k["w"]), i64(k["C"]), p(k["pc"]), p(k["a"]), p(k["s"]), p(k["P"]),
        i64(k["N"]), i64(k["Na"]), d(cal["alpha"]), d(cal["delta"]), d(cal["beta"]),
        d(cal["sigma"]), d(cal["amin"]), C.c_int(k["labor_flag"]), d(k["phi"]), d(k["theta"]),
        d(cal["labor"]), d(k["tol"]), i64(k["max_iter"]), d(k["dtol"]), i64(k["dmax"]), p(k["lam"]),
        C.c_int(k["nd"]), p(k["Ks"]), p(k["Kd"]), p(k["it"]), p(k["dit"]), p(k["st"]))


def test_ge_hist_batch_validates_before_device_work(pkg):
    rep = _ge_args(pkg)["a"]
    rep[3] = rep[2]
    cases = [(dict(r=None), BAD_ARG), (dict(v=None), BAD_ARG), (dict(s=None), BAD_ARG),
             (dict(P=None), BAD_ARG), (dict(Ks=None), BAD_ARG), (dict(Kd=None), BAD_ARG),
             (dict(it=None), BAD_ARG), (dict(dit=None), BAD_ARG), (dict(C=0), BAD_SHAPE),
             (dict(N=0), BAD_SHAPE), (dict(Na=1), BAD_SHAPE), (dict(max_iter=0), BAD_ARG),
             (dict(dmax=0), BAD_ARG), (dict(a=rep), BAD_ARG),
             (dict(r=np.array([0.0, -0.08])), BAD_ARG), (dict(r=np.array([0.0, np.nan])), BAD_ARG)]
    for over, code in cases:
        assert _ge_call(pkg, _ge_args(pkg, **over)) == code, over
    assert _ge_call(pkg, _ge_args(pkg)) == (OK if _has_gpu() else NO_DEVICE)  # NULL lambda_start


def test_egm_ge_hist_batch_validates_before_device_work(pkg):
    rep = _egm_args(pkg)["a"]
    rep[3] = rep[2]
    cases = [(dict(r=None), BAD_ARG), (dict(w=None), BAD_ARG), (dict(pc=None), BAD_ARG),
             (dict(st=None), BAD_ARG), (dict(dit=None), BAD_ARG), (dict(C=0), BAD_SHAPE),
             (dict(Na=1), BAD_SHAPE), (dict(N=17), BAD_SHAPE), (dict(a=rep), BAD_ARG),
             (dict(r=np.array([0.0, -0.08])), BAD_ARG), (dict(max_iter=0), BAD_ARG),
             (dict(dmax=0), BAD_ARG), (dict(labor_flag=1, phi=np.nan), NON_FINITE),
             (dict(labor_flag=1, theta=np.inf), NON_FINITE)]
    for over, code in cases:
        assert _egm_call(pkg, _egm_args(pkg, **over)) == code, over
    # phi is not looked at without the labour flag
    assert _egm_call(pkg, _egm_args(pkg, phi=np.nan)) == (OK if _has_gpu() else NO_DEVICE)


def test_no_device_is_loud(pkg):
    if _has_gpu():
        pytest.skip("device present")
    for rc in (_ge_call(pkg, _ge_args(pkg)), _egm_call(pkg, _egm_args(pkg)),
               _dist_call(pkg, _dist_args(pkg))):
        assert rc == NO_DEVICE
        assert b"no HIP device" in pkg.lib().aiy_last_error()
    with pytest.raises(pkg.AiyError) as e:
        pkg.dist_stationary_batch(np.linspace(0, 1, 5), np.eye(2),
                                  policy_idx=np.ones((3, 2, 5), np.int32))
    assert e.value.status == "AIY_NO_DEVICE"
    cal = pkg.calibration.aiyagari(Na=20)
    with pytest.raises(pkg.AiyError):
        pkg.ge_batch.hip_hist_batch_evaluator(cal, np.zeros((7, 20))).many(
            pkg.ge_batch.subtree(-0.05, 0.04, 1, 2))


# ------------------------------------------------------------------ the gateways
def _mex_vfi(pkg):
    k = _ge_args(pkg)
    cal = k["cal"]
    return [k["r"], np.asarray(k["v"]), k["a"], k["s"], np.asarray(k["P"]), cal["alpha"],
            cal["delta"], cal["beta"], cal["sigma"], cal["labor"], 1e-5, 100.0, 1e-10, 50.0, 1.0]


def _mex_egm(pkg, labor=False):
    k = _egm_args(pkg)
    cal = k["cal"]
    args = [k["r"], k["pc"].T, k["a"], k["s"], np.asarray(k["P"]), 1.0, cal["alpha"], cal["delta"],
            cal["beta"], cal["sigma"], cal["amin"], cal["labor"], 1e-5, 100.0, 1e-10, 50.0, 1.0,
            np.zeros((0, 0))]
    return args + ([1.0, 1.0] if labor else [])


def test_gateway_errors_leave_the_lock_balanced(pkg):
    if not mexstub.LIB.exists():
        pytest.skip("libmexstub.so not built")
    L = mexstub.lib()
    d0 = L.stub_lock_depth()

    def err(name, args, nlhs):
        with pytest.raises(mexstub.MexError) as e:
            mexstub.call(name, nlhs, *args)
        assert L.stub_lock_depth() == d0
        return e.value.id
    V, good = "aiy_ge_hist_batch_mex", _mex_vfi(pkg)
    assert err(V, good[:-1], 4) == "aiy:usage"                       # 14 inputs
    assert err(V, good + [np.zeros((7, 20)), 1.0], 4) == "aiy:usage"  # 17 inputs
    assert err(V, good, 5) == "aiy:usage"
    assert err(V, good + [np.zeros((7, 19))], 4) == "aiy:shape"       # lambda_start is N x Na
    bad = list(good); bad[3] = good[3][:-1]                           # s length != N
    assert err(V, bad, 4) == "aiy:shape"
    bad = list(good); bad[13] = 50.5                                  # dist_max_iter: an integer
    assert err(V, bad, 4) == "aiy:type"
    bad = list(good); bad[11] = np.array([100.0, 100.0])              # max_iter: a scalar
    assert err(V, bad, 4) == "aiy:type"
    bad = list(good); bad[13] = 0.0                                   # library status via the gateway
    assert err(V, bad, 4) == "aiy:BAD_ARG"
    a = good[2].copy(); a[3] = a[2]
    bad = list(good); bad[2] = a
    assert err(V, bad, 4) == "aiy:BAD_ARG"
    E, good = "aiy_egm_ge_hist_batch_mex", _mex_egm(pkg)
    assert err(E, good[:-1], 5) == "aiy:usage"                        # 17 inputs
    assert err(E, good + [1.0], 5) == "aiy:usage"                     # phi without theta
    assert err(E, good + [1.0, 1.0, 1.0], 5) == "aiy:usage"           # 21 inputs
    assert err(E, good, 6) == "aiy:usage"
    bad = list(good); bad[17] = np.zeros((7, 20))                     # lambda_start is Na x N
    assert err(E, bad, 5) == "aiy:shape"
    bad = list(good); bad[5] = np.ones(3)                             # w: a scalar or one per rate
    assert err(E, bad, 5) == "aiy:shape"
    bad = list(good); bad[15] = 0.0
    assert err(E, bad, 5) == "aiy:BAD_ARG"
    bad = _mex_egm(pkg, labor=True); bad[18] = np.nan
    assert err(E, bad, 5) == "aiy:NON_FINITE"
    if not _has_gpu():
        assert err(V, _mex_vfi(pkg), 4) == "aiy:NO_DEVICE"
        assert err(E, _mex_egm(pkg), 5) == "aiy:NO_DEVICE"
        assert err(E, _mex_egm(pkg, labor=True), 5) == "aiy:NO_DEVICE"


# ------------------------------------------------------------------ the host driver over the oracle
def _oracle_hist_evaluator(pkg, egm, Na=40):
    gb, cb = pkg.ge_batch, pkg.calibration
    if egm:
        cal, r0, w, guess = gb.egm_calibration(Na, False)
    else:
        cal = cb.aiyagari(Na=Na)
    a, s, P = cal["a_grid"], cal["s"], cal["P"]
    uni = np.full((cal["N"], Na), 1.0 / (cal["N"] * Na))

    def solve(start, r):
        if egm:
            return corc.egm_solve(start, a, s, P, r, w, cal["beta"], cal["sigma"], cal["amin"])
        return corc.vfi_solve(start, a, s, P, r, cb.wage(r, cal["alpha"], cal["delta"]),
                              cal["beta"], cal["sigma"])

    def supply(R):
        kw = dict(kp=R["policy_k"]) if egm else dict(idx=R["idx"])
        _, K, it, _ = corc.dist_stationary(uni, a, P, tol=1e-13, max_iter=100000, **kw)
        return K, it
    R0 = solve(guess if egm else np.zeros((cal["N"], Na)), 0.04)
    return gb.hist_evaluator(cal, solve, supply, R0["policy_c"] if egm else R0["v_old"]), cal


@pytest.mark.parametrize("egm", [False, True], ids=["vfi", "egm"])
def test_multisection_equals_bisection_over_the_oracle(pkg, egm):
    gb = pkg.ge_batch
    ev, cal = _oracle_hist_evaluator(pkg, egm)
    lo, hi = -0.05, 1 / cal["beta"] - 1
    A = gb.multisection(ev, lo, hi, levels=3)
    S = gb.bisection(ev, lo, hi)
    assert A.r_history == S.r_history and A.k_supply == S.k_supply and A.iters == S.iters
    assert A.k_demand == S.k_demand and A.r == S.r
    assert A.rounds == 4 and A.candidates == 7 + 7 + 7 + 1
    assert len(A.r_history) == 10 and all(math.isfinite(x) for x in A.k_supply)
    # a node's result: (K_s, K_d, iters, status, pushes); a failed solve has no supply
    v = ev(gb.Node(1, 0.01, lo, hi))
    assert len(v) == 5 and v[3] == 0 and v[4] > 1
    failing = gb.hist_evaluator(cal, lambda st, r: dict(iters=0, status=1), None, None)
    f = failing(gb.Node(1, 0.01, lo, hi))
    assert math.isnan(f[0]) and f[2:] == (0, 1, 0)
    with pytest.raises(gb.NodeFailed):
        gb.bisection(failing, lo, hi)


def test_supply_keyword_is_checked(pkg):
    gb = pkg.ge_batch
    with pytest.raises(ValueError):
        gb.aiyagari_vfi_multisection(Na=20, supply="histogramme")
    with pytest.raises(ValueError):
        gb.aiyagari_egm_multisection(Na=20, supply="")


# ------------------------------------------------------------------ the blocks, sanitized
def test_batch_blocks_under_sanitizers(tmp_path):
    exe = _build(tmp_path, "dist_batch_blocks_main.cpp",
                 ["-D__HIP_PLATFORM_AMD__", f"-I{ROCM}/include", f"-L{ROCM}/lib", "-lamdhip64",
                  f"-Wl,-rpath,{ROCM}/lib"])
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1",
               LSAN_OPTIONS=f"suppressions={ROOT / 'tests' / 'cpp' / 'lsan.supp'}:print_suppressions=0")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    assert r.stdout.strip().endswith("done") and "FAILED" not in r.stdout
