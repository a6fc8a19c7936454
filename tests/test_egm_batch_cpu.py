"""CPU: the batched EGM GE entry points without a GPU — argument validation before any device
work (library and gateway), the host driver (ge_batch.py: the EGM evaluators over the C
restatement, the path walk's handling of failed candidates) and the batch blocks' memory logic
in a stand-alone program built with AddressSanitizer and UBSan."""
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


def _ge_args(pkg, C_=2, Na=20, **over):
    """A valid aiy_egm_ge_batch argument list (as keyword dict, then flattened)."""
    cal, r0, w, guess = pkg.ge_batch.egm_calibration(Na, False)
    k = dict(r=np.linspace(0.0, 0.02, C_), w=np.full(C_, w), C=C_, pc=np.ascontiguousarray(guess),
             a=cal["a_grid"].copy(), s=cal["s"].copy(), P=np.asfortranarray(cal["P"]), N=cal["N"],
             Na=Na, alpha=0.36, delta=0.08, beta=0.96, sigma=5.0, amin=cal["amin"], labor_flag=0,
             phi=1.0, theta=1.0, labor=cal["labor"], tol=1e-5, max_iter=100, z1=1, k1=0.5, T=100,
             U=np.full((99, C_), 0.5, order="F"), nd=1, Ks=np.zeros(C_), Kd=np.zeros(C_),
             it=np.zeros(C_, np.int64), st=np.zeros(C_, np.int32))
    k.update(over)
    return k


def _ge_call(pkg, k):
    p = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)
    d, i64 = C.c_double, C.c_int64
    return pkg.lib().aiy_egm_ge_batch(
        p(k["r"]), p(k["w"]), i64(k["C"]), p(k["pc"]), p(k["a"]), p(k["s"]), p(k["P"]),
        i64(k["N"]), i64(k["Na"]), d(k["alpha"]), d(k["delta"]), d(k["beta"]), d(k["sigma"]),
        d(k["amin"]), C.c_int(k["labor_flag"]), d(k["phi"]), d(k["theta"]), d(k["labor"]),
        d(k["tol"]), i64(k["max_iter"]), i64(k["z1"]), d(k["k1"]), i64(k["T"]), p(k["U"]),
        C.c_int(k["nd"]), p(k["Ks"]), p(k["Kd"]), p(k["it"]), p(k["st"]))


def test_ge_batch_validates_before_device_work(pkg):
    """Each bad argument gives its status code, with or without a GPU (so: before device work)."""
    rep = _ge_args(pkg)["a"]
    rep[3] = rep[2]
    cases = [(dict(r=None), BAD_ARG), (dict(w=None), BAD_ARG), (dict(pc=None), BAD_ARG),
             (dict(st=None), BAD_ARG), (dict(U=None), BAD_ARG), (dict(C=0), BAD_SHAPE),
             (dict(Na=1), BAD_SHAPE), (dict(N=17), BAD_SHAPE), (dict(a=rep), BAD_ARG),
             (dict(r=np.array([0.0, -0.08])), BAD_ARG), (dict(r=np.array([0.0, np.nan])), BAD_ARG),
             (dict(z1=0), BAD_ARG), (dict(z1=8), BAD_ARG), (dict(max_iter=0), BAD_ARG),
             (dict(labor_flag=1, phi=np.nan), NON_FINITE),
             (dict(labor_flag=1, theta=np.inf), NON_FINITE)]
    for over, code in cases:
        assert _ge_call(pkg, _ge_args(pkg, **over)) == code, over
    # phi is not looked at without the labour flag
    import torch
    rc = _ge_call(pkg, _ge_args(pkg, phi=np.nan))
    assert rc == (OK if torch.cuda.is_available() else NO_DEVICE)


def test_no_device_is_loud(pkg):
    import torch
    if torch.cuda.is_available():
        pytest.skip("device present")
    assert _ge_call(pkg, _ge_args(pkg)) == NO_DEVICE
    assert b"no HIP device" in pkg.lib().aiy_last_error()


def test_solve_batch_dev_validates_before_device_work(pkg):
    """The device tier's argument errors need no workspace contents and no device."""
    L = pkg.lib()
    z = np.zeros(4)
    one, i1, s1 = np.zeros(1), np.zeros(1, np.int64), np.zeros(1, np.int32)
    p = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)

    def call(ws, Cn=1, r=one, pl=None, labor=0, phi=1.0, max_iter=5, st=s1):
        return L.aiy_egm_solve_batch_dev(ws, C.c_int64(Cn), p(r), p(one), p(z), p(z), p(z), p(z),
                                         C.c_double(0.96), C.c_double(5.0), C.c_double(0.0),
                                         C.c_int(labor), C.c_double(phi), C.c_double(1.0),
                                         C.c_double(1e-5), C.c_int64(max_iter), p(z), p(pl), p(i1),
                                         p(one), p(st), None)
    assert call(None) == BAD_ARG
    h = C.c_void_p()
    rc = L.aiy_ws_create(C.c_int64(2), C.c_int64(2), C.c_int64(1), C.byref(h))
    if rc != OK:  # no device: a workspace cannot be made; the NULL check above is what runs
        assert rc == NO_DEVICE
        return
    try:
        assert call(h, r=None) == BAD_ARG and call(h, st=None) == BAD_ARG
        assert call(h, Cn=0) == BAD_SHAPE
        assert call(h, labor=1) == BAD_ARG                 # labour needs policy_l
        assert call(h, labor=1, pl=z, phi=np.nan) == NON_FINITE
        assert call(h, max_iter=-1) == BAD_ARG
        assert L.aiy_ws_set_egm_batch(h, C.c_int(-2)) == BAD_ARG
    finally:
        L.aiy_ws_destroy(h)


def _mex_args(pkg, labor=False):
    k = _ge_args(pkg)
    args = [k["r"], k["pc"].T, k["a"], k["s"], np.asarray(k["P"]), 1.0, 0.36, 0.08, 0.96, 5.0,
            k["amin"], k["labor"], 1e-5, 100.0, 1.0, 0.5, np.asarray(k["U"]), 1.0]
    return args + ([1.0, 1.0] if labor else [])


def test_gateway_errors_leave_the_lock_balanced(pkg):
    if not mexstub.LIB.exists():
        pytest.skip("libmexstub.so not built")
    L = mexstub.lib()
    d0 = L.stub_lock_depth()
    good = _mex_args(pkg)

    def err(args, nlhs=4):
        with pytest.raises(mexstub.MexError) as e:
            mexstub.call("aiy_egm_ge_batch_mex", nlhs, *args)
        assert L.stub_lock_depth() == d0
        return e.value.id
    assert err(good[:-1]) == "aiy:usage"                       # 17 inputs
    assert err(good + [1.0]) == "aiy:usage"                    # phi without theta
    assert err(good + [1.0, 1.0, 1.0]) == "aiy:usage"          # 21 inputs
    assert err(good, nlhs=5) == "aiy:usage"
    bad = list(good); bad[16] = np.full((99, 3), 0.5)          # a column of uniforms per rate
    assert err(bad) == "aiy:shape"
    bad = list(good); bad[5] = np.ones(3)                      # w: a scalar or one per rate
    assert err(bad) == "aiy:shape"
    bad = list(good); bad[3] = good[3][:-1]                    # s length != N
    assert err(bad) == "aiy:shape"
    bad = list(good); bad[14] = 1.5                            # z1 must be an integer
    assert err(bad) == "aiy:type"
    bad = list(good); bad[13] = np.array([100.0, 100.0])       # max_iter must be a scalar
    assert err(bad) == "aiy:type"
    a = good[2].copy(); a[3] = a[2]                            # library status through the gateway
    bad = list(good); bad[2] = a
    assert err(bad) == "aiy:BAD_ARG"
    bad = _mex_args(pkg, labor=True); bad[18] = np.nan
    assert err(bad) == "aiy:NON_FINITE"
    import torch
    if not torch.cuda.is_available():
        assert err(good) == "aiy:NO_DEVICE"
        assert err(_mex_args(pkg, labor=True)) == "aiy:NO_DEVICE"


def _oracle_evaluator(pkg, labor, Na=40, T=2000):
    gb = pkg.ge_batch
    cal, r0, w, guess = gb.egm_calibration(Na, labor)
    a, s, P = cal["a_grid"], cal["s"], cal["P"]

    def solve(pc, r, w_):
        if labor:
            return corc.labor_egm_solve(pc, a, s, P, r, w_, cal["beta"], cal["sigma"], 1.0, 1.0,
                                        cal["amin"])
        return corc.egm_solve(pc, a, s, P, r, w_, cal["beta"], cal["sigma"], cal["amin"])

    def simulate(pk, z1, k1, u):
        return corc.sim_capital(pk, a, P, z1 - 1, k1, u)
    pc0 = solve(guess, r0, w)["policy_c"]
    return gb.egm_evaluator(cal, solve, simulate, pc0, w, labor, T=T), cal


@pytest.mark.parametrize("labor", [False, True])
def test_multisection_equals_bisection_over_the_oracle(pkg, labor):
    gb = pkg.ge_batch
    ev, cal = _oracle_evaluator(pkg, labor)
    lo, hi = -0.05, 1 / cal["beta"] - 1
    A = gb.multisection(ev, lo, hi, levels=3)
    S = gb.bisection(ev, lo, hi)
    assert A.r_history == S.r_history and A.k_supply == S.k_supply and A.iters == S.iters
    assert A.k_demand == S.k_demand and A.r == S.r
    assert A.rounds == 4 and A.candidates == 7 + 7 + 7 + 1
    assert len(A.r_history) == 10 and all(math.isfinite(x) for x in A.k_supply)


def test_walk_raises_on_a_failed_node_on_the_path_only(pkg):
    gb = pkg.ge_batch
    root = 0.0123

    def make(failed):
        def ev(n):
            return (n.r - root + 100.0, 100.0, 1, 1 if n.r in failed else 0)
        return ev
    S = gb.bisection(make(set()), -0.05, 0.04)
    nodes = gb.subtree(-0.05, 0.04, 1, 6)
    on_path = set(S.r_history)
    off = [n.r for n in nodes if n.r not in on_path]
    assert off and len(S.r_history) == 10
    # every off-path node failed: the same trace, through the plain and the batched interface
    A = gb.multisection(make(set(off)), -0.05, 0.04, levels=6)
    assert A.r_history == S.r_history and A.k_supply == S.k_supply
    evm = make(set(off))
    evm.many = lambda ns: [make(set(off))(n) for n in ns]
    assert gb.multisection(evm, -0.05, 0.04, levels=6).r_history == S.r_history
    # a failed node on the path raises, in the tree walk and in the sequential twin
    for bad in (S.r_history[0], S.r_history[4], S.r_history[9]):
        with pytest.raises(gb.NodeFailed) as e:
            gb.multisection(make({bad}), -0.05, 0.04, levels=6)
        assert e.value.node.r == bad and e.value.status == 1
        with pytest.raises(gb.NodeFailed):
            gb.bisection(make({bad}), -0.05, 0.04)
    # results without a status field (the VFI evaluators) walk as before
    B = gb.multisection(lambda n: (n.r - root + 100.0, 100.0, 1), -0.05, 0.04, levels=6)
    assert B.r_history == S.r_history


def test_batch_blocks_under_sanitizers(tmp_path):
    exe = _build(tmp_path, "egm_batch_blocks_main.cpp",
                 ["-D__HIP_PLATFORM_AMD__", f"-I{ROCM}/include", f"-L{ROCM}/lib", "-lamdhip64",
                  f"-Wl,-rpath,{ROCM}/lib"])
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1",
               LSAN_OPTIONS=f"suppressions={ROOT / 'tests' / 'cpp' / 'lsan.supp'}:print_suppressions=0")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    assert r.stdout.strip().endswith("done") and "FAILED" not in r.stdout
