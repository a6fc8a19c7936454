"""CPU: the batched labour VFI entry points without a GPU — argument validation before any device
work (library and gateway), the host driver (ge_batch.py: the labour evaluator over the C
restatement) and the batched sweep's index arithmetic (csrc/wide_batch.hpp) in a stand-alone
program built with AddressSanitizer and UBSan."""
import ctypes as C
import math
import subprocess

import numpy as np
import pytest

from oracle import corc
from oracle import np_oracle as no
from tests import mexstub
from tests.test_host_layer_cpu import _build

OK, BAD_SHAPE, NON_FINITE, NO_DEVICE, BAD_ARG = 0, 1, 2, 5, 6
PSI, ETA = 1.0, 2.0


def _ge_args(pkg, C_=2, Na=20, **over):
    """A valid aiy_labor_ge_batch argument list (as keyword dict)."""
    cal, L = pkg.ge_batch.labor_calibration(Na)
    N = cal["N"]
    z = lambda: np.zeros((N, Na), order="F")
    k = dict(r=np.linspace(0.0, 0.02, C_), C=C_, v=z(), vn=z(), pk=z(), pl=z(), pc=z(),
             lin=np.ones((N, Na), np.int32, order="F"), a=cal["a_grid"].copy(), s=cal["s"].copy(),
             P=np.asfortranarray(cal["P"]), L=np.ascontiguousarray(L), N=N, Na=Na, Nl=L.size,
             alpha=0.36, delta=0.08, beta=0.96, sigma=5.0, psi=PSI, eta=ETA, labor=cal["labor"],
             tol=1e-5, max_iter=100, z1=1, k1=0.5, T=100, U=np.full((99, C_), 0.5, order="F"), nd=1,
             Ks=np.zeros(C_), Kd=np.zeros(C_), it=np.zeros(C_, np.int64))
    k.update(over)
    return k


def _ge_call(pkg, k):
    p = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)
    d, i64 = C.c_double, C.c_int64
    return pkg.lib().aiy_labor_ge_batch(
        p(k["r"]), i64(k["C"]), p(k["v"]), p(k["vn"]), p(k["pk"]), p(k["pl"]), p(k["pc"]),
        p(k["lin"]), p(k["a"]), p(k["s"]), p(k["P"]), p(k["L"]), i64(k["N"]), i64(k["Na"]),
        i64(k["Nl"]), d(k["alpha"]), d(k["delta"]), d(k["beta"]), d(k["sigma"]), d(k["psi"]),
        d(k["eta"]), d(k["labor"]), d(k["tol"]), i64(k["max_iter"]), i64(k["z1"]), d(k["k1"]),
        i64(k["T"]), p(k["U"]), C.c_int(k["nd"]), p(k["Ks"]), p(k["Kd"]), p(k["it"]))


def test_ge_batch_validates_before_device_work(pkg):
    """Each bad argument gives its status code, with or without a GPU (so: before device work);
    the nullable starts are accepted."""
    rep = _ge_args(pkg)["a"]
    rep[3] = rep[2]
    cases = [(dict(r=None), BAD_ARG), (dict(v=None), BAD_ARG), (dict(L=None), BAD_ARG),
             (dict(it=None), BAD_ARG), (dict(U=None), BAD_ARG), (dict(C=0), BAD_SHAPE),
             (dict(Na=1), BAD_SHAPE), (dict(Nl=0), BAD_SHAPE), (dict(a=rep), BAD_ARG),
             (dict(r=np.array([0.0, -0.08])), BAD_ARG), (dict(r=np.array([0.0, np.nan])), BAD_ARG),
             (dict(z1=0), BAD_ARG), (dict(z1=8), BAD_ARG), (dict(max_iter=0), BAD_ARG),
             (dict(T=0), BAD_SHAPE), (dict(psi=np.nan), NON_FINITE), (dict(eta=np.inf), NON_FINITE)]
    for over, code in cases:
        assert _ge_call(pkg, _ge_args(pkg, **over)) == code, over
    import torch
    rc = _ge_call(pkg, _ge_args(pkg, vn=None, pk=None, pl=None, pc=None, lin=None))
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
    z, z2 = np.zeros(8), np.zeros(8)
    one, i1, s1 = np.zeros(1), np.zeros(1, np.int64), np.zeros(1, np.int32)
    lin = np.zeros(8, np.int32)
    p = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)

    def call(ws, Cn=1, r=one, w=one, va=z, vb=z2, lab=z, li=lin, max_iter=5, it=i1, which=s1):
        return L.aiy_labor_vfi_solve_batch_dev(
            ws, C.c_int64(Cn), p(r), p(w), p(va), p(vb), p(z), p(z), p(z), p(lab),
            C.c_double(0.96), C.c_double(5.0), C.c_double(PSI), C.c_double(ETA), C.c_double(1e-5),
            C.c_int64(max_iter), C.c_int(0), p(li), None, None, None, p(it), p(which), None)
    assert call(None) == BAD_ARG
    assert L.aiy_ws_set_labor_batch(None, C.c_int(1)) == BAD_ARG
    assert L.aiy_ws_labor_batch_counts(None, None, None) == BAD_ARG
    h = C.c_void_p()
    rc = L.aiy_ws_create(C.c_int64(2), C.c_int64(2), C.c_int64(2), C.byref(h))
    if rc != OK:  # no device: a workspace cannot be made; the NULL checks above are what runs
        assert rc == NO_DEVICE
        return
    try:
        for bad in (dict(r=None), dict(w=None), dict(va=None), dict(vb=None), dict(lab=None),
                    dict(li=None), dict(it=None), dict(which=None), dict(vb=z)):
            assert call(h, **bad) == BAD_ARG, bad
        assert call(h, Cn=0) == BAD_SHAPE and call(h, Cn=(1 << 20) + 1) == BAD_SHAPE
        assert call(h, max_iter=0) == BAD_ARG
        assert call(h, r=np.array([np.nan])) == NON_FINITE
        assert call(h, w=np.array([np.inf])) == NON_FINITE
        assert L.aiy_ws_set_labor_batch(h, C.c_int(-1)) == BAD_ARG
        a, b = C.c_int64(-1), C.c_int64(-1)
        assert L.aiy_ws_labor_batch_counts(h, C.byref(a), C.byref(b)) == OK
        assert (a.value, b.value) == (0, 0)
    finally:
        L.aiy_ws_destroy(h)
    # C * Nl * N * Na past int32 (host arithmetic only: r and w are the only arrays read first)
    rc = L.aiy_ws_create(C.c_int64(16), C.c_int64(1 << 12), C.c_int64(16), C.byref(h))
    assert rc == OK
    try:
        big = np.zeros(1 << 12)
        assert call(h, Cn=1 << 12, r=big, w=big) == BAD_SHAPE
    finally:
        L.aiy_ws_destroy(h)


def _mex_args(pkg):
    k = _ge_args(pkg)
    return [k["r"], k["v"], k["vn"], k["pk"], k["pl"], k["pc"], k["lin"].astype(np.float64), k["a"],
            k["s"], np.asarray(k["P"]), k["L"], 0.36, 0.08, 0.96, 5.0, PSI, ETA, k["labor"], 1e-5,
            100.0, 1.0, 0.5, np.asarray(k["U"]), 1.0]


def test_gateway_errors_leave_the_lock_balanced(pkg):
    if not mexstub.LIB.exists():
        pytest.skip("libmexstub.so not built")
    L = mexstub.lib()
    d0 = L.stub_lock_depth()
    good = _mex_args(pkg)

    def err(args, nlhs=3):
        with pytest.raises(mexstub.MexError) as e:
            mexstub.call("aiy_labor_ge_batch_mex", nlhs, *args)
        assert L.stub_lock_depth() == d0
        return e.value.id
    assert err(good[:-1]) == "aiy:usage"                       # 23 inputs
    assert err(good + [1.0]) == "aiy:usage"                    # 25 inputs
    assert err(good, nlhs=4) == "aiy:usage"
    bad = list(good); bad[22] = np.full((99, 3), 0.5)          # a column of uniforms per rate
    assert err(bad) == "aiy:shape"
    bad = list(good); bad[2] = np.zeros((7, 19))               # v_new: N x Na or []
    assert err(bad) == "aiy:shape"
    bad = list(good); bad[8] = good[8][:-1]                    # s length != N
    assert err(bad) == "aiy:shape"
    bad = list(good); bad[20] = 1.5                            # z1 must be an integer
    assert err(bad) == "aiy:type"
    bad = list(good); bad[19] = np.array([100.0, 100.0])       # max_iter must be a scalar
    assert err(bad) == "aiy:type"
    bad = list(good); bad[6] = good[6] + 0.5                   # policy_lin must hold integers
    assert err(bad) == "aiy:type"
    a = good[7].copy(); a[3] = a[2]                            # library status through the gateway
    bad = list(good); bad[7] = a
    assert err(bad) == "aiy:BAD_ARG"
    bad = list(good); bad[15] = np.nan
    assert err(bad) == "aiy:NON_FINITE"
    import torch
    if not torch.cuda.is_available():
        assert err(good) == "aiy:NO_DEVICE"
        empty = list(good)
        for q in range(2, 7):
            empty[q] = np.zeros((0, 0))                        # [] starts are accepted
        assert err(empty) == "aiy:NO_DEVICE"


def test_multisection_equals_bisection_over_the_oracle(pkg):
    """The driver's tree walk over the labour evaluator with oracle callables at Na = 20: the
    sequential bisection's trace."""
    gb = pkg.ge_batch
    cal, L = gb.labor_calibration(20)
    a, s, P = cal["a_grid"], cal["s"], cal["P"]

    def solve(st, r, w):
        return corc.labor_vfi_solve(st["v_old"], a, s, P, L, r, w, cal["beta"], cal["sigma"], PSI,
                                    ETA)

    def simulate(pk, z1, k1, u):
        return corc.sim_capital(pk, a, P, z1 - 1, k1, u)
    R0 = solve(dict(v_old=np.zeros((cal["N"], 20))), 0.04, no.wage(0.04, 0.36, 0.08))
    ev = gb.labor_vfi_evaluator(cal, solve, simulate, gb.labor_start(dict(R0, lin=R0["lin"] + 1)),
                                T=2000)
    lo, hi = -0.05, 1 / cal["beta"] - 1
    A = gb.multisection(ev, lo, hi, levels=3)
    S = gb.bisection(ev, lo, hi)
    assert A.r_history == S.r_history and A.k_supply == S.k_supply and A.iters == S.iters
    assert A.k_demand == S.k_demand and A.r == S.r
    assert A.rounds == 4 and A.candidates == 7 + 7 + 7 + 1
    assert len(A.r_history) == 10 and all(math.isfinite(x) for x in A.k_supply)


def test_wide_batch_index_arithmetic_under_sanitizers(tmp_path):
    exe = _build(tmp_path, "wide_batch_main.cpp")
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    assert r.stdout.strip().endswith("done") and "FAILED" not in r.stdout
