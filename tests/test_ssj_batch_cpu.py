"""No GPU: which refusal aiy_ssj_jacobian_batch answers before it asks for a device (in the
manner of test_ssj_cpu.py: each defect and its message, defect pairs to pin the order of the
checks, the economy's index in the per-economy messages), and jacobian_batch's own shape checks."""
import ctypes as C

import numpy as np
import pytest

N_, NA_, NC_, T_ = 2, 5, 3, 4
i64, d = C.c_int64, C.c_double
NO_DEVICE = (5, "no HIP device visible")
JAC_FIT = ("Jacobian: the transition passes' arrays exceed one CU's LDS "
           "(aiy_transition_batch's fit rules)")


def _base():
    n, tt = N_ * NA_, T_ * T_
    return dict(C=NC_, T=T_, N=N_, Na=NA_, h=1e-4, chunk=0,
                pc=np.ones(NC_ * n), lam=np.full(NC_ * n, 1.0 / n),
                r=np.full(NC_, 0.02), w=np.full(NC_, 1.2),
                a=np.tile(np.arange(NA_, dtype=np.float64), NC_), s=np.tile([0.8, 1.2], NC_),
                P=np.full(NC_ * N_ * N_, 0.5), beta=np.full(NC_, 0.96), sigma=np.full(NC_, 5.0),
                amin=np.zeros(NC_), J_r=np.zeros(NC_ * tt), J_w=np.zeros(NC_ * tt),
                F_r=np.zeros(NC_ * tt), F_w=np.zeros(NC_ * tt), E=np.zeros(NC_ * T_ * n),
                sb=np.zeros(NC_, np.int32), sf=np.zeros(NC_, np.int32))


def _set(key, index, value):
    return lambda a: a[key].__setitem__(index, value)


DEFECTS = {
    "valid": lambda a: None, "C0": lambda a: a.update(C=0), "T0": lambda a: a.update(T=0),
    "T32769": lambda a: a.update(T=32769),
    "N0": lambda a: a.update(N=0), "Na1": lambda a: a.update(Na=1), "N17": lambda a: a.update(N=17),
    "Na1025": lambda a: a.update(Na=1025),
    "h0": lambda a: a.update(h=0.0), "h_nan": lambda a: a.update(h=np.nan),
    "chunk_neg": lambda a: a.update(chunk=-1), "chunk_big": lambda a: a.update(chunk=32768),
    # economy 1's grid is a[5:10], economy 2's a[10:15]
    "a1_nan": _set("a", NA_ + 0, np.nan), "a1_dec": _set("a", NA_ + 2, 0.5),
    "a2_rep": _set("a", 2 * NA_ + 4, 3.0), "a0_rep": _set("a", 4, 3.0),
    "r0_m1": _set("r", 0, -1.0), "r2_nan": _set("r", 2, np.nan), "w1_nan": _set("w", 1, np.nan),
    "w1_inf": _set("w", 1, np.inf),
    "beta2_0": _set("beta", 2, 0.0), "beta0_nan": _set("beta", 0, np.nan),
    "sigma1_neg": _set("sigma", 1, -2.0), "sigma2_inf": _set("sigma", 2, np.inf),
    "amin1_nan": _set("amin", 1, np.nan), "amin0_inf": _set("amin", 0, -np.inf),
    **{f"null:{k}": (lambda a, k=k: a.update({k: None}))
       for k in ("pc", "lam", "r", "w", "a", "s", "P", "beta", "sigma", "amin", "J_r", "J_w", "F_r",
                 "F_w", "E", "sb", "sf")},
}


def _p(x):
    return None if x is None else x.ctypes.data_as(C.c_void_p)


def _call(L, a):
    return L.aiy_ssj_jacobian_batch(
        i64(a["C"]), _p(a["pc"]), _p(a["lam"]), _p(a["r"]), _p(a["w"]), _p(a["a"]), _p(a["s"]),
        _p(a["P"]), i64(a["N"]), i64(a["Na"]), _p(a["beta"]), _p(a["sigma"]), _p(a["amin"]),
        i64(a["T"]), d(a["h"]), _p(a["J_r"]), _p(a["J_w"]), _p(a["F_r"]), _p(a["F_w"]), _p(a["E"]),
        _p(a["sb"]), _p(a["sf"]), None, i64(a["chunk"]))


NULL = (6, "NULL argument")
H_BAD = (6, "h must be positive and finite")
CHUNK = (6, "chunk must be in [0, 32767] (0: the default)")
R_BAD = "r_ss must be finite with 1 + r_ss > 0"
# defects -> the answer; a defect pair shows which check comes first
EXPECTED = {
    **{f"null:{k}": NULL for k in ("pc", "lam", "r", "w", "a", "s", "P", "beta", "sigma", "amin",
                                   "J_r", "J_w", "sb", "sf")},
    "null:pc+C0": NULL,
    "null:sf+T0": NULL,
    "C0": (1, "need 1 <= C <= 2^24"),
    "C0+N0": (1, "need 1 <= C <= 2^24"),
    "N0": (1, "need N >= 1 and Na >= 2"),
    "Na1": (1, "need N >= 1 and Na >= 2"),
    "N0+T0": (1, "need N >= 1 and Na >= 2"),
    "N17": (6, JAC_FIT),
    "Na1025": (6, JAC_FIT),
    "N17+T0": (6, JAC_FIT),
    "T0": (1, "T must be in [1, 32768]"),
    "T32769": (1, "T must be in [1, 32768]"),
    "T0+h_nan": (1, "T must be in [1, 32768]"),
    "h0": H_BAD,
    "h_nan": H_BAD,
    "h_nan+chunk_neg": H_BAD,
    "chunk_neg": CHUNK,
    "chunk_big": CHUNK,
    "chunk_neg+a0_rep": CHUNK,
    "a1_nan": (2, "economy 1: a_grid(1) is not finite"),
    "a1_dec": (6, "economy 1: a_grid must be non-decreasing (a_grid(3) < a_grid(2))"),
    "a2_rep": (6, "economy 2: grid must be strictly increasing (point 5 repeats point 4)"),
    "a0_rep": (6, "economy 0: grid must be strictly increasing (point 5 repeats point 4)"),
    "a2_rep+a1_dec": (6, "economy 1: a_grid must be non-decreasing (a_grid(3) < a_grid(2))"),
    "r0_m1": (6, "economy 0: " + R_BAD),
    "r2_nan": (6, "economy 2: " + R_BAD),
    "r0_m1+a1_dec": (6, "economy 0: " + R_BAD),          # economy by economy, not check by check
    "r2_nan+a2_rep": (6, "economy 2: grid must be strictly increasing (point 5 repeats point 4)"),
    "w1_nan": (6, "economy 1: w_ss must be finite"),
    "w1_inf": (6, "economy 1: w_ss must be finite"),
    "w1_nan+r2_nan": (6, "economy 1: w_ss must be finite"),
    "beta2_0": (6, "economy 2: beta must be positive and finite"),
    "beta0_nan": (6, "economy 0: beta must be positive and finite"),
    "beta0_nan+sigma1_neg": (6, "economy 0: beta must be positive and finite"),
    "sigma1_neg": (6, "economy 1: sigma must be positive and finite"),
    "sigma2_inf": (6, "economy 2: sigma must be positive and finite"),
    "sigma1_neg+amin1_nan": (6, "economy 1: sigma must be positive and finite"),
    "amin1_nan": (6, "economy 1: amin must be finite"),
    "amin0_inf": (6, "economy 0: amin must be finite"),
    "amin1_nan+beta2_0": (6, "economy 1: amin must be finite"),
    "null:F_r": NO_DEVICE,
    "null:F_w": NO_DEVICE,
    "null:E": NO_DEVICE,
    "valid": NO_DEVICE,
}


@pytest.mark.parametrize("defects", sorted(EXPECTED))
def test_jacobian_batch_refusal(pkg, defects):
    want = EXPECTED[defects]
    if want == NO_DEVICE:
        import torch
        if torch.cuda.is_available():
            return  # not a refusal: with a device the call would run
    a = _base()
    for x in defects.split("+"):
        DEFECTS[x](a)
    L = pkg.lib()
    rc = _call(L, a)
    assert (rc, L.aiy_last_error().decode()) == want


def _fake_ss(N, Na):
    cal = dict(a_grid=np.arange(Na, dtype=np.float64), s=np.ones(N), P=np.full((N, N), 1.0 / N),
               beta=0.96, sigma=2.0, amin=0.0, N=N, Na=Na)
    return dict(r=0.03, w=1.0, K=1.0, policy_c=np.ones((N, Na)), lam=np.full((N, Na), 1.0 / (N * Na)),
                cal=cal)


def test_jacobian_batch_refuses_mixed_shapes(pkg):
    with pytest.raises(ValueError, match="economy 1 has another N or Na"):
        pkg.jacobian_batch([_fake_ss(2, 5), _fake_ss(2, 6)], 4)
    with pytest.raises(ValueError, match="economy 2 has another N or Na"):
        pkg.jacobian_batch([_fake_ss(2, 5), _fake_ss(2, 5), _fake_ss(3, 5)], 4)
    with pytest.raises(ValueError, match="at least one"):
        pkg.jacobian_batch([], 4)
    bad = _fake_ss(2, 5)
    bad["lam"] = np.ones((2, 4))
    with pytest.raises(ValueError, match="economy 1: "):
        pkg.jacobian_batch([_fake_ss(2, 5), bad], 4)
