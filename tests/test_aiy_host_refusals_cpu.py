"""No GPU: which refusal an Aiyagari host entry point answers, and in which order.

Every host entry validates its arguments before it asks for a device, and a caller with two
defects sees the first check of that entry's own sequence.  The sequences differ between entries
(the solves test `iters` ahead of everything else, aiy_egm_ge_batch tests N <= 16 before T and
z1, aiy_labor_ge_batch tests psi / eta where the EGM entries test phi / theta, the histogram
entries have dist_max_iter where the chains have T and z1), so each row below is one
(entry, defect) or one (entry, two defects) with the status and the full aiy_last_error() text.
The expectations are what the library answered before the Aiyagari host tier moved onto the typed
staging helpers: `python -m tests.test_aiy_host_refusals_cpu --record` prints them from the
library in the tree.

Shapes: N = 2, Na = 5, Nl = 2, C = 3, T = 4.

A row recorded as AIY_NO_DEVICE is a call that passed every host check: what it has wrong (or
nothing, the `valid` rows) is looked at behind the device query, if at all — psi and eta of the
single labour solves, T and z1 of aiy_sim_capital, a repeated grid point where nothing
interpolates, the nullable arguments.  With a device present such a row would run (and some would
read past these tiny arrays), so it is asked only where there is none."""
import ctypes as C
import sys

import numpy as np
import pytest

N, NA, NL, NC, T = 2, 5, 2, 3, 4
NO_DEVICE = (5, "no HIP device visible")


def _base():
    """Fresh, valid, flat arguments."""
    n = N * NA
    return dict(
        N=N, Na=NA, Nl=NL, C=NC, T=T, z1=1, max_iter=5, dmax=5, psi=1.0, eta=2.0, phi=1.0,
        theta=1.0, labor_flag=1,
        r=np.array([0.01, 0.02, 0.03]), w=np.full(NC, 1.2), a=np.arange(NA, dtype=np.float64),
        s=np.array([0.8, 1.2]), P=np.full(N * N, 0.5), L=np.array([0.5, 1.0]),
        v=np.zeros(n), vnew=np.zeros(n), pk=np.zeros(n), pl=np.zeros(n), pc=np.ones(n),
        pcn=np.zeros(n), lin=np.ones(n, np.int32), idx=np.ones(NC * n, np.int32), kp=None,
        lam=np.full(NC * n, 1.0 / n), U=np.full((T - 1) * NC, 0.5), Ks=np.zeros(NC),
        Kd=np.zeros(NC), it=np.zeros(NC, np.int64), dit=np.zeros(NC, np.int64),
        st=np.zeros(NC, np.int32), dist=np.zeros(NC), iters=np.zeros(1, np.int64),
        simk=np.zeros(T), simz=np.zeros(T, np.int32))


def _set(key, idx, v):
    def f(a):
        if a[key] is not None:  # (a row may null the same argument)
            a[key][idx] = v
    return f


DEFECTS = {
    "valid": lambda a: None,
    "C0": lambda a: a.update(C=0), "N0": lambda a: a.update(N=0), "N17": lambda a: a.update(N=17),
    "Na1": lambda a: a.update(Na=1), "Nl0": lambda a: a.update(Nl=0), "T0": lambda a: a.update(T=0),
    "z1_0": lambda a: a.update(z1=0), "z1_big": lambda a: a.update(z1=N + 1),
    "maxiter0": lambda a: a.update(max_iter=0), "dmax0": lambda a: a.update(dmax=0),
    "psi_nan": lambda a: a.update(psi=np.nan), "eta_inf": lambda a: a.update(eta=np.inf),
    "phi_nan": lambda a: a.update(phi=np.nan), "theta_inf": lambda a: a.update(theta=np.inf),
    "noflag": lambda a: a.update(labor_flag=0),
    "lottery": lambda a: a.update(idx=None, kp=np.zeros(NC * N * NA)),
    # three places, so that a pair of them shows which test of the grid comes first
    "a_nan": _set("a", 0, np.nan), "a_dec": _set("a", 2, 0.5), "a_rep": _set("a", 4, 3.0),
    "r_bad": _set("r", -1, -1.0), "r_nan": _set("r", -1, np.nan),     # the last candidate's
}


def _apply(a, defect):
    if defect.startswith("null:"):
        a[defect[5:]] = None
    else:
        DEFECTS[defect](a)


def _p(x):
    return None if x is None else x.ctypes.data_as(C.c_void_p)


i64, d, ci = C.c_int64, C.c_double, C.c_int
R, W, BETA, SIGMA, AMIN, ALPHA, DELTA, LABOR, TOL = 0.02, 1.2, 0.96, 5.0, 0.0, 0.36, 0.08, 1.0, 1e-5


# ---- one caller per entry point: a -> status
def _vfi_sweep(L, a):
    return L.aiy_vfi_sweep(_p(a["v"]), _p(a["a"]), _p(a["s"]), _p(a["P"]), i64(a["N"]),
                           i64(a["Na"]), d(R), d(W), d(BETA), d(SIGMA), _p(a["vnew"]), _p(a["pk"]),
                           _p(a["pc"]), _p(a["lin"]))


def _vfi_solve(L, a):
    return L.aiy_vfi_solve(_p(a["v"]), _p(a["a"]), _p(a["s"]), _p(a["P"]), i64(a["N"]),
                           i64(a["Na"]), d(R), d(W), d(BETA), d(SIGMA), d(TOL), i64(a["max_iter"]),
                           _p(a["vnew"]), _p(a["pk"]), _p(a["pc"]), _p(a["lin"]), _p(a["iters"]))


def _labor_sweep(L, a):
    return L.aiy_labor_vfi_sweep(_p(a["v"]), _p(a["a"]), _p(a["s"]), _p(a["P"]), _p(a["L"]),
                                 i64(a["N"]), i64(a["Na"]), i64(a["Nl"]), d(R), d(W), d(BETA),
                                 d(SIGMA), d(a["psi"]), d(a["eta"]), _p(a["vnew"]), _p(a["pk"]),
                                 _p(a["pl"]), _p(a["pc"]), _p(a["lin"]))


def _labor_solve(L, a):
    return L.aiy_labor_vfi_solve(_p(a["v"]), _p(a["a"]), _p(a["s"]), _p(a["P"]), _p(a["L"]),
                                 i64(a["N"]), i64(a["Na"]), i64(a["Nl"]), d(R), d(W), d(BETA),
                                 d(SIGMA), d(a["psi"]), d(a["eta"]), d(TOL), i64(a["max_iter"]),
                                 _p(a["vnew"]), _p(a["pk"]), _p(a["pl"]), _p(a["pc"]), _p(a["lin"]),
                                 _p(a["iters"]))


def _egm_step(L, a):
    return L.aiy_egm_step(_p(a["pc"]), _p(a["a"]), _p(a["s"]), _p(a["P"]), i64(a["N"]),
                          i64(a["Na"]), d(R), d(W), d(BETA), d(SIGMA), d(AMIN), _p(a["pcn"]),
                          _p(a["pk"]), _p(a["dist"]))


def _egm_solve(L, a):
    return L.aiy_egm_solve(_p(a["pc"]), _p(a["a"]), _p(a["s"]), _p(a["P"]), i64(a["N"]),
                           i64(a["Na"]), d(R), d(W), d(BETA), d(SIGMA), d(AMIN), d(TOL),
                           i64(a["max_iter"]), _p(a["pk"]), _p(a["dist"]), _p(a["iters"]))


def _labor_egm_step(L, a):
    return L.aiy_labor_egm_step(_p(a["pc"]), _p(a["a"]), _p(a["s"]), _p(a["P"]), i64(a["N"]),
                                i64(a["Na"]), d(R), d(W), d(BETA), d(SIGMA), d(a["phi"]),
                                d(a["theta"]), d(AMIN), _p(a["pcn"]), _p(a["pk"]), _p(a["pl"]),
                                _p(a["dist"]))


def _labor_egm_solve(L, a):
    return L.aiy_labor_egm_solve(_p(a["pc"]), _p(a["a"]), _p(a["s"]), _p(a["P"]), i64(a["N"]),
                                 i64(a["Na"]), d(R), d(W), d(BETA), d(SIGMA), d(a["phi"]),
                                 d(a["theta"]), d(AMIN), d(TOL), i64(a["max_iter"]), _p(a["pk"]),
                                 _p(a["pl"]), _p(a["dist"]), _p(a["iters"]))


def _sim(L, a):
    return L.aiy_sim_capital(_p(a["pk"]), ci(1), _p(a["a"]), _p(a["P"]), i64(a["N"]), i64(a["Na"]),
                             i64(a["z1"]), d(1.0), i64(a["T"]), _p(a["U"]), _p(a["Ks"]),
                             _p(a["simk"]), _p(a["simz"]))


def _dist(L, a):
    return L.aiy_dist_stationary(_p(a["idx"]), _p(a["kp"]), ci(1), _p(a["a"]), _p(a["P"]),
                                 i64(a["N"]), i64(a["Na"]), d(1e-10), i64(a["max_iter"]),
                                 _p(a["lam"]), _p(a["Ks"]), _p(a["iters"]), _p(a["dist"]))


def _dist_batch(L, a):
    return L.aiy_dist_stationary_batch(i64(a["C"]), _p(a["idx"]), _p(a["kp"]), ci(1), _p(a["a"]),
                                       _p(a["P"]), i64(a["N"]), i64(a["Na"]), d(1e-10),
                                       i64(a["max_iter"]), _p(a["lam"]), _p(a["Ks"]), _p(a["it"]),
                                       _p(a["dist"]))


def _ge(L, a):
    return L.aiy_ge_batch(_p(a["r"]), i64(a["C"]), _p(a["v"]), _p(a["a"]), _p(a["s"]), _p(a["P"]),
                          i64(a["N"]), i64(a["Na"]), d(ALPHA), d(DELTA), d(BETA), d(SIGMA),
                          d(LABOR), d(TOL), i64(a["max_iter"]), i64(a["z1"]), d(1.0), i64(a["T"]),
                          _p(a["U"]), ci(1), _p(a["Ks"]), _p(a["Kd"]), _p(a["it"]))


def _labor_ge(L, a):
    return L.aiy_labor_ge_batch(_p(a["r"]), i64(a["C"]), _p(a["v"]), _p(a["vnew"]), _p(a["pk"]),
                                _p(a["pl"]), _p(a["pc"]), _p(a["lin"]), _p(a["a"]), _p(a["s"]),
                                _p(a["P"]), _p(a["L"]), i64(a["N"]), i64(a["Na"]), i64(a["Nl"]),
                                d(ALPHA), d(DELTA), d(BETA), d(SIGMA), d(a["psi"]), d(a["eta"]),
                                d(LABOR), d(TOL), i64(a["max_iter"]), i64(a["z1"]), d(1.0),
                                i64(a["T"]), _p(a["U"]), ci(1), _p(a["Ks"]), _p(a["Kd"]),
                                _p(a["it"]))


def _egm_ge(L, a):
    return L.aiy_egm_ge_batch(_p(a["r"]), _p(a["w"]), i64(a["C"]), _p(a["pc"]), _p(a["a"]),
                              _p(a["s"]), _p(a["P"]), i64(a["N"]), i64(a["Na"]), d(ALPHA),
                              d(DELTA), d(BETA), d(SIGMA), d(AMIN), ci(a["labor_flag"]),
                              d(a["phi"]), d(a["theta"]), d(LABOR), d(TOL), i64(a["max_iter"]),
                              i64(a["z1"]), d(1.0), i64(a["T"]), _p(a["U"]), ci(1), _p(a["Ks"]),
                              _p(a["Kd"]), _p(a["it"]), _p(a["st"]))


def _ge_hist(L, a):
    return L.aiy_ge_hist_batch(_p(a["r"]), i64(a["C"]), _p(a["v"]), _p(a["a"]), _p(a["s"]),
                               _p(a["P"]), i64(a["N"]), i64(a["Na"]), d(ALPHA), d(DELTA), d(BETA),
                               d(SIGMA), d(LABOR), d(TOL), i64(a["max_iter"]), d(1e-10),
                               i64(a["dmax"]), _p(a["lam"]), ci(1), _p(a["Ks"]), _p(a["Kd"]),
                               _p(a["it"]), _p(a["dit"]))


def _egm_ge_hist(L, a):
    return L.aiy_egm_ge_hist_batch(_p(a["r"]), _p(a["w"]), i64(a["C"]), _p(a["pc"]), _p(a["a"]),
                                   _p(a["s"]), _p(a["P"]), i64(a["N"]), i64(a["Na"]), d(ALPHA),
                                   d(DELTA), d(BETA), d(SIGMA), d(AMIN), ci(a["labor_flag"]),
                                   d(a["phi"]), d(a["theta"]), d(LABOR), d(TOL),
                                   i64(a["max_iter"]), d(1e-10), i64(a["dmax"]), _p(a["lam"]),
                                   ci(1), _p(a["Ks"]), _p(a["Kd"]), _p(a["it"]), _p(a["dit"]),
                                   _p(a["st"]))


def _nulls(*keys):
    return [(f"null:{k}",) for k in keys]


# entry -> (caller, its sequence of checks as one defect each, further rows).  Rows: every defect
# of the sequence alone, every adjacent pair of it, and the extras.
ENTRIES = {
    "aiy_vfi_sweep": (_vfi_sweep, ["null:v", "N0", "null:a", "a_nan", "a_dec"],
                      _nulls("s", "P", "vnew", "pk", "pc", "lin") +
                      [("Na1",), ("a_rep",), ("valid",)]),
    "aiy_vfi_solve": (_vfi_solve, ["null:iters", "null:v", "Na1", "null:a", "a_nan", "a_dec"],
                      _nulls("s", "P", "vnew", "pk", "pc", "lin") +
                      [("N0",), ("maxiter0",), ("a_rep",), ("valid",)]),
    "aiy_labor_vfi_sweep": (_labor_sweep, ["null:L", "Nl0", "null:a", "a_nan", "a_dec"],
                            _nulls("v", "s", "P", "vnew", "pk", "pl", "pc", "lin") +
                            [("N0",), ("Na1",), ("psi_nan",), ("eta_inf",), ("Nl0", "psi_nan"),
                             ("a_rep",), ("valid",)]),
    "aiy_labor_vfi_solve": (_labor_solve, ["null:iters", "null:L", "Nl0", "a_nan", "a_dec"],
                            _nulls("v", "pl", "lin") +
                            [("psi_nan",), ("eta_inf",), ("maxiter0",), ("a_dec", "eta_inf"),
                             ("valid",)]),
    "aiy_egm_step": (_egm_step, ["null:pcn", "null:pc", "Na1", "null:a", "a_nan", "a_dec"],
                     _nulls("s", "P", "pk", "dist") + [("N0",), ("a_rep",), ("valid",)]),
    "aiy_egm_solve": (_egm_solve, ["null:pc", "N0", "a_nan", "a_dec"],
                      _nulls("s", "P", "pk", "dist", "iters") +
                      [("Na1",), ("maxiter0",), ("a_rep",), ("valid",)]),
    "aiy_labor_egm_step": (_labor_egm_step, ["null:pl", "null:pc", "Na1", "a_nan", "a_dec"],
                           _nulls("pcn", "dist") +
                           [("null:pcn", "null:pl"), ("phi_nan",), ("theta_inf",),
                            ("a_dec", "phi_nan"), ("valid",)]),
    "aiy_labor_egm_solve": (_labor_egm_solve, ["null:pl", "null:dist", "N0", "a_nan", "a_dec"],
                            _nulls("pc", "iters") +
                            [("phi_nan",), ("theta_inf",), ("maxiter0",), ("valid",)]),
    "aiy_sim_capital": (_sim, ["null:pk", "N0", "null:a", "a_nan", "a_dec", "a_rep"],
                        _nulls("P", "Ks", "U", "simk", "simz") +
                        [("Na1",), ("T0",), ("z1_0",), ("z1_big",), ("a_rep", "T0"), ("valid",)]),
    "aiy_dist_stationary": (_dist, ["null:idx", "Na1", "maxiter0", "null:a", "a_nan", "a_dec"],
                            _nulls("P", "lam", "Ks", "iters", "dist") +
                            [("N0",), ("a_rep",), ("lottery",), ("lottery", "a_rep"),
                             ("lottery", "a_dec"), ("lottery", "maxiter0", "a_rep"), ("valid",)]),
    "aiy_dist_stationary_batch": (_dist_batch,
                                  ["null:idx", "C0", "Na1", "maxiter0", "null:a", "a_nan", "a_dec"],
                                  _nulls("P", "lam", "Ks", "it", "dist") +
                                  [("N0",), ("a_rep",), ("lottery",), ("lottery", "a_rep"),
                                   ("lottery", "C0", "a_rep"), ("valid",)]),
    "aiy_ge_batch": (_ge, ["null:r", "C0", "T0", "z1_0", "maxiter0", "null:a", "a_nan", "a_dec",
                           "a_rep", "r_bad"],
                     _nulls("v", "s", "P", "Ks", "Kd", "it", "U") +
                     [("N0",), ("Na1",), ("z1_big",), ("r_nan",), ("Na1", "T0"),
                      ("T0", "null:U"), ("valid",)]),
    "aiy_labor_ge_batch": (_labor_ge, ["null:L", "Nl0", "T0", "z1_big", "maxiter0", "psi_nan",
                                       "a_nan", "a_dec", "a_rep", "r_bad"],
                           _nulls("r", "v", "s", "P", "Ks", "Kd", "it", "U", "vnew", "pk", "pl",
                                  "pc", "lin", "a") +
                           [("C0",), ("N0",), ("Na1",), ("z1_0",), ("eta_inf",), ("r_nan",),
                            ("C0", "T0"), ("eta_inf", "r_bad"), ("valid",)]),
    "aiy_egm_ge_batch": (_egm_ge, ["null:w", "C0", "N17", "T0", "z1_0", "maxiter0", "phi_nan",
                                   "a_nan", "a_dec", "a_rep", "r_bad"],
                         _nulls("r", "pc", "s", "P", "Ks", "Kd", "it", "st", "U", "a") +
                         [("N0",), ("Na1",), ("z1_big",), ("theta_inf",), ("r_nan",),
                          ("Na1", "N17"), ("noflag", "phi_nan"), ("noflag", "phi_nan", "r_bad"),
                          ("valid",)]),
    "aiy_ge_hist_batch": (_ge_hist, ["null:dit", "Na1", "maxiter0", "dmax0", "null:a", "a_nan",
                                     "a_dec", "a_rep", "r_bad"],
                          _nulls("r", "v", "s", "P", "Ks", "Kd", "it", "lam") +
                          [("C0",), ("N0",), ("r_nan",), ("C0", "dmax0"), ("dmax0", "r_nan"),
                           ("valid",)]),
    "aiy_egm_ge_hist_batch": (_egm_ge_hist, ["null:st", "C0", "N17", "maxiter0", "dmax0",
                                             "theta_inf", "a_nan", "a_dec", "a_rep", "r_nan"],
                              _nulls("r", "w", "pc", "s", "P", "Ks", "Kd", "it", "dit", "lam",
                                     "a") +
                              [("N0",), ("Na1",), ("phi_nan",), ("r_bad",), ("Na1", "N17"),
                               ("N17", "dmax0"), ("noflag", "theta_inf"),
                               ("noflag", "theta_inf", "r_bad"), ("valid",)]),
}


def _rows():
    out = []
    for entry, (_, seq, extra) in ENTRIES.items():
        rows = [(x,) for x in seq] + list(zip(seq, seq[1:])) + list(extra)
        out += [f"{entry}:{'+'.join(r)}" for r in rows]
    return out


ROWS = _rows()


def _answer(L, row):
    entry, defects = row.split(":", 1)
    a = _base()
    for x in defects.split("+"):
        _apply(a, x)
    rc = ENTRIES[entry][0](L, a)
    return rc, L.aiy_last_error().decode()


EXPECTED = {
    'aiy_vfi_sweep:null:v': (6, 'NULL argument'),
    'aiy_vfi_sweep:N0': (1, 'need N >= 1 and Na >= 2'),
    'aiy_vfi_sweep:null:a': (6, 'a_grid is NULL'),
    'aiy_vfi_sweep:a_nan': (2, 'a_grid(1) is not finite'),
    'aiy_vfi_sweep:a_dec': (6, 'a_grid must be non-decreasing (a_grid(3) < a_grid(2))'),
    'aiy_vfi_sweep:null:v+N0': (6, 'NULL argument'),
    'aiy_vfi_sweep:N0+null:a': (1, 'need N >= 1 and Na >= 2'),
    'aiy_vfi_sweep:null:a+a_nan': (6, 'a_grid is NULL'),
    'aiy_vfi_sweep:a_nan+a_dec': (2, 'a_grid(1) is not finite'),
    'aiy_vfi_sweep:null:s': (6, 'NULL argument'),
    'aiy_vfi_sweep:null:P': (6, 'NULL argument'),
    'aiy_vfi_sweep:null:vnew': (6, 'NULL argument'),
    'aiy_vfi_sweep:null:pk': (6, 'NULL argument'),
    'aiy_vfi_sweep:null:pc': (6, 'NULL argument'),
    'aiy_vfi_sweep:null:lin': (5, 'no HIP device visible'),
    'aiy_vfi_sweep:Na1': (1, 'need N >= 1 and Na >= 2'),
    'aiy_vfi_sweep:a_rep': (5, 'no HIP device visible'),
    'aiy_vfi_sweep:valid': (5, 'no HIP device visible'),
    'aiy_vfi_solve:null:iters': (6, 'NULL iters'),
    'aiy_vfi_solve:null:v': (6, 'NULL argument'),
    'aiy_vfi_solve:Na1': (1, 'need N >= 1 and Na >= 2'),
    'aiy_vfi_solve:null:a': (6, 'a_grid is NULL'),
    'aiy_vfi_solve:a_nan': (2, 'a_grid(1) is not finite'),
    'aiy_vfi_solve:a_dec': (6, 'a_grid must be non-decreasing (a_grid(3) < a_grid(2))'),
    'aiy_vfi_solve:null:iters+null:v': (6, 'NULL iters'),
    'aiy_vfi_solve:null:v+Na1': (6, 'NULL argument'),
    'aiy_vfi_solve:Na1+null:a': (1, 'need N >= 1 and Na >= 2'),
    'aiy_vfi_solve:null:a+a_nan': (6, 'a_grid is NULL'),
    'aiy_vfi_solve:a_nan+a_dec': (2, 'a_grid(1) is not finite'),
    'aiy_vfi_solve:null:s': (6, 'NULL argument'),
    'aiy_vfi_solve:null:P': (6, 'NULL argument'),
    'aiy_vfi_solve:null:vnew': (6, 'NULL argument'),
    'aiy_vfi_solve:null:pk': (6, 'NULL argument'),
    'aiy_vfi_solve:null:pc': (6, 'NULL argument'),
    'aiy_vfi_solve:null:lin': (5, 'no HIP device visible'),
    'aiy_vfi_solve:N0': (1, 'need N >= 1 and Na >= 2'),
    'aiy_vfi_solve:maxiter0': (5, 'no HIP device visible'),
    'aiy_vfi_solve:a_rep': (5, 'no HIP device visible'),
    'aiy_vfi_solve:valid': (5, 'no HIP device visible'),
    'aiy_labor_vfi_sweep:null:L': (6, 'NULL argument'),
    'aiy_labor_vfi_sweep:Nl0': (1, 'need N >= 1, Na >= 2, Nl >= 1'),
    'aiy_labor_vfi_sweep:null:a': (6, 'a_grid is NULL'),
    'aiy_labor_vfi_sweep:a_nan': (2, 'a_grid(1) is not finite'),
    'aiy_labor_vfi_sweep:a_dec': (6, 'a_grid must be non-decreasing (a_grid(3) < a_grid(2))'),
    'aiy_labor_vfi_sweep:null:L+Nl0': (6, 'NULL argument'),
    'aiy_labor_vfi_sweep:Nl0+null:a': (1, 'need N >= 1, Na >= 2, Nl >= 1'),
    'aiy_labor_vfi_sweep:null:a+a_nan': (6, 'a_grid is NULL'),
    'aiy_labor_vfi_sweep:a_nan+a_dec': (2, 'a_grid(1) is not finite'),
    'aiy_labor_vfi_sweep:null:v': (6, 'NULL argument'),
    'aiy_labor_vfi_sweep:null:s': (6, 'NULL argument'),
    'aiy_labor_vfi_sweep:null:P': (6, 'NULL argument'),
    'aiy_labor_vfi_sweep:null:vnew': (6, 'NULL argument'),
    'aiy_labor_vfi_sweep:null:pk': (6, 'NULL argument'),
    'aiy_labor_vfi_sweep:null:pl': (6, 'NULL argument'),
    'aiy_labor_vfi_sweep:null:pc': (6, 'NULL argument'),
    'aiy_labor_vfi_sweep:null:lin': (5, 'no HIP device visible'),
    'aiy_labor_vfi_sweep:N0': (1, 'need N >= 1, Na >= 2, Nl >= 1'),
    'aiy_labor_vfi_sweep:Na1': (1, 'need N >= 1, Na >= 2, Nl >= 1'),
    'aiy_labor_vfi_sweep:psi_nan': (5, 'no HIP device visible'),
    'aiy_labor_vfi_sweep:eta_inf': (5, 'no HIP device visible'),
    'aiy_labor_vfi_sweep:Nl0+psi_nan': (1, 'need N >= 1, Na >= 2, Nl >= 1'),
    'aiy_labor_vfi_sweep:a_rep': (5, 'no HIP device visible'),
    'aiy_labor_vfi_sweep:valid': (5, 'no HIP device visible'),
    'aiy_labor_vfi_solve:null:iters': (6, 'NULL iters'),
    'aiy_labor_vfi_solve:null:L': (6, 'NULL argument'),
    'aiy_labor_vfi_solve:Nl0': (1, 'need N >= 1, Na >= 2, Nl >= 1'),
    'aiy_labor_vfi_solve:a_nan': (2, 'a_grid(1) is not finite'),
    'aiy_labor_vfi_solve:a_dec': (6, 'a_grid must be non-decreasing (a_grid(3) < a_grid(2))'),
    'aiy_labor_vfi_solve:null:iters+null:L': (6, 'NULL iters'),
    'aiy_labor_vfi_solve:null:L+Nl0': (6, 'NULL argument'),
    'aiy_labor_vfi_solve:Nl0+a_nan': (1, 'need N >= 1, Na >= 2, Nl >= 1'),
    'aiy_labor_vfi_solve:a_nan+a_dec': (2, 'a_grid(1) is not finite'),
    'aiy_labor_vfi_solve:null:v': (6, 'NULL argument'),
    'aiy_labor_vfi_solve:null:pl': (6, 'NULL argument'),
    'aiy_labor_vfi_solve:null:lin': (5, 'no HIP device visible'),
    'aiy_labor_vfi_solve:psi_nan': (5, 'no HIP device visible'),
    'aiy_labor_vfi_solve:eta_inf': (5, 'no HIP device visible'),
    'aiy_labor_vfi_solve:maxiter0': (5, 'no HIP device visible'),
    'aiy_labor_vfi_solve:a_dec+eta_inf': (6, 'a_grid must be non-decreasing (a_grid(3) < a_grid(2))'),
    'aiy_labor_vfi_solve:valid': (5, 'no HIP device visible'),
    'aiy_egm_step:null:pcn': (6, 'NULL policy_c_next'),
    'aiy_egm_step:null:pc': (6, 'NULL argument'),
    'aiy_egm_step:Na1': (1, 'need N >= 1 and Na >= 2'),
    'aiy_egm_step:null:a': (6, 'a_grid is NULL'),
    'aiy_egm_step:a_nan': (2, 'a_grid(1) is not finite'),
    'aiy_egm_step:a_dec': (6, 'a_grid must be non-decreasing (a_grid(3) < a_grid(2))'),
    'aiy_egm_step:null:pcn+null:pc': (6, 'NULL policy_c_next'),
    'aiy_egm_step:null:pc+Na1': (6, 'NULL argument'),
    'aiy_egm_step:Na1+null:a': (1, 'need N >= 1 and Na >= 2'),
    'aiy_egm_step:null:a+a_nan': (6, 'a_grid is NULL'),
    'aiy_egm_step:a_nan+a_dec': (2, 'a_grid(1) is not finite'),
    'aiy_egm_step:null:s': (6, 'NULL argument'),
    'aiy_egm_step:null:P': (6, 'NULL argument'),
    'aiy_egm_step:null:pk': (6, 'NULL argument'),
    'aiy_egm_step:null:dist': (6, 'NULL argument'),
    'aiy_egm_step:N0': (1, 'need N >= 1 and Na >= 2'),
    'aiy_egm_step:a_rep': (5, 'no HIP device visible'),
    'aiy_egm_step:valid': (5, 'no HIP device visible'),
    'aiy_egm_solve:null:pc': (6, 'NULL argument'),
    'aiy_egm_solve:N0': (1, 'need N >= 1 and Na >= 2'),
    'aiy_egm_solve:a_nan': (2, 'a_grid(1) is not finite'),
    'aiy_egm_solve:a_dec': (6, 'a_grid must be non-decreasing (a_grid(3) < a_grid(2))'),
    'aiy_egm_solve:null:pc+N0': (6, 'NULL argument'),
    'aiy_egm_solve:N0+a_nan': (1, 'need N >= 1 and Na >= 2'),
    'aiy_egm_solve:a_nan+a_dec': (2, 'a_grid(1) is not finite'),
    'aiy_egm_solve:null:s': (6, 'NULL argument'),
    'aiy_egm_solve:null:P': (6, 'NULL argument'),
    'aiy_egm_solve:null:pk': (6, 'NULL argument'),
    'aiy_egm_solve:null:dist': (6, 'NULL argument'),
    'aiy_egm_solve:null:iters': (5, 'no HIP device visible'),
    'aiy_egm_solve:Na1': (1, 'need N >= 1 and Na >= 2'),
    'aiy_egm_solve:maxiter0': (5, 'no HIP device visible'),
    'aiy_egm_solve:a_rep': (5, 'no HIP device visible'),
    'aiy_egm_solve:valid': (5, 'no HIP device visible'),
    'aiy_labor_egm_step:null:pl': (6, 'NULL output'),
    'aiy_labor_egm_step:null:pc': (6, 'NULL argument'),
    'aiy_labor_egm_step:Na1': (1, 'need N >= 1 and Na >= 2'),
    'aiy_labor_egm_step:a_nan': (2, 'a_grid(1) is not finite'),
    'aiy_labor_egm_step:a_dec': (6, 'a_grid must be non-decreasing (a_grid(3) < a_grid(2))'),
    'aiy_labor_egm_step:null:pl+null:pc': (6, 'NULL output'),
    'aiy_labor_egm_step:null:pc+Na1': (6, 'NULL argument'),
    'aiy_labor_egm_step:Na1+a_nan': (1, 'need N >= 1 and Na >= 2'),
    'aiy_labor_egm_step:a_nan+a_dec': (2, 'a_grid(1) is not finite'),
    'aiy_labor_egm_step:null:pcn': (6, 'NULL output'),
    'aiy_labor_egm_step:null:dist': (6, 'NULL argument'),
    'aiy_labor_egm_step:null:pcn+null:pl': (6, 'NULL output'),
    'aiy_labor_egm_step:phi_nan': (5, 'no HIP device visible'),
    'aiy_labor_egm_step:theta_inf': (5, 'no HIP device visible'),
    'aiy_labor_egm_step:a_dec+phi_nan': (6, 'a_grid must be non-decreasing (a_grid(3) < a_grid(2))'),
    'aiy_labor_egm_step:valid': (5, 'no HIP device visible'),
    'aiy_labor_egm_solve:null:pl': (6, 'NULL policy_l'),
    'aiy_labor_egm_solve:null:dist': (6, 'NULL argument'),
    'aiy_labor_egm_solve:N0': (1, 'need N >= 1 and Na >= 2'),
    'aiy_labor_egm_solve:a_nan': (2, 'a_grid(1) is not finite'),
    'aiy_labor_egm_solve:a_dec': (6, 'a_grid must be non-decreasing (a_grid(3) < a_grid(2))'),
    'aiy_labor_egm_solve:null:pl+null:dist': (6, 'NULL policy_l'),
    'aiy_labor_egm_solve:null:dist+N0': (6, 'NULL argument'),
    'aiy_labor_egm_solve:N0+a_nan': (1, 'need N >= 1 and Na >= 2'),
    'aiy_labor_egm_solve:a_nan+a_dec': (2, 'a_grid(1) is not finite'),
    'aiy_labor_egm_solve:null:pc': (6, 'NULL argument'),
    'aiy_labor_egm_solve:null:iters': (5, 'no HIP device visible'),
    'aiy_labor_egm_solve:phi_nan': (5, 'no HIP device visible'),
    'aiy_labor_egm_solve:theta_inf': (5, 'no HIP device visible'),
    'aiy_labor_egm_solve:maxiter0': (5, 'no HIP device visible'),
    'aiy_labor_egm_solve:valid': (5, 'no HIP device visible'),
    'aiy_sim_capital:null:pk': (6, 'NULL argument'),
    'aiy_sim_capital:N0': (1, 'need N >= 1 and Na >= 2'),
    'aiy_sim_capital:null:a': (6, 'a_grid is NULL'),
    'aiy_sim_capital:a_nan': (2, 'a_grid(1) is not finite'),
    'aiy_sim_capital:a_dec': (6, 'a_grid must be non-decreasing (a_grid(3) < a_grid(2))'),
    'aiy_sim_capital:a_rep': (6, 'grid must be strictly increasing (point 5 repeats point 4)'),
    'aiy_sim_capital:null:pk+N0': (6, 'NULL argument'),
    'aiy_sim_capital:N0+null:a': (1, 'need N >= 1 and Na >= 2'),
    'aiy_sim_capital:null:a+a_nan': (6, 'a_grid is NULL'),
    'aiy_sim_capital:a_nan+a_dec': (2, 'a_grid(1) is not finite'),
    'aiy_sim_capital:a_dec+a_rep': (6, 'a_grid must be non-decreasing (a_grid(3) < a_grid(2))'),
    'aiy_sim_capital:null:P': (6, 'NULL argument'),
    'aiy_sim_capital:null:Ks': (6, 'NULL argument'),
    'aiy_sim_capital:null:U': (5, 'no HIP device visible'),
    'aiy_sim_capital:null:simk': (5, 'no HIP device visible'),
    'aiy_sim_capital:null:simz': (5, 'no HIP device visible'),
    'aiy_sim_capital:Na1': (1, 'need N >= 1 and Na >= 2'),
    'aiy_sim_capital:T0': (5, 'no HIP device visible'),
    'aiy_sim_capital:z1_0': (5, 'no HIP device visible'),
    'aiy_sim_capital:z1_big': (5, 'no HIP device visible'),
    'aiy_sim_capital:a_rep+T0': (6, 'grid must be strictly increasing (point 5 repeats point 4)'),
    'aiy_sim_capital:valid': (5, 'no HIP device visible'),
    'aiy_dist_stationary:null:idx': (6, 'NULL argument'),
    'aiy_dist_stationary:Na1': (1, 'need N >= 1 and Na >= 2'),
    'aiy_dist_stationary:maxiter0': (6, 'max_iter must be >= 1'),
    'aiy_dist_stationary:null:a': (6, 'a_grid is NULL'),
    'aiy_dist_stationary:a_nan': (2, 'a_grid(1) is not finite'),
    'aiy_dist_stationary:a_dec': (6, 'a_grid must be non-decreasing (a_grid(3) < a_grid(2))'),
    'aiy_dist_stationary:null:idx+Na1': (6, 'NULL argument'),
    'aiy_dist_stationary:Na1+maxiter0': (1, 'need N >= 1 and Na >= 2'),
    'aiy_dist_stationary:maxiter0+null:a': (6, 'max_iter must be >= 1'),
    'aiy_dist_stationary:null:a+a_nan': (6, 'a_grid is NULL'),
    'aiy_dist_stationary:a_nan+a_dec': (2, 'a_grid(1) is not finite'),
    'aiy_dist_stationary:null:P': (6, 'NULL argument'),
    'aiy_dist_stationary:null:lam': (6, 'NULL argument'),
    'aiy_dist_stationary:null:Ks': (6, 'NULL argument'),
    'aiy_dist_stationary:null:iters': (6, 'NULL argument'),
    'aiy_dist_stationary:null:dist': (6, 'NULL argument'),
    'aiy_dist_stationary:N0': (1, 'need N >= 1 and Na >= 2'),
    'aiy_dist_stationary:a_rep': (5, 'no HIP device visible'),
    'aiy_dist_stationary:lottery': (5, 'no HIP device visible'),
    'aiy_dist_stationary:lottery+a_rep': (6, 'grid must be strictly increasing (point 5 repeats point 4)'),
    'aiy_dist_stationary:lottery+a_dec': (6, 'a_grid must be non-decreasing (a_grid(3) < a_grid(2))'),
    'aiy_dist_stationary:lottery+maxiter0+a_rep': (6, 'max_iter must be >= 1'),
    'aiy_dist_stationary:valid': (5, 'no HIP device visible'),
    'aiy_dist_stationary_batch:null:idx': (6, 'NULL argument'),
    'aiy_dist_stationary_batch:C0': (1, 'need 1 <= C < 2^31'),
    'aiy_dist_stationary_batch:Na1': (1, 'need N >= 1 and Na >= 2'),
    'aiy_dist_stationary_batch:maxiter0': (6, 'max_iter must be >= 1'),
    'aiy_dist_stationary_batch:null:a': (6, 'a_grid is NULL'),
    'aiy_dist_stationary_batch:a_nan': (2, 'a_grid(1) is not finite'),
    'aiy_dist_stationary_batch:a_dec': (6, 'a_grid must be non-decreasing (a_grid(3) < a_grid(2))'),
    'aiy_dist_stationary_batch:null:idx+C0': (6, 'NULL argument'),
    'aiy_dist_stationary_batch:C0+Na1': (1, 'need 1 <= C < 2^31'),
    'aiy_dist_stationary_batch:Na1+maxiter0': (1, 'need N >= 1 and Na >= 2'),
    'aiy_dist_stationary_batch:maxiter0+null:a': (6, 'max_iter must be >= 1'),
    'aiy_dist_stationary_batch:null:a+a_nan': (6, 'a_grid is NULL'),
    'aiy_dist_stationary_batch:a_nan+a_dec': (2, 'a_grid(1) is not finite'),
    'aiy_dist_stationary_batch:null:P': (6, 'NULL argument'),
    'aiy_dist_stationary_batch:null:lam': (6, 'NULL argument'),
    'aiy_dist_stationary_batch:null:Ks': (6, 'NULL argument'),
    'aiy_dist_stationary_batch:null:it': (6, 'NULL argument'),
    'aiy_dist_stationary_batch:null:dist': (6, 'NULL argument'),
    'aiy_dist_stationary_batch:N0': (1, 'need N >= 1 and Na >= 2'),
    'aiy_dist_stationary_batch:a_rep': (5, 'no HIP device visible'),
    'aiy_dist_stationary_batch:lottery': (5, 'no HIP device visible'),
    'aiy_dist_stationary_batch:lottery+a_rep': (6, 'grid must be strictly increasing (point 5 repeats point 4)'),
    'aiy_dist_stationary_batch:lottery+C0+a_rep': (1, 'need 1 <= C < 2^31'),
    'aiy_dist_stationary_batch:valid': (5, 'no HIP device visible'),
    'aiy_ge_batch:null:r': (6, 'NULL argument'),
    'aiy_ge_batch:C0': (1, 'need C >= 1, N >= 1, Na >= 2'),
    'aiy_ge_batch:T0': (1, 'T must be in [1, 2^31)'),
    'aiy_ge_batch:z1_0': (6, 'z1 (1-based) out of range'),
    'aiy_ge_batch:maxiter0': (6, 'max_iter must be >= 1'),
    'aiy_ge_batch:null:a': (6, 'a_grid is NULL'),
    'aiy_ge_batch:a_nan': (2, 'a_grid(1) is not finite'),
    'aiy_ge_batch:a_dec': (6, 'a_grid must be non-decreasing (a_grid(3) < a_grid(2))'),
    'aiy_ge_batch:a_rep': (6, 'grid must be strictly increasing (point 5 repeats point 4)'),
    'aiy_ge_batch:r_bad': (6, 'candidate 3: r must be finite with r + delta > 0'),
    'aiy_ge_batch:null:r+C0': (6, 'NULL argument'),
    'aiy_ge_batch:C0+T0': (1, 'need C >= 1, N >= 1, Na >= 2'),
    'aiy_ge_batch:T0+z1_0': (1, 'T must be in [1, 2^31)'),
    'aiy_ge_batch:z1_0+maxiter0': (6, 'z1 (1-based) out of range'),
    'aiy_ge_batch:maxiter0+null:a': (6, 'max_iter must be >= 1'),
    'aiy_ge_batch:null:a+a_nan': (6, 'a_grid is NULL'),
    'aiy_ge_batch:a_nan+a_dec': (2, 'a_grid(1) is not finite'),
    'aiy_ge_batch:a_dec+a_rep': (6, 'a_grid must be non-decreasing (a_grid(3) < a_grid(2))'),
    'aiy_ge_batch:a_rep+r_bad': (6, 'grid must be strictly increasing (point 5 repeats point 4)'),
    'aiy_ge_batch:null:v': (6, 'NULL argument'),
    'aiy_ge_batch:null:s': (6, 'NULL argument'),
    'aiy_ge_batch:null:P': (6, 'NULL argument'),
    'aiy_ge_batch:null:Ks': (6, 'NULL argument'),
    'aiy_ge_batch:null:Kd': (6, 'NULL argument'),
    'aiy_ge_batch:null:it': (6, 'NULL argument'),
    'aiy_ge_batch:null:U': (6, 'NULL argument'),
    'aiy_ge_batch:N0': (1, 'need C >= 1, N >= 1, Na >= 2'),
    'aiy_ge_batch:Na1': (1, 'need C >= 1, N >= 1, Na >= 2'),
    'aiy_ge_batch:z1_big': (6, 'z1 (1-based) out of range'),
    'aiy_ge_batch:r_nan': (6, 'candidate 3: r must be finite with r + delta > 0'),
    'aiy_ge_batch:Na1+T0': (1, 'need C >= 1, N >= 1, Na >= 2'),
    'aiy_ge_batch:T0+null:U': (1, 'T must be in [1, 2^31)'),
    'aiy_ge_batch:valid': (5, 'no HIP device visible'),
    'aiy_labor_ge_batch:null:L': (6, 'NULL argument'),
    'aiy_labor_ge_batch:Nl0': (1, 'need C >= 1, N >= 1, Na >= 2, Nl >= 1'),
    'aiy_labor_ge_batch:T0': (1, 'T must be in [1, 2^31)'),
    'aiy_labor_ge_batch:z1_big': (6, 'z1 (1-based) out of range'),
    'aiy_labor_ge_batch:maxiter0': (6, 'max_iter must be >= 1'),
    'aiy_labor_ge_batch:psi_nan': (2, 'psi and eta must be finite'),
    'aiy_labor_ge_batch:a_nan': (2, 'a_grid(1) is not finite'),
    'aiy_labor_ge_batch:a_dec': (6, 'a_grid must be non-decreasing (a_grid(3) < a_grid(2))'),
    'aiy_labor_ge_batch:a_rep': (6, 'grid must be strictly increasing (point 5 repeats point 4)'),
    'aiy_labor_ge_batch:r_bad': (6, 'candidate 3: r must be finite with r + delta > 0'),
    'aiy_labor_ge_batch:null:L+Nl0': (6, 'NULL argument'),
    'aiy_labor_ge_batch:Nl0+T0': (1, 'need C >= 1, N >= 1, Na >= 2, Nl >= 1'),
    'aiy_labor_ge_batch:T0+z1_big': (1, 'T must be in [1, 2^31)'),
    'aiy_labor_ge_batch:z1_big+maxiter0': (6, 'z1 (1-based) out of range'),
    'aiy_labor_ge_batch:maxiter0+psi_nan': (6, 'max_iter must be >= 1'),
    'aiy_labor_ge_batch:psi_nan+a_nan': (2, 'psi and eta must be finite'),
    'aiy_labor_ge_batch:a_nan+a_dec': (2, 'a_grid(1) is not finite'),
    'aiy_labor_ge_batch:a_dec+a_rep': (6, 'a_grid must be non-decreasing (a_grid(3) < a_grid(2))'),
    'aiy_labor_ge_batch:a_rep+r_bad': (6, 'grid must be strictly increasing (point 5 repeats point 4)'),
    'aiy_labor_ge_batch:null:r': (6, 'NULL argument'),
    'aiy_labor_ge_batch:null:v': (6, 'NULL argument'),
    'aiy_labor_ge_batch:null:s': (6, 'NULL argument'),
    'aiy_labor_ge_batch:null:P': (6, 'NULL argument'),
    'aiy_labor_ge_batch:null:Ks': (6, 'NULL argument'),
    'aiy_labor_ge_batch:null:Kd': (6, 'NULL argument'),
    'aiy_labor_ge_batch:null:it': (6, 'NULL argument'),
    'aiy_labor_ge_batch:null:U': (6, 'NULL argument'),
    'aiy_labor_ge_batch:null:vnew': (5, 'no HIP device visible'),
    'aiy_labor_ge_batch:null:pk': (5, 'no HIP device visible'),
    'aiy_labor_ge_batch:null:pl': (5, 'no HIP device visible'),
    'aiy_labor_ge_batch:null:pc': (5, 'no HIP device visible'),
    'aiy_labor_ge_batch:null:lin': (5, 'no HIP device visible'),
    'aiy_labor_ge_batch:null:a': (6, 'a_grid is NULL'),
    'aiy_labor_ge_batch:C0': (1, 'need C >= 1, N >= 1, Na >= 2, Nl >= 1'),
    'aiy_labor_ge_batch:N0': (1, 'need C >= 1, N >= 1, Na >= 2, Nl >= 1'),
    'aiy_labor_ge_batch:Na1': (1, 'need C >= 1, N >= 1, Na >= 2, Nl >= 1'),
    'aiy_labor_ge_batch:z1_0': (6, 'z1 (1-based) out of range'),
    'aiy_labor_ge_batch:eta_inf': (2, 'psi and eta must be finite'),
    'aiy_labor_ge_batch:r_nan': (6, 'candidate 3: r must be finite with r + delta > 0'),
    'aiy_labor_ge_batch:C0+T0': (1, 'need C >= 1, N >= 1, Na >= 2, Nl >= 1'),
    'aiy_labor_ge_batch:eta_inf+r_bad': (2, 'psi and eta must be finite'),
    'aiy_labor_ge_batch:valid': (5, 'no HIP device visible'),
    'aiy_egm_ge_batch:null:w': (6, 'NULL argument'),
    'aiy_egm_ge_batch:C0': (1, 'need C >= 1, N >= 1, Na >= 2'),
    'aiy_egm_ge_batch:N17': (1, 'EGM kernels support N <= 16 productivity states'),
    'aiy_egm_ge_batch:T0': (1, 'T must be in [1, 2^31)'),
    'aiy_egm_ge_batch:z1_0': (6, 'z1 (1-based) out of range'),
    'aiy_egm_ge_batch:maxiter0': (6, 'max_iter must be >= 1'),
    'aiy_egm_ge_batch:phi_nan': (2, 'phi and theta must be finite'),
    'aiy_egm_ge_batch:a_nan': (2, 'a_grid(1) is not finite'),
    'aiy_egm_ge_batch:a_dec': (6, 'a_grid must be non-decreasing (a_grid(3) < a_grid(2))'),
    'aiy_egm_ge_batch:a_rep': (6, 'grid must be strictly increasing (point 5 repeats point 4)'),
    'aiy_egm_ge_batch:r_bad': (6, 'candidate 3: r must be finite with r + delta > 0'),
    'aiy_egm_ge_batch:null:w+C0': (6, 'NULL argument'),
    'aiy_egm_ge_batch:C0+N17': (1, 'need C >= 1, N >= 1, Na >= 2'),
    'aiy_egm_ge_batch:N17+T0': (1, 'EGM kernels support N <= 16 productivity states'),
    'aiy_egm_ge_batch:T0+z1_0': (1, 'T must be in [1, 2^31)'),
    'aiy_egm_ge_batch:z1_0+maxiter0': (6, 'z1 (1-based) out of range'),
    'aiy_egm_ge_batch:maxiter0+phi_nan': (6, 'max_iter must be >= 1'),
    'aiy_egm_ge_batch:phi_nan+a_nan': (2, 'phi and theta must be finite'),
    'aiy_egm_ge_batch:a_nan+a_dec': (2, 'a_grid(1) is not finite'),
    'aiy_egm_ge_batch:a_dec+a_rep': (6, 'a_grid must be non-decreasing (a_grid(3) < a_grid(2))'),
    'aiy_egm_ge_batch:a_rep+r_bad': (6, 'grid must be strictly increasing (point 5 repeats point 4)'),
    'aiy_egm_ge_batch:null:r': (6, 'NULL argument'),
    'aiy_egm_ge_batch:null:pc': (6, 'NULL argument'),
    'aiy_egm_ge_batch:null:s': (6, 'NULL argument'),
    'aiy_egm_ge_batch:null:P': (6, 'NULL argument'),
    'aiy_egm_ge_batch:null:Ks': (6, 'NULL argument'),
    'aiy_egm_ge_batch:null:Kd': (6, 'NULL argument'),
    'aiy_egm_ge_batch:null:it': (6, 'NULL argument'),
    'aiy_egm_ge_batch:null:st': (6, 'NULL argument'),
    'aiy_egm_ge_batch:null:U': (6, 'NULL argument'),
    'aiy_egm_ge_batch:null:a': (6, 'a_grid is NULL'),
    'aiy_egm_ge_batch:N0': (1, 'need C >= 1, N >= 1, Na >= 2'),
    'aiy_egm_ge_batch:Na1': (1, 'need C >= 1, N >= 1, Na >= 2'),
    'aiy_egm_ge_batch:z1_big': (6, 'z1 (1-based) out of range'),
    'aiy_egm_ge_batch:theta_inf': (2, 'phi and theta must be finite'),
    'aiy_egm_ge_batch:r_nan': (6, 'candidate 3: r must be finite with r + delta > 0'),
    'aiy_egm_ge_batch:Na1+N17': (1, 'need C >= 1, N >= 1, Na >= 2'),
    'aiy_egm_ge_batch:noflag+phi_nan': (5, 'no HIP device visible'),
    'aiy_egm_ge_batch:noflag+phi_nan+r_bad': (6, 'candidate 3: r must be finite with r + delta > 0'),
    'aiy_egm_ge_batch:valid': (5, 'no HIP device visible'),
    'aiy_ge_hist_batch:null:dit': (6, 'NULL argument'),
    'aiy_ge_hist_batch:Na1': (1, 'need C >= 1, N >= 1, Na >= 2'),
    'aiy_ge_hist_batch:maxiter0': (6, 'max_iter must be >= 1'),
    'aiy_ge_hist_batch:dmax0': (6, 'dist_max_iter must be >= 1'),
    'aiy_ge_hist_batch:null:a': (6, 'a_grid is NULL'),
    'aiy_ge_hist_batch:a_nan': (2, 'a_grid(1) is not finite'),
    'aiy_ge_hist_batch:a_dec': (6, 'a_grid must be non-decreasing (a_grid(3) < a_grid(2))'),
    'aiy_ge_hist_batch:a_rep': (6, 'grid must be strictly increasing (point 5 repeats point 4)'),
    'aiy_ge_hist_batch:r_bad': (6, 'candidate 3: r must be finite with r + delta > 0'),
    'aiy_ge_hist_batch:null:dit+Na1': (6, 'NULL argument'),
    'aiy_ge_hist_batch:Na1+maxiter0': (1, 'need C >= 1, N >= 1, Na >= 2'),
    'aiy_ge_hist_batch:maxiter0+dmax0': (6, 'max_iter must be >= 1'),
    'aiy_ge_hist_batch:dmax0+null:a': (6, 'dist_max_iter must be >= 1'),
    'aiy_ge_hist_batch:null:a+a_nan': (6, 'a_grid is NULL'),
    'aiy_ge_hist_batch:a_nan+a_dec': (2, 'a_grid(1) is not finite'),
    'aiy_ge_hist_batch:a_dec+a_rep': (6, 'a_grid must be non-decreasing (a_grid(3) < a_grid(2))'),
    'aiy_ge_hist_batch:a_rep+r_bad': (6, 'grid must be strictly increasing (point 5 repeats point 4)'),
    'aiy_ge_hist_batch:null:r': (6, 'NULL argument'),
    'aiy_ge_hist_batch:null:v': (6, 'NULL argument'),
    'aiy_ge_hist_batch:null:s': (6, 'NULL argument'),
    'aiy_ge_hist_batch:null:P': (6, 'NULL argument'),
    'aiy_ge_hist_batch:null:Ks': (6, 'NULL argument'),
    'aiy_ge_hist_batch:null:Kd': (6, 'NULL argument'),
    'aiy_ge_hist_batch:null:it': (6, 'NULL argument'),
    'aiy_ge_hist_batch:null:lam': (5, 'no HIP device visible'),
    'aiy_ge_hist_batch:C0': (1, 'need C >= 1, N >= 1, Na >= 2'),
    'aiy_ge_hist_batch:N0': (1, 'need C >= 1, N >= 1, Na >= 2'),
    'aiy_ge_hist_batch:r_nan': (6, 'candidate 3: r must be finite with r + delta > 0'),
    'aiy_ge_hist_batch:C0+dmax0': (1, 'need C >= 1, N >= 1, Na >= 2'),
    'aiy_ge_hist_batch:dmax0+r_nan': (6, 'dist_max_iter must be >= 1'),
    'aiy_ge_hist_batch:valid': (5, 'no HIP device visible'),
    'aiy_egm_ge_hist_batch:null:st': (6, 'NULL argument'),
    'aiy_egm_ge_hist_batch:C0': (1, 'need C >= 1, N >= 1, Na >= 2'),
    'aiy_egm_ge_hist_batch:N17': (1, 'EGM kernels support N <= 16 productivity states'),
    'aiy_egm_ge_hist_batch:maxiter0': (6, 'max_iter must be >= 1'),
    'aiy_egm_ge_hist_batch:dmax0': (6, 'dist_max_iter must be >= 1'),
    'aiy_egm_ge_hist_batch:theta_inf': (2, 'phi and theta must be finite'),
    'aiy_egm_ge_hist_batch:a_nan': (2, 'a_grid(1) is not finite'),
    'aiy_egm_ge_hist_batch:a_dec': (6, 'a_grid must be non-decreasing (a_grid(3) < a_grid(2))'),
    'aiy_egm_ge_hist_batch:a_rep': (6, 'grid must be strictly increasing (point 5 repeats point 4)'),
    'aiy_egm_ge_hist_batch:r_nan': (6, 'candidate 3: r must be finite with r + delta > 0'),
    'aiy_egm_ge_hist_batch:null:st+C0': (6, 'NULL argument'),
    'aiy_egm_ge_hist_batch:C0+N17': (1, 'need C >= 1, N >= 1, Na >= 2'),
    'aiy_egm_ge_hist_batch:N17+maxiter0': (1, 'EGM kernels support N <= 16 productivity states'),
    'aiy_egm_ge_hist_batch:maxiter0+dmax0': (6, 'max_iter must be >= 1'),
    'aiy_egm_ge_hist_batch:dmax0+theta_inf': (6, 'dist_max_iter must be >= 1'),
    'aiy_egm_ge_hist_batch:theta_inf+a_nan': (2, 'phi and theta must be finite'),
    'aiy_egm_ge_hist_batch:a_nan+a_dec': (2, 'a_grid(1) is not finite'),
    'aiy_egm_ge_hist_batch:a_dec+a_rep': (6, 'a_grid must be non-decreasing (a_grid(3) < a_grid(2))'),
    'aiy_egm_ge_hist_batch:a_rep+r_nan': (6, 'grid must be strictly increasing (point 5 repeats point 4)'),
    'aiy_egm_ge_hist_batch:null:r': (6, 'NULL argument'),
    'aiy_egm_ge_hist_batch:null:w': (6, 'NULL argument'),
    'aiy_egm_ge_hist_batch:null:pc': (6, 'NULL argument'),
    'aiy_egm_ge_hist_batch:null:s': (6, 'NULL argument'),
    'aiy_egm_ge_hist_batch:null:P': (6, 'NULL argument'),
    'aiy_egm_ge_hist_batch:null:Ks': (6, 'NULL argument'),
    'aiy_egm_ge_hist_batch:null:Kd': (6, 'NULL argument'),
    'aiy_egm_ge_hist_batch:null:it': (6, 'NULL argument'),
    'aiy_egm_ge_hist_batch:null:dit': (6, 'NULL argument'),
    'aiy_egm_ge_hist_batch:null:lam': (5, 'no HIP device visible'),
    'aiy_egm_ge_hist_batch:null:a': (6, 'a_grid is NULL'),
    'aiy_egm_ge_hist_batch:N0': (1, 'need C >= 1, N >= 1, Na >= 2'),
    'aiy_egm_ge_hist_batch:Na1': (1, 'need C >= 1, N >= 1, Na >= 2'),
    'aiy_egm_ge_hist_batch:phi_nan': (2, 'phi and theta must be finite'),
    'aiy_egm_ge_hist_batch:r_bad': (6, 'candidate 3: r must be finite with r + delta > 0'),
    'aiy_egm_ge_hist_batch:Na1+N17': (1, 'need C >= 1, N >= 1, Na >= 2'),
    'aiy_egm_ge_hist_batch:N17+dmax0': (1, 'EGM kernels support N <= 16 productivity states'),
    'aiy_egm_ge_hist_batch:noflag+theta_inf': (5, 'no HIP device visible'),
    'aiy_egm_ge_hist_batch:noflag+theta_inf+r_bad': (6, 'candidate 3: r must be finite with r + delta > 0'),
    'aiy_egm_ge_hist_batch:valid': (5, 'no HIP device visible'),
}


def _has_gpu():
    import torch
    return torch.cuda.is_available()


@pytest.mark.parametrize("row", ROWS)
def test_refusal_is_the_recorded_one(pkg, row):
    assert row in EXPECTED, "no recorded answer: run --record on the parent"
    if EXPECTED[row] == NO_DEVICE and _has_gpu():
        return  # not a refusal: with a device the call would run (see the module docstring)
    assert _answer(pkg.lib(), row) == EXPECTED[row]


def test_every_recorded_row_is_asked():
    assert sorted(EXPECTED) == sorted(ROWS) and len(set(ROWS)) == len(ROWS)


def test_the_table_shows_the_orders_that_differ():
    """Pairs of defects that two entries answer differently, because they order their checks
    differently: without these rows a shared validation helper could swap them unnoticed."""
    e = EXPECTED
    assert e["aiy_ge_batch:Na1+T0"][1] != e["aiy_ge_batch:T0"][1]                  # shape, then T
    assert e["aiy_egm_ge_batch:N17+T0"] == e["aiy_egm_ge_batch:N17"]               # N <= 16 first
    assert e["aiy_ge_hist_batch:maxiter0+dmax0"] == e["aiy_ge_hist_batch:maxiter0"]
    assert e["aiy_labor_ge_batch:maxiter0+psi_nan"] == e["aiy_labor_ge_batch:maxiter0"]
    assert e["aiy_labor_ge_batch:psi_nan+a_nan"] == e["aiy_labor_ge_batch:psi_nan"]
    assert e["aiy_vfi_solve:null:iters+null:v"][1] != e["aiy_vfi_solve:null:v"][1]
    assert e["aiy_dist_stationary:a_rep"] == NO_DEVICE                             # on-grid: allowed
    assert e["aiy_dist_stationary:lottery+a_rep"][0] == 6
    assert e["aiy_labor_vfi_sweep:psi_nan"] == NO_DEVICE != e["aiy_labor_ge_batch:psi_nan"]


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python -m tests.test_aiy_host_refusals_cpu --record")
    from tests.conftest import load_pkg
    lib_ = load_pkg().lib()
    for row_ in ROWS:
        print(f"    {row_!r}: {_answer(lib_, row_)!r},")
