"""No GPU: which refusal a Krusell-Smith host entry point answers, and in which order.

Every entry point validates its host arguments before it asks for a device, and a caller with two
defects sees the first check of that entry's own sequence.  The sequences differ between entries
(the two histogram tiers order grids and params differently, ks_egm_solve_jacobi tests its fit
rule before max_iter and has no k_size <= 2^20 test), so each row below is one (entry, defect) or
one (entry, two defects) with the status and the full aiy_last_error() text.  The expectations
are what the library answered before the host tier moved onto the typed staging helpers:
`python -m tests.test_ks_host_refusals_cpu --record` prints them from the library in the tree.

Shapes: nk = 5, nK = 2, nx = 5, T = 4, M = 2, C = 3 (ks_hist_cases.case(5, 5, 2, 4, 2)); the
device tiers get dummy host pointers in their device slots, which no refusal dereferences.

Left out: ks_policy_improve and ks_howard test only `k_opt == NULL` before they ask for a device
(the rest of their checks sit in the staging step behind it), so that is their one row here;
ks_vfi_solve is covered up to its shape test, the last one in front of the device, on one device
(n_devices > 1 goes to the sharded solve).  ks_shocks tests ug and ub in its device tier, behind
the device, likewise."""
import ctypes as C
import sys

import numpy as np
import pytest

from tests import ks_hist_cases as cases

NK, NKK, NX, T, M, NC, POP = 5, 2, 5, 4, 2, 3, 3


def _base(multi):
    """Fresh, valid, flat float64 arguments; `multi`: NC candidates' k_opt, K_grid and params."""
    c = cases.case(NX, NK, NKK, T, M)
    n = NC if multi else 1
    ko = np.asfortranarray(c["k_opt"]).reshape(-1, order="F")
    return dict(
        C=NC, nk=NK, nK=NKK, nx=NX, T=T, M=M, pop=POP, max_iter=5, max_vfi=5,
        k_opt=np.tile(ko, n), k_grid=c["k_grid"].copy(),
        K_grid=np.tile(c["K_grid"], n), x=c["x"].copy(), params=np.tile(c["params"], n),
        zi=np.asfortranarray(c["zi"].astype(np.float64)).reshape(-1, order="F"),
        zi8=np.zeros(T * M, np.int8), lam=np.ascontiguousarray(c["lam0"]).reshape(-1),
        K_ts=np.zeros(T * M), slow=np.zeros(M, np.int64), pol=np.array([0, 2], np.int32),
        U=np.full((T - 1) + POP + (T - 1) * POP, 0.5), zi1=np.zeros(T), eps=np.ones(T * POP),
        k_pop=np.full(POP, 30.0), B=np.tile([0.0, 1.0, 0.0, 1.0], n), P=np.full(16 * n, 0.25),
        iters=np.zeros(n, np.int64), diff=np.zeros(n), status=np.zeros(n, np.int32),
        value=np.zeros(NK * NKK * 4), nfev=np.zeros(NK * NKK * 4, np.int32), rel=np.zeros(1),
        scratch=np.zeros(64), dummy=np.zeros(64))


def _set(key, idx, v):
    def f(a):
        a[key][idx] = v
    return f


def _nx_big(a):
    a.update(nx=3000, x=cases.grid7(3000), lam=np.zeros(2 * 3000 * max(a["M"], 1)))


def _egm_big(a):          # past ks_egm_fits and past the Jacobi rule 32 * nk <= 150 KiB
    n = a["K_grid"].size // NKK
    a.update(nk=6000, nK=4, k_grid=np.linspace(1.0, 2.0, 6000),
             K_grid=np.linspace(30.0, 50.0, 4 * n), k_opt=np.ones(6000 * 4 * 4 * n))


DEFECTS = {
    "T0": lambda a: a.update(T=0), "M0": lambda a: a.update(M=0),
    "pop0": lambda a: a.update(pop=0), "C0": lambda a: a.update(C=0),
    "nK1": lambda a: a.update(nK=1), "nk2": lambda a: a.update(nk=2),
    "nk_huge": lambda a: a.update(nk=2 ** 20 + 1),
    "maxiter0": lambda a: a.update(max_iter=0), "maxvfi0": lambda a: a.update(max_vfi=0),
    "nx_big": _nx_big, "egm_big": _egm_big,
    "nK0": lambda a: a.update(nK=0),
    # the repeated point differs per grid, so the message tells which grid was refused
    "kgrid_repeat": lambda a: _set("k_grid", 2, a["k_grid"][1])(a),
    "Kgrid_repeat": lambda a: _set("K_grid", -1, a["K_grid"][-2])(a),   # the last candidate's
    "Kgrid_neg": _set("K_grid", -1, 0.0),
    "x_repeat": lambda a: _set("x", 3, a["x"][2])(a),
    "params_nan": _set("params", -13, np.nan), "ug_bad": _set("params", -13 + 5, 1.5),
    "pol_bad": _set("pol", 1, 3), "kopt_inf": _set("k_opt", 3, np.inf),
    "lam_nan": _set("lam", 3, np.nan), "zi_bad": _set("zi", 2, 2.0),
    "zi1_bad": _set("zi1", 2, 0.5), "eps_bad": _set("eps", 1, 3.0),
    "kpop_nan": _set("k_pop", 0, np.nan),
}


def _apply(a, defect):
    if defect.startswith("null:"):
        a[defect[5:]] = None
    else:
        DEFECTS[defect](a)


def _p(x):
    return None if x is None else x.ctypes.data_as(C.c_void_p)


def _i(v):
    return C.c_int64(v)


# ---- one caller per entry point: a -> status.  Device slots get a["dummy"] unless the defect
# under test is that very pointer (then the row names the host key it replaced).
def _shocks(L, a):
    return L.ks_shocks(_i(a["T"]), _i(a["pop"]), _p(a["U"]), _p(a["params"]), _p(a["zi1"]),
                       _p(a["eps"]))


def _capital(L, a):
    return L.ks_simulate_capital(_p(a["k_opt"]), _p(a["k_grid"]), _p(a["K_grid"]), _i(a["nk"]),
                                 _i(a["nK"]), _p(a["zi1"]), _p(a["eps"]), _i(a["T"]),
                                 _i(a["pop"]), _p(a["k_pop"]), _p(a["K_ts"]))


def _hist(L, a):
    return L.ks_simulate_hist(_p(a["k_opt"]), _p(a["k_grid"]), _p(a["K_grid"]), _i(a["nk"]),
                              _i(a["nK"]), _p(a["x"]), _i(a["nx"]), _p(a["params"]), _p(a["zi"]),
                              _i(a["T"]), _i(a["M"]), _p(a["lam"]), _p(a["K_ts"]), _p(a["slow"]))


def _hist_multi(L, a):
    return L.ks_simulate_hist_multi(_i(a["C"]), _p(a["k_opt"]), _p(a["k_grid"]), _p(a["K_grid"]),
                                    _i(a["nk"]), _i(a["nK"]), _p(a["x"]), _i(a["nx"]),
                                    _p(a["params"]), _p(a["pol"]), _p(a["zi"]), _i(a["T"]),
                                    _i(a["M"]), _p(a["lam"]), _p(a["K_ts"]), _p(a["slow"]))


def _dev(a, key):
    """The dummy pointer for a device slot, NULL when the row nulls that argument."""
    return None if a[key] is None else _p(a["dummy"])


def _hist_dev(L, a):
    return L.ks_simulate_hist_dev(_i(a["nk"]), _i(a["nK"]), _dev(a, "k_grid"), _dev(a, "K_grid"),
                                  _dev(a, "k_opt"), _dev(a, "x"), _i(a["nx"]), _p(a["params"]),
                                  _dev(a, "zi8"), _i(a["T"]), _i(a["M"]), _dev(a, "lam"),
                                  _dev(a, "K_ts"), None, None)


def _hist_multi_dev(L, a):
    return L.ks_simulate_hist_multi_dev(
        _i(a["C"]), _i(a["nk"]), _i(a["nK"]), _dev(a, "k_grid"), _dev(a, "K_grid"),
        _dev(a, "k_opt"), _dev(a, "x"), _i(a["nx"]), _p(a["params"]), _p(a["pol"]),
        _dev(a, "zi8"), _i(a["T"]), _i(a["M"]), _dev(a, "lam"), _dev(a, "K_ts"), None,
        _dev(a, "scratch"), None)


def _egm_args(a):
    return (_p(a["k_opt"]), _p(a["k_grid"]), _p(a["K_grid"]), _p(a["B"]), _p(a["P"]),
            _p(a["params"]), _i(a["nk"]), _i(a["nK"]), C.c_double(1e-6), _i(a["max_iter"]),
            _p(a["iters"]), _p(a["diff"]))


def _egm(L, a):
    return L.ks_egm_solve(*_egm_args(a))


def _egm_jacobi(L, a):
    return L.ks_egm_solve_jacobi(*_egm_args(a))


def _egm_batch(L, a):
    return L.ks_egm_solve_batch(_i(a["C"]), *_egm_args(a), _p(a["status"]))


def _egm_batch_dev(L, a):
    args = list(_egm_args(a))
    args[0], args[1] = _dev(a, "k_opt"), _dev(a, "k_grid")
    args[10], args[11] = _dev(a, "iters"), _dev(a, "diff")
    return L.ks_egm_solve_batch_dev(_i(a["C"]), *args, _dev(a, "status"), _dev(a, "scratch"),
                                    None)


def _improve(L, a):
    return L.ks_policy_improve(_p(a["value"]), _p(a["k_grid"]), _p(a["K_grid"]), _p(a["B"]),
                               _p(a["P"]), _p(a["params"]), _i(a["nk"]), _i(a["nK"]),
                               _p(a["k_opt"]), _p(a["nfev"]))


def _howard(L, a):
    return L.ks_howard(_p(a["value"]), _p(a["k_opt"]), _p(a["k_grid"]), _p(a["K_grid"]),
                       _p(a["B"]), _p(a["P"]), _p(a["params"]), _i(a["nk"]), _i(a["nK"]), _i(3))


def _vfi(L, a):
    return L.ks_vfi_solve(_p(a["value"]), _p(a["k_opt"]), _p(a["k_grid"]), _p(a["K_grid"]),
                          _p(a["B"]), _p(a["P"]), _p(a["params"]), _i(a["nk"]), _i(a["nK"]),
                          _i(2), C.c_double(1e-6), _i(a["max_vfi"]), C.c_int(1), _p(a["iters"]),
                          _p(a["rel"]))


# entry -> (caller, candidate-major inputs, its sequence of checks as one defect each, further
# rows).  Rows: every defect of the sequence alone, every adjacent pair of it, and the extras.
ENTRIES = {
    "ks_shocks": (_shocks, False, ["null:U", "T0", "pop0"], []),
    "ks_simulate_capital": (_capital, False,
                            ["null:k_opt", "T0", "pop0", "nK1", "kgrid_repeat", "Kgrid_repeat",
                             "zi1_bad", "eps_bad", "kpop_nan"],
                            [("null:k_grid",), ("null:K_grid",)]),
    "ks_simulate_hist": (_hist, False,
                         ["null:k_opt", "T0", "M0", "nx_big", "kgrid_repeat", "Kgrid_repeat",
                          "x_repeat", "params_nan", "ug_bad", "kopt_inf", "lam_nan", "zi_bad"],
                         [("kgrid_repeat", "params_nan"), ("x_repeat", "ug_bad")]),
    "ks_simulate_hist_multi": (_hist_multi, True,
                               ["null:pol", "T0", "M0", "nx_big", "C0", "params_nan", "ug_bad",
                                "pol_bad", "kgrid_repeat", "Kgrid_repeat", "x_repeat",
                                "kopt_inf", "lam_nan", "zi_bad"],
                               [("kgrid_repeat", "params_nan"), ("pol_bad", "x_repeat"),
                                ("x_repeat", "ug_bad")]),
    "ks_simulate_hist_dev": (_hist_dev, False,
                             ["null:k_opt", "T0", "M0", "nx_big", "params_nan", "ug_bad"],
                             [("null:params",)]),
    "ks_simulate_hist_multi_dev": (_hist_multi_dev, True,
                                   ["null:scratch", "T0", "M0", "nx_big", "C0", "params_nan",
                                    "ug_bad", "pol_bad"], [("null:pol",)]),
    "ks_egm_solve": (_egm, False,
                     ["null:B", "nk2", "maxiter0", "egm_big", "kgrid_repeat", "Kgrid_neg"],
                     [("nk_huge",), ("nk_huge", "maxiter0")]),
    "ks_egm_solve_jacobi": (_egm_jacobi, False,
                            ["null:B", "nK0", "egm_big", "maxiter0", "kgrid_repeat", "Kgrid_neg"],
                            [("nk2",), ("nk_huge",), ("nk_huge", "maxiter0")]),
    "ks_egm_solve_batch": (_egm_batch, True,
                           ["null:status", "C0", "nk2", "maxiter0", "egm_big", "Kgrid_neg",
                            "kgrid_repeat"], [("nk_huge",), ("nk_huge", "maxiter0")]),
    "ks_egm_solve_batch_dev": (_egm_batch_dev, True,
                               ["null:scratch", "C0", "nk2", "maxiter0", "egm_big", "Kgrid_neg"],
                               [("nk_huge",)]),
    "ks_policy_improve": (_improve, False, ["null:k_opt"], []),
    "ks_howard": (_howard, False, ["null:k_opt"], []),
    "ks_vfi_solve": (_vfi, False, ["null:iters", "maxvfi0", "null:value", "nk2"],
                     [("null:k_opt",), ("null:rel",)]),
}


def _rows():
    out = []
    for entry, (_, _, seq, extra) in ENTRIES.items():
        rows = [(d,) for d in seq] + list(zip(seq, seq[1:])) + list(extra)
        out += [f"{entry}:{'+'.join(r)}" for r in rows]
    return out


ROWS = _rows()


def _answer(L, row):
    entry, defects = row.split(":", 1)
    call, multi, _, _ = ENTRIES[entry]
    a = _base(multi)
    for d in sorted(defects.split("+"), key=lambda d: not d.endswith("_big")):  # resizing first
        _apply(a, d)
    rc = call(L, a)
    return rc, L.aiy_last_error().decode()


EXPECTED = {
    'ks_shocks:null:U': (6, 'NULL argument'),
    'ks_shocks:T0': (1, 'T must be in [1, 2^30]'),
    'ks_shocks:pop0': (1, 'population must be in [1, 2^31)'),
    'ks_shocks:null:U+T0': (6, 'NULL argument'),
    'ks_shocks:T0+pop0': (1, 'T must be in [1, 2^30]'),
    'ks_simulate_capital:null:k_opt': (6, 'NULL argument'),
    'ks_simulate_capital:T0': (1, 'T must be in [1, 2^30]'),
    'ks_simulate_capital:pop0': (1, 'population must be in [1, 2^31)'),
    'ks_simulate_capital:nK1': (1, 'need k_size, K_size >= 2'),
    'ks_simulate_capital:kgrid_repeat': (6, 'grid must be strictly increasing (point 3 repeats point 2)'),
    'ks_simulate_capital:Kgrid_repeat': (6, 'grid must be strictly increasing (point 2 repeats point 1)'),
    'ks_simulate_capital:zi1_bad': (6, 'zi_shock must hold 0 (good) or 1 (bad)'),
    'ks_simulate_capital:eps_bad': (6, 'epsi_shock must hold 1 (employed) or 2 (unemployed)'),
    'ks_simulate_capital:kpop_nan': (2, 'non-finite k_population'),
    'ks_simulate_capital:null:k_opt+T0': (6, 'NULL argument'),
    'ks_simulate_capital:T0+pop0': (1, 'T must be in [1, 2^30]'),
    'ks_simulate_capital:pop0+nK1': (1, 'population must be in [1, 2^31)'),
    'ks_simulate_capital:nK1+kgrid_repeat': (1, 'need k_size, K_size >= 2'),
    'ks_simulate_capital:kgrid_repeat+Kgrid_repeat': (6, 'grid must be strictly increasing (point 3 repeats point 2)'),
    'ks_simulate_capital:Kgrid_repeat+zi1_bad': (6, 'grid must be strictly increasing (point 2 repeats point 1)'),
    'ks_simulate_capital:zi1_bad+eps_bad': (6, 'zi_shock must hold 0 (good) or 1 (bad)'),
    'ks_simulate_capital:eps_bad+kpop_nan': (6, 'epsi_shock must hold 1 (employed) or 2 (unemployed)'),
    'ks_simulate_capital:null:k_grid': (6, 'a_grid is NULL'),
    'ks_simulate_capital:null:K_grid': (6, 'a_grid is NULL'),
    'ks_simulate_hist:null:k_opt': (6, 'NULL argument'),
    'ks_simulate_hist:T0': (1, 'T must be in [2, 2^30]'),
    'ks_simulate_hist:M0': (1, 'need 1 <= M <= 65,535 shock paths'),
    'ks_simulate_hist:nx_big': (1, "histogram simulation: need nx, k_size, K_size >= 2 and a path's state inside one CU's LDS: 8*(8*nx + K_size + 8) + 4*(5*nx + 4) <= 160 KiB"),
    'ks_simulate_hist:kgrid_repeat': (6, 'grid must be strictly increasing (point 3 repeats point 2)'),
    'ks_simulate_hist:Kgrid_repeat': (6, 'grid must be strictly increasing (point 2 repeats point 1)'),
    'ks_simulate_hist:x_repeat': (6, 'grid must be strictly increasing (point 4 repeats point 3)'),
    'ks_simulate_hist:params_nan': (2, 'non-finite params'),
    'ks_simulate_hist:ug_bad': (6, 'ug and ub must lie in (0, 1)'),
    'ks_simulate_hist:kopt_inf': (2, 'non-finite k_opt'),
    'ks_simulate_hist:lam_nan': (2, 'non-finite lam'),
    'ks_simulate_hist:zi_bad': (6, 'zi_shock must hold 0 (good) or 1 (bad)'),
    'ks_simulate_hist:null:k_opt+T0': (6, 'NULL argument'),
    'ks_simulate_hist:T0+M0': (1, 'T must be in [2, 2^30]'),
    'ks_simulate_hist:M0+nx_big': (1, 'need 1 <= M <= 65,535 shock paths'),
    'ks_simulate_hist:nx_big+kgrid_repeat': (1, "histogram simulation: need nx, k_size, K_size >= 2 and a path's state inside one CU's LDS: 8*(8*nx + K_size + 8) + 4*(5*nx + 4) <= 160 KiB"),
    'ks_simulate_hist:kgrid_repeat+Kgrid_repeat': (6, 'grid must be strictly increasing (point 3 repeats point 2)'),
    'ks_simulate_hist:Kgrid_repeat+x_repeat': (6, 'grid must be strictly increasing (point 2 repeats point 1)'),
    'ks_simulate_hist:x_repeat+params_nan': (6, 'grid must be strictly increasing (point 4 repeats point 3)'),
    'ks_simulate_hist:params_nan+ug_bad': (2, 'non-finite params'),
    'ks_simulate_hist:ug_bad+kopt_inf': (6, 'ug and ub must lie in (0, 1)'),
    'ks_simulate_hist:kopt_inf+lam_nan': (2, 'non-finite k_opt'),
    'ks_simulate_hist:lam_nan+zi_bad': (2, 'non-finite lam'),
    'ks_simulate_hist:kgrid_repeat+params_nan': (6, 'grid must be strictly increasing (point 3 repeats point 2)'),
    'ks_simulate_hist:x_repeat+ug_bad': (6, 'grid must be strictly increasing (point 4 repeats point 3)'),
    'ks_simulate_hist_multi:null:pol': (6, 'NULL argument'),
    'ks_simulate_hist_multi:T0': (1, 'T must be in [2, 2^30]'),
    'ks_simulate_hist_multi:M0': (1, 'need 1 <= M <= 65,535 shock paths'),
    'ks_simulate_hist_multi:nx_big': (1, "histogram simulation: need nx, k_size, K_size >= 2 and a path's state inside one CU's LDS: 8*(8*nx + K_size + 8) + 4*(5*nx + 4) <= 160 KiB"),
    'ks_simulate_hist_multi:C0': (1, 'need 1 <= C <= 65,535 candidates'),
    'ks_simulate_hist_multi:params_nan': (2, 'non-finite params'),
    'ks_simulate_hist_multi:ug_bad': (6, 'ug and ub must lie in (0, 1)'),
    'ks_simulate_hist_multi:pol_bad': (6, 'policy_of_path(2) = 3 is outside [0, C)'),
    'ks_simulate_hist_multi:kgrid_repeat': (6, 'grid must be strictly increasing (point 3 repeats point 2)'),
    'ks_simulate_hist_multi:Kgrid_repeat': (6, 'grid must be strictly increasing (point 2 repeats point 1)'),
    'ks_simulate_hist_multi:x_repeat': (6, 'grid must be strictly increasing (point 4 repeats point 3)'),
    'ks_simulate_hist_multi:kopt_inf': (2, 'non-finite k_opt'),
    'ks_simulate_hist_multi:lam_nan': (2, 'non-finite lam'),
    'ks_simulate_hist_multi:zi_bad': (6, 'zi_shock must hold 0 (good) or 1 (bad)'),
    'ks_simulate_hist_multi:null:pol+T0': (6, 'NULL argument'),
    'ks_simulate_hist_multi:T0+M0': (1, 'T must be in [2, 2^30]'),
    'ks_simulate_hist_multi:M0+nx_big': (1, 'need 1 <= M <= 65,535 shock paths'),
    'ks_simulate_hist_multi:nx_big+C0': (1, "histogram simulation: need nx, k_size, K_size >= 2 and a path's state inside one CU's LDS: 8*(8*nx + K_size + 8) + 4*(5*nx + 4) <= 160 KiB"),
    'ks_simulate_hist_multi:C0+params_nan': (1, 'need 1 <= C <= 65,535 candidates'),
    'ks_simulate_hist_multi:params_nan+ug_bad': (2, 'non-finite params'),
    'ks_simulate_hist_multi:ug_bad+pol_bad': (6, 'ug and ub must lie in (0, 1)'),
    'ks_simulate_hist_multi:pol_bad+kgrid_repeat': (6, 'policy_of_path(2) = 3 is outside [0, C)'),
    'ks_simulate_hist_multi:kgrid_repeat+Kgrid_repeat': (6, 'grid must be strictly increasing (point 3 repeats point 2)'),
    'ks_simulate_hist_multi:Kgrid_repeat+x_repeat': (6, 'grid must be strictly increasing (point 2 repeats point 1)'),
    'ks_simulate_hist_multi:x_repeat+kopt_inf': (6, 'grid must be strictly increasing (point 4 repeats point 3)'),
    'ks_simulate_hist_multi:kopt_inf+lam_nan': (2, 'non-finite k_opt'),
    'ks_simulate_hist_multi:lam_nan+zi_bad': (2, 'non-finite lam'),
    'ks_simulate_hist_multi:kgrid_repeat+params_nan': (2, 'non-finite params'),
    'ks_simulate_hist_multi:pol_bad+x_repeat': (6, 'policy_of_path(2) = 3 is outside [0, C)'),
    'ks_simulate_hist_multi:x_repeat+ug_bad': (6, 'ug and ub must lie in (0, 1)'),
    'ks_simulate_hist_dev:null:k_opt': (6, 'NULL argument'),
    'ks_simulate_hist_dev:T0': (1, 'T must be in [2, 2^30]'),
    'ks_simulate_hist_dev:M0': (1, 'need 1 <= M <= 65,535 shock paths'),
    'ks_simulate_hist_dev:nx_big': (1, "histogram simulation: need nx, k_size, K_size >= 2 and a path's state inside one CU's LDS: 8*(8*nx + K_size + 8) + 4*(5*nx + 4) <= 160 KiB"),
    'ks_simulate_hist_dev:params_nan': (2, 'non-finite params'),
    'ks_simulate_hist_dev:ug_bad': (6, 'ug and ub must lie in (0, 1)'),
    'ks_simulate_hist_dev:null:k_opt+T0': (6, 'NULL argument'),
    'ks_simulate_hist_dev:T0+M0': (1, 'T must be in [2, 2^30]'),
    'ks_simulate_hist_dev:M0+nx_big': (1, 'need 1 <= M <= 65,535 shock paths'),
    'ks_simulate_hist_dev:nx_big+params_nan': (1, "histogram simulation: need nx, k_size, K_size >= 2 and a path's state inside one CU's LDS: 8*(8*nx + K_size + 8) + 4*(5*nx + 4) <= 160 KiB"),
    'ks_simulate_hist_dev:params_nan+ug_bad': (2, 'non-finite params'),
    'ks_simulate_hist_dev:null:params': (6, 'NULL argument'),
    'ks_simulate_hist_multi_dev:null:scratch': (6, 'NULL argument'),
    'ks_simulate_hist_multi_dev:T0': (1, 'T must be in [2, 2^30]'),
    'ks_simulate_hist_multi_dev:M0': (1, 'need 1 <= M <= 65,535 shock paths'),
    'ks_simulate_hist_multi_dev:nx_big': (1, "histogram simulation: need nx, k_size, K_size >= 2 and a path's state inside one CU's LDS: 8*(8*nx + K_size + 8) + 4*(5*nx + 4) <= 160 KiB"),
    'ks_simulate_hist_multi_dev:C0': (1, 'need 1 <= C <= 65,535 candidates'),
    'ks_simulate_hist_multi_dev:params_nan': (2, 'non-finite params'),
    'ks_simulate_hist_multi_dev:ug_bad': (6, 'ug and ub must lie in (0, 1)'),
    'ks_simulate_hist_multi_dev:pol_bad': (6, 'policy_of_path(2) = 3 is outside [0, C)'),
    'ks_simulate_hist_multi_dev:null:scratch+T0': (6, 'NULL argument'),
    'ks_simulate_hist_multi_dev:T0+M0': (1, 'T must be in [2, 2^30]'),
    'ks_simulate_hist_multi_dev:M0+nx_big': (1, 'need 1 <= M <= 65,535 shock paths'),
    'ks_simulate_hist_multi_dev:nx_big+C0': (1, "histogram simulation: need nx, k_size, K_size >= 2 and a path's state inside one CU's LDS: 8*(8*nx + K_size + 8) + 4*(5*nx + 4) <= 160 KiB"),
    'ks_simulate_hist_multi_dev:C0+params_nan': (1, 'need 1 <= C <= 65,535 candidates'),
    'ks_simulate_hist_multi_dev:params_nan+ug_bad': (2, 'non-finite params'),
    'ks_simulate_hist_multi_dev:ug_bad+pol_bad': (6, 'ug and ub must lie in (0, 1)'),
    'ks_simulate_hist_multi_dev:null:pol': (6, 'NULL argument'),
    'ks_egm_solve:null:B': (6, 'NULL argument'),
    'ks_egm_solve:nk2': (1, 'need k_size >= 3 and K_size >= 1'),
    'ks_egm_solve:maxiter0': (6, 'max_iter in [1, 2^31)'),
    'ks_egm_solve:egm_big': (1, 'k_size x K_size too large for the one-workgroup EGM solve'),
    'ks_egm_solve:kgrid_repeat': (6, 'grid must be strictly increasing (point 3 repeats point 2)'),
    'ks_egm_solve:Kgrid_neg': (2, 'K_grid must be positive and finite'),
    'ks_egm_solve:null:B+nk2': (6, 'NULL argument'),
    'ks_egm_solve:nk2+maxiter0': (1, 'need k_size >= 3 and K_size >= 1'),
    'ks_egm_solve:maxiter0+egm_big': (6, 'max_iter in [1, 2^31)'),
    'ks_egm_solve:egm_big+kgrid_repeat': (1, 'k_size x K_size too large for the one-workgroup EGM solve'),
    'ks_egm_solve:kgrid_repeat+Kgrid_neg': (6, 'grid must be strictly increasing (point 3 repeats point 2)'),
    'ks_egm_solve:nk_huge': (1, 'need k_size >= 3 and K_size >= 1'),
    'ks_egm_solve:nk_huge+maxiter0': (1, 'need k_size >= 3 and K_size >= 1'),
    'ks_egm_solve_jacobi:null:B': (6, 'NULL argument'),
    'ks_egm_solve_jacobi:nK0': (1, 'need k_size >= 3 and K_size >= 1'),
    'ks_egm_solve_jacobi:egm_big': (1, 'k_size too large for one workgroup per (s, K) pair'),
    'ks_egm_solve_jacobi:maxiter0': (6, 'max_iter in [1, 2^31)'),
    'ks_egm_solve_jacobi:kgrid_repeat': (6, 'grid must be strictly increasing (point 3 repeats point 2)'),
    'ks_egm_solve_jacobi:Kgrid_neg': (2, 'K_grid must be positive and finite'),
    'ks_egm_solve_jacobi:null:B+nK0': (6, 'NULL argument'),
    'ks_egm_solve_jacobi:nK0+egm_big': (1, 'need k_size >= 3 and K_size >= 1'),
    'ks_egm_solve_jacobi:egm_big+maxiter0': (1, 'k_size too large for one workgroup per (s, K) pair'),
    'ks_egm_solve_jacobi:maxiter0+kgrid_repeat': (6, 'max_iter in [1, 2^31)'),
    'ks_egm_solve_jacobi:kgrid_repeat+Kgrid_neg': (6, 'grid must be strictly increasing (point 3 repeats point 2)'),
    'ks_egm_solve_jacobi:nk2': (1, 'need k_size >= 3 and K_size >= 1'),
    'ks_egm_solve_jacobi:nk_huge': (1, 'k_size too large for one workgroup per (s, K) pair'),
    'ks_egm_solve_jacobi:nk_huge+maxiter0': (1, 'k_size too large for one workgroup per (s, K) pair'),
    'ks_egm_solve_batch:null:status': (6, 'NULL argument'),
    'ks_egm_solve_batch:C0': (1, 'need 1 <= C <= 65,535 candidates'),
    'ks_egm_solve_batch:nk2': (1, 'need k_size >= 3 and K_size >= 1'),
    'ks_egm_solve_batch:maxiter0': (6, 'max_iter in [1, 2^31)'),
    'ks_egm_solve_batch:egm_big': (1, 'k_size x K_size too large for the one-workgroup EGM solve'),
    'ks_egm_solve_batch:Kgrid_neg': (2, 'K_grid must be positive and finite (candidate 3)'),
    'ks_egm_solve_batch:kgrid_repeat': (6, 'grid must be strictly increasing (point 3 repeats point 2)'),
    'ks_egm_solve_batch:null:status+C0': (6, 'NULL argument'),
    'ks_egm_solve_batch:C0+nk2': (1, 'need 1 <= C <= 65,535 candidates'),
    'ks_egm_solve_batch:nk2+maxiter0': (1, 'need k_size >= 3 and K_size >= 1'),
    'ks_egm_solve_batch:maxiter0+egm_big': (6, 'max_iter in [1, 2^31)'),
    'ks_egm_solve_batch:egm_big+Kgrid_neg': (1, 'k_size x K_size too large for the one-workgroup EGM solve'),
    'ks_egm_solve_batch:Kgrid_neg+kgrid_repeat': (2, 'K_grid must be positive and finite (candidate 3)'),
    'ks_egm_solve_batch:nk_huge': (1, 'need k_size >= 3 and K_size >= 1'),
    'ks_egm_solve_batch:nk_huge+maxiter0': (1, 'need k_size >= 3 and K_size >= 1'),
    'ks_egm_solve_batch_dev:null:scratch': (6, 'NULL argument'),
    'ks_egm_solve_batch_dev:C0': (1, 'need 1 <= C <= 65,535 candidates'),
    'ks_egm_solve_batch_dev:nk2': (1, 'need k_size >= 3 and K_size >= 1'),
    'ks_egm_solve_batch_dev:maxiter0': (6, 'max_iter in [1, 2^31)'),
    'ks_egm_solve_batch_dev:egm_big': (1, 'k_size x K_size too large for the one-workgroup EGM solve'),
    'ks_egm_solve_batch_dev:Kgrid_neg': (2, 'K_grid must be positive and finite (candidate 3)'),
    'ks_egm_solve_batch_dev:null:scratch+C0': (6, 'NULL argument'),
    'ks_egm_solve_batch_dev:C0+nk2': (1, 'need 1 <= C <= 65,535 candidates'),
    'ks_egm_solve_batch_dev:nk2+maxiter0': (1, 'need k_size >= 3 and K_size >= 1'),
    'ks_egm_solve_batch_dev:maxiter0+egm_big': (6, 'max_iter in [1, 2^31)'),
    'ks_egm_solve_batch_dev:egm_big+Kgrid_neg': (1, 'k_size x K_size too large for the one-workgroup EGM solve'),
    'ks_egm_solve_batch_dev:nk_huge': (1, 'need k_size >= 3 and K_size >= 1'),
    'ks_policy_improve:null:k_opt': (6, 'NULL k_opt'),
    'ks_howard:null:k_opt': (6, 'NULL k_opt'),
    'ks_vfi_solve:null:iters': (6, 'NULL argument'),
    'ks_vfi_solve:maxvfi0': (6, 'max_vfi >= 1, howard_steps >= 0'),
    'ks_vfi_solve:null:value': (6, 'NULL argument'),
    'ks_vfi_solve:nk2': (1, 'need k_size >= 3 and K_size >= 1'),
    'ks_vfi_solve:null:iters+maxvfi0': (6, 'NULL argument'),
    'ks_vfi_solve:maxvfi0+null:value': (6, 'max_vfi >= 1, howard_steps >= 0'),
    'ks_vfi_solve:null:value+nk2': (6, 'NULL argument'),
    'ks_vfi_solve:null:k_opt': (6, 'NULL argument'),
    'ks_vfi_solve:null:rel': (6, 'NULL argument'),
}


@pytest.mark.parametrize("row", ROWS)
def test_refusal_is_the_recorded_one(pkg, row):
    assert row in EXPECTED, "no recorded answer: run --record on the parent"
    assert _answer(pkg.lib(), row) == EXPECTED[row]


def test_every_recorded_row_is_asked():
    assert sorted(EXPECTED) == sorted(ROWS) and len(set(ROWS)) == len(ROWS)


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python -m tests.test_ks_host_refusals_cpu --record")
    from tests.conftest import load_pkg
    lib_ = load_pkg().lib()
    for row_ in ROWS:
        print(f"    {row_!r}: {_answer(lib_, row_)!r},")
