"""No GPU: the inputs of the batched Krusell-Smith EGM tests do what the GPU comparisons rely on
(asserted with the C oracle and the numpy restatement), every refusal of the new entry points
comes back with its status before a device is needed, and the Python layer's shape errors."""
import ctypes as C

import numpy as np
import pytest

from tests import ks_egm_batch_cases as bc


def _raises(pkg, status, fn, *a, **kw):
    with pytest.raises(pkg.AiyError) as e:
        fn(*a, **kw)
    assert e.value.status == status, str(e.value)


# ------------------------------------------------------------------ the inputs' conditions
@pytest.mark.parametrize("carry", [False, True])
def test_alm_rounds_exercise_what_the_gpu_tests_compare(pkg, carry):
    """Three ALM rounds of E0, E1, E2 from the oracles, with λ restarted each round and with the
    carried λ of the drivers: no candidate lacks valid EGM points (the oracle would raise), K_ts
    stays positive and finite, the sweep counts differ across candidates and rounds (the cap,
    and early stops), and E2 alone has slow-path periods in rounds 2 and 3, so one launch runs
    both gather orders side by side."""
    R = bc.oracle_rounds(pkg, carry)
    iters = [r["iters"] for r in R]
    if carry:
        assert iters == [[400, 370, 128], [400, 400, 400], [400, 306, 125]]
        slow2 = [[0, 0], [9, 4], [9, 4]]
    else:
        assert iters == [[400, 370, 120], [400, 400, 400], [400, 306, 118]]
        slow2 = [[0, 0], [7, 4], [7, 4]]
    assert [s.tolist() for s in R[2]["slow"]] == slow2
    for e in (0, 1):
        assert not np.any(R[e]["slow"])
    for r in R:
        assert len(r["B_history"]) == bc.ROUNDS          # no economy converges in three rounds
        for K in r["K_ts"]:
            assert np.all(np.isfinite(K)) and np.all(K > 0)
        for ko in r["k_opt"]:
            assert np.all(np.isfinite(ko))


def test_regression_window_has_both_aggregate_states(pkg):
    zi = bc.inputs(pkg)["zi"]
    ts = np.arange(bc.T_DISCARD - 1, bc.T - 1)
    assert (int((zi[ts] == 0).sum()), int((zi[ts] == 1).sum())) == (49, 11)
    assert zi.shape == (bc.T, bc.N_PATHS) and not np.array_equal(zi[:, 0], zi[:, 1])


def test_economies_differ_where_the_batch_is_per_candidate(pkg):
    I = bc.inputs(pkg)
    assert not np.array_equal(I["P"][0], I["P"][2]) and np.array_equal(I["P"][0], I["P"][1])
    assert not np.array_equal(I["K_grid"][0], I["K_grid"][1])
    assert len({tuple(p) for p in I["prm"]}) == 3
    # the three-sweep policies of the histogram test: finite, and E2's employment table differs
    assert np.all(np.isfinite(bc.sweeps3(pkg)))
    from tests import ks_hist_ref as ref
    assert not np.array_equal(ref.thr_table(I["prm"][0]), ref.thr_table(I["prm"][2]))


def test_failing_candidate_fails_in_the_oracle(pkg):
    """The failing candidate of the GPU test.  An all-NaN k_opt start does not fail: the c_next
    floor maps NaN to 1e-8 (Krusell_Smith_EGM.m:181), so every k_current is finite and the
    oracle runs it.  What has no valid EGM point is ks_cases' `nanP` construction, a NaN row
    P(4, :): every k_current of the s = 4 pairs is NaN and the oracle returns rc != 0."""
    I = bc.inputs(pkg)
    S = bc.oracle_solve(I, 0, np.full_like(I["k0"], np.nan), bc.B_IDENTITY, max_iter=3)
    assert S["iters"] == 3
    J = dict(I, P=np.stack([bc.nan_row_P(I["P"][0])] * 3))
    with pytest.raises(ValueError):
        bc.oracle_solve(J, 0, I["k0"], bc.B_IDENTITY, max_iter=3)


# ------------------------------------------------------------------ refusals, no device
def _egm_args(pkg, C_=3):
    I = bc.inputs(pkg)
    k0 = np.broadcast_to(I["k0"], (C_,) + I["k0"].shape)
    return [k0, I["k_grid"], I["K_grid"][:C_], bc.B_IDENTITY, I["P"][:C_], I["prm"][:C_]]


def test_egm_batch_refusals(pkg):
    a = _egm_args(pkg)
    bad = list(a)
    bad[1] = a[1].copy()
    bad[1][5] = bad[1][4]
    _raises(pkg, "AIY_BAD_ARG", pkg.ks_egm_solve_batch, *bad)            # non-strict k_grid
    bad = list(a)
    bad[2] = a[2].copy()
    bad[2][1, 2] = 0.0
    _raises(pkg, "AIY_NON_FINITE", pkg.ks_egm_solve_batch, *bad)         # candidate 1's row only
    bad[2][1, 2] = np.inf
    _raises(pkg, "AIY_NON_FINITE", pkg.ks_egm_solve_batch, *bad)
    _raises(pkg, "AIY_BAD_ARG", pkg.ks_egm_solve_batch, *a, max_iter=0)
    _raises(pkg, "AIY_BAD_ARG", pkg.ks_egm_solve_batch, *a, max_iter=2 ** 31)


def _egm_raw(pkg, C_, nk, nK, null=None, dev=False):
    """ks_egm_solve_batch[_dev] on small zero arrays (refused before they are read), argument
    `null` passed as NULL."""
    L = pkg.lib()
    n = max(C_, 1)
    arrs = dict(k_opt=np.ones(8), k_grid=np.arange(1.0, nk + 1.0) if nk < 10 ** 6 else np.ones(8),
                K_grid=np.ones(n * nK if nK < 10 ** 6 else 8), B=np.zeros(4 * n),
                P=np.zeros(16 * n), params=np.zeros(13 * n), iters=np.zeros(n, np.int64),
                diff=np.zeros(n), status=np.zeros(n, np.int32), scratch=np.zeros(8))
    p = {k: (None if k == null else v.ctypes.data_as(C.c_void_p)) for k, v in arrs.items()}
    head = (C.c_int64(C_), p["k_opt"], p["k_grid"], p["K_grid"], p["B"], p["P"], p["params"],
            C.c_int64(nk), C.c_int64(nK), C.c_double(1e-6), C.c_int64(5), p["iters"], p["diff"],
            p["status"])
    if dev:
        return L.ks_egm_solve_batch_dev(*head, p["scratch"], None)
    return L.ks_egm_solve_batch(*head)


@pytest.mark.parametrize("dev", [False, True])
def test_egm_batch_raw_refusals(pkg, dev):
    BAD_SHAPE, BAD_ARG = 1, 6
    names = ["k_opt", "k_grid", "K_grid", "B", "P", "params", "iters", "diff", "status"]
    for name in names + (["scratch"] if dev else []):
        assert _egm_raw(pkg, 2, 5, 2, null=name, dev=dev) == BAD_ARG, name
    assert _egm_raw(pkg, 0, 5, 2, dev=dev) == BAD_SHAPE
    assert _egm_raw(pkg, 65536, 5, 2, dev=dev) == BAD_SHAPE
    assert _egm_raw(pkg, 2, 2, 2, dev=dev) == BAD_SHAPE                  # k_size < 3
    # 8·(4·nk + 8·nk·nK) > 150 KiB: past the one-workgroup LDS rule
    assert _egm_raw(pkg, 2, 1000, 4, dev=dev) == BAD_SHAPE
    assert b"too large" in pkg.lib().aiy_last_error()


def _hist_args(pkg, M=4):
    I = bc.inputs(pkg)
    zi = np.tile(I["zi"], (1, M // 2))
    lam0 = pkg.ks_panel.hist_start(I["x"], 30.0, 0.04)
    return [bc.sweeps3(pkg), I["k_grid"], I["K_grid"], I["x"], zi, lam0, I["prm"]]


def test_hist_multi_refusals(pkg):
    f = pkg.ks_panel.ks_simulate_hist_multi
    a = _hist_args(pkg)
    _raises(pkg, "AIY_BAD_ARG", f, *a, [0, 1, -1, 2])
    _raises(pkg, "AIY_BAD_ARG", f, *a, [0, 1, 3, 2])                      # C = 3
    bad = list(a)
    bad[2] = a[2].copy()
    bad[2][1] = bad[2][1][::-1]
    _raises(pkg, "AIY_BAD_ARG", f, *bad, [0, 1, 2, 2])                    # candidate 1's K_grid
    bad = list(a)
    bad[6] = a[6].copy()
    bad[6][2, 6] = 1.5
    _raises(pkg, "AIY_BAD_ARG", f, *bad, [0, 1, 2, 2])                    # candidate 2's ub
    bad = list(a)
    bad[0] = a[0].copy()
    bad[0][1, 3, 1, 2] = np.nan
    _raises(pkg, "AIY_NON_FINITE", f, *bad, [0, 1, 2, 2])
    # nx past the fit rule
    bad = list(a)
    bad[3] = np.linspace(1e-4, 1000.0, 3000)
    bad[5] = np.zeros((2, 3000))
    _raises(pkg, "AIY_BAD_SHAPE", f, *bad, [0, 1, 2, 2])


def test_hist_multi_dev_refusals_before_the_device(pkg):
    """The device tier validates its host arguments first: called with dummy host pointers in
    the device slots, each refusal returns before anything dereferences them."""
    L = pkg.lib()
    I = bc.inputs(pkg)
    dummy = np.zeros(8)
    dp = dummy.ctypes.data_as(C.c_void_p)
    prm = np.ascontiguousarray(I["prm"])

    def call(C_, pol, nx=64, params=prm, null_pol=False):
        pol = np.asarray(pol, np.int32)
        return L.ks_simulate_hist_multi_dev(
            C.c_int64(C_), C.c_int64(24), C.c_int64(3), dp, dp, dp, dp, C.c_int64(nx),
            params.ctypes.data_as(C.c_void_p),
            None if null_pol else pol.ctypes.data_as(C.c_void_p), dp, C.c_int64(40),
            C.c_int64(pol.size), dp, dp, None, dp, None)

    assert call(3, [0, 1, 2], null_pol=True) == 6
    assert call(3, [0, -1, 2]) == 6
    assert call(3, [0, 3, 2]) == 6
    assert call(0, [0]) == 1
    assert call(65536, [0]) == 1
    assert call(3, [0, 1, 2], nx=3000) == 1
    bad = prm.copy()
    bad[1, 5] = 0.0
    assert call(3, [0, 1, 2], params=bad) == 6


# ------------------------------------------------------------------ Python layer
def test_python_shape_and_broadcast_errors(pkg):
    a = _egm_args(pkg)
    with pytest.raises(ValueError):
        pkg.ks_egm_solve_batch(a[0][0], *a[1:])                           # k_opt not 4-D
    with pytest.raises(ValueError):
        pkg.ks_egm_solve_batch(a[0], a[1][:-1], *a[2:])                   # k_grid length
    for q, bad in ((2, a[2][:2]), (3, np.zeros((2, 4))), (4, a[4][:2]), (5, a[5][:, :12])):
        b = list(a)
        b[q] = bad
        with pytest.raises(ValueError):
            pkg.ks_egm_solve_batch(*b)
    h = _hist_args(pkg)
    f = pkg.ks_panel.ks_simulate_hist_multi
    with pytest.raises(ValueError):
        f(*h, [0, 1, 2])                                                  # M = 4 paths
    with pytest.raises(ValueError):
        f(*h, [0.0, 1.0, 2.0, 2.0])                                       # not integers
    with pytest.raises(ValueError):
        f(h[0], h[1], h[2][:2], *h[3:], [0, 1, 2, 2])
    with pytest.raises(ValueError):
        f(h[0][0], *h[1:], [0, 0, 0, 0])


def test_broadcast_builds_candidate_major_blocks(pkg):
    I = bc.inputs(pkg)
    Kg, B, P, prm = pkg.ks.egm_batch_inputs(3, 3, I["K_grid"][0], bc.B_IDENTITY, I["P"], I["prm"][2])
    assert Kg.shape == (3, 3) and np.array_equal(Kg[2], I["K_grid"][0])
    assert B.shape == (3, 4) and prm.shape == (3, 13) and np.array_equal(prm[0], I["prm"][2])
    # each P block is handed over column-major, as ks_egm_solve passes MATLAB's 4 x 4
    assert np.array_equal(P[2].reshape(-1), np.asfortranarray(I["P"][2]).reshape(-1, order="F"))


def test_driver_argument_errors(pkg):
    kp = pkg.ks_panel
    with pytest.raises(ValueError):
        kp.krusell_smith_egm(simulate="x")
    with pytest.raises(TypeError):
        kp.krusell_smith_egm(no_such_parameter=1.0)
    for name in ("ks_egm_solve_batch", "ks_egm_solve_batch_dev", "HistSimMulti",
                 "krusell_smith_egm", "krusell_smith_egm_batch", "ks_simulate_hist_multi"):
        assert name in pkg.__all__ and hasattr(pkg, name)
