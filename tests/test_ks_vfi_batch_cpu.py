"""No GPU: the inputs of the batched Krusell-Smith VFI tests do what the GPU comparisons rely on
(asserted with the C oracle and a numpy restatement of the forecast index), every refusal of
ks_vfi_solve_batch[_dev] that sits in front of the device comes back with its status and its
aiy_last_error() text, and the Python layer's shape errors."""
import ctypes as C

import numpy as np
import pytest

from tests import ks_vfi_batch_cases as vc

BAD_SHAPE, NON_FINITE, BAD_ARG = 1, 2, 6


# ------------------------------------------------------------------ the inputs' conditions
def test_oracle_iteration_counts_differ_per_B(pkg):
    """k = 24, K = 3, howard 50, tol 1e-6 from the script's start: the three economies stop at
    different iterations under each B, so one launch holds workgroups that leave at different
    times."""
    got = {B: [vc.oracle_cold(pkg, e, B)["iters"] for e in range(3)]
           for B in (vc.B_IDENTITY, vc.B_SHIFT)}
    assert got[vc.B_IDENTITY] == [43, 28, 41]
    assert got[vc.B_SHIFT] == [44, 30, 36]
    for counts in got.values():
        assert len(set(counts)) == 3
    for B in got:
        for e in range(3):
            R = vc.oracle_cold(pkg, e, B)
            assert R["rel_diff"] < 1e-6 and np.all(np.isfinite(R["value"]))


def test_B_shift_moves_the_forecast_index_in_both_states(pkg):
    """B_SHIFT changes the nearest-K index against the identity ALM in the good and in the bad
    aggregate state on K in [30, 50] (E0, E2) and on [15, 35] (E1); ks_egm_batch_cases.B_OTHER
    changes none, which is why these tests do not use it."""
    I = vc.inputs(pkg)
    from tests import ks_egm_batch_cases as bc
    for e in range(3):
        ident = vc.forecast_index(I["K_grid"][e], vc.B_IDENTITY)
        assert np.array_equal(ident, np.tile(np.arange(vc.KK_SIZE), (2, 1)))
        shift = vc.forecast_index(I["K_grid"][e], vc.B_SHIFT)
        for z in (0, 1):
            assert not np.array_equal(shift[z], ident[z]), (e, z)
        assert np.array_equal(vc.forecast_index(I["K_grid"][e], bc.B_OTHER), ident)


def test_starts_differ_per_economy(pkg):
    I = vc.inputs(pkg)
    assert I["V0"].shape == (3, vc.K_SIZE, vc.KK_SIZE, 4) and np.all(np.isfinite(I["V0"]))
    assert not np.array_equal(I["V0"][0], I["V0"][1])        # beta enters V0
    assert np.array_equal(I["V0"][0], I["V0"][2])


# ------------------------------------------------------------------ refusals, no device
def _raw(pkg, C_=2, nk=5, nK=2, null=None, dev=False, max_vfi=5, howard=2, edit=None):
    """ks_vfi_solve_batch[_dev] on small valid arrays, argument `null` passed as NULL; `edit`
    changes the arrays first.  Returns (status, message)."""
    L = pkg.lib()
    n = max(C_, 1)
    small = nk * nK * 4 * n <= 10 ** 6
    arrs = dict(value=np.zeros(nk * nK * 4 * n if small else 8),
                k_opt=np.ones(nk * nK * 4 * n if small else 8),
                k_grid=np.arange(1.0, nk + 1.0) if nk < 10 ** 6 else np.ones(8),
                K_grid=np.tile(np.linspace(30.0, 50.0, nK), n) if nK < 10 ** 6 else np.ones(8),
                B=np.tile([0.0, 1.0, 0.0, 1.0], n), P=np.full(16 * n, 0.25),
                params=np.tile(pkg.ks_params(), n), iters=np.zeros(n, np.int64),
                rel_diff=np.zeros(n), scratch=np.zeros(8))
    if edit:
        edit(arrs)
    p = {k: (None if k == null else v.ctypes.data_as(C.c_void_p)) for k, v in arrs.items()}
    head = (C.c_int64(C_), p["value"], p["k_opt"], p["k_grid"], p["K_grid"], p["B"], p["P"],
            p["params"], C.c_int64(nk), C.c_int64(nK), C.c_int64(howard), C.c_double(1e-6),
            C.c_int64(max_vfi), p["iters"], p["rel_diff"])
    rc = (L.ks_vfi_solve_batch_dev(*head, p["scratch"], None) if dev
          else L.ks_vfi_solve_batch(*head))
    return rc, L.aiy_last_error().decode()


@pytest.mark.parametrize("dev", [False, True])
def test_raw_refusals(pkg, dev):
    names = ["value", "k_opt", "k_grid", "K_grid", "B", "P", "params", "iters", "rel_diff"]
    for name in names + (["scratch"] if dev else []):
        assert _raw(pkg, null=name, dev=dev) == (BAD_ARG, "NULL argument"), name
    for C_ in (0, 65536, -1):
        assert _raw(pkg, C_=C_, dev=dev) == (BAD_SHAPE, "need 1 <= C <= 65,535 candidates")
    assert _raw(pkg, nk=2, dev=dev) == (BAD_SHAPE, "need k_size >= 3 and K_size >= 1")
    assert _raw(pkg, nK=0, dev=dev) == (BAD_SHAPE, "need k_size >= 3 and K_size >= 1")
    for mv in (0, 2 ** 31):
        rc, msg = _raw(pkg, max_vfi=mv, dev=dev)
        assert rc == BAD_ARG and msg.startswith("max_vfi in [1, 2^31)")
    assert _raw(pkg, howard=-1, dev=dev)[0] == BAD_ARG
    # past ks_fused_fits (4,096 nodes): no tiled batch
    for nk, nK in ((257, 4), (100, 11), (2 ** 20, 4), (5, 2 ** 40)):
        rc, msg = _raw(pkg, nk=nk, nK=nK, dev=dev)
        assert rc == BAD_SHAPE and "too large" in msg and "no tiled" in msg, (nk, nK)
    # the order: the candidate count is tested before the sizes, the sizes before max_vfi
    assert _raw(pkg, C_=0, nk=2, dev=dev)[1] == "need 1 <= C <= 65,535 candidates"
    assert _raw(pkg, nk=2, max_vfi=0, dev=dev)[0] == BAD_SHAPE


def test_host_tier_content_refusals(pkg):
    def repeat(a):
        a["k_grid"][3] = a["k_grid"][2]
    rc, msg = _raw(pkg, edit=repeat)
    assert (rc, msg) == (BAD_ARG, "grid must be strictly increasing (point 4 repeats point 3)")

    def down(a):
        a["k_grid"][3] = 0.5
    assert _raw(pkg, edit=down)[0] == BAD_ARG
    n1 = 5 * 2 * 4
    for c, q, v in ((0, 0, np.inf), (1, 7, -np.inf), (2, n1 - 1, np.inf)):
        def inf(a, c=c, q=q, v=v):
            a["value"][c * n1 + q] = v
        rc, msg = _raw(pkg, C_=3, edit=inf)
        assert rc == NON_FINITE
        assert msg == (f"value({q + 1}) of candidate {c + 1} is infinite "
                       f"(finite or NaN entries only)")

    # the grid is tested before the values
    def both(a):
        repeat(a)
        a["value"][0] = np.inf
    assert _raw(pkg, edit=both)[0] == BAD_ARG


def test_scratch_bytes(pkg):
    L = pkg.lib()
    L.ks_vfi_batch_scratch_bytes.restype = C.c_int64
    f = lambda c, k: int(L.ks_vfi_batch_scratch_bytes(C.c_int64(c), C.c_int64(k)))  # noqa: E731
    assert f(0, 4) == 0 and f(3, 0) == 0
    one = f(1, 4)
    assert one >= 19 * 8 + 16 * 36 and f(7, 4) == 7 * one and f(1, 8) > one


# ------------------------------------------------------------------ Python layer
def _args(pkg, C_=3):
    I = vc.inputs(pkg)
    k0 = np.broadcast_to(I["k0"], (C_,) + I["k0"].shape)
    return [I["V0"][:C_], k0, I["k_grid"], I["K_grid"][:C_], vc.B_IDENTITY, I["P"][:C_],
            I["prm"][:C_]]


def test_python_shape_errors(pkg):
    a = _args(pkg)
    with pytest.raises(ValueError):
        pkg.ks_vfi_solve_batch(a[0][0], *a[1:])                          # value not 4-D
    with pytest.raises(ValueError):
        pkg.ks_vfi_solve_batch(a[0], a[1][:2], *a[2:])                   # k_opt another C
    with pytest.raises(ValueError):
        pkg.ks_vfi_solve_batch(a[0], a[1], a[2][:-1], *a[3:])            # k_grid length
    with pytest.raises(ValueError):
        pkg.ks_vfi_solve_batch(a[0][..., :3], a[1][..., :3], *a[2:])     # S = 3
    for q, bad in ((3, a[3][:2]), (4, np.zeros((2, 4))), (5, a[5][:2]), (6, a[6][:, :12])):
        b = list(a)
        b[q] = bad
        with pytest.raises(ValueError):
            pkg.ks_vfi_solve_batch(*b)


def test_python_refusals_carry_the_status(pkg):
    a = _args(pkg)
    bad = list(a)
    bad[0] = a[0].copy()
    bad[0][1, 3, 1, 2] = np.inf
    with pytest.raises(pkg.AiyError) as e:
        pkg.ks_vfi_solve_batch(*bad)
    assert e.value.status == "AIY_NON_FINITE" and "candidate 2" in str(e.value)
    with pytest.raises(pkg.AiyError) as e:
        pkg.ks_vfi_solve_batch(*a, max_vfi=0)
    assert e.value.status == "AIY_BAD_ARG"
    I = vc.inputs(pkg, 257, 4)
    with pytest.raises(pkg.AiyError) as e:
        pkg.ks_vfi_solve_batch(I["V0"], np.stack([I["k0"]] * 3), I["k_grid"], I["K_grid"],
                               vc.B_IDENTITY, I["P"], I["prm"])
    assert e.value.status == "AIY_BAD_SHAPE"


def test_driver_arguments_and_exports(pkg):
    kp = pkg.ks_panel
    with pytest.raises(TypeError):
        kp.krusell_smith_vfi(no_such_parameter=1.0)
    with pytest.raises(ValueError):
        kp.krusell_smith_vfi(simulate="x", beta=0.98)
    with pytest.raises(ValueError):
        kp.krusell_smith_vfi_batch([])
    for name in ("ks_vfi_solve_batch", "ks_vfi_solve_batch_dev", "krusell_smith_vfi",
                 "krusell_smith_vfi_batch"):
        assert name in pkg.__all__ and hasattr(pkg, name)
    assert "ks_vfi_solve_batch" in pkg.declared_symbols()
    assert "ks_vfi_solve_batch_dev" in pkg.declared_symbols()
    assert "ks_vfi_batch_scratch_bytes" in pkg.declared_symbols()


def test_economy_helper_defaults_are_the_script(pkg):
    """krusell_smith_vfi with no economy keywords stages what it staged before it took them."""
    kp = pkg.ks_panel
    prm, kg, Kg, P, V0 = kp._economy(24, 3, {})
    assert np.array_equal(prm, pkg.ks_params())
    kg0, Kg0, P0, V00 = pkg.calibration.krusell_smith(k_size=24, K_size=3)
    for a, b in ((kg, kg0), (Kg, Kg0), (P, P0), (V0, V00)):
        assert np.array_equal(a, b)


# ------------------------------------------------------------------ the driver cases
def test_driver_cases_exercise_the_warm_start_and_an_early_leave(pkg):
    """The two ALM cases of test_ks_vfi_driver_gpu.py from the oracles alone.  k = 20, K = 12,
    damping 0.5: the warm solves of rounds 2-4 run different iteration counts per economy, K_ts
    is finite and positive and no period takes the histogram's slow path.  k = 24, K = 8,
    undamped, tol_B = 2e-4: economy 1 alone converges at round 4."""
    R = vc.oracle_rounds(pkg, 20, 12, 4, 0.5)
    assert [r["iters"] for r in R] == [[39, 1, 10, 2], [30, 1, 1, 2], [42, 1, 9, 9]]
    for r in R:
        assert all(np.all(np.isfinite(K)) and np.all(K > 0) for K in r["K_ts"])
        assert not any(np.any(s) for s in r["slow"])
    R = vc.oracle_rounds(pkg, 24, 8, 5, 1.0, tol_B=2e-4)
    d4 = [r["diff_B"][3] for r in R]
    assert d4[1] < 2e-4 < min(d4[0], d4[2])
    assert [len(r["B_history"]) for r in R] == [5, 4, 5]
    assert min(r["diff_B"][-1] for r in (R[0], R[2])) > 2e-4


def test_reference_size_counts(pkg):
    got = [vc.oracle_cold(pkg, e, vc.B_IDENTITY, 50, 1e-6, 200, 100, 4)["iters"] for e in range(3)]
    assert got == [44, 40, 45]
