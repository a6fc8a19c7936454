"""The identity behind the tree screen's unclamped body.  The screen
value of candidate k for a state with cash on hand coh is t = dd · max(coh − a_k, 0)^n, and the
state's feasible prefix is kf = #{k : a_k < coh} (a increasing).  In IEEE fp64 the difference of
two distinct finite doubles is never zero — gradual underflow keeps it representable — so
coh − a_k > 0 ⟺ a_k < coh, and for every k < kf the clamp max(·, 0) returns its argument bit for
bit: a block of candidates below the smallest prefix of a wave may drop it.  Past the prefix
it may not: for even n the unclamped power of a negative difference is positive."""
import numpy as np

TINY = np.float64(5e-324)  # the smallest subnormal


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def _grids():
    """(a, coh) pairs: a increasing, coh a vector of cash values to test against all of a."""
    rng = np.random.default_rng(7)
    out = []
    # an asset grid as the model's, cash at, just below and just above grid points
    a = np.linspace(0.0, 50.0, 257)
    coh = np.concatenate([a, np.nextafter(a, np.inf), np.nextafter(a, -np.inf),
                          rng.uniform(-1.0, 60.0, 300)])
    out.append((a, coh))
    # values adjacent in fp64: runs of consecutive doubles around several magnitudes
    for x0 in (1.0, 0.1, 37.5, 1e-300, 1e300, -2.0):
        run = [np.float64(x0)]
        for _ in range(40):
            run.append(np.nextafter(run[-1], np.inf))
        a = np.array(run)
        out.append((a, np.concatenate([a, [np.nextafter(a[0], -np.inf), np.nextafter(a[-1], np.inf)]])))
    # subnormal gaps: a grid of subnormals (differences are subnormal or zero only when equal)
    a = np.arange(0, 64, dtype=np.float64) * TINY
    out.append((a, np.concatenate([a, a + TINY, [np.float64(2.2250738585072014e-308)]])))
    # normal values whose difference is subnormal: neighbours just above the smallest normal
    m = np.float64(2.2250738585072014e-308)
    run = [m]
    for _ in range(30):
        run.append(np.nextafter(run[-1], np.inf))
    a = np.array(run)
    assert 0 < a[1] - a[0] < m
    out.append((a, a.copy()))
    # a grid with negative entries (a borrowing limit below zero) and negative cash
    a = np.linspace(-3.0, 5.0, 129)
    out.append((a, np.concatenate([a, rng.uniform(-4.0, 6.0, 200), [-0.0, 0.0]])))
    return out


def test_less_than_is_positive_difference():
    """a_k < coh ⟺ coh − a_k > 0, with coh == a_k (difference exactly 0), adjacent doubles and
    subnormal differences."""
    with np.errstate(over="ignore"):
        for a, coh in _grids():
            d = coh[:, None] - a[None, :]
            assert np.array_equal(a[None, :] < coh[:, None], d > 0)
            assert np.array_equal(a[None, :] == coh[:, None], d == 0)


def test_clamp_is_identity_below_the_feasible_prefix():
    """For k < kf = #{k : a_k < coh}: max(coh − a_k, 0) == coh − a_k bit for bit (and the
    difference is never −0.0, whose clamp would be +0.0)."""
    n_checked = 0
    with np.errstate(over="ignore"):
        for a, coh in _grids():
            assert (np.diff(a) > 0).all()
            kf = (a[None, :] < coh[:, None]).sum(axis=1)
            d = coh[:, None] - a[None, :]
            below = np.arange(a.size)[None, :] < kf[:, None]
            assert np.array_equal(_bits(np.maximum(d, 0.0))[below], _bits(d)[below])
            assert (d[below] > 0).all()
            n_checked += int(below.sum())
            # on and past the prefix edge the difference is <= 0: the clamp is not an identity
            # there (it gives +0.0), except where the difference is exactly +0.0
            assert (d[~below] <= 0).all()
    assert n_checked > 10_000


def test_unclamped_differs_past_the_prefix_for_even_n():
    """For k >= kf and even n the clamped t is dd · 0 = 0 and the unclamped one dd · (negative)^n
    > 0: the unclamped body would pass infeasible candidates, so the clamped body must remain
    for every block that reaches the smallest prefix of its wave."""
    a = np.linspace(0.0, 50.0, 257)
    coh, dd = np.float64(10.0), np.float64(3.0)
    kf = int((a < coh).sum())
    cx = coh - a
    for n in (2, 4):
        t_clamped = dd * np.maximum(cx, 0.0) ** n
        t_plain = dd * cx ** n
        assert np.array_equal(_bits(t_clamped[:kf]), _bits(t_plain[:kf]))
        past = np.arange(a.size) >= kf
        strictly = past & (cx < 0)
        assert strictly.any()
        assert (t_clamped[past] == 0).all() and (t_plain[strictly] > 0).all()
        assert (t_plain[strictly] >= 0.99999999999999644729).any()  # would pass the screen
    for n in (1, 3):  # odd n: the sign survives, but the values still differ (0 against < 0)
        t_clamped = dd * np.maximum(cx, 0.0) ** n
        t_plain = dd * cx ** n
        assert (t_plain[cx < 0] < 0).all() and (t_clamped[cx < 0] == 0).all()
