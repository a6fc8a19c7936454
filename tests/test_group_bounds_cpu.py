"""The tree kernel's group-level 8-block bound: each 8-block bound is tested once
per group of G consecutive lanes, against the group's lowest bar and its largest cash on hand,
instead of once per lane.  A numpy restatement of the kernel's operation order (screen_B,
screen_t, the fmin / fmax reductions that drop NaN): the group test has no false negatives."""
import numpy as np
import pytest

K_TAU = 2.0 ** -46
K_THR = 1.0 - 2.0 ** -48


def _screen_B(best, idx, dis, n):
    """bell_dev.hpp screen_B, operation for operation."""
    nd = float(n)
    with np.errstate(all="ignore"):
        B = nd * (best + dis) - (K_TAU * nd) * (np.abs(best) + np.abs(dis))
    return np.where(idx < 0, -np.inf, B)


def _screen_t(cx, dd, n):
    """bell_dev.hpp screen_t: t = dd · max(cx, 0)^n by square-and-multiply from the top bit."""
    with np.errstate(all="ignore"):
        c = np.fmax(cx, 0.0)
        p = c.copy()
        for b in range(n.bit_length() - 2, -1, -1):
            p = p * p
            if (n >> b) & 1:
                p = p * c
        return dd * p


@pytest.mark.parametrize("G", [4, 8, 16, 32])
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6, 7, 8])
def test_group_bound_has_no_false_negative(n, G):
    """On random (D, a0, coh, best) with NaN, ±inf and ±0 mixed in, idx < 0 lanes (bar −inf) and
    invalid sub-states (NaN bar, cash −inf in the maximum), the group-level test — (D − min B)·
    max(max coh − a0, 0)^n ≥ 1 − 2^-48 over the group's valid sub-states — is true for every
    (block, group) in which some member's own test is, and false for a group without a valid
    sub-state."""
    rng = np.random.default_rng(1000 * G + n)
    nw, LB = 600, 5                       # waves; sub-states per lane (labour groups)
    ng = 64 // G
    special = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0])

    def mix(x, frac):
        m = rng.random(x.shape) < frac
        return np.where(m, rng.choice(special, x.shape), x)

    # bars around the bounds' own scale, so that tests pass and fail in comparable numbers
    best = mix(-rng.lognormal(0.0, 2.0, (nw, 64, 1)) * np.ones((1, 1, LB)), 0.03)
    dis = rng.random((1, 1, LB)) * (LB > 1)
    idx = np.where(rng.random((nw, 64, 1)) < 0.05, -1, 7)
    valid = rng.random((nw, 64, LB)) < 0.9
    gv = valid.reshape(nw, ng, G, LB)      # (a view: edits below land in `valid`)
    gv[: nw // 4, ::2] &= rng.random((nw // 4, (ng + 1) // 2, G, 1)) < 0.1   # nearly empty groups
    gv[: nw // 8, -1] = False                                                # and wholly empty ones
    gv[:4] = False                                                           # and empty waves
    coh = mix(rng.lognormal(0.0, 1.5, (nw, 64, LB)) - 0.5, 0.02)
    B = np.where(valid, _screen_B(best, idx, dis, n), np.nan)
    nblk = 16                                                  # block bounds per wave
    with np.errstate(all="ignore"):
        D = mix(n * -rng.lognormal(0.0, 2.0, (nw, nblk)) + 1.0, 0.03)
    a0 = mix(rng.lognormal(0.0, 1.5, (nw, nblk)) - 0.5, 0.02)

    with np.errstate(all="ignore"):
        # own tests: (wave, block, lane, sub-state) -> (wave, block, group)
        t_lane = _screen_t(coh[:, None] - a0[:, :, None, None], D[:, :, None, None] - B[:, None], n)
        member_pass = (t_lane >= K_THR).reshape(nw, nblk, ng, G * LB).any(axis=3)
        bmin = np.fmin.reduce(B.reshape(nw, ng, G * LB), axis=2)
        cmax = np.fmax.reduce(np.where(valid, coh, -np.inf).reshape(nw, ng, G * LB), axis=2)
        t_grp = _screen_t(cmax[:, None, :] - a0[:, :, None], D[:, :, None] - bmin[:, None, :], n)
        group_pass = t_grp >= K_THR
    # all three categories occur: member passes, nothing passes, the group alone passes
    assert member_pass.any() and (~group_pass).any() and (group_pass & ~member_pass).any()
    empty = ~valid.reshape(nw, ng, G * LB).any(axis=2)
    assert empty.any() and (~empty).any()
    assert not (group_pass & empty[:, None, :]).any()          # every bar NaN: false
    assert not (member_pass & ~group_pass).any()
