"""The tree kernel's per-group fine-screen walk, restated in numpy.

`prep` leaves every lane the OR of the own pass masks of its group of G consecutive lanes (bit u:
some lane of the group passes 8-block u of the superblock).  `finish` walks in trips: in a trip
every lane whose group mask still has a bit takes the lowest one, screens that block's eight
candidates and clears the bit; a lane whose group has run out reads the wave's highest passing
block (staged by construction) with its votes masked.  The walk ends when no lane has a bit
left.  Checked on random masks, with empty groups, all-equal groups and full masks:

  * every lane sees each block of its group's mask — hence each of its own passing blocks —
    exactly once, in ascending order;
  * no lane votes on a block outside its group's mask, and every read is of a staged block;
  * the trip count is the largest group popcount."""
import numpy as np
import pytest

FULL = (1 << 64) - 1


def group_masks(own, G):
    """own[64] (python ints, one 64-bit mask per lane) -> the lanes' group masks."""
    gm = []
    for g0 in range(0, 64, G):
        m = 0
        for x in own[g0:g0 + G]:
            m |= x
        gm += [m] * G
    return gm


def walk(gm):
    """The kernel's walk: a list of trips, each (block per lane, active per lane)."""
    union = 0
    for m in gm:
        union |= m
    if union == 0:
        return []                               # (finish is not entered with an empty pass mask)
    hb = union.bit_length() - 1                 # the highest staged block
    gm = list(gm)
    trips = []
    while any(gm):
        act = [m != 0 for m in gm]
        blk = [(m & -m).bit_length() - 1 if m else hb for m in gm]
        gm = [m & (m - 1) if m else 0 for m in gm]
        trips.append((blk, act))
    return trips


def check(own, G):
    gm = group_masks(own, G)
    union = 0
    for m in own:
        union |= m
    trips = walk(gm)
    assert len(trips) == max(bin(m).count("1") for m in gm)
    for lane in range(64):
        seen = [blk[lane] for blk, act in trips if act[lane]]
        assert seen == sorted(set(seen)), "ascending, each block once"
        assert seen == [u for u in range(64) if (gm[lane] >> u) & 1]
        assert all((own[lane] >> u) & 1 == 0 or u in seen for u in range(64))
        for blk, act in trips:
            assert (union >> blk[lane]) & 1, "a read of a block that was not staged"
    # groups' lanes move together: one LDS address per group and trip
    for blk, act in trips:
        for g0 in range(0, 64, G):
            assert len(set(blk[g0:g0 + G])) == 1 and len(set(act[g0:g0 + G])) == 1


def _rand_masks(rng, density):
    bits = rng.random((64, 64)) < density
    return [sum(1 << int(u) for u in np.flatnonzero(row)) for row in bits]  # (python ints)


@pytest.mark.parametrize("G", [8, 16, 32, 64])
def test_random_masks(G):
    rng = np.random.default_rng(15)
    for density in (0.02, 0.2, 0.7):
        for _ in range(20):
            check(_rand_masks(rng, density), G)


@pytest.mark.parametrize("G", [8, 16, 32, 64])
def test_empty_groups_beside_busy_ones(G):
    rng = np.random.default_rng(16)
    for _ in range(20):
        own = _rand_masks(rng, 0.3)
        for g0 in range(0, 64, G):
            if rng.random() < 0.5:
                own[g0:g0 + G] = [0] * G        # (a group past Na: NaN bars, no pass at all)
        own[63] |= 1 << int(rng.integers(64))   # at least one pass: finish is entered
        check(own, G)
    check([0] * 63 + [1 << 63], G)              # one lane, the last block
    check([1] + [0] * 63, G)                    # one lane, the first block


@pytest.mark.parametrize("G", [8, 16, 32, 64])
def test_all_equal_and_full(G):
    check([0x00ff00ff00ff00ff] * 64, G)
    check([FULL] * 64, G)
    check([FULL] * 8 + [0] * 56, G)
    # drifting optima: lane l passes blocks l/4 .. l/4 + 10 (the headline's shape)
    check([((1 << 11) - 1) << (l // 4) for l in range(64)], G)


def test_empty_pass_mask_makes_no_trip():
    assert walk([0] * 64) == []
