"""The tree kernel's word walk, restated in numpy
(tools/emu_fine_groups.py --walks): the trips of the walk as the kernel runs it — every group's
mask one 32-bit word per window of 32 blocks, the windows counted from the lowest passing block
left — against a brute-force count, and the range walk's emulation (measured there, not built)
on a hand-made tile.  The padded candidate rows of the same round were measured and deleted, so
there is no index map to restate."""
import importlib.util
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module")
def emu():
    spec = importlib.util.spec_from_file_location("emu_fine_groups",
                                                  ROOT / "tools" / "emu_fine_groups.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _random_tile(rng, q):
    """own[block, lane] of one tile: a drifting window per lane (the kernel's usual shape), plus
    scattered far blocks in every third tile and a dense cold tile now and then."""
    nb = int(rng.integers(1, 200))
    nl = int(rng.choice([1, 9, 63, 64]))
    own = np.zeros((nb, nl), dtype=bool)
    if q % 5 == 4:
        return rng.random((nb, nl)) < 0.9
    c0, wid = rng.integers(0, nb), rng.integers(1, 40)
    for lane in range(nl):
        lo = int(c0 + lane // 8 + rng.integers(-2, 3))
        own[max(lo, 0):max(lo + int(wid), 0), lane] = True
    if q % 3 == 0:
        own |= rng.random((nb, nl)) < 0.02
    return own


def test_word_walk_trips_match_a_brute_force_count(emu):
    """Brute force: the union's blocks of a superblock cut into windows — from the lowest block
    left, 32 blocks wide — and per window the largest number of blocks any group passes there.
    With one window that is the mask walk's count (the busiest group's blocks); the emulated
    walk visits, per group, exactly its own blocks in ascending order either way."""
    rng = np.random.default_rng(16)
    n1 = n2 = 0
    for q in range(20):
        own = _random_tile(rng, q)
        trips, nsb, none, visited = emu.walk_words(own)
        brute, sbs, single = 0, 0, 0
        for b0 in range(0, own.shape[0], 64):
            blk = own[b0:b0 + 64]
            per_group = [np.flatnonzero(blk[:, g:g + 8].any(axis=1)).tolist()
                         for g in range(0, own.shape[1], 8)]
            if not any(per_group):
                continue
            assert visited[sbs] == per_group, (q, b0)
            left, nwin = sorted(set().union(*per_group)), 0
            while left:
                lo = left[0]
                brute += max(sum(lo <= u < lo + 32 for u in grp) for grp in per_group)
                left = [u for u in left if u >= lo + 32]
                nwin += 1
            single += nwin == 1
            sbs += 1
        assert trips == brute, q
        assert (nsb, none) == (sbs, single)
        if single == sbs:
            assert trips == emu.group_trips(own, 8), q
        else:
            assert trips >= emu.group_trips(own, 8), q
        n1 += single
        n2 += sbs - single
    assert n1 > 0 and n2 > 0, "one-window and two-window superblocks both occurred"


def test_range_walk_counts(emu):
    """The range walk's emulation (the walk itself is not built: DESIGN.md §5, round 12) on a
    hand-made tile: group 0 passes block 3, and 70 and 72 with a hole at 71; group 1 passes
    blocks 10 and 30, nineteen holes, eight of them in the 64-block 16 … 23 that nothing staged."""
    own = np.zeros((80, 16), dtype=bool)
    own[[3, 70, 72], 0] = True
    own[[10, 30], 9] = True
    trips, holes, unstaged = emu.range_walk(own)
    # superblock 0: group 0 range 3..3, group 1 range 10..30 (21 trips); superblock 1: 6..8 (3)
    assert trips == 21 + 3
    assert holes == 19 + 1
    # staged 64-blocks of superblock 0: blocks 0-7, 8-15, 24-31; holes 16..23 are unstaged
    assert unstaged == 8
