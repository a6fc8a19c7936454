"""CPU emulation of the tree kernel's fine-screen walk at different sharing widths (DESIGN.md §5,
round 11): how many 8-block trips a wave makes per tile when every group of G consecutive lanes
walks the union of its own lanes' passing 8-blocks and the groups advance in lockstep.

    python tools/emu_fine_groups.py [--na 20000] [--sweeps 6 15 25] [--groups 64 32 16 8]
                                    [--walks]

The set-up is tools/emu_block_bounds.py's (C-oracle sweeps from v = 0 at the benchmark's
calibration, the bar of a state its optimum of that sweep, the per-lane 8-block test in the
kernel's operation order).  A wave stages one superblock (64 8-blocks) at a time, so the trips
of a tile are counted per superblock — the largest group's count of passing blocks there — and
summed; G = 64 is the wave's union, what the kernel walked before.  Prints, per sweep, the mean
over the tiles of: the per-lane pass count (own) and the trips of each group size.  No GPU is
used.

--walks (round 12) adds, for G = 8: the trips of the kernel's word walk (walk_words: the bit walk
as the kernel does it, in 32-bit windows counted from the lowest passing block left — one window,
and then the mask walk's trips exactly, when the union spans fewer than 32 blocks; the sum of the
windows' busiest groups otherwise) with the share of superblocks walked in one window, and the
trips of a range walk (range_walk: every group counts through lo..hi of its mask)
with its holes — blocks inside a group's range that the group's own lanes rejected — and how
many of those lie in a 64-block the wave's union did not stage."""
import argparse
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
from emu_block_bounds import K_TAU, K_THR, corc, no, screen_t  # noqa: E402


def group_trips(own, G):
    """own[block, lane] (bool) of one tile -> trips: per superblock of 64 blocks the largest
    number of blocks any group of G consecutive lanes passes, summed over the superblocks."""
    nb, nl = own.shape
    trips = 0
    for b0 in range(0, nb, 64):
        blk = own[b0:b0 + 64]
        trips += max(int(blk[:, g0:g0 + G].any(axis=1).sum()) for g0 in range(0, nl, G))
    return trips


def walk_words(own, G=8):
    """The kernel's walk of one tile, run word by word -> (trips, superblocks, superblocks walked
    in one window, blocks visited per group as a list of lists per superblock)."""
    nb, nl = own.shape
    trips = nsb = none = 0
    visited = []
    for b0 in range(0, nb, 64):
        blk = own[b0:b0 + 64]
        masks = [sum(1 << int(u) for u in np.flatnonzero(blk[:, g0:g0 + G].any(axis=1)))
                 for g0 in range(0, nl, G)]
        pw = 0
        for m in masks:
            pw |= m
        if not pw:
            continue
        nsb += 1
        seen, nwin = [[] for _ in masks], 0
        while pw:
            nwin += 1
            lb = (pw & -pw).bit_length() - 1                         # ctz
            hw = ((pw >> lb) & 0xffffffff).bit_length() - 1          # 31 - clz of the window
            g = [(m >> lb) & 0xffffffff for m in masks]
            pw = 0 if lb >= 32 else pw & ~((1 << (lb + 32)) - 1)
            while any(g):
                trips += 1
                for q, m in enumerate(g):
                    if m:
                        seen[q].append(lb + min((m & -m).bit_length() - 1, hw))   # ffbl, min
                    g[q] = m & (m - 1)
        none += nwin == 1
        visited.append(seen)
    return trips, nsb, none, visited


def range_walk(own, G=8):
    """Range walk of one tile: per superblock every group counts through lo..hi of its mask ->
    (trips, holes, holes in a 64-block without a passing block of the wave's union)."""
    nb, nl = own.shape
    trips = holes = unstaged = 0
    for b0 in range(0, nb, 64):
        blk = own[b0:b0 + 64]
        staged = np.repeat(_pad8(blk.any(axis=1)).reshape(-1, 8).any(axis=1), 8)
        longest = 0
        for g0 in range(0, nl, G):
            m = blk[:, g0:g0 + G].any(axis=1)
            u = np.flatnonzero(m)
            if not len(u):
                continue
            lo, hi = int(u[0]), int(u[-1])
            longest = max(longest, hi - lo + 1)
            hole = ~m[lo:hi + 1]
            holes += int(hole.sum())
            unstaged += int((hole & ~staged[lo:hi + 1]).sum())
        trips += longest
    return trips, holes, unstaged


def _pad8(x):
    return np.concatenate([x, np.zeros(-len(x) % 8, dtype=bool)])


def tile_trips(V, vopt, a, s, P, r, w, beta, n, groups, walks=False):
    """Per tile (row-major, 64 states each): own mean, then the trips of each group size; with
    walks also (word-walk trips, superblocks, one-window superblocks, range-walk trips, holes,
    unstaged holes) of G = 8."""
    N, Na = V.shape
    EV = no.ev_rows(P, V, beta)
    ne = n * EV
    D = (ne + 1.0) + K_TAU * (np.abs(ne) + 1.0)                 # table_D
    nb8 = (Na + 7) // 8
    Dp = np.full((N, nb8 * 8), -np.inf)
    Dp[:, :Na] = D
    Dm8 = Dp.reshape(N, nb8, 8).max(axis=2)
    a8 = a[::8]
    B = n * vopt - (K_TAU * n) * np.abs(vopt)                   # screen_B with dis = 0
    rows = []
    for i in range(N):
        coh = (1 + r) * a + w * s[i]
        kf = np.searchsorted(a, coh, side="left")               # candidates with coh - a_k > 0
        for j0 in range(0, Na, 64):
            sl = slice(j0, min(j0 + 64, Na))
            nfe = (int(kf[sl].max()) + 7) // 8
            if nfe == 0:
                rows.append([0.0] * (1 + len(groups) + (6 if walks else 0)))
                continue
            d, a0 = Dm8[i, :nfe], a8[:nfe]
            own = screen_t(coh[sl][None, :] - a0[:, None], d[:, None] - B[i, sl][None, :], n) >= K_THR
            row = [own.sum(axis=0).mean()] + [float(group_trips(own, G)) for G in groups]
            if walks:
                row += [float(x) for x in walk_words(own)[:3]] + [float(x) for x in range_walk(own)]
            rows.append(row)
    return np.array(rows)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--na", type=int, default=20000)
    ap.add_argument("--sweeps", type=int, nargs="+", default=[6, 10, 15, 25])
    ap.add_argument("--groups", type=int, nargs="+", default=[64, 32, 16, 8])
    ap.add_argument("--r", type=float, default=0.04)
    ap.add_argument("--walks", action="store_true",
                    help="also the word walk and the range walk of G = 8 (round 12)")
    args = ap.parse_args()
    cal = no.calib_aiyagari(Na=args.na, shocks="rouwenhorst")
    a, s, P, beta, sigma = cal["a_grid"], cal["s"], cal["P"], cal["beta"], cal["sigma"]
    n = int(sigma) - 1
    w = no.wage(args.r, cal["alpha"], cal["delta"])
    V = np.zeros((len(s), args.na))
    print("trips per tile, counted per superblock (G = 64: the wave's union)")
    print("sweep  tiles  own    " + "  ".join(f"G={g:<3d}" for g in args.groups) +
          ("  | word walk: trips, one-window share of superblocks | range walk: trips, holes,"
           " unstaged holes (per tile)" if args.walks else ""), flush=True)
    with np.errstate(all="ignore"):
        for q in range(1, max(args.sweeps) + 1):
            vn = corc.vfi_sweep(V, a, s, P, args.r, w, beta, sigma)[0]
            if q in args.sweeps:
                T = tile_trips(V, vn, a, s, P, args.r, w, beta, n, args.groups, args.walks)
                m, ng = T.mean(axis=0), 1 + len(args.groups)
                line = f"{q:5d}  {len(T):5d}  " + "  ".join(f"{x:5.1f}" for x in m[:ng])
                if args.walks:
                    ww, nsb, nnar, rt, ho, un = T[:, ng:].sum(axis=0)
                    line += (f"  | {ww / len(T):5.1f}, {nnar / max(nsb, 1):6.4f} | {rt / len(T):5.1f},"
                             f" {ho / len(T):5.2f}, {un / len(T):6.4f} ({int(un)} in all)")
                print(line, flush=True)
            V = vn


if __name__ == "__main__":
    main()
