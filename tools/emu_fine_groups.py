"""CPU emulation of the tree kernel's fine-screen walk at different sharing widths (DESIGN.md §5,
round 11): how many 8-block trips a wave makes per tile when every group of G consecutive lanes
walks the union of its own lanes' passing 8-blocks and the groups advance in lockstep.

    python tools/emu_fine_groups.py [--na 20000] [--sweeps 6 15 25] [--groups 64 32 16 8]

The set-up is tools/emu_block_bounds.py's (C-oracle sweeps from v = 0 at the benchmark's
calibration, the bar of a state its optimum of that sweep, the per-lane 8-block test in the
kernel's operation order).  A wave stages one superblock (64 8-blocks) at a time, so the trips
of a tile are counted per superblock — the largest group's count of passing blocks there — and
summed; G = 64 is the wave's union, what the kernel walked before.  Prints, per sweep, the mean
over the tiles of: the per-lane pass count (own) and the trips of each group size.  No GPU is
used."""
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


def tile_trips(V, vopt, a, s, P, r, w, beta, n, groups):
    """Per tile (row-major, 64 states each): own mean, then the trips of each group size."""
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
                rows.append([0.0] * (1 + len(groups)))
                continue
            d, a0 = Dm8[i, :nfe], a8[:nfe]
            own = screen_t(coh[sl][None, :] - a0[:, None], d[:, None] - B[i, sl][None, :], n) >= K_THR
            rows.append([own.sum(axis=0).mean()] + [float(group_trips(own, G)) for G in groups])
    return np.array(rows)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--na", type=int, default=20000)
    ap.add_argument("--sweeps", type=int, nargs="+", default=[6, 10, 15, 25])
    ap.add_argument("--groups", type=int, nargs="+", default=[64, 32, 16, 8])
    ap.add_argument("--r", type=float, default=0.04)
    args = ap.parse_args()
    cal = no.calib_aiyagari(Na=args.na, shocks="rouwenhorst")
    a, s, P, beta, sigma = cal["a_grid"], cal["s"], cal["P"], cal["beta"], cal["sigma"]
    n = int(sigma) - 1
    w = no.wage(args.r, cal["alpha"], cal["delta"])
    V = np.zeros((len(s), args.na))
    print("trips per tile, counted per superblock (G = 64: the wave's union)")
    print("sweep  tiles  own    " + "  ".join(f"G={g:<3d}" for g in args.groups), flush=True)
    with np.errstate(all="ignore"):
        for q in range(1, max(args.sweeps) + 1):
            vn = corc.vfi_sweep(V, a, s, P, args.r, w, beta, sigma)[0]
            if q in args.sweeps:
                T = tile_trips(V, vn, a, s, P, args.r, w, beta, n, args.groups)
                print(f"{q:5d}  {len(T):5d}  " + "  ".join(f"{x:5.1f}" for x in T.mean(axis=0)),
                      flush=True)
            V = vn


if __name__ == "__main__":
    main()
