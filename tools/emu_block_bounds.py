"""CPU emulation of the tree kernel's 8-block bound at different sharing widths (DESIGN.md §5,
"group-level bound"): how many 8-blocks of a tile pass when the bound is tested per lane, per
group of G consecutive lanes (the group's lowest bar, its largest cash on hand) or per wave.

    python tools/emu_block_bounds.py [--na 20000] [--sweeps 10 15 25] [--groups 64 32 16 8 4]

C-oracle sweeps from v = 0 at the benchmark's calibration (r = 0.04, Rouwenhorst shocks); sweep q
is the q-th sweep (its input is v after q − 1 sweeps).  The bar of a state is
its optimum of that sweep (the bar the kernel holds once its start-up has climbed to the
argmax); the test is (Dm8 − B)·max(coh − a8, 0)^n ≥ 1 − 2^-48 in the kernel's operation order,
over every 8-block inside the tile's feasible range.  Prints, per sweep, the mean over the
tiles of: the per-lane pass count (own), the union over the tile's 64 lanes, and the count of
each group size (a block counts when any group of the tile passes it).  No GPU is used."""
import argparse
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from oracle import corc  # noqa: E402
from oracle import np_oracle as no  # noqa: E402

K_TAU = 2.0 ** -46
K_THR = 1.0 - 2.0 ** -48


def screen_t(cx, dd, n):
    """bell_dev.hpp screen_t: dd · max(cx, 0)^n by square-and-multiply from the top bit."""
    c = np.fmax(cx, 0.0)
    p = c.copy()
    for b in range(n.bit_length() - 2, -1, -1):
        p = p * p
        if (n >> b) & 1:
            p = p * c
    return dd * p


def tile_counts(V, vopt, a, s, P, r, w, beta, n, groups):
    """Per tile (row-major, 64 states each): own mean, union, and one count per group size."""
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
            kg = int(kf[sl].max())
            nfe = (kg + 7) // 8
            if nfe == 0:
                rows.append([0.0, 0.0] + [0.0] * len(groups))
                continue
            d, a0 = Dm8[i, :nfe], a8[:nfe]
            own = screen_t(coh[sl][None, :] - a0[:, None], d[:, None] - B[i, sl][None, :], n) >= K_THR
            rec = [own.sum(axis=0).mean(), float(own.any(axis=1).sum())]
            for G in groups:
                nl = sl.stop - sl.start
                ok = np.zeros(nfe, bool)
                for g0 in range(0, nl, G):
                    bmin = np.fmin.reduce(B[i, sl][g0:g0 + G])
                    cmax = np.fmax.reduce(coh[sl][g0:g0 + G])
                    ok |= screen_t(cmax - a0, d - bmin, n) >= K_THR
                rec.append(float(ok.sum()))
            rows.append(rec)
    return np.array(rows)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--na", type=int, default=20000)
    ap.add_argument("--sweeps", type=int, nargs="+", default=[10, 15, 25])
    ap.add_argument("--groups", type=int, nargs="+", default=[64, 32, 16, 8, 4])
    ap.add_argument("--r", type=float, default=0.04)
    args = ap.parse_args()
    cal = no.calib_aiyagari(Na=args.na, shocks="rouwenhorst")
    a, s, P, beta, sigma = cal["a_grid"], cal["s"], cal["P"], cal["beta"], cal["sigma"]
    n = int(sigma) - 1
    w = no.wage(args.r, cal["alpha"], cal["delta"])
    V = np.zeros((len(s), args.na))
    print("sweep  tiles  own    union  " + "  ".join(f"G={g:<3d}" for g in args.groups), flush=True)
    with np.errstate(all="ignore"):
        for q in range(1, max(args.sweeps) + 1):
            vn = corc.vfi_sweep(V, a, s, P, args.r, w, beta, sigma)[0]
            if q in args.sweeps:
                T = tile_counts(V, vn, a, s, P, args.r, w, beta, n, args.groups)
                print(f"{q:5d}  {len(T):5d}  " + "  ".join(f"{x:5.1f}" for x in T.mean(axis=0)),
                      flush=True)
            V = vn


if __name__ == "__main__":
    main()
