"""Timing record of the batched Krusell-Smith VFI solve and the lockstep ALM driver (one MI355X).

    python tools/ks_vfi_batch_ab.py [--out profiles/ks_vfi_batch_ab.txt] [--repeats 5]
                                    [--parts a,b,c] [--sizes 1,8,64,256,512,1024]
                                    [--round-sizes 8,64] [--max-vfi 10000]

Reference size: k_size = 100, K_size = 4, cold start (V0 of the script, 0.9 k_grid), identity
ALM, howard 50, tol 1e-6, T = 1,100, nx = 1,000.  The candidates are the reference economy with
beta spread evenly over [0.985, 0.99], so their iteration counts differ.  One process, one library.
  (a) C ks_vfi_solve calls one after another (the existing entry point: the baseline) against one
      ks_vfi_solve_batch of the same C candidates through the host tier (the library's geometry),
      and the device tier's one launch alone under each thread-count instantiation (1,024, 512
      and 256 lanes per economy, through AIY_KS_VFI_BATCH_THREADS).  Per C the record applies the
      margin rule: geometry X replaces geometry Y only where median(X) < median(Y) by more than
      the sum of the two legs' [min..max] spreads; the incumbent is 1,024 (the single solve's).
  (b) one ALM round, n_paths = 4: C times (ks_vfi_solve, upload, HistSim) against one
      ks_vfi_solve_batch_dev plus one HistSimMulti launch of 4 C paths.
  (c) krusell_smith_vfi_batch to tol_B for 8 economies against 8 krusell_smith_vfi runs
      (simulate="histogram", n_paths = 4); wall clock, one run each.
Each timed leg of (a) and (b) is bracketed by device events: a warm-up, then the median of
`repeats` runs [min..max].  A looped leg of more than `--long` calls is long and steady, so it is
run once, without warm-up (marked "1 run").  In every part the batched results are compared
with the looped ones of the same run bit for bit, and the geometries with one another; a mismatch
aborts the record.  --max-vfi caps the VFI iterations of every leg alike (the script's 10,000 by
default): in the finer beta spreads some candidate never meets tol, and a launch lasts as long as
its slowest workgroup, so the record states how many candidates stopped at the cap.
"""
import argparse
import os
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from tests.conftest import load_pkg  # noqa: E402

K_SIZE, KK_SIZE, T, NX, N_PATHS, HOWARD, TOL, MAX_VFI = 100, 4, 1100, 1000, 4, 50, 1e-6, 10000
B0 = np.array([0.0, 1.0, 0.0, 1.0])
KNOB = "AIY_KS_VFI_BATCH_THREADS"
GEOMETRIES = (1024, 512, 256)


def timed(fn, repeats, warm=True):
    """(median, min, max) in ms of `repeats` event-bracketed runs of fn(), after a warm-up."""
    import torch
    if warm:
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def fmt(m, runs):
    return (f"{m[0]:10.3f} ms [{m[1]:.3f}..{m[2]:.3f}]" if runs > 1
            else f"{m[0]:10.3f} ms (1 run)")


def beats(x, y):
    """The margin rule: leg x replaces leg y."""
    return x[0] < y[0] - ((x[2] - x[1]) + (y[2] - y[1]))


def choose(legs):
    """The geometry the rule leaves standing, the incumbent being 1,024: a challenger must beat
    the current holder by the margin, the narrower geometry challenging last."""
    hold = 1024
    for g in (512, 256):
        if beats(legs[g], legs[hold]):
            hold = g
    return hold


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--parts", default="a,b,c")
    ap.add_argument("--sizes", default="1,8,64,256,512,1024")
    ap.add_argument("--round-sizes", default="8,64")
    ap.add_argument("--long", type=int, default=64)
    ap.add_argument("--max-vfi", type=int, default=MAX_VFI)
    args = ap.parse_args()
    import torch
    pkg = load_pkg()
    kp = pkg.ks_panel
    dev = torch.device("cuda", 0)
    parts = args.parts.split(",")
    sizes = [int(s) for s in args.sizes.split(",") if s]
    round_sizes = [int(s) for s in args.round_sizes.split(",") if s]
    kg, Kg, P, _ = pkg.calibration.krusell_smith(k_size=K_SIZE, K_size=KK_SIZE)
    k0 = 0.9 * np.repeat(np.repeat(kg[:, None, None], KK_SIZE, 1), 4, 2)
    k0_dev = np.ascontiguousarray(k0.transpose(2, 1, 0))
    kw = dict(howard_steps=HOWARD, tol=TOL, max_vfi=args.max_vfi)
    lines = [f"ks_vfi_batch_ab: {torch.cuda.get_device_name(0)}, k_size = {K_SIZE}, K_size = "
             f"{KK_SIZE}, cold start, howard {HOWARD}, tol {TOL:g}, max_vfi {args.max_vfi}, T = {T}, nx = {NX}; device "
             f"events around each leg, warm-up then median of {args.repeats} [min..max]; parts "
             f"{args.parts}, (a) C in {sizes}, (b) C in {round_sizes}"]

    def say(s):
        lines.append(s)
        print(s, flush=True)
    print(lines[0], flush=True)

    def economy(C_):
        """params (C, 13) and V0 (C, nk, nK, 4): beta enters the script's start value."""
        betas = np.linspace(0.985, 0.99, C_) if C_ > 1 else np.array([0.99])
        prm = np.stack([pkg.ks_params(beta=b) for b in betas])
        V0 = np.stack([pkg.calibration.krusell_smith(k_size=K_SIZE, K_size=KK_SIZE, beta=b)[3]
                       for b in betas])
        return prm, V0

    def rows(blocks):
        return torch.as_tensor(np.ascontiguousarray(blocks.transpose(0, 3, 2, 1)), device=dev)

    x = kp.hist_grid(NX, float(kg[0]), float(kg[-1]))
    zi = kp.zi_paths(T, N_PATHS, kp.matlab_rand(N_PATHS * (T - 1)), pkg.ks_params())
    kg_dev = torch.as_tensor(kg, device=dev)
    os.environ.pop(KNOB, None)

    if "a" in parts:
        for C_ in sizes:
            prm, V0 = economy(C_)
            runs = args.repeats if C_ <= args.long else 1
            solo = [None] * C_

            def chain():
                for c in range(C_):
                    solo[c] = pkg.ks_vfi_solve(V0[c], k0, kg, Kg, B0, P, prm[c], **kw)
            mc = timed(chain, runs, warm=runs > 1)
            out = {}
            k0s = np.broadcast_to(k0, (C_,) + k0.shape)

            def batch():
                out["R"] = pkg.ks_vfi_solve_batch(V0, k0s, kg, Kg, B0, P, prm, **kw)
            mb = timed(batch, args.repeats)
            R = out["R"]
            for c in range(C_):
                assert R["iters"][c] == solo[c]["iters"] and R["rel_diff"][c] == solo[c]["rel_diff"], c
                assert np.array_equal(R["value"][c], solo[c]["value"]), c
                assert np.array_equal(R["k_opt"][c], solo[c]["k_opt"]), c
            V = torch.empty((C_,) + k0_dev.shape, dtype=torch.float64, device=dev)
            ko = torch.empty_like(V)
            V_start, k_start = rows(V0), torch.as_tensor(k0_dev, device=dev)
            outs = (torch.zeros(C_, dtype=torch.int64, device=dev),
                    torch.zeros(C_, dtype=torch.float64, device=dev))
            scr = {}

            def batch_dev():
                V.copy_(V_start)
                ko.copy_(k_start)
                scr["s"] = pkg.ks_vfi_solve_batch_dev(V, ko, kg_dev, Kg, B0, P, prm, out=outs,
                                                      scratch=scr.get("s"), **kw)[2]
            legs = {}
            for g in GEOMETRIES:
                os.environ[KNOB] = str(g)
                legs[g] = timed(batch_dev, args.repeats)
                assert np.array_equal(V.cpu().numpy().transpose(0, 3, 2, 1), R["value"]), g
                assert np.array_equal(ko.cpu().numpy().transpose(0, 3, 2, 1), R["k_opt"]), g
                assert np.array_equal(outs[0].cpu().numpy(), R["iters"]), g
            os.environ.pop(KNOB, None)
            it = R["iters"]
            pick = choose(legs)
            say(f"(a) C = {C_:4d}: {C_} x ks_vfi_solve {fmt(mc, runs)} | ks_vfi_solve_batch "
                f"{fmt(mb, args.repeats)} | chained/batched = {mc[0] / mb[0]:.2f}; iterations "
                f"{int(it.min())}..{int(it.max())}, {int((it == args.max_vfi).sum())} at the cap; "
                f"bit-identical")
            say("      device tier, one launch: " +
                " | ".join(f"{g} lanes {fmt(legs[g], args.repeats)}" for g in GEOMETRIES) +
                f" | margin rule keeps {pick}")
    if "b" in parts:
        for C_ in round_sizes:
            prm, V0 = economy(C_)
            runs = args.repeats if C_ <= args.long else 1
            lam0 = kp.hist_start(x, Kg[0], 0.04)
            sims = kp.HistSim(kg, Kg, x, zi, lam0, prm[0])
            solo_K = [None] * C_

            def round_loop():
                for c in range(C_):
                    S = pkg.ks_vfi_solve(V0[c], k0, kg, Kg, B0, P, prm[c], **kw)
                    kd = torch.as_tensor(np.ascontiguousarray(S["k_opt"].transpose(2, 1, 0)),
                                         device=dev)
                    sims.set_lam(lam0)
                    solo_K[c] = sims(kd).cpu().numpy().T
            ml = timed(round_loop, runs, warm=runs > 1)
            simm = kp.HistSimMulti(kg, x, np.tile(zi, (1, C_)), lam0)
            V = torch.empty((C_,) + k0_dev.shape, dtype=torch.float64, device=dev)
            ko = torch.empty_like(V)
            V_start, k_start = rows(V0), torch.as_tensor(k0_dev, device=dev)
            Kg_dev = torch.as_tensor(np.array(np.broadcast_to(Kg, (C_, KK_SIZE)), order="C"),
                                     device=dev)
            pol = np.repeat(np.arange(C_, dtype=np.int32), N_PATHS)
            got = {}

            def round_batch():
                V.copy_(V_start)
                ko.copy_(k_start)
                simm.set_lam(lam0)
                pkg.ks_vfi_solve_batch_dev(V, ko, kg_dev, Kg, B0, P, prm, **kw)
                got["K"] = simm(ko, Kg_dev, prm, pol).cpu().numpy()
            mr = timed(round_batch, args.repeats)
            bad = [c for c in range(C_)
                   if not np.array_equal(got["K"][c * N_PATHS:(c + 1) * N_PATHS].T, solo_K[c])]
            assert not bad, f"batched round differs from the solo rounds at candidates {bad}"
            say(f"(b) C = {C_:4d}: {C_} solo rounds (solve + {N_PATHS}-path histogram) "
                f"{fmt(ml, runs)} | one batched round, two launches ({C_ * N_PATHS} paths) "
                f"{fmt(mr, args.repeats)} | looped/batched = {ml[0] / mr[0]:.2f}; bit-identical")
    if "c" in parts:
        ecos = [dict(beta=float(b)) for b in np.linspace(0.985, 0.99, 8)]
        ckw = dict(k_size=K_SIZE, K_size=KK_SIZE, T=T, nx=NX, n_paths=N_PATHS,
                   howard_steps=HOWARD, tol_vfi=TOL, max_vfi=args.max_vfi)
        kp.krusell_smith_vfi(simulate="histogram", max_iter_B=1, **ckw)         # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        solo = [kp.krusell_smith_vfi(simulate="histogram", **ckw, **e) for e in ecos]
        t1 = time.perf_counter()
        bat = kp.krusell_smith_vfi_batch(ecos, **ckw)
        t2 = time.perf_counter()
        for s, b in zip(solo, bat):
            assert b["failed"] is None and len(s["B_history"]) == len(b["B_history"])
            assert all(np.array_equal(p, q) for p, q in zip(s["B_history"], b["B_history"]))
            assert np.array_equal(s["K_ts"], b["K_ts"]) and np.array_equal(s["k_opt"], b["k_opt"])
            assert np.array_equal(s["value"], b["value"]) and s["vfi_iters"] == b["vfi_iters"]
        rounds = [len(s["B_history"]) for s in solo]
        say(f"(c) 8 economies to tol_B = 1e-6: 8 x krusell_smith_vfi {1e3 * (t1 - t0):10.1f} ms | "
            f"krusell_smith_vfi_batch {1e3 * (t2 - t1):10.1f} ms | solo/batch = "
            f"{(t1 - t0) / (t2 - t1):.2f}; ALM rounds per economy {rounds}, VFI iterations "
            f"{sum(sum(s['vfi_iters']) for s in solo)} in all; wall clock, 1 run; bit-identical")
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
