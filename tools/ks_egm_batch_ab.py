"""Timing record of the batched Krusell-Smith EGM solve and the lockstep ALM driver (one MI355X).

    python tools/ks_egm_batch_ab.py [--out profiles/ks_egm_batch_ab.txt] [--repeats 5]
                                    [--parts a,b,c] [--sizes 1,8,64,256,512]

Reference size: k_size = 100, K_size = 4, cold start 0.9 k_grid, identity ALM, tol 1e-6,
T = 1,100, nx = 1,000.  The candidates are the reference economy with beta spread evenly over
[0.985, 0.99], so their sweep counts differ.  One process, one library.
  (a) C ks_egm_solve calls one after another (the existing entry point: the baseline) against one
      ks_egm_solve_batch of the same C candidates, both through the host tier, and the device
      tier's one launch alone.
  (b) one ALM round, n_paths = 4: C times (ks_egm_solve, upload, HistSim) against one
      ks_egm_solve_batch_dev plus one HistSimMulti launch of 4 C paths.
  (c) krusell_smith_egm_batch to tol_B for 8 economies against 8 krusell_smith_egm runs
      (simulate="histogram", n_paths = 4); wall clock, one run each.
Each timed leg of (a) and (b) is bracketed by device events: a warm-up, then the median of
`repeats` runs [min..max].  A looped leg of more than `--long` calls is long and steady, so it is
run once, without warm-up (marked "1 run").  In every part the batched results are compared
with the looped ones of the same run bit for bit; a mismatch aborts the record.
"""
import argparse
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from tests.conftest import load_pkg  # noqa: E402

K_SIZE, KK_SIZE, T, NX, N_PATHS, TOL, MAX_EGM = 100, 4, 1100, 1000, 4, 1e-6, 10000
B0 = np.array([0.0, 1.0, 0.0, 1.0])


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--parts", default="a,b,c")
    ap.add_argument("--sizes", default="1,8,64,256,512")
    ap.add_argument("--long", type=int, default=64)
    args = ap.parse_args()
    import torch
    pkg = load_pkg()
    kp = pkg.ks_panel
    dev = torch.device("cuda", 0)
    parts = args.parts.split(",")
    sizes = [int(s) for s in args.sizes.split(",")]
    kg, Kg, P, _ = pkg.calibration.krusell_smith(k_size=K_SIZE, K_size=KK_SIZE)
    k0 = 0.9 * np.repeat(np.repeat(kg[:, None, None], KK_SIZE, 1), 4, 2)
    k0_dev = np.ascontiguousarray(k0.transpose(2, 1, 0))
    lines = [f"ks_egm_batch_ab: {torch.cuda.get_device_name(0)}, k_size = {K_SIZE}, K_size = "
             f"{KK_SIZE}, cold start, tol {TOL:g}, T = {T}, nx = {NX}; device events around each "
             f"leg, warm-up then median of {args.repeats} [min..max]; parts {args.parts}, C in "
             f"{sizes}"]

    def say(s):
        lines.append(s)
        print(s, flush=True)
    print(lines[0], flush=True)

    def params_of(C_):
        betas = np.linspace(0.985, 0.99, C_) if C_ > 1 else np.array([0.99])
        return np.stack([pkg.ks_params(beta=b) for b in betas])

    x = kp.hist_grid(NX, float(kg[0]), float(kg[-1]))
    zi = kp.zi_paths(T, N_PATHS, kp.matlab_rand(N_PATHS * (T - 1)), pkg.ks_params())
    kg_dev = torch.as_tensor(kg, device=dev)

    for C_ in sizes:
        prm = params_of(C_)
        runs = args.repeats if C_ <= args.long else 1
        if "a" in parts:
            solo = [None] * C_

            def chain():
                for c in range(C_):
                    solo[c] = pkg.ks_egm_solve(k0, kg, Kg, B0, P, prm[c], tol=TOL, max_iter=MAX_EGM)
            mc = timed(chain, runs, warm=runs > 1)
            out = {}

            def batch():
                out["R"] = pkg.ks_egm_solve_batch(np.broadcast_to(k0, (C_,) + k0.shape), kg, Kg, B0,
                                                  P, prm, tol=TOL, max_iter=MAX_EGM)
            mb = timed(batch, args.repeats)
            R = out["R"]
            for c in range(C_):
                assert R["status"][c] == 0 and R["iters"][c] == solo[c]["iters"], c
                assert R["diff"][c] == solo[c]["diff"], c
                assert np.array_equal(R["k_opt"][c], solo[c]["k_opt"]), c
            ko = torch.empty((C_,) + k0_dev.shape, dtype=torch.float64, device=dev)
            start = torch.as_tensor(k0_dev, device=dev)
            outs = (torch.zeros(C_, dtype=torch.int64, device=dev),
                    torch.zeros(C_, dtype=torch.float64, device=dev),
                    torch.zeros(C_, dtype=torch.int32, device=dev))
            scr = {}

            def batch_dev():
                ko.copy_(start)
                scr["s"] = pkg.ks_egm_solve_batch_dev(ko, kg_dev, Kg, B0, P, prm, tol=TOL,
                                                      max_iter=MAX_EGM, out=outs,
                                                      scratch=scr.get("s"))[3]
            md = timed(batch_dev, args.repeats)
            assert np.array_equal(ko.cpu().numpy().transpose(0, 3, 2, 1), R["k_opt"])
            it = R["iters"]
            say(f"(a) C = {C_:3d}: {C_} x ks_egm_solve {fmt(mc, runs)} | ks_egm_solve_batch "
                f"{fmt(mb, args.repeats)} | device tier {fmt(md, args.repeats)} | chained/batched "
                f"= {mc[0] / mb[0]:.2f}, chained/device = {mc[0] / md[0]:.2f}; sweeps "
                f"{int(it.min())}..{int(it.max())}; bit-identical")
        if "b" in parts:
            lam0 = kp.hist_start(x, Kg[0], 0.04)
            sims = kp.HistSim(kg, Kg, x, zi, lam0, prm[0])
            solo_K = [None] * C_

            def round_loop():
                for c in range(C_):
                    S = pkg.ks_egm_solve(k0, kg, Kg, B0, P, prm[c], tol=TOL, max_iter=MAX_EGM)
                    kd = torch.as_tensor(np.ascontiguousarray(S["k_opt"].transpose(2, 1, 0)),
                                         device=dev)
                    sims.set_lam(lam0)
                    solo_K[c] = sims(kd).cpu().numpy().T
            ml = timed(round_loop, runs, warm=runs > 1)
            simm = kp.HistSimMulti(kg, x, np.tile(zi, (1, C_)), lam0)
            ko = torch.empty((C_,) + k0_dev.shape, dtype=torch.float64, device=dev)
            start = torch.as_tensor(k0_dev, device=dev)
            Kg_dev = torch.as_tensor(np.array(np.broadcast_to(Kg, (C_, KK_SIZE)), order="C"), device=dev)
            pol = np.repeat(np.arange(C_, dtype=np.int32), N_PATHS)
            got = {}

            def round_batch():
                ko.copy_(start)
                simm.set_lam(lam0)
                pkg.ks_egm_solve_batch_dev(ko, kg_dev, Kg, B0, P, prm, tol=TOL, max_iter=MAX_EGM)
                got["K"] = simm(ko, Kg_dev, prm, pol).cpu().numpy()
                got["slow"] = simm.slow[:C_ * N_PATHS].cpu().numpy()
            mr = timed(round_batch, args.repeats)
            bad = [c for c in range(C_)
                   if not np.array_equal(got["K"][c * N_PATHS:(c + 1) * N_PATHS].T, solo_K[c])]
            assert not bad, f"batched round differs from the solo rounds at candidates {bad}"
            say(f"(b) C = {C_:3d}: {C_} solo rounds (solve + {N_PATHS}-path histogram) "
                f"{fmt(ml, runs)} | one batched round ({C_ * N_PATHS} paths) "
                f"{fmt(mr, args.repeats)} | looped/batched = {ml[0] / mr[0]:.2f}; slow-path periods "
                f"per path {int(got['slow'].min())}..{int(got['slow'].max())}; bit-identical")
    if "c" in parts:
        ecos = [dict(beta=float(b)) for b in np.linspace(0.985, 0.99, 8)]
        kw = dict(k_size=K_SIZE, K_size=KK_SIZE, T=T, nx=NX, n_paths=N_PATHS, tol_egm=TOL,
                  max_egm=MAX_EGM)
        kp.krusell_smith_egm(simulate="histogram", max_iter_B=1, **kw)          # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        solo = [kp.krusell_smith_egm(simulate="histogram", **kw, **e) for e in ecos]
        t1 = time.perf_counter()
        bat = kp.krusell_smith_egm_batch(ecos, **kw)
        t2 = time.perf_counter()
        for s, b in zip(solo, bat):
            assert b["failed"] is None and len(s["B_history"]) == len(b["B_history"])
            assert all(np.array_equal(p, q) for p, q in zip(s["B_history"], b["B_history"]))
            assert np.array_equal(s["K_ts"], b["K_ts"]) and np.array_equal(s["k_opt"], b["k_opt"])
            assert s["egm_iters"] == b["egm_iters"]
        rounds = [len(s["B_history"]) for s in solo]
        say(f"(c) 8 economies to tol_B = 1e-6: 8 x krusell_smith_egm {1e3 * (t1 - t0):10.1f} ms | "
            f"krusell_smith_egm_batch {1e3 * (t2 - t1):10.1f} ms | solo/batch = "
            f"{(t1 - t0) / (t2 - t1):.2f}; ALM rounds per economy {rounds}, EGM sweeps "
            f"{sum(sum(s['egm_iters']) for s in solo)} in all; wall clock, 1 run; bit-identical")
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
