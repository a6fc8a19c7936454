"""A/B of the batched multi-rate EGM solve against one solve after another (one MI355X).

    python tools/egm_batch_ab.py [--out profiles/r07_egm_batch_ab.txt] [--repeats 5]

Workload: the 63 nodes of the 6-level bisection tree of the EGM scripts' GE search, every
candidate from the r0 = 0.04 policy at the scripts' stale wage — A4 and A5 at Na = 400, A4 at
Na = 1,000 (N = 7).
  (a) aiy_egm_solve_batch_dev on its one-launch path (one workgroup per candidate);
  (b) the same candidates through aiy_egm_solve_dev, one call after another on one workspace.
Per variant: a warm-up, then the median wall time of `repeats` runs (host clock around the
synchronising call; the starting policies are copied outside the timed region), and that time
per step of the longest candidate.  The same for the first C in {1, 2, 4, 8, 16} nodes of the
tree (breadth-first: the rates the bisection visits first) — the dispatch threshold's evidence.
Then the GE wall to the equilibrium r: ge_batch.aiyagari_egm_multisection(levels=6) against
ge.aiyagari_egm() (the chained script loop), both scripts.  Outputs are checked equal (a) == (b).
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


def median_ms(fn, repeats):
    fn()  # warm-up
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def workload(pkg, Na, labor):
    gb = pkg.ge_batch
    cal, r0, w, guess = gb.egm_calibration(Na, labor)
    a, s, P = cal["a_grid"], cal["s"], cal["P"]
    if labor:
        R0 = pkg.labor_egm_solve(guess.T, a, s, P, r0, w, cal["beta"], cal["sigma"], 1.0, 1.0,
                                 cal["amin"])
    else:
        R0 = pkg.egm_solve(guess.T, a, s, P, r0, w, cal["beta"], cal["sigma"], cal["amin"])
    nodes = gb.subtree(-0.05, 1 / cal["beta"] - 1, 1, 6)
    return cal, w, np.ascontiguousarray(R0["policy_c"].T), np.array([n.r for n in nodes])


def ab(pkg, Na, labor, repeats, lines):
    import torch
    dev = torch.device("cuda", 0)
    t = lambda x: torch.as_tensor(np.ascontiguousarray(x, dtype=np.float64), device=dev)
    cal, w, pc0, r_all = workload(pkg, Na, labor)
    N = cal["N"]
    a_t, s_t, P_t = t(cal["a_grid"]), t(cal["s"]), t(cal["P"])
    wsb, wss = pkg.Workspace(N, Na), pkg.Workspace(N, Na)
    wsb.set_egm_batch(1)
    name = f"{'A5' if labor else 'A4'} Na = {Na}"
    lines.append(f"{name}: C, (a) batched ms [min..max], (b) separate ms [min..max], (b)/(a), "
                 f"longest candidate's steps, us per such step (a) / (b)")
    for C in (1, 2, 4, 8, 16, 63):
        r = r_all[:C]
        wv = np.full(C, w)
        start = t(np.broadcast_to(pc0, (C, N, Na)))
        c, pk = start.clone(), torch.zeros_like(start)
        pl = torch.zeros_like(start) if labor else None
        res = {}

        def batched():
            c.copy_(start)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res["b"] = pkg.egm_solve_batch_dev(wsb, r, wv, c, a_t, s_t, P_t, cal["beta"],
                                               cal["sigma"], cal["amin"], 1e-5, 1000, pk,
                                               labor=labor, policy_l=pl)
            res["tb"] = (time.perf_counter() - t0) * 1e3

        def separate():
            c.copy_(start)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            its = []
            for q in range(C):
                it, _ = pkg.egm_solve_dev(wss, c[q], a_t, s_t, P_t, r[q], w, cal["beta"],
                                          cal["sigma"], cal["amin"], 1e-5, 1000, pk[q],
                                          labor=labor, policy_l=pl[q] if labor else None)
                its.append(it)
            res["ts"] = (time.perf_counter() - t0) * 1e3
            res["s"] = its

        def timed(fn, key):
            fn()
            ts = []
            for _ in range(repeats):
                fn()
                ts.append(res[key])
            return statistics.median(ts), min(ts), max(ts)
        mb = timed(batched, "tb")
        cb_, kb = c.cpu().numpy().copy(), pk.cpu().numpy().copy()
        ms = timed(separate, "ts")
        it_b, _, st = res["b"]
        assert list(st) == [0] * C and list(it_b) == res["s"], (list(it_b), res["s"])
        assert np.array_equal(cb_, c.cpu().numpy()) and np.array_equal(kb, pk.cpu().numpy())
        steps = int(max(it_b))
        lines.append(f"  C = {C:2d}: (a) {mb[0]:8.3f} [{mb[1]:.3f}..{mb[2]:.3f}]   (b) {ms[0]:8.3f} "
                     f"[{ms[1]:.3f}..{ms[2]:.3f}]   x{ms[0] / mb[0]:6.2f}   steps {steps:4d} "
                     f"(sum {int(sum(it_b))})   {1e3 * mb[0] / steps:7.2f} / {1e3 * ms[0] / steps:7.2f}")
    assert wsb.egm_batch_counts()[1] == 0
    wsb.close()
    wss.close()


def ge_wall(pkg, labor, repeats, lines):
    gb = pkg.ge_batch
    fa = lambda: gb.aiyagari_egm_multisection(Na=400, labor=labor, levels=6)
    fb = (lambda: pkg.ge.aiyagari_labor_egm()) if labor else (lambda: pkg.ge.aiyagari_egm())
    A, B = fa(), fb()
    assert A.r_history == B["r_history"]
    ma, mb = median_ms(fa, repeats), median_ms(fb, repeats)
    lines.append(f"GE to the equilibrium r, {'A5' if labor else 'A4'} Na = 400 (r = {A.r!r}, "
                 f"{len(A.r_history)} steps; calibration and the r0 solve included in both): "
                 f"multisection(levels=6) {ma[0]:.1f} ms [{ma[1]:.1f}..{ma[2]:.1f}], "
                 f"chained script loop {mb[0]:.1f} ms [{mb[1]:.1f}..{mb[2]:.1f}], x{mb[0] / ma[0]:.2f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--skip-ge", action="store_true")
    args = ap.parse_args()
    import torch
    pkg = load_pkg()
    lines = [f"egm_batch_ab: {torch.cuda.get_device_name(0)}, median of {args.repeats} after a "
             f"warm-up, host clock, tol 1e-5, max_iter 1000"]
    for Na, labor in ((400, False), (400, True), (1000, False)):
        ab(pkg, Na, labor, args.repeats, lines)
    if not args.skip_ge:
        for labor in (False, True):
            ge_wall(pkg, labor, args.repeats, lines)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text)


if __name__ == "__main__":
    main()
