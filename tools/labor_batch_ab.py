"""A/B of the batched multi-rate labour VFI solve against one solve after another (one MI355X).

    python tools/labor_batch_ab.py [--out profiles/r10_labor_batch_ab.txt] [--repeats 5]

Workload: the 63 first-round nodes of the 6-level bisection tree of
Aiyagari_Endogenous_Labor_VFI.m's GE search at the script's defaults (N = 7, Na = 400, Nl = 10),
every candidate from the r0 = 0.04 solution at its own wage, and the first C in {1, 2, 4, 8, 16}
of them (breadth-first: the rates the bisection visits first) — the dispatch threshold's evidence.
  (a) aiy_labor_vfi_solve_batch_dev on its batched path (one launch per sweep over all candidates);
  (b) the same candidates through the host-tier aiy_labor_vfi_solve, one call after another (the
      only labour solve there was before the batched one);
  (c) the same device call as (a) with the batched path off: one single-rate solve after another
      on device tensors (what the default dispatch chooses below its threshold).
Per C: a warm-up of each variant, then `repeats` rounds that run (a), (b), (c) in turn in one
process; the median wall time of each (host clock around the synchronising call; the starting
arrays are copied outside the timed region) with its min..max spread.  Outputs are checked equal.
Then the GE wall to the script's r: ge_batch.aiyagari_labor_vfi_multisection at levels in
{2, 3, 6} against ge.aiyagari_labor_vfi() (the chained script loop).
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

PSI, ETA = 1.0, 2.0


def stats(ts):
    return statistics.median(ts), min(ts), max(ts)


def ab(pkg, Na, repeats, lines):
    import torch
    gb = pkg.ge_batch
    dev = torch.device("cuda", 0)
    t = lambda x, dt=np.float64: torch.as_tensor(np.ascontiguousarray(x, dtype=dt), device=dev)
    cal, L = gb.labor_calibration(Na)
    a, s, P, N = cal["a_grid"], cal["s"], cal["P"], cal["N"]
    wage = lambda r: pkg.calibration.wage(r, cal["alpha"], cal["delta"])
    R0 = pkg.labor_vfi_solve(np.zeros((N, Na)), a, s, P, L, 0.04, wage(0.04), cal["beta"],
                             cal["sigma"], PSI, ETA)
    st = gb.labor_start(R0)
    r_all = np.array([n.r for n in gb.subtree(-0.05, 1 / cal["beta"] - 1, 1, 6)])
    a_t, s_t, P_t, L_t = t(a), t(s), t(P), t(L)
    wa, wc = pkg.Workspace(N, Na, L.size), pkg.Workspace(N, Na, L.size)
    wa.set_labor_batch(1)
    wc.set_labor_batch(1 << 20)
    lines.append(f"Na = {Na}: C, (a) batched ms [min..max], (b) host-tier separate ms [min..max], "
                 f"(c) device-tier separate ms [min..max], (b)/(a), (c)/(a), longest candidate's "
                 f"sweeps (sum), us per such sweep (a)")
    for C in (1, 2, 4, 8, 16, 63):
        r = r_all[:C]
        w = np.array([wage(x) for x in r])
        rep = lambda x, dt=np.float64: t(np.broadcast_to(np.asarray(x), (C, N, Na)), dt)
        src = [rep(st["v_old"]), rep(st["v_new"]), rep(st["policies"][0]), rep(st["policies"][1]),
               rep(st["policies"][2]), rep(st["policies"][3] - 1, np.int32)]
        buf = [x.clone() for x in src]
        res = {}

        def device(ws, key):
            for x, y in zip(buf, src):
                x.copy_(y)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            it, which = pkg.labor_solve_batch_dev(ws, r, w, buf[0], buf[1], a_t, s_t, P_t, L_t,
                                                  cal["beta"], cal["sigma"], PSI, ETA, 1e-5, 1000,
                                                  buf[5], buf[2], buf[3], buf[4])
            res["t" + key] = (time.perf_counter() - t0) * 1e3
            vn = torch.stack([buf[which[q]][q] for q in range(C)]).cpu().numpy()
            res[key] = (it, vn, buf[2].cpu().numpy().copy(), buf[5].cpu().numpy().copy())

        def host():
            t0 = time.perf_counter()
            out = [pkg.labor_vfi_solve(st["v_old"], a, s, P, L, r[q], w[q], cal["beta"],
                                       cal["sigma"], PSI, ETA, 1e-5, 1000, v_new=st["v_new"],
                                       policies=st["policies"]) for q in range(C)]
            res["tb"] = (time.perf_counter() - t0) * 1e3
            res["b"] = ([R["iters"] for R in out], np.stack([R["v_new"] for R in out]),
                        np.stack([R["policy_k"] for R in out]),
                        np.stack([R["lin"] - 1 for R in out]))
        variants = (lambda: device(wa, "a"), host, lambda: device(wc, "c"))
        for fn in variants:
            fn()  # warm-up
        ts = {"ta": [], "tb": [], "tc": []}
        for _ in range(repeats):
            for fn in variants:
                fn()
            for k in ts:
                ts[k].append(res[k])
        for k in ("b", "c"):
            assert list(res["a"][0]) == list(res[k][0]), (res["a"][0], res[k][0])
            for x, y in zip(res["a"][1:], res[k][1:]):
                assert np.array_equal(x, y), k
        ma, mb, mc = stats(ts["ta"]), stats(ts["tb"]), stats(ts["tc"])
        its = res["a"][0]
        lines.append(f"  C = {C:2d}: (a) {ma[0]:8.3f} [{ma[1]:.3f}..{ma[2]:.3f}]   (b) {mb[0]:8.3f} "
                     f"[{mb[1]:.3f}..{mb[2]:.3f}]   (c) {mc[0]:8.3f} [{mc[1]:.3f}..{mc[2]:.3f}]   "
                     f"x{mb[0] / ma[0]:6.2f}  x{mc[0] / ma[0]:6.2f}   sweeps {max(its):4d} "
                     f"(sum {sum(its)})   {1e3 * ma[0] / max(its):7.2f}")
    assert wa.labor_batch_counts()[1] == 0 and wc.labor_batch_counts()[0] == 0
    wa.close()
    wc.close()


def ge_wall(pkg, repeats, lines):
    gb = pkg.ge_batch
    fns = {f"multisection(levels={lv})": (lambda lv=lv: gb.aiyagari_labor_vfi_multisection(levels=lv))
           for lv in (2, 3, 6)}
    fns["chained script loop"] = lambda: pkg.ge.aiyagari_labor_vfi()
    out = {k: fn() for k, fn in fns.items()}  # warm-up
    G = out["chained script loop"]
    for k, A in out.items():
        if k != "chained script loop":
            assert A.r_history == G["r_history"], k
    ts = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            t0 = time.perf_counter()
            fn()
            ts[k].append((time.perf_counter() - t0) * 1e3)
    lines.append(f"GE to the script's r at the defaults (r = {G['r_history'][-1]!r}, "
                 f"{len(G['r_history'])} steps; calibration and the r0 solve included in all; "
                 f"chained sweeps per step {G['iters']}):")
    for k in fns:
        m = stats(ts[k])
        extra = "" if k.startswith("chained") else \
            f"   {out[k].candidates} candidates in {out[k].rounds} rounds"
        lines.append(f"  {k:26s} {m[0]:8.1f} ms [{m[1]:.1f}..{m[2]:.1f}]{extra}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--skip-ge", action="store_true")
    args = ap.parse_args()
    import torch
    pkg = load_pkg()
    lines = [f"labor_batch_ab: {torch.cuda.get_device_name(0)}, median of {args.repeats} after a "
             f"warm-up, variants alternating in one process, host clock, tol 1e-5, max_iter 1000"]
    ab(pkg, 400, args.repeats, lines)
    if not args.skip_ge:
        ge_wall(pkg, args.repeats, lines)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text)


if __name__ == "__main__":
    main()
