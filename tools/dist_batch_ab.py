"""A/B of the batched stationary-distribution solve against one solve after another (one MI355X).

    python tools/dist_batch_ab.py [--out profiles/r12_dist_batch_ab.txt] [--repeats 5]

Workload: the policies of the 63 nodes of the 6-level bisection tree of the GE search at the
scripts' size (N = 7, Na = 400), every candidate solved warm from r0 = 0.04 — the index policies
of Aiyagari_VFI.m (on-grid histogram) and the policy_k of Aiyagari_EGM.m (lottery histogram) —
each histogram from the uniform λ₀ to max|Δλ| < 1e-13.
  (a) aiy_dist_stationary_batch_dev on its one-launch path (one workgroup per candidate);
  (b) the same candidates through aiy_dist_stationary_dev, one call after another on one
      workspace.
For the first C in {2, 16, 63} nodes of the tree (breadth-first: the rates the bisection visits
first): a warm-up of both sides, then `repeats` rounds that run (a) then (b) — the two sides
alternate on one box — and the median wall time of each (host clock around the synchronising
call), with that time per push of the longest candidate.  Outputs are checked equal (a) == (b).
Then the GE wall to the equilibrium r with the histogram supply: ge_batch's multisection
(levels = 6, supply = "histogram") against the chained script loop ge.aiyagari_vfi /
ge.aiyagari_egm (supply = "histogram"), alternating in the same way.
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

TOL, CAP = 1e-13, 100000


def alternate(fa, fb, repeats):
    """Warm both, then `repeats` rounds of fa(), fb(); each returns its own wall in ms."""
    fa(), fb()
    ta, tb = [], []
    for _ in range(repeats):
        ta.append(fa())
        tb.append(fb())
    st = lambda ts: (statistics.median(ts), min(ts), max(ts))
    return st(ta), st(tb)


def policies(pkg, Na, egm):
    """The 63 first-round candidates' policies [63][N][Na] (idx 0-based int32, or policy_k)."""
    gb, cb = pkg.ge_batch, pkg.calibration
    if egm:
        cal, r0, w, guess = gb.egm_calibration(Na, False)
    else:
        cal = cb.aiyagari(Na=Na)
    a, s, P = cal["a_grid"], cal["s"], cal["P"]
    nodes = gb.subtree(-0.05, 1 / cal["beta"] - 1, 1, 6)
    if egm:
        pc0 = pkg.egm_solve(guess.T, a, s, P, r0, w, cal["beta"], cal["sigma"],
                            cal["amin"])["policy_c"]
        pol = np.stack([np.ascontiguousarray(
            pkg.egm_solve(pc0, a, s, P, n.r, w, cal["beta"], cal["sigma"],
                          cal["amin"])["policy_k"].T) for n in nodes])
    else:
        v0 = pkg.vfi_solve(np.zeros((cal["N"], Na)), a, s, P, 0.04,
                           cb.wage(0.04, cal["alpha"], cal["delta"]), cal["beta"],
                           cal["sigma"])["v_old"]
        pol = np.stack([pkg.vfi_solve(v0, a, s, P, n.r, cb.wage(n.r, cal["alpha"], cal["delta"]),
                                      cal["beta"], cal["sigma"])["idx"] - 1
                        for n in nodes]).astype(np.int32)
    return cal, pol


def ab(pkg, Na, egm, repeats, lines):
    import torch
    dev = torch.device("cuda", 0)
    t = lambda x: torch.as_tensor(np.ascontiguousarray(x), device=dev)
    cal, pol = policies(pkg, Na, egm)
    N = cal["N"]
    a_t, P_t = t(cal["a_grid"]), t(cal["P"])
    wsb, wss = pkg.Workspace(N, Na), pkg.Workspace(N, Na)
    wsb.set_dist_batch(1)
    name = f"{'EGM policy_k (lottery)' if egm else 'VFI index policy (on-grid)'} Na = {Na}"
    lines.append(f"{name}: C, (a) batched ms [min..max], (b) separate ms [min..max], (b)/(a), "
                 f"longest candidate's pushes, us per such push (a) / (b)")
    for C in (2, 16, 63):
        pol_t = t(pol[:C])
        kw = dict(policy_k=pol_t) if egm else dict(policy_idx=pol_t)
        lam0 = torch.full((C, N, Na), 1.0 / (N * Na), dtype=torch.float64, device=dev)
        out_b, out_s = torch.zeros_like(lam0), torch.zeros_like(lam0)
        K_b = torch.zeros(C, dtype=torch.float64, device=dev)
        K_s = torch.zeros(C, dtype=torch.float64, device=dev)
        res = {}

        def batched():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res["b"] = pkg.dist_stationary_batch_dev(wsb, lam0, a_t, P_t, out_b, tol=TOL,
                                                     max_iter=CAP, k_supply=K_b, **kw)
            return (time.perf_counter() - t0) * 1e3

        def separate():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            its = []
            for q in range(C):
                one = {k: v[q] for k, v in kw.items()}
                it, _ = pkg.dist_stationary_dev(wss, lam0[q], a_t, P_t, out_s[q], tol=TOL,
                                                max_iter=CAP, k_supply=K_s[q:q + 1], **one)
                its.append(it)
            res["s"] = its
            return (time.perf_counter() - t0) * 1e3
        mb, ms = alternate(batched, separate, repeats)
        it_b = res["b"][0]
        assert list(it_b) == res["s"], (list(it_b), res["s"])
        assert torch.equal(out_b, out_s) and torch.equal(K_b, K_s)
        pushes = int(max(it_b))
        lines.append(f"  C = {C:2d}: (a) {mb[0]:8.3f} [{mb[1]:.3f}..{mb[2]:.3f}]   (b) {ms[0]:8.3f} "
                     f"[{ms[1]:.3f}..{ms[2]:.3f}]   x{ms[0] / mb[0]:6.2f}   pushes {pushes:4d} "
                     f"(min {int(min(it_b))}, sum {int(sum(it_b))})   "
                     f"{1e3 * mb[0] / pushes:7.2f} / {1e3 * ms[0] / pushes:7.2f}")
    assert wsb.dist_batch_counts()[1] == 0
    wsb.close()
    wss.close()


def ge_wall(pkg, egm, repeats, lines):
    gb = pkg.ge_batch
    res = {}

    def fa():
        t0 = time.perf_counter()
        f = gb.aiyagari_egm_multisection if egm else gb.aiyagari_vfi_multisection
        res["a"] = f(Na=400, levels=6, supply="histogram")
        return (time.perf_counter() - t0) * 1e3

    def fb():
        t0 = time.perf_counter()
        res["b"] = (pkg.ge.aiyagari_egm if egm else pkg.ge.aiyagari_vfi)(supply="histogram")
        return (time.perf_counter() - t0) * 1e3
    ma, mb = alternate(fa, fb, repeats)
    A, B = res["a"], res["b"]
    lines.append(f"GE to the equilibrium r with the histogram supply, "
                 f"{'Aiyagari_EGM' if egm else 'Aiyagari_VFI'} Na = 400 (calibration and the r0 "
                 f"solve included in both): multisection(levels=6) r = {A.r!r}, "
                 f"{len(A.r_history)} steps, {ma[0]:.1f} ms [{ma[1]:.1f}..{ma[2]:.1f}]; chained "
                 f"script loop r = {B['r']!r}, {len(B['r_history'])} steps, {mb[0]:.1f} ms "
                 f"[{mb[1]:.1f}..{mb[2]:.1f}]; x{mb[0] / ma[0]:.2f}; same r path: "
                 f"{A.r_history == B['r_history']}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--skip-ge", action="store_true")
    args = ap.parse_args()
    import torch
    pkg = load_pkg()
    lines = [f"dist_batch_ab: {torch.cuda.get_device_name(0)}, the two sides alternating, median "
             f"of {args.repeats} after a warm-up, host clock, N = 7, uniform start, tol {TOL:g}"]
    for egm in (False, True):
        ab(pkg, 400, egm, args.repeats, lines)
    if not args.skip_ge:
        for egm in (False, True):
            ge_wall(pkg, egm, args.repeats, lines)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text)


if __name__ == "__main__":
    main()
