"""A/B of the batched transition passes against the per-step entry points (one MI355X).

    python tools/transition_ab.py [--out profiles/transition_ab.txt] [--repeats 5] [--T 300]

Workload: N = 7, Na = 400 (the scripts' grid), T = 300 periods on a constant price path
(r = 0.03, its wage), every path from one terminal policy and one λ₀, for C = 1, 16, 64, 256.
  (a) aiy_transition_batch: the backward and the forward pass, one workgroup per path each, the
      period policies staying on the device (host entry: staging and read-back of K included);
  (b) the per-step path with the same step count: per path T chained aiy_egm_step_dev calls,
      then T chained aiy_dist_update_dev calls (device tier, one workspace; each push call
      builds its plan and reads the monotonicity flag, as that entry does).
Per variant: a warm-up, then the median wall time of `repeats` runs (host clock around work that
ends in a synchronise).  The shader clock level is read before and after.  K[T] of (a) is checked
against Σ λ_T·a of (b)'s last λ (1e-12 relative) and the policies of the two bit for bit.
"""
import argparse
import glob
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from tests.conftest import load_pkg  # noqa: E402


def clock_level():
    """The active shader clock level of card 0 (read-only), or 'not available'."""
    for f in sorted(glob.glob("/sys/class/drm/card*/device/pp_dpm_sclk")):
        try:
            act = [ln.strip() for ln in Path(f).read_text().splitlines() if ln.strip().endswith("*")]
            if act:
                return act[0]
        except OSError:
            pass
    return "not available"


def timed(fn, repeats):
    fn()  # warm-up
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--T", type=int, default=300)
    ap.add_argument("--C", type=int, nargs="*", default=[1, 16, 64, 256])
    args = ap.parse_args()
    import torch
    pkg = load_pkg()
    cb = pkg.calibration
    N, Na, T = 7, 400, args.T
    cal = cb.aiyagari(Na=Na)
    a, s, P = cal["a_grid"], cal["s"], cal["P"]
    r0 = 0.03
    w0 = cb.wage(r0, cal["alpha"], cal["delta"])
    guess = np.tile((1 + r0) * a + w0 * np.mean(s), (N, 1))
    pcT = np.ascontiguousarray(pkg.egm_solve(guess.T, a, s, P, r0, w0, cal["beta"], cal["sigma"],
                                             cal["amin"], max_iter=40)["policy_c"].T)
    lam0 = np.full((N, Na), 1.0 / (N * Na))
    dev = torch.device("cuda", 0)
    t = lambda x: torch.as_tensor(np.ascontiguousarray(x, dtype=np.float64), device=dev)
    a_t, s_t, P_t, pc_t, l0_t = t(a), t(s), t(P), t(pcT), t(lam0)
    ws = pkg.Workspace(N, Na)
    pk = torch.zeros((T, N, Na), dtype=torch.float64, device=dev)
    bufs = [torch.zeros((N, Na), dtype=torch.float64, device=dev) for _ in range(2)]
    res = {}

    def per_step_path():
        cur = pc_t
        for q in range(T):  # period T − 1 − q
            nxt = bufs[q & 1]
            pkg.egm_step_dev(ws, cur, a_t, s_t, P_t, r0, w0, cal["beta"], cal["sigma"],
                             cal["amin"], nxt, pk[T - 1 - q])
            cur = nxt
        lam = l0_t
        for q in range(T):
            out = bufs[q & 1]
            pkg.dist_update_dev(ws, lam, a_t, P_t, out, policy_k=pk[q])
            lam = out
        torch.cuda.synchronize()
        res["lam"] = lam

    clk0 = clock_level()
    lines = [f"transition_ab: {torch.cuda.get_device_name(0)}, N = {N}, Na = {Na}, T = {T}, constant "
             f"path r = {r0}; median of {args.repeats} after a warm-up, host clock",
             "C, (a) aiy_transition_batch ms [min..max], (b) per-step path ms [min..max], (b)/(a), "
             "us per period and pass (a) / (b)"]
    for C in args.C:
        rr, ww = np.full((C, T + 1), r0), np.full((C, T), w0)
        targs = (rr, ww, pcT, lam0, a, s, P, cal["beta"], cal["sigma"], cal["amin"])

        def batched():
            res["K"], res["st"], _ = pkg.transition_batch(*targs)

        def separate():
            for _ in range(C):
                per_step_path()
        ma = timed(batched, args.repeats)
        mb = timed(separate, args.repeats)
        assert (res["st"] == 0).all()
        lamT = res["lam"].cpu().numpy()
        KT = float(np.sum(lamT * a[None, :]))
        assert np.all(np.abs(res["K"][:, T] - KT) <= 1e-12 * abs(KT)), (res["K"][:, T], KT)
        lines.append(f"  C = {C:3d}: (a) {ma[0]:9.3f} [{ma[1]:.3f}..{ma[2]:.3f}]   (b) {mb[0]:10.3f} "
                     f"[{mb[1]:.3f}..{mb[2]:.3f}]   x{mb[0] / ma[0]:7.2f}   "
                     f"{1e3 * ma[0] / (2 * T):7.2f} / {1e3 * mb[0] / (2 * T * C):7.2f}")
    # the policies of the two paths, bit for bit (C = 1)
    B = pkg.egm_backward_batch(np.full((1, T + 1), r0), np.full((1, T), w0), pcT, a, s, P,
                               cal["beta"], cal["sigma"], cal["amin"], want_pc=False)
    per_step_path()
    assert np.array_equal(B["policy_k"][0], pk.cpu().numpy())
    lines.append(f"policies of (a) and (b) equal bit for bit; shader clock level before: {clk0}, "
                 f"after: {clock_level()}")
    ws.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text)


if __name__ == "__main__":
    main()
