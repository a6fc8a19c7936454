"""Timing record of the Krusell-Smith histogram simulation beside the agent panel (one MI355X).

    python tools/ks_hist_ab.py [--out profiles/r13_ks_hist_ab.txt] [--repeats 5]

All at the reference size (k_size = 100, K_size = 4, T = 1,100), policy = the committed fixture
tests/golden/ks_panel_small.npz (a script-sized policy), one process, one library:
  (a) ks_simulate_hist_dev at nx = 1,000 for M = 1, 8 and 64 shock paths (one launch each);
  (b) ks_simulate_capital_dev with 10,000 agents on path 0's shocks (1,099 launches).
Each is bracketed by device events on the stream: a warm-up run, then the median of `repeats`
runs (min..max beside it).  The panel leg's time in the parent commit's full benchmark record
(profiles/r06_final_bench_detail.json, ks_panel.reference.simulate_ms) is quoted beside (b).
  (c) (a) at M = 1 with an identity policy, and with a uniform histogram grid: every run of
      sources short, to show what the long runs of the x^7 grid cost.
For the record only: max |K_ts histogram - K_ts panel| on path 0 (the panel carries sampling
noise of 10,000 agents; nothing is asserted about it).
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from tests.conftest import load_pkg  # noqa: E402

T, NX, POP = 1100, 1000, 10000
PARENT = ROOT / "profiles" / "r06_final_bench_detail.json"


def timed(fn, repeats):
    """Warm-up, then `repeats` event-bracketed runs of fn(); (median, min, max) in ms."""
    import torch
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    import torch
    pkg = load_pkg()
    kp = pkg.ks_panel
    dev = torch.device("cuda", 0)
    g = dict(np.load(ROOT / "tests" / "golden" / "ks_panel_small.npz", allow_pickle=False))
    prm = pkg.ks_params()
    kg, Kg, _, _ = pkg.calibration.krusell_smith(k_size=100, K_size=4)
    k_opt = g["k_opt"]
    assert k_opt.shape == (100, 4, 4)
    ko = torch.as_tensor(np.ascontiguousarray(k_opt.transpose(2, 1, 0)), device=dev)
    x = kp.hist_grid(NX, prm[3], prm[4])
    lam0 = kp.hist_start(x, Kg[0], prm[5])
    lines = [f"ks_hist_ab: {torch.cuda.get_device_name(0)}, k_size = 100, K_size = 4, T = {T}, "
             f"device events around each run, warm-up then median of {args.repeats} [min..max]"]

    # the panel: the script's shocks (path 0 of the histogram runs is the same aggregate chain)
    U = kp.matlab_rand(kp.shock_draws(T, POP))
    zi_d, eps_d = kp.ks_shocks_dev(torch.as_tensor(U, device=dev), prm, T, POP)
    k_pop = torch.full((POP,), float(Kg[0]), dtype=torch.float64, device=dev)
    panel = kp.PanelSim(torch.as_tensor(kg, device=dev), torch.as_tensor(Kg, device=dev), zi_d,
                        eps_d, k_pop)

    def run_panel():
        panel.k_pop.fill_(float(Kg[0]))
        panel(ko)
    mp = timed(run_panel, args.repeats)
    K_panel = panel.K_ts.cpu().numpy().copy()
    parent = json.loads(PARENT.read_text())["ks_panel"]["reference"]["simulate_ms"]
    lines.append(f"(b) panel, {POP} agents, {T - 1} launches: {mp[0]:8.3f} ms [{mp[1]:.3f}.."
                 f"{mp[2]:.3f}]  = {1e3 * mp[0] / (T - 1):.2f} us per period   (parent's full "
                 f"benchmark record: {parent:.3f} ms)")

    zi_all = kp.zi_paths(T, 64, kp.matlab_rand(64 * (T - 1)), prm)
    assert np.array_equal(zi_all[:, 0], zi_d.cpu().numpy())
    obs = T - 100
    for M in (1, 8, 64):
        sim = kp.HistSim(kg, Kg, x, zi_all[:, :M], lam0, prm)
        lam_start = sim.lam.clone()

        def run_hist():
            sim.lam.copy_(lam_start)
            sim(ko)
        mh = timed(run_hist, args.repeats)
        K_hist = sim.K_ts.cpu().numpy().T
        slow = sim.slow.cpu().numpy()
        lines.append(f"(a) histogram nx = {NX}, M = {M:2d}, one launch: {mh[0]:8.3f} ms "
                     f"[{mh[1]:.3f}..{mh[2]:.3f}]  = {1e3 * mh[0] / (T - 1):.2f} us per period, "
                     f"{M * obs} regression observations, (b)/(a) = {mp[0] / mh[0]:.2f}, "
                     f"slow periods {int(slow.sum())}")
        if M == 1:
            d = np.abs(K_hist[:, 0] - K_panel)
            lines.append(f"    path 0: max |K_ts histogram - K_ts panel| = {d.max():.4f} at t = "
                         f"{int(d.argmax())} (K_ts there {K_panel[int(d.argmax())]:.3f}); after "
                         f"t = 100: {d[100:].max():.4f}")
    # where a period's time goes: the same run (M = 1) with every run of sources short
    ident = np.ascontiguousarray(np.broadcast_to(kg[None, None, :], (4, 4, 100)))
    for name, pol, grid in (("identity policy k' = k (runs of 1-2 sources)", ident, x),
                            ("fixture policy, uniform x on [k_min, 200]", ko.cpu().numpy(),
                             np.linspace(float(prm[3]), 200.0, NX))):
        sim = kp.HistSim(kg, Kg, grid, zi_all[:, :1], kp.hist_start(grid, Kg[0], prm[5]), prm)
        lam_start = sim.lam.clone()
        pol_t = torch.as_tensor(pol, device=dev)

        def run_var():
            sim.lam.copy_(lam_start)
            sim(pol_t)
        mv = timed(run_var, args.repeats)
        lines.append(f"(c) histogram nx = {NX}, M =  1, {name}: {mv[0]:8.3f} ms [{mv[1]:.3f}.."
                     f"{mv[2]:.3f}]  = {1e3 * mv[0] / (T - 1):.2f} us per period")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text)


if __name__ == "__main__":
    main()
