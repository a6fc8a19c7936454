"""Jacobians and GE responses of many economies per launch, measured (one MI355X).

    python tools/ssj_batch_ab.py [--out profiles/ssj_batch_ab.txt] [--repeats 5] [--T 300]
                                 [--parent-lib PATH]

Workload: N = 7, Na = 400 (the scripts' grid), T = 300.  The economies are 16 steady states,
β = 0.94 … 0.965, each found by transition.steady_state; a batch of C lists them in turn (a batch
larger than 16 repeats them: an economy's bits and time do not depend on its neighbours).
  (a) jacobian_batch(C) against C jacobian() calls, with the four stages' device times;
  (b) dense_solve_batch at n = T, R = 1 and R = T (the systems I − M of (a)'s Jacobians; the
      right-hand sides are the first and all columns of J_r + J_w) against one stacked
      np.linalg.solve on the host;
  (c) structural_loglik end to end with its split: Jacobians, host assembly, solve, likelihood;
  (d) --parent-lib: jacobian() under this build and under the parent commit's library (another
      process each, AIY_HIP_LIB), five repeats each with their spread.
Per variant: a warm-up, then the median wall time of `repeats` runs (host clock around work that
ends in a synchronise).  The shader clock level is read before and after."""
import argparse
import json
import os
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from tests.conftest import load_pkg  # noqa: E402
from tools.transition_ab import clock_level, timed  # noqa: E402

N, NA = 7, 400


def solo_probe(T, repeats):
    """The solo jacobian() of the default calibration under whatever library AIY_HIP_LIB names:
    one JSON line (median, min, max ms and the stages)."""
    pkg = load_pkg()
    ss = pkg.steady_state(pkg.calibration.aiyagari(Na=NA))
    stages = []

    def run():
        ms = np.zeros(4)
        pkg.jacobian(ss, T, 1e-4, stage_ms=ms)
        stages.append(ms)
    m = timed(run, repeats)
    print(json.dumps(dict(ms=m, stages=list(np.median(np.stack(stages[1:]), axis=0)))))


def probe(lib, T, repeats):
    env = dict(os.environ)
    if lib:
        env["AIY_HIP_LIB"] = str(Path(lib).resolve())
    out = subprocess.run([sys.executable, __file__, "--solo-probe", "--T", str(T), "--repeats",
                          str(repeats)], env=env, check=True, capture_output=True, text=True,
                         timeout=300)
    return json.loads(out.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--T", type=int, default=300)
    ap.add_argument("--C", type=int, nargs="*", default=[1, 16, 64, 256])
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--solo-probe", action="store_true")
    args = ap.parse_args()
    T, h = args.T, 1e-4
    if args.solo_probe:
        return solo_probe(T, args.repeats)
    import torch
    pkg = load_pkg()
    cb, est = pkg.calibration, pkg.estimation
    t0 = time.perf_counter()
    pool = [pkg.steady_state(cb.aiyagari(Na=NA, beta=float(b))) for b in np.linspace(0.94, 0.965, 16)]
    t_ss = time.perf_counter() - t0
    clk0 = clock_level()
    lines = [f"ssj_batch_ab: {torch.cuda.get_device_name(0)}, N = {N}, Na = {NA}, T = {T}, "
             f"h = {h:g}; 16 steady states, beta = 0.94 .. 0.965 ({t_ss:.2f} s); median of "
             f"{args.repeats} after a warm-up [min..max], host clock, {os.cpu_count()} CPUs seen, "
             f"OMP_NUM_THREADS = {os.environ.get('OMP_NUM_THREADS', 'unset')}"]
    print(lines[0], file=sys.stderr, flush=True)
    res = {}

    lines.append("(a) jacobian_batch (F and E left on the device) | C jacobian() calls | solo/batch "
                 "| device time of the batch's stages: backward, forward, expectation, contraction")
    for C in args.C:
        eco = [pool[c % 16] for c in range(C)]
        stages = []

        def batch():
            ms = np.zeros(4)
            res["B"] = pkg.jacobian_batch(eco, T, h, stage_ms=ms, want_F=False, want_E=False)
            stages.append(ms)

        def solo():
            res["S"] = [pkg.jacobian(ss, T, h) for ss in eco]
        mb, msolo = timed(batch, args.repeats), timed(solo, args.repeats)
        assert not res["B"]["status"].any()
        assert all(np.array_equal(res["B"]["J_r"][c], res["S"][c]["J_r"]) for c in range(C))
        sm = np.median(np.stack(stages[1:]), axis=0)
        lines.append(f"  C = {C:3d}: {mb[0]:9.2f} ms [{mb[1]:.2f}..{mb[2]:.2f}] | {msolo[0]:9.2f} ms "
                     f"[{msolo[1]:.2f}..{msolo[2]:.2f}] | x{msolo[0] / mb[0]:.2f} | "
                     f"{sm[0]:.2f}, {sm[1]:.2f}, {sm[2]:.2f}, {sm[3]:.2f} ms")
        res[("jac", C)] = res["B"]

    lines.append("(b) dense_solve_batch, n = T: R = 1 device | host np.linalg.solve (stacked) | "
                 "host/device || R = T device | host | host/device")
    for C in args.C:
        eco = [pool[c % 16] for c in range(C)]
        J = res[("jac", C)]
        A = np.stack([-pkg.transition._newton_matrix(eco[c], dict(J_r=J["J_r"][c], J_w=J["J_w"][c]))
                      for c in range(C)])
        b1 = np.stack([J["J_r"][c][:, :1] + J["J_w"][c][:, :1] for c in range(C)])
        bT = np.stack([J["J_r"][c] + J["J_w"][c] for c in range(C)])
        row = f"  C = {C:3d}:"
        for B in (b1, bT):
            def dev():
                res["X"] = est.dense_solve_batch(A, B)

            def host():
                res["Xh"] = np.linalg.solve(A, B)
            md, mh = timed(dev, args.repeats), timed(host, args.repeats)
            assert not res["X"]["status"].any()
            err = np.max(np.abs(res["X"]["X"] - res["Xh"])) / np.max(np.abs(res["Xh"]))
            row += (f" {md[0]:9.2f} ms [{md[1]:.2f}..{md[2]:.2f}] | {mh[0]:9.2f} ms "
                    f"[{mh[1]:.2f}..{mh[2]:.2f}] | x{mh[0] / md[0]:.2f} (max rel diff {err:.1e}) ||")
        lines.append(row.rstrip("|"))

    lines.append("(c) structural_loglik (Y, C, K; L = 40): total | Jacobians, host assembly, solve, "
                 "likelihood (host clock, ms)")
    rng = np.random.default_rng(1)
    y = 0.01 * rng.standard_normal((40, 3))
    for C in args.C:
        eco = [pool[c % 16] for c in range(C)]
        rho, sg = np.linspace(0.7, 0.95, C), np.full(C, 0.01)
        splits = []

        def chain():
            sp = np.zeros(4)
            res["L"] = est.structural_loglik(eco, y, rho, sg, np.full(3, 1e-4), T, split_ms=sp)
            splits.append(sp)
        mc = timed(chain, args.repeats)
        assert not res["L"]["status"].any()
        sp = np.median(np.stack(splits[1:]), axis=0)
        lines.append(f"  C = {C:3d}: {mc[0]:9.2f} ms [{mc[1]:.2f}..{mc[2]:.2f}] | {sp[0]:.2f}, "
                     f"{sp[1]:.2f}, {sp[2]:.2f}, {sp[3]:.2f}")

    if args.parent_lib:
        here, parent = probe("", T, args.repeats), probe(args.parent_lib, T, args.repeats)
        for name, p in (("this build", here), ("parent commit", parent)):
            m, s = p["ms"], p["stages"]
            lines.append(f"(d) jacobian() solo, {name}: {m[0]:.3f} ms [{m[1]:.3f}..{m[2]:.3f}]; "
                         f"stages {s[0]:.3f}, {s[1]:.3f}, {s[2]:.3f}, {s[3]:.3f} ms")
    lines.append(f"shader clock level before: {clk0}, after: {clock_level()}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text)


if __name__ == "__main__":
    main()
