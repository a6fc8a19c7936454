"""The sequence-space Jacobian and the Newton driver, measured (one MI355X).

    python tools/ssj_ab.py [--out profiles/ssj_ab.txt] [--repeats 5] [--T 300]

Workload: N = 7, Na = 400 (the scripts' grid), T = 300, around transition.steady_state's point.
  (a) aiy_ssj_jacobian (host entry: staging and read-back included), and the device time of its
      four stages from events recorded as they are dispatched;
  (b) the same Jacobians by brute force: 2T + 1 price paths through aiy_transition_batch, in one
      call (their period policies, 2T + 1 times T·N·Na doubles, stay resident), then the
      one-sided differences on the host;
  (c) aiyagari_transition (damp = 0.5) against aiyagari_transition_newton to tol = 1e-6 for 1, 16
      and 256 AR(1) TFP shocks: rounds and wall time, the Newton leg with its Jacobian's time.
Per variant: a warm-up, then the median wall time of `repeats` runs (host clock around work that
ends in a synchronise).  The shader clock level is read before and after.
"""
import argparse
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from tests.conftest import load_pkg  # noqa: E402
from tools.transition_ab import clock_level, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--T", type=int, default=300)
    ap.add_argument("--C", type=int, nargs="*", default=[1, 16, 256])
    ap.add_argument("--h", type=float, default=1e-4)
    args = ap.parse_args()
    import torch
    pkg = load_pkg()
    cb = pkg.calibration
    N, Na, T, h = 7, 400, args.T, args.h
    cal = cb.aiyagari(Na=Na)
    t0 = time.perf_counter()
    ss = pkg.steady_state(cal)
    t_ss = time.perf_counter() - t0
    clk0 = clock_level()
    lines = [f"ssj_ab: {torch.cuda.get_device_name(0)}, N = {N}, Na = {Na}, T = {T}, h = {h:g}, "
             f"steady state r = {ss['r']:.6f}, K = {ss['K']:.6f} ({t_ss:.2f} s); median of "
             f"{args.repeats} after a warm-up, host clock"]
    res = {}
    print(lines[0], file=sys.stderr, flush=True)  # (progress; the report is printed at the end)

    # (a) the fake-news Jacobian
    stages = []

    def fake_news():
        ms = np.zeros(4)
        res["jac"] = pkg.jacobian(ss, T, h, stage_ms=ms)
        stages.append(ms)
    ma = timed(fake_news, args.repeats)
    assert res["jac"]["status"] == (0, 0)
    sm = np.median(np.stack(stages[1:]), axis=0)
    lines += [f"(a) aiy_ssj_jacobian: {ma[0]:.3f} ms [{ma[1]:.3f}..{ma[2]:.3f}]; device time of "
              f"the stages: backward (3 paths) {sm[0]:.3f} ms, forward (3T one-step paths) "
              f"{sm[1]:.3f} ms, expectation {sm[2]:.3f} ms, contraction + diagonals {sm[3]:.3f} ms",
              f"    expectation pass: {1e3 * sm[2] / max(T - 1, 1):.2f} us per period (the forward "
              f"pass: 13-14 us per period, profiles/transition_ab.txt)"]

    # (b) brute force: the base path, T paths with r_s + h, T paths with w_s + h
    r = np.full((2 * T + 1, T + 1), float(ss["r"]))
    w = np.full((2 * T + 1, T), float(ss["w"]))
    for q in range(T):
        r[1 + q, q] += h
        w[1 + T + q, q] += h
    targs = (r, w, ss["policy_c"], ss["lam"], cal["a_grid"], cal["s"], cal["P"], cal["beta"],
             cal["sigma"], cal["amin"])

    def brute():
        K, st, _ = pkg.transition_batch(*targs)
        assert (st == 0).all()
        res["Jb_r"] = ((K[1:T + 1, 1:] - K[0, 1:]) / h).T
        res["Jb_w"] = ((K[T + 1:, 1:] - K[0, 1:]) / h).T
    mb = timed(brute, args.repeats)
    err = {x: np.max(np.abs(res["jac"]["J_" + x] - res["Jb_" + x])) / np.max(np.abs(res["Jb_" + x]))
           for x in ("r", "w")}
    gb = (2 * T + 1) * T * N * Na * 8 / 2 ** 30
    lines += [f"(b) brute force, {2 * T + 1} paths in one aiy_transition_batch call ({gb:.2f} GiB of "
              f"period policies resident): {mb[0]:.3f} ms [{mb[1]:.3f}..{mb[2]:.3f}]   "
              f"x{mb[0] / ma[0]:.2f} of (a)",
              f"    max |J - J_brute| / max |J_brute|: {err['r']:.3e} (r), {err['w']:.3e} (w)"]

    # (c) the drivers
    lines.append("(c) C AR(1) shocks Z = 1 + e·rho^t (e in [-0.01, 0.01], rho in [0.5, 0.9]) to "
                 "tol = 1e-6: damped (damp = 0.5) rounds min..max, ms | Newton rounds min..max, ms "
                 "(its Jacobian included) | damped/Newton | max |K_newton - K_damped|")
    q = np.arange(T)
    for C in args.C:
        e = np.linspace(-0.01, 0.01, C + 1)[1:] if C > 1 else np.array([-0.01])
        e = np.where(e == 0, 0.005, e)
        rho = np.linspace(0.5, 0.9, C) if C > 1 else np.array([0.8])
        Z = 1 + e[:, None] * rho[:, None] ** q[None, :]

        def damped():
            res["D"] = pkg.aiyagari_transition(ss, Z, T, damp=0.5, tol=1e-6, max_iter=200)

        def newton():
            res["N"] = pkg.aiyagari_transition_newton(ss, Z, T, tol=1e-6)
        md = timed(damped, args.repeats)
        mn = timed(newton, args.repeats)
        D, Nw = res["D"], res["N"]
        assert (D["status"] == 0).all() and (Nw["status"] == 0).all()
        assert (D["resid"] < 1e-6).all() and (Nw["resid"] < 1e-6).all()
        lines.append(f"  C = {C:3d}: damped {D['rounds'].min()}..{D['rounds'].max()} rounds, "
                     f"{md[0]:9.2f} ms [{md[1]:.2f}..{md[2]:.2f}] | Newton {Nw['rounds'].min()}.."
                     f"{Nw['rounds'].max()} rounds, {mn[0]:9.2f} ms [{mn[1]:.2f}..{mn[2]:.2f}] | "
                     f"x{md[0] / mn[0]:.2f} | {np.max(np.abs(D['K'] - Nw['K'])):.2e}")
    lines.append(f"shader clock level before: {clk0}, after: {clock_level()}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text)


if __name__ == "__main__":
    main()
