"""A/B of the labour economy's transition passes, Jacobian and drivers (one MI355X).

    python tools/labor_transition_ab.py [--out profiles/labor_transition_ab.txt] [--repeats 5]
                                        [--T 300]

Workload: N = 7, Na = 400 on the labour script's calibration (rho = .6, sigma_e = .2,
phi = theta = 1), T = 300 periods.
 1. Passes, on a constant price path (r = 0.03, its wage), every path from one terminal policy
    and one λ₀, for C = 1, 16, 64, 256:
      (a) aiy_labor_transition_batch: the backward and the forward pass with hours, one workgroup
          per path each, the period policies staying on the device (host entry: staging and
          read-back of K and H included);
      (b) the per-step path with the same step count: per path T chained aiy_egm_step_dev calls
          (labor = 1), then T chained aiy_dist_update_dev calls (device tier, one workspace).
    K[T] of (a) is checked against Σ λ_T·a of (b)'s last λ (1e-12 relative) and the policies of the
    two bit for bit.
 2. Jacobian, around steady_state_labor's point: aiy_ssj_jacobian_labor (four T × T matrices)
    against the brute force it replaces — 1 + 2T whole transitions in ONE
    aiy_labor_transition_batch call (one-sided differences in every r_s and w_s).
 3. Drivers, 1 and 16 TFP shocks (AR(0.9), sizes spread over ±1 %), tol = 1e-8: rounds and wall
    time of aiyagari_labor_transition_newton (the Jacobian given; its time is item 2's) against
    aiyagari_labor_transition at its default damp.
Per timed variant: a warm-up, then the median wall time of `repeats` runs (host clock around work
that ends in a synchronise); the drivers are run once after a warm-up of the passes.  The shader
clock level is read before and after.
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
    ap.add_argument("--shocks", type=int, nargs="*", default=[1, 16])
    args = ap.parse_args()
    import torch
    pkg = load_pkg()
    cb = pkg.calibration
    N, Na, T = 7, 400, args.T
    phi = theta = 1.0
    cal = cb.aiyagari(Na=Na, rho=0.6, sigma_e=0.2)
    a, s, P = cal["a_grid"], cal["s"], cal["P"]
    r0 = 0.03
    w0 = cb.wage(r0, cal["alpha"], cal["delta"])
    guess = np.tile((1 + r0) * a + w0 * np.mean(s), (N, 1))
    pcT = np.ascontiguousarray(pkg.labor_egm_solve(guess.T, a, s, P, r0, w0, cal["beta"],
                                                   cal["sigma"], phi, theta, cal["amin"],
                                                   max_iter=40)["policy_c"].T)
    lam0 = np.full((N, Na), 1.0 / (N * Na))
    dev = torch.device("cuda", 0)
    t = lambda x: torch.as_tensor(np.ascontiguousarray(x, dtype=np.float64), device=dev)
    a_t, s_t, P_t, pc_t, l0_t = t(a), t(s), t(P), t(pcT), t(lam0)
    ws = pkg.Workspace(N, Na)
    pk = torch.zeros((T, N, Na), dtype=torch.float64, device=dev)
    pl = torch.zeros((T, N, Na), dtype=torch.float64, device=dev)
    bufs = [torch.zeros((N, Na), dtype=torch.float64, device=dev) for _ in range(2)]
    res = {}

    def per_step_path():
        cur = pc_t
        for q in range(T):  # period T − 1 − q
            nxt = bufs[q & 1]
            pkg.egm_step_dev(ws, cur, a_t, s_t, P_t, r0, w0, cal["beta"], cal["sigma"],
                             cal["amin"], nxt, pk[T - 1 - q], labor=True, phi=phi, theta=theta,
                             policy_l=pl[T - 1 - q])
            cur = nxt
        lam = l0_t
        for q in range(T):
            out = bufs[q & 1]
            pkg.dist_update_dev(ws, lam, a_t, P_t, out, policy_k=pk[q])
            lam = out
        torch.cuda.synchronize()
        res["lam"] = lam

    clk0 = clock_level()
    lines = [f"labor_transition_ab: {torch.cuda.get_device_name(0)}, N = {N}, Na = {Na}, T = {T}; "
             f"median of {args.repeats} after a warm-up, host clock",
             f"1. passes on a constant path r = {r0}",
             "C, (a) aiy_labor_transition_batch ms [min..max], (b) per-step path ms [min..max], "
             "(b)/(a), us per period and pass (a) / (b)"]
    for C in args.C:
        rr, ww = np.full((C, T + 1), r0), np.full((C, T), w0)
        targs = (rr, ww, pcT, lam0, a, s, P, cal["beta"], cal["sigma"], phi, theta, cal["amin"])

        def batched():
            res["K"], res["H"], res["st"], _ = pkg.labor_transition_batch(*targs)

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
    B = pkg.labor_egm_backward_batch(np.full((1, T + 1), r0), np.full((1, T), w0), pcT, a, s, P,
                                     cal["beta"], cal["sigma"], phi, theta, cal["amin"],
                                     want_pc=False)
    per_step_path()
    assert np.array_equal(B["policy_k"][0], pk.cpu().numpy())
    assert np.array_equal(B["policy_l"][0], pl.cpu().numpy())
    lines.append("   policies (k and l) of (a) and (b) equal bit for bit")
    ws.close()

    # 2. the Jacobian against brute force
    t0 = time.perf_counter()
    ss = pkg.steady_state_labor(cal, phi, theta)
    t_ss = time.perf_counter() - t0
    kd = (cal["alpha"] / (ss["r"] + cal["delta"])) ** (1 / (1 - cal["alpha"]))
    lines.append(f"2. steady state: r = {ss['r']:.10f}, K = {ss['K']:.8f}, H = {ss['H']:.8f}, "
                 f"K - H k_d(r) = {ss['K'] - ss['H'] * kd:.2e}, {t_ss:.2f} s")
    h = 1e-4
    stage = np.zeros(4)
    jac = {}

    def fake_news():
        jac.update(pkg.jacobian_labor(ss, T, h, stage_ms=stage))
    rb = np.full((1 + 2 * T, T + 1), ss["r"])
    wb = np.full((1 + 2 * T, T), ss["w"])
    for q in range(T):
        rb[1 + q, q] += h
        wb[1 + T + q, q] += h
    bf = {}

    def brute():
        bf["K"], bf["H"], bf["st"], _ = pkg.labor_transition_batch(
            rb, wb, ss["policy_c"], ss["lam"], a, s, P, cal["beta"], cal["sigma"], phi, theta,
            cal["amin"])
    mj = timed(fake_news, args.repeats)
    mbf = timed(brute, args.repeats)
    assert jac["status"] == (0, 0) and (bf["st"] == 0).all()
    JK = ((bf["K"][1:, 1:] - bf["K"][:1, 1:]) / h).reshape(2, T, T).transpose(0, 2, 1)
    JH = ((bf["H"][1:] - bf["H"][:1]) / h).reshape(2, T, T).transpose(0, 2, 1)
    rel = lambda X, Y: np.max(np.abs(X - Y)) / np.max(np.abs(Y))
    lines += [f"   aiy_ssj_jacobian_labor {mj[0]:9.3f} ms [{mj[1]:.3f}..{mj[2]:.3f}] (device stages "
              f"backward {stage[0]:.3f}, forward {stage[1]:.3f}, expectations {stage[2]:.3f}, "
              f"contractions {stage[3]:.3f} ms)",
              f"   brute force, {1 + 2 * T} paths in one aiy_labor_transition_batch call "
              f"{mbf[0]:9.3f} ms [{mbf[1]:.3f}..{mbf[2]:.3f}]   x{mbf[0] / mj[0]:7.2f}",
              f"   max relative difference (the one-sided difference's O(h)): J_Kr "
              f"{rel(jac['J_Kr'], JK[0]):.2e}, J_Kw {rel(jac['J_Kw'], JK[1]):.2e}, J_Hr "
              f"{rel(jac['J_Hr'], JH[0]):.2e}, J_Hw {rel(jac['J_Hw'], JH[1]):.2e}"]
    M = pkg.transition._labor_newton_matrix(ss, jac) + np.eye(T)
    lines.append(f"   spectral radius of M = d kappa_supply / d kappa: "
                 f"{np.max(np.abs(np.linalg.eigvals(M))):.2f}")

    # 3. the drivers
    lines.append("3. drivers, tol = 1e-8: shocks, Newton rounds (max) and s, damped rounds (max) "
                 "and s, max |K_newton - K_damped|")
    q = np.arange(T)
    for n_s in args.shocks:
        size = np.array([0.01]) if n_s == 1 else np.linspace(-0.01, 0.01, n_s)
        Z = 1 + size[:, None] * 0.9 ** q[None, :]
        t0 = time.perf_counter()
        Nw = pkg.aiyagari_labor_transition_newton(ss, Z, T, jac=jac, tol=1e-8)
        t_n = time.perf_counter() - t0
        t0 = time.perf_counter()
        Dm = pkg.aiyagari_labor_transition(ss, Z, T, tol=1e-8)
        t_d = time.perf_counter() - t0
        okn = bool((Nw["status"] == 0).all() and (Nw["resid"] < 1e-8).all())
        okd = bool((Dm["status"] == 0).all() and (Dm["resid"] < 1e-8).all())
        lines.append(f"   {n_s:3d}: Newton {int(Nw['rounds'].max()):4d} rounds {t_n:8.3f} s"
                     f"{'' if okn else ' (NOT converged)'}   damped {int(Dm['rounds'].max()):4d} "
                     f"rounds {t_d:8.3f} s{'' if okd else ' (NOT converged)'}   x{t_d / t_n:7.2f}   "
                     f"{np.max(np.abs(Nw['K'] - Dm['K'])):.2e}")
    lines.append(f"shader clock level before: {clk0}, after: {clock_level()}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text)


if __name__ == "__main__":
    main()
