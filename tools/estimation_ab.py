"""A/B of the batched likelihood (one MI355X).

    python tools/estimation_ab.py [--out profiles/estimation_ab.txt] [--repeats 5] [--T 300]

Workload: N = 7, Na = 400, T = 300 periods, the three observables (Y, C, K), L = 60 observed
periods (n = 180) simulated from the MA of an AR(1) TFP shock (rho = 0.9, sigma = 0.007) with
measurement error of 1 % of each observable's variance.  The Jacobians come from
steady_state + jacobian + ge_jacobians, once.
 1. C = 1, 64, 1024, 4096 candidate (rho, sigma) pairs:
      (a) ONE ar1_loglik call: two launches behind the host entries (staging of G [3][T][T] and of
          m, and the read-backs, included);
      (b) the same candidates one ar1_loglik call after another;
      (c) the C reference (tests/support/estimation_ref.c) and (d) numpy Cholesky on the dense V,
          both on the host over min(C, 64) candidates, reported per candidate.
    (a)'s log-likelihoods are checked against (b)'s bit for bit and against (d)'s to 1e-9.
 2. The two kernels alone on device tensors (ma_batch_dev, loglik_batch_dev), per C.
 3. One ar1_mle (width 16, 6 rounds: 6 calls of 256 candidates).
Per timed variant: a warm-up, then the median wall time of `repeats` runs (host clock around work
that ends in a synchronise).  The shader clock level is read before and after.
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
from tests import estimation_ref as er  # noqa: E402
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


def cholesky_loglik(G, y, rho, sigma, me):
    """numpy on the host, one candidate after another: matmul, lag sums, dense V, Cholesky."""
    T, L = G.shape[1], y.shape[0]
    yv = y.ravel()
    out = np.empty(len(rho))
    for c in range(len(rho)):
        m = G @ (sigma[c] * rho[c] ** np.arange(T))
        Gam = np.stack([m[:, l:] @ m[:, :T - l].T for l in range(L)])
        Lc = np.linalg.cholesky(er.dense_V(Gam, me))
        z = np.linalg.solve(Lc, yv)
        out[c] = -0.5 * (yv.size * np.log(2 * np.pi) + 2 * np.sum(np.log(np.diag(Lc))) + z @ z)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--T", type=int, default=300)
    ap.add_argument("--Na", type=int, default=400)
    ap.add_argument("--L", type=int, default=60)
    ap.add_argument("--C", type=int, nargs="*", default=[1, 64, 1024, 4096])
    args = ap.parse_args()
    import torch
    pkg = load_pkg()
    est = pkg.estimation
    T, L, outs = args.T, args.L, ("Y", "C", "K")
    cal = pkg.calibration.aiyagari(Na=args.Na)
    t0 = time.perf_counter()
    ss = pkg.steady_state(cal)
    t_ss = time.perf_counter() - t0
    t0 = time.perf_counter()
    jac = pkg.jacobian(ss, T)
    t_jac = time.perf_counter() - t0
    assert jac["status"] == (0, 0)
    t0 = time.perf_counter()
    G = est.ge_jacobians(ss, jac, outs)
    t_ge = time.perf_counter() - t0
    m0 = er.ma_batch(G, est.ar1_ma([0.9], [0.007], T))[0]
    me = 1e-2 * np.einsum("ot,ot->o", m0, m0)
    y = er.simulate(m0, L, me, 2021)
    n_o, n = len(outs), len(outs) * L
    dev = torch.device("cuda", 0)
    f64 = dict(dtype=torch.float64, device=dev)
    clk0 = clock_level()
    lines = [f"estimation_ab: {torch.cuda.get_device_name(0)}, N = {cal['N']}, Na = {args.Na}, "
             f"T = {T}, observables {outs}, L = {L} (n = {n}); median of {args.repeats} after a "
             f"warm-up, host clock",
             f"set-up, once (first calls, not warmed): steady_state {t_ss:.2f} s, jacobian "
             f"{1e3 * t_jac:.1f} ms, ge_jacobians (host, one {T} x {T} solve) {1e3 * t_ge:.1f} ms",
             "1. C, (a) one ar1_loglik call ms [min..max], (b) C calls of one candidate ms, (b)/(a), "
             "us per candidate (a); host per candidate: (c) C reference ms, (d) numpy Cholesky ms"]
    rng = np.random.default_rng(1)
    res, dev_lines = {}, []
    for C in args.C:
        rho, sig = rng.uniform(0.5, 0.98, C), rng.uniform(0.003, 0.02, C)

        def batched():
            res["a"] = est.ar1_loglik(G, y, rho, sig, me)

        def separate():
            res["b"] = np.array([est.ar1_loglik(G, y, rho[c:c + 1], sig[c:c + 1], me)["loglik"][0]
                                 for c in range(C)])
        ch = min(C, 64)

        def cref():
            res["c"] = est.ar1_loglik(G, y, rho[:ch], sig[:ch], me, backend=er.BACKEND)["loglik"]

        def chol():
            res["d"] = cholesky_loglik(G, y, rho[:ch], sig[:ch], me)
        ta, tb = timed(batched, args.repeats), timed(separate, args.repeats)
        tc, td = timed(cref, args.repeats), timed(chol, args.repeats)
        A = res["a"]
        assert (A["status"] == 0).all()
        assert np.array_equal(A["loglik"], res["b"]), "a candidate depends on its batch"
        assert np.max(np.abs(A["loglik"][:ch] - res["d"]) / np.abs(res["d"])) <= 1e-9
        assert np.max(np.abs(A["loglik"][:ch] - res["c"]) / np.abs(res["c"])) <= 1e-9
        lines.append(f"  C = {C:4d}: (a) {ta[0]:9.3f} [{ta[1]:.3f}..{ta[2]:.3f}]   (b) {tb[0]:10.3f} "
                     f"[{tb[1]:.3f}..{tb[2]:.3f}]   x{tb[0] / ta[0]:7.2f}   {1e3 * ta[0] / C:8.2f} us   "
                     f"(c) {tc[0] / ch:7.3f}   (d) {td[0] / ch:7.3f}")
        # 2. the kernels alone, on device tensors
        G_t, y_t, me_t = (torch.as_tensor(x, **f64) for x in (G, y, me))
        dZ_t = torch.as_tensor(est.ar1_ma(rho, sig, T), **f64)
        m_t = torch.empty((C, n_o, T), **f64)
        ll_t = torch.empty(C, **f64)
        st_t = torch.empty(C, dtype=torch.int32, device=dev)
        fl_t = torch.empty(C, dtype=torch.int32, device=dev)

        def k_ma():
            est.ma_batch_dev(G_t, dZ_t, m_t)
            torch.cuda.synchronize()

        def k_lik():
            est.loglik_batch_dev(m_t, y_t, me_t, ll_t, st_t, fl_t)
            torch.cuda.synchronize()
        tm, tl = timed(k_ma, args.repeats), timed(k_lik, args.repeats)
        assert np.array_equal(ll_t.cpu().numpy(), A["loglik"])
        tot = tm[0] + tl[0]
        dev_lines.append(f"  C = {C:4d}: MA {tm[0]:8.3f} ms ({100 * tm[0] / tot:4.1f} %)   likelihood "
                         f"{tl[0]:8.3f} ms ({100 * tl[0] / tot:4.1f} %)   sum {tot:8.3f} ms = "
                         f"{100 * tot / ta[0]:5.1f} % of (a)   {1e3 * tl[0] / C:8.2f} us per "
                         f"candidate (likelihood)")
    lines.append("2. the two kernels alone on device tensors (launch + synchronise), shares of "
                 "their sum")
    lines += dev_lines
    mle = {}

    def run_mle():
        mle.update(est.ar1_mle(G, y, me, (0.3, 0.99), (0.001, 0.03), width=16, rounds=6))
    tmle = timed(run_mle, args.repeats)
    lines.append(f"3. ar1_mle, width 16, 6 rounds ({int(mle['evals'].sum())} evaluations in "
                 f"{len(mle['evals'])} calls): {tmle[0]:.3f} ms [{tmle[1]:.3f}..{tmle[2]:.3f}]; "
                 f"rho = {mle['rho']:.6f}, sigma = {mle['sigma']:.6f} (data: 0.9, 0.007), loglik "
                 f"{mle['loglik']:.6f}")
    lines.append(f"shader clock level before: {clk0}, after: {clock_level()}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text)


if __name__ == "__main__":
    main()
