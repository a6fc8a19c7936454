"""The speculative batch loop (csrc/spec_loop.hpp) without a GPU: a stand-alone host program
(tests/cpp/spec_loop_main.cpp, AddressSanitizer + UBSan) drives it with fake callables serving a
given distance sequence and prints every call; `restate` below is the rule written down a second
time ("A2 solve loop"), independent of the header.  Besides equality of the two:
the loop stops at the first step that meets the predicate, issues no step beyond max_iter, never
holds more than two unread batches, and sizes batches the same with and without the `tol > 0`
guard the histogram solve once had."""
import math

import pytest

from tests.test_host_layer_cpu import _build

NAN, INF = math.nan, math.inf
PRED = [lambda d, tol: d < tol, lambda d, tol: not (d > tol)]  # VFI / histogram, EGM


def _log(x):  # C's log on the whole line
    return NAN if x != x or x < 0 else -INF if x == 0 else math.log(x)


def _ceil(x):
    return x if x != x or abs(x) == INF else float(math.ceil(x))


def restate(M, max_iter, tol, pred, ds, step_err=0, read_err=0, guard=False):
    """-> (calls, [rc, g*, stop, enq, any, last d])"""
    calls, q = [], []
    enq = hb = stop = rc = 0
    dp = dl = last = NAN
    seen = False

    def enqueue():
        nonlocal enq, hb
        m = M
        if dl == dl and dp == dp and 0 < dl < dp and (tol > 0 or not guard):
            need = _ceil(_log(tol / dl) / _log(dl / dp))
            ahead = sum(b[1] for b in q)
            if need >= 1 and need - ahead < m:
                m = int(max(1.0, need - ahead))
        m = min(max(m, 1), max_iter - enq)
        for g in range(enq + 1, enq + m + 1):
            calls.append(f"S{g}")
            if g == step_err:
                return 7
        calls.append(f"F{hb}")
        q.append((enq, m, hb))
        hb ^= 1
        enq += m
        return 0

    if max_iter > 0:
        rc = enqueue()
    while rc == 0 and q:
        if len(q) < 2 and enq < max_iter:
            rc = enqueue()
            if rc:
                break
        s0, m, h = q[0]
        calls.append(f"W{h}")
        for g in range(s0 + 1, s0 + m + 1):
            calls.append(f"R{g}")
            if g == read_err:
                rc = 9
                break
            dp, dl, last, seen = dl, ds[g - 1], ds[g - 1], True
            if PRED[pred](dl, tol):
                stop = g
                break
        q.pop(0)
        if rc or stop:
            break
    return calls, [rc, stop if stop else enq, stop, enq, int(seen), last]


def geo(rho, n, d0=1.0):
    return [d0 * rho ** g for g in range(n)]


def cases():
    """[(name, M, max_iter, tol, pred, ds, step_err, read_err)]"""
    out = []
    for M in (1, 2, 16):
        out.append((f"exact power M={M}", M, 1000, 2.0 ** -20, 0, geo(0.5, 1000), 0, 0))
        out.append((f"rho 0.9 M={M}", M, 1000, 1e-5, 0, geo(0.9, 1000), 0, 0))
        out.append((f"rho 0.9 egm M={M}", M, 1000, 1e-5, 1, geo(0.9, 1000), 0, 0))
        out.append((f"first step M={M}", M, 1000, 1e-5, 0, [1e-9] * 1000, 0, 0))
        for mi in (1, M - 1, M, M + 1, 2 * M + 1, 0):
            out.append((f"max_iter {mi} slow M={M}", M, mi, 1e-5, 0, geo(0.99, 64), 0, 0))
            out.append((f"max_iter {mi} fast M={M}", M, mi, 1e-5, 1, geo(0.5, 64), 0, 0))
        out.append((f"increasing M={M}", M, 50, 1e-5, 0, [1 + 0.1 * g for g in range(50)], 0, 0))
        out.append((f"constant M={M}", M, 50, 1e-5, 1, [0.5] * 50, 0, 0))
    for pred in (0, 1):
        out.append((f"zero d pred {pred}", 16, 100, 1e-5, pred, [1.0, 0.5] + [0.0] * 98, 0, 0))
        out.append((f"all zero, tol 0, pred {pred}", 4, 20, 0.0, pred, [0.0] * 20, 0, 0))
        nan_mid = [NAN if g in (4, 19) else d for g, d in enumerate(geo(0.9, 300))]
        out.append((f"nan mid pred {pred}", 16, 300, 1e-5, pred, nan_mid, 0, 0))
        out.append((f"d == tol pred {pred}", 16, 100, 0.25, pred, geo(0.5, 100), 0, 0))
        for tol in (0.0, -1.0, NAN):
            for rho in (0.5, 0.9):
                out.append((f"tol {tol} rho {rho} pred {pred}", 16, 100, tol, pred,
                            geo(rho, 100), 0, 0))
    for at in (5, 20):
        out.append((f"step error at {at}", 16, 1000, 1e-5, 0, geo(0.9, 1000), at, 0))
    for at in (3, 18):
        out.append((f"read error at {at}", 16, 1000, 1e-5, 1, geo(0.9, 1000), 0, at))
    return out


def _num(x):
    return "nan" if x != x else repr(float(x))


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """Every case through the program, once: [(case, calls, result)]."""
    import subprocess
    exe = _build(tmp_path_factory.mktemp("spec_loop"), "spec_loop_main.cpp")
    cs = cases()
    lines = [str(len(cs))]
    for _, M, mi, tol, pred, ds, se, re_ in cs:
        lines.append(f"{M} {mi} {_num(tol)} {pred} {se} {re_} {len(ds)}")
        lines.append(" ".join(_num(d) for d in ds))
    r = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0 and "FAILED" not in r.stdout, (r.stdout[-1500:], r.stderr[-1500:])
    outs = r.stdout.strip("\n").split("\n")
    assert len(outs) == len(cs)
    got = []
    for c, o in zip(cs, outs):
        calls, res = o.split("=")
        res = res.split()
        got.append((c, calls.split(), [int(v) for v in res[:5]] + [float(res[5])]))
    return got


def _same(a, b):
    return a[:5] == b[:5] and (a[5] == b[5] or (a[5] != a[5] and b[5] != b[5]))


def test_cases_cover_the_rule():
    cs = cases()
    r = {c[0]: restate(*c[1:]) for c in cs}
    batches = lambda calls: " ".join(calls).split("F")
    # the exact-power case shortens a batch below M; errors land mid-batch and in a later batch
    assert any(0 < b.count("S") < 16 for b in batches(r["exact power M=16"][0])[1:-1])
    assert r["step error at 5"][1][0] == 7 and r["step error at 20"][1][0] == 7
    assert r["read error at 3"][1][0] == 9 and r["read error at 18"][1][0] == 9
    assert r["d == tol pred 0"][1][2] == 4 and r["d == tol pred 1"][1][2] == 3
    assert r["nan mid pred 0"][1][2] > 20 and r["nan mid pred 1"][1][2] == 5
    assert r["max_iter 0 slow M=16"][0] == [] and r["max_iter 17 slow M=16"][1][3] == 17
    mids = [b.count("S") for b in batches(r["rho 0.9 M=16"][0])[1:-1]]
    assert any(1 < m < 16 for m in mids)  # and a batch cut to the steps the decay still needs


def test_loop_equals_the_restated_rule(runs):
    for c, calls, res in runs:
        want_calls, want = restate(*c[1:])
        assert calls == want_calls, c[0]
        assert _same(res, want), (c[0], res, want)


def test_guard_on_tol_never_mattered(runs):
    """tol <= 0 or NaN: the schedule with the histogram solve's former `tol > 0` guard is the
    schedule without it (and the loop's)."""
    n = 0
    for c, calls, res in runs:
        if not c[3] > 0:
            want_calls, want = restate(*c[1:], guard=True)
            assert calls == want_calls and _same(res, want), c[0]
            n += 1
    assert n >= 12


def test_stop_bound_and_depth(runs):
    for c, calls, res in runs:
        name, M, max_iter, tol, pred, ds, step_err, read_err = c
        steps = [int(t[1:]) for t in calls if t[0] == "S"]
        assert steps == list(range(1, len(steps) + 1)) and len(steps) <= max(max_iter, 0), name
        unread = 0
        for t in calls:
            unread += (t[0] == "F") - (t[0] == "W")
            assert 0 <= unread <= 2, name
        batch = [b.count("S") for b in " ".join(calls).split("F")[:-1]]
        assert all(1 <= m <= M for m in batch), name
        if step_err or read_err:
            continue
        first = next((g for g in range(1, max_iter + 1) if PRED[pred](ds[g - 1], tol)), 0)
        rc, g, stop, enq, seen, d = res
        assert rc == 0 and stop == first and g == (first or max(max_iter, 0)), name
        assert enq == len(steps) and seen == (max_iter > 0), name
        if seen:
            assert _same([0] * 5 + [d], [0] * 5 + [ds[g - 1]]), name
