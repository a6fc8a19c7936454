"""CPU census of tests/ks_hist_adv_cases.py: the restatement alone reaches every branch the GPU
parity tests (tests/test_ks_hist_adversarial_gpu.py) are meant to pin, and agrees with the
independent long-double reference.  These are the conditions that keep those comparisons from
passing vacuously, not measurements: if one fails, the inputs change, not the condition.  The
defect table at the end restates the kernel with one defect at a time and counts the cases on
which the outputs change — the evidence that the bit-for-bit GPU comparison would notice the
same defect in csrc/ks_hist_kernels.hip."""
import numpy as np
import pytest

from tests import ks_hist_adv_cases as cases
from tests import ks_hist_cases as base
from tests import ks_hist_ref as ref

ALL = cases.names()


# ------------------------------------------------------------------ every case


@pytest.mark.parametrize("name", ALL)
def test_outputs_are_finite_and_mass_is_conserved(name):
    c = cases.get(name)
    K_ts, lam, slow = cases.restatement(name)
    T, M = c["zi"].shape
    assert K_ts.shape == (T, M) and lam.shape == (M, 2, c["x"].size) and slow.shape == (M,)
    assert np.all(np.isfinite(K_ts)) and np.all(np.isfinite(lam)) and np.all(lam >= 0)
    start = np.broadcast_to(c["lam0"], lam.shape).sum((1, 2))
    assert np.abs(lam.sum((1, 2)) - start).max() <= 1e-12
    assert cases.fits(*cases.shape(c))
    assert 6 <= T <= 12 or name in ("shock-many", "shock-T1100")


def test_tolerance_is_eight_times_the_recorded_maxima_and_under_the_ceiling():
    assert cases.TOL_REL_K == 8 * cases.MEASURED_MAX_REL_K <= cases.TOL_CEILING
    assert cases.TOL_ABS_LAM == 8 * cases.MEASURED_MAX_ABS_LAM <= cases.TOL_CEILING
    assert cases.MEASURED_MAX_REL_K > 0 and cases.MEASURED_MAX_ABS_LAM > 0


@pytest.mark.parametrize("name", ALL)
def test_restatement_agrees_with_the_independent_reference(name):
    dK, dl = cases.differences(cases.restatement(name), cases.independent(name))
    print(name, "max rel dK", dK, "max abs dlam", dl)
    assert dK <= cases.TOL_REL_K and dl <= cases.TOL_ABS_LAM


def test_independent_reference_on_the_existing_cases():
    """The cases the kernel arrived with, at the same tolerance (T cut to 12 for the long ones)."""
    cs = [base.case(*s, seed=s[0] + s[3] + s[4]) for s in base.SHAPES]
    cs += [base.plateau_case(), base.slow_case()]
    for c in cs:
        c = dict(c, zi=c["zi"][:12])
        dK, dl = cases.differences(cases.restatement_of(c), cases.independent_of(c))
        assert dK <= cases.TOL_REL_K and dl <= cases.TOL_ABS_LAM, (c["x"].size, dK, dl)


# ------------------------------------------------------------------ thread map and LDS


def test_sweep_holds_every_listed_nx():
    want = {127, 128, 129, 160, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 1900}
    got = {cases.get(n)["x"].size for n in cases.names("sweep")}
    assert got == want
    for n in cases.names("sweep"):
        nx, nk, nK = cases.shape(cases.get(n))
        assert (nk, nK, cases.get(n)["zi"].shape[1]) == (100, 4, 2)
    # what the sizes are for: the block's threads against 2·nx, and the moment's stride
    thr = {nx: min(1024, max(256, (2 * nx + 63) & ~63)) for nx in want}
    assert {nx for nx in want if thr[nx] == 2 * nx} == {128, 160, 256, 512}
    assert {nx for nx in want if thr[nx] // nx == 0} == {1025, 1900}          # de == 0
    assert min(nx for nx in want if 2 * nx > thr[nx]) == 513                   # first strided walk
    assert [cases.FOLD % nx for nx in (255, 256, 257)] == [1, 0, 256]


def test_fit_rule_mirror_matches_the_library(pkg):
    """The mirror's verdict at the known points, and the library's own refusal of the same sizes
    (as test_fit_rule_admits_the_reference_size_and_names_itself reads it)."""
    import torch
    assert cases.lds_bytes(1000, 100, 4, False) == 84112
    assert cases.lds_bytes(1000, 100, 4, True) == 96912
    assert cases.fits(1000, 100, 4) and cases.kopt_in_lds(1000, 100, 4)
    assert cases.fits(1900, 100, 4) and not cases.kopt_in_lds(1900, 100, 4)
    assert cases.lds_bytes(1900, 100, 4, False) == 159712
    assert not cases.fits(2000, 100, 4)
    for nx in (1000, 1900, 2000):
        c = base.case(nx, 100, 4, 2, 1)
        if cases.fits(nx, 100, 4):
            if not torch.cuda.is_available():
                with pytest.raises(pkg.AiyError) as e:
                    pkg.ks_panel.ks_simulate_hist(c["k_opt"], c["k_grid"], c["K_grid"], c["x"],
                                                  c["zi"], c["lam0"], c["params"])
                assert e.value.status == "AIY_NO_DEVICE"
        else:
            with pytest.raises(pkg.AiyError) as e:
                pkg.ks_panel.ks_simulate_hist(c["k_opt"], c["k_grid"], c["K_grid"], c["x"],
                                              c["zi"], c["lam0"], c["params"])
            assert e.value.status == "AIY_BAD_SHAPE"


def test_lds_cases_sit_on_the_intended_side():
    got = {n: cases.instantiation(cases.get(n)) for n in cases.names("lds")}
    print(got)
    top = cases.largest_staged_nk(65, 4)
    assert top == 1236
    assert got[f"lds-nk{top}"][0] == "<true>" and got[f"lds-nk{top}"][1] > 64 * 1024
    assert got[f"lds-nk{top + 1}"][0] == "<false>"
    c = cases.get("lds-nk16400")
    assert c["k_grid"].size * c["K_grid"].size > 1 << 16 and got["lds-nk16400"][0] == "<false>"
    # ... and the 2^16 clause alone decides it: the bytes of a smaller k_opt at nK = 4 fit
    assert got["lds-nx1900"] == ("<false>", 159712) and 159712 > 64 * 1024
    for n in cases.names("lds"):
        assert cases.fits(*cases.shape(cases.get(n)))
    # both instantiations run with and without the attribute call over the whole set
    seen = {(i, b > 64 * 1024) for i, b in (cases.instantiation(c) for c in cases.all_cases())}
    assert seen == {("<true>", False), ("<true>", True), ("<false>", False), ("<false>", True)}


@pytest.mark.parametrize("name", cases.names("rows"))
def test_whole_row_cases_have_a_run_of_the_whole_row(name):
    c = cases.get(name)
    K_ts, _, slow = cases.restatement(name)
    assert not slow.any()
    nx = c["x"].size
    seen = set()
    for t in range(2):
        seen |= base.run_lengths(c, K_ts[t, 0], int(c["zi"][t, 0]))
    assert nx in seen
    assert -(-nx // ref.CHUNK) <= 64      # (the wave's single pass of 64 chunks)


# ------------------------------------------------------------------ the vote


@pytest.mark.parametrize("name", cases.names("vote"))
def test_vote_cases_have_the_expected_slow_counts(name):
    c = cases.get(name)
    _, _, slow = cases.restatement(name)
    want = cases.expected_slow(c)
    assert np.array_equal(slow, want) and list(want) == [4, 4, 8]
    zi = c["zi"][:-1]
    steps = {(int(a), int(b)) for m in range(zi.shape[1]) for a, b in zip(zi[:-1, m], zi[1:, m])}
    assert {(0, 1), (1, 0), (0, 0), (1, 1)} <= steps       # slow→fast, fast→slow, and repeats
    # the constructor delivers its keys: the restatement's keys are the intended ones
    for z in (0, 1):
        key, w = cases.keys_weights_at(c, 40.0, z)
        assert np.array_equal(key, c["keys"][2 * z:2 * z + 2])
        assert np.all((w > 0.2) & (w < 0.8))
    inv = [np.nonzero(np.diff(c["keys"][s]) < 0)[0] for s in range(4)]
    assert inv[2].size == 0 and inv[3].size == 0
    nx = c["x"].size
    kind = name.split("-")[1]
    if kind == "last1":
        assert inv[0].size == 0 and list(inv[1]) == [nx - 2]
    elif kind == "first0":
        assert list(inv[0]) == [0] and inv[1].size == 0
    elif kind == "both":
        assert list(inv[0]) == [0] and list(inv[1]) == [nx - 2]
    else:
        assert inv[0].size == 1 and inv[1].size == 0
        want_run = min(100, nx - 20)
        assert max(base.run_lengths(c, 40.0, 0)) >= want_run > ref.CHUNK
        assert nx == 64 or want_run > 2 * ref.CHUNK


@pytest.mark.parametrize("nx", cases.VOTE_NX)
@pytest.mark.parametrize("kind", cases.VOTE_KINDS)
def test_without_the_inversion_no_period_is_slow(nx, kind):
    c = cases.vote_case(nx, kind, inverted=False)
    assert not cases.restatement_of(c)[2].any()


def test_slow_path_runs_at_more_than_65_nodes():
    assert max(cases.VOTE_NX) > 1024 and sum(nx > 65 for nx in cases.VOTE_NX) >= 3


# ------------------------------------------------------------------ ties


def test_tie_cases_land_on_nodes():
    c = cases.get("tie-w0")
    nx = c["x"].size
    for z in (0, 1):
        key, w = cases.keys_weights_at(c, 40.0, z)
        assert np.count_nonzero(w == 0) >= 2 * (nx - 1)       # (the last source has tk = 1)
        assert np.array_equal(key[:, :-1], c["keys"][2 * z:2 * z + 2, :-1])
    c = cases.get("tie-top")
    for z in (0, 1):
        key, w = cases.keys_weights_at(c, 40.0, z)
        top = (key == nx - 2) & (w == 1)
        assert top.sum() == 2 * 40 and np.all(np.diff(key, axis=1) >= 0)
        inside = (key == nx - 2) & (w > 0) & (w < 1)
        assert np.all(inside[:, 80:])                         # after them, inside the last segment
    assert not cases.restatement("tie-top")[2].any()
    c = cases.get("tie-node-run")
    for z in (0, 1):
        key, w = cases.keys_weights_at(c, 40.0, z)
        assert np.array_equal(key, c["keys"][2 * z:2 * z + 2])
        assert np.all(w[:, 10:50] == 0) and np.all(w[:, 50:100] > 0.2)
        assert np.all(key[:, 50:100] == key[:, 10:11] + 1)
        assert 90 in base.run_lengths(c, 40.0, z)             # 40 terms of λ·0, then 50
    assert not cases.restatement("tie-node-run")[2].any()
    for name, j in (("tie-K-interior", 1), ("tie-K-last", 3)):
        c = cases.get(name)
        K_ts = cases.restatement(name)[0]
        assert np.all(K_ts[0] == cases.NODE_K) and c["K_grid"][j] == cases.NODE_K
        assert c["K_grid"].size == 4 and np.all(np.diff(c["K_grid"]) > 0)
        assert c["x"][39] == cases.NODE_K


def test_identity_policy_keeps_the_capital_marginal():
    c = cases.get("tie-identity")
    K_ts, lam, slow = cases.restatement("tie-identity")
    T, M = c["zi"].shape
    marg0 = np.broadcast_to(c["lam0"], lam.shape).sum(1)
    assert np.abs(lam.sum(1) - marg0).max() <= 1e-15 * T
    assert np.abs(K_ts / K_ts[0] - 1).max() <= 1e-14 and not slow.any()
    assert np.abs(lam[:, 1] - c["lam0"][:, 1]).max() > 1e-3      # the employment split does move


# ------------------------------------------------------------------ shocks, paths and λ


def test_shock_cases_cover_the_listed_paths():
    zi = cases.get("shock-starts")["zi"]
    assert zi[0, 0] == 1 and np.all(zi[:, 1] == 1) and np.all(zi[:, 2] == 0) and zi[0, 3] == 1
    many = cases.get("shock-many")
    assert many["zi"].shape == (4, 300) and cases.shape(many)[0] == 10
    assert len({many["lam0"][m].tobytes() for m in range(300)}) == 300
    assert 0 < many["zi"][0].sum() < 300
    K0 = cases.restatement("shock-many")[0][0]
    Kg = many["K_grid"]
    assert np.any(K0 < Kg[0]) and np.any(K0 > Kg[-1]) and np.any((K0 > Kg[0]) & (K0 < Kg[-1]))
    long = cases.get("shock-T1100")
    assert long["zi"].shape == (1100, 1) and cases.shape(long)[0] == 65
    K = cases.restatement("shock-T1100")[0]
    assert K.min() < long["K_grid"][0] and K.max() > long["K_grid"][-1]


def test_lam_cases_hold_what_they_name():
    z = cases.get("lam-zeros")["lam0"]
    assert np.all(z[:, :, :50] == 0) and np.all(z[:, :, 100:] == 0) and np.all(z[1, 1] == 0)
    assert np.all(z[0, :, 50:100] > 0)
    t = cases.get("lam-tiny")["lam0"]
    assert np.count_nonzero(t == 1e-300) > 500 and np.count_nonzero(t > 0.05) > 20
    assert np.all(t > 0)
    u = cases.get("lam-unnormalised")["lam0"]
    assert np.allclose(u.sum((1, 2)), 3.7)


# ------------------------------------------------------------------ defect table

DEFECTS = ("chunk_33", "chunks_reversed", "search_lt", "no_key_clamp", "vote_row0_only",
           "vote_skips_last_pair", "vote_skips_first_pair", "vote_never_cleared",
           "thr_transposed", "mix_roles_swapped", "moment_other_fold", "zi0_taken_as_0")
# cases the table runs: all but the two whose size is their whole point
TABLE = [n for n in ALL if n not in ("shock-many", "shock-T1100")]


def _moment(lam, x, defect):
    if defect != "moment_other_fold":
        return ref.moment(lam, x)
    nx = x.size
    prod = np.zeros(-(-2 * nx // ref.FOLD) * ref.FOLD)
    prod[:2 * nx] = lam.reshape(-1) * np.tile(x, 2)
    s = np.zeros(ref.FOLD)
    for row in prod.reshape(-1, ref.FOLD):
        s = s + row
    s = s.reshape(4, 64)
    h = 32
    while h >= 1:
        s = s.copy()
        s[:, :h] = s[:, :h] + s[:, h:2 * h]
        h //= 2
    q = s[:, 0]
    return (q[0] + q[1]) + (q[2] + q[3])


def _push_fast(lam_row, w_row, key_row, chunk, reverse):
    """ks_hist_ref.push_fast with the chunk length and the order of the chunk sums open."""
    nx = lam_row.size
    off = np.searchsorted(key_row, np.arange(nx + 1), side="left")
    up = lam_row * w_row
    dn = lam_row * (1 - w_row)
    out = np.zeros(nx)
    for k in range(nx):
        js, je = off[k], off[k + 1]
        jb = off[k - 1] if k else js
        terms = [up[j] if j < js else dn[j] for j in range(jb, je)]
        parts = []
        for b in range(0, len(terms), chunk):
            part = 0.0
            for v in terms[b:b + chunk]:
                part = part + v
            parts.append(part)
        if len(terms) <= chunk:
            out[k] = parts[0] if parts else 0.0
        else:
            total = 0.0
            for part in (parts[::-1] if reverse else parts):
                total = total + part
            out[k] = total
    return out


def _push_slow(lam_row, w_row, key_row):
    """ks_hist_ref.push_slow for keys up to nx − 1 (destination nx does not exist)."""
    nx = lam_row.size
    up = lam_row * w_row
    dn = lam_row * (1 - w_row)
    out = np.zeros(nx + 1)
    for j in range(nx):
        kk = key_row[j]
        out[kk + 1] = out[kk + 1] + up[j]
        out[kk] = out[kk] + dn[j]
    return out[:nx]


def _variant_path(c, zi, lam0, defect):
    k_opt, k_grid, K_grid, x = c["k_opt"], c["k_grid"], c["K_grid"], c["x"]
    thr = ref.thr_table(c["params"])
    nx = x.size
    side = "left" if defect == "search_lt" else "right"

    def seg(g, q, top=None):
        raw = np.searchsorted(g, q, side=side) - 1
        return np.clip(raw, 0, g.size - 2 if top is None else top)

    ik = seg(k_grid, x)
    tk = (x - k_grid[ik]) / (k_grid[ik + 1] - k_grid[ik])
    lam = np.array(lam0, np.float64, copy=True)
    T = len(zi)
    K_ts = np.zeros(T)
    slow = 0
    words = [0, 0]
    for t in range(T - 1):
        z, zn = int(zi[t]), int(zi[t + 1])
        if t == 0 and defect == "zi0_taken_as_0":
            z = 0
        K = _moment(lam, x, defect)
        K_ts[t] = K
        iK = int(seg(K_grid, np.array([K]))[0])
        tK = (K - K_grid[iK]) / (K_grid[iK + 1] - K_grid[iK])
        key = np.zeros((2, nx), np.int64)
        w = np.zeros((2, nx))
        for e in (0, 1):
            s = 2 * z + e
            f00 = k_opt[ik, iK, s]; f10 = k_opt[ik + 1, iK, s]
            f01 = k_opt[ik, iK + 1, s]; f11 = k_opt[ik + 1, iK + 1, s]
            f0 = f00 + tk * (f10 - f00)
            f1 = f01 + tk * (f11 - f01)
            kn = f0 + tK * (f1 - f0)
            kn = np.where(kn < x[0], x[0], kn)
            kn = np.where(kn > x[-1], x[-1], kn)
            key[e] = seg(x, kn, nx - 1 if defect == "no_key_clamp" else None)
            up = x[(key[e] + 1) % nx]      # (a read past the end wraps)
            w[e] = (kn - x[key[e]]) / (up - x[key[e]])
        # the vote: word t & 1, the other word cleared for the next period
        if defect != "vote_never_cleared":
            words[(t + 1) & 1] = 0
        for e in ((0,) if defect == "vote_row0_only" else (0, 1)):
            inv = key[e][:-1] > key[e][1:]
            if defect == "vote_skips_last_pair":
                inv = inv[:-1]
            if defect == "vote_skips_first_pair":
                inv = inv[1:]
            if inv.any():
                words[t & 1] = 1
        slow_period = bool(words[t & 1])
        slow += slow_period
        pushed = []
        for e in (0, 1):
            if slow_period:
                pushed.append(_push_slow(lam[e], w[e], key[e]))
            elif defect == "chunk_33":
                pushed.append(_push_fast(lam[e], w[e], key[e], 33, False))
            elif defect == "chunks_reversed":
                pushed.append(_push_fast(lam[e], w[e], key[e], ref.CHUNK, True))
            else:     # (on keys a defective vote let through, some finite answer: as the kernel)
                pushed.append(ref.push_fast(lam[e], w[e], key[e]))
        p = thr[z, zn] if defect == "thr_transposed" else thr[zn, z]
        new = np.zeros_like(lam)
        for en in (0, 1):
            if defect == "mix_roles_swapped":     # P(e | e') in place of P(e' | e)
                a0 = p[en]
                a1 = 1 - p[en]
            else:
                a0 = p[0] if en == 0 else 1 - p[0]
                a1 = p[1] if en == 0 else 1 - p[1]
            acc = np.zeros(nx)
            acc = acc + a0 * pushed[0]
            acc = acc + a1 * pushed[1]
            new[en] = acc
        lam = new
    K_ts[T - 1] = _moment(lam, x, defect)
    return K_ts, lam, slow


def _variant(c, defect):
    zi = c["zi"]
    T, M = zi.shape
    nx = c["x"].size
    lam0 = np.broadcast_to(c["lam0"], (M, 2, nx))
    K_ts = np.zeros((T, M))
    lam = np.zeros((M, 2, nx))
    slow = np.zeros(M, np.int64)
    for m in range(M):
        K_ts[:, m], lam[m], slow[m] = _variant_path(c, zi[:, m], lam0[m], defect)
    return K_ts, lam, slow


def _differs(got, want):
    return not all(np.array_equal(g, w) for g, w in zip(got, want))


@pytest.fixture(scope="module")
def defect_counts():
    counts = {}
    with np.errstate(all="ignore"):
        for d in DEFECTS:
            counts[d] = [n for n in TABLE
                         if _differs(_variant(cases.get(n), d), cases.restatement(n))]
    return counts


def test_restated_table_without_a_defect_is_the_restatement():
    for n in TABLE:
        assert not _differs(_variant(cases.get(n), None), cases.restatement(n)), n
    # the two open parameters of the fast path at the kernel's values, on the long runs
    for n in ("row-segment-1000", "vote-long-129"):
        c = cases.get(n)
        key, w = cases.keys_weights_at(c, 40.0, 1)
        lam = np.broadcast_to(c["lam0"], (c["zi"].shape[1], 2, c["x"].size))[0]
        for e in (0, 1):
            assert np.array_equal(_push_fast(lam[e], w[e], key[e], ref.CHUNK, False),
                                  ref.push_fast(lam[e], w[e], key[e]))


@pytest.mark.parametrize("defect", DEFECTS)
def test_defect_table(defect_counts, defect):
    """Every defect changes K_ts, λ or the slow count of at least one case.  Cases that differ,
    of the 52 the table runs (all but shock-many and shock-T1100), counted when the cases were
    written; the assertion is one case at least per defect:

        chunk length 33 instead of 32                     26 of 52
        chunk sums folded in reverse order                17 of 52
        x[mid] < q instead of <= in the segment searches  1 of 52
        no clamp of the lottery key to nx - 2             1 of 52
        the vote reads row 0 only                         4 of 52
        the vote skips the last pair of keys              4 of 52
        the vote skips the first pair of keys             4 of 52
        the vote's word is never cleared                  16 of 52
        thr indexed [z, z_next]                           52 of 52
        e and e' exchanged in the mix                     52 of 52
        wave sums folded (q0 + q1) + (q2 + q3)            40 of 52
        zi[0] taken as 0                                  5 of 52

    An unclamped key changes no sum (λ·1 to the node above either way); it is seen because the
    sources after those on x[-1] have key nx − 2, so the row stops being monotone and the period
    turns slow (tie-top).  The tie rule of the searches is as quiet: a source on a node gives
    the same two terms with w = 0 in the segment above as with w = 1 in the one below, so it
    shows only through the 40 terms of λ·0 that move the chunk boundaries of the run they head
    (tie-node-run).  A strictly alternating path does not see a vote that is never cleared
    (its slow periods share one word); the 0011 path does."""
    print(defect, defect_counts[defect])
    assert len(defect_counts[defect]) >= 1
    pinned = {"vote_row0_only": "vote-last1-", "vote_skips_last_pair": "vote-last1-",
              "vote_skips_first_pair": "vote-first0-", "no_key_clamp": "tie-top",
              "vote_never_cleared": "vote-", "zi0_taken_as_0": "shock-starts",
              "search_lt": "tie-node-run"}
    if defect in pinned:
        assert any(n.startswith(pinned[defect]) for n in defect_counts[defect])
    if defect.startswith("vote_skips") or defect == "vote_row0_only":
        # the single-inversion cases at every nx, the strided walk's nx = 600 and 1100 among them
        hit = [n for n in defect_counts[defect] if n.startswith(pinned[defect])]
        assert len(hit) == len(cases.VOTE_NX)
