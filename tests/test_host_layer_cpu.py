"""The workspace's host layer without a GPU: the tree dispatch order (csrc/tree_perm.hpp) against
orders recorded from the implementation it replaced, and the owning buffers (csrc/devbuf.hpp).
Both through stand-alone host programs built with AddressSanitizer and UBSan."""
import json
import os
import shutil
import subprocess

import pytest

from tests.conftest import GOLDEN, ROOT

CSRC = ROOT / "aiyagari-replication_amd" / "csrc"
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
SAN = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
       "-Wall", "-Werror", f"-I{CSRC}"]


def _cxx():
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    return cxx


def _build(tmp, src, extra=()):
    exe = tmp / src.replace(".cpp", "")
    cxx = _cxx()
    # the sanitizer runtimes linked into the program itself (clang's default), so that it runs
    # the same whatever else the environment loads
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    subprocess.run([cxx, *SAN, *static, str(ROOT / "tests" / "cpp" / src), "-o", str(exe), *extra],
                   check=True, cwd=tmp)
    return exe


@pytest.fixture(scope="module")
def perm_runs(tmp_path_factory):
    """Every fixture case through the program, once: [(case, table, slots)]."""
    fx = json.loads((GOLDEN / "tree_perm.json").read_text())
    exe = _build(tmp_path_factory.mktemp("tree_perm"), "tree_perm_main.cpp")
    lines = [str(len(fx["cases"]))]
    for c in fx["cases"]:
        t = fx["tables"][c["table"]]
        lines.append(f'{t["N"]} {t["ntile"]} {t["Nl"]} {c["PK"]} {c["mode"]} {c["coop"]}')
        lines.append(" ".join(map(str, t["kl"])))
    r = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    outs = r.stdout.strip("\n").split("\n")
    assert len(outs) == len(fx["cases"])
    return [(c, fx["tables"][c["table"]], [int(v) for v in o.split()])
            for c, o in zip(fx["cases"], outs)]


def test_tree_perm_fixture_covers_the_shapes():
    fx = json.loads((GOLDEN / "tree_perm.json").read_text())
    G = {k: t["N"] * t["ntile"] for k, t in fx["tables"].items()}
    cs = fx["cases"]
    assert {c["PK"] for c in cs if c["mode"] < 2} == {1, 2, 4}
    assert {c["mode"] for c in cs} == {0, 1, 2}
    assert any(fx["tables"][c["table"]]["ntile"] == 1 for c in cs)
    assert any(fx["tables"][c["table"]]["Nl"] > 1 for c in cs)
    assert any(G[c["table"]] % (8 * c["PK"]) for c in cs if c["mode"] < 2)
    assert any(G[c["table"]] // 8 < 256 for c in cs if c["mode"] == 1)      # empty tail
    assert any(G[c["table"]] // 8 > 256 for c in cs if c["mode"] == 1)      # and a real one
    hy = [c for c in cs if c["mode"] == 2]
    assert any(c["coop"] == 0 for c in hy)
    assert any(c["coop"] > G[c["table"]] // 8 + 1 for c in hy)               # H past a range


def test_tree_perm_equals_recorded_orders(perm_runs):
    for c, _, slots in perm_runs:
        assert slots == c["slots"], (c["table"], c["PK"], c["mode"], c["coop"])


def test_tree_perm_is_a_permutation(perm_runs):
    """Every item 0..G-1 exactly once; the rest are the documented markers: -1 (an unused slot)
    in either order, and in the hybrid order -2 as the second slot of a cooperative pair."""
    for c, t, slots in perm_runs:
        G = t["N"] * t["ntile"]
        assert sorted(v for v in slots if v >= 0) == list(range(G))
        assert all(v >= -2 for v in slots)
        if c["mode"] == 2:
            assert len(slots) % 16 == 0
            pairs = list(zip(slots[0::2], slots[1::2]))
            assert all(p[0] >= -1 and (p[0] >= 0 or p[1] == -1) for p in pairs)
            ncoop = sum(p[1] == -2 for p in pairs)
            sizes = [G // 8 + (x < G % 8) for x in range(8)]
            assert ncoop == sum(min(s, c["coop"]) for s in sizes)
        else:
            PK = c["PK"]
            assert len(slots) == (G + PK - 1) // PK * PK
            assert -2 not in slots and slots.count(-1) == len(slots) - G


def _run_hip_host_program(tmp_path, src):
    exe = _build(tmp_path, src,
                 ["-D__HIP_PLATFORM_AMD__", f"-I{ROCM}/include", f"-L{ROCM}/lib", "-lamdhip64",
                  f"-Wl,-rpath,{ROCM}/lib"])
    # no device visible; leak checking stays on for the program, off for the ROCm runtime's own
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1",
               LSAN_OPTIONS=f"suppressions={ROOT / 'tests' / 'cpp' / 'lsan.supp'}:print_suppressions=0")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    assert r.stdout.strip().endswith("done") and "FAILED" not in r.stdout


def test_devbuf_edge_cases(tmp_path):
    _run_hip_host_program(tmp_path, "devbuf_main.cpp")


def test_host_ctx_named_buffers(tmp_path):
    """The host tier's name -> buffer map and its typed staging (broadcast, layout helpers; csrc/
    host_ctx.hpp) on malloc-backed memory."""
    _run_hip_host_program(tmp_path, "host_ctx_main.cpp")
