"""The plain benchmark run and `--dump-outputs` (one bench process, a small grid).

`bench.py --gpus 1 --steps 3 --warmup 2 --na 1500 --dump-outputs DIR` times exactly 3 sweeps
after 2 warm-up sweeps of a solve from v = 0 and prints the result line without the `--full`
legs; DIR then holds what sweep 5 returned (v_new, policy_k, policy_c, idx) as float64 .npy,
which must equal the C oracle's sweep 5 of the same solve bit for bit (Na = 1500: the odd
size of tests/test_vfi_gpu.py, sweeps with and without the hint).
"""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from oracle import corc
from oracle import np_oracle as no

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
NA, WARMUP, STEPS = 1500, 2, 3


def test_plain_run_line_and_dumped_outputs(pkg, gpu, tmp_path):
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps",
                        str(STEPS), "--warmup", str(WARMUP), "--na", str(NA), "--dump-outputs",
                        str(out)], cwd=tmp_path, env=env, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    c = json.loads(r.stdout.strip().splitlines()[-1])
    assert c["steps"] == STEPS and c["warmup"] == WARMUP and c["n_gpus"] == 1
    assert c["unit"] == "evals/s" and c["dtype"] == "f64" and c["higher_is_better"] is True
    assert c["ms_per_step"] > 0
    assert c["value"] == pytest.approx(7 * NA * NA / (c["ms_per_step"] * 1e-3), rel=1e-12)
    assert c["repeats"]["n"] == 1   # one timed block of exactly --steps sweeps
    for moved in ("legs", "roofline", "cpu_baseline", "detail"):   # behind --full
        assert moved not in c, moved

    cal = no.calib_aiyagari(Na=NA, shocks="rouwenhorst")
    w = no.wage(0.04, cal["alpha"], cal["delta"])
    v = np.zeros((cal["N"], NA))
    for _ in range(WARMUP + STEPS):
        v, io, pko, pco = corc.vfi_sweep(v, cal["a_grid"], cal["s"], cal["P"], 0.04, w,
                                         cal["beta"], cal["sigma"])
    assert sorted(p.name for p in out.iterdir()) == ["idx.npy", "policy_c.npy", "policy_k.npy",
                                                     "v_new.npy"]
    for name, ref in (("v_new", v), ("idx", io), ("policy_k", pko), ("policy_c", pco)):
        got = np.load(out / f"{name}.npy")
        assert got.dtype == np.float64 and got.shape == (cal["N"], NA), name
        assert np.array_equal(got, ref), name
