"""bench.py's command line: a plain run is lean and exact about --steps, --dump-outputs writes the
last timed step's arrays reproducibly, --full adds the evidence blocks without changing them.

One small instance (QP n=128, m=32): its barrier-phase solve converges after ~330 Newton steps, so
--steps 1200 (600 per segment) makes the bench chain fresh solvers to reach the count.
"""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO

ARGS = ["--gpus", "1", "--steps", "1200", "--warmup", "2", "--n", "128", "--m", "32"]
FULL_ONLY = ("parity", "hbm_kernels", "cpu_baseline")


def run_bench(extra, out):
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py")] + ARGS + ["--dump-outputs", str(out)] + extra,
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0]), {os.path.basename(f)[:-4]: np.load(f) for f in sorted(glob.glob(str(out / "*.npy")))}


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    return run_bench([], tmp_path_factory.mktemp("plain"))


def test_bench_help_lists_the_options():
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--help"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    for opt in ("--gpus", "--steps", "--warmup", "--dump-outputs", "--full"):
        assert opt in r.stdout


@pytest.mark.gpu
def test_bench_plain_run_times_exactly_the_steps_and_dumps_outputs(plain):
    rec, arrs = plain
    assert rec["steps"] == 1200 and rec["newton_iters"] == 1200
    assert [rec["phases"][k]["iters"] for k in ("phase1", "barrier")] == [600, 600]
    assert rec["unit"] == "Newton iters/s" and rec["higher_is_better"] is True and rec["dtype"] == "f64"
    # one GPU, one instance: the headline is the reciprocal of the step time
    assert rec["ms_per_step"] > 0
    assert rec["value"] == pytest.approx(1e3 / rec["ms_per_step"], rel=1e-9)
    assert not [k for k in FULL_ONLY if k in rec]
    assert set(arrs) == {f"inst0_{seg}_{k}" for seg in ("phase1", "barrier") for k in ("x", "steps", "xstar", "value")} \
        | {"inst0_phase1_xs", "inst0_phase1_xs_steps"}
    for k, a in arrs.items():
        assert a.dtype == np.float64 and np.isfinite(a).all(), k
    assert arrs["inst0_barrier_x"].shape == (128,) and arrs["inst0_phase1_xs"].shape == (129,)
    assert sum(a.nbytes for a in arrs.values()) <= 64 << 20


@pytest.mark.gpu
def test_bench_full_adds_evidence_and_computes_the_same(plain, tmp_path):
    rec0, arrs0 = plain
    rec, arrs = run_bench(["--full", "--no-cpu"], tmp_path)
    assert "parity" in rec and "cpu_baseline" not in rec
    assert set(rec["hbm_kernels"]) == {"phase1", "barrier"}
    for k in ("metric", "unit", "higher_is_better", "dtype", "steps", "newton_iters"):
        assert rec[k] == rec0[k]
    assert set(arrs) == set(arrs0)
    for k in arrs0:
        assert np.array_equal(arrs[k], arrs0[k]), k
