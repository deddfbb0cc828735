"""bench.py as the command every change is measured with: a plain run (`--gpus 1 --steps N --warmup W`) prints the
headline line only, and `--dump-outputs DIR` writes what the last timed step computed. Run once, as a child process,
on config 2 at a small size (one forest launch per step), and checked against the CPU oracle on the same seeded
inputs: probabilities within 1e-5, the bar of the bench's own parity check and of smoke()."""
import json
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO

B, T, D, F, POOL, STEPS, WARMUP = 4096, 40, 5, 50, 2, 3, 1
MOVED = ("parity_vs_oracle", "p99_batch_latency_ms", "loaded_latency", "roofline", "kernel_avg_us", "cpu_baseline",
         "secondary_workloads")


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_the_last_step(tmp_path):
    import fdengine
    import oracle
    from fdengine import synth
    out = tmp_path / "dump"
    cmd = [sys.executable, str(REPO / "bench.py"), "--gpus", "1", "--steps", str(STEPS), "--warmup", str(WARMUP),
           "--workload", "config2", "--batch", str(B), "--trees", str(T), "--depth", str(D), "--pool", str(POOL),
           "--dump-outputs", str(out)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(rows) == 1
    d = json.loads(rows[0])
    assert (d["steps"], d["warmup"], d["n_gpus"], d["full"]) == (STEPS, WARMUP, 1, False)
    assert d["metric"] == "scored transactions/sec (whole node)" and d["unit"] == "txn/s"
    assert d["higher_is_better"] is True and d["dtype"] == "f32" and d["config"]["batch"] == B
    assert d["ms_per_step"] > 0 and d["value"] == pytest.approx(B / (d["ms_per_step"] * 1e-3), rel=1e-3)
    assert not [k for k in MOVED if k in d]  # those belong to --full
    assert sorted(p.name for p in out.iterdir()) == ["fraud_prob.npy"]
    got = np.load(out / "fraud_prob.npy")
    assert got.dtype == np.float64 and got.shape == (B,)
    # the same seeded model and micro-batch the bench built (Config2: seeds 7 / 8, pool seed 1000 + rank)
    doc = synth.xgboost_doc(T, D, F, synth.feature_matrix(2048, F, seed=7), seed=8)
    synth.write_xgboost_json(str(tmp_path / "fraud_classifier.json"), doc)
    forest = fdengine.load_xgboost_json(str(tmp_path / "fraud_classifier.json"))
    s = (STEPS - 1) % POOL  # the pool slot of the last timed step
    X = synth.feature_matrix(POOL * B, F, seed=1000)[s * B:(s + 1) * B]
    ref, _, _ = oracle.xgb_predict(forest, X)
    assert np.abs(got - ref).max() <= 1e-5
    assert got.std() > 1e-3  # a real spread of scores, not a constant
