#!/usr/bin/env python3
"""Measure the IsolationForest fit on the engine (csrc/iforest_fit.hip, FraudEngine.fit_iforest), in ONE process:

 trainer   the drop-in's own shape: the normal rows of ModelTrainer's synthetic split (7,600 x 33), 100 trees,
           psi 256, contamination 0.05 (the reference's parameters);
 serving   a serving-sized one: 1 M x 64 scoring-vector-shaped rows (synth.feature_matrix), 1,000 trees, psi 1024,
           contamination 0.05.

Each timed region is one whole fit from host arrays (staging, the two launches, the copy back, the renumbering, the
offset's scoring pass and sort), after warm-up fits, repeated; the line carries every region, the median and the
spread. The CPU figure beside it is scikit-learn's IsolationForest(n_estimators, max_samples, contamination,
n_jobs=threads).fit on the same data with the process's thread limit (OMP_NUM_THREADS, 16 where this is run). It grows
other trees (its own random stream); the wall time is what is compared.

Prints one JSON line per part and appends it to profiles/iforest_fit/iforest_fit_bench.jsonl (OUT overrides the path).
Arguments: the parts to run (default: trainer serving)."""
import json
import os
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(REPO), str(REPO / "realtime-fraud-detection_amd")]
import numpy as np

import fdengine
from fdengine import synth
from fdengine.training import ModelTrainer

OUT = Path(os.environ.get("OUT", REPO / "profiles" / "iforest_fit" / "iforest_fit_bench.jsonl"))
THREADS = int(os.environ.get("OMP_NUM_THREADS", "16"))


def emit(line):
    print(json.dumps(line), flush=True)
    OUT.parent.mkdir(parents=True, exist_ok=True)
    with open(OUT, "a") as f:
        f.write(json.dumps(line) + "\n")


def timed(fit, warmup, regions):
    for _ in range(warmup):
        fit()
    out = []
    for _ in range(regions):
        t0 = time.perf_counter()
        res = fit()
        out.append(time.perf_counter() - t0)
    return out, res


def sklearn_fit(X, trees, psi, contamination, regions):
    try:
        from sklearn.ensemble import IsolationForest
    except ImportError:
        return None, None
    out = []
    for _ in range(regions):
        m = IsolationForest(n_estimators=trees, max_samples=psi, contamination=contamination, random_state=0,
                            n_jobs=THREADS)
        t0 = time.perf_counter()
        m.fit(X)
        out.append(time.perf_counter() - t0)
    return out, m


def part(eng, name, X, params, warmup, regions, sk_regions):
    first = time.perf_counter()
    eng.fit_iforest(X, **params)
    first = time.perf_counter() - first
    if first > 40.0:  # a long fit: fewer regions, so that the part ends
        warmup, regions = 0, max(1, min(regions, int(150.0 / first)))
    secs, fa = timed(lambda: eng.fit_iforest(X, **params), warmup, regions)
    # the same fit without the offset pass: what growing the trees alone takes
    grow, _ = timed(lambda: eng.fit_iforest(X, **dict(params, contamination=0)), 1, regions)
    print(f"[{name}] engine: first {first:.3f} s, then {secs}, trees only {grow}", file=sys.stderr, flush=True)
    sk, m = sklearn_fit(X, params["n_estimators"], params["max_samples"], params["contamination"], sk_regions)
    line = {"part": name, "rows": int(X.shape[0]), "features": int(X.shape[1]), "trees": params["n_estimators"],
            "max_samples": params["max_samples"], "contamination": params["contamination"], "first_fit_s": first,
            "warmup_fits": warmup, "engine_fit_s": secs, "engine_fit_s_median": float(np.median(secs)),
            "engine_fit_s_spread": float(max(secs) - min(secs)), "engine_grow_only_s": grow,
            "engine_grow_only_s_median": float(np.median(grow)), "nodes": int(len(fa.left)),
            "engine_offset": fa.if_offset}
    if sk is not None:
        line.update({"sklearn_fit_s": sk, "sklearn_fit_s_median": float(np.median(sk)),
                     "sklearn_fit_s_spread": float(max(sk) - min(sk)), "sklearn_threads": THREADS,
                     "sklearn_offset": float(m.offset_)})
    emit(line)


def main():
    parts = sys.argv[1:] or ["trainer", "serving"]
    eng = fdengine.FraudEngine(0)
    if "trainer" in parts:
        tr = ModelTrainer(output_dir=os.environ.get("TMPDIR", "/tmp") + "/iforest_fit_bench_models", engine=eng)
        Xa, _, ya, _ = tr.prepare_training_data()
        X = np.ascontiguousarray(Xa[ya == 0].astype(np.float32))
        part(eng, "trainer", X, dict(n_estimators=100, max_samples=256, contamination=0.05, seed=42), 2, 7, 3)
    if "serving" in parts:
        n = int(os.environ.get("SERVING_ROWS", 1000000))
        X = np.nan_to_num(synth.feature_matrix(n, 64, seed=2000).astype(np.float32))
        part(eng, "serving", X, dict(n_estimators=1000, max_samples=1024, contamination=0.05, seed=42), 1, 3, 1)
    eng.close()


if __name__ == "__main__":
    main()
