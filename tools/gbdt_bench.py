#!/usr/bin/env python3
"""Measure the histogram GBDT fit on the engine (csrc/gbdt.hip, FraudEngine.fit_gbdt), in ONE process:

 trainer   the drop-in's own shape: ModelTrainer's synthetic split (8,000 x 33), 100 rounds, depth 6, subsample and
           colsample_bytree 0.8 (the reference's parameters);
 serving   a serving-sized one: 1 M x 64 scoring-vector-shaped rows (synth.feature_matrix) with a synthetic fraud
           label, 100 rounds, depth 8;
 headline  one fit of the headline forest's shape (500 rounds x depth 8) on scoring vectors whose 42 serving-time
           constant slots hold their constants: the grown forest's depth distribution, and what contract_forest_host
           leaves of it, next to the random forest's figures.

Each timed region is one whole fit from host arrays (staging, cuts, binning, every tree, the copy back), after
warm-up fits, repeated; the line carries every region, the median and the spread. The CPU figure beside it is
scikit-learn's HistGradientBoostingClassifier(max_iter, max_depth, learning_rate, max_bins=255, l2_regularization=1,
early_stopping=False) on the same data with the process's thread limit (OMP_NUM_THREADS, 16 where this is run): the
only histogram GBDT on the machine. It is another algorithm's wall time, not a parity check.

Prints one JSON line per part and appends it to profiles/gbdt/gbdt_bench.jsonl (OUT overrides the path).
Arguments: the parts to run (default: trainer serving headline)."""
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
from fdengine.engine import contract_forest_host
from fdengine.training import ModelTrainer, roc_auc_midrank

OUT = Path(os.environ.get("OUT", REPO / "profiles" / "gbdt" / "gbdt_bench.jsonl"))
THREADS = int(os.environ.get("OMP_NUM_THREADS", "16"))
CONSTANT_HALF = (12, 24, 25, 33, 34)  # serving-time constants 0.5; the other non-varying slots are 0
VARYING = (0, 1, 5, 6, 7, 14, 15, 16, 17, 19, 21, 23, 26, 27, 31, 32, 41, 42, 43, 44, 45, 46)


def emit(line):
    print(json.dumps(line), flush=True)
    OUT.parent.mkdir(parents=True, exist_ok=True)
    with open(OUT, "a") as f:
        f.write(json.dumps(line) + "\n")


def fraud_label(X, seed, rate=0.05):
    """A synthetic fraud label on scoring vectors: a noisy score of a few varying slots, the top `rate` flagged."""
    rng = np.random.Generator(np.random.PCG64(seed))
    Z = np.nan_to_num(X[:, VARYING[:8]].astype(np.float64))
    Z = (Z - Z.mean(0)) / (Z.std(0) + 1e-12)
    score = Z @ np.array([0.9, 0.7, -0.5, 0.4, 0.3, 0.3, -0.2, 0.2]) + 0.6 * Z[:, 0] * Z[:, 1]
    score = score + rng.normal(0.0, 1.0, len(X))
    return (score > np.quantile(score, 1.0 - rate)).astype(np.uint8)


def timed_fits(fit, warmup, regions):
    for _ in range(warmup):
        fit()
    out = []
    for _ in range(regions):
        t0 = time.perf_counter()
        res = fit()
        out.append(time.perf_counter() - t0)
    return out, res


def sklearn_fit(X, y, rounds, depth, regions):
    try:
        from sklearn.ensemble import HistGradientBoostingClassifier
    except ImportError:
        return None, None
    out = []
    for _ in range(regions):
        m = HistGradientBoostingClassifier(max_iter=rounds, max_depth=depth, learning_rate=0.1, max_bins=255,
                                           l2_regularization=1.0, early_stopping=False, random_state=0)
        t0 = time.perf_counter()
        m.fit(X, y)
        out.append(time.perf_counter() - t0)
    return out, m


def part(eng, name, X, y, Xt, yt, params, warmup, regions, sk_regions):
    first = time.perf_counter()
    eng.fit_gbdt(X, y, **params)
    first = time.perf_counter() - first
    if first > 40.0:  # a long fit: fewer regions, so that the part ends
        warmup, regions = 0, max(1, min(regions, int(150.0 / first)))
    c0 = eng.counter("gbdt_hist_launches")
    secs, fa = timed_fits(lambda: eng.fit_gbdt(X, y, **params), warmup, regions)
    launches = (eng.counter("gbdt_hist_launches") - c0) // (warmup + regions)
    eng.load_forest(0, fa)
    auc = roc_auc_midrank(yt, eng.predict(0, Xt))
    eng.unload_forest(0)
    sk, m = sklearn_fit(X, y, params["n_rounds"], params["max_depth"], sk_regions)
    line = {"part": name, "rows": int(X.shape[0]), "features": int(X.shape[1]), "rounds": params["n_rounds"],
            "max_depth": params["max_depth"], "subsample": params.get("subsample", 1.0),
            "colsample_bytree": params.get("colsample_bytree", 1.0), "first_fit_s": first, "warmup_fits": warmup,
            "engine_fit_s": secs, "engine_fit_s_median": float(np.median(secs)),
            "engine_fit_s_spread": float(max(secs) - min(secs)), "hist_launches_per_fit": int(launches),
            "nodes": int(len(fa.left)), "engine_test_auc": auc}
    if sk is not None:
        line.update({"sklearn_hist_gbdt_fit_s": sk, "sklearn_hist_gbdt_fit_s_median": float(np.median(sk)),
                     "sklearn_threads": THREADS, "sklearn_test_auc": roc_auc_midrank(yt, m.predict_proba(Xt)[:, 1])})
    emit(line)


def tree_depths(fa):
    out = []
    for t in range(fa.n_trees):
        o = int(fa.offsets[t])
        depth = {0: 0}
        for i in range(int(fa.offsets[t + 1]) - o):  # breadth-first numbering: a child follows its parent
            if fa.left[o + i] != -1:
                depth[int(fa.left[o + i])] = depth[int(fa.right[o + i])] = depth[i] + 1
        out.append(max(depth.values()))
    return np.asarray(out)


def headline(eng):
    n = int(os.environ.get("HEADLINE_ROWS", 65536))
    X = synth.feature_matrix(n, 64, seed=3000)
    for s in range(64):
        if s not in VARYING:
            X[:, s] = 0.5 if s in CONSTANT_HALF else 0.0
    y = fraud_label(X, 3001)
    t0 = time.perf_counter()
    fa = eng.fit_gbdt(X, y, n_rounds=500, max_depth=8, eta=0.1, subsample=0.8, colsample_bytree=0.8, seed=42)
    secs = time.perf_counter() - t0
    depths = tree_depths(fa)
    _, cdepths, pruned = contract_forest_host(fa)
    split = fa.left >= 0
    emit({"part": "headline", "rows": n, "features": 64, "rounds": 500, "max_depth": 8, "engine_fit_s": secs,
          "nodes": int(len(fa.left)), "splits": int(split.sum()), "mean_tree_depth": float(depths.mean()),
          "depth_histogram_from_0": np.bincount(depths, minlength=9).tolist(),
          "splits_on_constant_slots": int((~np.isin(fa.feature[split], VARYING)).sum()),
          "contract_pruned_splits": int(pruned), "mean_contracted_depth": float(np.mean(cdepths)),
          "sum_contracted_depth": int(np.sum(cdepths)),
          "random_forest_mean_contracted_depth": 4.21, "random_forest_sum_contracted_depth": 2104,
          "train_auc": roc_auc_midrank(y, fa.meta["margins"])})


def main():
    parts = sys.argv[1:] or ["trainer", "serving", "headline"]
    eng = fdengine.FraudEngine(0)
    if "trainer" in parts:
        tr = ModelTrainer(output_dir=os.environ.get("TMPDIR", "/tmp") + "/gbdt_bench_models", engine=eng)
        Xa, Xb, ya, yb = tr.prepare_training_data()
        Xa, Xb = Xa.astype(np.float32), Xb.astype(np.float32)
        part(eng, "trainer", Xa, ya, Xb, yb, dict(n_rounds=100, max_depth=6, eta=0.1, subsample=0.8,
                                                   colsample_bytree=0.8, seed=42), 2, 7, 3)
    if "serving" in parts:
        n = int(os.environ.get("SERVING_ROWS", 1000000))
        X = synth.feature_matrix(n + 100000, 64, seed=2000)
        y = fraud_label(X, 2001)
        part(eng, "serving", X[:n], y[:n], X[n:], y[n:], dict(n_rounds=100, max_depth=8, eta=0.1, seed=42), 1, 3, 1)
    if "headline" in parts:
        headline(eng)
    eng.close()


if __name__ == "__main__":
    main()
