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

The watched fit (eval_set, early stopping; DESIGN §4.14 "Evaluation") has four parts of its own, written to
profiles/gbdt_eval/gbdt_eval_bench.jsonl:

 unchanged   a fit without the new arguments at the trainer and the serving shape, timed by child processes that
             alternate between another build of the tree (PARENT_TREE, default ab_prev/: a checkout of the parent
             commit, built) and this one: what the new code costs a caller who does not use it;
 eval_cost   the same two fits with a 20 % eval set (2,000 / 200,000 rows), AUC and error: the overhead per round;
 caller_loop the trainer shape's curve on the device against what a caller did before: per round truncate, load_forest,
             predict, roc_auc_midrank on the host;
 early_stop  both shapes with early_stopping_rounds=10: rounds run, wall time and held-out AUC of the cut forest
             against the full 100 rounds.

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

if len(sys.argv) > 2 and sys.argv[1] == "_plain_child":  # a child of the "unchanged" part: the tree it is told to use
    sys.path[:0] = [sys.argv[2], sys.argv[2] + "/realtime-fraud-detection_amd"]

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


EVAL_OUT = REPO / "profiles" / "gbdt_eval" / "gbdt_eval_bench.jsonl"
TRAINER_PARAMS = dict(n_rounds=100, max_depth=6, eta=0.1, subsample=0.8, colsample_bytree=0.8, seed=42)
SERVING_PARAMS = dict(n_rounds=100, max_depth=8, eta=0.1, seed=42)


def trainer_data():
    tr = ModelTrainer(output_dir=os.environ.get("TMPDIR", "/tmp") + "/gbdt_bench_models")
    Xa, Xb, ya, yb = tr.prepare_training_data()
    return Xa.astype(np.float32), ya.astype(np.uint8), Xb.astype(np.float32), yb.astype(np.uint8)


def serving_data(n_eval):
    n = int(os.environ.get("SERVING_ROWS", 1000000))
    X = synth.feature_matrix(n + n_eval, 64, seed=2000)
    y = fraud_label(X, 2001)
    return X[:n], y[:n], X[n:], y[n:]


def plain_child(shape, regions):
    """Timed fits without the new arguments, in this process's tree -> one JSON line on stdout."""
    X, y, _, _ = trainer_data() if shape == "trainer" else serving_data(1000)
    params = TRAINER_PARAMS if shape == "trainer" else SERVING_PARAMS
    eng = fdengine.FraudEngine(0)
    secs, _ = timed_fits(lambda: eng.fit_gbdt(X, y, **params), 1, regions)
    eng.close()
    print(json.dumps({"fit_s": secs}), flush=True)


def unchanged():
    import subprocess
    parent = os.environ.get("PARENT_TREE", str(REPO / "ab_prev"))
    for shape, regions, turns in (("trainer", 7, 3), ("serving", 2, 2)):
        runs = {"parent": [], "this": []}
        for _ in range(turns):  # parent, this, parent, this ...: drift of the machine falls on both alike
            for who, tree in (("parent", parent), ("this", str(REPO))):
                r = subprocess.run([sys.executable, __file__, "_plain_child", tree, shape, str(regions)],
                                   capture_output=True, text=True, timeout=600, check=True)
                runs[who].append(json.loads(r.stdout.strip().splitlines()[-1])["fit_s"])
        med = {w: [float(np.median(t)) for t in v] for w, v in runs.items()}
        emit({"part": "unchanged", "shape": shape, "fits_per_turn": regions, "parent_fit_s": runs["parent"],
              "this_fit_s": runs["this"], "parent_turn_medians_s": med["parent"], "this_turn_medians_s": med["this"],
              "parent_median_s": float(np.median(sum(runs["parent"], []))),
              "this_median_s": float(np.median(sum(runs["this"], []))),
              "parent_spread_of_turn_medians_s": max(med["parent"]) - min(med["parent"]),
              "parent_spread_of_fits_s": max(sum(runs["parent"], [])) - min(sum(runs["parent"], []))})


def eval_cost(eng, shape, X, y, Xe, ye, params, warmup, regions):
    line = {"part": "eval_cost", "shape": shape, "rows": len(X), "eval_rows": len(Xe), "rounds": params["n_rounds"]}
    plain, _ = timed_fits(lambda: eng.fit_gbdt(X, y, **params), warmup, regions)
    line.update(plain_fit_s=plain, plain_round_ms=float(np.median(plain)) / params["n_rounds"] * 1e3)
    for metric in ("auc", "error"):
        secs, fa = timed_fits(lambda: eng.fit_gbdt(X, y, eval_set=(Xe, ye), eval_metric=metric, **params), warmup,
                              regions)
        line.update({f"{metric}_fit_s": secs, f"{metric}_overhead_per_round_ms":
                     (float(np.median(secs)) - float(np.median(plain))) / params["n_rounds"] * 1e3,
                     f"{metric}_last": fa.meta["evals_result"]["validation_0"][metric][-1]})
    emit(line)
    return fa


def caller_loop(eng, X, y, Xe, ye, params):
    from fdengine import truncate_forest
    dev, _ = timed_fits(lambda: eng.fit_gbdt(X, y, eval_set=(Xe, ye), **params), 1, 5)
    fa = eng.fit_gbdt(X, y, **params)

    def loop():
        fit = eng.fit_gbdt(X, y, **params)
        curve = []
        for t in range(fit.n_trees):
            eng.load_forest(0, truncate_forest(fit, t + 1))
            curve.append(roc_auc_midrank(ye, eng.predict(0, Xe, want_raw=True)[1]))
            eng.unload_forest(0)
        return curve

    host, curve = timed_fits(loop, 0, 2)
    watched = eng.fit_gbdt(X, y, eval_set=(Xe, ye), **params)
    emit({"part": "caller_loop", "rows": len(X), "eval_rows": len(Xe), "rounds": params["n_rounds"],
          "device_curve_fit_s": dev, "device_curve_fit_s_median": float(np.median(dev)),
          "fit_then_host_loop_s": host, "fit_then_host_loop_s_median": float(np.median(host)),
          "curves_equal": curve == watched.meta["evals_result"]["validation_0"]["auc"], "nodes": int(len(fa.left))})


def early_stop(eng, shape, X, y, Xe, ye, params, k):
    eng.fit_gbdt(X, y, eval_set=(Xe, ye), early_stopping_rounds=k, **params)  # warm-up: the buffers exist
    t0 = time.perf_counter()
    full = eng.fit_gbdt(X, y, eval_set=(Xe, ye), **params)
    t_full = time.perf_counter() - t0
    t0 = time.perf_counter()
    cut = eng.fit_gbdt(X, y, eval_set=(Xe, ye), early_stopping_rounds=k, **params)
    t_cut = time.perf_counter() - t0
    curve = full.meta["evals_result"]["validation_0"]["auc"]
    emit({"part": "early_stop", "shape": shape, "rows": len(X), "eval_rows": len(Xe), "rounds": params["n_rounds"],
          "early_stopping_rounds": k, "rounds_run": cut.meta["rounds_run"], "best_iteration": cut.meta["best_iteration"],
          "full_fit_s": t_full, "stopped_fit_s": t_cut, "trees_returned": cut.n_trees,
          "eval_auc_cut_forest": cut.meta["best_score"], "eval_auc_full_forest": curve[-1],
          "eval_auc_curve_every_10": curve[9::10]})


def main():
    global OUT
    if len(sys.argv) > 2 and sys.argv[1] == "_plain_child":
        return plain_child(sys.argv[3], int(sys.argv[4]))
    parts = sys.argv[1:] or ["trainer", "serving", "headline"]
    if {"unchanged", "eval_cost", "caller_loop", "early_stop"} & set(parts) and "OUT" not in os.environ:
        OUT = EVAL_OUT
    if "unchanged" in parts:  # (before this process opens the device: one process at a time holds it)
        unchanged()
    eng = fdengine.FraudEngine(0)
    if {"eval_cost", "caller_loop", "early_stop"} & set(parts):
        Xa, ya, Xb, yb = trainer_data()
        if "eval_cost" in parts:
            eval_cost(eng, "trainer", Xa, ya, Xb, yb, TRAINER_PARAMS, 2, 7)
        if "caller_loop" in parts:
            caller_loop(eng, Xa, ya, Xb, yb, TRAINER_PARAMS)
        if "early_stop" in parts:
            early_stop(eng, "trainer", Xa, ya, Xb, yb, TRAINER_PARAMS, 10)
    if {"eval_cost", "early_stop"} & set(parts):
        X, y, Xe, ye = serving_data(200000)
        if "eval_cost" in parts:
            eval_cost(eng, "serving", X, y, Xe, ye, SERVING_PARAMS, 1, 2)
        if "early_stop" in parts:
            early_stop(eng, "serving", X, y, Xe, ye, SERVING_PARAMS, 10)
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
