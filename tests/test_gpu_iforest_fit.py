"""GPU: the IsolationForest fit on the engine (csrc/iforest_fit.hip) against the single-threaded host
reference, bit for bit: the sample kernel, the grow kernel on explicit rows, whole fits (trees, counts, offset), a fit
from a device tensor, and the trained forest through the serving side: load, predict, leaf ids, the contamination
share, the fused path, explain, the blend with a forest grown by fit_gbdt, and the ModelTrainer drop-in end to end."""
import asyncio
import math

import numpy as np
import pytest

import gbdt_cases as GC
import iforest_fit_cases as IC
import oracle
import shap_cases as SC
from fdengine import (FraudEngine, iforest_fit_grow_tree_ref_host, iforest_fit_ref_host, iforest_fit_sample_ref_host,
                      iforest_from_sklearn)
from fdengine import _native as N
from fdengine.training import ModelTrainer, roc_auc_midrank
from oracle import scoring_ref as S

pytestmark = pytest.mark.gpu
SLOT = 5


def trainer_like():
    """2,048 x 33, the trainer's parameters"""
    X = np.random.Generator(np.random.PCG64(77)).normal(size=(2048, 33)).astype(np.float32)
    X[:, 7] = np.float32(0.0)  # a constant column, as the flag columns of a small frame can be
    X[:, 20] = np.round(X[:, 20])  # and one with heavy ties
    return X, dict(n_estimators=100, max_samples=256, contamination=0.05, seed=42)


# ------------------------------------------------------------------ 1. the seams
@pytest.mark.parametrize("n", IC.SAMPLER_N)
def test_sample_kernel_equals_host(engine, n):
    for tree, seed, ms in ((0, 0, 0), (7, 12345, 1024), (65535, 2 ** 64 - 1, 2)):
        np.testing.assert_array_equal(engine.iforest_fit_sample(n, tree, seed=seed, max_samples=ms),
                                      iforest_fit_sample_ref_host(n, tree, seed=seed, max_samples=ms))


@pytest.mark.parametrize("name", list(IC.GROW_CASES))
def test_grow_kernel_equals_host(engine, name):
    X, rows, mask, _ = IC.grow_inputs(name)
    want = iforest_fit_grow_tree_ref_host(X, rows, 41, mask, seed=99)
    t0, s0 = engine.counter("iforest_fit_trees"), engine.counter("iforest_fit_nodes_split")
    got = engine.iforest_fit_grow_tree(X, rows, 41, mask, seed=99)
    IC.assert_same_tree(IC.forest_trees(got)[0], IC.forest_trees(want)[0], name)
    assert engine.counter("iforest_fit_trees") - t0 == 1
    assert engine.counter("iforest_fit_nodes_split") - s0 == int((want.left >= 0).sum())


# ------------------------------------------------------------------ 2. whole fits
@pytest.mark.parametrize("name", IC.FIT_CASES)
def test_fit_equals_host_reference(engine, name):
    X, p = IC.fit_case(name)
    want = iforest_fit_ref_host(X, **p)
    t0, s0 = engine.counter("iforest_fit_trees"), engine.counter("iforest_fit_nodes_split")
    got = engine.fit_iforest(X, **p)
    IC.assert_same_forest(got, want, name)
    assert got.meta["max_samples"] == want.meta["max_samples"]
    assert engine.counter("iforest_fit_trees") - t0 == p["n_estimators"]
    assert engine.counter("iforest_fit_nodes_split") - s0 == int((want.left >= 0).sum())


def test_trainer_like_fit_equals_host_reference(engine):
    X, p = trainer_like()
    want = iforest_fit_ref_host(X, **p)
    got = engine.fit_iforest(X, **p)
    IC.assert_same_forest(got, want, "2048 x 33, T 100, psi 256, contamination 0.05")
    IC.assert_same_forest(engine.fit_iforest(X, **p), got, "the same seed twice")
    other = engine.fit_iforest(X, **dict(p, seed=43))
    assert not np.array_equal(other.threshold[:50], got.threshold[:50])


def test_fit_from_a_device_tensor(engine):
    import torch
    X, p = trainer_like()
    p = dict(p, n_estimators=20)
    got = engine.fit_iforest(torch.from_numpy(X).to(torch.device("cuda", engine.device)), **p)
    IC.assert_same_forest(got, engine.fit_iforest(X, **p), "device tensor against numpy")
    IC.assert_same_forest(got, iforest_fit_ref_host(X, **p), "device tensor against the host reference")


# ------------------------------------------------------------------ 3. the fit is what is served
def test_trained_forest_is_served_and_explained(engine):
    X, p = trainer_like()
    fa = engine.fit_iforest(X, **p)
    n, T, psi = len(X), fa.n_trees, fa.meta["max_samples"]
    engine.load_forest(SLOT, fa)
    try:
        prob, raw, leaf = engine.predict(SLOT, X, want_raw=True, want_leaf=True)
        rp, rd, rl = oracle.iforest_predict(fa, X, want_leaf=True)
        np.testing.assert_array_equal(leaf, rl)
        np.testing.assert_array_equal(raw, rd)
        assert np.abs(prob - rp).max() <= 1e-12
        # every tree's own rows, walked through the served forest, reproduce every leaf's count
        counts = fa.meta["n_node_samples"]
        for t in range(T):
            rows = iforest_fit_sample_ref_host(n, t, seed=p["seed"], max_samples=psi)
            m = int(fa.offsets[t + 1] - fa.offsets[t])
            got = np.bincount(leaf[rows, t], minlength=m)
            is_leaf = fa.left[fa.offsets[t]:fa.offsets[t + 1]] == -1
            np.testing.assert_array_equal(got[is_leaf], counts[fa.offsets[t]:fa.offsets[t + 1]][is_leaf])
            assert not got[~is_leaf].any()
        # a probability above 0.5 is decision_function < 0: the share is the contamination, up to a row and ties
        score = -(2.0 ** (-raw / fa.if_denominator))
        k = p["contamination"] * (n - 1)
        ties = int((score == np.sort(score)[int(math.floor(k))]).sum()) + int((score == fa.if_offset).sum())
        share = float((prob > 0.5).mean())
        print(f"share of fit rows with probability > 0.5: {share:.5f} (contamination {p['contamination']}, "
              f"ties {ties})")
        assert abs(share - p["contamination"]) <= (1 + ties) / n
        # a serving-sized batch (>= 128 tiles of 256 rows, no leaf ids) goes to the fused single-forest kernel
        s0 = engine.counter("ensemble_single_launches")
        reps = 128 * 256 // n + 1
        _, raw_big = engine.predict(SLOT, np.tile(X, (reps, 1)), want_raw=True)
        assert engine.counter("ensemble_single_launches") == s0 + 1
        np.testing.assert_array_equal(raw_big, np.tile(raw, reps))
        # attribution with the trained covers, no set_cover: additivity as tests/test_gpu_shap.py checks it
        rows = np.arange(0, n, 41)
        phi = engine.explain(SLOT, X[rows])
        got = np.array([math.fsum(row) for row in phi])
        err = float(np.abs(got - raw[rows]).max()) / SC.scale(fa)
        print(f"additivity of a trained IsolationForest: max |delta| / S = {err:.2e} (tol {SC.TOL:.2e})")
        assert err <= SC.TOL
    finally:
        engine.unload_forest(SLOT)


def test_both_members_trained_here_and_blended(engine):
    X, y, gp = GC.fit_case("trainer_4099x33")
    X, y = X[:2048], y[:2048]
    fx = engine.fit_gbdt(X, y, **dict(gp, n_rounds=20))
    fi = engine.fit_iforest(X, n_estimators=50, contamination=0.05, seed=1)
    names = ["xgboost_primary", "isolation_forest"]
    w = S.normalized_weights({"xgboost_primary": 0.4, "isolation_forest": 0.05})
    params = FraudEngine.blend_params([w[k] for k in names], [S.CONF_MULT[k] for k in names])
    engine.load_forest(0, fx)
    engine.load_forest(1, fi)
    try:
        mp, fp, conf, dec, risk = engine.score_matrix(params, [0, 1], X)
        px, pi = oracle.xgb_predict(fx, X)[0], oracle.iforest_predict(fi, X)[0]
        assert np.abs(mp[0] - px).max() <= 1e-5 and np.abs(mp[1] - pi).max() <= 1e-12
        for i in range(0, len(X), 41):
            rfp, rconf, rdec, rrisk = S.blend_row(names, [float(mp[0, i]), float(mp[1, i])], w)
            assert fp[i] == rfp and conf[i] == rconf
            assert N.DECISIONS[dec[i]] == rdec and N.RISK_LEVELS[risk[i]] == rrisk
            ofp = S.blend_row(names, [float(px[i]), float(pi[i])], w)[0]
            assert abs(fp[i] - ofp) <= 1e-5
    finally:
        engine.unload_forest(0)
        engine.unload_forest(1)


# ------------------------------------------------------------------ 4. the drop-in, end to end
def test_model_trainer_end_to_end(engine, tmp_path):
    import joblib
    from fdengine.model_manager import ModelManager
    from fdengine.registry import ScoringConfig
    tr = ModelTrainer(output_dir=str(tmp_path), engine=engine)
    df = tr._generate_synthetic_data(2000)
    feats = [c for c in df.columns if c not in ("is_fraud", "transaction_id", "user_id", "merchant_id")]
    X, y = df[feats].values, df["is_fraud"].values
    cut = 1600
    t0, s0 = engine.counter("iforest_fit_trees"), engine.counter("iforest_fit_nodes_split")
    res = tr.train_isolation_forest(X[:cut], y[:cut], X[cut:], y[cut:])
    assert list(res) == ["model_type", "model_path", "auc_score", "training_time_seconds"]
    assert res["model_type"] == "isolation_forest"
    assert res["model_path"] == str(tmp_path / "sklearn" / "isolation_forest.joblib")
    assert engine.counter("iforest_fit_trees") - t0 == 100 and engine.counter("iforest_fit_nodes_split") > s0
    # the file holds the forest the host reference grows from the same rows
    want = iforest_fit_ref_host(X[:cut][y[:cut] == 0], n_estimators=100, contamination=0.05, seed=42)
    back = iforest_from_sklearn(joblib.load(res["model_path"]))
    for k in ("offsets", "left", "right", "feature", "threshold", "leaf_value", "cover"):
        np.testing.assert_array_equal(getattr(back, k), getattr(want, k), err_msg=k)
    assert back.if_offset == want.if_offset and back.if_denominator == want.if_denominator
    # and reloads through the serving side's ModelManager
    cfg = ScoringConfig(str(tmp_path))
    for name in list(cfg.models):
        if name != "isolation_forest":
            cfg.disable_model(name)
    mm = ModelManager(cfg, engine=engine)
    asyncio.run(mm.load_all_models())
    slot = mm.engine_slot("isolation_forest")
    assert slot >= 0
    try:
        Xt = X[cut:].astype(np.float32)
        prob, raw = engine.predict(slot, Xt, want_raw=True)
        assert res["auc_score"] == roc_auc_midrank(y[cut:], -raw)
        np.testing.assert_array_equal(raw, oracle.iforest_predict(want, Xt)[1])
        served = asyncio.run(mm.predict("isolation_forest", X[cut:]))
        np.testing.assert_array_equal(np.asarray(served).reshape(-1), prob)
    finally:
        engine.unload_forest(slot)
    assert 0.0 <= res["auc_score"] <= 1.0
    tr.save_training_metadata({"isolation_forest": res})
    assert (tmp_path / "training_metadata.json").exists()
