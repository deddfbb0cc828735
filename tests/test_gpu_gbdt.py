"""GPU: the histogram GBDT fit on the engine (csrc/gbdt.hip) against the single-threaded host reference,
bit for bit: the bin kernel, the split search on every case of tests/gbdt_cases.py, whole fits (trees, covers, gains
and final margins), independence of the histogram kernel's launch shape, and the trained forest through the serving
side: load, predict, the written JSON, the fused path, explain, and the ModelTrainer drop-in end to end."""
import json
import math

import numpy as np
import pytest

import gbdt_cases as GC
import shap_cases as SC
from fdengine import (gbdt_cuts_host, gbdt_fit_ref_host, gbdt_grow_tree_ref_host, xgboost_doc_from_forest)
from fdengine.engine import gbdt_bin_ref_host, gbdt_grad_ref_host
from fdengine.training import ModelTrainer, roc_auc_midrank

pytestmark = pytest.mark.gpu
SLOT = 5


def _same_forest(got, want, what):
    np.testing.assert_array_equal(got.offsets, want.offsets, err_msg=what)
    GC.assert_same_tree(GC.tree_fields(got), GC.tree_fields(want), what)
    np.testing.assert_array_equal(np.asarray(got.meta["margins"]).view(np.uint32),
                                  np.asarray(want.meta["margins"]).view(np.uint32), err_msg=what)


# ------------------------------------------------------------------ 1. the bin kernel
def test_bin_kernel_equals_host(engine):
    mats = [GC.edge_matrix()] + [GC.split_case(name)["X"] for name in ("rows1", "rows65_f1_depth10", "rows257_depth10",
                                                                      "rows4099_f64_bin16", "all_nan_column")]
    for X in mats:
        for max_bin in (2, 16, 256):
            cuts, off = gbdt_cuts_host(X, max_bin)
            want = gbdt_bin_ref_host(X, cuts, off)
            np.testing.assert_array_equal(engine.gbdt_bin(X, cuts, off), want)
            np.testing.assert_array_equal(want, GC.bin_numpy(X, cuts, off))


def test_gradient_kernel_equals_host(engine):
    big = np.finfo(np.float32).max
    m = np.concatenate([np.linspace(-40, 40, 4099), [0.0, -0.0, 88.0, -88.0, big, -big, np.inf, -np.inf]])
    m = m.astype(np.float32)
    for label in (0, 1):
        y = np.full(len(m), label, np.uint8)
        g, h = engine.gbdt_grad(m, y)
        rg, rh = gbdt_grad_ref_host(m, y)
        np.testing.assert_array_equal(g, rg)
        np.testing.assert_array_equal(h, rh)


# ------------------------------------------------------------------ 2. the split search
@pytest.mark.parametrize("name", GC.SPLIT_CASES)
def test_grow_tree_equals_host_reference(engine, name):
    c = GC.split_inputs(name, gbdt_cuts_host)
    args = (c["bins"], c["cuts"], c["offsets"], c["g"], c["h"], c["row_mask"], c["feature_mask"])
    want = gbdt_grow_tree_ref_host(*args, **c["params"])
    t0, s0 = engine.counter("gbdt_trees"), engine.counter("gbdt_nodes_split")
    got = engine.gbdt_grow_tree(*args, **c["params"])
    np.testing.assert_array_equal(got.offsets, want.offsets)
    GC.assert_same_tree(GC.tree_fields(got), GC.tree_fields(want), name)
    assert engine.counter("gbdt_trees") - t0 == 1
    assert engine.counter("gbdt_nodes_split") - s0 == int((want.left >= 0).sum())


# ------------------------------------------------------------------ 3. whole fits
@pytest.mark.parametrize("name", list(GC.FIT_CASES))
def test_fit_equals_host_reference(engine, name):
    X, y, params = GC.fit_case(name)
    want = gbdt_fit_ref_host(X, y, **params)
    h0 = engine.counter("gbdt_hist_launches")
    got = engine.fit_gbdt(X, y, **params)
    _same_forest(got, want, name)
    np.testing.assert_array_equal(got.cover, want.cover)
    assert engine.counter("gbdt_hist_launches") - h0 == params["n_rounds"] * params["max_depth"]
    again = engine.fit_gbdt(X, y, **params)
    _same_forest(again, got, name + ": the same seed twice")
    if params.get("subsample", 1.0) < 1.0:
        other = engine.fit_gbdt(X, y, **dict(params, seed=params["seed"] + 1))
        assert len(other.left) != len(got.left) or not np.array_equal(other.threshold, got.threshold)


def test_fit_from_device_tensors(engine):
    import torch
    X, y, params = GC.fit_case("nan_257x64")
    want = gbdt_fit_ref_host(X, y, **params)
    dev = torch.device("cuda", engine.device)
    got = engine.fit_gbdt(torch.from_numpy(X).to(dev), torch.from_numpy(y).to(dev), **params)
    got.meta["margins"] = got.meta["margins"].cpu().numpy()
    _same_forest(got, want, "device tensors")


# ------------------------------------------------------------------ 4. histogram shape independence
def test_histogram_launch_shape_does_not_change_a_bit(engine):
    X, y, params = GC.fit_case("trainer_4099x33")
    params["n_rounds"] = 4
    fits = []
    try:
        for rows in (64, 1000, 4096, 1 << 20):  # 65 workgroups of one wave's rows ... one workgroup for everything
            engine.set_option("gbdt_hist_rows", rows)
            fits.append(engine.fit_gbdt(X, y, **params))
    finally:
        engine.set_option("gbdt_hist_rows", 4096)
    for f in fits[1:]:
        _same_forest(f, fits[0], "gbdt_hist_rows")
    _same_forest(fits[0], gbdt_fit_ref_host(X, y, **params), "against the host reference")


# ------------------------------------------------------------------ 5. trainer to server
def test_trained_forest_is_served_and_explained(engine, tmp_path):
    X, y, params = GC.fit_case("trainer_4099x33")
    fa = engine.fit_gbdt(X, y, **params)
    margins = fa.meta["margins"]
    engine.load_forest(SLOT, fa)
    try:
        prob, raw, leaf = engine.predict(SLOT, X, want_raw=True, want_leaf=True)
        np.testing.assert_array_equal(raw.astype(np.float32).view(np.uint32), margins.view(np.uint32))
        # a serving-sized batch (>= 128 tiles of 256 rows, no leaf ids) goes to the fused single-forest kernel
        s0 = engine.counter("ensemble_single_launches")
        _, raw_big = engine.predict(SLOT, np.tile(X, (9, 1)), want_raw=True)
        assert engine.counter("ensemble_single_launches") == s0 + 1
        np.testing.assert_array_equal(raw_big.astype(np.float32).view(np.uint32), np.tile(margins, 9).view(np.uint32))
        # attribution with the trained covers, no set_cover: additivity as tests/test_gpu_shap.py checks it
        rows = np.arange(0, len(X), 41)
        phi = engine.explain(SLOT, X[rows])
        lv = SC.leaf_values(fa)
        base = SC.base_margin(fa)
        want = np.array([math.fsum(lv[fa.offsets[t] + leaf[r, t]] for t in range(fa.n_trees)) + base for r in rows])
        got = np.array([math.fsum(row) for row in phi])
        err = float(np.abs(got - want).max()) / SC.scale(fa)
        print(f"additivity of a trained forest: max |delta| / S = {err:.2e} (tol {SC.TOL:.2e})")
        assert err <= SC.TOL
        # the written file scores identically
        path = tmp_path / "fraud_classifier.json"
        path.write_text(json.dumps(xgboost_doc_from_forest(fa)))
        engine.load_xgboost_file(SLOT, path)
        prob2, raw2 = engine.predict(SLOT, X, want_raw=True)
        np.testing.assert_array_equal(raw2, raw)
        np.testing.assert_array_equal(prob2, prob)
        phi2 = engine.explain(SLOT, X[rows])  # the file's sum_hessian serves as the covers
        np.testing.assert_array_equal(phi2, phi)
    finally:
        engine.unload_forest(SLOT)


# ------------------------------------------------------------------ 6. the drop-in, end to end
def test_model_trainer_end_to_end(engine, tmp_path):
    tr = ModelTrainer(output_dir=str(tmp_path), engine=engine)
    df = tr._generate_synthetic_data(2000)
    feats = [c for c in df.columns if c not in ("is_fraud", "transaction_id", "user_id", "merchant_id")]
    X, y = df[feats].values, df["is_fraud"].values
    cut = 1600
    t0, h0, s0 = (engine.counter(k) for k in ("gbdt_trees", "gbdt_hist_launches", "gbdt_nodes_split"))
    res = tr.train_xgboost_model(X[:cut], y[:cut], X[cut:], y[cut:])
    assert list(res) == ["model_type", "model_path", "auc_score", "training_time_seconds", "feature_importance"]
    assert res["model_type"] == "xgboost" and res["model_path"] == str(tmp_path / "xgboost" / "fraud_classifier.json")
    assert engine.counter("gbdt_trees") - t0 == 100 and engine.counter("gbdt_hist_launches") - h0 == 600
    assert engine.counter("gbdt_nodes_split") > s0
    engine.load_xgboost_file(SLOT, res["model_path"])
    try:
        prob = engine.predict(SLOT, X[cut:].astype(np.float32))
    finally:
        engine.unload_forest(SLOT)
    assert res["auc_score"] == roc_auc_midrank(y[cut:], prob)
    assert 0.5 < res["auc_score"] <= 1.0
    imp = res["feature_importance"]
    assert list(imp) == list(range(33)) and abs(sum(imp.values()) - 1.0) < 1e-12
    # the same fit on the host reference: the file the drop-in wrote holds those trees
    want = gbdt_fit_ref_host(X[:cut], y[:cut], n_rounds=100, max_depth=6, eta=0.1, subsample=0.8, colsample_bytree=0.8,
                             seed=42)
    doc = json.loads(open(res["model_path"]).read())
    assert doc == json.loads(json.dumps(xgboost_doc_from_forest(want)))
    tr.save_training_metadata({"xgboost": res})
    assert (tmp_path / "training_metadata.json").exists()
