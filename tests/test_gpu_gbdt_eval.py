"""GPU: the watched GBDT fit on the engine (fd_gbdt_fit_eval_*, csrc/gbdt.hip, DESIGN §4.14 "Evaluation") against the
single-threaded host reference, bit for bit, and against serving as the independent oracle: the metric seam on crafted
margins, eval fits from numpy and from device tensors, early stopping (a case that must fire and a noisy one) with the
counters it declares, independence of the launch shape, a fit without the new arguments, and the ModelTrainer drop-in."""
import json

import numpy as np
import pytest

import gbdt_cases as GC
import gbdt_eval_cases as EC
from fdengine import gbdt_fit_ref_host, gbdt_metric_ref_host, xgboost_doc_from_forest
from fdengine.training import ModelTrainer, roc_auc_midrank

pytestmark = pytest.mark.gpu
SLOT = 5
VECTORS = EC.metric_vectors()
COUNTERS = ("gbdt_trees", "gbdt_hist_launches", "gbdt_eval_launches", "gbdt_rounds_run")


def _counters(engine):
    return {k: engine.counter(k) for k in COUNTERS}


def _advance(engine, before):
    return {k: engine.counter(k) - v for k, v in before.items()}


def _host(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def _same_watched_fit(got, want, what):
    np.testing.assert_array_equal(got.offsets, want.offsets, err_msg=what)
    GC.assert_same_tree(GC.tree_fields(got), GC.tree_fields(want), what)
    for k in ("margins", "eval_margins"):
        np.testing.assert_array_equal(EC.bits32(_host(got.meta[k])), EC.bits32(want.meta[k]), err_msg=f"{what}: {k}")
    assert got.meta["evals_result"].keys() == want.meta["evals_result"].keys()
    for metric, curve in want.meta["evals_result"]["validation_0"].items():
        np.testing.assert_array_equal(EC.bits64(got.meta["evals_result"]["validation_0"][metric]), EC.bits64(curve),
                                      err_msg=f"{what}: the curve")
    for k in ("best_iteration", "rounds_run", "best_score"):
        assert got.meta[k] == want.meta[k], (what, k)


def _served_raw(engine, fa, X):
    engine.load_forest(SLOT, fa)
    try:
        return engine.predict(SLOT, np.asarray(X, np.float32), want_raw=True)[1].astype(np.float32)
    finally:
        engine.unload_forest(SLOT)


# ------------------------------------------------------------------ 1. the metric seam
@pytest.mark.parametrize("name", list(VECTORS))
def test_auc_kernels_equal_host_reference(engine, name):
    m, y, _ = VECTORS[name]  # the tie5000_* groups span 20 workgroups of the count kernel
    assert EC.bits64(engine.gbdt_metric(m, y, "auc")) == EC.bits64(gbdt_metric_ref_host(m, y, "auc"))


def test_auc_kernels_take_nan_as_the_host_does(engine):
    m = np.array([np.nan, np.inf, -np.nan, 1.0, np.nan, -np.inf], np.float32)
    y = np.array([1, 0, 1, 0, 0, 1], np.uint8)
    assert EC.bits64(engine.gbdt_metric(m, y, "auc")) == EC.bits64(gbdt_metric_ref_host(m, y, "auc"))


@pytest.mark.parametrize("name", list(EC.error_vectors()))
def test_error_kernel_equals_host_reference(engine, name):
    m, y = EC.error_vectors()[name]
    assert engine.gbdt_metric(m, y, "error") == gbdt_metric_ref_host(m, y, "error") == EC.error_numpy(m, y)


# ------------------------------------------------------------------ 2. eval fits
@pytest.mark.parametrize("n_eval", [2, 65, 1025])
@pytest.mark.parametrize("name", list(GC.FIT_CASES))
def test_eval_fit_equals_host_reference(engine, name, n_eval):
    import torch
    X, y, params = GC.fit_case(name)
    Xe, ye = EC.eval_rows(name, n_eval)
    if name == "nan_257x64":
        assert np.isnan(Xe).any()
    want = gbdt_fit_ref_host(X, y, eval_set=(Xe, ye), **params)
    c0 = _counters(engine)
    got = engine.fit_gbdt(X, y, eval_set=(Xe, ye), **params)
    R, D = params["n_rounds"], params["max_depth"]
    assert _advance(engine, c0) == {"gbdt_trees": R, "gbdt_hist_launches": R * D, "gbdt_eval_launches": R,
                                    "gbdt_rounds_run": R}
    _same_watched_fit(got, want, f"{name}, {n_eval} eval rows, numpy")
    dev = torch.device("cuda", engine.device)
    t = [torch.from_numpy(a).to(dev) for a in (X, y, Xe, ye)]
    got = engine.fit_gbdt(t[0], t[1], eval_set=[(t[2], t[3])], **params)
    _same_watched_fit(got, want, f"{name}, {n_eval} eval rows, device tensors")
    if n_eval == 65:
        err = engine.fit_gbdt(X, y, eval_set=(Xe, ye), eval_metric="error", **params)
        _same_watched_fit(err, gbdt_fit_ref_host(X, y, eval_set=(Xe, ye), eval_metric="error", **params),
                          f"{name}: error")


def test_class_weight_fit_equals_host_reference(engine):
    X, y, params = GC.fit_case("nan_257x64")
    Xe, ye = EC.eval_rows("nan_257x64", 65)
    for w in (0.25, 19.0):
        _same_watched_fit(engine.fit_gbdt(X, y, eval_set=(Xe, ye), scale_pos_weight=w, **params),
                          gbdt_fit_ref_host(X, y, eval_set=(Xe, ye), scale_pos_weight=w, **params), f"w = {w}")
    got = engine.fit_gbdt(X, y, scale_pos_weight=19.0, **params)  # the weight alone: no eval set
    want = gbdt_fit_ref_host(X, y, scale_pos_weight=19.0, **params)
    GC.assert_same_tree(GC.tree_fields(got), GC.tree_fields(want), "weight only")
    np.testing.assert_array_equal(EC.bits32(got.meta["margins"]), EC.bits32(want.meta["margins"]))
    assert "evals_result" not in got.meta


# ------------------------------------------------------------------ 3. serving as the independent oracle
def test_eval_margins_equal_served_raw_output(engine):
    X, y, params = GC.fit_case("trainer_4099x33")
    Xe, ye = EC.eval_rows("trainer_4099x33", 1025)
    fa = engine.fit_gbdt(X, y, eval_set=(Xe, ye), **params)
    assert fa.n_trees == params["n_rounds"]  # nothing was cut
    raw = _served_raw(engine, fa, Xe)
    np.testing.assert_array_equal(EC.bits32(raw), EC.bits32(fa.meta["eval_margins"]))
    curve = fa.meta["evals_result"]["validation_0"]["auc"]
    assert EC.bits64(curve[-1]) == EC.bits64(roc_auc_midrank(ye, raw))


# ------------------------------------------------------------------ 4. early stopping
@pytest.mark.parametrize("metric", ["auc", "error"])
def test_early_stopping_fires_on_the_saturating_case(engine, metric):
    X, y, _ = GC.threshold_case(n=200)
    rows = np.arange(0, 200, 3)
    Xe, ye = X[rows], y[rows]
    kw = dict(n_rounds=40, max_bin=256, eval_set=(Xe, ye), eval_metric=metric, early_stopping_rounds=3)
    c0 = _counters(engine)
    fa = engine.fit_gbdt(X, y, **kw)
    # launches that returned at the stop flag are not counted: the counters advance by the rounds that ran
    assert _advance(engine, c0) == {"gbdt_trees": 4, "gbdt_hist_launches": 4 * 6, "gbdt_eval_launches": 4,
                                    "gbdt_rounds_run": 4}
    curve = fa.meta["evals_result"]["validation_0"][metric]
    assert fa.meta["best_iteration"] == 0 and fa.meta["rounds_run"] == 4 and len(curve) == 4
    assert curve[0] == (1.0 if metric == "auc" else 0.0)
    assert fa.n_trees == 1
    _same_watched_fit(fa, gbdt_fit_ref_host(X, y, **kw), metric)
    np.testing.assert_array_equal(EC.bits32(_served_raw(engine, fa, X)), EC.bits32(fa.meta["margins"]))
    assert _c_abi_trees(engine, X, y, Xe, ye, metric) == (4, 4, 0)


def _c_abi_trees(engine, X, y, Xe, ye, metric):
    """fd_gbdt_fit_eval_host called directly -> (trees written, rounds_run, best_iteration)"""
    import ctypes as C
    from fdengine import _native as N
    from fdengine.engine import _GbdtOut, _gbdt_eval_struct, _gbdt_xy, _ptr, gbdt_params
    X, y = _gbdt_xy(X, y)
    p = gbdt_params(n_rounds=40, max_bin=256)
    ev, keep = _gbdt_eval_struct((Xe, ye), metric, 3, 1.0, p, *X.shape)
    cap = C.c_int64()
    args = (engine._h, _ptr(X), _ptr(y), X.shape[0], X.shape[1], X.shape[1], C.byref(p))
    N.call("fd_gbdt_fit_eval_host", *args, None, None, C.byref(cap), None)
    out = _GbdtOut(p.n_rounds, cap.value)
    out.a["offsets"][:] = -1
    nn = C.c_int64()
    N.call("fd_gbdt_fit_eval_host", *args, C.byref(ev), C.byref(out.model), C.byref(nn), None)
    written = int((out.a["offsets"] >= 0).sum()) - 1
    assert out.a["offsets"][written] == nn.value
    return written, ev.rounds_run, ev.best_iteration


@pytest.fixture(scope="module")
def noisy():
    X, y, params = GC.fit_case("trainer_4099x33")
    params["n_rounds"] = 30
    cut = 3 * len(X) // 4
    return X[:cut], y[:cut], X[cut:], y[cut:], params


@pytest.mark.parametrize("metric", ["auc", "error"])
def test_early_stopping_equals_the_rule_applied_to_the_full_curve(engine, noisy, metric):
    X, y, Xe, ye, params = noisy
    full = engine.fit_gbdt(X, y, eval_set=(Xe, ye), eval_metric=metric, **params)
    curve = full.meta["evals_result"]["validation_0"][metric]
    run, best = EC.stop_rule(curve, 2, maximise=metric == "auc")
    assert run < 30, "the case must stop"
    c0 = _counters(engine)
    got = engine.fit_gbdt(X, y, eval_set=(Xe, ye), eval_metric=metric, early_stopping_rounds=2, **params)
    assert _advance(engine, c0) == {"gbdt_trees": run, "gbdt_hist_launches": run * params["max_depth"],
                                    "gbdt_eval_launches": run, "gbdt_rounds_run": run}
    assert (got.meta["rounds_run"], got.meta["best_iteration"]) == (run, best)
    assert got.meta["evals_result"]["validation_0"][metric] == curve[:run] and got.n_trees == best + 1
    GC.assert_same_tree(GC.tree_fields(got), EC.prefix_fields(full, best + 1), metric)
    _same_watched_fit(got, gbdt_fit_ref_host(X, y, eval_set=(Xe, ye), eval_metric=metric, early_stopping_rounds=2,
                                             **params), metric)
    # the cut forest's margins are what serving reports for the training rows
    np.testing.assert_array_equal(EC.bits32(_served_raw(engine, got, X)), EC.bits32(got.meta["margins"]))


# ------------------------------------------------------------------ 5. launch shape
def test_launch_shape_does_not_change_the_curve_or_the_trees(engine):
    X, y, params = GC.fit_case("trainer_4099x33")
    Xe, ye = EC.eval_rows("trainer_4099x33", 1025)
    params["n_rounds"] = 4
    fits = []
    try:
        for rows in (64, 4096, 1 << 20):
            engine.set_option("gbdt_hist_rows", rows)
            fits.append(engine.fit_gbdt(X, y, eval_set=(Xe, ye), early_stopping_rounds=3, **params))
    finally:
        engine.set_option("gbdt_hist_rows", 4096)
    for f in fits[1:]:
        _same_watched_fit(f, fits[0], "gbdt_hist_rows")


# ------------------------------------------------------------------ 6. without the new arguments
def test_plain_fit_launches_no_eval_kernel(engine):
    X, y, params = GC.fit_case("deep_65x1")
    c0 = _counters(engine)
    got = engine.fit_gbdt(X, y, **params)
    R, D = params["n_rounds"], params["max_depth"]
    assert _advance(engine, c0) == {"gbdt_trees": R, "gbdt_hist_launches": R * D, "gbdt_eval_launches": 0,
                                    "gbdt_rounds_run": R}
    want = gbdt_fit_ref_host(X, y, **params)
    GC.assert_same_tree(GC.tree_fields(got), GC.tree_fields(want), "plain")
    assert "evals_result" not in got.meta and "rounds_run" not in got.meta


# ------------------------------------------------------------------ 7. the drop-in
@pytest.fixture(scope="module")
def frame(tmp_path_factory):
    df = ModelTrainer(output_dir=str(tmp_path_factory.mktemp("frame")))._generate_synthetic_data(2000)
    feats = [c for c in df.columns if c not in ("is_fraud", "transaction_id", "user_id", "merchant_id")]
    return df[feats].values, df["is_fraud"].values, 1600


def test_model_trainer_defaults_write_todays_file_and_keep_the_curve(engine, tmp_path, frame):
    X, y, cut = frame
    tr = ModelTrainer(output_dir=str(tmp_path), engine=engine)
    res = tr.train_xgboost_model(X[:cut], y[:cut], X[cut:], y[cut:])
    assert list(res) == ["model_type", "model_path", "auc_score", "training_time_seconds", "feature_importance"]
    want = gbdt_fit_ref_host(X[:cut], y[:cut], n_rounds=100, max_depth=6, eta=0.1, subsample=0.8, colsample_bytree=0.8,
                             seed=42)
    doc = json.loads(open(res["model_path"]).read())
    assert doc == json.loads(json.dumps(xgboost_doc_from_forest(want)))
    curve = tr.evals_result_["validation_0"]["auc"]
    assert len(curve) == 100
    engine.load_xgboost_file(SLOT, res["model_path"])
    try:
        raw = engine.predict(SLOT, X[cut:].astype(np.float32), want_raw=True)[1]
    finally:
        engine.unload_forest(SLOT)
    assert EC.bits64(curve[-1]) == EC.bits64(roc_auc_midrank(y[cut:], raw))


def test_model_trainer_with_early_stopping_and_class_weight(engine, tmp_path, frame):
    X, y, cut = frame
    tr = ModelTrainer(output_dir=str(tmp_path), engine=engine)
    tr.early_stopping_rounds, tr.scale_pos_weight = 5, 19.0
    res = tr.train_xgboost_model(X[:cut], y[:cut], X[cut:], y[cut:])
    curve = tr.evals_result_["validation_0"]["auc"]
    best = int(np.argmax(curve))  # the first maximum: a later equal value is no improvement
    assert len(curve) == min(100, best + 6)
    from fdengine import load_xgboost_json
    assert load_xgboost_json(res["model_path"]).n_trees == best + 1
    engine.load_xgboost_file(SLOT, res["model_path"])
    try:
        raw = engine.predict(SLOT, X[cut:].astype(np.float32), want_raw=True)[1]
    finally:
        engine.unload_forest(SLOT)
    assert EC.bits64(roc_auc_midrank(y[cut:], raw)) == EC.bits64(curve[best])
