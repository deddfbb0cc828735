"""CPU: the host side of the histogram GBDT fit — the split search of fd_gbdt_grow_tree_ref_host against
the numpy brute force of tests/gbdt_cases.py, cuts and binning at their edges, the fixed-point gradients against
numpy's f64 sigmoid, the fit's margins against the forest oracle, the XGBoost JSON round trip, that it learns, the AUC
helper, the ModelTrainer drop-in's shape, and the kernels' compiled resources. No device code runs here."""
import inspect
import json
from pathlib import Path

import numpy as np
import pytest

import gbdt_cases as GC
import oracle
from fdengine import (ForestArrays, gbdt_cuts_host, gbdt_fit_ref_host, gbdt_grow_tree_ref_host, synth,
                      xgboost_doc_from_forest, xgboost_from_json_doc)
from fdengine import _native as N
from fdengine.build import RESOURCES
from fdengine.engine import (gbdt_bin_ref_host, gbdt_grad_ref_host, read_xgboost_json_cover_native,
                             read_xgboost_json_native)
from fdengine.training import ModelTrainer, gain_importance, roc_auc_midrank, stratified_split
from oracle import forest_ref

GOLDEN = Path(__file__).resolve().parent / "golden" / "model_trainer_names.json"


# ------------------------------------------------------------------ 1. split search against brute force
@pytest.mark.parametrize("name", GC.SPLIT_CASES)
def test_split_search_against_brute_force(name):
    c = GC.split_inputs(name, gbdt_cuts_host)
    want = GC.grow_tree_numpy(c["bins"], c["cuts"], c["offsets"], c["g"], c["h"], c["row_mask"], c["feature_mask"],
                              **c["params"])
    got = gbdt_grow_tree_ref_host(c["bins"], c["cuts"], c["offsets"], c["g"], c["h"], c["row_mask"],
                                  c["feature_mask"], **c["params"])
    GC.assert_same_tree(GC.tree_fields(got), want, name)
    n_nodes = len(want["left"])
    split = want["left"] >= 0
    if name in ("root_cannot_split", "labels_equal", "row_mask_empty", "rows1"):
        assert n_nodes == 1
    if name in ("rows4099", "rows257_depth10", "rows65_f1_depth10", "identical_columns", "nan_rows_positive"):
        assert n_nodes > 1, "the case must exercise the search"
    if name == "constant_column" or name == "all_nan_column":
        assert c["offsets"][1] == 0 and not (want["feature"][split] == 0).any()
    if name == "identical_columns":
        assert not np.isin(want["feature"][split], (1, 2)).any()  # the lower index wins every tie
    if name == "nan_rows_positive":
        assert want["feature"][0] == 0 and want["default_left"][0] == 1
    if name == "one_feature_mask":
        assert n_nodes > 1 and (want["feature"][split] == 2).all()
    if name == "rows257_depth10":
        assert n_nodes < 2 ** 11 - 1  # most of the depth-10 heap stays empty
    if name == "row_mask_empty":
        assert np.signbit(want["leaf_value"][0]) and want["sum_hessian"][0] == 0.0  # -0 / (0 + lambda) * eta


def test_grow_tree_rejects_bad_arguments():
    c = GC.split_inputs("rows63_f33_bin16", gbdt_cuts_host)
    for bad in (dict(max_depth=0), dict(max_depth=11), dict(reg_lambda=-1.0), dict(reg_lambda=0.0,
                                                                                     min_child_weight=0.0)):
        with pytest.raises(N.NativeError) as ei:
            gbdt_grow_tree_ref_host(c["bins"], c["cuts"], c["offsets"], c["g"], c["h"], **dict(c["params"], **bad))
        assert ei.value.code == N.FD_ERR_INVALID_ARG
    with pytest.raises(N.NativeError):
        gbdt_grow_tree_ref_host(c["bins"], c["cuts"], c["offsets"], c["g"], c["h"], feature_mask=0, **c["params"])


# ------------------------------------------------------------------ 2. cuts and binning
@pytest.mark.parametrize("max_bin", [2, 16, 256])
def test_cuts_are_the_declared_quantiles(max_bin):
    rng = np.random.default_rng(3)
    X = GC._matrix(rng, 1000, 8, nan_frac=0.1)
    X[:, 4] = np.nan
    X[:, 5] = 2.5
    X[:, 6] = np.arange(1000)  # 1000 distinct values: max_bin 256 gives 255 candidates, clamped to 254
    cuts, off = gbdt_cuts_host(X, max_bin)
    assert off[0] == 0 and len(cuts) == off[-1]
    for f in range(8):
        v = np.sort(X[~np.isnan(X[:, f]), f])
        want = []
        for k in range(1, max_bin):
            if len(v) == 0:
                break
            c = v[k * len(v) // max_bin]
            if c != v[0] and (not want or c != want[-1]):
                want.append(c)
        want = np.asarray(want[:254], np.float32)
        np.testing.assert_array_equal(cuts[off[f]:off[f + 1]], want)
    assert off[5] - off[4] == 0 and off[6] - off[5] == 0
    if max_bin == 256:
        assert off[7] - off[6] == 254


def test_binning_convention_and_edge_values():
    X = GC.edge_matrix()
    # cuts that sit on the values themselves: equality with a cut is the case that matters
    cuts, off = gbdt_cuts_host(X, 256)
    bins = gbdt_bin_ref_host(X, cuts, off)
    np.testing.assert_array_equal(bins, GC.bin_numpy(X, cuts, off))
    for f in range(X.shape[1]):
        c = cuts[off[f]:off[f + 1]]
        assert len(c) > 3 and (np.diff(c) > 0).all()
        for r in range(X.shape[0]):
            x = X[r, f]
            if np.isnan(x):
                assert bins[r, f] == 255
                continue
            assert bins[r, f] < 255
            for j in range(len(c)):
                assert (bins[r, f] <= j) == bool(x < c[j]), (r, f, j)
    col = X[:, 0]
    b0 = bins[:, 0]
    assert b0[np.nonzero(np.signbit(col) & (col == 0))[0][0]] == b0[np.nonzero(~np.signbit(col) & (col == 0))[0][0]]
    assert b0[np.nonzero(col == -np.inf)[0][0]] == 0
    assert b0[np.nonzero(col == np.inf)[0][0]] == off[1] - off[0]  # +inf is a cut: every cut is <= it
    tiny = np.float32(1e-45)
    assert b0[np.nonzero(col == tiny)[0][0]] == b0[np.nonzero(col == 0)[0][0]] + 1  # a denormal is not flushed


def test_binning_random_against_numpy():
    rng = np.random.default_rng(4)
    X = GC._matrix(rng, 777, 13, nan_frac=0.07)
    for max_bin in (2, 16, 256):
        cuts, off = gbdt_cuts_host(X, max_bin)
        np.testing.assert_array_equal(gbdt_bin_ref_host(X, cuts, off), GC.bin_numpy(X, cuts, off))
        assert gbdt_bin_ref_host(X, cuts, off)[~np.isnan(X)].max() <= max_bin - 1


# ------------------------------------------------------------------ 3. gradients
def test_gradients_against_numpy_sigmoid():
    """Bound 2^-23: half a quantum (2^-25) for the rounding, one quantum (2^-24) where h takes its floor of one
    quantum, plus the sigmoid's own error (measured 1.7e-16 at worst over a dense f32 sweep): 1.5
    quanta and a little, under the 2 quanta asserted. Measured here: 3.0e-8 for g, 6.0e-8 for h."""
    big = np.finfo(np.float32).max
    m = np.concatenate([np.linspace(-40, 40, 20001), [0.0, -0.0, 88.0, -88.0, big, -big, np.inf, -np.inf, 1e-30,
                                                     -1e-30, 16.6, -16.6, 17.4, -17.4]]).astype(np.float32)
    with np.errstate(over="ignore"):
        p = 1.0 / (1.0 + np.exp(-m.astype(np.float64)))
    for label in (0, 1):
        y = np.full(len(m), label, np.uint8)
        g, h = gbdt_grad_ref_host(m, y)
        eg = np.abs(g / GC.SCALE - (p - label)).max()
        eh = np.abs(h / GC.SCALE - p * (1 - p)).max()
        print(f"label {label}: max |g - (sigma - y)| = {eg:.3e}, max |h - sigma (1 - sigma)| = {eh:.3e}")
        assert eg <= 2.0 ** -23 and eh <= 2.0 ** -23
        assert (h >= 1).all()
    g0, h0 = gbdt_grad_ref_host(np.zeros(1, np.float32), np.zeros(1, np.uint8))
    assert g0[0] == 2 ** 23 and h0[0] == 2 ** 22  # sigma(0) = 1/2 exactly
    with pytest.raises(N.NativeError):
        gbdt_grad_ref_host(np.zeros(2, np.float32), np.array([0, 2], np.uint8))


# ------------------------------------------------------------------ 4. fit consistency
def test_fit_margins_equal_the_oracle_walk():
    X, y, params = GC.fit_case("nan_257x64")
    fa = gbdt_fit_ref_host(X, y, **params)
    assert fa.n_trees == params["n_rounds"] and fa.offsets[-1] == len(fa.left) > fa.n_trees
    margins = fa.meta["margins"]
    assert margins.dtype == np.float32
    # the pure-Python walker, row by row: rows outside every round's sample included (subsample 0.5, 5 rounds)
    walked = np.array([forest_ref.xgb_walk(fa, X[r])[0] for r in range(len(X))], np.float32)
    np.testing.assert_array_equal(walked.view(np.uint32), margins.view(np.uint32))
    raw = np.asarray(oracle.xgb_predict(fa, X, want_leaf=True)[1], np.float32)
    np.testing.assert_array_equal(raw.view(np.uint32), margins.view(np.uint32))


def test_fit_covers_are_consistent_and_seed_matters():
    X, y, params = GC.fit_case("trainer_4099x33")
    fa = gbdt_fit_ref_host(X, y, **params)
    raw = np.asarray(oracle.xgb_predict(fa, X, want_leaf=True)[1], np.float32)
    np.testing.assert_array_equal(raw.view(np.uint32), fa.meta["margins"].view(np.uint32))
    inner = fa.left >= 0
    off = np.repeat(fa.offsets[:-1], np.diff(fa.offsets))
    np.testing.assert_array_equal(fa.cover[inner], fa.cover[(off + fa.left)[inner]] + fa.cover[(off + fa.right)[inner]])
    assert (fa.cover > 0).all() and (fa.meta["loss_changes"][inner] > 1e-6).all()
    again = gbdt_fit_ref_host(X, y, **params)
    GC.assert_same_tree(GC.tree_fields(again), GC.tree_fields(fa), "same seed")
    other = gbdt_fit_ref_host(X, y, **dict(params, seed=43))
    assert len(other.left) != len(fa.left) or not np.array_equal(other.threshold, fa.threshold)


def test_fit_rejects_bad_arguments():
    X, y, params = GC.fit_case("deep_65x1")
    for bad in (dict(max_bin=1), dict(max_bin=257), dict(max_depth=11), dict(subsample=0.0), dict(subsample=1.5),
                dict(colsample_bytree=0.0), dict(n_rounds=0), dict(base_score=1.0)):
        with pytest.raises(N.NativeError) as ei:
            gbdt_fit_ref_host(X, y, **dict(params, **bad))
        assert ei.value.code == N.FD_ERR_INVALID_ARG, bad
    with pytest.raises(N.NativeError) as ei:
        gbdt_fit_ref_host(np.zeros((4, 65), np.float32), np.zeros(4, np.uint8))
    assert ei.value.code == N.FD_ERR_INVALID_ARG
    with pytest.raises(ValueError):
        gbdt_fit_ref_host(X, np.full(len(X), 2))
    # the row cap is checked before anything is read: the size query needs no buffers
    p = N.fd_gbdt_params(1, 6, 256, 0, 0.1, 1.0, 1.0, 1.0, 1.0, 0.5, 0)
    import ctypes as C
    cap = C.c_int64()
    rc = N.lib.fd_gbdt_fit_ref_host(None, None, 2 ** 28 + 1, 4, 4, C.byref(p), None, C.byref(cap), None)
    assert rc == N.FD_ERR_UNSUPPORTED
    rc = N.lib.fd_gbdt_fit_ref_host(None, None, 2 ** 28, 4, 4, C.byref(p), None, C.byref(cap), None)
    assert rc == 0 and cap.value == 127


# ------------------------------------------------------------------ 5. round trip
def test_json_round_trip(tmp_path):
    X, y, params = GC.fit_case("nan_257x64")
    fa = gbdt_fit_ref_host(X, y, base_score=0.25, **params)
    doc = xgboost_doc_from_forest(fa)
    path = tmp_path / "xgboost" / "fraud_classifier.json"
    path.parent.mkdir()
    synth.write_xgboost_json(str(path), doc)
    back = read_xgboost_json_native(path)
    py = xgboost_from_json_doc(json.loads(path.read_text()))
    for other in (back, py):
        assert other.num_feature == fa.num_feature and other.base_score == fa.base_score
        for k in ("offsets", "left", "right", "feature", "threshold", "default_left", "leaf_value"):
            np.testing.assert_array_equal(getattr(other, k), getattr(fa, k), err_msg=k)
    np.testing.assert_array_equal(read_xgboost_json_cover_native(path), fa.cover)
    np.testing.assert_array_equal(py.cover, fa.cover)
    trees = doc["learner"]["gradient_booster"]["model"]["trees"]
    assert doc["learner"]["learner_model_param"]["base_score"] == "2.500000E-01"
    assert set(trees[0]) == set(synth.xgboost_doc(1, 2, 4, X[:, :4])["learner"]["gradient_booster"]["model"]["trees"][0])
    for t, tr in enumerate(trees):
        s = slice(fa.offsets[t], fa.offsets[t + 1])
        assert tr["tree_param"]["num_nodes"] == str(s.stop - s.start) and tr["id"] == t
        assert tr["parents"][0] == 2147483647
        for i, (l, r) in enumerate(zip(tr["left_children"], tr["right_children"])):
            if l != -1:
                assert tr["parents"][l] == i and tr["parents"][r] == i
        np.testing.assert_array_equal(tr["loss_changes"], fa.meta["loss_changes"][s])
        np.testing.assert_array_equal(tr["base_weights"], fa.meta["base_weights"][s])
    # synth's writer is untouched: a forest read from its document goes back to equal arrays
    fa2 = xgboost_from_json_doc(synth.xgboost_doc(4, 3, 6, X[:, :6], seed=9, p_leaf=0.3))
    again = xgboost_from_json_doc(xgboost_doc_from_forest(fa2))
    for k in ("offsets", "left", "right", "feature", "threshold", "default_left", "leaf_value", "cover"):
        np.testing.assert_array_equal(getattr(again, k), getattr(fa2, k), err_msg=k)


# ------------------------------------------------------------------ 6. it learns
def test_stump_finds_the_threshold():
    X, y, c = GC.threshold_case()
    fa = gbdt_fit_ref_host(X, y, n_rounds=1, max_depth=1)
    cuts, off = gbdt_cuts_host(X, 256)
    c0 = cuts[off[0]:off[1]]
    assert fa.feature[0] == 0 and fa.left[0] == 1
    assert np.float32(fa.threshold[0]) == c0[c0 >= c].min()  # the nearest cut at or above c
    assert fa.leaf_value[1] < 0 < fa.leaf_value[2]


def _trainer_split(tmp_path, rows=2000):
    tr = ModelTrainer(output_dir=str(tmp_path))
    df = tr._generate_synthetic_data(rows)
    feats = [c for c in df.columns if c not in ("is_fraud", "transaction_id", "user_id", "merchant_id")]
    X, y = df[feats].values.astype(np.float32), df["is_fraud"].values
    a, b = stratified_split(y, 0.2, 42)
    return X[a], y[a], X[b], y[b]


def test_learns_as_well_as_sklearn_hist_gbdt(tmp_path):
    """The drop-in's synthetic set, 2,000 rows, 20 rounds, depth 6, eta 0.1, lambda 1, held-out AUC against
    HistGradientBoostingClassifier at the same settings. The margin is scikit-learn's own spread over ten
    random_state values on this split (max - min); the engine may lie below scikit-learn's median by at most that.
    Measured here: see DESIGN §4.14 (the test prints both)."""
    ens = pytest.importorskip("sklearn.ensemble")
    Xa, ya, Xb, yb = _trainer_split(tmp_path)
    fa = gbdt_fit_ref_host(Xa, ya, n_rounds=20, max_depth=6, eta=0.1, seed=42)
    ours = roc_auc_midrank(yb, oracle.xgb_predict(fa, Xb, want_leaf=True)[1])
    theirs = []
    for rs in range(10):
        m = ens.HistGradientBoostingClassifier(max_iter=20, max_depth=6, learning_rate=0.1, max_bins=255,
                                               l2_regularization=1.0, early_stopping=False, random_state=rs)
        m.fit(Xa, ya)
        theirs.append(roc_auc_midrank(yb, m.predict_proba(Xb)[:, 1]))
    med, spread = float(np.median(theirs)), float(max(theirs) - min(theirs))
    print(f"engine AUC {ours:.4f}; sklearn median {med:.4f}, spread {spread:.4f} over 10 seeds")
    assert spread < med - 0.5, "the label is too noisy for the comparison to mean anything"
    assert ours >= med - spread


# ------------------------------------------------------------------ 7. AUC helper
def test_auc_helper_equals_sklearn():
    metrics = pytest.importorskip("sklearn.metrics")
    rng = np.random.default_rng(8)
    y = (rng.random(500) < 0.3).astype(int)
    cases = {"continuous": rng.normal(size=500) + y, "heavy ties": np.round(rng.normal(size=500) + y),
             "two values": (rng.random(500) < 0.5 + 0.2 * y).astype(float), "all tied": np.zeros(500)}
    for name, s in cases.items():
        assert abs(roc_auc_midrank(y, s) - metrics.roc_auc_score(y, s)) <= 1e-12, name
    assert roc_auc_midrank(y, np.zeros(500)) == 0.5
    for single in (np.zeros(10, int), np.ones(10, int)):
        with pytest.raises(ValueError, match="Only one class"):
            roc_auc_midrank(single, np.arange(10.0))
        # scikit-learn raises that ValueError up to 1.6; later versions warn with the same words and return NaN
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            try:
                assert np.isnan(metrics.roc_auc_score(single, np.arange(10.0)))
            except ValueError as e:
                assert "Only one class" in str(e)


# ------------------------------------------------------------------ 8. drop-in shape
def test_model_trainer_has_the_reference_shape(tmp_path):
    names = json.loads(GOLDEN.read_text())
    sig = inspect.signature(ModelTrainer.__init__)
    assert list(sig.parameters)[1:1 + len(names["constructor_args"])] == names["constructor_args"]
    assert sig.parameters["output_dir"].default == names["constructor_default_output_dir"]
    tr = ModelTrainer(output_dir=str(tmp_path / "models"))
    assert (tmp_path / "models").is_dir()
    for a in names["attribute_names"]:
        assert hasattr(tr, a), a
    for a, v in names["attributes"].items():
        assert getattr(tr, a) == v
    for m in names["methods"]:
        assert callable(getattr(tr, m)), m
    assert list(inspect.signature(tr.train_xgboost_model).parameters) == ["X_train", "y_train", "X_test", "y_test"]
    assert list(inspect.signature(tr.prepare_training_data).parameters) == ["data_path"]
    df = tr._generate_synthetic_data()
    assert list(df.columns) == names["id_columns"][1:] + names["feature_columns"] + ["is_fraud"]
    assert len(df) == names["synthetic_rows"] and df["is_fraud"].mean() == names["fraud_rate"]
    Xa, Xb, ya, yb = tr.prepare_training_data()
    assert Xa.shape == (8000, 33) and Xb.shape == (2000, 33) and ya.mean() == yb.mean() == names["fraud_rate"]
    csv = tmp_path / "d.csv"
    df.iloc[:500].to_csv(csv, index=False)
    Xc, Xd, yc, yd = tr.prepare_training_data(str(csv))
    assert Xc.shape == (400, 33) and Xd.shape == (100, 33)
    tr.save_training_metadata({"xgboost": {"auc_score": np.float64(0.9), "feature_importance": {0: np.float64(1.0)}}})
    meta = json.loads((tmp_path / "models" / names["metadata_relpath"]).read_text())
    assert list(meta) == names["metadata_keys"]
    assert list(meta["configuration"]) == names["metadata_configuration_keys"]


def test_gain_importance_is_the_normalised_mean_gain():
    fa = ForestArrays(kind=N.FD_FOREST_XGB_BINARY_LOGISTIC, num_feature=3, offsets=np.array([0, 5, 8]),
                      left=np.array([1, 3, -1, -1, -1, 1, -1, -1]), right=np.array([2, 4, -1, -1, -1, 2, -1, -1]),
                      feature=np.array([0, 1, 0, 0, 0, 0, 0, 0]), threshold=np.zeros(8), default_left=np.zeros(8),
                      leaf_value=np.zeros(8), meta={"loss_changes": np.array([4.0, 3.0, 0, 0, 0, 2.0, 0, 0])})
    np.testing.assert_allclose(gain_importance(fa), [0.5, 0.5, 0.0])  # feature 0: mean(4, 2) = 3; feature 1: 3


# ------------------------------------------------------------------ compiled resources
def test_gbdt_kernels_do_not_spill():
    res = json.loads(RESOURCES.read_text())
    mine = {k: v for k, v in res.items() if "gbdt_" in k}
    assert len(mine) >= 7, sorted(mine)
    for k, v in mine.items():
        assert v["scratch"] == 0, k
    committed = json.loads((Path(__file__).resolve().parent.parent / "profiles" / "gbdt" /
                            "kernel_resources.json").read_text())
    assert set(committed) == set(mine)
