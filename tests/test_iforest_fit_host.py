"""CPU: the host side of the IsolationForest fit — fd_iforest_fit_ref_host and its two seams against
the numpy restatement of tests/iforest_fit_cases.py bit for bit, the invariants of every grown forest, the sampler, the
offset against numpy's percentile of the oracle's scores, bad arguments, the scikit-learn / joblib round trip, that it
isolates as scikit-learn's own fit does, the ModelTrainer drop-in (on an engine stub over the host reference) and the
kernels' compiled resources. No device code runs here."""
import functools
import inspect
import io
import json
from pathlib import Path

import numpy as np
import pytest

import iforest_fit_cases as IC
import oracle
from fdengine import (iforest_fit_grow_tree_ref_host, iforest_fit_ref_host, iforest_fit_sample_ref_host,
                      iforest_from_sklearn, sklearn_iforest_from_forest)
from fdengine import _native as N
from fdengine.build import RESOURCES
from fdengine.training import ModelTrainer, roc_auc_midrank


@functools.lru_cache(maxsize=None)
def _fits(name):
    X, p = IC.fit_case(name)
    return X, p, iforest_fit_ref_host(X, **p), IC.fit(X, **p)


def _ulps(a, b):
    return abs(a - b) / np.spacing(abs(b))


# ------------------------------------------------------------------ 1. the reference against the restatement
@pytest.mark.parametrize("name", IC.FIT_CASES)
def test_fit_equals_the_restatement(name):
    X, p, fa, want = _fits(name)
    assert fa.n_trees == p["n_estimators"] == len(want["trees"])
    for t, (got, w) in enumerate(zip(IC.forest_trees(fa), want["trees"])):
        IC.assert_same_tree(got, w, f"{name}: tree {t}")
    assert fa.meta["max_samples"] == want["psi"]
    assert fa.if_denominator == want["denominator"]
    if p.get("contamination", 0.0) == 0.0:
        assert fa.if_offset == -0.5
    else:
        assert _ulps(fa.if_offset, want["offset"]) <= 8
    split = fa.left >= 0
    if name == "n2_psi2_f1":
        assert list(fa.offsets) == [0, 3, 6, 9] and fa.meta["max_samples"] == 2
    if name == "n100_below_default_psi":
        assert fa.meta["max_samples"] == 100
    if name == "psi1024_f64_n5000":
        assert max(int(t["depth"].max()) for t in want["trees"]) == 10
    if name == "f33_ld40":
        assert fa.num_feature == 33 and fa.feature.max() < 33 and np.abs(fa.threshold).max() < 100
    if name == "all_rows_identical":
        assert len(fa.left) == 4 and (fa.leaf_value == IC.average_path_length(256)).all()
    if name == "three_constant_columns":
        assert split.sum() > 100 and not np.isin(fa.feature[split], (1, 4, 7)).any()
    if name == "signed_zero_column":
        assert split.sum() > 100 and not (fa.feature[split] == 1).any()
    if name == "heavy_duplicates":
        D = IC.depth_cap(256)
        depth = np.concatenate([t["depth"] for t in want["trees"]])
        assert ((fa.left == -1) & (fa.meta["n_node_samples"] > 1) & (depth < D)).any()
    if name == "column_spans_3e38":
        assert (fa.feature[split] == 0).any() and np.isfinite(fa.threshold).all()
    if name == "denormals":
        assert split.sum() > 100 and 0 < np.abs(fa.threshold[split]).max() < 1e-40
    if name == "max_features_half":
        for t, tr in enumerate(IC.forest_trees(fa)):
            kept = IC.kept_features(p["seed"], t, 9, 0.5)
            assert len(kept) == 4 and np.isin(tr["feature"][tr["left"] >= 0], kept).all()
        assert len({tuple(IC.kept_features(p["seed"], t, 9, 0.5)) for t in range(12)}) > 1
    if name == "u_rounds_up_to_max":
        # mn + u (mx - mn) rounded to mx and was put back to mn: the rows still part one and one
        assert fa.threshold[0] == 1.0 and list(fa.meta["n_node_samples"]) == [2, 1, 1]
        h2 = IC.hash_of(IC.key_of(p["seed"]), 0, 0, IC.TAG_THRESHOLD)
        u = np.float64(h2 >> 11) * 2.0 ** -53
        assert np.float64(1.0) + u * (np.float64(X[1, 0]) - np.float64(1.0)) == np.float64(X[1, 0])


@pytest.mark.parametrize("name", IC.FIT_CASES)
def test_invariants_of_a_grown_forest(name):
    from sklearn.ensemble._iforest import _average_path_length
    X, p, fa, want = _fits(name)
    n, F = len(X), fa.num_feature
    psi = fa.meta["max_samples"]
    D = IC.depth_cap(psi)
    counts = fa.meta["n_node_samples"]
    for t in range(fa.n_trees):
        rows = iforest_fit_sample_ref_host(n, t, **{k: p[k] for k in ("max_samples", "seed") if k in p})
        assert len(rows) == psi == len(set(rows.tolist())) and rows.min() >= 0 and rows.max() < n
        np.testing.assert_array_equal(rows, want["rows"][t])
        o = int(fa.offsets[t])
        m = int(fa.offsets[t + 1]) - o
        assert counts[o] == psi
        members, depth = {0: rows}, {0: 0}
        for i in range(m):  # breadth-first: a parent comes before its children
            l, r = fa.left[o + i], fa.right[o + i]
            if l < 0:
                assert depth[i] <= D and r == -1
                continue
            assert counts[o + l] + counts[o + r] == counts[o + i] and counts[o + l] >= 1 and counts[o + r] >= 1
            x = X[members[i], fa.feature[o + i]].astype(np.float64)
            thr = fa.threshold[o + i]
            assert x.min() <= thr < x.max()
            members[l], members[r] = members[i][x <= thr], members[i][~(x <= thr)]
            assert len(members[l]) == counts[o + l]
            depth[l] = depth[r] = depth[i] + 1
    assert fa.if_denominator == fa.n_trees * _average_path_length([psi])[0]
    other = iforest_fit_ref_host(X, **dict(p, seed=p["seed"] + 1))
    if name not in ("all_rows_identical", "n2_psi2_f1", "u_rounds_up_to_max"):  # (those have one possible shape)
        assert len(other.left) != len(fa.left) or not np.array_equal(other.threshold, fa.threshold)


# ------------------------------------------------------------------ 2. the sampler
@pytest.mark.parametrize("n", IC.SAMPLER_N)
def test_sampler_is_injective_and_equals_the_restatement(n):
    for tree, seed, ms in ((0, 0, 0), (7, 12345, 1024), (65535, 2 ** 64 - 1, 2)):
        rows = iforest_fit_sample_ref_host(n, tree, seed=seed, max_samples=ms)
        psi = IC.psi_of(n, ms)
        assert len(rows) == psi == len(set(rows.tolist())) and rows.min() >= 0 and rows.max() < n
        np.testing.assert_array_equal(rows, IC.sample_rows(n, psi, seed, tree))
    a = iforest_fit_sample_ref_host(n, 0, seed=1, max_samples=1024)
    if n > 3:
        assert not np.array_equal(a, iforest_fit_sample_ref_host(n, 1, seed=1, max_samples=1024))
        assert not np.array_equal(a, iforest_fit_sample_ref_host(n, 0, seed=2, max_samples=1024))


# ------------------------------------------------------------------ 3. one tree from explicit rows
@pytest.mark.parametrize("name", list(IC.GROW_CASES))
def test_grow_tree_equals_the_restatement(name):
    X, rows, mask, kept = IC.grow_inputs(name)
    for tree, seed in ((0, 0), (41, 99)):
        got = iforest_fit_grow_tree_ref_host(X, rows, tree, mask, seed=seed)
        want = IC.grow_tree(X, rows, seed, tree, kept)
        IC.assert_same_tree(IC.forest_trees(got)[0], want, name)
    if kept is not None:
        assert np.isin(got.feature[got.left >= 0], kept).all()
    if name in ("rows1", "rows2_same"):
        assert len(got.left) == 1 and got.leaf_value[0] == IC.average_path_length(len(rows))


# ------------------------------------------------------------------ 4. the offset
def test_offset_is_the_percentile_of_the_fit_rows_scores():
    X, p = IC.fit_case("n100_below_default_psi")
    X2 = np.random.Generator(np.random.PCG64(3)).normal(size=(1001, 4)).astype(np.float32)
    for data, base in ((X, p), (X2, dict(n_estimators=10, seed=5))):
        n = len(data)
        for c in (0.05, 0.5, 1.0 / n):
            fa = iforest_fit_ref_host(data, **dict(base, contamination=c))
            _, raw, _ = oracle.iforest_predict(fa, data)
            want = np.percentile(-(2.0 ** (-raw / fa.if_denominator)), 100.0 * c)
            print(f"n {n} contamination {c:.6f}: offset {fa.if_offset!r} numpy {float(want)!r} "
                  f"({_ulps(fa.if_offset, want):.1f} ulp)")
            assert _ulps(fa.if_offset, want) <= 8
            assert fa.meta["contamination"] == c
        auto = iforest_fit_ref_host(data, **dict(base, contamination=0))
        assert auto.if_offset == -0.5
        assert iforest_fit_ref_host(data, **dict(base, contamination="auto")).if_offset == -0.5
        np.testing.assert_array_equal(auto.threshold, fa.threshold)  # the offset changes no tree


# ------------------------------------------------------------------ 5. bad arguments
def test_fit_rejects_bad_arguments():
    X = np.random.Generator(np.random.PCG64(1)).normal(size=(50, 4)).astype(np.float32)
    bad = [dict(n_estimators=0), dict(n_estimators=65537), dict(max_samples=1), dict(max_samples=1025),
           dict(max_samples=-1), dict(max_features=0.0), dict(max_features=1.5), dict(contamination=-0.1),
           dict(contamination=0.6), dict(contamination=float("nan")), dict(num_feature=5), dict(num_feature=0)]
    for kw in bad:
        with pytest.raises(N.NativeError) as ei:
            iforest_fit_ref_host(X, **kw)
        assert ei.value.code == N.FD_ERR_INVALID_ARG, kw
    for value in (np.nan, np.inf, -np.inf):
        Y = X.copy()
        Y[17, 2] = value
        with pytest.raises(N.NativeError) as ei:
            iforest_fit_ref_host(Y, n_estimators=2)
        assert ei.value.code == N.FD_ERR_INVALID_ARG and "non-finite" in str(ei.value)
    Y = np.concatenate([X, np.full((50, 1), np.nan, np.float32)], axis=1)  # a NaN outside the model's columns is unseen
    assert iforest_fit_ref_host(Y, n_estimators=2, num_feature=4).n_trees == 2
    with pytest.raises(N.NativeError) as ei:
        iforest_fit_ref_host(X[:1], n_estimators=2)
    assert ei.value.code == N.FD_ERR_INVALID_ARG
    with pytest.raises(N.NativeError) as ei:
        iforest_fit_ref_host(np.zeros((2, 65), np.float32), n_estimators=2)
    assert ei.value.code == N.FD_ERR_INVALID_ARG
    # more than 2^31 - 1 rows: refused by the capacity call, before X is read
    import ctypes as C
    p = N.fd_iforest_fit_params(1, 0, 1.0, 0.0, 0)
    cap = C.c_int64()
    rc = N.lib.fd_iforest_fit_ref_host(None, 2 ** 31, 4, 4, C.byref(p), None, None, None, C.byref(cap))
    assert rc == N.FD_ERR_UNSUPPORTED
    rc = N.lib.fd_iforest_fit_ref_host(None, 2 ** 31 - 1, 4, 4, C.byref(p), None, None, None, C.byref(cap))
    assert rc == N.FD_OK and cap.value == 511
    p = N.fd_iforest_fit_params(7, 1024, 1.0, 0.0, 0)
    rc = N.lib.fd_iforest_fit_ref_host(None, 5000, 4, 4, C.byref(p), None, None, None, C.byref(cap))
    assert rc == N.FD_OK and cap.value == 7 * 2047
    with pytest.raises(TypeError):
        iforest_fit_ref_host(X, bootstrap=True)
    with pytest.raises(N.NativeError):
        iforest_fit_grow_tree_ref_host(X, np.array([50]))  # a row id outside [0, n)
    with pytest.raises(N.NativeError):
        iforest_fit_grow_tree_ref_host(X, np.arange(10), feature_mask=1 << 4)  # keeps no feature of the four
    with pytest.raises(N.NativeError):
        iforest_fit_sample_ref_host(1, 0)


# ------------------------------------------------------------------ 6. scikit-learn round trip
def test_sklearn_round_trip_and_decision_function():
    import joblib
    X, p = IC.fit_case("max_features_half")
    for data, params in ((X, p), IC.fit_case("heavy_duplicates"), IC.fit_case("all_rows_identical")):
        fa = iforest_fit_ref_host(data, **params)
        buf = io.BytesIO()
        joblib.dump(sklearn_iforest_from_forest(fa), buf)
        buf.seek(0)
        model = joblib.load(buf)
        back = iforest_from_sklearn(model)
        for k in ("offsets", "left", "right", "feature", "threshold", "default_left", "leaf_value", "cover"):
            np.testing.assert_array_equal(getattr(back, k), getattr(fa, k), err_msg=k)
        assert back.if_offset == fa.if_offset and back.if_denominator == fa.if_denominator
        assert back.num_feature == fa.num_feature and back.kind == fa.kind
        Q = np.random.Generator(np.random.PCG64(9)).normal(size=(500, data.shape[1])).astype(np.float32)
        Q[:len(data[:100])] = data[:100]
        _, raw, _ = oracle.iforest_predict(fa, Q)
        want = -(2.0 ** (-raw / fa.if_denominator)) - fa.if_offset
        np.testing.assert_allclose(model.decision_function(Q), want, rtol=0, atol=1e-12)
        np.testing.assert_array_equal(model.predict(Q) == -1, want < 0)
        assert model.max_samples_ == fa.meta["max_samples"] and len(model.estimators_) == fa.n_trees


# ------------------------------------------------------------------ 7. it isolates as scikit-learn does
def test_isolates_as_sklearn_does():
    from sklearn.ensemble import IsolationForest
    Xf, Xt, y = IC.planted()
    sk, eng = [], []
    for seed in range(10):
        m = IsolationForest(n_estimators=100, contamination=0.05, random_state=seed).fit(Xf)
        fs = iforest_from_sklearn(m)
        sk.append((roc_auc_midrank(y, -m.decision_function(Xt)),
                   float(oracle.iforest_predict(fs, Xf)[1].mean()) / fs.n_trees))
        fa = iforest_fit_ref_host(Xf, n_estimators=100, contamination=0.05, seed=seed)
        eng.append((roc_auc_midrank(y, -oracle.iforest_predict(fa, Xt)[1]),
                    float(oracle.iforest_predict(fa, Xf)[1].mean()) / fa.n_trees))
    sk, eng = np.array(sk), np.array(eng)
    for k, what in enumerate(("held-out AUC of -raw", "mean path length per tree over the fit rows")):
        lo, hi = sk[:, k].min(), sk[:, k].max()
        spread = hi - lo
        print(f"{what}: scikit-learn {lo:.4f} .. {hi:.4f} over ten random_states; engine "
              f"{eng[:, k].min():.4f} .. {eng[:, k].max():.4f} over ten seeds")
        assert spread > 0
        assert (eng[:, k] >= lo - spread).all() and (eng[:, k] <= hi + spread).all()


# ------------------------------------------------------------------ 8. the drop-in, on the host reference
class _EngineStub:
    """What train_isolation_forest asks of an engine, answered by the host reference and the CPU oracle."""

    def __init__(self):
        self.forests, self.fitted = {}, []

    def fit_iforest(self, X, **params):
        self.fitted.append((np.asarray(X).shape, dict(params)))
        return iforest_fit_ref_host(X, **params)

    def load_forest(self, slot, fa):
        self.forests[slot] = fa

    def unload_forest(self, slot):
        del self.forests[slot]

    def predict(self, slot, X, want_raw=False, want_leaf=False):
        prob, raw, _ = oracle.iforest_predict(self.forests[slot], X)
        return (prob, raw) if want_raw else prob


def test_model_trainer_fits_the_isolation_forest_on_the_engine(tmp_path, monkeypatch):
    import joblib
    from sklearn.ensemble import IsolationForest
    real_fit = IsolationForest.fit

    def guarded_fit(self, X, y=None, sample_weight=None):
        assert np.asarray(X).shape[0] <= 2, "IsolationForest.fit saw the training data"
        return real_fit(self, X, y, sample_weight)

    monkeypatch.setattr(IsolationForest, "fit", guarded_fit)
    eng = _EngineStub()
    tr = ModelTrainer(output_dir=str(tmp_path), engine=eng)
    assert list(inspect.signature(tr.train_isolation_forest).parameters) == ["X_train", "y_train", "X_test", "y_test"]
    df = tr._generate_synthetic_data(1500)
    feats = [c for c in df.columns if c not in ("is_fraud", "transaction_id", "user_id", "merchant_id")]
    X, y = df[feats].values, df["is_fraud"].values
    cut = 1200
    res = tr.train_isolation_forest(X[:cut], y[:cut], X[cut:], y[cut:])
    assert list(res) == ["model_type", "model_path", "auc_score", "training_time_seconds"]
    assert res["model_type"] == "isolation_forest"
    assert res["model_path"] == str(tmp_path / "sklearn" / "isolation_forest.joblib")
    (shape, params), = eng.fitted
    assert shape == (int((y[:cut] == 0).sum()), 33)  # normal transactions only
    assert params == dict(n_estimators=100, contamination=0.05, seed=42)
    assert not eng.forests  # the scoring slot was given back
    model = joblib.load(res["model_path"])
    want = iforest_fit_ref_host(X[:cut][y[:cut] == 0], n_estimators=100, contamination=0.05, seed=42)
    back = iforest_from_sklearn(model)
    for k in ("offsets", "left", "right", "feature", "threshold", "leaf_value"):
        np.testing.assert_array_equal(getattr(back, k), getattr(want, k), err_msg=k)
    assert model.offset_ == want.if_offset and model.contamination == 0.05
    assert res["auc_score"] == roc_auc_midrank(y[cut:], -oracle.iforest_predict(want, X[cut:].astype(np.float32))[1])
    assert res["auc_score"] == pytest.approx(roc_auc_midrank(y[cut:], -model.decision_function(X[cut:])), abs=1e-3)
    tr.save_training_metadata({"isolation_forest": res})
    assert (tmp_path / "training_metadata.json").exists()


# ------------------------------------------------------------------ compiled resources
def test_iforest_fit_kernels_do_not_spill():
    res = json.loads(RESOURCES.read_text())
    mine = {k: v for k, v in res.items() if "iforest_fit_" in k}
    assert len(mine) >= 3, sorted(mine)
    for k, v in mine.items():
        assert v["scratch"] == 0, k
        assert not any(s in k for s in ("gbdt_", "shap", "mlp_", "metrics_record_kernel")), k
    committed = json.loads((Path(__file__).resolve().parent.parent / "profiles" / "iforest_fit" /
                            "kernel_resources.json").read_text())
    assert set(committed) == set(mine)
