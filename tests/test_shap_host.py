"""CPU: the host side of forest attribution (path-dependent TreeSHAP) — covers through the loaders, the
path table, the recursive host reference against the brute-force Shapley sum, the tolerance measurement, the kernels'
compiled resources, and the drop-in's switch left off. No device code runs here."""
import json

import numpy as np
import pytest

import shap_cases as SC
from fdengine import ForestArrays, shap_paths_host, shap_ref_host, synth, xgboost_from_json_doc
from fdengine import _native as N
from fdengine.build import RESOURCES
from fdengine.engine import read_xgboost_json_cover_native, read_xgboost_json_native


# ------------------------------------------------------------------ covers
def test_json_reader_keeps_sum_hessian(tmp_path):
    fa, _ = SC.small_cases()["xgb"]
    Xr = SC.background()
    doc = synth.xgboost_doc(6, 4, SC.NF, Xr, seed=323, p_leaf=0.2, base_score=0.35)
    want = SC.with_covers(doc, Xr)  # overwrites the document's sum_hessian
    synth.write_xgboost_json(str(tmp_path / "m.json"), doc)
    cover = read_xgboost_json_cover_native(tmp_path / "m.json")
    flat = np.concatenate([tr["sum_hessian"] for tr in doc["learner"]["gradient_booster"]["model"]["trees"]])
    np.testing.assert_array_equal(cover, flat)
    np.testing.assert_array_equal(want.cover, flat)
    np.testing.assert_array_equal(read_xgboost_json_native(tmp_path / "m.json").left, want.left)
    # consistent: a parent is the exact sum of its children
    inner = want.left >= 0
    off = np.repeat(want.offsets[:-1], np.diff(want.offsets))
    np.testing.assert_array_equal(want.cover[inner],
                                  want.cover[(off + want.left)[inner]] + want.cover[(off + want.right)[inner]])


def test_json_without_sum_hessian_has_no_cover(tmp_path):
    doc = synth.xgboost_doc(3, 3, SC.NF, SC.background(), seed=5)
    for tr in doc["learner"]["gradient_booster"]["model"]["trees"]:
        del tr["sum_hessian"]
    assert xgboost_from_json_doc(doc).cover is None
    synth.write_xgboost_json(str(tmp_path / "m.json"), doc)
    with pytest.raises(N.NativeError) as ei:
        read_xgboost_json_cover_native(tmp_path / "m.json")
    assert ei.value.code == N.FD_ERR_INVALID_ARG


def test_sklearn_covers_are_weighted_n_node_samples():
    from fdengine import forest_from_sklearn_classifier, iforest_from_sklearn
    bg = SC.background()
    ifm = synth.isolation_forest(bg.astype(np.float64), n_estimators=5, max_samples=64, random_state=326)
    rfm = synth.random_forest(bg, synth.fraud_labels(bg), n_estimators=6, random_state=328, max_depth=5)
    for fa, ests in ((iforest_from_sklearn(ifm), ifm.estimators_), (forest_from_sklearn_classifier(rfm), rfm.estimators_)):
        np.testing.assert_array_equal(fa.cover, np.concatenate([e.tree_.weighted_n_node_samples for e in ests]))
        assert fa.cover.dtype == np.float64 and len(fa.cover) == len(fa.left)


@pytest.mark.parametrize("bad", [0.0, -1.0, np.nan, np.inf])
def test_unusable_covers_are_rejected(bad):
    fa, X = SC.small_cases()["hand"]
    cover = fa.cover.copy()
    cover[int(fa.offsets[2]) + 4] = bad  # tree 2, node 4
    broken = ForestArrays(**{**fa.__dict__, "cover": cover})
    for call in (lambda: shap_paths_host(broken), lambda: shap_ref_host(broken, X)):
        with pytest.raises(N.NativeError) as ei:
            call()
        assert ei.value.code == N.FD_ERR_INVALID_ARG
        assert "tree 2 node 4" in str(ei.value)


# ------------------------------------------------------------------ the path table
@pytest.mark.parametrize("key", ["hand", "stump", "xgb", "iforest", "rf", "et"])
def test_path_table(key):
    fa, _ = SC.small_cases()[key]
    paths, elems, info = shap_paths_host(fa)
    want = SC.python_paths(fa)
    # one path per leaf, trees in order, leaves left-first; the unique features in order of first appearance
    assert info.n_paths == len(paths) == len(want) == int((fa.left < 0).sum())
    assert info.n_elems == len(elems) == sum(len(els) for _, _, els in want)
    lv = SC.leaf_values(fa)
    at = 0
    for p, (tree, leaf, els) in zip(paths, want):
        assert (p["tree"], p["len"], p["elem_offset"]) == (tree, len(els), at)
        assert p["value"] == lv[leaf]
        el = elems[at:at + len(els)]
        assert list(el["feature"]) == [f for f, _, _ in els] and len(set(el["feature"])) == len(els)
        np.testing.assert_allclose(el["z"], [z for _, _, z in els], rtol=1e-15)
        np.testing.assert_allclose(p["pz"], np.prod([z for _, _, z in els]), rtol=1e-14)
        for e, (_, edges, _) in zip(el, els):  # nan_follows: every edge is its node's default direction
            assert bool(e["nan_follows"]) == all(bool(fa.default_left[node]) == left for node, left in edges)
            assert bool(e["has_hi"]) == any(left for _, left in edges)
        at += len(els)
    # per tree the leaves' shares of the weight sum to 1, to the rounding of the cover ratios
    for t in range(fa.n_trees):
        sel = paths["tree"] == t
        assert abs(paths["pz"][sel].sum() - 1.0) <= 1e-14 * sel.sum()
    assert info.max_len == paths["len"].max() <= N.FD_SHAP_MAX_PATH
    assert info.n_chunks == -(-info.n_paths // info.chunk_paths) and 1 <= info.n_chunks <= 32
    want_bias = float((paths["value"] * paths["pz"]).sum()) + SC.base_margin(fa)
    assert abs(info.bias - want_bias) <= 1e-14 * max(1.0, SC.scale(fa))


def test_single_leaf_tree_is_one_empty_path():
    fa, _ = SC.small_cases()["hand"]
    paths, _, _ = shap_paths_host(fa)
    first = paths[paths["tree"] == 0]
    assert len(first) == 1 and first[0]["len"] == 0 and first[0]["pz"] == 1.0 and first[0]["value"] == np.float32(0.125)


@pytest.mark.parametrize("key", ["hand", "xgb", "iforest", "rf"])
def test_intervals_agree_with_the_walk(key):
    """a row follows a path's edges on a feature exactly when it lies in the merged interval (NaN: nan_follows):
    every background row then reaches exactly one leaf per tree, whose intervals are not empty"""
    fa, X = SC.small_cases()[key]
    rows = np.concatenate([np.asarray(X), SC.background()[:100, :X.shape[1]]])
    gl = SC.node_goes_left(fa, rows)
    paths, elems, _ = shap_paths_host(fa)
    reached = np.zeros((fa.n_trees, len(rows)), np.int64)
    for p, (tree, leaf, els) in zip(paths, SC.python_paths(fa)):
        on = np.ones(len(rows), bool)
        el = elems[p["elem_offset"]:p["elem_offset"] + p["len"]]
        for e, (f, edges, _) in zip(el, els):
            want = np.ones(len(rows), bool)
            for node, left in edges:
                want &= gl[node] == left
            x = rows[:, f]
            inside = ~(x < e["lo"]) & ((x < e["hi"]) if e["has_hi"] else True)
            got = np.where(np.isnan(x), bool(e["nan_follows"]), inside)
            np.testing.assert_array_equal(got, want)
            on &= got
        if on.any():
            assert all(e["lo"] < e["hi"] for e in el)
        reached[tree] += on
    assert (reached == 1).all()


def test_sixteen_unique_features_fit_and_seventeen_do_not():
    fa = SC.chain_forest(16)
    paths, elems, info = shap_paths_host(fa)
    assert info.max_len == 16
    deepest = paths[0]  # the chain's end (left-first: the first leaf): 16 features, feature 0's three splits merged
    assert deepest["len"] == 16 and elems[deepest["elem_offset"]]["feature"] == 0
    assert paths[-1]["len"] == 1  # the root's right leaf
    X = SC.chain_rows(fa)
    np.testing.assert_allclose(SC.path_form(fa, X), shap_ref_host(fa, X), rtol=0, atol=SC.TOL * SC.scale(fa))
    wide = SC.chain_forest(17)
    with pytest.raises(N.NativeError) as ei:
        shap_paths_host(wide)
    assert ei.value.code == N.FD_ERR_UNSUPPORTED and "tree 0" in str(ei.value)
    assert np.isfinite(shap_ref_host(wide, SC.chain_rows(wide))).all()  # the recursive reference has no such bound


# ------------------------------------------------------------------ the recursive reference
@pytest.mark.parametrize("key", ["hand", "stump", "xgb", "xgb_ld", "iforest", "rf", "et"])
def test_ref_host_against_brute_force(key):
    fa, X = SC.small_cases()[key]
    phi = SC.reference(key, fa, X)
    want = SC.brute(key)
    S = SC.scale(fa)
    err = float(np.abs(phi - want).max()) / S
    print(f"{key}: max |ref_host - brute force| / S = {err:.2e} (S = {S:.3g})")
    assert err <= SC.TOL
    # a feature the forest never splits on contributes exactly nothing
    used = set(fa.feature[fa.left >= 0].tolist())
    for f in set(range(fa.num_feature)) - used:
        assert (phi[:, f] == 0.0).all()


def test_ref_host_additivity_against_the_walk():
    """sum_f phi = the leaf values the walk reaches (oracle/boundary_ref.py follows the child ids) + the base margin"""
    from oracle import boundary_ref as B
    for key in ("hand", "xgb_ld", "iforest", "rf"):
        fa, X = SC.small_cases()[key]
        leaf, _ = B.walk_reference(fa, X)
        lv = SC.leaf_values(fa)
        want = np.array([sum(lv[fa.offsets[t] + leaf[r, t]] for t in range(fa.n_trees)) for r in range(len(X))])
        got = SC.reference(key, fa, X).sum(axis=1)
        assert np.abs(got - (want + SC.base_margin(fa))).max() <= SC.TOL * SC.scale(fa)


def test_path_form_against_ref_host_mid_size():
    fa, X = SC.mid_case()
    assert fa.n_trees == 40 and fa.num_feature == 50 and X.shape == (32, 50)
    err = float(np.abs(SC.path_form(fa, X) - SC.reference("mid", fa, X)).max()) / SC.scale(fa)
    print(f"mid: max |path form - ref_host| / S = {err:.2e}")
    assert err <= SC.TOL


def test_tolerance_measurement_still_holds():
    e0, e1 = SC.measure()
    print(f"e0 = {e0:.2e} (recorded {SC.E0:.2e}), e1 = {e1:.2e} (recorded {SC.E1:.2e}), tol = {SC.TOL:.2e}")
    assert e0 <= 4 * SC.E0 and e1 <= 4 * SC.E1
    assert SC.TOL == 64 * max(SC.E0, SC.E1) <= 1e-9


# ------------------------------------------------------------------ the compiled kernels
def test_shap_kernels_use_no_scratch():
    if not RESOURCES.exists():
        pytest.skip("no kernel_resources.json: build the library first (__graft_entry__.build())")
    res = {k: v for k, v in json.loads(RESOURCES.read_text()).items() if "shap" in k}
    assert {"shap_kernel", "shap_reduce_kernel", "shap_topk_kernel"} <= {
        n for k in res for n in ("shap_kernel", "shap_reduce_kernel", "shap_topk_kernel") if n in k}
    for name, v in res.items():
        assert v["scratch"] == 0, f"{name} spills {v['scratch']} B/lane"


# ------------------------------------------------------------------ the drop-in's switch, off
class _StubEngine:
    def score_matrix(self, params, slots, X, ext, present):
        n = X.shape[0]
        mp = np.stack([np.linspace(0.05, 0.95, n), np.linspace(0.9, 0.1, n)])
        fp = mp[0].copy()
        return mp, fp, np.full(n, 0.8), (fp > 0.5).astype(np.uint8) * 2, np.minimum((fp * 5).astype(np.uint8), 4)


class _StubManager:
    """two engine-resident forests, no device: score_matrix answers from a table, explain counts its calls"""

    def __init__(self):
        from fdengine.model_manager import EngineForest
        self.engine = _StubEngine()
        self.models = {"xgboost_primary": EngineForest(0, "xgboost", 64, 3, 4),
                       "isolation_forest": EngineForest(1, "isolation_forest", 64, 3, 4)}
        self.explain_calls = []

    def is_model_loaded(self, name):
        return name in self.models

    def engine_slot(self, name):
        return self.models[name].slot

    def explain(self, name, X, rows=None, top_k=None, by_abs=True):
        self.explain_calls.append((name, list(rows), top_k))
        m = len(rows)
        return np.ones((m, 65)), np.tile(np.arange(top_k, dtype=np.int32), (m, 1)), np.ones((m, top_k))


def _stub_predictor(monkeypatch, setting):
    import asyncio
    from fdengine.ensemble import EnsemblePredictor
    from fdengine.registry import ScoringConfig
    if setting is None:
        monkeypatch.delenv("EXPLAIN_CONTRIBUTIONS", raising=False)
    else:
        monkeypatch.setenv("EXPLAIN_CONTRIBUTIONS", setting)
    cfg = ScoringConfig("/nonexistent")
    for name in list(cfg.models):
        if name not in ("xgboost_primary", "isolation_forest"):
            cfg.disable_model(name)
    mm = _StubManager()
    ep = EnsemblePredictor(mm, cfg)
    feats = [{"transaction_id": f"t{i}", "amount": 20000.0 * (i % 2), "features": {"a": 0.5, "b": float(i)}}
             for i in range(12)]
    out = asyncio.run(ep.predict_batch(feats))
    for r in out:
        r["processing_time_ms"] = 0.0
    return mm, ep, out


def test_explain_contributions_defaults_off_and_changes_nothing(monkeypatch):
    import pickle
    mm, ep, base = _stub_predictor(monkeypatch, None)
    assert ep.explain_contributions is False and not mm.explain_calls
    assert all("feature_contributions" not in r["explanation"] for r in base)
    mm_f, _, off = _stub_predictor(monkeypatch, "false")
    assert not mm_f.explain_calls and pickle.dumps(off) == pickle.dumps(base)
    mm_on, ep_on, on = _stub_predictor(monkeypatch, "true")
    assert ep_on.explain_contributions is True
    hot = [i for i, r in enumerate(base) if r["fraud_probability"] > 0.7]
    # one call per forest model over the rows above the high-risk threshold; nothing else in the results moves
    assert mm_on.explain_calls == [("xgboost_primary", hot, 10), ("isolation_forest", hot, 10)] and 0 < len(hot) < len(base)
    for i, (a, b) in enumerate(zip(on, base)):
        fc = a["explanation"].pop("feature_contributions", None)
        assert (fc is not None) == (i in hot) and a == b
