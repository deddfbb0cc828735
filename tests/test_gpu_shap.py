"""GPU: forest attribution on the engine (fd_forest_shap_*, fd_shap_topk_*) against the brute-force
Shapley sum and the recursive host reference of tests/shap_cases.py, additivity against the leaves the scoring kernels
reach, exact zeros, bit-for-bit independence of a row's place, top-k reason codes, and scoring left untouched.
Tolerance: |delta| <= SC.TOL * S (measured on the CPU between the oracles, shap_cases.py)."""
import math

import numpy as np
import pytest

import shap_cases as SC
from fdengine import _native as N
from fdengine import synth

pytestmark = pytest.mark.gpu
SLOT = 5


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _load(engine, fa):
    engine.load_forest(SLOT, fa)
    return engine


def _close(got, want, fa, what):
    S = SC.scale(fa)
    err = float(np.abs(got - want).max()) / S
    print(f"{what}: max |delta| / S = {err:.2e} (tol {SC.TOL:.2e}, S = {S:.3g})")
    assert err <= SC.TOL, what


# ------------------------------------------------------------------ against brute force
@pytest.mark.parametrize("key", ["hand", "stump", "xgb", "xgb_ld", "iforest", "rf", "et"])
def test_kernel_against_brute_force(engine, key):
    fa, X = SC.small_cases()[key]
    want = SC.brute(key)
    _load(engine, fa)
    c0 = engine.counter("forest_shap_launches")
    for n in (1, 63, 64, 65, 257):
        reps = np.arange(n) % len(X)  # the small row set tiled to n
        phi = engine.explain(SLOT, X[reps])
        assert phi.shape == (n, fa.num_feature + 1) and phi.dtype == np.float64
        _close(phi, want[reps], fa, f"{key} n={n}")
    assert engine.counter("forest_shap_launches") - c0 == 5


# ------------------------------------------------------------------ against the recursive host reference
def _deep_xgb():
    """the depth-12 sparse-layout XGBoost of test_gpu_forest_sparse.py's recipe, with consistent covers"""
    Xr = synth.feature_matrix(3000, 50, seed=221)
    fa = SC.with_covers(synth.xgboost_doc(23, 12, 50, Xr, seed=222, p_leaf=0.12, base_score=0.3), Xr)
    X = np.ascontiguousarray(synth.feature_matrix(70, 50, seed=223, nan_frac=0.05)[:, :43])  # ld < num_feature
    return fa, X


def _ref_cases():
    yield ("mid",) + SC.mid_case()
    yield ("deep",) + _deep_xgb()
    for key in ("iforest", "rf"):
        yield (key,) + SC.small_cases()[key]
    fa = SC.chain_forest(16)
    yield "chain16", fa, SC.chain_rows(fa)


@pytest.mark.parametrize("case", ["mid", "deep", "iforest", "rf", "chain16"])
def test_kernel_against_ref_host(engine, case):
    name, fa, X = next(c for c in _ref_cases() if c[0] == case)
    _load(engine, fa)
    if case == "deep":
        assert engine.forest_info(SLOT)["depth"] == 12
    phi = engine.explain(SLOT, X)
    _close(phi, SC.reference(name, fa, X), fa, case)


def test_a_path_of_17_unique_features_is_refused(engine):
    fa = SC.chain_forest(17)
    _load(engine, fa)
    X = SC.chain_rows(fa)
    assert engine.predict(SLOT, X).shape == (len(X),)  # the forest itself loads and scores
    with pytest.raises(N.NativeError) as ei:
        engine.explain(SLOT, X)
    assert ei.value.code == N.FD_ERR_UNSUPPORTED and "tree 0" in str(ei.value)


def test_a_forest_without_covers_is_not_explained(engine):
    fa, X = SC.small_cases()["xgb"]
    bare = type(fa)(**{**fa.__dict__, "cover": None})
    _load(engine, bare)
    with pytest.raises(ValueError, match="no covers"):  # FD_ERR_NOT_LOADED, as for a model that is not loaded
        engine.explain(SLOT, X)
    bad = fa.cover.copy()
    bad[3] = -2.0
    with pytest.raises(N.NativeError) as ei:
        engine.set_cover(SLOT, bad)
    assert ei.value.code == N.FD_ERR_INVALID_ARG and "tree 0 node 3" in str(ei.value)
    engine.set_cover(SLOT, fa.cover)
    _close(engine.explain(SLOT, X), SC.brute("xgb"), fa, "covers attached afterwards")


def test_xgboost_file_brings_its_covers(engine, tmp_path):
    Xr = SC.background()
    doc = synth.xgboost_doc(6, 4, SC.NF, Xr, seed=323, p_leaf=0.2, base_score=0.35)
    SC.with_covers(doc, Xr)
    synth.write_xgboost_json(str(tmp_path / "m.json"), doc)
    engine.load_xgboost_file(SLOT, tmp_path / "m.json")
    fa, X = SC.small_cases()["xgb"]
    _close(engine.explain(SLOT, X), SC.brute("xgb"), fa, "fd_load_xgboost_json")


# ------------------------------------------------------------------ additivity against the scoring kernels
@pytest.mark.parametrize("case", ["mid", "deep", "iforest", "rf"])
def test_additivity_against_predicted_leaves(engine, case):
    name, fa, X = next(c for c in _ref_cases() if c[0] == case)
    _load(engine, fa)
    _, raw, leaf = engine.predict(SLOT, X, want_raw=True, want_leaf=True)
    phi = engine.explain(SLOT, X)
    lv = SC.leaf_values(fa)
    base = SC.base_margin(fa)
    want = np.array([math.fsum(lv[fa.offsets[t] + leaf[r, t]] for t in range(fa.n_trees)) + base
                     for r in range(len(X))])
    got = np.array([math.fsum(row) for row in phi])
    _close(got, want, fa, f"{case}: sum of phi against the walked leaves")
    if fa.kind != N.FD_FOREST_XGB_BINARY_LOGISTIC:  # the sklearn kinds' raw is that f64 sum (XGBoost's is an f32 one)
        _close(got, raw, fa, f"{case}: sum of phi against raw")


def test_unused_columns_are_exactly_zero(engine):
    for key in ("hand", "xgb", "rf"):
        fa, X = SC.small_cases()[key]
        _load(engine, fa)
        phi = engine.explain(SLOT, np.tile(X, (6, 1)))
        unused = sorted(set(range(fa.num_feature)) - set(fa.feature[fa.left >= 0].tolist()))
        if key == "hand":
            assert set(unused) >= {5, 6, 7}
        for f in unused:
            assert (_bits(phi[:, f]) == 0).all(), (key, f)  # +0.0, bit for bit


# ------------------------------------------------------------------ a row's bits depend on the row and the forest only
def test_position_independence_bit_for_bit(engine):
    fa, _ = SC.mid_case()
    X = synth.feature_matrix(300, 50, seed=351, nan_frac=0.03)
    _load(engine, fa)
    whole = engine.explain(SLOT, X[:257])
    again = engine.explain(SLOT, X[:257])
    np.testing.assert_array_equal(_bits(whole), _bits(again))  # two runs
    rng = np.random.Generator(np.random.PCG64(352))
    perm = rng.permutation(257)
    permuted = engine.explain(SLOT, X[:257][perm])
    np.testing.assert_array_equal(_bits(permuted), _bits(whole[perm]))
    for i in (0, 63, 64, 200, 256):
        alone = engine.explain(SLOT, X[i:i + 1])
        np.testing.assert_array_equal(_bits(alone[0]), _bits(whole[i]))
        sub = engine.explain(SLOT, X, rows=[299, i, 5, i])  # through rows, and twice in one list
        np.testing.assert_array_equal(_bits(sub[1]), _bits(whole[i]))
        np.testing.assert_array_equal(_bits(sub[3]), _bits(whole[i]))
        np.testing.assert_array_equal(_bits(sub[2]), _bits(whole[5]))
    assert engine.explain(SLOT, X, rows=[]).shape == (0, 51)
    with pytest.raises(N.NativeError) as ei:
        engine.explain(SLOT, X, rows=[3, 300])
    assert ei.value.code == N.FD_ERR_INVALID_ARG


def test_device_tensors_and_row_batches(engine):
    """device input is explained in place; more rows than one launch takes (4096) give the same bits per row"""
    import torch
    fa, X = SC.small_cases()["xgb"]
    _load(engine, fa)
    want = engine.explain(SLOT, X)
    reps = np.arange(4096 + 130) % len(X)
    c0 = engine.counter("forest_shap_launches")
    dX = torch.from_numpy(np.ascontiguousarray(X[reps])).to("cuda:0")
    phi, idx, val = engine.explain(SLOT, dX, top_k=3)
    assert engine.counter("forest_shap_launches") - c0 == 2
    assert phi.is_cuda and idx.dtype == torch.int32
    np.testing.assert_array_equal(_bits(phi.cpu().numpy()), _bits(want[reps]))
    sub = engine.explain(SLOT, dX, rows=torch.tensor([4100, 7], device="cuda:0"))
    np.testing.assert_array_equal(_bits(sub.cpu().numpy()), _bits(want[reps[[4100, 7]]]))
    h_phi, h_idx, h_val = engine.explain(SLOT, X, top_k=3)
    np.testing.assert_array_equal(idx.cpu().numpy()[:len(X)], h_idx)
    np.testing.assert_array_equal(val.cpu().numpy()[:len(X)], h_val)


# ------------------------------------------------------------------ top-k
def _topk_ref(phi, nf, k, by_abs):
    n = phi.shape[0]
    idx = np.full((n, k), -1, np.int32)
    val = np.zeros((n, k), np.float64)
    for r in range(n):
        v = phi[r, :nf]
        key = np.abs(v) if by_abs else v
        order = np.argsort(-key, kind="stable")  # ties: the lower column first
        order = [f for f in order if v[f] != 0.0][:k]
        idx[r, :len(order)] = order
        val[r, :len(order)] = v[order]
    return idx, val


@pytest.mark.parametrize("nf", [50, 64, 70])
def test_topk_against_stable_argsort(engine, nf):
    rng = np.random.Generator(np.random.PCG64(360 + nf))
    phi = rng.normal(size=(67, nf + 3))  # ld_phi > num_feature + 1; the bias column is the largest of every row
    phi[:, nf] = 100.0
    phi[rng.random(phi.shape) < 0.3] = 0.0
    phi[0, :nf] = 0.0
    phi[0, [4, 9, 30, nf - 1]] = [0.5, -0.5, 0.5, -0.5]   # four tied |phi|, constructed
    phi[1, :nf] = 0.0
    phi[1, [nf - 1, 2]] = [-3.0, 1.0]                       # fewer than k non-zeros
    phi[2, :nf] = 0.0                                       # none
    phi[3, :nf] = -np.abs(phi[3, :nf]) - 1.0                # all negative: the signed order still reports them
    import ctypes as C
    for k in (1, 10, 16):
        for by_abs in (True, False):
            idx = np.full((len(phi), k), 7, np.int32)
            val = np.full((len(phi), k), 7.0)
            N.call("fd_shap_topk_host", engine.handle, C.c_void_p(phi.ctypes.data), len(phi), phi.shape[1], nf, k,
                   1 if by_abs else 0, C.c_void_p(idx.ctypes.data), C.c_void_p(val.ctypes.data))
            want_idx, want_val = _topk_ref(phi, nf, k, by_abs)
            np.testing.assert_array_equal(idx, want_idx, err_msg=f"k={k} by_abs={by_abs}")
            np.testing.assert_array_equal(_bits(val), _bits(want_val))
    idx, _ = _topk_ref(phi, nf, 4, True)
    assert list(idx[0]) == [4, 9, 30, nf - 1]


def test_explain_with_topk(engine):
    fa, X = SC.mid_case()
    _load(engine, fa)
    phi, idx, val = engine.explain(SLOT, X, top_k=10)
    want_idx, want_val = _topk_ref(phi, fa.num_feature, 10, True)
    np.testing.assert_array_equal(idx, want_idx)
    np.testing.assert_array_equal(val, want_val)
    _, idx_s, val_s = engine.explain(SLOT, X, rows=[3, 1], top_k=16, by_abs=False)
    want_idx, want_val = _topk_ref(phi[[3, 1]], fa.num_feature, 16, False)
    np.testing.assert_array_equal(idx_s, want_idx)
    np.testing.assert_array_equal(val_s, want_val)
    with pytest.raises(ValueError):
        engine.explain(SLOT, X, top_k=17)


# ------------------------------------------------------------------ scoring is left untouched
def test_explain_leaves_scoring_untouched_and_follows_reloads(engine):
    fa, X = SC.mid_case()
    _load(engine, fa)
    before = engine.predict(SLOT, X, want_raw=True, want_leaf=True)
    phi = engine.explain(SLOT, X)
    after = engine.predict(SLOT, X, want_raw=True, want_leaf=True)
    for a, b in zip(before, after):
        np.testing.assert_array_equal(a, b)
    # another forest on the slot: the first one's table must not survive the unload / load
    engine.unload_forest(SLOT)
    with pytest.raises(ValueError):
        engine.explain(SLOT, X)
    other, Xo = SC.small_cases()["rf"]
    _load(engine, other)
    _close(engine.explain(SLOT, Xo), SC.brute("rf"), other, "after unload + load of another forest")
    _load(engine, fa)  # and a reload without an unload
    np.testing.assert_array_equal(_bits(engine.explain(SLOT, X)), _bits(phi))


# ------------------------------------------------------------------ the drop-in: explanation["feature_contributions"]
def _dropin(tmp_path, on):
    import asyncio
    import joblib
    from fdengine.ensemble import EnsemblePredictor
    from fdengine.model_manager import ModelManager
    from fdengine.registry import ScoringConfig
    (tmp_path / "xgboost").mkdir(exist_ok=True)
    (tmp_path / "sklearn").mkdir(exist_ok=True)
    Xref = synth.feature_matrix(1024, 64, seed=371)
    doc = synth.xgboost_doc(20, 6, 64, Xref, seed=372, p_leaf=0.1, base_score=0.5)
    SC.with_covers(doc, Xref)
    synth.write_xgboost_json(str(tmp_path / "xgboost" / "fraud_classifier.json"), doc)
    joblib.dump(synth.isolation_forest(Xref.astype(np.float64), n_estimators=20),
                tmp_path / "sklearn" / "isolation_forest.joblib")
    cfg = ScoringConfig(str(tmp_path))
    for name in ("bert_text", "graph_neural"):
        cfg.disable_model(name)
    cfg.ensemble.explain_contributions = on
    mm = ModelManager(cfg, device=0)
    asyncio.run(mm.load_all_models())
    return mm, EnsemblePredictor(mm, cfg), Xref


def test_dropin_feature_contributions(tmp_path):
    import asyncio
    mm, ep, Xref = _dropin(tmp_path, True)
    try:
        feats = [{"transaction_id": f"t{i}", "features": {f"f{k}": float(v) for k, v in enumerate(Xref[i])}}
                 for i in range(48)]
        off = type(ep)(mm, ep.config)
        off.explain_contributions = False
        plain = asyncio.run(off.predict_batch(feats))
        assert all("feature_contributions" not in r["explanation"] for r in plain)
        # the class's threshold is the Flink job's 0.7; the test moves the instance's to the batch's median so that
        # rows fall on both sides
        assert type(ep).CONTRIBUTION_THRESHOLD == 0.7 and type(ep).CONTRIBUTION_TOP_K == 10
        ep.CONTRIBUTION_THRESHOLD = float(np.median([r["fraud_probability"] for r in plain]))
        got = asyncio.run(ep.predict_batch(feats))
        flagged = [i for i, r in enumerate(plain) if r["fraud_probability"] > ep.CONTRIBUTION_THRESHOLD]
        assert 0 < len(flagged) < len(feats)
        from fdengine.ensemble import prepare_features
        kept = {}
        for i, (r, p) in enumerate(zip(got, plain)):
            fc = kept[i] = r["explanation"].pop("feature_contributions", None)
            p = dict(p, processing_time_ms=r["processing_time_ms"])
            assert r == p  # everything else is as without the switch
            if i not in flagged:
                assert fc is None
                continue
            assert set(fc) == {"xgboost_primary", "isolation_forest"}
            x = prepare_features(feats[i])
            for name, c in fc.items():
                phi, idx, val = mm.explain(name, x, top_k=10)
                assert c["bias"] == phi[0, -1]
                assert c["top"] == [[int(a), float(b)] for a, b in zip(idx[0], val[0]) if a >= 0]
                assert 0 < len(c["top"]) <= 10
        one = asyncio.run(ep.predict(dict(feats[flagged[0]], transaction_id="single")))
        assert one["explanation"]["feature_contributions"] == kept[flagged[0]]  # predict() adds the same block
        with pytest.raises(ValueError):
            mm.explain("lstm_sequential", prepare_features(feats[0]))
    finally:
        asyncio.run(mm.cleanup())
