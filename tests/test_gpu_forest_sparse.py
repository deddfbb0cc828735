"""GPU: forest_sparse_kernel (csrc/forest_sparse.hip) — the sparse layout's walk of trees of any depth — held to
scikit-learn itself for the predict_proba kind (RandomForestClassifier / ExtraTreesClassifier: probabilities bit for
bit, apply() leaf ids), to the child-following walkers of oracle/forest_ref.py for XGBoost deeper than 10 and an
IsolationForest with max_samples = 2048, then the shapes a heap cannot hold, option forest_kernel = 11 against the
default paths, the blend through fd_score_matrix, the ModelManager drop-in, and the unchanged dispatch of forests
the heap layouts hold. tests/test_forest_sparse_host.py proves the inputs and the layout on the CPU."""
import asyncio

import numpy as np
import pytest

import forest_sparse_cases as SC
from fdengine import FraudEngine, forest_from_sklearn_classifier, iforest_from_sklearn, synth, xgboost_from_json_doc
from fdengine import _native as N
from oracle import forest_ref as FR
from oracle import scoring_ref as S

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:invalid value encountered in reduce")]

SIZES = [1, 255, 256, 257, 1500]  # one row, the tile's edges, several tiles with a ragged one


def _predict_sparse(engine, slot, X):
    """prob, raw, leaf of one launch; the launch must be forest_sparse_kernel's"""
    c0 = engine.counter("forest_sparse_launches")
    out = engine.predict(slot, X, want_raw=True, want_leaf=True)
    assert engine.counter("forest_sparse_launches") - c0 == 1
    return out


# ------------------------------------------------------------------ 1. the predict_proba kind against sklearn
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", ["boundary", "nan"])
@pytest.mark.parametrize("name", ["rf", "et"])
def test_classifier_matches_sklearn(engine, name, kind, n):
    fa, m = SC.classifier(name)
    X = SC.rows(name, kind)[:n]
    leaf, proba, raw = (a[:n] for a in SC.sklearn_answers(name, kind))
    engine.load_forest(2, fa)
    info = engine.forest_info(2)
    assert info["depth"] == max(est.tree_.max_depth for est in m.estimators_) > 10 and info["n_trees"] == fa.n_trees
    p, r, lf = _predict_sparse(engine, 2, X)
    np.testing.assert_array_equal(lf, leaf)    # apply()
    np.testing.assert_array_equal(r, raw)      # the f64 sum in estimator order
    np.testing.assert_array_equal(p, proba)    # predict_proba[:, 1], bit for bit
    p2 = engine.predict(2, X)                  # without raw / leaf outputs
    np.testing.assert_array_equal(p2, proba)


# ------------------------------------------------------------------ 2. XGBoost deeper than the heaps
def test_xgboost_depth_12(engine):
    """23 ragged trees of depth 12 over 50 features, rows of 43 columns (ld < num_feature: the columns beyond are
    missing), 5 % NaN: leaf ids and the f32 margin bit for bit against forest_ref.xgb_walk"""
    Xr = synth.feature_matrix(3000, 50, seed=221)
    fa = xgboost_from_json_doc(synth.xgboost_doc(23, 12, 50, Xr, seed=222, p_leaf=0.12, base_score=0.3))
    X = np.ascontiguousarray(synth.feature_matrix(515, 50, seed=223, nan_frac=0.05)[:, :43])
    engine.load_forest(2, fa)
    assert engine.forest_info(2)["depth"] == 12
    p, r, lf = _predict_sparse(engine, 2, X)
    ref = [FR.xgb_walk(fa, x) for x in X]
    np.testing.assert_array_equal(lf, np.array([l for _, l in ref], np.int32))
    margin = np.array([m for m, _ in ref], np.float32)
    np.testing.assert_array_equal(r.astype(np.float32), margin)
    np.testing.assert_array_equal(r, r.astype(np.float32).astype(np.float64))
    assert (lf[:64] != np.array([FR.xgb_walk(fa, np.r_[x, np.zeros(7, np.float32)])[1] for x in X[:64]])).any(), \
        "the missing columns must matter"
    import oracle
    assert np.abs(p - oracle.xgb_predict(fa, X)[0]).max() <= 1e-5


def test_xgboost_depth_12_from_the_json_file(engine, tmp_path):
    """fd_load_xgboost_json takes the same route: the file of a depth-12 model loads (sparse layout) and scores as the
    arrays loaded through fd_load_forest do"""
    Xr = synth.feature_matrix(3000, 50, seed=221)
    doc = synth.xgboost_doc(23, 12, 50, Xr, seed=222, p_leaf=0.12, base_score=0.3)
    X = synth.feature_matrix(300, 50, seed=224, nan_frac=0.05)
    engine.load_forest(2, xgboost_from_json_doc(doc))
    want = _predict_sparse(engine, 2, X)
    synth.write_xgboost_json(str(tmp_path / "deep.json"), doc)
    engine.load_xgboost_file(3, tmp_path / "deep.json")
    assert engine.forest_info(3)["depth"] == 12
    for a, b in zip(want, _predict_sparse(engine, 3, X)):
        np.testing.assert_array_equal(a, b)


# ------------------------------------------------------------------ 3. IsolationForest beyond max_samples = 1024
def test_iforest_max_samples_2048(engine):
    Xr = synth.feature_matrix(3000, 50, seed=231).astype(np.float64)
    m = synth.isolation_forest(Xr, n_estimators=25, max_samples=2048)
    fa = iforest_from_sklearn(m)
    X = synth.feature_matrix(515, 50, seed=232)
    engine.load_forest(2, fa)
    assert engine.forest_info(2)["depth"] == max(est.tree_.max_depth for est in m.estimators_) > 10
    p, r, lf = _predict_sparse(engine, 2, X)
    ref = [FR.iforest_walk(fa, x) for x in X]
    np.testing.assert_array_equal(lf, np.array([l for _, l in ref], np.int32))
    np.testing.assert_array_equal(r, np.array([d for d, _ in ref]))  # the f64 path-length sum, in order
    sk = 1.0 / (1.0 + np.exp(m.decision_function(X)))
    assert np.abs(p - sk).max() <= 1e-12


# ------------------------------------------------------------------ 4. the shapes a heap cannot hold
@pytest.mark.parametrize("kind", [N.FD_FOREST_XGB_BINARY_LOGISTIC, N.FD_FOREST_SKLEARN_IFOREST,
                                  N.FD_FOREST_SKLEARN_PROBA])
def test_hand_built_forest(engine, kind):
    """a root that is a leaf, a stump, a left and a right chain of depth 40, rows with NaN; whole and short rows"""
    fa = SC.hand_forest(kind)
    engine.load_forest(3, fa)
    assert engine.forest_info(3) == {"kind": kind, "n_trees": 4, "depth": SC.CHAIN, "num_feature": 7}
    for X in (SC.hand_rows(700), np.ascontiguousarray(SC.hand_rows(700)[:, :4]), SC.hand_rows(1)):
        leaf, sums = SC.hand_reference(fa, X)
        p, r, lf = _predict_sparse(engine, 3, X)
        np.testing.assert_array_equal(lf, leaf)
        if kind == N.FD_FOREST_XGB_BINARY_LOGISTIC:
            np.testing.assert_array_equal(r.astype(np.float32), sums)
        else:
            np.testing.assert_array_equal(r, sums)
        if kind == N.FD_FOREST_SKLEARN_PROBA:
            np.testing.assert_array_equal(p, sums / 4.0)


# ------------------------------------------------------------------ 5. option 11 against the default paths
@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("n", [1021, 33000])
def test_option_11_matches_default_path(engine, depth, n):
    """a forest the heap layouts hold: the sparse kernel's outputs are bit-identical to the default path's (depth 8:
    the tree-split path at 1021 rows, kernel 6 at 33000 with leaf ids, the fused kernel without; depth 10: kernel 1)"""
    Xr = synth.feature_matrix(4096, 50, seed=241)
    fa = xgboost_from_json_doc(synth.xgboost_doc(40, depth, 50, Xr, seed=242 + depth, p_leaf=0.1, base_score=0.4))
    X = synth.feature_matrix(n, 50, seed=243, nan_frac=0.01)
    engine.load_forest(2, fa)
    assert engine.forest_info(2)["depth"] == depth
    c0 = engine.counter("forest_sparse_launches")
    base = engine.predict(2, X, want_raw=True, want_leaf=True)
    base_p = engine.predict(2, X)
    assert engine.counter("forest_sparse_launches") == c0, "a heap forest must not take the sparse kernel by default"
    engine.set_option("forest_kernel", 11)
    try:
        got = _predict_sparse(engine, 2, X)
        got_p = engine.predict(2, X)
    finally:
        engine.set_option("forest_kernel", 0)
    for a, b in zip(base, got):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(got_p, base_p)
    np.testing.assert_array_equal(got_p, base[0])


# ------------------------------------------------------------------ 6. the blend through fd_score_matrix
def test_score_matrix_blends_heap_and_sparse_forest(engine):
    """a depth-8 XGBoost (heap paths) and the deep RandomForest, weighted average: the generic per-model branch of
    score_matrix; equals scoring_ref's blend of the two probability columns, with both and with one model dropped"""
    names = ["xgboost_primary", "isolation_forest"]  # the registry names of the two blend positions
    rf, m = SC.classifier("rf")
    Xr = SC.train_matrix()
    xgb = xgboost_from_json_doc(synth.xgboost_doc(30, 8, SC.NF, Xr, seed=251, p_leaf=0.1))
    X = SC.rows("rf", "nan")[:1300]
    proba = SC.sklearn_answers("rf", "nan")[1][:1300]
    engine.load_forest(0, xgb)
    engine.load_forest(1, rf)
    w = S.normalized_weights({"xgboost_primary": 0.4, "isolation_forest": 0.05})
    params = FraudEngine.blend_params([w[k] for k in names], [S.CONF_MULT[k] for k in names])
    px = engine.predict(0, X)
    for present in ([1, 1], [1, 0], [0, 1]):
        c0 = engine.counter("forest_sparse_launches")
        mp, fp, conf, dec, risk = engine.score_matrix(params, [0, 1], X, present=present)
        assert engine.counter("forest_sparse_launches") - c0 == present[1]
        if present[0]:
            np.testing.assert_array_equal(mp[0], px)
        if present[1]:
            np.testing.assert_array_equal(mp[1], proba)
        for i in range(0, len(X), 41):
            probs = [float(px[i]) if present[0] else None, float(proba[i]) if present[1] else None]
            rfp, rconf, rdec, rrisk = S.blend_row(names, probs, w)
            assert fp[i] == rfp and conf[i] == rconf
            assert N.DECISIONS[dec[i]] == rdec and N.RISK_LEVELS[risk[i]] == rrisk


def test_pipelined_step_with_a_sparse_forest_writes_full_vectors():
    """fd_score_batch_pipelined, two batches of 128 tiles + 77 rows, a depth-8 XGBoost and a deep RandomForest over the
    engine's own 64-wide vectors: the fused kernel does not apply, so no batch may be scored from compact rows; the
    RandomForest's column equals sklearn's predict_proba on the vectors, bit for bit"""
    import torch
    from fdengine._native import TXN_FIELDS
    nb = 32768 + 77
    pop = synth.population(20000, 5000, seed=7)
    tx = synth.txn_stream(pop, 2 * nb, seed=8)
    batches = [{f: np.ascontiguousarray(tx[f][a:a + nb]) for f in TXN_FIELDS} for a in (0, nb)]

    def state_engine():
        U, M = pop["users"], pop["merchants"]
        e = FraudEngine(0)
        e.state_init(1 << 17, 1, 16)
        e.load_users(U["key"], U["avg_amount"], U["account_age_days"], U["device_fp"])
        e.load_merchants(M["fraud_rate"], M["risk_multiplier"])
        return e

    twin = state_engine()
    try:
        V = [twin.features(b) for b in batches]
    finally:
        twin.close()
    m = synth.random_forest(V[0][:3000], n_estimators=15, random_state=271)
    assert max(est.tree_.max_depth for est in m.estimators_) > 10
    xgb = xgboost_from_json_doc(synth.xgboost_doc(30, 8, 64, V[0], seed=272, p_leaf=0.1, max_bin=None))
    names = ["xgboost_primary", "isolation_forest"]
    w = S.normalized_weights({"xgboost_primary": 0.4, "isolation_forest": 0.05})
    params = FraudEngine.blend_params([w[k] for k in names], [S.CONF_MULT[k] for k in names])
    eng = state_engine()
    try:
        eng.load_forest(0, xgb)
        eng.load_forest(1, forest_from_sklearn_classifier(m))
        eng.set_stream(torch.cuda.current_stream().cuda_stream)
        c0, s0 = eng.counter("pipelined_compact_batches"), eng.counter("forest_sparse_launches")
        outs, keep = [], []
        for b in batches:
            dev = {f: torch.from_numpy(b[f]).cuda() for f in TXN_FIELDS}
            o = [torch.empty(nb, dtype=t, device="cuda") for t in (torch.float64, torch.float64, torch.uint8, torch.uint8)]
            mp = torch.empty((2, nb), dtype=torch.float64, device="cuda")
            eng.score_batch_pipelined(params, [0, 1], {f: t.data_ptr() for f, t in dev.items()}, nb,
                                      *[x.data_ptr() for x in o], model_probs_ptr=mp.data_ptr())
            outs.append((mp, o))
            keep.append(dev)
        torch.cuda.synchronize()
        eng.sync()
        assert eng.counter("pipelined_batches") >= 2
        assert eng.counter("pipelined_compact_batches") == c0
        assert eng.counter("forest_sparse_launches") - s0 == 2
        for (mp, o), v in zip(outs, V):
            mp = mp.cpu().numpy()
            proba = m.predict_proba(v)[:, 1]
            np.testing.assert_array_equal(mp[1], proba)
            fp, conf = o[0].cpu().numpy(), o[1].cpu().numpy()
            for i in range(0, nb, 1499):
                rfp, rconf, _, _ = S.blend_row(names, [float(mp[0][i]), float(proba[i])], w)
                assert fp[i] == rfp and conf[i] == rconf
    finally:
        eng.close()


# ------------------------------------------------------------------ 7. the ModelManager drop-in
def test_model_manager_serves_a_random_forest(tmp_path):
    import joblib
    from fdengine.model_manager import ModelManager
    from fdengine.registry import ScoringConfig
    rf, m = SC.classifier("rf")
    Xr = SC.train_matrix()
    ifm = synth.isolation_forest(Xr.astype(np.float64), n_estimators=20)
    (tmp_path / "sklearn").mkdir()
    path = tmp_path / "sklearn" / "isolation_forest.joblib"  # the registry's one model_type "sklearn" entry
    joblib.dump(m, path)
    cfg = ScoringConfig(str(tmp_path))
    for k in ("xgboost_primary", "lstm_sequential", "bert_text", "graph_neural"):
        cfg.disable_model(k)
    mm = ModelManager(cfg, device=0)
    name = "isolation_forest"
    X = SC.rows("rf", "nan")[:700]
    proba = SC.sklearn_answers("rf", "nan")[1][:700]
    try:
        asyncio.run(mm.load_all_models())
        slot = mm.engine_slot(name)
        assert slot >= 0
        eng_info = mm.get_model_info()["models"][name]["engine"]
        assert eng_info["kind"] == "sklearn_classifier" and eng_info["model_class"] == "RandomForestClassifier"
        assert eng_info["n_trees"] == 37 and eng_info["depth"] > 10
        got = asyncio.run(mm.predict(name, X.astype(np.float64)))
        assert got.dtype == np.float64
        np.testing.assert_array_equal(got, proba)
        with pytest.raises(ValueError) as ei:  # sklearn's own message, with the estimator's class
            asyncio.run(mm.predict(name, X[:, :49]))
        with pytest.raises(ValueError) as sk:
            m.predict_proba(X[:, :49])
        assert str(ei.value) == str(sk.value)
        asyncio.run(mm.reload_model(name))
        np.testing.assert_array_equal(asyncio.run(mm.predict(name, X)), proba)
        # the slot alternates between a sparse and a heap forest
        joblib.dump(ifm, path)
        asyncio.run(mm.reload_model(name))
        assert mm.get_model_info()["models"][name]["engine"]["kind"] == "isolation_forest"
        Xc = np.nan_to_num(X)
        sk_if = 1.0 / (1.0 + np.exp(ifm.decision_function(Xc)))
        assert np.abs(asyncio.run(mm.predict(name, Xc)) - sk_if).max() <= 1e-12
        joblib.dump(m, path)
        asyncio.run(mm.reload_model(name))
        np.testing.assert_array_equal(asyncio.run(mm.predict(name, X)), proba)
        asyncio.run(mm.cleanup())
        assert not mm.is_model_loaded(name)
        with pytest.raises(ValueError, match="not loaded"):
            mm.engine.predict(slot, X)
    finally:
        mm.engine.close()


# ------------------------------------------------------------------ 8. unchanged dispatch (passes before and after)
def test_heap_forest_dispatch_is_unchanged(engine):
    """a depth-8 forest at a large batch still runs the fused kernel over one forest, never the sparse kernel"""
    Xr = synth.feature_matrix(4096, 50, seed=261)
    fa = xgboost_from_json_doc(synth.xgboost_doc(40, 8, 50, Xr, seed=262, p_leaf=0.1))
    X = synth.feature_matrix(32768 + 77, 50, seed=263)
    engine.load_forest(2, fa)
    counters = {}
    for k in ("ensemble_single_launches", "forest_sparse_launches"):
        try:
            counters[k] = engine.counter(k)
        except N.NativeError:  # (an engine without the sparse kernel has no such counter: nothing to move)
            counters[k] = None
    engine.predict(2, X)
    assert engine.counter("ensemble_single_launches") - counters["ensemble_single_launches"] == 1
    if counters["forest_sparse_launches"] is not None:
        assert engine.counter("forest_sparse_launches") == counters["forest_sparse_launches"]
