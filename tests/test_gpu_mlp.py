"""GPU parity of the MLP head (csrc/mlp.hip, f32 MFMA; the reference's model_type "pytorch" member graph_neural)
against torch fp32 on the CPU (tests/mlp_cases.py), tolerance 1e-5 on probabilities; then the head as an ensemble
member of the scoring calls and behind the drop-in ModelManager / EnsemblePredictor."""
import asyncio

import numpy as np
import pytest

import mlp_cases as K
from fdengine import FraudEngine, synth
from fdengine import mlp as M
from fdengine._native import DECISIONS, FD_SLOT_MLP, RISK_LEVELS, TXN_FIELDS
from oracle import scoring_ref as S

pytestmark = pytest.mark.gpu

TOL = K.TOL


@pytest.fixture
def mlp_engine(engine):
    yield engine
    engine.unload_mlp()


@pytest.mark.parametrize("n", K.NS)
@pytest.mark.parametrize("shape_idx", range(len(K.SHAPES)))
def test_mlp_matches_torch(mlp_engine, shape_idx, n):
    w, X, ref = K.case(shape_idx)
    mlp_engine.load_mlp(w)
    assert mlp_engine.mlp_shape() == {"n_layers": w.n_layers, "in_dim": w.in_dim, "hidden": w.hidden}
    p = mlp_engine.mlp_predict(X[:n])
    d = np.abs(p - ref[:n]).max()
    print(f"shape {K.SHAPES[shape_idx]} n {n}: max |dp| = {d:.3e}")
    assert p.shape == (n,) and p.dtype == np.float64
    assert d <= TOL, d
    assert (p == p.astype(np.float32)).all()  # the f64 of an f32 value


@pytest.mark.parametrize("n", K.NS)
def test_mlp_strided_rows_never_read_beyond_in_dim(mlp_engine, n):
    """ld = 70 on a matrix whose columns 64..69 hold NaN: they are not the model's input"""
    w, X, ref = K.case(0)
    mlp_engine.load_mlp(w)
    Xw = np.full((n, 70), np.nan, np.float32)
    Xw[:, :64] = X[:n]
    p = mlp_engine.mlp_predict(Xw)
    assert not np.isnan(p).any()
    assert np.abs(p - ref[:n]).max() <= TOL
    np.testing.assert_array_equal(p, mlp_engine.mlp_predict(X[:n]))  # the 16-B and the scalar row loads agree


@pytest.mark.parametrize("n", [17, 4099])
def test_mlp_reference_shape_in_the_lds_form(mlp_engine, n):
    """option mlp_form = 1: the reference shape through the kernel form every other shape takes (weights in LDS);
    option mlp_wgs_per_cu: the persistent grid's size does not change a bit"""
    w, X, ref = K.case(0)
    mlp_engine.load_mlp(w)
    base = mlp_engine.mlp_predict(X[:n])
    try:
        mlp_engine.set_option("mlp_form", 1)
        p = mlp_engine.mlp_predict(X[:n])
        mlp_engine.set_option("mlp_form", 0)
        mlp_engine.set_option("mlp_wgs_per_cu", 1)
        q = mlp_engine.mlp_predict(X[:n])
    finally:
        mlp_engine.set_option("mlp_form", 0)
        mlp_engine.set_option("mlp_wgs_per_cu", 0)
    assert np.abs(p - ref[:n]).max() <= TOL
    np.testing.assert_array_equal(q, base)


def test_mlp_stride_below_in_dim_is_refused(mlp_engine):
    from fdengine._native import FD_ERR_INVALID_ARG, NativeError
    mlp_engine.load_mlp(K.case(0)[0])
    with pytest.raises(NativeError) as ei:
        mlp_engine.mlp_predict(np.zeros((3, 63), np.float32))
    assert ei.value.code == FD_ERR_INVALID_ARG
    assert mlp_engine.mlp_predict(np.zeros((0, 64), np.float32)).shape == (0,)  # n == 0: a no-op


def test_mlp_saturation(mlp_engine):
    """the last layer x64: probabilities reach 0 and 1 (torch fp32 on the CPU puts 2,369 of these 4,099 rows within
    1e-6 of 0 or 1 and is itself about 2e-6 from an f64 evaluation), no NaN, within the bar (measured 3.3e-6)"""
    w, X, ref = K.case(0, last_scale=64.0)
    mlp_engine.load_mlp(w)
    p = mlp_engine.mlp_predict(X)
    d = np.abs(p - ref).max()
    print(f"saturation: max |dp| = {d:.3e}, saturated rows {(np.minimum(p, 1 - p) < 1e-6).sum()}")
    assert not np.isnan(p).any()
    assert p.min() >= 0.0 and p.max() <= 1.0
    assert (np.minimum(ref, 1 - ref) < 1e-6).sum() > 2000 and (np.minimum(p, 1 - p) < 1e-6).sum() > 2000
    assert p.min() < 1e-6 and p.max() > 1 - 1e-6
    assert d <= TOL, d


def test_mlp_nan_row(mlp_engine):
    """one input row holds a NaN: that row's output is NaN as torch's is (ReLU propagates it), every other row is
    bit-identical to the same batch without it"""
    w, X, _ = K.case(0)
    mlp_engine.load_mlp(w)
    Xn = X[:257].copy()
    Xn[100, 37] = np.nan
    ref = K.torch_forward(w, Xn)
    assert np.isnan(ref[100]) and np.isnan(ref).sum() == 1
    p, clean = mlp_engine.mlp_predict(Xn), mlp_engine.mlp_predict(X[:257])
    assert np.isnan(p[100])
    keep = np.arange(257) != 100
    np.testing.assert_array_equal(p[keep], clean[keep])


def test_mlp_batch_independence(mlp_engine):
    w, X, _ = K.case(0)
    mlp_engine.load_mlp(w)
    p = mlp_engine.mlp_predict(X)
    for i in (0, 15, 16, K.N_MAX - 1):
        assert mlp_engine.mlp_predict(X[i:i + 1])[0] == p[i], i


def test_mlp_not_loaded_raises(engine):
    engine.unload_mlp()
    with pytest.raises(ValueError, match="not loaded"):
        engine.mlp_predict(np.zeros((2, 64), np.float32))
    with pytest.raises(ValueError, match="not loaded"):
        engine.mlp_shape()
    engine.load_mlp(K.case(0)[0])
    engine.mlp_predict(np.zeros((2, 64), np.float32))
    engine.unload_mlp()
    engine.unload_mlp()  # idempotent
    with pytest.raises(ValueError, match="not loaded"):
        engine.mlp_predict(np.zeros((2, 64), np.float32))


def test_mlp_load_refuses_a_limit_on_the_engine(engine):
    from fdengine._native import FD_ERR_UNSUPPORTED, NativeError
    wide = M.MlpWeights([np.zeros((65, 64), np.float32), np.zeros((2, 65), np.float32)], [None, None])
    with pytest.raises(NativeError) as ei:
        engine.load_mlp(wide)
    assert ei.value.code == FD_ERR_UNSUPPORTED and "hidden width" in str(ei.value)


NAMES = ["xgboost_primary", "isolation_forest", "graph_neural"]
WEIGHTS = {"xgboost_primary": 0.4, "isolation_forest": 0.05, "graph_neural": 0.15}


@pytest.fixture(scope="module")
def forests():
    from fdengine import iforest_from_sklearn, xgboost_from_json_doc
    X = synth.feature_matrix(3000, 64, seed=3)
    xgb = xgboost_from_json_doc(synth.xgboost_doc(60, 6, 64, X, seed=4, p_leaf=0.1))
    ifm = iforest_from_sklearn(synth.isolation_forest(X.astype(np.float64), n_estimators=20))
    return xgb, ifm


@pytest.mark.parametrize("n", [300, 40000])  # the latency (tree-split) path, and a batch the fused pair kernel would take
def test_mlp_as_an_ensemble_member(mlp_engine, forests, n):
    """score_matrix with [XGBoost, IsolationForest, MLP]: the MLP column is mlp_predict's, bit for bit; the blend is
    oracle/scoring_ref.py's over the three engine columns; present = 0 drops the MLP"""
    eng = mlp_engine
    w = K.case(0)[0]
    eng.load_forest(0, forests[0])
    eng.load_forest(1, forests[1])
    eng.load_mlp(w)
    X = synth.feature_matrix(n, 64, seed=11).astype(np.float32)
    wn = S.normalized_weights(WEIGHTS)
    params = FraudEngine.blend_params([wn[k] for k in NAMES], [S.CONF_MULT[k] for k in NAMES])
    alone = eng.mlp_predict(X)
    before = eng.counter("mlp_launches")
    try:
        for present in ([1, 1, 1], [1, 1, 0]):
            mp, fp, conf, dec, risk = eng.score_matrix(params, [0, 1, FD_SLOT_MLP], X, present=present)
            if present[2]:
                np.testing.assert_array_equal(mp[2], alone)
                assert eng.counter("mlp_launches") == before + 1
            for i in range(0, n, max(1, n // 400)):
                probs = [float(mp[m, i]) if present[m] else None for m in range(3)]
                rfp, rconf, rdec, rrisk = S.blend_row(NAMES, probs, wn)
                assert fp[i] == rfp and conf[i] == rconf, (i, fp[i], rfp, conf[i], rconf)
                assert DECISIONS[dec[i]] == rdec and RISK_LEVELS[risk[i]] == rrisk
        assert eng.counter("mlp_launches") == before + 1  # the dropped member launches nothing
    finally:
        eng.unload_forest(0)
        eng.unload_forest(1)


def _hot_path_engine(pop, forests, w, stream):
    U, Mc = pop["users"], pop["merchants"]
    e = FraudEngine(0)
    e.set_stream(stream)
    e.state_init(4 * len(U["key"]) + 4096, 1, 8)
    e.load_users(U["key"], U["avg_amount"], U["account_age_days"], U["device_fp"])
    e.load_merchants(Mc["fraud_rate"], Mc["risk_multiplier"])
    e.load_forest(0, forests[0])
    e.load_forest(1, forests[1])
    e.load_mlp(w)
    return e


def test_mlp_in_the_whole_hot_path(forests):
    """fd_score_batch_device over a synthetic stream with the three models: the MLP column equals torch on the
    returned vectors; fd_score_batch_pipelined and the records form (partition -> fd_score_records_device ->
    scatter) over the same stream are bit-identical to it, every output"""
    import torch
    from fdengine.sharding import EngineShardBackend
    w = K.case(0)[0]
    pop = synth.population(1500, 100, seed=31)
    tx = synth.txn_stream(pop, 9000, seed=12, rate_per_s=2.0)
    wn = S.normalized_weights(WEIGHTS)
    params = FraudEngine.blend_params([wn[k] for k in NAMES], [S.CONF_MULT[k] for k in NAMES])
    slots = [0, 1, FD_SLOT_MLP]
    stream = torch.cuda.current_stream().cuda_stream
    engines = [_hot_path_engine(pop, forests, w, stream) for _ in range(3)]
    serial, piped, routed = engines
    be = EngineShardBackend(routed, params, slots)
    try:
        for a, b in [(0, 700), (700, 5000), (5000, 9000)]:  # card state carried across micro-batches
            n = b - a
            dev = {f: torch.from_numpy(np.ascontiguousarray(tx[f][a:b])).cuda() for f in TXN_FIELDS}
            ptrs = {f: t.data_ptr() for f, t in dev.items()}
            got = []
            for form in ("serial", "pipelined"):
                out = [torch.empty(n, dtype=d, device="cuda") for d in (torch.float64, torch.float64, torch.uint8,
                                                                         torch.uint8)]
                vec = torch.empty((n, 64), dtype=torch.float32, device="cuda")
                mp = torch.empty((3, n), dtype=torch.float64, device="cuda")
                call = serial.score_batch_device if form == "serial" else piped.score_batch_pipelined
                call(params, slots, ptrs, n, *[o.data_ptr() for o in out], vec_ptr=vec.data_ptr(),
                     model_probs_ptr=mp.data_ptr())
                torch.cuda.synchronize()
                got.append([o.cpu().numpy() for o in out] + [mp.cpu().numpy(), vec.cpu().numpy()])
            for x, y in zip(*got):
                np.testing.assert_array_equal(x, y)
            fp, conf, dec, risk, MP, V = got[0]
            d = np.abs(MP[2] - K.torch_forward(w, V)).max()
            print(f"hot path batch {a}:{b}: MLP column max |dp| = {d:.3e}")
            assert d <= TOL, d
            for i in range(0, n, 37):
                rfp, rconf, rdec, rrisk = S.blend_row(NAMES, [float(MP[m, i]) for m in range(3)], wn)
                assert fp[i] == rfp and conf[i] == rconf
                assert DECISIONS[dec[i]] == rdec and RISK_LEVELS[risk[i]] == rrisk
            rec, _ = be.partition(dev, n, 1)
            back = be.scatter_results(be.score_records(rec, n), n)
            torch.cuda.synchronize()
            for x, y in zip(back, (fp, conf, dec, risk)):
                np.testing.assert_array_equal(x.cpu().numpy(), y)
        assert all(e.counter("mlp_launches") == 3 for e in engines)
    finally:
        for e in engines:
            e.sync()
            e.close()


def test_mlp_behind_the_drop_in(tmp_path, forests):
    """a models directory with pytorch/gnn_fraud_model.pth: ModelManager loads graph_neural onto the engine, predict
    returns float32 within the bar of torch, another width raises, the ensemble lists the member"""
    import joblib
    import torch
    from fdengine.ensemble import EnsemblePredictor
    from fdengine.model_manager import EngineMlp, ModelManager
    from fdengine.registry import ScoringConfig
    w, X, ref = K.case(0)
    for sub in ("xgboost", "sklearn", "pytorch"):
        (tmp_path / sub).mkdir()
    Xref = synth.feature_matrix(2048, 64, seed=3)
    synth.write_xgboost_json(str(tmp_path / "xgboost" / "fraud_classifier.json"),
                             synth.xgboost_doc(40, 6, 64, Xref, seed=4, p_leaf=0.1))
    joblib.dump(synth.isolation_forest(Xref.astype(np.float64), n_estimators=20),
                tmp_path / "sklearn" / "isolation_forest.joblib")
    pth = tmp_path / "pytorch" / "gnn_fraud_model.pth"
    torch.save({k: torch.from_numpy(v) for k, v in M.state_dict(w).items()}, str(pth))
    cfg = ScoringConfig(str(tmp_path))
    cfg.disable_model("bert_text")
    cfg.disable_model("lstm_sequential")
    mm = ModelManager(cfg, device=0)
    try:
        asyncio.run(mm.load_all_models())
        assert mm.is_model_loaded("graph_neural") and isinstance(mm.models["graph_neural"], EngineMlp)
        assert mm.engine_slot("graph_neural") == FD_SLOT_MLP
        assert mm.get_model_info()["models"]["graph_neural"]["engine"]["in_dim"] == 64
        p = asyncio.run(mm.predict("graph_neural", X[:257]))
        assert p.dtype == np.float32 and p.shape == (257,)
        assert np.abs(p.astype(np.float64) - ref[:257]).max() <= TOL
        one = asyncio.run(mm.predict("graph_neural", X[5]))  # a 1-D input is one row
        assert one.shape == (1,) and one[0] == p[5]
        with pytest.raises(RuntimeError, match="cannot be multiplied"):
            asyncio.run(mm.predict("graph_neural", X[:4, :63]))
        ep = EnsemblePredictor(mm, cfg)
        feats = [{"transaction_id": f"t{i}", "amount": float(10 + i), "hour_of_day": 3 + i, "x": 0.25 * i}
                 for i in range(5)]
        batch = asyncio.run(ep.predict_batch(feats))
        from fdengine.ensemble import prepare_matrix
        pm = K.torch_forward(w, prepare_matrix(feats).astype(np.float32))
        for i, r in enumerate(batch):
            assert set(r["model_predictions"]) == {"xgboost_primary", "isolation_forest", "graph_neural"}
            assert abs(r["model_predictions"]["graph_neural"] - pm[i]) <= TOL
            single = asyncio.run(ep.predict(dict(feats[i], transaction_id=f"s{i}")))
            assert single["model_predictions"]["graph_neural"] == r["model_predictions"]["graph_neural"]
            assert single["fraud_probability"] == r["fraud_probability"]
        # a config whose architecture differs from the file: logged, not loaded (the reference's RuntimeError)
        cfg.models["graph_neural"].hyperparameters = {"num_layers": 4}
        with pytest.raises(Exception, match="size mismatch"):
            asyncio.run(mm.reload_model("graph_neural"))
        assert not mm.is_model_loaded("graph_neural")
        with pytest.raises(ValueError, match="not loaded"):
            mm.engine.mlp_predict(X[:2])
        cfg.models["graph_neural"].hyperparameters = {}
        asyncio.run(mm.reload_model("graph_neural"))
        assert mm.is_model_loaded("graph_neural")
        np.testing.assert_array_equal(asyncio.run(mm.predict("graph_neural", X[:257])), p)
        asyncio.run(mm.cleanup())
        assert not mm.is_model_loaded("graph_neural")
        with pytest.raises(ValueError, match="not loaded"):
            mm.engine.mlp_predict(X[:2])
    finally:
        mm.engine.close()
