"""GPU: every device search that turns a feature value into a bin — and the walks behind them — on rows that hold the
models' thresholds, their f32 next-up and next-down, +-0.0, +-FLT_MAX and +- the smallest denormal
(oracle/boundary_ref.py; tests/test_forest_boundaries_cpu.py proves the inputs and the reference on the CPU: every
(feature, threshold) is met, and a `<` for a `<=` or the reverse changes the leaves of at least 25 % of the rows).

The searches: split_bin_body (tree-split path: split_bin_kernel, split_bin_pair_kernel, the LSTM launch's bin blocks),
bin_of (forest kernels 4 and 6, tables in LDS or global memory), the full-row lockstep search of the fused
ensemble_kernel (LDS and global arm, several passes), search_lockstep / bin_compact_pass and the host-built constant
and small-integer bins of the pipeline's compact rows, the LSTM launch's inline search, and the float compares of the
threshold-layout kernels 1 and 3; under all of them the host rewrite of sklearn's `(double)x <= thr` to `x < t_f32`.

Bars (those of test_gpu_forest.py / test_gpu_ensemble.py): leaf ids exact; XGBoost raw margin bit-identical to the f32
reference sum; IsolationForest raw depth bit-identical to the f64 sum; probabilities within 1e-5 of the oracle;
IsolationForest probability within 1e-12 of sklearn. The reference is the plain numpy walk (walk_reference), which the
CPU tests tie to the C oracle and to sklearn."""
import numpy as np
import pytest

import oracle
from fdengine import FraudEngine, iforest_from_sklearn, synth, xgboost_from_json_doc
from fdengine import lstm as L
from fdengine._native import FD_SLOT_LSTM, FD_TIMING_ENSEMBLE, TXN_FIELDS
from oracle import boundary_ref as B
from oracle import scoring_ref as S

# (sklearn's own input check sums the matrix, and +FLT_MAX + -FLT_MAX rows overflow that sum: harmless)
pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:invalid value encountered in reduce")]

PROB_TOL = 1e-5
SK_TOL = 1e-12
NAMES = ["xgboost_primary", "isolation_forest"]

_probs = {}


def _oracle_prob(tag, fa, X):
    """the C oracle's probabilities (f64), once per (matrix, model)"""
    if tag not in _probs:
        p = (oracle.xgb_predict if B._is_xgb(fa) else oracle.iforest_predict)(fa, X)[0]
        _probs[tag] = p.astype(np.float64)
    return _probs[tag]


def _sklearn_prob(tag, m, X):
    if ("sk",) + tag not in _probs:
        _probs[("sk",) + tag] = 1.0 / (1.0 + np.exp(m.decision_function(X)))
    return _probs[("sk",) + tag]


def _check_raw(fa, raw, sums):
    if B._is_xgb(fa):
        np.testing.assert_array_equal(raw.astype(np.float32), sums)  # the reference's f32 sum sequence
        np.testing.assert_array_equal(raw, raw.astype(np.float32).astype(np.float64))
    else:
        np.testing.assert_array_equal(raw, sums)  # the same f64 sequence


def _check_prob(key, name, X, prob):
    fa, m = B.model(name)
    assert np.abs(prob - _oracle_prob((key, name), fa, X)).max() <= PROB_TOL
    if m is not None and not np.isnan(X).any():
        assert np.abs(prob - _sklearn_prob((key, name), m, X)).max() <= SK_TOL


def _params(strategy=0, lstm=False):
    names = NAMES + (["lstm_sequential"] if lstm else [])
    w = S.normalized_weights({"xgboost_primary": 0.4, "isolation_forest": 0.05, **({"lstm_sequential": 0.3} if lstm else {})})
    return FraudEngine.blend_params([w[k] for k in names], [S.CONF_MULT[k] for k in names], strategy=strategy)


# ------------------------------------------------------------------ 1. every forest kernel
SINGLE = [("ladder_nan", "ladder"), ("ladder_d3", "ladder_d3"), ("hist", "hist"), ("iforest", "iforest"),
          ("iforest_d3", "iforest_d3")]


@pytest.mark.parametrize("variant", [0, 1, 2, 3, 6, 8])
@pytest.mark.parametrize("key,name", SINGLE)
def test_every_forest_kernel(engine, key, name, variant):
    """forest_kernel 0 (at 1021 rows the tree-split path: split_bin_kernel), 1 / 2 (threshold layout: float compares),
    3 / 8 (kernels 4 / 6: bin_of), 6 (tree-split, forced): leaves and sums exact on boundary rows, NaNs included"""
    X, ref, _ = B.matrix(key)
    fa, _ = B.model(name)
    leaf, sums = ref[name]
    engine.load_forest(0, fa)
    engine.set_option("forest_kernel", variant)
    try:
        prob, raw, lf = engine.predict(0, X, want_raw=True, want_leaf=True)
    finally:
        engine.set_option("forest_kernel", 0)
    np.testing.assert_array_equal(lf, leaf)
    _check_raw(fa, raw, sums)
    _check_prob(key, name, X, prob)


@pytest.mark.parametrize("variant", [0, 2, 8])
def test_short_rows_on_boundary_values(engine, variant):
    """rows of 13 columns for the 18-feature ladder: the columns beyond are missing (default direction)"""
    X, _, _ = B.matrix("ladder")
    fa, _ = B.model("ladder")
    Xs = np.ascontiguousarray(X[:, :13])
    leaf, sums = B.walk_reference(fa, Xs)
    assert (leaf != B.matrix("ladder")[1]["ladder"][0]).any()
    engine.load_forest(0, fa)
    engine.set_option("forest_kernel", variant)
    try:
        prob, raw, lf = engine.predict(0, Xs, want_raw=True, want_leaf=True)
    finally:
        engine.set_option("forest_kernel", 0)
    np.testing.assert_array_equal(lf, leaf)
    _check_raw(fa, raw, sums)
    assert np.abs(prob - oracle.xgb_predict(fa, Xs)[0]).max() <= PROB_TOL


# ------------------------------------------------------------------ 2. one forest through the fused kernel
@pytest.mark.parametrize("key,name", [("ladder_fused", "ladder"), ("iforest_fused", "iforest")])
def test_single_forest_through_fused_kernel(engine, key, name):
    """128 tiles and a ragged one: fd_forest_predict without leaf ids runs ensemble_kernel over the one forest
    (counter ensemble_single_launches), with and without the raw output"""
    X, ref, _ = B.matrix(key)
    fa, _ = B.model(name)
    engine.load_forest(1, fa)
    c0 = engine.counter("ensemble_single_launches")
    prob = engine.predict(1, X)
    assert engine.counter("ensemble_single_launches") - c0 == 1
    prob2, raw = engine.predict(1, X, want_raw=True)
    assert engine.counter("ensemble_single_launches") - c0 == 2
    _check_raw(fa, raw, ref[name][1])
    np.testing.assert_array_equal(prob2, prob)
    _check_prob(key, name, X, prob)


# ------------------------------------------------------------------ 3. the fused pair
def _score(engine, params, X, fused):
    engine.set_option("ensemble", 1 if fused else 0)
    try:
        engine.read_timing()
        engine.set_timing(True)
        out = engine.score_matrix(params, [0, 1], X)
        engine.set_timing(False)
        used = engine.read_timing(FD_TIMING_ENSEMBLE)[1] > 0
    finally:
        engine.set_option("ensemble", 1)
    return out, used


# pair_passcut: plan_passes fills a pass while count + count / 32 + 1 <= stage_floats, where stage_floats =
# (2 * chunk buffer + 2 * 8 KiB of tiles) / 4 = 28672 (wide chunks) or 24576 (compact chunks). The merged tables of
# features 0 .. 4 hold about 20.1 k thresholds, which fit either; feature 5's 9 k more do not: pass 0 is features
# 0 .. 4, pass 1 starts at FEATURE 5, inside the lockstep group of features 4 .. 7
# (tests/test_forest_boundaries_cpu.py::test_passcut_plan_cuts_a_group_of_four asserts it for both layouts).
# pair_raw2: both tables (28 k entries) exceed stage_floats: the search in global memory.
@pytest.mark.parametrize("key,chunks,strategy", [("pair_passcut", 1, 0), ("pair_passcut", 2, 0), ("pair_passcut", 1, 1),
                                                 ("pair_passcut", 2, 1), ("pair_passcut", 1, 2), ("pair_passcut", 2, 2),
                                                 ("pair_raw2", 1, 0), ("pair_raw2", 2, 0)])
def test_fused_pair_on_boundary_rows(engine, key, chunks, strategy):
    X, ref, _ = B.matrix(key)
    names = B.MATRICES[key]["names"]
    fas = [B.model(n)[0] for n in names]
    params = _params(strategy)
    engine.load_forest(0, fas[0])
    engine.load_forest(1, fas[1])
    engine.set_option("ensemble_chunks", chunks)
    try:
        fused, used = _score(engine, params, X, True)
        assert used, "the fused ensemble kernel did not run"
        per_model, used2 = _score(engine, params, X, False)
        assert not used2
        engine.set_option("ensemble", 0)
        for slot, (n, fa) in enumerate(zip(names, fas)):  # the per-model path against the reference
            _, raw, lf = engine.predict(slot, X, want_raw=True, want_leaf=True)
            np.testing.assert_array_equal(lf, ref[n][0])
            _check_raw(fa, raw, ref[n][1])
    finally:
        engine.set_option("ensemble", 1)
        engine.set_option("ensemble_chunks", 0)
    for a, b in zip(fused, per_model):  # model probabilities, fraud probability, confidence, decision, risk
        np.testing.assert_array_equal(a, b)
    for m, n in enumerate(names):
        _check_prob(key, n, X, fused[0][m])


# ------------------------------------------------------------------ 4. the latency pair
def test_latency_pair_on_boundary_rows(engine):
    """score_matrix at 1021 rows (split_bin_pair_kernel + the pair walk): latency_fused 1 and 0 bit-identical, the
    forests' leaves exact"""
    key = "pair_latency"
    X, ref, _ = B.matrix(key)
    names = B.MATRICES[key]["names"]
    fas = [B.model(n)[0] for n in names]
    engine.load_forest(0, fas[0])
    engine.load_forest(1, fas[1])
    params = _params()
    try:
        engine.set_option("latency_fused", 1)
        a = engine.score_matrix(params, [0, 1], X)
        engine.set_option("latency_fused", 0)
        b = engine.score_matrix(params, [0, 1], X)
    finally:
        engine.set_option("latency_fused", 1)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)
    for slot, (n, fa) in enumerate(zip(names, fas)):
        prob, raw, lf = engine.predict(slot, X, want_raw=True, want_leaf=True)
        np.testing.assert_array_equal(lf, ref[n][0])
        _check_raw(fa, raw, ref[n][1])
        np.testing.assert_array_equal(a[0][slot], prob)
        _check_prob(key, n, X, a[0][slot])


# ------------------------------------------------------------------ 5. paths that see only the feature kernel's vectors
def _state_engine(pop, seq_len=0):
    U, M = pop["users"], pop["merchants"]
    eng = FraudEngine(0)
    eng.state_init(1 << 17, 1, 16, seq_len=seq_len)
    eng.load_users(U["key"], U["avg_amount"], U["account_age_days"], U["device_fp"])
    eng.load_merchants(M["fraud_rate"], M["risk_multiplier"])
    return eng


def _vector_world(pop, tx, sizes, seq_len, seed):
    """The vectors V of the batches to be scored (a warm twin's features, batch after batch), models whose thresholds
    are V's own values and their f32 neighbours, and what the models give on V: the numpy reference, the oracle's
    probabilities, and forest kernel 6's / 4's outputs (k6)."""
    cuts = np.concatenate([[0], np.cumsum(sizes)])
    batches = [{f: np.ascontiguousarray(tx[f][a:b]) for f in TXN_FIELDS} for a, b in zip(cuts[:-1], cuts[1:])]
    twin = _state_engine(pop, seq_len)
    try:
        V = [twin.features(b) for b in batches]
    finally:
        twin.close()
    Vall = np.concatenate(V)
    doc = synth.xgboost_doc(40, 8, 64, Vall, seed=seed, p_leaf=0.05, max_bin=None, base_score=0.3)
    xgb = xgboost_from_json_doc(B.nudge_split_conditions(doc, seed + 1))
    m = synth.isolation_forest(Vall.astype(np.float64), n_estimators=30)
    ifm = iforest_from_sklearn(B.rewrite_iforest_thresholds(m, Vall, seed=seed + 2))
    ref = [B.walk_reference(fa, Vall) for fa in (xgb, ifm)]
    orc = [oracle.xgb_predict(xgb, Vall)[0].astype(np.float64), oracle.iforest_predict(ifm, Vall)[0]]
    k6 = []
    eng = FraudEngine(0)
    try:
        # kernel 6 (option 8) for XGBoost; an IsolationForest over 64 features has no kernel 6 (its node-only chunks
        # with f64 leaf buffers exceed the 160 KiB LDS budget), so kernel 4 (option 3): the same bin_of search
        for slot, fa in enumerate((xgb, ifm)):
            eng.load_forest(slot, fa)
            eng.set_option("forest_kernel", 8 if slot == 0 else 3)
            k6.append(eng.predict(slot, Vall, want_raw=True, want_leaf=True))
    finally:
        eng.close()
    return dict(pop=pop, batches=batches, cuts=cuts, V=Vall, models=(xgb, ifm), sk=m, ref=ref, orc=orc, k6=k6)


def _check_vector_world(w):
    """kernel 6 / 4 on V against the reference (leaves and sums exact), so that bit-identity with their
    probabilities ties a path to the reference; and V detects a wrong comparison in at least 25 % of its rows"""
    for fa, (leaf, sums), orc, (prob, raw, lf) in zip(w["models"], w["ref"], w["orc"], w["k6"]):
        np.testing.assert_array_equal(lf, leaf)
        _check_raw(fa, raw, sums)
        assert np.abs(prob - orc).max() <= PROB_TOL
        for cmp_ in (("le",) if B._is_xgb(fa) else ("lt", "lt_f32", "le_f32")):
            share = B.changed_share(fa, w["V"], cmp_)
            print(f"coverage vectors wrong compare {cmp_:7s} changes {100 * share:5.1f} % of the rows")
            assert share >= 0.25
    assert np.abs(w["k6"][1][0] - 1.0 / (1.0 + np.exp(w["sk"].decision_function(w["V"])))).max() <= SK_TOL


def _check_model_probs(w, b, mp):
    a, e = w["cuts"][b], w["cuts"][b + 1]
    for m in range(2):
        np.testing.assert_array_equal(mp[m], w["k6"][m][0][a:e])  # kernel 6's / 4's bits, whose leaves are the reference's
        assert np.abs(mp[m] - w["orc"][m][a:e]).max() <= PROB_TOL


@pytest.fixture(scope="module")
def pipe_world():
    pop = synth.population(20000, 5000, seed=7)
    tx = synth.txn_stream(pop, 2 * B.N_FUSED, seed=8)
    return _vector_world(pop, tx, [B.N_FUSED, B.N_FUSED], 0, seed=31)


@pytest.fixture(scope="module")
def latency_world():
    pop = synth.population(3000, 500, seed=95)
    tx = synth.txn_stream(pop, 1 + 997 + 1024, seed=96, rate_per_s=50.0)
    return _vector_world(pop, tx, [1, 997, 1024], 10, seed=41)


def test_vector_models_reference_and_coverage(pipe_world, latency_world):
    _check_vector_world(pipe_world)
    _check_vector_world(latency_world)


@pytest.mark.parametrize("compact,bin_global", [(0, 0), (1, 0), (2, 0), (1, 1)])
def test_pipelined_rows_on_threshold_vectors(pipe_world, compact, bin_global):
    """score_batch_pipelined, two batches of 128 tiles + 77 rows, no vectors output: the 64-wide vector
    (compact_vectors 0: ensemble_kernel's full-row search), the compact 64-B row (1) and split rows (2): search_lockstep,
    the fixed 16-level global search, the plan's constant bins and small-integer table; ensemble_bin_global 1: every
    search in global memory"""
    import torch
    w = pipe_world
    eng = _state_engine(w["pop"])
    try:
        eng.load_forest(0, w["models"][0])
        eng.load_forest(1, w["models"][1])
        eng.set_option("compact_vectors", compact)
        eng.set_option("ensemble_bin_global", bin_global)
        eng.set_stream(torch.cuda.current_stream().cuda_stream)
        params = _params()
        outs, keep = [], []
        for b in w["batches"]:
            n = len(b["card_key"])
            dev = {f: torch.from_numpy(b[f]).cuda() for f in TXN_FIELDS}
            o = [torch.empty(n, dtype=t, device="cuda") for t in (torch.float64, torch.float64, torch.uint8, torch.uint8)]
            mp = torch.empty((2, n), dtype=torch.float64, device="cuda")
            eng.score_batch_pipelined(params, [0, 1], {f: t.data_ptr() for f, t in dev.items()}, n,
                                      *[x.data_ptr() for x in o], model_probs_ptr=mp.data_ptr())
            outs.append(mp)
            keep.append((dev, o))
        torch.cuda.synchronize()
        eng.sync()
        assert eng.counter("pipelined_compact_batches") == (2 if compact else 0)
        assert eng.counter("pipelined_split_batches") == (2 if compact == 2 else 0)
        for b, mp in enumerate(outs):
            _check_model_probs(w, b, mp.cpu().numpy())
    finally:
        eng.close()


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_latency_prebin_on_threshold_vectors(latency_world, mode):
    """score_batch_device with the LSTM head at latency sizes: split_bin_pair_kernel (latency_prebin 0), the LSTM
    launch's bin blocks (1, 2) and its inline search (3; the batch of 1 takes 2)"""
    import torch
    w = latency_world
    eng = _state_engine(w["pop"], seq_len=10)
    try:
        eng.load_forest(0, w["models"][0])
        eng.load_forest(1, w["models"][1])
        eng.load_lstm(L.random_weights(seed=8))
        eng.set_option("latency_prebin", mode)
        eng.set_stream(torch.cuda.current_stream().cuda_stream)
        params = _params(lstm=True)
        outs, keep = [], []
        for b in w["batches"]:
            n = len(b["card_key"])
            dev = {f: torch.from_numpy(b[f]).cuda() for f in TXN_FIELDS}
            o = [torch.empty(n, dtype=t, device="cuda") for t in (torch.float64, torch.float64, torch.uint8, torch.uint8)]
            mp = torch.empty((3, n), dtype=torch.float64, device="cuda")
            eng.score_batch_device(params, [0, 1, FD_SLOT_LSTM], {f: t.data_ptr() for f, t in dev.items()}, n,
                                   *[x.data_ptr() for x in o], model_probs_ptr=mp.data_ptr())
            outs.append(mp)
            keep.append((dev, o))
        torch.cuda.synchronize()
        assert eng.counter("latency_prebinned_batches") == (len(w["batches"]) if mode else 0)
        for b, mp in enumerate(outs):
            _check_model_probs(w, b, mp.cpu().numpy())
    finally:
        eng.close()
