"""GPU: the A/B tests on the engine (csrc/abtest.hip, fd_ab_* in engine.hip): assignment against the host bucket
function, the stable partition, routed scoring bit for bit against score_matrix on each variant's rows, the recorded
state against fd_ab_record_ref_host and the reference's own summaries (tests/golden/abtest_cases.npz), and the
drop-in ABTestManager. Tolerances: tests/abtest_cases.py.

Capacities the shapes are sized around (abtest.hip): a workgroup is 256 lanes (4 waves of 64) and takes 256 rows of an
assignment or a partition; the partition's offsets pass scans 256 workgroup counts per round (65 537 rows need a
second round); the record kernel gives a lane 4 rows before it adds workgroups, up to 256."""
import numpy as np
import pytest

import abtest_cases as T
from fdengine import FraudEngine, iforest_from_sklearn, synth, xgboost_from_json_doc

pytestmark = pytest.mark.gpu

ASSIGN_N = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097)
SCORE_N = (1, 65, 257, 1025, 4097)
NF = 12
TID = 5  # the engine test id these tests create and destroy
SLOT_X, SLOT_IF = 4, 5  # forest slots, unloaded again after the module


@pytest.fixture(scope="module")
def cases():
    return T.load()


@pytest.fixture()
def ab(engine):
    """creates engine test ids on request and destroys them afterwards (the engine is the session's)"""
    made = []

    def create(tid, name, split):
        import fdengine.ab_testing as A
        engine.ab_create(tid, A.salt_of(name), A.threshold_of(split))
        made.append(tid)
        return tid
    yield create
    for tid in made:
        try:
            engine.ab_destroy(tid)
        except ValueError:  # the test destroyed it itself
            pass


@pytest.fixture(scope="module")
def model_sets(engine):
    """control: a small XGBoost forest blended alone; treatment: that forest and a small IsolationForest"""
    Xr = synth.feature_matrix(2048, NF, seed=31)
    xgb = xgboost_from_json_doc(synth.xgboost_doc(24, 5, NF, Xr, seed=32, base_score=0.3))
    ifm = iforest_from_sklearn(synth.isolation_forest(Xr.astype(np.float64), n_estimators=16))
    engine.load_forest(SLOT_X, xgb)
    engine.load_forest(SLOT_IF, ifm)
    control = {"params": FraudEngine.blend_params([1.0], [1.0]), "slots": [SLOT_X]}
    treatment = {"params": FraudEngine.blend_params([0.8, 0.2], [1.0, 0.9]), "slots": [SLOT_X, SLOT_IF]}
    yield control, treatment
    engine.unload_forest(SLOT_X)  # the engine is the session's: other modules expect the slots they did not load empty
    engine.unload_forest(SLOT_IF)


def keys_of(n, seed):
    k = np.random.default_rng(seed).integers(0, 1 << 64, n, dtype=np.uint64)
    k[0] = 0  # (counts as key 1)
    return k


@pytest.mark.parametrize("split", T.SPLITS)
def test_assign_equals_the_host_rule(engine, ab, split):
    import fdengine.ab_testing as A
    name = f"assign_{split}"
    tid = ab(TID, name, split)
    for n in ASSIGN_N:
        keys = keys_of(n, n)
        got = engine.ab_assign(tid, keys)
        want = A.variants_of(keys, name, split)
        assert got.dtype == np.uint8 and (got == want).all(), (n, split)
    assert len(engine.ab_assign(tid, np.zeros(0, np.uint64))) == 0


def partition_columns():
    rng = np.random.default_rng(3)
    cols = {}
    for n in (1, 63, 64, 65, 255, 256, 257, 1025, 4097, 65537):
        cols[f"random_{n}"] = (rng.random(n) < 0.3).astype(np.uint8)
    cols["all_control"] = np.zeros(1025, np.uint8)
    cols["all_treatment"] = np.ones(1025, np.uint8)
    cols["alternating"] = (np.arange(1025) & 1).astype(np.uint8)
    cols["alternating_waves"] = ((np.arange(4097) >> 6) & 1).astype(np.uint8)
    cols["one_treatment_first"] = np.r_[1, np.zeros(600)].astype(np.uint8)
    cols["one_control_last"] = np.r_[np.ones(600), 0].astype(np.uint8)
    return cols


def test_partition_is_stable(engine):
    for name, v in partition_columns().items():
        idx, counts = engine.ab_partition(v)
        nc = int((v == 0).sum())
        assert counts.tolist() == [nc, len(v) - nc], name
        assert (idx[:nc] == np.flatnonzero(v == 0)).all(), name  # control rows, ascending
        assert (idx[nc:] == np.flatnonzero(v != 0)).all(), name  # then treatment rows, ascending
    idx, counts = engine.ab_partition(np.zeros(0, np.uint8))
    assert len(idx) == 0 and counts.tolist() == [0, 0]


def expect_routed(engine, control, treatment, X, variant):
    """score_matrix run separately on each variant's rows with its model set, put back by row"""
    n = len(X)
    m_max = max(control["params"].n_models, treatment["params"].n_models)
    mp = np.full((m_max, n), np.nan)
    fp, conf = np.empty(n), np.empty(n)
    dec, risk = np.empty(n, np.uint8), np.empty(n, np.uint8)
    for v, ms in enumerate((control, treatment)):
        rows = np.flatnonzero(variant == v)
        if len(rows) == 0:
            continue
        cols = None if ms.get("ext_probs") is None else [None if c is None else c[rows] for c in ms["ext_probs"]]
        out = engine.score_matrix(ms["params"], ms["slots"], X[rows], ext_probs=cols, present=ms.get("present"))
        mp[:out[0].shape[0], rows] = out[0]
        fp[rows], conf[rows], dec[rows], risk[rows] = out[1:]
    return mp, fp, conf, dec, risk


def assert_same_bits(got, want, what):
    for g, w, col in zip(got, want, ("model_probs", "fraud_prob", "confidence", "decision", "risk")):
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), (what, col)


@pytest.mark.parametrize("split", [0.0, 0.3, 1.0])
@pytest.mark.parametrize("n", SCORE_N)
def test_routed_scoring_equals_score_matrix_per_variant(engine, ab, model_sets, n, split):
    import fdengine.ab_testing as A
    control, treatment = model_sets
    name = f"route_{split}"
    tid = ab(TID, name, split)
    X = synth.feature_matrix(n, 16, seed=100 + n).astype(np.float32)
    keys = keys_of(n, 7 * n)
    var, *got = engine.ab_score_matrix(tid, control, treatment, X, keys)
    assert (var == A.variants_of(keys, name, split)).all() and (var == engine.ab_assign(tid, keys)).all()
    assert_same_bits(got, expect_routed(engine, control, treatment, X, var), (n, split))
    if split in (0.0, 1.0):  # one variant takes every row: plain score_matrix
        ms = treatment if split == 1.0 else control
        plain = engine.score_matrix(ms["params"], ms["slots"], X)
        M = ms["params"].n_models
        assert got[0][:M].tobytes() == plain[0].tobytes() and np.isnan(got[0][M:]).all()
        assert_same_bits(got[1:], plain[1:], (n, split, "plain"))


def test_routed_scoring_odd_stride_and_external_columns(engine, ab, model_sets):
    control, _ = model_sets
    n = 1025
    tid = ab(TID, "route_ext", 0.55)
    X = synth.feature_matrix(n, 16, seed=9).astype(np.float32)[:, :13].copy()  # ld 13: the scalar gather
    keys = keys_of(n, 11)
    rng = np.random.default_rng(12)
    # treatment: the forest, one externally computed column, and a dropped model
    treatment = {"params": FraudEngine.blend_params([0.5, 0.3, 0.2], [1.0, 0.9, 0.8]), "slots": [SLOT_X, -1, SLOT_IF],
                 "ext_probs": [None, rng.random(n), None], "present": [1, 1, 0]}
    var, *got = engine.ab_score_matrix(tid, control, treatment, X, keys)
    assert 0 < var.sum() < n
    want = expect_routed(engine, control, treatment, X, var)
    rows = var == 1
    assert (got[0][1, rows] == treatment["ext_probs"][1][rows]).all()
    # (a dropped model's column is whatever score_matrix leaves there: not compared)
    got[0][2, rows] = want[0][2, rows] = 0.0
    assert_same_bits(got, want, "external")


def test_routed_scoring_device_pointers(engine, ab, model_sets):
    import torch
    control, treatment = model_sets
    n = 1025
    tid = ab(TID, "route_dev", 0.3)
    X = synth.feature_matrix(n, 16, seed=5).astype(np.float32)
    keys = keys_of(n, 6)
    var, mp, fp, conf, dec, risk = engine.ab_score_matrix(tid, control, treatment, X, keys)
    dX, dk = torch.from_numpy(X).cuda(), torch.from_numpy(keys.view(np.int64)).cuda()
    dfp = torch.zeros(n, dtype=torch.float64, device="cuda")
    ddec = torch.zeros(n, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    engine.ab_score_matrix_device(tid, control, treatment, dX.data_ptr(), dk.data_ptr(), n, 16, dfp.data_ptr(),
                                  dec_ptr=ddec.data_ptr())  # no variant, model_probs, confidence or risk wanted
    engine.sync()
    assert dfp.cpu().numpy().tobytes() == fp.tobytes() and ddec.cpu().numpy().tobytes() == dec.tobytes()


def test_manager_score_batch(engine, model_sets):
    import fdengine.ab_testing as A
    control, treatment = model_sets
    mgr = A.ABTestManager(engine=engine)
    assert mgr.create_test(A.ABTestConfig("rollout", "champion", "challenger", 0.3, "s", "e"))
    users = [f"user_{i}" for i in range(300)]
    X = synth.feature_matrix(300, 16, seed=77).astype(np.float32)
    out = mgr.score_batch("rollout", X, users, control=control, treatment=treatment)
    assert out["variant"].tolist() == [int(mgr.get_variant("rollout", u) == A.TestVariant.TREATMENT) for u in users]
    want = expect_routed(engine, control, treatment, X, out["variant"])
    assert_same_bits([out[k] for k in ("model_probs", "fraud_probability", "confidence", "decision", "risk_level")],
                     want, "manager")
    mgr.record_batch("rollout", out["variant"], out["fraud_probability"], out["decision"], 0.8)
    s = mgr.get_test_summary("rollout")
    assert s["total_samples"] == 300 and s["control_metrics"]["avg_processing_time_ms"] == 0.8
    mgr.close()
    with pytest.raises(ValueError):  # close() freed the test's id
        engine.ab_state(0)


def test_manager_takes_ids_that_are_free_on_a_shared_engine(engine, ab):
    import fdengine.ab_testing as A
    ab(0, "someone_elses", 0.5)  # held by a direct caller before the manager asks
    ab(2, "and_another", 0.5)
    mgr = A.ABTestManager(engine=engine)
    cfg = lambda k: A.ABTestConfig(f"shared_{k}", "a", "b", 0.5, "s", "e")  # noqa: E731
    assert all(mgr.create_test(cfg(k)) for k in range(6))
    assert sorted(mgr._ids.values()) == [1, 3, 4, 5, 6, 7]
    assert mgr.create_test(cfg(6)) is False and mgr.get_active_tests() == [f"shared_{k}" for k in range(6)]
    mgr.record_batch("shared_0", np.array([0, 1], np.uint8), [0.25, 0.75], ["APPROVE", "DECLINE"], 1.0)
    assert mgr.get_test_summary("shared_0")["total_samples"] == 2
    assert engine.ab_state(0).variant[0].rows == 0  # the other caller's test is untouched
    assert mgr.stop_test("shared_0") and mgr.create_test(cfg(6)) and mgr._ids["shared_6"] == 1
    mgr.close()
    engine.ab_state(0), engine.ab_state(2)  # close() freed only the manager's ids
    with pytest.raises(ValueError):
        engine.ab_state(1)


def record(engine, tid, case, cut=None):
    n = len(case["variant"])
    for a, b in T.pieces(n, cut or max(n, 1)):
        engine.ab_record(tid, case["variant"][a:b], case["prediction"][a:b], case["decision"][a:b],
                         case["time_ms"][a:b], case["label"][a:b])
    return engine.ab_state(tid)


def counts_of(state):
    return [(s.rows, list(s.decisions), s.labeled, s.tp, s.fp, s.tn, s.fn) for s in state.variant]


@pytest.mark.parametrize("cut", [None, *T.CUTS])
def test_record_equals_host_counts_and_reference_summary(engine, ab, cases, cut):
    import fdengine.ab_testing as A
    from fdengine import _native as N
    ratios = {}
    for c in cases:
        tid = ab(TID, c["name"], c["split"])
        state = record(engine, tid, c, cut)
        host = N.fd_ab_state()
        A.record_ref(host, c["variant"], c["prediction"], c["decision"], c["time_ms"], c["label"])
        assert counts_of(state) == counts_of(host), c["name"]
        T.check_summary(A.summary_from_state(T.config_of(c), state), c, ratios)
        engine.ab_clear(tid)
        assert counts_of(engine.ab_state(tid)) == counts_of(N.fd_ab_state())
        engine.ab_destroy(tid)
    print("largest error / bound per field:", {k: round(v, 4) for k, v in ratios.items()})


def test_record_is_deterministic_and_scalar_time(engine, ab, cases):
    c = next(c for c in cases if c["name"] == "time_5000")
    a = record(engine, ab(TID, "twice", 0.5), c)
    b = record(engine, ab(TID + 1, "twice_again", 0.5), c)
    assert bytes(a) == bytes(b)
    n = len(c["variant"])
    tid = ab(TID + 2, "scalar", 0.5)
    engine.ab_record(tid, c["variant"], c["prediction"], c["decision"], 12.5, None)
    s = engine.ab_state(tid)
    assert s.variant[0].rows + s.variant[1].rows == n and s.variant[0].labeled == 0
    for v in s.variant:
        assert (v.time_ms.sum_hi + v.time_ms.sum_lo) / v.rows == 12.5 and v.time_ms.m2_hi == 0.0


def test_record_device_pointers(engine, ab, cases):
    import torch
    c = next(c for c in cases if c["name"] == "score_1025")
    want = record(engine, ab(TID, "host_cols", 0.5), c)
    dev = {k: torch.from_numpy(c[k]).cuda() for k in ("variant", "prediction", "decision", "time_ms", "label")}
    torch.cuda.synchronize()
    tid = ab(TID + 1, "device_cols", 0.5)
    engine.ab_record_device(tid, dev["variant"].data_ptr(), dev["prediction"].data_ptr(), dev["decision"].data_ptr(),
                            len(c["variant"]), time_ptr=dev["time_ms"].data_ptr(), label_ptr=dev["label"].data_ptr())
    assert bytes(engine.ab_state(tid)) == bytes(want)


def test_errors(engine, ab):
    from fdengine._native import NativeError
    with pytest.raises(ValueError):  # not created
        engine.ab_assign(TID, np.zeros(4, np.uint64))
    tid = ab(TID, "errors", 0.5)
    with pytest.raises(NativeError):  # the id is taken
        engine.ab_create(tid, 1, 50.0)
    for bad in (-1, 8):
        with pytest.raises(NativeError):
            engine.ab_create(bad, 1, 50.0)
    with pytest.raises(NativeError):
        engine.ab_create(TID + 1, 1, 100.5)


def test_drop_in_reproduces_the_reference(engine, cases):
    import fdengine.ab_testing as A
    mgr = A.ABTestManager(engine=engine, keep_results=True)
    small = next(c for c in cases if c["name"] == "small_both")
    for c in cases:
        assert mgr.create_test(T.config_of(c))
        name, n = c["name"], len(c["variant"])
        users = T.user_ids(name, n, 500 + [s[0] for s in T.SPECS].index(name))
        assert (mgr.assign_batch(name, users) == c["variant"]).all()  # the fixture's assignments, on the device
        assert (mgr.assign_batch(name, c["key"]) == c["variant"]).all()
        if c is small:  # row by row, by the reference's signature
            for i, u in enumerate(users):
                v = mgr.get_variant(name, u)
                assert v == (A.TestVariant.TREATMENT if c["variant"][i] else A.TestVariant.CONTROL)
                lab = int(c["label"][i])
                mgr.record_result(name, f"txn_{i}", v, "model", float(c["prediction"][i]),
                                  T.DECISIONS[c["decision"][i]], float(c["time_ms"][i]),
                                  None if lab == T.NO_LABEL else bool(lab))
            exp = mgr.export_results(name)
            assert exp["total_results"] == n == len(exp["results"]) and exp["results"][3]["transaction_id"] == "txn_3"
        else:
            dec = [T.DECISIONS[d] if d < 4 else T.OTHER_NAME for d in c["decision"]]
            lab = [None if x == T.NO_LABEL else bool(x) for x in c["label"]]
            mgr.record_batch(name, c["variant"], c["prediction"], dec, c["time_ms"], lab)
        T.check_summary(mgr.get_test_summary(name), c)
        assert mgr.stop_test(name) and mgr.get_test_summary(name) == {}
        assert mgr.export_results(name)["total_results"] == n
    assert mgr.get_active_tests() == []
    mgr.close()
