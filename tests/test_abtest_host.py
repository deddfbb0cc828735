"""CPU: the A/B tests' declared rule without a device: the bucket function against a restatement, the
threshold product's edges, the consistency of assignments, the summary assembled from fd_ab_record_ref_host's state
against the reference's own get_test_summary outputs (tests/golden/abtest_cases.npz, written by
golden/make_abtest_golden.py from ABTestManager), and the drop-in's surface. Tolerances: tests/abtest_cases.py."""
import numpy as np
import pytest

import abtest_cases as T

MASK = (1 << 64) - 1


def fmix64(k):
    k ^= k >> 33
    k = k * 0xFF51AFD7ED558CCD & MASK
    k ^= k >> 33
    k = k * 0xC4CEB9FE1A85EC53 & MASK
    return k ^ (k >> 33)


@pytest.fixture(scope="module")
def cases():
    return T.load()


def state_of(case, cut=None):
    """The case's rows through fd_ab_record_ref_host: one call, or calls of `cut` rows merged by the host merge"""
    import fdengine.ab_testing as A
    from fdengine import _native as N
    n = len(case["variant"])
    total = N.fd_ab_state()
    for a, b in T.pieces(n, cut or max(n, 1)):
        part = N.fd_ab_state()
        A.record_ref(part, case["variant"][a:b], case["prediction"][a:b], case["decision"][a:b],
                     case["time_ms"][a:b], case["label"][a:b])
        total = A.merge_states(total, part)
    return total


def counts_of(state):
    return [(s.rows, list(s.decisions), s.labeled, s.tp, s.fp, s.tn, s.fn) for s in state.variant]


def test_names_and_constants():
    import fdengine.ab_testing as A
    from fdengine import _native as N
    assert (N.FD_AB_MAX_TESTS, N.FD_AB_NO_LABEL, N.FD_TIMING_ABTEST) == (8, 255, 12)
    assert tuple(N.DECISIONS) == T.DECISIONS and T.NO_LABEL == N.FD_AB_NO_LABEL and T.OTHER == A.OTHER_DECISION
    assert [v.value for v in A.TestVariant] == ["control", "treatment"]
    cfg = A.ABTestConfig("t", "a", "b", 0.5, "s", "e")
    assert (cfg.success_metric, cfg.minimum_sample_size, cfg.significance_level) == ("fraud_detection_rate", 1000, 0.05)
    import ctypes as C
    assert C.sizeof(N.fd_ab_variant_state) == 144 and C.sizeof(N.fd_ab_state) == 288


def test_buckets_equal_the_restatement():
    import fdengine.ab_testing as A
    rng = np.random.default_rng(7)
    keys = rng.integers(0, 1 << 64, 10000, dtype=np.uint64)
    keys[:3] = (0, 1, MASK)
    for salt in (0, 1, A.salt_of("model_v2_rollout"), MASK):
        got = A.buckets_of(keys, salt)
        want = [fmix64((int(k) or 1) ^ salt) % 100 for k in keys]
        assert got.tolist() == want
    assert A.buckets_of(keys[:1], 5)[0] == A.buckets_of(keys[1:2], 5)[0]  # key 0 counts as key 1
    assert len(set(A.buckets_of(keys, 3).tolist())) == 100


def test_threshold_edges():
    import fdengine.ab_testing as A
    # a key for every bucket, found by search, so that the variant of each bucket goes through variants_of
    name = "edges"
    keys = np.arange(1, 4000, dtype=np.uint64)
    buckets = A.buckets_of(keys, A.salt_of(name))
    first = {int(b): int(k) for k, b in reversed(list(zip(keys, buckets)))}
    assert sorted(first) == list(range(100))
    per_bucket = np.array([first[b] for b in range(100)], np.uint64)
    for split, want in zip(T.SPLITS, T.TREATMENT_BUCKETS):
        got = A.variants_of(per_bucket, name, split)
        assert got.sum() == want, (split, int(got.sum()))
        assert got.tolist() == [1 if b < split * 100 else 0 for b in range(100)]
    assert 0.07 * 100 == 7.000000000000001  # the product the 8th bucket comes from


def test_assignment_is_consistent():
    import fdengine.ab_testing as A
    m1, m2 = A.ABTestManager(), A.ABTestManager()
    cfgs = [A.ABTestConfig("test_a", "x", "y", 0.5, "s", "e"), A.ABTestConfig("test_b", "x", "y", 0.5, "s", "e")]
    for m in (m1, m2):
        assert all(m.create_test(c) for c in cfgs)
    users = [f"user_{i}" for i in range(400)]
    a1 = [m1.get_variant("test_a", u) for u in users]
    assert a1 == [m1.get_variant("test_a", u) for u in users] == [m2.get_variant("test_a", u) for u in users]
    assert set(a1) == {A.TestVariant.CONTROL, A.TestVariant.TREATMENT}
    assert m1.get_variant("unknown", users[0]) is None
    # two test names: two salts
    keys = np.array([A.ABTestManager._key(u) for u in users], np.uint64)
    for name in ("test_a", "test_b"):
        want = [fmix64((int(k) or 1) ^ A.salt_of(name)) % 100 < 50 for k in keys]
        got = [m1.get_variant(name, u) == A.TestVariant.TREATMENT for u in users]
        assert got == want
    assert a1 != [m1.get_variant("test_b", u) for u in users]
    assert m1.get_variant("test_a", 12345) == m1.get_variant("test_a", "12345")


def test_fixture_holds_the_cases_it_should(cases):
    assert [c["name"] for c in cases] == [s[0] for s in T.SPECS]
    assert sorted({len(c["variant"]) for c in cases}) == [1, 63, 64, 65, 199, 200, 257, 1025, 5000]
    import fdengine.ab_testing as A
    for c in cases:  # the recorded variants are the engine's assignment of the recorded keys
        assert (A.variants_of(c["key"], c["name"], c["split"]) == c["variant"]).all()
    by = {c["name"]: c["summary"] for c in cases}
    assert by["empty_treatment"]["treatment_metrics"] == {} and by["empty_control"]["control_metrics"] == {}
    assert "statistical_analysis" not in by["one_side_small"] and "labeled_samples" not in by["rate_5000"]["control_metrics"]
    assert by["constant_scores"]["statistical_analysis"]["effect_size"] == 0.0
    assert by["zero_control_mean"]["statistical_analysis"]["relative_improvement_percent"] == 0
    assert "error" in by["unknown_metric"]["statistical_analysis"]
    assert "error" in by["precision_unlabeled_rows"]["statistical_analysis"]
    assert by["time_5000"]["statistical_analysis"]["is_significant"] is True
    assert T.GOLDEN.stat().st_size <= 512 * 1024


@pytest.mark.parametrize("cut", [None, *T.CUTS])
def test_summary_equals_the_reference(cases, cut):
    import fdengine.ab_testing as A
    ratios = {}
    for c in cases:
        state = state_of(c, cut)
        assert counts_of(state) == counts_of(state_of(c)), c["name"]
        T.check_summary(A.summary_from_state(T.config_of(c), state), c, ratios)
    print("largest error / bound per field:", {k: round(v, 4) for k, v in ratios.items()})


def test_merge_is_a_then_b_and_takes_empty_states(cases):
    import fdengine.ab_testing as A
    from fdengine import _native as N
    c = cases[7]
    whole = state_of(c)
    empty = N.fd_ab_state()
    for merged in (A.merge_states(empty, whole), A.merge_states(whole, empty)):
        assert bytes(merged) == bytes(whole)
    assert bytes(A.merge_states(empty, empty)) == bytes(empty)
    # a batch caller's one time per batch: the scalar form equals a column of that value
    a, b = N.fd_ab_state(), N.fd_ab_state()
    A.record_ref(a, c["variant"], c["prediction"], c["decision"], 12.5, c["label"])
    A.record_ref(b, c["variant"], c["prediction"], c["decision"], np.full(len(c["variant"]), 12.5), c["label"])
    assert bytes(a) == bytes(b)
    s = A.summary_from_state(T.config_of(c), a)
    assert s["control_metrics"]["avg_processing_time_ms"] == 12.5


def test_surface_matches_the_reference():
    import fdengine.ab_testing as A
    m = A.ABTestManager()
    ok = dict(test_name="t", control_model="a", treatment_model="b", traffic_split=0.3, start_time="s", end_time="e")
    for bad in (dict(traffic_split=-0.01), dict(traffic_split=1.01), dict(minimum_sample_size=99),
                dict(significance_level=0.009), dict(significance_level=0.11), dict(traffic_split="half")):
        assert m.create_test(A.ABTestConfig(**{**ok, **bad})) is False
    assert m.get_active_tests() == []
    for edge in (dict(traffic_split=0.0), dict(traffic_split=1.0, test_name="u"),
                 dict(minimum_sample_size=100, significance_level=0.01, test_name="v"),
                 dict(significance_level=0.1, test_name="w")):
        assert m.create_test(A.ABTestConfig(**{**ok, **edge})) is True
    assert m.create_test(A.ABTestConfig(**ok)) is False  # the name is taken
    assert m.get_active_tests() == ["t", "u", "v", "w"]
    assert m.get_test_summary("t") == {"test_name": "t", "status": "no_data", "total_samples": 0}
    assert m.get_test_summary("nope") == {} and m.export_results("nope") == {}
    exp = m.export_results("t")
    assert sorted(exp) == ["export_timestamp", "results", "test_name", "total_results"]
    assert exp["results"] == [] and exp["total_results"] == 0
    assert m.stop_test("t") is True and m.stop_test("t") is False
    assert m.get_active_tests() == ["u", "v", "w"] and m.get_test_summary("t") == {}
    assert m.get_variant("t", "user") is None
    m.record_result("t", "txn", A.TestVariant.CONTROL, "a", 0.5, "APPROVE", 1.0)  # a stopped test: ignored
    assert m.export_results("t")["total_results"] == 0
    assert m.create_test(A.ABTestConfig(**ok)) is True  # and the name is free again
    assert "keep_results=True" in A.ABTestManager.export_results.__doc__
    # the signatures a caller of the reference uses
    import inspect
    assert list(inspect.signature(m.record_result).parameters) == [
        "test_name", "transaction_id", "variant", "model_used", "prediction", "decision", "processing_time_ms",
        "actual_fraud"]
    assert list(inspect.signature(m.get_variant).parameters) == ["test_name", "user_id"]
