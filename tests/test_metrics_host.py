"""CPU: the prediction metrics' declared rule without a device: fd_metrics_record_ref_host /
fd_metrics_query_ref_host and the drop-in MetricsCollector over them (host_state=True) against the reference's own
outputs (tests/golden/metrics_cases.npz, written by golden/make_metrics_golden.py from MetricsCollector), the merge of
two ranks' summaries, the ring's eviction, the clock rules, the text exposition, and the record kernel's resources.
Tolerances: tests/metrics_cases.py."""
import asyncio
import ctypes as C
import inspect
import json
import math

import numpy as np
import pytest

import metrics_cases as T


@pytest.fixture(scope="module")
def cases():
    return T.load()


def collector(clock, **kw):
    import fdengine.monitoring as M
    return M.MetricsCollector(clock=lambda: clock[0], resolution_s=kw.pop("resolution_s", 0.0), host_state=True, **kw)


def ints_of(x):
    """every integer of a ctypes struct, by path (sums, min / max / timestamps are doubles and are left out)"""
    out = {}

    def walk(v, path):
        if isinstance(v, C.Structure):
            for name, _ in v._fields_:
                walk(getattr(v, name), f"{path}.{name}")
        elif isinstance(v, C.Array):
            for i, e in enumerate(v):
                walk(e, f"{path}[{i}]")
        elif isinstance(v, int):
            out[path] = v
    walk(x, "")
    return out


def floats_of(x):
    out = {}

    def walk(v, path):
        if isinstance(v, C.Structure):
            for name, _ in v._fields_:
                walk(getattr(v, name), f"{path}.{name}")
        elif isinstance(v, C.Array):
            for i, e in enumerate(v):
                walk(e, f"{path}[{i}]")
        elif isinstance(v, float):
            out[path] = v
    walk(x, "")
    return out


def test_names_constants_and_layout():
    import fdengine.monitoring as M
    from fdengine import _native as N
    assert (N.FD_METRICS_MAX_MODELS, N.FD_METRICS_SERIES, N.FD_METRICS_SCORE_BUCKETS, N.FD_METRICS_TIME_BUCKETS) == \
        (8, 9, 12, 12)
    assert N.METRICS_SCORE_BOUNDS == T.SCORE_BOUNDS and tuple(b * 1000 for b in N.METRICS_TIME_BOUNDS) == T.TIME_BOUND_MS
    assert (C.sizeof(N.fd_metrics_series), C.sizeof(N.fd_metrics_cumulative), C.sizeof(N.fd_metrics_window_model),
            C.sizeof(N.fd_metrics_window), C.sizeof(N.fd_metrics_summary)) == (176, 1760, 80, 680, 3144)
    assert N.lib.fd_abi_version() == 15
    assert N.lib.fd_metrics_state_bytes(1) == 40 + 1760 + 688 and N.lib.fd_metrics_state_bytes(0) == 0
    assert N.lib.fd_metrics_state_bytes(4096) - N.lib.fd_metrics_state_bytes(4095) == 688
    m = M.MetricsCollector()  # no engine, no device: an empty collector answers
    got = asyncio.run(m.get_metrics())
    assert got["system"]["total_predictions"] == 0 and got["models"] == {} and m.engine is None
    assert got["performance"] == {"avg_processing_time_ms": 0.0, "predictions_per_second": 0.0,
                                  "predictions_last_hour": 0, "predictions_last_minute": 0}
    assert asyncio.run(m.get_model_performance_report())["models"] == {}
    M.MetricsCollector()  # a second one in the process: no DuplicateTimeseries
    assert M.PredictionMetric("t", 1.0, 2.0, 0.5, "APPROVE").model_predictions == {}


def test_fixture_holds_the_streams_it_should(cases):
    assert [c["name"] for c in cases] == [s[0] for s in T.SPECS]
    sizes = {op[1] for c in cases for op in c["script"] if op[0] == "rec"}
    assert sizes == set(T.CALL_SIZES)
    assert all(len(c["p"]) <= 10000 for c in cases)
    assert sorted(len(c["model_names"]) for c in cases) == [0, 1, 2, 2, 8]
    edges = cases[0]
    for v in T.SCORE_EDGES:
        assert (edges["p"] == v).any()
    for v in T.TIME_EDGES:
        assert (edges["time_ms"] == v).any()
    for v in T.MODEL_EDGES:
        assert (edges["mp"][0] == v).any()
    assert set(edges["decision"].tolist()) == {0, 1, 2, 3, T.OTHER}
    assert np.isnan(cases[3]["mp"]).any() and np.isnan(cases[3]["mp"][7, :1025]).all()
    assert T.GOLDEN.stat().st_size <= 1024 * 1024


@pytest.mark.parametrize("cut", [None, *T.CUTS])
def test_host_form_equals_the_reference(cases, cut):
    ratios = {}
    for c in cases:
        clock = [0.0]
        m = collector(clock)

        def check(now, want, rows, stamps):
            T.check_metrics(m.metrics_dict(), want["metrics"], c, now, rows, stamps, ratios)
            T.check_report(m.model_performance_report(), want["report"], c, now, rows, stamps, ratios)
            assert m.last_predictions() == want["last_prediction"], (c["name"], now)
        T.replay(m, clock, c, cut, check)
        m.update_system_metrics()
        T.check_samples(m.prometheus_samples(), c, ratios)
    print("largest error / bound per quantity:", {k: round(v, 4) for k, v in ratios.items()})


def test_merge_of_two_ranks_equals_the_whole(cases):
    import fdengine.monitoring as M
    c = cases[3]
    whole, a, b = M.HostState(8, 64), M.HostState(8, 64), M.HostState(8, 64)
    empty = M.HostState(8, 64).query(0.0)
    for st in T.steps(c):
        if st[0] == "rec":
            _, x, y, ts, t = st
            cols = lambda rows: (c["p"][rows], c["decision"][rows], c["mp"][:, rows],  # noqa: E731
                                 t if np.ndim(t) == 0 else c["time_ms"][rows])
            whole.record(*cols(slice(x, y)), ts)
            a.record(*cols(slice(x, y, 2)), ts)       # rank a: every other row of the call
            if y - x > 1:
                b.record(*cols(slice(x + 1, y, 2)), ts)
            continue
        now = st[1]
        w, merged = whole.query(now), M.merge_summaries(a.query(now), b.query(now))
        wi, mi = ints_of(w), ints_of(merged)
        wi.pop(".slots_used"), mi.pop(".slots_used")  # (the ranks' rings are counted separately)
        assert wi == mi, now
        wf, mf = floats_of(w), floats_of(merged)
        for k, v in wf.items():
            if k.endswith((".hi", ".lo")):
                continue
            assert mf[k] == v, (now, k)  # min, max, last_timestamp, newest
        for k in [k[:-3] for k in wf if k.endswith(".hi")]:
            sw, sm = wf[k + ".hi"] + wf[k + ".lo"], mf[k + ".hi"] + mf[k + ".lo"]
            assert abs(sw - sm) <= 2 * math.ulp(sw), (now, k, sw, sm)
        for s in (w, merged):  # merging with an empty summary changes nothing
            assert bytes(M.merge_summaries(s, empty)) == bytes(s) and bytes(M.merge_summaries(empty, s)) == bytes(s)


def test_sums_are_within_an_ulp_of_exact(cases):
    import fdengine.monitoring as M
    c = cases[4]
    h = M.HostState(2, 16)
    for st in T.steps(c):
        if st[0] == "rec":
            _, x, y, ts, t = st
            h.record(c["p"][x:y], c["decision"][x:y], c["mp"][:, x:y], t, ts)
    s = h.query(0.0).total
    for got, x in ((s.score_sum, c["p"]), (s.series[0].time_ms, c["time_ms"]),
                   (s.series[0].seconds, c["time_ms"] / 1000.0)):
        exact = math.fsum(x.tolist())
        assert abs(got.value - exact) <= math.ulp(exact), (got.value, exact)


def test_ring_of_eight_slots_evicts_the_oldest():
    import fdengine.monitoring as M
    rng = np.random.default_rng(5)
    h = M.HostState(1, 8)
    stamps = 1000.0 + 25.0 * np.arange(13)  # 13 stamps through 8 slots
    rows = rng.integers(1, 40, len(stamps))
    p, t, q, ts_of = [], [], [], []
    for ts, n in zip(stamps, rows):
        for _ in range(2):  # two calls per stamp: the second merges
            pp, tt, qq = rng.random(n), 1.0 + 99.0 * rng.random(n), rng.random(n)
            h.record(pp, np.zeros(n, np.uint8), qq[None, :], tt, ts)
            p.append(pp), t.append(tt), q.append(qq), ts_of.append(np.full(n, ts))
    p, t, q, ts_of = map(np.concatenate, (p, t, q, ts_of))
    for now in (stamps[-1], stamps[-1] + 35.0, stamps[-1] + 60.0, stamps[5] + 3600.0):
        s = h.query(now)
        assert (s.evictions, s.slots_used, s.newest) == (5, 8, stamps[-1])
        assert s.total.predictions == len(p)  # the cumulative part forgets nothing
        kept = ts_of >= stamps[5]  # the 8 newest stamps
        for win, limit in ((s.hour, 3600.0), (s.minute, 60.0)):
            rows_in = kept & (now - ts_of <= limit)
            assert win.rows == rows_in.sum() and win.fraud == (p[rows_in] > 0.5).sum()
            assert win.high_risk == (p[rows_in] > 0.8).sum()
            m = win.model[0]
            assert m.rows == rows_in.sum()
            assert list(m.dist) == [(q[rows_in] < 0.3).sum(), ((q[rows_in] >= 0.3) & (q[rows_in] < 0.7)).sum(),
                                    (q[rows_in] >= 0.7).sum()]
            if rows_in.any():
                assert (m.min_time_ms, m.max_time_ms) == (t[rows_in].min(), t[rows_in].max())
                assert abs(win.time_ms.value - math.fsum(t[rows_in].tolist())) <= math.ulp(win.time_ms.value)
            else:
                assert (m.min_time_ms, m.max_time_ms, win.time_ms.value) == (0.0, 0.0, 0.0)
    h.clear()
    s = h.query(0.0)
    assert (s.evictions, s.slots_used, s.total.predictions) == (0, 0, 0)


def test_clock_may_not_run_backwards_and_bad_arguments():
    import fdengine.monitoring as M
    from fdengine import _native as N
    h = M.HostState(2, 4)
    one = (np.array([0.7]), np.array([2], np.uint8))
    h.record(*one, None, 1.0, 100.0)
    for bad in (99.999, float("nan")):
        with pytest.raises(N.NativeError) as e:
            h.record(*one, None, 1.0, bad)
        assert e.value.code == N.FD_ERR_INVALID_ARG
    h.record(*one, None, 1.0, 100.0)  # the same stamp again is fine, and the rejected calls left nothing
    with pytest.raises(N.NativeError) as e:  # more model columns than the collector was made for
        h.record(*one, np.zeros((3, 1)), 1.0, 100.0)
    assert e.value.code == N.FD_ERR_INVALID_ARG
    s = h.query(100.0)
    assert (s.total.predictions, s.total.declined, s.hour.rows, s.slots_used) == (2, 2, 2, 1)
    for params in ((9, 4), (-1, 4), (2, 0), (2, 65537)):
        with pytest.raises(N.NativeError):
            M.HostState(*params)
    blank = np.zeros(N.lib.fd_metrics_state_bytes(4) // 8, np.uint64)  # a state nobody initialised
    with pytest.raises(ValueError):
        N.call("fd_metrics_query_ref_host", C.c_void_p(blank.ctypes.data), 0.0, C.byref(N.fd_metrics_summary()))


def test_drop_in_quantises_timestamps_as_documented():
    import fdengine.monitoring as M
    clock = [0.0]
    m = collector(clock, resolution_s=1.0, slots=4)
    assert [m.stamp(t) for t in (1000.0, 1000.999, 1001.0, -0.5)] == [1000.0, 1000.0, 1001.0, -1.0]
    assert collector(clock, resolution_s=0.25).stamp(1000.6) == 1000.5 and collector(clock).stamp(1000.6) == 1000.6
    for t in (1000.0, 1000.4, 1000.999, 1001.2, 1002.0, 1002.5):  # six calls, three stamps
        clock[0] = t
        m.record_batch([0.9], ["DECLINE"], None, (), 2.0)
    clock[0] = 1061.5
    s = m.summary()
    assert (s.slots_used, s.newest, s.evictions) == (3, 1002.0, 0)
    # the windows are the reference's over the stamps: at 1061.5 the rows stamped 1001.0 are 60.5 s old, although
    # the call at 1001.2... was made 60.3 s ago
    assert s.minute.rows == 2 and s.hour.rows == 6
    clock[0] = 1061.0  # ... and at 1061.0 the row recorded at 1001.2 is still in, stamped 1001.0
    assert m.summary().minute.rows == 3
    assert "floor(clock() / resolution_s) * resolution_s" in M.__doc__


def test_drop_in_surface_matches_the_reference():
    import fdengine.monitoring as M
    clock = [500.0]
    m = collector(clock)
    sig = lambda f: list(inspect.signature(f).parameters)  # noqa: E731
    assert sig(m.record_prediction) == ["transaction_id", "processing_time_ms", "fraud_probability", "decision",
                                        "model_predictions"]
    assert sig(m.record_error) == ["error_message", "error_type"]
    assert sig(m.update_model_metrics) == ["model_name", "is_active", "accuracy"]
    for name in ("record_prediction", "record_error", "update_model_metrics", "get_metrics",
                 "get_model_performance_report", "get_error_summary"):
        assert inspect.iscoroutinefunction(getattr(m, name)), name
    for name in ("update_system_metrics", "get_prometheus_metrics", "get_uptime", "_get_risk_level", "reset_metrics"):
        assert callable(getattr(m, name)) and not inspect.iscoroutinefunction(getattr(m, name)), name
    assert [m._get_risk_level(p) for p in (0.95, 0.8, 0.6, 0.3, 0.29)] == ["CRITICAL", "HIGH", "MEDIUM", "LOW",
                                                                           "VERY_LOW"]
    # model_predictions=None, the reference's default (it raises there after counting the row): treated as {}
    asyncio.run(m.record_prediction("t0", 12.0, 0.97, "DECLINE"))
    asyncio.run(m.record_prediction("t1", 8.0, 0.2, "APPROVE", {"xgb": 0.25, "iforest": 0.75}))
    asyncio.run(m.record_prediction("t2", 4.0, 0.55, "REVIEW", {"iforest": 0.4}))
    asyncio.run(m.record_error("boom " * 40, "timeout"))
    clock[0] = 530.0
    asyncio.run(m.update_model_metrics("xgb", accuracy=0.91))
    got = asyncio.run(m.get_metrics())
    assert got["system"] == {"uptime_seconds": 30.0, "total_predictions": 3, "total_errors": 1, "fraud_detections": 2,
                             "declined_transactions": 1, "error_rate": 1 / 3}
    assert got["performance"] == {"avg_processing_time_ms": 8.0, "predictions_per_second": 3 / 60.0,
                                  "predictions_last_hour": 3, "predictions_last_minute": 3}
    assert got["fraud_detection"] == {"fraud_rate": 2 / 3, "fraud_detections_last_hour": 2,
                                      "high_risk_transactions": 1}
    assert list(got["models"]) == ["xgb", "iforest"] and got["models"]["iforest"]["avg_processing_time_ms"] == 6.0
    assert got["models"]["xgb"] == {**got["models"]["xgb"], "total_predictions": 1, "error_rate": 0.0}
    rep = asyncio.run(m.get_model_performance_report())
    assert rep["time_window"] == "1 hour" and rep["total_predictions"] == 3
    assert rep["models"]["iforest"] == {
        "total_predictions": 2, "avg_processing_time_ms": 6.0, "min_processing_time_ms": 4.0,
        "max_processing_time_ms": 8.0, "avg_prediction_score": (0.75 + 0.4) / 2,
        "prediction_distribution": {"low_risk": 0, "medium_risk": 1, "high_risk": 1}}
    err = asyncio.run(m.get_error_summary())
    assert err["total_errors_last_hour"] == 1 and err["error_types"] == {"timeout": 1}
    assert len(err["recent_errors"][0]["message"]) == 100 and err["error_rate"] == 1 / 3
    samples = m.prometheus_samples()
    assert samples[("ml_errors_total", (("error_type", "timeout"),))] == 1.0
    assert samples[("ml_model_accuracy", (("model_name", "xgb"),))] == 0.91 * 100
    assert samples[("ml_avg_processing_time_ms", (("model_name", "xgb"),))] == 8.0
    assert samples[("ml_active_models", ())] == 1.0
    text = m.get_prometheus_metrics()
    assert isinstance(text, bytes) and b"ml_prediction_throughput_per_second 0.05\n" in text
    assert m.get_uptime() == 30.0
    with pytest.raises(ValueError):  # a ninth model name
        m.record_batch([0.5], ["APPROVE"], np.zeros((9, 1)), [f"m{k}" for k in range(9)], 1.0)
    m.reset_metrics()
    got = asyncio.run(m.get_metrics())
    assert got["system"]["total_predictions"] == 0 and got["models"] == {} and got["system"]["total_errors"] == 0


def test_text_exposition_parses_to_the_reference_samples(cases):
    parser = pytest.importorskip("prometheus_client.parser")
    for c in cases:
        clock = [0.0]
        m = collector(clock)
        T.replay(m, clock, c)
        text = m.get_prometheus_metrics().decode()
        got = {}
        for fam in parser.text_string_to_metric_families(text):
            for s in fam.samples:
                got[T.sample_key(s.name, dict(s.labels))] = float(s.value)
        assert got == {k: v for k, v in m.prometheus_samples().items()}  # the text says what the samples say
        T.check_samples(got, c)
        types = dict(line.split()[2:4] for line in text.splitlines() if line.startswith("# TYPE"))
        assert types["ml_predictions_total"] == "counter" and types["ml_fraud_score_distribution"] == "histogram"
        assert types["ml_active_models"] == "gauge"


def test_record_kernel_resources():
    from fdengine.build import RESOURCES
    if not RESOURCES.exists():
        pytest.skip("no kernel_resources.json: build the library first (__graft_entry__.build())")
    res = json.loads(RESOURCES.read_text())
    rec = [v for k, v in res.items() if "metrics_record_kernel" in k]
    assert len(rec) == 1
    assert rec[0]["scratch"] == 0, rec[0]
    # LDS: 4 wave partials of 70 doubles, 208 32-bit counters, the last-workgroup flag (padded to 8 bytes)
    assert rec[0]["lds"] == 4 * 70 * 8 + 208 * 4 + 8, rec[0]
    import fdengine
    src = (fdengine._native.PKG_ROOT / "csrc" / "metrics.hip").read_text()
    code = [line.split("//")[0] for line in src.splitlines()]
    adds = [line for line in code if "atomicAdd(" in line or "atomic_fetch" in line]
    assert len(adds) == 3 and all("unsigned" in a or "s_cnt" in a or "ticket" in a for a in adds), adds
