"""GPU: the prediction metrics on the engine (csrc/metrics.hip, fd_metrics_* in engine.hip): the device summary
against fd_metrics_record_ref_host bit for bit, the device and the drop-in MetricsCollector against the reference's own
outputs (tests/golden/metrics_cases.npz), determinism across engines, the device-pointer path fed by a scoring call's
outputs, a pinned-column host call, and the error paths (every bad argument is rejected on the host before any launch).
Tolerances: tests/metrics_cases.py.

Capacities the shapes are sized around (metrics.hip): a workgroup is 256 lanes (4 waves of 64); the record kernel gives
a lane 4 rows before it adds workgroups (1025 rows: two workgroups and the ticket reduction; 5000: five); a ring of 64
slots holds every stream's stamps without eviction (eviction is tested on the host form, tests/test_metrics_host.py)."""
import ctypes as C

import numpy as np
import pytest

import metrics_cases as T

pytestmark = pytest.mark.gpu

SLOT_X, SLOT_IF = 4, 5  # forest slots, unloaded again after the test that loads them
NF = 12


@pytest.fixture(scope="module")
def cases():
    return T.load()


def walk(v, path=""):
    """(path, value) of every number of a ctypes struct"""
    if isinstance(v, C.Structure):
        for name, _ in v._fields_:
            yield from walk(getattr(v, name), f"{path}.{name}")
    elif isinstance(v, C.Array):
        for i, e in enumerate(v):
            yield from walk(e, f"{path}[{i}]")
    else:
        yield path, v


def assert_same_summary(dev, host, what):
    """every integer equal; min / max / last and the float sums equal in bits (the calls are cut the same way)"""
    for (path, d), (_, h) in zip(walk(dev), walk(host)):
        if isinstance(d, float):
            assert np.float64(d).tobytes() == np.float64(h).tobytes(), (what, path, d, h)
        else:
            assert d == h, (what, path, d, h)
    assert bytes(dev) == bytes(host), what


def feed(record, case, cut=None, query=None):
    for st in T.steps(case, cut):
        if st[0] == "rec":
            _, a, b, ts, t = st
            record(case["p"][a:b], case["decision"][a:b], case["mp"][:, a:b] if len(case["mp"]) else None, t, ts)
        elif query is not None:
            query(st[1])


@pytest.mark.parametrize("cut", [None, 1, 64, 1000])
def test_device_summary_equals_the_host_reference(engine, cases, cut):
    import fdengine.monitoring as M
    for c in cases:
        if cut == 1 and len(c["p"]) > 500:  # one launch per row: the small streams only
            continue
        engine.metrics_init(8, 64)
        host = M.HostState(8, 64)
        seen = []

        def both(*cols):
            engine.metrics_record(*cols)
            host.record(*cols)

        def query(now):
            assert_same_summary(engine.metrics_query(now), host.query(now), (c["name"], cut, now))
            seen.append(now)
        feed(both, c, cut, query)
        assert len(seen) == len(c["results"])
    engine.metrics_clear()
    s = engine.metrics_query(0.0)
    assert bytes(s) == bytes(M.HostState(8, 64).query(0.0)) and s.total.predictions == 0


def test_device_and_drop_in_equal_the_reference(engine, cases):
    import fdengine.monitoring as M
    ratios = {}
    for c in cases:
        clock = [0.0]
        m = M.MetricsCollector(engine=engine, clock=lambda: clock[0], resolution_s=0.0, slots=64)

        def check(now, want, rows, stamps):
            T.check_metrics(m.metrics_dict(), want["metrics"], c, now, rows, stamps, ratios)
            T.check_report(m.model_performance_report(), want["report"], c, now, rows, stamps, ratios)
            assert m.last_predictions() == want["last_prediction"], (c["name"], now)
        T.replay(m, clock, c, None, check)
        m.update_system_metrics()
        T.check_samples(m.prometheus_samples(), c, ratios)
        m.close()  # (not the session's engine: the collector does not own it)
    print("largest error / bound per quantity:", {k: round(v, 4) for k, v in ratios.items()})


def test_two_fresh_engines_give_identical_bytes(cases):
    from fdengine import FraudEngine
    c = cases[4]  # 5000 + 1025 rows under one stamp: five and two workgroups, merged into one slot
    out = []
    for _ in range(2):
        with FraudEngine(0) as eng:
            eng.metrics_init(2, 16)
            got = []
            feed(eng.metrics_record, c, None, lambda now: got.append(bytes(eng.metrics_query(now))))
            out.append(got)
    assert out[0] == out[1] and len(out[0]) == len(c["results"])


def test_device_pointers_from_a_scoring_call(engine):
    import torch
    from fdengine import FraudEngine, iforest_from_sklearn, synth, xgboost_from_json_doc
    import fdengine.monitoring as M
    n = 257
    Xr = synth.feature_matrix(2048, NF, seed=31)
    engine.load_forest(SLOT_X, xgboost_from_json_doc(synth.xgboost_doc(24, 5, NF, Xr, seed=32, base_score=0.3)))
    engine.load_forest(SLOT_IF, iforest_from_sklearn(synth.isolation_forest(Xr.astype(np.float64), n_estimators=16)))
    try:
        params = FraudEngine.blend_params([0.8, 0.2], [1.0, 0.9])
        X = synth.feature_matrix(n, 16, seed=8).astype(np.float32)
        dX = torch.from_numpy(X).cuda()
        dmp = torch.zeros((2, n), dtype=torch.float64, device="cuda")
        dfp = torch.zeros(n, dtype=torch.float64, device="cuda")
        ddec = torch.zeros(n, dtype=torch.uint8, device="cuda")
        dtime = torch.from_numpy(0.5 + np.arange(n) * 0.25).cuda()
        torch.cuda.synchronize()
        engine.score_matrix_device(params, [SLOT_X, SLOT_IF], dX.data_ptr(), n, 16, dfp.data_ptr(),
                                   mp_ptr=dmp.data_ptr(), dec_ptr=ddec.data_ptr())
        # the scoring call's outputs straight into the collector, on the same stream, nothing read back in between
        engine.metrics_init(2, 8)
        engine.metrics_record_device(dfp.data_ptr(), ddec.data_ptr(), n, 1000.0, dmp.data_ptr(), 2, dtime.data_ptr())
        engine.metrics_record_device(dfp.data_ptr(), ddec.data_ptr(), n, 1000.0, dmp.data_ptr(), 2, 0, 3.5)
        dev = engine.metrics_query(1000.0)
        assert dev.total.predictions == 2 * n and dev.hour.model[1].rows == 2 * n
        host = M.HostState(2, 8)  # the host-column path on the columns read back
        fp, dec, mp, t = dfp.cpu().numpy(), ddec.cpu().numpy(), dmp.cpu().numpy(), dtime.cpu().numpy()
        host.record(fp, dec, mp, t, 1000.0)
        host.record(fp, dec, mp, 3.5, 1000.0)
        assert_same_summary(dev, host.query(1000.0), "device pointers")
        engine.metrics_init(2, 8)
        engine.metrics_record(fp, dec, mp, t, 1000.0)
        engine.metrics_record(fp, dec, mp, 3.5, 1000.0)
        assert bytes(engine.metrics_query(1000.0)) == bytes(dev)
        # the drop-in on the device tensors
        clock = [1000.75]
        m = M.MetricsCollector(engine=engine, clock=lambda: clock[0])
        m.record_batch(dfp, ddec, dmp, ["xgboost_primary", "isolation_forest"], dtime)
        m.record_batch(dfp, ddec, dmp, ["xgboost_primary", "isolation_forest"], 3.5)
        assert bytes(m.summary(1000.0)) == bytes(dev)  # stamped floor(1000.75) = 1000.0
        got = m.metrics_dict()
        assert got["system"]["total_predictions"] == 2 * n and list(got["models"]) == ["xgboost_primary",
                                                                                         "isolation_forest"]
        # columns given in another order than the names were first seen in: rearranged on the device
        m2 = M.MetricsCollector(engine=engine, clock=lambda: clock[0])
        m2.record_batch(dfp, ddec, dmp[:1].contiguous(), ["isolation_forest"], dtime)
        m2.record_batch(dfp, ddec, dmp, ["xgboost_primary", "isolation_forest"], dtime)
        s2 = m2.summary()
        assert [s2.total.series[k].rows for k in (0, 1, 2)] == [2 * n, 2 * n, n]
        assert list(m2.metrics_dict()["models"]) == ["isolation_forest", "xgboost_primary"]
    finally:
        engine.unload_forest(SLOT_X)
        engine.unload_forest(SLOT_IF)


def test_pinned_columns(engine, cases):
    import torch
    import fdengine.monitoring as M
    c = cases[3]
    n = 1025
    engine.metrics_init(8, 8)
    pinned = [torch.from_numpy(np.ascontiguousarray(a)).pin_memory() for a in
              (c["p"][:n], c["decision"][:n], c["mp"][:, :n], c["time_ms"][:n])]
    engine.metrics_record(*[t.numpy() for t in pinned], 100.0)
    dev = engine.metrics_query(100.0)  # waits for the stream: the pinned columns may go after it
    host = M.HostState(8, 8)
    host.record(c["p"][:n], c["decision"][:n], c["mp"][:, :n], c["time_ms"][:n], 100.0)
    assert_same_summary(dev, host.query(100.0), "pinned")


def test_errors(cases):
    from fdengine import FraudEngine
    from fdengine._native import FD_ERR_INVALID_ARG, NativeError
    p, dec = np.array([0.5, 0.7]), np.zeros(2, np.uint8)
    with FraudEngine(0) as eng:
        for call in (lambda: eng.metrics_query(0.0), lambda: eng.metrics_clear(),
                     lambda: eng.metrics_record(p, dec, None, 1.0, 0.0)):
            with pytest.raises(ValueError):  # FD_ERR_NOT_LOADED before fd_metrics_init
                call()
        for bad in ((9, 16), (2, 0), (2, 65537), (-1, 16)):
            with pytest.raises(NativeError) as e:
                eng.metrics_init(*bad)
            assert e.value.code == FD_ERR_INVALID_ARG
        eng.metrics_init(2, 4)
        eng.metrics_record(p, dec, None, 1.0, 50.0)
        for call in (lambda: eng.metrics_record(p, dec, np.zeros((3, 2)), 1.0, 50.0),   # more models than init said
                     lambda: eng.metrics_record(p, dec, None, 1.0, 49.0),                # the clock ran backwards
                     lambda: eng.metrics_record(p, dec, None, 1.0, float("nan")),
                     lambda: eng.metrics_record_device(0, 0, 2, 50.0),                   # null columns
                     lambda: eng.metrics_record_device(8, 8, 2, 50.0, 0, 2)):            # models without a matrix
            with pytest.raises(NativeError) as e:
                call()
            assert e.value.code == FD_ERR_INVALID_ARG
        eng.metrics_record(p[:0], dec[:0], None, 1.0, 10.0)  # no rows: nothing happens, whatever the stamp
        s = eng.metrics_query(50.0)
        assert (s.total.predictions, s.hour.rows, s.slots_used, s.evictions) == (2, 2, 1, 0)
