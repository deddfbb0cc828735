"""Prediction-metrics cases shared by tests/golden/make_metrics_golden.py (which runs the reference's MetricsCollector
on them), tests/test_metrics_host.py and tests/test_gpu_metrics.py: how the streams are drawn, how the fixture is read,
how a stream is replayed into a collector, and the comparison with the reference's outputs. Nothing here touches the
GPU.

A stream is a script of record calls (rows, timestamp, a time column or one scalar time) and query instants over the
columns fraud probability, decision code (enum fd_decision; OTHER for a string outside the four), per-model
predictions (NaN: the row has no such model) and processing time. The reference was fed row by row with its clock
scripted to each call's timestamp; at each query instant its get_metrics and get_model_performance_report dicts were
recorded (without uptime_seconds, timestamp, report_timestamp and the ISO rendering of last_prediction, which depend on
wall clock and timezone; the raw last_prediction floats are recorded instead), and at the end its ml_* Prometheus
samples (without _created and the uptime gauge).

Tolerances:
  equal   every count, every Prometheus counter / bucket / _count, every quotient of counts, min / max / last_prediction
  means   |got - ref| <= 2 n 2^-53 max|x|: the reference's left-to-right sum() of n values errs by at most
          (n - 1) 2^-53 sum|x| <= (n - 1) 2^-53 n max|x| before its one division by n; the engine's compensated sum is
          within an ulp of exact
  _sum    |got - ref| <= 2 n 2^-53 sum|x|, the same bound before the division
"""
import json
from pathlib import Path

import numpy as np

GOLDEN = Path(__file__).resolve().parent / "golden" / "metrics_cases.npz"
DECISIONS = ("APPROVE", "REVIEW", "DECLINE", "APPROVE_WITH_MONITORING")  # enum fd_decision
OTHER = 254
OTHER_NAME = "HOLD"
MODEL_NAMES = ("xgboost_primary", "isolation_forest", "lstm_sequential", "random_forest", "mlp_head",
               "graph_detector", "text_analyzer", "late_challenger")
CALL_SIZES = (1, 63, 64, 65, 257, 1025, 5000)
CUTS = (1, 64, 1000)
EXCLUDED = {"uptime_seconds", "timestamp", "report_timestamp", "last_prediction"}
U = 2.0 ** -53

up = lambda x: float(np.nextafter(x, np.inf))  # noqa: E731
down = lambda x: float(np.nextafter(x, -np.inf))  # noqa: E731


def around(values):
    return [f(v) for v in values for f in (down, float, up)]


SCORE_BOUNDS = (0.0, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9, 1.0)
SCORE_EDGES = around(SCORE_BOUNDS + (0.95,))       # includes 0.3, 0.5, 0.6, 0.7, 0.8 and their neighbours
MODEL_EDGES = around((0.3, 0.7))
TIME_BOUND_MS = (1.0, 5.0, 10.0, 25.0, 50.0, 100.0, 250.0, 500.0, 1000.0, 2500.0, 5000.0)
TIME_EDGES = around(TIME_BOUND_MS)

# name, models, values ("edges" / "random"), script: ("rec", rows, timestamp, None for a time column or the scalar
# time) and ("query", now)
SPECS = (
    ("edges_two_models", 2, "edges", (
        ("rec", 257, 1000.0, None), ("rec", 63, 1000.0, 25.0),  # two calls, one stamp: one slot
        ("rec", 64, 3540.0, None), ("rec", 65, 4540.0, None), ("rec", 1, 4600.0, 5000.0),
        ("query", 4600.0),        # 1000.0 is exactly 3600.0 back, 4540.0 exactly 60.0: both included
        ("query", up(4600.0)),    # one ulp later: both excluded
        ("query", 1.0e9))),       # long after: empty windows, cumulative intact
    ("no_models", 0, "random", (
        ("rec", 64, 10.0, 12.5), ("rec", 1, 10.0, None), ("query", 10.0), ("query", 70.0), ("query", up(70.0)))),
    ("one_model", 1, "random", (("rec", 65, 50.0, None), ("query", 50.0), ("query", 3650.0), ("query", up(3650.0)))),
    ("eight_models", 8, "random", (
        ("rec", 1025, 100.0, None), ("query", 100.0),
        ("rec", 257, 100.5, None),   # the late model's first rows
        ("rec", 63, 130.25, 0.75), ("query", 160.5), ("query", up(160.5)),
        ("query", 3700.0), ("query", up(3700.0)), ("query", 3700.5), ("query", up(3700.5)), ("query", 1.0e7))),
    ("big_two_models", 2, "random", (
        ("rec", 5000, 7200.0, None), ("rec", 1025, 7200.0, None), ("rec", 1025, 7230.0, 3.25),
        ("rec", 257, 7261.0, None), ("query", 7261.0), ("query", 7290.0), ("query", up(7290.0)),
        ("query", 10800.0), ("query", up(10800.0)), ("query", 1.0e7))),
)


def total_rows(spec):
    return sum(op[1] for op in spec[3] if op[0] == "rec")


def draw_stream(idx, spec):
    """The columns of a stream: p [N], decision u8 [N], model_probs [M, N] (NaN: absent), time_ms [N]"""
    name, M, values, script = spec
    N = total_rows(spec)
    rng = np.random.default_rng(4000 + idx)
    if values == "edges":
        p = rng.permutation(np.resize(np.array(SCORE_EDGES), N))
        time_ms = rng.permutation(np.resize(np.array(TIME_EDGES), N))
        decision = np.resize(np.array([0, 1, 2, 3, OTHER], np.uint8), N)
    else:
        p = np.minimum(1.0, rng.random(N) * 1.04)
        time_ms = 0.2 + rng.random(N) * rng.choice([1.0, 10.0, 100.0, 1000.0, 6000.0], N)
        decision = np.where(p > 0.8, 2, np.where(p > 0.55, 1, np.where(p > 0.35, 3, 0))).astype(np.uint8)
        decision[rng.choice(N, max(1, N // 97), replace=False)] = OTHER
    mp = np.clip(p[None, :] + 0.2 * (rng.random((M, N)) - 0.5), 0.0, 1.0)
    if M:
        mp[0] = rng.permutation(np.resize(np.array(MODEL_EDGES), N)) if values == "edges" else mp[0]
        if values == "edges":
            mp[1, rng.random(N) < 0.3] = np.nan
    if M == 8:
        mp[rng.random((M, N)) < 0.25] = np.nan  # rows with differing model sets
        mp[0] = np.where(np.isnan(mp[0]), 0.5, mp[0])  # (every row keeps a model)
        mp[2, :10] = np.nan   # seen after the models of the higher columns: the dicts' key order is not column order
        mp[3, 0] = 0.25
        mp[7, :1025] = np.nan  # first appears in the second call
    a = 0
    for op in script:  # a scalar-time call's rows all carry that time
        if op[0] == "rec":
            if op[3] is not None:
                time_ms[a:a + op[1]] = op[3]
            a += op[1]
    return {"p": p, "decision": decision, "mp": np.ascontiguousarray(mp), "time_ms": time_ms}


def load():
    """-> list of cases: {"name", "model_names", "script", "results" (the reference's, one per query), "samples",
    and the columns p, decision, mp, time_ms}"""
    z = np.load(GOLDEN)
    meta = json.loads(str(z["meta"]))
    cases = []
    for i, m in enumerate(meta):
        c = dict(m)
        for col in ("p", "decision", "mp", "time_ms"):
            c[col] = z[f"{i}_{col}"]
        c["script"] = [tuple(op) for op in c["script"]]
        cases.append(c)
    return cases


def pieces(a, b, cut):
    return [(x, min(b, x + cut)) for x in range(a, b, cut)]


def steps(case, cut=None):
    """The script with row ranges: ("rec", a, b, timestamp, time argument) with the call re-cut into pieces of `cut`
    rows within its timestamp, and ("query", now, the reference's result)"""
    a, q = 0, 0
    for op in case["script"]:
        if op[0] == "rec":
            _, rows, ts, scalar = op
            for x, y in pieces(a, a + rows, cut or rows):
                yield ("rec", x, y, ts, case["time_ms"][x:y] if scalar is None else scalar)
            a += rows
        else:
            yield ("query", op[1], case["results"][q])
            q += 1


def decision_names(codes):
    return [DECISIONS[d] if d < 4 else OTHER_NAME for d in codes]


def replay(collector, clock, case, cut=None, check=None, as_strings=True):
    """The stream into a fdengine.monitoring.MetricsCollector whose clock reads clock[0]; check(now, want, rows so far,
    stamps of the recorded rows) at every query."""
    names = case["model_names"]
    rows, stamps = 0, np.zeros(len(case["p"]))
    for st in steps(case, cut):
        if st[0] == "rec":
            _, a, b, ts, t = st
            clock[0] = ts
            dec = decision_names(case["decision"][a:b]) if as_strings else case["decision"][a:b]
            collector.record_batch(case["p"][a:b], dec, case["mp"][:, a:b] if names else None, names, t)
            stamps[a:b] = ts
            rows = b
        else:
            clock[0] = st[1]
            if check is not None:
                check(st[1], st[2], rows, stamps)


# ------------------------------------------------------------------------------------------------- comparisons
def _strip(d):
    return {k: (_strip(v) if isinstance(v, dict) else v) for k, v in d.items() if k not in EXCLUDED}


def _close(got, want, n, scale, what, ratios, key):
    tol = 2 * n * U * scale
    err = abs(got - want)
    if ratios is not None and tol > 0:
        ratios[key] = max(ratios.get(key, 0.0), err / tol)
    assert err <= tol, (what, got, want, err, tol)


def check_metrics(got, want, case, now, rows, stamps, ratios=None):
    """get_metrics' dict against the reference's at a query instant (rows: recorded so far)"""
    got = _strip(got)
    what = (case["name"], now)
    assert list(got) == list(want) and all(list(got[k]) == list(want[k]) for k in want), (what, got, want)
    assert got["system"] == want["system"], (what, got["system"], want["system"])
    assert got["fraud_detection"] == want["fraud_detection"], (what, got["fraud_detection"], want["fraud_detection"])
    hour = now - stamps[:rows] <= 3600
    t = case["time_ms"][:rows]
    for k, v in want["performance"].items():
        if k == "avg_processing_time_ms" and hour.any():
            _close(got["performance"][k], v, int(hour.sum()), float(np.abs(t[hour]).max()), what + (k,), ratios,
                   "performance.avg_processing_time_ms")
        else:
            assert got["performance"][k] == v, (what, k, got["performance"][k], v)
    for name, w in want["models"].items():
        g = got["models"][name]
        assert list(g) == list(w), (what, name)
        has = ~np.isnan(case["mp"][case["model_names"].index(name), :rows])
        for k, v in w.items():
            if k == "avg_processing_time_ms":
                _close(g[k], v, int(has.sum()), float(np.abs(t[has]).max()), what + (name, k), ratios,
                       "models.avg_processing_time_ms")
            else:
                assert g[k] == v and type(g[k]) is type(v), (what, name, k, g[k], v)


def check_report(got, want, case, now, rows, stamps, ratios=None):
    """get_model_performance_report's dict against the reference's"""
    got = _strip(got)
    what = (case["name"], now, "report")
    assert list(got) == list(want) and list(got["models"]) == list(want["models"]), (what, got, want)
    assert got["time_window"] == want["time_window"] and got["total_predictions"] == want["total_predictions"], what
    hour = now - stamps[:rows] <= 3600
    for name, w in want["models"].items():
        g = got["models"][name]
        assert list(g) == list(w), (what, name)
        q = case["mp"][case["model_names"].index(name), :rows]
        has = hour & ~np.isnan(q)
        for k, v in w.items():
            if k in ("avg_processing_time_ms", "avg_prediction_score"):
                x = case["time_ms"][:rows][has] if k == "avg_processing_time_ms" else q[has]
                _close(g[k], v, int(has.sum()), float(np.abs(x).max()), what + (name, k), ratios, "report." + k)
            else:
                assert g[k] == v, (what, name, k, g[k], v)


def sample_key(name, labels):
    return (name, tuple(sorted(labels.items())))


def check_samples(got, case, ratios=None):
    """{(sample name, label items): value} against the reference's final ml_* samples"""
    want = {sample_key(n, l): v for n, l, v in case["samples"]}
    got = {k: v for k, v in got.items() if k[0] != "ml_system_uptime_seconds"}
    assert sorted(got) == sorted(want), (case["name"], sorted(set(got) ^ set(want)))
    sec = case["time_ms"] / 1000.0
    for k, v in want.items():
        name, labels = k[0], dict(k[1])
        if name.endswith("_sum"):
            if name.startswith("ml_fraud_score"):
                x = case["p"]
            elif labels["model_name"] == "ensemble":
                x = sec
            else:
                x = sec[~np.isnan(case["mp"][case["model_names"].index(labels["model_name"])])]
            _close(got[k], v, len(x), float(np.abs(x).sum()), (case["name"],) + k, ratios, name)
        else:
            assert got[k] == v, (case["name"], k, got[k], v)
