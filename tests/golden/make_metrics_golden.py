#!/usr/bin/env python3
"""Generate tests/golden/metrics_cases.npz by running the REFERENCE's own MetricsCollector
(services/ml-models/src/monitoring/metrics.py) in the build container. Only the rows' columns, the script of calls and
query instants, and what the reference returned travel; the reference never does. Never runs on the GPU machine; needs
prometheus_client, no engine library and no GPU.

Run:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_metrics_golden.py

Reference code exercised (unchanged): record_prediction (row by row), update_system_metrics, get_metrics,
get_model_performance_report, and the prometheus_client registry it fills. Its clock (monitoring.metrics.time) is
replaced by a scripted one before the collector is constructed; the collectors it registered in prometheus_client's
global registry are unregistered between streams. utils.logging_config is used as it is when it imports, else
registered as a module whose get_logger returns a standard logger.

Streams: tests/metrics_cases.py SPECS. What each is there for is asserted below on the reference's outputs."""
import asyncio
import importlib.machinery
import json
import logging
import sys
import types
from pathlib import Path

import numpy as np

sys.dont_write_bytecode = True
HERE = Path(__file__).resolve().parent
REF_SRC = Path("/root/reference/services/ml-models/src")
sys.path.insert(0, str(HERE.parent))

import metrics_cases as T  # noqa: E402


class Clock:
    now = 0.0

    def time(self):
        return self.now


def reference_module():
    sys.path.insert(0, str(REF_SRC))
    try:
        import utils.logging_config  # noqa: F401
    except Exception:
        for name in ("utils", "utils.logging_config"):
            m = types.ModuleType(name)
            m.__spec__ = importlib.machinery.ModuleSpec(name, None)
            sys.modules[name] = m
        sys.modules["utils"].__path__ = []
        sys.modules["utils.logging_config"].get_logger = logging.getLogger
    import monitoring.metrics as R
    return R


def strip(d):
    return {k: (strip(v) if isinstance(v, dict) else v) for k, v in d.items() if k not in T.EXCLUDED}


def registry_samples():
    from prometheus_client import REGISTRY
    out = []
    for fam in REGISTRY.collect():
        for s in fam.samples:
            if s.name.startswith("ml_") and not s.name.endswith("_created") and s.name != "ml_system_uptime_seconds":
                out.append([s.name, dict(s.labels), float(s.value)])
    return out


def unregister_all():
    from prometheus_client import REGISTRY
    for c in list(REGISTRY._collector_to_names):
        REGISTRY.unregister(c)


async def run_reference(R, clock, case, names, script):
    clock.now = 0.0
    col = R.MetricsCollector()
    results, a = [], 0
    dec = T.decision_names(case["decision"])
    for op in script:
        clock.now = op[2] if op[0] == "rec" else op[1]
        if op[0] == "rec":
            for i in range(a, a + op[1]):
                preds = {names[m]: float(case["mp"][m, i]) for m in range(len(names)) if not np.isnan(case["mp"][m, i])}
                await col.record_prediction(f"txn_{i}", float(case["time_ms"][i]), float(case["p"][i]), dec[i], preds)
            a += op[1]
        else:
            m = await col.get_metrics()
            r = await col.get_model_performance_report()
            results.append({"now": op[1], "metrics": strip(m), "report": strip(r),
                            "last_prediction": {k: v["last_prediction"] for k, v in col.model_performance.items()}})
    assert len(col.prediction_history) == a <= 10000  # the deque's cap never dropped a row
    col.update_system_metrics()
    return results, registry_samples()


def main():
    R = reference_module()
    clock = Clock()
    R.time = clock  # monitoring.metrics.time.time is the scripted clock from here on
    arrays, meta = {}, []
    sizes = set()
    for i, spec in enumerate(T.SPECS):
        name, M, values, script = spec
        assert T.total_rows(spec) <= 10000, name
        sizes |= {op[1] for op in script if op[0] == "rec"}
        case = T.draw_stream(i, spec)
        names = list(T.MODEL_NAMES[:M])
        unregister_all()
        results, samples = asyncio.run(run_reference(R, clock, case, names, script))
        for col in ("p", "decision", "mp", "time_ms"):
            arrays[f"{i}_{col}"] = case[col]
        meta.append({"name": name, "model_names": names, "script": [list(op) for op in script], "results": results,
                     "samples": samples})
        print(name, "rows", T.total_rows(spec), "queries", len(results), "samples", len(samples))
    by = {m["name"]: m for m in meta}
    assert sizes == set(T.CALL_SIZES), sizes
    # what the streams are there for, on the reference's own outputs
    e = by["edges_two_models"]["results"]
    n_edges = T.total_rows(T.SPECS[0])
    assert e[0]["metrics"]["performance"] == {**e[0]["metrics"]["performance"], "predictions_last_hour": n_edges,
                                              "predictions_last_minute": 66}
    assert e[1]["metrics"]["performance"]["predictions_last_hour"] == n_edges - 320  # the 1000.0 slot left the hour
    assert e[1]["metrics"]["performance"]["predictions_last_minute"] == 1       # ... and 4540.0 the minute
    assert e[2]["metrics"]["performance"]["predictions_last_hour"] == 0
    assert e[2]["metrics"]["system"]["total_predictions"] == n_edges and e[2]["report"]["models"] == {}
    s = {T.sample_key(n, l): v for n, l, v in by["edges_two_models"]["samples"]}
    p = T.draw_stream(0, T.SPECS[0])
    for b, le in zip(T.SCORE_BOUNDS, ("0.0", "0.1", "0.2", "0.3", "0.4", "0.5", "0.6", "0.7", "0.8", "0.9", "1.0")):
        # a value at a bound and the one below it are in the bound's bucket, the one above it is not
        assert s[("ml_fraud_score_distribution_bucket", (("le", le),))] == float((p["p"] <= b).sum())
        assert (p["p"] == b).any() and (p["p"] == T.up(b)).any() and (p["p"] == T.down(b)).any()
    for ms, le in zip(T.TIME_BOUND_MS, ("0.001", "0.005", "0.01", "0.025", "0.05", "0.1", "0.25", "0.5", "1.0", "2.5",
                                        "5.0")):
        assert ms / 1000.0 == float(le) and (p["time_ms"] == ms).any()
        assert s[("ml_prediction_duration_seconds_bucket", (("le", le), ("model_name", "ensemble")))] == \
            float((p["time_ms"] / 1000.0 <= float(le)).sum())
    assert ("ml_predictions_total", (("decision", T.OTHER_NAME), ("model_name", "ensemble"))) in s
    assert s[("ml_fraud_detected_total", (("risk_level", "LOW"),))] == float(((p["p"] > 0.5) & (p["p"] < 0.6)).sum()) > 0
    assert by["no_models"]["results"][0]["metrics"]["models"] == {}
    m8 = by["eight_models"]["results"]
    order = list(m8[0]["metrics"]["models"])
    assert len(order) == 7 and order.index("random_forest") < order.index("lstm_sequential")  # not column order
    assert list(m8[1]["metrics"]["models"])[-1] == "late_challenger" and len(m8[1]["metrics"]["models"]) == 8
    assert m8[1]["metrics"]["performance"]["predictions_last_minute"] == 320  # 100.5 exactly 60.0 back; 100.0 is out
    assert m8[2]["metrics"]["performance"]["predictions_last_minute"] == 63
    assert [r["report"]["total_predictions"] for r in m8[3:]] == [1345, 320, 320, 63, 0]
    big = by["big_two_models"]["results"]
    assert [r["metrics"]["performance"]["predictions_last_minute"] for r in big] == [1282, 1282, 257, 0, 0, 0]
    assert [r["metrics"]["performance"]["predictions_last_hour"] for r in big] == [7307, 7307, 7307, 7307, 1282, 0]
    arrays["meta"] = np.array(json.dumps(meta))
    np.savez_compressed(T.GOLDEN, **arrays)
    print("wrote", T.GOLDEN, T.GOLDEN.stat().st_size, "bytes")
    assert T.GOLDEN.stat().st_size <= 1024 * 1024


if __name__ == "__main__":
    main()
