"""Drop-in for the reference's MetricsCollector (ml/monitoring/metrics.py), which ml/main.py feeds once per scored
transaction and serves /metrics and /metrics/prometheus from. The numbers live on the engine (csrc/metrics.hip): the
cumulative counters and Prometheus series, and a ring of time slots the "last hour / last minute" figures are reduced
from. record_batch feeds it whole scored batches, from numpy columns or from torch device tensors that never leave the
device; the reference's dicts and the Prometheus text are assembled on the host from one fd_metrics_summary.

Time. Every record call carries one timestamp for its rows: floor(clock() / resolution_s) * resolution_s (resolution_s
= 0 passes clock() through unchanged). A timestamp opens a slot of the ring, later calls with the same stamp merge into
it, so with the default 1 s resolution and 4096 slots an hour of batches fits the ring whatever the batch rate. The
windows are the reference's windows (now - timestamp <= 3600 / <= 60, now = clock() unquantised) over these stamps:
a row counts as recorded up to resolution_s earlier than it was. The clock may not run backwards: the engine rejects
a stamp before the newest recorded one (NativeError, FD_ERR_INVALID_ARG) and records nothing of that call.

What differs from the reference, on purpose:
  * No cap of 10,000 rows. The reference keeps its history in a deque(maxlen=10000), so its "last hour" silently means
    "the last 10,000 predictions"; the engine's windows hold every row of the hour. The ring's own limit is its slot
    count: fd_metrics_summary.evictions (MetricsCollector.evictions()) counts the slots dropped from a full ring.
  * record_prediction(model_predictions=None), the reference's default, raises AttributeError there after the counters
    and the history were already updated; here None is {}.
  * No global registry: a second MetricsCollector in one process is fine (the reference raises DuplicateTimeseries),
    and prometheus_client is not imported. get_prometheus_metrics writes the text exposition format itself, for this
    collector's ml_* families only.
  * Decisions outside the four of enum fd_decision are counted in every total and reported under ONE decision label:
    the first such string this collector was given ("OTHER" when it only ever saw codes).
  * reset_metrics also empties the Prometheus series (they are the same accumulators).
  * Float sums are compensated pairs, not left-to-right sum(); counts and quotients of counts are equal, means agree
    to rounding.
Errors, the error history and the gauges are strings and a handful of floats: they stay on the host.

Model names map to engine model indices 0..7 in first-seen order (the reference's model_performance key order): host
columns are searched for each new name's first row; device columns are not read back, new names there take indices in
column order.

Constructing a collector and reading its (empty) metrics need no GPU; the engine and its collector state are created
at the first call that records, unless an engine is passed in. host_state=True keeps the state in host memory through
the engine library's reference entry points (fd_metrics_*_ref_host: no device; for tools and tests).
"""
from __future__ import annotations

import ctypes as C
import logging
import math
import time
from collections import deque
from dataclasses import dataclass, field
from datetime import datetime
from threading import Lock
from typing import Any, Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _native as N
from .ab_testing import DECISION_CODES, OTHER_DECISION

HELP = {
    "ml_predictions_total": "Total number of predictions made",
    "ml_errors_total": "Total number of errors",
    "ml_fraud_detected_total": "Total number of fraud cases detected",
    "ml_prediction_duration_seconds": "Time spent on predictions",
    "ml_fraud_score_distribution": "Distribution of fraud scores",
    "ml_active_models": "Number of active ML models",
    "ml_model_accuracy": "Model accuracy percentage",
    "ml_avg_processing_time_ms": "Average processing time in milliseconds",
    "ml_system_uptime_seconds": "System uptime in seconds",
    "ml_prediction_throughput_per_second": "Predictions per second",
}
_TYPES = {"ml_predictions_total": "counter", "ml_errors_total": "counter", "ml_fraud_detected_total": "counter",
          "ml_prediction_duration_seconds": "histogram", "ml_fraud_score_distribution": "histogram"}


@dataclass
class PredictionMetric:
    """Individual prediction metric (the reference's record; the engine keeps accumulators, not these)."""
    transaction_id: str
    timestamp: float
    processing_time_ms: float
    fraud_probability: float
    decision: str
    model_predictions: Dict[str, float] = field(default_factory=dict)
    error: Optional[str] = None


# ---------------------------------------------------------------------------------------------- host-only pieces
def _p(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def _columns(fraud_prob, decision, model_probs, processing_time_ms):
    fraud_prob = np.ascontiguousarray(fraud_prob, np.float64)
    n = len(fraud_prob)
    decision = np.ascontiguousarray(decision, np.uint8)
    mp = None if model_probs is None else np.ascontiguousarray(model_probs, np.float64).reshape(-1, n)
    if mp is not None and mp.shape[0] == 0:
        mp = None
    scalar = np.ndim(processing_time_ms) == 0
    times = None if scalar else np.ascontiguousarray(processing_time_ms, np.float64)
    if len(decision) != n or (times is not None and len(times) != n):
        raise ValueError("columns of different lengths")
    return fraud_prob, decision, mp, times, (float(processing_time_ms) if scalar else 0.0), n


class HostState:
    """The collector's state in host memory (fd_metrics_state_bytes), fed and queried by fd_metrics_record_ref_host /
    fd_metrics_query_ref_host: the functions the kernels' lanes use, in the kernels' order of reduction."""

    def __init__(self, n_models: int = N.FD_METRICS_MAX_MODELS, slots: int = 4096):
        self.params = N.fd_metrics_params(int(n_models), int(slots))
        nbytes = N.lib.fd_metrics_state_bytes(int(slots))
        self.buf = np.zeros(max(int(nbytes), 8) // 8 + 1, np.uint64)
        self.clear()

    def clear(self) -> None:
        N.call("fd_metrics_state_init_host", _p(self.buf), C.byref(self.params))

    def record(self, fraud_prob, decision, model_probs, processing_time_ms, timestamp: float) -> None:
        fp, dec, mp, times, scalar, n = _columns(fraud_prob, decision, model_probs, processing_time_ms)
        N.call("fd_metrics_record_ref_host", _p(self.buf), _p(fp), _p(dec), _p(mp), 0 if mp is None else mp.shape[0],
               _p(times), scalar, float(timestamp), n)

    def query(self, now: float) -> N.fd_metrics_summary:
        out = N.fd_metrics_summary()
        N.call("fd_metrics_query_ref_host", _p(self.buf), float(now), C.byref(out))
        return out


def merge_summaries(a: N.fd_metrics_summary, b: N.fd_metrics_summary) -> N.fd_metrics_summary:
    """fd_metrics_summary_merge_host: a then b (one collector per rank, queried at one `now`; a node's is the merge)"""
    out = N.fd_metrics_summary()
    N.call("fd_metrics_summary_merge_host", C.byref(a), C.byref(b), C.byref(out))
    return out


def decision_codes(decisions) -> np.ndarray:
    a = np.asarray(decisions)
    if a.dtype.kind in "iu":
        return np.ascontiguousarray(a, np.uint8)
    return np.fromiter((DECISION_CODES.get(d, OTHER_DECISION) for d in decisions), np.uint8, len(decisions))


def _mean(s: N.fd_metrics_sum, n: int) -> float:
    return (s.hi + s.lo) / n


def _go(x: float) -> str:
    """a float as the Prometheus text format writes it"""
    if math.isinf(x):
        return "+Inf" if x > 0 else "-Inf"
    return "NaN" if math.isnan(x) else repr(float(x))


def _is_device(a) -> bool:
    return hasattr(a, "data_ptr") and bool(getattr(a, "is_cuda", False))


# ---------------------------------------------------------------------------------------------- the collector
class MetricsCollector:
    def __init__(self, engine=None, device: int = 0, slots: int = 4096, clock: Callable[[], float] = time.time,
                 resolution_s: float = 1.0, host_state: bool = False):
        """engine: a FraudEngine to keep the collector on (its collector state is (re)created at the first record;
        an engine holds one). Without one, an engine is created on GPU `device` at the first call that records.
        clock: the time source (seconds); resolution_s: see the module docstring; slots: the ring's size."""
        self.logger = logging.getLogger("metrics_collector")
        self.engine = engine
        self._own = False
        self._device = int(device)
        self._slots = int(slots)
        self._clock = clock
        self.resolution_s = float(resolution_s)
        self._host = bool(host_state)
        self._state = None  # HostState, or True once the engine's collector is initialised
        self.lock = Lock()
        self.start_time = clock()
        self._models: Dict[str, int] = {}  # name -> engine model index, in first-seen order
        self._other_name: Optional[str] = None
        self.error_history: deque = deque(maxlen=1000)
        self.error_count = 0
        self._errors_by_type: Dict[str, int] = {}
        self._active_models = 0.0
        self._model_accuracy: Dict[str, float] = {}
        self._avg_processing_time: Dict[str, float] = {}
        self._uptime_gauge = 0.0
        self._throughput_gauge = 0.0

    def close(self) -> None:
        if self._own and self.engine is not None:
            self.engine.close()
        self.engine, self._state = None, None

    # ------------------------------------------------------------------ state
    def _backend(self):
        if self._state is None:
            if self._host:
                self._state = HostState(N.FD_METRICS_MAX_MODELS, self._slots)
            else:
                if self.engine is None:
                    from .engine import FraudEngine
                    self.engine, self._own = FraudEngine(self._device), True
                self.engine.metrics_init(N.FD_METRICS_MAX_MODELS, self._slots)
                self._state = True
        return self._state

    def summary(self, now: Optional[float] = None) -> N.fd_metrics_summary:
        """The engine's fd_metrics_summary at `now` (default: the clock). Empty, and without touching a device,
        before anything was recorded."""
        if self._state is None:
            return N.fd_metrics_summary()
        now = self._clock() if now is None else now
        return self._state.query(now) if self._host else self.engine.metrics_query(now)

    def evictions(self) -> int:
        return self.summary().evictions

    def stamp(self, t: float) -> float:
        """The timestamp a record call at clock time t hands to the engine"""
        r = self.resolution_s
        return math.floor(t / r) * r if r > 0 else float(t)

    def _indices(self, names: Sequence[str], mp_host: Optional[np.ndarray]) -> List[int]:
        """Engine model indices of a batch's columns; new names are registered in first-seen order"""
        new = [j for j, name in enumerate(names) if name not in self._models]
        if new and mp_host is not None:
            present = ~np.isnan(mp_host[new])
            first = np.where(present.any(axis=1), present.argmax(axis=1), -1)
            new = [j for f, j in sorted(zip(first.tolist(), new)) if f >= 0]  # a column without rows: not seen yet
        for j in new:
            if len(self._models) >= N.FD_METRICS_MAX_MODELS:
                raise ValueError(f"the engine's collector holds at most {N.FD_METRICS_MAX_MODELS} model names")
            self._models[names[j]] = len(self._models)
        return [self._models.get(name, -1) for name in names]

    # ------------------------------------------------------------------ batches
    def record_batch(self, fraud_prob, decision, model_probs=None, model_names: Sequence[str] = (),
                     processing_time_ms=0.0, timestamp: Optional[float] = None) -> None:
        """n scored transactions at once, under one timestamp (default: the clock's, quantised by resolution_s).
        fraud_prob f64 [n]; decision: strings or enum fd_decision codes (uint8) [n]; model_probs: None or f64
        [len(model_names), n], one row per model, NaN where a row has no such model (fd_ab_score_matrix's layout);
        processing_time_ms: [n], or one float for the whole batch. numpy arrays / sequences, or torch device tensors
        (float64 / uint8, contiguous): those go to fd_metrics_record_device and are not copied to the host. A device
        batch must be complete on the engine's stream (or the device idle) when this is called."""
        ts = self.stamp(self._clock() if timestamp is None else timestamp)
        names = list(model_names)
        if model_probs is not None and len(names) != len(model_probs):
            raise ValueError("one model name per row of model_probs")
        if model_probs is None or not names:
            model_probs, names = None, []
        with self.lock:
            if _is_device(fraud_prob):
                self._record_device(fraud_prob, decision, model_probs, names, processing_time_ms, ts)
                return
            if not isinstance(decision, np.ndarray) or decision.dtype.kind not in "iu":
                for d in decision:
                    if isinstance(d, str) and d not in DECISION_CODES and self._other_name is None:
                        self._other_name = d
            fp, dec, mp, times, scalar, n = _columns(fraud_prob, decision_codes(decision), model_probs,
                                                     processing_time_ms)
            if n == 0:
                return
            if mp is not None:
                idx = self._indices(names, mp)
                k = max(idx) + 1
                if idx != list(range(len(idx))) or k != len(idx):
                    full = np.full((max(k, 0), n), np.nan)
                    for j, i in enumerate(idx):
                        if i >= 0:
                            full[i] = mp[j]
                    mp = full if k > 0 else None
            state = self._backend()
            record = state.record if self._host else self.engine.metrics_record
            record(fp, dec, mp, scalar if times is None else times, ts)

    def _record_device(self, fraud_prob, decision, model_probs, names, processing_time_ms, ts) -> None:
        import torch
        n = int(fraud_prob.numel())
        if n == 0:
            return
        if self._host:
            raise ValueError("a host_state collector takes host columns")
        for t, dt in ((fraud_prob, torch.float64), (decision, torch.uint8), (model_probs, torch.float64)):
            if t is not None and (not _is_device(t) or t.dtype != dt or not t.is_contiguous()):
                raise ValueError("device columns must be contiguous device tensors: float64 probabilities, uint8 decisions")
        mp_ptr, k = 0, 0
        if model_probs is not None:
            idx = self._indices(names, None)
            k = max(idx) + 1
            if idx != list(range(len(idx))) or k != len(idx):
                full = torch.full((k, n), float("nan"), dtype=torch.float64, device=model_probs.device)
                full[torch.tensor(idx, device=model_probs.device)] = model_probs.reshape(len(idx), n)
                torch.cuda.current_stream().synchronize()
                model_probs = full
            mp_ptr = model_probs.data_ptr()
        scalar = not _is_device(processing_time_ms)
        if not scalar and (processing_time_ms.dtype != torch.float64 or not processing_time_ms.is_contiguous()):
            raise ValueError("a device time column must be contiguous float64")
        self._backend()
        self.engine.metrics_record_device(fraud_prob.data_ptr(), decision.data_ptr(), n, ts, mp_ptr, k,
                                          0 if scalar else processing_time_ms.data_ptr(),
                                          float(processing_time_ms) if scalar else 0.0)
        if model_probs is not None:
            self._keep = model_probs  # (a rearranged copy must outlive the kernel; the next call replaces it)

    # ------------------------------------------------------------------ the reference's surface
    async def record_prediction(self, transaction_id: str, processing_time_ms: float, fraud_probability: float,
                                decision: str, model_predictions: Dict[str, float] = None):
        """Record a prediction metric (one row; a batch caller uses record_batch)."""
        preds = model_predictions or {}
        names = list(preds)
        mp = np.array([[float(preds[k])] for k in names], np.float64) if names else None
        self.record_batch([float(fraud_probability)], [decision], mp, names, [float(processing_time_ms)])

    async def record_error(self, error_message: str, error_type: str = "unknown"):
        with self.lock:
            self.error_history.append({"timestamp": self._clock(), "error_message": error_message,
                                       "error_type": error_type})
            self.error_count += 1
            self._errors_by_type[error_type] = self._errors_by_type.get(error_type, 0) + 1

    async def update_model_metrics(self, model_name: str, is_active: bool = True, accuracy: float = None):
        if is_active:
            self._active_models += 1
        if accuracy is not None:
            self._model_accuracy[model_name] = accuracy * 100
        idx = self._models.get(model_name)
        if idx is not None:
            ser = self.summary().total.series[1 + idx]
            if ser.rows > 0:
                self._avg_processing_time[model_name] = _mean(ser.time_ms, ser.rows)

    def update_system_metrics(self, summary: Optional[N.fd_metrics_summary] = None):
        now = self._clock()
        self._uptime_gauge = now - self.start_time
        s = self.summary(now) if summary is None else summary
        self._throughput_gauge = s.minute.rows / 60.0

    async def get_metrics(self) -> Dict[str, Any]:
        return self.metrics_dict()

    def metrics_dict(self, now: Optional[float] = None) -> Dict[str, Any]:
        """get_metrics' dict at clock time `now`"""
        now = self._clock() if now is None else now
        s = self.summary(now)
        t, hour, minute = s.total, s.hour, s.minute
        models = {}
        for name, idx in self._models.items():
            ser = t.series[1 + idx]
            if ser.rows > 0:
                models[name] = {"total_predictions": ser.rows,
                                "avg_processing_time_ms": _mean(ser.time_ms, ser.rows),
                                "error_rate": 0 / ser.rows,  # the reference never increments a model's errors
                                "last_prediction": datetime.fromtimestamp(ser.last_timestamp).isoformat()}
        return {
            "system": {"uptime_seconds": now - self.start_time, "total_predictions": t.predictions,
                       "total_errors": self.error_count, "fraud_detections": t.fraud_detections,
                       "declined_transactions": t.declined,
                       "error_rate": self.error_count / max(t.predictions, 1)},
            "performance": {"avg_processing_time_ms": _mean(hour.time_ms, hour.rows) if hour.rows else 0.0,
                            "predictions_per_second": minute.rows / 60.0,
                            "predictions_last_hour": hour.rows, "predictions_last_minute": minute.rows},
            "fraud_detection": {"fraud_rate": hour.fraud / max(hour.rows, 1),
                                "fraud_detections_last_hour": hour.fraud,
                                "high_risk_transactions": hour.high_risk},
            "models": models,
            "timestamp": datetime.now().isoformat(),
        }

    def last_predictions(self, summary: Optional[N.fd_metrics_summary] = None) -> Dict[str, float]:
        """model name -> the raw timestamp get_metrics renders as models[..]["last_prediction"]"""
        s = self.summary() if summary is None else summary
        return {name: s.total.series[1 + idx].last_timestamp for name, idx in self._models.items()
                if s.total.series[1 + idx].rows > 0}

    def get_prometheus_metrics(self) -> bytes:
        s = self.summary()
        self.update_system_metrics(s)
        return self.exposition(s).encode("utf-8")

    def get_uptime(self) -> float:
        return self._clock() - self.start_time

    def _get_risk_level(self, fraud_probability: float) -> str:
        if fraud_probability >= 0.95:
            return "CRITICAL"
        elif fraud_probability >= 0.8:
            return "HIGH"
        elif fraud_probability >= 0.6:
            return "MEDIUM"
        elif fraud_probability >= 0.3:
            return "LOW"
        return "VERY_LOW"

    async def get_model_performance_report(self) -> Dict[str, Any]:
        return self.model_performance_report()

    def model_performance_report(self, now: Optional[float] = None) -> Dict[str, Any]:
        s = self.summary(now)
        reports = {}
        for name, idx in self._models.items():
            m = s.hour.model[idx]
            if m.rows > 0:
                reports[name] = {"total_predictions": m.rows,
                                 "avg_processing_time_ms": _mean(m.time_ms, m.rows),
                                 "min_processing_time_ms": m.min_time_ms, "max_processing_time_ms": m.max_time_ms,
                                 "avg_prediction_score": _mean(m.prediction, m.rows),
                                 "prediction_distribution": {"low_risk": m.dist[0], "medium_risk": m.dist[1],
                                                             "high_risk": m.dist[2]}}
        return {"report_timestamp": datetime.now().isoformat(), "time_window": "1 hour",
                "total_predictions": s.hour.rows, "models": reports}

    async def get_error_summary(self) -> Dict[str, Any]:
        now = self._clock()
        with self.lock:
            recent = [e for e in self.error_history if now - e["timestamp"] <= 3600]
            types: Dict[str, int] = {}
            for e in recent:
                types[e["error_type"]] = types.get(e["error_type"], 0) + 1
            last = list(self.error_history)[-10:]
        predictions = self.summary(now).total.predictions
        return {"total_errors_last_hour": len(recent), "error_rate": len(recent) / max(predictions, 1),
                "error_types": types,
                "recent_errors": [{"timestamp": datetime.fromtimestamp(e["timestamp"]).isoformat(),
                                   "error_type": e["error_type"], "message": e["error_message"][:100]} for e in last]}

    def reset_metrics(self):
        with self.lock:
            if self._state is not None:
                if self._host:
                    self._state.clear()
                else:
                    self.engine.metrics_clear()
            self.error_history.clear()
            self._models.clear()
            self._errors_by_type.clear()
            self.error_count = 0
            self.start_time = self._clock()

    # ------------------------------------------------------------------ Prometheus
    def prometheus_samples(self, summary: Optional[N.fd_metrics_summary] = None) -> Dict[Tuple, float]:
        """{(sample name, sorted label items): value} of this collector's ml_* families, as prometheus_client's
        registry would list them (without the _created samples)."""
        return {(name, tuple(sorted(labels.items()))): value
                for _, rows in self._families(self.summary() if summary is None else summary)
                for name, labels, value in rows}

    def _families(self, s: N.fd_metrics_summary):
        t = s.total
        labels = [("ensemble", t.series[0])] + [(name, t.series[1 + idx]) for name, idx in self._models.items()]
        labels = [(name, ser) for name, ser in labels if ser.rows > 0]
        other = self._other_name or "OTHER"
        fam = []
        rows = []
        for name, ser in labels:
            for d, code in DECISION_CODES.items():
                if ser.decisions[code]:
                    rows.append(("ml_predictions_total", {"model_name": name, "decision": d},
                                 float(ser.decisions[code])))
            rest = ser.rows - sum(ser.decisions)
            if rest:
                rows.append(("ml_predictions_total", {"model_name": name, "decision": other}, float(rest)))
        fam.append(("ml_predictions_total", rows))
        fam.append(("ml_errors_total", [("ml_errors_total", {"error_type": k}, float(v))
                                        for k, v in self._errors_by_type.items()]))
        fam.append(("ml_fraud_detected_total", [("ml_fraud_detected_total", {"risk_level": N.RISK_LEVELS[r]},
                                                 float(t.risk_detected[r]))
                                                for r in range(N.FD_METRICS_RISK_LEVELS) if t.risk_detected[r]]))

        def histogram(name, extra, hist, bounds, total, count):
            out, acc = [], 0
            for b, le in zip(hist, list(bounds) + [math.inf]):
                acc += b
                out.append((name + "_bucket", {**extra, "le": _go(le)}, float(acc)))
            out.append((name + "_count", dict(extra), float(count)))
            out.append((name + "_sum", dict(extra), total))
            return out
        rows = []
        for name, ser in labels:
            rows += histogram("ml_prediction_duration_seconds", {"model_name": name}, ser.time_hist,
                              N.METRICS_TIME_BOUNDS, ser.seconds.value, ser.rows)
        fam.append(("ml_prediction_duration_seconds", rows))
        fam.append(("ml_fraud_score_distribution", histogram("ml_fraud_score_distribution", {}, t.score_hist,
                                                             N.METRICS_SCORE_BOUNDS, t.score_sum.value,
                                                             t.predictions)))
        fam.append(("ml_active_models", [("ml_active_models", {}, float(self._active_models))]))
        fam.append(("ml_model_accuracy", [("ml_model_accuracy", {"model_name": k}, float(v))
                                          for k, v in self._model_accuracy.items()]))
        fam.append(("ml_avg_processing_time_ms", [("ml_avg_processing_time_ms", {"model_name": k}, float(v))
                                                  for k, v in self._avg_processing_time.items()]))
        fam.append(("ml_system_uptime_seconds", [("ml_system_uptime_seconds", {}, float(self._uptime_gauge))]))
        fam.append(("ml_prediction_throughput_per_second", [("ml_prediction_throughput_per_second", {},
                                                             float(self._throughput_gauge))]))
        return fam

    def exposition(self, summary: Optional[N.fd_metrics_summary] = None) -> str:
        """The text exposition format (version 0.0.4) of the families above"""
        esc = lambda v: str(v).replace("\\", "\\\\").replace("\n", "\\n").replace('"', '\\"')  # noqa: E731
        lines = []
        for family, rows in self._families(self.summary() if summary is None else summary):
            lines.append(f"# HELP {family} {HELP[family]}")
            lines.append(f"# TYPE {family} {_TYPES.get(family, 'gauge')}")
            for name, labels, value in rows:
                lab = ",".join(f'{k}="{esc(v)}"' for k, v in labels.items())
                lines.append(f"{name}{{{lab}}} {_go(value)}" if lab else f"{name} {_go(value)}")
        return "\n".join(lines) + "\n"
