"""Drop-in for the reference's ABTestManager (ml/testing/ab_testing.py): users are assigned to CONTROL or TREATMENT
by a stable hash and the test's traffic split, one result per transaction is recorded, and get_test_summary reduces
them per variant. The results live on the engine (csrc/abtest.hip) as two accumulators per test, not as a list of
objects; the summary is assembled on the host from those numbers.

What differs from the reference, on purpose:
  * The assignment hash. The reference takes Python's hash() of "<test>_<user>", which is salted per process: its
    own assignments change from run to run. Here bucket = fmix64(fd_hash64(user_id) ^ fd_hash64(test_name)) % 100,
    the same in every process and on the device. The comparison is the reference's: treatment when
    bucket < traffic_split * 100, against the f64 product (0.07 gives 8 treatment buckets, not 7).
  * Assignments are not cached: they are a function of (test name, user id, traffic split). A test created again
    under an old name with another split assigns by the new split.
  * Float sums. The reference adds prediction and processing_time_ms left to right (sum()) in the metrics and
    pairwise (numpy) in the statistical analysis, so it differs from itself in the last digits; the engine keeps
    compensated sums. Counts and every quotient of counts are equal; means, stds and what derives from them agree to
    rounding.
  * Rows are kept on the host (for export_results) only with keep_results=True.
  * An engine holds at most FD_AB_MAX_TESTS tests; create_test returns False when the manager, or the engine it was
    given, has no id left.

Batch entry points beyond the reference's surface: assign_batch, record_batch, score_batch.
"""
from __future__ import annotations

import ctypes as C
import logging
import time
from dataclasses import dataclass
from enum import Enum
from typing import Any, Dict, List, Optional

import numpy as np

from . import _native as N
from .ingest import hash64

DECISION_CODES = {name: code for code, name in enumerate(N.DECISIONS)}  # enum fd_decision
OTHER_DECISION = 254  # any other decision string: counted in total_samples only
_RATE_ORDER = ("APPROVE", "APPROVE_WITH_MONITORING", "REVIEW", "DECLINE")  # the metrics dict's key order
_INSUFFICIENT = {"error": "Insufficient data for statistical test"}


class TestVariant(Enum):
    __test__ = False  # (not a pytest class)
    CONTROL = "control"
    TREATMENT = "treatment"


@dataclass
class ABTestConfig:
    test_name: str
    control_model: str
    treatment_model: str
    traffic_split: float  # share of traffic for the treatment, 0.0-1.0
    start_time: str
    end_time: str
    success_metric: str = "fraud_detection_rate"
    minimum_sample_size: int = 1000
    significance_level: float = 0.05


@dataclass
class TestResult:
    __test__ = False
    transaction_id: str
    variant: TestVariant
    model_used: str
    prediction: float
    decision: str
    actual_fraud: Optional[bool]
    processing_time_ms: float
    timestamp: float


# ---------------------------------------------------------------------------------------------- host-only pieces
def salt_of(test_name: str) -> int:
    return hash64(test_name)


def threshold_of(traffic_split: float) -> float:
    """The f64 the buckets are compared against: the product as the reference forms it."""
    return traffic_split * 100


def buckets_of(keys, salt: int) -> np.ndarray:
    """uint64 keys -> uint8 buckets 0..99 (fd_ab_bucket_host: no engine, no device)"""
    keys = np.ascontiguousarray(keys, np.uint64)
    out = np.empty(len(keys), np.uint8)
    N.call("fd_ab_bucket_host", C.c_void_p(keys.ctypes.data), len(keys), C.c_uint64(int(salt)),
           C.c_void_p(out.ctypes.data))
    return out


def variants_of(keys, test_name: str, traffic_split: float) -> np.ndarray:
    """uint8 [n]: 1 where the key's bucket is below traffic_split * 100"""
    return (buckets_of(keys, salt_of(test_name)).astype(np.float64) < threshold_of(traffic_split)).astype(np.uint8)


def decision_codes(decisions) -> np.ndarray:
    a = np.asarray(decisions)
    if a.dtype.kind in "iu":
        return np.ascontiguousarray(a, np.uint8)
    return np.fromiter((DECISION_CODES.get(d, OTHER_DECISION) for d in decisions), np.uint8, len(decisions))


def label_codes(actual_fraud, n: int) -> Optional[np.ndarray]:
    """None / a sequence of None, False, True (or codes 0, 1, FD_AB_NO_LABEL) -> uint8 [n] or None"""
    if actual_fraud is None:
        return None
    a = np.asarray(actual_fraud)
    if a.dtype.kind in "iub":
        return np.ascontiguousarray(a, np.uint8)
    return np.fromiter((N.FD_AB_NO_LABEL if v is None else (1 if v else 0) for v in actual_fraud), np.uint8, n)


def record_ref(state: N.fd_ab_state, variant, prediction, decision, processing_time_ms, actual_fraud=None) -> None:
    """fd_ab_record_ref_host: the rows, in order, into `state` on the host (no engine)."""
    variant = np.ascontiguousarray(variant, np.uint8)
    n = len(variant)
    prediction = np.ascontiguousarray(prediction, np.float64)
    decision = decision_codes(decision)
    scalar = np.ndim(processing_time_ms) == 0
    times = None if scalar else np.ascontiguousarray(processing_time_ms, np.float64)
    label = label_codes(actual_fraud, n)
    p = lambda a: None if a is None else C.c_void_p(a.ctypes.data)  # noqa: E731
    N.call("fd_ab_record_ref_host", p(variant), p(prediction), p(decision), p(times),
           float(processing_time_ms) if scalar else 0.0, p(label), n, C.byref(state))


def merge_states(a: N.fd_ab_state, b: N.fd_ab_state) -> N.fd_ab_state:
    """fd_ab_state_merge_host: a then b (one state per rank; a node's summary is the merge)"""
    out = N.fd_ab_state()
    N.call("fd_ab_state_merge_host", C.byref(a), C.byref(b), C.byref(out))
    return out


def _mean(m: N.fd_ab_moments, n: int) -> float:
    return (m.sum_hi + m.sum_lo) / n


def _metrics(s: N.fd_ab_variant_state) -> Dict[str, float]:
    n = s.rows
    if n == 0:
        return {}
    by_name = {name: s.decisions[code] for name, code in DECISION_CODES.items()}
    out = {"total_samples": n,
           "fraud_detection_rate": (by_name["DECLINE"] + by_name["REVIEW"]) / n,
           "avg_processing_time_ms": _mean(s.time_ms, n),
           "avg_prediction_score": _mean(s.prediction, n)}
    for name in _RATE_ORDER:
        out[f"{name.lower()}_rate"] = by_name[name] / n
    if s.labeled:
        precision = s.tp / (s.tp + s.fp) if s.tp + s.fp > 0 else 0.0
        recall = s.tp / (s.tp + s.fn) if s.tp + s.fn > 0 else 0.0
        f1 = 2 * (precision * recall) / (precision + recall) if precision + recall > 0 else 0.0
        out.update({"precision": precision, "recall": recall, "f1_score": f1,
                    "accuracy": (s.tp + s.tn) / s.labeled, "labeled_samples": s.labeled})
    return out


def _metric_moments(s: N.fd_ab_variant_state, metric: str):
    """(n, mean, M2) of the value list the reference builds for `metric`, or None for its empty list"""
    def of_flags(n, k):  # n values, k of them 1.0 and the rest 0.0
        return (n, k / n, (k * (n - k)) / n) if n else None
    if metric == "fraud_detection_rate":
        return of_flags(s.rows, s.decisions[DECISION_CODES["DECLINE"]] + s.decisions[DECISION_CODES["REVIEW"]])
    if metric == "processing_time":
        return s.rows, _mean(s.time_ms, s.rows), s.time_ms.m2_hi + s.time_ms.m2_lo
    if metric == "prediction_score":
        return s.rows, _mean(s.prediction, s.rows), s.prediction.m2_hi + s.prediction.m2_lo
    if metric == "precision" and s.labeled == s.rows:  # one value per flagged row, 1.0 when it was fraud
        return of_flags(s.tp + s.fp, s.tp)
    return None


def _statistics(c: N.fd_ab_variant_state, t: N.fd_ab_variant_state, metric: str) -> Dict[str, Any]:
    mc, mt = _metric_moments(c, metric), _metric_moments(t, metric)
    if mc is None or mt is None:
        return dict(_INSUFFICIENT)
    f = np.float64
    with np.errstate(all="ignore"):  # one value in a list: its sample std is NaN, as numpy's is
        (nc, c_mean, c_m2), (nt, t_mean, t_m2) = mc, mt
        c_std = np.sqrt(f(c_m2) / (nc - 1))
        t_std = np.sqrt(f(t_m2) / (nt - 1))
        pooled = np.sqrt(((nc - 1) * c_std ** 2 + (nt - 1) * t_std ** 2) / f(nc + nt - 2))
        diff = f(t_mean) - f(c_mean)
        effect = diff / pooled if pooled > 0 else 0.0
        margin = 1.96 * (pooled * np.sqrt(1 / nc + 1 / nt))
        improvement = diff / c_mean * 100 if c_mean != 0 else 0
    return {"metric": metric, "control_mean": float(c_mean), "treatment_mean": float(t_mean),
            "control_std": float(c_std), "treatment_std": float(t_std), "effect_size": float(effect),
            "relative_improvement_percent": float(improvement) if c_mean != 0 else 0,
            "confidence_interval_95": [float(diff - margin), float(diff + margin)],
            "is_significant": bool(abs(effect) > 0.2),
            "sample_sizes": {"control": nc, "treatment": nt}}


def summary_from_state(config: ABTestConfig, state: N.fd_ab_state) -> Dict[str, Any]:
    """get_test_summary's dict for an active test with this state"""
    c, t = state.variant[0], state.variant[1]
    total = c.rows + t.rows
    if total == 0:
        return {"test_name": config.test_name, "status": "no_data", "total_samples": 0}
    out = {"test_name": config.test_name,
           "config": {"control_model": config.control_model, "treatment_model": config.treatment_model,
                      "traffic_split": config.traffic_split, "success_metric": config.success_metric},
           "total_samples": total, "control_samples": c.rows, "treatment_samples": t.rows,
           "control_metrics": _metrics(c), "treatment_metrics": _metrics(t)}
    if c.rows >= 100 and t.rows >= 100:
        out["statistical_analysis"] = _statistics(c, t, config.success_metric)
    return out


# ---------------------------------------------------------------------------------------------- the manager
class ABTestManager:
    def __init__(self, engine=None, device: int = 0, keep_results: bool = False):
        """engine: a FraudEngine to keep the tests on. It may be shared (other managers, direct ab_create callers):
        create_test then takes an engine test id that is free on that engine at once, and returns False when none
        is. Without one, an engine is created on GPU `device` at the first call that needs the device (creating
        tests, get_variant and the summary of a test without data need none); that engine is this manager's alone,
        so the ids it takes then are free by construction.
        keep_results: also keep every recorded row on the host, for export_results."""
        self.logger = logging.getLogger("ab_test_manager")
        self.engine = engine
        self._own = False
        self._device = int(device)
        self.keep_results = bool(keep_results)
        self.active_tests: Dict[str, ABTestConfig] = {}
        self.test_results: Dict[str, List[TestResult]] = {}  # rows, with keep_results only
        self._ids: Dict[str, int] = {}     # test name -> engine test id, once the test has touched the device
        self._totals: Dict[str, int] = {}  # rows recorded per test name (export_results after stop_test)

    def close(self) -> None:
        for name in list(self._ids):
            self._release(name)
        if self._own and self.engine is not None:
            self.engine.close()
        self.engine = None

    # ------------------------------------------------------------------ engine test ids
    def _id(self, test_name: str) -> int:
        tid = self._ids.get(test_name)
        if tid is None:
            if self.engine is None:
                from .engine import FraudEngine
                self.engine, self._own = FraudEngine(self._device), True
            tid = self._take_id(test_name, self.active_tests[test_name])
            if tid is None:  # (cannot happen on the manager's own engine: it holds at most FD_AB_MAX_TESTS tests)
                raise RuntimeError(f"no free A/B test id on the engine for {test_name}")
        return tid

    def _take_id(self, test_name: str, cfg: ABTestConfig) -> Optional[int]:
        """Create the test on the engine under the first id that is free there; None when every id is in use"""
        for tid in range(N.FD_AB_MAX_TESTS):
            if tid in self._ids.values():
                continue
            try:
                self.engine.ab_create(tid, salt_of(test_name), threshold_of(cfg.traffic_split))
            except N.NativeError as exc:
                if exc.code != N.FD_ERR_INVALID_ARG:
                    raise
                continue  # held by someone else on a shared engine
            self._ids[test_name] = tid
            return tid
        return None

    def _release(self, test_name: str) -> None:
        tid = self._ids.pop(test_name, None)
        if tid is not None and self.engine is not None:
            self.engine.ab_destroy(tid)

    # ------------------------------------------------------------------ the reference's surface
    def create_test(self, config: ABTestConfig) -> bool:
        try:
            if not self._validate_config(config):
                return False
            if config.test_name in self.active_tests:
                self.logger.warning("an active test is already named %s", config.test_name)
                return False
            if len(self.active_tests) >= N.FD_AB_MAX_TESTS:
                self.logger.error("an engine holds at most %d tests at once", N.FD_AB_MAX_TESTS)
                return False
            if self.engine is not None and self._take_id(config.test_name, config) is None:
                self.logger.error("every A/B test id of the engine is in use")
                return False
            self.active_tests[config.test_name] = config
            self.test_results[config.test_name] = []
            self._totals[config.test_name] = 0
            self.logger.info("test %s started: %s (control) against %s, %.1f%% of users on the latter",
                             config.test_name, config.control_model, config.treatment_model,
                             100 * config.traffic_split)
            return True
        except Exception as exc:  # a config whose fields do not compare: the reference reports False too
            self.logger.error("test %s not started: %s", getattr(config, "test_name", "?"), exc)
            return False

    def _validate_config(self, config: ABTestConfig) -> bool:
        if not 0.0 <= config.traffic_split <= 1.0:
            self.logger.error("traffic_split %r is outside [0, 1]", config.traffic_split)
            return False
        if config.minimum_sample_size < 100:
            self.logger.error("minimum_sample_size %r is below 100", config.minimum_sample_size)
            return False
        if not 0.01 <= config.significance_level <= 0.1:
            self.logger.error("significance_level %r is outside [0.01, 0.1]", config.significance_level)
            return False
        return True

    def get_variant(self, test_name: str, user_id: str) -> Optional[TestVariant]:
        """The user's variant in the test, None for an unknown test. Host only (fd_ab_bucket_host)."""
        cfg = self.active_tests.get(test_name)
        if cfg is None:
            return None
        v = variants_of([self._key(user_id)], test_name, cfg.traffic_split)[0]
        return TestVariant.TREATMENT if v else TestVariant.CONTROL

    def record_result(self, test_name: str, transaction_id: str, variant: TestVariant, model_used: str,
                      prediction: float, decision: str, processing_time_ms: float,
                      actual_fraud: Optional[bool] = None) -> None:
        if test_name not in self.active_tests:
            return
        self.record_batch(test_name, [1 if variant == TestVariant.TREATMENT else 0], [prediction], [decision],
                          [processing_time_ms], [actual_fraud])
        if self.keep_results:
            self.test_results[test_name].append(TestResult(transaction_id, variant, model_used, prediction, decision,
                                                           actual_fraud, processing_time_ms, time.time()))

    def get_test_summary(self, test_name: str) -> Dict[str, Any]:
        cfg = self.active_tests.get(test_name)
        if cfg is None:
            return {}
        state = self.engine.ab_state(self._ids[test_name]) if test_name in self._ids else N.fd_ab_state()
        return summary_from_state(cfg, state)

    def stop_test(self, test_name: str) -> bool:
        if test_name not in self.active_tests:
            return False
        del self.active_tests[test_name]
        self._release(test_name)
        self.logger.info("test %s ended", test_name)
        return True

    def get_active_tests(self) -> List[str]:
        return list(self.active_tests.keys())

    def export_results(self, test_name: str) -> Dict[str, Any]:
        """The reference's export. 'results' holds the recorded rows only when the manager was created with
        keep_results=True (the engine keeps accumulators, not rows); otherwise it is []. 'total_results' counts every
        recorded row either way."""
        if test_name not in self.test_results:
            return {}
        rows = self.test_results[test_name]
        return {"test_name": test_name, "export_timestamp": time.time(), "total_results": self._totals[test_name],
                "results": [{"transaction_id": r.transaction_id, "variant": r.variant.value,
                             "model_used": r.model_used, "prediction": r.prediction, "decision": r.decision,
                             "actual_fraud": r.actual_fraud, "processing_time_ms": r.processing_time_ms,
                             "timestamp": r.timestamp} for r in rows]}

    # ------------------------------------------------------------------ batches
    @staticmethod
    def _key(user_id) -> int:
        return hash64(user_id if isinstance(user_id, (str, bytes)) else str(user_id))

    def _keys(self, user_ids_or_keys) -> np.ndarray:
        a = user_ids_or_keys
        if isinstance(a, np.ndarray) and a.dtype.kind in "iu":
            return np.ascontiguousarray(a, np.uint64)
        return np.fromiter((self._key(u) for u in a), np.uint64, len(a))

    def assign_batch(self, test_name: str, user_ids_or_keys) -> Optional[np.ndarray]:
        """get_variant for a batch, on the device: user ids (hashed as get_variant does) or a uint64 array of keys
        -> uint8 [n], 0 control and 1 treatment; None for an unknown test."""
        if test_name not in self.active_tests:
            return None
        return self.engine_for(test_name).ab_assign(self._ids[test_name], self._keys(user_ids_or_keys))

    def engine_for(self, test_name: str):
        """The engine the test lives on (creates the engine and the test's id on first use) """
        self._id(test_name)
        return self.engine

    def test_id(self, test_name: str) -> int:
        """The engine test id, for the engine's ab_*_device calls on device-resident columns"""
        return self._id(test_name)

    def record_batch(self, test_name: str, variant, prediction, decision, processing_time_ms, actual_fraud=None,
                     n: Optional[int] = None) -> None:
        """n results at once. Arrays: variant (0 / 1 or TestVariant), prediction, decision (strings or enum
        fd_decision codes), processing_time_ms (an array, or one float for the whole batch), actual_fraud (None, or
        per row None / bool, or codes 0 / 1 / FD_AB_NO_LABEL). Device pointers (ints, with n): the same columns as
        uint8 / f64 / uint8 / f64 or a float / uint8 or None, recorded without leaving the device."""
        if test_name not in self.active_tests:
            return
        tid = self._id(test_name)
        if isinstance(variant, int) and n is not None:
            scalar = isinstance(processing_time_ms, float)
            self.engine.ab_record_device(tid, variant, int(prediction), int(decision), n,
                                         0 if scalar else int(processing_time_ms),
                                         processing_time_ms if scalar else 0.0, int(actual_fraud or 0))
        else:
            var = np.fromiter((1 if (v == TestVariant.TREATMENT or v == 1) else 0 for v in variant), np.uint8,
                              len(variant)) if not isinstance(variant, np.ndarray) else variant
            n = len(var)
            self.engine.ab_record(tid, var, prediction, decision_codes(decision), processing_time_ms,
                                  label_codes(actual_fraud, n))
        self._totals[test_name] += n

    def score_batch(self, test_name: str, X, keys, control: dict, treatment: dict) -> Dict[str, Any]:
        """Routed scoring: row i of X is scored by the model set of its user's variant. control / treatment: dicts
        of FraudEngine.score_matrix's arguments (params, slots, ext_probs, present). keys: user ids or uint64 keys."""
        if test_name not in self.active_tests:
            raise ValueError(f"A/B test {test_name} not found")
        tid = self._id(test_name)
        var, mp, fp, conf, dec, risk = self.engine.ab_score_matrix(tid, control, treatment, X, self._keys(keys))
        return {"variant": var, "model_probs": mp, "fraud_probability": fp, "confidence": conf, "decision": dec,
                "risk_level": risk}
