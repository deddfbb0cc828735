"""A/B test cases shared by tests/golden/make_abtest_golden.py (which runs the reference on them), tests/test_abtest_host.py
and tests/test_gpu_abtest.py: how the streams are drawn, how the fixture is read, and the comparison of a summary with
the reference's. Nothing here touches the GPU.

A case is one test (name, traffic split, success metric) and a stream of n results: user key, variant, prediction,
decision code (enum fd_decision; OTHER for a string outside the four), processing time, label (0, 1, 255 = None).
The variant of a row is the engine's own assignment of its user key (fdengine.ab_testing.variants_of), which the
generator hands to the reference through its user_assignments cache.

Tolerances:
  equal       counts, quotients of counts, is_significant, sample_sizes, and the means of the two 0/1 metrics: each is
              one f64 operation on equal integers, in the reference's operation order
  means       |got - ref| <= 2 n 2^-53 max|x|. Either side is a sum of n f64 values, whose error in any order is at
              most (n - 1) 2^-53 sum|x| <= (n - 1) 2^-53 n max|x|, then one division by n: two such errors apart
  the rest    stds, effect size, improvement, confidence bounds: both sides are stable algorithms with different
              constants (compensated sums and Chan's merge here, numpy's two-pass pairwise sums there), so each is
              measured against the exact value, computed from the fixture's f64 inputs with fractions and 60-digit
              decimal square roots. The engine may err at most 4 x the reference's own error; where the reference's
              error is (nearly) 0, at most 16 ulp of the exact value.
"""
import json
import math
from decimal import Decimal, getcontext
from fractions import Fraction
from pathlib import Path

import numpy as np

GOLDEN = Path(__file__).resolve().parent / "golden" / "abtest_cases.npz"
COLUMNS = ("key", "variant", "prediction", "decision", "time_ms", "label")
DECISIONS = ("APPROVE", "REVIEW", "DECLINE", "APPROVE_WITH_MONITORING")  # enum fd_decision
OTHER = 254
OTHER_NAME = "HOLD"
NO_LABEL = 255
SPLITS = (0.0, 0.07, 0.28, 0.29, 0.3, 0.55, 0.58, 1.0)
TREATMENT_BUCKETS = (0, 8, 29, 29, 30, 56, 58, 100)
CUTS = (1, 64, 1000)

# name, n, split, success metric, labels ("all" / "part" / "none"), predictions ("random" / "const" / "zero_control")
SPECS = (
    ("one_row", 1, 0.3, "fraud_detection_rate", "none", "random"),
    ("empty_treatment", 63, 0.0, "fraud_detection_rate", "all", "random"),
    ("empty_control", 64, 1.0, "prediction_score", "part", "random"),
    ("small_both", 65, 0.5, "processing_time", "none", "random"),
    ("one_side_small", 199, 0.3, "precision", "part", "random"),
    ("n200", 200, 0.5, "processing_time", "all", "random"),
    ("rate_257", 257, 0.5, "fraud_detection_rate", "all", "random"),
    ("score_1025", 1025, 0.3, "prediction_score", "part", "random"),
    ("precision_1025", 1025, 0.55, "precision", "all", "random"),
    ("precision_unlabeled_rows", 1025, 0.55, "precision", "part", "random"),
    ("time_5000", 5000, 0.07, "processing_time", "all", "random"),
    ("unknown_metric", 5000, 0.58, "latency_p99", "part", "random"),
    ("constant_scores", 1025, 0.29, "prediction_score", "none", "const"),
    ("zero_control_mean", 1025, 0.28, "prediction_score", "all", "zero_control"),
    ("rate_5000", 5000, 0.28, "fraud_detection_rate", "none", "random"),
)


def user_ids(name, n, seed):
    """n user ids from a pool of about n / 3 users, so that users return"""
    rng = np.random.default_rng(seed)
    return [f"{name}_user_{u}" for u in rng.integers(0, max(1, n // 3) + 1, n)]


def draw_case(idx, spec, keys, variant):
    """The columns of a case, given its users' keys and variants (which need the engine's library)"""
    name, n, split, metric, labels, preds = spec
    rng = np.random.default_rng(1000 + idx)
    prediction = rng.random(n)
    # the treatment scores a little higher and flags more, so that the two variants differ
    prediction = np.where(variant == 1, np.minimum(1.0, prediction * 1.08), prediction)
    if preds == "const":
        prediction = np.full(n, 0.5)
    elif preds == "zero_control":
        prediction = np.where(variant == 0, 0.0, prediction)
    decision = np.where(prediction > 0.8, 2, np.where(prediction > 0.55, 1, np.where(prediction > 0.35, 3, 0)))
    if preds != "random":
        decision = rng.integers(0, 4, n)
    decision = decision.astype(np.uint8)
    if name == "score_1025":
        decision[rng.choice(n, 7, replace=False)] = OTHER
    time_ms = 20.0 + 60.0 * rng.random(n) + np.where(variant == 1, 3.0, 0.0)
    fraud = (rng.random(n) < 0.15 + 0.5 * prediction).astype(np.uint8)
    if labels == "none":
        label = np.full(n, NO_LABEL, np.uint8)
    elif labels == "part":
        label = np.where(rng.random(n) < 0.6, fraud, NO_LABEL).astype(np.uint8)
    else:
        label = fraud
    return {"key": np.asarray(keys, np.uint64), "variant": np.asarray(variant, np.uint8), "prediction": prediction,
            "decision": decision, "time_ms": time_ms, "label": label}


def load():
    """-> list of cases: {"name", "split", "metric", "summary" (the reference's), and the COLUMNS arrays}"""
    z = np.load(GOLDEN)
    meta = json.loads(str(z["meta"]))
    cases = []
    for i, m in enumerate(meta):
        c = dict(m)
        for col in COLUMNS:
            c[col] = z[f"{i}_{col}"]
        cases.append(c)
    return cases


def config_of(case):
    from fdengine.ab_testing import ABTestConfig
    return ABTestConfig(case["name"], "champion", "challenger", case["split"], "2026-01-01", "2026-02-01",
                        success_metric=case["metric"])


def pieces(n, cut):
    return [(a, min(n, a + cut)) for a in range(0, n, cut)]


# ------------------------------------------------------------------------------------------- exact statistics
getcontext().prec = 60


def _dec(fr):
    return Decimal(fr.numerator) / Decimal(fr.denominator)


def metric_values(case, v):
    """The value list the reference builds for the case's metric over variant v's rows, or None where it is empty"""
    rows = case["variant"] == v
    dec, lab = case["decision"][rows], case["label"][rows]
    flagged = (dec == 1) | (dec == 2)
    m = case["metric"]
    if m == "fraud_detection_rate":
        return flagged.astype(np.float64)
    if m == "processing_time":
        return case["time_ms"][rows]
    if m == "prediction_score":
        return case["prediction"][rows]
    if m == "precision" and (lab != NO_LABEL).all():
        return (lab[flagged] == 1).astype(np.float64)
    return None


def exact_statistics(case):
    """The statistical analysis's float fields, exactly rounded from the f64 inputs (Decimal, 60 digits)"""
    vals = [metric_values(case, v) for v in (0, 1)]
    mom = []
    for x in vals:
        fx = [Fraction(float(a)) for a in x]
        n = len(fx)
        mean = sum(fx) / n
        var = sum((a - mean) ** 2 for a in fx) / (n - 1)
        mom.append((n, mean, var))
    (nc, mc, vc), (nt, mt, vt) = mom
    pooled = _dec(((nc - 1) * vc + (nt - 1) * vt) / (nc + nt - 2)).sqrt()
    diff = _dec(mt - mc)
    margin = Decimal(1.96) * pooled * _dec(Fraction(1, nc) + Fraction(1, nt)).sqrt()
    return {"control_std": _dec(vc).sqrt(), "treatment_std": _dec(vt).sqrt(),
            "effect_size": diff / pooled if pooled > 0 else Decimal(0),
            "relative_improvement_percent": _dec((mt - mc) / mc * 100) if mc != 0 else Decimal(0),
            "ci_low": diff - margin, "ci_high": diff + margin}


def error_ratio(got, ref, exact):
    """(|got - exact| in units of the bound max(4 |ref - exact|, 16 ulp(exact)), the bound): <= 1 passes"""
    bound = max(4 * abs(Decimal(ref) - exact), 16 * Decimal(math.ulp(float(exact))))
    return float(abs(Decimal(got) - exact) / bound), bound


def check_summary(got, case, ratios=None):
    """Assert `got` (a get_test_summary dict) against the reference's for the case; ratios (a dict) collects the
    largest error ratio per field."""
    want = case["summary"]
    assert list(got) == list(want), (list(got), list(want))
    for k in want:
        if k not in ("control_metrics", "treatment_metrics", "statistical_analysis"):
            assert got[k] == want[k], (case["name"], k, got[k], want[k])
    for v, side in enumerate(("control_metrics", "treatment_metrics")):
        g, w = got[side], want[side]
        assert list(g) == list(w), (case["name"], side, list(g), list(w))
        rows = case["variant"] == v
        n = int(rows.sum())
        for k in w:
            if k in ("avg_processing_time_ms", "avg_prediction_score"):
                x = case["time_ms" if k == "avg_processing_time_ms" else "prediction"][rows]
                tol = 2 * n * 2.0 ** -53 * float(np.abs(x).max())
                print(f"{case['name']} {side} {k}: |diff| {abs(g[k] - w[k]):.3e} tol {tol:.3e}")
                assert abs(g[k] - w[k]) <= tol, (case["name"], side, k, g[k], w[k], tol)
            else:
                assert g[k] == w[k], (case["name"], side, k, g[k], w[k])
    if "statistical_analysis" not in want:
        return
    g, w = got["statistical_analysis"], want["statistical_analysis"]
    assert list(g) == list(w), (case["name"], list(g), list(w))
    if "error" in w:
        assert g == w
        return
    assert g["metric"] == w["metric"] and g["sample_sizes"] == w["sample_sizes"]
    assert g["is_significant"] == w["is_significant"], (case["name"], g["effect_size"], w["effect_size"])
    exact_means = case["metric"] in ("fraud_detection_rate", "precision")
    for v, k in enumerate(("control_mean", "treatment_mean")):
        if exact_means:
            assert g[k] == w[k], (case["name"], k, g[k], w[k])
        else:
            x = metric_values(case, v)
            tol = 2 * len(x) * 2.0 ** -53 * float(np.abs(x).max())
            print(f"{case['name']} {k}: |diff| {abs(g[k] - w[k]):.3e} tol {tol:.3e}")
            assert abs(g[k] - w[k]) <= tol, (case["name"], k, g[k], w[k], tol)
    ex = exact_statistics(case)
    flat = lambda s: {**{k: s[k] for k in ("control_std", "treatment_std", "effect_size",  # noqa: E731
                                           "relative_improvement_percent")},
                      "ci_low": s["confidence_interval_95"][0], "ci_high": s["confidence_interval_95"][1]}
    fg, fw = flat(g), flat(w)
    for k, e in ex.items():
        if math.isnan(fw[k]):
            assert math.isnan(fg[k]), (case["name"], k, fg[k])
            continue
        r, bound = error_ratio(fg[k], fw[k], e)
        print(f"{case['name']} {k}: engine {fg[k]!r} reference {fw[k]!r} error / bound {r:.3f}")
        if ratios is not None:
            ratios[k] = max(ratios.get(k, 0.0), r)
        assert r <= 1.0, (case["name"], k, fg[k], fw[k], str(e), str(bound))
