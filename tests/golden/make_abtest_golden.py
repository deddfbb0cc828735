#!/usr/bin/env python3
"""Generate tests/golden/abtest_cases.npz by running the REFERENCE's own ABTestManager
(services/ml-models/src/testing/ab_testing.py) in the build container. Only the rows' columns and the dicts its
get_test_summary returned travel; the reference never does. Never runs on the GPU machine. Needs the engine's library
(host entry points only: fd_hash64, fd_ab_bucket_host), no GPU.

Run:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_abtest_golden.py

Reference code exercised (unchanged): create_test, get_variant, record_result, get_test_summary. Its get_variant
hashes with Python's per-process salted hash(), so its own assignments are not reproducible; it consults its
user_assignments cache first, so each user's variant, computed by the engine's host bucket function, is placed there
before get_variant is called and the reference replays it. Everything after the assignment is the reference's.
utils.logging_config is used as it is when it imports, else registered as a module whose get_logger returns a
standard logger.

Cases: tests/abtest_cases.py SPECS. What each is there for is asserted below on the reference's outputs."""
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
sys.path.insert(0, str(HERE.parent.parent / "realtime-fraud-detection_amd"))

import abtest_cases as T  # noqa: E402
from fdengine.ab_testing import variants_of  # noqa: E402
from fdengine.ingest import hash64_many  # noqa: E402


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
    import testing.ab_testing as R
    return R


def plain(x):
    """numpy scalars out of the reference's dicts -> Python values (json); the values are unchanged"""
    if isinstance(x, dict):
        return {k: plain(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [plain(v) for v in x]
    if isinstance(x, (bool, np.bool_)):
        return bool(x)
    if isinstance(x, (int, np.integer)):
        return int(x)
    if isinstance(x, (float, np.floating)):
        return float(x)
    return x


def run_reference(R, case, users):
    mgr = R.ABTestManager()
    name = case["name"]
    cfg = R.ABTestConfig(name, "champion", "challenger", case["split"], "2026-01-01", "2026-02-01",
                         success_metric=case["metric"])
    assert mgr.create_test(cfg)
    to_variant = {0: R.TestVariant.CONTROL, 1: R.TestVariant.TREATMENT}
    mgr.user_assignments[name] = {u: to_variant[int(v)] for u, v in zip(users, case["variant"])}
    names = {code: d for code, d in enumerate(T.DECISIONS)}
    names[T.OTHER] = T.OTHER_NAME
    for i, u in enumerate(users):
        v = mgr.get_variant(name, u)
        assert v == to_variant[int(case["variant"][i])]
        lab = int(case["label"][i])
        mgr.record_result(name, f"txn_{i}", v, cfg.treatment_model if v == R.TestVariant.TREATMENT
                          else cfg.control_model, float(case["prediction"][i]), names[int(case["decision"][i])],
                          float(case["time_ms"][i]), None if lab == T.NO_LABEL else bool(lab))
    return plain(mgr.get_test_summary(name))


def main():
    R = reference_module()
    arrays, meta = {}, []
    seen = {"empty": 0, "small": 0, "stats": 0, "error": 0, "zero_pooled": 0, "zero_control": 0, "unlabeled": 0}
    for i, spec in enumerate(T.SPECS):
        name, n, split, metric, labels, preds = spec
        users = T.user_ids(name, n, 500 + i)
        keys = hash64_many(users)
        case = T.draw_case(i, spec, keys, variants_of(keys, name, split))
        case.update(name=name, split=split, metric=metric)
        with np.errstate(all="ignore"):
            summary = run_reference(R, case, users)
        nc, nt = summary.get("control_samples", 0), summary.get("treatment_samples", 0)
        seen["empty"] += n > 1 and min(nc, nt) == 0
        seen["small"] += 0 < min(nc, nt) < 100
        seen["unlabeled"] += any("labeled_samples" not in summary[s] and summary[s]
                                 for s in ("control_metrics", "treatment_metrics"))
        st = summary.get("statistical_analysis")
        if st is not None:
            seen["error" if "error" in st else "stats"] += 1
            if "error" not in st:
                # is_significant must not be able to flip inside the comparison's tolerance
                assert abs(abs(st["effect_size"]) - 0.2) > 1e-6, (name, st["effect_size"])
                seen["zero_pooled"] += st["control_std"] == 0 and st["treatment_std"] == 0 and st["effect_size"] == 0
                seen["zero_control"] += st["control_mean"] == 0 and st["relative_improvement_percent"] == 0
        for col in T.COLUMNS:
            arrays[f"{i}_{col}"] = case[col]
        meta.append({"name": name, "split": split, "metric": metric, "summary": summary})
        print(f"{name}: n {n} control {nc} treatment {nt} analysis "
              f"{'-' if st is None else st.get('error', st.get('effect_size'))}")
    assert sorted({s[1] for s in T.SPECS}) == [1, 63, 64, 65, 199, 200, 257, 1025, 5000]
    assert {s[3] for s in T.SPECS} >= {"fraud_detection_rate", "processing_time", "prediction_score", "precision"}
    assert seen["empty"] >= 2 and seen["small"] >= 1 and seen["unlabeled"] >= 1 and seen["stats"] >= 6, seen
    assert seen["error"] >= 2 and seen["zero_pooled"] >= 1 and seen["zero_control"] >= 1, seen
    arrays["meta"] = np.array(json.dumps(meta))
    np.savez_compressed(T.GOLDEN, **arrays)
    print("wrote", T.GOLDEN, T.GOLDEN.stat().st_size, "bytes", seen)


if __name__ == "__main__":
    main()
