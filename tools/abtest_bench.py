#!/usr/bin/env python3
"""Measure the A/B tests' routed scoring and recording (csrc/abtest.hip, fd_ab_score_matrix_device) alone, in ONE
process, everything resident on the device. Model pair: the headline's shapes, an XGBoost forest of 500 trees of depth
8 over 64 features and the IsolationForest of the reference trainer's recipe; both variants use the pair, so the routed
call scores exactly the rows the plain call scores. Per batch size N, after WARMUP calls, STEPS calls each of:

  score_matrix      one fd_score_matrix_device over the N rows                                   wall ms per call
  ab_score_matrix   fd_ab_score_matrix_device at split 0.5 over the same rows                    wall ms per call
                    and, from the engine's timing (FD_TIMING_ABTEST), the device ms of its own kernels
                    (assign, partition, gather, scatter) inside those calls
  ab_assign         fd_ab_assign_device alone                                                    device ms
  ab_partition      fd_ab_partition_device alone                                                 device ms
  ab_record         fd_ab_record_device alone (variant, prediction, decision, time, label)       device ms

Wall times are host clocks around the call and a device synchronisation: the routed call waits once inside itself
(it reads the two counts back), which no device timer sees. Medians, minima and maxima are reported.

Prints one JSON line per leg and appends it to OUT (default profiles/abtest/abtest_bench.jsonl). Environment: SIZES
(default 65536,1024), STEPS (30), WARMUP (5), OUT."""
import ctypes as C
import json
import os
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(REPO), str(REPO / "realtime-fraud-detection_amd")]
import numpy as np

SIZES = [int(s) for s in os.environ.get("SIZES", "65536,1024").split(",")]
STEPS = int(os.environ.get("STEPS", 30))
WARMUP = int(os.environ.get("WARMUP", 5))
OUT = Path(os.environ.get("OUT", REPO / "profiles" / "abtest" / "abtest_bench.jsonl"))
TID = 0


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    OUT.parent.mkdir(parents=True, exist_ok=True)
    with open(OUT, "a") as f:
        f.write(line + "\n")


def stats(ms):
    return {"ms_median": float(np.median(ms)), "ms_min": float(np.min(ms)), "ms_max": float(np.max(ms))}


def main():
    import torch

    import fdengine
    from fdengine import FraudEngine, synth, _native as N
    from fdengine.ab_testing import salt_of, threshold_of
    eng = FraudEngine(0)
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    Xr = synth.feature_matrix(8192, 64, seed=21)
    eng.load_forest(0, fdengine.xgboost_from_json_doc(synth.xgboost_doc(500, 8, 64, Xr, seed=13)))
    eng.load_forest(1, fdengine.iforest_from_sklearn(synth.isolation_forest(Xr.astype(np.float64))))
    pair = {"params": FraudEngine.blend_params([0.8, 0.2], [1.0, 0.9]), "slots": [0, 1]}
    _, (params, slots, present, ext) = FraudEngine._ab_model_set(pair, True)  # score_matrix's marshalled arguments
    eng.ab_create(TID, salt_of("bench"), threshold_of(0.5))

    def wall(fn):
        ms = []
        for step in range(WARMUP + STEPS):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if step >= WARMUP:
                ms.append((time.perf_counter() - t0) * 1e3)
        return ms

    def device(fn, entries):
        """device ms of the FD_TIMING_ABTEST entries of one call"""
        ms = []
        eng.read_timing(N.FD_TIMING_ABTEST)
        for step in range(WARMUP + STEPS):
            eng.set_timing(step >= WARMUP)
            fn()
            torch.cuda.synchronize()
            if step >= WARMUP:
                t, launches = eng.read_timing(N.FD_TIMING_ABTEST)
                assert launches == entries, (launches, entries)
                ms.append(t)
        eng.set_timing(False)
        return ms

    for n in SIZES:
        rng = np.random.default_rng(n)
        X = torch.from_numpy(synth.feature_matrix(n, 64, seed=22).astype(np.float32)).cuda()
        keys = torch.from_numpy(rng.integers(0, 1 << 63, n, dtype=np.int64)).cuda()
        var = torch.empty(n, dtype=torch.uint8, device="cuda")
        idx = torch.empty(n, dtype=torch.int32, device="cuda")
        counts = torch.empty(2, dtype=torch.int64, device="cuda")
        fp, conf = (torch.empty(n, dtype=torch.float64, device="cuda") for _ in range(2))
        dec, risk = (torch.empty(n, dtype=torch.uint8, device="cuda") for _ in range(2))
        times = torch.from_numpy(20 + 60 * rng.random(n)).cuda()
        label = torch.from_numpy(rng.integers(0, 2, n).astype(np.uint8)).cuda()
        p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

        def plain():
            N.call("fd_score_matrix_device", eng.handle, C.byref(params), C.c_void_p(slots.ctypes.data), ext,
                   C.c_void_p(present.ctypes.data), p(X), n, 64, None, p(fp), p(conf), p(dec), p(risk))

        def routed():
            eng.ab_score_matrix_device(TID, pair, pair, X.data_ptr(), keys.data_ptr(), n, 64, fp.data_ptr(),
                                       variant_ptr=var.data_ptr(), conf_ptr=conf.data_ptr(), dec_ptr=dec.data_ptr(),
                                       risk_ptr=risk.data_ptr())

        base = {"n": n, "steps": STEPS, "warmup": WARMUP}
        plain_ms = wall(plain)
        want = fp.clone()
        emit({"leg": "score_matrix", **base, "clock": "wall", **stats(plain_ms)})
        routed_ms = wall(routed)
        n_treat = int(var.sum().item())
        emit({"leg": "ab_score_matrix", **base, "clock": "wall", "split": 0.5, "treatment_rows": n_treat,
              "fraud_prob_equals_score_matrix": bool(torch.equal(fp, want)),
              **stats(routed_ms), "over_score_matrix_median": float(np.median(routed_ms) / np.median(plain_ms))})
        emit({"leg": "ab_score_matrix_own_kernels", **base, "clock": "device",
              "entries": "assign, partition, gather, scatter", **stats(device(routed, 4))})
        emit({"leg": "ab_assign", **base, "clock": "device",
              **stats(device(lambda: eng.ab_assign_device(TID, keys.data_ptr(), n, var.data_ptr()), 1))})
        emit({"leg": "ab_partition", **base, "clock": "device",
              **stats(device(lambda: eng.ab_partition_device(var.data_ptr(), n, idx.data_ptr(), counts.data_ptr()),
                             1))})
        rec_ms = device(lambda: eng.ab_record_device(TID, var.data_ptr(), fp.data_ptr(), dec.data_ptr(), n,
                                                     time_ptr=times.data_ptr(), label_ptr=label.data_ptr()), 1)
        emit({"leg": "ab_record", **base, "clock": "device", **stats(rec_ms),
              "rows_per_s_median": n / float(np.median(rec_ms)) * 1e3})
    s = eng.ab_state(TID)
    assert s.variant[0].rows + s.variant[1].rows == sum(SIZES) * (WARMUP + STEPS)
    eng.close()


if __name__ == "__main__":
    main()
