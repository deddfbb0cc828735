#!/usr/bin/env python3
"""Measure the prediction metrics' kernels (csrc/metrics.hip) alone, in ONE process, every column resident on the
device, beside the closest existing kernel, fd_ab_record_device (one streaming pass plus a ticket reduction), at the
same row counts. Per batch size N and model count M, after WARMUP windows, STEPS windows of CALLS back-to-back calls
each, the legs alternating window by window:

  metrics_record   fd_metrics_record_device: fraud_prob, decision, M model columns, a time column      device ms / call
  ab_record        fd_ab_record_device: variant, prediction, decision, time, label                     device ms / call
  metrics_query    fd_metrics_query_host with SLOTS_USED slots in the ring (kernel, copy of one struct
                   back, stream wait)                                                                  wall ms / call

Device times are device events around a window on the engine's stream, divided by CALLS (a call is a 4-byte memset of
the ticket and one launch; a record call that opens a slot adds a 688-byte memset: every window opens one). Medians,
minima and maxima over the windows are reported, and for the record legs the bytes a row brings in: 9 + 8 M + 8
against ab_record's 19 + 8.

Prints one JSON line per leg and appends it to OUT (default profiles/metrics/metrics_bench.jsonl); writes the kernels'
registers / LDS / scratch (the compiler's remarks the build recorded) to profiles/metrics/kernel_resources.json.
Environment: SIZES (default 1024,65536), MODELS (2,8), STEPS (20), WARMUP (3), CALLS (200), OUT."""
import json
import os
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(REPO), str(REPO / "realtime-fraud-detection_amd")]
import numpy as np

SIZES = [int(s) for s in os.environ.get("SIZES", "1024,65536").split(",")]
MODELS = [int(s) for s in os.environ.get("MODELS", "2,8").split(",")]
STEPS = int(os.environ.get("STEPS", 20))
WARMUP = int(os.environ.get("WARMUP", 3))
CALLS = int(os.environ.get("CALLS", 200))
OUT = Path(os.environ.get("OUT", REPO / "profiles" / "metrics" / "metrics_bench.jsonl"))
SLOTS = 4096


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    OUT.parent.mkdir(parents=True, exist_ok=True)
    with open(OUT, "a") as f:
        f.write(line + "\n")


def stats(ms):
    return {"ms_median": float(np.median(ms)), "ms_min": float(np.min(ms)), "ms_max": float(np.max(ms))}


def write_resources():
    from fdengine.build import RESOURCES
    res = json.loads(RESOURCES.read_text())
    keep = {k: v for k, v in res.items() if "metrics_" in k or "ab_record_kernel" in k}
    (OUT.parent / "kernel_resources.json").write_text(json.dumps(keep, indent=1, sort_keys=True) + "\n")


def main():
    import torch

    from fdengine import FraudEngine
    eng = FraudEngine(0)
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    eng.ab_create(0, 1, 50.0)
    stamp = [0.0]

    def window(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        stamp[0] += 1.0
        a.record()
        for _ in range(CALLS):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / CALLS

    for n in SIZES:
        rng = np.random.default_rng(n)
        fp = torch.from_numpy(rng.random(n)).cuda()
        dec = torch.from_numpy(rng.integers(0, 4, n).astype(np.uint8)).cuda()
        times = torch.from_numpy(0.2 + 80 * rng.random(n)).cuda()
        var = torch.from_numpy((rng.random(n) < 0.5).astype(np.uint8)).cuda()
        label = torch.from_numpy(rng.integers(0, 2, n).astype(np.uint8)).cuda()
        mp = torch.from_numpy(rng.random((max(MODELS), n))).cuda()
        torch.cuda.synchronize()

        def ab():
            eng.ab_record_device(0, var.data_ptr(), fp.data_ptr(), dec.data_ptr(), n, time_ptr=times.data_ptr(),
                                 label_ptr=label.data_ptr())

        for M in MODELS:
            eng.metrics_init(M, SLOTS)

            def rec():
                eng.metrics_record_device(fp.data_ptr(), dec.data_ptr(), n, stamp[0], mp.data_ptr(), M,
                                          times.data_ptr())

            got = {"metrics_record": [], "ab_record": []}
            for step in range(WARMUP + STEPS):
                for leg, fn in (("metrics_record", rec), ("ab_record", ab)):
                    ms = window(fn)
                    if step >= WARMUP:
                        got[leg].append(ms)
            base = {"n": n, "models": M, "steps": STEPS, "warmup": WARMUP, "calls_per_window": CALLS,
                    "clock": "device"}
            m_ms, a_ms = np.median(got["metrics_record"]), np.median(got["ab_record"])
            emit({"leg": "metrics_record", **base, **stats(got["metrics_record"]), "bytes_per_row": 9 + 8 * M + 8,
                  "rows_per_s_median": n / float(m_ms) * 1e3, "over_ab_record_median": float(m_ms / a_ms),
                  "bytes_ratio_to_ab_record": (9 + 8 * M + 8) / 27})
            emit({"leg": "ab_record", **base, **stats(got["ab_record"]), "bytes_per_row": 27,
                  "rows_per_s_median": n / float(a_ms) * 1e3})
            s = eng.metrics_query(stamp[0])
            assert s.total.predictions == n * CALLS * (WARMUP + STEPS) and s.slots_used == WARMUP + STEPS
    # the query, with the ring as full as an hour at the default resolution makes it
    used = 3600
    eng.metrics_init(2, SLOTS)
    n = 1024
    for k in range(used):
        eng.metrics_record_device(fp.data_ptr(), dec.data_ptr(), n, float(k), mp.data_ptr(), 2, times.data_ptr())
    ms = []
    for step in range(WARMUP + STEPS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s = eng.metrics_query(float(used))
        if step >= WARMUP:
            ms.append((time.perf_counter() - t0) * 1e3)
    assert s.slots_used == used and s.hour.rows == n * used and s.minute.rows == n * 60
    emit({"leg": "metrics_query", "slots_used": used, "slots": SLOTS, "steps": STEPS, "warmup": WARMUP,
          "clock": "wall", **stats(ms)})
    write_resources()
    eng.close()


if __name__ == "__main__":
    main()
