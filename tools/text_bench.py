#!/usr/bin/env python3
"""Measure the text patterns and features (csrc/text.hip) alone, in ONE process: calls of N rows through
fd_text_features_device, blob and offsets resident on the device, timed by the engine (FD_TIMING_TEXT: HIP events
around all kernels of a call). After WARMUP calls STEPS calls are timed one by one; the median, minimum and maximum are
reported with rows/s and bytes/s, per stream:

  random  rows of the fixture's random stream (tests/text_cases.py random_rows: four fields of 0-300 bytes from word
          lists, keywords mixed in): DISTINCT rows generated, repeated to N
  4k      every row 4096 bytes (64 of merchant_name, 3900 of description, the rest category and location):
          DISTINCT / 16 rows generated, repeated to N

--reference: instead, the reference's own BertTextAnalyzer.detect_fraud_patterns + get_text_features over the first
REF_ROWS rows of each stream on this host's CPU, ms per row. Runs only where the reference tree exists
(tests/golden/make_text_golden.py knows where).

Prints one JSON line per stream and appends it to OUT (default profiles/text/text_bench.jsonl). Environment: N
(default 65536), STEPS (20), WARMUP (3), STREAMS (random,4k), DISTINCT (4096), REF_ROWS (2000), OUT."""
import json
import os
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(REPO), str(REPO / "realtime-fraud-detection_amd"), str(REPO / "tests")]
import numpy as np

N_ROWS = int(os.environ.get("N", 65536))
STEPS = int(os.environ.get("STEPS", 20))
WARMUP = int(os.environ.get("WARMUP", 3))
STREAMS = os.environ.get("STREAMS", "random,4k").split(",")
DISTINCT = int(os.environ.get("DISTINCT", 4096))
REF_ROWS = int(os.environ.get("REF_ROWS", 2000))
OUT = Path(os.environ.get("OUT", REPO / "profiles" / "text" / "text_bench.jsonl"))


def distinct_rows(which, n):
    """n rows of four str"""
    import text_cases as T
    if which == "random":
        return T.random_rows(T.keywords(), n=n, seed=77)[:n]
    rng = np.random.default_rng(78)
    rows = []
    for _ in range(n):
        rows.append([T.random_text(rng, 64), T.random_text(rng, 3900), T.random_text(rng, 66),
                     T.random_text(rng, 66)])
    return rows


def stream(which, n):
    """(uint8 blob, int64 offsets [4n + 1]) of n rows: DISTINCT rows repeated"""
    import text_cases as T
    blob, off = T.encode(distinct_rows(which, min(DISTINCT if which == "random" else DISTINCT // 16, n)))
    d = len(off) // 4
    reps = -(-n // d)
    lens = np.tile(np.diff(off), reps)[:4 * n]
    full = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return np.tile(blob, reps)[:full[-1]].copy(), full


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    OUT.parent.mkdir(parents=True, exist_ok=True)
    with open(OUT, "a") as f:
        f.write(line + "\n")


def reference_leg():
    sys.path.insert(0, str(REPO / "tests" / "golden"))
    import make_text_golden as MG
    import text_cases as T
    if not MG.REF_SRC.exists():
        print("reference tree not present: nothing measured")
        return
    det = MG.reference_class()(device="cpu")
    for which in STREAMS:
        rows = [dict(zip(T.FIELDS, r)) for r in distinct_rows(which, REF_ROWS)]
        nbytes = sum(len(s) for r in rows for s in r.values())
        t0 = time.perf_counter()
        for r in rows:
            det.detect_fraud_patterns(r)
            det.get_text_features(r)
        dt = time.perf_counter() - t0
        emit({"leg": "reference_python", "stream": which, "rows": len(rows), "bytes": nbytes, "seconds": dt,
              "ms_per_row": dt / len(rows) * 1e3, "rows_per_s": len(rows) / dt, "bytes_per_s": nbytes / dt})


def main():
    if "--reference" in sys.argv:
        return reference_leg()
    import torch

    import fdengine
    from fdengine import _native as N
    eng = fdengine.FraudEngine(0)
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    feat = torch.empty((N_ROWS, N.FD_TEXT_FEATURES), dtype=torch.float64, device="cuda")
    pat = torch.empty(N_ROWS, dtype=torch.uint8, device="cuda")
    st = torch.empty(N_ROWS, dtype=torch.uint8, device="cuda")
    for which in STREAMS:
        blob, off = stream(which, N_ROWS)
        d_blob, d_off = torch.from_numpy(blob).cuda(), torch.from_numpy(off).cuda()
        eng.read_timing(N.FD_TIMING_TEXT)
        ms = []
        for step in range(WARMUP + STEPS):
            eng.set_timing(step >= WARMUP)
            eng.text_features_device(d_blob.data_ptr(), d_off.data_ptr(), N_ROWS, feat.data_ptr(), pat.data_ptr(),
                                     st.data_ptr())
            torch.cuda.synchronize()
            if step >= WARMUP:
                t_ms, launches = eng.read_timing(N.FD_TIMING_TEXT)
                assert launches == 1
                ms.append(t_ms)
        eng.set_timing(False)
        p = pat.cpu().numpy()
        med = float(np.median(ms))
        emit({"leg": "engine", "stream": which, "n": N_ROWS, "bytes": int(len(blob)), "steps": STEPS,
              "warmup": WARMUP, "ms_per_call_median": med, "ms_per_call_min": float(np.min(ms)),
              "ms_per_call_max": float(np.max(ms)), "rows_per_s_median": N_ROWS / med * 1e3,
              "bytes_per_s_median": len(blob) / med * 1e3,
              "last_call_rows_with_a_flag": int((p != 0).sum()), "last_call_nonascii_rows": int(st.sum().item()),
              "last_call_mean_total_text_length": float(feat[:, 2].mean().item())})
        del d_blob, d_off
    eng.close()


if __name__ == "__main__":
    main()
