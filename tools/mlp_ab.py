#!/usr/bin/env python3
"""A/B of the MLP head's kernel forms on the reference shape (64 -> 64 -> 64 -> 2), ONE process, interleaved rounds:
option mlp_form (0 weights in registers, 1 weights in LDS) x option mlp_wgs_per_cu (the persistent grid's workgroups
per CU, 0 auto), at 16 / 1,024 / 16,384 / 65,536 rows: us per launch from the engine's timing (FD_TIMING_MLP), the
median of ROUNDS rounds of REPS launches after 3 warm-up launches each; then the wall time per launch of 500
back-to-back untimed launches. Prints one JSON line per variant (profiles/mlp/mlp_ab.txt)."""
import json
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(REPO), str(REPO / "realtime-fraud-detection_amd")]
import numpy as np
import torch

import fdengine
from fdengine import _native as N
from fdengine import mlp as M

B = 65536
ROUNDS, REPS = 4, 20
VARIANTS = [(0, 0), (0, 1), (1, 1), (1, 2), (1, 3), (1, 4)]  # (mlp_form, mlp_wgs_per_cu)
SIZES = (16, 1024, 16384, 65536)


def main():
    eng = fdengine.FraudEngine(0)
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    eng.load_mlp(M.random_weights(64, 64, 3, seed=1))
    dX = (torch.randn(B, 64) * 3).cuda()
    dp = torch.empty(B, dtype=torch.float64, device="cuda")

    def launch(n):
        eng.mlp_predict_device(dX.data_ptr(), n, 64, dp.data_ptr())

    def timed(n):
        for _ in range(3):
            launch(n)
        torch.cuda.synchronize()
        eng.read_timing(N.FD_TIMING_MLP)
        eng.set_timing(True)
        for _ in range(REPS):
            launch(n)
        torch.cuda.synchronize()
        eng.set_timing(False)
        ms, c = eng.read_timing(N.FD_TIMING_MLP)
        assert c == REPS
        return ms / c * 1e3

    res = {v: {} for v in VARIANTS}
    for _ in range(ROUNDS):
        for v in VARIANTS:
            eng.set_option("mlp_form", v[0])
            eng.set_option("mlp_wgs_per_cu", v[1])
            for n in SIZES:
                res[v].setdefault(n, []).append(timed(n))
    for v in VARIANTS:
        print(json.dumps({"form": v[0], "wgs_per_cu": v[1],
                          **{str(n): round(float(np.median(x)), 2) for n, x in res[v].items()}}))
    for v in ((0, 0), (1, 2)):
        eng.set_option("mlp_form", v[0])
        eng.set_option("mlp_wgs_per_cu", v[1])
        for _ in range(10):
            launch(B)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(500):
            launch(B)
        torch.cuda.synchronize()
        print(json.dumps({"form": v[0], "wgs_per_cu": v[1],
                          "back_to_back_us": (time.perf_counter() - t0) / 500 * 1e6}))
    eng.close()


if __name__ == "__main__":
    main()
