#!/usr/bin/env python3
"""Measure the MLP head's kernel (csrc/mlp.hip) alone, in ONE process: the reference shape (64 -> 64 -> 64 -> 2) at a
64 k x 64 batch resident in HBM.

 * us per launch from the engine's timing (FD_TIMING_MLP: HIP events around the kernel): ROUNDS rounds of REPS timed
   launches after 3 warm-up launches each, the median and the minimum of the rounds' means;
 * the same call in torch fp32 on this host's CPU with JOBS threads (the reference's library and dtype), wall time;
 * max |dp| between the two, and the two computed floors the measured time stands beside:
   HBM   B x (in_dim x 4 + 8) bytes at the achievable 6.3 TB/s (MI355X_MICROARCH: float4 copy),
   MFMA  2 x (64 x 64 x 2 + 64 x 16) x B FLOP (the output layer padded to 16 units) at the f32 MFMA's 155 TF.

Prints one JSON line and appends it to OUT (default profiles/mlp/mlp_bench.jsonl). Environment: B (batch, default
65536), JOBS (default 16), OUT."""
import json
import os
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

B = int(os.environ.get("B", 65536))
JOBS = int(os.environ.get("JOBS", 16))
OUT = Path(os.environ.get("OUT", REPO / "profiles" / "mlp" / "mlp_bench.jsonl"))
ROUNDS, REPS = 5, 20
HBM_BPS = 6.3e12
MFMA_F32_FLOPS = 155e12


def torch_forward(w, x):
    import torch.nn.functional as F
    with torch.no_grad():
        for i in range(w.n_layers):
            x = F.linear(x, torch.from_numpy(w.weights[i]), torch.from_numpy(w.biases[i]))
            if i + 1 < w.n_layers:
                x = torch.relu(x)
        return torch.softmax(x, dim=1)[:, 1]


def main():
    eng = fdengine.FraudEngine(0)
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    w = M.random_weights(64, 64, 3, seed=1)
    eng.load_mlp(w)
    g = torch.Generator().manual_seed(7)
    X = torch.randn(B, 64, generator=g) * 3
    X[:, :32] = X[:, :32].abs().clamp(max=10)
    dX = X.cuda()
    dp = torch.empty(B, dtype=torch.float64, device="cuda")
    us = []
    c0 = eng.counter("mlp_launches")
    for _ in range(ROUNDS):
        for _i in range(3):
            eng.mlp_predict_device(dX.data_ptr(), B, 64, dp.data_ptr())
        torch.cuda.synchronize()
        eng.read_timing(N.FD_TIMING_MLP)
        eng.set_timing(True)
        for _i in range(REPS):
            eng.mlp_predict_device(dX.data_ptr(), B, 64, dp.data_ptr())
        torch.cuda.synchronize()
        eng.set_timing(False)
        ms, n = eng.read_timing(N.FD_TIMING_MLP)
        assert n == REPS, (ms, n)
        us.append(ms / n * 1e3)
    assert eng.counter("mlp_launches") - c0 == ROUNDS * (REPS + 3)
    got = dp.cpu().numpy()
    eng.close()

    torch.set_num_threads(JOBS)
    torch_forward(w, X[:1024])
    cpu = []
    for _ in range(5):
        t0 = time.perf_counter()
        ref = torch_forward(w, X)
        cpu.append(time.perf_counter() - t0)
    ref = ref.numpy().astype(np.float64)

    med = float(np.median(us))
    hbm_bytes = B * (64 * 4 + 8)
    flop = 2 * (64 * 64 * 2 + 64 * 16) * B
    hbm_us, mfma_us = hbm_bytes / HBM_BPS * 1e6, flop / MFMA_F32_FLOPS * 1e6
    line = json.dumps({"kernel": "mlp_kernel", "shape": [64, 64, 64, 2], "batch": B, "rounds": ROUNDS, "reps": REPS,
                       "us_per_launch_median": med, "us_per_launch_min": float(np.min(us)),
                       "txn_per_s": B / (med * 1e-6), "hbm_bytes": hbm_bytes, "hbm_floor_us": hbm_us, "flop": flop,
                       "mfma_f32_floor_us": mfma_us, "binding_floor": "mfma_f32" if mfma_us > hbm_us else "hbm",
                       "times_binding_floor": med / max(hbm_us, mfma_us),
                       "torch_cpu_fp32_us_threads_%d" % JOBS: float(np.median(cpu)) * 1e6,
                       "max_abs_dp_vs_torch_cpu": float(np.abs(got - ref).max())})
    print(line)
    OUT.parent.mkdir(parents=True, exist_ok=True)
    with open(OUT, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
