#!/usr/bin/env python3
"""Measure the MLP member's fit on the engine (csrc/mlp_fit.hip, FraudEngine.fit_mlp) at two shapes:

 trainer   the drop-in's own shape: 8,000 x 64 scoring-vector rows, 64 -> 64 -> 64 -> 2, 20 epochs of 256, Adam 1e-3,
           dropout 0.1 (ModelTrainer.train_graph_neural_model's fit);
 serving   1 M x 64 rows, 1 epoch of 4,096.

Each timed region is one whole fit from host arrays (staging, every epoch's index array, every step, the copy back),
after a warm-up fit, repeated; the line carries every region, the median and the spread, the steps and the time per step.
Beside them the only other MLP trainers on the machine, same model, data, optimiser and batch size (their own shuffles
and dropout draws; another implementation's wall time, not a parity check):

 torch_gpu  torch eager on the same GPU (device tensors, one host sync at the end);
 torch_cpu  torch on the CPU with the process's thread limit (OMP_NUM_THREADS, 16 where this is run).

Arguments: PART SHAPE, PART in engine | torch_gpu | torch_cpu | resources, SHAPE in trainer | serving. One part per
process: the caller chains them, each under its own time limit, and runs none again. Prints one JSON line and appends
it to profiles/mlp_fit/mlp_fit_bench.jsonl (OUT overrides the path); `resources` writes the mlp_fit kernels' entries of
the build's kernel_resources.json to profiles/mlp_fit/kernel_resources.json."""
import json
import os
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(REPO), str(REPO / "realtime-fraud-detection_amd")]
import numpy as np

OUT = Path(os.environ.get("OUT", REPO / "profiles" / "mlp_fit" / "mlp_fit_bench.jsonl"))
THREADS = int(os.environ.get("OMP_NUM_THREADS", "16"))
SHAPES = {"trainer": dict(n=8000, epochs=20, batch_size=256, regions=5),
          "serving": dict(n=1_000_000, epochs=1, batch_size=4096, regions=3)}
HP = dict(hidden=64, n_layers=3, dropout=0.1, lr=1e-3)


def emit(line):
    print(json.dumps(line), flush=True)
    OUT.parent.mkdir(parents=True, exist_ok=True)
    with open(OUT, "a") as f:
        f.write(json.dumps(line) + "\n")


def data(n):
    from fdengine import synth
    X = synth.feature_matrix(n, 64, seed=11)
    rng = np.random.Generator(np.random.PCG64(12))
    Z = np.nan_to_num(X[:, :8].astype(np.float64))
    Z = (Z - Z.mean(0)) / (Z.std(0) + 1e-12)
    s = Z @ np.array([0.9, 0.7, -0.5, 0.4, 0.3, 0.3, -0.2, 0.2]) + rng.normal(0.0, 1.0, n)
    return np.ascontiguousarray(X, np.float32), (s > np.quantile(s, 0.95)).astype(np.uint8)


def timed(fit, regions):
    fit()
    out = []
    for _ in range(regions):
        t0 = time.perf_counter()
        res = fit()
        out.append(time.perf_counter() - t0)
    return out, res


def line(part, shape, cfg, secs, extra):
    steps = cfg["epochs"] * -(-cfg["n"] // cfg["batch_size"])
    med = float(np.median(secs))
    return dict(part=part, shape=shape, n=cfg["n"], epochs=cfg["epochs"], batch_size=cfg["batch_size"], steps=steps,
                regions_s=[round(s, 4) for s in secs], median_s=round(med, 4),
                spread=round((max(secs) - min(secs)) / med, 3), us_per_step=round(med / steps * 1e6, 1), **extra)


def run_engine(shape, cfg):
    import fdengine
    X, y = data(cfg["n"])
    eng = fdengine.FraudEngine(0)
    try:
        l0 = eng.counter("mlp_fit_launches")
        secs, w = timed(lambda: eng.fit_mlp(X, y, epochs=cfg["epochs"], batch_size=cfg["batch_size"], seed=1, **HP),
                        cfg["regions"])
        launches = (eng.counter("mlp_fit_launches") - l0) // (cfg["regions"] + 1)
        emit(line("engine", shape, cfg, secs, dict(launches=launches, loss_first=float(w.meta["loss_curve"][0]),
                                                   loss_last=float(w.meta["loss_curve"][-1]))))
    finally:
        eng.close()


def run_torch(shape, cfg, device):
    import torch
    import torch.nn.functional as F
    torch.set_num_threads(THREADS)
    X, y = data(cfg["n"])
    n, bs = cfg["n"], cfg["batch_size"]

    def fit():
        torch.manual_seed(1)
        x = torch.from_numpy(X).to(device)
        t = torch.from_numpy(y.astype(np.int64)).to(device)
        layers = [torch.nn.Linear(64, 64), torch.nn.Linear(64, 64), torch.nn.Linear(64, 2)]
        model = torch.nn.Sequential(layers[0], torch.nn.ReLU(), torch.nn.Dropout(0.1), layers[1], torch.nn.ReLU(),
                                    torch.nn.Dropout(0.1), layers[2]).to(device)
        opt = torch.optim.Adam(model.parameters(), lr=1e-3)
        model.train()
        losses = []
        for _ in range(cfg["epochs"]):
            perm = torch.randperm(n, device=device)
            tot = torch.zeros((), device=device)
            for j in range(0, n, bs):
                rows = perm[j:j + bs]
                opt.zero_grad(set_to_none=True)
                loss = F.cross_entropy(model(x[rows]), t[rows])
                loss.backward()
                opt.step()
                tot += loss.detach()
            losses.append(tot)
        return [float(v) / -(-n // bs) for v in losses]  # (the one wait for the device)

    secs, losses = timed(fit, max(2, cfg["regions"] - 2))
    emit(line("torch_gpu" if device != "cpu" else "torch_cpu", shape, cfg, secs,
              dict(threads=THREADS if device == "cpu" else None, loss_first=losses[0], loss_last=losses[-1])))


def run_resources():
    from fdengine.build import RESOURCES
    res = {k: v for k, v in json.loads(RESOURCES.read_text()).items() if "mlp_fit" in k}
    path = OUT.parent / "kernel_resources.json"
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text(json.dumps(res, indent=0, sort_keys=True) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    part = sys.argv[1] if len(sys.argv) > 1 else "engine"
    shape = sys.argv[2] if len(sys.argv) > 2 else "trainer"
    if part == "resources":
        run_resources()
    elif part == "engine":
        run_engine(shape, SHAPES[shape])
    elif part == "torch_gpu":
        run_torch(shape, SHAPES[shape], "cuda:0")
    elif part == "torch_cpu":
        run_torch(shape, SHAPES[shape], "cpu")
    else:
        raise SystemExit(f"unknown part {part!r}")
