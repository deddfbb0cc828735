#!/usr/bin/env python3
"""Measure forest attribution (csrc/shap.hip, fd_forest_shap_device) at the headline forests, in ONE process:

  XGBoost 500 trees x depth 8 and IsolationForest 100 trees (max_samples 256), 64 features, covers from a background
  set; for each: 1 k rows, 64 k rows, and a 5 % row subset of the 64 k batch (d_rows).

Per case one JSON line: ms per call (median and min over rounds of device-event timings on the engine's stream),
rows/s, and the f64 operations the path form needs per row (counted from the path table: a path of m unique features
costs m (m + 1) / 2 + m multiply-adds for the polynomial, m for the shared sum and 2 m - 1 per element for the
divided one; an FMA counts 2) over the kernel time, as a share of the MI355X's published vector-f64 peak
(78.6 TFLOP/s). The share is an end-to-end figure of the explain call (two launches per 4096 rows), not a profile.
Environment: ROUNDS (default 5)."""
import json
import os
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(REPO), str(REPO / "realtime-fraud-detection_amd")]
import ctypes as C

import numpy as np
import torch

import fdengine
from fdengine import _native as N
from fdengine import synth

F = 64
B = 65536
ROUNDS = int(os.environ.get("ROUNDS", 5))
PEAK_F64 = 78.6e12


def covers_from_leaves(fa, leaf):
    """1 + the background rows per leaf (leaf: [n, T] node ids from the engine's own walk), parents = sum of children"""
    cover = np.zeros(len(fa.left), np.float64)
    for t, a in enumerate(fa.offsets[:-1]):
        m = int(fa.offsets[t + 1] - a)
        c = np.bincount(leaf[:, t], minlength=m).astype(np.float64)
        is_leaf = fa.left[a:a + m] < 0
        c[is_leaf] += 1.0
        c[~is_leaf] = 0.0
        for o in range(m - 1, -1, -1):  # both libraries number a child after its parent
            if not is_leaf[o]:
                c[o] = c[fa.left[a + o]] + c[fa.right[a + o]]
        cover[a:a + m] = c
    return cover


def flops_per_row(fa):
    paths, _, info = fdengine.shap_paths_host(fa)
    m = paths["len"].astype(np.float64)
    fma = m * (m + 1) / 2 + m + m + m * np.maximum(2 * m - 1, 0)
    return float(2 * fma.sum()), info


def time_call(eng, slot, dX, n, rows, dphi):
    nr = n if rows is None else int(rows.numel())
    args = (eng.handle, slot, C.c_void_p(dX.data_ptr()), n, F, C.c_void_p(rows.data_ptr()) if rows is not None else None,
            nr, C.c_void_p(dphi.data_ptr()), F + 1)
    N.call("fd_forest_shap_device", *args)  # warm: builds the table, loads the code object
    torch.cuda.synchronize()
    out = []
    for _ in range(ROUNDS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        N.call("fd_forest_shap_device", *args)
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return out, nr


def main():
    eng = fdengine.FraudEngine(0)
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    bg = synth.feature_matrix(4096, F, seed=7)
    X = synth.feature_matrix(B, F, seed=1000)
    dX = torch.from_numpy(X).cuda()
    dphi = torch.empty((B, F + 1), dtype=torch.float64, device="cuda")
    rng = np.random.Generator(np.random.PCG64(5))
    subset = torch.from_numpy(np.sort(rng.choice(B, B // 20, replace=False)).astype(np.int64)).cuda()
    models = {
        "xgboost_500x8": fdengine.xgboost_from_json_doc(synth.xgboost_doc(500, 8, F, bg, seed=8)),
        "isolation_forest_100": fdengine.iforest_from_sklearn(synth.isolation_forest(bg.astype(np.float64))),
    }
    for slot, (name, fa) in enumerate(models.items()):
        fa.cover = None
        eng.load_forest(slot, fa)
        _, _, leaf = eng.predict(slot, bg, want_raw=True, want_leaf=True)
        fa.cover = covers_from_leaves(fa, leaf)
        eng.set_cover(slot, fa.cover)
        flops, info = flops_per_row(fa)
        for case, n, rows in (("1k", 1024, None), ("64k", B, None), ("64k_subset_5pct", B, subset)):
            c0 = eng.counter("forest_shap_launches")
            ms, nr = time_call(eng, slot, dX, n, rows, dphi)
            launches = (eng.counter("forest_shap_launches") - c0) // (ROUNDS + 1)
            med = float(np.median(ms))
            phi = dphi[:min(nr, 256)].cpu().numpy()
            print(json.dumps({"model": name, "case": case, "rows": nr, "batch": n, "trees": fa.n_trees,
                              "paths": int(info.n_paths), "max_path": int(info.max_len), "chunks": int(info.n_chunks),
                              "launches_per_call": int(launches), "ms_median": med, "ms_min": float(np.min(ms)),
                              "rows_per_s": nr / (med * 1e-3), "f64_flop_per_row": flops,
                              "f64_flop_per_s": flops * nr / (med * 1e-3),
                              "share_of_vector_f64_peak": flops * nr / (med * 1e-3) / PEAK_F64,
                              "phi_finite": bool(np.isfinite(phi).all())}), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
