#!/usr/bin/env python3
"""Generate tests/golden/graph_network_cases.npz by running the REFERENCE's own GraphFraudDetector
(services/ml-models/src/models/graph_neural_network.py) in the build container. Only the input columns and the
five outputs written here travel; the reference never does. Never runs on the GPU machine.

Run:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_graph_golden.py

Reference code exercised (unchanged): _add_transaction_to_history (:228-242) and _calculate_network_features
(:338-392), with the instance attribute max_history_size set per stream. utils.logging_config (structlog) is
registered as a module whose get_logger returns a standard logger.

Streams (tests/graph_cases.py FIXTURE_STREAMS): H in {2, 3, 7, 8, 64, 256, 1000} and one of 10200 rows at the default
H = 10000 that crosses the first truncation (as long as the 256 KB limit on a fixture file allows). About 5 % null users and 5 % null merchants; amounts positive with two
decimals. Coverage asserted per stream: each of the first four columns strictly inside (0, 1) on >= 10 % of rows and
community_anomaly both values on >= 10 % — except clustering_coefficient at H = 2, where no stream can have it: a
window of two entries with dM = 2 holds exactly the user's two pairs, so T = dM and the value is 0.
"""
import importlib.machinery
import logging
import sys
import types
from pathlib import Path

import numpy as np

sys.dont_write_bytecode = True
HERE = Path(__file__).resolve().parent
REF_SRC = Path("/root/reference/services/ml-models/src")
sys.path.insert(0, str(HERE.parent))

import graph_cases as G  # noqa: E402


def reference_class():
    if "utils.logging_config" not in sys.modules:
        for name in ("utils", "utils.logging_config"):
            m = types.ModuleType(name)
            m.__spec__ = importlib.machinery.ModuleSpec(name, None)
            sys.modules[name] = m
        sys.modules["utils"].__path__ = []
        sys.modules["utils.logging_config"].get_logger = logging.getLogger
    sys.path.insert(0, str(REF_SRC))
    from models.graph_neural_network import GraphFraudDetector
    return GraphFraudDetector


def run_reference(cls, user, merchant, cents, H):
    det = cls(device="cpu")
    if H is not None:
        det.max_history_size = H
    out = np.zeros((len(user), 5))
    for i in range(len(user)):
        d = G.txn_dict(user[i], merchant[i], cents[i])
        det._add_transaction_to_history(d)
        f = det._calculate_network_features(d)
        out[i] = [f[c] for c in G.COLUMNS]
    assert det.get_performance_stats()["transaction_history_size"] == G.held_after(len(user), H or G.DEFAULT_H)
    return out


def main():
    cls = reference_class()
    arrays = {}
    for name, (H, n, users, merchants, seed) in G.FIXTURE_STREAMS.items():
        u, m, c = G.make_stream(n, users, merchants, seed)
        out = run_reference(cls, u, m, c, H)
        inside = [float(((out[:, k] > 0) & (out[:, k] < 1)).mean()) for k in range(4)]
        comm = (float((out[:, 4] == 0).mean()), float((out[:, 4] == 1).mean()))
        print(name, "H", H, "rows", n, "inside(0,1)", [round(x, 3) for x in inside], "community 0/1", comm,
              flush=True)
        for k in range(4):
            if H == 2 and k == 2:
                assert inside[k] == 0.0
                continue
            assert inside[k] >= 0.10, (name, G.COLUMNS[k], inside[k])
        assert min(comm) >= 0.10, (name, comm)
        arrays[f"{name}_H"] = np.int32(H or G.DEFAULT_H)
        arrays[f"{name}_user"] = u.astype(np.int16)
        arrays[f"{name}_merchant"] = m.astype(np.int16)
        arrays[f"{name}_cents"] = c.astype(np.int32)
        arrays[f"{name}_out"] = out
    np.savez_compressed(G.GOLDEN, **arrays)
    print("wrote", G.GOLDEN, G.GOLDEN.stat().st_size, "bytes")
    assert G.GOLDEN.stat().st_size <= 256 * 1000


if __name__ == "__main__":
    main()
