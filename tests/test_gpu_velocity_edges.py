"""GPU parity of the feature kernels (csrc/features.hip) on the velocity edge streams of
tests/velocity_edge_cases.py: events exactly W - 1, W, 0 and -1 ms from a prior event of the card at every code
site (incremental windows, full scans, the rebuild, the cooperative path and the carry out of it, the oversized
bucket's passes), session gaps of exactly one TTL and one more, full-ring overwrites under a spanning window,
negative event times. tests/test_velocity_edges_cpu.py proves on the CPU that the streams hold those edges and that
an off-by-one at any of them would change rows.

Against the sequential C oracle batch by batch, the bars of tests/test_gpu_features_segments.py: raw features
bit-exact (column 1 within 1 f64 ulp), vectors bit-exact except slot 1 within 1 f32 ulp, in sliding mode the
window_saturated counter; then the LSTM history the cooperative path moves through LDS, and the pipelined stream
(lean bucket kernel, its groupings and row forms) against a twin serial engine bit for bit."""
import numpy as np
import pytest

import velocity_edge_cases as V
from test_gpu_features_segments import _check, _run
from test_gpu_pipeline import _run as _run_pipelined

pytestmark = pytest.mark.gpu


def _host(engine, mode, K, layout, slot_gather):
    tx, cuts = V.stream(layout, K)
    engine.set_option("slot_gather", slot_gather)
    try:
        orc = V.oracle_pair(engine, mode, K)
        _run(engine, orc, tx, cuts)
    finally:
        engine.set_option("slot_gather", 1)


@pytest.mark.parametrize("slot_gather", [1, 0], ids=["gather", "slot_bucket"])
@pytest.mark.parametrize("mode", [0, 1], ids=["redis_compat", "sliding"])
@pytest.mark.parametrize("layout", V.LAYOUTS)
@pytest.mark.parametrize("K", [3, 16])
def test_edge_stream_host_path(engine, K, layout, mode, slot_gather):
    """engine.features: batches of <= 4096 rows through the gather kernel (slot_gather 1) or the slot pass and
    feat_bucket_kernel (0); the batch with the 4 500-event run always takes the latter and its oversized bucket the
    passes by arrival range"""
    _host(engine, mode, K, layout, slot_gather)


@pytest.mark.parametrize("slot_gather", [1, 0], ids=["gather", "slot_bucket"])
@pytest.mark.parametrize("mode", [0, 1], ids=["redis_compat", "sliding"])
@pytest.mark.parametrize("K", [1, 2, 64])
def test_edge_stream_ring_sizes(engine, K, mode, slot_gather):
    """the smallest rings and the largest (kMaxK) on the layout that reaches every site"""
    _host(engine, mode, K, "mixed", slot_gather)


def test_edge_stream_lstm_history(engine):
    """seq_len = 10: the features as above and every transaction's emitted sequence against the oracle's card
    histories (the cooperative path carries the history through LDS, tile by tile, and writes the ring back)"""
    import torch

    from fdengine._native import TXN_FIELDS
    from oracle import lstm_ref as R
    T, K = 10, 16
    tx, cuts = V.stream("mixed", K)
    orc = V.oracle_pair(engine, 1, K, seq_len=T)
    hist = R.SequenceState(T)
    others = [c for c in range(16) if c != 1]
    try:
        engine.set_stream(torch.cuda.current_stream().cuda_stream)
        for a, b in zip(cuts[:-1], cuts[1:]):
            n = b - a
            part = {k: v[a:b] for k, v in tx.items()}
            dev = {f: torch.from_numpy(np.array(part[f])).cuda() for f in TXN_FIELDS}
            vec = torch.empty((n, 64), dtype=torch.float32, device="cuda")
            raw = torch.empty((n, 16), dtype=torch.float64, device="cuda")
            seq = torch.empty((n, T, 16), dtype=torch.float32, device="cuda")
            engine.features_seq_device({f: t.data_ptr() for f, t in dev.items()}, n, vec.data_ptr(), seq.data_ptr(),
                                       raw.data_ptr())
            torch.cuda.synchronize()
            rraw, rvec = orc.run(part)
            _check(vec.cpu().numpy(), raw.cpu().numpy(), rvec, rraw)
            exp = hist.run(part["card_key"], rraw)
            got = seq.cpu().numpy()
            np.testing.assert_array_max_ulp(got, exp, maxulp=1)
            assert (got[:, :, others] == exp[:, :, others]).all()
    finally:
        engine.set_stream(None)


@pytest.fixture(scope="module")
def forests():
    """XGBoost and IsolationForest over the edge stream's own vectors: the trees split on the count and amount
    slots at the values the windows produce"""
    from fdengine import iforest_from_sklearn, synth, xgboost_from_json_doc
    tx, _ = V.stream("mixed", 16)
    _, X = V.oracle_pair(None, 1, 16).run(tx)
    doc = synth.xgboost_doc(100, 8, 64, X, seed=3)
    used = {int(f) for t in doc["learner"]["gradient_booster"]["model"]["trees"]
            for f, l in zip(t["split_indices"], t["left_children"]) if l != -1}
    assert {14, 15, 16, 31, 32} <= used  # the 1 h / 24 h counts, the 24 h / 1 h amounts, the 5 min count
    ifm = iforest_from_sklearn(synth.isolation_forest(X[::2].astype(np.float64), n_estimators=40))
    return xgboost_from_json_doc(doc), ifm


def _pipe_cases():
    cases = [("mixed", 16, 0, lg, cv) for lg in (0, 1, 2) for cv in (0, 1, 2)]
    cases += [("short", 16, 0, lg, 2) for lg in (0, 1, 2)] + [("short", 16, 0, 2, cv) for cv in (0, 1)]
    cases += [("mixed", 64, 0, lg, 2) for lg in (0, 1, 2)] + [("mixed", 64, 0, 2, cv) for cv in (0, 1)]
    cases += [(layout, K, 1, 2, 2) for layout, K in (("mixed", 16), ("short", 16), ("mixed", 64))]
    return cases


@pytest.mark.timeout(300)
@pytest.mark.parametrize("layout,K,gather,lean_group,compact", _pipe_cases())
def test_edge_stream_pipelined_matches_serial(forests, layout, K, gather, lean_group, compact):
    """fd_score_batch_pipelined on the edge stream against fd_score_batch_device on a twin engine: outputs and end
    state bit for bit. pipeline_gather 0 sends these small batches through the slot pass and the lean bucket kernel
    (`short`: its own grouping, by lean_group; `mixed`: long segments and the hot run through its slow path), 1
    through the gather kernel. compact_vectors picks the form of the fused ensemble kernel's rows; that kernel takes
    batches of more than 32 512 transactions only (fd_internal.h kSplitTiles), so on these streams the option must
    simply change nothing (the compact and split rows themselves are pinned at full batch size by
    tests/test_gpu_pipeline.py). The stream's last two batches are the end-state probe."""
    tx, cuts = V.stream(layout, K)
    _run_pipelined((V.population(), tx) + forests, list(cuts[:-2]), K=K,
                   opts=(("pipeline_gather", gather), ("lean_group", lean_group), ("compact_vectors", compact)))
