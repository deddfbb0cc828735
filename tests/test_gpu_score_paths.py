"""The scoring scheduler's choices (csrc/score.hip: score_matrix, score_batch_body, pipe_step) at the batch sizes and
model sets where they flip: every combination of the engine options small_streams {0, 1, 2} and latency_fused {0, 1}
(with the LSTM head also latency_prebin {0, 3}) gives all five outputs bit for bit equal to the same call on a second
engine set to the plain per-model route (ensemble 0, small_streams 0, latency_fused 0, latency_prebin 0). The
per-model route itself is pinned to the CPU oracle by the forest, LSTM, MLP and blend tests.

Sizes: 1, 255, 257 (either side of one 256-row tile), 32512 (127 tiles: the last latency batch), 32513 (128 tiles:
the first large one, where the fused ensemble kernel applies); the pipelined step also 4096 and 4097 (either side of
the gather bucket kernel's limit). Model sets: two forests; two forests with one hidden by `present`; three forests
(where side streams 1 and 2 carry the other forests); two forests + the MLP slot + an external column; two forests +
the LSTM head (through fd_score_batch_device and fd_score_batch_pipelined, which supply the sequences).
Reference chain: ml/models/ensemble_predictor.py:75-148 (predict over the loaded models, then the blend)."""
import itertools

import numpy as np
import pytest

from fdengine import FraudEngine, iforest_from_sklearn, synth, xgboost_from_json_doc
from fdengine import lstm as L
from fdengine import mlp as M
from fdengine._native import FD_SLOT_LSTM, FD_SLOT_MLP, TXN_FIELDS

pytestmark = pytest.mark.gpu

SIZES = [1, 255, 257, 32512, 32513]
PIPE_SIZES = [1, 255, 257, 4096, 4097, 32512, 32513]
PLAIN = {"ensemble": 0, "small_streams": 0, "latency_fused": 0, "latency_prebin": 0}
OPTIONS = [{"small_streams": s, "latency_fused": f} for s, f in itertools.product((0, 1, 2), (0, 1))]
OPTIONS_LSTM = [dict(o, latency_prebin=p) for o in OPTIONS for p in (0, 3)]

# model set -> (slots, present, index of the external column or None)
SETS = {
    "two_forests": ([0, 1], None, None),
    "one_hidden": ([0, 1], [1, 0], None),
    "three_forests": ([0, 1, 2], None, None),
    "mlp_and_external": ([0, 1, FD_SLOT_MLP, -1], None, 3),
}


def _params(n_models):
    w = np.array([0.4, 0.05, 0.3, 0.25][:n_models])
    return FraudEngine.blend_params(list(w / w.sum()), [1.0, 0.8, 0.9, 0.7][:n_models])


@pytest.fixture(scope="module")
def world():
    Xr = synth.feature_matrix(2048, 64, seed=3)
    forests = [xgboost_from_json_doc(synth.xgboost_doc(12, 4, 64, Xr, seed=4)),
               iforest_from_sklearn(synth.isolation_forest(Xr.astype(np.float64), n_estimators=12, max_samples=16)),
               xgboost_from_json_doc(synth.xgboost_doc(12, 4, 64, Xr, seed=5))]
    X = synth.feature_matrix(max(SIZES), 64, seed=6)
    ext = np.random.Generator(np.random.PCG64(7)).random(max(SIZES))
    pop = synth.population(1500, 300, seed=8)
    tx = synth.txn_stream(pop, sum(PIPE_SIZES), seed=9, rate_per_s=50.0)
    return {"forests": forests, "X": X, "ext": ext, "pop": pop, "tx": tx,
            "mlp": M.random_weights(seed=10), "lstm": L.random_weights(seed=11)}


def _engine(world, n_forests, options, mlp=False, state=False, lstm=False):
    eng = FraudEngine(0)
    for s in range(n_forests):
        eng.load_forest(s, world["forests"][s])
    if mlp:
        eng.load_mlp(world["mlp"])
    if state:
        U, Mr = world["pop"]["users"], world["pop"]["merchants"]
        eng.state_init(1 << 12, 1, 16, seq_len=10 if lstm else 0)
        eng.load_users(U["key"], U["avg_amount"], U["account_age_days"], U["device_fp"])
        eng.load_merchants(Mr["fraud_rate"], Mr["risk_multiplier"])
        if lstm:
            eng.load_lstm(world["lstm"])
    for k, v in options.items():
        eng.set_option(k, v)
    return eng


@pytest.mark.timeout(200)
@pytest.mark.parametrize("name", list(SETS))
def test_score_matrix_routes_identical(world, name):
    slots, present, ext_at = SETS[name]
    params = _params(len(slots))
    n_forests = sum(0 <= s < 64 for s in slots)
    ref = _engine(world, n_forests, PLAIN, mlp=FD_SLOT_MLP in slots)
    var = _engine(world, n_forests, {}, mlp=FD_SLOT_MLP in slots)
    try:
        for n in SIZES:
            X = world["X"][:n]
            ext = None if ext_at is None else [world["ext"][:n] if m == ext_at else None for m in range(len(slots))]
            want = ref.score_matrix(params, slots, X, ext_probs=ext, present=present)
            for opt in OPTIONS:
                for k, v in opt.items():
                    var.set_option(k, v)
                got = var.score_matrix(params, slots, X, ext_probs=ext, present=present)
                for out, (g, w) in enumerate(zip(got, want)):
                    if out == 0 and present is not None:  # a hidden model's column is never written
                        g, w = g[np.array(present, bool)], w[np.array(present, bool)]
                    assert np.array_equal(g, w), f"{name} n={n} {opt} output {out}"
    finally:
        ref.close()
        var.close()


def _run_stream(eng, world, params, slots, sizes, pipelined):
    import torch
    dev = {f: torch.from_numpy(np.ascontiguousarray(world["tx"][f])).cuda() for f in TXN_FIELDS}
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    call = eng.score_batch_pipelined if pipelined else eng.score_batch_device
    out, a = [], 0
    for B in sizes:
        fp, conf = (torch.empty(B, dtype=torch.float64, device="cuda") for _ in range(2))
        dec, risk = (torch.empty(B, dtype=torch.uint8, device="cuda") for _ in range(2))
        mp = torch.empty((len(slots), B), dtype=torch.float64, device="cuda")
        call(params, slots, {f: t[a:a + B].data_ptr() for f, t in dev.items()}, B, fp.data_ptr(), conf.data_ptr(),
             dec.data_ptr(), risk.data_ptr(), model_probs_ptr=mp.data_ptr())
        out.append([mp, fp, conf, dec, risk])
        a += B
    eng.sync()
    torch.cuda.synchronize()
    return [[t.cpu().numpy() for t in batch] for batch in out]


def _stream_case(world, slots, sizes, pipelined, options, lstm):
    params = _params(len(slots))
    ref = _engine(world, 2, PLAIN, state=True, lstm=lstm)
    try:
        want = _run_stream(ref, world, params, slots, sizes, pipelined)
    finally:
        ref.close()
    for opt in options:
        var = _engine(world, 2, opt, state=True, lstm=lstm)
        try:
            got = _run_stream(var, world, params, slots, sizes, pipelined)
        finally:
            var.close()
        for B, g_b, w_b in zip(sizes, got, want):
            for out, (g, w) in enumerate(zip(g_b, w_b)):
                assert np.array_equal(g, w), f"n={B} {opt} output {out}"


@pytest.mark.timeout(200)
@pytest.mark.parametrize("pipelined", [False, True], ids=["batch_device", "pipelined"])
def test_lstm_set_routes_identical(world, pipelined):
    """two forests + the LSTM head: the engine's feature kernel supplies the sequences, batch after batch over the
    same card state"""
    _stream_case(world, [0, 1, FD_SLOT_LSTM], PIPE_SIZES if pipelined else SIZES, pipelined, OPTIONS_LSTM, lstm=True)


@pytest.mark.timeout(200)
def test_pipelined_two_forests_routes_identical(world):
    """the pipelined step without the LSTM head: the large batches take the fused kernel over compact / split rows
    (nobody asks for the vectors), the others the latency pair"""
    _stream_case(world, [0, 1], PIPE_SIZES, True, OPTIONS, lstm=False)


@pytest.mark.parametrize("n", [1000, 32513], ids=["latency", "large"])
def test_second_forest_not_loaded(world, n):
    """the second forest's slot is empty: FD_ERR_NOT_LOADED (ValueError in the Python shim) naming the slot, from the
    latency pair path and from a large batch alike"""
    eng = _engine(world, 1, {})
    try:
        with pytest.raises(ValueError, match=r"^Model in slot 5 not loaded$"):
            eng.score_matrix(_params(2), [0, 5], world["X"][:n])
    finally:
        eng.close()
