"""Device memory goes with its owner (csrc/fd_internal.h DeviceBuffer, ~Engine; DESIGN §1 "Lifetime and ownership"),
held to the counter "device_bytes_live": the bytes the library holds through DeviceBuffer, over every engine of the
process. Every test builds its own engine; the session engine only reads the counter (it is process-wide, so it reads
the same through any engine, also after the engine under test is gone).

* destroying an engine that has used every owner returns the counter to its value before the engine existed;
* a repeated load / query / checkpoint call holds no more after the third call than after the first;
* load, predict, unload of a forest is a closed cycle, and unload alone returns what load took;
* a call that fails (an error status: "card table full") holds no more after the third failure than after the first.

Shapes: 300 rows (two tiles, the second ragged) wherever a kernel only has to run; 32 768 rows (128 tiles) where the
fused ensemble kernel has to — it takes batches of at least 128 tiles (fd_internal.h kSplitTiles), and only it builds
the joint plans (EnsemblePlan: nodes, contracted nodes, table image) — checked by its launch counters."""
import numpy as np
import pytest

import text_cases as T
from fdengine import (FraudEngine, forest_from_sklearn_classifier, iforest_from_sklearn, synth,
                      xgboost_from_json_doc)
from fdengine import _native as N
from fdengine import lstm as L
from fdengine import mlp as M
from fdengine.ingest import IngestCodec

pytestmark = pytest.mark.gpu

N_SMALL, N_FUSED = 300, 32768


def live(reader) -> int:
    return reader.counter("device_bytes_live")


@pytest.fixture(scope="module")
def world():
    X = synth.feature_matrix(N_FUSED, 64, seed=31)
    X.setflags(write=False)
    pop = synth.population(256, 16, seed=32)
    tx = synth.txn_stream(pop, N_FUSED + N_SMALL, seed=33, rate_per_s=100.0, unknown_user_frac=0.0)
    ref = X[:2048]
    return {
        "X": X, "pop": pop, "tx": tx,
        "xgb": xgboost_from_json_doc(synth.xgboost_doc(8, 4, 64, ref, seed=34, p_leaf=0.1)),
        "ifm": iforest_from_sklearn(synth.isolation_forest(ref.astype(np.float64), n_estimators=8)),
        "deep": xgboost_from_json_doc(synth.xgboost_doc(2, 12, 64, ref, seed=35)),  # deeper than 10: sparse layout only
        "proba": forest_from_sklearn_classifier(synth.random_forest(ref, n_estimators=5, random_state=36)),
    }


def _state(eng, pop, capacity=1024):
    U, Mr = pop["users"], pop["merchants"]
    eng.state_init(capacity, N.FD_WINDOW_SLIDING, 4, 4)
    eng.load_users(U["key"], U["avg_amount"], U["account_age_days"], U["device_fp"])
    eng.load_merchants(Mr["fraud_rate"], Mr["risk_multiplier"])


def _users_ext(eng, pop):
    ue = synth.users_ext(pop)
    eng.load_users_ext(ue["key"], **{k: v for k, v in ue.items() if k != "key"})


def _pair_params():
    from oracle import scoring_ref as S
    names = ["xgboost_primary", "isolation_forest"]
    w = S.normalized_weights({"xgboost_primary": 0.4, "isolation_forest": 0.05})
    return FraudEngine.blend_params([w[k] for k in names], [S.CONF_MULT[k] for k in names])


def _pipelined(eng, tx, lo, n):
    """one pipelined XGBoost + IsolationForest batch of rows [lo, lo + n), no vectors asked for"""
    import torch
    dev = {f: torch.from_numpy(np.ascontiguousarray(tx[f][lo:lo + n])).cuda() for f in N.TXN_FIELDS}
    out = [torch.empty(n, dtype=t, device="cuda") for t in (torch.float64, torch.float64, torch.uint8, torch.uint8)]
    torch.cuda.synchronize()
    eng.score_batch_pipelined(_pair_params(), [0, 1], {f: t.data_ptr() for f, t in dev.items()}, n,
                              *[o.data_ptr() for o in out])
    eng.sync()
    return dev


def _touch_every_owner(B, w, tmp_path):
    import torch
    X, pop, tx = w["X"], w["pop"], w["tx"]
    _state(B, pop)
    _users_ext(B, pop)
    me = synth.merchants_ext(pop)
    B.load_merchants_ext(len(pop["merchants"]["category"]), **me)
    B.load_vocab(*synth.vocab_flags())
    IngestCodec(B, ["m1", "m2"], ["visa"], ["purchase"], ["debit"])
    B.load_forest(0, w["xgb"])
    B.load_forest(1, w["ifm"])
    B.load_forest(2, w["deep"])
    for v in (0, 6, 8, 11):  # auto, the split scratch, the node-only chunks, the sparse image
        B.set_option("forest_kernel", v)
        for slot in (0, 1)[:1 if v == 8 else 2]:  # this IsolationForest has no node-only layout
            B.predict(slot, X[:N_SMALL], want_raw=True, want_leaf=True)
    B.set_option("forest_kernel", 0)
    B.predict(2, X[:N_SMALL])
    assert B.counter("forest_sparse_launches") >= 3
    # the pipelined stream (its rings) and the pair plan: contracted and dense, then uncontracted
    for contract in (4, 0):
        B.set_option("ensemble_contract", contract)
        _pipelined(B, tx, 0, N_SMALL)
        _pipelined(B, tx, N_SMALL, N_FUSED)
    assert B.counter("pipelined_batches") == 4 and B.counter("pipelined_compact_batches") >= 2
    assert B.counter("ensemble_contracted_launches") >= 1
    # one forest through the fused kernel: its per-slot plan
    B.set_option("ensemble", 1)
    B.predict(0, X[:N_SMALL])
    B.predict(0, X)
    assert B.counter("ensemble_single_launches") >= 1
    B.explain(0, X[:8])
    B.load_lstm(L.random_weights(16, 128, 1, seed=37))
    B.lstm_predict(np.zeros((8, 4, 16), np.float32))
    B.load_mlp(M.random_weights(seed=38))
    B.mlp_predict(synth.feature_matrix(8, 64, seed=39))
    k, ts, cents, mer = (tx[f][:N_SMALL] for f in ("card_key", "ts_ms", "amount_cents", "merchant"))
    B.windows_init(4096)
    B.windows_step_host(k, ts, cents, mer, flush=True)
    B.sink_init(1 << 10, 1 << 10)
    B.sink_update_host(k, ts, cents, mer)
    hour = int(ts[0] // 3_600_000)
    B.sink_query(N.FD_AGG_HOURLY, [hour])
    B.sink_evict_before(hour)
    B.graph_init(64)
    B.graph_step(k, mer, cents)
    B.text_features(*T.encode([T.row("amazon", "gift card", "retail", "NY")] * 3))
    B.ab_create(0, 123, 50.0)
    variant = B.ab_assign(0, k)
    B.ab_record(0, variant, np.full(N_SMALL, 0.25), np.zeros(N_SMALL, np.uint8), 1.0)
    B.metrics_init(2, 64)
    B.metrics_record(np.full(N_SMALL, 0.25), np.zeros(N_SMALL, np.uint8), None, 1.0, 1000.0)
    B.metrics_query(1000.0)
    Xf = np.ascontiguousarray(X[:256, :4])
    B.fit_gbdt(Xf, (Xf[:, 0] > 0).astype(np.uint8), n_rounds=2, max_depth=2)
    B.fit_iforest(Xf, n_estimators=4, contamination=0.1)  # a contamination: the fit's scorer forest too
    dev = {f: torch.from_numpy(np.ascontiguousarray(tx[f][:N_SMALL])).cuda() for f in N.TXN_FIELDS}
    records = torch.empty(N_SMALL * N.FD_ROUTE_RECORD_BYTES, dtype=torch.uint8, device="cuda")
    counts = torch.empty(2, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    B.route_partition_device({f: t.data_ptr() for f, t in dev.items()}, N_SMALL, 2, records.data_ptr(),
                             counts.data_ptr())
    B.sync()
    B.state_snapshot(tmp_path / "b.fdsnap")
    B.state_restore(tmp_path / "b.fdsnap")


def test_destroy_returns_everything(engine, world, tmp_path):
    base = live(engine)
    B = FraudEngine(0)
    try:
        _touch_every_owner(B, world, tmp_path)
        held = live(engine)
        print(f"base {base}, with the engine {held} ({held - base} bytes held)")
        assert held > base
    finally:
        B.close()
    after = live(engine)
    print(f"after destroy {after} ({after - base} bytes not returned)")
    assert after == base


def _snapshot_engine(eng, w):
    _state(eng, w["pop"])
    tx = w["tx"]
    eng.sink_init(1 << 10, 1 << 10)
    eng.sink_update_host(*(tx[f][:N_SMALL] for f in ("card_key", "ts_ms", "amount_cents", "merchant")))


REPEATED = {
    "load_users": lambda e, w, p: e.load_users(*(w["pop"]["users"][f][:3] for f in
                                                 ("key", "avg_amount", "account_age_days", "device_fp"))),
    "load_users_ext": lambda e, w, p: _users_ext(e, w["pop"]),
    "state_info": lambda e, w, p: e.state_info(),
    "sink_query": lambda e, w, p: e.sink_query(N.FD_AGG_HOURLY, [int(w["tx"]["ts_ms"][0] // 3_600_000)]),
    "sink_evict_before": lambda e, w, p: e.sink_evict_before(int(w["tx"]["ts_ms"][0] // 3_600_000)),
    "snapshot": lambda e, w, p: e.state_snapshot(p),
    "restore": lambda e, w, p: e.state_restore(p),
}


@pytest.mark.parametrize("call", sorted(REPEATED))
def test_repeated_calls_do_not_accumulate(engine, world, tmp_path, call):
    """the engine's own scratch grows to a high-water mark on the first call and stays; nothing else may"""
    path = tmp_path / "r.fdsnap"
    B = FraudEngine(0)
    try:
        _snapshot_engine(B, world)
        if call == "restore":
            B.state_snapshot(path)
        REPEATED[call](B, world, path)
        c1 = live(engine)
        REPEATED[call](B, world, path)
        REPEATED[call](B, world, path)
        c2 = live(engine)
        print(f"{call}: {c1} after the first call, {c2} after the third ({c2 - c1} bytes kept by two calls)")
        assert c2 == c1
    finally:
        B.close()


@pytest.mark.parametrize("kind", ["heap_xgb", "deep_sparse", "sklearn_proba"])
def test_load_predict_unload_is_a_closed_cycle(engine, world, kind):
    fa = world[{"heap_xgb": "xgb", "deep_sparse": "deep", "sklearn_proba": "proba"}[kind]]
    X = world["X"][:N_SMALL]
    B = FraudEngine(0)
    try:
        if kind == "heap_xgb":
            B.set_option("forest_kernel", 8)  # the node-only chunks and their leaf array are read

        def cycle():
            B.load_forest(0, fa)
            B.predict(0, X)
            before = live(engine)
            B.unload_forest(0)
            after = live(engine)
            assert after < before
            return after

        # unload returns what load took (no predict between them: no engine scratch grows)
        c0 = live(engine)
        B.load_forest(0, fa)
        loaded = live(engine)
        B.unload_forest(0)
        c_unloaded = live(engine)
        print(f"{kind}: load took {loaded - c0} bytes, unload left {c_unloaded - c0} of them")
        assert loaded > c0 and c_unloaded == c0
        c1 = cycle()  # warm: the staging scratch of the host predict grows once
        c2 = cycle()
        print(f"{kind}: {c1} after the warm cycle, {c2} after the next ({c2 - c1} bytes kept)")
        assert c2 == c1
    finally:
        B.close()


def test_a_failing_call_frees_its_locals(engine, world):
    """16 distinct cards into a table of 8 slots: fd_state_load_users_host reports "card table full" (an error status of
    the load kernel, tests/test_gpu_features.py::test_table_full_is_reported) after its staging buffers were allocated"""
    U = synth.population(16, 2, seed=40)["users"]
    B = FraudEngine(0)
    try:
        B.state_init(8, N.FD_WINDOW_SLIDING, 4, 4)

        def fail():
            with pytest.raises(Exception, match="card table full"):
                B.load_users(U["key"], U["avg_amount"], U["account_age_days"], U["device_fp"])

        fail()
        c1 = live(engine)
        fail()
        fail()
        c2 = live(engine)
        print(f"{c1} after the first failure, {c2} after the third ({c2 - c1} bytes kept by two failures)")
        assert c2 == c1
    finally:
        B.close()
