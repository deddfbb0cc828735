"""GPU: restored and re-sharded state (csrc/snapshot.hip) against the CPU oracles.

tests/test_gpu_snapshot.py compares a restored engine with the same engine left running; a fault that snapshot and
restore share, or state that both engines get wrong alike, passes there. Here the oracle runs the whole stream
uncut and unsharded, and the engine is replaced at every cut by a fresh FraudEngine of another capacity that calls
only state_init (+ windows_init) and state_restore: profiles, extended profiles, merchants, vocabulary, threshold
and window logs come from the image. Every comparison has an oracle (or the stream itself) on its right-hand side.

The cuts through the velocity edge streams are those of tests/snapshot_cases.py, whose CPU census
(tests/test_snapshot_cases_cpu.py) proves which card states they hold: ring partly filled / exactly full / wrapped
with the head at and off 0, unsorted with the rebuild to come, the first restored event W - 1 / W ms after a ring
event, a session gap of TTL / TTL + 1 across the cut, negative last times and the crossing of ts = 0.

Bars, the project's own: raw features and vectors as tests/test_gpu_features_segments.py `_check`; the feature map
and rules as tests/test_gpu_fmap.py; LSTM sequences <= 1 f32 ulp and exact outside column 1, probabilities 1e-5
(tests/test_gpu_lstm.py); window fields exact (tests/test_gpu_windows.py `_compare`)."""
import functools

import numpy as np
import pytest

import snapshot_cases as S
import velocity_edge_cases as V
import window_edge_cases as WE
from fdengine import FraudEngine, synth
from fdengine._native import CTX_FIELDS, RULE_DTYPE, TXN_FIELDS
from fdengine.engine import shard_of
from oracle import fmap_ref, lstm_ref
from oracle import windows_ref as W
from oracle.features_c import OracleFeatureState
from test_gpu_features_segments import _check
from test_gpu_windows import MF, UF, _compare

pytestmark = pytest.mark.gpu

NO_WM = -(1 << 63)
CAPS = (1 << 15, 3000, 1 << 14, 4096)  # the fresh engines' table capacities: records land in other slots
NOT_LOG = [c for c in range(16) if c != 1]


def _held(loaded, tx, rows):
    """distinct card keys the oracle holds after `rows` rows: the loaded users and the stream's unseen keys"""
    return np.union1d(np.asarray(loaded, np.uint64), np.asarray(tx["card_key"][:rows], np.uint64))


def _part(d, a, b):
    return {k: v[a:b] for k, v in d.items()}


def _dev(part, fields):
    import torch
    return {f: torch.from_numpy(np.ascontiguousarray(part[f])).cuda() for f in fields}


def _full(eng, part, cpart):
    """features_full_device -> vectors, raw, feature map, rule records"""
    import torch
    n = len(part["card_key"])
    dev, dctx = _dev(part, TXN_FIELDS), _dev(cpart, CTX_FIELDS)
    vec = torch.empty((n, 64), dtype=torch.float32, device="cuda")
    raw = torch.empty((n, 16), dtype=torch.float64, device="cuda")
    fmap = torch.empty((n, 64), dtype=torch.float64, device="cuda")
    rules = torch.empty((n, 24), dtype=torch.uint8, device="cuda")
    eng.features_full_device({f: t.data_ptr() for f, t in dev.items()}, {f: t.data_ptr() for f, t in dctx.items()},
                             n, vec.data_ptr(), fmap.data_ptr(), rules.data_ptr(), raw.data_ptr())
    eng.sync()
    torch.cuda.synchronize()
    return vec.cpu().numpy(), raw.cpu().numpy(), fmap.cpu().numpy(), \
        rules.cpu().numpy().reshape(-1).view(np.dtype(RULE_DTYPE))


def _seq(eng, part, T):
    """features_seq_device -> vectors, raw, sequences"""
    import torch
    n = len(part["card_key"])
    dev = _dev(part, TXN_FIELDS)
    vec = torch.empty((n, 64), dtype=torch.float32, device="cuda")
    raw = torch.empty((n, 16), dtype=torch.float64, device="cuda")
    seq = torch.empty((n, T, 16), dtype=torch.float32, device="cuda")
    eng.features_seq_device({f: t.data_ptr() for f, t in dev.items()}, n, vec.data_ptr(), seq.data_ptr(),
                            raw.data_ptr())
    eng.sync()
    torch.cuda.synchronize()
    return vec.cpu().numpy(), raw.cpu().numpy(), seq.cpu().numpy()


def _check_fmap(fmap, rules, efm, erules):
    exact = [c for c in range(64) if c not in (1, 25)]
    np.testing.assert_array_equal(fmap[:, exact], efm[:, exact])
    np.testing.assert_array_max_ulp(fmap[:, 1], efm[:, 1], maxulp=1)
    np.testing.assert_allclose(fmap[:, 25], efm[:, 25], rtol=1e-9, equal_nan=True)
    for f in ("tp_score", "fe_score", "tp_decision", "tp_risk", "fe_decision", "fe_risk"):
        np.testing.assert_array_equal(rules[f], erules[f], err_msg=f)


def _check_seq(seq, exp):
    if len(seq):
        np.testing.assert_array_max_ulp(seq, exp, maxulp=1)
    assert (seq[:, :, NOT_LOG] == exp[:, :, NOT_LOG]).all()


# ---------------------------------------------------------------------------------------------------------------
# card state across the cuts of the edge streams; the image against the stream

def _check_image(path, tx, rows, loaded, mode, K):
    """the image written after `rows` rows, parsed on the host, against the stream alone"""
    hd, cards, ring = S.parse_image(path.read_bytes())
    keys = _held(loaded, tx, rows)
    assert hd["magic"] == b"FDSNAP\x00\x01" and hd["header_bytes"] == S.IMAGE_HEADER_BYTES
    assert (hd["version"], hd["window_mode"], hd["ring_k"], hd["seq_len"]) == (S.IMAGE_VERSION, mode, K, 0)
    assert hd["n_cards"] == len(keys) and hd["has_uext"] == 0 and hd["record_bytes"] == S.record_bytes(K, 0, False)
    assert (hd["shard"], hd["n_shards"], hd["windows_present"]) == (0, 1, 0)
    np.testing.assert_array_equal(np.sort(cards["key"]), keys)
    at = {int(k): i for i, k in enumerate(cards["key"].tolist())}
    seen = 0
    for key in np.unique(tx["card_key"][:rows]).tolist():
        idx = np.flatnonzero(tx["card_key"][:rows] == key)
        c, n = cards[at[key]], min(K, len(idx))
        assert c["last_ts"] == tx["ts_ms"][idx[-1]]
        assert c["ring_n"] == n and c["ring_head"] == len(idx) % K
        # the ring_n entries behind the head (a slot's words past them are not part of the state: the table does
        # not clear them)
        held = [(int(c["ring_head"]) - 1 - j) % K for j in range(n)]
        got = sorted(zip(ring["ts"][at[key], held].tolist(), ring["cents"][at[key], held].tolist()))
        assert got == sorted(zip(tx["ts_ms"][idx[-n:]].tolist(), tx["amount_cents"][idx[-n:]].tolist()))
        seen += 1
    idle = ~np.isin(cards["key"], tx["card_key"][:rows])  # loaded users without an event yet
    assert (cards["ring_n"][idle] == 0).all() and seen + int(idle.sum()) == len(keys)


def _edge_run(engine, tmp_path, layout, K, mode, image=False):
    tx, bounds = V.stream(layout, K)
    chosen = S.cuts(layout, K)
    orc = V.oracle_pair(engine, mode, K)
    loaded = V.population()["users"]["key"]
    eng, fresh = engine, None
    sat = eng.counter("window_saturated") if mode == 1 else None
    try:
        for b, (a, e) in enumerate(zip(bounds[:-1], bounds[1:])):
            if b in chosen:
                path = tmp_path / f"cut-{b}.fdsnap"
                assert eng.state_snapshot(path) == path.stat().st_size
                held = len(_held(loaded, tx, a))
                nxt = FraudEngine(0)
                try:
                    nxt.state_init(CAPS[chosen.index(b) % len(CAPS)], mode, K)
                    assert nxt.state_restore(path) == held
                    assert nxt.state_info()["cards"] == held
                    if mode == 1:
                        assert nxt.counter("window_saturated") == 0
                        sat = 0
                finally:
                    if fresh is not None:
                        fresh.close()
                    eng = fresh = nxt
                if image:
                    _check_image(path, tx, a, loaded, mode, K)
            part = _part(tx, a, e)
            vec, raw = eng.features(part, want_raw=True)
            rraw, rvec = orc.run(part)
            _check(vec, raw, rvec, rraw)
            if mode == 1:
                now = eng.counter("window_saturated")
                assert now - sat == int((rraw[:, 11] >= K).sum())
                sat = now
        assert eng.state_info()["cards"] == len(_held(loaded, tx, bounds[-1]))
    finally:
        if fresh is not None:
            fresh.close()


@pytest.mark.parametrize("mode", [0, 1], ids=["redis_compat", "sliding"])
@pytest.mark.parametrize("layout,K", S.PAIRS)
def test_edge_streams_across_cuts(engine, tmp_path, layout, K, mode):
    """every batch before the first cut and after each cut against the sequential C oracle; each restore's count
    and the fresh engine's state_info()["cards"] against the keys the oracle holds; sliding mode: the
    window_saturated counter of each fresh engine counts from 0"""
    _edge_run(engine, tmp_path, layout, K, mode)


def test_image_contents_match_the_stream(engine, tmp_path):
    """`one` / 16, sliding: the image written at each cut, parsed on the host (snapshot_cases.parse_image): header
    fields, the key set, and per card its last event time, ring fill, head and the multiset of ring events"""
    _edge_run(engine, tmp_path, "one", 16, 1, image=True)


# ---------------------------------------------------------------------------------------------------------------
# feature map, rules (a threshold carried in the header) and LSTM history across a cut

def _fmap_setup(engine, n_users, mode, K=8, T=10):
    """tests/test_gpu_fmap.py `_setup` with an LSTM history plane"""
    pop = synth.population(n_users, 150, seed=n_users + 3)
    U, M = pop["users"], pop["merchants"]
    cap = 4 * n_users + 4096
    engine.state_init(cap, mode, K, seq_len=T)
    engine.load_users(U["key"], U["avg_amount"], U["account_age_days"], U["device_fp"])
    engine.load_merchants(M["fraud_rate"], M["risk_multiplier"])
    ue = synth.users_ext(pop)
    keep = np.random.default_rng(1).random(n_users) < 0.9  # some loaded users without extended fields
    engine.load_users_ext(ue["key"][keep], **{k: v[keep] for k, v in ue.items() if k != "key"})
    me = synth.merchants_ext(pop)
    n_me = 140  # merchants 140..149 have no extended profile
    engine.load_merchants_ext(n_me, **{k: v[:n_me] for k, v in me.items()})
    pay, ref = synth.vocab_flags()
    engine.load_vocab(pay, ref)
    orc = OracleFeatureState(cap, mode, K)
    orc.load_users(U["key"], U["avg_amount"], U["account_age_days"], U["device_fp"])
    orc.load_merchants(M["fraud_rate"], M["risk_multiplier"])
    users_ext = {int(k): {f: ue[f][i] for f in ue if f != "key"} for i, k in enumerate(ue["key"]) if keep[i]}
    mext = {k: v[:n_me] for k, v in me.items()}
    return pop, orc, users_ext, mext, pay, ref


def _fmap_stream(pop, n, seed):
    tx = synth.txn_stream(pop, n, seed=seed, rate_per_s=2.0, unknown_user_frac=0.05, unknown_merchant_frac=0.05)
    rng = np.random.default_rng(4)
    tx["hour"] = tx["hour"].copy()
    has_h = rng.random(n) < 0.6
    tx["hour"][has_h] = rng.integers(0, 24, int(has_h.sum()))
    tx["weekend"] = tx["weekend"].copy()
    tx["weekend"][rng.random(n) < 0.3] = 1
    tx["amount_cents"] = tx["amount_cents"].copy()
    tx["amount_cents"][::17] = (tx["amount_cents"][::17] // 1000) * 1000  # round amounts
    return tx, synth.txn_context(tx)


@pytest.mark.parametrize("mode", [0, 1], ids=["redis_compat", "sliding"])
def test_feature_map_rules_and_history_across_a_cut(engine, tmp_path, mode):
    """1 500 users (90 % with extended profiles, merchants 140..149 without), unknown users / merchants, context
    with NaNs, the rule threshold at 0.65 (it travels in the image's header: the fresh engine sets no option).
    After the restore the feature map and rule records against oracle/fmap_ref.py, and (sliding) a second restore
    of the same image emitting the LSTM sequences against SequenceState fed from row 0."""
    T = 10
    pop, orc, users_ext, mext, pay, ref = _fmap_setup(engine, 1500, mode, T=T)
    tx, ctx = _fmap_stream(pop, 12000, 21 + mode)
    M = {"fraud_rate": pop["merchants"]["fraud_rate"], "risk_multiplier": pop["merchants"]["risk_multiplier"]}
    hist = lstm_ref.SequenceState(T)
    bounds = [0, 3000, 6000, 12000]

    def expect(a, b):
        part, cpart = _part(tx, a, b), _part(ctx, a, b)
        raw, rvec, vel5 = orc.run_ex(part)
        efm, erules = fmap_ref.feature_map(part, cpart, raw, vel5, users_ext, M, mext, pay, ref, threshold=0.65)
        return part, cpart, raw, rvec, efm, erules, hist.run(part["card_key"], raw)

    def check_full(eng, part, cpart, raw, rvec, efm, erules):
        vec, graw, fmap, rules = _full(eng, part, cpart)
        _check(vec, graw, rvec, raw)
        _check_fmap(fmap, rules, efm, erules)
        assert len(np.unique(rules["tp_decision"])) >= 2 and len(np.unique(rules["fe_risk"])) >= 3
        assert np.isnan(fmap[:, 19]).any() and (~np.isnan(fmap[:, 43])).any()
        return rules

    engine.set_option("rule_fraud_threshold_permille", 650)
    try:
        for a, b in zip(bounds[:2], bounds[1:3]):
            part, cpart, raw, rvec, efm, erules, _ = expect(a, b)
            check_full(engine, part, cpart, raw, rvec, efm, erules)
        path = tmp_path / "fmap.fdsnap"
        engine.state_snapshot(path)
    finally:
        engine.set_option("rule_fraud_threshold_permille", 700)
    held = len(_held(pop["users"]["key"], tx, bounds[2]))
    part, cpart, raw, rvec, efm, erules, eseq = expect(bounds[2], bounds[3])
    # the threshold decides rows: between 0.65 and 0.7 the decision differs from the default's
    assert ((erules["tp_score"] >= 0.65) & (erules["tp_score"] < 0.7)).any()
    for want_seq in ((False, True) if mode == 1 else (False,)):
        fresh = FraudEngine(0)
        try:
            fresh.state_init(1 << 15 if want_seq else 3000 * 4, mode, 8, T)
            assert fresh.state_restore(path) == held
            assert fresh.state_info()["cards"] == held
            if want_seq:
                vec, graw, seq = _seq(fresh, part, T)
                _check(vec, graw, rvec, raw)
                _check_seq(seq, eseq)
            else:
                check_full(fresh, part, cpart, raw, rvec, efm, erules)
        finally:
            fresh.close()


# ---------------------------------------------------------------------------------------------------------------
# the 4-row LSTM kernel reading a restored history ring in place

def test_lstm_reads_restored_ring_through_descriptors(engine, tmp_path):
    """[XGBoost 80 x 8, IsolationForest 30, LSTM] through fd_score_batch_device in batches of 1 000 (under 4 096:
    the 4-row kernel reads each card's last sequence in its history ring through descriptors: head, n, wrap).
    300 cards, the cut after three batches: cards with fewer than T events, exactly T, and more with the head
    mid-ring, asserted from the stream. The LSTM column against the torch forward over the oracle's uncut
    histories, the blend against scoring_ref.blend_row."""
    import torch

    import oracle
    from fdengine import iforest_from_sklearn, xgboost_from_json_doc
    from fdengine import lstm as L
    from fdengine._native import FD_SLOT_LSTM
    from oracle import scoring_ref as SR
    T, K, B, n_users = 10, 8, 1000, 300
    pop = synth.population(n_users, 100, seed=n_users + 1)
    U, Mm = pop["users"], pop["merchants"]
    cap = 4 * n_users + 4096
    engine.state_init(cap, 1, K, seq_len=T)
    engine.load_users(U["key"], U["avg_amount"], U["account_age_days"], U["device_fp"])
    engine.load_merchants(Mm["fraud_rate"], Mm["risk_multiplier"])
    orc = OracleFeatureState(cap, 1, K)
    orc.load_users(U["key"], U["avg_amount"], U["account_age_days"], U["device_fp"])
    orc.load_merchants(Mm["fraud_rate"], Mm["risk_multiplier"])
    tx = synth.txn_stream(pop, 6 * B, seed=9, rate_per_s=2.0)
    cut = 3 * B
    keys, n_at = np.unique(tx["card_key"][:cut], return_counts=True)
    later = np.isin(keys, tx["card_key"][cut:])  # the restored history is read by a later transaction
    assert ((n_at < T) & later).any() and ((n_at == T) & later).any()
    assert ((n_at > T) & (n_at % T != 0) & later).any() and ((n_at > T) & (n_at % T == 0) & later).any()
    X = synth.feature_matrix(3000, 64, seed=3)
    xgb = xgboost_from_json_doc(synth.xgboost_doc(80, 8, 64, X, seed=4, p_leaf=0.1))
    ifm = iforest_from_sklearn(synth.isolation_forest(X.astype(np.float64), n_estimators=30))
    lw = L.random_weights(16, 128, 1, seed=5)
    names = ["xgboost_primary", "isolation_forest", "lstm_sequential"]
    w = SR.normalized_weights({"xgboost_primary": 0.4, "isolation_forest": 0.05, "lstm_sequential": 0.25})
    params = FraudEngine.blend_params([w[k] for k in names], [SR.CONF_MULT[k] for k in names])
    hist = lstm_ref.SequenceState(T)

    def load(eng):
        eng.load_forest(0, xgb)
        eng.load_forest(1, ifm)
        eng.load_lstm(lw)

    def step(eng, a, b):
        n = b - a
        part = _part(tx, a, b)
        dev = _dev(part, TXN_FIELDS)
        out = [torch.empty(n, dtype=d, device="cuda") for d in (torch.float64, torch.float64, torch.uint8,
                                                                 torch.uint8)]
        vec = torch.empty((n, 64), dtype=torch.float32, device="cuda")
        mp = torch.empty((3, n), dtype=torch.float64, device="cuda")
        eng.score_batch_device(params, [0, 1, FD_SLOT_LSTM], {f: t.data_ptr() for f, t in dev.items()}, n,
                               *[o.data_ptr() for o in out], vec_ptr=vec.data_ptr(), model_probs_ptr=mp.data_ptr())
        eng.sync()
        torch.cuda.synchronize()
        rraw, rvec = orc.run(part)
        P, Vv = mp.cpu().numpy(), vec.cpu().numpy()
        _check(Vv, rraw, rvec, rraw)  # vectors only: this path emits no raw features
        px, _, _ = oracle.xgb_predict(xgb, Vv)
        pi, _, _ = oracle.iforest_predict(ifm, Vv)
        pl = lstm_ref.lstm_forward(lw, hist.run(part["card_key"], rraw))
        assert np.abs(P[0] - px).max() <= 1e-5 and np.abs(P[1] - pi).max() <= 1e-5
        assert np.abs(P[2] - pl).max() <= 1e-5, np.abs(P[2] - pl).max()
        fp = out[0].cpu().numpy()
        for i in range(0, n, 11):
            rfp, _, _, _ = SR.blend_row(names, [float(P[0, i]), float(P[1, i]), float(P[2, i])], w)
            assert fp[i] == rfp

    fresh = FraudEngine(0)
    try:
        load(engine)
        for a in range(0, cut, B):
            step(engine, a, a + B)
        path = tmp_path / "lstm.fdsnap"
        engine.state_snapshot(path)
        fresh.state_init(3000, 1, K, T)
        held = len(_held(U["key"], tx, cut))
        assert fresh.state_restore(path) == held and fresh.state_info()["cards"] == held
        load(fresh)  # models are not part of the image
        for a in range(cut, 6 * B, B):
            step(fresh, a, a + B)
    finally:
        fresh.close()
        engine.unload_lstm()


# ---------------------------------------------------------------------------------------------------------------
# Flink windows across a cut

@functools.lru_cache(maxsize=None)
def _window_case(name):
    """-> (batches, per step the oracle's (user windows, merchant windows, watermark); the last step is the flush).
    The oracle runs once per stream, uncut; the tests leave it unchanged."""
    batches = {"stream": lambda: synth.window_stream(12, 3000, 400, 60, seed=5),
               "hour_boundary": lambda: WE.watermark_batches(WE.T0),
               "around_zero": lambda: WE.watermark_batches(0)}[name]()
    orc, steps = W.WindowOracle(), []
    for b in batches:
        u, m = orc.step(WE.oracle_batch(b))
        steps.append((u, m, orc.wm))
    u, m = orc.step([], flush=True)
    steps.append((u, m, orc.wm))
    return batches, steps


def _window_cut(name, where, steps):
    n = len(steps) - 1  # batches
    if where == "before_first":
        return 0
    if where == "last":
        return n
    if name == "stream":
        return n // 2
    # edge batches: the boundary after which the watermark sits on end - 1 of an open user window (every minute
    # ends one, and the batch's own events keep the windows over the next minutes open)
    on_edge = [b for b in range(n // 3, n) if (steps[b - 1][2] + 1) % WE.SLIDE == 0]
    return on_edge[0]


def _win_step(eng, b, flush=False):
    return eng.windows_step_host(b["key"], b["ts_ms"], b["amount_cents"], b["merchant"], b["payment_method"],
                                 b["is_fraud"], b["fraud_score"], flush=flush)


@pytest.mark.parametrize("where", ["before_first", "middle", "last"])
@pytest.mark.parametrize("name", ["stream", "hour_boundary", "around_zero"])
def test_windows_across_a_cut(engine, tmp_path, name, where):
    """every fired window of every step (before the cut, after it, the flush) on all of UF / MF, and the
    watermark after each step; a cut before the first batch writes an image without window state, whose restore
    leaves a never-stepped window state"""
    batches, steps = _window_case(name)
    cut = _window_cut(name, where, steps)
    empty = {k: v[:0] for k, v in batches[0].items()}
    fired = [0, 0]

    def run(eng, lo, hi):
        for i in range(lo, hi):
            flush = i == len(batches)
            gu, gm = _win_step(eng, empty if flush else batches[i], flush)
            ou, om, wm = steps[i]
            _compare(gu, ou, UF, (0, 1))
            _compare(gm, om, MF, (0, 1))
            assert eng.windows_stats()["watermark"] == (wm if wm is not None else NO_WM)
            if i >= cut:
                fired[0] += len(gu)
                fired[1] += len(gm)

    engine.state_init(1 << 15, 0, 4)
    engine.windows_init(1 << 16)
    run(engine, 0, cut)
    path = tmp_path / "win.fdsnap"
    engine.state_snapshot(path)
    hd, _, _ = S.parse_image(path.read_bytes())
    assert hd["windows_present"] == (1 if cut else 0)
    if where == "middle" and name != "stream":
        assert (steps[cut - 1][2] + 1) % WE.SLIDE == 0  # the watermark on end - 1
    fresh = FraudEngine(0)
    try:
        fresh.state_init(1 << 13, 0, 4)
        fresh.windows_init(1 << 16)
        keys = np.unique(np.concatenate([b["key"] for b in batches[:cut]] + [empty["key"]]))
        assert fresh.state_restore(path) == len(keys) and fresh.state_info()["cards"] == len(keys)
        before = steps[cut - 1][2] if cut else None
        st = fresh.windows_stats()
        assert st["watermark"] == (before if before is not None else NO_WM)
        if cut == 0:
            assert (st["user_events"], st["merchant_events"]) == (0, 0)
        run(fresh, cut, len(batches) + 1)
    finally:
        fresh.close()
    # windows did fire after the cut (the flush alone fires 15 user and 2 merchant windows of the edge batches)
    assert fired[0] >= (1000 if name == "stream" else 15) and fired[1] >= (50 if name == "stream" else 2)


# ---------------------------------------------------------------------------------------------------------------
# re-shard against the oracles

@functools.lru_cache(maxsize=None)
def _reshard_case():
    """the stream and, per batch, what the uncut unsharded oracles give; computed once, left unchanged"""
    T, K = 10, 8
    pop = synth.population(600, 120, seed=51)
    tx, ctx = _fmap_stream(pop, 6000, 52)
    U, M = pop["users"], pop["merchants"]
    ue, me = synth.users_ext(pop), synth.merchants_ext(pop)
    pay, ref = synth.vocab_flags()
    orc = OracleFeatureState(1 << 13, 1, K)
    orc.load_users(U["key"], U["avg_amount"], U["account_age_days"], U["device_fp"])
    orc.load_merchants(M["fraud_rate"], M["risk_multiplier"])
    users_ext = {int(k): {f: ue[f][i] for f in ue if f != "key"} for i, k in enumerate(ue["key"])}
    hist, win = lstm_ref.SequenceState(T), W.WindowOracle()
    bounds = list(range(0, 6001, 1000))
    out = []
    for a, b in zip(bounds[:-1], bounds[1:]):
        part, cpart = _part(tx, a, b), _part(ctx, a, b)
        raw, rvec, vel5 = orc.run_ex(part)
        efm, erules = fmap_ref.feature_map(part, cpart, raw, vel5, users_ext,
                                           {"fraud_rate": M["fraud_rate"], "risk_multiplier": M["risk_multiplier"]},
                                           me, pay, ref)
        seq = hist.run(part["card_key"], raw)
        win.observe(int(part["ts_ms"].max()))
        wu, wm = win.step(WE.oracle_batch(_win_batch(tx, ctx, slice(a, b))))
        out.append(dict(raw=raw, vec=rvec, fmap=efm, rules=erules, seq=seq, wu=wu, wm=wm, mark=win.wm))
    wu, wm = win.step([], flush=True)
    out.append(dict(wu=wu, wm=wm, mark=win.wm))
    return pop, tx, ctx, bounds, out


def _win_batch(tx, ctx, m):
    return dict(key=tx["card_key"][m], ts_ms=tx["ts_ms"][m], amount_cents=tx["amount_cents"][m],
                merchant=tx["merchant"][m], payment_method=ctx["payment_method"][m],
                is_fraud=tx["is_fraud"][m].astype(np.uint8), fraud_score=ctx["fraud_score"][m])


def _check_shard_windows(per_shard, exp):
    """user windows: the union over shards is the oracle's; merchant windows: per (merchant, window_start) the
    shards' partial counts and integer cents sum to the oracle's"""
    gu = [r for u, _ in per_shard for r in u]
    _compare(gu, exp["wu"], UF, (0, 1))
    got = {}
    for _, m in per_shard:
        for r in m:
            k = (int(r["merchant"]), int(r["window_start"]))
            c = got.setdefault(k, [0, 0])
            c[0] += int(r["count"])
            c[1] += int(r["cents"])
    assert got == {(r["merchant"], r["window_start"]): [r["count"], r["cents"]] for r in exp["wm"]}


@pytest.mark.parametrize("old_w,new_w", [(1, 2), (2, 3), (3, 1)])
def test_reshard_against_the_oracles(engine, tmp_path, old_w, new_w):
    """Emulated shards (one engine per shard, each fed its cards' rows by shard_of), sliding mode, K = 8, LSTM
    history, extended profiles, windows with the node-wide watermark (windows_observe on every shard). Every new
    shard restores every old image: the owner filter, the re-slot of the window events through the card table, the
    append to a log another image already filled and its watermark check. Per transaction the vectors, feature map
    and rules (even batches) or the LSTM sequences (odd batches: the history is appended either way) against the
    uncut unsharded oracles; the windows as `_check_shard_windows`; each restore count against the oracle-held keys
    the shard owns."""
    T, K = 10, 8
    pop, tx, ctx, bounds, exp = _reshard_case()
    U, M = pop["users"], pop["merchants"]
    ue, me = synth.users_ext(pop), synth.merchants_ext(pop)
    pay, ref = synth.vocab_flags()
    n_cut = 3

    def batch(shards, world, bi):
        a, b = bounds[bi], bounds[bi + 1]
        own = shard_of(tx["card_key"][a:b], world)
        top = int(tx["ts_ms"][a:b].max())
        fired = []
        for r, e in enumerate(shards):
            m = a + np.flatnonzero(own == r)
            part, cpart = {k: v[m] for k, v in tx.items()}, {k: v[m] for k, v in ctx.items()}
            x = exp[bi]
            if bi % 2 == 0:
                vec, raw, fmap, rules = _full(e, part, cpart)
                _check_fmap(fmap, rules, x["fmap"][m - a], x["rules"][m - a])
            else:
                vec, raw, seq = _seq(e, part, T)
                _check_seq(seq, x["seq"][m - a])
            _check(vec, raw, x["vec"][m - a], x["raw"][m - a])
            e.windows_observe(top)
            fired.append(_win_step(e, _win_batch(tx, ctx, m)))
            assert e.windows_stats()["watermark"] == x["mark"]
        _check_shard_windows(fired, exp[bi])
        return sum(len(u) for u, _ in fired)

    old = [FraudEngine(0) for _ in range(old_w)]
    new = [FraudEngine(0) for _ in range(new_w)]
    try:
        paths = []
        for r, e in enumerate(old):
            keep = shard_of(U["key"], old_w) == r
            e.state_init(1 << 13, 1, K, T)
            e.load_users(U["key"][keep], U["avg_amount"][keep], U["account_age_days"][keep], U["device_fp"][keep])
            e.load_merchants(M["fraud_rate"], M["risk_multiplier"])
            e.load_users_ext(ue["key"][keep], **{k: v[keep] for k, v in ue.items() if k != "key"})
            e.load_merchants_ext(len(me["avg_amount"]), **me)
            e.load_vocab(pay, ref)
            e.windows_init(1 << 16)
        for bi in range(n_cut):
            batch(old, old_w, bi)
        for r, e in enumerate(old):
            paths.append(tmp_path / f"state-{r}-of-{old_w}.fdsnap")
            e.state_snapshot(paths[-1], r, old_w)
        held = _held(U["key"], tx, bounds[n_cut])
        for r, e in enumerate(new):
            e.state_init(3000 if r else 1 << 14, 1, K, T)
            e.windows_init(1 << 16)
            mine = int((shard_of(held, new_w) == r).sum())
            assert sum(e.state_restore(p, r, new_w) for p in paths) == mine
            assert e.state_info()["cards"] == mine
            assert e.windows_stats()["watermark"] == exp[n_cut - 1]["mark"]
        fired = sum(batch(new, new_w, bi) for bi in range(n_cut, len(bounds) - 1))
        empty = {k: v[:0] for k, v in _win_batch(tx, ctx, slice(0, 0)).items()}
        last = [_win_step(e, empty, flush=True) for e in new]
        _check_shard_windows(last, exp[-1])
        assert fired > 100 and len(exp[-1]["wm"]) >= 1
    finally:
        for e in old + new:
            e.close()


# ---------------------------------------------------------------------------------------------------------------
# both chunk loops

def test_snapshot_and_restore_take_a_second_chunk(engine, tmp_path):
    """A table of 2^20 slots (four snapshot chunks of 2^18: lo > 0, counting_iterator(lo), absolute slots in
    the gather) holding 300 000 loaded users (more than 2^18 records: the restore loop's second pass), no LSTM
    plane, K = 1. 4 000 rows in two batches, the snapshot between them, restored into 2^19 slots: the image's key
    set, the restore count, both batches and state_info()["cards"] against the oracle. A ~45 MB image; measured
    wall time on an MI355X 0.2 s (0.20 and 0.24 s in two runs), so it carries no timeout mark."""
    n_users = 300_000
    pop = synth.population(n_users, 50, seed=91)
    U, M = pop["users"], pop["merchants"]
    engine.state_init(1 << 20, 1, 1)
    engine.load_users(U["key"], U["avg_amount"], U["account_age_days"], U["device_fp"])
    engine.load_merchants(M["fraud_rate"], M["risk_multiplier"])
    orc = OracleFeatureState(1 << 20, 1, 1)
    orc.load_users(U["key"], U["avg_amount"], U["account_age_days"], U["device_fp"])
    orc.load_merchants(M["fraud_rate"], M["risk_multiplier"])
    tx = synth.txn_stream(pop, 4000, seed=92, rate_per_s=50.0, unknown_user_frac=0.05)
    sat = engine.counter("window_saturated")

    def step(eng, a, b, sat):
        part = _part(tx, a, b)
        vec, raw = eng.features(part, want_raw=True)
        rraw, rvec = orc.run(part)
        _check(vec, raw, rvec, rraw)
        now = eng.counter("window_saturated")
        assert now - sat == int((rraw[:, 11] >= 1).sum())

    step(engine, 0, 2000, sat)
    path = tmp_path / "big.fdsnap"
    engine.state_snapshot(path)
    held = _held(U["key"], tx, 2000)
    assert len(held) > 1 << 18
    hd, cards, ring = S.parse_image(path.read_bytes())
    assert hd["n_cards"] == len(held) and hd["record_bytes"] == S.record_bytes(1, 0, False)
    np.testing.assert_array_equal(np.sort(cards["key"]), held)
    first = {}
    for i in range(2000):
        first[int(tx["card_key"][i])] = i  # the card's last event before the cut
    order = np.argsort(cards["key"])
    at = order[np.searchsorted(cards["key"][order], np.array(list(first), np.uint64))]
    rows = np.array(list(first.values()))
    np.testing.assert_array_equal(cards["last_ts"][at], tx["ts_ms"][rows])
    np.testing.assert_array_equal(ring["cents"][at, 0], tx["amount_cents"][rows])
    assert int((cards["ring_n"] == 1).sum()) == len(first)
    fresh = FraudEngine(0)
    try:
        fresh.state_init(1 << 19, 1, 1)
        assert fresh.state_restore(path) == len(held)
        assert fresh.state_info()["cards"] == len(held)
        step(fresh, 2000, 4000, 0)
        assert fresh.state_info()["cards"] == len(_held(U["key"], tx, 4000))
    finally:
        fresh.close()
