"""GPU: the host (`_host`) entry points' device staging (csrc/host_stage.h) against the matching `_device` entry
points, which stage nothing. Each of the eleven host calls runs on freshly initialised engine state and must give
bit-equal outputs to the device call on the same inputs and the same fresh state.

What this adds to the per-feature tests (which drive the same entry points against the oracle at large, even sizes):
  sizes 1, 3, 7, 65   odd counts, so 1-byte and 4-byte columns leave whatever follows them misaligned under any
                      hand-computed layout; 65 is one over a wave
  optional columns    every optional output present alone and absent, optional inputs singly and all absent, a
                      `present` mask with a model absent
  growth and reuse    n = 65, 1, 300, 7 on one new engine: the staging buffer grows between calls
  n = 0               success, nothing written
  bad arguments       the codes and fd_last_error texts of csrc/engine.hip and the schedulers it calls (csrc/score.hip), unchanged
The device call gets its arrays as views that start one element into their allocation, so it does not see the
allocator's alignment either.
"""
import ctypes as C
from functools import lru_cache

import numpy as np
import pytest

from fdengine import FraudEngine, forest, lstm, mlp, synth
from fdengine import _native as N
from fdengine.ingest import IngestCodec, pack

import graph_cases as GC
import text_cases as TC

pytestmark = pytest.mark.gpu

NS = (1, 3, 7, 65)
GROWTH = (65, 1, 300, 7)
SENTINEL = 0xA5
NF = 5  # forest features = ld


class Mem:
    """The arrays of one call: numpy for a host entry point, torch views one element into their allocation for a
    device entry point. inp / out return the pointer to pass (None for an absent column)."""

    def __init__(self, device):
        self.device, self.keep, self.outs = device, [], []

    def inp(self, a):
        if a is None:
            return None
        a = np.ascontiguousarray(a)
        if not self.device:
            self.keep.append(a)
            return a.ctypes.data
        import torch
        raw = torch.from_numpy((a.view(np.int64) if a.dtype == np.uint64 else a).reshape(-1).copy())
        t = torch.empty(raw.numel() + 1, dtype=raw.dtype, device="cuda")
        t[1:].copy_(raw)
        self.keep.append(t)
        return t[1:].data_ptr()

    def out(self, shape, dtype, want=True):
        if not want:
            self.outs.append(None)
            return None
        dtype = np.dtype(dtype)
        nbytes = int(np.prod(shape)) * dtype.itemsize
        if not self.device:
            a = np.full(nbytes, SENTINEL, np.uint8)
            self.outs.append((a, shape, dtype))
            return a.ctypes.data
        import torch
        t = torch.full((nbytes + dtype.itemsize,), SENTINEL, dtype=torch.uint8, device="cuda")
        self.outs.append((t[dtype.itemsize:], shape, dtype))
        return t[dtype.itemsize:].data_ptr()

    def ready(self):
        if self.device:
            import torch
            torch.cuda.synchronize()

    def results(self):
        res = []
        for o in self.outs:
            if o is None:
                res.append(None)
                continue
            a, shape, dtype = o
            a = a.cpu().numpy() if self.device else a
            res.append(a.view(dtype).reshape(shape).copy())
        return res


def invoke(eng, name, mem, *args):
    """fd_<name>_host or _device -> (status code, fd_last_error text); a device call is waited for"""
    mem.ready()
    code = getattr(N.lib, f"fd_{name}_{'device' if mem.device else 'host'}")(eng.handle, *args)
    msg = N.lib.fd_last_error().decode()
    if mem.device and code == 0:
        eng.sync()
    return code, msg


def ok(eng, name, mem, *args):
    code, msg = invoke(eng, name, mem, *args)
    assert code == 0, f"fd_{name}: {code} {msg}"
    return mem.results()


# ---------------------------------------------------------------------------------------------- models and data
@lru_cache(maxsize=None)
def small_forest():
    X = synth.feature_matrix(64, NF, seed=2)
    return forest.xgboost_from_json_doc(synth.xgboost_doc(3, 2, NF, X, seed=3))


@lru_cache(maxsize=None)
def population():
    return synth.population(40, 12, seed=5)


MESSAGES = (b'{"user_id":"u1","amount":12.5,"timestamp":"2024-01-01T00:00:00","merchant_id":"m2","payment_method":"visa"}',
            b'{"user_id":"u2","amount":0.07,"timestamp":"2024-01-01T00:00:01Z","is_fraud":true,"fraud_score":0.75}',
            b'{"amount":"x"}')


def new_engine():
    eng = FraudEngine(0)
    eng.load_forest(0, small_forest())
    eng.load_mlp(mlp.random_weights(1, 1, 2, seed=1))
    eng.load_lstm(lstm.random_weights(1, 128, 1, seed=2))
    IngestCodec(eng, ["m1", "m2"], ["visa"], ["purchase"], ["debit"])
    return eng


@pytest.fixture(scope="module")
def eng():
    e = new_engine()
    yield e
    e.close()


def fresh_cards(eng):
    pop = population()
    U, M = pop["users"], pop["merchants"]
    eng.state_init(1024, N.FD_WINDOW_SLIDING, 4)
    eng.load_users(U["key"], U["avg_amount"], U["account_age_days"], U["device_fp"])
    eng.load_merchants(M["fraud_rate"], M["risk_multiplier"])


def txns(n):
    t = synth.txn_stream(population(), max(n, 1), seed=100 + n, rate_per_s=0.05, unknown_user_frac=0.2)
    return {k: a[:n] for k, a in t.items()}


def window_batch(n):
    b = synth.window_stream(1, max(n, 1), 9, 4, seed=n, batch_span_ms=7_200_000)[0]
    return {k: a[:n] for k, a in b.items()}


def txn_struct(mem, cols, fields):
    return N.fd_txn_batch(**{f: mem.inp(cols[f]) for f in fields})


def rng_of(n, salt):
    return np.random.default_rng(1000 * salt + n)


# ---------------------------------------------------------------------------------------------- the eleven calls
# run(eng, device, n, variant) -> list of output arrays (None = column not asked for). Each one first puts the engine
# state its call reads or writes back to its initial value. VARIANTS[name]: the optional-column combinations.
def run_forest_predict(eng, device, n, v):
    mem = Mem(device)
    X = synth.feature_matrix(max(n, 1), NF, seed=n, nan_frac=0.1)[:n]
    return ok(eng, "forest_predict", mem, 0, mem.inp(X), n, NF, mem.out((n,), "f8"), mem.out((n,), "f8", "raw" in v),
              mem.out((n, 3), "i4", "leaf" in v))


def run_features(eng, device, n, v):
    fresh_cards(eng)
    mem = Mem(device)
    b = txn_struct(mem, txns(n), N.TXN_FIELDS)
    return ok(eng, "features", mem, C.byref(b), n, mem.out((n, N.FD_VECTOR_WIDTH), "f4"),
              mem.out((n, N.FD_RAW_FEATURES), "f8", "raw" in v))


def _blend_args(mem, n, v, M):
    present = np.array([0 if f"absent{m}" in v else 1 for m in range(M)], np.uint8)
    outs = [mem.out((n,), "f8"), mem.out((n,), "f8", "confidence" in v), mem.out((n,), "u1", "decision" in v),
            mem.out((n,), "u1", "risk" in v)]
    return present, outs


def run_score_matrix(eng, device, n, v):
    mem = Mem(device)
    p = FraudEngine.blend_params([0.6, 0.4], [1.0, 0.9])
    slots = np.array([0, -1] + [-1] * (N.FD_MAX_MODELS - 2), np.int32)
    present, outs = _blend_args(mem, n, v, 2)
    ext = (C.c_void_p * N.FD_MAX_MODELS)()
    if present[1]:
        ext[1] = mem.inp(rng_of(n, 3).random(n))
    X = synth.feature_matrix(max(n, 1), NF, seed=n + 1)[:n]
    res = ok(eng, "score_matrix", mem, C.byref(p), slots.ctypes.data, ext, present.ctypes.data, mem.inp(X), n, NF,
             mem.out((2, n), "f8", "model_probs" in v), *outs)
    if res[4] is not None:
        res[4][present == 0] = 0.0  # an absent model's column of model_probs is not written: unspecified
    return res


def run_blend(eng, device, n, v):
    mem = Mem(device)
    p = FraudEngine.blend_params([0.5, 0.3, 0.2], [1.0, 0.8, 0.9])
    present, outs = _blend_args(mem, n, v, 3)
    cols = (C.c_void_p * N.FD_MAX_MODELS)()
    for m in range(3):
        if present[m]:
            cols[m] = mem.inp(rng_of(n, 10 + m).random(n))
    return ok(eng, "blend", mem, C.byref(p), n, cols, present.ctypes.data, *outs)


def run_windows_step(eng, device, n, v):
    fresh_cards(eng)
    eng.windows_init(4096)
    mem = Mem(device)
    b = window_batch(n)
    t = txn_struct(mem, {"card_key": b["key"], **b}, ("card_key", "ts_ms", "amount_cents", "merchant"))
    wi = N.fd_window_inputs(*[mem.inp(b[f]) if f in v else None for f in ("payment_method", "is_fraud", "fraud_score")])
    uo, mo = eng._windows_out(5 * n + 16, n + 16)
    nu, nm = C.c_int64(), C.c_int64()
    ok(eng, "windows_step", mem, C.byref(t), C.byref(wi), n, 1, uo.ctypes.data, len(uo), C.byref(nu), mo.ctypes.data,
       len(mo), C.byref(nm))
    # (the fired windows leave in no fixed order: one row per key, sorted here as tests/test_gpu_windows.py does)
    return [np.sort(uo[:nu.value], order=["user_key", "window_start"]),
            np.sort(mo[:nm.value], order=["merchant", "window_start"])]


def run_sink_update(eng, device, n, v):
    eng.sink_init(1 << 10, 1 << 10)
    mem = Mem(device)
    b = window_batch(n)
    t = txn_struct(mem, {"card_key": b["key"], **b}, ("card_key", "ts_ms", "amount_cents", "merchant"))
    wi = N.fd_window_inputs(None, *[mem.inp(b[f]) if f in v else None for f in ("is_fraud", "fraud_score")])
    ok(eng, "sink_update", mem, C.byref(t), C.byref(wi), n)
    if n == 0:
        return []
    hours = np.unique(b["ts_ms"] // 3_600_000)
    pairs = sorted({(int(m), int(h)) for m, h in zip(b["merchant"], b["ts_ms"] // 3_600_000) if m >= 0})
    res = [eng.sink_query(N.FD_AGG_HOURLY, hours), eng.sink_query(N.FD_AGG_DAILY, np.unique(hours // 24))]
    if pairs:
        res.append(eng.sink_query(N.FD_AGG_MERCHANT, [h for _, h in pairs], [m for m, _ in pairs]))
    assert all(r["found"].all() for r in res)
    return res


def run_ingest_json(eng, device, n, v):
    mem = Mem(device)
    buf, off = pack([MESSAGES[i % 3] for i in range(n)])
    out = N.fd_ingest_out(*[mem.out((n,), dt, k in v) for k, dt in N.INGEST_FIELDS])
    return ok(eng, "ingest_json", mem, mem.inp(buf), mem.inp(off), n, C.byref(out))


def run_lstm_predict(eng, device, n, v):
    mem = Mem(device)
    T = 2 if "T2" in v else 1
    seq = rng_of(n, 20 + T).standard_normal((n, T, N.FD_SEQ_INPUT)).astype(np.float32)
    return ok(eng, "lstm_predict", mem, mem.inp(seq), n, T, mem.out((n,), "f8"))


def run_mlp_predict(eng, device, n, v):
    mem = Mem(device)
    ld = 3 if "ld3" in v else 1
    X = rng_of(n, 30).standard_normal((n, ld)).astype(np.float32)
    return ok(eng, "mlp_predict", mem, mem.inp(X), n, ld, mem.out((n,), "f8"))


def run_graph_step(eng, device, n, v):
    eng.graph_init(16)
    mem = Mem(device)
    u, m, cents = GC.make_stream(n, 5, 3, seed=n)
    t = txn_struct(mem, {"card_key": GC.key_of(u), "merchant": m, "amount_cents": cents},
                   ("card_key", "merchant", "amount_cents"))
    return ok(eng, "graph_step", mem, C.byref(t), n, mem.out((n, N.FD_GRAPH_FEATURES), "f8"))


def text_rows(n):
    """rows of 0 to a few dozen bytes: row 0 is one byte, row 1 (when there is one) empty; "empty": every row empty"""
    pool = [TC.row("x"), TC.row(), TC.row("Bitcoin ATM 24/7", "buy gift card now!!", "crypto", "NYC"),
            TC.row("", "urgent: wire 100", "", "x"), TC.row("Shop 7", "", "groceries")]
    return [pool[i % len(pool)] for i in range(n)]


def run_text_features(eng, device, n, v):
    mem = Mem(device)
    blob, off = TC.encode([TC.row()] * n if "empty" in v else text_rows(n))
    b = N.fd_text_batch(mem.inp(blob) if len(blob) else None, mem.inp(off))
    return ok(eng, "text_features", mem, C.byref(b), n, mem.out((n, N.FD_TEXT_FEATURES), "f8", "feat" in v),
              mem.out((n,), "u1", "patterns" in v), mem.out((n,), "u1", "status" in v))


def _singly(names, base=()):
    """all of `names`, none of them, and each alone (each with `base` added)"""
    return [tuple(base) + tuple(names), tuple(base)] + [tuple(base) + (k,) for k in names]


BLEND_OUTS = ("confidence", "decision", "risk")
RUN = {
    "forest_predict": (run_forest_predict, _singly(("raw", "leaf"))),
    "features": (run_features, _singly(("raw",))),
    "score_matrix": (run_score_matrix, _singly(("model_probs",) + BLEND_OUTS) +
                     [("model_probs", "absent1") + BLEND_OUTS, ("model_probs", "absent0") + BLEND_OUTS]),
    "windows_step": (run_windows_step, _singly(("payment_method", "is_fraud", "fraud_score"))),
    "sink_update": (run_sink_update, _singly(("is_fraud", "fraud_score"))),
    "ingest_json": (run_ingest_json, _singly(tuple(k for k, _ in N.INGEST_FIELDS))),
    "lstm_predict": (run_lstm_predict, [(), ("T2",)]),
    "mlp_predict": (run_mlp_predict, [(), ("ld3",)]),
    "graph_step": (run_graph_step, [()]),
    "text_features": (run_text_features, _singly(("feat", "patterns", "status")) + [("feat", "patterns", "status", "empty")]),
    "blend": (run_blend, _singly(BLEND_OUTS) + [BLEND_OUTS + ("absent1",)]),
}


def assert_same(host, dev, what):
    assert len(host) == len(dev), what
    for k, (h, d) in enumerate(zip(host, dev)):
        assert (h is None) == (d is None), f"{what}: output {k}"
        if h is not None:
            assert h.dtype == d.dtype and h.shape == d.shape, f"{what}: output {k}"
            assert h.tobytes() == d.tobytes(), f"{what}: output {k} differs"


@pytest.mark.parametrize("name", sorted(RUN))
def test_host_call_equals_device_call(eng, name):
    run, variants = RUN[name]
    for n in NS:
        for v in variants:
            assert_same(run(eng, False, n, v), run(eng, True, n, v), f"{name} n={n} {v}")


@pytest.mark.parametrize("name", sorted(RUN))
def test_growth_and_reuse(name):
    """a new engine, so the staging buffer starts empty: it grows at 65 and at 300 and is reused at 1 and 7"""
    run, variants = RUN[name]
    e = new_engine()
    try:
        for n in GROWTH:
            assert_same(run(e, False, n, variants[0]), run(e, True, n, variants[0]), f"{name} n={n}")
    finally:
        e.close()


@pytest.mark.parametrize("name", sorted(RUN))
def test_empty_batch_writes_nothing(eng, name):
    run, variants = RUN[name]
    for out in run(eng, False, 0, variants[0]):
        if out is not None and out.dtype.names is None:
            assert out.size == 0
    # the same call with room for one element in every output: none of it is touched
    if name in ("windows_step", "sink_update"):
        return  # (their results leave through other calls; run() above saw success and no window fired)
    seen = []
    orig_out = Mem.out

    def roomy(self, shape, dtype, want=True):
        p = orig_out(self, tuple(max(s, 1) for s in shape), dtype, want)
        if want:
            seen.append(self.outs[-1][0])
        return p
    Mem.out = roomy
    try:
        run(eng, False, 0, variants[0])
    finally:
        Mem.out = orig_out
    assert seen and all((a == SENTINEL).all() for a in seen)


# ---------------------------------------------------------------------------------------------- bad arguments
def _bad_cases(eng, bare):
    """(entry point, engine, arguments after the engine, code, fd_last_error text): the checks of csrc/engine.hip"""
    n = 3
    mem = Mem(False)
    f8 = mem.out((1024,), "f8")              # a valid output of any kind
    x = mem.inp(np.zeros(1024, np.float32))  # a valid input of any kind
    p2 = FraudEngine.blend_params([0.5, 0.5], [1.0, 1.0])
    p0 = FraudEngine.blend_params([], [])
    p9 = FraudEngine.blend_params([0.5, 0.5], [1.0, 1.0])
    p9.n_models = 9
    slots = mem.inp(np.array([0, -1] + [-1] * 6, np.int32))
    none8 = (C.c_void_p * N.FD_MAX_MODELS)()
    full = txn_struct(mem, txns(n), N.TXN_FIELDS)
    no_hour = txn_struct(mem, txns(n), [f for f in N.TXN_FIELDS if f != "hour"])
    no_key = txn_struct(mem, txns(n), [f for f in N.TXN_FIELDS if f != "card_key"])
    cnt = C.byref(C.c_int64())
    off0 = mem.inp(np.array([1, 2, 3, 4], np.int64))
    offs = mem.inp(np.array([0, 1, 2, 3], np.int64))
    out = C.byref(N.fd_ingest_out())
    t_off = np.arange(4 * n + 1, dtype=np.int64)
    t_bad = t_off[::-1].copy()
    text = lambda b, o: C.byref(N.fd_text_batch(b, None if o is None else mem.inp(o)))  # noqa: E731
    IA, NL = N.FD_ERR_INVALID_ARG, N.FD_ERR_NOT_LOADED
    needs4 = "batch needs card_key, ts_ms, amount_cents and merchant"
    return [
        ("forest_predict", eng, (8, x, n, NF, f8, None, None), IA, "slot out of range"),
        ("forest_predict", eng, (3, x, n, NF, f8, None, None), NL, "Model in slot 3 not loaded"),
        ("forest_predict", eng, (0, None, n, NF, f8, None, None), IA, "bad arguments"),
        ("forest_predict", eng, (0, x, n, NF, None, None, None), IA, "bad arguments"),
        ("forest_predict", eng, (0, x, n, 0, f8, None, None), IA, "bad arguments"),
        ("forest_predict", eng, (0, x, -1, NF, f8, None, None), IA, "bad arguments"),
        ("features", eng, (None, n, f8, None), IA, "bad arguments"),
        ("features", eng, (C.byref(full), n, None, None), IA, "bad arguments"),
        ("features", eng, (C.byref(full), -1, f8, None), IA, "bad arguments"),
        ("features", eng, (C.byref(no_hour), n, f8, None), IA, "incomplete transaction batch"),
        ("score_matrix", eng, (C.byref(p2), slots, none8, None, None, n, NF, None, f8, None, None, None), IA,
         "bad arguments"),
        ("score_matrix", eng, (C.byref(p2), slots, none8, None, x, n, NF, None, None, None, None, None), IA,
         "bad arguments"),
        ("score_matrix", eng, (C.byref(p0), slots, none8, None, x, n, NF, None, f8, None, None, None), IA,
         "n_models out of range"),
        ("score_matrix", eng, (C.byref(p2), slots, none8, None, x, n, NF, None, f8, None, None, None), IA,
         "model without slot needs an external probability column"),
        ("windows_step", eng, (C.byref(full), None, n, 0, None, 0, None, None, 0, cnt), IA, "null result counts"),
        ("windows_step", eng, (C.byref(full), None, -1, 0, None, 0, cnt, None, 0, cnt), IA, "bad batch"),
        ("windows_step", eng, (None, None, n, 0, None, 0, cnt, None, 0, cnt), IA, "bad batch"),
        ("windows_step", eng, (C.byref(no_key), None, n, 0, None, 0, cnt, None, 0, cnt), IA, needs4),
        ("sink_update", eng, (None, None, n), IA, "bad arguments"),
        ("sink_update", eng, (C.byref(full), None, -1), IA, "bad arguments"),
        ("sink_update", eng, (C.byref(no_key), None, n), IA, needs4),
        ("ingest_json", eng, (x, offs, n, None), IA, "bad arguments"),
        ("ingest_json", eng, (x, None, n, out), IA, "bad arguments"),
        ("ingest_json", eng, (x, off0, n, out), IA, "offsets must start at 0"),
        ("lstm_predict", eng, (x, n, 0, f8), IA, "bad arguments"),
        ("lstm_predict", eng, (x, n, N.FD_MAX_SEQ_LEN + 1, f8), IA, "bad arguments"),
        ("lstm_predict", eng, (None, n, 1, f8), IA, "null sequence / output"),
        ("lstm_predict", eng, (x, n, 1, None), IA, "null sequence / output"),
        ("mlp_predict", bare, (x, n, 1, f8), NL, "Model graph_neural (MLP) not loaded"),
        ("mlp_predict", eng, (x, -1, 1, f8), IA, "batch size out of range"),
        ("mlp_predict", eng, (x, n, 0, f8), IA, "row stride 0 is below the MLP's in_dim 1"),
        ("mlp_predict", eng, (None, n, 1, f8), IA, "null vectors / output"),
        ("graph_step", eng, (None, n, f8), IA, "null txns"),
        ("graph_step", bare, (C.byref(full), n, f8), NL, "graph log not initialised (fd_graph_init)"),
        ("graph_step", eng, (C.byref(full), 1 << 31, f8), IA, "batch size out of range"),
        ("graph_step", eng, (C.byref(no_key), n, f8), IA, "null card_key / merchant / amount_cents / output"),
        ("graph_step", eng, (C.byref(full), n, None), IA, "null card_key / merchant / amount_cents / output"),
        ("text_features", eng, (None, n, f8, None, None), IA, "null text batch"),
        ("text_features", eng, (text(x, t_off), 1 << 31, f8, None, None), IA, "batch size out of range"),
        ("text_features", eng, (text(x, None), n, f8, None, None), IA, "null text offsets"),
        ("text_features", eng, (text(x, t_bad), n, f8, None, None), IA,
         "text offsets must start at 0 and never decrease"),
        ("text_features", eng, (text(None, t_off), n, f8, None, None), IA, "null text bytes"),
        ("blend", eng, (None, n, none8, None, f8, None, None, None), IA, "bad arguments"),
        ("blend", eng, (C.byref(p2), n, None, None, f8, None, None, None), IA, "bad arguments"),
        ("blend", eng, (C.byref(p2), n, none8, None, None, None, None, None), IA, "bad arguments"),
        ("blend", eng, (C.byref(p9), n, none8, None, f8, None, None, None), IA, "n_models out of range"),
        ("blend", eng, (C.byref(p2), n, none8, None, f8, None, None, None), IA, "null probability column"),
    ], mem


def test_bad_arguments_keep_their_codes_and_messages(eng):
    eng.graph_init(16)
    bare = FraudEngine(0)
    try:
        cases, mem = _bad_cases(eng, bare)
        wrong = []
        for k, (name, e, args, code, text) in enumerate(cases):
            got = invoke(e, name, mem, *args)
            if got != (code, text):
                wrong.append(f"case {k} fd_{name}_host: {got}, expected {(code, text)}")
        assert not wrong, "\n".join(wrong)
        assert all((a == SENTINEL).all() for a, _, _ in mem.outs)
    finally:
        bare.close()
