"""Shared cases of the transaction-network feature tests (test_graph_host.py, test_gpu_graph.py,
golden/make_graph_golden.py): seeded stream generators, the id mappings, and a plain-Python restatement of the
declared rule (DESIGN.md "Transaction-network features"; GraphFraudDetector._calculate_network_features,
ml/models/graph_neural_network.py:338-392).

A stream is three integer columns: user (index into the user pool, 0 = null user_id), merchant (index into the
merchant pool, -1 = null merchant_id) and cents (> 0). The reference is fed user_id "user_<i>", merchant_id
"merchant_<j>" and amount cents / 100; the engine is fed card_key = key_of(user) and the merchant index."""
from pathlib import Path

import numpy as np

GOLDEN = Path(__file__).resolve().parent / "golden" / "graph_network_cases.npz"
COLUMNS = ("user_centrality", "merchant_centrality", "clustering_coefficient", "path_length_anomaly",
           "community_anomaly")
PATH_COL = 3
PATH_BAR = 1e-9  # path_length_anomaly: exact integer sum here, a left-to-right float sum in the reference

# fixture streams: name -> (H, rows, users, merchants, seed); H None = the reference's default 10000
FIXTURE_STREAMS = {
    "h2": (2, 240, 2, 2, 11),
    "h3": (3, 240, 2, 2, 12),
    "h7": (7, 300, 3, 3, 13),
    "h8": (8, 300, 3, 3, 14),
    "h64": (64, 600, 6, 9, 15),
    "h256": (256, 1000, 12, 30, 16),
    "h1000": (1000, 1800, 40, 300, 17),
    "default": (None, 10200, 150, 1200, 18),
}
DEFAULT_H = 10000


def make_stream(n, users, merchants, seed, null_user=0.05, null_merchant=0.05):
    """(user int32 [n] in 0..users, merchant int32 [n] in -1..merchants-1, cents int64 [n] in 100..50000)."""
    rng = np.random.default_rng(seed)
    u = rng.integers(1, users + 1, n).astype(np.int32)
    m = rng.integers(0, merchants, n).astype(np.int32)
    u[rng.random(n) < null_user] = 0
    m[rng.random(n) < null_merchant] = -1
    cents = rng.integers(100, 50001, n).astype(np.int64)
    return u, m, cents


def key_of(user):
    """user index -> card_key (u64, 0 stays 0): splitmix64's finaliser, so keys differ in every bit position"""
    x = np.asarray(user).astype(np.uint64)
    with np.errstate(over="ignore"):
        z = x * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return np.where(x == 0, np.uint64(0), z | np.uint64(1)).astype(np.uint64)


def txn_dict(user, merchant, cents):
    """one row as the reference's / the drop-in's transaction dict"""
    return {"user_id": f"user_{int(user)}" if user else None,
            "merchant_id": f"merchant_{int(merchant)}" if merchant >= 0 else None,
            "amount": int(cents) / 100.0, "timestamp": "2024-01-01T00:00:00"}


def window_start(g, H):
    """s(g): first index transaction g sees"""
    if g < H:
        return 0
    keep = -(-H // 2)
    P = H - keep
    return H + (g - H) // P * P - keep


def held_after(total, H):
    """the reference's transaction_history_size after `total` transactions"""
    return 0 if total == 0 else total - window_start(total - 1, H)


def restate(user, merchant, cents, H):
    """The declared rule: integer counts over each window (numpy masks), the five values in Python floats. n x 5."""
    n = len(user)
    user = np.asarray(user, np.int64)
    merchant = np.asarray(merchant, np.int64)
    cents = np.asarray(cents, np.int64)
    out = np.zeros((n, 5))
    last, prev = {}, np.full(n, -1, np.int64)
    for g in range(n):
        pr = (int(user[g]), int(merchant[g]))
        prev[g] = last.get(pr, -1)
        last[pr] = g
        u, m, s = pr[0], pr[1], window_start(g, H)
        if u == 0 or m == -1:
            continue
        wu, wm, wc = user[s:g + 1], merchant[s:g + 1], cents[s:g + 1]
        first = prev[s:g + 1] < s
        mine = wu == u
        cntU, S = int(mine.sum()), int(wc[mine].sum())
        um = mine & first & (wm >= 0)
        dM = int(um.sum())
        dU = int((first & (wm == m) & (wu != 0)).sum())
        T = int((first & np.isin(wm, wm[um])).sum())
        out[g, 0] = min(dM / 10.0, 1.0)
        out[g, 1] = min(dU / 100.0, 1.0)
        out[g, 2] = min((T - dM) / (dM * 10), 1.0) if dM > 1 else 0.0
        avg = (S / 100.0) / cntU
        out[g, 3] = min(abs(int(cents[g]) / 100.0 - avg) / avg, 1.0) if avg > 0 else 0.0
        out[g, 4] = 1.0 if prev[g] < s else 0.0
    return out


def assert_matches(got, want, what=""):
    """the two bars: four columns bit-equal, path_length_anomaly within PATH_BAR"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    for c in range(5):
        if c == PATH_COL:
            err = float(np.abs(got[:, c] - want[:, c]).max()) if len(got) else 0.0
            assert err <= PATH_BAR, f"{what}: {COLUMNS[c]} differs by {err}"
        else:
            bad = np.flatnonzero(got[:, c].view(np.uint64) != want[:, c].view(np.uint64))
            assert bad.size == 0, f"{what}: {COLUMNS[c]} differs on {bad.size} rows, first {bad[:5]}: " \
                                  f"{got[bad[:5], c]} vs {want[bad[:5], c]}"


def load_fixture():
    """name -> dict(H, user, merchant, cents, out)"""
    z = np.load(GOLDEN)
    cases = {}
    for name in FIXTURE_STREAMS:
        cases[name] = dict(H=int(z[f"{name}_H"]), user=z[f"{name}_user"].astype(np.int32),
                           merchant=z[f"{name}_merchant"].astype(np.int32),
                           cents=z[f"{name}_cents"].astype(np.int64), out=z[f"{name}_out"])
    return cases


def features_host(key, merchant, cents, H):
    """fd_graph_features_host over a whole stream"""
    import ctypes as C

    from fdengine import _native as N
    key = np.ascontiguousarray(key, np.uint64)
    merchant = np.ascontiguousarray(merchant, np.int32)
    cents = np.ascontiguousarray(cents, np.int64)
    out = np.empty((len(key), 5))
    N.call("fd_graph_features_host", key.ctypes.data_as(C.c_void_p), merchant.ctypes.data_as(C.c_void_p),
           cents.ctypes.data_as(C.c_void_p), len(key), int(H), out.ctypes.data_as(C.c_void_p))
    return out
