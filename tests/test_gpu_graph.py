"""GPU: the transaction-network features (csrc/graph.hip) against the reference's own outputs
(tests/golden/graph_network_cases.npz) and, on streams the fixture does not hold, against the pure host form
fd_graph_features_host (itself pinned to the fixture by test_graph_host.py). Bars: four columns bit-equal,
path_length_anomaly within 1e-9.

Internal capacities of the implementation the streams are sized around (graph.hip / fd_internal.h):
  TXN_WG  = 64     transactions per workgroup of the prev / scan tile kernels
  BLOCK   = 256    threads per workgroup: the entries one step of the cluster kernel (and of the small kernels) reads
  TILE    = 1024   log entries per LDS tile of the prev / scan kernels
  LIST    = 1024   merchants per LDS list of the cluster kernel
  LINEAR  = 32     lists up to this long are probed linearly; longer ones are sorted (at 64, 128, ... 1024 entries)
  CHUNK   = 16384  transactions per pass (a larger call is cut into chunks)
  SMALL   = 512    a chunk below this many transactions takes the kernels with one workgroup per transaction"""
import numpy as np
import pytest

import graph_cases as G

pytestmark = pytest.mark.gpu

TXN_WG, BLOCK, TILE, LIST, LINEAR, CHUNK, SMALL = 64, 256, 1024, 1024, 32, 16384, 512


@pytest.fixture(scope="module")
def fixture():
    return G.load_fixture()


def run(eng, H, key, merchant, cents, splits=None):
    """a fresh log of window H, the stream fed in calls of the given sizes (cycled; None: one call)"""
    eng.graph_init(H)
    n = len(key)
    if splits is None:
        return eng.graph_step(key, merchant, cents)
    parts, a, i = [], 0, 0
    while a < n:
        b = min(n, a + splits[i % len(splits)])
        parts.append(eng.graph_step(key[a:b], merchant[a:b], cents[a:b]))
        a, i = b, i + 1
    return np.concatenate(parts)


def check_against_host(eng, H, user, merchant, cents, splits=None, what=""):
    key = G.key_of(user)
    got = run(eng, H, key, merchant, cents, splits)
    G.assert_matches(got, G.features_host(key, merchant, cents, H), what)
    return got


UNEVEN = (1, 7, 64, 257, 3, 1000, 255, 256, 2049)


@pytest.mark.parametrize("name", list(G.FIXTURE_STREAMS))
def test_fixture_parity_however_the_stream_is_cut(engine, fixture, name):
    c = fixture[name]
    key = G.key_of(c["user"])
    whole = run(engine, c["H"], key, c["merchant"], c["cents"])
    G.assert_matches(whole, c["out"], f"{name} one call")
    ones = run(engine, c["H"], key, c["merchant"], c["cents"], (1,))
    G.assert_matches(ones, c["out"], f"{name} calls of 1")
    uneven = run(engine, c["H"], key, c["merchant"], c["cents"], UNEVEN)
    G.assert_matches(uneven, c["out"], f"{name} uneven")
    assert whole.tobytes() == ones.tobytes() == uneven.tobytes()
    assert engine.graph_info() == {"total": len(key), "held": G.held_after(len(key), c["H"])}


@pytest.mark.parametrize("H", [2, 3, 7, 8])
def test_many_truncations_inside_one_call(engine, H):
    u, m, c = G.make_stream(700, 3, 3, 100 + H, null_user=0.1, null_merchant=0.1)
    check_against_host(engine, H, u, m, c, None, f"H={H}")


def test_call_longer_than_the_window(engine):
    u, m, c = G.make_stream(1000, 6, 9, 21)
    check_against_host(engine, 64, u, m, c, None, "H=64 n=1000")


@pytest.mark.parametrize("boundary", [64, 96, 128])
@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_truncation_on_a_call_boundary(engine, boundary, delta):
    # H = 64: the history is cut before the appends of g = 64, 96, 128, ...
    H = 64
    assert G.window_start(boundary, H) > G.window_start(boundary - 1, H)
    u, m, c = G.make_stream(200, 5, 7, 22)
    check_against_host(engine, H, u, m, c, (boundary + delta, 200), f"cut at {boundary + delta}")


def test_default_window_across_three_truncations(engine):
    # 21 000 rows at H = 10000 cross the truncations at 10000, 15000 and 20000; one call is two chunks
    n = 21000
    u, m, c = G.make_stream(n, 150, 1200, 23)
    whole = check_against_host(engine, G.DEFAULT_H, u, m, c, None, "default one call")
    cut = run(engine, G.DEFAULT_H, G.key_of(u), m, c, (9999, 2, 4999, 5001, 64))
    assert whole.tobytes() == cut.tobytes()
    assert engine.graph_info() == {"total": n, "held": G.held_after(n, G.DEFAULT_H)}


def test_repeated_pair_inside_and_outside_the_window(engine):
    H = 8  # windows: [0, g] for g < 8, then [4, g] for g = 8..11, [8, g] for g = 12..15
    user = np.array([1, 1, 2, 2, 3, 3, 2, 3, 1, 2, 3, 2, 1, 1], np.int32)
    merchant = np.array([5, 5, 6, 7, 6, 7, 6, 5, 5, 6, 7, 7, 5, 5], np.int32)
    cents = np.arange(1, 15, dtype=np.int64) * 100
    got = check_against_host(engine, H, user, merchant, cents)
    G.assert_matches(got, G.restate(user, merchant, cents, H), "restatement")
    assert got[0, 4] == 1.0 and got[1, 4] == 0.0  # (1, 5) repeats inside the window
    assert got[8, 4] == 1.0   # g = 8 sees [4, 8]: the occurrences at 0 and 1 fell out at the truncation
    assert got[12, 4] == 0.0  # g = 12 sees [8, 12]: the occurrence at 8 is the window's first entry, still inside
    assert got[13, 4] == 0.0


def test_repeated_pair_after_its_earlier_occurrence_fell_out(engine):
    H = 8
    user = np.array([1] + [2] * 7 + [1, 1], np.int32)  # (1, 5) at g = 0, again at g = 8 (sees [4, 8]) and g = 9
    merchant = np.array([5] + [6] * 7 + [5, 5], np.int32)
    cents = np.full(10, 250, np.int64)
    got = check_against_host(engine, H, user, merchant, cents)
    assert got[0, 4] == 1.0 and got[8, 4] == 1.0 and got[9, 4] == 0.0
    assert got[8, 0] == 0.1  # and the user's merchant counts once again


def one_user_many_merchants(distinct, sharers=200):
    """`sharers` rows of users 2..5 at merchants 0..sharers-1, then user 1 at `distinct` distinct merchants"""
    user = np.concatenate([2 + np.arange(sharers) % 4, np.ones(distinct)]).astype(np.int32)
    merchant = np.concatenate([np.arange(sharers), np.arange(distinct)]).astype(np.int32)
    cents = (100 + 7 * np.arange(len(user))).astype(np.int64)
    return user, merchant, cents


@pytest.mark.parametrize("distinct", [LINEAR - 1, LINEAR, LINEAR + 1, 63, 64, 65, 127, 128, 129, 511, 512, 513,
                                      LIST - 1, LIST, LIST + 1, LIST + 55, LIST + 56, LIST + 57, LIST + BLOCK - 1,
                                      LIST + BLOCK, LIST + BLOCK + 1, 2 * LIST + 700])
def test_user_with_more_merchants_than_the_cluster_list(engine, distinct):
    # the cluster kernel gathers the user's merchants LIST at a time, in steps of the BLOCK entries a workgroup reads
    # (the first step holds 56 of the user's rows behind the 200 sharers)
    user, merchant, cents = one_user_many_merchants(distinct)
    got = check_against_host(engine, 4096, user, merchant, cents, None, f"{distinct} merchants")
    small = run(engine, 4096, G.key_of(user), merchant, cents, (SMALL - 1, 100))  # the per-transaction kernels
    assert small.tobytes() == got.tobytes()
    T_minus_dM = min(200, distinct)  # the sharers' rows at the user's merchants
    assert got[-1, 2] == min(T_minus_dM / (distinct * 10), 1.0) and got[-1, 0] == 1.0


def test_merchant_with_more_than_100_users_saturates(engine):
    n = 180
    user = (1 + np.arange(n)).astype(np.int32)
    merchant = np.zeros(n, np.int32)
    cents = np.full(n, 999, np.int64)
    got = check_against_host(engine, 512, user, merchant, cents)
    assert got[98, 1] == 0.99 and got[99, 1] == 1.0 and got[-1, 1] == 1.0


def test_null_users_count_in_clustering_not_in_merchant_centrality(engine):
    # user 1 at merchants 0 and 1; a null user at merchant 0 (twice: one pair), user 2 at merchant 1
    user = np.array([0, 0, 2, 1, 1], np.int32)
    merchant = np.array([0, 0, 1, 0, 1], np.int32)
    cents = np.array([100, 200, 300, 400, 500], np.int64)
    got = check_against_host(engine, 64, user, merchant, cents)
    G.assert_matches(got, G.restate(user, merchant, cents, 64), "restatement")
    assert (got[:2] == 0).all()            # null-user rows score 0
    assert got[3, 1] == 0.01               # merchant 0: user 1 only, the null user is no user
    assert got[4, 1] == 0.02               # merchant 1: users 2 and 1
    assert got[4, 2] == (4 - 2) / (2 * 10)  # T = (0,0) (2,1) (1,0) (1,1): the null user's pair counts


def test_null_merchant_rows_count_in_the_users_average(engine):
    user = np.array([1, 1], np.int32)
    merchant = np.array([-1, 0], np.int32)
    cents = np.array([1000, 3000], np.int64)
    got = check_against_host(engine, 64, user, merchant, cents)
    assert (got[0] == 0).all()
    assert got[1].tolist() == [0.1, 0.01, 0.0, 0.5, 1.0]  # avg = (10 + 30) / 2 = 20; |30 - 20| / 20


@pytest.mark.parametrize("n", [TXN_WG - 1, TXN_WG, TXN_WG + 1, BLOCK - 1, BLOCK, BLOCK + 1, SMALL - 1, SMALL, SMALL + 1, CHUNK - 1, CHUNK,
                               CHUNK + 1, CHUNK + SMALL - 1, CHUNK + SMALL])
def test_call_sizes_around_the_workgroup_the_small_path_and_the_chunk(engine, n):
    u, m, c = G.make_stream(n, 6, 9, 24)
    check_against_host(engine, 64, u, m, c, None, f"n={n}")


@pytest.mark.parametrize("H", [TILE - 1, TILE, TILE + 1, 2 * TILE + 1])
def test_windows_around_the_tile(engine, H):
    # full windows hold H entries: one below, exactly and one above an LDS tile of the prev / scan kernels
    u, m, c = G.make_stream(2 * H + 300, 40, 300, 25)
    got = check_against_host(engine, H, u, m, c, (H - 1, 1, 1, 1, 700), f"H={H}")
    assert got.tobytes() == run(engine, H, G.key_of(u), m, c, (SMALL - 1,)).tobytes()


def test_largest_window(engine):
    u, m, c = G.make_stream(3000, 40, 300, 26)
    check_against_host(engine, 65536, u, m, c, None, "H=65536")


def test_device_pointers_on_the_engine_stream(engine):
    import torch
    H = 64
    u, m, c = G.make_stream(777, 6, 9, 27)
    key = G.key_of(u)
    want = run(engine, H, key, m, c)
    dev = {"card_key": torch.from_numpy(key.view(np.int64)).cuda(), "merchant": torch.from_numpy(m).cuda(),
           "amount_cents": torch.from_numpy(c).cuda()}
    out = torch.full((777, 5), -1.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    engine.graph_init(H)
    for a, b in ((0, 1), (1, 1), (1, 500), (500, 777)):  # n = 1, n = 0, then the rest
        ptrs = {f: t.data_ptr() + a * t.element_size() for f, t in dev.items()}
        engine.graph_step_device(ptrs, b - a, out.data_ptr() + a * 5 * 8)
    engine.sync()
    assert out.cpu().numpy().tobytes() == want.tobytes()
    assert engine.graph_info()["total"] == 777
    engine.graph_step_device({f: 0 for f in dev}, 0, 0)  # n = 0 reads no pointer


def test_clear_and_reinit_restart_the_index(engine):
    u, m, c = G.make_stream(300, 3, 3, 28)
    key = G.key_of(u)
    first = run(engine, 7, key, m, c)
    assert engine.graph_info() == {"total": 300, "held": G.held_after(300, 7)}
    engine.graph_clear()
    assert engine.graph_info() == {"total": 0, "held": 0}
    again = engine.graph_step(key, m, c)
    assert first.tobytes() == again.tobytes()  # nothing of the first run is seen
    other = run(engine, 8, key, m, c)           # re-init with another window
    G.assert_matches(other, G.features_host(key, m, c, 8), "H=8 after H=7")
    assert engine.graph_info() == {"total": 300, "held": G.held_after(300, 8)}
    for total in range(1, 40):
        engine.graph_init(5)
        engine.graph_step(key[:total], m[:total], c[:total])
        assert engine.graph_info() == {"total": total, "held": G.held_after(total, 5)}


def test_errors_counter_and_timing():
    import fdengine
    from fdengine import _native as N
    eng = fdengine.FraudEngine(0)
    try:
        one = (np.ones(1, np.uint64), np.zeros(1, np.int32), np.ones(1, np.int64))
        with pytest.raises(ValueError, match="fd_graph_init"):  # FD_ERR_NOT_LOADED
            eng.graph_step(*one)
        with pytest.raises(ValueError):
            eng.graph_info()
        with pytest.raises(ValueError):
            eng.graph_clear()
        for H in (1, 0, 65537):
            with pytest.raises(N.NativeError) as ei:
                eng.graph_init(H)
            assert ei.value.code == N.FD_ERR_INVALID_ARG and "max_history" in str(ei.value)
        eng.graph_init(16)
        with pytest.raises(N.NativeError) as ei:
            eng.graph_step_device({"card_key": 0, "merchant": 0, "amount_cents": 0}, 3, 0)
        assert ei.value.code == N.FD_ERR_INVALID_ARG and "null" in str(ei.value)
        assert eng.counter("graph_steps") == 0
        eng.set_timing(True)
        eng.graph_step(*one)
        eng.graph_step(np.zeros(0, np.uint64), np.zeros(0, np.int32), np.zeros(0, np.int64))  # a no-op
        assert eng.counter("graph_steps") == 1
        ms, launches = eng.read_timing(N.FD_TIMING_GRAPH)
        assert launches == 1 and ms > 0
    finally:
        eng.close()


@pytest.mark.parametrize("name", ["h7", "h64", "h1000"])
def test_drop_in_reproduces_the_reference(engine, fixture, name):
    from fdengine.graph import GraphFraudDetector
    c = fixture[name]
    rows = [G.txn_dict(u, m, x) for u, m, x in zip(c["user"], c["merchant"], c["cents"])]
    det = GraphFraudDetector(engine=engine, max_history_size=c["H"])
    det.load_model()
    single = 50
    got = []
    for r in rows[:single]:
        res = det.analyze_transaction_network(r)
        assert list(res) == ["network_risk_score", *G.COLUMNS] and res["network_risk_score"] == 0.0
        assert all(type(v) is float for v in res.values())
        got.append([res[k] for k in G.COLUMNS])
    got = np.concatenate([np.array(got), det.analyze_batch(rows[single:])])
    G.assert_matches(got, c["out"], name)
    stats = det.get_performance_stats()
    assert stats["total_predictions"] == len(rows)
    assert stats["transaction_history_size"] == G.held_after(len(rows), c["H"])
    assert set(stats) == {"total_predictions", "avg_processing_time_ms", "total_processing_time_ms",
                          "transaction_history_size"}
    det.close()
    engine.graph_info()  # the shared engine is not closed by a detector that did not create it
