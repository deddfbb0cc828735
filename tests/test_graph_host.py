"""CPU: the transaction-network features' declared rule against the reference's own outputs
(tests/golden/graph_network_cases.npz, written by golden/make_graph_golden.py from GraphFraudDetector), the pure host
form fd_graph_features_host against the same, the window rule's closed form, argument errors and the new kernels'
resource remarks."""
import ctypes as C
import json

import numpy as np
import pytest

import graph_cases as G


@pytest.fixture(scope="module")
def fixture():
    return G.load_fixture()


def test_fixture_covers_what_it_should(fixture):
    assert {c["H"] for c in fixture.values()} == {2, 3, 7, 8, 64, 256, 1000, 10000}
    d = fixture["default"]
    assert len(d["user"]) > 10000  # crosses the first truncation
    for name, c in fixture.items():
        out = c["out"]
        for k in range(4):
            inside = ((out[:, k] > 0) & (out[:, k] < 1)).mean()
            if c["H"] == 2 and k == 2:
                continue  # a two-entry window with dM = 2 holds only the user's own pairs: always 0
            assert inside >= 0.10, (name, G.COLUMNS[k], inside)
        assert 0.10 <= (out[:, 4] == 1).mean() <= 0.90, name
        assert 0.02 <= (c["user"] == 0).mean() <= 0.09 and 0.02 <= (c["merchant"] == -1).mean() <= 0.09, name


@pytest.mark.parametrize("name", list(G.FIXTURE_STREAMS))
def test_restatement_equals_reference(fixture, name):
    c = fixture[name]
    G.assert_matches(G.restate(c["user"], c["merchant"], c["cents"], c["H"]), c["out"], name)


@pytest.mark.parametrize("name", list(G.FIXTURE_STREAMS))
def test_host_function_equals_reference(fixture, name):
    c = fixture[name]
    got = G.features_host(G.key_of(c["user"]), c["merchant"], c["cents"], c["H"])
    G.assert_matches(got, c["out"], name)


def test_host_function_equals_restatement_beyond_the_fixture():
    # merchants shared between null and real users, a saturated merchant, repeats across truncations
    for H, n, users, merchants, seed in ((5, 400, 3, 4, 1), (9, 500, 2, 12, 2), (33, 700, 150, 2, 3),
                                         (100, 900, 4, 60, 4)):
        u, m, c = G.make_stream(n, users, merchants, seed, null_user=0.15, null_merchant=0.15)
        G.assert_matches(G.features_host(G.key_of(u), m, c, H), G.restate(u, m, c, H), f"H={H}")


@pytest.mark.parametrize("H", [2, 3, 4, 5, 7, 8, 9, 64, 101])
def test_window_start_closed_form_matches_list_simulation(H):
    history = []
    for g in range(6 * H + 7):
        if len(history) >= H:  # _add_transaction_to_history
            history = history[-H // 2:]
        history.append(g)
        assert history[0] == G.window_start(g, H), (H, g)
        assert history[-1] == g
        assert len(history) == G.held_after(g + 1, H) <= H
    assert G.held_after(0, H) == 0


def test_host_function_window_matches_list_simulation():
    # one user, all-distinct merchants: user_centrality = min(held / 10, 1) exposes the window length row by row
    for H in (3, 7, 8):
        n = 5 * H
        u = np.ones(n, np.int32)
        m = np.arange(n, dtype=np.int32)
        out = G.features_host(G.key_of(u), m, np.full(n, 100, np.int64), H)
        want = [min(G.held_after(g + 1, H) / 10.0, 1.0) for g in range(n)]
        assert out[:, 0].tolist() == want


def test_argument_errors_return_status_codes():
    from fdengine import _native as N
    key = np.ones(4, np.uint64)
    mer = np.zeros(4, np.int32)
    cents = np.ones(4, np.int64)
    out = np.zeros((4, 5))
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    f = N.lib.fd_graph_features_host
    assert f(p(key), p(mer), p(cents), 4, 10, p(out)) == N.FD_OK
    for H in (1, 0, -5, 65537):
        assert f(p(key), p(mer), p(cents), 4, H, p(out)) == N.FD_ERR_INVALID_ARG
        assert b"max_history" in N.lib.fd_last_error()
    assert f(None, p(mer), p(cents), 4, 10, p(out)) == N.FD_ERR_INVALID_ARG
    assert f(p(key), None, p(cents), 4, 10, p(out)) == N.FD_ERR_INVALID_ARG
    assert f(p(key), p(mer), None, 4, 10, p(out)) == N.FD_ERR_INVALID_ARG
    assert f(p(key), p(mer), p(cents), 4, 10, None) == N.FD_ERR_INVALID_ARG
    assert b"null" in N.lib.fd_last_error()
    assert f(p(key), p(mer), p(cents), -1, 10, p(out)) == N.FD_ERR_INVALID_ARG
    assert f(None, None, None, 0, 10, None) == N.FD_OK  # n = 0 reads nothing
    # engine entry points: a null engine is a status code, not a crash
    b = N.fd_txn_batch()
    assert N.lib.fd_graph_init(None, C.byref(N.fd_graph_params(10))) == N.FD_ERR_INVALID_ARG
    assert b"null engine" in N.lib.fd_last_error()
    assert N.lib.fd_graph_clear(None) == N.FD_ERR_INVALID_ARG
    assert N.lib.fd_graph_info(None, None, None) == N.FD_ERR_INVALID_ARG
    assert N.lib.fd_graph_step_device(None, C.byref(b), 1, None) == N.FD_ERR_INVALID_ARG
    assert N.lib.fd_graph_step_host(None, C.byref(b), 1, None) == N.FD_ERR_INVALID_ARG
    assert N.FD_GRAPH_FEATURES == len(N.GRAPH_COLUMNS) == len(G.COLUMNS) and N.GRAPH_COLUMNS == G.COLUMNS
    assert N.FD_TIMING_GRAPH == 10


def test_graph_kernels_use_no_scratch():
    from fdengine import _native as N
    res = json.loads((N.PKG_ROOT / "lib" / "kernel_resources.json").read_text())
    found = {}
    for name, r in res.items():
        for k in ("graph_move_kernel", "graph_append_kernel", "graph_prev_kernel", "graph_scan_kernel",
                  "graph_prev_small_kernel", "graph_scan_small_kernel", "graph_cluster_kernel"):
            if k + "E" in name:  # (the mangled name: the identifier, then its parameter list)
                found[k] = r
    assert len(found) == 7, sorted(found)
    for k, r in found.items():
        assert r["scratch"] == 0, (k, r)
