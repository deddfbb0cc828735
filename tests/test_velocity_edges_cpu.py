"""CPU proof of the velocity edge streams (tests/velocity_edge_cases.py) that tests/test_gpu_velocity_edges.py
feeds the feature kernels: the oracle they are compared with is itself pinned on such a stream, every code site of
csrc/features.hip meets every time edge often enough (the census), and an off-by-one at any of those comparisons
would change rows of the stream (the sensitivity).

Two comparisons are deliberately not demanded. `>` against `>=` in rebuild_windows and in the cooperative path's
final header rebuild only admits an event at exactly t - W into the rebuilt window; the next incremental step
evicts it (its eviction test is <=) before anything reads the window, so no output can show it."""
import operator

import numpy as np
import pytest

import velocity_edge_cases as V
from oracle import velocity_ref as VR

FLOOR = 10


@pytest.fixture(scope="module")
def census():
    cache = {}

    def get(layout, K):
        if (layout, K) not in cache:
            cache[layout, K] = V.census(*V.stream(layout, K), K)
        return cache[layout, K]
    return get


@pytest.mark.parametrize("mode", [0, 1])
def test_c_oracle_equals_python_chain_on_edge_stream(mode):
    """The C oracle equals the pinned Python chain on the `short` stream at K = 3: raw columns exact (column 1,
    the logarithm, within 1 f64 ulp), vectors exact."""
    tx, _ = V.stream("short", 3)
    U, M = V.population()["users"], V.population()["merchants"]
    py = VR.FeatureState(window_mode=mode, ring_k=3)
    py.load_users(U["key"], U["avg_amount"], U["account_age_days"], U["device_fp"])
    py.load_merchants(M["fraud_rate"], M["risk_multiplier"])
    raw_py = py.run(tx)
    raw_c, vec_c = V.oracle_pair(None, mode, 3).run(tx)
    cols = [c for c in range(raw_c.shape[1]) if c != 1]
    np.testing.assert_array_equal(raw_c[:, cols], raw_py[:, cols])
    np.testing.assert_array_max_ulp(raw_c[:, 1], raw_py[:, 1], maxulp=1)
    np.testing.assert_array_equal(vec_c, VR.vectors(raw_py).astype(np.float32))
    # the negative-time card: hours and ISO weekdays by floor, not truncation
    neg = tx["ts_ms"] < 0
    assert neg.sum() >= FLOOR and (tx["ts_ms"][tx["card_key"] == tx["card_key"][neg][0]] > 0).any()
    assert (raw_c[neg, 2] >= 0).all() and (raw_c[neg, 2] <= 23).all() and len(set(raw_c[neg, 2])) > 3
    assert (raw_c[neg, 3] >= 1).all() and (raw_c[neg, 3] <= 7).all()


@pytest.mark.parametrize("layout", V.LAYOUTS)
@pytest.mark.parametrize("K", [3, 16])
def test_full_scan_definition_equals_c_oracle(layout, K):
    """the parametrised plain reference, with the declared operators, is the oracle's velocity columns"""
    tx, _ = V.stream(layout, K)
    counts, sums = V.windows_full_scan(tx, K)
    raw, _ = V.oracle_pair(None, 1, K).run(tx)
    np.testing.assert_array_equal(raw[:, 9:12], counts.astype(np.float64))
    np.testing.assert_array_equal(raw[:, 12:14], sums[:, 1:] / 100.0)
    c0, s0 = V.session_scan(tx)
    raw, _ = V.oracle_pair(None, 0, K).run(tx)
    for col in (9, 10, 11):
        np.testing.assert_array_equal(raw[:, col], c0.astype(np.float64))
    np.testing.assert_array_equal(raw[:, 12], s0 / 100.0)


def _reached(layout):
    return {"one": ("inc", "full", "rebuild"), "short": ("inc", "full", "rebuild"), "long": ("long",),
            "mixed": V.SITES}[layout]


@pytest.mark.parametrize("layout", V.LAYOUTS)
@pytest.mark.parametrize("K", [3, 16])
def test_census_floors(census, layout, K):
    """Conditions on the streams, per layout and site the layout reaches: every (site, window, in / out) cell, the
    equal-timestamp cell and the future cell hold >= 10 rows; both session-gap cells; >= 10 full-ring overwrites
    with a spanning window; >= 10 first short rows behind a long segment in each carried state, carried values 1
    and K among them.

    Structurally empty cells, asserted as such: a future event (et > t) in the ring at an incremental step or at
    the rebuild step. Both read a time-sorted ring whose newest event is the previous one, and neither is a
    descent, so every ring event is <= t.

    One floor is lowered on purpose: in `mixed` only a third of the rows are short and ~1 / (3 K) of those are
    rebuild steps, so its rebuild cells are asked for one row in total, not ten per cell. The rebuild site is the
    same code behind a long segment as anywhere (`short` and `one` hold it to the floor); what only `mixed` can
    show is the carry out of the cooperative path, which has its own floor here."""
    c = census(layout, K)
    print(f"census {layout} K={K}: {c}")
    sites = _reached(layout)
    for s in V.SITES:
        if s not in sites:
            assert c[s, "rows"] == 0, (s, c[s, "rows"])
            continue
        cells = [c[s, W, e] for W in V.WINDOWS for e in ("in", "out")] + [c[s, "equal"]]
        if s in ("inc", "rebuild"):
            assert c[s, "future"] == 0
        else:
            cells.append(c[s, "future"])
        if layout == "mixed" and s == "rebuild":
            assert c[s, "rows"] >= FLOOR and sum(cells) >= 1, (s, cells)
        else:
            assert min(cells) >= FLOOR, (s, cells)
    for path, reached in (("short", "inc" in sites), ("long", "long" in sites)):
        if reached:
            assert c["session", path, V.TTL] >= FLOOR and c["session", path, V.TTL + 1] >= FLOOR, path
    if "inc" in sites:
        assert c["spanning_overwrites"] >= FLOOR
    if layout == "mixed":
        assert c["after_long", "sorted"] >= FLOOR and c["after_long", "unsorted"] >= FLOOR
        assert c["after_long", "carried_1"] >= 1 and c["after_long", "carried_K"] >= 1


@pytest.mark.parametrize("K", [1, 2, 64])
def test_census_small_and_large_rings_reach_every_site(census, K):
    c = census("mixed", K)
    print(f"census mixed K={K}: {c}")
    for s in V.SITES:
        assert c[s, "rows"] >= 1, s
    assert c["after_long", "sorted"] >= 1 and c["after_long", "unsorted"] >= 1
    assert c["spanning_overwrites"] >= 1


def test_stream_layouts():
    """what the layouts promise: batch sizes, the long-run lengths, the hot run, rows under ~16 k"""
    for K in (3, 16):
        for layout in V.LAYOUTS:
            tx, cuts = V.stream(layout, K)
            assert len(tx["ts_ms"]) <= 16384 and cuts[-1] == len(tx["ts_ms"])
            runs = set()
            for a, b in zip(cuts[:-1], cuts[1:]):
                runs |= set(np.unique(tx["card_key"][a:b], return_counts=True)[1].tolist())
            if layout == "one":
                assert runs == {1}
            elif layout == "short":
                assert runs == set(range(1, 17))
            else:
                assert set(V.LONG_RUNS) | {V.HOT_RUN} <= runs
                assert (min(runs) > V.SEG_LONG) == (layout == "long")


@pytest.mark.parametrize("layout", V.LAYOUTS)
@pytest.mark.parametrize("K", [3, 16])
def test_sensitivity_to_off_by_one(layout, K):
    """Each off-by-one variant of the definition changes at least one row at every site the layout reaches (the
    future-counting one where a future event can be in the ring: full scans and the cooperative path)."""
    tx, cuts = V.stream(layout, K)
    site, _ = V.sites(tx, cuts, K)
    base_c, base_s = V.windows_full_scan(tx, K)
    for name, kw in V.window_mutants(K).items():
        mc, ms = V.windows_full_scan(tx, K, **kw)
        changed = (mc != base_c).any(1) | (ms != base_s).any(1)
        for s in _reached(layout):
            hit = int((changed & (site == V.SITES.index(s))).sum())
            print(f"{layout} K={K} {name} at {s}: {hit} rows")
            if name == "future_counted" and s in ("inc", "rebuild"):
                assert hit == 0
            else:
                assert hit >= 1, (name, s)
    base = V.session_scan(tx)
    mut = V.session_scan(tx, live=operator.lt)
    changed = (mut[0] != base[0]) | (mut[1] != base[1])
    for path, m in (("short", site != 0), ("long", site == 0)):
        if m.any():
            assert (changed & m).any(), ("session_strict", path)
