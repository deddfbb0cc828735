"""CPU: the cuts tests/test_gpu_snapshot_oracle.py takes through the velocity edge streams hold the card states a
snapshot -> restore can get wrong (tests/snapshot_cases.py), proved from the streams alone; the image parser reads
the byte offsets the v3 format states."""
import struct

import numpy as np
import pytest

import snapshot_cases as S
import velocity_edge_cases as V


@pytest.mark.parametrize("layout,K", S.PAIRS)
def test_cuts_hold_every_state(layout, K):
    _, bounds = V.stream(layout, K)
    chosen = S.cuts(layout, K)
    assert 1 <= len(chosen) <= 4 and len(set(chosen)) == len(chosen)
    assert all(0 < b < len(bounds) - 1 for b in chosen)
    c = S.stream_census(layout, K, chosen)
    missing = [s for s in S.required(layout, K) if c[s] == 0]
    assert not missing, f"{layout}/{K}: no card at the cuts {chosen} in {missing}"


@pytest.mark.parametrize("layout,K", S.PAIRS)
def test_states_not_required_exist_at_no_boundary(layout, K):
    """a state is left out for a pair only where no cut could hold it"""
    _, bounds = V.stream(layout, K)
    everywhere = S.stream_census(layout, K, tuple(range(1, len(bounds) - 1)))
    for s in S.absent(layout, K):
        assert everywhere[s] == 0, (layout, K, s)
    assert set(S.required(layout, K)) | set(S.absent(layout, K)) >= set(S.STATES)


def test_every_state_is_held_by_some_pair_and_the_one_streams_hold_all():
    for s in S.STATES + (S.CROSSING,):
        assert any(s in S.required(layout, K) for layout, K in S.PAIRS)
    for K in (3, 16):
        assert not S.absent("one", K) and S.CROSSING in S.required("one", K)
    # `mixed`: every card's ring has wrapped at the first boundary (the reason its two ring states are absent)
    for K in (3, 16):
        tx, bounds = V.stream("mixed", K)
        _, n = np.unique(tx["card_key"][:bounds[1]], return_counts=True)
        assert len(n) == len(np.unique(tx["card_key"])) and n.min() > K


@pytest.mark.parametrize("layout,K", S.PAIRS)
def test_every_cut_is_needed(layout, K):
    """the census notices a moved cut: without any one of the chosen cuts a required state has no card"""
    chosen = S.cuts(layout, K)
    for drop in chosen:
        c = S.stream_census(layout, K, tuple(b for b in chosen if b != drop))
        assert any(c[s] == 0 for s in S.required(layout, K)), (layout, K, drop)


def test_cuts_are_the_greedy_cover():
    for layout, K in S.PAIRS:
        found, left = S.greedy_cover(layout, K)
        assert not left and found == S.cuts(layout, K)


def test_census_restates_the_states_on_a_hand_made_stream():
    """two cards, K = 2, one event per card per batch: counts known by hand"""
    K, W5, TTL = 2, V.W5, V.TTL
    a = [0, 10, 5, W5 + 4, W5 + 5]                # descent at event 2; ring full at cut 2, wrapped head 1 at cut 3
    b = [-TTL - 5, -5, TTL - 5, TTL - 4, 2 * TTL - 3]  # session gaps TTL, .., TTL + 1; negative until event 2
    tx = {"card_key": np.array([1, 2] * 5, np.uint64), "ts_ms": np.array([t for p in zip(a, b) for t in p], np.int64),
          "amount_cents": np.arange(10, dtype=np.int64) + 100}
    bounds = tuple(range(0, 11, 2))
    c = S.census(tx, bounds, K, (1,))
    assert c["ring_partial"] == 2 and c["ring_full"] == 0 and c["negative_last_ts"] == 1
    assert c["session", TTL] == 1 and c["unsorted"] == 0
    c = S.census(tx, bounds, K, (2,))   # card 1's next event is a descent (unknown), card 2 crosses zero with gap TTL
    assert c["ring_full"] == 2 and c[S.CROSSING] == 1 and c["session", TTL] == 1 and c["unsorted"] == 0
    c = S.census(tx, bounds, K, (3,))   # card 1: unsorted = 2 at the cut, first event W5 - 1 after the one at 5
    assert c["ring_wrapped_head_mid"] == 2 and c["unsorted"] == 1 and c["rebuild"] == 0
    assert c[W5, "in"] == 1 and c[W5, "out"] == 0
    c = S.census(tx, bounds, K, (4,))   # card 1: unsorted = 1, the rebuild, W5 after the 5; card 2: gap TTL + 1
    assert c["ring_wrapped_head_0"] == 2 and c["unsorted"] == 1 and c["rebuild"] == 1
    assert c[W5, "out"] == 1 and c["session", TTL + 1] == 1


def test_image_parser_reads_the_v3_offsets():
    """the record the v3 layout spells out with struct (tests/test_gpu_snapshot.py _downgrade_to_v2 reads the same
    offsets), parsed back field by field"""
    K, n = 3, 2
    hd = bytearray(256)
    struct.pack_into("<8sII8i4qd6q", hd, 0, b"FDSNAP\x00\x01", 3, 256, 1, K, 0, 0, 0, 1, 1, 0, n,
                     S.record_bytes(K, 0, False), 50, 0, 0.65, 10000, 7, -8, 9, 0, 0)
    struct.pack_into("<6Q", hd, 136, *range(11, 17))
    struct.pack_into("<iiQ", hd, 184, 2, 0, 99)
    recs = b""
    for r in range(n):
        recs += struct.pack("<q8BIi3q3II", -5 - r, 2, 1, 3, 0, 4, 5, 6, 0, 0x0201, 7, 100, 200, 300, 1, 2, 3, 0)
        recs += struct.pack("<Qdii3Q2q", 1000 + r, 12.5, 77, 0, 21, 22, 23, 0, 0)
        recs += b"".join(struct.pack("<qq", 10 * r + e, 500 + e) for e in range(K))
    h, cards, ring = S.parse_image(bytes(hd) + recs + b"tail")
    assert (h["version"], h["header_bytes"], h["window_mode"], h["ring_k"], h["seq_len"], h["has_uext"]) == \
           (3, 256, 1, K, 0, 0)
    assert (h["n_shards"], h["vocab_loaded"], h["n_cards"], h["record_bytes"], h["n_merchants"]) == (1, 1, n, 176, 50)
    assert h["tp_threshold"] == 0.65 and (h["win_ooo"], h["win_wm"], h["win_min_seen"], h["win_max_seen"]) == \
           (10000, 7, -8, 9)
    assert h["checksum"].tolist() == list(range(11, 17)) and h["ext_flags"] == 2 and h["ext_checksum"] == 99
    assert cards["last_ts"].tolist() == [-5, -6] and cards["key"].tolist() == [1000, 1001]
    assert (cards["ring_n"][0], cards["ring_head"][0], cards["unsorted"][0]) == (2, 1, 3)
    assert cards["wc"][0].tolist() == [4, 5, 6] and cards["flags"][0] == 0x0201 and cards["rc_cnt"][0] == 7
    assert cards["ws"][0].tolist() == [100, 200, 300] and cards["wod"][0].tolist() == [1, 2, 3]
    assert cards["avg"][0] == 12.5 and cards["age"][0] == 77 and cards["fp"][0].tolist() == [21, 22, 23]
    assert ring["ts"].tolist() == [[0, 1, 2], [10, 11, 12]] and ring["cents"][1].tolist() == [500, 501, 502]
    assert S.record_bytes(8, 10, True) == 128 + 128 + 640 + 48
