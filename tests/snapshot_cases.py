"""Where to cut the velocity edge streams (tests/velocity_edge_cases.py) for snapshot -> restore, the CPU census of
the card states those cuts hold, and a host parser of the snapshot image (csrc/snapshot.hip). No GPU.

A stream cut by linspace over Poisson arrivals puts no card into a chosen state at the cut. The states a restore can
get wrong are a property of one card at one batch boundary: how far its ring is filled and where its head stands,
whether it is still unsorted (the rebuild yet to come), whether the first event after the restore lands exactly on a
window edge of an event the image carried in the ring, whether a redis_compat session gap of exactly one TTL (or one
more) spans the cut, and a negative last event time (v3 keeps the oldest in-window times as offsets below it). CUTS
names, per (layout, K), at most four batch boundaries of the edge stream that together hold every one of them;
`census` restates them from the stream alone and tests/test_snapshot_cases_cpu.py asserts that none is missing.

The image layout is stated here once, from SnapHeader (snapshot.hip) and CardHeader / RingEvent (fd_internal.h): a
format pinned by something other than the restore code that reads it."""
import functools

import numpy as np

import velocity_edge_cases as V

PAIRS = (("one", 3), ("one", 16), ("short", 16), ("mixed", 3), ("mixed", 16))

# batch indices b of V.stream(layout, K): the snapshot is taken before batch b (after rows [0, cuts[b]))
CUTS = {
    ("one", 3): (1, 3, 6, 142),
    ("one", 16): (1, 16, 32, 115),
    ("short", 16): (3,),
    ("mixed", 3): (6, 7),
    ("mixed", 16): (6, 9),
}

RING = ("ring_partial", "ring_full", "ring_wrapped_head_mid", "ring_wrapped_head_0")
EDGES = tuple((W, d) for W in V.WINDOWS for d in ("in", "out"))  # first event W - 1 / W ms after a ring event
STATES = RING + ("unsorted", "rebuild") + EDGES + (("session", V.TTL), ("session", V.TTL + 1), "negative_last_ts")
CROSSING = "crosses_zero"


def absent(layout, K):
    """States no batch boundary of (layout, K) holds, whichever cut is chosen. `mixed` opens every card with a long
    run (LONG_RUNS: at least 17 events, more than either K), so at the first boundary every ring has wrapped: no
    partly filled ring and none exactly full; `one` and `short` hold both. `mixed` / 16 has no card with a negative
    last time at a boundary either (its card 0 passes ts = 0 inside a run). The CPU test proves both from the
    stream."""
    out = ("ring_partial", "ring_full") if layout == "mixed" else ()
    return out + (("negative_last_ts",) if (layout, K) == ("mixed", 16) else ())


def required(layout, K):
    """the states the cuts of (layout, K) must hold; the `one` streams also hold the crossing of ts = 0"""
    req = [s for s in STATES if s not in absent(layout, K)]
    return tuple(req) + ((CROSSING,) if layout == "one" else ())


def cuts(layout, K):
    return CUTS[layout, K]


@functools.lru_cache(maxsize=None)
def _per_row(layout, K):
    tx, bounds = V.stream(layout, K)
    et, _, valid = V.prior_events(tx, K)
    site, _ = V.sites(tx, bounds, K)
    seen = np.zeros(len(tx["ts_ms"]), np.int64)  # events of the row's card before it
    count = {}
    for i, k in enumerate(tx["card_key"].tolist()):
        seen[i] = count.get(k, 0)
        count[k] = seen[i] + 1
    return et, valid, site, seen


def first_rows(tx, bounds, b):
    """the first row of each card in batch b"""
    a, e = bounds[b], bounds[b + 1]
    _, idx = np.unique(tx["card_key"][a:e], return_index=True)
    return a + np.sort(idx)


def census(tx, bounds, K, chosen, per_row=None):
    """-> dict state -> number of cards in it, over the first row of each card in the batch that follows each chosen
    cut. The state at the cut is what the image carries for the card: ring fill and head from its event count,
    `unsorted` from the site V.sites gives the row (a row that is no descent and still scans in full meets
    unsorted > 0; the one at which it returns to 0 is the rebuild), the window edges from the row's distance to the
    K events before it (all of them are in the restored ring), the session gap from the distance to the last one."""
    if per_row is None:
        et, _, valid = V.prior_events(tx, K)
        site, _ = V.sites(tx, bounds, K)
        seen = np.zeros(len(tx["ts_ms"]), np.int64)
        count = {}
        for i, k in enumerate(tx["card_key"].tolist()):
            seen[i] = count.get(k, 0)
            count[k] = seen[i] + 1
    else:
        et, valid, site, seen = per_row
    out = dict.fromkeys(STATES + (CROSSING,), 0)
    for b in chosen:
        assert 0 < b < len(bounds) - 1, "a cut lies between two batches"
        rows = first_rows(tx, bounds, b)
        rows = rows[seen[rows] > 0]  # cards the image holds events of
        n, t = seen[rows], tx["ts_ms"][rows]
        dt = t[:, None] - et[rows]
        ok = valid[rows]
        last = et[rows, 0]
        out["ring_partial"] += int((n < K).sum())
        out["ring_full"] += int((n == K).sum())
        out["ring_wrapped_head_mid"] += int(((n > K) & (n % K != 0)).sum())
        out["ring_wrapped_head_0"] += int(((n > K) & (n % K == 0)).sum())
        short = site[rows] != V.SITES.index("long")
        scans = short & (site[rows] != V.SITES.index("inc")) & (t >= last)
        out["unsorted"] += int(scans.sum())
        out["rebuild"] += int((scans & (site[rows] == V.SITES.index("rebuild"))).sum())
        for W in V.WINDOWS:
            out[W, "in"] += int((ok & (dt == W - 1)).any(1).sum())
            out[W, "out"] += int((ok & (dt == W)).any(1).sum())
        for gap in (V.TTL, V.TTL + 1):
            out["session", gap] += int((dt[:, 0] == gap).sum())
        out["negative_last_ts"] += int((last < 0).sum())
        out[CROSSING] += int(((last < 0) & (t >= 0)).sum())
    return out


def stream_census(layout, K, chosen):
    tx, bounds = V.stream(layout, K)
    return census(tx, bounds, K, chosen, _per_row(layout, K))


def greedy_cover(layout, K, limit=4):
    """how CUTS was found: the boundary that adds the most missing states, until none is missing"""
    tx, bounds = V.stream(layout, K)
    need, chosen = set(required(layout, K)), []
    per = {b: {s for s, c in stream_census(layout, K, (b,)).items() if c} for b in range(1, len(bounds) - 1)}
    while need and len(chosen) < limit:
        b = max(per, key=lambda q: (len(per[q] & need), -q))
        if not per[b] & need:
            break
        chosen.append(b)
        need -= per[b]
    return tuple(sorted(chosen)), need


# ---------------------------------------------------------------------------------------------------------------
# the image: a 256-B header, n_cards records, the replicated tables, the window logs, the extension sections

IMAGE_HEADER_BYTES = 256
IMAGE_VERSION = 3
SNAP_HEADER = np.dtype({  # SnapHeader, packed, little-endian
    "names": ["magic", "version", "header_bytes", "window_mode", "ring_k", "seq_len", "has_uext", "shard", "n_shards",
              "vocab_loaded", "windows_present", "n_cards", "record_bytes", "n_merchants", "n_mext", "tp_threshold",
              "win_ooo", "win_wm", "win_min_seen", "win_max_seen", "ucount", "mcount", "checksum", "ext_flags",
              "ext_checksum"],
    "formats": ["S8", "<u4", "<u4", "<i4", "<i4", "<i4", "<i4", "<i4", "<i4", "<i4", "<i4", "<i8", "<i8", "<i8", "<i8",
                "<f8", "<i8", "<i8", "<i8", "<i8", "<i8", "<i8", ("<u8", 6), "<i4", "<u8"],
    "offsets": [0, 8, 12, 16, 20, 24, 28, 32, 36, 40, 44, 48, 56, 64, 72, 80, 88, 96, 104, 112, 120, 128, 136, 184,
                192],
    "itemsize": IMAGE_HEADER_BYTES})
CARD_HEADER_BYTES = 128
CARD_HEADER = np.dtype({  # the v3 CardHeader: what a transaction rewrites in bytes 0-63, the key at byte 64
    "names": ["last_ts", "ring_n", "ring_head", "unsorted", "wc", "flags", "rc_cnt", "ws", "wod", "key", "avg", "age",
              "fp"],
    "formats": ["<i8", "u1", "u1", "u1", ("u1", 3), "<u4", "<i4", ("<i8", 3), ("<u4", 3), "<u8", "<f8", "<i4",
                ("<u8", 3)],
    "offsets": [0, 8, 9, 10, 12, 16, 20, 24, 48, 64, 72, 80, 88],
    "itemsize": CARD_HEADER_BYTES})
RING_EVENT = np.dtype([("ts", "<i8"), ("cents", "<i8")])  # 16 B; K of them follow the header (zero in redis_compat)


def record_bytes(K, seq_len, has_uext):
    """header | K ring events | seq_len x 16 f32 LSTM history | 48-B extended profile"""
    return CARD_HEADER_BYTES + 16 * K + 64 * seq_len + (48 if has_uext else 0)


def parse_image(blob):
    """-> (header record, card headers [n_cards], ring events [n_cards, K])"""
    hd = np.frombuffer(blob, SNAP_HEADER, 1)[0]
    n, rb, K = int(hd["n_cards"]), int(hd["record_bytes"]), int(hd["ring_k"])
    assert len(blob) >= IMAGE_HEADER_BYTES + n * rb
    recs = np.frombuffer(blob, np.uint8, n * rb, IMAGE_HEADER_BYTES).reshape(n, rb)
    cards = np.ascontiguousarray(recs[:, :CARD_HEADER_BYTES]).view(CARD_HEADER).reshape(n)
    ring = np.ascontiguousarray(recs[:, CARD_HEADER_BYTES:CARD_HEADER_BYTES + 16 * K]).view(RING_EVENT).reshape(n, K)
    return hd, cards, ring
