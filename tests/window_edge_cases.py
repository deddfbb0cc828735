"""Micro-batches for the Flink window aggregates (csrc/windows.hip) and the sink aggregates (csrc/sink.hip) with
event times, watermarks and values exactly on the edges their comparisons test. synth.window_stream draws times
and amounts at random, so it almost never puts one there.

watermark_batches(base): around user window ends E = base + k * 60 000 (k = 60: also a merchant window end) three
batches each, whose largest event time puts the watermark (max - 10 000 - 1) on E - 2, E - 1 and E. Every batch
carries events at E - 300 000, E - 240 000, E - 60 000 and E, each -1 / 0 / +1 ms, so the same events are on time in
the first batch, late but kept by their newest window in the second (its end - 1 == w_prev + 1) and dropped in the
third (end - 1 == w_prev); the event at E - 300 000 sits on the compaction edge (w_new + 2 - size) of the first
batch and is still needed by the window that fires in the second, the one 1 ms below it is compacted away. base 0
puts events at negative times (floor division, the hour that ends at 0).

threshold_batches(base): one batch whose windows hold exactly the counts, sums and ratios that the velocity and
merchant risk scores compare with, one below and one above; fraud scores of 0.7, the next float up and NaN.

sink_batches(): event times around 0, +-1 h and +-1 day (the sink's hour and day keys truncate toward zero)."""
import numpy as np

USER_SIZE, SLIDE, HOUR, DAY, LAG = 300_000, 60_000, 3_600_000, 86_400_000, 10_000
T0 = 1_756_684_800_000  # a multiple of one hour
STEPS = (1, 2, 5, 6, 58, 59, 60, 61, 65)
SCORE_UP = float(np.nextafter(0.7, 1.0))
SCORES = (0.7, SCORE_UP, float("nan"), 0.0, 0.9)


def _batch(rows):
    """rows: (key, ts, cents, merchant, payment method, is_fraud, fraud_score)"""
    cols = list(zip(*rows)) if rows else [[]] * 7
    return dict(key=np.array(cols[0], np.uint64), ts_ms=np.array(cols[1], np.int64),
                amount_cents=np.array(cols[2], np.int64), merchant=np.array(cols[3], np.int32),
                payment_method=np.array(cols[4], np.uint8), is_fraud=np.array(cols[5], np.uint8),
                fraud_score=np.array(cols[6], np.float64))


def watermark_batches(base):
    out, q = [], 0
    for k in STEPS:
        E = base + k * SLIDE
        for top in (E + LAG - 1, E + LAG, E + LAG + 1):  # watermark -> E - 2, E - 1, E
            rows = []
            for off in (-USER_SIZE, -USER_SIZE + SLIDE, -SLIDE, 0):
                for d in (-1, 0, 1, SLIDE - 1):
                    for key in (7, 8, 9):
                        q += 1
                        if E + off + d > top:
                            continue
                        rows.append((key, E + off + d, 100 + 37 * q % 5000, (q + key) % 3 - 1, (0, 3, 255)[q % 3],
                                     q % 7 == 0, SCORES[q % len(SCORES)]))
            rows.append((7, top, 4242, 1, 2, 0, 0.5))  # the batch's largest event time
            out.append(_batch(rows))
    return out


def threshold_batches(base):
    rows, ts, q = [], base + 2 * SLIDE, 0

    def add(key, n, cents, merchants, users=None):
        nonlocal q
        for i in range(n):
            q += 1
            c = cents[i] if isinstance(cents, (list, tuple)) else cents
            rows.append(((key if users is None else users[i % len(users)]), ts + q % (SLIDE - 1), c,
                         merchants[i % len(merchants)], i % 4, i % 11 == 0, SCORES[i % len(SCORES)]))

    # user windows: counts 5 / 6, 10 / 11, 20 / 21 with unique_merchants / count 0.2 exactly and just below
    for key, n, nm in ((101, 5, 1), (102, 6, 1), (103, 10, 2), (104, 11, 2), (105, 20, 4), (106, 21, 4)):
        add(key, n, 150, list(range(20, 20 + nm)))
    # sums of exactly 100 000 / 100 001, 500 000 / 500 001, 1 000 000 / 1 000 001 cents
    for key, total in ((111, 100_000), (112, 100_001), (113, 500_000), (114, 500_001), (115, 1_000_000),
                       (116, 1_000_001)):
        add(key, 2, [total // 2, total - total // 2], [30, 31])
    # merchant windows: 500 / 501 and 1 000 / 1 001 events, unique_users / count 0.1 exactly and just below
    for m, n, nu in ((40, 500, 50), (41, 501, 50), (42, 1000, 100), (43, 1001, 100)):
        add(None, n, 700 + m, [m], users=[10_000 + 1000 * m + u for u in range(nu)])
    return [_batch(rows)]


def sink_batches():
    rows, q = [], 0
    for unit in (HOUR, DAY):
        for s in (-1, 1):
            for t in (unit - 1, unit, unit + 1, 1):
                for sc in SCORES:
                    q += 1
                    rows.append((50 + q % 3, s * t, 1000 + q, q % 4 - 1, 0, q % 2, sc))
    rows += [(50, 0, 5, 2, 0, 0, sc) for sc in SCORES]
    return [_batch(rows[:len(rows) // 2]), _batch(rows[len(rows) // 2:])]


def _floor(ts, size):
    return ts // size * size


def time_edges(batches):
    """Counts of the time edges in a stream, by the micro-batch watermark rule (watermark advances after the
    batch's elements are assigned; an element's window is dropped when its end - 1 <= the watermark before the
    batch)."""
    c = dict.fromkeys(("user_wm_end-2", "user_wm_end-1", "user_wm_end", "merchant_wm_end-2", "merchant_wm_end-1",
                       "merchant_wm_end", "user_late_dropped", "user_late_kept", "merchant_late_dropped",
                       "merchant_late_kept", "user_compacted", "user_kept_and_needed", "merchant_compacted",
                       "merchant_kept_and_needed", "negative_ts", "on_slide", "below_slide", "above_slide"), 0)
    wm, seen, log = None, None, []
    for b in batches:
        ts = [int(t) for t in b["ts_ms"]]
        for t, m in zip(ts, b["merchant"]):
            c["negative_ts"] += t < 0
            c["on_slide"] += t % SLIDE == 0
            c["below_slide"] += t % SLIDE == SLIDE - 1
            c["above_slide"] += t % SLIDE == 1
            if wm is not None:
                u_end, m_end = _floor(t, SLIDE) + USER_SIZE, _floor(t, HOUR) + HOUR
                c["user_late_dropped"] += u_end - 1 == wm
                c["user_late_kept"] += u_end - 1 == wm + 1
                if m >= 0:
                    c["merchant_late_dropped"] += m_end - 1 == wm
                    c["merchant_late_kept"] += m_end - 1 == wm + 1
        log += [(t, int(m)) for t, m in zip(ts, b["merchant"])]
        seen = max(ts + ([seen] if seen is not None else []))
        new = seen - LAG - 1
        if wm is not None and new <= wm:
            continue
        wm = new
        for name, size in (("user", SLIDE), ("merchant", HOUR)):
            for d in (2, 1, 0):
                c[f"{name}_wm_end" + (f"-{d}" if d else "")] += (wm + d) % size == 0
        for t, m in log:  # what the compaction after this batch meets
            c["user_compacted"] += t == wm + 1 - USER_SIZE
            c["user_kept_and_needed"] += t == wm + 2 - USER_SIZE and _floor(t, SLIDE) + USER_SIZE - 1 > wm
            if m >= 0:
                c["merchant_compacted"] += t == wm + 1 - HOUR
                c["merchant_kept_and_needed"] += t == wm + 2 - HOUR and _floor(t, HOUR) + HOUR - 1 > wm
    return c


def oracle_batch(b):
    """a batch as oracle.windows_ref.WindowOracle.step takes it"""
    return [dict(key=int(b["key"][i]), ts=int(b["ts_ms"][i]), cents=int(b["amount_cents"][i]),
                 merchant=int(b["merchant"][i]), pm=int(b["payment_method"][i]), fraud=bool(b["is_fraud"][i]),
                 score=float(b["fraud_score"][i])) for i in range(len(b["key"]))]
