"""CPU: known answers of the RedisTransactionSink aggregate restatement (oracle/sink_ref.py;
RedisTransactionSink.java:140-262)."""
from oracle.sink_ref import SinkOracle, java_div

H = 3_600_000


def test_java_division_truncates():
    assert java_div(7, 2) == 3 and java_div(-7, 2) == -3 and java_div(-1, H) == 0


def test_hourly_daily_merchant_known_answers():
    o = SinkOracle()
    t0 = 1_757_030_400_000  # 2025-09-05T00:00:00Z, an hour and day boundary
    o.process(11, 10.0, t0 + 5, 3, False, 0.9)
    o.process(11, 2.5, t0 + H - 1, 3, True, None)
    o.process(12, 1.25, t0 + H, 3, False, 0.7)      # next hour; 0.7 is not > 0.7
    o.process(13, 4.0, t0 + 2 * H, None, True, 0.71)  # merchantId null: no merchant aggregation
    h0, h1, h2 = t0 // H, t0 // H + 1, t0 // H + 2
    a = o.redis[f"hourly:{h0}"]
    assert (a["total_count"], a["total_amount"], a["fraud_count"], a["high_risk_count"]) == (2, 12.5, 1, 1)
    assert a["fraud_rate"] == 0.5 and a["avg_amount"] == 6.25
    assert o.redis[f"hourly:{h1}"]["high_risk_count"] == 0
    assert o.redis[f"hourly:{h2}"]["high_risk_count"] == 1
    d = o.redis[f"daily:{t0 // 86_400_000}"]
    assert (d["total_count"], d["fraud_count"]) == (4, 2) and d["total_amount"] == 17.75
    m = o.redis[f"merchant:3:{h0}"]
    assert m["unique_user_count"] == 1 and m["total_count"] == 2
    assert f"merchant:None:{h2}" not in o.redis and not any(k.endswith(f":{h2}") and k.startswith("merchant")
                                                             for k in o.redis)


def test_negative_times_truncate_toward_zero_and_score_edge():
    """hour key 0 takes (-3 600 000, 3 600 000) and day key 0 (-86 400 000, 86 400 000): Java long division;
    fraudScore > 0.7 is strict, a null score counts nothing"""
    import numpy as np
    up = float(np.nextafter(0.7, 1.0))
    o = SinkOracle()
    o.process(1, 1.0, -(H - 1), 2, False, 0.7)
    o.process(1, 2.0, H - 1, 2, True, up)
    o.process(2, 4.0, -H, 2, False, None)
    o.process(2, 8.0, H, None, False, 0.71)
    o.process(3, 16.0, -86_400_000, 2, False, None)
    a = o.redis["hourly:0"]
    assert (a["total_count"], a["total_amount"], a["fraud_count"], a["high_risk_count"]) == (2, 3.0, 1, 1)
    assert o.redis["hourly:-1"]["total_count"] == 1 and o.redis["hourly:1"]["high_risk_count"] == 1
    assert o.redis["hourly:-24"]["total_count"] == 1
    assert o.redis["daily:0"]["total_count"] == 4 and o.redis["daily:-1"]["total_count"] == 1
    assert o.redis["merchant:2:0"]["unique_user_count"] == 1 and o.redis["merchant:2:-1"]["total_count"] == 1
    assert "merchant:None:1" not in o.redis


def test_edge_batches_hold_every_edge():
    import numpy as np

    import window_edge_cases as WE
    ts = np.concatenate([b["ts_ms"] for b in WE.sink_batches()])
    for unit in (H, 86_400_000):
        for s in (-1, 1):
            assert {s * (unit - 1), s * unit, s * (unit + 1)} <= set(ts.tolist())
    assert {-1, 0, 1} <= set(ts.tolist())
    sc = np.concatenate([b["fraud_score"] for b in WE.sink_batches()])
    assert (sc == 0.7).any() and (sc == WE.SCORE_UP).any() and np.isnan(sc).any()
