"""CPU: the JSON ingest codec — the scalar conversions of ingest_parse.h, evaluated on the host
through fd_ingest_scalar_host, pinned against Python's own correctly rounded float(), decimal.Decimal and datetime;
the identity hash; and known answers of the oracle (oracle/ingest_ref.py) on simulator-format messages
(services/data-simulator/src/main/python/simulator.py:186) and on the shared scalar cases
(tests/ingest_scalar_cases.py). The device kernel shares decimal_to_double, decimal_to_cents and the calendar
arithmetic with this host code but scans numbers, instants, hours, booleans and locations with code of its own
(ingest.hip: scan_number_w, parse_iso_w, scan_latlon); tests/test_gpu_ingest_scalars.py pins those on the same cases.
Bars: bit-exact (doubles compared as bit patterns, cents and epoch ms as integers)."""
import ctypes as C
import datetime as dt
import json
import math
import struct

import numpy as np
import pytest

import ingest_scalar_cases as K
from oracle import ingest_ref as R

_number_corpus = K.number_corpus


def _scalar(kind, text):
    from fdengine import _native as N
    b = text.encode() if isinstance(text, str) else text
    arr = np.frombuffer(b, np.uint8) if b else np.zeros(1, np.uint8)
    f, i, fl = C.c_double(), C.c_int64(), C.c_int32()
    N.call("fd_ingest_scalar_host", kind, C.c_void_p(arr.ctypes.data), len(b), C.byref(f), C.byref(i), C.byref(fl))
    return f.value, i.value, fl.value


def _bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def test_decimal_to_double_matches_python_float():
    rng = np.random.default_rng(1)
    corpus = _number_corpus(rng, 40000) + K.NUMBER_SPECIALS
    corpus += K.long_mantissas(np.random.default_rng(11), 6000) + K.boundary_numbers(np.random.default_rng(12))
    bad = []
    n_many = n_amb = 0
    for s in corpus:
        if not R.NUMBER_RE.match(s):
            continue
        v, _, fl = _scalar(0, s)
        assert not (fl & 1), s
        # the declared rule: the first 19 significant digits, flagged when the dropped ones could matter
        exp, inexact = R.f64_of(s)
        if _bits(v) != _bits(exp) or bool(fl & 2) != inexact:
            bad.append((s, v, exp, fl, inexact))
        # ... which is the correctly rounded value whenever the flag is clear
        if not inexact and _bits(exp) != _bits(float(s)):
            bad.append((s, exp, float(s)))
        n_many += R._sig_digits(s) > 19
        n_amb += inexact
    assert not bad, bad[:5]
    assert n_many > 5000 and n_amb > 500, (n_many, n_amb)


def test_number_grammar_errors():
    for s in ["", "-", "01", "1.", ".5", "1e", "1e+", "+1", "0x10", "1.5e3.2", "NaN", "Infinity", " 1"]:
        assert _scalar(0, s)[2] & 1, s
    for s in K.bad_numbers():
        assert _scalar(0, s)[2] & 1 and not R.NUMBER_RE.match(s), s


def test_cents_exact():
    from decimal import Decimal
    rng = np.random.default_rng(2)
    cases = [f"{rng.integers(0, 10**9)}.{rng.integers(0, 100):02d}" for _ in range(5000)]
    cases += ["1", "1.5", "0.005", "0.015", "0.025", "-3.335", "12.3", "1e2", "1.23e1", "99999999999999.99",
              "0.0000001", "7.125", "2.675"]
    for s in cases:
        _, c, fl = _scalar(1, s)
        ec, inexact = R.cents_of(Decimal(s))
        assert c == ec and bool(fl & 2) == inexact, (s, c, ec)


def test_cents_of_the_number_corpus():
    """amounts of any length and exponent: the host conversion against the oracle's exact cents of the first 19
    significant digits, and against the full Decimal wherever nothing was dropped"""
    from decimal import Decimal
    corpus = _number_corpus(np.random.default_rng(21), 6000) + K.NUMBER_SPECIALS
    corpus += K.long_mantissas(np.random.default_rng(22), 3000) + K.boundary_numbers(np.random.default_rng(23))
    corpus += ["0.12500000000000000001", "0.1250000000000000000", "61902604193838002.5165", "92233720368547758.07",
               "92233720368547758.08", "-92233720368547758.07", "1e27", "1e400", "0e400", "1e-400"]
    n_ok = n_many = 0
    for s in corpus:
        _, c, fl = _scalar(1, s)
        try:
            ec, inexact = R.amount_of(s)
        except R.Malformed:
            assert fl & 1, s
            continue
        assert not (fl & 1) and c == ec and bool(fl & 2) == inexact, (s, c, ec, fl)
        n_ok += 1
        if R._sig_digits(s) <= 19:
            assert (ec, inexact) == R.cents_of(Decimal(s)), s
        else:
            n_many += 1
            assert inexact, s
    assert n_ok > 4000 and n_many > 300, (n_ok, n_many)
    # the 19-digit view drops the digit that would break this tie upward: 12 cents, flagged
    assert R.amount_of("0.12500000000000000001") == (12, True) and R.amount_of("0.125") == (12, True)
    assert R.amount_of("0.1250000000000000001") == (13, True)  # 19 digits: seen


def test_iso_instants():
    rng = np.random.default_rng(3)
    for _ in range(3000):
        us = int(rng.integers(0, 4_102_444_800_000_000))
        t = dt.datetime(1970, 1, 1) + dt.timedelta(microseconds=us)
        s = t.isoformat()
        _, ms, fl = _scalar(2, s)
        assert fl == 0 and ms == us // 1000, s
        z = s + ("Z" if us % 2 else "+05:30")
        _, ms2, fl2 = _scalar(2, z)
        assert fl2 == 0 and ms2 == R.iso_to_ms(z), z
    for bad in ["2025-02-29T00:00:00", "2025-13-01T00:00:00", "2025-01-01 00:00:00", "2025-01-01T24:00:00",
                "2025-01-01T00:00:00.", "2025-01-01T00:00:00.1234567890", "2025-01-01T00:00:00+5:30", "x"]:
        assert _scalar(2, bad)[2] == 1 and R.iso_to_ms(bad) is None, bad
    assert _scalar(2, "2024-02-29T12:00:00.999999999-01:00")[1] == R.iso_to_ms("2024-02-29T12:00:00.999999999-01:00")


def test_hash64_matches_oracle():
    from fdengine.ingest import hash64
    for s in ["", "user_89346311", "é中", "\U0001F600", "a" * 1000]:
        assert hash64(s) == R.h64(s.encode("utf-8"))


def test_oracle_known_answers_simulator_message():
    from fdengine import synth
    sp = synth.sim_population(50, 10, seed=1)
    msg = synth.json_messages(sp, 1, seed=2)[0]
    doc = json.loads(msg)
    merchants = {m: i for i, m in enumerate(sp["merchant_ids"])}
    vocabs = [{s: i for i, s in enumerate(v)} for v in (synth.SIM_PAYMENT_METHODS, synth.SIM_TXN_TYPES,
                                                         synth.SIM_CARD_TYPES)]
    row = R.parse_message(msg, merchants, vocabs)
    assert row["status"] == 0
    assert row["card_key"] == R.h64(doc["user_id"].encode())
    assert row["amount_cents"] == round(doc["amount"] * 100)
    t = dt.datetime.fromisoformat(doc["timestamp"]).replace(tzinfo=dt.timezone.utc)
    assert row["ts_ms"] == int(t.timestamp() * 1000) // 1 or abs(row["ts_ms"] - t.timestamp() * 1000) < 1
    assert row["merchant"] == merchants.get(doc["merchant_id"], -1)
    assert row["geo_lat"] == doc["geolocation"]["lat"]
    assert row["merchant_lat"] == float(doc["merchant_location"]["lat"])  # Decimal -> str on the wire
    assert row["payment_method"] == vocabs[0][doc["payment_method"]]
    assert row["hour"] == doc["hour_of_day"] and row["weekend"] == int(doc["is_weekend"])
    assert row["is_fraud"] == int(doc["is_fraud"]) and row["fraud_score"] == doc["fraud_score"]


@pytest.mark.parametrize("raw,status", [
    (b'{"user_id": "u", "amount": 1, "timestamp": "2025-01-01T00:00:00"}', 0),
    (b'{"user_id": "u", "amount": 1}', R.MISSING),
    (b'{"user_id": null, "amount": 1, "timestamp": "2025-01-01T00:00:00"}', R.MISSING),
    (b'{"user_id": "u", "amount": 1, "timestamp": "2025-01-01T00:00:00",}', R.MALFORMED),
    (b'[1, 2]', R.MALFORMED),
    (b'{"user_id": "u", "amount": NaN, "timestamp": "2025-01-01T00:00:00"}', R.MALFORMED),
    (b'{"user_id": "u", "amount": 1, "timestamp": "2025-01-01T00:00:00"} x', R.MALFORMED),
    (b'{"user_id": "u", "amount": "1.005", "timestamp": "2025-01-01T00:00:00"}', R.INEXACT),
    (b'{"user_id": "u", "amount": 1, "timestamp": "2025-01-01T00:00:00", "payment_method": "crypto"}',
     R.UNKNOWN_VOCAB),
    (b'{"user_id": "u", "amount": 1, "timestamp": "2025-01-01T00:00:00", "hour_of_day": -1}', R.MALFORMED),
    (b'{"userId": "u", "amount": 1, "timestamp": "2025-01-01T00:00:00Z", "user_id": "v"}', 0),
])
def test_oracle_status(raw, status):
    row = R.parse_message(raw, {}, [{"credit_card": 0}, {}, {}])
    assert row["status"] == status
    if raw.endswith(b'"user_id": "v"}'):
        assert row["card_key"] == R.h64(b"v")  # the last alias wins


def test_oracle_amount_edge():
    row = R.parse_message(b'{"user_id": "u", "amount": "12.30", "timestamp": "2025-01-01T00:00:00"}', {}, [{}] * 3)
    assert row["amount_cents"] == 1230 and row["status"] == 0
    assert math.isnan(row["geo_lat"]) and row["merchant"] == -1 and row["hour"] == 255


# ---- the shared scalar cases through the oracle alone (and the host scanners), against answers computed independently

def _row(raw):
    return R.parse_message(raw, {}, [{}] * 3)


def test_oracle_instants_known_answers():
    cases = K.random_instants() + K.fraction_instants() + K.edge_instants()
    assert sum(ms is None for _, ms in cases) > 80 and len(cases) > 6100
    for text, ms in cases:
        assert R.iso_to_ms(text) == ms, text
        _, got, fl = _scalar(2, text)
        assert (fl == 1) if ms is None else (fl == 0 and got == ms), text
        row = _row(K.message(timestamp=json.dumps(text, ensure_ascii=False)))
        assert (row["status"], row["ts_ms"]) == ((R.MALFORMED, 0) if ms is None else (0, ms)), text
    # datetime's own parser on the forms every Python version reads: no Z, a fraction of 0, 3 or 6 digits
    n_read = 0
    for text, ms in K.fraction_instants() + K.random_instants()[:400]:
        if ms is None or text[-1] in "Zz" or len(text[19:].split("+")[0].split("-")[0]) not in (0, 4, 7):
            continue
        n_read += 1
        t = dt.datetime.fromisoformat(text)
        if t.tzinfo is None:
            t = t.replace(tzinfo=dt.timezone.utc)
        assert (t - dt.datetime(1970, 1, 1, tzinfo=dt.timezone.utc)) // dt.timedelta(milliseconds=1) == ms, text
    assert n_read > 300


def test_oracle_hours_and_booleans_known_answers():
    from decimal import Decimal
    for text in K.HOUR_TEXTS:
        d = Decimal(text)
        exp = None if (d < 0 or int(d) > 254) else int(d)  # truncation toward zero, 0..254; -0 is zero
        for raw in (text, f'"{text}"'):
            row = _row(K.message(hour_of_day=raw))
            assert (row["status"], row["hour"]) == ((R.MALFORMED, 255) if exp is None else (0, exp)), raw
    assert _row(K.message(hour_of_day='"2\\u0033"'))["hour"] == 23  # spelled with an escape
    for raw, exp in K.BOOL_CASES:
        for field, col, dflt in (("is_weekend", "weekend", 255), ("is_fraud", "is_fraud", 0)):
            row = _row(K.message(**{field: raw}))
            assert (row["status"], row[col]) == ((R.MALFORMED, dflt) if exp is None else (0, exp)), raw


def test_oracle_locations_known_answers():
    for tmpl, has_lat, has_lon in K.LOCATION_SHAPES:
        for a, b in (("1.5", "-2.25"), ('"3.000001"', '"-4.5"'), ("1e-7", '"12345678901234567890.5"')):
            row = _row(K.message(geolocation=tmpl.format(a=a, b=b)))
            if has_lat is None:
                assert row["status"] == R.MALFORMED, tmpl
                continue
            assert row["status"] == 0, tmpl
            for has, col, raw in ((has_lat, "geo_lat", a), (has_lon, "geo_lon", b)):
                exp = float(raw.strip('"')) if has else float("nan")
                assert _bits(row[col]) == _bits(exp), (tmpl, col)


def test_oracle_is_total_and_follows_the_declared_semantics():
    """the disagreements between oracle and kernel found by reading both (each a named case)"""
    # amounts beyond Decimal's default precision or exponent range are malformed, not an exception
    for amount in ("1e27", "1e400", "12345678901234567890123456789", '"1e27"', "1e99999999999999999999"):
        assert _row(K.message(amount=amount))["status"] == R.MALFORMED, amount
    assert _row(K.message(amount="0e99999999999999999999"))["amount_cents"] == 0
    row = _row(K.message(amount="0.1234567890123456789012345678901"))
    assert (row["status"], row["amount_cents"]) == (R.INEXACT, 12)
    # a timestamp in fullwidth digits is no timestamp
    assert R.iso_to_ms("２025-09-05T10:11:12") is None
    # more than 19 significant digits at a rounding tie: the 19-digit value, flagged
    tie = "9007199254740993.00000000000000000001"
    row = _row(K.message(fraud_score=tie))
    assert (row["status"], row["fraud_score"]) == (R.INEXACT, 9007199254740992.0) and float(tie) == 9007199254740994.0
    row = _row(K.message(fraud_score="9007199254740993.00000000000000000000"))
    assert (row["status"], row["fraud_score"]) == (0, 9007199254740992.0)


def test_oracle_decodes_escapes_before_it_reads_scalars():
    """Jackson decodes a string before it coerces it: an escaped spelling gives the plain one's row"""
    for raw, text in K.ESCAPED_NUMBERS:
        assert "".join(c if ord(c) < 128 else "?" for c in json.loads(raw)) == text
        ok = bool(R.NUMBER_RE.match(text))
        for field in ("amount", "fraud_score", "hour_of_day"):
            row = _row(K.message(**{field: raw}))
            if ok:
                twin = _row(K.message(**{field: f'"{text}"'}))
                assert list(map(repr, row.values())) == list(map(repr, twin.values())), (raw, field)
            assert (row["status"] == R.MALFORMED) == (not ok or twin["status"] == R.MALFORMED), (raw, field)
    assert _row(K.message(amount='"9\\u0039.99"'))["amount_cents"] == 9999
    for raw, text in K.ESCAPED_INSTANTS:
        ms = R.iso_to_ms(text)
        row = _row(K.message(timestamp=raw))
        assert (row["status"], row["ts_ms"]) == ((R.MALFORMED, 0) if ms is None else (0, ms)), raw
    assert _row(K.message(timestamp=K.ESCAPED_INSTANTS[0][0]))["ts_ms"] == K._ms(2025, 9, 5, 10, 11, 12)
    for raw, key in K.ESCAPED_KEYS:
        row = _row(K.message(geolocation=f'{{"lat": 8, "lon": 9, {raw}: "1.5"}}'))
        assert row["status"] == 0 and row["geo_lat"] == (1.5 if key == "lat" else 8.0), raw
        assert row["geo_lon"] == (1.5 if key == "lon" else 9.0), raw
    row = _row(b'{"user\\u005fid": "\\u0075", "amount": 1, "timestamp": "2025-01-01T00:00:00"}')
    assert row["status"] == 0 and row["card_key"] == R.h64(b"u")
