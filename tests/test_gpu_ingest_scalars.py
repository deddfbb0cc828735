"""GPU: the ingest kernel's own scanners — scan_number_w / digit_run / Reader::word, parse_iso_w, the hour and
boolean coercions, scan_latlon's two paths (ingest.hip) — and its device arithmetic (decimal_to_double and
decimal_to_cents with __umul64hi and device f64 conversion / division) on the shared scalar cases of
tests/ingest_scalar_cases.py. Minimal messages (user_id, amount, timestamp and the fields under test); valid numbers
five to a message (fraud_score bare, geolocation in the simulator's shape, merchant_location quoted in a general
shape), every text expected to be invalid in a message of its own.
Bars: every column of every row equals oracle/ingest_ref.py bit for bit (doubles as bit patterns, NaN == NaN; the
19-digit rule of DESIGN 4.6 for longer numbers), and every text's column equals fd_ingest_scalar_host of the same
text (kind 0 doubles, 1 cents, 2 instants), so a failure names which of kernel, host code and oracle disagrees."""
import ctypes as C
import json

import numpy as np
import pytest

import ingest_scalar_cases as K
from fdengine import _native as N
from fdengine._native import INGEST_FIELDS
from fdengine.ingest import IngestCodec, device_columns, pack
from oracle import ingest_ref as R

pytestmark = pytest.mark.gpu

DOUBLE_COLS = ("fraud_score", "geo_lat", "geo_lon", "merchant_lat", "merchant_lon")
_cache = {}


def _scalar(kind, text):
    b = text.encode("utf-8")
    arr = np.frombuffer(b, np.uint8) if b else np.zeros(1, np.uint8)
    f, i, fl = C.c_double(), C.c_int64(), C.c_int32()
    N.call("fd_ingest_scalar_host", kind, C.c_void_p(arr.ctypes.data), len(b), C.byref(f), C.byref(i), C.byref(fl))
    return f.value, i.value, fl.value


def _bits(x):
    return int(np.float64(x).view(np.uint64))


def _same(got, exp, msgs):
    for k, _ in INGEST_FIELDS:
        g, e = got[k], exp[k]
        ok = (g.view(np.uint64) == e.view(np.uint64)) | (np.isnan(g) & np.isnan(e)) if g.dtype.kind == "f" else g == e
        if not ok.all():
            i = int(np.flatnonzero(~ok)[0])
            raise AssertionError(f"{k}[{i}] ({int((~ok).sum())} rows differ): device {got[k][i]!r} oracle "
                                 f"{exp[k][i]!r} status {got['status'][i]}/{exp['status'][i]} msg {msgs[i][-300:]}")


@pytest.fixture(scope="module")
def codec(engine):
    return IngestCodec(engine, [], [], [], [])


def _check(codec, msgs, device=False):
    """parse on the device, compare every column of every row with the oracle -> the device's columns"""
    exp = R.parse_batch(msgs, {}, [{}, {}, {}])
    got = codec.parse(msgs)
    _same(got, exp, msgs)
    if device:  # the device-resident entry point on the same packed buffer
        import torch
        buf, off = pack(msgs)
        dbuf, doff = torch.from_numpy(buf.copy()).cuda(), torch.from_numpy(off).cuda()
        cols, ptrs = device_columns(len(msgs))
        codec.eng.set_stream(torch.cuda.current_stream().cuda_stream)
        try:
            codec.parse_device(dbuf.data_ptr(), doff.data_ptr(), len(msgs), ptrs)
            torch.cuda.synchronize()
        finally:
            codec.eng.set_stream(None)
        _same({k: cols[k].cpu().numpy().view(dt) for k, dt in INGEST_FIELDS}, exp, msgs)
    return got


def _numbers():
    """the number corpus, once: (all texts, the slice of long mantissas)"""
    if "numbers" not in _cache:
        a = K.number_corpus(np.random.default_rng(31), 6000) + K.NUMBER_SPECIALS
        b = K.long_mantissas(np.random.default_rng(32), 4000)
        c = K.boundary_numbers(np.random.default_rng(33))
        assert all(R.NUMBER_RE.match(s) for s in a + b + c)
        _cache["numbers"] = (a + b + c, slice(len(a), len(a) + len(b)))
    return _cache["numbers"]


def _double_message(t):
    return K.message(fraud_score=t[0], geolocation=f'{{"lat": {t[1]}, "lon": {t[2]}}}',
                     merchant_location=f'{{"lon" : "{t[4]}" ,"x": 0, "lat":"{t[3]}"}}')


def test_numbers_in_double_fields(codec):
    texts, long_ones = _numbers()
    texts = texts + texts[:(-len(texts)) % 5]
    groups = [texts[i:i + 5] for i in range(0, len(texts), 5)]
    msgs = [_double_message(g) for g in groups]
    got = _check(codec, msgs, device=True)
    n_many = n_inexact = 0
    seen = set()
    for i, g in enumerate(groups):
        host = [_scalar(0, t) for t in g]
        assert not any(fl & 1 for _, _, fl in host), g
        assert got["status"][i] == (R.INEXACT if any(fl & 2 for _, _, fl in host) else 0), (g, got["status"][i])
        n_inexact += got["status"][i] == R.INEXACT
        for t, col, (v, _, _) in zip(g, DOUBLE_COLS, host):
            x = got[col][i]
            assert _bits(x) == _bits(v), (t, col, x, v)
            n_many += R.first19(t)[3]
            seen.add("subnormal" if 0 < abs(x) < 2.2250738585072014e-308 else "inf" if np.isinf(x) else
                     "+0" if _bits(x) == 0 else "-0" if _bits(x) == 1 << 63 else "")
    assert n_many >= 1000 and n_inexact >= 100, (n_many, n_inexact)
    assert {"subnormal", "inf", "+0", "-0"} <= seen, seen
    assert long_ones.stop - long_ones.start == 4000


def test_numbers_as_amounts_bare_and_quoted(codec):
    texts, _ = _numbers()
    msgs = [K.message(amount=t if q == 0 else f'"{t}"') for t in texts for q in (0, 1)]
    got = _check(codec, msgs)
    n_ok = n_inexact = 0
    for j, t in enumerate(texts):
        _, cents, fl = _scalar(1, t)
        for i in (2 * j, 2 * j + 1):
            if fl & 1:
                assert got["status"][i] == R.MALFORMED, (t, got["status"][i])
            else:
                assert got["status"][i] == (R.INEXACT if fl & 2 else 0) and got["amount_cents"][i] == cents, \
                    (t, got["status"][i], got["amount_cents"][i], cents, fl)
                n_ok += 1
                n_inexact += bool(fl & 2)
    assert n_ok > 8000 and n_inexact > 4000 and n_ok - n_inexact > 2000, (n_ok, n_inexact)


def test_bad_numbers_alone(codec):
    """no JSON numbers: as a bare score, a quoted score and a quoted amount, each in a message of its own"""
    msgs, bare = [], []
    for t in K.bad_numbers():
        assert _scalar(0, t)[2] & 1 and _scalar(1, t)[2] & 1, t
        q = json.dumps(t, ensure_ascii=False)
        msgs += [K.message(fraud_score=t), K.message(fraud_score=q), K.message(amount=q),
                 K.message(geolocation=f'{{"lat": {t}, "lon": 1}}'), K.message(merchant_location=f'{{"lon": {q}}}')]
        bare.append(t.strip() != "1")  # " 1" is a number behind JSON whitespace when it stands bare
    got = _check(codec, msgs)
    st = got["status"].reshape(-1, 5)
    assert (st[:, [1, 2, 4]] == R.MALFORMED).all()
    assert (st[np.array(bare)][:, [0, 3]] == R.MALFORMED).all() and (st[~np.array(bare)][:, [0, 3]] == 0).all()


def test_digit_run_phase_matrix(codec):
    b = K.phase_matrix()
    got = _check(codec, b.msgs, device=True)
    _, off = pack(b.msgs)
    cells = set()
    for i, (text, phase, il, fl) in enumerate(b.meta):
        at = int(off[i]) + b.msgs[i].index(b'"fraud_score": ') + 15
        assert b.msgs[i][at - int(off[i]):].startswith(text.encode()) and at & 3 == phase
        cells.add((at & 3, il, fl))
        v, _, hfl = _scalar(0, text)
        assert hfl in (0, 2) and _bits(got["fraud_score"][i]) == _bits(v), text
        assert got["status"][i] == (R.INEXACT if hfl else 0), text
    assert cells == {(p, il, fl) for p in range(4) for il in range(1, 25) for fl in range(25)}


def test_instants(codec):
    cases = K.random_instants() + K.edge_instants()
    msgs = [K.message(timestamp=json.dumps(t, ensure_ascii=False)) for t, _ in cases]
    b = K.phased_instants()
    got = _check(codec, msgs + b.msgs)
    _, off = pack(msgs + b.msgs)
    phases = set()
    for i, (text, ms, phase) in enumerate(b.meta, len(msgs)):
        at = int(off[i]) + b.msgs[i - len(msgs)].index(b'"timestamp": "') + 14
        assert at & 3 == phase
        phases.add((at & 3, text))
        cases.append((text, ms))
    assert len(phases) == 4 * 11 * 5
    for i, (text, ms) in enumerate(cases):
        _, hms, hfl = _scalar(2, text)
        assert (hfl == 1) if ms is None else (hfl == 0 and hms == ms), text
        assert (got["status"][i], got["ts_ms"][i]) == ((R.MALFORMED, 0) if ms is None else (0, ms)), text


def test_hours_booleans_locations(codec):
    from decimal import Decimal
    msgs, exp = [], []  # exp: (column, value) or None = malformed
    for t in K.HOUR_TEXTS:
        d = Decimal(t)
        for raw in (t, f'"{t}"'):
            msgs.append(K.message(hour_of_day=raw))
            exp.append(None if (d < 0 or int(d) > 254) else ("hour", int(d)))
    for raw, val in K.BOOL_CASES:
        for field, col in (("is_weekend", "weekend"), ("is_fraud", "is_fraud")):
            msgs.append(K.message(**{field: raw}))
            exp.append(None if val is None else (col, val))
    n_scalar = len(msgs)
    texts, long_ones = _numbers()
    pairs = [("1.5", "-2.25"), ("-33.868820", "151.209290"), ("1e-7", "0.0"), ("12345678901234567890.5", "-0"),
             (texts[long_ones][0], texts[long_ones][1]), (texts[-1], texts[-2])]
    locs = []
    for tmpl, has_lat, has_lon in K.LOCATION_SHAPES:
        for k, (a, bb) in enumerate(pairs):
            for field, cols in (("geolocation", ("geo_lat", "geo_lon")),
                                ("merchant_location", ("merchant_lat", "merchant_lon"))):
                qa, qb = (f'"{a}"' if k & 1 else a), (f'"{bb}"' if (k >> 1) & 1 else bb)
                msgs.append(K.message(**{field: tmpl.format(a=qa, b=qb)}))
                locs.append((has_lat, has_lon, a, bb, cols))
    got = _check(codec, msgs)
    for i, e in enumerate(exp):
        if e is None:
            assert got["status"][i] == R.MALFORMED, msgs[i]
        else:
            assert got["status"][i] == 0 and got[e[0]][i] == e[1], (msgs[i], got[e[0]][i])
    for i, (has_lat, has_lon, a, bb, cols) in enumerate(locs, n_scalar):
        if has_lat is None:
            assert got["status"][i] == R.MALFORMED, msgs[i]
            continue
        assert not got["status"][i] & R.INVALID, msgs[i]
        for has, t, col in ((has_lat, a, cols[0]), (has_lon, bb, cols[1])):
            want = _scalar(0, t)[0] if has else float("nan")
            assert _bits(got[col][i]) == _bits(want) or (np.isnan(got[col][i]) and not has), (msgs[i], col)


def test_length_boundary(codec):
    b = K.length_boundary(["12.34", "1234567890123456.78", "0.12345678901234567891", "1.5e3", "7"])
    got = _check(codec, b.msgs)
    _, off = pack(b.msgs)
    seen = set()
    for i, meta in enumerate(b.meta):
        if meta is None:
            assert got["status"][i] == 0
            continue
        text, length, mod16 = meta
        assert len(b.msgs[i]) == length and int(off[i]) % 16 == mod16 and b.msgs[i][-2:] == text[-1:].encode() + b"}"
        seen.add((length, mod16))
        if length > K.MAX_MSG:
            assert got["status"][i] == R.TOO_LONG
        else:
            _, cents, fl = _scalar(1, text)
            assert (got["status"][i], got["amount_cents"][i]) == (R.INEXACT if fl & 2 else 0, cents), meta
    assert seen == {(n, a) for n in (4079, 4080, 4081) for a in (0, 1, 15)}


def test_findings_of_the_oracle_review(codec):
    """the disagreements between kernel and oracle found by reading both, each as a named case with the answer the
    declared semantics give"""
    cases = [
        # 1: an escaped spelling of a location key is the same key
        (K.message(geolocation='{"l\\u0061t": 1.5, "lon": 2}'), 0, {"geo_lat": 1.5, "geo_lon": 2.0}),
        (K.message(merchant_location='{"lat": 1.5, "lo\\u006e": "2"}'), 0, {"merchant_lat": 1.5, "merchant_lon": 2.0}),
        # 2: numeric strings, timestamps and boolean strings are decoded before they are read
        (K.message(amount='"9\\u0039.99"'), 0, {"amount_cents": 9999}),
        (K.message(timestamp='"2025-09-05T10:11:12\\u005A"'), 0, {"ts_ms": K._ms(2025, 9, 5, 10, 11, 12)}),
        (K.message(is_fraud='"tru\\u0065"'), 0, {"is_fraud": 1}),
        (K.message(hour_of_day='"2\\u0033"'), 0, {"hour": 23}),
        (K.message(fraud_score='"0.\\u0035"'), 0, {"fraud_score": 0.5}),
        # 3: more than 19 significant digits at a rounding tie: the 19-digit value, flagged (float() gives ...994)
        (K.message(fraud_score="9007199254740993.00000000000000000001"), R.INEXACT,
         {"fraud_score": 9007199254740992.0}),
        (K.message(fraud_score="9007199254740993.00000000000000000000"), 0, {"fraud_score": 9007199254740992.0}),
        # 4: amounts beyond 19 integer digits of cents are malformed
        (K.message(amount="1e27"), R.MALFORMED, {}),
        (K.message(amount="1e400"), R.MALFORMED, {}),
        (K.message(amount="12345678901234567890123456789"), R.MALFORMED, {}),
        (K.message(amount="0e400"), 0, {"amount_cents": 0}),
        # 5: a timestamp in fullwidth digits
        (K.message(timestamp='"２025-09-05T10:11:12"'), R.MALFORMED, {}),
        # amounts take the first 19 significant digits too: the 21st digit does not break the half-cent tie
        (K.message(amount="0.12500000000000000001"), R.INEXACT, {"amount_cents": 12}),
        (K.message(amount="0.1250000000000000001"), R.INEXACT, {"amount_cents": 13}),
    ]
    msgs = [m for m, _, _ in cases]
    got = _check(codec, msgs)
    for i, (m, status, cols) in enumerate(cases):
        assert got["status"][i] == status, (m, got["status"][i])
        for col, v in cols.items():
            assert got[col][i] == v or (v != v and np.isnan(got[col][i])), (m, col, got[col][i])


def test_escaped_spellings(codec):
    """strings spelled with escapes where the kernel reads a number, an instant or a location key (decoded in place
    over the staged bytes): the row of the plain spelling, or malformed where the decoded text means nothing"""
    msgs, want = [], []  # want: the index of the plain twin, or None = malformed

    def add(escaped, plain):
        msgs.append(escaped)
        want.append(None if plain is None else len(msgs))
        if plain is not None:
            msgs.append(plain)
            want.append(-1)

    for raw, text in K.ESCAPED_NUMBERS:
        ok = bool(R.NUMBER_RE.match(text))
        for lead in range(4):  # every alignment of the decoded bytes against the dword reads
            for field in ("amount", "fraud_score", "hour_of_day"):
                add(K.message(lead=lead, **{field: raw}), K.message(lead=lead, **{field: f'"{text}"'}) if ok else None)
            add(K.message(lead=lead, geolocation=f'{{"lon": {raw}, "lat": "1"}}'),
                K.message(lead=lead, geolocation=f'{{"lon": "{text}", "lat": "1"}}') if ok else None)
            add(K.message(lead=lead, merchant_location=f'{{"lat": {raw}, "lon": {raw}}}'),  # the fast path's shape
                K.message(lead=lead, merchant_location=f'{{"lat": "{text}", "lon": "{text}"}}') if ok else None)
    for raw, text in K.ESCAPED_INSTANTS:
        for lead in range(4):
            add(K.message(lead=lead, timestamp=raw),
                K.message(lead=lead, timestamp=f'"{text}"') if R.iso_to_ms(text) is not None else None)
    for raw, key in K.ESCAPED_KEYS:
        for tmpl in ('{{"lat": 8, "lon": 9, {k}: "1.5"}}', '{{{k}: 1.5}}', '{{"lat": 8, {k} : 1e0, "lon": 9}}'):
            add(K.message(geolocation=tmpl.format(k=raw)), K.message(geolocation=tmpl.format(k=f'"{key or "x"}"')))
    for raw, val in K.BOOL_CASES:
        if "\\" in raw:
            add(K.message(is_weekend=raw),
                None if val is None else K.message(is_weekend='"true"' if val else '"false"'))
    # escapes elsewhere in a location: ignored members that hold quotes, braces and brackets in their strings, nested
    # objects, and invalid escapes (malformed wherever they stand)
    for loc, plain in (('{"x": "a\\"}b\\\\", "l\\u0061t": 1, "lon": "\\u0032"}', '{"x": 0, "lat": 1, "lon": "2"}'),
                       ('{"x": {"l\\u0061t": 5, "y": ["\\u005d", "}"]}, "lat": 1, "lon": 2}', '{"lat": 1, "lon" : 2}'),
                       ('{"lat": "\\u0031", "x": ["\\u0041]", "\\\\"], "lon": 2 }', '{"lat": "1", "lon": 2 }'),
                       ('{"\\u006c\\u0061\\u0074":"\\u002d\\u0031\\u002e\\u0035",'
                        '"\\u006c\\u006f\\u006e":\n"2\\u0065\\u0031"}', '{"lat":"-1.5","lon":"2e1"}'),
                       ('{"x": "\\q", "lat": 1, "lon": 2}', None), ('{"x": "\\u12G4", "lat": 1, "lon": 2}', None),
                       ('{"lat": 1, "lon": 2, "x\\u00": 3}', None), ('{"lat": 1, "lon": "2\\"}', None),
                       ('{"lat\\": 1, "lon": 2}', None)):
        for field in ("geolocation", "merchant_location"):
            add(K.message(**{field: loc}), None if plain is None else K.message(**{field: plain}))
    # an escaped member's decoded text is shorter than its raw text: the members after it are not disturbed
    add(K.message(amount='"\\u0031\\u0032"', fraud_score='"0.\\u0035"', timestamp=K.ESCAPED_INSTANTS[0][0]),
        K.message(amount='"12"', fraud_score='"0.5"', timestamp=f'"{K.TS0}Z"'))
    got = _check(codec, msgs)
    n_twins = 0
    for i, w in enumerate(want):
        if w is None:
            assert got["status"][i] == R.MALFORMED, msgs[i]
        elif w >= 0:
            n_twins += 1
            for k, _ in INGEST_FIELDS:
                a, b = got[k][i], got[k][w]
                assert a == b or (a != a and b != b), (msgs[i], k, a, b)
    assert n_twins > 150 and (got["status"] == 0).sum() > 200
