"""GPU: the text patterns and features (csrc/text.hip) against the reference's own outputs
(tests/golden/text_cases.npz) and, on shapes the fixture does not hold, against the pure host form
fd_text_features_ref_host (itself pinned to the fixture by test_text_host.py). Bar: every feature column bit-equal,
flags and status equal.

Internal capacities of the implementation the shapes are sized around (text.hip / fd_internal.h):
  SEG     = 64      tile bytes per lane: a row longer than this is shared by several lanes
  TILE    = 16384   bytes per LDS tile, the staging span (256 lanes x SEG); tiles lie at multiples of TILE in a call's blob
  PRE     = 15      bytes a lane enters its first row early (the longest keyword minus one)
  ROWS_WG = 256     rows per workgroup of the finishing kernel
  GRID    = 1024    workgroups of the scan kernel: a call of more than GRID tiles gives a workgroup a second tile
  CHUNK   = 65536   rows per pass (a larger call is cut into chunks; a chunk's first byte may lie inside a tile)"""
import ctypes as C

import numpy as np
import pytest

import text_cases as T

pytestmark = pytest.mark.gpu

SEG, TILE, PRE, ROWS_WG, GRID, CHUNK = 64, 16384, 15, 256, 1024, 65536
UNEVEN = (1, 7, 64, 257, 3, 1000, 255, 256, 2049)


@pytest.fixture(scope="module")
def fixture():
    return T.load_fixture()


def run(eng, blob, off, splits=None):
    """the rows fed in calls of the given sizes (cycled; None: one call) -> (feat, patterns, status)"""
    n = len(off) // 4
    if splits is None:
        return eng.text_features(blob, off)
    parts, a, i = [], 0, 0
    while a < n:
        b = min(n, a + splits[i % len(splits)])
        parts.append(eng.text_features(*T.slice_rows(blob, off, a, b)))
        a, i = b, i + 1
    return tuple(np.concatenate([p[k] for p in parts]) for k in range(3))


def check_against_host(eng, rows, what="", splits=None):
    blob, off = T.encode(rows)
    got = run(eng, blob, off, splits)
    T.assert_matches(got, T.ref_host(blob, off), what)
    return got


def same_bytes(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_fixture_parity_however_the_rows_are_cut(engine, fixture):
    blob, off = fixture["blob"], fixture["off"]
    want = T.expected_native(fixture)
    whole = run(engine, blob, off)
    T.assert_matches(whole, want, "one call")
    ones = run(engine, blob, off, (1,))
    T.assert_matches(ones, want, "calls of 1")
    uneven = run(engine, blob, off, UNEVEN)
    T.assert_matches(uneven, want, "uneven")
    assert same_bytes(whole, ones) and same_bytes(whole, uneven)
    # the status is the isascii rule exactly: no row is hidden behind the flag
    rows = T.decode(blob, off)
    assert (whole[2] == [0 if all(s.isascii() for s in r.values()) else T.NONASCII for r in rows]).all()
    assert not whole[0][whole[2] != 0].any() and not whole[1][whole[2] != 0].any()


def test_drop_in_reproduces_the_reference(engine, fixture):
    from fdengine.text import BertTextAnalyzer
    rows = T.decode(fixture["blob"], fixture["off"])
    det = BertTextAnalyzer(engine=engine)
    det.load_model()
    flags, feat = det.analyze_batch(rows)
    assert flags.dtype == bool and flags.shape == (len(rows), 5) and feat.shape == (len(rows), 14)
    want_bits = (fixture["patterns"][:, None] >> np.arange(5)) & 1
    assert (flags == want_bits.astype(bool)).all()
    assert feat.tobytes() == fixture["feat"].tobytes()  # the non-ASCII rows included
    lo, hi = fixture["groups"]["non_ascii"]
    g = fixture["groups"]
    some = list(range(0, lo, 41)) + list(range(lo, hi)) + [g["unique"][0] + 1, g["whitespace"][0], g["random"][1] - 1]
    for i in some:
        p = det.detect_fraud_patterns(rows[i])
        assert list(p) == list(T.PATTERNS) and all(type(v) is bool for v in p.values())
        assert [int(v) for v in p.values()] == want_bits[i].tolist(), (i, rows[i])
        f = det.get_text_features(rows[i])
        assert list(f) == list(T.COLUMNS)
        assert all(type(v) is (float if k == "merchant_name_char_diversity" else int) for k, v in f.items())
        assert [f[k] for k in T.COLUMNS] == fixture["feat"][i].tolist(), (i, rows[i])
    # a missing key is the empty field; a None raises as the reference's join and len do
    assert det.detect_fraud_patterns({"description": "send BTC"})["crypto_keywords"] is True
    assert det.get_text_features({})["total_text_length"] == 0
    assert det.get_text_features({"merchant_name": "ab", "category": None})["merchant_name_length"] == 2
    with pytest.raises(TypeError):
        det.detect_fraud_patterns({"merchant_name": "ab", "category": None})
    with pytest.raises(TypeError):
        det.get_text_features({"merchant_name": None})
    assert det.analyze_transaction_text(rows[0]) == {"overall_text_risk": 0.0}
    stats = det.get_performance_stats()
    assert stats["total_predictions"] == len(rows)
    assert set(stats) == {"total_predictions", "avg_processing_time_ms", "total_processing_time_ms"}
    det.close()
    engine.text_features(b"", np.zeros(1, np.int64))  # the shared engine is not closed by an analyzer it was lent to


def filler(n, seed=0):
    """n bytes of keyword-free text with spaces, digits and specials"""
    unit = "lorem 12 shop, no-9 (x) "
    s = unit[seed % len(unit):] + unit * (n // len(unit) + 1)
    return s[:n]


@pytest.mark.parametrize("n", [1, 2, ROWS_WG - 1, ROWS_WG, ROWS_WG + 1, 3 * ROWS_WG + 5])
def test_row_counts_around_the_finishing_workgroup(engine, n):
    rows = [T.row(m=filler(i % 90, i), d="act now" if i % 3 == 0 else filler(i % 7), l="x" * (i % 5)) for i in range(n)]
    got = check_against_host(engine, rows, f"n={n}")
    assert got[1][0] == 4  # "act now"


@pytest.mark.parametrize("length", [SEG - 1, SEG, SEG + 1, TILE - 1, TILE, TILE + 1, 2 * TILE, 2 * TILE + 1])
def test_row_lengths_around_the_segment_and_the_staging_span(engine, length):
    body = filler(length - 7) + "act now"  # the keyword at the row's very end
    for lead in ("", "ab", filler(SEG - 3), filler(TILE - 5)):  # the row's start at several places of a tile
        rows = ([T.row(m=lead)] if lead else []) + [T.row(d=body), T.row(m=body), T.row(m=body[:length // 2],
                                                                                        d=body[length // 2:])]
        got = check_against_host(engine, rows, f"length {length} after {len(lead)}")
        assert (got[1][-3:] == 4).all() and got[0][-3, 1] == length and got[0][-2, 0] == length


def straddle_rows(boundary, stride):
    """every two-word keyword at every offset across `boundary` (a position inside rows that are `stride` bytes long,
    so that with stride a multiple of TILE or SEG every row starts on the same kind of boundary): inside one field,
    and with the keyword's space replaced by a field boundary at the same place"""
    rows, bits = [], []
    for k, b in T.two_word():
        a, z = k.split(" ")
        for shift in range(len(k) + 1):  # the keyword's first byte at boundary - shift
            head = filler(boundary - shift)
            tail = "." * (stride - len(head) - len(k))
            rows.append(T.row(d=head + k + tail))
            bits.append(b)
            rows.append(T.row(m=head + a, d=z + tail + "."))  # one byte fewer in the blob: pad it back
            bits.append(b)
    return rows, bits


@pytest.mark.parametrize("boundary,stride", [(SEG, 4 * SEG), (3 * SEG, 4 * SEG), (TILE, 3 * TILE)])
def test_keyword_straddling_a_boundary_at_every_offset(engine, boundary, stride):
    rows, bits = straddle_rows(boundary, stride)
    blob, off = T.encode(rows)
    assert (off[::4] % stride == 0).all()  # every row starts where the first does
    got = run(engine, blob, off)
    T.assert_matches(got, T.ref_host(blob, off), f"boundary {boundary}")
    assert ((got[1] >> np.array(bits)) & 1).all()
    if stride == 3 * TILE:
        assert len(blob) > GRID * TILE  # and a workgroup takes a second tile
        shifted = run(engine, *T.encode([T.row(m="0123456")] + rows[:200]))  # the same rows off the boundary
        assert same_bytes(tuple(x[1:] for x in shifted), tuple(x[:200] for x in got))


def test_long_row_between_empty_rows_and_all_rows_empty(engine):
    long_d = filler(3 * TILE + 100) + "tax refund"
    got = check_against_host(engine, [T.row()] * 3 + [T.row(m="Shop 24", d=long_d, c="misc")] + [T.row()] * 300,
                             "long row between empty rows")
    assert got[1][3] == 16 and got[1].sum() == 16 and got[0][3, 1] == len(long_d)
    for n in (1, 2, ROWS_WG + 1):
        got = check_against_host(engine, [T.row()] * n, f"{n} empty rows")
        assert not got[0].any() and not got[1].any() and not got[2].any()
    got = engine.text_features(np.zeros(0, np.uint8), np.zeros(1, np.int64))  # n = 0
    assert got[0].shape == (0, 14) and got[1].shape == (0,)


def test_one_70000_byte_row_alone(engine):
    d = filler(T.LONG_ROW - 16) + "warranty expired"
    got = check_against_host(engine, [T.row(d=d)], "70000 bytes")
    assert got[1][0] == 16 and got[0][0, 1] == T.LONG_ROW
    got = check_against_host(engine, [T.row(m=d[:35000], d=d[35000:-8], c=d[-8:])], "70000 bytes in three fields")
    assert got[1][0] == 0  # "warranty" "expired" with a separator more between them


@pytest.mark.parametrize("n", [CHUNK - 1, CHUNK, CHUNK + 1])
def test_call_crossing_the_chunk(engine, n):
    # short rows: the second chunk's first byte lies inside a tile, and a keyword cut by the row boundary there is none
    words = ("shop 12", "", "Gift", "Card x", "a\tb  c", "IRS", "plain text, no flags")
    rows = [T.row(m=words[i % 7], d=words[(i * 3 + 1) % 7]) for i in range(n)]
    rows[n - 2] = T.row(m="x", l="lottery winne")  # (n = CHUNK + 1: the last row of the first chunk)
    rows[n - 1] = T.row(m="r", d="urgent")
    blob, off = T.encode(rows)
    got = run(engine, blob, off)
    T.assert_matches(got, T.ref_host(blob, off), f"n={n}")
    assert got[1][n - 2] == 0 and got[1][n - 1] == 4
    if n == CHUNK + 1:
        cut = run(engine, blob, off, (CHUNK - 1, 2))
        assert same_bytes(got, cut)


def test_device_pointers_null_outputs_and_an_unaligned_blob(engine, fixture):
    import torch
    lo, hi = fixture["groups"]["random"][0], fixture["groups"]["random"][0] + 700
    blob, off = T.slice_rows(fixture["blob"], fixture["off"], lo, hi)
    n = hi - lo
    want = T.ref_host(blob, off)
    for shift in (0, 1, 13):  # the blob at an address that is no multiple of 16: the byte-wise staging
        d_blob = torch.zeros(len(blob) + 32, dtype=torch.uint8, device="cuda")
        d_blob[shift:shift + len(blob)] = torch.from_numpy(blob.copy()).cuda()
        d_off = torch.from_numpy(off).cuda()
        feat = torch.full((n, 14), -1.0, dtype=torch.float64, device="cuda")
        pat = torch.full((n,), 255, dtype=torch.uint8, device="cuda")
        st = torch.full((n,), 255, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        engine.text_features_device(d_blob.data_ptr() + shift, d_off.data_ptr(), n, feat.data_ptr(), pat.data_ptr(),
                                    st.data_ptr())
        engine.sync()
        T.assert_matches((feat.cpu().numpy(), pat.cpu().numpy(), st.cpu().numpy()), want, f"shift {shift}")
    # any output may be null
    for keep in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0)):
        feat.fill_(-1.0), pat.fill_(255), st.fill_(255)
        torch.cuda.synchronize()
        engine.text_features_device(d_blob.data_ptr() + shift, d_off.data_ptr(), n, feat.data_ptr() * keep[0],
                                    pat.data_ptr() * keep[1], st.data_ptr() * keep[2])
        engine.sync()
        for out, w, k, blank in ((feat, want[0], keep[0], -1.0), (pat, want[1], keep[1], 255), (st, want[2], keep[2], 255)):
            got = out.cpu().numpy()
            assert got.tobytes() == w.tobytes() if k else (got == blank).all()
    engine.text_features_device(0, 0, 0)  # n = 0 reads no pointer
    # the host entry with null outputs
    from fdengine import _native as N
    b = N.fd_text_batch(blob.ctypes.data, off.ctypes.data)
    only = np.full(n, 255, np.uint8)
    N.call("fd_text_features_host", engine._h, C.byref(b), n, None, only.ctypes.data_as(C.c_void_p), None)
    assert only.tobytes() == want[1].tobytes()
    N.call("fd_text_features_host", engine._h, C.byref(b), n, None, None, None)


def test_errors_counters_and_timing():
    import fdengine
    from fdengine import _native as N
    eng = fdengine.FraudEngine(0)
    try:
        assert eng.counter("text_calls") == 0 and eng.counter("text_nonascii_rows") == 0
        blob, off = T.encode([T.row(m="caf\u00e9"), T.row(m="cafe"), T.row(d="\u212a")])
        for bad in ([1] + off[1:].tolist(), off[:5].tolist() + [0] + off[6:].tolist()):
            with pytest.raises(N.NativeError) as ei:
                eng.text_features(blob, np.array(bad, np.int64))
            assert ei.value.code == N.FD_ERR_INVALID_ARG and "offsets" in str(ei.value)
        with pytest.raises(ValueError):
            eng.text_features(blob, off[:-1])
        with pytest.raises(ValueError):
            eng.text_features(blob[:-1], off)
        with pytest.raises(N.NativeError) as ei:
            eng.text_features_device(0, 0, 3)
        assert ei.value.code == N.FD_ERR_INVALID_ARG and "null" in str(ei.value)
        assert eng.counter("text_calls") == 0
        eng.set_timing(True)
        feat, pat, st = eng.text_features(blob, off)
        assert st.tolist() == [1, 0, 1] and feat[1, 0] == 4
        eng.text_features(b"", np.zeros(1, np.int64))  # a no-op
        assert eng.counter("text_calls") == 1 and eng.counter("text_nonascii_rows") == 2
        ms, launches = eng.read_timing(N.FD_TIMING_TEXT)
        assert launches == 1 and ms > 0
        eng.text_features(blob, off)
        assert eng.counter("text_calls") == 2 and eng.counter("text_nonascii_rows") == 4
    finally:
        eng.close()
