"""Shared inputs of tests/test_ingest_oracle.py (host) and tests/test_gpu_ingest_scalars.py (device): the texts that
pin the ingest codec's scalar scanners — numbers, ISO-8601 instants, hours, booleans, locations — and the messages
that place them at chosen byte phases and at the message-length limit. Deterministic (seeded numpy generators),
nothing here touches the GPU. A "text" is the JSON number or the content of a JSON string; a "raw" value is JSON
text as it stands in a message."""
import datetime as dt
from decimal import Decimal

import numpy as np

FULLWIDTH_1 = "１"  # a digit to str.isdigit() and to a regex \d, three non-digit bytes on the wire
TS0 = "2025-09-05T10:11:12"
MAX_MSG = 4080

# ------------------------------------------------------------------------------------------------- numbers

NUMBER_SPECIALS = ["0", "-0", "-0.0", "1e-400", "2.2250738585072011e-308", "4.9406564584124654e-324",
                   "2.4703282292062327e-324", "2.4703282292062328e-324", "1.7976931348623157e308",
                   "1.7976931348623158e308", "9007199254740993", "0.1", "123.45", "1e22", "1e23",
                   "8.98846567431158e307"]

GRAMMAR_ERRORS = ["", "-", "01", "1.", ".5", "1e", "1e+", "+1", "0x10", "1.5e3.2", "NaN", "Infinity", " 1"]


def number_corpus(rng, n):
    """n numbers of six kinds (the corpus the host test has always used)"""
    out = []
    for _ in range(n):
        kind = rng.integers(0, 6)
        if kind == 0:  # shortest repr of a random double (Python json.dumps of floats)
            out.append(repr(float(np.frombuffer(rng.bytes(8), np.float64)[0])))
        elif kind == 1:  # lat / lon style
            out.append(f"{rng.uniform(-180, 180):.{int(rng.integers(1, 8))}f}")
        elif kind == 2:  # 17 digit mantissas with exponents
            out.append(f"{rng.integers(10**16, 10**17)}e{rng.integers(-330, 300)}")
        elif kind == 3:  # amounts
            out.append(f"{rng.integers(0, 10**7)}.{rng.integers(0, 100):02d}")
        elif kind == 4:  # halfway-ish: 2^k-boundary decimal expansions
            m = int(rng.integers(1, 2**53))
            e = int(rng.integers(-60, 60))
            out.append(str(Decimal(m) * (Decimal(2) ** e) + (Decimal(2) ** (e - 1))))
        else:  # long (> 19 digit) mantissas
            out.append("0." + "".join(str(int(d)) for d in rng.integers(0, 10, int(rng.integers(20, 40)))))
    return [s.replace("inf", "1e400").replace("nan", "0") for s in out]


def _digits(rng, n, nonzero=False):
    lo = 1 if nonzero else 0
    return "".join(str(int(d)) for d in rng.integers(lo, 10, n))


def long_mantissas(rng, n):
    """18..45 random digits written d.ddd...e(+|-)x, x in [-345, 311], 30 % negative: subnormals, underflow to zero,
    overflow to infinity, significands above 2^53, exponents around Clinger's limit of 22"""
    out = []
    for k in range(n):
        nd = int(rng.integers(18, 46))
        x = int(rng.integers(-345, 312)) if k % 8 else int(rng.choice([-23, -22, 22, 23])) + nd - 1
        s = f"{_digits(rng, 1, True)}.{_digits(rng, nd - 1)}e{x}"
        out.append("-" + s if rng.random() < 0.3 else s)
    return out


def boundary_numbers(rng):
    """the 19th-digit boundary of the significand, written deliberately"""
    out = ["0", "-0", "0.0", "-0.0e5", "0.000e-7", "1" + "0" * 25]
    for total in (18, 19, 20, 21, 22, 25):
        for _ in range(6):
            head = _digits(rng, min(total, 19), True)
            zeros = "0" * (total - len(head))
            tails = [zeros] if total <= 19 else [zeros, zeros[:-1] + _digits(rng, 1, True),
                                                 _digits(rng, 1, True) + zeros[1:]]
            for tail in tails:
                m = head + tail
                out.append(m)  # the crossing inside the integer run
                out.append(m + ".0")
                out.append(m + "e-7")
                out.append("0." + m)  # ... inside the fraction run
                out.append(m[0] + "." + m[1:] + "e5")
                if total > 19:
                    out.append(m[:19] + "." + m[19:])  # ... exactly at the point
                    out.append(m[:18] + "." + m[18:])
                    out.append(m[:20] + "." + m[20:] + "5")
                for z in (1, 7, 19, 20, 30):  # leading fraction zeros
                    out.append("0." + "0" * z + m)
    # exact ties between two doubles with more than 19 digits: the 19-digit prefix sits on or below the tie and the
    # dropped digits decide the correctly rounded answer
    for _ in range(150):
        m = int(rng.integers(2**52, 2**53))
        e = int(rng.integers(-40, 12))
        tie = Decimal(m) * (Decimal(2) ** e) + (Decimal(2) ** (e - 1))
        t = format(tie, "f")
        if "." not in t:
            t += "."
        out.append(t + "0" * max(0, 21 - len(t)) + "0001")
    return out


def bad_numbers():
    """texts that are no JSON number: the grammar errors, and bytes next to the digits in ASCII (or with a digit's
    low nibble) directly after a digit run of every length modulo four and inside a fraction"""
    out = list(GRAMMAR_ERRORS)
    for b in list("/:;<=>?@") + [FULLWIDTH_1]:
        for pre in ("7", "73", "731", "7319", "73190"):
            out += [pre + b, pre + b + "5", "0." + pre + b, "0." + pre + b + "5"]
    return out


# ------------------------------------------------------------------------------------------------- instants

EPOCH = dt.datetime(1970, 1, 1)


def _ms(y, mo, d, h=0, mi=0, s=0, frac="", off_min=0):
    """epoch ms through datetime (years 1..9999)"""
    secs = (dt.datetime(y, mo, d, h, mi, s) - EPOCH) // dt.timedelta(seconds=1)
    return (secs - 60 * off_min) * 1000 + (int((frac + "000")[:3]) if frac else 0)


def random_instants():
    """the 3,000 random instants of the host test, each naive and with Z / +05:30 -> [(text, epoch ms)]"""
    rng = np.random.default_rng(3)
    out = []
    for _ in range(3000):
        us = int(rng.integers(0, 4_102_444_800_000_000))
        s = (EPOCH + dt.timedelta(microseconds=us)).isoformat()
        out.append((s, us // 1000))
        out.append((s + "Z", us // 1000) if us % 2 else (s + "+05:30", us // 1000 - 330 * 60000))
    return out


TERMINATORS = [("", 0), ("Z", 0), ("z", 0), ("+05:30", 330), ("-11:45", -705)]


def fraction_instants():
    """fraction lengths 0..10 x terminators -> [(text, epoch ms or None)]"""
    out = []
    for n in range(11):
        frac = "9876543210"[:n]
        for term, off in TERMINATORS:
            text = TS0 + ("." + frac if n else "") + term
            out.append((text, _ms(2025, 9, 5, 10, 11, 12, frac, off) if n <= 9 else None))
    return out


def edge_instants():
    """calendar, range and grammar edges -> [(text, epoch ms or None)]"""
    out = []
    for y in (1600, 1900, 2000, 2024, 2100, 2400):
        leap = y % 4 == 0 and (y % 100 != 0 or y % 400 == 0)
        out.append((f"{y}-02-29T00:00:00", _ms(y, 2, 29) if leap else None))
    for y in (2023, 2024):
        for mo in range(1, 13):
            last = ((dt.datetime(y + mo // 12, mo % 12 + 1, 1) - dt.timedelta(days=1)).day)
            out.append((f"{y}-{mo:02d}-{last:02d}T23:59:59", _ms(y, mo, last, 23, 59, 59)))
            out.append((f"{y}-{mo:02d}-{last + 1:02d}T00:00:00", None))
    out.append(("0000-01-01T00:00:00", -719528 * 86_400_000))  # year 0 is a leap year; datetime starts at year 1
    out.append(("0000-02-29T00:00:00", (-719528 + 59) * 86_400_000))
    out.append(("0001-01-01T00:00:00", _ms(1, 1, 1)))
    out.append(("9999-12-31T23:59:59.999999999", _ms(9999, 12, 31, 23, 59, 59, "999999999")))
    for off, ok in (("+18:00", 1080), ("-18:00", -1080), ("+18:59", 1139), ("+19:00", None), ("+00:60", None),
                    ("+5:30", None), ("+00:00", 0), ("-00:00", 0)):
        out.append((TS0 + off, None if ok is None else _ms(2025, 9, 5, 10, 11, 12, "", ok)))
    for bad in ("2025-09-05T24:00:00", "2025-09-05T10:60:00", "2025-09-05T10:11:60", "2025-00-05T10:11:12",
                "2025-13-05T10:11:12", "2025-09-00T10:11:12"):
        out.append((bad, None))
    digit_at = [0, 1, 2, 3, 5, 6, 8, 9, 11, 12, 14, 15, 17, 18]
    for p in digit_at:
        for c in "/:":
            out.append((TS0[:p] + c + TS0[p + 1:], None))
    for p, near in ((4, ",."), (7, ",."), (10, "SUt "), (13, "9;"), (16, "9;")):
        for c in near:
            out.append((TS0[:p] + c + TS0[p + 1:], None))
    out.append((TS0 + " ", None))
    out.append((" " + TS0, None))
    out.append((TS0[:18], None))
    out.append(("", None))
    for p in (0, 3, 9, 18):
        out.append((TS0[:p] + FULLWIDTH_1 + TS0[p + 1:], None))
    out.append((TS0 + "." + FULLWIDTH_1, None))
    out.append((TS0 + ".5" + FULLWIDTH_1, None))
    out.append((TS0 + "+0" + FULLWIDTH_1 + ":00", None))
    return out


# ------------------------------------------------------------------------------------------------- hours, booleans

HOUR_TEXTS = ["0", "-0", "-0.0", "-0.4", "254", "254.9", "255", "2.54e2", "2540e-1", "0.0254e4", "25e1", "26e1", "3e2",
              "1e3", "1e4", "1e-30", "254.99999999999999999999", "0.00000000000000000000000001",
              "1234567890123456789012345", "23", "7.999", "-1", "0.254e3", "25.4e1", "100e0", "0.00001e7"]

# raw JSON value -> the boolean, None = rejected. A string is compared decoded
BOOL_CASES = [("0", 0), ("1", 1), ("-0", 0), ("2", 1), ("10", 1), ("1.0", None), ("1e0", None), ('"true"', 1),
              ('"false"', 0), ('"True"', None), ('"tru\\u0065"', 1), ('"\\u0066alse"', 0), ('"tru\\u0045"', None),
              ('"true\\u0000"', None), ("true", 1), ("false", 0), ('"1"', None), ("12345678901234567890123", 1)]

# strings spelled with escapes where the codec reads a number, an instant or a location key: Jackson decodes them
# first, so does the codec. raw JSON string -> the decoded text ('?' where it holds a character that no
# number, instant or key holds); what the text then means is the plain scanners' business
ESCAPED_NUMBERS = [('"9\\u0039.99"', "99.99"), ('"\\u0031\\u0032.5"', "12.5"), ('"1\\u0065\\u002b2"', "1e+2"),
                   ('"1\\u0045\\u002B2"', "1E+2"), ('"\\u002D5"', "-5"), ('"\\u002d0.25"', "-0.25"),
                   ('"\\u0031\\u0032\\u0033\\u0034"', "1234"), ('"12\\u0033"', "123"), ('"2\\u0033"', "23"),
                   ('"\\u0030"', "0"), ('"1234567890123456789\\u0030\\u0031"', "123456789012345678901"),
                   ('"\\/1"', "/1"), ('"1\\n"', "1\n"), ('"\\t1"', "\t1"), ('"1\\\\"', "1\\"), ('"\\"1"', '"1'),
                   ('"1\\u00e9"', "1?"), ('"\\ud83d\\ude00"', "?"), ('"1\\u0000"', "1\0"), ('"\\u0031 "', "1 "),
                   ('"1\\u002e"', "1."), ('"\\u00311"', "11"), ('"1\\b"', "1\b"), ('"\\f\\r"', "\f\r")]
ESCAPED_INSTANTS = [(f'"{TS0}\\u005A"', TS0 + "Z"), (f'"{TS0[:10]}\\u0054{TS0[11:]}"', TS0),
                    (f'"\\u0032{TS0[1:]}"', TS0), (f'"{TS0[:4]}\\u002d{TS0[5:]}.5\\u002B05:30"', TS0 + ".5+05:30"),
                    (f'"{TS0[:18]}\\u0032"', TS0), (f'"{TS0}\\u002e123456789"', TS0 + ".123456789"),
                    (f'"{TS0}\\n"', TS0 + "\n"), (f'"{TS0[:10]}\\u0074{TS0[11:]}"', TS0.replace("T", "t")),
                    (f'"{TS0}\\u00e9"', TS0 + "?"), (f'"{TS0[:13]}\\u003a{TS0[14:]}"', TS0),
                    ('"' + "".join(f"\\u00{ord(c):02x}" for c in TS0) + '"', TS0), (f'"\\/{TS0}"', "/" + TS0)]
# raw JSON key -> "lat", "lon" or None (another key)
ESCAPED_KEYS = [('"l\\u0061t"', "lat"), ('"\\u006c\\u0061\\u0074"', "lat"), ('"la\\u0074"', "lat"),
                ('"\\u006Con"', "lon"), ('"lo\\u006e"', "lon"), ('"lat\\u0000"', None), ('"l\\u00e1t"', None),
                ('"lat\\\\"', None), ('"\\u004cat"', None), ('"la\\t"', None), ('"l\\/t"', None), ('"lo\\n"', None),
                ('"\\u006c\\u0061"', None), ('"\\ud83d\\ude00"', None)]

# ------------------------------------------------------------------------------------------------- locations

# {a} / {b}: the latitude / longitude as raw JSON values. (template, has_lat, has_lon): what the codec reads from it;
# None = the whole message is malformed
LOCATION_SHAPES = [
    ('{{"lat": {a}, "lon": {b}}}', True, True),  # the simulator's shape: the fast path
    ('{{"lon": {b}, "lat": {a}}}', True, True),
    ('{{ "lat": {a}, "lon": {b}}}', True, True),
    ('{{"lat" : {a}, "lon": {b}}}', True, True),
    ('{{"lat":  {a}, "lon": {b}}}', True, True),
    ('{{"lat":{a}, "lon": {b}}}', True, True),
    ('{{"lat": {a} , "lon": {b}}}', True, True),
    ('{{"lat": {a},  "lon": {b}}}', True, True),
    ('{{"lat": {a},"lon": {b}}}', True, True),
    ('{{"lat": {a}, "lon" : {b}}}', True, True),
    ('{{"lat": {a}, "lon":  {b}}}', True, True),
    ('{{"lat": {a}, "lon":{b}}}', True, True),
    ('{{"lat": {a}, "lon": {b} }}', True, True),  # a space before the closing brace
    ('{{"lat": {a}, "lon": {b}\n}}', True, True),
    ('{{"lat":{a},"lon":{b}}}', True, True),
    ('{{"x": [1, {{"lat": 5}}], "lat": {a}, "lon": {b}}}', True, True),
    ('{{"lat": {a}, "x": "lon", "lon": {b}}}', True, True),
    ('{{"lat": {a}, "lon": {b}, "x": null}}', True, True),
    ('{{"lat": {a}, "lon": {b}, "lat": null}}', False, True),  # duplicate key: the last wins
    ('{{"lat": 1, "lon": {b}, "lat": {a}}}', True, True),
    ('{{"lat": null, "lon": {b}}}', False, True),
    ('{{"lat": {a}, "lon": null}}', True, False),
    ('{{"lat": {a}}}', True, False),
    ('{{"l\\u0061t": {a}, "lon": {b}}}', True, True),  # an escaped spelling is the same key
    ('{{"lat": {a}, "lo\\u006e": {b}}}', True, True),
    ('{{"lat": 0, "l\\u0061t": {a}, "lon": {b}, "lo\\u006e": null}}', True, False),
    ('{{"lat": {a}, "lon": 1.}}', None, None),  # the fast path's prefix, then a malformed second coordinate
    ('{{"lat": {a}, "lon": -}}', None, None),
    ('{{"lat": {a}, "lon": "1"x}}', None, None),
    ('{{"lat": {a}, "lon": {b}]', None, None),
    ('{{"lat": {a}, "lon": {b}, }}', None, None),
    ('{{"lat": {a} "lon": {b}}}', None, None),
]

# ------------------------------------------------------------------------------------------------- messages


def message(amount="1", timestamp='"' + TS0 + '"', lead=0, **fields) -> bytes:
    """a minimal message: user_id, amount, timestamp and the fields under test, every value raw JSON text"""
    parts = ['"user_id": "u"', f'"amount": {amount}', f'"timestamp": {timestamp}']
    parts += [f'"{k}": {v}' for k, v in fields.items()]
    return b" " * lead + ("{" + ", ".join(parts) + "}").encode("utf-8")


class Batch:
    """messages in packing order with the running offset, so that a byte of a message can be put at a chosen phase
    (offset in the packed buffer modulo four) or the message at a chosen alignment"""

    def __init__(self):
        self.msgs, self.meta, self.off = [], [], 0

    def add(self, msg: bytes, meta=None):
        self.msgs.append(msg)
        self.meta.append(meta)
        self.off += len(msg)

    def add_phased(self, msg: bytes, at: int, phase: int, meta=None):
        """msg behind as many spaces as put its byte `at` on `phase`"""
        self.add(b" " * ((phase - self.off - at) & 3) + msg, meta)

    def align(self, mod16: int):
        """a valid filler message after which the offset is mod16 modulo 16"""
        m = message()
        self.add(m + b" " * ((mod16 - self.off - len(m)) & 15), None)


def phase_matrix() -> Batch:
    """integer runs of 1..24 digits x fraction runs of 0..24 digits (random, non-zero), the first digit at every byte
    phase, as the fraud score of a message each. meta = (text, phase, integer length, fraction length)"""
    rng = np.random.default_rng(41)
    b = Batch()
    for phase in range(4):
        for il in range(1, 25):
            for fl in range(25):
                text = _digits(rng, il, True) + ("." + _digits(rng, fl, True) if fl else "")
                msg = message(fraud_score=text)
                b.add_phased(msg, msg.index(b'"fraud_score": ') + 15, phase, (text, phase, il, fl))
    return b


def phased_instants() -> Batch:
    """fraction_instants() with the first byte of each text at every byte phase. meta = (text, ms, phase)"""
    b = Batch()
    for phase in range(4):
        for text, ms in fraction_instants():
            msg = message(timestamp=f'"{text}"')
            b.add_phased(msg, msg.index(b'"timestamp": "') + 14, phase, (text, ms, phase))
    return b


def length_boundary(numbers) -> Batch:
    """messages of 4079, 4080 and 4081 bytes at buffer alignments 0, 1 and 15 modulo 16, padded by an ignored string
    member and ending in "amount": <number>} (the number's last byte at L-2, the brace at L-1).
    meta = (text, length, alignment)"""
    b = Batch()
    for text in numbers:
        for length in (MAX_MSG - 1, MAX_MSG, MAX_MSG + 1):
            for mod16 in (0, 1, 15):
                b.align(mod16)
                head = f'{{"user_id": "u", "timestamp": "{TS0}", "pad": "'
                tail = f'", "amount": {text}}}'
                msg = (head + "y" * (length - len(head) - len(tail)) + tail).encode()
                assert len(msg) == length and b.off % 16 == mod16
                b.add(msg, (text, length, mod16))
    return b
