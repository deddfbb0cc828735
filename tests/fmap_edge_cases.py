"""Edge cases for the feature map and the two Flink rule cascades (csrc/features.hip feat_ext_kernel), and the CPU
census of which comparator meets which operand.

The kernel is a block of about forty comparisons against constants, two chains of f64 additions whose bits decide
a decision or a risk code, and a calendar computation. A random stream reaches few of their edges, so this stream
is constructed: every comparator's operand is put on the cutoff, one step below and one step above it. The step is
1 for hours, days, counts and cents, one f64 ulp (np.nextafter) for doubles that are inputs, and at most two ulps
for the two scores, which are rounded sums (`_W2`): each score cutoff gets rows whose driving input (the incoming
fraud_score, or without one the user's risk_score) was bisected over f64 against the oracle down to adjacent
doubles, for six settings of the other terms. A grid of the amount terms against the temporal terms
(`_chain_cases`) gives the chain's first partial sums all their values, so that a contracted multiply-add shows
(test_fmap_edges_cpu.py).

`build()` returns the population (users, users_ext, merchants, merchants_ext, vocab), the stream with its
micro-batch cuts (1, 255, 256, 257 rows and larger ones: the kernel is one thread per row in blocks of 256) and the
context arrays. Rows are interleaved at random, each card's rows in their order. `oracle_outputs(mode, ...)` runs
the C feature oracle and oracle/fmap_ref.py over the batches; `sites()` restates every comparator as (operand,
cutoff, rows that reach it) from inputs and oracle outputs alone (never from the builder's intent), `census()`
counts the rows per (site, side), and `report()` prints the table below.

Census of the committed stream, the same in both window modes (rows per side; `-` = the side cannot exist, see
test_fmap_edges_cpu.py, which fails if this table is not the one `report()` prints):

site                                below     at  above
cents % 100 == 0                       44    261     37
cents % 1000 == 0                      40    204     27
cents % 10000 == 0                     20    194     23
user avg > 0                            4     12      4
ratio > 3.0                             4     62      4
merchant avg > 0                        4      4      4
amount > merchant avg * 2.0             4      4      4
amount < 10                            20      4      4
amount < 100                            4      4      4
amount < 1000                           4      7      4
amount < 10000                          4     80      4
hour >= 6                              68    106     48
hour < 12                              12     63    720
hour < 18                               8     29     12
hour < 22                              48     40    223
hour >= 9                              69     44    218
hour <= 17                              8      8     29
hour <= 6                              68    106     48
hour >= 22                             48     40    223
pref_start >= 0                         4     24      8
pref_end >= 0                           4      8      8
hour >= pref_start                     34     20      8
hour <= pref_end                        4     20     16
weekday >= 6 (time)                  1439    114     23
z >= 0 (civil era)                      5      5      4
|lat| > 60                              4      5      4
|lat| < 10                              4      4      4
|lon| < 10                              4      5      4
intl < 0.1                              4      4      4
age >= 0                                4      4      4
age < 7                                 4      4      4
age < 30                               62      4      4
merchant >= 0                          49   1208      4
merchant < nm                          62      4      4
merchant < n_mext                      66      4      4
hour_field >= open                     16     16     12
hour_field < close                     16     20     16
velocity_5min > 5                       5      5      5
velocity_1hour > 20                     5      5      5
fe: weekend_activity < 0.3              4      4      4
fe: velocity_5min > 3                   5      5      5
fe: velocity_1hour > 10                 5      5      5
tp: fraud_rate > 0.05                   4      4      4
tp: amount / avg > 5.0                  4      4      4
tp: age < 30                           62      4      4
tp: hour_field <= 5                    32     36     98
tp: hour_field >= 23                   36    115     36
fe >= 0.3                              11     14     11
fe >= 0.6                              11     11     11
fe >= 0.8                              11     13     11
fe >= 0.95                             11     13     11
fe clamp at 0                           -     47     11
fe clamp at 1                          11     30      -
tp >= 0.5                               6     10      6
tp >= 0.9                               6     10      6
tp >= threshold 0                       -     25      6
tp >= threshold 0.5                     6     10      6
tp >= threshold 0.7                     6      9      6
tp >= threshold 0.899                   6      8      6
tp >= threshold 0.9                     6     10      6
tp >= threshold 1.0                     6    110      -
tp clamp at 0                           -     25      6
tp clamp at 1                           6    110      -
"""
import functools
import math

import numpy as np

from fdengine._native import CTX_FIELDS, TXN_FIELDS
from fdengine import synth
from oracle import fmap_ref as R

RING_K = 32            # 22 events of one card inside an hour must stay in the ring
CAP = 16384
FLOOR = 4
DAY, HOUR = 86_400_000, 3_600_000
T0 = 1_757_030_400_000                       # 2025-09-05 00:00 UTC, a Friday
THRESHOLDS_PERMILLE = (0, 500, 700, 899, 900, 1000)
FE_CUTS = (0.3, 0.6, 0.8, 0.95)
HOURS = (5, 6, 7, 8, 9, 10, 11, 12, 13, 16, 17, 18, 19, 21, 22, 23, 0)
INF = float("inf")
NaN = float("nan")


def up(x):
    return float(np.nextafter(x, INF))


def dn(x):
    return float(np.nextafter(x, -INF))


def days_from_civil(y, m, d):
    """day count since 1970-01-01 of a proleptic Gregorian date, counted explicitly (year 0 = 1 BC is leap)"""
    leap = lambda yy: yy % 4 == 0 and (yy % 100 != 0 or yy % 400 == 0)  # noqa: E731
    n = 0
    if y >= 1970:
        for yy in range(1970, y):
            n += 366 if leap(yy) else 365
    else:
        for yy in range(y, 1970):
            n -= 366 if leap(yy) else 365
    ml = (31, 29 if leap(y) else 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31)
    return n + sum(ml[:m - 1]) + d - 1


# (year, month, day): the day itself and the midnight on both of its sides are visited
DATES = ((2023, 2, 28), (2023, 3, 1), (2024, 2, 28), (2024, 2, 29), (2024, 3, 1), (2000, 2, 29), (2000, 3, 1),
         (2100, 2, 28), (2100, 3, 1), (1900, 2, 28), (1900, 3, 1), (2025, 4, 30), (2025, 5, 1), (2025, 7, 31),
         (2025, 8, 1), (2025, 12, 31), (2026, 1, 1), (1970, 1, 1), (1969, 12, 31), (0, 2, 29), (0, 3, 1), (0, 3, 2),
         (-1, 6, 15), (-1, 12, 31), (0, 1, 1), (-400, 2, 29), (-400, 3, 1))

USER_EXT_DEFAULT = dict(risk_score=0.1, kyc_status=0, verified=1, pref_start=-1, pref_end=-1, weekend_activity=0.5,
                        online_preference=0.7, intl_preference=0.5, txn_frequency=3, has_patterns=1)
MERCH_EXT_DEFAULT = dict(avg_amount=NaN, risk_level=0, blacklisted=0, category=3, high_risk_category=0,
                         open_hour=255, close_hour=255, suspicious_name=0)
CTX_DEFAULT = dict(geo_lat=NaN, geo_lon=NaN, merchant_lat=NaN, merchant_lon=NaN, payment_method=0,
                   transaction_type=0, card_type=0, user_agent_flag=0, fraud_score=NaN)
CTX_DT = dict(geo_lat=np.float64, geo_lon=np.float64, merchant_lat=np.float64, merchant_lon=np.float64,
              payment_method=np.uint8, transaction_type=np.uint8, card_type=np.uint8, user_agent_flag=np.uint8,
              fraud_score=np.float64)
USER_EXT_DT = dict(risk_score=np.float64, kyc_status=np.uint8, verified=np.uint8, pref_start=np.int8,
                   pref_end=np.int8, weekend_activity=np.float64, online_preference=np.float64,
                   intl_preference=np.float64, txn_frequency=np.int32, has_patterns=np.uint8)
MERCH_EXT_DT = dict(avg_amount=np.float64, risk_level=np.uint8, blacklisted=np.uint8, category=np.uint8,
                    high_risk_category=np.uint8, open_hour=np.uint8, close_hour=np.uint8, suspicious_name=np.uint8)


class _Builder:
    def __init__(self, seed=11):
        self.rng = np.random.Generator(np.random.PCG64(seed))
        self.users, self.merchants, self.rows = [], [], []
        self.frozen = None
        self.n_group = 0

    def _u64(self):
        return int(self.rng.integers(1, 1 << 62)) | (1 << 63)

    # users / merchants are dicts; rows refer to them by object
    def U(self, loaded=True, ext=True, **over):
        u = dict(key=self._u64(), avg=100.0, age=400, fps=(self._u64(), 0, 0), loaded=loaded,
                 ext=(dict(USER_EXT_DEFAULT) if (ext and loaded) else None))
        for k, v in over.items():
            if k in ("avg", "age", "fps"):
                u[k] = v
            else:
                assert k in USER_EXT_DEFAULT and u["ext"] is not None, k
                u["ext"][k] = v
        self.users.append(u)
        return u

    def clone(self, u, **over):
        c = dict(u, key=self._u64(), ext=(dict(u["ext"]) if u["ext"] is not None else None))
        for k, v in over.items():
            c["ext"][k] = v
        self.users.append(c)
        return c

    def M(self, ext=True, **over):
        assert self.frozen is None, "merchant tables are frozen"
        m = dict(fraud_rate=0.01, mult=1.0, ext=(dict(MERCH_EXT_DEFAULT) if ext else None))
        for k, v in over.items():
            if k in ("fraud_rate", "mult"):
                m[k] = v
            else:
                assert k in MERCH_EXT_DEFAULT and m["ext"] is not None, k
                m["ext"][k] = v
        self.merchants.append(m)
        return m

    def group(self):
        self.n_group += 1
        return self.n_group

    def add(self, user=None, merchant=None, group=-1, **over):
        """one transaction; user None: a fresh default user; merchant None: the shared default merchant"""
        if user is None:
            user = self.U()
        row = dict(user=user, merchant=self.m0 if merchant is None else merchant, cents=12345, ts=T0 + 13 * HOUR + 777,
                   hour=255, weekend=255, dfp=user["fps"][0], ipc=2, group=group, **CTX_DEFAULT)
        for k, v in over.items():
            assert k in row, k
            row[k] = v
        self.rows.append(row)
        return row

    def freeze_merchants(self):
        """merchants with an extended record first; the last ones have none (n_mext < nm)"""
        with_ext = [m for m in self.merchants if m["ext"] is not None]
        without = [m for m in self.merchants if m["ext"] is None]
        assert len(without) >= 2 and len(with_ext) >= 2
        order = with_ext + without
        for i, m in enumerate(order):
            m["index"] = i
        self.frozen = order
        self.n_mext = len(with_ext)
        M = {"fraud_rate": np.array([m["fraud_rate"] for m in order], np.float64),
             "risk_multiplier": np.array([m["mult"] for m in order], np.float64)}
        mext = {f: np.array([m["ext"][f] for m in with_ext], dt) for f, dt in MERCH_EXT_DT.items()}
        return M, mext

    def merchant_index(self, m):
        nm = len(self.frozen)
        special = {"nm": nm, "nm+1": nm + 1, "nm-1": nm - 1, "n_mext": self.n_mext, "n_mext-1": self.n_mext - 1,
                   "n_mext+1": self.n_mext + 1}
        if isinstance(m, str):
            return special[m]
        return m if isinstance(m, int) else m["index"]


def _ord(x):
    """f64 -> an integer that orders like the doubles (adjacent doubles are adjacent integers)"""
    b = int(np.float64(x).view(np.int64))
    return b if b >= 0 else -(b & 0x7FFFFFFFFFFFFFFF)


def _from_ord(k):
    return float(np.int64(k).view(np.float64)) if k >= 0 else -float(np.int64(-k).view(np.float64))


def _first(fn, lo, hi):
    """smallest double x in [lo, hi] with fn(x) true, fn monotone (false .. true); None unless it changes inside"""
    a, b = _ord(lo), _ord(hi)
    if fn(lo) or not fn(hi):
        return None
    while b - a > 1:
        mid = (a + b) // 2
        if fn(_from_ord(mid)):
            b = mid
        else:
            a = mid
    return _from_ord(b)


def _amount_cases(b):
    for rep in range(FLOOR):
        for cents in (0, 99, 100, 101, 999, 1000, 1001, 9_999, 10_000, 10_001, 99_999, 100_000, 100_001, 999_999,
                      1_000_000, 1_000_001, 19_999, 20_000, 20_001, 2_999_999, 3_000_000, 3_000_001):
            b.add(cents=cents)
    # ratio > 3.0 (is_large_for_user), amount / avg > 5.0 (large_amount_flag): averages amount / 3, amount / 5 and
    # their neighbours; the avg values are 100 * 2^k, where one ulp of the average is one ulp of the quotient
    for cents, avg in ((30_000, 100.0), (60_000, 200.0), (15_000, 50.0), (7_500, 25.0), (50_000, 100.0),
                       (100_000, 200.0), (25_000, 50.0), (12_500, 25.0)):
        g = b.group()
        for a in (dn(avg), avg, up(avg)):
            b.add(user=b.U(avg=a), cents=cents, group=g)
    tiny = 5e-324
    for rep in range(FLOOR):
        for a in (NaN, 0.0, -0.0, -tiny, tiny, -1.0, 1e-300):
            b.add(user=b.U(avg=a), cents=12345 + rep)
    # amount > merchant avg * 2.0: avg = amount / 2 and its neighbours (the doubling is exact)
    for cents in (12_345, 20_001, 777, 31_415):
        amount = cents / 100.0
        for a in (dn(amount / 2), amount / 2, up(amount / 2)):
            b.add(merchant=b.M(avg_amount=a), cents=cents)
    for rep in range(FLOOR):
        for a in (NaN, 0.0, -tiny, tiny, -3.0, 1e-300):
            b.add(merchant=b.M(avg_amount=a), cents=500 + rep)


def _hour_cases(b):
    for rep, off in enumerate((0, 1, HOUR - 1, 1_234_567)):
        for h in HOURS + (24,):
            if h < 24:  # the hour comes from the event time (the field is null)
                b.add(ts=T0 + (rep + 3) * DAY + h * HOUR + off, hour=255)
            b.add(ts=T0 + (rep + 3) * DAY + 13 * HOUR + off, hour=h)  # the field wins over the time
        # negative event times: the hour is a floor, not a truncation
        b.add(ts=-(rep + 1) * DAY - 1, hour=255)           # 23:59:59.999
        b.add(ts=-(rep + 1) * DAY - 18 * HOUR, hour=255)   # 06:00
    # preferred windows [ps, pe]
    for rep in range(FLOOR):
        for ps, pe, hours in ((8, 20, (7, 8, 9, 19, 20, 21)), (20, 8, (7, 8, 14, 20, 21)), (-1, 20, (12,)),
                              (8, -1, (12,)), (-1, -1, (12,)), (0, 23, (0, 23)), (1, 23, (0, 1)), (0, 0, (0, 1)),
                              (0, 1, (1, 2)), (12, 12, (11, 12, 13))):
            for h in hours:
                by_field = (rep + h) % 2 == 0
                b.add(user=b.U(pref_start=ps, pref_end=pe), hour=h if by_field else 255,
                      ts=T0 + (5 + rep) * DAY + (13 if by_field else h) * HOUR + 5)


def _operating_cases(b):
    for rep in range(FLOOR):
        for oh, ch in ((9, 21), (6, 23), (5, 22), (9, 9), (255, 21), (9, 255), (0, 24), (None, None)):
            m = b.M(ext=False) if oh is None else b.M(open_hour=oh, close_hour=ch, risk_level=rep % 3)
            g = b.group()
            for h in (0, 4, 5, 6, 7, 8, 9, 10, 20, 21, 22, 23, 24, 255):
                b.add(merchant=m, hour=h, group=g)


def _calendar_cases(b):
    for k, (y, mo, d) in enumerate(DATES):
        z = days_from_civil(y, mo, d)
        for ts in (z * DAY - 1, z * DAY, z * DAY + 1, z * DAY + DAY - 1, z * DAY + 12 * HOUR + k):
            b.add(ts=ts)
    # each weekday, Saturday and Sunday from the time (field null) and from the field
    for rep in range(FLOOR):
        for k in range(7):
            for wk in (255, 0, 1):
                b.add(ts=T0 + (k + 7 * rep) * DAY + (3 + 5 * rep) * HOUR + wk, weekend=wk)
            b.add(ts=-(k + 7 * rep + 1) * DAY + 5 * HOUR, weekend=255)  # before 1970


def _user_cases(b):
    sat = T0 + DAY + 10 * HOUR
    for rep in range(FLOOR):
        g = b.group()
        for age in (-1, 0, 1, 6, 7, 8, 29, 30, 31, -2, 100_000):
            b.add(user=b.U(age=age, verified=rep % 2), group=g)
        for v in (dn(0.1), 0.1, up(0.1), NaN, 0.0):
            b.add(user=b.U(intl_preference=v))
        # weekend_activity < 0.3 counts on weekend rows of users with behaviour patterns
        g = b.group()
        for v in (dn(0.3), 0.3, up(0.3), NaN):
            wk, ts = ((255, sat), (255, sat + DAY), (1, sat + 3 * DAY), (255, sat + 7 * DAY))[rep]
            b.add(user=b.U(weekend_activity=v), ts=ts + rep, weekend=wk, group=g if v == v else -1)
            b.add(user=b.U(weekend_activity=v, has_patterns=0), ts=ts + rep, weekend=wk)
            b.add(user=b.U(weekend_activity=v), ts=sat + 4 * DAY, weekend=(255, 0)[rep % 2])  # a weekday
        for r in (NaN, 0.0, 1.0, 0.5):
            for ver in (0, 1):
                b.add(user=b.U(risk_score=r, verified=ver, kyc_status=(0, 1, 2, 255)[rep]))
        b.add(user=b.U(loaded=False))                       # an unknown card: the minimal profile
        b.add(user=b.U(loaded=False), hour=23, merchant=-1)
        b.add(user=b.U(ext=False))                          # a loaded user without an extended record
        b.add(user=b.U(ext=False, age=3, avg=20.0))
        b.add(user=b.U(txn_frequency=-1, online_preference=NaN))
        u = b.U()
        b.add(user=u, dfp=b._u64())                         # a new device
        b.add(user=b.U(), dfp=0)                            # no fingerprint
        b.add(user=b.U(), ipc=(0, 1, 2, 0)[rep])


def _merchant_cases(b):
    for rep in range(FLOOR):
        g = b.group()
        for fr in (dn(0.05), 0.05, up(0.05)):
            b.add(merchant=b.M(fraud_rate=fr, risk_level=(0, 1, 2, 255)[rep]), group=g)
        for fr in (NaN, 0.0, 0.2):
            b.add(merchant=b.M(fraud_rate=fr))
        for rl in (0, 1, 2, 255, 3):
            b.add(merchant=b.M(risk_level=rl, high_risk_category=rep % 2, suspicious_name=(0, 1, 255, 1)[rep]))
        b.add(merchant=b.M(blacklisted=1))                  # low score: the override must win
        b.add(merchant=b.M(blacklisted=1), fraud_score=0.0)
        b.add(merchant=b.M(blacklisted=255))
        b.add(merchant=b.M(blacklisted=2))
        for m in (-1, 0, 1, "nm-1", "nm", "nm+1", "n_mext-1", "n_mext", "n_mext+1", -2, 2**31 - 1, -2**31):
            b.add(merchant=m, hour=(255, 12, 23, 3)[rep])


def _velocity_cases(b):
    """one card per ring: 26 events 40 s apart. Sliding windows see 0..7 earlier events in 5 minutes and 0..25 in
    the hour; the session counter of the redis_compat mode sees 0..25 in both."""
    for c in range(FLOOR + 1):
        u, g = b.U(), b.group()
        for i in range(26):
            b.add(user=u, ts=T0 + 10 * HOUR + 600_000 + c * 7 + i * 40_000, cents=1_111 + i, group=g)


def _geo_cases(b):
    for s in (1.0, -1.0):
        for t in (1.0, -1.0):
            for lat in (dn(60.0), 60.0, up(60.0)):
                b.add(geo_lat=s * lat, geo_lon=t * 50.0)
            for v in (dn(10.0), 10.0, up(10.0)):
                b.add(geo_lat=s * v, geo_lon=t * 5.0)
                b.add(geo_lat=s * 5.0, geo_lon=t * v)
                b.add(geo_lat=s * v, geo_lon=t * 30.0)       # |lon| >= 10: the latitude alone decides nothing
            b.add(geo_lat=NaN, geo_lon=t * 5.0, merchant_lat=1.0, merchant_lon=1.0)
            b.add(geo_lat=s * 5.0, geo_lon=NaN, merchant_lat=NaN, merchant_lon=1.0)
            b.add(geo_lat=s * 5.0, geo_lon=t * 5.0, merchant_lat=1.0, merchant_lon=NaN)
    pairs = [((12.5, 77.6), (12.5, 77.6)), ((0.0, 0.0), (0.0, 0.0)), ((-33.9, 151.2), (-33.9, 151.2)),
             ((90.0, 0.0), (90.0, 0.0)),                                    # identical points
             ((0.0, 0.0), (0.0, 180.0)), ((0.0, -90.0), (0.0, 90.0)), ((0.0, 10.0), (0.0, -170.0)),
             ((0.0, 180.0), (0.0, 0.0)),                                    # the equator's antipodes
             ((90.0, 0.0), (-90.0, 0.0)), ((-90.0, 30.0), (90.0, -100.0)), ((90.0, -45.0), (-90.0, -45.0)),
             ((-90.0, 0.0), (90.0, 180.0)),                                 # pole to pole
             ((90.0, 0.0), (0.0, 50.0)), ((0.0, -120.0), (-90.0, 7.0)), ((90.0, 10.0), (0.0, 10.0)),
             ((0.0, 0.0), (90.0, 0.0)),                                     # pole to equator
             ((45.0, 20.0), (-45.0, -160.0)), ((30.0, 100.0), (-30.0, -80.0)), ((0.0, 0.0), (0.0, 179.999999)),
             ((1e-7, 0.0), (0.0, 180.0)), ((60.0, 0.0), (-60.0, 179.9999999999)),   # at and next to the antipode
             ((40.7128, -74.006), (34.0522, -118.2437)), ((51.5, -0.12), (51.5 + 1e-9, -0.12)),
             ((48.85, 2.35), (48.85, dn(2.35))), ((-70.0, 179.0), (-70.0, -179.0)), ((0.0, 0.0), (1e-300, 0.0))]
    for g, m in pairs:
        b.add(geo_lat=g[0], geo_lon=g[1], merchant_lat=m[0], merchant_lon=m[1])
    for rep in range(FLOOR):
        for code in (0, 1, 2, 3, 4, 5, 6, 7, 255):
            b.add(payment_method=code, transaction_type=code if code < 4 else 255, card_type=(code % 5, 255)[code > 7],
                  user_agent_flag=(0, 1, 255)[code % 3])


def _chain_cases(b):
    """every combination of the amount terms with the temporal terms of the feature-based score: the first two
    partial sums of the chain take all their values (a contracted `temporal * 0.1` shows on some of them only)"""
    for large in (0, 1):
        for cents in (1_234_567, 1_000_000, 999, 0, 12_345, 50_000):   # category 4 / 0 / neither, round or not
            if large and cents == 0:
                continue
            for night in (0, 1):
                hour = 23 if night else 13
                for outside in (0, 1):
                    ps, pe = ((9, 17) if night else (14, 17)) if outside else (-1, -1)
                    for wk in (0, 1):
                        u = b.U(avg=(cents / 100.0) / 4 if large else 1e6, pref_start=ps, pref_end=pe,
                                weekend_activity=0.2 if wk else 0.9)
                        b.add(user=u, cents=cents, ts=T0 + 4 * DAY + hour * HOUR + 99, weekend=wk)


def _score_templates(b):
    """six settings of the other terms, so the partial sums of both chains differ; -> [(user, row fields)]"""
    sat = T0 + DAY + 2 * HOUR
    return [
        (b.U(), dict()),
        (b.U(age=3, verified=0, risk_score=0.4, pref_start=8, pref_end=20),
         dict(hour=23, merchant=b.M(risk_level=2, high_risk_category=1, fraud_rate=0.02, open_hour=9, close_hour=21))),
        (b.U(avg=40.0), dict(cents=1_000_000, merchant=b.M(suspicious_name=1, risk_level=1, avg_amount=100.0),
                             dfp=b._u64(), user_agent_flag=1)),
        (b.U(risk_score=0.9, pref_start=9, pref_end=17, age=20),
         dict(hour=6, merchant=b.M(fraud_rate=0.2, risk_level=1), ipc=1)),
        (b.U(loaded=False), dict(merchant=-1, hour=3, cents=500)),
        (b.U(weekend_activity=0.2, age=29, verified=0, risk_score=NaN),
         dict(ts=sat, merchant=b.M(ext=False, fraud_rate=0.06), ipc=0, cents=30_000)),
    ]


def _score_cases(b, templates, M, mext, pay, ref):
    from oracle.features_c import OracleFeatureState

    def one_row(user, fields):
        row = b.add(user=user, **fields)
        b.rows.pop()
        tx, ctx = _arrays(b, [row])
        orc = OracleFeatureState(64, 1, RING_K)
        if user["loaded"]:
            orc.load_users([user["key"]], [user["avg"]], [user["age"]], [list(user["fps"])])
        orc.load_merchants(M["fraud_rate"], M["risk_multiplier"])
        raw, _, vel5 = orc.run_ex(tx)
        return tx, ctx, raw, vel5

    def scorer(user, fields, drive):
        tx, ctx, raw, vel5 = one_row(user, fields)
        key = int(user["key"])

        def s(x):
            ext = {}
            if user["ext"] is not None:
                ext = {key: dict(user["ext"])}
            if drive == "fraud_score":
                ctx["fraud_score"][0] = x
            else:
                ext[key]["risk_score"] = x
            _, rules = R.feature_map(tx, ctx, raw, vel5, ext, M, mext, pay, ref)
            return float(rules["fe_score"][0]), float(rules["tp_score"][0])
        return s

    def emit(user, fields, drive, x, g):
        if drive == "fraud_score":
            b.add(user=b.clone(user), group=g, **dict(fields, fraud_score=x))
        else:
            b.add(user=b.clone(user, risk_score=x), group=g, **fields)

    tp_cuts = sorted({0.5, 0.9} | {v / 1000 for v in THRESHOLDS_PERMILLE})
    for user, fields in templates:
        plans = [("fraud_score", 0, FE_CUTS + (0.0, 1.0)), ("fraud_score", 1, tuple(tp_cuts))]
        if user["ext"] is not None:
            plans.append(("risk_score", 0, FE_CUTS + (0.0, 1.0)))
        for drive, which, cuts in plans:
            s = scorer(user, fields, drive)
            for c in cuts:
                g = b.group()
                x1 = _first(lambda x: s(x)[which] >= c, -64.0, 64.0)   # noqa: B023
                x2 = _first(lambda x: s(x)[which] > c, -64.0, 64.0)    # noqa: B023
                for x in sorted({v for x in (x1, x2) if x is not None for v in (_from_ord(_ord(x) - 1), x)}):
                    emit(user, fields, drive, x, g)
        for x in (NaN, INF, -INF, -0.5, 1.5, -0.0, 0.0, 1.0):
            emit(user, fields, "fraud_score", x, -1)


def _arrays(b, rows):
    n = len(rows)
    tx = {"card_key": np.array([r["user"]["key"] for r in rows], np.uint64),
          "ts_ms": np.array([r["ts"] for r in rows], np.int64),
          "amount_cents": np.array([r["cents"] for r in rows], np.int64),
          "merchant": np.array([b.merchant_index(r["merchant"]) for r in rows], np.int32),
          "device_fp": np.array([r["dfp"] for r in rows], np.uint64),
          "ip_class": np.array([r["ipc"] for r in rows], np.uint8),
          "hour": np.array([r["hour"] for r in rows], np.uint8),
          "weekend": np.array([r["weekend"] for r in rows], np.uint8)}
    ctx = {f: np.array([r[f] for r in rows], CTX_DT[f]) for f in CTX_FIELDS}
    assert set(TXN_FIELDS) <= set(tx) and all(len(v) == n for v in tx.values())
    return tx, ctx


def _interleave(b):
    """a random order of the rows in which each card's rows keep theirs"""
    keys = b.rng.random(len(b.rows))
    by_card = {}
    for i, r in enumerate(b.rows):
        by_card.setdefault(r["user"]["key"], []).append(i)
    slot = np.empty(len(b.rows))
    for idx in by_card.values():
        slot[idx] = np.sort(keys[idx])
    return [b.rows[i] for i in np.argsort(slot, kind="stable")]


@functools.lru_cache(maxsize=None)
def build():
    """-> dict: users, users_ext (arrays, loaded users with a record), users_ext_by_key (the oracle's form),
    merchants, merchants_ext, n_mext, vocab (pay, refund), tx, ctx, cuts, group. Built once; leave it unchanged."""
    b = _Builder()
    b.m0 = b.M()
    b.M(), b.M(ext=False), b.M(ext=False)   # indices 0 / 1 and nm - 1 / n_mext exist whatever the cases add
    _amount_cases(b)
    _hour_cases(b)
    _operating_cases(b)
    _calendar_cases(b)
    _user_cases(b)
    _merchant_cases(b)
    _velocity_cases(b)
    _geo_cases(b)
    _chain_cases(b)
    templates = _score_templates(b)
    M, mext = b.freeze_merchants()
    pay, ref = synth.vocab_flags()
    _score_cases(b, templates, M, mext, pay, ref)
    rows = _interleave(b)
    tx, ctx = _arrays(b, rows)
    n = len(rows)
    cuts = [c for c in (0, 1, 256, 512, 769, 1500) if c < n] + [n]
    loaded = [u for u in b.users if u["loaded"]]
    users = {"key": np.array([u["key"] for u in loaded], np.uint64),
             "avg_amount": np.array([u["avg"] for u in loaded], np.float64),
             "account_age_days": np.array([u["age"] for u in loaded], np.int32),
             "device_fp": np.array([u["fps"] for u in loaded], np.uint64)}
    with_ext = [u for u in loaded if u["ext"] is not None]
    uext = {"key": np.array([u["key"] for u in with_ext], np.uint64)}
    for f, dt in USER_EXT_DT.items():
        uext[f] = np.array([u["ext"][f] for u in with_ext], dt)
    by_key = {int(u["key"]): {f: uext[f][i] for f in USER_EXT_DT} for i, u in enumerate(with_ext)}
    # the reference's own haversine `a` stays in [0, 1] on every row (Math.sqrt of neither operand is NaN)
    for i in range(n):
        co = [float(ctx[f][i]) for f in ("geo_lat", "geo_lon", "merchant_lat", "merchant_lon")]
        if not any(math.isnan(v) for v in co):
            a = R.haversine_a(*co)
            assert 0.0 <= a <= 1.0, (co, a)
    assert len(np.unique(users["key"])) == len(users["key"]) and n < 8192
    case = {"users": users, "users_ext": uext, "users_ext_by_key": by_key, "merchants": M, "merchants_ext": mext,
            "n_mext": b.n_mext, "vocab": (pay, ref), "tx": tx, "ctx": ctx, "cuts": tuple(cuts),
            "group": np.array([r["group"] for r in rows], np.int64)}
    for d in (tx, ctx, users, uext, M, mext):
        for v in d.values():
            v.setflags(write=False)
    return case


def new_oracle(case, mode):
    from oracle.features_c import OracleFeatureState
    U, M = case["users"], case["merchants"]
    orc = OracleFeatureState(CAP, mode, RING_K)
    orc.load_users(U["key"], U["avg_amount"], U["account_age_days"], U["device_fp"])
    orc.load_merchants(M["fraud_rate"], M["risk_multiplier"])
    return orc


@functools.lru_cache(maxsize=None)
def oracle_raw(mode):
    """the C oracle's (raw, vel5) of the whole stream, batch by batch; leave them unchanged"""
    case = build()
    orc = new_oracle(case, mode)
    raws, v5 = [], []
    for a, b in zip(case["cuts"][:-1], case["cuts"][1:]):
        raw, _, vel5 = orc.run_ex({k: v[a:b] for k, v in case["tx"].items()})
        raws.append(raw)
        v5.append(vel5)
    return np.concatenate(raws), np.concatenate(v5)


def oracle_outputs(mode, ctx=None, threshold=0.7, drop=()):
    """-> (raw, fmap, rules) of the whole stream; ctx None: no context at all; drop: context fields left out"""
    case = build()
    raw, vel5 = oracle_raw(mode)
    c = None if ctx is None else {k: v for k, v in ctx.items() if k not in drop}
    pay, ref = case["vocab"]
    with np.errstate(over="ignore"):  # amount / 5e-324 is +inf, as in Java
        fm, rules = R.feature_map(case["tx"], c, raw, vel5, case["users_ext_by_key"], case["merchants"],
                                  case["merchants_ext"], pay, ref, threshold=threshold)
    return raw, fm, rules


@functools.lru_cache(maxsize=None)
def reference(mode):
    """the default run (full context, threshold 0.7), computed once per mode"""
    return oracle_outputs(mode, ctx=build()["ctx"])


# -----------------------------------------------------------------------------------------------------------------
# the census

_W2 = 2   # ulps within which a score counts as just below / just above its cutoff


class Site:
    """one comparison `x OP c`: operand, cutoff, the rows that reach it with an observable outcome, the side(s) on
    which the outcome differs from the rows at the cutoff (`past`), and where that shows:
    ("col", k): feature-map column k (NaN counts as a value); ("rule", field); ("pair", score field): the score
    differs between the at-row and the past-row of one matched group; None: nothing can show it (`why`)."""

    def __init__(self, name, x, c, reach, past, obs, kind="f64", width=1, absent=(), why="", tol=None):
        self.name, self.x, self.c, self.reach, self.kind, self.width = name, np.asarray(x), c, reach, kind, width
        self.tol = tol  # an absolute width instead of ulps: next to 0.0 an ulp is a denormal no sum ever lands on
        self.past = (past,) if isinstance(past, str) else tuple(past)
        self.obs, self.absent, self.why = obs, tuple(absent), why

    def rows(self):
        x = self.x.astype(np.int64 if self.kind == "int" else np.float64)
        c = np.broadcast_to(np.asarray(self.c, x.dtype), x.shape)
        if self.kind == "int":
            lo, hi, lo2, hi2 = c - 1, c + 1, c - 1, c + 1
        else:
            lo = hi = c
            for _ in range(self.width):
                lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
            lo2, hi2 = np.nextafter(c, -np.inf), np.nextafter(c, np.inf)
            if self.tol is not None:
                lo, hi = c - self.tol, c + self.tol
        r = self.reach
        return {"below": np.flatnonzero(r & (x >= lo) & (x <= lo2)), "at": np.flatnonzero(r & (x == c)),
                "above": np.flatnonzero(r & (x >= hi2) & (x <= hi))}


def sites(case, raw, fm, rules):
    """every comparator of feat_ext_kernel as a Site, from the inputs and the oracle's outputs"""
    tx, ctx = case["tx"], case["ctx"]
    n = len(raw)
    I = R.IDX
    ue, M, mx, nm, n_mext = case["users_ext_by_key"], case["merchants"], case["merchants_ext"], \
        len(case["merchants"]["fraud_rate"]), case["n_mext"]
    yes = np.ones(n, bool)
    has_user = ~np.isnan(raw[:, 8])
    key = tx["card_key"]
    uget = lambda f, d: np.array([ue.get(int(k), {}).get(f, d) if hu else d for k, hu in zip(key, has_user)])  # noqa
    ps, pe = uget("pref_start", -1), uget("pref_end", -1)
    m = tx["merchant"].astype(np.int64)
    has_m = (m >= 0) & (m < nm)
    ml = has_m & (m < n_mext)
    mi = np.where(ml, m, 0)
    mavg = np.where(ml, mx["avg_amount"][mi], np.nan)
    oh = np.where(ml, mx["open_hour"][mi], 255).astype(np.int64)
    ch = np.where(ml, mx["close_hour"][mi], 255).astype(np.int64)
    fr = np.where(has_m, M["fraud_rate"][np.where(has_m, m, 0)], 0.05)
    cents = tx["amount_cents"]
    amount, hour, hf = raw[:, 0], raw[:, 2].astype(np.int64), tx["hour"].astype(np.int64)
    age = raw[:, 15].astype(np.int64)
    uavg = raw[:, 8]
    ratio_ok = has_user & (uavg > 0)
    ratio = np.where(ratio_ok, amount / np.where(ratio_ok, uavg, 1.0), np.nan)
    glat, glon = ctx["geo_lat"], ctx["geo_lon"]
    geo = ~np.isnan(glat) & ~np.isnan(glon)
    days = np.floor_divide(tx["ts_ms"], DAY)
    hours_known = ml & (oh != 255) & (ch != 255) & (hf != 255)
    fe, tp = rules["fe_score"], rules["tp_score"]
    out = [
        # the remainder, signed: mod - 1 counts as one step below a multiple
        Site("cents % 100 == 0", cents % 100 - 100 * (cents % 100 > 50), 0, yes, ("below", "above"),
             ("col", I["is_round_amount"]), "int"),
        Site("cents % 1000 == 0", cents % 1000 - 1000 * (cents % 1000 > 500), 0, yes, ("below", "above"),
             ("col", I["is_round_10"]), "int"),
        Site("cents % 10000 == 0", cents % 10000 - 10000 * (cents % 10000 > 5000), 0, yes, ("below", "above"),
             ("col", I["is_round_100"]), "int"),
        Site("user avg > 0", uavg, 0.0, has_user, "above", ("col", I["amount_to_user_avg_ratio"])),
        Site("ratio > 3.0", ratio, 3.0, ratio_ok, "above", ("col", I["is_large_for_user"])),
        Site("merchant avg > 0", mavg, 0.0, has_m, "above", ("col", I["amount_to_merchant_avg_ratio"])),
        Site("amount > merchant avg * 2.0", amount, mavg * 2.0, has_m & (mavg > 0), "above",
             ("col", I["is_large_for_merchant"])),
    ]
    for cut in (1000, 10_000, 100_000, 1_000_000):
        out.append(Site(f"amount < {cut // 100}", cents, cut, yes, "below", ("col", I["amount_category"]), "int"))
    for name, c, past, col in (("hour >= 6", 6, "below", "time_period"), ("hour < 12", 12, "below", "time_period"),
                               ("hour < 18", 18, "below", "time_period"), ("hour < 22", 22, "below", "time_period"),
                               ("hour >= 9", 9, "below", "is_business_hours"),
                               ("hour <= 17", 17, "above", "is_business_hours"),
                               ("hour <= 6", 6, "above", "is_night_time"),
                               ("hour >= 22", 22, "below", "is_night_time")):
        out.append(Site(name, hour, c, yes, past, ("col", I[col]), "int"))
    pref = has_user & (ps >= 0) & (pe >= 0)
    out += [
        Site("pref_start >= 0", ps, 0, has_user & (pe >= 0), "below", ("col", I["in_user_preferred_time"]), "int"),
        Site("pref_end >= 0", pe, 0, has_user & (ps >= 0), "below", ("col", I["in_user_preferred_time"]), "int"),
        Site("hour >= pref_start", hour, ps, pref & (hour <= pe), "below", ("col", I["in_user_preferred_time"]), "int"),
        Site("hour <= pref_end", hour, pe, pref & (hour >= ps), "above", ("col", I["in_user_preferred_time"]), "int"),
        Site("weekday >= 6 (time)", raw[:, 3], 6, tx["weekend"] == 255, "below", ("col", I["is_weekend"]), "int"),
        Site("z >= 0 (civil era)", days + 719468, 0, yes, "below", ("col", I["day_of_month"]), "int"),
        Site("|lat| > 60", np.abs(glat), 60.0, geo, "above", ("col", I["is_high_risk_country"])),
        Site("|lat| < 10", np.abs(glat), 10.0, geo & (np.abs(glon) < 10), "below", ("col", I["is_high_risk_country"])),
        Site("|lon| < 10", np.abs(glon), 10.0, geo & (np.abs(glat) < 10), "below", ("col", I["is_high_risk_country"])),
        Site("intl < 0.1", fm[:, I["user_intl_preference"]], 0.1, has_user, "below",
             ("col", I["unexpected_intl_transaction"])),
        Site("age >= 0", age, 0, has_user, "below", ("col", I["is_new_account"]), "int"),
        Site("age < 7", age, 7, has_user, "below", ("col", I["is_very_new_account"]), "int"),
        Site("age < 30", age, 30, has_user, "below", ("col", I["is_new_account"]), "int"),
        Site("merchant >= 0", m, 0, yes, "below", ("col", I["merchant_risk_multiplier"]), "int"),
        Site("merchant < nm", m, nm, yes, "below", ("col", I["merchant_risk_multiplier"]), "int"),
        Site("merchant < n_mext", m, n_mext, yes, "below", ("col", I["merchant_category"]), "int"),
        Site("hour_field >= open", hf, oh, hours_known & (hf < ch), "below", ("col", I["within_merchant_hours"]),
             "int"),
        Site("hour_field < close", hf, ch, hours_known & (hf >= oh), "below", ("col", I["within_merchant_hours"]),
             "int"),
        Site("velocity_5min > 5", raw[:, 9], 5, yes, "above", ("col", I["high_velocity_5min"]), "int"),
        Site("velocity_1hour > 20", raw[:, 10], 20, yes, "above", ("col", I["high_velocity_1hour"]), "int"),
        # the comparisons that only the cascades show
        Site("fe: weekend_activity < 0.3", fm[:, I["weekend_activity_factor"]], 0.3, raw[:, 4] > 0.5, "below",
             ("pair", "fe_score")),
        Site("fe: velocity_5min > 3", raw[:, 9], 3, yes, "above", ("pair", "fe_score"), "int"),
        Site("fe: velocity_1hour > 10", raw[:, 10], 10, yes, "above", ("pair", "fe_score"), "int"),
        Site("tp: fraud_rate > 0.05", fr, 0.05, has_m, "above", ("pair", "tp_score")),
        Site("tp: amount / avg > 5.0", ratio, 5.0, ratio_ok, "above", ("pair", "tp_score")),
        Site("tp: age < 30", age, 30, has_user & (age >= 0), "below", ("pair", "tp_score"), "int"),
        Site("tp: hour_field <= 5", hf, 5, hf != 255, "above", ("pair", "tp_score"), "int"),
        Site("tp: hour_field >= 23", hf, 23, hf != 255, "below", ("pair", "tp_score"), "int"),
    ]
    for c in FE_CUTS:
        out.append(Site(f"fe >= {c}", fe, c, yes, "below", ("rule", "fe_risk"), width=_W2))
    out.append(Site("fe clamp at 0", fe, 0.0, yes, (), None, tol=1e-12, absent=("below",),
                    why="max(0, x): at the cutoff both operands are equal; below it the score is clamped"))
    out.append(Site("fe clamp at 1", fe, 1.0, yes, (), None, width=_W2, absent=("above",),
                    why="min(1, x): at the cutoff both operands are equal; above it the score is clamped"))
    not_bl = fm[:, I["is_blacklisted_merchant"]] != 1.0
    out.append(Site("tp >= 0.5", tp, 0.5, not_bl, "below", ("rule", "tp_risk"), width=_W2))
    out.append(Site("tp >= 0.9", tp, 0.9, not_bl, "below", ("rule", "tp_risk"), width=_W2))
    for v in THRESHOLDS_PERMILLE:
        c = v / 1000
        if v == 0:
            out.append(Site("tp >= threshold 0", tp, c, not_bl, (), None, tol=1e-12, absent=("below",),
                            why="the clamped score is never below 0: every row is at least REVIEW"))
        elif v >= 900:
            out.append(Site(f"tp >= threshold {c}", tp, c, not_bl, (), None, width=_W2,
                            absent=("above",) if v == 1000 else (),
                            why="shadowed: tp >= 0.9 declines before the threshold is read"))
        else:
            out.append(Site(f"tp >= threshold {c}", tp, c, not_bl, "below", ("threshold", v), width=_W2))
    out.append(Site("tp clamp at 0", tp, 0.0, yes, (), None, tol=1e-12, absent=("below",),
                    why="max(0, x): at the cutoff both operands are equal; below it the score is clamped"))
    out.append(Site("tp clamp at 1", tp, 1.0, yes, (), None, width=_W2, absent=("above",),
                    why="min(1, x): at the cutoff both operands are equal; above it the score is clamped"))
    return out


def values(case, raw, fm, rules):
    """rows per value of the fields that are compared for equality or tested for null"""
    tx, I = case["tx"], R.IDX
    isn = lambda k: int(np.isnan(fm[:, I[k]]).sum())  # noqa: E731
    eq = lambda k, v: int((fm[:, I[k]] == v).sum())   # noqa: E731
    out = {}
    for v in (0, 1, 2, 254):
        out["merchant_risk_level", v] = eq("merchant_risk_level", float(v))
    for k in ("is_blacklisted_merchant", "is_kyc_verified", "is_high_risk_category", "is_new_device", "is_refund",
              "is_high_risk_payment", "has_geolocation", "has_merchant_location"):
        for v in (0, 1):
            out[k, v] = eq(k, float(v))
    for k in ("suspicious_merchant_name", "suspicious_user_agent", "is_private_ip", "within_merchant_hours",
              "in_user_preferred_time", "user_intl_preference", "weekend_activity_factor",
              "amount_to_user_avg_ratio", "distance_to_merchant_km", "latitude"):
        out[k, "null"] = isn(k)
        out[k, "present"] = len(fm) - isn(k)
    has_user = ~np.isnan(raw[:, 8])
    out["user", "unknown card"] = int((~has_user).sum())
    out["user", "no extended record"] = int((has_user & (fm[:, I["kyc_status"]] == R.UNKNOWN)
                                             & (fm[:, I["user_transaction_frequency"]] == 0)).sum())
    for k, v in (("user_risk_score", 0.0), ("user_risk_score", 1.0), ("user_risk_score", 0.5), ("kyc_status", 254.0)):
        out[k, v] = eq(k, v)
    by_time, by_field = tx["hour"] == 255, tx["hour"] != 255
    for h in HOURS:
        out["hour from time", h] = int((by_time & (raw[:, 2] == h)).sum())
        out["hour from field", h] = int((by_field & (raw[:, 2] == h)).sum())
    for d in range(1, 8):
        out["weekday from time", d] = int(((tx["weekend"] == 255) & (raw[:, 3] == d)).sum())
    for d in (1, 28, 29, 30, 31):
        out["day_of_month", d] = eq("day_of_month", float(d))
    out["event time", "< 0"] = int((tx["ts_ms"] < 0).sum())
    out["blacklisted override", "tp < 0.9"] = int(((fm[:,
     I["is_blacklisted_merchant"]] == 1) & (rules["tp_score"] < 0.9)).sum())
    fs = case["ctx"]["fraud_score"]
    for name, mask in (("nan", np.isnan(fs)), ("+inf", fs == np.inf), ("-inf", fs == -np.inf), ("< 0", fs < 0),
     ("> 1", fs > 1)):
        out["fraud_score", name] = int(mask.sum())
    return out


def census(case, raw, fm, rules):
    """-> {(site name, side): rows} over every Site, plus values()"""
    out = {}
    with np.errstate(over="ignore"):
        all_sites = sites(case, raw, fm, rules)
    for s in all_sites:
        for side, idx in s.rows().items():
            out[s.name, side] = len(idx)
    out.update(values(case, raw, fm, rules))
    return out


def report(case, raw, fm, rules):
    lines = [f"{'site':34s} {'below':>6s} {'at':>6s} {'above':>6s}"]
    with np.errstate(over="ignore"):
        all_sites = sites(case, raw, fm, rules)
    for s in all_sites:
        r = s.rows()
        cell = lambda side: "-" if side in s.absent else str(len(r[side]))  # noqa: E731, B023
        lines.append(f"{s.name:34s} {cell('below'):>6s} {cell('at'):>6s} {cell('above'):>6s}")
    return "\n".join(lines)
