"""CPU proof of the feature-map edge stream (tests/fmap_edge_cases.py) that tests/test_gpu_fmap_edges.py feeds
feat_ext_kernel: every comparator of the kernel meets its cutoff, the step below and the step above it often enough
(the census), an off-by-one at any of them would change a row of the stream (the sensitivity), a fused multiply-add
or a reordered sum in either score chain would change score bits, and the oracle the kernel is compared with has hand-derived known answers on the calendar dates and on one straddling pair of each
cascade.

Sites at which no output can differ between the cutoff and the step past it, by name (Site.why has the reason):
`fe clamp at 0`, `fe clamp at 1`, `tp clamp at 0`, `tp clamp at 1` (max / min return the same value whichever operand
they pick at equality), `tp >= threshold 0` (no score is below 0), `tp >= threshold 0.9` and `tp >= threshold 1.0`
(tp >= 0.9 declines first). Their sides are still counted, because the values next to them pin the sums' bits.
Sides that cannot exist: a score below 0 or above 1.

Where only a cascade reads a comparison (`fe: ...`, `tp: ...` sites) the observable output is the score itself,
which the GPU test compares bit for bit: the row at the cutoff and the row past it come from one matched group that
differs in that operand alone."""
import math

import numpy as np
import pytest

import fmap_edge_cases as F
from oracle import fmap_ref as R


@pytest.fixture(scope="module")
def case():
    return F.build()


@pytest.fixture(scope="module", params=[0, 1])
def run(request, case):
    with np.errstate(over="ignore"):
        raw, fm, rules = F.reference(request.param)
        return request.param, raw, fm, rules, F.sites(case, raw, fm, rules)


def test_stream_shape(case):
    tx, cuts = case["tx"], case["cuts"]
    n = len(tx["ts_ms"])
    assert n < 4096 and cuts[0] == 0 and cuts[-1] == n
    sizes = set(np.diff(cuts).tolist())
    assert {1, 255, 256, 257} <= sizes and max(sizes) > 257
    # each card's rows keep their order: the velocity cards' times ascend
    for key in np.unique(tx["card_key"]):
        ts = tx["ts_ms"][tx["card_key"] == key]
        assert (np.diff(ts) >= 0).all()
    # the edge rows spread over lanes: rows of a matched group are not neighbours
    g = case["group"]
    assert np.mean(np.abs(np.diff(np.flatnonzero(g == g[g >= 0][0]))) > 1) > 0.5
    assert len(case["merchants"]["fraud_rate"]) > case["n_mext"] > 0
    assert len(case["users_ext"]["key"]) < len(case["users"]["key"])


def test_census_floors(case, run):
    """every site on every side that can exist, and every value of the equality / null tests, with >= 4 rows"""
    mode, raw, fm, rules, sites = run
    rep = F.report(case, raw, fm, rules)
    print(rep)
    for s in sites:
        for side, idx in s.rows().items():
            if side in s.absent:
                assert len(idx) == 0, f"{s.name} {side}: declared impossible\n{rep}"
            else:
                assert len(idx) >= F.FLOOR, f"mode {mode}: {s.name} {side}: {len(idx)} rows\n{rep}"
    vals = F.values(case, raw, fm, rules)
    low = {k: v for k, v in vals.items() if v < F.FLOOR}
    assert not low, f"{low}\n{rep}"
    assert "\n".join(line.rstrip() for line in rep.split("\n")) in F.__doc__, f"the docstring's table is stale:\n{rep}"


def test_velocity_counts_come_from_the_oracle(run):
    """the targets of the issue, read from raw[:, 9] / raw[:, 10]: whether the current event counts is not assumed"""
    _, raw, _, _, _ = run
    for v in (3, 4, 5, 6, 7):
        assert (raw[:, 9] == v).sum() >= F.FLOOR, v
    for v in (10, 11, 20, 21, 22):
        assert (raw[:, 10] == v).sum() >= F.FLOOR, v


def test_sensitivity_to_off_by_one(case, run):
    """at every observable site the rows at the cutoff and the rows one step past it differ in an output"""
    mode, raw, fm, rules, sites = run
    group = case["group"]
    unobservable = []
    for s in sites:
        r = s.rows()
        if s.obs is None:
            assert s.why, s.name
            unobservable.append(s.name)
            continue
        kind, what = s.obs
        for past in s.past:
            at, ps = r["at"], r[past]
            assert len(at) and len(ps), (s.name, past)
            if kind == "pair":
                pairs = [(i, j) for i in at for j in ps if group[i] >= 0 and group[i] == group[j]]
                assert len(pairs) >= F.FLOOR, (s.name, len(pairs))
                assert all(rules[what][i] != rules[what][j] for i, j in pairs), s.name
                continue
            if kind == "col":
                out = np.where(np.isnan(fm[:, what]), -12345.0, fm[:, what])
            elif kind == "rule":
                out = rules[what]
            else:  # the cascade's configured threshold
                _, _, thr_rules = F.oracle_outputs(mode, ctx=case["ctx"], threshold=what / 1000)
                out = thr_rules["tp_risk"]
            a, p = set(out[at].tolist()), set(out[ps].tolist())
            assert a and p and not (a & p), (s.name, past, a, p)
    assert sorted(unobservable) == sorted(["fe clamp at 0", "fe clamp at 1", "tp clamp at 0", "tp clamp at 1",
                                           "tp >= threshold 0", "tp >= threshold 0.9", "tp >= threshold 1.0"])


def test_straddling_pairs_are_adjacent_doubles(case, run):
    """the bisected rows: for each score cutoff there are rows whose driving input differs by one f64 ulp and whose
    scores lie on the two sides of the cutoff"""
    _, raw, fm, rules, _ = run
    group, fs = case["group"], case["ctx"]["fraud_score"]
    risk = fm[:, R.IDX["user_risk_score"]]
    for field, cuts in (("fe_score", F.FE_CUTS + (1.0,)), ("tp_score", (0.5, 0.7, 0.899, 0.9, 1.0))):
        for c in cuts:
            found = 0
            s = rules[field]
            for i in np.flatnonzero((s >= c) & (s <= c + 1e-15) & (group >= 0)):
                for j in np.flatnonzero((group == group[i]) & (s < c)):
                    drive = fs if not math.isnan(fs[i]) else risk
                    found += bool(F._ord(drive[i]) - F._ord(drive[j]) == 1)
            assert found >= F.FLOOR, (field, c, found)


# products whose sum starts from 0.0: fma(a, b, 0.0) is the rounded product itself
FIRST_ADDS = ("amount * 0.2", "user_risk * 0.2")


@pytest.mark.parametrize("site", R.INEXACT_PRODUCTS + R.EXACT_PRODUCTS + R.REORDERINGS)
def test_sensitivity_to_contraction(case, site):
    """A fused multiply-add in place of any product-then-add of the two chains, or either chain added in the
    reverse order, changes score bits on at least 4 rows. Three kinds cannot show and are asserted as such: products by a power of two (0.25, 0.5, 2.0) are exact,
    and the first term of a chain is added to 0.0."""
    raw, fm, rules = F.reference(1)
    _, vel5 = F.oracle_raw(1)
    pay, ref = case["vocab"]
    with np.errstate(over="ignore"):
        _, mut = R.feature_map(case["tx"], case["ctx"], raw, vel5, case["users_ext_by_key"], case["merchants"],
                               case["merchants_ext"], pay, ref, contract={site})
    changed = int(((mut["fe_score"] != rules["fe_score"]) | (mut["tp_score"] != rules["tp_score"])).sum())
    print(site, changed)
    if site in R.EXACT_PRODUCTS or site in FIRST_ADDS:
        assert changed == 0
    else:
        assert changed >= F.FLOOR, (site, changed)


# ---------------------------------------------------------------------------------------------------------------
# known answers

# day counts since 1970-01-01, by hand: 1970..2023 has 53 years and 13 leap days (1972..2020) = 19 358 days to
# 2023-01-01; +31 +27 = 2023-02-28. The others by the same count; before 1970 backwards. The proleptic year 0 is
# leap; 0000-03-01 is day -719 468, the origin of the civil-from-days era arithmetic.
KNOWN_DAYS = (
    (19416, 28, "2023-02-28"), (19417, 1, "2023-03-01"),
    (19781, 28, "2024-02-28"), (19782, 29, "2024-02-29"), (19783, 1, "2024-03-01"),
    (11016, 29, "2000-02-29"), (11017, 1, "2000-03-01"),
    (47540, 28, "2100-02-28"), (47541, 1, "2100-03-01"),
    (-25509, 28, "1900-02-28"), (-25508, 1, "1900-03-01"),
    (20208, 30, "2025-04-30"), (20209, 1, "2025-05-01"), (20300, 31, "2025-07-31"), (20301, 1, "2025-08-01"),
    (20453, 31, "2025-12-31"), (20454, 1, "2026-01-01"),
    (0, 1, "1970-01-01"), (-1, 31, "1969-12-31"),
    (-719469, 29, "0000-02-29"), (-719468, 1, "0000-03-01"), (-719528, 1, "0000-01-01"),
    (-719529, 31, "-0001-12-31"), (-719728, 15, "-0001-06-15"),
    (-719468 - 146097, 1, "-0400-03-01"), (-719469 - 146097, 29, "-0400-02-29"),
)


def test_day_of_month_known_answers():
    for days, dom, name in KNOWN_DAYS:
        assert R.day_of_month(days) == dom, name
    # the explicit count of the case builder agrees with the hand-derived numbers
    for days, dom, name in KNOWN_DAYS:
        y, m, d = name.rsplit("-", 2)
        assert F.days_from_civil(int(y), int(m), int(d)) == days, name
        assert int(d) == dom


def test_calendar_rows_known_answers(case, run):
    """each listed date is in the stream at its first and last millisecond, and the millisecond before it belongs
    to the previous day"""
    _, raw, fm, _, _ = run
    ts, dom = case["tx"]["ts_ms"], fm[:, R.IDX["day_of_month"]]
    by_day = {days: d for days, d, _ in KNOWN_DAYS}
    for y, m, d in F.DATES:
        z = F.days_from_civil(y, m, d)
        for t, want in ((z * F.DAY, d), (z * F.DAY + F.DAY - 1, d), (z * F.DAY - 1, by_day.get(z - 1))):
            rows = np.flatnonzero(ts == t)
            assert len(rows) >= 1, (y, m, d, t)
            if want is not None:
                assert (dom[rows] == want).all(), (y, m, d, t, dom[rows])
    # 1970-01-01 +- 1 ms, and the hour / weekday of the last millisecond of 1969 (a Wednesday, 23 h)
    i = np.flatnonzero(ts == -1)[0]
    assert (raw[i, 2], raw[i, 3], dom[i]) == (23.0, 3.0, 31.0)
    i = np.flatnonzero(ts == 1)[0]
    assert (raw[i, 2], raw[i, 3], dom[i]) == (0.0, 4.0, 1.0)


def _plain_row(fraud_score):
    """a verified two-year-old user (risk 0.1, average 100) buys for 123.45 at a low-risk merchant (fraud rate 0.01)
    at 13 h on a Friday from a known device and a public address"""
    raw = np.zeros((1, 16))
    raw[0, 0], raw[0, 1], raw[0, 2], raw[0, 3] = 123.45, math.log(124.45), 13, 5
    raw[0, 5], raw[0, 7], raw[0, 8], raw[0, 14], raw[0, 15] = 0.01, 0.3, 100.0, 1.0, 400
    tx = {"card_key": np.array([7], np.uint64), "ts_ms": np.array([F.T0 + 13 * F.HOUR], np.int64),
          "amount_cents": np.array([12345], np.int64), "merchant": np.array([0], np.int32),
          "device_fp": np.array([5], np.uint64), "ip_class": np.array([2], np.uint8),
          "hour": np.array([255], np.uint8), "weekend": np.array([255], np.uint8)}
    users = {7: dict(F.USER_EXT_DEFAULT)}
    merchants = {"fraud_rate": np.array([0.01]), "risk_multiplier": np.array([1.0])}
    mext = {k: np.array([v], F.MERCH_EXT_DT[k]) for k, v in F.MERCH_EXT_DEFAULT.items()}
    z = np.zeros(256, np.uint8)
    ctx = {"user_agent_flag": np.array([0], np.uint8), "fraud_score": np.array([fraud_score])}
    _, rules = R.feature_map(tx, ctx, raw, np.array([0.0]), users, merchants, mext, z, z)
    return rules[0]


def _smallest(fn, guess, cut):
    """the smallest double near `guess` whose fn reaches `cut` (fn is non-decreasing)"""
    x = guess
    while fn(x) >= cut:
        x = F.dn(x)
    while fn(x) < cut:
        x = F.up(x)
    return x


def test_known_answer_fe_pair():
    """FeatureEnrichmentProcessor.java:80-93,122-149 by hand: amount 0; temporal 0; user risk .1 * .5; merchant
    .01 * 2; velocity 0; device ip risk .3 -> weighted .0125 + .004 + .03; combined x * .6 + that * .4"""
    fb = 0.0
    fb += 0.0 * 0.2
    fb += 0.0 * 0.1
    fb += (0.1 * 0.5) * 0.25
    fb += (0.01 * 2.0) * 0.2
    fb += 0.0 * 0.15
    fb += 0.3 * 0.1
    fe = lambda x: (x * 0.6) + (fb * 0.4)  # noqa: E731
    hi = _smallest(fe, (0.6 - fb * 0.4) / 0.6, 0.6)
    lo = F.dn(hi)
    assert fe(lo) < 0.6 <= fe(hi) and 0.96 < hi < 0.97
    a, b = _plain_row(lo), _plain_row(hi)
    assert (a["fe_score"], b["fe_score"]) == (fe(lo), fe(hi))
    assert (a["fe_risk"], a["fe_decision"]) == (R.LOW, R.APPROVE)
    assert (b["fe_risk"], b["fe_decision"]) == (R.MEDIUM, R.REVIEW)


def test_known_answer_tp_pair():
    """TransactionProcessor.java:330-345 by hand: x * .5, user risk .1 * .2, nothing from the merchant or the flags;
    REVIEW / HIGH from the default threshold 0.7 on"""
    def tp(x):
        s = x * 0.5
        s += 0.1 * 0.2
        s += 0.0
        s += 0.0
        return s
    hi = _smallest(tp, (0.7 - 0.02) / 0.5, 0.7)
    lo = F.dn(hi)
    assert tp(lo) < 0.7 <= tp(hi) and 1.35 < hi < 1.37
    a, b = _plain_row(lo), _plain_row(hi)
    assert (a["tp_score"], b["tp_score"]) == (tp(lo), tp(hi))
    assert (a["tp_decision"], a["tp_risk"]) == (R.APPROVE, R.MEDIUM)
    assert (b["tp_decision"], b["tp_risk"]) == (R.REVIEW, R.HIGH)


def test_distance_is_nan_where_java_sqrt_is():
    """FeatureExtractor.java:407-418: Math.sqrt of a negative operand is NaN and atan2 passes it on"""
    assert math.isnan(R.distance_from_a(F.up(1.0))) and math.isnan(R.distance_from_a(-1e-300))
    assert math.isnan(R.distance_from_a(F.NaN))
    assert R.distance_from_a(0.0) == 0.0 and R.distance_from_a(1.0) == 6371 * math.pi
    assert math.isnan(R.haversine_a(F.INF, 0.0, 0.0, 0.0))
    assert R.haversine_a(0.0, 0.0, 0.0, 180.0) == 1.0 and R.haversine_a(12.5, 77.6, 12.5, 77.6) == 0.0
