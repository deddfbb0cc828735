"""Edge streams for the card velocity windows (csrc/features.hip velocity_step / process_long), the CPU census
of which code site meets which edge, and a plain full-scan reference whose comparison operators are parameters.

Every time decision of the feature kernels is an integer-millisecond comparison (t - W < et <= t for W in
5 min / 1 h / 24 h; t - last <= 3 600 000 for the redis_compat session). Random Poisson streams almost never put
an event exactly on such an edge, so these streams are built from them:

* per-card time scripts (`_script`): gaps from ALPHABET (members and pairwise sums land on every edge), "hits"
  that place an event exactly W - 1, W or 0 ms after one of the card's last K events (and 1 ms before one while
  the ring is unsorted), descents ts[i - j] + d (j within the ring, d in -1 / 0 / +1) at a rate of 1 / (3 K),
  bursts of >= K + 2 events inside 5 minutes (a full ring whose window spans it), one card that starts at negative
  event times and crosses ts = 0. The script tracks the kernel's `unsorted` countdown only to steer hits to the
  rare step at which the ring becomes sorted again (the rebuild: always a hit there, never a descent or a burst).
* four layouts of micro-batches (`edge_stream`): `one` (one event per card per batch), `short` (runs of 1..16),
  `long` (runs from LONG_RUNS, all cooperative), `mixed` (long and short runs alternating per card). `long` and
  `mixed` place a descent K, K - 1 or 0 events before the end of a long run (the `unsorted` value carried out of
  the cooperative path is then 0, 1 or K) and give one card a run of HOT_RUN events in one batch (an oversized
  bucket: passes by arrival range). `one` / `short` use 64 cards x 240 events; `long` / `mixed` fewer cards with
  longer scripts (a 300-event run does not fit 240 events) from the same script generator.

Rows of a batch interleave the cards at random and keep each card's order. Streams stay under ~16 k rows.
"""
import functools
import operator

import numpy as np

from fdengine import synth
from fdengine._native import TXN_FIELDS

W5, W1H, W24H = 300_000, 3_600_000, 86_400_000
WINDOWS = (W5, W1H, W24H)
TTL = 3_600_000
SEG_LONG = 16      # features.hip kSegLong: longer segments take the cooperative path
TILE = 256         # features.hip kBT: the cooperative path's tile
LAYOUTS = ("one", "short", "long", "mixed")
LONG_RUNS = (17, 40, 255, 256, 257, 300)
HOT_RUN = 4500     # > kChunkCap (4096) keys in one bucket
T0 = 1_757_030_400_000

ALPHABET = (0, 1, 2, W5 - 2, W5 - 1, W5, W5 + 1,
            (W1H - W5) - 1, W1H - W5, (W1H - W5) + 1,
            (W24H - W1H) - 1, W24H - W1H, (W24H - W1H) + 1,
            W1H, W1H + 1, W24H)
HITS = tuple(W + d for W in WINDOWS for d in (-1, 0)) + (0,)


def _script(rng, n, K, t0, anchors=frozenset(), quiet=frozenset()):
    """One card's n event times. `anchors`: indices that must be a descent; `quiet`: indices that must not."""
    ts = np.empty(n, np.int64)
    ts[0] = t0
    us = burst = 0
    p_desc, p_burst = 1.0 / (3 * K), 0.15 / (K + 2)
    for i in range(1, n):
        prev, depth = int(ts[i - 1]), min(K, i)
        if i in anchors:
            t = min(int(ts[i - int(rng.integers(1, depth + 1))]) + int(rng.integers(-1, 2)), prev - 1)
        elif i not in quiet and us != 1 and rng.random() < p_desc:
            t = int(ts[i - int(rng.integers(1, depth + 1))]) + int(rng.integers(-1, 2))
        elif burst > 0 or (i not in quiet and us != 1 and rng.random() < p_burst):
            burst = burst - 1 if burst > 0 else K + 1 + int(rng.integers(0, 4))
            t = prev + int(rng.choice((0, 1, 2, int(rng.integers(0, W5 // (K + 8))))))
        else:
            t = None
            if us == 1 or rng.random() < 0.5:  # us == 1: this step rebuilds the windows
                off = int(rng.choice(HITS + (-1,) if us > 1 else HITS))
                ok = [int(e) + off for e in ts[i - depth:i] if int(e) + off >= prev]  # not a descent
                if ok:
                    t = ok[int(rng.integers(0, len(ok)))]
            if t is None:
                t = prev + int(rng.choice(ALPHABET))
        us = K if t < prev else max(us - 1, 0)
        ts[i] = t
    return ts


def _runs(rng, layout, n, hot=False):
    """run lengths (events of the card per batch) that cut a script of n events"""
    if layout == "one":
        return [1] * n
    runs, left, long_next = [], n, True
    if hot:  # a few ordinary runs, the hot run, then the rest
        runs = [17, 5 if layout == "mixed" else 20, HOT_RUN]
        left = n - sum(runs)
    while left > 0:
        if layout == "short" or (layout == "mixed" and not long_next):
            r = int(rng.integers(1, SEG_LONG + 1))
        else:
            r = int(rng.choice(LONG_RUNS, p=(0.3, 0.3, 0.1, 0.1, 0.1, 0.1)))
            if layout == "mixed":  # more alternations: more short rows behind a long segment
                r = int(rng.choice(LONG_RUNS, p=(0.6, 0.2, 0.05, 0.05, 0.05, 0.05)))
        long_next = not long_next
        if r > left or (r > SEG_LONG and left - r <= SEG_LONG and layout == "long"):
            r = left
        if layout == "long" and r <= SEG_LONG:  # a remainder too short for a run of its own joins the last run
            runs[-1] += r
        else:
            runs.append(r)
        left -= r
    return runs


def _anchors(rng, runs, K):
    """descents placed so that the cooperative path carries unsorted = 0, 1 and K out of a long run"""
    anchors, quiet, pos = set(), set(), 0
    for r in runs:
        if r > SEG_LONG and pos > 0 and rng.random() < 0.5:
            back = int(rng.choice((K, K - 1, 0)))
            last = pos + r - 1
            if last - back > pos:  # the descent stays inside the run (K = 64 needs a run of more than 65)
                anchors.add(last - back)
                quiet.update(range(last - back + 1, last + 1))
        pos += r
    return frozenset(anchors), frozenset(quiet - anchors)


def edge_stream(pop, layout, K, seed=0):
    """-> (tx, cuts): a transaction dict with every TXN_FIELDS column (and is_fraud) in arrival order, and the
    micro-batch boundaries. Card keys are the population's first users."""
    assert layout in LAYOUTS
    rng = np.random.default_rng([seed, K, LAYOUTS.index(layout)])
    big = layout in ("long", "mixed")
    n_cards, n_ev = (13, 800) if big else (64, 240)
    keys = pop["users"]["key"][:n_cards]
    scripts, plans = [], []
    for c in range(n_cards):
        hot = big and c == 1
        n = HOT_RUN + 300 if hot else n_ev
        runs = _runs(rng, layout, n, hot=hot)
        anchors, quiet = _anchors(rng, runs, K) if big else (frozenset(), frozenset())
        t0 = -20 * W24H - 1 if c == 0 else T0 + int(rng.integers(0, W24H))  # card 0 crosses ts = 0
        scripts.append(_script(rng, n, K, t0, anchors, quiet))
        plans.append(runs)
    card, pos, cuts = [], [], [0]
    done = [0] * n_cards
    for b in range(max(len(p) for p in plans)):
        who = np.concatenate([np.full(plans[c][b], c) for c in range(n_cards) if b < len(plans[c])])
        who = rng.permutation(who)
        for c in who:  # a card's rows keep their order
            card.append(c)
            pos.append(done[c])
            done[c] += 1
        cuts.append(len(card))
    card, pos = np.array(card), np.array(pos)
    tx = synth.txn_stream(pop, len(card), seed=seed + 1, unknown_merchant_frac=0.02)
    tx["card_key"] = keys[card].copy()
    tx["ts_ms"] = np.array([scripts[c][p] for c, p in zip(card, pos)], np.int64)
    assert set(TXN_FIELDS) <= set(tx)
    return tx, cuts


@functools.lru_cache(maxsize=None)
def population():
    return synth.population(64, 50, seed=77)


@functools.lru_cache(maxsize=None)
def stream(layout, K):
    """the suite's edge stream for (layout, K), built once; callers leave it unchanged"""
    tx, cuts = edge_stream(population(), layout, K)
    for v in tx.values():
        v.setflags(write=False)
    return tx, tuple(cuts)


def oracle_pair(engine, mode, K, seq_len=0):
    """the engine's card state and the C oracle's, both empty, over the edge streams' population"""
    from oracle.features_c import OracleFeatureState
    U, M = population()["users"], population()["merchants"]
    cap = 8192
    if engine is not None:
        engine.state_init(cap, mode, K, seq_len=seq_len)
        engine.load_users(U["key"], U["avg_amount"], U["account_age_days"], U["device_fp"])
        engine.load_merchants(M["fraud_rate"], M["risk_multiplier"])
    orc = OracleFeatureState(cap, mode, K)
    orc.load_users(U["key"], U["avg_amount"], U["account_age_days"], U["device_fp"])
    orc.load_merchants(M["fraud_rate"], M["risk_multiplier"])
    return orc


# ---------------------------------------------------------------------------------------------------------------
# the census: which code site handles each row, and which edges it meets there

def prior_events(tx, K):
    """each row's previous K events of its card, newest first: (et, cents, valid), each [n, K]"""
    n = len(tx["ts_ms"])
    et = np.zeros((n, K), np.int64)
    ec = np.zeros((n, K), np.int64)
    valid = np.zeros((n, K), bool)
    for key in np.unique(tx["card_key"]):
        idx = np.flatnonzero(tx["card_key"] == key)
        for j in range(1, min(K, len(idx) - 1) + 1):
            et[idx[j:], j - 1] = tx["ts_ms"][idx[:-j]]
            ec[idx[j:], j - 1] = tx["amount_cents"][idx[:-j]]
            valid[idx[j:], j - 1] = True
    return et, ec, valid


SITES = ("long", "inc", "full", "rebuild")


def sites(tx, cuts, K):
    """Restates the kernels' dispatch. Per row: site (index into SITES: the cooperative path, or in a short segment
    the incremental windows, a full scan, the full-scan step at which `unsorted` returns to 0 and the windows are
    rebuilt), and for the first short row behind a long segment of its card the `unsorted` value carried out of it
    (-1 elsewhere). An oversized bucket's passes by arrival range are not modelled (the hot run counts as long)."""
    ts, key = tx["ts_ms"], tx["card_key"]
    site = np.zeros(len(ts), np.int8)
    carried = np.full(len(ts), -1, np.int64)
    st = {}  # card -> [ring_n, last_ts, unsorted, behind a long segment]
    for a, b in zip(cuts[:-1], cuts[1:]):
        rows = {}
        for i in range(a, b):
            rows.setdefault(int(key[i]), []).append(i)
        for k, idx in rows.items():
            s = st.setdefault(k, [0, 0, 0, False])
            if len(idx) > SEG_LONG:
                site[idx] = 0
                for t0 in range(0, len(idx), TILE):  # process_long's carry, tile by tile
                    tile = idx[t0:t0 + TILE]
                    d = -1
                    for j, i in enumerate(tile):
                        prev = s[1] if (t0 == 0 and j == 0) else int(ts[idx[t0 + j - 1]])
                        if (s[0] > 0 or t0 + j > 0) and int(ts[i]) < prev:
                            d = j
                    s[2] = max(0, K - (len(tile) - 1 - d)) if d >= 0 else max(0, s[2] - len(tile))
                s[0], s[1], s[3] = min(K, s[0] + len(idx)), int(ts[idx[-1]]), True
                continue
            for q, i in enumerate(idx):
                t = int(ts[i])
                descent = s[0] > 0 and t < s[1]
                inc = s[2] == 0 and not descent
                if q == 0 and s[3]:
                    carried[i] = s[2]
                s[2] = K if descent else max(s[2] - 1, 0)
                site[i] = 1 if inc else (3 if s[2] == 0 else 2)
                s[0], s[1] = min(K, s[0] + 1), t
            s[3] = False
    return site, carried


def census(tx, cuts, K):
    """-> dict of counts: (site, W, 'in' | 'out'), (site, 'equal'), (site, 'future'), ('session', path, gap),
    'spanning_overwrites', ('after_long', 'sorted' | 'unsorted')."""
    et, _, valid = prior_events(tx, K)
    dt = tx["ts_ms"][:, None] - et
    site, carried = sites(tx, cuts, K)
    out = {}
    for s, name in enumerate(SITES):
        out[name, "rows"] = int((site == s).sum())
        at = (site == s)[:, None] & valid
        for W in WINDOWS:
            out[name, W, "in"] = int((at & (dt == W - 1)).any(1).sum())
            out[name, W, "out"] = int((at & (dt == W)).any(1).sum())
        out[name, "equal"] = int((at & (dt == 0)).any(1).sum())
        out[name, "future"] = int((at & (dt == -1)).any(1).sum())
    for path, m in (("short", site != 0), ("long", site == 0)):
        for gap in (TTL, TTL + 1):
            out["session", path, gap] = int((m & valid[:, 0] & (dt[:, 0] == gap)).sum())
    in24 = (valid & (dt >= 0) & (dt < W24H)).sum(1)
    out["spanning_overwrites"] = int(((site == 1) & (valid.sum(1) == K) & (in24 == K)).sum())
    out["after_long", "sorted"] = int((carried == 0).sum())
    out["after_long", "unsorted"] = int((carried > 0).sum())
    out["after_long", "carried_1"] = int((carried == 1).sum())
    out["after_long", "carried_K"] = int((carried == K).sum())
    return out


# ---------------------------------------------------------------------------------------------------------------
# the definition, operators as parameters

def windows_full_scan(tx, K, lower=operator.lt, upper=operator.le, depth=None):
    """Sliding mode by the definition: prior events e among the card's last `depth` (K) with
    lower(t - W, e.ts) and upper(e.ts, t). -> counts [n, 3], cents sums [n, 3]."""
    et, ec, valid = prior_events(tx, K if depth is None else depth)
    t = tx["ts_ms"][:, None]
    counts, sums = [], []
    for W in WINDOWS:
        m = valid & lower(t - W, et) & upper(et, t)
        counts.append(m.sum(1))
        sums.append((ec * m).sum(1))
    return np.stack(counts, 1), np.stack(sums, 1)


def always(a, b):
    return np.ones(np.broadcast(a, b).shape, bool)


def session_scan(tx, live=operator.le):
    """redis_compat: the session counter a read at t sees, live(t - last, TTL). -> counts [n], cents sums [n]"""
    st = {}
    n = len(tx["ts_ms"])
    counts, sums = np.zeros(n, np.int64), np.zeros(n, np.int64)
    for i in range(n):
        k, t = int(tx["card_key"][i]), int(tx["ts_ms"][i])
        c, s, last = st.get(k, (0, 0, None))
        if last is None or not live(t - last, TTL):
            c = s = 0
        counts[i], sums[i] = c, s
        st[k] = (c + 1, s + int(tx["amount_cents"][i]), t)
    return counts, sums


def window_mutants(K):
    """off-by-one variants of the sliding definition (keyword arguments of windows_full_scan)"""
    return {"lower_edge_inclusive": dict(lower=operator.le),   # t - W <= et
            "upper_edge_strict": dict(upper=operator.lt),      # et < t
            "future_counted": dict(upper=always),              # no upper edge
            "ring_depth_k_minus_1": dict(depth=K - 1)}
