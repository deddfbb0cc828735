"""GPU: feat_ext_kernel (the 64-column FeatureExtractor map and both Flink rule cascades) on the edge stream of
tests/fmap_edge_cases.py, against the C oracle's raw features and oracle/fmap_ref.py. The stream puts every
comparator's operand on, just below and just above its cutoff (tests/test_fmap_edges_cpu.py proves that on the CPU),
so an off-by-one comparison, a contracted multiply-add or a reordered sum changes a row here.

Bars, those of test_gpu_fmap.py: every column bit-equal (the sign of zero included) except amount_log (device log,
<= 1 ulp) and distance_to_merchant_km; every rule score and code bit-equal, the straddling pairs included.

Distance: rtol 1e-9 where the reference's own haversine `a` is below 1 - 1e-6. Nearer to 1 the result
6371 * 2 * atan2(sqrt(a), sqrt(1 - a)) is ill-conditioned in `a` and no implementation can hold that bar; there the
bar is the spread of the reference's own result when its `a` moves by +-A_ULPS ulps, and NaN is accepted where
a + A_ULPS ulps exceeds 1 (Java's Math.sqrt(1 - a) is NaN there). ASSUMPTION behind A_ULPS = 20: the device's sin
and cos err by at most 4 ulp each, OpenCL's bound for double precision, which the ROCm device library implements;
the ROCm install carries no HIP math accuracy table to take a tighter number from. `a` is sin^2 + cos * cos * sin^2:
the four-factor product carries 4 * 4 ulp from its factors and 3 from its multiplications, the sum one more. The
number is not fitted to what the kernel returns."""
import numpy as np
import pytest

import fmap_edge_cases as F
from fdengine import FraudEngine
from fdengine._native import CTX_FIELDS, RULE_DTYPE, TXN_FIELDS
from oracle import fmap_ref as R

pytestmark = pytest.mark.gpu

A_ULPS = 20
RULE_FIELDS = ("tp_score", "fe_score", "tp_decision", "tp_risk", "fe_decision", "fe_risk")
COL_LOG, COL_DIST = R.IDX["amount_log"], R.IDX["distance_to_merchant_km"]


def _load(eng, case, mode, cap=F.CAP):
    U, M, ue, me = case["users"], case["merchants"], case["users_ext"], case["merchants_ext"]
    eng.state_init(cap, mode, F.RING_K)
    eng.load_users(U["key"], U["avg_amount"], U["account_age_days"], U["device_fp"])
    eng.load_merchants(M["fraud_rate"], M["risk_multiplier"])
    eng.load_users_ext(ue["key"], **{k: v for k, v in ue.items() if k != "key"})
    eng.load_merchants_ext(case["n_mext"], **me)
    eng.load_vocab(*case["vocab"])


def _run(eng, case, batches=None, ctx_fields=CTX_FIELDS, want_fmap=True, want_rules=True):
    """the stream's batches through features_full_device -> (fmap [n, 64] or None, rule records or None)"""
    import torch
    tx, ctx, cuts = case["tx"], case["ctx"], case["cuts"]
    fms, rls = [], []
    for a, b in (list(zip(cuts[:-1], cuts[1:])) if batches is None else batches):
        n = b - a
        dev = {f: torch.from_numpy(tx[f][a:b].copy()).cuda() for f in TXN_FIELDS}
        dctx = {f: torch.from_numpy(ctx[f][a:b].copy()).cuda() for f in ctx_fields}
        vec = torch.empty((n, 64), dtype=torch.float32, device="cuda")
        fmap = torch.full((n, 64), -7.0, dtype=torch.float64, device="cuda")
        rules = torch.full((n, 24), 0xEE, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()  # the fills ran on torch's stream; a fresh engine writes on its own
        eng.features_full_device({f: t.data_ptr() for f, t in dev.items()},
                                 {f: t.data_ptr() for f, t in dctx.items()} if ctx_fields else None, n,
                                 vec.data_ptr(), fmap.data_ptr() if want_fmap else 0,
                                 rules.data_ptr() if want_rules else 0)
        torch.cuda.synchronize()
        fms.append(fmap.cpu().numpy())
        rls.append(rules.cpu().numpy().reshape(-1).view(np.dtype(RULE_DTYPE)))
    return (np.concatenate(fms) if want_fmap else None), (np.concatenate(rls) if want_rules else None)


def _bits_equal(got, want, msg):
    np.testing.assert_array_equal(got, want, err_msg=msg)
    ok = ~np.isnan(want)
    np.testing.assert_array_equal(np.signbit(got[ok]), np.signbit(want[ok]), err_msg=msg + " (sign of zero)")


def _distance_bars(case, rows):
    """per row of `rows`: (absolute bar, NaN allowed) from the reference's own `a` (module docstring)"""
    ctx = case["ctx"]
    bars, nan_ok = np.zeros(len(rows)), np.zeros(len(rows), bool)
    for k, i in enumerate(rows):
        a = R.haversine_a(*[float(ctx[f][i]) for f in ("geo_lat", "geo_lon", "merchant_lat", "merchant_lon")])
        d = R.distance_from_a(a)
        if a < 1 - 1e-6:
            bars[k] = 1e-9 * abs(d)
            continue
        hi = a + A_ULPS * np.spacing(a)
        lo = a - A_ULPS * (a - np.nextafter(a, 0.0))
        nan_ok[k] = hi > 1.0
        bars[k] = max(abs(R.distance_from_a(min(hi, 1.0)) - d), abs(R.distance_from_a(lo) - d))
    return bars, nan_ok


def _check_fmap(case, got, efm):
    exact = [c for c in range(64) if c not in (COL_LOG, COL_DIST)]
    for c in exact:
        _bits_equal(got[:, c], efm[:, c], R.NAMES[c])
    np.testing.assert_array_max_ulp(got[:, COL_LOG], efm[:, COL_LOG], maxulp=1)
    want = efm[:, COL_DIST]
    rows = np.flatnonzero(~np.isnan(want))
    np.testing.assert_array_equal(np.isnan(got[np.isnan(want), COL_DIST]), True)
    bars, nan_ok = _distance_bars(case, rows)
    g = got[rows, COL_DIST]
    bad = np.where(np.isnan(g), ~nan_ok, np.abs(g - want[rows]) > bars)
    assert not bad.any(), [(int(rows[k]), float(g[k]), float(want[rows[k]]),
                           float(bars[k])) for k in np.flatnonzero(bad)]


def _check_rules(got, erules, rows=slice(None)):
    for f in RULE_FIELDS:
        if f.endswith("score"):
            _bits_equal(got[f], erules[f][rows], f)
        else:
            np.testing.assert_array_equal(got[f], erules[f][rows], err_msg=f)


@pytest.fixture
def stream_engine(engine):
    import torch
    engine.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        yield engine
    finally:
        engine.set_option("rule_fraud_threshold_permille", 700)
        engine.set_stream(None)


@pytest.mark.parametrize("mode", [0, 1])
def test_edges_match_oracle(stream_engine, mode):
    case = F.build()
    _, efm, erules = F.reference(mode)
    _load(stream_engine, case, mode)
    got, rules = _run(stream_engine, case)
    _check_fmap(case, got, efm)
    _check_rules(rules, erules)
    assert (rules["pad"] == 0).all()
    # the distance cases did reach the ill-conditioned end
    d = got[:, COL_DIST]
    assert (d == 0.0).sum() >= 4 and (d > 20000.0).sum() >= 8


def test_null_context(stream_engine):
    """no context at all, and each context field left out in turn (the kernel's `ptr ? ptr[i] : null` arms)"""
    case, mode = F.build(), 1
    for drop in (None,) + tuple(CTX_FIELDS):
        fields = () if drop is None else tuple(f for f in CTX_FIELDS if f != drop)
        _, efm, erules = F.oracle_outputs(mode, ctx=None if drop is None else case["ctx"], drop=(drop,))
        _load(stream_engine, case, mode)
        got, rules = _run(stream_engine, case, ctx_fields=fields)
        _check_fmap(case, got, efm)
        _check_rules(rules, erules)
    assert np.isnan(efm[:, R.IDX["suspicious_user_agent"]]).sum() > 0


def test_rules_only_and_map_only(stream_engine):
    case, mode = F.build(), 1
    _, efm, erules = F.reference(mode)
    _load(stream_engine, case, mode)
    got, rules = _run(stream_engine, case, want_fmap=False)
    assert got is None
    _check_rules(rules, erules)
    _load(stream_engine, case, mode)
    got, rules = _run(stream_engine, case, want_rules=False)
    assert rules is None
    _check_fmap(case, got, efm)


@pytest.mark.parametrize("permille", F.THRESHOLDS_PERMILLE)
def test_rule_threshold(stream_engine, permille):
    """JobConfig.fraudThreshold as the engine option: the rows bisected onto that threshold (and every other row)
    against feature_map(..., threshold=permille / 1000)"""
    case, mode = F.build(), 1
    _, _, erules = F.oracle_outputs(mode, ctx=case["ctx"], threshold=permille / 1000)
    _, _, default = F.reference(mode)
    c = permille / 1000
    tp = erules["tp_score"]
    assert (tp == c).sum() >= F.FLOOR
    if permille > 0:
        assert ((tp < c) & (tp >= c - 1e-15)).sum() >= F.FLOOR
    if permille != 700:
        assert (erules["tp_risk"] != default["tp_risk"]).any()
    stream_engine.set_option("rule_fraud_threshold_permille", permille)
    _load(stream_engine, case, mode)
    _, rules = _run(stream_engine, case, want_fmap=False)
    _check_rules(rules, erules)


def test_snapshot_carries_rule_threshold(stream_engine, tmp_path):
    """a non-default threshold, snapshot, restore into a fresh engine: the same rules without setting it again"""
    case, mode = F.build(), 1
    cuts = case["cuts"]
    batches = list(zip(cuts[:-1], cuts[1:]))
    _, _, erules = F.oracle_outputs(mode, ctx=case["ctx"], threshold=0.899)
    _, _, default = F.reference(mode)
    first = batches[3][0]
    assert (erules["tp_risk"][first:] != default["tp_risk"][first:]).any()
    stream_engine.set_option("rule_fraud_threshold_permille", 899)
    _load(stream_engine, case, mode)
    _run(stream_engine, case, batches=batches[:3], want_fmap=False)
    path = tmp_path / "edges.fdsnap"
    stream_engine.state_snapshot(path)
    cards = stream_engine.state_info()["cards"]
    fresh = FraudEngine(0)
    try:
        fresh.state_init(1 << 15, mode, F.RING_K)  # another capacity; no option, no tables: all from the image
        assert fresh.state_restore(path) == cards
        _, rules = _run(fresh, case, batches=batches[3:], want_fmap=False)
    finally:
        fresh.close()
    _check_rules(rules, erules, slice(first, None))
