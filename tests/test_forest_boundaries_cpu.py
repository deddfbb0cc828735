"""CPU: the boundary-valued models and rows of oracle/boundary_ref.py, proved before any kernel sees them.

* The plain numpy walk (walk_reference) agrees with the C oracle on every boundary model, and — IsolationForest —
  with sklearn itself: apply() per estimator, and 1 / (1 + exp(decision_function)) within 1e-12 (the bar of
  test_iforest_parity_vs_sklearn). sklearn honours thresholds written into tree_.threshold, so it stays the reference
  for the hand-placed ones.
* Coverage: every (feature, threshold) of a model is met by a row holding the threshold, its f32 next-up and its
  next-down, and each wrong comparison (`<=` for XGBoost's `<`; `<` for sklearn's `<=`; sklearn's compare against
  (float)thr) changes the leaf-id vector of at least 25 % of the rows of every matrix the GPU tests use.
* The engine's host packing (threshold layout and binned layout, walked in Python) on boundary rows."""
import numpy as np
import pytest

import oracle
from oracle import boundary_ref as B
from oracle import forest_ref
from fdengine import pack_forest_host
from fdengine.engine import pack_forest_binned_host

# (sklearn's own input check sums the matrix, and +FLT_MAX + -FLT_MAX rows overflow that sum: harmless)
pytestmark = pytest.mark.filterwarnings("ignore:invalid value encountered in reduce")

MIN_SHARE = 0.25
WRONG = {True: ("le",), False: ("lt", "lt_f32", "le_f32")}


def test_ladder_properties():
    doc, sets = B.ladder_xgboost_doc(seed=101)
    sizes = [len(s) for s in sets]
    assert set(sizes) >= {0, 1, 2, 3, 4, 5, 7, 8, 9, 31, 32, 33, 63, 64, 65, 255, 256, 257}
    assert len(sizes) % 4 != 0 and len(sizes) % 16 != 0
    fa = B.model("ladder")[0]
    for f, (s, t) in enumerate(zip(sets, B.feature_thresholds(fa))):
        np.testing.assert_array_equal(s, t)  # every (feature, threshold) pair is a split of the model
        if len(s) >= 8:  # the mix: both signs, a run of three consecutive floats, 0.0, a denormal, a value above 2^24
            assert (s < 0).any() and (s > 0).any() and (s == 0).any() and (s > 2.0 ** 24).any()
            assert ((s != 0) & (np.abs(s) < np.finfo(np.float32).tiny)).any()
            assert any(s[i + 1] == B.up32(s[i]) and s[i + 2] == B.up32(s[i + 1]) for i in range(len(s) - 2))
    kinds = set()
    for s in sets:  # the small sets together hold every kind
        kinds |= {"zero"} if (s == 0).any() else set()
        kinds |= {"denormal"} if ((s != 0) & (np.abs(s) < np.finfo(np.float32).tiny)).any() else set()
        kinds |= {"big"} if (s > 2.0 ** 24).any() else set()
    assert kinds == {"zero", "denormal", "big"}


def test_rewritten_iforest_thresholds_are_at_and_beside_data_values():
    fa, m = B.model("iforest")
    thr = fa.threshold[fa.left != -1]
    near = B.floor32(thr)
    d = near.astype(np.float64)
    kinds = {"equal": (thr == d).sum(), "above": (thr > d).sum(), "zero": (thr == 0.0).sum()}
    assert all(v > 0 for v in kinds.values()), kinds
    up = B.up32(near).astype(np.float64)
    assert (thr < up).all() and ((thr > d) & (thr - d > (up - d) / 4)).any()  # f64 next-up, and the midpoint
    # sklearn reads the rewritten array: its own leaves differ from those of the thresholds rounded to f32
    X, ref, _ = B.matrix("iforest")
    np.testing.assert_array_equal(ref["iforest"][0], np.stack([e.apply(X) for e in m.estimators_], 1))


@pytest.mark.parametrize("key", sorted(B.MATRICES))
def test_reference_agrees_and_rows_cover(key):
    X, ref, depth = B.matrix(key)
    for name, (leaf, sums) in ref.items():
        fa, m = B.model(name)
        xgb = B._is_xgb(fa)
        if xgb:
            _, margin, oleaf = oracle.xgb_predict(fa, X, want_leaf=True)
            np.testing.assert_array_equal(leaf, oleaf)
            assert sums.dtype == np.float32
            np.testing.assert_array_equal(sums, margin)
        else:
            prob, dsum, oleaf = oracle.iforest_predict(fa, X, want_leaf=True)
            np.testing.assert_array_equal(leaf, oleaf)
            np.testing.assert_array_equal(sums, dsum)
            np.testing.assert_array_equal(leaf, np.stack([e.apply(X) for e in m.estimators_], 1))
            sk = 1.0 / (1.0 + np.exp(m.decision_function(X)))
            assert np.abs(prob - sk).max() <= 1e-12
            mine = 1.0 / (1.0 + np.exp(-np.exp2(-sums / fa.if_denominator) - fa.if_offset))
            assert np.abs(mine - sk).max() <= 1e-12
        assert B.covers(fa, X, depth[name]), f"{key}: a threshold of {name} or a neighbour of it is in no row"
        for cmp_ in WRONG[xgb]:
            share = B.changed_share(fa, X, cmp_)
            print(f"coverage {key:14s} {name:16s} wrong compare {cmp_:7s} changes {100 * share:5.1f} % of the rows")
            assert share >= MIN_SHARE, (key, name, cmp_, share)


def _plan_passes(counts, stage_floats):
    """the pass boundaries ensemble_plan.hip's plan_passes chooses for per-feature table sizes `counts`: a pass takes
    consecutive features while count + count / 32 + 1 <= stage_floats (one pad word per 32 entries); a table that
    does not fit alone is searched in global memory"""
    off = np.concatenate([[0], np.cumsum(counts)])
    f, cuts = 0, []
    while f < len(counts):
        g = f
        while g < len(counts) and (off[g + 1] - off[f]) + (off[g + 1] - off[f]) // 32 + 1 <= stage_floats:
            g += 1
        glob = g == f
        g = f + 1 if glob else g
        cuts.append((f, g, glob))
        f = g
    return cuts


def _merged_counts(names):
    tabs = []
    for n in names:
        _, thr, off, _ = pack_forest_binned_host(B.model(n)[0])
        tabs.append([thr[off[f]:off[f + 1]] for f in range(len(off) - 1)])
    return [len(np.unique(np.concatenate([t[f] for t in tabs]))) for f in range(len(tabs[0]))]


def test_passcut_plan_cuts_a_group_of_four():
    """The fused kernel stages the merged threshold tables in passes; stage_floats = (2 * chunk buffer + 2 * 8 KiB of
    tiles) / 4 = 28672 floats with the wide chunks (48 KiB buffers) and 24576 with the compact ones (40 KiB). The
    pass-cut pair's features 0 .. 4 fit a pass under either, feature 5 does not: pass 1 starts at feature 5, inside
    the lockstep group of four features 4 .. 7. The two-feature pair's tables each exceed the staging area."""
    counts = _merged_counts(B.MATRICES["pair_passcut"]["names"])
    for stage_floats in ((2 * 49152 + 2 * 8192) // 4, (2 * 40960 + 2 * 8192) // 4):
        cuts = _plan_passes(counts, stage_floats)
        assert cuts == [(0, 5, False), (5, len(counts), False)], cuts
    for stage_floats in (28672, 24576):
        assert _plan_passes(_merged_counts(B.MATRICES["pair_raw2"]["names"]), stage_floats) == [(0, 1, True),
                                                                                                (1, 2, True)]


def test_boundary_rows_hold_the_special_values():
    X, _, _ = B.matrix("ladder")
    for f in range(X.shape[1]):
        col = X[:, f]
        for v in (B.FLT_MAX, -B.FLT_MAX, B.DENORM_MIN, -B.DENORM_MIN):
            assert (col == v).any()
        assert ((col == 0) & ~np.signbit(col)).any() and ((col == 0) & np.signbit(col)).any()
        assert np.isfinite(col).all()
    Xn, _, _ = B.matrix("ladder_nan")
    assert np.isnan(Xn).any() and not np.isinf(Xn).any()


@pytest.mark.parametrize("key,name", [("ladder_nan", "ladder"), ("ladder_d3", "ladder_d3"), ("iforest", "iforest"),
                                      ("iforest_d3", "iforest_d3")])
def test_host_packing_on_boundary_rows(key, name):
    """the threshold layout (which holds sklearn's `(double)x <= thr` rewritten to `x < t_f32`) and the binned layout,
    walked row by row in Python, against the C oracle on boundary rows"""
    X, _, _ = B.matrix(key)
    fa, _ = B.model(name)
    xgb = B._is_xgb(fa)
    rows = np.random.default_rng(5).choice(len(X), 160, replace=False)
    Xs = np.ascontiguousarray(X[rows])
    _, sums, leaf = (oracle.xgb_predict if xgb else oracle.iforest_predict)(fa, Xs, want_leaf=True)
    blob, ids, info = pack_forest_host(fa)
    bblob, thr, off, binfo = pack_forest_binned_host(fa)
    for r in range(len(Xs)):
        s, lv = forest_ref.packed_walk(blob, ids, info, xgb, Xs[r])
        assert lv == list(leaf[r]), f"threshold layout, row {rows[r]}"
        bs, blv = forest_ref.packed_walk_binned(bblob, ids, thr, off, binfo, xgb, Xs[r])
        assert blv == list(leaf[r]), f"binned layout, row {rows[r]}"
        if xgb:
            assert np.float32(s) == sums[r] == np.float32(bs)
        else:
            assert s == sums[r] == bs
