"""ORACLE — TEST INFRASTRUCTURE ONLY. Boundary-valued forests and rows, and a plain numpy walk.

Every scoring path bins a feature value as #{thresholds <= x} and compares bins; the places where such code goes wrong
(`<` against `<=`, first / last table entry, counts at and beside powers of two, an empty table, adjacent thresholds
one ulp apart, 0.0 / -0.0, denormals) are hit only when a row holds a threshold's exact value or its f32 neighbour.
This module builds models and rows that do, and the reference they are held to:

  ladder_xgboost_doc          an XGBoost JSON document whose features have prescribed distinct-threshold counts
  rewrite_iforest_thresholds  hand-placed f64 thresholds in a fitted sklearn IsolationForest (sklearn stays the reference)
  boundary_rows               rows made of every threshold, its f32 neighbours and the special values
  walk_reference              vectorised numpy walk of the original arrays (shares no code with oracle_forest.c /
                              forest_ref.py); `compare` swaps in a wrong comparison to measure what the rows detect
"""
from __future__ import annotations

import numpy as np

F32 = np.float32
FLT_MAX = np.finfo(np.float32).max
DENORM_MIN = np.float32(1e-45)  # 2^-149, the smallest positive f32
_INF = np.float32(np.inf)

# distinct thresholds per feature: 0 (a feature no split uses), 1, counts at and beside the powers of two the binary
# lifting starts from, 31 / 32 / 33 (one pad word per 32 table entries), 255 / 256 / 257. 18 features: no multiple of
# 4 (the lockstep search's group) nor of 16 (a thread's share of the row). Neighbours in a group of four differ widely
# in count, so the shared step count is some other feature's.
DEFAULT_LADDER = (33, 0, 257, 1, 64, 2, 31, 3, 256, 4, 65, 5, 255, 7, 32, 8, 63, 9)


def up32(v):
    return np.nextafter(np.asarray(v, F32), _INF)


def down32(v):
    return np.nextafter(np.asarray(v, F32), -_INF)


def floor32(thr) -> np.ndarray:
    """largest f32 <= the f64 value(s): (double)x <= thr  <=>  x <= floor32(thr) for every f32 x"""
    thr = np.asarray(thr, np.float64)
    with np.errstate(over="ignore"):
        t = thr.astype(F32)
    return np.where(t.astype(np.float64) > thr, down32(t), t).astype(F32)


def _is_xgb(fa) -> bool:
    from fdengine import _native as N
    return fa.kind == N.FD_FOREST_XGB_BINARY_LOGISTIC


def threshold_set(k: int, rng, rot: int = 0) -> np.ndarray:
    """k distinct finite f32 thresholds, ascending: 0.0, a run t / next-up / next-up again, one denormal, one value above
    2^24, a negative and a positive value first (as many of them as k allows, starting at kind `rot`), the rest further
    runs of consecutive floats and scattered values of both signs."""
    if k == 0:
        return np.zeros(0, F32)
    t = F32(rng.normal() * 10.0 ** int(rng.integers(-2, 3)))
    run = [t, up32(t), up32(up32(t))]
    kinds = [[F32(0.0)], run, [F32(DENORM_MIN * F32(int(rng.integers(1, 9))) * F32(rng.choice([-1.0, 1.0])))],
             [F32(2.0 ** 24 + 2.0 * int(rng.integers(1, 1000)))], [F32(-abs(rng.normal()) - 0.5)],
             [F32(abs(rng.normal()) + 0.5)]]
    kinds = kinds[rot % len(kinds):] + kinds[:rot % len(kinds)]
    got = {}

    def add(v):
        v = F32(v)
        if np.isfinite(v) and abs(v) < F32(1e30) and len(got) < k and not (v == 0 and np.signbit(v)):
            got.setdefault(v.view(np.uint32).item(), v)

    for kind in kinds:
        for v in kind:
            add(v)
    while len(got) < k:
        v = F32(rng.normal() * 10.0 ** int(rng.integers(-3, 4)))
        add(v)
        if rng.random() < 0.3:  # another run of consecutive floats
            add(up32(v))
            add(up32(up32(v)))
    out = np.sort(np.array(list(got.values()), F32))
    assert len(out) == k and np.all(np.diff(out) > 0)
    return out


def ladder_xgboost_doc(sizes=DEFAULT_LADDER, depth: int = 8, n_trees: int = 40, seed: int = 0, p_leaf: float = 0.0,
                       base_score: float = 0.5, small_first: bool = False):
    """-> (XGBoost JSON document, [per-feature ascending f32 thresholds]). synth.xgboost_doc's trees with every
    internal node's (split_index, split_condition) reassigned from the prescribed sets, cycling over a shuffled list
    of all (feature, threshold) pairs so that every pair is used at least once. small_first: the pairs of the features
    with the fewest thresholds go to the shallowest nodes (a ladder with very large tables: a row holds one given
    threshold of such a table with a chance of one in tens of thousands, so its nodes detect little wherever they sit,
    while the small tables' nodes near the roots are visited by rows that hold their thresholds)."""
    from fdengine import synth
    nf = len(sizes)
    assert nf % 4 != 0 and nf % 16 != 0, "the feature count must cut the lockstep group and the thread's share"
    rng = np.random.Generator(np.random.PCG64(seed))
    sets = [threshold_set(int(k), rng, rot=f) for f, k in enumerate(sizes)]
    doc = synth.xgboost_doc(n_trees, depth, nf, rng.normal(size=(64, nf)).astype(F32), seed=seed + 1, p_leaf=p_leaf,
                            base_score=base_score, max_bin=None)
    trees = doc["learner"]["gradient_booster"]["model"]["trees"]
    pairs = [(f, float(t)) for f in range(nf) for t in sets[f]]
    nodes = [(ti, i) for ti, tr in enumerate(trees) for i, l in enumerate(tr["left_children"]) if l != -1]
    assert len(nodes) >= len(pairs), f"{len(nodes)} internal nodes cannot hold {len(pairs)} (feature, threshold) pairs"
    pair_order = rng.permutation(len(pairs))
    node_order = rng.permutation(len(nodes))  # pairs land at every depth
    if small_first:  # (synth.xgboost_doc numbers a tree's nodes breadth-first: a lower index is no deeper)
        pair_order = np.array(sorted(pair_order, key=lambda j: sizes[pairs[j][0]]))
        node_order = np.array(sorted(node_order, key=lambda ni: nodes[ni][1]))
    used = set()
    for j, ni in enumerate(node_order):
        ti, i = nodes[ni]
        f, t = pairs[pair_order[j % len(pairs)]]
        trees[ti]["split_indices"][i] = f
        trees[ti]["split_conditions"][i] = t
        used.add((f, t))
    assert used == set(pairs)
    return doc, sets


def rewrite_iforest_thresholds(model, X, seed: int = 0, pool=None):
    """Overwrite tree_.threshold of every internal node of a fitted sklearn IsolationForest, in place, with an f64 value
    at or beside an f32 value v the data holds in that node's column: (double)v, its f64 next-up, its f64 next-down, or
    the midpoint of v and its f32 next-up; exactly 0.0 for a share of the nodes whose column holds zeros. The structure
    is untouched: sklearn's apply / decision_function honour the new values and stay the reference. pool: draw v from
    at most this many distinct values per column (so thresholds of different nodes coincide and neighbour)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    X = np.ascontiguousarray(X, F32)
    cols = []
    for f in range(X.shape[1]):
        u = np.unique(X[:, f][np.abs(X[:, f]) < FLT_MAX])  # finite, and with finite f32 neighbours
        if pool is not None and len(u) > pool:
            u = np.sort(rng.choice(u, pool, replace=False))
        cols.append(u)
    for est, feats in zip(model.estimators_, model.estimators_features_):
        tr = est.tree_
        thr = tr.threshold  # a writable view of the tree's node array
        for node in np.nonzero(tr.children_left != -1)[0]:
            u = cols[int(feats[tr.feature[node]])]
            v = F32(u[rng.integers(0, len(u))])
            how = int(rng.integers(0, 4))
            d = np.float64(v)
            if (u == 0).any() and rng.random() < 0.2:
                new = 0.0
            elif how == 0:
                new = d
            elif how == 1:
                new = np.nextafter(d, np.inf)
            elif how == 2:
                new = np.nextafter(d, -np.inf)
            else:
                new = 0.5 * d + 0.5 * np.float64(up32(v))  # strictly between v and its f32 next-up, exact in f64
                assert d < new < np.float64(up32(v))
            thr[node] = new
        assert np.shares_memory(thr, tr.threshold)
    return model


def node_depths(fa) -> np.ndarray:
    """depth of every node (both model formats number a child after its parent)"""
    d = np.zeros(len(fa.left), np.int32)
    for t in range(fa.n_trees):
        a = int(fa.offsets[t])
        for i in range(a, int(fa.offsets[t + 1])):
            if fa.left[i] != -1:
                d[a + fa.left[i]] = d[a + fa.right[i]] = d[i] + 1
    return d


def feature_thresholds(fa, max_depth=None):
    """per feature, the ascending distinct f32 values a row must meet: XGBoost (float)split_condition; sklearn
    floor32(threshold). max_depth: of the nodes no deeper than this only."""
    internal = fa.left != -1
    if max_depth is not None:
        internal &= node_depths(fa) <= max_depth
    t = fa.threshold[internal]
    t32 = t.astype(F32) if _is_xgb(fa) else floor32(t)
    f = fa.feature[internal]
    return [np.unique(t32[f == j]) for j in range(fa.num_feature)]


def candidates(thr32: np.ndarray) -> np.ndarray:
    """the values of one feature's column: every threshold, its f32 next-up and next-down, one value below the minimum
    and one above the maximum, +-0.0, +-FLT_MAX, +- the smallest denormal (no +-inf: DMatrix and sklearn refuse it)"""
    spec = [F32(0.0), F32(-0.0), FLT_MAX, -FLT_MAX, DENORM_MIN, -DENORM_MIN]
    if len(thr32) == 0:
        return np.array(spec + [F32(-1.5), F32(2.5)], F32)
    lo, hi = thr32.min(), thr32.max()
    edge = [F32(lo - abs(lo) - F32(1.0)), F32(hi + abs(hi) + F32(1.0))]
    c = np.concatenate([thr32, up32(thr32), down32(thr32), np.array(edge + spec, F32)]).astype(F32)
    return c[np.isfinite(c)]


def boundary_rows(fa, n_rows: int, seed: int = 0, nan_frac: float = 0.0, max_depth=None,
                  shares=None) -> np.ndarray:
    """[n_rows, num_feature] f32: candidate i of feature f in row i mod n_rows (a column with fewer candidates than rows
    repeats them), each column then permuted, so every candidate of every feature occurs when n_rows >= the largest
    candidate count. A column with more candidates than rows keeps the first and the last table entry and a seeded
    sample of the others, each with both neighbours, and the special values. nan_frac: that share of each column,
    taken from the repeats only, becomes NaN. fa: one forest, or several over the same features (a scored pair: the
    union of their thresholds). max_depth (one per forest, None = all): only the thresholds of that forest's nodes no
    deeper than this, and the first and last entry of each of its tables — for tables with more entries than any
    matrix has rows, so that rows meet the thresholds of the nodes most of them visit. shares (one per forest): give
    each forest's candidates that share of the rows instead of one row per candidate of the union, so that a forest
    with few thresholds is met as often as one with many."""
    rng = np.random.Generator(np.random.PCG64(seed))
    forests = list(fa) if isinstance(fa, (list, tuple)) else [fa]
    nf = forests[0].num_feature
    assert all(m.num_feature == nf for m in forests)
    md = list(max_depth) if isinstance(max_depth, (list, tuple)) else [max_depth] * len(forests)
    tables = []
    for m, d in zip(forests, md):
        tb = feature_thresholds(m)
        if d is not None:
            tb = [np.unique(np.concatenate([s_, a_[:1], a_[-1:]])) for s_, a_ in zip(feature_thresholds(m, d), tb)]
        tables.append(tb)
    X = np.empty((n_rows, nf), F32)
    if shares is None:
        parts = [(list(range(len(forests))), n_rows)]
    else:  # each forest's candidates in a share of the rows of their own
        assert len(shares) == len(forests) and nan_frac == 0.0
        cut = [int(round(n_rows * sum(shares[:k]) / sum(shares))) for k in range(len(forests) + 1)]
        parts = [([k], cut[k + 1] - cut[k]) for k in range(len(forests))]
    for f in range(nf):
        col = np.concatenate([_column(np.unique(np.concatenate([tables[k][f] for k in ks])), rows, rng, nan_frac)
                              for ks, rows in parts])
        X[:, f] = col[rng.permutation(n_rows)]
    return X


def _column(t, n_rows, rng, nan_frac):
    c = candidates(t)
    col = np.empty(n_rows, F32)
    if len(c) > n_rows:
        keep = (n_rows - 8) // 3
        mid = 1 + rng.choice(len(t) - 2, keep - 2, replace=False)
        c = candidates(np.sort(np.concatenate([t[:1], t[mid], t[-1:]])))
    if len(c) >= n_rows:
        col[:] = c[:n_rows]
    else:
        col[:] = np.resize(c, n_rows)
        k = min(n_rows - len(c), int(round(nan_frac * n_rows)))
        if k > 0:
            col[len(c) + rng.choice(n_rows - len(c), k, replace=False)] = np.nan
    return col


def covers(fa, X, max_depth=None) -> bool:
    """every (feature, threshold) of the model (of its nodes no deeper than max_depth) is met by a row holding the
    threshold, its next-up and its next-down"""
    for f, t in enumerate(feature_thresholds(fa, max_depth)):
        col = X[:, f] if f < X.shape[1] else np.zeros(0, F32)
        if not (np.isin(t, col).all() and np.isin(up32(t), col).all() and np.isin(down32(t), col).all()):
            return False
    return True


def xgb_base_margin(base_score: float) -> np.float32:
    """ProbToMargin of binary:logistic in f32: -log(1 / p - 1)"""
    p = F32(base_score)
    r = F32(F32(1.0) / p - F32(1.0))
    return F32(-F32(np.log(np.float64(r))))


def walk_reference(fa, X, compare=None):
    """-> (leaf ids int32 [n, T], sums). XGBoost: x < (float)thr in f32, NaN and columns beyond the row's width to
    default_left, f32 leaf weights summed in tree order from the f32 base margin (sums f32). sklearn: (double)x <= thr,
    f64 sums in estimator order. compare: None, or a wrong comparison — "le" (XGBoost `<=`), "lt" (sklearn `<` in f64),
    "lt_f32" / "le_f32" (sklearn against (float)thr)."""
    xgb = _is_xgb(fa)
    assert compare in ((None, "le") if xgb else (None, "lt", "lt_f32", "le_f32"))
    X = np.asarray(X, F32)
    n = X.shape[0]
    Xp = np.full((n, max(fa.num_feature, X.shape[1])), np.nan, F32)
    Xp[:, :X.shape[1]] = X
    T = fa.n_trees
    leaf = np.empty((n, T), np.int32)
    acc = np.full(n, xgb_base_margin(fa.base_score), F32) if xgb else np.zeros(n, np.float64)
    with np.errstate(over="ignore"):
        thr32 = fa.threshold.astype(F32)
    for t in range(T):
        a, b = int(fa.offsets[t]), int(fa.offsets[t + 1])
        L, R, Fe, DL = fa.left[a:b], fa.right[a:b], fa.feature[a:b], fa.default_left[a:b]
        t64, t32 = fa.threshold[a:b], thr32[a:b]
        node = np.zeros(n, np.int64)
        idx = np.arange(n)
        while True:
            idx = idx[L[node[idx]] != -1]
            if len(idx) == 0:
                break
            nd = node[idx]
            x = Xp[idx, Fe[nd]]
            if xgb:
                left = x < t32[nd] if compare is None else x <= t32[nd]
            elif compare is None:
                left = x.astype(np.float64) <= t64[nd]
            elif compare == "lt":
                left = x.astype(np.float64) < t64[nd]
            else:
                left = x < t32[nd] if compare == "lt_f32" else x <= t32[nd]
            left = np.where(np.isnan(x), DL[nd] != 0, left)
            node[idx] = np.where(left, L[nd], R[nd])
        leaf[:, t] = node
        lv = fa.leaf_value[a:b][node]
        acc = (acc + lv.astype(F32)).astype(F32) if xgb else acc + lv
    return leaf, acc


def changed_share(fa, X, compare) -> float:
    """share of the rows whose leaf-id vector changes under the wrong comparison"""
    good, _ = walk_reference(fa, X)
    bad, _ = walk_reference(fa, X, compare=compare)
    return float((good != bad).any(axis=1).mean())


# ------------------------------------------------------------------ the boundary models the tests share
SHALLOW_LADDER = (3, 0, 9, 1, 33, 2, 5)
# Features 0 .. 4 hold about 20 k thresholds and feature 5 another 9 k: see tests/test_gpu_forest_boundaries.py
# (the fused pair's binning passes must cut the group of four features 4 .. 7)
PASSCUT_LADDER = (8000, 8000, 4000, 33, 31, 9000) + DEFAULT_LADDER[1:]

_models = {}


def _iforest(X32, n_estimators, max_samples, seed, pool):
    from fdengine import iforest_from_sklearn, synth
    m = synth.isolation_forest(np.clip(X32, -1e6, 1e6).astype(np.float64), n_estimators=n_estimators,
                               max_samples=max_samples)
    rewrite_iforest_thresholds(m, X32, seed=seed, pool=pool)
    return iforest_from_sklearn(m), m


def model(name: str):
    """-> (ForestArrays, fitted sklearn model or None), built once per process:
    ladder / ladder_d3 / ladder_passcut  ladder XGBoost (depth 8 x 40 trees; depth 3; depth 8 x 128 trees with the
                                         large tables of PASSCUT_LADDER)
    hist                                 max_bin=256 XGBoost over synth.feature_matrix (50 features)
    iforest / iforest_d3                 rewritten IsolationForest, 30 estimators on 24 features / max_samples=8
    iforest_ladder                       rewritten IsolationForest over the ladder's boundary rows (its pair)
    iforest_passcut                      rewritten IsolationForest over ladder_passcut's boundary rows (its pair)
    raw2 / iforest_raw2                  two features, raw-valued thresholds from 60,000 samples (a table too large
                                         for LDS), and the IsolationForest scored with it"""
    if name in _models:
        return _models[name]
    from fdengine import synth, xgboost_from_json_doc
    if name == "ladder":
        out = xgboost_from_json_doc(ladder_xgboost_doc(seed=101)[0]), None
    elif name == "ladder_d3":
        out = xgboost_from_json_doc(ladder_xgboost_doc(SHALLOW_LADDER, depth=3, n_trees=20, seed=102,
                                                       base_score=0.4)[0]), None
    elif name == "ladder_passcut":
        out = xgboost_from_json_doc(ladder_xgboost_doc(PASSCUT_LADDER, depth=8, n_trees=128, seed=103,
                                                       base_score=0.3, small_first=True)[0]), None
    elif name == "hist":
        Xr = synth.feature_matrix(4096, 50, seed=104)
        out = xgboost_from_json_doc(synth.xgboost_doc(40, 8, 50, Xr, seed=105, p_leaf=0.1, base_score=0.3)), None
    elif name == "iforest":
        out = _iforest(synth.feature_matrix(2000, 24, seed=106), 30, "auto", 107, 96)
    elif name == "iforest_d3":
        out = _iforest(synth.feature_matrix(2000, 24, seed=108), 20, 8, 109, 96)
    elif name == "iforest_ladder":  # the ladder's partner in a scored pair: thresholds at and beside the ladder's own
        out = _iforest(boundary_rows(model("ladder")[0], 2048, seed=115), 30, "auto", 116, 40)
    elif name == "iforest_passcut":
        out = _iforest(boundary_rows(model("ladder_passcut")[0], 8192, seed=110), 20, "auto", 111, None)
    elif name == "raw2":
        Xr = np.random.default_rng(112).normal(size=(60000, 2)).astype(F32)
        out = xgboost_from_json_doc(synth.xgboost_doc(300, 8, 2, Xr, seed=113, max_bin=None)), None
    elif name == "iforest_raw2":
        Xr = np.random.default_rng(112).normal(size=(60000, 2)).astype(F32)
        out = _iforest(Xr[:8192], 80, "auto", 114, 16)
    else:
        raise KeyError(name)
    _models[name] = out
    return out


_cases = {}

N_SMALL = 1021         # four tiles of 256 less three rows: the tree-split (latency) path
N_FUSED = 32768 + 77   # 128 full tiles, the smallest batch the fused kernel takes, and a ragged one
# the boundary matrices of tests/test_gpu_forest_boundaries.py, by name: case() arguments. tests/
# test_forest_boundaries_cpu.py proves the coverage conditions of every one of them.
MATRICES = {
    "ladder": dict(names=("ladder",), n_rows=N_SMALL),
    "ladder_nan": dict(names=("ladder",), n_rows=N_SMALL, nan_frac=0.01),
    "ladder_d3": dict(names=("ladder_d3",), n_rows=N_SMALL),
    "hist": dict(names=("hist",), n_rows=N_SMALL, nan_frac=0.01),
    "iforest": dict(names=("iforest",), n_rows=N_SMALL),
    "iforest_d3": dict(names=("iforest_d3",), n_rows=N_SMALL),
    "ladder_fused": dict(names=("ladder",), n_rows=N_FUSED),
    "iforest_fused": dict(names=("iforest",), n_rows=N_FUSED),
    "pair_latency": dict(names=("ladder", "iforest_ladder"), n_rows=N_SMALL),
    "pair_passcut": dict(names=("ladder_passcut", "iforest_passcut"), n_rows=N_FUSED),
    # tables of 28 k entries and 32 k rows: the rows meet the root nodes' thresholds and each table's ends
    "pair_raw2": dict(names=("raw2", "iforest_raw2"), n_rows=N_FUSED, max_depth=(0, None), shares=(1, 1)),
}


def matrix(key: str):
    """-> (X, {model name: (leaf ids, sums)}, {model name: max_depth of the covered nodes})"""
    kw = MATRICES[key]
    md = kw.get("max_depth") or (None,) * len(kw["names"])
    return case(**kw) + (dict(zip(kw["names"], md)),)


def case(names, n_rows: int, nan_frac: float = 0.0, seed: int = 7, max_depth=None, shares=None):
    """-> (X, {name: (leaf ids, sums)}): boundary rows of the named model (or pair of models) and walk_reference of each
    on them, computed once per process and shared; callers must not write to them."""
    names = (names,) if isinstance(names, str) else tuple(names)
    key = (names, n_rows, nan_frac, seed, max_depth, shares)
    if key not in _cases:
        fas = [model(n)[0] for n in names]
        X = boundary_rows(fas, n_rows, seed=seed, nan_frac=nan_frac, max_depth=max_depth, shares=shares)
        X.setflags(write=False)
        _cases[key] = X, {n: walk_reference(fa, X) for n, fa in zip(names, fas)}
    return _cases[key]


def nudge_split_conditions(doc: dict, seed: int = 0, share: float = 0.6) -> dict:
    """Move `share` of an XGBoost document's split conditions, in place, to the f32 next-up or next-down of their value:
    for a model whose conditions are values of the very rows to be scored (rows that cannot be chosen, such as the
    feature kernel's vectors), so that rows lie on a threshold and one f32 step to either side of one."""
    rng = np.random.Generator(np.random.PCG64(seed))
    for tr in doc["learner"]["gradient_booster"]["model"]["trees"]:
        for i, l in enumerate(tr["left_children"]):
            if l != -1 and rng.random() < share:
                v = F32(tr["split_conditions"][i])
                tr["split_conditions"][i] = float(up32(v) if rng.random() < 0.5 else down32(v))
    return doc
