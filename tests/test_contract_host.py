"""CPU: fd_contract_forest_host, the contraction of a forest against the constant slots of the compact scoring
vector (include/fdengine.h; csrc/ensemble_plan.hip contract_forest_host). The pipelined stream's compact and split rows
carry 22 varying slots; slots 12, 24, 25, 33 and 34 are always 0.5 and the other 37 always 0, so a split on one of
them sends every transaction the same way (left iff value < threshold in f32) and the fused kernel walks the forest
with those splits resolved. Here: hand-built trees at the comparison's edges and synth.xgboost_doc forests, the
contracted forest against the original on vectors whose constant slots hold those values — a plain Python walk over
the arrays, and the CPU oracle's f32 margins."""
import numpy as np
import pytest

import oracle
from fdengine import ForestArrays, _native as N, synth, xgboost_from_json_doc
from fdengine.engine import contract_forest_host

VARYING = [0, 1, 5, 6, 7, 14, 15, 16, 17, 19, 21, 23, 26, 27, 31, 32, 41, 42, 43, 44, 45, 46]
HALF = [12, 24, 25, 33, 34]
CONST = {f: (0.5 if f in HALF else 0.0) for f in range(64) if f not in VARYING}
assert len(CONST) == 42

F32 = np.float32
UP = lambda v: float(np.nextafter(F32(v), F32(np.inf)))    # noqa: E731
DOWN = lambda v: float(np.nextafter(F32(v), F32(-np.inf)))  # noqa: E731


def S(f, thr, left, right, dl=0):
    return ("split", f, thr, dl, left, right)


def forest(trees, kind=N.FD_FOREST_XGB_BINARY_LOGISTIC):
    """nested S(...) / leaf-value specs -> ForestArrays, nodes numbered breadth-first (XGBoost's order)"""
    offs, cols = [0], {k: [] for k in ("left", "right", "feature", "threshold", "default_left", "leaf_value")}
    for spec in trees:
        nodes, queue = [], [spec]
        while queue:  # breadth-first: children ids are known when the parent is written
            nodes.append(queue.pop(0))
            if isinstance(nodes[-1], tuple):
                queue += [nodes[-1][4], nodes[-1][5]]
        nxt = 1
        for nd in nodes:
            if isinstance(nd, tuple):
                row = (nxt, nxt + 1, nd[1], nd[2], nd[3], 0.0)
                nxt += 2
            else:
                row = (-1, -1, 0, 0.0, 0, float(nd))
            for k, v in zip(cols, row):
                cols[k].append(v)
        offs.append(len(cols["left"]))
    return ForestArrays(kind=kind, num_feature=64, offsets=np.array(offs, np.int64),
                        left=np.array(cols["left"], np.int32), right=np.array(cols["right"], np.int32),
                        feature=np.array(cols["feature"], np.int32), threshold=np.array(cols["threshold"], np.float64),
                        default_left=np.array(cols["default_left"], np.uint8),
                        leaf_value=np.array(cols["leaf_value"], np.float64), if_denominator=1.0)


def vectors(n, seed):
    X = synth.feature_matrix(n, 64, seed=seed)
    for f, v in CONST.items():
        X[:, f] = v
    return X


def walk(fa, X):
    """leaf value per (row, tree): left iff x < f32(threshold) (XGBoost) / (double)x <= threshold (sklearn)"""
    xgb = fa.kind == N.FD_FOREST_XGB_BINARY_LOGISTIC
    out = np.empty((len(X), fa.n_trees))
    for t in range(fa.n_trees):
        a = int(fa.offsets[t])
        L, R, Fe = fa.left[a:], fa.right[a:], fa.feature[a:]
        thr = fa.threshold[a:].astype(np.float32) if xgb else fa.threshold[a:]
        o, rows = np.zeros(len(X), np.int64), np.arange(len(X))
        while (L[o] >= 0).any():  # every row one level down (rows at a leaf stay)
            x = X[rows, Fe[o]]
            go_left = x < thr[o] if xgb else x.astype(np.float64) <= thr[o]
            o = np.where(L[o] >= 0, np.where(go_left, L[o], R[o]), o)
        out[:, t] = fa.leaf_value[a + o]
    return out


def depths_of(fa):
    out = []
    for t in range(fa.n_trees):
        a = int(fa.offsets[t])
        best, st = 0, [(0, 0)]
        while st:
            o, d = st.pop()
            if fa.left[a + o] < 0:
                best = max(best, d)
            else:
                st += [(int(fa.left[a + o]), d + 1), (int(fa.right[a + o]), d + 1)]
        out.append(max(best, 1))
    return out


def check(fa, n_rows=3000, seed=5):
    c, depth, pruned = contract_forest_host(fa)
    assert c.n_trees == fa.n_trees and list(depth) == depths_of(c)
    splits = c.left >= 0
    fully = [int(c.offsets[t + 1] - c.offsets[t]) == 3 and depth[t] == 1 and
             c.leaf_value[c.offsets[t] + 1] == c.leaf_value[c.offsets[t] + 2] for t in range(c.n_trees)]
    for t in range(c.n_trees):  # no remaining node tests a constant slot
        a, b = int(c.offsets[t]), int(c.offsets[t + 1])
        assert all(int(f) in VARYING for f in c.feature[a:b][splits[a:b]]), t
    assert pruned == int((fa.left >= 0).sum()) - int(splits.sum()) + sum(fully)
    X = vectors(n_rows, seed)
    np.testing.assert_array_equal(walk(c, X), walk(fa, X))
    if fa.kind == N.FD_FOREST_XGB_BINARY_LOGISTIC:
        p0, m0, _ = oracle.xgb_predict(fa, X)
        p1, m1, _ = oracle.xgb_predict(c, X)
    else:
        p0, m0, _ = oracle.iforest_predict(fa, X)
        p1, m1, _ = oracle.iforest_predict(c, X)
    np.testing.assert_array_equal(m1, m0)
    np.testing.assert_array_equal(p1, p0)
    return c, list(depth), pruned


def test_root_on_a_constant_slot():
    sub_l = S(0, 1.0, S(5, 3.0, 1.0, 2.0), 3.0)  # depth 2
    sub_r = S(1, 1.0, 4.0, 5.0)                   # depth 1
    fa = forest([S(12, 0.7, sub_l, sub_r), S(12, 0.3, sub_l, sub_r), S(2, 0.1, sub_l, sub_r), S(2, -0.1, sub_l, sub_r)])
    c, depth, pruned = check(fa)
    assert depth == [2, 1, 2, 1]  # 0.5 < 0.7 left; 0.5 < 0.3 no: right; 0 < 0.1 left; 0 < -0.1 no: right
    assert pruned == 2 + 3 + 2 + 3  # the root and the subtree that went with it


def test_whole_tree_on_constant_slots():
    fa = forest([S(12, 0.6, S(2, 0.5, 1.0, 2.0), S(3, 0.5, 3.0, 4.0)),   # left, then 0 < 0.5: left -> 1.0
                 S(24, 0.5, 5.0, S(33, UP(0.5), 6.0, 7.0)),              # right (0.5 < 0.5 no), then left -> 6.0
                 S(0, 1.0, 8.0, 9.0)])
    c, depth, pruned = check(fa)
    assert depth == [1, 1, 1] and pruned == 3 + 2
    for t, v in ((0, 1.0), (1, 6.0)):
        a = int(c.offsets[t])
        assert c.offsets[t + 1] - a == 3 and c.left[a] == 1 and c.right[a] == 2
        assert c.leaf_value[a + 1] == v and c.leaf_value[a + 2] == v


def test_chain_of_constants_above_a_varying_node():
    vary = S(14, 2.0, S(15, 1.0, 1.0, 2.0), 3.0)
    fa = forest([S(3, 0.25, S(25, 0.75, S(4, 1.0, vary, 7.0), 8.0), 9.0),     # three constants, all left
                 S(0, 1.0, S(8, 0.5, S(9, -1.0, 4.0, vary), 5.0), 6.0)])      # below a varying root: left, right
    c, depth, pruned = check(fa)
    assert depth == [2, 3] and pruned == 3 + 2
    a = int(c.offsets[1])
    assert c.feature[a] == 0 and c.feature[a + c.left[a]] == 14  # the varying node now hangs off the root


def test_no_constant_node_comes_back_unchanged():
    fa = xgboost_from_json_doc(synth.xgboost_doc(12, 5, 64, synth.feature_matrix(500, 64, seed=2), seed=4, p_leaf=0.3))
    fa.feature = np.array(VARYING, np.int32)[fa.feature % len(VARYING)]
    c, depth, pruned = check(fa, n_rows=500)
    assert pruned == 0 and depth == depths_of(fa)
    for k in ("offsets", "left", "right", "feature", "threshold", "default_left", "leaf_value"):
        np.testing.assert_array_equal(getattr(c, k), getattr(fa, k))
    lone = forest([0.25, S(0, 1.0, 1.0, 2.0)])  # a tree that is one leaf stays one (walked as one pad level)
    c, depth, pruned = check(lone, n_rows=50)
    assert depth == [1, 1] and pruned == 0 and list(c.offsets) == [0, 1, 4]


@pytest.mark.parametrize("slot,value", [(12, 0.5), (2, 0.0)])
@pytest.mark.parametrize("dl", [0, 1])
def test_threshold_edges(slot, value, dl):
    """value < threshold in f32: a threshold equal to the constant goes right, the next f32 above it left, the one
    below right; default_left (the NaN direction) plays no part"""
    fa = forest([S(slot, value, 1.0, 2.0, dl), S(slot, UP(value), 1.0, 2.0, dl), S(slot, DOWN(value), 1.0, 2.0, dl),
                 S(slot, -0.0 if value == 0.0 else 0.5, 1.0, 2.0, dl)])
    c, depth, pruned = check(fa, n_rows=20)
    assert depth == [1, 1, 1, 1] and pruned == 4
    assert [float(c.leaf_value[int(a) + 1]) for a in c.offsets[:-1]] == [2.0, 1.0, 2.0, 2.0]


def test_sklearn_comparison():
    """IsolationForest kind: (double)x <= threshold goes left — at the constant itself left, just below it right"""
    below = float(np.nextafter(0.5, 0.0))  # f64 neighbours: between two f32 values
    fa = forest([S(12, 0.5, 1.0, 2.0), S(12, below, 1.0, 2.0), S(2, 0.0, 1.0, 2.0), S(2, -1e-300, 1.0, 2.0),
                 S(0, 1.5, S(34, 0.49999, 3.0, S(1, 0.5, 4.0, 5.0)), 6.0)], kind=N.FD_FOREST_SKLEARN_IFOREST)
    c, depth, pruned = check(fa, n_rows=200)
    assert depth == [1, 1, 1, 1, 2] and pruned == 5
    assert [float(c.leaf_value[int(a) + 1]) for a in c.offsets[:4]] == [1.0, 2.0, 1.0, 2.0]


@pytest.mark.parametrize("p_leaf", [0.0, 0.3])
@pytest.mark.parametrize("depth", [3, 8])
def test_synthetic_forests(p_leaf, depth):
    """split features uniform over the 64 slots, thresholds from cuts of vectors whose constant slots hold their
    values (a threshold equal to the constant: right), as the benchmark's model is drawn"""
    Xr = vectors(2000, 9)
    fa = xgboost_from_json_doc(synth.xgboost_doc(40, depth, 64, Xr, seed=6, p_leaf=p_leaf))
    c, d, pruned = check(fa, n_rows=3000)
    assert pruned > 0 and max(d) <= depth and sum(d) < 40 * depth
    # and with thresholds off the constants' values (raw draws of a generic matrix): both directions occur
    fb = xgboost_from_json_doc(synth.xgboost_doc(40, depth, 64, synth.feature_matrix(2000, 64, seed=3), seed=7,
                                                 p_leaf=p_leaf, max_bin=None))
    check(fb, n_rows=3000)
