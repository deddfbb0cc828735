"""CPU: the sparse (pointer) forest layout — fd_pack_forest_sparse_host — walked by a numpy walker written against
the layout's documentation (include/fdengine.h), and held to scikit-learn itself: RandomForestClassifier /
ExtraTreesClassifier apply() leaf ids exactly and predict_proba[:, 1] bit for bit (an in-order f64 sum of the leaf
values divided once by the tree count), on rows planted on the thresholds and one f32 step to either side, and on
rows with NaN. Then the shapes a heap cannot hold (a root that is a leaf, chains of depth 40), the refusals of
malformed trees, and the loader's refusals."""
import numpy as np
import pytest

import forest_sparse_cases as SC
from fdengine import UnsupportedModel, forest_from_sklearn_classifier, pack_forest_sparse_host
from fdengine import _native as N
from oracle import boundary_ref as B

pytestmark = pytest.mark.filterwarnings("ignore:invalid value encountered in reduce")

LEAF = np.uint32(1 << 31)


def sparse_walk(nodes, leaf_val, leaf_ids, info, X):
    """The documented walk over the packed image. nodes: [n_nodes, 2] u32 {f32 threshold bits, meta}; tree t starts
    at record t. Internal: go left <=> x < t (f32); NaN and columns beyond the row's width follow default_left
    (bit 30); child = meta & 0xFFFFFF is the left child's record, + 1 the right; feature = meta >> 24 & 63. Leaf (bit
    31): ordinal = meta & 0x7FFFFFFF indexes leaf_val / leaf_ids. -> (leaf ids [n, T], sums in tree order: f32 from
    the base margin for XGBoost, f64 from 0 for the sklearn kinds)"""
    X = np.asarray(X, np.float32)
    n, T = len(X), info.n_trees
    thr = nodes[:, 0].copy().view(np.float32)
    meta = nodes[:, 1]
    xgb = info.kind == N.FD_FOREST_XGB_BINARY_LOGISTIC
    acc = np.full(n, np.float32(info.base_margin), np.float32) if xgb else np.zeros(n, np.float64)
    leaves = np.empty((n, T), np.int32)
    for t in range(T):
        cur = np.full(n, t, np.int64)
        idx = np.arange(n)
        while True:
            idx = idx[(meta[cur[idx]] & LEAF) == 0]
            if len(idx) == 0:
                break
            m = meta[cur[idx]]
            f = ((m >> np.uint32(24)) & np.uint32(63)).astype(np.int64)
            x = np.where(f < X.shape[1], X[idx, np.minimum(f, X.shape[1] - 1)], np.float32(np.nan))
            left = np.where(np.isnan(x), (m >> np.uint32(30)) & np.uint32(1) != 0, x < thr[cur[idx]])
            cur[idx] = (m & np.uint32(0xFFFFFF)).astype(np.int64) + np.where(left, 0, 1)
        o = (meta[cur] & ~LEAF).astype(np.int64)
        leaves[:, t] = leaf_ids[o]
        acc = (acc + leaf_val[o]).astype(np.float32) if xgb else acc + leaf_val[o]
    return leaves, acc


@pytest.mark.parametrize("name", ["rf", "et"])
@pytest.mark.parametrize("kind", ["boundary", "nan"])
def test_packed_walk_reproduces_sklearn(name, kind):
    fa, m = SC.classifier(name)
    X = SC.rows(name, kind)
    leaf, proba, raw = SC.sklearn_answers(name, kind)
    nodes, vals, ids, info = pack_forest_sparse_host(fa)
    depths = [est.tree_.max_depth for est in m.estimators_]
    assert info.kind == N.FD_FOREST_SKLEARN_PROBA and info.n_trees == len(m.estimators_) and info.leaf_bytes == 8
    assert info.depth == max(depths) > 10, "the forests of this test must be deeper than the heap layouts reach"
    assert info.n_nodes == sum(est.tree_.node_count for est in m.estimators_)
    assert info.n_leaves == sum(int((est.tree_.children_left == -1).sum()) for est in m.estimators_)
    if kind == "nan":
        assert np.isnan(X).mean() > 0.03
    else:  # the rows hold thresholds and both neighbours (every one when the column has room for all its candidates)
        t = B.feature_thresholds(fa)
        met = np.mean([np.isin(tf, X[:, f]).mean() for f, tf in enumerate(t) if len(tf)])
        assert met > 0.5, met
    got_leaf, got_raw = sparse_walk(nodes, vals, ids, info, X)
    np.testing.assert_array_equal(got_leaf, leaf)            # apply()
    np.testing.assert_array_equal(got_raw, raw)              # the in-order sum
    np.testing.assert_array_equal(got_raw / info.n_trees, proba)  # predict_proba[:, 1], bit for bit


def test_children_are_adjacent_and_roots_come_first():
    fa, _ = SC.classifier("rf")
    nodes, vals, ids, info = pack_forest_sparse_host(fa)
    meta = nodes[:, 1]
    internal = (meta & LEAF) == 0
    child = (meta[internal] & np.uint32(0xFFFFFF)).astype(np.int64)
    assert child.min() >= info.n_trees and child.max() + 1 < info.n_nodes
    both = np.sort(np.concatenate([child, child + 1]))  # every non-root record is the child of exactly one node
    np.testing.assert_array_equal(both, np.arange(info.n_trees, info.n_nodes))
    ords = np.sort((meta[~internal] & ~LEAF).astype(np.int64))
    np.testing.assert_array_equal(ords, np.arange(info.n_leaves))


@pytest.mark.parametrize("kind", [N.FD_FOREST_XGB_BINARY_LOGISTIC, N.FD_FOREST_SKLEARN_IFOREST,
                                  N.FD_FOREST_SKLEARN_PROBA])
def test_hand_built_forest_packs_and_walks(kind):
    fa = SC.hand_forest(kind)
    X = SC.hand_rows(600)
    nodes, vals, ids, info = pack_forest_sparse_host(fa)
    assert info.depth == SC.CHAIN and info.n_trees == 4
    assert info.n_nodes == len(fa.left) and info.n_leaves == int((fa.left == -1).sum())
    assert nodes[0, 1] & LEAF, "tree 0's root is a leaf record"
    assert vals.dtype == (np.float32 if kind == N.FD_FOREST_XGB_BINARY_LOGISTIC else np.float64)
    ref_leaf, ref_sum = SC.hand_reference(fa, X)
    assert (ref_leaf[:, 2] == 2 * SC.CHAIN).any() and (ref_leaf[:, 3] == 2 * SC.CHAIN).any(), "rows reach depth 40"
    got_leaf, got_sum = sparse_walk(nodes, vals, ids, info, X)
    np.testing.assert_array_equal(got_leaf, ref_leaf)
    np.testing.assert_array_equal(got_sum, ref_sum)
    # short rows: the columns beyond are missing (default direction)
    got_leaf, got_sum = sparse_walk(nodes, vals, ids, info, X[:, :4])
    ref_leaf, ref_sum = SC.hand_reference(fa, X[:, :4])
    np.testing.assert_array_equal(got_leaf, ref_leaf)
    np.testing.assert_array_equal(got_sum, ref_sum)


def test_malformed_trees_are_refused():
    fa = SC.hand_forest(N.FD_FOREST_SKLEARN_PROBA)
    a = int(fa.offsets[2])
    cyc = SC.hand_forest(N.FD_FOREST_SKLEARN_PROBA)
    cyc.left[a + 4] = 0  # the left chain's third node points back at the root
    with pytest.raises(N.NativeError) as ei:
        pack_forest_sparse_host(cyc)
    assert ei.value.code == N.FD_ERR_INVALID_ARG and "twice" in str(ei.value)
    oob = SC.hand_forest(N.FD_FOREST_SKLEARN_PROBA)
    oob.right[a + 6] = int(fa.offsets[3] - fa.offsets[2])  # one past the tree's last node
    with pytest.raises(N.NativeError) as ei:
        pack_forest_sparse_host(oob)
    assert ei.value.code == N.FD_ERR_INVALID_ARG and "out of range" in str(ei.value)
    wide = SC.hand_forest(N.FD_FOREST_SKLEARN_PROBA)
    wide.num_feature = 65
    with pytest.raises(N.NativeError) as ei:
        pack_forest_sparse_host(wide)
    assert ei.value.code == N.FD_ERR_UNSUPPORTED and "64" in str(ei.value)


def test_loader_refusals():
    from sklearn.ensemble import GradientBoostingClassifier, RandomForestClassifier
    from sklearn.tree import DecisionTreeClassifier
    X = SC.train_matrix()[:400]
    y2 = (X[:, 1] > 1.0).astype(int)
    y3 = (X[:, 1] > 1.0).astype(int) + (X[:, 3] > 0.3).astype(int)
    with pytest.raises(UnsupportedModel, match="RandomForestClassifier.*3 classes"):
        forest_from_sklearn_classifier(RandomForestClassifier(n_estimators=3, random_state=0).fit(X, y3))
    with pytest.raises(UnsupportedModel, match="RandomForestClassifier.*2 outputs"):
        forest_from_sklearn_classifier(RandomForestClassifier(n_estimators=3, random_state=0)
                                       .fit(X, np.stack([y2, 1 - y2], axis=1)))
    with pytest.raises(UnsupportedModel, match="GradientBoostingClassifier"):
        forest_from_sklearn_classifier(GradientBoostingClassifier(n_estimators=3, random_state=0).fit(X, y2))
    one = forest_from_sklearn_classifier(DecisionTreeClassifier(random_state=0).fit(X, y2))
    assert one.n_trees == 1 and one.kind == N.FD_FOREST_SKLEARN_PROBA


def test_heap_packers_still_refuse_deep_trees():
    from fdengine import pack_forest_host
    with pytest.raises(N.NativeError) as ei:
        pack_forest_host(SC.hand_forest(N.FD_FOREST_XGB_BINARY_LOGISTIC))
    assert ei.value.code == N.FD_ERR_UNSUPPORTED
