"""Forests and a plain-Python reader of the dense chunk layout (include/fdengine.h fd_dense_layout_host), shared by
test_dense_host.py (CPU) and test_gpu_ensemble_dense.py."""
import numpy as np

from fdengine import ForestArrays, _native as N, synth, xgboost_from_json_doc

VARYING = np.array([0, 1, 5, 6, 7, 14, 15, 16, 17, 19, 21, 23, 26, 27, 31, 32, 41, 42, 43, 44, 45, 46], np.int32)


def on_varying(fa):
    """every split moved to one of the 22 varying slots: nothing for the contraction to resolve"""
    fa.feature = VARYING[fa.feature % len(VARYING)]
    return fa


def concat(a, b):
    """the trees of a, then those of b (same kind)"""
    cat = lambda k: np.concatenate([getattr(a, k), getattr(b, k)])  # noqa: E731
    return ForestArrays(kind=a.kind, num_feature=a.num_feature,
                        offsets=np.concatenate([a.offsets, b.offsets[1:] + a.offsets[-1]]), left=cat("left"),
                        right=cat("right"), feature=cat("feature"), threshold=cat("threshold"),
                        default_left=cat("default_left"), leaf_value=cat("leaf_value"), base_score=a.base_score,
                        if_offset=a.if_offset, if_denominator=a.if_denominator)


def shallow200(X):
    """200 trees of depth <= 2: eight bundles hold far less than a chunk buffer, so the bundle cap ends a chunk"""
    return xgboost_from_json_doc(synth.xgboost_doc(200, 2, 64, X, seed=21, p_leaf=0.3))


def deep_then_shallow(X):
    """30 perfect depth-8 trees on varying slots only (2 KiB each: the byte cap ends their chunks), then 40 shallow"""
    deep = on_varying(xgboost_from_json_doc(synth.xgboost_doc(30, 8, 64, X, seed=22)))
    return concat(deep, xgboost_from_json_doc(synth.xgboost_doc(40, 2, 64, X, seed=23, p_leaf=0.3)))


def as_iforest(fa, seed):
    """the trees of an XGBoost-shaped forest as an IsolationForest (sklearn's comparison, f64 path-length leaves)"""
    rng = np.random.default_rng(seed)
    return ForestArrays(kind=N.FD_FOREST_SKLEARN_IFOREST, num_feature=64, offsets=fa.offsets, left=fa.left,
                        right=fa.right, feature=fa.feature, threshold=fa.threshold,
                        default_left=np.zeros_like(fa.default_left), leaf_value=rng.uniform(1.0, 9.0, len(fa.left)),
                        if_offset=-0.5, if_denominator=fa.n_trees * 10.24)


def chunk_table(lay, c):
    """chunk c's table as u32 words"""
    end = int(lay["chunk_offsets"][c]) + int(lay["chunk_lengths"][c])
    return lay["blob"][end - 1024:end].view(np.uint32)


def walk_blob(lay, xgb, X):
    """leaf value per (row, tree), read from the blob by the documented node word alone"""
    thr, off = lay["thresholds"], lay["thr_offsets"]
    bins = np.zeros((len(X), len(VARYING)), np.int64)  # #{t <= x} per varying slot; NaN: -1
    for s, f in enumerate(VARYING):
        col = X[:, f]
        bins[:, s] = np.where(np.isnan(col), -1, np.searchsorted(thr[off[f]:off[f + 1]], col, side="right"))
    out = np.empty((len(X), len(lay["trees"])))
    rows = np.arange(len(X))
    for t, info in enumerate(lay["trees"]):
        base, d = int(lay["chunk_offsets"][info["chunk"]]), int(info["depth"])
        w = lay["blob"][base + info["node_offset"]:base + info["node_offset"] + (4 << d)].view(np.uint32).astype(np.int64)
        s = np.ones(len(X), np.int64)
        for level in range(d):
            node = w[s]
            slot = ((node >> 10) & 63) * 2 + ((node >> 1) & 1)
            b = bins[rows, slot]
            right = np.where(b < 0, (node & 1) == 0, b > (node >> 16)).astype(np.int64)
            s = 2 * ((node >> 3) & 127) + right  # the next heap slot, or on the last level the leaf index
        lo = base + info["leaf_offset"]
        leaves = lay["blob"][lo:lo + ((4 if xgb else 8) << d)].view(np.float32 if xgb else np.float64)
        out[:, t] = leaves[s]
    return out
