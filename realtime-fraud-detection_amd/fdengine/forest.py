"""Model-file formats on the path, read unchanged, flattened to the engine's original-tree arrays.

* XGBoost 2.0.3 JSON (`XGBClassifier.save_model(".../xgboost/fraud_classifier.json")`,
  reference ml/training/model_trainer.py:95-108; loaded by ml/models/model_manager.py:157-161).
  Schema: learner.gradient_booster.model.trees[i].{left_children, right_children, split_indices,
  split_conditions, default_left, split_type}; a node is a leaf when left_children[i] == -1 and its
  leaf weight is split_conditions[i]; learner.learner_model_param.{base_score, num_feature,
  num_class}; learner.objective.name.
* scikit-learn IsolationForest pickled with joblib (ml/training/model_trainer.py:246-266; loaded by
  ml/models/model_manager.py:197-200). The host unpickles it with sklearn exactly as the reference
  does, then passes tree_.{children_left, children_right, feature, threshold, missing_go_to_left}
  and the per-node path-length terms sklearn itself adds in `_compute_score_samples`.
"""
from __future__ import annotations

import json
from dataclasses import dataclass, field
from typing import Any, Dict, List, Optional

import numpy as np

from . import _native as N


class UnsupportedModel(ValueError):
    pass


@dataclass
class ForestArrays:
    """Original trees, concatenated (CSR by `offsets`). Mirrors fd_tree_arrays."""
    kind: int
    num_feature: int
    offsets: np.ndarray          # int64 [T+1]
    left: np.ndarray             # int32
    right: np.ndarray            # int32
    feature: np.ndarray          # int32
    threshold: np.ndarray        # float64
    default_left: np.ndarray     # uint8
    leaf_value: np.ndarray       # float64
    base_score: float = 0.5
    if_offset: float = 0.0
    if_denominator: float = 0.0
    meta: Dict[str, Any] = field(default_factory=dict)
    # float64, one per node: the weight the tree was grown with at that node (XGBoost sum_hessian, sklearn
    # weighted_n_node_samples). TreeSHAP splits by cover[child] / cover[node]; None: the model carries none
    cover: Optional[np.ndarray] = None

    @property
    def n_trees(self) -> int:
        return len(self.offsets) - 1

    def c_structs(self):
        """(fd_forest_params, fd_tree_arrays, keepalive) for the C-ABI."""
        arrs = dict(
            offsets=np.ascontiguousarray(self.offsets, dtype=np.int64),
            left=np.ascontiguousarray(self.left, dtype=np.int32),
            right=np.ascontiguousarray(self.right, dtype=np.int32),
            feature=np.ascontiguousarray(self.feature, dtype=np.int32),
            threshold=np.ascontiguousarray(self.threshold, dtype=np.float64),
            default_left=np.ascontiguousarray(self.default_left, dtype=np.uint8),
            leaf_value=np.ascontiguousarray(self.leaf_value, dtype=np.float64),
        )
        import ctypes as C

        def P(a, t):
            return a.ctypes.data_as(C.POINTER(t))

        t = N.fd_tree_arrays(
            self.n_trees, P(arrs["offsets"], C.c_int64), P(arrs["left"], C.c_int32), P(arrs["right"], C.c_int32),
            P(arrs["feature"], C.c_int32), P(arrs["threshold"], C.c_double), P(arrs["default_left"], C.c_uint8),
            P(arrs["leaf_value"], C.c_double))
        p = N.fd_forest_params(self.kind, self.num_feature, float(self.base_score), float(self.if_offset),
                               float(self.if_denominator))
        return p, t, arrs


def truncate_forest(fa: ForestArrays, n_trees: int) -> ForestArrays:
    """The first n_trees trees of a forest, with the per-node arrays of fit_gbdt's meta cut alike."""
    end = int(fa.offsets[n_trees])
    meta = dict(fa.meta, n_trees=n_trees)
    for k in ("sum_hessian", "loss_changes", "base_weights"):
        if k in meta:
            meta[k] = np.asarray(meta[k])[:end].copy()
    return ForestArrays(kind=fa.kind, num_feature=fa.num_feature, offsets=fa.offsets[:n_trees + 1].copy(),
                        left=fa.left[:end].copy(), right=fa.right[:end].copy(), feature=fa.feature[:end].copy(),
                        threshold=fa.threshold[:end].copy(), default_left=fa.default_left[:end].copy(),
                        leaf_value=fa.leaf_value[:end].copy(), base_score=fa.base_score, meta=meta,
                        cover=None if fa.cover is None else meta.get("sum_hessian", fa.cover[:end].copy()))


def _concat(trees: List[Dict[str, np.ndarray]], kind: int, num_feature: int, **kw) -> ForestArrays:
    sizes = [len(t["left"]) for t in trees]
    offsets = np.zeros(len(trees) + 1, dtype=np.int64)
    offsets[1:] = np.cumsum(sizes)

    def cat(k, dt):
        return np.concatenate([np.asarray(t[k], dtype=dt) for t in trees]) if trees else np.zeros(0, dt)

    return ForestArrays(kind=kind, num_feature=num_feature, offsets=offsets, left=cat("left", np.int32),
                        right=cat("right", np.int32), feature=cat("feature", np.int32),
                        threshold=cat("threshold", np.float64), default_left=cat("default_left", np.uint8),
                        leaf_value=cat("leaf_value", np.float64),
                        cover=cat("cover", np.float64) if trees and all("cover" in t for t in trees) else None, **kw)


# ----------------------------------------------------------------------------------------- XGBoost

def xgboost_from_json_doc(doc: Dict[str, Any]) -> ForestArrays:
    learner = doc["learner"]
    obj = learner.get("objective", {}).get("name")
    if obj != "binary:logistic":
        raise UnsupportedModel(f"objective {obj!r} not supported (binary:logistic only)")
    gb = learner["gradient_booster"]
    if gb.get("name") != "gbtree":
        raise UnsupportedModel(f"booster {gb.get('name')!r} not supported (gbtree only)")
    lmp = learner["learner_model_param"]
    if int(float(lmp.get("num_class", "0"))) > 1:
        raise UnsupportedModel("multi-class models are not supported")
    num_feature = int(float(lmp["num_feature"]))
    base_score = float(lmp["base_score"])
    model = gb["model"]
    trees = []
    for tr in model["trees"]:
        left = np.asarray(tr["left_children"], dtype=np.int64)
        st = tr.get("split_type")
        if st is not None and np.any(np.asarray(st) != 0):
            raise UnsupportedModel("categorical splits are not supported")
        tp = tr.get("tree_param", {})
        if int(float(tp.get("size_leaf_vector", "1"))) > 1:
            raise UnsupportedModel("vector leaves are not supported")
        leaf = left == -1
        cond = np.asarray(tr["split_conditions"], dtype=np.float64)
        feat = np.where(leaf, 0, np.asarray(tr["split_indices"], dtype=np.int64))
        sh = tr.get("sum_hessian")
        cover = {} if sh is None or len(sh) != len(left) else {"cover": np.asarray(sh, dtype=np.float64)}
        trees.append(dict(
            **cover, left=np.where(leaf, -1, left), right=np.asarray(tr["right_children"], dtype=np.int64),
            feature=feat, threshold=np.where(leaf, 0.0, cond),
            default_left=np.asarray(tr["default_left"], dtype=np.uint8),
            # XGBoost holds node values as f32; JSON prints them round-trip exact
            leaf_value=np.where(leaf, cond.astype(np.float32).astype(np.float64), 0.0)))
    fa = _concat(trees, N.FD_FOREST_XGB_BINARY_LOGISTIC, num_feature, base_score=base_score,
                 meta={"n_trees": len(trees)})
    # sum_hessian is the cover when it can serve as one (a model grown with min_child_weight = 0 may hold zeros:
    # such a forest still loads and scores, it only cannot be explained)
    if fa.cover is not None and not (np.isfinite(fa.cover).all() and (fa.cover > 0).all()):
        fa.cover = None
    return fa


def xgboost_doc_from_forest(fa: ForestArrays, sum_hessian=None, loss_changes=None, base_weights=None) -> Dict[str, Any]:
    """The inverse of xgboost_from_json_doc: a binary:logistic gbtree forest as an XGBoost 2.0.3 JSON document (the
    schema synth.xgboost_doc writes and XGBClassifier.save_model produces). The per-node arrays default to
    fa.meta["sum_hessian" | "loss_changes" | "base_weights"] (what FraudEngine.fit_gbdt attaches), then to fa.cover
    for sum_hessian, then to 1.0 / 0.0 / the leaf value. Every number is written as the shortest decimal that reads
    back to the same f64, so f32 thresholds and leaf weights survive the file bit for bit."""
    if fa.kind != N.FD_FOREST_XGB_BINARY_LOGISTIC:
        raise UnsupportedModel("only a binary:logistic gbtree forest has an XGBoost JSON form")
    M = int(fa.offsets[-1])

    def per_node(given, key, default):
        a = given if given is not None else fa.meta.get(key)
        if a is None:
            return default
        a = np.asarray(a, dtype=np.float64)
        if a.shape != (M,):
            raise ValueError(f"{key}: one value per node ({M})")
        return a

    leaf_all = np.asarray(fa.left) == -1
    sh = per_node(sum_hessian, "sum_hessian", fa.cover if fa.cover is not None else np.ones(M))
    lc = per_node(loss_changes, "loss_changes", np.zeros(M))
    bw = per_node(base_weights, "base_weights", np.where(leaf_all, fa.leaf_value, 0.0))
    trees = []
    for tid in range(fa.n_trees):
        s = slice(int(fa.offsets[tid]), int(fa.offsets[tid + 1]))
        left, right = np.asarray(fa.left[s], np.int64), np.asarray(fa.right[s], np.int64)
        m = len(left)
        leaf = left == -1
        parents = np.full(m, 2147483647, np.int64)
        idx = np.nonzero(~leaf)[0]
        parents[left[idx]] = idx
        parents[right[idx]] = idx
        cond = np.where(leaf, np.asarray(fa.leaf_value[s], np.float64), np.asarray(fa.threshold[s], np.float64))
        trees.append({
            "base_weights": [float(v) for v in bw[s]],
            "categories": [], "categories_nodes": [], "categories_segments": [], "categories_sizes": [],
            "default_left": [int(v) for v in np.where(leaf, 0, np.asarray(fa.default_left[s]))], "id": tid,
            "left_children": [int(v) for v in left],
            "loss_changes": [float(v) for v in np.where(leaf, 0.0, lc[s])],
            "parents": [int(v) for v in parents],
            "right_children": [int(v) for v in np.where(leaf, -1, right)],
            "split_conditions": [float(v) for v in cond],
            "split_indices": [int(v) for v in np.where(leaf, 0, np.asarray(fa.feature[s]))],
            "split_type": [0] * m, "sum_hessian": [float(v) for v in sh[s]],
            "tree_param": {"num_deleted": "0", "num_feature": str(fa.num_feature), "num_nodes": str(m),
                           "size_leaf_vector": "1"},
        })
    T = fa.n_trees
    return {
        "learner": {
            "attributes": {}, "feature_names": [], "feature_types": [],
            "gradient_booster": {
                "model": {
                    "gbtree_model_param": {"num_parallel_tree": "1", "num_trees": str(T)},
                    "iteration_indptr": list(range(T + 1)),
                    "tree_info": [0] * T,
                    "trees": trees,
                },
                "name": "gbtree",
            },
            "learner_model_param": {"base_score": f"{float(fa.base_score):E}", "boost_from_average": "1",
                                    "num_class": "0", "num_feature": str(fa.num_feature), "num_target": "1"},
            "objective": {"name": "binary:logistic", "reg_loss_param": {"scale_pos_weight": "1"}},
        },
        "version": [2, 0, 3],
    }


def load_xgboost_json(path: str) -> ForestArrays:
    with open(path, "r") as f:
        return xgboost_from_json_doc(json.load(f))


# ----------------------------------------------------------------------------------- IsolationForest

def iforest_from_sklearn(model) -> ForestArrays:
    """Flatten a fitted sklearn IsolationForest (sklearn/ensemble/_iforest.py)."""
    from sklearn.ensemble._iforest import _average_path_length

    n_features = int(model.n_features_in_)
    subsample = int(model._max_features) != n_features
    trees = []
    for i, (est, feats) in enumerate(zip(model.estimators_, model.estimators_features_)):
        t = est.tree_
        left = np.asarray(t.children_left, dtype=np.int64)
        leaf = left == -1
        f = np.asarray(t.feature, dtype=np.int64)
        if subsample:
            f = np.where(leaf, 0, np.asarray(feats, dtype=np.int64)[np.where(leaf, 0, f)])
        else:
            f = np.where(leaf, 0, f)
        dl = getattr(t, "missing_go_to_left", None)
        dl = np.zeros(len(left), np.uint8) if dl is None else np.asarray(dl, dtype=np.uint8)
        # exactly the per-leaf term _parallel_compute_tree_depths adds: (dpl + apl) - 1.0, f64
        lv = (np.asarray(model._decision_path_lengths[i], dtype=np.float64)
              + np.asarray(model._average_path_length_per_tree[i], dtype=np.float64) - 1.0)
        trees.append(dict(left=np.where(leaf, -1, left), right=np.asarray(t.children_right, dtype=np.int64),
                          feature=f, threshold=np.where(leaf, 0.0, np.asarray(t.threshold, dtype=np.float64)),
                          default_left=dl, leaf_value=np.where(leaf, lv, 0.0),
                          cover=np.asarray(t.weighted_n_node_samples, dtype=np.float64)))
    max_samples = getattr(model, "_max_samples", model.max_samples_)
    denom = float(len(model.estimators_) * _average_path_length([max_samples])[0])
    return _concat(trees, N.FD_FOREST_SKLEARN_IFOREST, n_features, if_offset=float(model.offset_),
                   if_denominator=denom, meta={"n_trees": len(trees)})


def sklearn_iforest_from_forest(fa: ForestArrays, max_samples: Optional[int] = None, contamination=None):
    """The inverse of iforest_from_sklearn: a scikit-learn IsolationForest holding the trees of `fa` (what
    FraudEngine.fit_iforest returns), which joblib pickles and ModelManager loads like one scikit-learn fitted. The
    training data is not needed: a template is fitted on two rows for its fitted attributes, then every estimator's
    tree_ is rebuilt from fa's arrays through Tree.__setstate__ and the per-tree path-length arrays recomputed from
    the rebuilt trees as IsolationForest.fit does. max_samples defaults to fa.meta["max_samples"], contamination to
    fa.meta["contamination"] (0: "auto"); per-node sample counts come from fa.meta["n_node_samples"], then fa.cover.
    Features are stored as the model's own columns (estimators_features_ is every column, whatever max_features
    grew the trees)."""
    from sklearn.ensemble import IsolationForest
    from sklearn.ensemble._iforest import _average_path_length
    from sklearn.tree._tree import Tree

    if fa.kind != N.FD_FOREST_SKLEARN_IFOREST:
        raise UnsupportedModel("only an IsolationForest has a scikit-learn IsolationForest form")
    T, F = fa.n_trees, int(fa.num_feature)
    psi = int(fa.meta["max_samples"] if max_samples is None else max_samples)
    cont = fa.meta.get("contamination", 0.0) if contamination is None else contamination
    cont = "auto" if isinstance(cont, str) or float(cont) == 0.0 else float(cont)
    counts = fa.meta.get("n_node_samples", fa.cover)
    if counts is None:
        raise ValueError("the forest carries no per-node sample counts (meta['n_node_samples'] or cover)")
    counts = np.asarray(counts, dtype=np.float64)
    model = IsolationForest(n_estimators=T, max_samples=2, contamination="auto", random_state=0)
    model.fit(np.arange(2 * F, dtype=np.float64).reshape(2, F))
    node_dtype = model.estimators_[0].tree_.__getstate__()["nodes"].dtype
    model._decision_path_lengths, model._average_path_length_per_tree = [], []
    for tid, est in enumerate(model.estimators_):
        s = slice(int(fa.offsets[tid]), int(fa.offsets[tid + 1]))
        left = np.asarray(fa.left[s], np.int64)
        leaf = left == -1
        m = len(left)
        nodes = np.zeros(m, dtype=node_dtype)
        nodes["left_child"] = np.where(leaf, -1, left)
        nodes["right_child"] = np.where(leaf, -1, np.asarray(fa.right[s], np.int64))
        nodes["feature"] = np.where(leaf, -2, np.asarray(fa.feature[s], np.int64))
        nodes["threshold"] = np.where(leaf, -2.0, np.asarray(fa.threshold[s], np.float64))
        nodes["n_node_samples"] = counts[s].astype(np.int64)
        nodes["weighted_n_node_samples"] = counts[s]
        if "missing_go_to_left" in node_dtype.names:
            nodes["missing_go_to_left"] = np.where(leaf, 0, np.asarray(fa.default_left[s], np.uint8))
        depth = np.zeros(m, np.int64)
        for i in np.nonzero(~leaf)[0]:  # breadth-first or any parent-before-child numbering
            depth[left[i]] = depth[fa.right[s][i]] = depth[i] + 1
        tree = Tree(F, np.array([1], dtype=np.intp), 1)
        tree.__setstate__({"max_depth": int(depth.max()), "node_count": m, "nodes": nodes,
                           "values": np.zeros((m, 1, 1), np.float64)})
        est.tree_ = tree
        est.max_features_ = 1
        model._decision_path_lengths.append(tree.compute_node_depths())
        model._average_path_length_per_tree.append(_average_path_length(tree.n_node_samples))
    model.estimators_features_ = [np.arange(F) for _ in range(T)]
    model.max_samples = psi
    model.max_samples_ = psi
    model._max_samples = psi
    model._max_features = F
    model.contamination = cont
    model.offset_ = float(fa.if_offset)
    return model


def load_isolation_forest_joblib(path: str) -> ForestArrays:
    import joblib
    return iforest_from_sklearn(joblib.load(path))


# ------------------------------------------------------------------------- sklearn forest classifiers

_CLASSIFIERS = ("RandomForestClassifier", "ExtraTreesClassifier", "DecisionTreeClassifier")


def forest_from_sklearn_classifier(model) -> ForestArrays:
    """Flatten a fitted sklearn RandomForestClassifier / ExtraTreesClassifier / DecisionTreeClassifier (one tree)
    with two classes and one output: the models whose predict_proba is the mean of the trees' leaf class fractions
    (sklearn/ensemble/_forest.py predict_proba: the trees' probabilities summed, divided once by n_estimators).
    The leaf value is tree_.value[node, 0, 1], column 1 of classes_: what the reference's
    predict_proba(X)[:, 1] takes (ml/models/model_manager.py:338-346). Anything else (GradientBoosting, whose
    probability is not a leaf mean; more classes; several outputs) raises UnsupportedModel."""
    name = type(model).__name__
    if name not in _CLASSIFIERS:
        raise UnsupportedModel(f"sklearn model {name} is not on the engine path")
    if int(getattr(model, "n_outputs_", 1)) != 1:
        raise UnsupportedModel(f"{name} with {model.n_outputs_} outputs is not supported (one output only)")
    if len(model.classes_) != 2:
        raise UnsupportedModel(f"{name} with {len(model.classes_)} classes is not supported (two classes only)")
    estimators = [model] if name == "DecisionTreeClassifier" else list(model.estimators_)
    trees = []
    for est in estimators:
        t = est.tree_
        left = np.asarray(t.children_left, dtype=np.int64)
        leaf = left == -1
        value = np.asarray(t.value, dtype=np.float64)
        if value.shape[1:] != (1, 2):  # a tree of a 2-class forest that saw one class still has two columns
            raise UnsupportedModel(f"{name}: tree value shape {value.shape} is not [nodes, 1, 2]")
        dl = getattr(t, "missing_go_to_left", None)
        dl = np.zeros(len(left), np.uint8) if dl is None else np.asarray(dl, dtype=np.uint8)
        trees.append(dict(left=np.where(leaf, -1, left), right=np.asarray(t.children_right, dtype=np.int64),
                          feature=np.where(leaf, 0, np.asarray(t.feature, dtype=np.int64)),
                          threshold=np.where(leaf, 0.0, np.asarray(t.threshold, dtype=np.float64)),
                          default_left=dl, leaf_value=np.where(leaf, value[:, 0, 1], 0.0),
                          cover=np.asarray(t.weighted_n_node_samples, dtype=np.float64)))
    return _concat(trees, N.FD_FOREST_SKLEARN_PROBA, int(model.n_features_in_),
                   meta={"n_trees": len(trees), "class": name})
