"""Shared inputs of tests/test_forest_sparse_host.py and tests/test_gpu_forest_sparse.py: the forests trained in
the tests (3,000 rows x 50 features of synth.feature_matrix, fixed random_state), their rows, sklearn's answers
(computed once per process and left unchanged), and the hand-built forest of extreme shapes."""
import numpy as np

from fdengine import ForestArrays, forest_from_sklearn_classifier, synth
from fdengine import _native as N
from oracle import boundary_ref as B

N_TRAIN, NF, N_ROWS = 3000, 50, 2048
_cache = {}


def train_matrix() -> np.ndarray:
    if "X" not in _cache:
        _cache["X"] = synth.feature_matrix(N_TRAIN, NF, seed=201)
    return _cache["X"]


def classifier(name: str):
    """"rf": RandomForestClassifier, 37 trees; "et": ExtraTreesClassifier, 21 trees; sklearn's defaults otherwise
    (unbounded depth, n_jobs untouched: predict_proba's summation order depends on it). -> (ForestArrays, model)"""
    if name not in _cache:
        X = train_matrix()
        m = synth.random_forest(X, n_estimators={"rf": 37, "et": 21}[name], random_state={"rf": 202, "et": 203}[name],
                                extra=name == "et")
        _cache[name] = forest_from_sklearn_classifier(m), m
    return _cache[name]


def rows(name: str, kind: str) -> np.ndarray:
    """2,048 rows: "boundary" = every column made of the model's thresholds (as an f32 row meets them), their f32
    next-up and next-down and the special values of oracle/boundary_ref.py; "nan" = fresh rows with 5 % NaN."""
    key = (name, kind)
    if key not in _cache:
        fa, _ = classifier(name)
        X = (B.boundary_rows(fa, N_ROWS, seed=211) if kind == "boundary"
             else synth.feature_matrix(N_ROWS, NF, seed=212, nan_frac=0.05))
        X.setflags(write=False)
        _cache[key] = X
    return _cache[key]


def sklearn_answers(name: str, kind: str):
    """-> (apply() leaf ids int32 [n, T], predict_proba[:, 1], the f64 sum of tree_.value[leaf, 0, 1] in estimator
    order) for rows(name, kind), from sklearn itself"""
    key = (name, kind, "sk")
    if key not in _cache:
        _, m = classifier(name)
        X = rows(name, kind)
        leaf = m.apply(X).astype(np.int32)
        raw = np.zeros(len(X), np.float64)
        for t, est in enumerate(m.estimators_):  # in order: the sum sklearn's accumulate makes with one job
            raw = raw + est.tree_.value[leaf[:, t], 0, 1]
        _cache[key] = leaf, m.predict_proba(X)[:, 1], raw
    return _cache[key]


CHAIN = 40


def hand_forest(kind: int, nf: int = 7, seed: int = 5) -> ForestArrays:
    """Four trees: a root that is a leaf; a stump; a LEFT chain of depth 40 (every right child a leaf); a RIGHT chain
    of depth 40. Thresholds around the rows' values (hand_rows), default directions mixed."""
    rng = np.random.Generator(np.random.PCG64(seed))

    def leafv():
        return float(np.float32(rng.normal(0.0, 0.3))) if kind == N.FD_FOREST_XGB_BINARY_LOGISTIC else float(rng.random())

    def chain(left_chain: bool):
        m = 2 * CHAIN + 1
        t = dict(left=np.full(m, -1), right=np.full(m, -1), feature=np.zeros(m, np.int64), threshold=np.zeros(m),
                 default_left=np.zeros(m, np.uint8), leaf_value=np.zeros(m))
        for k in range(CHAIN):  # internal nodes 0, 2, 4, ...; the off-chain child of node 2k is the leaf 2k + 1
            i = 2 * k
            on, off = i + 2, i + 1
            t["left"][i], t["right"][i] = (on, off) if left_chain else (off, on)
            t["feature"][i] = k % nf
            # mostly keep walking: the chain child is taken for ~93 % of the values, so rows reach every depth
            q = float(np.float32(1.5 if left_chain else -1.5) + np.float32(rng.normal(0.0, 0.1)))
            t["threshold"][i] = q
            t["default_left"][i] = rng.integers(0, 2)
            t["leaf_value"][off] = leafv()
        t["leaf_value"][m - 1] = leafv()
        return t

    def tree(left, right, feature, threshold, dl, lv):
        return dict(left=np.array(left), right=np.array(right), feature=np.array(feature),
                    threshold=np.array(threshold, np.float64), default_left=np.array(dl, np.uint8),
                    leaf_value=np.array(lv, np.float64))

    trees = [tree([-1], [-1], [0], [0.0], [0], [leafv()]),
             tree([1, -1, -1], [2, -1, -1], [3, 0, 0], [0.25, 0.0, 0.0], [1, 0, 0], [0.0, leafv(), leafv()]),
             chain(True), chain(False)]
    sizes = [len(t["left"]) for t in trees]
    off = np.zeros(len(trees) + 1, np.int64)
    off[1:] = np.cumsum(sizes)

    def cat(k, dt):
        return np.concatenate([np.asarray(t[k], dt) for t in trees])

    return ForestArrays(kind=kind, num_feature=nf, offsets=off, left=cat("left", np.int32), right=cat("right", np.int32),
                        feature=cat("feature", np.int32), threshold=cat("threshold", np.float64),
                        default_left=cat("default_left", np.uint8), leaf_value=cat("leaf_value", np.float64),
                        base_score=0.3, if_offset=-0.5, if_denominator=4.0 * 3.0)


def hand_rows(n: int, nf: int = 7, seed: int = 6) -> np.ndarray:
    """standard-normal rows with 3 % NaN, a few rows that walk a whole chain (all below / all above its thresholds)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    X = rng.normal(size=(n, nf)).astype(np.float32)
    X[rng.random(X.shape) < 0.03] = np.nan
    X[0] = -5.0
    if n > 1:
        X[1] = 5.0
    return X


def hand_reference(fa: ForestArrays, X: np.ndarray):
    """-> (leaf ids [n, T], sums) by oracle/boundary_ref.walk_reference (follows child ids: no depth limit)"""
    return B.walk_reference(fa, X)
