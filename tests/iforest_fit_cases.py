"""The IsolationForest fit's declared rule (include/fdengine.h) restated in numpy and Python integers,
without the rule header: the keyed permutation a tree's rows come from, a breadth-first queue over min / max / nonzero,
the two hashes of a node, the per-tree feature subset, the leaf term and np.percentile for the offset. Shared by
tests/test_iforest_fit_host.py (the host reference against this) and tests/test_gpu_iforest_fit.py (the device against
the host reference on the same cases)."""
import functools

import numpy as np

M64 = (1 << 64) - 1
TAG_FEATURE, TAG_THRESHOLD, TAG_SUBSET, TAG_ROUND = 0, 1, 2, 3
# the root's threshold hash under this seed (tree 0) has its top 30 bits set: u is within 2^-30 of 1 and
# mn + u (mx - mn) rounds up to mx when mn and mx are adjacent f32 values (found by search over seeds)
SEED_U_ROUNDS_UP = 2507362904


def fmix64(k: int) -> int:
    k ^= k >> 33
    k = (k * 0xff51afd7ed558ccd) & M64
    k ^= k >> 33
    k = (k * 0xc4ceb9fe1a85ec53) & M64
    k ^= k >> 33
    return k


def key_of(seed: int) -> int:
    return fmix64((seed + 0x9e3779b97f4a7c15) & M64)


def hash_of(key: int, tree: int, a: int, tag: int) -> int:
    return fmix64(key ^ ((tree << 32) | (a << 2) | tag))


def psi_of(n: int, max_samples: int = 0) -> int:
    return min(256 if max_samples == 0 else max_samples, n)


def depth_cap(psi: int) -> int:
    return max(1, (max(psi, 2) - 1).bit_length())


def sample_rows(n: int, psi: int, seed: int, tree: int) -> np.ndarray:
    """perm_t(0 .. psi - 1): a 4-round Feistel network on 2 b bits, walked into [0, n)."""
    key = key_of(seed)
    b = 1
    while (1 << (2 * b)) < n:
        b += 1
    mask = (1 << b) - 1
    ks = [hash_of(key, tree, r, TAG_ROUND) for r in range(4)]
    out = np.zeros(psi, np.int64)
    for j in range(psi):
        x = j
        while True:
            L, R = x >> b, x & mask
            for r in range(4):
                L, R = R, L ^ (fmix64(ks[r] ^ R) & mask)
            x = (L << b) | R
            if x < n:
                break
        out[j] = x
    return out


def kept_features(seed: int, tree: int, F: int, max_features: float) -> np.ndarray:
    keep = max(1, int(np.floor(max_features * F)))
    if keep >= F:
        return np.arange(F)
    key = key_of(seed)
    order = sorted(range(F), key=lambda f: (hash_of(key, tree, f, TAG_SUBSET), f))
    return np.sort(np.array(order[:keep]))


def average_path_length(m: int) -> float:
    if m <= 1:
        return 0.0
    if m == 2:
        return 1.0
    v = np.float64(m)
    return float(2.0 * (np.log(v - 1.0) + np.euler_gamma) - 2.0 * (v - 1.0) / v)


def grow_tree(X, rows, seed: int, tree: int, kept=None):
    """One tree from its row ids -> dict of per-node arrays, breadth-first numbering."""
    X = np.asarray(X, np.float32)
    rows = np.asarray(rows, np.int64)
    F = X.shape[1]
    kept = np.arange(F) if kept is None else np.asarray(kept)
    psi = len(rows)
    D = depth_cap(psi)
    key = key_of(seed)
    S = X[rows]
    out = dict(left=[], right=[], feature=[], threshold=[], leaf_value=[], n_node_samples=[], depth=[])
    queue = [(0, 0, np.arange(psi))]  # heap index, depth, sample slots
    q = 0
    while q < len(queue):
        idx, d, seg = queue[q]
        m = len(seg)
        split = False
        if m > 1 and d < D:
            sub = S[seg][:, kept]
            mn, mx = sub.min(axis=0), sub.max(axis=0)
            varying = np.nonzero(mx > mn)[0]
            c = len(varying)
            if c > 0:
                r = (hash_of(key, tree, idx, TAG_FEATURE) * c) >> 64
                col = varying[r]
                a, b = np.float64(mn[col]), np.float64(mx[col])
                u = np.float64(hash_of(key, tree, idx, TAG_THRESHOLD) >> 11) * np.float64(2.0 ** -53)
                w = u * (b - a)
                thr = a + w
                if not thr < b:
                    thr = a
                goes_left = sub[:, col].astype(np.float64) <= thr
                split = True
        if split:
            out["left"].append(len(queue))
            out["right"].append(len(queue) + 1)
            out["feature"].append(int(kept[col]))
            out["threshold"].append(float(thr))
            out["leaf_value"].append(0.0)
            queue.append((2 * idx + 1, d + 1, seg[goes_left]))
            queue.append((2 * idx + 2, d + 1, seg[~goes_left]))
        else:
            out["left"].append(-1)
            out["right"].append(-1)
            out["feature"].append(0)
            out["threshold"].append(0.0)
            out["leaf_value"].append(float((np.float64(d + 1) + np.float64(average_path_length(m))) - 1.0))
        out["n_node_samples"].append(float(m))
        out["depth"].append(d)
        q += 1
    dt = dict(left=np.int32, right=np.int32, feature=np.int32, depth=np.int32)
    return {k: np.asarray(v, dt.get(k, np.float64)) for k, v in out.items()}


def raw_scores(trees, X):
    """The f64 sum of the leaf values in tree order, as the serving side adds them."""
    X = np.asarray(X, np.float32)
    raw = np.zeros(len(X), np.float64)
    for t in trees:
        node = np.zeros(len(X), np.int64)
        for _ in range(int(t["depth"].max()) + 1):
            inner = t["left"][node] != -1
            x = X[np.arange(len(X)), t["feature"][node]].astype(np.float64)
            nxt = np.where(x <= t["threshold"][node], t["left"][node], t["right"][node])
            node = np.where(inner, nxt, node)
        raw = raw + t["leaf_value"][node]
    return raw


def fit(X, num_feature=None, n_estimators=100, max_samples=0, max_features=1.0, contamination=0.0, seed=0):
    """The whole fit -> dict(trees, rows, denominator, offset, psi)."""
    X = np.asarray(X, np.float32)
    n = len(X)
    F = X.shape[1] if num_feature is None else num_feature
    psi = psi_of(n, max_samples)
    trees, rows = [], []
    for t in range(n_estimators):
        r = sample_rows(n, psi, seed, t)
        rows.append(r)
        trees.append(grow_tree(X[:, :F], r, seed, t, kept_features(seed, t, F, max_features)))
    denom = float(np.float64(n_estimators) * np.float64(average_path_length(psi)))
    offset = -0.5
    raw = None
    if contamination != 0:
        raw = raw_scores(trees, X[:, :F])
        offset = float(np.percentile(-(2.0 ** (-(raw / denom))), 100.0 * contamination))
    return dict(trees=trees, rows=rows, denominator=denom, offset=offset, psi=psi, raw=raw)


def forest_trees(fa):
    """A ForestArrays as the list of per-tree dicts grow_tree returns (without depth)."""
    out = []
    counts = fa.meta["n_node_samples"]
    for t in range(fa.n_trees):
        s = slice(int(fa.offsets[t]), int(fa.offsets[t + 1]))
        out.append(dict(left=fa.left[s], right=fa.right[s], feature=fa.feature[s], threshold=fa.threshold[s],
                        leaf_value=fa.leaf_value[s], n_node_samples=counts[s], default_left=fa.default_left[s]))
    return out


def assert_same_tree(got, want, what=""):
    """Structure, feature, threshold bits, counts and leaf values."""
    for k in ("left", "right", "feature", "n_node_samples"):
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{what}: {k}")
    for k in ("threshold", "leaf_value"):
        np.testing.assert_array_equal(np.asarray(got[k], np.float64).view(np.uint64),
                                      np.asarray(want[k], np.float64).view(np.uint64), err_msg=f"{what}: {k}")
    if "default_left" in got:
        assert not np.asarray(got["default_left"]).any(), what


def assert_same_forest(got, want, what=""):
    """Two ForestArrays of fits: every array, the offset and the denominator, bit for bit."""
    np.testing.assert_array_equal(got.offsets, want.offsets, err_msg=what)
    for a, b in zip(forest_trees(got), forest_trees(want)):
        assert_same_tree(a, b, what)
    np.testing.assert_array_equal(got.cover, want.cover, err_msg=what)
    assert np.float64(got.if_offset).view(np.uint64) == np.float64(want.if_offset).view(np.uint64), what
    assert np.float64(got.if_denominator).view(np.uint64) == np.float64(want.if_denominator).view(np.uint64), what


# ------------------------------------------------------------------------------------------------ cases

def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


@functools.lru_cache(maxsize=None)
def fit_case(name):
    """-> (X f32 [n, ld], params): the fits both test files run. Small on purpose: T is kept low where psi is high."""
    r = _rng(sum(map(ord, name)))
    if name == "n2_psi2_f1":  # the smallest fit
        return np.array([[1.0], [2.0]], np.float32), dict(n_estimators=3, seed=1)
    if name == "n100_below_default_psi":  # psi = n
        return r.normal(size=(100, 5)).astype(np.float32), dict(n_estimators=6, seed=2, contamination=0.05)
    if name == "psi1024_f64_n5000":  # depth 10, the largest
        return r.normal(size=(5000, 64)).astype(np.float32), dict(n_estimators=8, max_samples=1024, seed=3,
                                                                 contamination=0.05)
    if name == "f33_ld40":  # row stride wider than the model; the other columns hold values no tree may see
        X = r.normal(size=(700, 40)).astype(np.float32)
        X[:, 33:] = 1e30
        return X, dict(n_estimators=5, num_feature=33, seed=4, contamination=0.1)
    if name == "all_rows_identical":  # each tree a single leaf of value c(psi)
        return np.tile(r.normal(size=(1, 6)).astype(np.float32), (300, 1)), dict(n_estimators=4, seed=5)
    if name == "three_constant_columns":  # never chosen
        X = r.normal(size=(400, 8)).astype(np.float32)
        X[:, [1, 4, 7]] = np.float32(3.25)
        return X, dict(n_estimators=8, seed=6)
    if name == "signed_zero_column":  # -0.0 and +0.0 only: constant
        X = r.normal(size=(300, 3)).astype(np.float32)
        X[:, 1] = np.where(r.random(300) < 0.5, np.float32(-0.0), np.float32(0.0))
        return X, dict(n_estimators=8, seed=7)
    if name == "heavy_duplicates":  # interior leaves with m > 1 above depth D
        return r.integers(0, 3, size=(500, 2)).astype(np.float32), dict(n_estimators=8, seed=8, contamination=0.2)
    if name == "column_spans_3e38":  # mx - mn overflows f32, finite in f64
        X = r.normal(size=(200, 3)).astype(np.float32)
        X[:, 0] = np.where(r.random(200) < 0.5, np.float32(-3e38), np.float32(3e38))
        X[:5, 0] = np.float32(0.0)
        return X, dict(n_estimators=8, seed=9)
    if name == "denormals":  # not flushed
        X = (r.integers(1, 50, size=(200, 4)).astype(np.float64) * 1.4e-45).astype(np.float32)
        return X, dict(n_estimators=8, seed=10)
    if name == "max_features_half":  # the per-tree feature subset
        return r.normal(size=(300, 9)).astype(np.float32), dict(n_estimators=12, max_features=0.5, seed=11,
                                                                contamination=0.05)
    if name == "one_tree":
        return r.normal(size=(300, 4)).astype(np.float32), dict(n_estimators=1, seed=12, contamination=0.5)
    if name == "trees300":  # more trees than CUs
        return r.normal(size=(64, 3)).astype(np.float32), dict(n_estimators=300, max_samples=16, seed=13,
                                                               contamination=0.05)
    if name in ("psi504_f64", "psi505_f64"):  # either side of the grow kernel's choice: 504 rows of 65 floats are the
        # most that fit its 128 KiB of LDS; from 505 on it reads the rows of X directly
        return r.normal(size=(600, 64)).astype(np.float32), dict(n_estimators=3, max_samples=int(name[3:6]), seed=14,
                                                                contamination=0.05)
    if name == "u_rounds_up_to_max":  # two adjacent f32 values and a u within 2^-30 of 1: the reset to mn
        one = np.float32(1.0)
        return np.array([[one], [np.nextafter(one, np.float32(2.0))]], np.float32), dict(n_estimators=1,
                                                                                         seed=SEED_U_ROUNDS_UP)
    raise KeyError(name)


FIT_CASES = ("n2_psi2_f1", "n100_below_default_psi", "psi1024_f64_n5000", "f33_ld40", "all_rows_identical",
             "three_constant_columns", "signed_zero_column", "heavy_duplicates", "column_spans_3e38", "denormals",
             "max_features_half", "one_tree", "trees300", "psi504_f64", "psi505_f64", "u_rounds_up_to_max")
SAMPLER_N = (2, 3, 64, 65, 1000, 2 ** 20 + 1)


# one tree from explicit row ids: (rows, feature mask or None) over grow_inputs' 300 x 5 matrix
GROW_CASES = {
    "rows1": (np.array([3]), None),
    "rows2_same": (np.array([4, 4]), None),
    "rows3": (np.array([0, 9, 5]), None),
    "rows65_dup": (np.r_[np.arange(60), np.arange(5)], None),
    "rows1024": (np.arange(1024) % 300, None),
    "mask_one_feature": (np.arange(100), 1 << 2),
    "mask_two": (np.arange(257), (1 << 0) | (1 << 4)),
}


def grow_inputs(name):
    rows, mask = GROW_CASES[name]
    X = np.random.Generator(np.random.PCG64(7)).normal(size=(300, 5)).astype(np.float32)
    kept = None if mask is None else np.array([f for f in range(5) if (mask >> f) & 1])
    return X, rows, mask, kept


def planted(seed=0, n_fit=4096, n_test=4096, share=0.05):
    """Planted anomalies: 8 features of which one is constant; about `share` of the held-out rows shifted by two
    standard deviations in three of the features (hard enough that scikit-learn's own AUC varies with its seed)."""
    r = _rng(1000 + seed)
    fit_rows = r.normal(size=(n_fit, 8)).astype(np.float32)
    test = r.normal(size=(n_test, 8)).astype(np.float32)
    y = (r.random(n_test) < share).astype(np.int64)
    test[y == 1, :3] += np.float32(2.0)
    fit_rows[:, 5] = np.float32(1.5)
    test[:, 5] = np.float32(1.5)
    return fit_rows, test, y
