"""Case builders and the numpy reference of the histogram GBDT fit, shared by tests/test_gbdt_host.py (CPU) and
tests/test_gpu_gbdt.py (GPU).

`grow_tree_numpy` restates the declared split search (include/fdengine.h "training") without the rule
header: int64 histograms by np.add.at, every candidate's gain in f64 in the declared order, the first maximum of the
array laid out (feature, cut, missing direction) — which is the declared total order — and a breadth-first queue, which
is XGBoost's depth-wise numbering. Integer inputs, so nothing here depends on a sigmoid.
"""
from __future__ import annotations

import numpy as np

SCALE = float(2 ** 24)
MISSING = 255
MIN_GAIN = 1e-6
FIELDS = ("left", "right", "feature", "threshold", "default_left", "leaf_value", "sum_hessian", "loss_changes",
          "base_weights")


def bin_numpy(X, cuts, offsets):
    """bin(x) = #{cuts <= x}, NaN -> 255"""
    X = np.asarray(X, np.float32)
    out = np.zeros(X.shape, np.uint8)
    for f in range(X.shape[1]):
        c = cuts[offsets[f]:offsets[f + 1]]
        col = X[:, f]
        b = np.searchsorted(c, np.where(np.isnan(col), 0, col), side="right")
        out[:, f] = np.where(np.isnan(col), MISSING, b)
    return out


def quantised_grad_numpy(margin, y):
    """Fixed-point (g, h) from numpy's own sigmoid: inputs for the split search (not the engine's gradient rule)."""
    p = 1.0 / (1.0 + np.exp(-np.asarray(margin, np.float64)))
    g = np.rint((p - y) * SCALE).astype(np.int32)
    h = np.maximum(np.rint(p * (1 - p) * SCALE), 1).astype(np.int32)
    return g, h


def grow_tree_numpy(bins, cuts, offsets, g, h, row_mask=None, feature_mask=None, max_depth=6, reg_lambda=1.0,
                    min_child_weight=1.0, eta=0.1):
    bins = np.asarray(bins, np.uint8)
    n, F = bins.shape
    g64, h64 = np.asarray(g, np.int64), np.asarray(h, np.int64)
    sampled = np.ones(n, bool) if row_mask is None else np.asarray(row_mask).astype(bool)
    kept = [f for f in range(F) if feature_mask is None or (int(feature_mask) >> f) & 1]
    out = {k: [] for k in FIELDS}
    queue = [(np.arange(n), 0)]
    q = 0
    while q < len(queue):
        rows, depth = queue[q]
        s = rows[sampled[rows]]
        G, H = int(g64[s].sum()), int(h64[s].sum())
        weight = -(G / SCALE) / (H / SCALE + reg_lambda) * eta
        best = None
        if depth < max_depth:
            hg = np.zeros((F, 256), np.int64)
            hh = np.zeros((F, 256), np.int64)
            cols = np.broadcast_to(np.arange(F), (len(s), F))
            np.add.at(hg, (cols, bins[s]), g64[s][:, None])
            np.add.at(hh, (cols, bins[s]), h64[s][:, None])
            gains = np.full((F, 254, 2), -np.inf)
            GLs = np.zeros((F, 254, 2), np.int64)
            HLs = np.zeros((F, 254, 2), np.int64)
            for f in kept:
                nc = int(offsets[f + 1] - offsets[f])
                if nc == 0:
                    continue
                cg, ch = np.cumsum(hg[f, :nc]), np.cumsum(hh[f, :nc])
                GL = np.stack([cg, cg + hg[f, MISSING]], axis=1)
                HL = np.stack([ch, ch + hh[f, MISSING]], axis=1)
                gl, hl = GL / SCALE, HL / SCALE
                gr, hr = (G - GL) / SCALE, (H - HL) / SCALE
                a = gl * gl / (hl + reg_lambda)
                b = gr * gr / (hr + reg_lambda)
                c = (G / SCALE) * (G / SCALE) / (H / SCALE + reg_lambda)
                gain = (a + b) - c
                valid = (hl >= min_child_weight) & (hr >= min_child_weight)
                gains[f, :nc] = np.where(valid, gain, -np.inf)
                GLs[f, :nc], HLs[f, :nc] = GL, HL
            k = int(np.argmax(gains))  # the first maximum in (feature, cut, direction) order
            f, j, d = np.unravel_index(k, gains.shape)
            if gains[f, j, d] > MIN_GAIN:
                best = (int(f), int(j), int(d), float(gains[f, j, d]))
        if best is None:
            vals = (-1, -1, 0, 0.0, 0, float(np.float32(weight)), H / SCALE, 0.0, weight)
        else:
            f, j, d, gain = best
            b = bins[rows, f]
            left = np.where(b == MISSING, d == 1, b <= j)
            vals = (len(queue), len(queue) + 1, f, float(cuts[offsets[f] + j]), d, 0.0, H / SCALE, gain, weight)
            queue.append((rows[left], depth + 1))
            queue.append((rows[~left], depth + 1))
        for key, v in zip(FIELDS, vals):
            out[key].append(v)
        q += 1
    dt = dict(left=np.int32, right=np.int32, feature=np.int32, default_left=np.uint8)
    return {k: np.asarray(v, dt.get(k, np.float64)) for k, v in out.items()}


def tree_fields(fa):
    """The same fields of a one-tree (or whole) ForestArrays as fit / grow_tree return it."""
    d = {k: np.asarray(getattr(fa, k)) for k in FIELDS[:6]}
    for k in FIELDS[6:]:
        d[k] = np.asarray(fa.meta[k])
    return d


def assert_same_tree(got, want, what=""):
    """Structure equal and every float bit-equal (compared as bit patterns, so -0.0 != 0.0 and NaN == NaN)."""
    for k in FIELDS:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.shape == b.shape, f"{what}: {k} has {a.shape} nodes, expected {b.shape}"
        if a.dtype.kind == "f":
            same = a.astype(np.float64).view(np.uint64) == b.astype(np.float64).view(np.uint64)
        else:
            same = a.astype(np.int64) == b.astype(np.int64)
        assert same.all(), f"{what}: {k} differs at nodes {np.nonzero(~same)[0][:8]}: {a[~same][:4]} vs {b[~same][:4]}"


def _matrix(rng, n, F, nan_frac=0.0):
    cols = []
    for j in range(F):
        kind = j % 4
        if kind == 0:
            c = rng.normal(size=n)
        elif kind == 1:
            c = rng.poisson(3.0, n).astype(np.float64)  # few distinct values: ties with the cuts
        elif kind == 2:
            c = rng.lognormal(0.0, 1.0, n)
        else:
            c = (rng.random(n) < 0.3).astype(np.float64)
        cols.append(c)
    X = np.stack(cols, axis=1).astype(np.float32)
    if nan_frac:
        X[rng.random(X.shape) < nan_frac] = np.nan
    return X


def _labels(rng, X):
    z = np.nan_to_num(X[:, 0]) + (0.5 * np.nan_to_num(X[:, 1 % X.shape[1]]) if X.shape[1] > 1 else 0.0)
    z = z + rng.normal(scale=0.5, size=len(X))
    return (z > np.median(z)).astype(np.uint8)


def split_case(name):
    """-> dict(X, y, max_bin, params, row_mask, feature_mask): the inputs of one split-search case. The caller derives
    cuts (fd_gbdt_cuts_host), bins (bin_numpy) and integer gradients (quantised_grad_numpy at random margins)."""
    shapes = {  # name: (rows, F, max_bin, depth, min_child_weight, nan_frac)
        "rows1": (1, 1, 2, 1, 1.0, 0.0),
        "rows63_f33_bin16": (63, 33, 16, 6, 0.1, 0.05),
        "rows64_f64": (64, 64, 256, 6, 0.1, 0.0),
        "rows65_f1_depth10": (65, 1, 256, 10, 0.01, 0.0),
        "rows257_bin2_depth1": (257, 64, 2, 1, 1.0, 0.05),
        "rows257_depth10": (257, 33, 256, 10, 0.1, 0.05),
        "rows4099": (4099, 33, 256, 6, 1.0, 0.02),
        "rows4099_f64_bin16": (4099, 64, 16, 6, 1.0, 0.0),
    }
    special = ("constant_column", "all_nan_column", "nan_rows_positive", "identical_columns", "root_cannot_split",
               "labels_equal", "one_feature_mask", "row_mask_half", "row_mask_one_side", "row_mask_empty")
    seed = (list(shapes) + list(special)).index(name)
    rng = np.random.default_rng(1000 + seed)
    n, F, max_bin, depth, mcw, nan_frac = shapes.get(name, (257, 5, 256, 4, 0.5, 0.0))
    X = _matrix(rng, n, F, nan_frac)
    y = _labels(rng, X)
    row_mask = feature_mask = None
    if name == "constant_column":
        X[:, 0] = 3.0
        y = _labels(rng, X[:, 1:])
    elif name == "all_nan_column":
        X[:, 0] = np.nan
        y = _labels(rng, X[:, 1:])
    elif name == "nan_rows_positive":
        y = (X[:, 0] < 0).astype(np.uint8)  # positives lie left of the cut at 0 ...
        pos = np.nonzero(y)[0]
        X[pos[::3], 0] = np.nan  # ... and so must the missing rows, which are all positives
    elif name == "identical_columns":
        X[:, 1] = X[:, 0]
        X[:, 2] = X[:, 0]
    elif name == "root_cannot_split":
        mcw = 1e6
    elif name == "labels_equal":
        y = np.ones(n, np.uint8)
    elif name == "one_feature_mask":
        feature_mask = 1 << 2
    elif name == "row_mask_half":
        row_mask = (rng.random(n) < 0.5).astype(np.uint8)
    elif name == "row_mask_one_side":
        row_mask = (X[:, 0] >= np.median(X[:, 0])).astype(np.uint8)  # the unsampled rows still travel to a child
    elif name == "row_mask_empty":
        row_mask = np.zeros(n, np.uint8)
    margin = np.zeros(n) if name == "labels_equal" else rng.normal(scale=0.5, size=n)
    return dict(name=name, X=X, y=y, max_bin=max_bin, margin=margin, row_mask=row_mask, feature_mask=feature_mask,
                params=dict(max_depth=depth, reg_lambda=1.0, min_child_weight=mcw, eta=0.1))


SPLIT_CASES = ("rows1", "rows63_f33_bin16", "rows64_f64", "rows65_f1_depth10", "rows257_bin2_depth1",
               "rows257_depth10", "rows4099", "rows4099_f64_bin16", "constant_column", "all_nan_column",
               "nan_rows_positive", "identical_columns", "root_cannot_split", "labels_equal", "one_feature_mask",
               "row_mask_half", "row_mask_one_side", "row_mask_empty")


def split_inputs(name, cuts_fn):
    """A split case with its cuts (cuts_fn = fdengine.gbdt_cuts_host), numpy bins and integer gradients."""
    c = split_case(name)
    cuts, offsets = cuts_fn(c["X"], c["max_bin"])
    c["cuts"], c["offsets"] = cuts, offsets
    c["bins"] = bin_numpy(c["X"], cuts, offsets)
    c["g"], c["h"] = quantised_grad_numpy(c["margin"], c["y"])
    return c


def edge_matrix():
    """Values at and around cuts, signed zeros, infinities, denormals and NaN (the binning test)."""
    tiny = np.float32(1e-45)  # the smallest f32 denormal
    base = np.array([-np.inf, -3.0, -1.0, -tiny, -0.0, 0.0, tiny, np.float32(1.1754942e-38), 0.5, 1.0,
                     np.nextafter(np.float32(1.0), np.float32(2.0)), 2.0, 7.0, np.inf, np.nan, np.nan], np.float32)
    rng = np.random.default_rng(5)
    cols = [base, base[::-1].copy(), np.where(np.isnan(base), 0.25, base).astype(np.float32),
            rng.permutation(base)]
    return np.ascontiguousarray(np.stack(cols, axis=1))


FIT_CASES = {  # name: (rows, F, nan_frac, params)
    "trainer_4099x33": (4099, 33, 0.0, dict(n_rounds=10, max_depth=6, eta=0.1, subsample=0.8, colsample_bytree=0.8,
                                           seed=42)),
    "deep_65x1": (65, 1, 0.0, dict(n_rounds=3, max_depth=10, min_child_weight=0.01, seed=7)),
    "nan_257x64": (257, 64, 0.1, dict(n_rounds=5, max_depth=6, subsample=0.5, colsample_bytree=0.3,
                                      min_child_weight=0.1, seed=3)),
}


def fit_case(name):
    n, F, nan_frac, params = FIT_CASES[name]
    rng = np.random.default_rng(2000 + list(FIT_CASES).index(name))
    X = _matrix(rng, n, F, nan_frac)
    return X, _labels(rng, X), dict(params)


def threshold_case(n=600, c=0.3, seed=11):
    """y = [x0 >= c] and 32 noise columns"""
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, 33)).astype(np.float32)
    return X, (X[:, 0] >= np.float32(c)).astype(np.uint8), np.float32(c)
