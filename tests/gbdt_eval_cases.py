"""Cases and plain restatements for the watched GBDT fit (eval_set curve, early stopping, class weight; DESIGN §4.14
"Evaluation"), shared by tests/test_gbdt_eval_host.py (CPU) and tests/test_gpu_gbdt_eval.py (GPU). The generators of
tests/gbdt_cases.py are reused; nothing here calls the rule header.
"""
from __future__ import annotations

import numpy as np

import gbdt_cases as GC

SCALE = float(2 ** 24)
TINY = np.float32(1e-45)  # the smallest f32 denormal


def _f32(*v):
    return np.array(v, np.float32)


def _tie_group(n_other, seed):
    """A tie group of 5000 rows (a few workgroups' worth) with n_other distinct values around it, both classes in
    every part, shuffled."""
    rng = np.random.default_rng(seed)
    lo = -1.0 - rng.random(n_other // 2)
    hi = 1.0 + rng.random(n_other - n_other // 2)
    m = np.concatenate([lo, np.full(5000, 0.125), hi]).astype(np.float32)
    y = (rng.random(len(m)) < 0.4).astype(np.uint8)
    y[:2] = (0, 1)
    y[n_other // 2:n_other // 2 + 2] = (0, 1)
    y[-2:] = (0, 1)
    p = rng.permutation(len(m))
    return m[p], y[p]


def metric_vectors():
    """name -> (f32 margins, 0 / 1 labels, the AUC known in advance or None)"""
    rng = np.random.default_rng(77)
    one = np.float32(1.0)
    up, down = np.nextafter(one, np.float32(2.0)), np.nextafter(one, np.float32(0.0))
    v = {
        "n2": (_f32(0.3, -0.1), [1, 0], 1.0),
        "n2_reversed": (_f32(-0.1, 0.3), [1, 0], 0.0),
        "all_equal": (np.full(50, 0.25, np.float32), np.arange(50) % 3 == 0, 0.5),
        "signed_zeros_only": (_f32(-0.0, 0.0, 0.0, -0.0, -0.0, 0.0), [1, 0, 1, 0, 0, 1], 0.5),
        # both zeros tie: the positive at -0 is neither below nor above the negative at +0
        "signed_zeros_mixed": (_f32(-1.0, -0.0, 0.0, 0.0, -0.0, 2.0, -TINY, TINY), [0, 1, 0, 1, 0, 1, 1, 0], None),
        "inf_and_denormals": (_f32(-np.inf, np.inf, -np.inf, np.inf, TINY, -TINY, 0.0, 1.1754942e-38, -1.1754942e-38,
                                   3.4e38, -3.4e38, TINY), [0, 1, 1, 0, 1, 0, 0, 1, 0, 0, 1, 0], None),
        "nextafter": (np.array([down, one, up, one, down, up, -one, -up, -down], np.float32),
                      [0, 1, 0, 0, 1, 1, 0, 1, 0], None),
        "separated_up": (np.r_[np.linspace(-3, -1, 40), np.linspace(1, 3, 25)].astype(np.float32),
                         np.r_[np.zeros(40), np.ones(25)], 1.0),
        "separated_down": (np.r_[np.linspace(-3, -1, 40), np.linspace(1, 3, 25)].astype(np.float32),
                           np.r_[np.ones(40), np.zeros(25)], 0.0),
        "one_positive": (rng.normal(size=1000).astype(np.float32), np.arange(1000) == 417, None),
        "one_negative": (rng.normal(size=1000).astype(np.float32), np.arange(1000) != 3, None),
        "coarse_ties": (np.round(rng.normal(size=4099) * 4).astype(np.float32) / 4, rng.random(4099) < 0.05, None),
    }
    for n in (63, 64, 65, 257, 1025, 4099):
        m, y = _tie_group(n, 100 + n)
        v[f"tie5000_plus{n}"] = (m, y, None)
    return {k: (np.ascontiguousarray(m, np.float32), np.asarray(y).astype(np.uint8), a) for k, (m, y, a) in v.items()}


def error_vectors():
    """Margins exactly 0 of both signs under both labels count as predicted 0 (margin > 0 is false)."""
    rng = np.random.default_rng(78)
    m = np.r_[_f32(0.0, 0.0, -0.0, -0.0, TINY, -TINY, np.inf, -np.inf), rng.normal(size=1025).astype(np.float32)]
    y = np.r_[[0, 1, 0, 1, 0, 1, 0, 1], rng.random(1025) < 0.5].astype(np.uint8)
    return {"zeros_of_both_signs": (m.astype(np.float32), y), "n2": (_f32(1.0, -1.0), np.array([0, 0], np.uint8)),
            "all_right": (_f32(2.0, -2.0, 3.0), np.array([1, 0, 1], np.uint8))}


def error_numpy(margins, y):
    return int(((np.asarray(margins) > 0) != (np.asarray(y) != 0)).sum()) / len(y)


def sklearn_scores(margins):
    """The margins as finite f64 in the same order (scikit-learn refuses infinities): the clip is monotone and ties
    nothing, every finite f32 lying inside it."""
    return np.clip(np.asarray(margins, np.float64), -1e300, 1e300)


def exp_declared(x):
    """The declared e^x (|x| <= 64) restated in numpy: the same f64 operations in the same order, none fused."""
    t = x * 1.4426950408889634
    k = np.where(t < 0.0, t - 0.5, t + 0.5).astype(np.int32)  # the C cast: towards zero
    kd = k.astype(np.float64)
    r = (x - kd * 0.693147180369123816490) - kd * 1.90821492927058770002e-10
    p = np.full_like(x, 1.0 / 6227020800.0)
    for c in (479001600.0, 39916800.0, 3628800.0, 362880.0, 40320.0, 5040.0, 720.0, 120.0, 24.0, 6.0):
        p = p * r + 1.0 / c
    p = p * r + 0.5
    p = p * r + 1.0
    p = p * r + 1.0
    return p * np.ldexp(1.0, k)


def sigmoid_declared(margin):
    x = np.clip(np.asarray(margin, np.float32).astype(np.float64), -64.0, 64.0)
    e = exp_declared(-np.abs(x))
    return np.where(x >= 0.0, 1.0 / (1.0 + e), e / (1.0 + e))


def weighted_grad_numpy(p, y, w):
    """The declared pair from a probability p (f64): positives g = rint(w (p - 1) 2^24), h = max(1, rint(w p (1 - p)
    2^24)); negatives unweighted. np.rint rounds ties to even, as the rule does."""
    y = np.asarray(y).astype(bool)
    wy = np.where(y, float(w), 1.0)
    g = np.rint(wy * (p - y) * SCALE).astype(np.int64)
    h = np.maximum(np.rint(wy * (p * (1.0 - p)) * SCALE), 1).astype(np.int64)
    return g, h


def margins_by_tree(fa, X):
    """[n_trees + 1, n] f32: the rows' margins after 0, 1, ... trees, the f32 adds in tree order (a numpy walk on the
    raw values: x < threshold goes left, a NaN follows default_left)."""
    X = np.asarray(X, np.float32)
    n = len(X)
    bs = np.float32(fa.base_score)
    m = np.full(n, -np.log(np.float32(1.0) / bs - np.float32(1.0)), np.float32)
    out = [m.copy()]
    rows = np.arange(n)
    for t in range(fa.n_trees):
        o = int(fa.offsets[t])
        node = np.zeros(n, np.int64)
        while True:
            left = fa.left[o + node]
            inner = left >= 0
            if not inner.any():
                break
            x = X[rows, fa.feature[o + node]]
            thr = fa.threshold[o + node].astype(np.float32)
            go_left = np.where(np.isnan(x), fa.default_left[o + node] != 0, x < thr)
            nxt = np.where(go_left, left, fa.right[o + node])
            node = np.where(inner, nxt, node)
        m = (m + fa.leaf_value[o + node].astype(np.float32)).astype(np.float32)
        out.append(m.copy())
    return np.stack(out)


def stop_rule(curve, k, maximise):
    """The stopping rule in plain Python over a whole curve -> (rounds_run, best_iteration)."""
    best = None
    best_t = since = 0
    for t, v in enumerate(curve):
        if best is None or (v > best if maximise else v < best):
            best, best_t, since = v, t, 0
        else:
            since += 1
            if since >= k:
                return t + 1, best_t
    return len(curve), best_t


def eval_rows(name, n_eval):
    """An eval set of n_eval rows from the generator of fit case `name` (its NaN share kept), both classes present."""
    rows, F, nan_frac, _ = GC.FIT_CASES[name]
    rng = np.random.default_rng(3000 + 10 * list(GC.FIT_CASES).index(name) + n_eval)
    X = GC._matrix(rng, n_eval, F, nan_frac)
    y = GC._labels(rng, X)
    y[0], y[-1] = 0, 1
    return X, y


def bits32(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def bits64(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def prefix_fields(fa, n_trees):
    """tree_fields of the first n_trees trees of a forest"""
    end = int(fa.offsets[n_trees])
    return {k: np.asarray(v)[:end] for k, v in GC.tree_fields(fa).items()}
