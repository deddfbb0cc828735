"""CPU: the host reference of the watched GBDT fit (fd_gbdt_fit_eval_ref_host, fd_gbdt_metric_ref_host; DESIGN §4.14
"Evaluation") against independent restatements — the metric seam against roc_auc_midrank (bit-equal) and scikit-learn
on crafted margins, the weighted gradient against numpy, the curve and the eval margins against a numpy walk of the
returned forest, the stopping rule against plain Python on a case that must fire and on a noisy one, the argument
errors, and the compiled resources of the new kernels. No device code runs here."""
import json
from pathlib import Path

import numpy as np
import pytest

import gbdt_cases as GC
import gbdt_eval_cases as EC
from fdengine import _native as N
from fdengine import gbdt_fit_ref_host, gbdt_metric_ref_host
from fdengine.build import RESOURCES
from fdengine.engine import gbdt_grad_ref_host, gbdt_grad_weighted_ref_host
from fdengine.training import ModelTrainer, roc_auc_midrank

VECTORS = EC.metric_vectors()


# ------------------------------------------------------------------ 1. the metric seam
@pytest.mark.parametrize("name", list(VECTORS))
def test_auc_equals_midrank_statistic(name):
    m, y, known = VECTORS[name]
    got = gbdt_metric_ref_host(m, y, "auc")
    want = roc_auc_midrank(y, m)
    assert EC.bits64(got) == EC.bits64(want), (name, got, want)
    if known is not None:
        assert got == known
    metrics = pytest.importorskip("sklearn.metrics")
    assert abs(got - metrics.roc_auc_score(y, EC.sklearn_scores(m))) <= 1e-12


def test_auc_does_not_depend_on_row_order():
    m, y, _ = VECTORS["tie5000_plus257"]
    p = np.random.default_rng(1).permutation(len(m))
    assert gbdt_metric_ref_host(m[p], y[p], "auc") == gbdt_metric_ref_host(m, y, "auc")


def test_auc_puts_nan_above_infinity_as_one_group():
    m = np.array([np.nan, np.inf, -np.nan, 1.0, np.nan], np.float32)
    y = np.array([1, 0, 1, 0, 0], np.uint8)
    # the same order with the NaNs replaced by one finite value above everything (inf by a large finite one)
    stand_in = np.array([9.0, 8.0, 9.0, 1.0, 9.0], np.float32)
    assert gbdt_metric_ref_host(m, y, "auc") == roc_auc_midrank(y, stand_in) == 5.0 / 6.0  # 2 * (2 + 1/2) / (2 * 3)


@pytest.mark.parametrize("name", list(EC.error_vectors()))
def test_error_is_the_share_of_wrong_signs(name):
    m, y = EC.error_vectors()[name]
    assert gbdt_metric_ref_host(m, y, "error") == EC.error_numpy(m, y)
    if name == "zeros_of_both_signs":  # the four zeros predict 0: the two labelled 1 are wrong
        assert gbdt_metric_ref_host(m[:4], y[:4], "error") == 0.5


def test_metric_rejects_bad_arguments():
    m = np.zeros(4, np.float32)
    for y in (np.zeros(4, np.uint8), np.ones(4, np.uint8)):
        with pytest.raises(N.NativeError, match="Only one class present in y_true") as ei:
            gbdt_metric_ref_host(m, y, "auc")
        assert ei.value.code == N.FD_ERR_INVALID_ARG
        assert gbdt_metric_ref_host(m, y, "error") == float(y[0])  # defined for one class
    with pytest.raises(ValueError):
        gbdt_metric_ref_host(m, np.array([0, 1, 2, 0]), "auc")
    with pytest.raises(ValueError):
        gbdt_metric_ref_host(m, np.array([0, 1, 1, 0]), "logloss")
    with pytest.raises(N.NativeError):
        gbdt_metric_ref_host(np.zeros(0, np.float32), np.zeros(0, np.uint8), "error")


# ------------------------------------------------------------------ 2. the weighted gradient
def _grad_margins():  # the margins of tests/test_gpu_gbdt.py::test_gradient_kernel_equals_host
    big = np.finfo(np.float32).max
    m = np.concatenate([np.linspace(-40, 40, 4099), [0.0, -0.0, 88.0, -88.0, big, -big, np.inf, -np.inf]])
    return m.astype(np.float32)


def test_weight_one_gives_todays_gradient_bits():
    m = _grad_margins()
    for label in (0, 1):
        y = np.full(len(m), label, np.uint8)
        g, h = gbdt_grad_weighted_ref_host(m, y, 1.0)
        rg, rh = gbdt_grad_ref_host(m, y)
        np.testing.assert_array_equal(g, rg)
        np.testing.assert_array_equal(h, rh)


@pytest.mark.parametrize("w", [0.25, 19.0, 64.0])
def test_weighted_gradient_against_numpy(w):
    m = _grad_margins()
    y = (np.arange(len(m)) % 2).astype(np.uint8)
    g, h = gbdt_grad_weighted_ref_host(m, y, w)
    ng, nh = EC.weighted_grad_numpy(EC.sigmoid_declared(m), y, w)
    np.testing.assert_array_equal(g, ng)
    np.testing.assert_array_equal(h, nh)
    neg = y == 0
    ug, uh = gbdt_grad_ref_host(m, y)
    np.testing.assert_array_equal(g[neg], ug[neg])  # negative rows are not weighted
    np.testing.assert_array_equal(h[neg], uh[neg])
    assert (h >= 1).all() and np.abs(g.astype(np.int64)).max() <= 2 ** 30
    assert g[~neg].min() == -int(w * 2 ** 24)  # a positive row far on the wrong side: p = 0 to the quantum, g = -w


def test_weight_limits():
    m, y = np.zeros(2, np.float32), np.array([0, 1], np.uint8)
    for w in (0.0, -1.0, 64.5, float("nan"), float("inf")):
        with pytest.raises(N.NativeError) as ei:
            gbdt_grad_weighted_ref_host(m, y, w)
        assert ei.value.code == N.FD_ERR_INVALID_ARG


# ------------------------------------------------------------------ 3. a watched fit that does not stop
@pytest.fixture(scope="module", params=list(GC.FIT_CASES))
def watched(request):
    name = request.param
    X, y, params = GC.fit_case(name)
    Xe, ye = EC.eval_rows(name, 65)
    plain = gbdt_fit_ref_host(X, y, **params)
    fa = gbdt_fit_ref_host(X, y, eval_set=(Xe, ye), **params)
    return name, X, y, params, Xe, ye, plain, fa


def test_eval_set_does_not_change_the_trees(watched):
    name, X, y, params, Xe, ye, plain, fa = watched
    np.testing.assert_array_equal(fa.offsets, plain.offsets)
    GC.assert_same_tree(GC.tree_fields(fa), GC.tree_fields(plain), name)
    np.testing.assert_array_equal(EC.bits32(fa.meta["margins"]), EC.bits32(plain.meta["margins"]))
    assert fa.meta["rounds_run"] == params["n_rounds"] == fa.n_trees
    again = gbdt_fit_ref_host(X, y, eval_set=[(Xe, ye)], scale_pos_weight=1.0, **params)  # the list form
    GC.assert_same_tree(GC.tree_fields(again), GC.tree_fields(plain), name)
    assert again.meta["evals_result"] == fa.meta["evals_result"]


def test_eval_margins_and_curve_equal_a_numpy_walk(watched):
    name, X, y, params, Xe, ye, plain, fa = watched
    by_tree = EC.margins_by_tree(fa, Xe)
    np.testing.assert_array_equal(EC.bits32(fa.meta["eval_margins"]), EC.bits32(by_tree[-1]))
    curve = fa.meta["evals_result"]["validation_0"]["auc"]
    assert len(curve) == params["n_rounds"]
    for t, v in enumerate(curve):
        assert EC.bits64(v) == EC.bits64(roc_auc_midrank(ye, by_tree[t + 1])), (name, t)
    assert fa.meta["best_score"] == max(curve) and fa.meta["best_iteration"] == int(np.argmax(curve))
    err = gbdt_fit_ref_host(X, y, eval_set=(Xe, ye), eval_metric="error", **params)
    ecurve = err.meta["evals_result"]["validation_0"]["error"]
    assert ecurve == [EC.error_numpy(by_tree[t + 1], ye) for t in range(params["n_rounds"])]
    assert err.meta["best_iteration"] == int(np.argmin(ecurve))


# ------------------------------------------------------------------ 4. early stopping
def _saturating():
    X, y, _ = GC.threshold_case(n=200)
    rows = np.arange(0, 200, 3)
    assert 0 < y[rows].sum() < len(rows)
    return X, y, X[rows], y[rows]


@pytest.mark.parametrize("metric", ["auc", "error"])
def test_early_stopping_fires_on_the_saturating_case(metric):
    X, y, Xe, ye = _saturating()
    kw = dict(n_rounds=40, max_bin=256, eval_set=(Xe, ye), eval_metric=metric, early_stopping_rounds=3)
    fa = gbdt_fit_ref_host(X, y, **kw)
    curve = fa.meta["evals_result"]["validation_0"][metric]
    assert fa.meta["best_iteration"] == 0 and fa.meta["rounds_run"] == 4 and len(curve) == 4
    assert curve[0] == (1.0 if metric == "auc" else 0.0)
    assert fa.n_trees == 1 and fa.meta["n_trees"] == 1 and len(fa.left) == fa.offsets[1] == len(fa.cover)
    np.testing.assert_array_equal(EC.bits32(fa.meta["margins"]), EC.bits32(EC.margins_by_tree(fa, X)[-1]))
    # the C ABI returns every grown tree
    n_trees, run, best = _c_abi_fit(X, y, Xe, ye, metric, 3, 40)
    assert (n_trees, run, best) == (4, 4, 0)


def _c_abi_fit(X, y, Xe, ye, metric, k, n_rounds):
    """fd_gbdt_fit_eval_ref_host called directly -> (trees written, rounds_run, best_iteration)"""
    import ctypes as C
    from fdengine.engine import _GbdtOut, _gbdt_eval_struct, _gbdt_xy, _ptr, gbdt_params
    X, y = _gbdt_xy(X, y)
    p = gbdt_params(n_rounds=n_rounds, max_bin=256)
    ev, keep = _gbdt_eval_struct((Xe, ye), metric, k, 1.0, p, *X.shape)
    cap = C.c_int64()
    args = (_ptr(X), _ptr(y), X.shape[0], X.shape[1], X.shape[1], C.byref(p))
    N.call("fd_gbdt_fit_eval_ref_host", *args, None, None, C.byref(cap), None)
    out = _GbdtOut(p.n_rounds, cap.value)
    out.a["offsets"][:] = -1
    nn = C.c_int64()
    N.call("fd_gbdt_fit_eval_ref_host", *args, C.byref(ev), C.byref(out.model), C.byref(nn), None)
    written = int((out.a["offsets"] >= 0).sum()) - 1
    assert out.a["offsets"][written] == nn.value
    return written, ev.rounds_run, ev.best_iteration


@pytest.fixture(scope="module")
def noisy():
    X, y, params = GC.fit_case("trainer_4099x33")
    params["n_rounds"] = 30
    cut = 3 * len(X) // 4
    return X[:cut], y[:cut], X[cut:], y[cut:], params


@pytest.mark.parametrize("metric", ["auc", "error"])
def test_early_stopping_equals_the_rule_applied_to_the_full_curve(noisy, metric):
    X, y, Xe, ye, params = noisy
    full = gbdt_fit_ref_host(X, y, eval_set=(Xe, ye), eval_metric=metric, **params)
    curve = full.meta["evals_result"]["validation_0"][metric]
    run, best = EC.stop_rule(curve, 2, maximise=metric == "auc")
    print(f"{metric}: the rule stops the 30-round fit after {run} rounds, best round {best}")
    got = gbdt_fit_ref_host(X, y, eval_set=(Xe, ye), eval_metric=metric, early_stopping_rounds=2, **params)
    assert (got.meta["rounds_run"], got.meta["best_iteration"]) == (run, best)
    assert got.meta["evals_result"]["validation_0"][metric] == curve[:run]
    assert got.meta["best_score"] == curve[best] and got.n_trees == best + 1
    GC.assert_same_tree(GC.tree_fields(got), EC.prefix_fields(full, best + 1), metric)
    np.testing.assert_array_equal(EC.bits32(got.meta["margins"]), EC.bits32(EC.margins_by_tree(got, X)[-1]))
    # the eval margins are those after the last round that ran, not after the best
    np.testing.assert_array_equal(EC.bits32(got.meta["eval_margins"]), EC.bits32(EC.margins_by_tree(full, Xe)[run]))


def test_class_weight_changes_the_fit_and_keeps_the_margin_invariant():
    X, y, params = GC.fit_case("nan_257x64")
    plain = gbdt_fit_ref_host(X, y, **params)
    fa = gbdt_fit_ref_host(X, y, scale_pos_weight=19.0, **params)
    assert "evals_result" not in fa.meta and fa.meta["rounds_run"] == params["n_rounds"]
    assert not np.array_equal(fa.leaf_value[:int(fa.offsets[1])], plain.leaf_value[:int(plain.offsets[1])])
    np.testing.assert_array_equal(EC.bits32(fa.meta["margins"]), EC.bits32(EC.margins_by_tree(fa, X)[-1]))
    assert fa.meta["margins"].mean() > plain.meta["margins"].mean()  # heavier positives push the margins up


# ------------------------------------------------------------------ 5. argument errors
def test_fit_eval_rejects_bad_arguments():
    X, y, params = GC.fit_case("deep_65x1")
    Xe, ye = EC.eval_rows("deep_65x1", 65)

    def code(**kw):
        with pytest.raises(N.NativeError) as ei:
            gbdt_fit_ref_host(X, y, **dict(params, **kw))
        return ei.value.code

    assert code(eval_set=(Xe, np.zeros(65, np.uint8))) == N.FD_ERR_INVALID_ARG  # one class, AUC
    with pytest.raises(N.NativeError, match="Only one class present in y_true"):
        gbdt_fit_ref_host(X, y, eval_set=(Xe, np.ones(65, np.uint8)), **params)
    assert code(early_stopping_rounds=3) == N.FD_ERR_INVALID_ARG  # no eval set
    for w in (0.0, -2.0, 64.000001):
        assert code(scale_pos_weight=w) == N.FD_ERR_INVALID_ARG, w
    with pytest.raises(ValueError, match="one eval set"):
        gbdt_fit_ref_host(X, y, eval_set=[(Xe, ye), (Xe, ye)], **params)
    with pytest.raises(ValueError, match="eval_metric"):
        gbdt_fit_ref_host(X, y, eval_set=(Xe, ye), eval_metric="logloss", **params)
    X2, y2, p2 = GC.fit_case("nan_257x64")
    with pytest.raises(ValueError, match="columns"):
        gbdt_fit_ref_host(X2, y2, eval_set=(X2[:, :63], y2), **p2)  # narrower than F
    # n * w above 2^28: refused before a row is read (the matrix is never touched)
    n = (1 << 22) + 1
    big = np.lib.stride_tricks.as_strided(np.zeros(1, np.float32), shape=(n, 1), strides=(0, 4))
    with pytest.raises(N.NativeError) as ei:
        _c_abi_limit(big, n, 64.0)
    assert ei.value.code == N.FD_ERR_UNSUPPORTED


def _c_abi_limit(X, n, w):
    import ctypes as C
    from fdengine.engine import _GbdtOut, gbdt_params
    p = gbdt_params(n_rounds=1, max_depth=1)
    ev = N.fd_gbdt_eval()
    ev.scale_pos_weight = w
    out = _GbdtOut(1, 3)
    y = np.zeros(1, np.uint8)
    nn = C.c_int64()
    N.call("fd_gbdt_fit_eval_ref_host", C.c_void_p(X.ctypes.data), C.c_void_p(y.ctypes.data), n, 1, 1, C.byref(p),
           C.byref(ev), C.byref(out.model), C.byref(nn), None)


# ------------------------------------------------------------------ 6. the drop-in's shape
def test_model_trainer_has_the_new_attributes(tmp_path):
    tr = ModelTrainer(output_dir=str(tmp_path))
    assert tr.early_stopping_rounds is None and tr.scale_pos_weight == 1.0 and tr.evals_result_ is None


# ------------------------------------------------------------------ 7. compiled resources
def test_eval_kernels_do_not_spill():
    res = json.loads(RESOURCES.read_text())
    mine = {k: v for k, v in res.items() if "gbeval_" in k}
    assert len(mine) >= 9, sorted(mine)
    for k, v in mine.items():
        assert v["scratch"] == 0, k
    committed = json.loads((Path(__file__).resolve().parent.parent / "profiles" / "gbdt_eval" /
                            "kernel_resources.json").read_text())
    assert set(committed) == set(mine)
    assert all(v["scratch"] == 0 for v in committed.values())
