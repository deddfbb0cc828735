"""The MLP fit without a GPU (csrc/mlp_fit.hip's host side): the counter-based batch order and dropout
masks, the plain-C++ reference's gradients against torch autograd and its trajectories against torch.optim, the file
round trip and the limits. Cases, oracle and bars: tests/mlp_fit_cases.py."""
import ctypes as C

import numpy as np
import pytest

import mlp_fit_cases as F
from fdengine import _native as N
from fdengine import mlp as M
from fdengine.forest import UnsupportedModel


# ---------------------------------------------------------------- 1. batch order and masks
@pytest.mark.parametrize("n", F.NS)
def test_every_epoch_is_a_permutation_and_epochs_and_seeds_differ(n):
    kw = dict(epochs=3, batch_size=16, dropout=0.0)
    orders = [M.mlp_fit_batch_host(n, e, 0, seed=0, **kw)[0] for e in range(3)]
    for o in orders:
        assert o.dtype == np.int32 and sorted(o.tolist()) == list(range(n))
    other = M.mlp_fit_batch_host(n, 0, 0, seed=1, **kw)[0]
    if n >= 15:  # (a permutation of one row cannot differ)
        assert not np.array_equal(orders[0], orders[1]) and not np.array_equal(orders[1], orders[2])
        assert not np.array_equal(orders[0], other)
    np.testing.assert_array_equal(orders[0], M.mlp_fit_batch_host(n, 0, 0, seed=0, **kw)[0])


@pytest.mark.parametrize("batch_size", F.BATCH_SIZES)
def test_last_batch_is_the_short_remainder(batch_size):
    n = 1027
    spe = -(-n // batch_size)
    kw = dict(epochs=2, batch_size=batch_size, dropout=0.1, seed=3)
    for step in (0, spe - 1, spe, 2 * spe - 1):
        masks = M.mlp_fit_batch_host(n, step // spe, step, **kw)[1]
        want = batch_size if (step % spe) < spe - 1 else n - (spe - 1) * batch_size
        assert masks.shape == (2, want, 64)
    with pytest.raises(N.NativeError):
        M.mlp_fit_batch_host(n, 1, 2 * spe, **kw)


@pytest.mark.parametrize("p", [0.0, 0.1, 0.5])
def test_mask_keep_rate(p):
    rows = 256
    m0 = M.mlp_fit_batch_host(rows, 0, 0, n_layers=3, epochs=1, batch_size=rows, dropout=p, seed=7)[1]
    assert m0.shape == (2, rows, 64) and set(np.unique(m0)) <= {0, 1}
    if p == 0.0:
        assert m0.all()
        return
    cnt = m0.size
    sigma = np.sqrt(cnt * p * (1 - p))
    assert abs(int(m0.sum()) - cnt * (1 - p)) <= 5 * sigma
    # another step, another layer, another seed: other masks
    m1 = M.mlp_fit_batch_host(4 * rows, 0, 1, n_layers=3, epochs=1, batch_size=rows, dropout=p, seed=7)[1]
    m2 = M.mlp_fit_batch_host(rows, 0, 0, n_layers=3, epochs=1, batch_size=rows, dropout=p, seed=8)[1]
    assert not np.array_equal(m0, m1) and not np.array_equal(m0, m2) and not np.array_equal(m0[0], m0[1])
    # a mask is a function of (seed, step, layer, row in batch, unit): a smaller batch's is a prefix
    m3 = M.mlp_fit_batch_host(100, 0, 0, n_layers=3, epochs=1, batch_size=100, dropout=p, seed=7)[1]
    np.testing.assert_array_equal(m3, m0[:, :100])


# ---------------------------------------------------------------- 2. gradients against torch autograd
def check_grad(got_loss, got, case, what):
    w, X, y, masks, loss, grads, bar = case
    d = max(abs(got_loss - loss), float(np.abs(F.flat_w(got) - grads).max()))
    print(f"{what}: max |d| = {d:.3e}, bar {bar:.3e}")
    assert d <= bar, (d, bar)


@pytest.mark.parametrize("p,pos_weight", [(0.0, 1.0), (0.1, 3.0), (0.1, 1.0), (0.0, 3.0)])
@pytest.mark.parametrize("n", F.NS)
@pytest.mark.parametrize("shape_idx", range(len(F.SHAPES)))
def test_ref_gradients_match_autograd(shape_idx, n, p, pos_weight):
    case = F.grad_case(shape_idx, n, p, pos_weight)
    w, X, y, masks = case[:4]
    loss, g = M.mlp_grad_ref_host(w, X, y, masks, dropout=p, pos_weight=pos_weight)
    check_grad(loss, g, case, f"shape {F.SHAPES[shape_idx]} n {n} p {p} pw {pos_weight}")


@pytest.mark.parametrize("shape_idx", [0, 2])
def test_ref_gradients_of_a_single_class_batch(shape_idx):
    case = F.grad_case(shape_idx, 65, 0.1, 3.0, True)
    w, X, y, masks = case[:4]
    assert not y.any()
    loss, g = M.mlp_grad_ref_host(w, X, y, masks, dropout=0.1, pos_weight=3.0)
    check_grad(loss, g, case, "one class")


# ---------------------------------------------------------------- 3. trajectories against torch.optim
@pytest.mark.parametrize("batch_size,epochs", [(256, 8), (100, 4)])
@pytest.mark.parametrize("opt", ["adam", "sgd"])
@pytest.mark.parametrize("shape_idx", [0, 2])
def test_ref_trajectory_matches_torch(shape_idx, opt, batch_size, epochs):
    init, X, y, kw, tw, tc = F.fit_case(shape_idx, opt, F.N_FIT, batch_size, epochs)
    w = M.mlp_fit_ref_host(X, y, init=init, **kw)
    d, moved = F.max_dw(w, tw), F.max_dw(w, init)
    rel = float(np.abs(w.meta["loss_curve"] - tc).max() / np.abs(tc).max())
    print(f"shape {F.SHAPES[shape_idx]} {opt} batch {batch_size}: max |dw| = {d:.3e}, moved {moved:.3e}, "
          f"loss rel {rel:.3e}, loss {w.meta['loss_curve'][0]:.4f} -> {w.meta['loss_curve'][-1]:.4f}")
    assert w.meta["steps"] == epochs * -(-F.N_FIT // batch_size) >= 40
    assert d <= F.TOL_W, d
    assert rel <= F.TOL_LOSS, rel
    assert moved >= 0.01, moved
    assert w.meta["loss_curve"][-1] < w.meta["loss_curve"][0]


def test_ref_fit_defaults_and_warm_start():
    X, y = F.data(1)
    a = M.mlp_fit_ref_host(X[:257], y[:257], hidden=48, n_layers=2, epochs=2, batch_size=100, seed=5)
    assert a.dims == [50, 48, 2] and a.meta["steps"] == 6 and a.meta["dropout"] == 0.1
    b = M.mlp_fit_ref_host(X[:257], y[:257], init=M.random_weights(50, 48, 2, 5), epochs=2, batch_size=100, seed=5)
    np.testing.assert_array_equal(F.flat_w(a), F.flat_w(b))  # the default start is random_weights(seed)
    c = M.mlp_fit_ref_host(X[:257], y[:257], init=a, epochs=1, batch_size=100, seed=5)
    assert F.max_dw(c, a) > 0


# ---------------------------------------------------------------- 4. file round trip and limits
@pytest.mark.parametrize("ext", [".pth", ".npz"])
def test_save_state_dict_round_trip(tmp_path, ext):
    w = M.random_weights(64, 64, 3, seed=11)
    path = M.save_state_dict(w, str(tmp_path / ("gnn_fraud_model" + ext)))
    back = M.load_mlp_file(path)
    M.check_architecture(back)
    sd, sb = M.state_dict(w), M.state_dict(back)
    assert list(sd) == list(sb) == [f"layers.{i}.{p}" for i in range(3) for p in ("weight", "bias")]
    for k in sd:
        assert sd[k].shape == sb[k].shape
        np.testing.assert_array_equal(sd[k], sb[k])
    if ext == ".pth":
        import torch
        raw = torch.load(path, map_location="cpu", weights_only=True)
        assert type(raw) is dict and all(isinstance(v, torch.Tensor) for v in raw.values())


def test_save_state_dict_needs_every_bias(tmp_path):
    w = M.random_weights(8, 8, 2, seed=1)
    w.biases[0] = None
    with pytest.raises(UnsupportedModel):
        M.save_state_dict(w, str(tmp_path / "m.pth"))


def _refused(code, **kw):
    X, y = F.data(2)
    X, y = np.array(X[:65]), np.array(y[:65])
    X, y, kw = kw.pop("edit", lambda X, y, kw: (X, y, kw))(X, y, kw)
    args = dict(hidden=5, n_layers=3, epochs=1)
    args.update(kw)
    with pytest.raises(N.NativeError) as ei:
        M.mlp_fit_ref_host(X, y, **args)
    assert ei.value.code == code, ei.value
    return str(ei.value)


def test_limits_are_refused_with_a_message():
    assert "batch_size" in _refused(N.FD_ERR_INVALID_ARG, batch_size=0)
    assert "epochs" in _refused(N.FD_ERR_INVALID_ARG, epochs=0)
    assert "dropout" in _refused(N.FD_ERR_INVALID_ARG, dropout=1.0)
    assert "pos_weight" in _refused(N.FD_ERR_INVALID_ARG, pos_weight=0.0)
    assert "lr" in _refused(N.FD_ERR_INVALID_ARG, lr=float("nan"))

    def label2(X, y, kw):
        y[7] = 2
        return X, y, kw
    assert "outside {0, 1}" in _refused(N.FD_ERR_INVALID_ARG, edit=label2)

    def nan_row(X, y, kw):
        X[3, 1] = np.nan
        return X, y, kw
    assert "non-finite" in _refused(N.FD_ERR_INVALID_ARG, edit=nan_row)

    def inf_row(X, y, kw):
        X[64, 6] = np.inf
        return X, y, kw
    assert "non-finite" in _refused(N.FD_ERR_INVALID_ARG, edit=inf_row)


def test_widths_over_64_and_bad_shapes_are_refused():
    X = np.zeros((4, 64), np.float32)
    y = np.zeros(4, np.uint8)
    wide = M.MlpWeights([np.zeros((65, 64), np.float32), np.zeros((2, 65), np.float32)],
                        [np.zeros(65, np.float32), np.zeros(2, np.float32)])
    with pytest.raises(N.NativeError) as ei:
        M.mlp_fit_ref_host(X, y, init=wide, epochs=1)
    assert ei.value.code == N.FD_ERR_UNSUPPORTED and "64" in str(ei.value)
    three_out = M.MlpWeights([np.zeros((8, 64), np.float32), np.zeros((3, 8), np.float32)],
                             [np.zeros(8, np.float32), np.zeros(3, np.float32)])
    with pytest.raises(N.NativeError) as ei:
        M.mlp_fit_ref_host(X, y, init=three_out, epochs=1)
    assert ei.value.code == N.FD_ERR_UNSUPPORTED
    with pytest.raises(UnsupportedModel):
        M.mlp_fit_ref_host(np.zeros((4, 65), np.float32), y, epochs=1)  # in_dim over 64, named before a start is drawn
    with pytest.raises(N.NativeError) as ei:  # ld below the model's in_dim
        M.mlp_fit_ref_host(np.zeros((4, 32), np.float32), y, init=M.random_weights(64, 8, 2, 0), epochs=1)
    assert ei.value.code == N.FD_ERR_INVALID_ARG
    with pytest.raises(ValueError):
        M.mlp_fit_ref_host(X, np.array([0, 1, 0.5, 0]), epochs=1)
    with pytest.raises(TypeError):
        M.fit_params(M.random_weights(4, 4, 2, 0), learning_rate=0.1)
    p, keep = M.fit_params(M.random_weights(4, 4, 2, 0), epochs=1)
    out = M.FitOut([4, 4, 2], 1)
    assert N.lib.fd_mlp_fit_ref_host(None, None, 4, 4, C.byref(p), C.byref(out.c)) == N.FD_ERR_INVALID_ARG
    assert N.lib.fd_mlp_fit_ref_host(None, None, 4, 4, None, None) == N.FD_ERR_INVALID_ARG
