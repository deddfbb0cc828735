"""The MLP fit on the device (csrc/mlp_fit.hip: f32 MFMA forward and backward, ordered chunk sums, Adam / SGD) against
torch autograd and torch.optim on the CPU and against the plain-C++ reference; its determinism, launch counts, and the
way from the trainer to the server. Cases, oracle and bars: tests/mlp_fit_cases.py."""
import asyncio

import numpy as np
import pytest

import mlp_cases as K
import mlp_fit_cases as F
from fdengine import mlp as M
from fdengine.training import ModelTrainer, roc_auc_midrank, scoring_matrix

pytestmark = pytest.mark.gpu


def flat_bits(w):
    return np.concatenate([a.reshape(-1).view(np.uint32) for i in range(w.n_layers)
                           for a in (w.weights[i], w.biases[i])])


# ---------------------------------------------------------------- 6. batches and masks
@pytest.mark.parametrize("n,batch_size,p", [(1027, 256, 0.1), (1027, 100, 0.5), (17, 16, 0.1), (65, 17, 0.0), (1, 16, 0.1)])
def test_device_batches_and_masks_equal_the_hosts(engine, n, batch_size, p):
    spe = -(-n // batch_size)
    kw = dict(n_layers=4, epochs=3, batch_size=batch_size, dropout=p, seed=9)
    for epoch, j in ((0, 0), (1, spe - 1), (2, spe // 2)):
        step = epoch * spe + j
        ho, hm = M.mlp_fit_batch_host(n, epoch, step, **kw)
        do, dm = engine.mlp_fit_batch(n, epoch, step, **kw)
        np.testing.assert_array_equal(do, ho)
        np.testing.assert_array_equal(dm, hm)
        assert hm.shape == (3, min(batch_size, n - j * batch_size), 64)


# ---------------------------------------------------------------- 7. gradients against torch autograd
@pytest.mark.parametrize("p,pos_weight", [(0.0, 1.0), (0.1, 3.0)])
@pytest.mark.parametrize("n", F.NS)
@pytest.mark.parametrize("shape_idx", range(len(F.SHAPES)))
def test_device_gradients_match_autograd(engine, shape_idx, n, p, pos_weight):
    w, X, y, masks, loss, grads, bar = F.grad_case(shape_idx, n, p, pos_weight)
    got_loss, g = engine.mlp_grad(w, X, y, masks, dropout=p, pos_weight=pos_weight)
    d = max(abs(got_loss - loss), float(np.abs(F.flat_w(g) - grads).max()))
    print(f"shape {F.SHAPES[shape_idx]} n {n} p {p} pw {pos_weight}: max |d| = {d:.3e}, bar {bar:.3e}")
    assert d <= bar, (d, bar)


@pytest.mark.parametrize("shape_idx", [0, 2])
def test_device_gradients_of_a_single_class_batch(engine, shape_idx):
    w, X, y, masks, loss, grads, bar = F.grad_case(shape_idx, 65, 0.1, 3.0, True)
    got_loss, g = engine.mlp_grad(w, X, y, masks, dropout=0.1, pos_weight=3.0)
    d = max(abs(got_loss - loss), float(np.abs(F.flat_w(g) - grads).max()))
    assert d <= bar, (d, bar)


def test_device_gradients_with_strided_rows(engine):
    """ld = 70 with NaN beyond in_dim: never read; the 16-B and the scalar row loads agree bit for bit"""
    w, X, y, masks, loss, grads, bar = F.grad_case(0, 257, 0.1, 3.0)
    Xw = np.full((257, 70), np.nan, np.float32)
    Xw[:, :64] = X
    l0, g0 = engine.mlp_grad(w, X, y, masks, dropout=0.1, pos_weight=3.0)
    l1, g1 = engine.mlp_grad(w, Xw, y, masks, dropout=0.1, pos_weight=3.0)
    assert l0 == l1
    np.testing.assert_array_equal(flat_bits(g0), flat_bits(g1))


# ---------------------------------------------------------------- 8. whole fits
@pytest.mark.parametrize("n,batch_size,epochs", [(F.N_FIT, 256, 8), (F.N_FIT, 100, 4), (17, 16, 10)])
@pytest.mark.parametrize("opt", ["adam", "sgd"])
@pytest.mark.parametrize("shape_idx", [0, 1, 2, 3])
def test_device_fit_matches_torch_and_the_reference(engine, shape_idx, opt, n, batch_size, epochs):
    init, X, y, kw, tw, tc = F.fit_case(shape_idx, opt, n, batch_size, epochs)
    w = engine.fit_mlp(X, y, init=init, **kw)
    r = M.mlp_fit_ref_host(X, y, init=init, **kw)
    steps = epochs * -(-n // batch_size)
    d_t, d_r, moved = F.max_dw(w, tw), F.max_dw(w, r), F.max_dw(w, init)
    rel_t = float(np.abs(w.meta["loss_curve"] - tc).max() / np.abs(tc).max())
    rel_r = float(np.abs(w.meta["loss_curve"] - r.meta["loss_curve"]).max() / np.abs(tc).max())
    print(f"shape {F.SHAPES[shape_idx]} {opt} n {n} batch {batch_size}: |dw| torch {d_t:.3e} ref {d_r:.3e}, "
          f"moved {moved:.3e}, loss rel torch {rel_t:.3e} ref {rel_r:.3e}")
    assert w.meta["steps"] == r.meta["steps"] == steps
    assert d_t <= F.TOL_W and d_r <= F.TOL_W, (d_t, d_r)
    assert rel_t <= F.TOL_LOSS and rel_r <= F.TOL_LOSS, (rel_t, rel_r)
    assert moved >= 0.01


# ---------------------------------------------------------------- 9. determinism
def test_fit_is_deterministic_and_grid_independent(engine):
    init, X, y, kw, tw, tc = F.fit_case(0, "adam", F.N_FIT, 256, 8)
    base = engine.fit_mlp(X, y, init=init, **kw)
    again = engine.fit_mlp(X, y, init=init, **kw)
    np.testing.assert_array_equal(flat_bits(base), flat_bits(again))
    np.testing.assert_array_equal(base.meta["loss_curve"], again.meta["loss_curve"])
    try:
        for cpw in (1 << 30, 1, 3):  # one workgroup for everything, a chunk per workgroup, an uneven deal
            engine.set_option("mlp_fit_chunks_per_wg", cpw)
            w = engine.fit_mlp(X, y, init=init, **kw)
            np.testing.assert_array_equal(flat_bits(base), flat_bits(w))
            np.testing.assert_array_equal(base.meta["loss_curve"], w.meta["loss_curve"])
    finally:
        engine.set_option("mlp_fit_chunks_per_wg", 0)
    other = engine.fit_mlp(X, y, init=init, **dict(kw, seed=kw["seed"] + 1))
    assert F.max_dw(other, base) > 1e-4


# ---------------------------------------------------------------- 10. launch counters
def test_two_launches_per_step(engine):
    X, y = F.data(0)
    l0, s0 = engine.counter("mlp_fit_launches"), engine.counter("mlp_fit_steps")
    w = engine.fit_mlp(X, y, epochs=3, batch_size=100, seed=1)
    steps = 3 * 11
    assert w.meta["steps"] == steps
    assert engine.counter("mlp_fit_steps") - s0 == steps
    assert engine.counter("mlp_fit_launches") - l0 == 2 * steps  # step + update: none per row or per tile
    l1 = engine.counter("mlp_fit_launches")
    engine.mlp_grad(w, X, y)
    assert engine.counter("mlp_fit_launches") - l1 == 2 and engine.counter("mlp_fit_steps") - s0 == steps


# ---------------------------------------------------------------- 11. trainer to server
def test_fitted_weights_serve(engine):
    X, y = F.data(0)
    w = engine.fit_mlp(X, y, epochs=2, batch_size=256, seed=4)
    engine.load_mlp(w)
    try:
        p = engine.mlp_predict(X)
    finally:
        engine.unload_mlp()
    assert np.abs(p - K.torch_forward(w, X)).max() <= K.TOL


def test_model_trainer_writes_what_the_manager_serves(engine, tmp_path):
    from fdengine.model_manager import EngineMlp, ModelManager
    from fdengine.registry import ScoringConfig
    tr = ModelTrainer(output_dir=str(tmp_path), engine=engine)
    assert (tr.mlp_epochs, tr.mlp_batch_size, tr.mlp_pos_weight) == (20, 256, 1.0)
    Xtr, Xte, ytr, yte = tr.prepare_training_data()
    res = tr.train_graph_neural_model(Xtr, ytr, Xte, yte)
    assert res["model_type"] == "graph_neural"
    assert res["model_path"] == str(tmp_path / "pytorch" / "gnn_fraud_model.pth")
    assert len(res["loss_curve"]) == 20 and res["loss_curve"][-1] < res["loss_curve"][0]
    assert res["training_time_seconds"] > 0
    w = M.load_mlp_file(res["model_path"])
    M.check_architecture(w)
    Xs = scoring_matrix(Xte)
    engine.load_mlp(w)
    try:
        p = engine.mlp_predict(Xs)
    finally:
        engine.unload_mlp()
    assert res["auc_score"] == roc_auc_midrank(yte, p)
    assert np.abs(p - K.torch_forward(w, Xs)).max() <= K.TOL
    print(f"engine AUC {res['auc_score']:.4f}, torch trajectory {F.TRAINER_TORCH_AUC:.4f}")
    assert res["auc_score"] >= F.TRAINER_TORCH_AUC - 0.01
    cfg = ScoringConfig(str(tmp_path))
    for name in ("bert_text", "lstm_sequential"):
        cfg.disable_model(name)
    mm = ModelManager(cfg, device=0)
    try:
        asyncio.run(mm.load_all_models())
        assert mm.is_model_loaded("graph_neural") and isinstance(mm.models["graph_neural"], EngineMlp)
        served = asyncio.run(mm.predict("graph_neural", Xs))
        np.testing.assert_array_equal(served, p.astype(np.float32))
        asyncio.run(mm.cleanup())
    finally:
        mm.engine.close()


# ---------------------------------------------------------------- 12. device tensors
def test_device_tensors_give_the_same_bits(engine):
    import torch
    init, X, y, kw, tw, tc = F.fit_case(1, "sgd", F.N_FIT, 100, 4)
    host = engine.fit_mlp(X, y, init=init, **kw)
    dX = torch.from_numpy(np.ascontiguousarray(X)).to("cuda:0")
    dy = torch.from_numpy(np.ascontiguousarray(y)).to("cuda:0")
    dev = engine.fit_mlp(dX, dy, init=init, **kw)
    np.testing.assert_array_equal(flat_bits(host), flat_bits(dev))
    np.testing.assert_array_equal(host.meta["loss_curve"], dev.meta["loss_curve"])
    with pytest.raises(ValueError):
        engine.fit_mlp(dX.double(), dy, init=init, **kw)
