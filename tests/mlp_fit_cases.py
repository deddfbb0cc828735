"""Shared cases of the MLP fit's tests (tests/test_mlp_fit_host.py, tests/test_gpu_mlp_fit.py): shapes, inputs,
labels and the oracle — torch fp32 on the CPU through library API only: a functional forward with F.linear / relu, the
engine's dropout masks multiplied in explicitly, F.cross_entropy(weight=) as the loss, autograd, torch.optim.Adam / SGD,
the engine's batch order (fdengine.mlp.mlp_fit_batch_host).

Bars:
* gradients: per case 4 x the largest gap between torch-fp32 and torch-f64 autograd on that case, plus 1e-9
  (grad_case computes it from the oracle alone);
* trajectories: max |dw| <= 1e-5 over all parameters, loss_curve within 1e-5 relative.
"""
from functools import lru_cache

import numpy as np

import mlp_cases as K
from fdengine import mlp as M

TOL_W = 1e-5
TOL_LOSS = 1e-5
SHAPES = K.SHAPES
NS = [1, 15, 16, 17, 65, 257, 1027]
BATCH_SIZES = [16, 17, 100, 256]
N_FIT = 1027
SGD = dict(optimizer="sgd", lr=0.05, momentum=0.9)
ADAM = dict(optimizer="adam")
# Trainer to server (test_gpu_mlp_fit.py): the held-out AUC the torch trajectory reaches on ModelTrainer's synthetic
# frame with the engine's batches, masks and the trainer's hyperparameters (hidden 64, 3 layers, dropout 0.1, 20 epochs
# of 256, Adam 1e-3, pos_weight 1, seed 42) — measured on the CPU by trainer_torch_auc() below. The engine must reach
# TRAINER_TORCH_AUC - 0.01.
TRAINER_TORCH_AUC = 0.4826263157894737  # (the frame's labels are mostly the 5 % quota's random flips: near chance)


def weights(shape_idx: int) -> M.MlpWeights:
    in_dim, hidden, L, scale = SHAPES[shape_idx]
    return K.weights(in_dim, hidden, L, scale, seed=shape_idx)


def labels(X: np.ndarray, seed: int = 0) -> np.ndarray:
    """a noisy linear rule at about 10 % positives (at least one of each class from 16 rows on)"""
    rng = np.random.Generator(np.random.PCG64(500 + seed))
    v = rng.normal(size=X.shape[1])
    s = X.astype(np.float64) @ v
    s = (s - s.mean()) / (s.std() + 1e-12) + rng.normal(0, 0.5, len(s))
    y = (s > np.quantile(s, 0.9)).astype(np.uint8)
    if len(y) >= 16 and y.sum() == 0:
        y[int(np.argmax(s))] = 1
    return y


@lru_cache(maxsize=None)
def data(shape_idx: int):
    """(X [1027, in_dim], y [1027]) of a shape, read-only"""
    X = K.inputs(N_FIT, SHAPES[shape_idx][0], seed=shape_idx)
    y = labels(X, shape_idx)
    X.setflags(write=False)
    y.setflags(write=False)
    return X, y


def masks_for(n_layers: int, n: int, p: float, seed: int = 0):
    """the engine's masks of step 0 of a fit whose one batch holds the n rows (None at p = 0)"""
    if p == 0.0:
        return None
    return M.mlp_fit_batch_host(n, 0, 0, n_layers=n_layers, epochs=1, batch_size=n, dropout=p, seed=seed)[1]


def _forward_loss(params, x, y, masks, scale, pos_weight):
    import torch
    import torch.nn.functional as F
    h = x
    L = len(params) // 2
    for i in range(L):
        h = F.linear(h, params[2 * i], params[2 * i + 1])
        if i + 1 < L:
            h = torch.relu(h)
            if masks is not None:
                h = h * masks[i][:, :h.shape[1]] * scale
    return F.cross_entropy(h, y, weight=torch.tensor([1.0, pos_weight], dtype=x.dtype))


def _params(w: M.MlpWeights, dtype):
    import torch
    out = []
    for i in range(w.n_layers):
        out.append(torch.tensor(w.weights[i], dtype=dtype, requires_grad=True))
        out.append(torch.tensor(w.biases[i], dtype=dtype, requires_grad=True))
    return out


def torch_grad(w: M.MlpWeights, X, y, masks, p: float, pos_weight: float, dtype=None):
    """-> (loss, [gradient arrays: w0, b0, w1, b1, ...]) by torch autograd on the CPU in `dtype` (default fp32)"""
    import torch
    dtype = dtype or torch.float32
    params = _params(w, dtype)
    x = torch.tensor(np.asarray(X), dtype=dtype)
    yt = torch.tensor(np.asarray(y), dtype=torch.int64)
    mt = None if masks is None else torch.tensor(np.asarray(masks), dtype=dtype)
    # the scale as the engine forms it: the f32 of 1 / (1 - p)
    loss = _forward_loss(params, x, yt, mt, float(np.float32(1.0 / (1.0 - p))), pos_weight)
    loss.backward()
    return float(loss.detach()), [q.grad.numpy().astype(np.float64) for q in params]


def flat(grads) -> np.ndarray:
    return np.concatenate([np.asarray(g, np.float64).reshape(-1) for g in grads])


def flat_w(w: M.MlpWeights) -> np.ndarray:
    return flat([a for i in range(w.n_layers) for a in (w.weights[i], w.biases[i])])


@lru_cache(maxsize=None)
def grad_case(shape_idx: int, n: int, p: float, pos_weight: float, one_class: bool = False):
    """(w, X[:n], y[:n], masks, torch fp32 loss, torch fp32 gradients flat, the case's bar): computed once"""
    import torch
    w = weights(shape_idx)
    X, y = data(shape_idx)
    X, y = X[:n], (np.zeros(n, np.uint8) if one_class else y[:n])
    masks = masks_for(w.n_layers, n, p, seed=shape_idx)
    l32, g32 = torch_grad(w, X, y, masks, p, pos_weight)
    l64, g64 = torch_grad(w, X, y, masks, p, pos_weight, dtype=torch.float64)
    gap = max(abs(l32 - l64), float(np.abs(flat(g32) - flat(g64)).max()))
    return w, X, y, masks, l32, flat(g32), 4.0 * gap + 1e-9


def torch_fit(init: M.MlpWeights, X, y, *, epochs, batch_size, optimizer="adam", lr=1e-3, betas=(0.9, 0.999),
              eps=1e-8, momentum=0.0, weight_decay=0.0, dropout=0.1, pos_weight=1.0, seed=0, dtype=None):
    """The torch trajectory on the engine's batches and masks -> (MlpWeights, loss_curve [epochs])"""
    import torch
    dtype = dtype or torch.float32
    params = _params(init, dtype)
    if optimizer == "adam":
        opt = torch.optim.Adam(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
    else:
        opt = torch.optim.SGD(params, lr=lr, momentum=momentum, weight_decay=weight_decay)
    n = len(y)
    x = torch.tensor(np.asarray(X), dtype=dtype)
    yt = torch.tensor(np.asarray(y), dtype=torch.int64)
    spe = (n + batch_size - 1) // batch_size
    scale = float(np.float32(1.0 / (1.0 - dropout)))
    curve = []
    for e in range(epochs):
        order = M.mlp_fit_batch_host(n, e, e * spe, n_layers=init.n_layers, epochs=epochs, batch_size=batch_size,
                                     dropout=0.0, seed=seed)[0]
        tot = 0.0
        for j in range(spe):
            rows = torch.from_numpy(order[j * batch_size:(j + 1) * batch_size].astype(np.int64))
            mt = None
            if dropout > 0:
                mk = M.mlp_fit_batch_host(n, e, e * spe + j, n_layers=init.n_layers, epochs=epochs,
                                          batch_size=batch_size, dropout=dropout, seed=seed)[1]
                assert mk.shape[1] == len(rows)
                mt = torch.tensor(mk, dtype=dtype)
            opt.zero_grad()
            loss = _forward_loss(params, x[rows], yt[rows], mt, scale, pos_weight)
            loss.backward()
            opt.step()
            tot += float(loss.detach())
        curve.append(tot / spe)
    L = init.n_layers
    out = M.MlpWeights([params[2 * i].detach().numpy().astype(np.float32) for i in range(L)],
                       [params[2 * i + 1].detach().numpy().astype(np.float32) for i in range(L)])
    return out, np.asarray(curve)


# (shape, optimiser kwargs, n, batch_size, epochs): 40 steps at batch 256 (8 epochs of 5), 44 at batch 100 (4 of 11)
def fit_kw(opt: dict, batch_size: int, epochs: int, seed: int = 0):
    return dict(epochs=epochs, batch_size=batch_size, dropout=0.1, pos_weight=3.0, seed=seed, **opt)


@lru_cache(maxsize=None)
def fit_case(shape_idx: int, opt_name: str, n: int, batch_size: int, epochs: int):
    """(init, X, y, kw, torch weights, torch loss_curve): the torch trajectory computed once"""
    init = weights(shape_idx)
    X, y = data(shape_idx)
    X, y = X[:n], y[:n]
    kw = fit_kw(SGD if opt_name == "sgd" else ADAM, batch_size, epochs, seed=shape_idx)
    tw, tc = torch_fit(init, X, y, **kw)
    return init, X, y, kw, tw, tc


def max_dw(a: M.MlpWeights, b: M.MlpWeights) -> float:
    return float(np.abs(flat_w(a) - flat_w(b)).max())


def trainer_split(seed: int = 42):
    """ModelTrainer's synthetic frame and split -> (X_train, X_test, y_train, y_test)"""
    import tempfile
    from fdengine.training import ModelTrainer
    with tempfile.TemporaryDirectory() as d:
        t = ModelTrainer(output_dir=d, engine=object())
        t.random_state = seed
        return t.prepare_training_data()


def trainer_torch_auc() -> float:
    """The measurement behind TRAINER_TORCH_AUC (CPU, a few seconds)."""
    from fdengine.training import MLP_PARAMS, roc_auc_midrank, scoring_matrix
    Xtr, Xte, ytr, yte = trainer_split()
    Xs = scoring_matrix(Xtr)
    init = M.random_weights(64, MLP_PARAMS["hidden"], MLP_PARAMS["n_layers"], 42)
    tw, _ = torch_fit(init, Xs, ytr.astype(np.uint8), epochs=20, batch_size=256, dropout=MLP_PARAMS["dropout"],
                      pos_weight=1.0, seed=42)
    return roc_auc_midrank(yte, K.torch_forward(tw, scoring_matrix(Xte)))

