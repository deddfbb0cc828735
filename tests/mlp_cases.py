"""Shared cases of the MLP head's tests (tests/test_mlp_host.py, tests/test_gpu_mlp.py): the shapes, the inputs and
the reference computation — torch fp32 on the CPU, the reference service's own library: F.linear / relu /
softmax(dim=1)[:, 1] (ml/models/model_manager.py:225-232, 321-330).

Tolerance: max |dp| <= 1e-5, the project's bar for its other f32-MFMA head against torch fp32
(tests/test_gpu_lstm.py). For these shapes at 4,099 rows torch fp32 itself is 6e-8 .. 2.6e-6 from an f64 evaluation
and an f32 evaluation in a permuted summation order 6e-8 .. 3.2e-6 from torch fp32, so the reference alone stays
inside the bar with margin. (Scaling every layer x8 does not: torch fp32 is then 1.4e-5 from f64. The saturation
case scales the last layer only.)
"""
from functools import lru_cache

import numpy as np

from fdengine import mlp as M

TOL = 1e-5
N_MAX = 4099
# (in_dim, hidden, n_layers, weight scale on every layer)
SHAPES = [(64, 64, 3, 1.0), (50, 48, 2, 1.0), (7, 5, 5, 1.0), (64, 64, 8, 1.0), (64, 16, 4, 3.0)]
# row-tile tails (16-row tiles, 4 per workgroup) and several workgroups
NS = [1, 15, 16, 17, 63, 64, 65, 257, N_MAX]


def weights(in_dim=64, hidden=64, n_layers=3, scale=1.0, seed=0, last_scale=None) -> M.MlpWeights:
    """default nn.Linear init ranges times `scale` (the last layer times `last_scale` when given)"""
    s = [scale] * n_layers
    if last_scale is not None:
        s[-1] = last_scale
    return M.random_weights(in_dim, hidden, n_layers, seed=seed, scale=s)


def inputs(n, in_dim, seed=0) -> np.ndarray:
    """randn * 3, the first half of the columns abs().clamp(max=10) (the scoring vector's amounts / counts)"""
    import torch
    g = torch.Generator().manual_seed(1000 + seed)
    X = torch.randn(n, in_dim, generator=g) * 3
    h = in_dim // 2
    X[:, :h] = X[:, :h].abs().clamp(max=10)
    return X.numpy().copy()


def torch_forward(w: M.MlpWeights, X: np.ndarray) -> np.ndarray:
    """-> softmax(model(X))[:, 1], torch fp32 on the CPU, returned as f64 [n]"""
    import torch
    import torch.nn.functional as F
    with torch.no_grad():
        x = torch.from_numpy(np.ascontiguousarray(X, np.float32))
        for i in range(w.n_layers):
            b = None if w.biases[i] is None else torch.from_numpy(w.biases[i])
            x = F.linear(x, torch.from_numpy(w.weights[i]), b)
            if i + 1 < w.n_layers:
                x = torch.relu(x)
        return torch.softmax(x, dim=1)[:, 1].numpy().astype(np.float64)


@lru_cache(maxsize=None)
def case(shape_idx: int, last_scale=None):
    """(weights, X [N_MAX, in_dim], torch reference [N_MAX]) of SHAPES[shape_idx], computed once; read-only"""
    in_dim, hidden, L, scale = SHAPES[shape_idx]
    w = weights(in_dim, hidden, L, scale, seed=shape_idx, last_scale=last_scale)
    X = inputs(N_MAX, in_dim, seed=shape_idx)
    ref = torch_forward(w, X)
    X.setflags(write=False)
    ref.setflags(write=False)
    return w, X, ref


def params_struct(n_layers, dims, null_weight=None, with_bias=True, seed=0):
    """fd_mlp_params over random arrays of the given dims, for the limit checks: -> (struct, keep-alive)"""
    from fdengine import _native as N
    rng = np.random.default_rng(seed)
    p = N.fd_mlp_params()
    p.n_layers = n_layers
    keep = []
    for i, d in enumerate(dims[:9]):
        p.dims[i] = d
    for i in range(min(n_layers, 8)):
        if i + 1 >= len(dims):
            break
        wgt = rng.uniform(-0.1, 0.1, (max(dims[i + 1], 1), max(dims[i], 1))).astype(np.float32)
        b = rng.uniform(-0.1, 0.1, max(dims[i + 1], 1)).astype(np.float32)
        keep += [wgt, b]
        p.weight[i] = None if null_weight == i else wgt.ctypes.data
        p.bias[i] = b.ctypes.data if with_bias else None
    return p, keep
