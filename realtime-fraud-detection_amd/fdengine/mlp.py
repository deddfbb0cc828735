"""The graph_neural member's weights (model_type "pytorch", ml/utils/config.py registry entry, weight 0.15) and
their loaders.

Despite its name the reference's model is a plain MLP over the 64-wide scoring vector:
`_create_pytorch_model_architecture` (ml/models/model_manager.py:202-242) builds `num_layers` nn.Linear layers of
width `hidden_channels` in an nn.ModuleList called `layers` (defaults 64 -> 64 -> 64 -> 2), ReLU (+ dropout, the
identity in eval()) after every layer but the last, softmax(dim=1); `_load_pytorch_model` (:168-179) does
`torch.load` of a state dict and a strict `load_state_dict`; `_predict_pytorch` (:321-330) returns column 1.

Files read here:
  * .pth / .pt   a state dict saved with torch.save (read with weights_only=True: a pickled whole module is refused);
  * .safetensors / .npz with the same keys.
Keys are the ModuleList's names: layers.{i}.weight [out, in], layers.{i}.bias [out], i = 0..n_layers-1; every
layer has both (nn.Linear's default bias=True, which a strict load_state_dict requires), nothing else is accepted.
"""
from __future__ import annotations

import ctypes as C
import re
from dataclasses import dataclass, field
from typing import List, Optional, Sequence

import numpy as np

from .forest import UnsupportedModel

IN_DIM = 64
HIDDEN = 64
N_LAYERS = 3
N_OUT = 2
MAX_LAYERS = 8
MAX_WIDTH = 64


@dataclass
class MlpWeights:
    weights: List[np.ndarray]                  # layer i: [out_i, in_i] f32 (nn.Linear.weight)
    biases: List[Optional[np.ndarray]]         # layer i: [out_i] f32 or None (zeros)
    meta: dict = field(default_factory=dict)   # a fitted model: "loss_curve", "steps" and the fit's parameters

    @property
    def n_layers(self) -> int:
        return len(self.weights)

    @property
    def dims(self) -> List[int]:
        """[in_dim, layer 0's outputs, ..., the last layer's outputs]"""
        return [int(self.weights[0].shape[1])] + [int(w.shape[0]) for w in self.weights]

    @property
    def in_dim(self) -> int:
        return int(self.weights[0].shape[1])

    @property
    def hidden(self) -> int:
        return int(self.weights[0].shape[0])

    def validate(self) -> "MlpWeights":
        if not self.weights or len(self.biases) != len(self.weights):
            raise UnsupportedModel("MLP needs one weight and one bias entry per layer")
        for i, w in enumerate(self.weights):
            if w.ndim != 2:
                raise UnsupportedModel(f"layers.{i}.weight must be 2-D, got shape {tuple(w.shape)}")
            if i and w.shape[1] != self.weights[i - 1].shape[0]:
                raise UnsupportedModel(f"layers.{i}.weight takes {w.shape[1]} inputs, layer {i - 1} gives "
                                       f"{self.weights[i - 1].shape[0]}")
            b = self.biases[i]
            if b is not None and b.shape != (w.shape[0],):
                raise UnsupportedModel(f"layers.{i}.bias has shape {tuple(b.shape)}, expected ({w.shape[0]},)")
        return self

    def c_struct(self):
        """-> (fd_mlp_params, the arrays it points into)"""
        from . import _native as N
        if self.n_layers > MAX_LAYERS:  # (the struct has 8 entries; the library names the limit for 2..8)
            raise UnsupportedModel(f"MLP n_layers must be in [2, {MAX_LAYERS}], got {self.n_layers}")
        keep_w = [np.ascontiguousarray(w, np.float32) for w in self.weights]
        keep_b = [None if b is None else np.ascontiguousarray(b, np.float32) for b in self.biases]
        p = N.fd_mlp_params()
        p.n_layers = self.n_layers
        for i, d in enumerate(self.dims):
            p.dims[i] = d
        for i in range(self.n_layers):
            p.weight[i] = keep_w[i].ctypes.data
            p.bias[i] = None if keep_b[i] is None else keep_b[i].ctypes.data
        return p, (keep_w, keep_b)


def check_architecture(w: MlpWeights, hidden_channels: int = HIDDEN, num_layers: int = N_LAYERS) -> None:
    """The reference builds SimpleGNN(input_dim=hidden_channels, hidden_dim=hidden_channels, output_dim=2,
    num_layers=num_layers) from the config's hyperparameters and then does a strict load_state_dict
    (model_manager.py:168-179, 237-242): a file of any other shape raises (RuntimeError there) and the model is not
    loaded. Pure host logic."""
    want = [int(hidden_channels)] * int(num_layers) + [N_OUT]
    if w.dims != want:
        raise UnsupportedModel(f"size mismatch: the file's layers are {w.dims}, the configured architecture "
                               f"(hidden_channels={hidden_channels}, num_layers={num_layers}) is {want}")
    if any(b is None for b in w.biases):
        raise UnsupportedModel("Missing key(s) in state_dict: a layer has no bias")


_KEY = re.compile(r"^layers\.(\d+)\.(weight|bias)$")


def from_state_dict(sd) -> MlpWeights:
    """layers.{i}.weight / layers.{i}.bias for i = 0..L-1, nothing missing, nothing else (a strict load_state_dict)."""
    if not isinstance(sd, dict):
        raise UnsupportedModel(f"expected a state dict, got {type(sd).__name__}")
    found = {}
    for k, v in sd.items():
        m = _KEY.match(str(k))
        if m is None:
            raise UnsupportedModel(f"Unexpected key(s) in state_dict: {k!r}")
        a = v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v)
        found[(int(m.group(1)), m.group(2))] = np.asarray(a, np.float32)
    L = 1 + max((i for i, _ in found), default=-1)
    if L == 0:
        raise UnsupportedModel("Missing key(s) in state_dict: layers.0.weight")
    for i in range(L):
        for part in ("weight", "bias"):
            if (i, part) not in found:
                raise UnsupportedModel(f"Missing key(s) in state_dict: 'layers.{i}.{part}'")
    return MlpWeights([found[(i, "weight")] for i in range(L)], [found[(i, "bias")] for i in range(L)]).validate()


def load_mlp_file(path: str) -> MlpWeights:
    path = str(path)
    if path.endswith(".safetensors"):
        from safetensors.numpy import load_file
        return from_state_dict(load_file(path))
    if path.endswith(".npz"):
        with np.load(path, allow_pickle=False) as z:
            return from_state_dict({k: z[k] for k in z.files})
    import pickle
    import torch
    try:  # tensors and plain containers only: a pickled nn.Module (torch.save(model)) does not load
        sd = torch.load(path, map_location="cpu", weights_only=True)
    except (pickle.UnpicklingError, RuntimeError, AttributeError, ValueError, EOFError) as e:
        raise UnsupportedModel(f"{path}: not a state dict of tensors (a pickled module is not read): {e}") from e
    return from_state_dict(sd)


def random_weights(in_dim: int = IN_DIM, hidden: int = HIDDEN, n_layers: int = N_LAYERS, seed: int = 0,
                   scale: Sequence[float] = ()) -> MlpWeights:
    """PyTorch's default nn.Linear init ranges: weight and bias U(-1/sqrt(fan_in), 1/sqrt(fan_in)); scale[i]
    multiplies layer i's (default 1). No trained checkpoint ships with the reference."""
    rng = np.random.Generator(np.random.PCG64(seed))
    dims = [in_dim] + [hidden] * (n_layers - 1) + [N_OUT]
    ws, bs = [], []
    for i in range(n_layers):
        k = 1.0 / np.sqrt(dims[i])
        s = float(scale[i]) if i < len(scale) else 1.0
        ws.append((rng.uniform(-k, k, (dims[i + 1], dims[i])) * s).astype(np.float32))
        bs.append((rng.uniform(-k, k, dims[i + 1]) * s).astype(np.float32))
    return MlpWeights(ws, bs).validate()


def state_dict(w: MlpWeights) -> dict:
    """The reference's key names -> arrays (np.savez(path, **state_dict(w)); torch.save of its tensors)."""
    out = {}
    for i in range(w.n_layers):
        out[f"layers.{i}.weight"] = w.weights[i]
        if w.biases[i] is not None:
            out[f"layers.{i}.bias"] = w.biases[i]
    return out


def pack_mlp_host(w: MlpWeights) -> np.ndarray:
    """Host-only validation + packing (no GPU): the engine's packed model as uint32 words (fd_pack_mlp_host)."""
    from . import _native as N
    p, keep = w.c_struct()
    nb = C.c_int64(0)
    N.call("fd_pack_mlp_host", C.byref(p), None, 0, C.byref(nb))
    blob = np.empty(nb.value // 4, np.uint32)
    N.call("fd_pack_mlp_host", C.byref(p), C.c_void_p(blob.ctypes.data), nb.value, C.byref(nb))
    del keep
    return blob


def save_state_dict(w: MlpWeights, path: str) -> str:
    """Write the weights under the reference's keys (state_dict(w)): .npz by numpy, anything else (.pth / .pt) by
    torch.save of a plain dict of tensors — what _load_pytorch_model's torch.load + strict load_state_dict reads, and
    what load_mlp_file reads back. Every layer needs its bias (nn.Linear's default)."""
    path = str(path)
    w.validate()
    if any(b is None for b in w.biases):
        raise UnsupportedModel("save_state_dict: every layer needs a bias (a strict load_state_dict requires it)")
    sd = {k: np.ascontiguousarray(v, np.float32) for k, v in state_dict(w).items()}
    if path.endswith(".npz"):
        with open(path, "wb") as f:  # (np.savez would append .npz to other names; here the name is kept)
            np.savez(f, **sd)
        return path
    import torch
    torch.save({k: torch.from_numpy(v.copy()) for k, v in sd.items()}, path)
    return path


# ---------------------------------------------------------------------- training (csrc/mlp_fit.hip)
OPTIMIZERS = {"adam": 0, "sgd": 1}
FIT_DEFAULTS = dict(epochs=20, batch_size=256, optimizer="adam", lr=1e-3, betas=(0.9, 0.999), eps=1e-8, momentum=0.0,
                    weight_decay=0.0, dropout=0.1, pos_weight=1.0, seed=0)


def fit_params(init: MlpWeights, **kw):
    """-> (fd_mlp_fit_params at FIT_DEFAULTS overridden by kw, the arrays it points into). init: the starting
    weights (the shape is theirs)."""
    from . import _native as N
    unknown = set(kw) - set(FIT_DEFAULTS)
    if unknown:
        raise TypeError(f"unknown MLP fit parameter(s): {sorted(unknown)}")
    a = {**FIT_DEFAULTS, **kw}
    if a["optimizer"] not in OPTIMIZERS:
        raise ValueError(f"optimizer must be 'adam' or 'sgd', got {a['optimizer']!r}")
    init.validate()
    q, keep = init.c_struct()
    p = N.fd_mlp_fit_params()
    p.n_layers = q.n_layers
    for i in range(9):
        p.dims[i] = q.dims[i]
    for i in range(8):
        p.init_weight[i] = q.weight[i]
        p.init_bias[i] = q.bias[i]
    p.epochs, p.batch_size, p.optimizer = int(a["epochs"]), int(a["batch_size"]), OPTIMIZERS[a["optimizer"]]
    p.lr, p.eps, p.momentum = float(a["lr"]), float(a["eps"]), float(a["momentum"])
    p.beta1, p.beta2 = (float(b) for b in a["betas"])
    p.weight_decay, p.dropout, p.pos_weight = float(a["weight_decay"]), float(a["dropout"]), float(a["pos_weight"])
    p.seed = int(a["seed"]) & 0xFFFFFFFFFFFFFFFF
    return p, keep


class FitOut:
    """fd_mlp_fit_out over numpy arrays of a shape's sizes"""

    def __init__(self, dims: Sequence[int], n_loss: int):
        from . import _native as N
        self.ws = [np.zeros((dims[i + 1], dims[i]), np.float32) for i in range(len(dims) - 1)]
        self.bs = [np.zeros(dims[i + 1], np.float32) for i in range(len(dims) - 1)]
        self.loss = np.zeros(max(1, n_loss), np.float64)
        self.c = N.fd_mlp_fit_out()
        for i, (w, b) in enumerate(zip(self.ws, self.bs)):
            self.c.weight[i] = w.ctypes.data
            self.c.bias[i] = b.ctypes.data
        self.c.loss_curve = self.loss.ctypes.data

    def weights(self, **meta) -> MlpWeights:
        return MlpWeights(self.ws, self.bs, dict(meta))


def fit_xy(X, y):
    """-> (contiguous f32 [n, ld], u8 [n]); labels outside 0..255 or fractional are refused here, outside {0, 1} by
    the library"""
    X = np.ascontiguousarray(np.asarray(X, dtype=np.float32))
    if X.ndim != 2:
        raise ValueError("X: a 2-d matrix")
    ya = np.asarray(y).reshape(-1)
    y8 = np.ascontiguousarray(ya.astype(np.uint8))
    if len(y8) != X.shape[0] or not np.array_equal(y8, ya):
        raise ValueError("y: one 0 / 1 label per row of X")
    return X, y8


def _init_for(X_cols: int, hidden: int, n_layers: int, seed: int, init: Optional[MlpWeights]) -> MlpWeights:
    if init is not None:
        return init
    if X_cols > MAX_WIDTH:
        raise UnsupportedModel(f"MLP in_dim must be in [1, {MAX_WIDTH}], got {X_cols}")
    return random_weights(X_cols, hidden, n_layers, seed)


def run_fit(fn: str, head: tuple, x_ptr, y_ptr, n: int, ld: int, init: MlpWeights, kw: dict) -> MlpWeights:
    """One fd_mlp_fit_* call -> the fitted MlpWeights, meta: loss_curve, steps and the fit's parameters."""
    from . import _native as N
    p, keep = fit_params(init, **kw)
    out = FitOut(init.dims, p.epochs)
    N.call(fn, *head, x_ptr, y_ptr, int(n), int(ld), C.byref(p), C.byref(out.c))
    del keep
    return out.weights(loss_curve=out.loss[:p.epochs].copy(), steps=int(out.c.steps), **{**FIT_DEFAULTS, **kw})


def run_grad(fn: str, head: tuple, x_ptr, y_ptr, m_ptr, n: int, ld: int, w: MlpWeights, dropout: float,
             pos_weight: float):
    """One fd_mlp_grad_* call -> (loss, the gradients as MlpWeights)"""
    from . import _native as N
    p, keep = fit_params(w, dropout=dropout, pos_weight=pos_weight)
    out = FitOut(w.dims, 1)
    N.call(fn, *head, x_ptr, y_ptr, int(n), int(ld), C.byref(p), m_ptr, C.byref(out.c))
    del keep
    return float(out.loss[0]), out.weights()


def _vp(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def mlp_fit_ref_host(X, y, *, hidden: int = HIDDEN, n_layers: int = N_LAYERS, init: Optional[MlpWeights] = None,
                     **kw) -> MlpWeights:
    """The fit's single-threaded plain-C++ restatement (fd_mlp_fit_ref_host, no GPU): FraudEngine.fit_mlp's
    arguments and result."""
    X, y = fit_xy(X, y)
    init = _init_for(X.shape[1], hidden, n_layers, int(kw.get("seed", 0)), init)
    return run_fit("fd_mlp_fit_ref_host", (), _vp(X), _vp(y), X.shape[0], X.shape[1], init, kw)


def check_masks(masks, n_layers: int, n: int):
    if masks is None:
        return None
    masks = np.ascontiguousarray(masks, np.uint8)
    if masks.shape != (n_layers - 1, n, MAX_WIDTH):
        raise ValueError(f"masks: [n_layers - 1, n, {MAX_WIDTH}] bytes, got {masks.shape}")
    return masks


def mlp_grad_ref_host(w: MlpWeights, X, y, masks=None, dropout: float = 0.0, pos_weight: float = 1.0):
    """Loss and gradients of the one batch (X, y) at w under masks ([n_layers - 1, n, 64] bytes, None: all kept; kept
    units scaled by 1 / (1 - dropout)), by fd_mlp_grad_ref_host -> (loss, MlpWeights of gradients)."""
    X, y = fit_xy(X, y)
    masks = check_masks(masks, w.n_layers, X.shape[0])
    return run_grad("fd_mlp_grad_ref_host", (), _vp(X), _vp(y), _vp(masks), X.shape[0], X.shape[1], w, dropout,
                    pos_weight)


def run_batch(fn: str, head: tuple, n: int, epoch: int, step: int, n_layers: int, kw: dict):
    from . import _native as N
    p, keep = fit_params(random_weights(1, 1, n_layers, 0), **kw)
    rows = C.c_int32()
    N.call(fn, *head, int(n), C.byref(p), int(epoch), int(step), None, None, C.byref(rows))
    order = np.zeros(n, np.int32)
    masks = np.zeros((n_layers - 1, rows.value, MAX_WIDTH), np.uint8)
    N.call(fn, *head, int(n), C.byref(p), int(epoch), int(step), _vp(order), _vp(masks), C.byref(rows))
    del keep
    return order, masks


def mlp_fit_batch_host(n: int, epoch: int, step: int, *, n_layers: int = N_LAYERS, **kw):
    """What a fit of n rows trains on (fd_mlp_fit_batch_host) -> (epoch `epoch`'s row order [n] int32, global step
    `step`'s masks [n_layers - 1, that batch's rows, 64] u8). kw: epochs, batch_size, dropout, seed."""
    return run_batch("fd_mlp_fit_batch_host", (), n, epoch, step, n_layers, kw)
