"""CPU: the MLP head's host side — fd_pack_mlp_host's validation and operand order, the weight-file formats
(fdengine/mlp.py), the drop-in's architecture check, and the kernel's resource budget."""
import ctypes as C
import json

import numpy as np
import pytest

import mlp_cases as K
from fdengine import _native as N
from fdengine import mlp as M
from fdengine.forest import UnsupportedModel


def _pack(p):
    nb = C.c_int64(-1)
    code = N.lib.fd_pack_mlp_host(C.byref(p), None, 0, C.byref(nb))
    return code, nb.value, N.lib.fd_last_error().decode()


def test_pack_accepts_the_reference_shape():
    w = K.weights(64, 64, 3)
    blob = M.pack_mlp_host(w)
    # header, 2 x (64 x 64 + 64), the head padded to 16 outputs (16 x 64 + 16)
    assert blob.size == 32 + 2 * (4096 + 64) + 1024 + 16
    assert blob[1] == 3 and list(blob[2:6]) == [64, 64, 64, 2] and blob[27] == blob.size
    p, keep = w.c_struct()
    code, nbytes, _ = _pack(p)
    assert code == N.FD_OK and nbytes == blob.size * 4
    small = np.empty(8, np.uint32)  # a buffer that is too small is refused, not overrun
    nb = C.c_int64(0)
    assert N.lib.fd_pack_mlp_host(C.byref(p), C.c_void_p(small.ctypes.data), small.nbytes,
                                  C.byref(nb)) == N.FD_ERR_INVALID_ARG


def _emulate(blob: np.ndarray, X: np.ndarray) -> np.ndarray:
    """the kernel's arithmetic from the packed words alone (f64 here): lane l's A operand [t][b][l][r] multiplies
    activation 16 b + 4 (l >> 4) + r and lands on output unit 16 t + (l & 15)"""
    f = blob.view(np.float32)
    L, dims = int(blob[1]), [int(d) for d in blob[2:11]]
    h = np.zeros((X.shape[0], 64))
    h[:, :dims[0]] = X
    lane = np.arange(64)
    for i in range(L):
        kb, ot = (dims[i] + 15) // 16, (dims[i + 1] + 15) // 16
        a = f[blob[11 + i]:blob[11 + i] + ot * kb * 256].reshape(ot, kb, 64, 4).astype(np.float64)
        bias = f[blob[19 + i]:blob[19 + i] + ot * 16].astype(np.float64)
        out = np.zeros((X.shape[0], 64))
        out[:, :ot * 16] = bias
        for t in range(ot):
            for b in range(kb):
                for r in range(4):
                    np.add.at(out, (slice(None), 16 * t + (lane & 15)), a[t, b, :, r] * h[:, 16 * b + 4 * (lane >> 4) + r])
        h = np.maximum(out, 0) if i + 1 < L else out
    z = h[:, :2] - h[:, :2].max(axis=1, keepdims=True)
    e = np.exp(z)
    return e[:, 1] / e.sum(axis=1)


@pytest.mark.parametrize("shape_idx", range(len(K.SHAPES)))
def test_packed_operands_compute_the_model(shape_idx):
    w, X, ref = K.case(shape_idx)
    got = _emulate(M.pack_mlp_host(w), X[:65].astype(np.float64))
    assert np.abs(got - ref[:65]).max() <= K.TOL


def test_null_bias_means_zeros():
    w = K.weights(50, 48, 2, seed=4)
    w0 = M.MlpWeights(w.weights, [None, None])
    wz = M.MlpWeights(w.weights, [np.zeros_like(b) for b in w.biases])
    np.testing.assert_array_equal(M.pack_mlp_host(w0), M.pack_mlp_host(wz))


@pytest.mark.parametrize("n_layers,dims,word", [
    (1, [64, 2], "n_layers"),
    (9, [64] * 9, "n_layers"),
    (3, [64, 65, 64, 2], "hidden width"),
    (3, [65, 64, 64, 2], "in_dim"),
    (3, [64, 64, 0, 2], "hidden width"),
    (3, [64, 64, 64, 3], "2 outputs"),
])
def test_pack_refuses_each_limit_by_name(n_layers, dims, word):
    p, keep = K.params_struct(n_layers, dims)
    code, _, msg = _pack(p)
    assert code == N.FD_ERR_UNSUPPORTED, (code, msg)
    assert word in msg, msg


def test_pack_refuses_inconsistent_dims_and_null_weight():
    p, keep = K.params_struct(3, [64, 64, 64, 2, 2])  # an entry beyond dims[n_layers]
    code, _, msg = _pack(p)
    assert code == N.FD_ERR_INVALID_ARG and "inconsistent" in msg, (code, msg)
    p, keep = K.params_struct(3, [64, 64, 64, 2], null_weight=1)
    code, _, msg = _pack(p)
    assert code == N.FD_ERR_INVALID_ARG and "null" in msg, (code, msg)
    nb = C.c_int64(0)
    assert N.lib.fd_pack_mlp_host(None, None, 0, C.byref(nb)) == N.FD_ERR_INVALID_ARG


def _same(a: M.MlpWeights, b: M.MlpWeights):
    assert a.dims == b.dims
    for x, y in zip(a.weights + a.biases, b.weights + b.biases):
        np.testing.assert_array_equal(x, y)


def test_state_dict_files_round_trip(tmp_path):
    import torch
    from safetensors.numpy import save_file
    w = K.weights(64, 64, 3, seed=7)
    sd = M.state_dict(w)
    torch.save({k: torch.from_numpy(v) for k, v in sd.items()}, str(tmp_path / "gnn_fraud_model.pth"))
    np.savez(str(tmp_path / "m.npz"), **sd)
    save_file(sd, str(tmp_path / "m.safetensors"))
    for f in ("gnn_fraud_model.pth", "m.npz", "m.safetensors"):
        w2 = M.load_mlp_file(str(tmp_path / f))
        _same(w, w2)
        assert (w2.n_layers, w2.in_dim, w2.hidden) == (3, 64, 64)


def test_a_saved_nn_module_state_dict_loads(tmp_path):
    """the file the reference's own architecture would write: torch.save(model.state_dict())"""
    import torch
    from torch import nn

    class Net(nn.Module):
        def __init__(self):
            super().__init__()
            self.layers = nn.ModuleList([nn.Linear(64, 64), nn.Linear(64, 64), nn.Linear(64, 2)])

    torch.manual_seed(3)
    net = Net()
    torch.save(net.state_dict(), str(tmp_path / "sd.pth"))
    w = M.load_mlp_file(str(tmp_path / "sd.pth"))
    assert w.dims == [64, 64, 64, 2]
    np.testing.assert_array_equal(w.weights[2], net.layers[2].weight.detach().numpy())
    # the whole pickled module is refused (weights_only: nothing but tensors is unpickled)
    torch.save(net.layers, str(tmp_path / "module.pth"))
    with pytest.raises(UnsupportedModel):
        M.load_mlp_file(str(tmp_path / "module.pth"))


def test_missing_and_extra_keys_are_refused(tmp_path):
    w = K.weights(64, 64, 3, seed=8)
    sd = M.state_dict(w)
    no_bias = {k: v for k, v in sd.items() if k != "layers.1.bias"}
    np.savez(str(tmp_path / "nobias.npz"), **no_bias)
    with pytest.raises(UnsupportedModel, match="Missing key"):
        M.load_mlp_file(str(tmp_path / "nobias.npz"))
    gap = {k: v for k, v in sd.items() if not k.startswith("layers.1.")}
    np.savez(str(tmp_path / "gap.npz"), **gap)
    with pytest.raises(UnsupportedModel, match="Missing key"):
        M.load_mlp_file(str(tmp_path / "gap.npz"))
    np.savez(str(tmp_path / "extra.npz"), **dict(sd, **{"norm.weight": np.ones(64, np.float32)}))
    with pytest.raises(UnsupportedModel, match="Unexpected key"):
        M.load_mlp_file(str(tmp_path / "extra.npz"))
    np.savez(str(tmp_path / "flat.npz"), **dict(sd, **{"layers.0.weight": np.ones(64 * 64, np.float32)}))
    with pytest.raises(UnsupportedModel, match="2-D"):
        M.load_mlp_file(str(tmp_path / "flat.npz"))


def test_architecture_check_follows_the_config(tmp_path):
    """the reference builds num_layers layers of hidden_channels and load_state_dict is strict: a 3 x 64 file against
    a num_layers = 4 config raises (pure host logic, no engine)"""
    from fdengine.model_manager import load_mlp_checked
    path = str(tmp_path / "gnn_fraud_model.npz")
    np.savez(path, **M.state_dict(K.weights(64, 64, 3, seed=9)))
    assert load_mlp_checked(path, {}).dims == [64, 64, 64, 2]
    assert load_mlp_checked(path, {"hidden_channels": 64, "num_layers": 3, "dropout": 0.1}).n_layers == 3
    with pytest.raises(UnsupportedModel, match="size mismatch"):
        load_mlp_checked(path, {"num_layers": 4})
    with pytest.raises(UnsupportedModel, match="size mismatch"):
        load_mlp_checked(path, {"hidden_channels": 32})
    np.savez(str(tmp_path / "narrow.npz"), **M.state_dict(K.weights(50, 64, 3, seed=9)))
    with pytest.raises(UnsupportedModel, match="size mismatch"):  # in = hidden_channels, as the reference builds it
        load_mlp_checked(str(tmp_path / "narrow.npz"), {})


def test_mlp_kernels_do_not_spill():
    from fdengine.build import RESOURCES
    if not RESOURCES.exists():
        pytest.skip("no kernel_resources.json: build the library first (__graft_entry__.build())")
    res = json.loads(RESOURCES.read_text())
    hits = {k: v for k, v in res.items() if "mlp_" in k}
    assert hits, "no mlp_ kernel in kernel_resources.json"
    for name, v in hits.items():
        assert v["scratch"] == 0, f"{name} spills {v['scratch']} B/lane"
