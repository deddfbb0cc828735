"""Thin object wrapper over the C-ABI (one FraudEngine per GPU).

Host-array calls (`predict`, `blend`) copy through engine-owned staging buffers; `*_device` calls
take device pointers (ints) so HBM-resident inputs (e.g. torch tensors' data_ptr()) are scored in
place. The engine never falls back to the CPU: every call goes through libfdengine.so.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, Optional, Sequence

import numpy as np

from . import _native as N
from .forest import ForestArrays, truncate_forest


def _ptr(a: Optional[np.ndarray]):
    return None if a is None else C.c_void_p(a.ctypes.data)


class FraudEngine:
    def __init__(self, device: int = 0):
        h = C.c_void_p()
        N.call("fd_engine_create", int(device), C.byref(h))
        self._h = h
        self.device = int(device)
        self.forests: Dict[int, dict] = {}

    # ------------------------------------------------------------------ lifecycle
    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h.value:
            N.call("fd_engine_destroy", self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    @property
    def handle(self):
        return self._h

    def set_stream(self, stream_ptr: Optional[int]) -> None:
        """stream_ptr: a hipStream_t handle (torch.cuda.Stream.cuda_stream; 0 = the null/default
        stream). None restores the engine's own stream."""
        if stream_ptr is None:
            N.call("fd_engine_reset_stream", self._h)
        else:
            N.call("fd_engine_set_stream", self._h, C.c_void_p(int(stream_ptr)) if stream_ptr else None)

    def sync(self) -> None:
        N.call("fd_engine_sync", self._h)

    def set_timing(self, enable: bool) -> None:
        N.call("fd_engine_set_timing", self._h, 1 if enable else 0)

    def set_option(self, key: str, value: int) -> None:
        N.call("fd_engine_set_option", self._h, key.encode(), int(value))

    def counter(self, key: str) -> int:
        """fd_engine_get_counter: "pipelined_batches", "sharded_steps", "sharded_host_ns_<phase>", "device_bytes_live"
        (device memory the library holds now, every engine of the process together) ... (include/fdengine.h)."""
        v = N._i64()
        N.call("fd_engine_get_counter", self._h, key.encode(), C.byref(v))
        return int(v.value)

    def read_timing(self, kinds=(N.FD_TIMING_XGB, N.FD_TIMING_IFOREST, N.FD_TIMING_FEATURES, N.FD_TIMING_BLEND,
                                 N.FD_TIMING_ROUTE, N.FD_TIMING_LSTM, N.FD_TIMING_WINDOWS, N.FD_TIMING_INGEST,
                                 N.FD_TIMING_ENSEMBLE),
                    reset: bool = True):
        """-> {kind: (total kernel ms, timed launches)} since the last reset (then resets).
        With a single int `kinds`, returns just that (ms, launches) pair."""
        single = isinstance(kinds, int)
        out = {}
        for k in ([kinds] if single else kinds):
            ms = C.c_double()
            cnt = C.c_int64()
            N.call("fd_timing_read", self._h, int(k), C.byref(ms), C.byref(cnt))
            out[k] = (ms.value, cnt.value)
        if reset:
            N.call("fd_timing_reset", self._h)
        return out[kinds] if single else out

    # ------------------------------------------------------------------ forests
    def load_forest(self, slot: int, fa: ForestArrays) -> None:
        p, t, keep = fa.c_structs()
        N.call("fd_load_forest", self._h, int(slot), C.byref(p), C.byref(t))
        del keep
        if fa.cover is not None:
            self.set_cover(slot, fa.cover)
        nt, d, nf = C.c_int32(), C.c_int32(), C.c_int32()
        N.call("fd_forest_info", self._h, int(slot), C.byref(nt), C.byref(d), C.byref(nf))
        self.forests[slot] = {"kind": fa.kind, "n_trees": nt.value, "depth": d.value, "num_feature": nf.value}

    def load_xgboost_file(self, slot: int, path) -> None:
        """The reference's XGBoost JSON model file, parsed by the engine itself (fd_load_xgboost_json)."""
        N.call("fd_load_xgboost_json", self._h, int(slot), os.fsencode(str(path)))
        nt, d, nf = C.c_int32(), C.c_int32(), C.c_int32()
        N.call("fd_forest_info", self._h, int(slot), C.byref(nt), C.byref(d), C.byref(nf))
        self.forests[slot] = {"kind": N.FD_FOREST_XGB_BINARY_LOGISTIC, "n_trees": nt.value, "depth": d.value,
                              "num_feature": nf.value}

    def unload_forest(self, slot: int) -> None:
        N.call("fd_unload_forest", self._h, int(slot))
        self.forests.pop(slot, None)

    def forest_info(self, slot: int) -> dict:
        if slot not in self.forests:
            raise ValueError(f"Model in slot {slot} not loaded")
        return dict(self.forests[slot])

    def predict(self, slot: int, X: np.ndarray, want_raw: bool = False, want_leaf: bool = False):
        """X: [n, ld] (cast to f32 as XGBoost's DMatrix / sklearn's validate_data do).
        -> prob f64 [n] (+ raw f64 [n], leaf int32 [n, T])."""
        X = np.ascontiguousarray(np.asarray(X, dtype=np.float32))
        if X.ndim == 1:
            X = X.reshape(1, -1)
        n, ld = X.shape
        prob = np.empty(n, np.float64)
        raw = np.empty(n, np.float64) if want_raw else None
        T = self.forests.get(slot, {}).get("n_trees", 0)
        leaf = np.empty((n, T), np.int32) if want_leaf else None
        N.call("fd_forest_predict_host", self._h, int(slot), _ptr(X), n, ld, _ptr(prob), _ptr(raw), _ptr(leaf))
        out = [prob]
        if want_raw:
            out.append(raw)
        if want_leaf:
            out.append(leaf)
        return out[0] if len(out) == 1 else tuple(out)

    def predict_device(self, slot: int, X_ptr: int, n: int, ld: int, prob_ptr: int, raw_ptr: int = 0,
                       leaf_ptr: int = 0) -> None:
        N.call("fd_forest_predict_device", self._h, int(slot), C.c_void_p(X_ptr), int(n), int(ld),
               C.c_void_p(prob_ptr), C.c_void_p(raw_ptr) if raw_ptr else None,
               C.c_void_p(leaf_ptr) if leaf_ptr else None)

    # ------------------------------------------------------------------ attribution (TreeSHAP)
    def set_cover(self, slot: int, cover) -> None:
        """Attach per-node covers (f64, the loaded forest's node order) to the forest in `slot` (fd_forest_set_cover)."""
        cover = np.ascontiguousarray(np.asarray(cover, dtype=np.float64))
        N.call("fd_forest_set_cover", self._h, int(slot), _ptr(cover), cover.size)

    def explain(self, slot: int, X, rows=None, top_k: Optional[int] = None, by_abs: bool = True):
        """Path-dependent TreeSHAP of the forest's raw output (fd_forest_shap_*). X: [n, ld] numpy, or a torch tensor
        on this engine's device (f32, contiguous), which is explained in place. rows: explain only these row indices
        of X, in that order. -> phi f64 [rows, num_feature + 1] (the last column is the bias; a row sums to the raw
        output), or with top_k (<= 16) -> (phi, idx int32 [rows, top_k], val f64 [rows, top_k]): each row's largest
        contributions by |phi| (by_abs) or by signed phi, -1 / 0 where fewer are non-zero. Device input gives device
        tensors back, complete on return (the call waits for the engine's stream)."""
        if slot not in self.forests:
            raise ValueError(f"Model in slot {slot} not loaded")
        F = self.forests[slot]["num_feature"]
        if top_k is not None and not 1 <= int(top_k) <= N.FD_SHAP_MAX_TOPK:
            raise ValueError(f"top_k must be in [1, {N.FD_SHAP_MAX_TOPK}]")
        if type(X).__module__.startswith("torch") and X.is_cuda:
            return self._explain_device(slot, X, rows, top_k, by_abs, F)
        X = np.ascontiguousarray(np.asarray(X, dtype=np.float32))
        if X.ndim == 1:
            X = X.reshape(1, -1)
        n, ld = X.shape
        r = None if rows is None else np.ascontiguousarray(np.asarray(rows, dtype=np.int64).reshape(-1))
        m = n if r is None else r.size
        phi = np.zeros((m, F + 1), np.float64)
        N.call("fd_forest_shap_host", self._h, int(slot), _ptr(X), n, ld, _ptr(r), m, _ptr(phi), F + 1)
        if top_k is None:
            return phi
        idx = np.full((m, int(top_k)), -1, np.int32)
        val = np.zeros((m, int(top_k)), np.float64)
        N.call("fd_shap_topk_host", self._h, _ptr(phi), m, F + 1, F, int(top_k), 1 if by_abs else 0, _ptr(idx),
               _ptr(val))
        return phi, idx, val

    def _explain_device(self, slot, X, rows, top_k, by_abs, F):
        import torch
        if X.dtype != torch.float32 or X.dim() != 2 or not X.is_contiguous():
            raise ValueError("device input: a contiguous 2-d float32 tensor")
        n, ld = X.shape
        r = None if rows is None else torch.as_tensor(rows, dtype=torch.int64, device=X.device).reshape(-1).contiguous()
        m = n if r is None else int(r.numel())
        phi = torch.zeros((m, F + 1), dtype=torch.float64, device=X.device)
        torch.cuda.current_stream(X.device).synchronize()  # the inputs are ready before the engine's stream reads them
        N.call("fd_forest_shap_device", self._h, int(slot), C.c_void_p(X.data_ptr()), n, ld,
               C.c_void_p(r.data_ptr()) if r is not None and m else None, m, C.c_void_p(phi.data_ptr()), F + 1)
        if top_k is None:
            self.sync()
            return phi
        idx = torch.full((m, int(top_k)), -1, dtype=torch.int32, device=X.device)
        val = torch.zeros((m, int(top_k)), dtype=torch.float64, device=X.device)
        torch.cuda.current_stream(X.device).synchronize()
        N.call("fd_shap_topk_device", self._h, C.c_void_p(phi.data_ptr()), m, F + 1, F, int(top_k),
               1 if by_abs else 0, C.c_void_p(idx.data_ptr()), C.c_void_p(val.data_ptr()))
        self.sync()
        return phi, idx, val

    # ------------------------------------------------------------------ training (histogram GBDT, gbdt.hip)
    def fit_gbdt(self, X, y, eval_set=None, eval_metric="auc", early_stopping_rounds=None, scale_pos_weight=1.0,
                 **params) -> ForestArrays:
        """Grow a binary:logistic gbtree forest on the engine (fd_gbdt_fit_*; the declared semantics are DESIGN
        §4.14). X: [n, F <= 64] numpy, or a contiguous f32 torch tensor on this engine's device (then y a uint8 tensor
        there); y: 0 / 1. params: GBDT_DEFAULTS (n_rounds, max_depth, max_bin, eta, reg_lambda, min_child_weight,
        subsample, colsample_bytree, base_score, seed). -> ForestArrays ready for load_forest, cover = sum_hessian,
        meta["sum_hessian" | "loss_changes" | "base_weights"] per node and meta["margins"], the final f32 margins of
        the rows of X (what predict(..., want_raw=True) reports for them).

        eval_set=(X_eval, y_eval) (or a list holding one such pair; the same kind of arrays as X) is evaluated after
        every round on the device (fd_gbdt_fit_eval_*): eval_metric "auc" or "error", early_stopping_rounds=k stops
        after k rounds without a strictly better metric, scale_pos_weight weights the positive rows' gradients. Then
        meta also holds "evals_result" ({"validation_0": {metric: [one value per round run]}}), "best_iteration",
        "best_score", "rounds_run" and "eval_margins" (the eval rows' margins after the last round run). With early
        stopping the forest returned is cut to the trees 0 .. best_iteration (what XGBClassifier.predict_proba uses
        after such a fit, and what any loader of the written file then scores with), and meta["margins"] are that
        forest's; without, every tree is returned."""
        p = gbdt_params(**params)
        watched = eval_set is not None or early_stopping_rounds is not None or float(scale_pos_weight) != 1.0
        if type(X).__module__.startswith("torch") and X.is_cuda:
            import torch
            if X.dtype != torch.float32 or X.dim() != 2 or not X.is_contiguous():
                raise ValueError("device input: a contiguous 2-d float32 tensor")
            y = y.to(device=X.device, dtype=torch.uint8).contiguous()
            n, ld = X.shape
            cap = C.c_int64()
            N.call("fd_gbdt_fit_device", self._h, None, None, n, ld, ld, C.byref(p), None, C.byref(cap), None)
            out = _GbdtOut(p.n_rounds, cap.value)
            margins = torch.zeros(n, dtype=torch.float32, device=X.device)
            nn = C.c_int64()
            if watched:
                ev, keep = _gbdt_eval_struct(eval_set, eval_metric, early_stopping_rounds, scale_pos_weight, p, n, ld,
                                             device=X.device)
                torch.cuda.current_stream(X.device).synchronize()
                N.call("fd_gbdt_fit_eval_device", self._h, C.c_void_p(X.data_ptr()), C.c_void_p(y.data_ptr()), n, ld,
                       ld, C.byref(p), C.byref(ev), C.byref(out.model), C.byref(nn), C.c_void_p(margins.data_ptr()))
                return _gbdt_eval_forest(out, nn.value, ld, p, ev, keep, margins, eval_metric, early_stopping_rounds)
            torch.cuda.current_stream(X.device).synchronize()
            N.call("fd_gbdt_fit_device", self._h, C.c_void_p(X.data_ptr()), C.c_void_p(y.data_ptr()), n, ld, ld,
                   C.byref(p), C.byref(out.model), C.byref(nn), C.c_void_p(margins.data_ptr()))
            fa = out.forest(nn.value, ld, p.base_score)
            fa.meta["margins"] = margins
            return fa
        X, y = _gbdt_xy(X, y)
        if watched:
            return _gbdt_fit_eval("fd_gbdt_fit_eval_host", (self._h,), X, y, p, eval_set, eval_metric,
                                  early_stopping_rounds, scale_pos_weight)
        return _gbdt_fit("fd_gbdt_fit_host", (self._h,), X, y, p)

    def gbdt_metric(self, margins, y, metric="auc") -> float:
        """The eval metric ("auc" or "error") of f32 margins and 0 / 1 labels by the fit's sort and count kernels
        (fd_gbdt_metric_host)."""
        return _gbdt_metric("fd_gbdt_metric_host", (self._h,), margins, y, metric)

    def gbdt_bin(self, X, cuts, offsets) -> np.ndarray:
        """The u8 bin matrix of X under the cuts, by the bin kernel (fd_gbdt_bin_host)."""
        X = np.ascontiguousarray(np.asarray(X, dtype=np.float32))
        n, ld = X.shape
        cuts = np.ascontiguousarray(np.concatenate([np.asarray(cuts, np.float32), np.zeros(1, np.float32)]))
        offsets = np.ascontiguousarray(offsets, dtype=np.int32)
        bins = np.zeros((n, ld), np.uint8)
        N.call("fd_gbdt_bin_host", self._h, _ptr(X), n, ld, ld, _ptr(cuts), _ptr(offsets), _ptr(bins))
        return bins

    def gbdt_grad(self, margin, y):
        """Margins and labels -> the fixed-point (g, h), by the gradient kernel (fd_gbdt_grad_host)."""
        margin = np.ascontiguousarray(margin, dtype=np.float32)
        y = np.ascontiguousarray(y, dtype=np.uint8)
        g, h = np.zeros(margin.size, np.int32), np.zeros(margin.size, np.int32)
        N.call("fd_gbdt_grad_host", self._h, _ptr(margin), _ptr(y), margin.size, _ptr(g), _ptr(h))
        return g, h

    def gbdt_grow_tree(self, bins, cuts, offsets, g, h, row_mask=None, feature_mask=None, **params) -> ForestArrays:
        """One tree from a binned matrix and fixed-point gradients, by the kernels (fd_gbdt_grow_tree_host)."""
        return _gbdt_grow("fd_gbdt_grow_tree_host", (self._h,), bins, cuts, offsets, g, h, row_mask, feature_mask,
                          params)

    # ------------------------------------------------------------------ training (IsolationForest, iforest_fit.hip)
    def fit_iforest(self, X, **params) -> ForestArrays:
        """Grow an IsolationForest on the engine and place its offset (fd_iforest_fit_*; the declared semantics are
        DESIGN §4.15). X: [n >= 2, F <= 64] numpy (finite values), or a contiguous f32 torch tensor on this engine's
        device. params: IFOREST_DEFAULTS (n_estimators, max_samples, max_features, contamination, seed; random_state
        is accepted for seed, "auto" for contamination 0 and for max_samples 0). -> ForestArrays ready for
        load_forest, cover = the nodes' sample counts, if_offset, if_denominator, meta["max_samples"] (psi),
        meta["n_node_samples"] and the parameters under their names. num_feature=F: only the first F columns of X are
        the model's (the rows are wider)."""
        F = params.pop("num_feature", None)
        p = iforest_fit_params(**params)
        if type(X).__module__.startswith("torch") and X.is_cuda:
            import torch
            if X.dtype != torch.float32 or X.dim() != 2 or not X.is_contiguous():
                raise ValueError("device input: a contiguous 2-d float32 tensor")
            n, ld = X.shape
            torch.cuda.current_stream(X.device).synchronize()
            return _iforest_fit("fd_iforest_fit_device", (self._h,), C.c_void_p(X.data_ptr()), n, ld, F, p)
        X = _iforest_x(X)
        return _iforest_fit("fd_iforest_fit_host", (self._h,), _ptr(X), X.shape[0], X.shape[1], F, p)

    def iforest_fit_sample(self, n: int, tree: int, **params) -> np.ndarray:
        """Tree `tree`'s row ids of a fit over n rows, by the sample kernel (fd_iforest_fit_sample_host)."""
        return _iforest_sample("fd_iforest_fit_sample_host", (self._h,), n, tree, params)

    def iforest_fit_grow_tree(self, X, rows, tree: int = 0, feature_mask=None, **params) -> ForestArrays:
        """One tree from explicit row ids, by the grow kernel (fd_iforest_fit_grow_tree_host)."""
        return _iforest_grow("fd_iforest_fit_grow_tree_host", (self._h,), X, rows, tree, feature_mask, params)

    # ------------------------------------------------------------------ card state + features
    _TXN_DTYPES ={"card_key": np.uint64, "ts_ms": np.int64, "amount_cents": np.int64, "merchant": np.int32,
                   "device_fp": np.uint64, "ip_class": np.uint8, "hour": np.uint8, "weekend": np.uint8}

    def state_init(self, capacity: int, window_mode: int = N.FD_WINDOW_REDIS_COMPAT, ring_k: int = 16,
                   seq_len: int = 0) -> None:
        """seq_len > 0 keeps each card's last seq_len events for the LSTM head (lstm_sequential)."""
        p = N.fd_state_params(int(capacity), int(window_mode), int(ring_k), int(seq_len))
        self.seq_len = int(seq_len)
        N.call("fd_state_init", self._h, C.byref(p))

    def state_clear(self) -> None:
        N.call("fd_state_clear", self._h)

    def state_info(self):
        cap, cards = C.c_int64(), C.c_int64()
        N.call("fd_state_info", self._h, C.byref(cap), C.byref(cards))
        return {"capacity": cap.value, "cards": cards.value}

    def load_users(self, key, avg_amount, account_age_days, device_fp) -> None:
        arr = [np.ascontiguousarray(key, np.uint64), np.ascontiguousarray(avg_amount, np.float64),
               np.ascontiguousarray(account_age_days, np.int32),
               np.ascontiguousarray(np.asarray(device_fp).reshape(-1, 3), np.uint64)]
        u = N.fd_users(len(arr[0]), *[a.ctypes.data for a in arr])
        N.call("fd_state_load_users_host", self._h, C.byref(u))

    def load_merchants(self, fraud_rate, risk_multiplier) -> None:
        arr = [np.ascontiguousarray(fraud_rate, np.float64), np.ascontiguousarray(risk_multiplier, np.float64)]
        m = N.fd_merchants(len(arr[0]), *[a.ctypes.data for a in arr])
        N.call("fd_load_merchants_host", self._h, C.byref(m))

    def features(self, txns: dict, want_raw: bool = False):
        """Host SoA batch (dict of arrays, arrival order) -> vectors f32 [n, 64] (+ raw f64 [n, 16])."""
        cols = [np.ascontiguousarray(txns[f], self._TXN_DTYPES[f]) for f in N.TXN_FIELDS]
        n = len(cols[0])
        vec = np.empty((n, N.FD_VECTOR_WIDTH), np.float32)
        raw = np.empty((n, N.FD_RAW_FEATURES), np.float64) if want_raw else None
        b = N.fd_txn_batch(*[c.ctypes.data for c in cols])
        N.call("fd_features_host", self._h, C.byref(b), n, _ptr(vec), _ptr(raw))
        return (vec, raw) if want_raw else vec

    def features_device(self, ptrs: dict, n: int, vec_ptr: int, raw_ptr: int = 0) -> None:
        """ptrs: field -> device pointer (see fdengine._native.TXN_FIELDS)."""
        b = N.fd_txn_batch(*[int(ptrs[f]) for f in N.TXN_FIELDS])
        N.call("fd_features_device", self._h, C.byref(b), int(n), C.c_void_p(vec_ptr),
               C.c_void_p(raw_ptr) if raw_ptr else None)

    def score_batch_device(self, params: N.fd_blend_params, slots: Sequence[int], txn_ptrs: dict, n: int,
                           fp_ptr: int, conf_ptr: int = 0, dec_ptr: int = 0, risk_ptr: int = 0,
                           vec_ptr: int = 0, model_probs_ptr: int = 0,
                           ext_ptrs: Optional[Sequence[Optional[int]]] = None,
                           present: Optional[Sequence[int]] = None) -> None:
        """Whole hot path for one device-resident micro-batch: features (card state updated) ->
        every forest model -> blend. All pointers are device pointers."""
        M = params.n_models
        sl = np.array(list(slots) + [-1] * (N.FD_MAX_MODELS - len(slots)), np.int32)
        pres = np.array([1] * M if present is None else list(present), np.uint8)
        ext = (C.c_void_p * N.FD_MAX_MODELS)()
        if ext_ptrs:
            for i, p in enumerate(ext_ptrs):
                ext[i] = p if p else None
        b = N.fd_txn_batch(*[int(txn_ptrs[f]) for f in N.TXN_FIELDS])
        opt = lambda p: C.c_void_p(p) if p else None  # noqa: E731
        N.call("fd_score_batch_device", self._h, C.byref(params), _ptr(sl), ext, _ptr(pres), C.byref(b), int(n),
               opt(vec_ptr), opt(model_probs_ptr), C.c_void_p(fp_ptr), opt(conf_ptr), opt(dec_ptr), opt(risk_ptr))

    def score_batch_pipelined(self, params: N.fd_blend_params, slots: Sequence[int], txn_ptrs: dict, n: int,
                              fp_ptr: int, conf_ptr: int = 0, dec_ptr: int = 0, risk_ptr: int = 0,
                              model_probs_ptr: int = 0, ext_ptrs: Optional[Sequence[Optional[int]]] = None,
                              present: Optional[Sequence[int]] = None, input_ready: int = 0,
                              vec_ptr: int = 0) -> None:
        """Streaming form of score_batch_device (fd_score_batch_pipelined): the batch's features run on the
        engine's feature stream, overlapping the previous batch's forests; outputs are ordered on the engine
        stream as with score_batch_device (written there by a copy from engine staging, so the caller may free
        them in that stream's order). input_ready: a hipEvent_t handle (e.g. torch.cuda.Event's cuda_event)
        recorded when the input columns were complete; 0 = complete before this call. The input columns must
        stay unchanged until the engine stream has passed the call."""
        M = params.n_models
        sl = np.array(list(slots) + [-1] * (N.FD_MAX_MODELS - len(slots)), np.int32)
        pres = np.array([1] * M if present is None else list(present), np.uint8)
        ext = (C.c_void_p * N.FD_MAX_MODELS)()
        if ext_ptrs:
            for i, p in enumerate(ext_ptrs):
                ext[i] = p if p else None
        b = N.fd_txn_batch(*[int(txn_ptrs[f]) for f in N.TXN_FIELDS])
        opt = lambda p: C.c_void_p(p) if p else None  # noqa: E731
        N.call("fd_score_batch_pipelined", self._h, C.byref(params), _ptr(sl), ext, _ptr(pres), C.byref(b),
               int(n), opt(vec_ptr), opt(model_probs_ptr), C.c_void_p(fp_ptr), opt(conf_ptr), opt(dec_ptr),
               opt(risk_ptr), opt(input_ready))

    def pipelined_scorer(self, params: N.fd_blend_params, slots: Sequence[int],
                         present: Optional[Sequence[int]] = None) -> "PipelinedScorer":
        """A prepared score_batch_pipelined for a fixed model set: per call only the batch's pointers change
        (the per-step host cost stays well below the GPU step)."""
        return PipelinedScorer(self, params, slots, present)

    def batch_scorer(self, params: N.fd_blend_params, slots: Sequence[int],
                     present: Optional[Sequence[int]] = None) -> "PipelinedScorer":
        """The same prepared call over score_batch_device (one stream; small latency batches, where the
        per-call host cost is the step's bound)."""
        return PipelinedScorer(self, params, slots, present, pipelined=False)

    def features_seq_device(self, ptrs: dict, n: int, vec_ptr: int, seq_ptr: int, raw_ptr: int = 0) -> None:
        """features_device plus each transaction's LSTM input sequence (n x seq_len x 16 f32)."""
        b = N.fd_txn_batch(*[int(ptrs[f]) for f in N.TXN_FIELDS])
        N.call("fd_features_seq_device", self._h, C.byref(b), int(n), C.c_void_p(vec_ptr),
               C.c_void_p(raw_ptr) if raw_ptr else None, C.c_void_p(seq_ptr) if seq_ptr else None)

    # ------------------------------------------------------------------ full feature map + rule scores
    _USER_EXT_DT = {"risk_score": np.float64, "kyc_status": np.uint8, "verified": np.uint8, "pref_start": np.int8,
                    "pref_end": np.int8, "weekend_activity": np.float64, "online_preference": np.float64,
                    "intl_preference": np.float64, "txn_frequency": np.int32, "has_patterns": np.uint8}
    _MERCH_EXT_DT = {"avg_amount": np.float64, "risk_level": np.uint8, "blacklisted": np.uint8, "category": np.uint8,
                     "high_risk_category": np.uint8, "open_hour": np.uint8, "close_hour": np.uint8,
                     "suspicious_name": np.uint8}

    def load_users_ext(self, key, **fields) -> None:
        """Extended UserProfile fields (fd_users_ext); omitted fields are null."""
        keep = {"key": np.ascontiguousarray(key, np.uint64)}
        for f, dt in self._USER_EXT_DT.items():
            if fields.get(f) is not None:
                keep[f] = np.ascontiguousarray(fields[f], dt)
        u = N.fd_users_ext(len(keep["key"]), keep["key"].ctypes.data,
                           *[keep[f].ctypes.data if f in keep else None for f in N.USER_EXT_FIELDS])
        N.call("fd_state_load_users_ext_host", self._h, C.byref(u))

    def load_merchants_ext(self, n: int, **fields) -> None:
        keep = {f: np.ascontiguousarray(fields[f], dt) for f, dt in self._MERCH_EXT_DT.items()
                if fields.get(f) is not None}
        m = N.fd_merchants_ext(int(n), *[keep[f].ctypes.data if f in keep else None for f in N.MERCHANT_EXT_FIELDS])
        N.call("fd_load_merchants_ext_host", self._h, C.byref(m))

    def load_vocab(self, payment_high_risk, type_is_refund) -> None:
        a = np.ascontiguousarray(payment_high_risk, np.uint8)
        b = np.ascontiguousarray(type_is_refund, np.uint8)
        assert len(a) == 256 and len(b) == 256
        N.call("fd_load_vocab_host", self._h, _ptr(a), _ptr(b))

    def features_full_device(self, txn_ptrs: dict, ctx_ptrs: Optional[dict], n: int, vec_ptr: int, fmap_ptr: int = 0,
                             rules_ptr: int = 0, raw_ptr: int = 0) -> None:
        """features_device plus the 64-wide FeatureExtractor map (f64) and the rule scores
        (N.RULE_DTYPE records); ctx_ptrs: field -> device pointer (N.CTX_FIELDS), missing = null."""
        b = N.fd_txn_batch(*[int(txn_ptrs[f]) for f in N.TXN_FIELDS])
        cx = N.fd_txn_context(*[int(ctx_ptrs[f]) if ctx_ptrs and ctx_ptrs.get(f) else None for f in N.CTX_FIELDS])
        opt = lambda p: C.c_void_p(p) if p else None  # noqa: E731
        N.call("fd_features_full_device", self._h, C.byref(b), C.byref(cx), int(n), C.c_void_p(vec_ptr), opt(raw_ptr),
               opt(fmap_ptr), opt(rules_ptr))

    # ------------------------------------------------------------------ Flink window aggregates (a5)
    def windows_init(self, log_capacity: int, max_out_of_orderness_ms: int = 10000) -> None:
        """WindowProcessor's user-velocity (sliding 5 min / 1 min) and merchant (tumbling 1 h) windows
        (fl/windows/WindowProcessor.java:36-66); needs state_init (cards are keyed by its table)."""
        p = N.fd_window_params(int(log_capacity), int(max_out_of_orderness_ms))
        N.call("fd_windows_init", self._h, C.byref(p))

    def _windows_out(self, user_cap: int, merchant_cap: int):
        uo = np.zeros(max(int(user_cap), 1), N.USER_WINDOW_DTYPE)
        mo = np.zeros(max(int(merchant_cap), 1), N.MERCHANT_WINDOW_DTYPE)
        return uo, mo

    def windows_step_host(self, key, ts_ms, amount_cents, merchant, payment_method=None, is_fraud=None,
                          fraud_score=None, flush: bool = False, user_cap: int = 0, merchant_cap: int = 0):
        """Add one micro-batch (host arrays) and return (user windows, merchant windows) fired by it
        as numpy record arrays (N.USER_WINDOW_DTYPE / N.MERCHANT_WINDOW_DTYPE)."""
        n = len(key)
        keep = [np.ascontiguousarray(key, np.uint64), np.ascontiguousarray(ts_ms, np.int64),
                np.ascontiguousarray(amount_cents, np.int64), np.ascontiguousarray(merchant, np.int32)]
        b = N.fd_txn_batch(*[a.ctypes.data for a in keep], None, None, None, None)
        ins = [None if a is None else np.ascontiguousarray(a, dt)
               for a, dt in ((payment_method, np.uint8), (is_fraud, np.uint8), (fraud_score, np.float64))]
        wi = N.fd_window_inputs(*[None if a is None else a.ctypes.data for a in ins])
        held = self.windows_stats()
        ucap = user_cap or 5 * (n + held["user_events"]) + 16   # each event is in at most 5 user windows
        mcap = merchant_cap or n + held["merchant_events"] + 16
        uo, mo = self._windows_out(ucap, mcap)
        nu, nm = C.c_int64(), C.c_int64()
        N.call("fd_windows_step_host", self._h, C.byref(b), C.byref(wi), int(n), int(bool(flush)),
               uo.ctypes.data, int(ucap), C.byref(nu), mo.ctypes.data, int(mcap), C.byref(nm))
        return uo[:nu.value].copy(), mo[:nm.value].copy()

    def windows_step_device(self, txn_ptrs: dict, n: int, in_ptrs: Optional[dict] = None, flush: bool = False,
                            user_cap: int = 0, merchant_cap: int = 0):
        """Device-resident variant: txn_ptrs as features_device; in_ptrs: payment_method / is_fraud /
        fraud_score device pointers (missing = null)."""
        b = N.fd_txn_batch(*[int(txn_ptrs.get(f) or 0) or None for f in N.TXN_FIELDS])
        wi = N.fd_window_inputs(*[int(in_ptrs[f]) if in_ptrs and in_ptrs.get(f) else None
                                  for f in ("payment_method", "is_fraud", "fraud_score")])
        held = self.windows_stats()
        ucap = user_cap or 5 * (n + held["user_events"]) + 16   # each event is in at most 5 user windows
        mcap = merchant_cap or n + held["merchant_events"] + 16
        uo, mo = self._windows_out(ucap, mcap)
        nu, nm = C.c_int64(), C.c_int64()
        N.call("fd_windows_step_device", self._h, C.byref(b), C.byref(wi), int(n), int(bool(flush)),
               uo.ctypes.data, int(ucap), C.byref(nu), mo.ctypes.data, int(mcap), C.byref(nm))
        return uo[:nu.value].copy(), mo[:nm.value].copy()

    def windows_stats(self) -> dict:
        wm, ue, me = C.c_int64(), C.c_int64(), C.c_int64()
        N.call("fd_windows_stats", self._h, C.byref(wm), C.byref(ue), C.byref(me))
        return {"watermark": wm.value, "user_events": ue.value, "merchant_events": me.value}

    def windows_observe(self, max_event_ts: int) -> None:
        """Sharded windows: the node-wide micro-batch's largest event time (all-reduce MAX), so every shard
        advances one watermark (fd_windows_observe)."""
        N.call("fd_windows_observe", self._h, int(max_event_ts))

    # ------------------------------------------------------------------ RedisTransactionSink aggregates
    def sink_init(self, capacity: int, user_capacity: int) -> None:
        """Hourly / daily / merchant-hour summaries of RedisTransactionSink.updateAggregations
        (fl/sinks/RedisTransactionSink.java:140-262), HBM-resident."""
        p = N.fd_sink_params(int(capacity), int(user_capacity))
        N.call("fd_sink_init", self._h, C.byref(p))

    def sink_update_host(self, key, ts_ms, amount_cents, merchant, is_fraud=None, fraud_score=None) -> None:
        keep = [np.ascontiguousarray(key, np.uint64), np.ascontiguousarray(ts_ms, np.int64),
                np.ascontiguousarray(amount_cents, np.int64), np.ascontiguousarray(merchant, np.int32)]
        b = N.fd_txn_batch(*[a.ctypes.data for a in keep], None, None, None, None)
        fr = None if is_fraud is None else np.ascontiguousarray(is_fraud, np.uint8)
        fs = None if fraud_score is None else np.ascontiguousarray(fraud_score, np.float64)
        wi = N.fd_window_inputs(None, None if fr is None else fr.ctypes.data, None if fs is None else fs.ctypes.data)
        N.call("fd_sink_update_host", self._h, C.byref(b), C.byref(wi), len(keep[0]))

    def sink_update_device(self, txn_ptrs: dict, n: int, in_ptrs: Optional[dict] = None) -> None:
        b = N.fd_txn_batch(*[int(txn_ptrs.get(f) or 0) or None for f in N.TXN_FIELDS])
        wi = N.fd_window_inputs(None, *[int(in_ptrs[f]) if in_ptrs and in_ptrs.get(f) else None
                                        for f in ("is_fraud", "fraud_score")])
        N.call("fd_sink_update_device", self._h, C.byref(b), C.byref(wi), int(n))

    def sink_query(self, kind: int, buckets, merchants=None) -> np.ndarray:
        """RedisService.getAggregation for hourly / daily (bucket) or merchant (merchant, hour) keys."""
        bk = np.ascontiguousarray(buckets, np.int64)
        mk = None if merchants is None else np.ascontiguousarray(merchants, np.int32)
        out = np.zeros(len(bk), N.AGGREGATE_DTYPE)
        N.call("fd_sink_query_host", self._h, int(kind), _ptr(bk) if len(bk) else None,
               _ptr(mk) if mk is not None and len(mk) else None, len(bk), out.ctypes.data if len(bk) else None)
        return out

    def sink_evict_before(self, hour_key: int):
        a, b = C.c_int64(), C.c_int64()
        N.call("fd_sink_evict_before", self._h, int(hour_key), C.byref(a), C.byref(b))
        return a.value, b.value

    # ------------------------------------------------------------------ state snapshot / restore
    def state_snapshot(self, path, shard: int = 0, n_shards: int = 1) -> int:
        """Durable key-addressed image of the HBM keyed state (+ replicated tables, window logs);
        Flink keyed-state checkpoint / Redis RDB counterpart. Returns the bytes written."""
        nb = C.c_int64()
        N.call("fd_state_snapshot", self._h, os.fsencode(str(path)), int(shard), int(n_shards), C.byref(nb))
        return nb.value

    def state_restore(self, path, shard: int = 0, n_shards: int = 1, skip_windows: bool = False,
                      skip_sink: bool = False) -> int:
        """Re-insert an image's cards owned by `shard` of `n_shards` (any table capacity); returns the
        number of cards restored. Restore every old shard's image on each new shard to re-shard."""
        nc = C.c_int64()
        N.call("fd_state_restore", self._h, os.fsencode(str(path)), int(shard), int(n_shards),
               (N.FD_RESTORE_SKIP_WINDOWS if skip_windows else 0) | (N.FD_RESTORE_SKIP_SINK if skip_sink else 0),
               C.byref(nc))
        return nc.value

    # ------------------------------------------------------------------ LSTM head
    def load_lstm(self, model) -> None:
        """model: fdengine.lstm.LstmWeights (PyTorch layout, f32)."""
        keep = [np.ascontiguousarray(a, np.float32) if a is not None else None
                for a in (model.w_ih, model.w_hh, model.b_ih, model.b_hh, model.w_out, model.b_out)]
        ptr = [a.ctypes.data if a is not None else None for a in keep]
        p = N.fd_lstm_params(int(model.input_size), int(model.hidden), int(model.n_out), *ptr)
        N.call("fd_load_lstm", self._h, C.byref(p))
        self.lstm_info = {"input_size": model.input_size, "hidden": model.hidden, "n_out": model.n_out}

    def unload_lstm(self) -> None:
        N.call("fd_unload_lstm", self._h)
        self.lstm_info = None

    def lstm_predict(self, seq: np.ndarray) -> np.ndarray:
        """seq: [n, T, 16] (or [n, T, input_size], zero-padded here) -> P(fraud) f64 [n]."""
        seq = np.asarray(seq, np.float32)
        if seq.ndim != 3:
            raise ValueError(f"LSTM input must be [n, T, features], got shape {seq.shape}")
        n, T, I = seq.shape
        if I < N.FD_SEQ_INPUT:
            seq = np.concatenate([seq, np.zeros((n, T, N.FD_SEQ_INPUT - I), np.float32)], axis=2)
        seq = np.ascontiguousarray(seq)
        prob = np.empty(n, np.float64)
        N.call("fd_lstm_predict_host", self._h, _ptr(seq), n, T, _ptr(prob))
        return prob

    def lstm_predict_device(self, seq_ptr: int, n: int, T: int, prob_ptr: int) -> None:
        N.call("fd_lstm_predict_device", self._h, C.c_void_p(seq_ptr), int(n), int(T), C.c_void_p(prob_ptr))

    # ------------------------------------------------------------------ MLP head (graph_neural, model_type "pytorch")
    def load_mlp(self, model) -> None:
        """model: fdengine.mlp.MlpWeights (PyTorch nn.Linear layout, f32)."""
        p, keep = model.c_struct()
        N.call("fd_load_mlp", self._h, C.byref(p))
        del keep
        self.mlp_info = self.mlp_shape()

    def unload_mlp(self) -> None:
        N.call("fd_unload_mlp", self._h)
        self.mlp_info = None

    def mlp_shape(self) -> dict:
        L, i, h = C.c_int32(), C.c_int32(), C.c_int32()
        N.call("fd_mlp_info", self._h, C.byref(L), C.byref(i), C.byref(h))
        return {"n_layers": L.value, "in_dim": i.value, "hidden": h.value}

    def mlp_predict(self, X: np.ndarray) -> np.ndarray:
        """X: [n, ld] with ld >= in_dim (columns beyond in_dim are not read) -> softmax(model(X))[:, 1] as f64 [n]."""
        X = np.ascontiguousarray(X, np.float32)
        if X.ndim != 2:
            raise ValueError(f"MLP input must be [n, features], got shape {X.shape}")
        n, ld = X.shape
        prob = np.empty(n, np.float64)
        N.call("fd_mlp_predict_host", self._h, _ptr(X), n, ld, _ptr(prob))
        return prob

    def mlp_predict_device(self, x_ptr: int, n: int, ld: int, prob_ptr: int) -> None:
        N.call("fd_mlp_predict_device", self._h, C.c_void_p(x_ptr), int(n), int(ld), C.c_void_p(prob_ptr))

    # ------------------------------------------------------------------ training (the MLP member, mlp_fit.hip)
    def fit_mlp(self, X, y, *, hidden=64, n_layers=3, epochs=20, batch_size=256, optimizer="adam", lr=1e-3,
                betas=(0.9, 0.999), eps=1e-8, momentum=0.0, weight_decay=0.0, dropout=0.1, pos_weight=1.0, seed=0,
                init=None):
        """Fit the MLP member by minibatch training on the engine (fd_mlp_fit_*; the declared semantics are DESIGN
        §4.16). X: [n, in_dim <= 64] numpy (finite values), or a contiguous f32 torch tensor on this engine's device
        (then y a uint8 tensor there); y: 0 / 1. The model is in_dim -> hidden x (n_layers - 1) -> 2, started at
        mlp.random_weights(in_dim, hidden, n_layers, seed) or at init (an MlpWeights: a warm start; its shape then
        holds and hidden / n_layers are not read). optimizer "adam" (lr, betas, eps, weight_decay) or "sgd" (lr,
        momentum, weight_decay); dropout after every ReLU; pos_weight the weight of class 1 in the cross-entropy;
        seed fixes the batches and the masks. -> MlpWeights ready for load_mlp / mlp.save_state_dict, meta["loss_curve"]
        (one mean batch loss per epoch), meta["steps"] and the parameters under their names."""
        from . import mlp as M
        kw = dict(epochs=epochs, batch_size=batch_size, optimizer=optimizer, lr=lr, betas=tuple(betas), eps=eps,
                  momentum=momentum, weight_decay=weight_decay, dropout=dropout, pos_weight=pos_weight, seed=seed)
        if type(X).__module__.startswith("torch") and X.is_cuda:
            import torch
            if X.dtype != torch.float32 or X.dim() != 2 or not X.is_contiguous():
                raise ValueError("device input: a contiguous 2-d float32 tensor")
            y = y.to(device=X.device, dtype=torch.uint8).contiguous()
            n, ld = X.shape
            if y.numel() != n:
                raise ValueError("y: one 0 / 1 label per row of X")
            init = M._init_for(ld, hidden, n_layers, seed, init)
            torch.cuda.current_stream(X.device).synchronize()
            return M.run_fit("fd_mlp_fit_device", (self._h,), C.c_void_p(X.data_ptr()), C.c_void_p(y.data_ptr()), n,
                             ld, init, kw)
        X, y = M.fit_xy(X, y)
        init = M._init_for(X.shape[1], hidden, n_layers, seed, init)
        return M.run_fit("fd_mlp_fit_host", (self._h,), _ptr(X), _ptr(y), X.shape[0], X.shape[1], init, kw)

    def mlp_grad(self, w, X, y, masks=None, dropout: float = 0.0, pos_weight: float = 1.0):
        """Loss and gradients of the one batch (X, y) at w under masks, by the step kernel (fd_mlp_grad_host) ->
        (loss, MlpWeights of gradients); mlp.mlp_grad_ref_host is the host twin."""
        from . import mlp as M
        X, y = M.fit_xy(X, y)
        masks = M.check_masks(masks, w.n_layers, X.shape[0])
        return M.run_grad("fd_mlp_grad_host", (self._h,), _ptr(X), _ptr(y), _ptr(masks), X.shape[0], X.shape[1], w,
                          dropout, pos_weight)

    def mlp_fit_batch(self, n: int, epoch: int, step: int, *, n_layers: int = 3, **kw):
        """What a fit of n rows trains on, from the device (fd_mlp_fit_batch_device) -> (row order, masks);
        mlp.mlp_fit_batch_host is the host twin."""
        from . import mlp as M
        return M.run_batch("fd_mlp_fit_batch_device", (self._h,), n, epoch, step, n_layers, kw)

    # ------------------------------------------------------------------ transaction-network features (graph detector)
    def graph_init(self, max_history: int = 10000) -> None:
        """An empty transaction log of the reference's max_history_size (GraphFraudDetector, 2..65536)."""
        p = N.fd_graph_params(int(max_history))
        N.call("fd_graph_init", self._h, C.byref(p))

    def graph_clear(self) -> None:
        N.call("fd_graph_clear", self._h)

    def graph_info(self) -> dict:
        total, held = C.c_int64(), C.c_int64()
        N.call("fd_graph_info", self._h, C.byref(total), C.byref(held))
        return {"total": total.value, "held": held.value}

    def graph_step(self, card_key, merchant, amount_cents) -> np.ndarray:
        """Host columns in arrival order (card_key 0 = null user, merchant -1 = null merchant) -> f64 [n, 5] in
        fdengine._native.GRAPH_COLUMNS order; the rows enter the log."""
        cols = {"card_key": np.ascontiguousarray(card_key, np.uint64),
                "merchant": np.ascontiguousarray(merchant, np.int32),
                "amount_cents": np.ascontiguousarray(amount_cents, np.int64)}
        n = len(cols["card_key"])
        if len(cols["merchant"]) != n or len(cols["amount_cents"]) != n:
            raise ValueError("graph_step columns differ in length")
        out = np.empty((n, N.FD_GRAPH_FEATURES), np.float64)
        b = N.fd_txn_batch(**{f: c.ctypes.data for f, c in cols.items()})
        N.call("fd_graph_step_host", self._h, C.byref(b), n, _ptr(out))
        return out

    def graph_step_device(self, ptrs: dict, n: int, out_ptr: int) -> None:
        """ptrs: device pointers of card_key, merchant and amount_cents; out_ptr: f64 [n, 5]; on the engine stream."""
        b = N.fd_txn_batch(**{f: int(ptrs[f]) for f in ("card_key", "merchant", "amount_cents")})
        N.call("fd_graph_step_device", self._h, C.byref(b), int(n), C.c_void_p(out_ptr) if out_ptr else None)

    # ------------------------------------------------------------------ text patterns and features (text analyzer)
    def text_features(self, data, off):
        """Rows of four fields (fdengine._native.TEXT_FIELDS) as one byte blob (bytes or a uint8 array) and 4n + 1
        offsets -> (f64 [n, 14] in TEXT_COLUMNS order, uint8 [n] pattern bits in TEXT_PATTERNS order, uint8 [n]
        status). Rows with a non-ASCII byte have status FD_TEXT_NONASCII and zero outputs."""
        blob = np.frombuffer(data, np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) \
            else np.ascontiguousarray(data, np.uint8)
        off = np.ascontiguousarray(off, np.int64)
        if off.ndim != 1 or len(off) % 4 != 1:
            raise ValueError("text offsets must have 4 n + 1 entries")
        n = len(off) // 4
        if n and int(off[-1]) > len(blob):
            raise ValueError("text offsets reach past the blob")
        feat = np.empty((n, N.FD_TEXT_FEATURES), np.float64)
        patterns = np.empty(n, np.uint8)
        status = np.empty(n, np.uint8)
        b = N.fd_text_batch(blob.ctypes.data if len(blob) else None, off.ctypes.data)
        N.call("fd_text_features_host", self._h, C.byref(b), n, _ptr(feat), _ptr(patterns), _ptr(status))
        return feat, patterns, status

    def text_features_device(self, bytes_ptr: int, off_ptr: int, n: int, feat_ptr: int = 0, patterns_ptr: int = 0,
                             status_ptr: int = 0) -> None:
        """Device pointers (blob, int64 offsets; outputs f64 [n, 14], uint8 [n], uint8 [n], any of them 0 = not
        wanted); on the engine stream, nothing read back."""
        b = N.fd_text_batch(int(bytes_ptr) or None, int(off_ptr) or None)
        N.call("fd_text_features_device", self._h, C.byref(b), int(n), *(C.c_void_p(p) if p else None
                                                                        for p in (feat_ptr, patterns_ptr, status_ptr)))

    # ------------------------------------------------------------------ A/B tests (fdengine/ab_testing.py)
    def ab_create(self, test_id: int, salt: int, threshold: float) -> None:
        """An empty test under id 0..FD_AB_MAX_TESTS-1. salt: fd_hash64 of the test's name; threshold: the f64
        traffic_split * 100 (formed by the caller: buckets below it are treatment)."""
        p = N.fd_ab_params(int(salt), float(threshold))
        N.call("fd_ab_create", self._h, int(test_id), C.byref(p))

    def ab_destroy(self, test_id: int) -> None:
        N.call("fd_ab_destroy", self._h, int(test_id))

    def ab_clear(self, test_id: int) -> None:
        N.call("fd_ab_clear", self._h, int(test_id))

    def ab_assign(self, test_id: int, keys) -> np.ndarray:
        """uint64 user keys -> uint8 [n]: 0 control, 1 treatment."""
        keys = np.ascontiguousarray(keys, np.uint64)
        out = np.empty(len(keys), np.uint8)
        N.call("fd_ab_assign_host", self._h, int(test_id), _ptr(keys), len(keys), _ptr(out))
        return out

    def ab_assign_device(self, test_id: int, keys_ptr: int, n: int, variant_ptr: int) -> None:
        N.call("fd_ab_assign_device", self._h, int(test_id), C.c_void_p(keys_ptr), int(n), C.c_void_p(variant_ptr))

    def ab_partition(self, variant):
        """uint8 [n] variants -> (int32 [n] row indices: control rows in arrival order, then treatment rows in arrival
        order; int64 [2] rows per variant)."""
        variant = np.ascontiguousarray(variant, np.uint8)
        idx = np.empty(len(variant), np.int32)
        counts = np.empty(2, np.int64)
        N.call("fd_ab_partition_host", self._h, _ptr(variant), len(variant), _ptr(idx), _ptr(counts))
        return idx, counts

    def ab_partition_device(self, variant_ptr: int, n: int, idx_ptr: int, counts_ptr: int) -> None:
        N.call("fd_ab_partition_device", self._h, C.c_void_p(variant_ptr), int(n), C.c_void_p(idx_ptr),
               C.c_void_p(counts_ptr))

    @staticmethod
    def _ab_model_set(ms: dict, device: bool):
        """{"params", "slots", "ext_probs"?, "present"?} (score_matrix's arguments) -> (fd_ab_model_set, what it
        points into). ext_probs: arrays, or device pointers when `device`."""
        params = ms["params"]
        M = params.n_models
        slots = list(ms["slots"])
        sl = np.array(slots + [-1] * (N.FD_MAX_MODELS - len(slots)), np.int32)
        present = ms.get("present")
        pres = np.array([1] * M if present is None else list(present), np.uint8)
        ext = (C.c_void_p * N.FD_MAX_MODELS)()
        keep = [params, sl, pres, ext]
        cols = ms.get("ext_probs")
        for m in range(M):
            if sl[m] < 0 and pres[m]:
                if device:
                    ext[m] = int(cols[m])
                else:
                    col = np.ascontiguousarray(cols[m], dtype=np.float64)
                    keep.append(col)
                    ext[m] = col.ctypes.data
        s = N.fd_ab_model_set(C.addressof(params), sl.ctypes.data, C.addressof(ext), pres.ctypes.data)
        return s, keep

    def ab_score_matrix(self, test_id: int, control: dict, treatment: dict, X: np.ndarray, keys):
        """score_matrix with one model set per variant (each a dict of score_matrix's arguments: params, slots,
        ext_probs, present; ext_probs columns are n long, in X's row order). Row i is scored by the set of its user
        key's variant. -> (variant u8 [n], model_probs [max M, n] f64 with NaN where the row's set has fewer models,
        fraud_prob, confidence, decision u8, risk u8)."""
        X = np.ascontiguousarray(np.asarray(X, dtype=np.float32))
        n, ld = X.shape
        keys = np.ascontiguousarray(keys, np.uint64)
        if len(keys) != n:
            raise ValueError("one key per row")
        cs, keep_c = self._ab_model_set(control, False)
        ts, keep_t = self._ab_model_set(treatment, False)
        m_max = max(control["params"].n_models, treatment["params"].n_models)
        var = np.empty(n, np.uint8)
        mp = np.empty((m_max, n), np.float64)
        fp = np.empty(n, np.float64)
        conf = np.empty(n, np.float64)
        dec = np.empty(n, np.uint8)
        risk = np.empty(n, np.uint8)
        N.call("fd_ab_score_matrix_host", self._h, int(test_id), C.byref(cs), C.byref(ts), _ptr(X), _ptr(keys), n, ld,
               _ptr(var), _ptr(mp), _ptr(fp), _ptr(conf), _ptr(dec), _ptr(risk))
        del keep_c, keep_t
        return var, mp, fp, conf, dec, risk

    def ab_score_matrix_device(self, test_id: int, control: dict, treatment: dict, X_ptr: int, keys_ptr: int, n: int,
                               ld: int, fp_ptr: int, variant_ptr: int = 0, mp_ptr: int = 0, conf_ptr: int = 0,
                               dec_ptr: int = 0, risk_ptr: int = 0) -> None:
        """Device pointers (ext_probs entries too); waits once for the engine stream, reads two counts back."""
        cs, keep_c = self._ab_model_set(control, True)
        ts, keep_t = self._ab_model_set(treatment, True)
        opt = lambda p: C.c_void_p(p) if p else None  # noqa: E731
        N.call("fd_ab_score_matrix_device", self._h, int(test_id), C.byref(cs), C.byref(ts), C.c_void_p(X_ptr),
               C.c_void_p(keys_ptr), int(n), int(ld), opt(variant_ptr), opt(mp_ptr), C.c_void_p(fp_ptr), opt(conf_ptr),
               opt(dec_ptr), opt(risk_ptr))
        del keep_c, keep_t

    def ab_record(self, test_id: int, variant, prediction, decision, processing_time_ms, actual_fraud=None) -> None:
        """n results into the test's device state. processing_time_ms: an array, or one float for every row.
        actual_fraud: None (no labels) or uint8 [n] of 0, 1, FD_AB_NO_LABEL."""
        variant = np.ascontiguousarray(variant, np.uint8)
        n = len(variant)
        prediction = np.ascontiguousarray(prediction, np.float64)
        decision = np.ascontiguousarray(decision, np.uint8)
        scalar = np.ndim(processing_time_ms) == 0
        times = None if scalar else np.ascontiguousarray(processing_time_ms, np.float64)
        label = None if actual_fraud is None else np.ascontiguousarray(actual_fraud, np.uint8)
        for a in (prediction, decision, times, label):
            if a is not None and len(a) != n:
                raise ValueError("columns of different lengths")
        N.call("fd_ab_record_host", self._h, int(test_id), _ptr(variant), _ptr(prediction), _ptr(decision), _ptr(times),
               float(processing_time_ms) if scalar else 0.0, _ptr(label), n)

    def ab_record_device(self, test_id: int, variant_ptr: int, prediction_ptr: int, decision_ptr: int, n: int,
                         time_ptr: int = 0, time_scalar: float = 0.0, label_ptr: int = 0) -> None:
        """Device pointers, on the engine stream, nothing read back. time_ptr 0: time_scalar for every row."""
        N.call("fd_ab_record_device", self._h, int(test_id), C.c_void_p(variant_ptr), C.c_void_p(prediction_ptr),
               C.c_void_p(decision_ptr), C.c_void_p(time_ptr) if time_ptr else None, float(time_scalar),
               C.c_void_p(label_ptr) if label_ptr else None, int(n))

    def ab_state(self, test_id: int) -> N.fd_ab_state:
        """The test's two accumulators (waits for the engine stream)."""
        out = N.fd_ab_state()
        N.call("fd_ab_state_host", self._h, int(test_id), C.byref(out))
        return out

    # ------------------------------------------------------------------ prediction metrics (fdengine/monitoring.py)
    def metrics_init(self, n_models: int = N.FD_METRICS_MAX_MODELS, slots: int = 4096) -> None:
        """An empty collector on this engine: at most n_models model columns per record call, a ring of `slots` time
        slots for the hour / minute windows."""
        p = N.fd_metrics_params(int(n_models), int(slots))
        N.call("fd_metrics_init", self._h, C.byref(p))

    def metrics_clear(self) -> None:
        N.call("fd_metrics_clear", self._h)

    def metrics_record(self, fraud_prob, decision, model_probs, processing_time_ms, timestamp: float) -> None:
        """n rows under one timestamp, from host columns. model_probs: None or f64 [n_models, n] (a model's column is
        a row of it), NaN where a row has no such model. processing_time_ms: an array, or one float for every row."""
        fraud_prob = np.ascontiguousarray(fraud_prob, np.float64)
        n = len(fraud_prob)
        decision = np.ascontiguousarray(decision, np.uint8)
        mp = None if model_probs is None else np.ascontiguousarray(model_probs, np.float64).reshape(-1, n)
        n_models = 0 if mp is None else mp.shape[0]
        scalar = np.ndim(processing_time_ms) == 0
        times = None if scalar else np.ascontiguousarray(processing_time_ms, np.float64)
        for a in (decision, times):
            if a is not None and len(a) != n:
                raise ValueError("columns of different lengths")
        N.call("fd_metrics_record_host", self._h, _ptr(fraud_prob), _ptr(decision), _ptr(mp) if n_models else None,
               n_models, _ptr(times), float(processing_time_ms) if scalar else 0.0, float(timestamp), n)

    def metrics_record_device(self, fraud_prob_ptr: int, decision_ptr: int, n: int, timestamp: float,
                              model_probs_ptr: int = 0, n_models: int = 0, time_ptr: int = 0,
                              time_scalar: float = 0.0) -> None:
        """Device pointers (fd_score_matrix_device's outputs as they are), on the engine stream, nothing read back.
        time_ptr 0: time_scalar for every row."""
        opt = lambda p: C.c_void_p(p) if p else None  # noqa: E731
        N.call("fd_metrics_record_device", self._h, C.c_void_p(fraud_prob_ptr), C.c_void_p(decision_ptr),
               opt(model_probs_ptr), int(n_models), opt(time_ptr), float(time_scalar), float(timestamp), int(n))

    def metrics_query(self, now: float) -> N.fd_metrics_summary:
        """The cumulative part and the hour / minute windows at `now` (waits for the engine stream)."""
        out = N.fd_metrics_summary()
        N.call("fd_metrics_query_host", self._h, float(now), C.byref(out))
        return out

    # ------------------------------------------------------------------ card-hash sharding (fdengine/sharding.py)
    def route_partition_device(self, txn_ptrs: dict, n: int, n_shards: int, records_ptr: int, counts_ptr: int) -> None:
        """Group one device-resident micro-batch by owner GPU: n records of FD_ROUTE_RECORD_BYTES at
        records_ptr (owner-major, arrival order kept), n_shards int64 counts at counts_ptr."""
        b = N.fd_txn_batch(*[int(txn_ptrs[f]) for f in N.TXN_FIELDS])
        N.call("fd_route_partition_device", self._h, C.byref(b), int(n), int(n_shards),
               C.c_void_p(records_ptr) if records_ptr else None, C.c_void_p(counts_ptr))

    def route_partition_ex_device(self, txn_ptrs: dict, extra_ptrs: Optional[dict], n: int, n_shards: int,
                                  records_ptr: int, counts_ptr: int) -> None:
        """route_partition_device with the owner's window / sink inputs riding in the records:
        extra_ptrs = {"payment_method": u8*, "is_fraud": u8*} device pointers (missing: null / false)."""
        b = N.fd_txn_batch(*[int(txn_ptrs[f]) for f in N.TXN_FIELDS])
        wi = N.fd_window_inputs(*[int(extra_ptrs[f]) if extra_ptrs and extra_ptrs.get(f) else None
                                  for f in ("payment_method", "is_fraud")], None)
        N.call("fd_route_partition_ex_device", self._h, C.byref(b), C.byref(wi), int(n), int(n_shards),
               C.c_void_p(records_ptr) if records_ptr else None, C.c_void_p(counts_ptr))

    def route_partition_stream(self, txn_ptrs: dict, extra_ptrs: Optional[dict], n: int, n_shards: int,
                               records_ptr: int, counts_ptr: int, stream_ptr: int) -> None:
        """route_partition_ex_device launched on `stream_ptr` (a hipStream_t), beside the pipelined stream."""
        b = N.fd_txn_batch(*[int(txn_ptrs[f]) for f in N.TXN_FIELDS])
        wi = N.fd_window_inputs(*[int(extra_ptrs[f]) if extra_ptrs and extra_ptrs.get(f) else None
                                  for f in ("payment_method", "is_fraud")], None)
        N.call("fd_route_partition_stream", self._h, C.byref(b), C.byref(wi), int(n), int(n_shards),
               C.c_void_p(records_ptr) if records_ptr else None, C.c_void_p(counts_ptr),
               C.c_void_p(int(stream_ptr)) if stream_ptr else None)

    def route_unpack_device(self, records_ptr: int, results_ptr: int, n: int, out_ptrs: dict, pm_ptr: int = 0,
                            fraud_ptr: int = 0, score_ptr: int = 0) -> None:
        """Owner side: received records (+ their result records) back to device columns (out_ptrs: any of
        TXN_FIELDS), payment method, isFraud and the fraud score (the result's fraud probability)."""
        opt = lambda p: C.c_void_p(p) if p else None  # noqa: E731
        b = N.fd_txn_batch(*[int(out_ptrs.get(f) or 0) or None for f in N.TXN_FIELDS])
        N.call("fd_route_unpack_device", self._h, opt(records_ptr), opt(results_ptr), int(n), C.byref(b),
               opt(pm_ptr), opt(fraud_ptr), opt(score_ptr))

    def score_records_device(self, params: N.fd_blend_params, slots: Sequence[int], records_ptr: int, n: int,
                             results_ptr: int, present: Optional[Sequence[int]] = None) -> None:
        """Owner side: features (this GPU's card state) -> forests -> blend over n received records;
        n result records of FD_RESULT_RECORD_BYTES at results_ptr."""
        M = params.n_models
        sl = np.array(list(slots) + [-1] * (N.FD_MAX_MODELS - len(slots)), np.int32)
        pres = np.array([1] * M if present is None else list(present), np.uint8)
        N.call("fd_score_records_device", self._h, C.byref(params), _ptr(sl), _ptr(pres),
               C.c_void_p(records_ptr) if records_ptr else None, int(n),
               C.c_void_p(results_ptr) if results_ptr else None)

    def score_records_pipelined(self, params: N.fd_blend_params, slots: Sequence[int], records_ptr: int, n: int,
                                results_ptr: int, input_ready: int = 0, present: Optional[Sequence[int]] = None) -> None:
        """Streaming form of score_records_device (fd_score_records_pipelined): the owner's features of this batch
        overlap the previous batch's forests; input_ready: a hipEvent_t recorded once the records had landed."""
        M = params.n_models
        sl = np.array(list(slots) + [-1] * (N.FD_MAX_MODELS - len(slots)), np.int32)
        pres = np.array([1] * M if present is None else list(present), np.uint8)
        N.call("fd_score_records_pipelined", self._h, C.byref(params), _ptr(sl), _ptr(pres),
               C.c_void_p(records_ptr) if records_ptr else None, int(n),
               C.c_void_p(results_ptr) if results_ptr else None, C.c_void_p(input_ready) if input_ready else None)

    # ---- card-hash sharding over the engine's own RCCL communicators (fd_comm_* / fd_sharded_step)
    @staticmethod
    def comm_unique_id(rccl_path: str) -> bytes:
        buf = (C.c_uint8 * 128)()
        N.call("fd_comm_unique_id", os.fsencode(rccl_path), C.cast(buf, C.c_void_p))
        return bytes(buf)

    def comm_init(self, rccl_path: str, rank: int, world: int, id_fwd: bytes, id_back: bytes) -> None:
        a = (C.c_uint8 * 128).from_buffer_copy(id_fwd)
        b = (C.c_uint8 * 128).from_buffer_copy(id_back)
        N.call("fd_comm_init", self._h, os.fsencode(rccl_path), int(rank), int(world), C.cast(a, C.c_void_p),
               C.cast(b, C.c_void_p))

    def comm_destroy(self) -> None:
        N.call("fd_comm_destroy", self._h)

    def sharded_scorer(self, params: N.fd_blend_params, slots: Sequence[int],
                       present: Optional[Sequence[int]] = None) -> "ShardedStep":
        """fd_sharded_step with its model arguments marshalled once"""
        return ShardedStep(self, params, slots, present)

    def route_scatter_results_device(self, results_ptr: int, n: int, fp_ptr: int, conf_ptr: int = 0,
                                     dec_ptr: int = 0, risk_ptr: int = 0) -> None:
        """Ingest side: put the n returned result records back in micro-batch order."""
        opt = lambda p: C.c_void_p(p) if p else None  # noqa: E731
        N.call("fd_route_scatter_results_device", self._h, opt(results_ptr), int(n), opt(fp_ptr), opt(conf_ptr),
               opt(dec_ptr), opt(risk_ptr))

    # ------------------------------------------------------------------ blend
    @staticmethod
    def blend_params(weights: Sequence[float], conf_mult: Sequence[float], strategy: int = 0,
                     fraud_threshold: float = 0.5, confidence_threshold: float = 0.7) -> N.fd_blend_params:
        p = N.fd_blend_params()
        p.n_models = len(weights)
        p.strategy = int(strategy)
        for i, (w, m) in enumerate(zip(weights, conf_mult)):
            p.weight[i] = float(w)
            p.conf_mult[i] = float(m)
        p.fraud_threshold = float(fraud_threshold)
        p.confidence_threshold = float(confidence_threshold)
        return p

    def blend(self, params: N.fd_blend_params, probs: Sequence[Optional[np.ndarray]]):
        """probs[m]: f64 [n] or None (model failed -> dropped). -> (fraud_prob, confidence, decision u8, risk u8)."""
        M = params.n_models
        assert len(probs) == M
        n = next((len(p) for p in probs if p is not None), 0)
        cols = [None if p is None else np.ascontiguousarray(p, dtype=np.float64) for p in probs]
        present = np.array([0 if c is None else 1 for c in cols], np.uint8)
        arr = (C.c_void_p * N.FD_MAX_MODELS)()
        for i, c in enumerate(cols):
            arr[i] = None if c is None else c.ctypes.data
        fp = np.empty(n, np.float64)
        conf = np.empty(n, np.float64)
        dec = np.empty(n, np.uint8)
        risk = np.empty(n, np.uint8)
        N.call("fd_blend_host", self._h, C.byref(params), n, arr, _ptr(present), _ptr(fp), _ptr(conf),
               _ptr(dec), _ptr(risk))
        return fp, conf, dec, risk

    def score_matrix(self, params: N.fd_blend_params, slots: Sequence[int], X: np.ndarray,
                     ext_probs: Optional[Sequence[Optional[np.ndarray]]] = None,
                     present: Optional[Sequence[int]] = None):
        """Every forest model (slots[m] >= 0) scores X, external columns fill the rest, then blend.
        -> (model_probs [M, n] f64, fraud_prob, confidence, decision u8, risk u8)."""
        X = np.ascontiguousarray(np.asarray(X, dtype=np.float32))
        n, ld = X.shape
        M = params.n_models
        sl = np.array(list(slots) + [-1] * (N.FD_MAX_MODELS - len(slots)), np.int32)
        pres = np.array([1] * M if present is None else list(present), np.uint8)
        ext = (C.c_void_p * N.FD_MAX_MODELS)()
        keep = []
        for m in range(M):
            if sl[m] < 0 and pres[m]:
                col = np.ascontiguousarray(ext_probs[m], dtype=np.float64)
                keep.append(col)
                ext[m] = col.ctypes.data
        mp = np.empty((M, n), np.float64)
        fp = np.empty(n, np.float64)
        conf = np.empty(n, np.float64)
        dec = np.empty(n, np.uint8)
        risk = np.empty(n, np.uint8)
        N.call("fd_score_matrix_host", self._h, C.byref(params), _ptr(sl), ext, _ptr(pres), _ptr(X), n, ld,
               _ptr(mp), _ptr(fp), _ptr(conf), _ptr(dec), _ptr(risk))
        return mp, fp, conf, dec, risk

    def score_matrix_device(self, params: N.fd_blend_params, slots: Sequence[int], X_ptr: int, n: int, ld: int,
                            fp_ptr: int, mp_ptr: int = 0, conf_ptr: int = 0, dec_ptr: int = 0,
                            risk_ptr: int = 0) -> None:
        """score_matrix on device pointers, every model a loaded forest (slots[m] >= 0): enqueued on the engine
        stream, nothing read back. mp_ptr: f64 [n_models, n]."""
        sl = np.array(list(slots) + [-1] * (N.FD_MAX_MODELS - len(slots)), np.int32)
        if (sl[:params.n_models] < 0).any():
            raise ValueError("score_matrix_device takes forest slots only")
        ext = (C.c_void_p * N.FD_MAX_MODELS)()
        opt = lambda p: C.c_void_p(p) if p else None  # noqa: E731
        N.call("fd_score_matrix_device", self._h, C.byref(params), _ptr(sl), ext, None, C.c_void_p(X_ptr), int(n),
               int(ld), opt(mp_ptr), C.c_void_p(fp_ptr), opt(conf_ptr), opt(dec_ptr), opt(risk_ptr))

    def blend_device(self, params: N.fd_blend_params, n: int, prob_ptrs: Sequence[Optional[int]],
                     fp_ptr: int, conf_ptr: int = 0, dec_ptr: int = 0, risk_ptr: int = 0) -> None:
        present = np.array([0 if p is None else 1 for p in prob_ptrs], np.uint8)
        arr = (C.c_void_p * N.FD_MAX_MODELS)()
        for i, p in enumerate(prob_ptrs):
            arr[i] = p if p else None
        N.call("fd_blend_device", self._h, C.byref(params), int(n), arr, _ptr(present), C.c_void_p(fp_ptr),
               C.c_void_p(conf_ptr) if conf_ptr else None, C.c_void_p(dec_ptr) if dec_ptr else None,
               C.c_void_p(risk_ptr) if risk_ptr else None)


def pack_forest_host(fa: ForestArrays):
    """Host-only repack (no GPU): -> (blob bytes, leaf_ids int32, fd_pack_info)."""
    p, t, keep = fa.c_structs()
    info = N.fd_pack_info()
    N.call("fd_pack_forest_host", C.byref(p), C.byref(t), None, 0, None, 0, C.byref(info))
    blob = np.empty(info.blob_bytes, np.uint8)
    ids = np.empty(info.n_leaf_ids, np.int32)
    N.call("fd_pack_forest_host", C.byref(p), C.byref(t), C.c_void_p(blob.ctypes.data), info.blob_bytes,
           C.c_void_p(ids.ctypes.data), info.n_leaf_ids, C.byref(info))
    del keep
    return blob.tobytes(), ids, info


def contract_forest_host(fa: ForestArrays):
    """Host-only (no GPU): the forest with every split on a constant slot of the compact scoring vector resolved
    (fd_contract_forest_host) -> (ForestArrays, depths int32 [n_trees], splits pruned)."""
    p, t, keep = fa.c_structs()
    nn, pruned = C.c_int64(), C.c_int64()
    N.call("fd_contract_forest_host", C.byref(p), C.byref(t), C.byref(nn), None, None, None)
    T, M = fa.n_trees, nn.value
    out = ForestArrays(kind=fa.kind, num_feature=fa.num_feature, offsets=np.zeros(T + 1, np.int64),
                       left=np.zeros(M, np.int32), right=np.zeros(M, np.int32), feature=np.zeros(M, np.int32),
                       threshold=np.zeros(M, np.float64), default_left=np.zeros(M, np.uint8),
                       leaf_value=np.zeros(M, np.float64), base_score=fa.base_score, if_offset=fa.if_offset,
                       if_denominator=fa.if_denominator)
    _, to, ko = out.c_structs()
    depths = np.zeros(T, np.int32)
    N.call("fd_contract_forest_host", C.byref(p), C.byref(t), C.byref(nn), C.byref(to),
           depths.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(pruned))
    del keep
    for name in ("offsets", "left", "right", "feature", "threshold", "default_left", "leaf_value"):
        setattr(out, name, ko[name])
    return out, depths, pruned.value


def dense_layout_host(fa: ForestArrays, wide: bool = True, mode: int = 4, owner_bias: int = 0):
    """Host-only (no GPU): the dense chunk layout of the contracted forest, as the fused kernel walks it under
    ensemble_contract 3 / 4 (fd_dense_layout_host; the chunk table and the node word: include/fdengine.h) -> dict of
    blob (uint8), chunk_offsets (int64), chunk_lengths (int32), trees (structured: chunk, bundle, group, depth,
    node_offset, leaf_offset), thresholds (f32) with thr_offsets (int32 [num_feature + 1]), and info (fd_dense_info)."""
    p, t, keep = fa.c_structs()
    info = N.fd_dense_info()
    args = (C.byref(p), C.byref(t), int(bool(wide)), int(mode), int(owner_bias), C.byref(info))
    N.call("fd_dense_layout_host", *args, None, None, None, None, None, None)
    blob = np.zeros(info.blob_bytes, np.uint8)
    offs = np.zeros(info.n_chunks, np.int64)
    lens = np.zeros(info.n_chunks, np.int32)
    trees = np.zeros(fa.n_trees, np.dtype([(k, np.int32) for k in ("chunk", "bundle", "group", "depth", "node_offset",
                                                                   "leaf_offset")]))
    thr = np.zeros(info.n_thresholds, np.float32)
    thr_off = np.zeros(fa.num_feature + 1, np.int32)
    N.call("fd_dense_layout_host", *args, *[C.c_void_p(x.ctypes.data) for x in (blob, offs, lens, trees, thr, thr_off)])
    del keep
    return dict(blob=blob, chunk_offsets=offs, chunk_lengths=lens, trees=trees, thresholds=thr, thr_offsets=thr_off,
                info=info)


def pack_forest_binned_host(fa: ForestArrays):
    """Host-only binned repack (no GPU): -> (blob bytes, thresholds f32, offsets int32, fd_pack_info).
    Raises NativeError(FD_ERR_UNSUPPORTED) when a feature has more than 65534 distinct thresholds."""
    p, t, keep = fa.c_structs()
    info = N.fd_pack_info()
    N.call("fd_pack_forest_binned_host", C.byref(p), C.byref(t), None, 0, None, 0, None, C.byref(info))
    blob = np.empty(info.blob_bytes, np.uint8)
    thr = np.empty(info.n_thresholds, np.float32)
    off = np.empty(fa.num_feature + 1, np.int32)
    N.call("fd_pack_forest_binned_host", C.byref(p), C.byref(t), C.c_void_p(blob.ctypes.data), info.blob_bytes,
           C.c_void_p(thr.ctypes.data), info.n_thresholds, C.c_void_p(off.ctypes.data), C.byref(info))
    del keep
    return blob.tobytes(), thr, off, info


def pack_forest_sparse_host(fa: ForestArrays):
    """Host-only sparse repack (no GPU; trees of any depth): -> (nodes uint32 [n_nodes, 2] {f32 threshold bits, meta},
    leaf values f32 / f64 [n_leaves], leaf ids int32 [n_leaves], fd_sparse_info). Words: include/fdengine.h."""
    p, t, keep = fa.c_structs()
    info = N.fd_sparse_info()
    N.call("fd_pack_forest_sparse_host", C.byref(p), C.byref(t), None, 0, None, 0, None, 0, C.byref(info))
    nodes = np.empty((info.n_nodes, 2), np.uint32)
    vals = np.empty(info.n_leaves, np.float32 if info.leaf_bytes == 4 else np.float64)
    ids = np.empty(info.n_leaves, np.int32)
    N.call("fd_pack_forest_sparse_host", C.byref(p), C.byref(t), C.c_void_p(nodes.ctypes.data), info.n_nodes,
           C.c_void_p(vals.ctypes.data), info.n_leaves, C.c_void_p(ids.ctypes.data), info.n_leaves, C.byref(info))
    del keep
    return nodes, vals, ids, info


def _cover_of(fa: ForestArrays) -> np.ndarray:
    if fa.cover is None:
        raise ValueError("the forest carries no covers (ForestArrays.cover): attribution needs them")
    return np.ascontiguousarray(fa.cover, dtype=np.float64)


def shap_paths_host(fa: ForestArrays):
    """Host-only: the TreeSHAP path table of a forest (fd_shap_paths_host) -> (paths, elems, fd_shap_info), two
    numpy record arrays with the fields of fd_shap_path / fd_shap_elem (include/fdengine.h)."""
    p, t, keep = fa.c_structs()
    cover = _cover_of(fa)
    info = N.fd_shap_info()
    N.call("fd_shap_paths_host", C.byref(p), C.byref(t), _ptr(cover), None, 0, None, 0, C.byref(info))
    paths = np.zeros(info.n_paths, np.dtype(N.fd_shap_path))
    elems = np.zeros(info.n_elems, np.dtype(N.fd_shap_elem))
    N.call("fd_shap_paths_host", C.byref(p), C.byref(t), _ptr(cover), _ptr(paths), info.n_paths, _ptr(elems),
           info.n_elems, C.byref(info))
    del keep
    return paths, elems, info


def shap_ref_host(fa: ForestArrays, X: np.ndarray) -> np.ndarray:
    """Host-only: recursive TreeSHAP on the trees (fd_forest_shap_ref_host) -> phi f64 [n, num_feature + 1]."""
    p, t, keep = fa.c_structs()
    cover = _cover_of(fa)
    X = np.ascontiguousarray(np.asarray(X, dtype=np.float32))
    if X.ndim == 1:
        X = X.reshape(1, -1)
    n, ld = X.shape
    phi = np.zeros((n, fa.num_feature + 1), np.float64)
    N.call("fd_forest_shap_ref_host", C.byref(p), C.byref(t), _ptr(cover), _ptr(X), n, ld, _ptr(phi),
           fa.num_feature + 1)
    del keep
    return phi


def read_xgboost_json_cover_native(path) -> np.ndarray:
    """Host-only: the sum_hessian arrays of an XGBoost JSON file as the engine's C++ reader keeps them."""
    nn = C.c_int64()
    N.call("fd_xgboost_json_read_cover", os.fsencode(str(path)), None, 0, C.byref(nn))
    cover = np.zeros(nn.value, np.float64)
    N.call("fd_xgboost_json_read_cover", os.fsencode(str(path)), _ptr(cover), nn.value, C.byref(nn))
    return cover


def read_xgboost_json_native(path) -> ForestArrays:
    """Host-only: the engine's C++ reader of the XGBoost JSON file (fd_xgboost_json_read), as ForestArrays."""
    p = N.fd_forest_params()
    nt, nn = C.c_int32(), C.c_int64()
    N.call("fd_xgboost_json_read", os.fsencode(str(path)), C.byref(p), C.byref(nt), C.byref(nn), None)
    T, M = nt.value, nn.value
    fa = ForestArrays(kind=p.kind, num_feature=p.num_feature, offsets=np.zeros(T + 1, np.int64),
                      left=np.zeros(M, np.int32), right=np.zeros(M, np.int32), feature=np.zeros(M, np.int32),
                      threshold=np.zeros(M, np.float64), default_left=np.zeros(M, np.uint8),
                      leaf_value=np.zeros(M, np.float64), base_score=p.base_score)
    _, t, keep = fa.c_structs()
    N.call("fd_xgboost_json_read", os.fsencode(str(path)), C.byref(p), C.byref(nt), C.byref(nn), C.byref(t))
    out = ForestArrays(kind=fa.kind, num_feature=fa.num_feature, offsets=keep["offsets"], left=keep["left"],
                       right=keep["right"], feature=keep["feature"], threshold=keep["threshold"],
                       default_left=keep["default_left"], leaf_value=keep["leaf_value"], base_score=p.base_score)
    return out


# ------------------------------------------------------------------------------------------- training (gbdt.hip)

GBDT_DEFAULTS = dict(n_rounds=100, max_depth=6, max_bin=256, eta=0.1, reg_lambda=1.0, min_child_weight=1.0,
                     subsample=1.0, colsample_bytree=1.0, base_score=0.5, seed=0)


def gbdt_params(**kw) -> "N.fd_gbdt_params":
    """fd_gbdt_params from keywords (GBDT_DEFAULTS; XGBClassifier's names n_estimators / learning_rate / random_state
    are accepted for n_rounds / eta / seed)."""
    alias = {"n_estimators": "n_rounds", "learning_rate": "eta", "random_state": "seed", "lambda_": "reg_lambda"}
    v = dict(GBDT_DEFAULTS)
    for k, x in kw.items():
        k = alias.get(k, k)
        if k not in v:
            raise TypeError(f"unknown GBDT parameter {k!r}")
        v[k] = x
    return N.fd_gbdt_params(int(v["n_rounds"]), int(v["max_depth"]), int(v["max_bin"]), 0, float(v["eta"]),
                            float(v["reg_lambda"]), float(v["min_child_weight"]), float(v["subsample"]),
                            float(v["colsample_bytree"]), float(v["base_score"]), int(v["seed"]) & (2 ** 64 - 1))


class _GbdtOut:
    """Caller arrays of an fd_gbdt_model with room for `cap` nodes of `n_trees` trees."""

    def __init__(self, n_trees: int, cap: int):
        self.a = dict(offsets=np.zeros(n_trees + 1, np.int64), left=np.zeros(cap, np.int32),
                      right=np.zeros(cap, np.int32), feature=np.zeros(cap, np.int32),
                      threshold=np.zeros(cap, np.float64), default_left=np.zeros(cap, np.uint8),
                      leaf_value=np.zeros(cap, np.float64), sum_hessian=np.zeros(cap, np.float64),
                      loss_changes=np.zeros(cap, np.float64), base_weights=np.zeros(cap, np.float64))
        a = self.a

        def P(x, t):
            return x.ctypes.data_as(C.POINTER(t))

        self.trees = N.fd_tree_arrays(n_trees, P(a["offsets"], C.c_int64), P(a["left"], C.c_int32),
                                      P(a["right"], C.c_int32), P(a["feature"], C.c_int32),
                                      P(a["threshold"], C.c_double), P(a["default_left"], C.c_uint8),
                                      P(a["leaf_value"], C.c_double))
        self.model = N.fd_gbdt_model(C.pointer(self.trees), a["sum_hessian"].ctypes.data,
                                     a["loss_changes"].ctypes.data, a["base_weights"].ctypes.data)

    def forest(self, n_nodes: int, num_feature: int, base_score: float) -> ForestArrays:
        a = {k: (v if k == "offsets" else v[:n_nodes].copy()) for k, v in self.a.items()}
        return ForestArrays(kind=N.FD_FOREST_XGB_BINARY_LOGISTIC, num_feature=num_feature, offsets=a["offsets"],
                            left=a["left"], right=a["right"], feature=a["feature"], threshold=a["threshold"],
                            default_left=a["default_left"], leaf_value=a["leaf_value"], base_score=base_score,
                            cover=a["sum_hessian"],
                            meta={"n_trees": len(a["offsets"]) - 1, "sum_hessian": a["sum_hessian"],
                                  "loss_changes": a["loss_changes"], "base_weights": a["base_weights"]})


def _gbdt_xy(X, y):
    X = np.ascontiguousarray(np.asarray(X, dtype=np.float32))
    if X.ndim != 2:
        raise ValueError("X: a 2-d matrix")
    yy = np.asarray(y)
    if yy.shape != (X.shape[0],):
        raise ValueError("y: one label per row of X")
    if not np.isin(yy, (0, 1)).all():
        raise ValueError("labels must be 0 or 1")
    return X, np.ascontiguousarray(yy.astype(np.uint8))


def _gbdt_fit(fn: str, head, X, y, p):
    """The two calls of fd_gbdt_fit_*: the capacity, then the fit -> ForestArrays with .meta['margins']."""
    n, ld = X.shape
    cap = C.c_int64()
    N.call(fn, *head, _ptr(X), _ptr(y), n, ld, ld, C.byref(p), None, C.byref(cap), None)
    out = _GbdtOut(p.n_rounds, cap.value)
    margins = np.zeros(n, np.float32)
    nn = C.c_int64()
    N.call(fn, *head, _ptr(X), _ptr(y), n, ld, ld, C.byref(p), C.byref(out.model), C.byref(nn), _ptr(margins))
    fa = out.forest(nn.value, ld, p.base_score)
    fa.meta["margins"] = margins
    return fa


GBDT_METRICS = {"auc": N.FD_GBDT_METRIC_AUC, "error": N.FD_GBDT_METRIC_ERROR}


def _gbdt_metric_id(metric) -> int:
    if metric not in GBDT_METRICS:
        raise ValueError(f"eval_metric must be one of {sorted(GBDT_METRICS)}, not {metric!r}")
    return GBDT_METRICS[metric]


def _gbdt_eval_struct(eval_set, eval_metric, early_stopping_rounds, scale_pos_weight, p, n, F, device=None):
    """fd_gbdt_eval for a fit of n rows x F columns, with its output arrays (numpy, or torch tensors on `device`)
    -> (struct, the arrays it points into)."""
    if isinstance(eval_set, list):
        if len(eval_set) > 1:
            raise ValueError("one eval set at most")
        eval_set = eval_set[0] if eval_set else None
    k = 0 if early_stopping_rounds is None else int(early_stopping_rounds)
    if k < 0:
        raise ValueError("early_stopping_rounds must be >= 0")
    keep = {"curve": np.zeros(p.n_rounds, np.float64)}
    ev = N.fd_gbdt_eval()
    ev.metric = _gbdt_metric_id(eval_metric)
    ev.early_stopping_rounds = k
    ev.scale_pos_weight = float(scale_pos_weight)
    ev.metric_out = keep["curve"].ctypes.data
    if eval_set is not None:
        Xe, ye = eval_set
        if device is not None:
            import torch
            if not (type(Xe).__module__.startswith("torch") and Xe.is_cuda and Xe.dtype == torch.float32
                    and Xe.dim() == 2 and Xe.is_contiguous()):
                raise ValueError("device input: the eval matrix is a contiguous 2-d float32 tensor there too")
            ye = ye.to(device=device, dtype=torch.uint8).contiguous()
            if ye.shape != (Xe.shape[0],):
                raise ValueError("y: one label per row of X")
            keep.update(X=Xe, y=ye, eval_margins=torch.zeros(Xe.shape[0], dtype=torch.float32, device=device),
                        best_margins=torch.zeros(n, dtype=torch.float32, device=device))
            ptr = {a: keep[a].data_ptr() for a in ("X", "y", "eval_margins", "best_margins")}
        else:
            Xe, ye = _gbdt_xy(Xe, ye)
            keep.update(X=Xe, y=ye, eval_margins=np.zeros(Xe.shape[0], np.float32),
                        best_margins=np.zeros(n, np.float32))
            ptr = {a: keep[a].ctypes.data for a in ("X", "y", "eval_margins", "best_margins")}
        if Xe.shape[1] < F:
            raise ValueError(f"the eval matrix has {Xe.shape[1]} columns, the fit {F}")
        ev.n, ev.ld = int(Xe.shape[0]), int(Xe.shape[1])
        if ev.n:
            ev.X, ev.y, ev.margins, ev.best_margins = ptr["X"], ptr["y"], ptr["eval_margins"], ptr["best_margins"]
    return ev, keep


def _gbdt_eval_forest(out, n_nodes, F, p, ev, keep, margins, eval_metric, early_stopping_rounds):
    """The ForestArrays of a watched fit from the C ABI's outputs (every grown tree): cut to the best round's trees
    when early stopping was asked for."""
    run = int(ev.rounds_run)
    out.a["offsets"] = out.a["offsets"][:run + 1]
    fa = out.forest(n_nodes, F, p.base_score)
    fa.meta["margins"] = margins
    fa.meta["rounds_run"] = run
    if ev.best_iteration < 0:  # no eval set: only the class weight acted
        return fa
    curve = keep["curve"][:run].copy()
    best = int(ev.best_iteration)
    if early_stopping_rounds is not None and best + 1 < run:
        fa = truncate_forest(fa, best + 1)
        fa.meta["margins"] = keep["best_margins"]
    fa.meta.update(evals_result={"validation_0": {eval_metric: [float(v) for v in curve]}}, best_iteration=best,
                   best_score=float(curve[best]), eval_margins=keep["eval_margins"])
    return fa


def _gbdt_fit_eval(fn: str, head, X, y, p, eval_set, eval_metric, early_stopping_rounds, scale_pos_weight):
    """The two calls of fd_gbdt_fit_eval_* on host arrays."""
    n, ld = X.shape
    ev, keep = _gbdt_eval_struct(eval_set, eval_metric, early_stopping_rounds, scale_pos_weight, p, n, ld)
    cap = C.c_int64()
    N.call(fn, *head, _ptr(X), _ptr(y), n, ld, ld, C.byref(p), None, None, C.byref(cap), None)
    out = _GbdtOut(p.n_rounds, cap.value)
    margins = np.zeros(n, np.float32)
    nn = C.c_int64()
    N.call(fn, *head, _ptr(X), _ptr(y), n, ld, ld, C.byref(p), C.byref(ev), C.byref(out.model), C.byref(nn),
           _ptr(margins))
    return _gbdt_eval_forest(out, nn.value, ld, p, ev, keep, margins, eval_metric, early_stopping_rounds)


def gbdt_fit_ref_host(X, y, eval_set=None, eval_metric="auc", early_stopping_rounds=None, scale_pos_weight=1.0,
                      **params) -> ForestArrays:
    """Host-only: the single-threaded reference fit (fd_gbdt_fit_ref_host / fd_gbdt_fit_eval_ref_host), as
    FraudEngine.fit_gbdt returns it."""
    X, y = _gbdt_xy(X, y)
    if eval_set is not None or early_stopping_rounds is not None or float(scale_pos_weight) != 1.0:
        return _gbdt_fit_eval("fd_gbdt_fit_eval_ref_host", (), X, y, gbdt_params(**params), eval_set, eval_metric,
                              early_stopping_rounds, scale_pos_weight)
    return _gbdt_fit("fd_gbdt_fit_ref_host", (), X, y, gbdt_params(**params))


def _gbdt_metric(fn: str, head, margins, y, metric) -> float:
    margins = np.ascontiguousarray(margins, dtype=np.float32).reshape(-1)
    yy = np.asarray(y).reshape(-1)
    if yy.shape != margins.shape:
        raise ValueError("y: one label per margin")
    if not np.isin(yy, (0, 1)).all():
        raise ValueError("labels must be 0 or 1")
    yy = np.ascontiguousarray(yy.astype(np.uint8))
    v = C.c_double()
    N.call(fn, *head, _ptr(margins), _ptr(yy), margins.size, _gbdt_metric_id(metric), C.byref(v))
    return v.value


def gbdt_metric_ref_host(margins, y, metric="auc") -> float:
    """Host-only: the eval metric ("auc" or "error") of f32 margins and 0 / 1 labels (fd_gbdt_metric_ref_host)."""
    return _gbdt_metric("fd_gbdt_metric_ref_host", (), margins, y, metric)


def gbdt_grad_weighted_ref_host(margin, y, scale_pos_weight):
    """Host-only: the fixed-point (g, h) under a class weight (fd_gbdt_grad_weighted_ref_host)."""
    margin = np.ascontiguousarray(margin, dtype=np.float32)
    y = np.ascontiguousarray(y, dtype=np.uint8)
    g, h = np.zeros(margin.size, np.int32), np.zeros(margin.size, np.int32)
    N.call("fd_gbdt_grad_weighted_ref_host", _ptr(margin), _ptr(y), margin.size, float(scale_pos_weight), _ptr(g),
           _ptr(h))
    return g, h


def gbdt_cuts_host(X, max_bin: int = 256):
    """Host-only: the per-feature cuts of a matrix (fd_gbdt_cuts_host) -> (cuts f32, offsets int32 [F + 1])."""
    X = np.ascontiguousarray(np.asarray(X, dtype=np.float32))
    n, ld = X.shape
    total = C.c_int64()
    cuts = np.zeros(max(ld, 1) * 254, np.float32)  # the most a feature can have: no size query, one pass
    offsets = np.zeros(ld + 1, np.int32)
    N.call("fd_gbdt_cuts_host", _ptr(X), n, ld, ld, int(max_bin), _ptr(cuts), _ptr(offsets), C.byref(total))
    return cuts[:total.value], offsets


def gbdt_bin_ref_host(X, cuts, offsets) -> np.ndarray:
    """Host-only: the u8 bin matrix (fd_gbdt_bin_ref_host)."""
    X = np.ascontiguousarray(np.asarray(X, dtype=np.float32))
    n, ld = X.shape
    cuts = np.ascontiguousarray(np.concatenate([np.asarray(cuts, np.float32), np.zeros(1, np.float32)]))
    offsets = np.ascontiguousarray(offsets, dtype=np.int32)
    bins = np.zeros((n, ld), np.uint8)
    N.call("fd_gbdt_bin_ref_host", _ptr(X), n, ld, ld, _ptr(cuts), _ptr(offsets), _ptr(bins))
    return bins


def gbdt_grad_ref_host(margin, y):
    """Host-only: margins and labels -> the fixed-point (g, h) (fd_gbdt_grad_ref_host); one quantum is 2^-24."""
    margin = np.ascontiguousarray(margin, dtype=np.float32)
    y = np.ascontiguousarray(y, dtype=np.uint8)
    g, h = np.zeros(margin.size, np.int32), np.zeros(margin.size, np.int32)
    N.call("fd_gbdt_grad_ref_host", _ptr(margin), _ptr(y), margin.size, _ptr(g), _ptr(h))
    return g, h


def _gbdt_grow(fn: str, head, bins, cuts, offsets, g, h, row_mask, feature_mask, params):
    bins = np.ascontiguousarray(bins, dtype=np.uint8)
    n, F = bins.shape
    cuts = np.ascontiguousarray(np.concatenate([np.asarray(cuts, np.float32), np.zeros(1, np.float32)]))
    offsets = np.ascontiguousarray(offsets, dtype=np.int32)
    g = np.ascontiguousarray(g, dtype=np.int32)
    h = np.ascontiguousarray(h, dtype=np.int32)
    rm = None if row_mask is None else np.ascontiguousarray(row_mask, dtype=np.uint8)
    fm = (2 ** F - 1) if feature_mask is None else int(feature_mask)
    p = gbdt_params(**params)
    out = _GbdtOut(1, 2 ** (p.max_depth + 1) - 1)
    nn = C.c_int64()
    N.call(fn, *head, _ptr(bins), n, F, _ptr(cuts), _ptr(offsets), _ptr(g), _ptr(h), _ptr(rm), C.c_uint64(fm),
           C.byref(p), C.byref(out.model), C.byref(nn))
    return out.forest(nn.value, F, p.base_score)


def gbdt_grow_tree_ref_host(bins, cuts, offsets, g, h, row_mask=None, feature_mask=None, **params) -> ForestArrays:
    """Host-only: one tree from a binned matrix and fixed-point gradients (fd_gbdt_grow_tree_ref_host). feature_mask:
    an integer whose bit f keeps feature f (None: all)."""
    return _gbdt_grow("fd_gbdt_grow_tree_ref_host", (), bins, cuts, offsets, g, h, row_mask, feature_mask, params)


# ------------------------------------------------------------------------------------ training (iforest_fit.hip)

IFOREST_DEFAULTS = dict(n_estimators=100, max_samples=0, max_features=1.0, contamination=0.0, seed=0)


def iforest_fit_params(**kw) -> "N.fd_iforest_fit_params":
    """fd_iforest_fit_params from keywords (IFOREST_DEFAULTS; scikit-learn's random_state is accepted for seed and
    "auto" for max_samples and contamination)."""
    v = dict(IFOREST_DEFAULTS)
    for k, x in kw.items():
        k = {"random_state": "seed"}.get(k, k)
        if k not in v:
            raise TypeError(f"unknown IsolationForest parameter {k!r}")
        v[k] = 0 if isinstance(x, str) and x == "auto" and k in ("max_samples", "contamination") else x
    return N.fd_iforest_fit_params(int(v["n_estimators"]), int(v["max_samples"]), float(v["max_features"]),
                                   float(v["contamination"]), int(v["seed"]) & (2 ** 64 - 1))


def _iforest_x(X) -> np.ndarray:
    X = np.ascontiguousarray(np.asarray(X, dtype=np.float32))
    if X.ndim != 2:
        raise ValueError("X: a 2-d matrix")
    return X


class _IForestOut:
    """Caller arrays of a grown IsolationForest with room for `cap` nodes of `n_trees` trees."""

    def __init__(self, n_trees: int, cap: int):
        self.a = dict(offsets=np.zeros(n_trees + 1, np.int64), left=np.zeros(cap, np.int32),
                      right=np.zeros(cap, np.int32), feature=np.zeros(cap, np.int32),
                      threshold=np.zeros(cap, np.float64), default_left=np.zeros(cap, np.uint8),
                      leaf_value=np.zeros(cap, np.float64), n_node_samples=np.zeros(cap, np.float64))
        a = self.a

        def P(x, t):
            return x.ctypes.data_as(C.POINTER(t))

        self.trees = N.fd_tree_arrays(n_trees, P(a["offsets"], C.c_int64), P(a["left"], C.c_int32),
                                      P(a["right"], C.c_int32), P(a["feature"], C.c_int32),
                                      P(a["threshold"], C.c_double), P(a["default_left"], C.c_uint8),
                                      P(a["leaf_value"], C.c_double))

    def forest(self, n_nodes: int, num_feature: int, fp=None, **meta) -> ForestArrays:
        a = {k: (v if k == "offsets" else v[:n_nodes].copy()) for k, v in self.a.items()}
        return ForestArrays(kind=N.FD_FOREST_SKLEARN_IFOREST, num_feature=num_feature, offsets=a["offsets"],
                            left=a["left"], right=a["right"], feature=a["feature"], threshold=a["threshold"],
                            default_left=a["default_left"], leaf_value=a["leaf_value"],
                            if_offset=fp.if_offset if fp is not None else 0.0,
                            if_denominator=fp.if_denominator if fp is not None else 0.0, cover=a["n_node_samples"],
                            meta=dict(meta, n_trees=len(a["offsets"]) - 1, n_node_samples=a["n_node_samples"]))


def _iforest_fit(fn: str, head, xptr, n: int, ld: int, F, p) -> ForestArrays:
    """The two calls of fd_iforest_fit_*: the capacity, then the fit. F: the model's columns (None: all ld)."""
    F = int(ld if F is None else F)
    cap = C.c_int64()
    N.call(fn, *head, xptr, n, ld, F, C.byref(p), None, None, None, C.byref(cap))
    out = _IForestOut(p.n_estimators, cap.value)
    fp = N.fd_forest_params()
    nn = C.c_int64()
    N.call(fn, *head, xptr, n, ld, F, C.byref(p), C.byref(out.trees), out.a["n_node_samples"].ctypes.data,
           C.byref(fp), C.byref(nn))
    psi = min(p.max_samples or 256, n)
    return out.forest(nn.value, F, fp, max_samples=psi, n_estimators=p.n_estimators, max_features=p.max_features,
                      contamination=p.contamination, seed=p.seed)


def iforest_fit_ref_host(X, **params) -> ForestArrays:
    """Host-only: the single-threaded reference fit (fd_iforest_fit_ref_host), as FraudEngine.fit_iforest returns
    it. num_feature=F: only the first F columns of X are the model's."""
    X = _iforest_x(X)
    F = params.pop("num_feature", None)
    return _iforest_fit("fd_iforest_fit_ref_host", (), _ptr(X), X.shape[0], X.shape[1], F,
                        iforest_fit_params(**params))


def _iforest_sample(fn: str, head, n: int, tree: int, params) -> np.ndarray:
    p = iforest_fit_params(**params)
    rows = np.zeros(1024, np.int32)
    psi = C.c_int32()
    N.call(fn, *head, int(n), C.byref(p), int(tree), _ptr(rows), C.byref(psi))
    return rows[:psi.value].copy()


def iforest_fit_sample_ref_host(n: int, tree: int, **params) -> np.ndarray:
    """Host-only: tree `tree`'s row ids of a fit over n rows (fd_iforest_fit_sample_ref_host)."""
    return _iforest_sample("fd_iforest_fit_sample_ref_host", (), n, tree, params)


def _iforest_grow(fn: str, head, X, rows, tree, feature_mask, params) -> ForestArrays:
    X = _iforest_x(X)
    n, F = X.shape
    rows = np.ascontiguousarray(rows, dtype=np.int32)
    m = rows.size
    fm = (2 ** F - 1) if feature_mask is None else int(feature_mask)
    p = iforest_fit_params(**params)
    depth = max(1, int(m - 1).bit_length())
    out = _IForestOut(1, 2 ** (depth + 1) - 1)
    nn = C.c_int64()
    N.call(fn, *head, _ptr(X), n, F, F, _ptr(rows), m, C.c_uint64(fm), C.byref(p), int(tree), C.byref(out.trees),
           out.a["n_node_samples"].ctypes.data, C.byref(nn))
    return out.forest(nn.value, F, max_samples=m)


def iforest_fit_grow_tree_ref_host(X, rows, tree: int = 0, feature_mask=None, **params) -> ForestArrays:
    """Host-only: one tree from explicit row ids (fd_iforest_fit_grow_tree_ref_host). feature_mask: an integer whose
    bit f keeps feature f (None: all)."""
    return _iforest_grow("fd_iforest_fit_grow_tree_ref_host", (), X, rows, tree, feature_mask, params)


def shard_of(keys, n_shards: int) -> np.ndarray:
    """Owner shard of each card key (host-only, no GPU): the partition fd_route_partition_device uses."""
    k = np.ascontiguousarray(keys, np.uint64)
    out = np.empty(len(k), np.int32)
    N.call("fd_shard_of_host", _ptr(k), len(k), int(n_shards), _ptr(out))
    return out


def device_count() -> int:
    c = C.c_int()
    rc = N.lib.fd_device_count(C.byref(c))
    return c.value if rc == N.FD_OK else 0


def merge_merchant_windows(parts) -> np.ndarray:
    """Combine merchant-window partials of several shards (N.MERCHANT_WINDOW_DTYPE arrays) into whole windows,
    sorted by (window_start, merchant): exact moments summed, derived fields recomputed by the library's own
    finalisation (fd_merchant_windows_merge, host only), so the result is bit-identical to an unsharded run."""
    a = np.concatenate([np.asarray(p, N.MERCHANT_WINDOW_DTYPE) for p in parts]) if len(parts) else \
        np.zeros(0, N.MERCHANT_WINDOW_DTYPE)
    a = np.ascontiguousarray(a)
    out = np.zeros(max(len(a), 1), N.MERCHANT_WINDOW_DTYPE)
    m = C.c_int64()
    N.call("fd_merchant_windows_merge", a.ctypes.data if len(a) else None, len(a), out.ctypes.data, C.byref(m))
    return out[:m.value].copy()


class PipelinedScorer:
    """fd_score_batch_pipelined (or, pipelined=False, fd_score_batch_device) with its model arguments marshalled
    once (FraudEngine.pipelined_scorer / batch_scorer)."""

    def __init__(self, eng: FraudEngine, params: N.fd_blend_params, slots: Sequence[int],
                 present: Optional[Sequence[int]] = None, pipelined: bool = True):
        M = params.n_models
        self.eng = eng
        self.params = params
        self._sl = np.array(list(slots) + [-1] * (N.FD_MAX_MODELS - len(slots)), np.int32)
        self._pres = np.array([1] * M if present is None else list(present), np.uint8)
        self._ext = (C.c_void_p * N.FD_MAX_MODELS)()
        self._batch = N.fd_txn_batch()
        self.pipelined = pipelined
        self._fn = N.lib.fd_score_batch_pipelined if pipelined else N.lib.fd_score_batch_device
        self._args = [C.byref(params), _ptr(self._sl), self._ext, _ptr(self._pres), C.byref(self._batch)]

    def __call__(self, txn_ptrs: dict, n: int, fp_ptr: int, conf_ptr: int = 0, dec_ptr: int = 0, risk_ptr: int = 0,
                 input_ready: int = 0, vec_ptr: int = 0, model_probs_ptr: int = 0) -> None:
        b = self._batch
        for f in N.TXN_FIELDS:
            setattr(b, f, txn_ptrs[f])
        if self.pipelined:
            rc = self._fn(self.eng._h, *self._args, int(n), vec_ptr or None, model_probs_ptr or None, fp_ptr,
                          conf_ptr or None, dec_ptr or None, risk_ptr or None, input_ready or None)
            N.check(rc, "fd_score_batch_pipelined")
        else:
            rc = self._fn(self.eng._h, *self._args, int(n), vec_ptr or None, model_probs_ptr or None, fp_ptr,
                          conf_ptr or None, dec_ptr or None, risk_ptr or None)
            N.check(rc, "fd_score_batch_device")


class ShardedStep:
    """fd_sharded_step for a fixed model set (FraudEngine.sharded_scorer): per call only the batch pointers change.
    batch_id / next_id: the C-ABI's prefetch ids (include/fdengine.h): next_id (nonzero) names the prefetched batch,
    the call that scores it passes it as batch_id; 0 = not the prefetched batch."""

    def __init__(self, eng: FraudEngine, params: N.fd_blend_params, slots: Sequence[int],
                 present: Optional[Sequence[int]] = None):
        M = params.n_models
        self.eng, self.params = eng, params
        self._sl = np.array(list(slots) + [-1] * (N.FD_MAX_MODELS - len(slots)), np.int32)
        self._pres = np.array([1] * M if present is None else list(present), np.uint8)
        self._cur, self._next = N.fd_txn_batch(), N.fd_txn_batch()
        self.split_sizes = np.zeros(2 * 64, np.int64)
        self._fn = N.lib.fd_sharded_step

    def __call__(self, txn_ptrs: dict, n: int, fp_ptr: int, conf_ptr: int, dec_ptr: int, risk_ptr: int,
                 input_ready: int = 0, next_ptrs: Optional[dict] = None, next_n: int = 0, next_ready: int = 0,
                 batch_id: int = 0, next_id: int = 0) -> None:
        for f in N.TXN_FIELDS:
            setattr(self._cur, f, txn_ptrs[f])
        nxt = None
        if next_ptrs is not None:
            for f in N.TXN_FIELDS:
                setattr(self._next, f, next_ptrs[f])
            nxt = C.byref(self._next)
        rc = self._fn(self.eng._h, C.byref(self.params), self._sl.ctypes.data, self._pres.ctypes.data,
                      C.byref(self._cur), int(n), int(batch_id), input_ready or None, nxt, int(next_n), int(next_id),
                      next_ready or None, fp_ptr or None, conf_ptr or None, dec_ptr or None, risk_ptr or None,
                      self.split_sizes.ctypes.data)
        N.check(rc, "fd_sharded_step")
