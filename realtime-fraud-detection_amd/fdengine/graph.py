"""Drop-in for the reference's GraphFraudDetector (ml/models/graph_neural_network.py:94-405): the rolling transaction
log and the five network features of _calculate_network_features, computed by the engine (csrc/graph.hip).

What differs from the reference, on purpose:
  * network_risk_score is 0.0. The reference runs its model over torch.randn node features (:244-336), so its value is
    noise by construction; nothing is ported and load_model() does nothing.
  * path_length_anomaly sums the window's amounts exactly in cents (the reference sums floats left to right): within
    1e-11 of the reference for positive two-decimal amounts. The other four features are the reference's values.
  * The log is one arrival sequence per engine. A sharded deployment keeps one log per rank.

User ids become fd_hash64 keys (a falsy id is the null user, key 0); merchant ids become dense int32 indices in order
of first sight (a falsy id is the null merchant, -1); amounts become round(amount * 100) cents.
"""
from __future__ import annotations

import time
from typing import Any, Dict, Optional, Sequence

import numpy as np

from . import _native as N
from .engine import FraudEngine
from .ingest import hash64

COLUMNS = N.GRAPH_COLUMNS


class GraphFraudDetector:
    def __init__(self, model_path: Optional[str] = None, device: Any = 0, engine: Optional[FraudEngine] = None,
                 max_history_size: int = 10000):
        """engine: an existing FraudEngine to keep the log on (its graph log is re-initialised); otherwise one is
        created on GPU `device` ("auto" / "cuda" = 0) and closed with close()."""
        self.model_path = model_path
        self._own = engine is None
        self.engine = engine if engine is not None else FraudEngine(device if isinstance(device, int) else 0)
        self.max_history_size = int(max_history_size)
        self.engine.graph_init(self.max_history_size)
        self._users: Dict[Any, int] = {}
        self._merchants: Dict[Any, int] = {}
        self.total_predictions = 0
        self.total_time_ms = 0.0

    def close(self) -> None:
        if self._own and self.engine is not None:
            self.engine.close()
        self.engine = None

    def load_model(self) -> None:
        """Accepted for the reference's call sequence; there is no model to load (network_risk_score is not ported)."""

    # ------------------------------------------------------------------ id mapping
    def _user_key(self, user_id) -> int:
        if not user_id:
            return 0
        k = self._users.get(user_id)
        if k is None:
            k = hash64(user_id if isinstance(user_id, (str, bytes)) else str(user_id)) or 1
            self._users[user_id] = k
        return k

    def _merchant_index(self, merchant_id) -> int:
        if not merchant_id:
            return -1
        return self._merchants.setdefault(merchant_id, len(self._merchants))

    def _columns(self, transactions: Sequence[Dict[str, Any]]):
        n = len(transactions)
        key, mer, cents = np.empty(n, np.uint64), np.empty(n, np.int32), np.empty(n, np.int64)
        for i, t in enumerate(transactions):
            key[i] = self._user_key(t.get("user_id"))
            mer[i] = self._merchant_index(t.get("merchant_id"))
            cents[i] = int(round(float(t.get("amount", 0) or 0) * 100))
        return key, mer, cents

    # ------------------------------------------------------------------ the reference's surface
    def analyze_batch(self, transactions: Sequence[Dict[str, Any]]) -> np.ndarray:
        """Transactions in arrival order -> f64 [n, 5] in COLUMNS order; later rows see earlier ones."""
        t0 = time.time()
        out = self.engine.graph_step(*self._columns(transactions))
        self.total_predictions += len(transactions)
        self.total_time_ms += (time.time() - t0) * 1000
        return out

    def analyze_transaction_network(self, transaction_data: Dict[str, Any]) -> Dict[str, float]:
        row = self.analyze_batch([transaction_data])[0]
        res = {"network_risk_score": 0.0}
        res.update({c: float(row[i]) for i, c in enumerate(COLUMNS)})
        return res

    def get_performance_stats(self) -> Dict[str, float]:
        avg = self.total_time_ms / self.total_predictions if self.total_predictions > 0 else 0.0
        return {"total_predictions": self.total_predictions, "avg_processing_time_ms": avg,
                "total_processing_time_ms": self.total_time_ms,
                "transaction_history_size": self.engine.graph_info()["held"]}
