"""Drop-in for the deterministic part of the reference's BertTextAnalyzer (ml/models/bert_text_analyzer.py:21-412):
detect_fraud_patterns (:283-344) and get_text_features (:346-399), computed by the engine (csrc/text.hip).

What differs from the reference, on purpose:
  * analyze_transaction_text returns {'overall_text_risk': 0.0}. The reference scores text with a DistilBERT checkpoint
    fetched by name; without one it runs a dummy model that returns torch.randn logits (:95-99), so its value is noise
    by construction. 0.0 is what the reference's own failure path returns (:175-177). load_model() does nothing.
  * The engine computes rows whose four fields are all ASCII. A row with any other character is flagged by the engine
    (FD_TEXT_NONASCII) and recomputed here with str operations, by the reference's rule, so the results equal the
    reference's for any str input. The keyword lists stay in csrc/text_row.h: the flags of such a row come from the
    host form of the same rule (fd_text_features_ref_host) over the row's lower-cased join with every non-ASCII
    character replaced by a byte no keyword holds (the keywords are ASCII, and str.lower() has been applied already).

A row is a dict with the keys merchant_name, description, category, location; a missing key is the empty string, a
value that is not a str raises TypeError (as the reference's join and len do for None).
"""
from __future__ import annotations

import re
import time
from typing import Any, Dict, Optional, Sequence, Tuple

import numpy as np

from . import _native as N
from .engine import FraudEngine

FIELDS = N.TEXT_FIELDS
COLUMNS = N.TEXT_COLUMNS
PATTERNS = N.TEXT_PATTERNS
_DIVERSITY = COLUMNS.index("merchant_name_char_diversity")
_NO_KEYWORD_BYTE = "\x01"


def encode_rows(rows: Sequence[Dict[str, str]], fields: Sequence[str] = FIELDS) -> Tuple[bytes, np.ndarray]:
    """rows -> (blob, int64 offsets [4 n + 1]); fields not in `fields` are encoded empty"""
    parts, off, pos = [], [0], 0
    for r in rows:
        for f in FIELDS:
            v = r.get(f, "") if f in fields else ""
            if not isinstance(v, str):
                raise TypeError(f"text field {f!r} must be str, not {type(v).__name__}")
            b = v.encode("utf-8", "surrogatepass")
            parts.append(b)
            pos += len(b)
            off.append(pos)
    return b"".join(parts), np.asarray(off, np.int64)


def features_of_str(merchant_name: str, description: str) -> list:
    """get_text_features by the reference's rule on str values (any Unicode), in COLUMNS order"""
    unique = len(set(merchant_name.lower())) if merchant_name else 0
    diversity = unique / max(len(merchant_name), 1) if merchant_name else 0
    num = [len(re.findall(r"\d", s)) for s in (merchant_name, description)]
    spec = [len(re.findall(r"[^a-zA-Z0-9\s]", s)) for s in (merchant_name, description)]
    words = [len(s.split()) if s else 0 for s in (merchant_name, description)]
    return [len(merchant_name), len(description), len(merchant_name) + len(description), unique, diversity,
            num[0], num[1], sum(num), spec[0], spec[1], sum(spec), words[0], words[1], sum(words)]


def patterns_of_str(fields: Sequence[str]) -> int:
    """detect_fraud_patterns' bits for four str fields of any Unicode (see the module docstring)"""
    joined = " ".join(fields).lower()
    data = "".join(ch if ch < "\x80" else _NO_KEYWORD_BYTE for ch in joined).encode("ascii")
    off = np.array([0, len(data), len(data), len(data), len(data)], np.int64)
    blob = np.frombuffer(data, np.uint8)
    out = np.zeros(1, np.uint8)
    N.call("fd_text_features_ref_host", blob.ctypes.data if len(blob) else None, off.ctypes.data, 1, None,
           out.ctypes.data, None)
    return int(out[0])


class BertTextAnalyzer:
    def __init__(self, model_path: str = "distilbert-base-uncased", device: Any = "auto",
                 engine: Optional[FraudEngine] = None):
        """engine: an existing FraudEngine to compute on; otherwise one is created on GPU `device` ("auto" / "cuda"
        = 0) and closed with close()."""
        self.model_path = model_path
        self.max_length = 512
        self._own = engine is None
        self.engine = engine if engine is not None else FraudEngine(device if isinstance(device, int) else 0)
        self.total_predictions = 0
        self.total_time_ms = 0.0

    def close(self) -> None:
        if self._own and self.engine is not None:
            self.engine.close()
        self.engine = None

    def load_model(self) -> None:
        """Accepted for the reference's call sequence; there is no model to load (the model score is not ported)."""

    def _analyze(self, rows: Sequence[Dict[str, str]], fields: Sequence[str]):
        blob, off = encode_rows(rows, fields)
        feat, bits, status = self.engine.text_features(blob, off)
        for i in np.flatnonzero(status == N.FD_TEXT_NONASCII):
            vals = [rows[i].get(f, "") if f in fields else "" for f in FIELDS]
            feat[i] = features_of_str(vals[0], vals[1])
            bits[i] = patterns_of_str(vals)
        return feat, bits

    # ------------------------------------------------------------------ the reference's surface
    def analyze_batch(self, rows: Sequence[Dict[str, str]]) -> Tuple[np.ndarray, np.ndarray]:
        """-> (bool [n, 5] in PATTERNS order, f64 [n, 14] in COLUMNS order)"""
        t0 = time.time()
        feat, bits = self._analyze(rows, FIELDS)
        flags = ((bits[:, None] >> np.arange(N.FD_TEXT_PATTERNS, dtype=np.uint8)) & 1).astype(bool)
        self.total_predictions += len(rows)
        self.total_time_ms += (time.time() - t0) * 1000
        return flags, feat

    def detect_fraud_patterns(self, text_data: Dict[str, str]) -> Dict[str, bool]:
        _, bits = self._analyze([text_data], FIELDS)
        return {name: bool((int(bits[0]) >> k) & 1) for k, name in enumerate(PATTERNS)}

    def get_text_features(self, text_data: Dict[str, str]) -> Dict[str, float]:
        feat, _ = self._analyze([text_data], FIELDS[:2])
        return {name: float(feat[0, k]) if k == _DIVERSITY else int(feat[0, k]) for k, name in enumerate(COLUMNS)}

    def analyze_transaction_text(self, text_data: Dict[str, str]) -> Dict[str, float]:
        """Not ported: the reference's value is random without a fetched checkpoint. Its failure path's answer."""
        return {"overall_text_risk": 0.0}

    def get_performance_stats(self) -> Dict[str, float]:
        avg = self.total_time_ms / self.total_predictions if self.total_predictions > 0 else 0.0
        return {"total_predictions": self.total_predictions, "avg_processing_time_ms": avg,
                "total_processing_time_ms": self.total_time_ms}
