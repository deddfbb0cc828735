#!/usr/bin/env python3
"""Generate tests/golden/text_cases.npz by running the REFERENCE's own BertTextAnalyzer
(services/ml-models/src/models/bert_text_analyzer.py) in the build container. Only the rows' bytes, their offsets and
the two methods' outputs written here travel; the reference never does. Never runs on the GPU machine.

Run:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_text_golden.py

Reference code exercised (unchanged): detect_fraud_patterns (:283-344) and get_text_features (:346-399); neither
touches a model or a tokenizer, so load_model() is not called and nothing is fetched. utils.logging_config
(structlog) is registered as a module whose get_logger returns a standard logger.

Rows (tests/text_cases.py build_groups): every keyword in every field in three cases, near misses, keywords across
field boundaries, positions and overlaps, every ASCII byte alone and between letters, whitespace, word counts, unique
characters, a seeded random stream (one description of 70 000 bytes), and non-ASCII rows. The coverage each group is
there for is asserted below on the reference's outputs."""
import importlib.machinery
import logging
import sys
import types
from pathlib import Path

import numpy as np

sys.dont_write_bytecode = True
HERE = Path(__file__).resolve().parent
REF_SRC = Path("/root/reference/services/ml-models/src")
sys.path.insert(0, str(HERE.parent))

import text_cases as T  # noqa: E402


def reference_class():
    if "utils.logging_config" not in sys.modules:
        for name in ("utils", "utils.logging_config"):
            m = types.ModuleType(name)
            m.__spec__ = importlib.machinery.ModuleSpec(name, None)
            sys.modules[name] = m
        sys.modules["utils"].__path__ = []
        sys.modules["utils.logging_config"].get_logger = logging.getLogger
    sys.path.insert(0, str(REF_SRC))
    from models.bert_text_analyzer import BertTextAnalyzer
    return BertTextAnalyzer


def run_reference(det, rows):
    feat = np.zeros((len(rows), len(T.COLUMNS)))
    pat = np.zeros(len(rows), np.uint8)
    for i, r in enumerate(rows):
        d = dict(zip(T.FIELDS, r))
        f = det.get_text_features(d)
        assert list(f) == list(T.COLUMNS)
        feat[i] = [f[c] for c in T.COLUMNS]
        p = det.detect_fraud_patterns(d)
        assert list(p) == list(T.PATTERNS)
        pat[i] = sum(int(p[c]) << k for k, c in enumerate(T.PATTERNS))
    return feat, pat


def check_coverage(groups, span, feat, pat):
    kws = T.keywords()
    bit = lambda name: pat[span[name][0]:span[name][1]]  # noqa: E731
    col = lambda name, c: feat[span[name][0]:span[name][1], T.COLUMNS.index(c)]  # noqa: E731
    # every keyword, wrapped in letters, in each field and case: its list's flag
    hits = bit("keyword_hits").reshape(len(kws), 12)
    for (k, b), row in zip(kws, hits):
        assert ((row >> b) & 1).all(), k
    # every keyword has a near miss that clears its list's flag
    rows, at = groups["near_misses"], 0
    for k, b in kws:
        cnt = 2 * len(k) + (2 if " " in k else 0)
        part = bit("near_misses")[at:at + cnt]
        assert (((part >> b) & 1) == 0).any(), k
        if " " in k:
            assert (((part[-2:] >> b) & 1) == 0).all(), k  # a doubled space and a tab are no 0x20
        at += cnt
    assert at == len(rows)
    two = T.two_word(kws)
    bh = bit("boundary_hits").reshape(len(two), 3)
    for (k, b), row in zip(two, bh):
        assert ((row >> b) & 1).all(), k
    bm = bit("boundary_misses").reshape(len(two), 5)
    for (k, b), row in zip(two, bm):
        assert (((row[:2] >> b) & 1) == 0).all(), k
    pos = bit("positions")[:3 * len(kws)].reshape(len(kws), 3)
    for (k, b), row in zip(kws, pos):
        assert ((row >> b) & 1).all(), k
    assert (bit("positions")[3 * len(kws):] != 0).all()  # every overlap string holds a keyword
    # byte classes: 4 rows per byte (m alone, d alone, a?b in m, a?b in d)
    space = {9, 10, 11, 12, 13, 28, 29, 30, 31, 32}
    words = col("byte_classes", "total_word_count").reshape(128, 4)
    spec = col("byte_classes", "total_special_chars").reshape(128, 4)
    nums = col("byte_classes", "total_numbers").reshape(128, 4)
    uniq = col("byte_classes", "merchant_name_unique_chars").reshape(128, 4)
    for b in range(128):
        ch = chr(b)
        assert (words[b] == ([0, 0, 2, 2] if b in space else [1, 1, 1, 1])).all(), b
        assert (nums[b] == (1 if ch in "0123456789" else 0)).all(), b
        assert (spec[b] == (0 if (b in space or ch.isalnum()) else 1)).all(), b
        assert uniq[b, 0] == 1 and uniq[b, 2] == (2 if ch in "aAbB" else 3), b
    u = col("unique", "merchant_name_unique_chars")
    assert u[0] == 2 and u[1] == 102
    rnd = bit("random")
    for b in range(5):
        share = float(((rnd >> b) & 1).mean())
        print("random stream, flag", T.PATTERNS[b], "set on", round(share, 3))
        assert 0.10 <= share <= 0.90, (b, share)
    lo, hi = span["random"]
    lengths = np.array([[len(s) for s in r] for r in groups["random"]])
    assert lengths[:-1].min() == 0 and (lengths[:-1] >= 290).any() and len(groups["random"]) >= 2000
    assert ((lengths[:, 1] > 4900) & (lengths[:, 1] < 5100)).sum() >= 3
    assert lengths[-1, 1] == T.LONG_ROW and rnd[-1] == 1 << 4  # the keyword at its end, and nothing else
    assert T.LONG_ROW == feat[hi - 1, 1]


def main():
    det = reference_class()(device="cpu")
    named = T.build_groups()
    groups = dict(named)
    rows, starts = [], [0]
    for _, rs in named:
        rows += rs
        starts.append(len(rows))
    span = {name: (starts[i], starts[i + 1]) for i, (name, _) in enumerate(named)}
    feat, pat = run_reference(det, rows)
    check_coverage(groups, span, feat, pat)
    nonascii = np.array([any(not s.isascii() for s in r) for r in rows])
    assert nonascii[span["non_ascii"][0]:].all() and not nonascii[:span["non_ascii"][0]].any()
    assert 30 <= nonascii.sum() <= 0.05 * len(rows)
    blob, off = T.encode(rows)
    np.savez_compressed(T.GOLDEN, blob=blob, off=off.astype(np.int32), feat=feat, patterns=pat,
                        nonascii=nonascii.astype(np.uint8), group_names=np.array([n for n, _ in named]),
                        group_starts=np.array(starts, np.int32))
    print("rows", len(rows), "bytes", len(blob), "non-ASCII rows", int(nonascii.sum()))
    print("wrote", T.GOLDEN, T.GOLDEN.stat().st_size, "bytes")
    assert T.GOLDEN.stat().st_size <= 256 * 1000


if __name__ == "__main__":
    main()
