"""CPU: fd_dense_layout_host, the dense chunk layout of a contracted forest that the fused kernel walks on compact and
split rows under ensemble_contract 3 (bundles of consecutive trees) and 4 (the chunk's trees sorted by depth), in the
wide and the compact chunk geometry (include/fdengine.h; csrc/ensemble_plan.hip dense_layout_host). The layout's
invariants from the per-tree records and the chunk tables, and every tree's leaf value read from the blob by the
documented node word against a plain walk of the original forest, on vectors whose constant slots hold their serving
values."""
import numpy as np
import pytest

import dense_cases as DC
import test_contract_host as H
from fdengine import _native as N, synth, xgboost_from_json_doc
from fdengine.engine import contract_forest_host, dense_layout_host

S = H.S
S_MAX = 8
TPG = {(True, True): 6, (True, False): 4, (False, True): 5, (False, False): 3}  # [wide, xgb]
BUF = {True: 48 * 1024, False: 40 * 1024}


def _forests():
    Xr = H.vectors(2000, 9)
    sub_l, sub_r = S(0, 1.0, S(5, 3.0, 1.0, 2.0), 3.0), S(1, 1.0, 4.0, 5.0)
    vary = S(14, 2.0, S(15, 1.0, 1.0, 2.0), 3.0)
    out = {
        "root_constant": H.forest([S(12, 0.7, sub_l, sub_r), S(12, 0.3, sub_l, sub_r), S(2, 0.1, sub_l, sub_r),
                                   S(2, -0.1, sub_l, sub_r)]),
        "whole_tree_constant": H.forest([S(12, 0.6, S(2, 0.5, 1.0, 2.0), S(3, 0.5, 3.0, 4.0)),
                                         S(24, 0.5, 5.0, S(33, H.UP(0.5), 6.0, 7.0)), S(0, 1.0, 8.0, 9.0)]),
        "chain": H.forest([S(3, 0.25, S(25, 0.75, S(4, 1.0, vary, 7.0), 8.0), 9.0),
                           S(0, 1.0, S(8, 0.5, S(9, -1.0, 4.0, vary), 5.0), 6.0)]),
        "lone_leaf": H.forest([0.25, S(0, 1.0, 1.0, 2.0)]),
        "sklearn": H.forest([S(12, 0.5, 1.0, 2.0), S(12, float(np.nextafter(0.5, 0.0)), 1.0, 2.0), S(2, 0.0, 1.0, 2.0),
                             S(2, -1e-300, 1.0, 2.0), S(0, 1.5, S(34, 0.49999, 3.0, S(1, 0.5, 4.0, 5.0)), 6.0)],
                            kind=N.FD_FOREST_SKLEARN_IFOREST),
        "no_constant_node": DC.on_varying(xgboost_from_json_doc(
            synth.xgboost_doc(12, 5, 64, synth.feature_matrix(500, 64, seed=2), seed=4, p_leaf=0.3))),
        "shallow200": DC.shallow200(Xr),
        "deep_then_shallow": DC.deep_then_shallow(Xr),
        "fifty": xgboost_from_json_doc(synth.xgboost_doc(50, 5, 64, Xr, seed=24, p_leaf=0.2)),
        "single": xgboost_from_json_doc(synth.xgboost_doc(1, 4, 64, Xr, seed=25)),
        "iforest": DC.as_iforest(xgboost_from_json_doc(synth.xgboost_doc(45, 7, 64, Xr, seed=26, p_leaf=0.15)), 27),
    }
    for p_leaf in (0.0, 0.3):
        for depth in (3, 8):
            out[f"synthetic_{depth}_{p_leaf}"] = xgboost_from_json_doc(
                synth.xgboost_doc(40, depth, 64, Xr, seed=6, p_leaf=p_leaf))
            # thresholds off the constants' values (raw draws of a generic matrix): both directions occur
            out[f"synthetic_raw_{depth}_{p_leaf}"] = xgboost_from_json_doc(synth.xgboost_doc(
                40, depth, 64, synth.feature_matrix(2000, 64, seed=3), seed=7, p_leaf=p_leaf, max_bin=None))
    # test_contract_host.py's threshold edges (a threshold at the constant, the next f32 above and below it, both
    # default directions): these trees resolve to one leaf each
    for slot, value in ((12, 0.5), (2, 0.0)):
        for dl in (0, 1):
            out[f"edges_{slot}_{dl}"] = H.forest(
                [S(slot, value, 1.0, 2.0, dl), S(slot, H.UP(value), 1.0, 2.0, dl), S(slot, H.DOWN(value), 1.0, 2.0, dl),
                 S(slot, -0.0 if value == 0.0 else 0.5, 1.0, 2.0, dl)])
    # the same edges on varying slots, where the threshold's index in the table decides: slot 0 holds small counts
    # (3.0 occurs in the vectors), slot 1 continuous values; neighbouring f32 thresholds are distinct table entries
    for dl in (0, 1):
        out[f"edges_varying_{dl}"] = H.forest(
            [S(f, t, 1.0, S(f, H.UP(t), 2.0, S(f, H.UP(H.UP(t)), 3.0, 4.0, dl), dl), dl)
             for f, v in ((0, 3.0), (1, 0.5), (5, 2.0)) for t in (H.DOWN(v), v, H.UP(v))] +
            [S(0, 3.0, 1.0, 2.0, dl), S(0, H.UP(3.0), 1.0, 2.0, dl), S(0, H.DOWN(3.0), 1.0, 2.0, dl)])
    return out


FORESTS = _forests()
_WALKS = {}


def _plain_walk(name):
    """the original forest's leaf values on the shared vectors, once per forest"""
    if name not in _WALKS:
        X = H.vectors(300, 5)
        _WALKS[name] = (X, H.walk(FORESTS[name], X))
    return _WALKS[name]


def check_layout(fa, lay, wide, mode):
    xgb = fa.kind == N.FD_FOREST_XGB_BINARY_LOGISTIC
    tpg, info, tr = TPG[wide, xgb], lay["info"], lay["trees"]
    _, own, _ = contract_forest_host(fa)
    T = fa.n_trees
    assert info.s_max == S_MAX and info.trees_per_bundle == tpg and info.buf_bytes == BUF[wide]
    assert len(tr) == T and info.n_chunks == len(lay["chunk_offsets"]) == len(lay["chunk_lengths"])
    # every tree placed once, the chunks runs of consecutive trees, back to back in the blob
    assert (np.diff(tr["chunk"]) >= 0).all() and set(tr["chunk"]) == set(range(info.n_chunks))
    assert lay["chunk_offsets"][0] == 0 and (lay["chunk_lengths"] % 1024 == 0).all()
    np.testing.assert_array_equal(np.cumsum(lay["chunk_lengths"]), list(lay["chunk_offsets"][1:]) + [info.blob_bytes])
    assert (tr["depth"] >= own).all() and tr["depth"].max() <= 8
    assert info.node_steps == int(tr["depth"].sum())
    lsz = 4 if xgb else 8
    for c in range(info.n_chunks):
        k = np.flatnonzero(tr["chunk"] == c)
        t, data = tr[k], int(lay["chunk_lengths"][c]) - 1024
        assert 0 < data <= BUF[wide]
        nb = int(t["bundle"].max()) + 1
        assert nb <= S_MAX and set(t["bundle"]) == set(range(nb))
        # blocks: aligned to their size, inside the data bytes, none overlapping
        spans = []
        for r in t:
            assert r["node_offset"] % (4 << r["depth"]) == 0 and r["leaf_offset"] % lsz == 0
            spans += [(int(r["node_offset"]), 4 << int(r["depth"])), (int(r["leaf_offset"]), lsz << int(r["depth"]))]
        spans.sort()
        assert all(a + n <= b for (a, n), (b, _) in zip(spans, spans[1:])) and sum(spans[-1]) <= data
        # bundles: at most tpg trees, one depth (the deepest of its trees' own), one tree group
        dsum = np.zeros(4, np.int64)
        for b in range(nb):
            m = t[t["bundle"] == b]
            assert 1 <= len(m) <= tpg and len(set(m["depth"])) == 1 and len(set(m["group"])) == 1
            assert m["depth"][0] == own[k[t["bundle"] == b]].max()
            assert 0 <= m["group"][0] < 4
            dsum[m["group"][0]] += m["depth"][0]
        assert dsum.max() - dsum.min() <= t["depth"].max()
        # the chunk table
        tab = DC.chunk_table(lay, c)
        assert tab[0] == len(k) | (nb << 8)
        nxt = (int(lay["chunk_offsets"][c + 1]) >> 10, int(lay["chunk_lengths"][c + 1]) >> 10) \
            if c + 1 < info.n_chunks else (0, 0)
        assert (int(tab[1]), int(tab[2])) == nxt
        seen = set()
        for g in range(4):
            last = 9
            for i in range((int(tab[3]) >> (8 * g)) & 0xFF):
                e = tab[(64 + 128 * g + 16 * i) // 4:][:4]
                d, b = int(e[0]) & 0xFF, (int(e[0]) >> 8) & 0xFF
                assert (int(e[0]) >> 16) == g and b not in seen and d <= last  # deepest first within a group
                seen.add(b)
                last = d
                m = t[t["bundle"] == b]
                assert d == m["depth"][0] and g == m["group"][0]
                offs = [(int(e[1 + j // 2]) >> (16 * (j & 1))) & 0xFFFF for j in range(6)]
                place = {int(tab[576 // 4 + q]) & 0xFFFF: q for q in range(len(k))}
                for j in range(6):  # place j of the bundle: its tree's block, or the first tree's again
                    q = place.get(2048 * b + j)
                    want = t[q]["node_offset"] if q is not None else offs[0]
                    assert offs[j] == want and (q is not None or j >= len(m))
        assert seen == set(range(nb))
        ent = tab[576 // 4:][:len(k)]
        assert len(set(ent & 0xFFFF)) == len(k)
        np.testing.assert_array_equal(ent >> 16, t["leaf_offset"])
        np.testing.assert_array_equal((ent & 0xFFFF) // 2048, t["bundle"])
        assert ((ent & 0xFFFF) % 2048 < tpg).all()
    if mode == 3:  # ensemble_contract 1's rule: each tree to the deepest of trees i / tpg
        want = [own[i // tpg * tpg:i // tpg * tpg + tpg].max() for i in range(T)]
        np.testing.assert_array_equal(tr["depth"], want)
        first = {c: int(np.flatnonzero(tr["chunk"] == c)[0]) for c in range(info.n_chunks)}
        np.testing.assert_array_equal(tr["bundle"], [(i - first[int(tr["chunk"][i])]) // tpg for i in range(T)])
        assert all(v % tpg == 0 for v in first.values())


@pytest.mark.parametrize("wide", [True, False], ids=["wide", "compact"])
@pytest.mark.parametrize("name", sorted(FORESTS))
def test_layout_and_leaf_values(name, wide):
    fa = FORESTS[name]
    xgb = fa.kind == N.FD_FOREST_XGB_BINARY_LOGISTIC
    X, want = _plain_walk(name)
    if xgb:
        want = want.astype(np.float32).astype(np.float64)
    steps = {}
    for mode in (3, 4):
        lay = dense_layout_host(fa, wide=wide, mode=mode)
        check_layout(fa, lay, wide, mode)
        np.testing.assert_array_equal(DC.walk_blob(lay, xgb, X), want)
        steps[mode] = lay["info"].node_steps
    assert steps[4] <= steps[3]


def test_caps_end_the_chunks():
    tpg = TPG[True, True]
    lay = dense_layout_host(FORESTS["shallow200"], wide=True, mode=4)
    per = np.bincount(lay["trees"]["chunk"])
    assert (per[:-1] == S_MAX * tpg).all() and (lay["chunk_lengths"][:-1] - 1024 < BUF[True] // 2).all()  # bundle cap
    lay = dense_layout_host(FORESTS["deep_then_shallow"], wide=True, mode=3)
    per = np.bincount(lay["trees"]["chunk"])
    assert per[0] == 24 and lay["chunk_lengths"][0] == BUF[True] + 1024  # byte cap: four depth-8 bundles fill it
    assert per.max() > 24  # the shallow tail packs more trees per chunk than a depth-8 chunk holds


@pytest.mark.parametrize("kind", ["xgb", "iforest"])
def test_depth_8_forest_keeps_todays_chunks(kind):
    fa = DC.on_varying(xgboost_from_json_doc(synth.xgboost_doc(50, 8, 64, H.vectors(2000, 9), seed=28)))
    if kind == "iforest":
        fa = DC.as_iforest(fa, 29)
    for wide, ch in ((True, (24, 16)), (False, (20, 12))):
        per = ch[0] if kind == "xgb" else ch[1]
        for mode in (3, 4):
            lay = dense_layout_host(fa, wide=wide, mode=mode)
            assert (lay["trees"]["depth"] == 8).all()
            np.testing.assert_array_equal(lay["trees"]["chunk"], np.arange(50) // per)


def test_owner_bias_lightens_group_0():
    fa = FORESTS["fifty"]
    a, b = (dense_layout_host(fa, wide=True, mode=4, owner_bias=k)["trees"] for k in (0, 16))
    d0 = lambda t: sum(int(x) for x in {(int(r["chunk"]), int(r["bundle"])): int(r["depth"])  # noqa: E731
                                        for r in t if r["group"] == 0}.values())
    assert d0(b) <= d0(a)
    np.testing.assert_array_equal(a["depth"], b["depth"])
