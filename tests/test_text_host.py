"""CPU: the text patterns' and features' declared rule against the reference's own outputs
(tests/golden/text_cases.npz, written by golden/make_text_golden.py from BertTextAnalyzer.detect_fraud_patterns and
get_text_features): the pure host form fd_text_features_ref_host bit-equal on every ASCII row, the status vector
exactly the isascii rule, the argument errors, the drop-in's host fallback on the non-ASCII rows, the automaton of
csrc/text_row.h against plain substring search, and the new kernels' resource remarks."""
import ctypes as C
import json
import subprocess

import numpy as np
import pytest

import text_cases as T


@pytest.fixture(scope="module")
def fixture():
    return T.load_fixture()


def test_module_imports_and_names_agree():
    import fdengine.text as M
    from fdengine import _native as N
    assert M.BertTextAnalyzer.__init__.__code__.co_varnames[:4] == ("self", "model_path", "device", "engine")
    assert N.TEXT_COLUMNS == T.COLUMNS == M.COLUMNS and N.TEXT_PATTERNS == T.PATTERNS and N.TEXT_FIELDS == T.FIELDS
    assert (N.FD_TEXT_FIELDS, N.FD_TEXT_PATTERNS, N.FD_TEXT_FEATURES, N.FD_TEXT_NONASCII) == (4, 5, 14, 1)
    assert N.FD_TEXT_FEATURES == len(N.TEXT_COLUMNS) and N.FD_TEXT_PATTERNS == len(N.TEXT_PATTERNS)
    assert N.FD_TIMING_TEXT == 11


def test_keyword_table_shape():
    kws = T.keywords()
    assert [sum(1 for _, b in kws if b == k) for k in range(5)] == [11, 8, 8, 10, 8]
    assert max(len(k) for k, _ in kws) == 16 and all(set(k) <= set("abcdefghijklmnopqrstuvwxyz ") for k, _ in kws)
    assert len(T.two_word(kws)) == 15


def test_fixture_holds_the_cases_it_should(fixture):
    g = fixture["groups"]
    n = len(fixture["patterns"])
    assert list(g) == ["keyword_hits", "near_misses", "boundary_hits", "boundary_misses", "positions",
                       "byte_classes", "whitespace", "word_counts", "unique", "random", "non_ascii"]
    assert g["keyword_hits"][1] - g["keyword_hits"][0] == 45 * 4 * 3 and g["byte_classes"][1] - g["byte_classes"][0] == 512
    assert g["random"][1] - g["random"][0] >= 2000
    assert 30 <= fixture["nonascii"].sum() <= 0.05 * n
    rows = T.decode(fixture["blob"], fixture["off"])
    isascii = np.array([all(s.isascii() for s in r.values()) for r in rows])
    assert (isascii == ~fixture["nonascii"]).all()
    lo, hi = g["random"]
    for b in range(5):
        share = ((fixture["patterns"][lo:hi] >> b) & 1).mean()
        assert 0.10 <= share <= 0.90
    assert fixture["feat"][hi - 1, 1] == T.LONG_ROW and fixture["patterns"][hi - 1] == 16
    assert fixture["feat"][g["unique"][0] + 1, 3] == 102
    assert T.GOLDEN.stat().st_size <= 256 * 1024


def test_ref_host_equals_reference(fixture):
    got = T.ref_host(fixture["blob"], fixture["off"])
    T.assert_matches(got, T.expected_native(fixture), "fixture")
    # and exactly the non-ASCII rows are flagged, with zero outputs
    bad = fixture["nonascii"]
    assert (got[2] == bad * T.NONASCII).all()
    assert not got[0][bad].any() and not got[1][bad].any()


def test_ref_host_does_not_depend_on_the_cut(fixture):
    whole = T.ref_host(fixture["blob"], fixture["off"])
    n = len(whole[1])
    for lo, hi in ((0, 1), (5, 5), (1000, 1777), (n - 300, n)):
        part = T.ref_host(*T.slice_rows(fixture["blob"], fixture["off"], lo, hi))
        T.assert_matches(part, tuple(w[lo:hi] for w in whole), f"rows {lo}:{hi}")


def test_null_outputs_and_empty_calls(fixture):
    blob, off = T.slice_rows(fixture["blob"], fixture["off"], 0, 50)
    full = T.ref_host(blob, off)
    for want in ((True, False, False), (False, True, False), (False, False, True), (False, False, False)):
        got = T.ref_host(blob, off, want)
        for g, f, w in zip(got, full, want):
            assert (g is None) if not w else (g.tobytes() == f.tobytes())
    from fdengine import _native as N
    assert N.lib.fd_text_features_ref_host(None, None, 0, None, None, None) == N.FD_OK  # n = 0 reads nothing
    # all rows empty: the blob may be null
    off0 = np.zeros(4 * 3 + 1, np.int64)
    feat, pat, st = T.ref_host(np.zeros(0, np.uint8), off0)
    assert not feat.any() and not pat.any() and not st.any()


def test_argument_errors_return_status_codes():
    from fdengine import _native as N
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    blob = np.frombuffer(b"abcdefgh", np.uint8)
    feat, pat, st = np.zeros((2, 14)), np.zeros(2, np.uint8), np.zeros(2, np.uint8)
    f = N.lib.fd_text_features_ref_host
    good = np.array([0, 1, 2, 3, 4, 5, 6, 7, 8], np.int64)
    assert f(p(blob), p(good), 2, p(feat), p(pat), p(st)) == N.FD_OK
    for bad in ([1, 1, 2, 3, 4, 5, 6, 7, 8], [0, 1, 2, 3, 4, 5, 4, 7, 8], [0, 1, 2, 3, 4, 5, 6, 7, 6],
                [0, -1, 2, 3, 4, 5, 6, 7, 8]):
        assert f(p(blob), p(np.array(bad, np.int64)), 2, p(feat), p(pat), p(st)) == N.FD_ERR_INVALID_ARG, bad
        assert b"offsets" in N.lib.fd_last_error()
    assert f(p(blob), None, 2, p(feat), p(pat), p(st)) == N.FD_ERR_INVALID_ARG
    assert f(None, p(good), 2, p(feat), p(pat), p(st)) == N.FD_ERR_INVALID_ARG
    assert b"null" in N.lib.fd_last_error()
    assert f(p(blob), p(good), -1, p(feat), p(pat), p(st)) == N.FD_ERR_INVALID_ARG
    # engine entry points: a null engine is a status code, not a crash
    b = N.fd_text_batch()
    assert N.lib.fd_text_features_device(None, C.byref(b), 1, None, None, None) == N.FD_ERR_INVALID_ARG
    assert b"null engine" in N.lib.fd_last_error()
    assert N.lib.fd_text_features_host(None, C.byref(b), 1, None, None, None) == N.FD_ERR_INVALID_ARG


def test_declared_examples():
    rows = [T.row(m="Bethany"), T.row(d="first"), T.row(c="Sloan"), T.row(m="Gift", d="Card"),
            T.row(m="Gift", c="Card"), T.row(m="gift\tcard"), T.row(m=" \x1c "), T.row(m="AaBb"), T.row()]
    feat, pat, st = T.ref_host(*T.encode(rows))
    assert pat.tolist() == [1, 16, 8, 2, 0, 0, 0, 0, 0] and not st.any()
    assert feat[6, 3] == 2 and feat[6, 4] == 2 / 3 and feat[6, 11] == 0  # whitespace only: not empty, no words
    assert feat[7, 3] == 2 and feat[7, 4] == 0.5
    assert not feat[8].any()


def test_host_fallback_equals_reference_on_non_ascii_rows(fixture):
    from fdengine import text as M
    lo, hi = fixture["groups"]["non_ascii"]
    rows = T.decode(fixture["blob"], fixture["off"])[lo:hi]
    for i, r in enumerate(rows, lo):
        vals = [r[f] for f in T.FIELDS]
        f = M.features_of_str(vals[0], vals[1])
        assert np.array(f, np.float64).tobytes() == fixture["feat"][i].tobytes(), (i, r)
        assert M.patterns_of_str(vals) == fixture["patterns"][i], (i, r)
    # and on ASCII text it is the same rule as everywhere else
    for i in list(range(0, lo, 37)) + [fixture["groups"]["random"][1] - 1]:
        r = T.decode(*T.slice_rows(fixture["blob"], fixture["off"], i, i + 1))[0]
        vals = [r[f] for f in T.FIELDS]
        assert np.array(M.features_of_str(vals[0], vals[1]), np.float64).tobytes() == fixture["feat"][i].tobytes()
        assert M.patterns_of_str(vals) == fixture["patterns"][i]


def test_encode_rows_and_type_errors():
    from fdengine import text as M
    blob, off = M.encode_rows([{"merchant_name": "ab", "location": "é"}, {}])
    assert blob == "abé".encode() and off.tolist() == [0, 2, 2, 2, 4, 4, 4, 4, 4]
    blob, off = M.encode_rows([{"merchant_name": "ab", "category": "zz"}], M.FIELDS[:2])
    assert blob == b"ab" and off.tolist() == [0, 2, 2, 2, 2]
    for bad in (None, 5, b"bytes"):
        with pytest.raises(TypeError):
            M.encode_rows([{"description": bad}])


def host_cxx():
    """a C++ compiler for a host-only program: the system's, else the one hipcc drives"""
    import shutil
    from pathlib import Path

    from fdengine import build
    for name in ("g++", "c++", "clang++"):
        if shutil.which(name):
            return name
    rocm = Path(build._hipcc()).resolve().parent.parent
    for cand in (rocm / "llvm" / "bin" / "clang++", rocm / "lib" / "llvm" / "bin" / "clang++"):
        if cand.exists():
            return str(cand)
    pytest.fail("no host C++ compiler found")


AUTOMATON_PROGRAM = r"""
#include <cstdio>
#include <random>
#include <vector>
#include "text_row.h"
using namespace fd;
static const TextAutomaton A = text_build_automaton();
int main() {
  if (A.states > (1 << kTextStateBits)) return 2;
  std::mt19937 rng(7);
  // rows of one field over a small alphabet that makes keywords likely, walked by the automaton and by direct scans
  const char* pieces[] = {"bit", "coin", "eth", "gift", " ", "card", "act", "now", "temp", "orary", "irs", "x", "  ",
                          "GIFT", "Loan", "\t", "crypt", "o", "warranty", "expired", "mlm", "ml", "social", "security"};
  long checked = 0;
  for (int it = 0; it < 20000; ++it) {
    std::vector<uint8_t> b;
    const int parts = 1 + rng() % 6;
    for (int k = 0; k < parts; ++k)
      for (const char* p = pieces[rng() % 24]; *p; ++p) b.push_back((uint8_t)*p);
    const int64_t n = (int64_t)b.size();
    int64_t off[5] = {0, 0, 0, 0, n};
    for (int j = 1; j < 4; ++j) off[j] = n ? (int64_t)(rng() % (n + 1)) : 0;
    for (int j = 1; j < 4; ++j) if (off[j] < off[j - 1]) off[j] = off[j - 1];
    uint8_t want = 0;
    text_features_rows_host(b.data(), off, 1, nullptr, &want, nullptr);
    uint32_t state = 0, flags = 0;
    for (int64_t p = 0; p < n; ++p) {
      for (int j = 1; j < 4; ++j)
        if (off[j] == p) { const uint32_t e = A.next[state * kTextSymbols + kTextSymSpace]; state = text_state_of(e); flags |= e; }
      const uint32_t e = A.next[state * kTextSymbols + text_symbol(b[p])];
      state = text_state_of(e);
      flags |= e;
    }
    if (((flags >> kTextStateBits) & 31u) != want) { std::printf("MISMATCH at %d\n", it); return 1; }
    ++checked;
  }
  std::printf("states %d checked %ld\n", A.states, checked);
  return 0;
}
"""


def test_automaton_equals_plain_search(tmp_path):
    """the table the kernel walks (text_build_automaton, with the separators fed at the field boundaries) against the
    host form's keyword-by-keyword search, as a stand-alone host program"""
    src = tmp_path / "automaton.cpp"
    src.write_text(AUTOMATON_PROGRAM)
    exe = tmp_path / "automaton"
    subprocess.run([host_cxx(), "-std=c++17", "-O1", f"-I{T.HEADER.parent}", str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    assert "checked 20000" in out, out
    states = int(out.split()[1])
    assert 300 <= states <= 400


def test_text_kernels_use_no_scratch():
    from fdengine import _native as N
    res = json.loads((N.PKG_ROOT / "lib" / "kernel_resources.json").read_text())
    found = {}
    for name, r in res.items():
        for k in ("text_scan_kernel", "text_finish_kernel"):
            if k + "E" in name:  # (the mangled name: the identifier, then its parameter list)
                found[k] = r
    assert len(found) == 2, sorted(found)
    for k, r in found.items():
        assert r["scratch"] == 0, (k, r)
    assert found["text_scan_kernel"]["lds"] <= 40 * 1024  # four workgroups per CU
