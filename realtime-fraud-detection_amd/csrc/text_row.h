// text_row.h — the text analyzer's fraud patterns and numeric features: the byte classes, the keyword table, the
// Aho–Corasick automaton over it and the f64 epilogue, shared by the kernels (text.hip) and the pure host form
// (fd_text_features_ref_host). Self-contained (no HIP, no engine headers) so the host form also compiles into a
// stand-alone program.
// Reference: BertTextAnalyzer (ml/models/bert_text_analyzer.py)
//   detect_fraud_patterns   :283-344   five flags: any keyword of a list is a substring of the lower-cased join
//   get_text_features       :346-399   fourteen numbers of merchant_name and description
// Declared rule: a row is four fields merchant_name, description, category, location; rows with a
// byte >= 0x80 in any field are not computed (FD_TEXT_NONASCII, outputs 0). For ASCII rows the text searched is
// m ' ' d ' ' c ' ' l with A-Z folded onto a-z; the features count bytes of m and d by class.
#pragma once

#include <cstdint>
#include <cstring>
#include <string>

#if defined(__HIPCC__)
#define FD_TEXT_HD __host__ __device__ __forceinline__
#else
#define FD_TEXT_HD inline
#endif

#define FD_TEXT_COLS 14  // FD_TEXT_FEATURES, in the reference's dict order

namespace fd {

// ---------------------------------------------------------------- byte classes (ASCII)
// Space is what Python's \s and str.split() take below 0x80: 0x09-0x0D, 0x1C-0x1F and 0x20.
FD_TEXT_HD bool text_is_space(uint32_t c) { return c == 0x20u || (c - 0x09u) < 5u || (c - 0x1cu) < 4u; }
FD_TEXT_HD bool text_is_digit(uint32_t c) { return (c - (uint32_t)'0') < 10u; }
FD_TEXT_HD bool text_is_alpha(uint32_t c) { return ((c | 0x20u) - (uint32_t)'a') < 26u; }
// str.lower() of an ASCII byte
FD_TEXT_HD uint32_t text_fold(uint32_t c) { return (c - (uint32_t)'A') < 26u ? c + 32u : c; }

// ---------------------------------------------------------------- the keyword lists (here and nowhere else)
constexpr int kTextPatterns = 5;  // bit 0 crypto_keywords, 1 gift_card_keywords, 2 urgent_language,
                                  // 3 suspicious_merchant, 4 known_scam_patterns
struct TextKeyword {
  const char* s;  // a-z and 0x20 only
  int bit;
};
constexpr TextKeyword kTextKeywords[] = {
    {"bitcoin", 0},       {"btc", 0},        {"ethereum", 0},     {"eth", 0},           {"crypto", 0},
    {"blockchain", 0},    {"coinbase", 0},   {"binance", 0},      {"wallet", 0},        {"mining", 0},
    {"satoshi", 0},
    {"gift card", 1},     {"giftcard", 1},   {"itunes", 1},       {"amazon card", 1},   {"google play", 1},
    {"steam card", 1},    {"prepaid card", 1}, {"reload card", 1},
    {"urgent", 2},        {"emergency", 2},  {"immediate", 2},    {"quickly", 2},       {"asap", 2},
    {"limited time", 2},  {"act now", 2},    {"expires soon", 2},
    {"temp", 3},          {"temporary", 3},  {"cash advance", 3}, {"payday", 3},        {"loan", 3},
    {"invest", 3},        {"forex", 3},      {"trading", 3},      {"pyramid", 3},       {"mlm", 3},
    {"nigerian prince", 4}, {"inheritance", 4}, {"lottery winner", 4}, {"tax refund", 4}, {"irs", 4},
    {"social security", 4}, {"medicare", 4}, {"warranty expired", 4},
};
constexpr int kTextKeywordCount = (int)(sizeof(kTextKeywords) / sizeof(kTextKeywords[0]));
constexpr int kTextMaxKeyword = 16;  // bytes of the longest keyword ("warranty expired", "social security")
static_assert(kTextKeywordCount == 45, "11 + 8 + 8 + 10 + 8 keywords");

// ---------------------------------------------------------------- the automaton
// One Aho–Corasick automaton over all 45 keywords, as a complete transition table (the failure links are folded in)
// over 28 symbol classes: a-z (upper case folded), 0x20, and everything else. Entry [state * 28 + symbol] is the
// target state in its low 9 bits and, above them, the target's 5-bit output mask (the lists with a keyword ending
// there, closed over the failure links), so one read per byte gives both.
constexpr int kTextSymbols = 28;
constexpr int kTextSymSpace = 26, kTextSymOther = 27;
constexpr int kTextMaxStates = 400;
constexpr int kTextStateBits = 9;

FD_TEXT_HD uint32_t text_symbol(uint32_t c) {
  const uint32_t l = (c | 0x20u) - (uint32_t)'a';
  return l < 26u ? l : (c == 0x20u ? (uint32_t)kTextSymSpace : (uint32_t)kTextSymOther);
}

struct TextAutomaton {
  uint16_t next[kTextMaxStates * kTextSymbols];
  int states;
};

constexpr TextAutomaton text_build_automaton() {
  TextAutomaton a{};
  int16_t go[kTextMaxStates * kTextSymbols] = {};  // the trie: 0 = no edge (no edge leads back to the root)
  uint8_t out[kTextMaxStates] = {};
  int16_t fail[kTextMaxStates] = {};
  int16_t dfa[kTextMaxStates * kTextSymbols] = {};
  int n = 1;
  for (int k = 0; k < kTextKeywordCount; ++k) {
    int s = 0;
    for (const char* p = kTextKeywords[k].s; *p; ++p) {
      const int sym = *p == ' ' ? kTextSymSpace : *p - 'a';
      if (go[s * kTextSymbols + sym] == 0) go[s * kTextSymbols + sym] = (int16_t)n++;
      s = go[s * kTextSymbols + sym];
    }
    out[s] = (uint8_t)(out[s] | (1u << kTextKeywords[k].bit));
  }
  int16_t queue[kTextMaxStates] = {};
  int head = 0, tail = 0;
  queue[tail++] = 0;
  while (head < tail) {  // breadth first: a state's failure target is shallower, so its row is complete
    const int s = queue[head++];
    for (int sym = 0; sym < kTextSymbols; ++sym) {
      const int t = go[s * kTextSymbols + sym];
      const int via_fail = s == 0 ? 0 : dfa[fail[s] * kTextSymbols + sym];
      if (t != 0) {
        fail[t] = (int16_t)via_fail;
        out[t] = (uint8_t)(out[t] | out[via_fail]);
        dfa[s * kTextSymbols + sym] = (int16_t)t;
        queue[tail++] = (int16_t)t;
      } else {
        dfa[s * kTextSymbols + sym] = (int16_t)via_fail;
      }
    }
  }
  for (int i = 0; i < n * kTextSymbols; ++i)
    a.next[i] = (uint16_t)((unsigned)dfa[i] | ((unsigned)out[dfa[i]] << kTextStateBits));
  a.states = n;
  return a;
}

// one step: the entry read for (state, symbol) -> new state; its mask is entry >> kTextStateBits
FD_TEXT_HD uint32_t text_state_of(uint32_t entry) { return entry & ((1u << kTextStateBits) - 1u); }

// ---------------------------------------------------------------- the epilogue
// What the scans leave per row: byte counts of merchant_name (m) and description (d), the set of byte values of m
// after folding (bit c of seen[c / 32]), the flags.
struct TextRowCounts {
  int64_t len_m, len_d;
  int64_t num_m, num_d;    // digits
  int64_t spec_m, spec_d;  // neither alpha, digit nor space
  int64_t word_m, word_d;  // maximal runs of non-space bytes
  uint32_t seen[4];
};

FD_TEXT_HD int text_popcount32(uint32_t v) {
  v = v - ((v >> 1) & 0x55555555u);
  v = (v & 0x33333333u) + ((v >> 2) & 0x33333333u);
  return (int)((((v + (v >> 4)) & 0x0f0f0f0fu) * 0x01010101u) >> 24);
}

// the fourteen features in the reference's dict order; one f64 division
FD_TEXT_HD void text_row_features(const TextRowCounts& r, double* out) {
#pragma clang fp contract(off)
  const int64_t uniq = text_popcount32(r.seen[0]) + text_popcount32(r.seen[1]) + text_popcount32(r.seen[2]) +
                       text_popcount32(r.seen[3]);
  out[0] = (double)r.len_m;
  out[1] = (double)r.len_d;
  out[2] = (double)(r.len_m + r.len_d);
  out[3] = (double)uniq;  // 0 for an empty m: nothing was seen
  out[4] = r.len_m > 0 ? (double)uniq / (double)r.len_m : 0.0;
  out[5] = (double)r.num_m;
  out[6] = (double)r.num_d;
  out[7] = (double)(r.num_m + r.num_d);
  out[8] = (double)r.spec_m;
  out[9] = (double)r.spec_d;
  out[10] = (double)(r.spec_m + r.spec_d);
  out[11] = (double)r.word_m;
  out[12] = (double)r.word_d;
  out[13] = (double)(r.word_m + r.word_d);
}

// off[0] == 0 and non-decreasing over its 4n + 1 entries
inline bool text_offsets_valid(const int64_t* off, int64_t n) {
  if (off[0] != 0) return false;
  for (int64_t k = 0; k < 4 * n; ++k)
    if (off[k + 1] < off[k]) return false;
  return true;
}

// ---------------------------------------------------------------- the declared rule by direct scans, on the host
// No automaton: the joined text is built and each keyword searched for in turn. Any output may be null.
inline void text_features_rows_host(const uint8_t* bytes, const int64_t* off, int64_t n, double* feat,
                                    uint8_t* patterns, uint8_t* status) {
  std::string joined;
  for (int64_t i = 0; i < n; ++i) {
    const int64_t* o = off + 4 * i;
    bool ascii = true;
    for (int64_t p = o[0]; p < o[4]; ++p) ascii = ascii && bytes[p] < 0x80;
    double row[FD_TEXT_COLS] = {};
    uint8_t flags = 0;
    if (ascii) {
      TextRowCounts r{};
      int64_t* const len[2] = {&r.len_m, &r.len_d};
      int64_t* const num[2] = {&r.num_m, &r.num_d};
      int64_t* const spec[2] = {&r.spec_m, &r.spec_d};
      int64_t* const word[2] = {&r.word_m, &r.word_d};
      for (int f = 0; f < 2; ++f) {
        *len[f] = o[f + 1] - o[f];
        bool in_word = false;
        for (int64_t p = o[f]; p < o[f + 1]; ++p) {
          const uint32_t c = bytes[p];
          const bool sp = text_is_space(c);
          if (text_is_digit(c)) ++*num[f];
          if (!sp && !text_is_digit(c) && !text_is_alpha(c)) ++*spec[f];
          if (!sp && !in_word) ++*word[f];
          in_word = !sp;
          if (f == 0) {
            const uint32_t l = text_fold(c);
            r.seen[l >> 5] |= 1u << (l & 31u);
          }
        }
      }
      text_row_features(r, row);
      joined.clear();
      for (int f = 0; f < 4; ++f) {
        if (f) joined.push_back(' ');
        for (int64_t p = o[f]; p < o[f + 1]; ++p) joined.push_back((char)text_fold(bytes[p]));
      }
      for (int k = 0; k < kTextKeywordCount; ++k)
        if (joined.find(kTextKeywords[k].s, 0, std::strlen(kTextKeywords[k].s)) != std::string::npos)
          flags = (uint8_t)(flags | (1u << kTextKeywords[k].bit));
    }
    if (feat) std::memcpy(feat + i * FD_TEXT_COLS, row, sizeof(row));
    if (patterns) patterns[i] = flags;
    if (status) status[i] = ascii ? 0 : 1;  // FD_TEXT_NONASCII
  }
}

}  // namespace fd
