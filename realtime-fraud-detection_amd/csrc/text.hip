// text.hip — the text analyzer's fraud patterns and numeric features (BertTextAnalyzer.detect_fraud_patterns and
// get_text_features, ml/models/bert_text_analyzer.py:283-399) over a batch of rows of four text fields.
//
// Rows run from 0 bytes to tens of thousands, so the work is cut by bytes, not by rows. The rows of a call are one
// contiguous byte stream (the blob; off gives its 4n + 1 field boundaries). text_scan_kernel walks it in tiles of
// kTextTile bytes: a workgroup stages a tile (and the kTextHalo bytes before it) into LDS with coalesced loads, then
// lane l takes the tile's bytes [l * kTextSeg, (l + 1) * kTextSeg): a long row is spread over many lanes and tiles,
// short rows share a lane. Everything a row needs is a sum or an OR of per-byte terms:
//   digit / special counts, the 128-bit seen-set   one byte at a time
//   word starts       a non-space byte whose predecessor is a space or the field's start: one byte of look-back
//   the five flags    the automaton of text_row.h; a lane enters its first row kTextMaxKeyword - 1 bytes early in
//                     state 0 (not before the row's start), which finds every keyword ending in its segment; what
//                     it finds in those early bytes is a true match of the same row, so OR-ing it in is harmless.
//                     The three separators of the join are fed before the byte at each field boundary.
// so a lane adds its part of each row it touched to the row's 12 words of accumulators with integer atomics, whose
// order does not matter: results do not depend on how rows fall on lanes, tiles, chunks or calls.
// text_finish_kernel (a lane per row) turns lengths and accumulators into the 14 f64 columns, flags and status.
//
// LDS: the automaton's table (u16 [states x 28], about 18 KB) and the tile. A lane reads its segment byte by byte, so
// the 32 lanes of an LDS access group read addresses kTextSeg = 64 B = 16 banks apart: 2 of the 32 banks, a 16-way
// conflict. Every 64 bytes of the tile are therefore followed by 4 bytes of padding (stride 17 banks, odd: the 32
// lanes hit 32 banks), and the staging writes a 16-byte global load as four 4-byte LDS stores.
//
// The grid is fixed (kTextGrid workgroups, each striding over the tiles): the device entry point knows the call's byte
// count only on the device (off[4n]) and reads nothing back. Per chunk of at most kTextChunk rows, on the caller's
// stream: a memset of the accumulators, text_scan_kernel, text_finish_kernel.
#include <algorithm>

#include "fd_internal.h"
#include "text_row.h"

namespace fd {
namespace {

constexpr int kTextThreads = 256;                     // threads per workgroup of both kernels
constexpr int kTextSeg = 64;                          // tile bytes per lane
constexpr int kTextTile = kTextThreads * kTextSeg;    // bytes per LDS tile (the staging span): 16384
constexpr int kTextHalo = 16;                         // bytes staged before the tile (>= kTextMaxKeyword - 1)
constexpr int kTextGrid = 1024;                       // workgroups of the scan kernel (4 per CU)
constexpr int kTextAcc = 12;                          // u32 accumulators per row, below
constexpr int kTextPre = kTextMaxKeyword - 1;         // bytes a lane enters its first row early
static_assert(kTextHalo >= kTextPre && kTextHalo % 16 == 0 && kTextSeg % 16 == 0, "the halo covers the early bytes");

// accumulators of a row: digits, specials, word starts of m and d; the seen-set of m; flags | nonascii << 8
enum { kAccNumM = 0, kAccNumD, kAccSpecM, kAccSpecD, kAccWordM, kAccWordD, kAccSeen, kAccFlags = kAccSeen + 4 };
static_assert(kAccFlags < kTextAcc, "12 words");

constexpr TextAutomaton kTextAutomatonHost = text_build_automaton();
constexpr int kTextStates = kTextAutomatonHost.states;
static_assert(kTextStates <= (1 << kTextStateBits) && kTextStates <= kTextMaxStates, "a state fits 9 bits");
__device__ const TextAutomaton d_text_automaton = text_build_automaton();

// LDS byte address of tile coordinate q (0 = the first halo-block byte; the tile's byte 0 is q = kTextSeg)
__device__ __forceinline__ int text_lds(int q) { return q + (q >> 6) * 4; }
constexpr int kTextLdsBytes = (kTextTile + kTextSeg) / 64 * 68;

__device__ __forceinline__ int text_rel(int64_t pos, int64_t base) {
  const int64_t d = pos - base;
  return (int)(d < -(1 << 30) ? -(1 << 30) : (d > (1 << 30) ? (1 << 30) : d));
}

// the largest r in [lo, hi] with off[4r] <= pos (off[4 lo] <= pos): the row holding byte pos, if it is a row's byte
__device__ __forceinline__ int text_row_of(const int64_t* __restrict__ off, int lo, int hi, int64_t pos) {
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (off[4 * (int64_t)mid] <= pos) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// off: the chunk's 4c + 1 boundaries (absolute positions in bytes); acc: c x kTextAcc, zeroed
__global__ void __launch_bounds__(kTextThreads) text_scan_kernel(const uint8_t* __restrict__ bytes,
                                                                 const int64_t* __restrict__ off, int c,
                                                                 uint32_t* __restrict__ acc) {
  __shared__ uint16_t s_next[kTextStates * kTextSymbols];
  __shared__ __attribute__((aligned(16))) uint8_t s_tile[kTextLdsBytes];
  __shared__ int s_rows[2];
  const int tid = threadIdx.x;
  const int64_t B0 = off[0], B1 = off[4 * (int64_t)c];
  if (B1 <= B0) return;  // (the whole grid) nothing but empty rows
  for (int k = tid; k < kTextStates * kTextSymbols; k += kTextThreads) s_next[k] = d_text_automaton.next[k];
  const bool aligned = (reinterpret_cast<uintptr_t>(bytes) & 15u) == 0;
  const int64_t T0 = B0 / kTextTile, T1 = (B1 + kTextTile - 1) / kTextTile;
  for (int64_t t = T0 + blockIdx.x; t < T1; t += gridDim.x) {
    const int64_t base = t * kTextTile;
    __syncthreads();  // the previous tile's reads
    // stage [base - kTextHalo, base + kTextTile) below B1, 16 bytes per thread and step (bytes before B0 belong to an
    // earlier chunk of the same blob: staged, never used)
    const int64_t slo = base >= kTextHalo ? base - kTextHalo : 0;
    const int groups = (int)((std::min<int64_t>(base + kTextTile, B1) - slo + 15) >> 4);
    for (int g = tid; g < groups; g += kTextThreads) {
      const int64_t pos = slo + 16 * (int64_t)g;
      const int a = text_lds((int)(pos - base) + kTextSeg);
      if (aligned && pos + 16 <= B1) {
        const uint4 v = *reinterpret_cast<const uint4*>(bytes + pos);
        uint32_t* w = reinterpret_cast<uint32_t*>(s_tile + a);  // (4-byte aligned: a 16-byte store would not be)
        w[0] = v.x;
        w[1] = v.y;
        w[2] = v.z;
        w[3] = v.w;
      } else {
        const int cnt = (int)std::min<int64_t>(16, B1 - pos);
        for (int k = 0; k < cnt; ++k) s_tile[a + k] = bytes[pos + k];
      }
    }
    if (tid == 0) s_rows[0] = text_row_of(off, 0, c - 1, std::max(base, B0));
    if (tid == 1) s_rows[1] = text_row_of(off, 0, c - 1, std::min<int64_t>(base + kTextTile, B1) - 1);
    __syncthreads();
    // this lane's bytes, in tile coordinates x (position base + x): [own, lim)
    int own = std::max(tid * kTextSeg, text_rel(B0, base));
    const int lim = std::min((tid + 1) * kTextSeg, text_rel(B1, base));
    if (own >= lim) continue;
    int r = text_row_of(off, s_rows[0], s_rows[1], base + own);
    for (;;) {
      const int64_t* o = off + 4 * (int64_t)r;
      const int q0 = text_rel(o[0], base), q1 = text_rel(o[1], base), q2 = text_rel(o[2], base),
                q3 = text_rel(o[3], base), q4 = text_rel(o[4], base);
      const int end = std::min(q4, lim);
      uint32_t state = 0, flags = 0, nonascii = 0;
      uint32_t num_m = 0, num_d = 0, spec_m = 0, spec_d = 0, word_m = 0, word_d = 0;
      uint64_t seen_lo = 0, seen_hi = 0;
      bool prev_space = false;
      for (int x = std::max(q0, own - kTextPre); x < end; ++x) {
        const uint32_t ch = s_tile[text_lds(x + kTextSeg)];
        // the join's separators stand before the first byte of description, category and location
        uint32_t e;
        if (x == q1) { e = s_next[state * kTextSymbols + kTextSymSpace]; state = text_state_of(e); flags |= e; }
        if (x == q2) { e = s_next[state * kTextSymbols + kTextSymSpace]; state = text_state_of(e); flags |= e; }
        if (x == q3) { e = s_next[state * kTextSymbols + kTextSymSpace]; state = text_state_of(e); flags |= e; }
        e = s_next[state * kTextSymbols + text_symbol(ch)];
        state = text_state_of(e);
        flags |= e;
        const bool sp = text_is_space(ch);
        if (x >= own) {
          const bool in_m = x < q1, in_d = x >= q1 && x < q2;
          const bool dg = text_is_digit(ch);
          const bool spec = !sp && !dg && !text_is_alpha(ch);
          const bool word = !sp && (prev_space || x == q0 || x == q1);
          nonascii |= ch >> 7;
          num_m += (in_m && dg) ? 1u : 0u;
          num_d += (in_d && dg) ? 1u : 0u;
          spec_m += (in_m && spec) ? 1u : 0u;
          spec_d += (in_d && spec) ? 1u : 0u;
          word_m += (in_m && word) ? 1u : 0u;
          word_d += (in_d && word) ? 1u : 0u;
          const uint32_t l = text_fold(ch) & 127u;
          const uint64_t bit = in_m ? 1ull << (l & 63u) : 0ull;
          seen_lo |= l < 64u ? bit : 0ull;
          seen_hi |= l < 64u ? 0ull : bit;
        }
        prev_space = sp;
      }
      uint32_t* ar = acc + (int64_t)r * kTextAcc;
      if (num_m) atomicAdd(ar + kAccNumM, num_m);
      if (num_d) atomicAdd(ar + kAccNumD, num_d);
      if (spec_m) atomicAdd(ar + kAccSpecM, spec_m);
      if (spec_d) atomicAdd(ar + kAccSpecD, spec_d);
      if (word_m) atomicAdd(ar + kAccWordM, word_m);
      if (word_d) atomicAdd(ar + kAccWordD, word_d);
      if ((uint32_t)seen_lo) atomicOr(ar + kAccSeen, (uint32_t)seen_lo);
      if ((uint32_t)(seen_lo >> 32)) atomicOr(ar + kAccSeen + 1, (uint32_t)(seen_lo >> 32));
      if ((uint32_t)seen_hi) atomicOr(ar + kAccSeen + 2, (uint32_t)seen_hi);
      if ((uint32_t)(seen_hi >> 32)) atomicOr(ar + kAccSeen + 3, (uint32_t)(seen_hi >> 32));
      const uint32_t fl = ((flags >> kTextStateBits) & 31u) | (nonascii << 8);
      if (fl) atomicOr(ar + kAccFlags, fl);
      if (end >= lim) break;
      own = end;  // the next row with a byte: base + own < B1 = off[4c], so r stays below c
      do ++r;
      while (off[4 * (int64_t)r + 4] <= base + own);
    }
  }
}

__global__ void __launch_bounds__(kTextThreads) text_finish_kernel(const int64_t* __restrict__ off, int c,
                                                                   const uint32_t* __restrict__ acc,
                                                                   double* __restrict__ feat,
                                                                   uint8_t* __restrict__ patterns,
                                                                   uint8_t* __restrict__ status,
                                                                   unsigned long long* __restrict__ nonascii_rows) {
  const int i = blockIdx.x * kTextThreads + threadIdx.x;
  bool bad = false;
  if (i < c) {
    const int64_t* o = off + 4 * (int64_t)i;
    const uint32_t* a = acc + (int64_t)i * kTextAcc;
    bad = (a[kAccFlags] >> 8) != 0;
    TextRowCounts r;
    r.len_m = o[1] - o[0];
    r.len_d = o[2] - o[1];
    r.num_m = a[kAccNumM];
    r.num_d = a[kAccNumD];
    r.spec_m = a[kAccSpecM];
    r.spec_d = a[kAccSpecD];
    r.word_m = a[kAccWordM];
    r.word_d = a[kAccWordD];
    for (int k = 0; k < 4; ++k) r.seen[k] = a[kAccSeen + k];
    if (feat) {
      double row[FD_TEXT_COLS];
      text_row_features(r, row);
      for (int k = 0; k < FD_TEXT_COLS; ++k) feat[(int64_t)i * FD_TEXT_COLS + k] = bad ? 0.0 : row[k];
    }
    if (patterns) patterns[i] = bad ? 0 : (uint8_t)(a[kAccFlags] & 31u);
    if (status) status[i] = bad ? FD_TEXT_NONASCII : 0;
  }
  const unsigned long long m = __ballot(bad);
  if (m != 0 && (threadIdx.x & 63) == 0) atomicAdd(nonascii_rows, (unsigned long long)__popcll(m));
}

}  // namespace

int64_t text_nonascii_rows(Engine& e) {
  if (!e.text.count.ptr) return 0;
  unsigned long long v = 0;
  FD_HIP(hipStreamSynchronize(e.stream));
  FD_HIP(hipMemcpy(&v, e.text.count.ptr, sizeof(v), hipMemcpyDeviceToHost));
  return (int64_t)v;
}

void text_features(Engine& e, const uint8_t* d_bytes, const int64_t* d_off, int64_t n, double* d_feat,
                   uint8_t* d_patterns, uint8_t* d_status) {
  FD_REQUIRE(n >= 0 && n < (1ll << 31), FD_ERR_INVALID_ARG, "batch size out of range");
  if (n == 0) return;
  FD_REQUIRE(d_off, FD_ERR_INVALID_ARG, "null text offsets");
  TextState& s = e.text;
  hipStream_t st = e.stream;
  if (!s.count.ptr) {
    s.count.ensure(sizeof(unsigned long long));
    FD_HIP(hipMemsetAsync(s.count.ptr, 0, sizeof(unsigned long long), st));
  }
  s.acc.ensure((size_t)std::min<int64_t>(n, kTextChunk) * kTextAcc * sizeof(uint32_t));
  Engine::Timed* ev = e.timing ? e.next_event_pair(FD_TIMING_TEXT) : nullptr;
  if (ev) FD_HIP(hipEventRecord(ev->a, st));
  for (int64_t a = 0; a < n; a += kTextChunk) {
    const int c = (int)std::min<int64_t>(kTextChunk, n - a);
    FD_HIP(hipMemsetAsync(s.acc.ptr, 0, (size_t)c * kTextAcc * sizeof(uint32_t), st));
    hipLaunchKernelGGL(text_scan_kernel, dim3(kTextGrid), dim3(kTextThreads), 0, st, d_bytes, d_off + 4 * a, c,
                       s.acc.as<uint32_t>());
    hipLaunchKernelGGL(text_finish_kernel, dim3((unsigned)((c + kTextThreads - 1) / kTextThreads)),
                       dim3(kTextThreads), 0, st, d_off + 4 * a, c, s.acc.as<uint32_t>(),
                       d_feat ? d_feat + a * FD_TEXT_COLS : nullptr, d_patterns ? d_patterns + a : nullptr,
                       d_status ? d_status + a : nullptr, s.count.as<unsigned long long>());
    FD_HIP(hipGetLastError());
  }
  ++s.calls;
  if (ev) FD_HIP(hipEventRecord(ev->b, st));
}

}  // namespace fd
