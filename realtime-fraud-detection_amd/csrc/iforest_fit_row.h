// iforest_fit_row.h — the arithmetic of the IsolationForest fit (iforest_fit.hip): the counter-based
// hashes, the keyed permutation a tree's rows come from, the choice among a node's non-constant features, the
// threshold between a feature's min and max, the side a row takes and the running min / max that decide whether a
// feature is constant. The kernels and the single-threaded host reference (fd_iforest_fit_*_ref_host) compile these
// same functions, so a tree grown on the device and one grown on the host cannot drift apart. The rule follows
// scikit-learn's IsolationForest wherever that is deterministic; its random stream is replaced by hashes of
// (seed, tree, node), so the trees are not scikit-learn's bit for bit.
//
// No expression here may be contracted into an fma or reassociated (the pragmas below; the library is not built with
// fast-math). Only + - * /, comparisons, integer operations and conversions are used: no logarithm is taken here (the
// leaf term's table c[0 .. psi] is built once per fit on the host, iforest_fit.hip).
#pragma once

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>  // FD_HD's attributes
#endif

#include <cstdint>

#include "fdengine.h"
#include "key_hash.h"

namespace fd {

constexpr int kIfMaxSamples = 1024;  // psi at most: depth 10, the deepest the heap layout and the fused kernel serve
constexpr int kIfMaxDepth = 10;
constexpr int kIfHeapMax = (1 << (kIfMaxDepth + 1)) - 1;
constexpr int kIfTagFeature = 0, kIfTagThreshold = 1, kIfTagSubset = 2, kIfTagRound = 3;

// D = ceil(log2(max(psi, 2)))
FD_HD int iforest_depth_cap(int psi) {
  int d = 1;
  while ((1 << d) < psi) ++d;
  return d;
}

FD_HD uint64_t iforest_key(uint64_t seed) { return fmix64(seed + 0x9e3779b97f4a7c15ULL); }
// every draw is a function of (seed, tree, a, tag): no generator state. a < 2^30.
FD_HD uint64_t iforest_hash(uint64_t key, uint32_t tree, uint32_t a, uint32_t tag) {
  return fmix64(key ^ (((uint64_t)tree << 32) | ((uint64_t)a << 2) | (uint64_t)tag));
}

// half the width of the permutation's domain: the smallest b >= 1 with 2^(2 b) >= n
FD_HD int iforest_half_bits(int64_t n) {
  int b = 1;
  while (((int64_t)1 << (2 * b)) < n) ++b;
  return b;
}

// perm_t(j): a 4-round Feistel network on 2 b bits, walked until it lands in [0, n) (j < n). A bijection of [0, n),
// so distinct j give distinct rows; at most 4 n points lie outside, a handful of steps on average.
FD_HD int64_t iforest_perm(uint64_t key, uint32_t tree, int64_t n, int b, int64_t j) {
  const uint64_t mask = ((uint64_t)1 << b) - 1;
  uint64_t k[4];
  for (int r = 0; r < 4; ++r) k[r] = iforest_hash(key, tree, (uint32_t)r, kIfTagRound);
  uint64_t x = (uint64_t)j;
  do {
    uint64_t L = x >> b, R = x & mask;
    for (int r = 0; r < 4; ++r) {
      const uint64_t nr = L ^ (fmix64(k[r] ^ R) & mask);
      L = R;
      R = nr;
    }
    x = (L << b) | R;
  } while (x >= (uint64_t)n);
  return (int64_t)x;
}

// (h * c) >> 64 for c < 2^32, in 64-bit arithmetic: uniform over [0, c)
FD_HD uint32_t iforest_pick(uint64_t h, uint32_t c) {
  const uint64_t lo = (h & 0xffffffffULL) * c, hi = (h >> 32) * c;
  return (uint32_t)((hi + (lo >> 32)) >> 32);
}

// the index of the r-th set bit of mask (r < popcount)
FD_HD int iforest_nth_bit(uint64_t mask, uint32_t r) {
  for (uint32_t k = 0; k < r; ++k) mask &= mask - 1;
  int f = 0;
  while (!((mask >> f) & 1ull)) ++f;
  return f;
}

// a feature's running min and max over a node's samples: a NaN enters neither; -0 and +0 compare equal, so a column
// of only those has max > min false and counts as constant
FD_HD void iforest_minmax(float x, float& mn, float& mx) {
  if (x < mn) mn = x;
  if (x > mx) mx = x;
}

// the threshold of a split between the chosen feature's min and max: uniform in [mn, mx) from the node's second hash
FD_HD double iforest_threshold(float mn, float mx, uint64_t h2) {
#pragma clang fp contract(off)
  const double a = (double)mn, b = (double)mx;
  const double u = (double)(h2 >> 11) * 1.1102230246251565e-16;  // 2^-53
  const double w = u * (b - a);
  double thr = a + w;
  if (!(thr < b)) thr = a;  // the sum rounded up to the max (scikit-learn: if threshold == max: threshold = min)
  return thr;
}

// scikit-learn's comparison; a NaN goes right
FD_HD bool iforest_goes_left(float x, double thr) { return (double)x <= thr; }

// One node of a tree under construction, in full-heap numbering (children of i: 2 i + 1, 2 i + 2). count == 0: absent.
struct IfNode {
  double threshold;
  int32_t feature;  // -1 at a leaf
  int32_t count;    // the node's samples
};

}  // namespace fd
