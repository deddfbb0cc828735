// gbdt_row.h — the arithmetic of the histogram gradient-boosting fit (gbdt.hip): the bin of a value, the
// deterministic sigmoid, the fixed-point gradient pair, the counter-based row and feature samples, the gain of a split
// candidate, the order among candidates and the leaf weight. The kernels and the single-threaded host reference
// (fd_gbdt_*_ref_host) compile these same functions, so a tree grown on the device and one grown on the host cannot
// drift apart. Everything here is the engine's own declared rule; it is not XGBoost's arithmetic bit for bit.
//
// No expression here may be contracted into an fma or reassociated (the pragmas below; the library is not built with
// fast-math): one flipped rounding of a gain changes a tree. Only + - * /, comparisons, integer conversions and exact
// power-of-two scalings are used: IEEE fixes their results, which it does not for exp().
#pragma once

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>  // FD_HD's attributes
#endif

#include <cstdint>
#include <cstring>

#include "fdengine.h"
#include "key_hash.h"

namespace fd {

constexpr int kGbdtMissingBin = 255;  // the u8 matrix's reserved bin of a NaN
constexpr int kGbdtMaxCuts = 254;     // bins 0 .. 254 are real: at most 254 cuts per feature
constexpr int kGbdtBins = 256;        // histogram slots per (node, feature)
constexpr int kGbdtScaleBits = 24;    // fixed point of g and h: one quantum is 2^-24
constexpr double kGbdtScale = 16777216.0;
constexpr double kGbdtInvScale = 1.0 / 16777216.0;
constexpr int64_t kGbdtMaxRows = 1ll << 28;  // |sum g| <= 2^28 * 2^24 = 2^52: every sum is exact in f64
constexpr double kGbdtMinGain = 1e-6;        // a node splits iff its best gain exceeds this

// bin(x) = #{cuts <= x}; a NaN takes the missing bin. x < cut_j <=> bin(x) <= j.
FD_HD int gbdt_bin(float x, const float* cuts, int n_cuts) {
  if (!(x == x)) return kGbdtMissingBin;
  int lo = 0, hi = n_cuts;  // first index whose cut is > x
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (cuts[mid] <= x) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// 2^k for -1022 <= k <= 1023, built from its bits
FD_HD double gbdt_pow2(int k) {
  const uint64_t bits = (uint64_t)(k + 1023) << 52;
  double d;
  memcpy(&d, &bits, 8);
  return d;
}

// e^x for |x| <= 64: x = k ln2 + r with |r| <= ln2 / 2 (Cody-Waite, ln2 split so that k * hi is exact), e^r by its
// Taylor polynomial to r^13 / 13! in Horner form (the remainder is below 5e-18 of e^r), times 2^k
FD_HD double gbdt_exp(double x) {
#pragma clang fp contract(off)
  const double kInvLn2 = 1.4426950408889634;
  const double kLn2Hi = 0.693147180369123816490;   // the top 32 bits of ln 2
  const double kLn2Lo = 1.90821492927058770002e-10;
  const double t = x * kInvLn2;
  const int k = (int)(t < 0.0 ? t - 0.5 : t + 0.5);
  const double kd = (double)k;
  const double r = (x - kd * kLn2Hi) - kd * kLn2Lo;
  double p = 1.0 / 6227020800.0;
  p = p * r + 1.0 / 479001600.0;
  p = p * r + 1.0 / 39916800.0;
  p = p * r + 1.0 / 3628800.0;
  p = p * r + 1.0 / 362880.0;
  p = p * r + 1.0 / 40320.0;
  p = p * r + 1.0 / 5040.0;
  p = p * r + 1.0 / 720.0;
  p = p * r + 1.0 / 120.0;
  p = p * r + 1.0 / 24.0;
  p = p * r + 1.0 / 6.0;
  p = p * r + 0.5;
  p = p * r + 1.0;
  p = p * r + 1.0;
  return p * gbdt_pow2(k);
}

// sigma(m) in f64 of an f32 margin: the margin is clamped to [-64, 64] (sigma is 1 - 1.6e-28 there, far below one
// quantum of the fixed point); a NaN margin gives 0.5
FD_HD double gbdt_sigmoid(float margin) {
#pragma clang fp contract(off)
  double x = (double)margin;
  if (!(x == x)) return 0.5;
  if (x > 64.0) x = 64.0;
  if (x < -64.0) x = -64.0;
  if (x >= 0.0) return 1.0 / (1.0 + gbdt_exp(-x));
  const double e = gbdt_exp(x);
  return e / (1.0 + e);
}

// v * 2^24 rounded to the nearest integer, ties to even (|v| <= 64, the class weight's limit): the sum with
// 1.5 * 2^52 rounds at the units place
FD_HD int32_t gbdt_quantise(double v) {
#pragma clang fp contract(off)
  const double kMagic = 6755399441055744.0;
  const double s = v * kGbdtScale + kMagic;
  return (int32_t)(s - kMagic);
}

// g = p - y and h = p (1 - p) in fixed point. A row's h is never below one quantum (2^-24, above the 1e-16 floor
// XGBoost applies): a node with a sampled row has H > 0.
FD_HD void gbdt_grad(float margin, int y, int32_t& g, int32_t& h) {
#pragma clang fp contract(off)
  const double p = gbdt_sigmoid(margin);
  g = gbdt_quantise(p - (double)y);
  const int32_t hq = gbdt_quantise(p * (1.0 - p));
  h = hq < 1 ? 1 : hq;
}

// The same pair under a class weight (scale_pos_weight = w, 0 < w <= 64): a positive row's g = quantise(w (p - 1))
// and h = max(1, quantise(w p (1 - p))), |g| <= 2^30; a negative row keeps gbdt_grad's pair. w == 1 gives gbdt_grad's
// bits (a product with 1.0 is exact).
constexpr double kGbdtMaxPosWeight = 64.0;
FD_HD void gbdt_grad_weighted(float margin, int y, double w, int32_t& g, int32_t& h) {
#pragma clang fp contract(off)
  if (!y) {
    gbdt_grad(margin, y, g, h);
    return;
  }
  const double p = gbdt_sigmoid(margin);
  g = gbdt_quantise(w * (p - 1.0));
  const int32_t hq = gbdt_quantise(w * (p * (1.0 - p)));
  h = hq < 1 ? 1 : hq;
}

// ------------------------------------------------------------------------------------------------ evaluation
// The metrics of a held-out set (fd_gbdt_fit_eval_*, fd_gbdt_metric_*): integer statistics and one division each, so
// their bits depend on neither the launch shape nor the order rows arrive in. Evaluation is never weighted.

// The order key of a margin: a u32 that orders like the float. -0 and +0 share a key (the base margin at base_score
// 0.5 is -0.0f; an empty node's leaf is -0), +-inf are ordinary values, and every NaN takes the one key above +inf's.
FD_HD uint32_t gbdt_order_key(float m) {
  if (!(m == m)) return 0xffffffffu;
  uint32_t u;
  memcpy(&u, &m, 4);
  if ((u & 0x7fffffffu) == 0u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
// What is sorted: (key << 1) | label in 33 bits, so that a tie group's negatives stand before its positives
constexpr int kGbdtSortBits = 33;
FD_HD uint64_t gbdt_sort_word(float m, int y) { return ((uint64_t)gbdt_order_key(m) << 1) | (uint64_t)(y ? 1 : 0); }

// auc = 2U / (2 P N), 2U = sum over the positive rows of #{negatives with a lower key} + #{negatives with a key not
// above}: the Mann-Whitney statistic over midranks, doubled. 2U <= 2 P N <= 2^55 at the row limit: both exact in f64.
FD_HD double gbdt_auc(uint64_t two_u, uint64_t n_pos, uint64_t n_neg) {
#pragma clang fp contract(off)
  return (double)two_u / (double)(2ull * n_pos * n_neg);
}
// error = #{rows with (margin > 0) != y} / n (a NaN margin predicts 0)
FD_HD int gbdt_is_error(float m, int y) { return ((m > 0.0f) ? 1 : 0) != (y ? 1 : 0); }
FD_HD double gbdt_error(uint64_t wrong, uint64_t n) {
#pragma clang fp contract(off)
  return (double)wrong / (double)n;
}

// The stopping rule of XGBoost's EarlyStopping callback, as its documentation states it: round t improves iff its
// metric is strictly better than the best so far (round 0 always improves); after k consecutive rounds without
// improvement the fit stops, so that rounds_run = best_round + k + 1. k == 0: never. One state per fit, updated once
// a round by one thread of the device (gbeval_state_kernel) or by the host reference.
struct GbdtStopState {
  double best;
  int32_t best_round;
  int32_t since;       // rounds since the best
  int32_t stop;        // set: no later round runs
  int32_t rounds_run;
};
FD_HD void gbdt_stop_update(GbdtStopState& s, int round, double metric, bool maximise, int k) {
  s.rounds_run = round + 1;
  const bool improved = round == 0 || (maximise ? metric > s.best : metric < s.best);
  if (improved) {
    s.best = metric;
    s.best_round = round;
    s.since = 0;
    return;
  }
  ++s.since;
  if (k > 0 && s.since >= k) s.stop = 1;
}

// The samples are functions of (seed, round, index): no generator state. mix() keeps rows and features apart.
FD_HD uint64_t gbdt_mix_row(uint32_t round, uint64_t row) { return (((uint64_t)round << 32) | row) << 1; }
FD_HD uint64_t gbdt_mix_feature(uint32_t round, uint32_t f) { return ((((uint64_t)round << 32) | f) << 1) | 1u; }
// row i is in round t's sample iff its hash is below subsample * 2^64 (threshold; all: subsample == 1)
FD_HD bool gbdt_row_sampled(uint64_t seed, uint32_t round, uint64_t row, uint64_t threshold, bool all) {
  return all || fmix64(seed ^ gbdt_mix_row(round, row)) < threshold;
}
FD_HD uint64_t gbdt_feature_hash(uint64_t seed, uint32_t round, uint32_t f) {
  return fmix64(seed ^ gbdt_mix_feature(round, f));
}

// A split candidate's gain from the integer sums of its left side and of the node:
//   gain = GL^2 / (HL + lambda) + GR^2 / (HR + lambda) - G^2 / (H + lambda),
// each sum converted exactly (|sum| < 2^53, the scale a power of two), evaluated in this order. valid: both children
// hold at least min_child_weight.
FD_HD double gbdt_gain(int64_t GL, int64_t HL, int64_t G, int64_t H, double lambda, double min_child_weight,
                       bool& valid) {
#pragma clang fp contract(off)
  const double gl = (double)GL * kGbdtInvScale, hl = (double)HL * kGbdtInvScale;
  const double gr = (double)(G - GL) * kGbdtInvScale, hr = (double)(H - HL) * kGbdtInvScale;
  const double g = (double)G * kGbdtInvScale, h = (double)H * kGbdtInvScale;
  valid = hl >= min_child_weight && hr >= min_child_weight;
  const double a = gl * gl / (hl + lambda);
  const double b = gr * gr / (hr + lambda);
  const double c = g * g / (h + lambda);
  return (a + b) - c;
}

// The best candidate of a node so far. key = cut * 2 + (missing goes left): among equal gains the lower feature wins,
// then the lower cut, then missing-right.
struct GbdtBest {
  double gain;
  int32_t feature;
  int32_t key;
  int64_t GL, HL;  // the left child's sums (the missing bin's included when it goes left)
};
FD_HD GbdtBest gbdt_best_none() { return GbdtBest{-1.0, 0x7fffffff, 0x7fffffff, 0, 0}; }
// does candidate a come before b? (every valid gain is compared; an invalid candidate never enters)
FD_HD bool gbdt_better(const GbdtBest& a, const GbdtBest& b) {
  if (a.gain > b.gain) return true;
  if (a.gain < b.gain) return false;
  if (a.feature != b.feature) return a.feature < b.feature;
  return a.key < b.key;
}

// -G / (H + lambda) * eta in f64: base_weights; the leaf weight is this rounded to f32
FD_HD double gbdt_weight(int64_t G, int64_t H, double lambda, double eta) {
#pragma clang fp contract(off)
  const double g = (double)G * kGbdtInvScale, h = (double)H * kGbdtInvScale;
  return -g / (h + lambda) * eta;
}

// One node of a tree under construction, in full-heap numbering (children of i: 2i + 1, 2i + 2)
struct GbdtNode {
  int64_t G, H;      // the node's sums over its sampled rows
  double gain;       // split nodes: the chosen gain
  double weight;     // gbdt_weight
  float threshold;   // split nodes: the cut's value
  float leaf;        // (float)weight
  int32_t state;     // 0 absent, 1 leaf, 2 split
  int32_t feature;
  int32_t cut;       // split nodes: rows with bin <= cut go left
  int32_t default_left;
};
constexpr int kGbdtAbsent = 0, kGbdtLeaf = 1, kGbdtSplit = 2;

FD_HD void gbdt_make_leaf(GbdtNode& nd, int64_t G, int64_t H, double lambda, double eta) {
  nd.G = G;
  nd.H = H;
  nd.gain = 0.0;
  nd.weight = gbdt_weight(G, H, lambda, eta);
  nd.threshold = 0.0f;
  nd.leaf = (float)nd.weight;
  nd.state = kGbdtLeaf;
  nd.feature = 0;
  nd.cut = 0;
  nd.default_left = 0;
}

// a row's child at a split node, from its bin of the node's feature
FD_HD bool gbdt_goes_left(const GbdtNode& nd, int bin) {
  return bin == kGbdtMissingBin ? nd.default_left != 0 : bin <= nd.cut;
}

}  // namespace fd
