// gbdt.hip — the histogram gradient-boosting fit (ModelTrainer.train_xgboost_model's fit, ml/training/
// model_trainer.py:83-96): kernels, launch loop and the single-threaded host reference. The arithmetic is gbdt_row.h,
// compiled by both; the semantics are declared in include/fdengine.h ("training") and DESIGN §4.14.
//
// Device state of a fit: the u8 bin matrix (n x F, row-major), int32 g and h, the round's u8 row mask, an int32 heap
// index per row (the node the row is in; rows of a finished leaf stay there) and the f32 margins. A tree is built in
// full-heap numbering (children of i: 2i + 1, 2i + 2), level by level, four launches a level:
//   memset               the level's histograms: [node of the level][feature][256 bins] of int64 (sum g, sum h)
//   gbdt_hist_kernel     every sampled row of a node of the level adds its (g, h) to the bins of the kept features.
//                        Levels of up to 16 nodes: a workgroup takes gbdt_hist_rows consecutive rows and a tile of
//                        16 / nodes features, accumulates in 64 KiB of LDS with 64-bit integer adds and flushes the
//                        non-zero slots with global 64-bit integer atomics (the root level would otherwise put every
//                        row of the matrix on F * 256 addresses). Deeper levels spread over >= 32 * F * 256 slots and
//                        add to global memory directly. Integer addition commutes: the histogram is the same bits for
//                        any grid, any rows per workgroup and any arrival order. No float is ever added atomically.
//   gbdt_split_kernel    a workgroup per node, a wave per feature (features strided over the four waves): 4 bins per
//                        lane, an int64 wave prefix scan, both missing directions, the gains of gbdt_row.h, a wave
//                        argmax under the declared total order, then the four waves' bests through LDS; thread 0
//                        writes the node's split and creates its two children as leaves with their sums and weights.
//   gbdt_route_kernel    every row (sampled or not) of a node that split moves to its child.
// Between trees gbdt_round_kernel adds the finished tree's leaf to every row's margin, puts the row back at the root,
// and computes the next round's gradients and sample. The loop issues launches only; the node heaps of all trees come
// back in one copy at the end and are renumbered breadth-first (XGBoost's depth-wise numbering) on the host.
// Histograms of both children are built (the sibling subtraction the integer sums would allow is left out).
//
// A watched fit (fd_gbdt_fit_eval_*: an eval set's metric per round, early stopping, a class weight) adds per round,
// after the tree's launches, gbeval_walk_kernel (the eval rows take the new tree's leaf; their sort words or the wrong
// rows' count), for AUC rocPRIM's radix sort and integer scan and gbeval_count_kernel, and the one-thread
// gbeval_state_kernel, which writes the round's metric and applies the stopping rule to a state on the device. The
// loop still only launches: with early stopping the tree's kernels are their gbeval_ twins, which return at the stop
// flag. A fit without those arguments issues none of this.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <exception>
#include <numeric>
#include <vector>

#include <rocprim/rocprim.hpp>

#include "fd_internal.h"
#include "gbdt_row.h"

namespace fd {
namespace {

constexpr int kGbdtThreads = 256;
constexpr int kGbdtWaves = kGbdtThreads / 64;
constexpr int kHistPairs = 16;  // (node, feature) histograms in a workgroup's LDS: 16 * 256 bins * 16 B = 64 KiB
constexpr int kNoFeature = 0x7fffffff;
constexpr int kCutThreads = 16;  // host threads of the device path's cut computation (the reference uses one)

inline int heap_nodes(int max_depth) { return (1 << (max_depth + 1)) - 1; }

// the slot of (node of the level, feature, bin) in a level's histogram, in 8-byte words (g, then h)
FD_HD size_t hist_slot(int node_local, int F, int f, int bin) {
  return ((((size_t)node_local * F + f) * kGbdtBins) + bin) * 2;
}

// What thread 0 of the split kernel and the host reference do with a node's sums and best candidate
FD_HD void finish_node(GbdtNode* heap, int idx, int level, int64_t G, int64_t H, const GbdtBest& best,
                       const float* cuts, const int32_t* offsets, double lambda, double eta) {
  GbdtNode& nd = heap[idx];
  if (level == 0) gbdt_make_leaf(nd, G, H, lambda, eta);  // the root comes to exist (a child was made by its parent)
  if (best.feature == kNoFeature || !(best.gain > kGbdtMinGain)) return;
  nd.state = kGbdtSplit;
  nd.feature = best.feature;
  nd.cut = best.key >> 1;
  nd.default_left = best.key & 1;
  nd.gain = best.gain;
  nd.threshold = cuts[offsets[best.feature] + nd.cut];
  gbdt_make_leaf(heap[2 * idx + 1], best.GL, best.HL, lambda, eta);
  gbdt_make_leaf(heap[2 * idx + 2], G - best.GL, H - best.HL, lambda, eta);
}

// ------------------------------------------------------------------------------------------------ kernels

// grid: (row blocks, F); a workgroup holds its feature's cuts (at most 254) in LDS
__global__ void __launch_bounds__(kGbdtThreads) gbdt_bin_kernel(const float* __restrict__ X, int64_t n, int32_t ld,
                                                                int32_t F, const float* __restrict__ cuts,
                                                                const int32_t* __restrict__ offsets,
                                                                uint8_t* __restrict__ bins) {
  __shared__ float s_cuts[kGbdtBins];
  const int f = blockIdx.y;
  const int o = offsets[f];
  const int nc = min(offsets[f + 1] - o, kGbdtMaxCuts);
  for (int k = threadIdx.x; k < nc; k += kGbdtThreads) s_cuts[k] = cuts[o + k];
  __syncthreads();
  for (int64_t r = (int64_t)blockIdx.x * kGbdtThreads + threadIdx.x; r < n; r += (int64_t)gridDim.x * kGbdtThreads)
    bins[r * F + f] = (uint8_t)gbdt_bin(X[r * ld + f], s_cuts, nc);
}

__global__ void __launch_bounds__(kGbdtThreads) gbdt_grad_kernel(const float* __restrict__ margin,
                                                                 const uint8_t* __restrict__ y, int64_t n,
                                                                 int32_t* __restrict__ g, int32_t* __restrict__ h) {
  const int64_t i = (int64_t)blockIdx.x * kGbdtThreads + threadIdx.x;
  if (i >= n) return;
  int32_t gi, hi;
  gbdt_grad(margin[i], y[i], gi, hi);
  g[i] = gi;
  h[i] = hi;
}

// Between trees: the margin takes the finished tree's leaf (prev: that tree's heap; null before the first tree, when
// the margin starts at `base`), the row returns to the root, and with compute != 0 the round's gradients and sample
// are written.
__global__ void __launch_bounds__(kGbdtThreads) gbdt_round_kernel(float* __restrict__ margin,
                                                                  const uint8_t* __restrict__ y, int64_t n,
                                                                  const GbdtNode* __restrict__ prev, float base,
                                                                  int32_t* __restrict__ pos, int32_t* __restrict__ g,
                                                                  int32_t* __restrict__ h, uint8_t* __restrict__ mask,
                                                                  uint64_t seed, uint32_t round, uint64_t threshold,
                                                                  int all, int compute) {
  const int64_t i = (int64_t)blockIdx.x * kGbdtThreads + threadIdx.x;
  if (i >= n) return;
  const float m = prev ? margin[i] + prev[pos[i]].leaf : base;
  margin[i] = m;
  pos[i] = 0;
  if (!compute) return;
  int32_t gi, hi;
  gbdt_grad(m, y[i], gi, hi);
  g[i] = gi;
  h[i] = hi;
  mask[i] = gbdt_row_sampled(seed, round, (uint64_t)i, threshold, all != 0) ? 1 : 0;
}

// The three per-level kernels exist twice: gbdt_* as they always were, and gbeval_* (further down), which take the
// stop state of a fit with early stopping and return at once when it is set. Both wrap the bodies below.
// kLds: grid (row blocks, feature tiles of ft features), nodes * ft <= kHistPairs; else grid (row blocks, 1)
template <bool kLds>
__device__ __forceinline__ void hist_body(const uint8_t* __restrict__ bins, const int32_t* __restrict__ g,
                                          const int32_t* __restrict__ h, const uint8_t* __restrict__ mask,
                                          const int32_t* __restrict__ pos, int64_t n, int F, int level,
                                          uint64_t feat_mask, int rows_per_wg, int ft,
                                          unsigned long long* __restrict__ hist) {
  __shared__ unsigned long long s_hist[kLds ? kHistPairs * kGbdtBins * 2 : 2];
  const int nn = 1 << level, first = nn - 1;
  const int f0 = kLds ? (int)blockIdx.y * ft : 0;
  const int f1 = kLds ? min(F, f0 + ft) : F;
  const int words = nn * ft * kGbdtBins * 2;  // (kLds) <= kHistPairs * 512
  if (kLds) {
    for (int k = threadIdx.x; k < words; k += kGbdtThreads) s_hist[k] = 0ull;
    __syncthreads();
  }
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_wg;
  const int64_t r1 = min(n, r0 + (int64_t)rows_per_wg);
  for (int64_t r = r0 + threadIdx.x; r < r1; r += kGbdtThreads) {
    if (mask && !mask[r]) continue;
    const int p = pos[r] - first;
    if ((unsigned)p >= (unsigned)nn) continue;  // the row rests in a leaf above this level
    const unsigned long long gv = (unsigned long long)(long long)g[r];
    const unsigned long long hv = (unsigned long long)(long long)h[r];
    const uint8_t* b = bins + r * F;
    for (int f = f0; f < f1; ++f) {
      if (!((feat_mask >> f) & 1ull)) continue;
      const int bin = b[f];
      if (kLds) {
        const size_t k = hist_slot(p, ft, f - f0, bin);
        atomicAdd(&s_hist[k], gv);
        atomicAdd(&s_hist[k + 1], hv);
      } else {
        const size_t k = hist_slot(p, F, f, bin);
        atomicAdd(&hist[k], gv);
        atomicAdd(&hist[k + 1], hv);
      }
    }
  }
  if (kLds) {
    __syncthreads();
    for (int k = threadIdx.x; k < words; k += kGbdtThreads) {
      const unsigned long long v = s_hist[k];
      if (v == 0ull) continue;
      const int pair = k >> 9, f = f0 + pair % ft, p = pair / ft;
      if (f < f1) atomicAdd(&hist[hist_slot(p, F, f, (k >> 1) & 255) + (k & 1)], v);
    }
  }
}

__device__ __forceinline__ GbdtBest shfl_xor_best(const GbdtBest& b, int d) {
  GbdtBest o;
  o.gain = __shfl_xor(b.gain, d);
  o.feature = __shfl_xor(b.feature, d);
  o.key = __shfl_xor(b.key, d);
  o.GL = __shfl_xor((long long)b.GL, d);
  o.HL = __shfl_xor((long long)b.HL, d);
  return o;
}

template <bool kLds>
__global__ void __launch_bounds__(kGbdtThreads) gbdt_hist_kernel(const uint8_t* __restrict__ bins,
                                                                 const int32_t* __restrict__ g,
                                                                 const int32_t* __restrict__ h,
                                                                 const uint8_t* __restrict__ mask,
                                                                 const int32_t* __restrict__ pos, int64_t n, int F,
                                                                 int level, uint64_t feat_mask, int rows_per_wg,
                                                                 int ft, unsigned long long* __restrict__ hist) {
  hist_body<kLds>(bins, g, h, mask, pos, n, F, level, feat_mask, rows_per_wg, ft, hist);
}

// grid: the level's nodes. hist: the level's histograms; heap: the tree's nodes
__device__ __forceinline__ void split_body(const unsigned long long* __restrict__ hist, GbdtNode* __restrict__ heap,
                                           int level, int F, uint64_t feat_mask, const float* __restrict__ cuts,
                                           const int32_t* __restrict__ offsets, double lambda,
                                           double min_child_weight, double eta) {
  __shared__ GbdtBest s_best[kGbdtWaves];
  __shared__ long long s_tot[kGbdtWaves][2];
  __shared__ int s_has[kGbdtWaves];
  const int node_local = blockIdx.x, idx = (1 << level) - 1 + node_local;
  if (level > 0 && heap[idx].state != kGbdtLeaf) return;  // (the whole workgroup: no barrier is skipped by a part)
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  GbdtBest best = gbdt_best_none();
  long long G = 0, H = 0;
  int has = 0;
  for (int f = wave; f < F; f += kGbdtWaves) {
    if (!((feat_mask >> f) & 1ull)) continue;
    const long long* hp = reinterpret_cast<const long long*>(hist) + hist_slot(node_local, F, f, lane * 4);
    long long bg[4], bh[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      bg[k] = hp[2 * k];
      bh[k] = hp[2 * k + 1];
    }
    const long long sg = bg[0] + bg[1] + bg[2] + bg[3], sh = bh[0] + bh[1] + bh[2] + bh[3];
    long long ig = sg, ih = sh;  // inclusive scan over the lanes
    for (int d = 1; d < 64; d <<= 1) {
      const long long ug = __shfl_up(ig, d), uh = __shfl_up(ih, d);
      if (lane >= d) {
        ig += ug;
        ih += uh;
      }
    }
    G = __shfl(ig, 63);  // every kept feature's bins sum to the node's sums
    H = __shfl(ih, 63);
    has = 1;
    const long long Gm = __shfl(bg[3], 63), Hm = __shfl(bh[3], 63);  // bin 255: the missing rows
    const int nc = min(offsets[f + 1] - offsets[f], kGbdtMaxCuts);
    long long cg = ig - sg, ch = ih - sh;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      cg += bg[k];
      ch += bh[k];
      const int j = lane * 4 + k;
      if (j >= nc) continue;
      for (int dir = 0; dir < 2; ++dir) {
        GbdtBest c;
        c.GL = cg + (dir ? Gm : 0);
        c.HL = ch + (dir ? Hm : 0);
        bool valid;
        c.gain = gbdt_gain(c.GL, c.HL, G, H, lambda, min_child_weight, valid);
        c.feature = f;
        c.key = j * 2 + dir;
        if (valid && gbdt_better(c, best)) best = c;
      }
    }
  }
  for (int d = 32; d >= 1; d >>= 1) {
    const GbdtBest o = shfl_xor_best(best, d);
    if (gbdt_better(o, best)) best = o;
  }
  if (lane == 0) {
    s_best[wave] = best;
    s_tot[wave][0] = G;
    s_tot[wave][1] = H;
    s_has[wave] = has;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  bool got = false;
  for (int w = 0; w < kGbdtWaves; ++w) {
    if (s_has[w] && !got) {
      G = s_tot[w][0];
      H = s_tot[w][1];
      got = true;
    }
    if (w > 0 && gbdt_better(s_best[w], best)) best = s_best[w];
  }
  finish_node(heap, idx, level, G, H, best, cuts, offsets, lambda, eta);
}

__global__ void __launch_bounds__(kGbdtThreads) gbdt_split_kernel(const unsigned long long* __restrict__ hist,
                                                                  GbdtNode* __restrict__ heap, int level, int F,
                                                                  uint64_t feat_mask, const float* __restrict__ cuts,
                                                                  const int32_t* __restrict__ offsets, double lambda,
                                                                  double min_child_weight, double eta) {
  split_body(hist, heap, level, F, feat_mask, cuts, offsets, lambda, min_child_weight, eta);
}

__device__ __forceinline__ void route_body(const uint8_t* __restrict__ bins, int32_t* __restrict__ pos, int64_t n,
                                           int F, const GbdtNode* __restrict__ heap, int level) {
  const int64_t i = (int64_t)blockIdx.x * kGbdtThreads + threadIdx.x;
  if (i >= n) return;
  const int p = pos[i];
  if (p < (1 << level) - 1) return;
  const GbdtNode nd = heap[p];
  if (nd.state != kGbdtSplit) return;
  pos[i] = 2 * p + (gbdt_goes_left(nd, bins[i * F + nd.feature]) ? 1 : 2);
}

__global__ void __launch_bounds__(kGbdtThreads) gbdt_route_kernel(const uint8_t* __restrict__ bins,
                                                                  int32_t* __restrict__ pos, int64_t n, int F,
                                                                  const GbdtNode* __restrict__ heap, int level) {
  route_body(bins, pos, n, F, heap, level);
}

// ------------------------------------------------------------------------------------------------ the watched fit
// Kernels of fd_gbdt_fit_eval_* (DESIGN §4.14 "Evaluation"); their names start gbeval_. st: the fit's stop state on
// the device (null: the fit has no eval set). A kernel that finds st->stop set returns at once.

template <bool kLds>
__global__ void __launch_bounds__(kGbdtThreads) gbeval_hist_kernel(const uint8_t* __restrict__ bins,
                                                                   const int32_t* __restrict__ g,
                                                                   const int32_t* __restrict__ h,
                                                                   const uint8_t* __restrict__ mask,
                                                                   const int32_t* __restrict__ pos, int64_t n, int F,
                                                                   int level, uint64_t feat_mask, int rows_per_wg,
                                                                   int ft, unsigned long long* __restrict__ hist,
                                                                   const GbdtStopState* __restrict__ st) {
  if (st->stop) return;  // (uniform: the whole grid)
  hist_body<kLds>(bins, g, h, mask, pos, n, F, level, feat_mask, rows_per_wg, ft, hist);
}

__global__ void __launch_bounds__(kGbdtThreads) gbeval_split_kernel(const unsigned long long* __restrict__ hist,
                                                                    GbdtNode* __restrict__ heap, int level, int F,
                                                                    uint64_t feat_mask, const float* __restrict__ cuts,
                                                                    const int32_t* __restrict__ offsets, double lambda,
                                                                    double min_child_weight, double eta,
                                                                    const GbdtStopState* __restrict__ st) {
  if (st->stop) return;
  split_body(hist, heap, level, F, feat_mask, cuts, offsets, lambda, min_child_weight, eta);
}

__global__ void __launch_bounds__(kGbdtThreads) gbeval_route_kernel(const uint8_t* __restrict__ bins,
                                                                    int32_t* __restrict__ pos, int64_t n, int F,
                                                                    const GbdtNode* __restrict__ heap, int level,
                                                                    const GbdtStopState* __restrict__ st) {
  if (st->stop) return;
  route_body(bins, pos, n, F, heap, level);
}

// gbdt_round_kernel with the class weight w. With an eval set: the first launch after the stop still gives the rows
// the last grown tree's leaf and does nothing else (later ones nothing at all), and best_margin keeps the margins as
// they stood after the best round's tree (the state kernel of round t - 1 ran before this launch of round t).
__global__ void __launch_bounds__(kGbdtThreads) gbeval_round_kernel(float* __restrict__ margin,
                                                                    const uint8_t* __restrict__ y, int64_t n,
                                                                    const GbdtNode* __restrict__ prev, float base,
                                                                    int32_t* __restrict__ pos, int32_t* __restrict__ g,
                                                                    int32_t* __restrict__ h, uint8_t* __restrict__ mask,
                                                                    uint64_t seed, uint32_t round, uint64_t threshold,
                                                                    int all, int compute, double w,
                                                                    const GbdtStopState* __restrict__ st,
                                                                    float* __restrict__ best_margin) {
  const int64_t i = (int64_t)blockIdx.x * kGbdtThreads + threadIdx.x;
  if (i >= n) return;
  if (st && st->stop) {
    if (prev && st->rounds_run == (int32_t)round) margin[i] = margin[i] + prev[pos[i]].leaf;
    return;
  }
  const float m = prev ? margin[i] + prev[pos[i]].leaf : base;
  margin[i] = m;
  if (st && prev && st->best_round == (int32_t)round - 1) best_margin[i] = m;
  pos[i] = 0;
  if (!compute) return;
  int32_t gi, hi;
  gbdt_grad_weighted(m, y[i], w, gi, hi);
  g[i] = gi;
  h[i] = hi;
  mask[i] = gbdt_row_sampled(seed, round, (uint64_t)i, threshold, all != 0) ? 1 : 0;
}

// One lane per eval row: with heap, the row walks the round's tree by its bins and its f32 margin takes the leaf (the
// same add in tree order that serving does; first: the margin starts at base); without, the margins are the caller's
// (fd_gbdt_metric_host). kAuc: the row's sort word is written; else the wave's wrong rows are counted (an integer
// atomic).
template <bool kAuc>
__global__ void __launch_bounds__(kGbdtThreads) gbeval_walk_kernel(const uint8_t* __restrict__ bins,
                                                                   const uint8_t* __restrict__ y, int64_t n, int F,
                                                                   const GbdtNode* __restrict__ heap, int max_depth,
                                                                   int first, float base, float* __restrict__ margin,
                                                                   uint64_t* __restrict__ words,
                                                                   unsigned long long* __restrict__ acc,
                                                                   const GbdtStopState* __restrict__ st) {
  if (st->stop) return;
  const int64_t i = (int64_t)blockIdx.x * kGbdtThreads + threadIdx.x;
  const bool in = i < n;
  float m = 0.0f;
  int label = 0;
  if (in) {
    m = first ? base : margin[i];
    label = y[i];
    if (heap) {
      const uint8_t* b = bins + i * F;
      int p = 0;
      for (int d = 0; d < max_depth && heap[p].state == kGbdtSplit; ++d) {
        const GbdtNode nd = heap[p];
        p = 2 * p + (gbdt_goes_left(nd, b[nd.feature]) ? 1 : 2);
      }
      m = m + heap[p].leaf;
      margin[i] = m;
    }
  }
  if (kAuc) {
    if (in) words[i] = gbdt_sort_word(m, label);
  } else {
    const unsigned long long wrong = __ballot(in && gbdt_is_error(m, label));
    if ((threadIdx.x & 63) == 0 && wrong) atomicAdd(acc, (unsigned long long)__popcll(wrong));
  }
}

// sorted: the eval rows' words in ascending order, so a tie group's negatives stand before its positives; neg_before[j]:
// the negatives at places < j (an exclusive integer scan). A positive at place j counts neg_before[j] (the negatives
// with a key not above its own) and neg_before[head], head the first place of its key, found by bisection (the
// negatives below). Integer sums, one integer atomic per wave: 2U is the same for any grid.
__global__ void __launch_bounds__(kGbdtThreads) gbeval_count_kernel(const uint64_t* __restrict__ sorted,
                                                                    const uint32_t* __restrict__ neg_before, int64_t n,
                                                                    unsigned long long* __restrict__ acc,
                                                                    const GbdtStopState* __restrict__ st) {
  if (st->stop) return;
  unsigned long long sum = 0;
  for (int64_t j = (int64_t)blockIdx.x * kGbdtThreads + threadIdx.x; j < n; j += (int64_t)gridDim.x * kGbdtThreads) {
    const uint64_t w = sorted[j];
    if (!(w & 1ull)) continue;
    const uint64_t head_word = w & ~1ull;
    int64_t lo = 0, hi = j;  // the first place whose word is >= head_word (place j's is)
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (sorted[mid] < head_word) lo = mid + 1;
      else hi = mid;
    }
    sum += (unsigned long long)neg_before[lo] + (unsigned long long)neg_before[j];
  }
  for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d);
  if ((threadIdx.x & 63) == 0 && sum) atomicAdd(acc, sum);
}

// One thread: the round's metric from the integer count, into curve[round]; the count returns to 0; the stopping rule
struct GbdtEvalState {
  GbdtStopState stop;
  unsigned long long acc;  // 2U, or the wrong rows, of the round under way
};
__global__ void gbeval_state_kernel(GbdtEvalState* __restrict__ es, const uint64_t* __restrict__ sorted,
                                    const uint32_t* __restrict__ neg_before, int64_t n, int metric, int round, int k,
                                    double* __restrict__ curve) {
  if (threadIdx.x != 0 || blockIdx.x != 0 || es->stop.stop) return;
  double v;
  if (metric == FD_GBDT_METRIC_AUC) {
    const uint64_t n_neg = (uint64_t)neg_before[n - 1] + ((sorted[n - 1] & 1ull) ? 0ull : 1ull);
    v = gbdt_auc(es->acc, (uint64_t)n - n_neg, n_neg);
  } else {
    v = gbdt_error(es->acc, (uint64_t)n);
  }
  es->acc = 0ull;
  curve[round] = v;
  gbdt_stop_update(es->stop, round, v, metric == FD_GBDT_METRIC_AUC, k);
}

struct EvalNegFlag {  // a sort word -> 1 for a negative row
  __host__ __device__ uint32_t operator()(uint64_t w) const { return (uint32_t)(~w & 1ull); }
};

// ------------------------------------------------------------------------------------------------ host pieces

unsigned row_blocks(int64_t n) { return (unsigned)((n + kGbdtThreads - 1) / kGbdtThreads); }

uint64_t all_features(int F) { return F >= 64 ? ~0ull : (1ull << F) - 1ull; }

// colsample_bytree: the max(1, floor(c F)) features with the smallest hash, ties to the lower index
uint64_t round_feature_mask(uint64_t seed, uint32_t round, int F, double colsample) {
  const int keep = std::max(1, (int)std::floor(colsample * (double)F));
  if (keep >= F) return all_features(F);
  std::vector<int> order(F);
  std::iota(order.begin(), order.end(), 0);
  std::vector<uint64_t> hash(F);
  for (int f = 0; f < F; ++f) hash[f] = gbdt_feature_hash(seed, round, (uint32_t)f);
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return hash[a] < hash[b]; });
  uint64_t m = 0;
  for (int k = 0; k < keep; ++k) m |= 1ull << order[k];
  return m;
}

struct RowSample {
  uint64_t threshold;
  bool all;
};
RowSample row_sample(double subsample) {
  if (subsample >= 1.0) return {~0ull, true};
  return {(uint64_t)(subsample * 18446744073709551616.0), false};
}

// a tree's heap appended to the caller's arrays in breadth-first numbering -> its node count
int64_t emit_tree(const GbdtNode* heap, const fd_gbdt_model& out, int64_t base, int tree, int64_t* n_split) {
  fd_tree_arrays& t = *out.trees;
  auto* left = const_cast<int32_t*>(t.left) + base;
  auto* right = const_cast<int32_t*>(t.right) + base;
  auto* feature = const_cast<int32_t*>(t.feature) + base;
  auto* threshold = const_cast<double*>(t.threshold) + base;
  auto* dleft = t.default_left ? const_cast<uint8_t*>(t.default_left) + base : nullptr;
  auto* leaf = const_cast<double*>(t.leaf_value) + base;
  std::vector<int> queue{0};
  for (size_t q = 0; q < queue.size(); ++q) {  // a split node's children take the next two numbers
    const GbdtNode& nd = heap[queue[q]];
    const bool split = nd.state == kGbdtSplit;
    if (split) {
      left[q] = (int32_t)queue.size();
      right[q] = (int32_t)queue.size() + 1;
      queue.push_back(2 * queue[q] + 1);
      queue.push_back(2 * queue[q] + 2);
      if (n_split) ++*n_split;
    } else {
      left[q] = right[q] = -1;
    }
    feature[q] = split ? nd.feature : 0;
    threshold[q] = split ? (double)nd.threshold : 0.0;
    if (dleft) dleft[q] = split ? (uint8_t)nd.default_left : 0;
    leaf[q] = split ? 0.0 : (double)nd.leaf;
    if (out.sum_hessian) out.sum_hessian[base + q] = (double)nd.H * kGbdtInvScale;
    if (out.loss_changes) out.loss_changes[base + q] = split ? nd.gain : 0.0;
    if (out.base_weights) out.base_weights[base + q] = nd.weight;
  }
  const_cast<int64_t*>(t.tree_offsets)[tree + 1] = base + (int64_t)queue.size();
  return (int64_t)queue.size();
}

void check_model(const fd_gbdt_model& out) {
  FD_REQUIRE(out.trees && out.trees->tree_offsets && out.trees->left && out.trees->right && out.trees->feature &&
                 out.trees->threshold && out.trees->leaf_value,
             FD_ERR_INVALID_ARG, "gbdt: null output arrays");
}

// one tree on the host: heap (heap_nodes entries) and pos (n) are written
void grow_heap_ref(const uint8_t* bins, int64_t n, int F, const float* cuts, const int32_t* offsets, const int32_t* g,
                   const int32_t* h, const uint8_t* mask, uint64_t feat_mask, const fd_gbdt_params& p,
                   std::vector<int32_t>& pos, std::vector<GbdtNode>& heap) {
  heap.assign((size_t)heap_nodes(p.max_depth), GbdtNode{});
  pos.assign((size_t)n, 0);
  std::vector<int64_t> hist;
  for (int level = 0; level < p.max_depth; ++level) {
    const int nn = 1 << level, first = nn - 1;
    hist.assign((size_t)nn * F * kGbdtBins * 2, 0);
    for (int64_t r = 0; r < n; ++r) {
      if (mask && !mask[r]) continue;
      const int pl = pos[r] - first;
      if (pl < 0) continue;
      for (int f = 0; f < F; ++f) {
        if (!((feat_mask >> f) & 1ull)) continue;
        const size_t k = hist_slot(pl, F, f, bins[r * F + f]);
        hist[k] += g[r];
        hist[k + 1] += h[r];
      }
    }
    for (int nl = 0; nl < nn; ++nl) {
      const int idx = first + nl;
      if (level > 0 && heap[idx].state != kGbdtLeaf) continue;
      GbdtBest best = gbdt_best_none();
      int64_t G = 0, H = 0;
      bool got = false;
      for (int f = 0; f < F; ++f) {
        if (!((feat_mask >> f) & 1ull)) continue;
        const int64_t* hp = hist.data() + hist_slot(nl, F, f, 0);
        if (!got) {
          for (int b = 0; b < kGbdtBins; ++b) {
            G += hp[2 * b];
            H += hp[2 * b + 1];
          }
          got = true;
        }
        const int64_t Gm = hp[2 * kGbdtMissingBin], Hm = hp[2 * kGbdtMissingBin + 1];
        const int nc = std::min(offsets[f + 1] - offsets[f], kGbdtMaxCuts);
        int64_t cg = 0, ch = 0;
        for (int j = 0; j < nc; ++j) {
          cg += hp[2 * j];
          ch += hp[2 * j + 1];
          for (int dir = 0; dir < 2; ++dir) {
            GbdtBest c;
            c.GL = cg + (dir ? Gm : 0);
            c.HL = ch + (dir ? Hm : 0);
            bool valid;
            c.gain = gbdt_gain(c.GL, c.HL, G, H, p.lambda, p.min_child_weight, valid);
            c.feature = f;
            c.key = j * 2 + dir;
            if (valid && gbdt_better(c, best)) best = c;
          }
        }
      }
      finish_node(heap.data(), idx, level, G, H, best, cuts, offsets, p.lambda, p.eta);
    }
    for (int64_t r = 0; r < n; ++r) {
      const int q = pos[r];
      if (q < first || heap[q].state != kGbdtSplit) continue;
      pos[r] = 2 * q + (gbdt_goes_left(heap[q], bins[r * F + heap[q].feature]) ? 1 : 2);
    }
  }
}

}  // namespace

// ------------------------------------------------------------------------------------------------ host API

void gbdt_check_params(const fd_gbdt_params& p, int64_t n, int32_t F, bool fit) {
  FD_REQUIRE(n >= 0, FD_ERR_INVALID_ARG, "gbdt: negative n");
  FD_REQUIRE(n <= kGbdtMaxRows, FD_ERR_UNSUPPORTED,
             "gbdt: more than 2^28 rows (a fixed-point sum could leave the range f64 holds exactly)");
  FD_REQUIRE(F >= 1 && F <= 64, FD_ERR_INVALID_ARG, "gbdt: F must be in 1..64");
  FD_REQUIRE(p.max_depth >= 1 && p.max_depth <= kMaxDepth, FD_ERR_INVALID_ARG, "gbdt: max_depth must be in 1..10");
  FD_REQUIRE(p.lambda >= 0.0 && p.min_child_weight >= 0.0 && p.lambda + p.min_child_weight > 0.0 &&
                 std::isfinite(p.lambda) && std::isfinite(p.min_child_weight),
             FD_ERR_INVALID_ARG, "gbdt: lambda and min_child_weight must be >= 0 and not both 0");
  FD_REQUIRE(std::isfinite(p.eta), FD_ERR_INVALID_ARG, "gbdt: eta must be finite");
  if (!fit) return;
  FD_REQUIRE(p.n_rounds >= 1 && p.n_rounds <= 65536, FD_ERR_INVALID_ARG, "gbdt: n_rounds must be in 1..65536");
  FD_REQUIRE(p.max_bin >= 2 && p.max_bin <= 256, FD_ERR_INVALID_ARG, "gbdt: max_bin must be in 2..256");
  FD_REQUIRE(p.subsample > 0.0 && p.subsample <= 1.0, FD_ERR_INVALID_ARG, "gbdt: subsample must be in (0, 1]");
  FD_REQUIRE(p.colsample_bytree > 0.0 && p.colsample_bytree <= 1.0, FD_ERR_INVALID_ARG,
             "gbdt: colsample_bytree must be in (0, 1]");
  FD_REQUIRE(p.base_score > 0.0 && p.base_score < 1.0, FD_ERR_INVALID_ARG, "gbdt: base_score must be in (0, 1)");
}

int64_t gbdt_cuts_host(const float* X, int64_t n, int32_t ld, int32_t F, int32_t max_bin, std::vector<float>& cuts,
                       std::vector<int32_t>& offsets, int threads) {
  FD_REQUIRE(F >= 1 && F <= 64 && ld >= F, FD_ERR_INVALID_ARG, "gbdt: F must be in 1..64 and ld >= F");
  FD_REQUIRE(max_bin >= 2 && max_bin <= 256, FD_ERR_INVALID_ARG, "gbdt: max_bin must be in 2..256");
  FD_REQUIRE(n >= 0 && (n == 0 || X), FD_ERR_INVALID_ARG, "gbdt: null X");
  // features [f0, f1): one pass over the rows gathers their non-NaN columns, then a sort and the candidates of each.
  // A feature's cuts depend on its column alone, so any split of the features over threads gives the same cuts.
  std::vector<std::vector<float>> per((size_t)F);
  auto work = [&](int f0, int f1) {
    std::vector<std::vector<float>> v((size_t)(f1 - f0));
    for (auto& c : v) c.reserve((size_t)n);
    for (int64_t r = 0; r < n; ++r)
      for (int f = f0; f < f1; ++f) {
        const float x = X[r * ld + f];
        if (x == x) v[f - f0].push_back(x);
      }
    for (int f = f0; f < f1; ++f) {
      std::vector<float>& c = v[f - f0];
      std::sort(c.begin(), c.end());
      const int64_t nf = (int64_t)c.size();
      std::vector<float>& out = per[f];
      for (int k = 1; k < max_bin && nf > 0 && (int)out.size() < kGbdtMaxCuts; ++k) {
        const float cand = c[(size_t)(k * nf / max_bin)];
        if (cand == c[0]) continue;                          // nothing is < it
        if (!out.empty() && cand == out.back()) continue;    // unique (sorted: equal candidates are adjacent)
        out.push_back(cand);
      }
      std::vector<float>().swap(c);
    }
  };
  const int T = std::max(1, std::min({threads, (int)F, (int)std::max<int64_t>(1, n / 4096)}));
  if (T == 1) {
    work(0, F);
  } else {
    std::vector<std::thread> pool;
    std::vector<std::exception_ptr> err((size_t)T);
    for (int t = 0; t < T; ++t)
      pool.emplace_back([&, t] {
        try {
          work((int)((int64_t)F * t / T), (int)((int64_t)F * (t + 1) / T));
        } catch (...) {
          err[t] = std::current_exception();
        }
      });
    for (auto& th : pool) th.join();
    for (auto& e : err)
      if (e) std::rethrow_exception(e);
  }
  cuts.clear();
  offsets.assign((size_t)F + 1, 0);
  for (int f = 0; f < F; ++f) {
    cuts.insert(cuts.end(), per[f].begin(), per[f].end());
    offsets[f + 1] = (int32_t)cuts.size();
  }
  return (int64_t)cuts.size();
}

void gbdt_bin_ref_host(const float* X, int64_t n, int32_t ld, int32_t F, const float* cuts, const int32_t* offsets,
                       uint8_t* bins) {
  for (int64_t r = 0; r < n; ++r)
    for (int f = 0; f < F; ++f)
      bins[r * F + f] = (uint8_t)gbdt_bin(X[r * ld + f], cuts + offsets[f],
                                          std::min(offsets[f + 1] - offsets[f], kGbdtMaxCuts));
}

void gbdt_grad_ref_host(const float* margin, const uint8_t* y, int64_t n, int32_t* g, int32_t* h) {
  for (int64_t i = 0; i < n; ++i) gbdt_grad(margin[i], y[i], g[i], h[i]);
}

void gbdt_grad_weighted_ref_host(const float* margin, const uint8_t* y, int64_t n, double w, int32_t* g, int32_t* h) {
  for (int64_t i = 0; i < n; ++i) gbdt_grad_weighted(margin[i], y[i], w, g[i], h[i]);
}

void gbdt_grow_tree_ref_host(const uint8_t* bins, int64_t n, int32_t F, const float* cuts, const int32_t* offsets,
                             const int32_t* g, const int32_t* h, const uint8_t* row_mask, uint64_t feature_mask,
                             const fd_gbdt_params& p, const fd_gbdt_model& out, int64_t* n_nodes) {
  gbdt_check_params(p, n, F, false);
  check_model(out);
  feature_mask &= all_features(F);
  FD_REQUIRE(feature_mask != 0, FD_ERR_INVALID_ARG, "gbdt: the feature mask keeps no feature");
  std::vector<int32_t> pos;
  std::vector<GbdtNode> heap;
  grow_heap_ref(bins, n, F, cuts, offsets, g, h, row_mask, feature_mask, p, pos, heap);
  const_cast<int64_t*>(out.trees->tree_offsets)[0] = 0;
  const int64_t m = emit_tree(heap.data(), out, 0, 0, nullptr);
  if (n_nodes) *n_nodes = m;
}

bool gbdt_check_eval(const fd_gbdt_eval& ev, int64_t n, int32_t F, bool host_labels) {
  const double w = ev.scale_pos_weight;
  FD_REQUIRE(w > 0.0 && w <= kGbdtMaxPosWeight, FD_ERR_INVALID_ARG, "gbdt: scale_pos_weight must be in (0, 64]");
  FD_REQUIRE((double)n * std::max(1.0, w) <= (double)kGbdtMaxRows, FD_ERR_UNSUPPORTED,
             "gbdt: n * max(1, scale_pos_weight) above 2^28 (a fixed-point sum could leave the range f64 holds exactly)");
  FD_REQUIRE(ev.metric == FD_GBDT_METRIC_AUC || ev.metric == FD_GBDT_METRIC_ERROR, FD_ERR_INVALID_ARG,
             "gbdt: unknown eval metric");
  FD_REQUIRE(ev.n >= 0 && ev.early_stopping_rounds >= 0, FD_ERR_INVALID_ARG,
             "gbdt: negative eval n or early_stopping_rounds");
  const bool has = ev.X != nullptr && ev.n > 0;
  FD_REQUIRE(has || ev.early_stopping_rounds == 0, FD_ERR_INVALID_ARG, "gbdt: early stopping needs an eval set");
  if (!has) return false;
  FD_REQUIRE(ev.y != nullptr, FD_ERR_INVALID_ARG, "gbdt: null eval labels");
  FD_REQUIRE(ev.ld >= F, FD_ERR_INVALID_ARG, "gbdt: the eval matrix is narrower than F");
  FD_REQUIRE(ev.n <= kGbdtMaxRows, FD_ERR_UNSUPPORTED, "gbdt: more than 2^28 eval rows");
  if (host_labels) gbdt_check_metric_labels(ev.y, ev.n, ev.metric);
  return true;
}

void gbdt_check_metric_labels(const uint8_t* y, int64_t n, int32_t metric) {
  int64_t pos = 0;
  for (int64_t i = 0; i < n; ++i) {
    FD_REQUIRE(y[i] <= 1, FD_ERR_INVALID_ARG, "gbdt: labels must be 0 or 1");
    pos += y[i];
  }
  FD_REQUIRE(metric != FD_GBDT_METRIC_AUC || (pos > 0 && pos < n), FD_ERR_INVALID_ARG,
             "gbdt: Only one class present in y_true. ROC AUC score is not defined in that case.");
}

// The metric on the host: the words sorted, then one pass over the tie groups (a group of a negatives and b
// positives after c negatives adds b (2 c + a) to 2U)
double gbdt_metric_ref_host(const float* margin, const uint8_t* y, int64_t n, int32_t metric) {
  if (metric == FD_GBDT_METRIC_ERROR) {
    uint64_t wrong = 0;
    for (int64_t i = 0; i < n; ++i) wrong += (uint64_t)gbdt_is_error(margin[i], y[i]);
    return gbdt_error(wrong, (uint64_t)n);
  }
  std::vector<uint64_t> words((size_t)n);
  for (int64_t i = 0; i < n; ++i) words[i] = gbdt_sort_word(margin[i], y[i]);
  std::sort(words.begin(), words.end());
  uint64_t two_u = 0, before = 0, n_pos = 0;
  for (size_t i = 0; i < words.size();) {
    uint64_t a = 0, b = 0;
    size_t j = i;
    for (; j < words.size() && (words[j] >> 1) == (words[i] >> 1); ++j) (words[j] & 1ull) ? ++b : ++a;
    two_u += b * (2 * before + a);
    before += a;
    n_pos += b;
    i = j;
  }
  return gbdt_auc(two_u, n_pos, before);
}

void gbdt_fit_ref_host(const float* X, const uint8_t* y, int64_t n, int32_t ld, int32_t F, const fd_gbdt_params& p,
                       const fd_gbdt_model& out, int64_t* n_nodes, float* margins, fd_gbdt_eval* ev) {
  gbdt_check_params(p, n, F, true);
  check_model(out);
  const bool watched = ev && gbdt_check_eval(*ev, n, F, true);
  const double w = ev ? ev->scale_pos_weight : 1.0;
  for (int64_t i = 0; i < n; ++i) FD_REQUIRE(y[i] <= 1, FD_ERR_INVALID_ARG, "gbdt: labels must be 0 or 1");
  std::vector<float> cuts;
  std::vector<int32_t> offsets;
  gbdt_cuts_host(X, n, ld, F, p.max_bin, cuts, offsets);
  cuts.push_back(0.0f);  // (data() of an empty vector may be null)
  std::vector<uint8_t> bins((size_t)n * F), mask((size_t)n);
  gbdt_bin_ref_host(X, n, ld, F, cuts.data(), offsets.data(), bins.data());
  std::vector<float> margin((size_t)n, xgb_base_margin(p.base_score));
  std::vector<int32_t> g((size_t)n), h((size_t)n), pos;
  std::vector<GbdtNode> heap;
  const RowSample rs = row_sample(p.subsample);
  const_cast<int64_t*>(out.trees->tree_offsets)[0] = 0;
  int64_t base = 0;
  std::vector<uint8_t> ebins;
  std::vector<float> emargin;
  GbdtStopState st{};
  if (watched) {
    ebins.resize((size_t)ev->n * F);
    gbdt_bin_ref_host(ev->X, ev->n, ev->ld, F, cuts.data(), offsets.data(), ebins.data());
    emargin.assign((size_t)ev->n, xgb_base_margin(p.base_score));
  }
  int t = 0;
  for (; t < p.n_rounds && !st.stop; ++t) {
    for (int64_t i = 0; i < n; ++i) {
      gbdt_grad_weighted(margin[i], y[i], w, g[i], h[i]);
      mask[i] = gbdt_row_sampled(p.seed, (uint32_t)t, (uint64_t)i, rs.threshold, rs.all) ? 1 : 0;
    }
    const uint64_t fm = round_feature_mask(p.seed, (uint32_t)t, F, p.colsample_bytree);
    grow_heap_ref(bins.data(), n, F, cuts.data(), offsets.data(), g.data(), h.data(), mask.data(), fm, p, pos, heap);
    for (int64_t i = 0; i < n; ++i) margin[i] = margin[i] + heap[pos[i]].leaf;
    base += emit_tree(heap.data(), out, base, t, nullptr);
    if (!watched) continue;
    for (int64_t i = 0; i < ev->n; ++i) {
      int q = 0;
      while (heap[q].state == kGbdtSplit)
        q = 2 * q + (gbdt_goes_left(heap[q], ebins[(size_t)i * F + heap[q].feature]) ? 1 : 2);
      emargin[i] = emargin[i] + heap[q].leaf;
    }
    const double v = gbdt_metric_ref_host(emargin.data(), ev->y, ev->n, ev->metric);
    if (ev->metric_out) ev->metric_out[t] = v;
    gbdt_stop_update(st, t, v, ev->metric == FD_GBDT_METRIC_AUC, ev->early_stopping_rounds);
    if (st.best_round == t && ev->best_margins) std::copy(margin.begin(), margin.end(), ev->best_margins);
  }
  if (ev) {
    ev->rounds_run = t;
    ev->best_iteration = watched ? st.best_round : -1;
    if (watched && ev->margins) std::copy(emargin.begin(), emargin.end(), ev->margins);
  }
  if (n_nodes) *n_nodes = base;
  if (margins) std::copy(margin.begin(), margin.end(), margins);
}

// ------------------------------------------------------------------------------------------------ device API

void launch_gbdt_bin(Engine& e, const float* d_X, int64_t n, int32_t ld, int32_t F, const float* d_cuts,
                     const int32_t* d_offsets, uint8_t* d_bins) {
  FD_REQUIRE(F >= 1 && F <= 64 && ld >= F && n >= 0, FD_ERR_INVALID_ARG, "gbdt: F must be in 1..64 and ld >= F");
  if (n == 0) return;
  const unsigned gx = std::min<unsigned>(row_blocks(n), 4096u);
  gbdt_bin_kernel<<<dim3(gx, (unsigned)F), kGbdtThreads, 0, e.stream>>>(d_X, n, ld, F, d_cuts, d_offsets, d_bins);
  FD_HIP(hipGetLastError());
}

void launch_gbdt_grad(Engine& e, const float* d_margin, const uint8_t* d_y, int64_t n, int32_t* d_g, int32_t* d_h) {
  if (n <= 0) return;
  gbdt_grad_kernel<<<row_blocks(n), kGbdtThreads, 0, e.stream>>>(d_margin, d_y, n, d_g, d_h);
  FD_HIP(hipGetLastError());
}

namespace {

// one tree's launches on e.stream: d_pos holds 0 for every row on entry; d_heap (heap_nodes entries) is zeroed
void launch_tree(Engine& e, const uint8_t* d_bins, int64_t n, int F, const float* d_cuts, const int32_t* d_offsets,
                 const int32_t* d_g, const int32_t* d_h, const uint8_t* d_mask, uint64_t feat_mask,
                 const fd_gbdt_params& p, int32_t* d_pos, GbdtNode* d_heap, const GbdtStopState* st = nullptr) {
  GbdtScratch& s = e.gbdt;
  auto* hist = s.hist.as<unsigned long long>();
  const int rows = s.hist_rows;
  const unsigned gx = (unsigned)((n + rows - 1) / rows);
  for (int level = 0; level < p.max_depth; ++level) {
    const int nn = 1 << level;
    FD_HIP(hipMemsetAsync(hist, 0, (size_t)nn * F * kGbdtBins * 16, e.stream));
    if (st) {  // a fit with early stopping: the same launches by the kernels that read the stop flag
      if (n > 0) {
        if (nn <= kHistPairs) {
          const int ft = std::min(F, kHistPairs / nn);
          gbeval_hist_kernel<true><<<dim3(gx, (unsigned)((F + ft - 1) / ft)), kGbdtThreads, 0, e.stream>>>(
              d_bins, d_g, d_h, d_mask, d_pos, n, F, level, feat_mask, rows, ft, hist, st);
        } else {
          gbeval_hist_kernel<false><<<dim3(gx, 1), kGbdtThreads, 0, e.stream>>>(d_bins, d_g, d_h, d_mask, d_pos, n, F,
                                                                                level, feat_mask, rows, F, hist, st);
        }
        ++s.hist_launches;
      }
      gbeval_split_kernel<<<nn, kGbdtThreads, 0, e.stream>>>(hist, d_heap, level, F, feat_mask, d_cuts, d_offsets,
                                                             p.lambda, p.min_child_weight, p.eta, st);
      if (n > 0)
        gbeval_route_kernel<<<row_blocks(n), kGbdtThreads, 0, e.stream>>>(d_bins, d_pos, n, F, d_heap, level, st);
      continue;
    }
    if (n > 0) {
      if (nn <= kHistPairs) {
        const int ft = std::min(F, kHistPairs / nn);
        gbdt_hist_kernel<true><<<dim3(gx, (unsigned)((F + ft - 1) / ft)), kGbdtThreads, 0, e.stream>>>(
            d_bins, d_g, d_h, d_mask, d_pos, n, F, level, feat_mask, rows, ft, hist);
      } else {
        gbdt_hist_kernel<false><<<dim3(gx, 1), kGbdtThreads, 0, e.stream>>>(d_bins, d_g, d_h, d_mask, d_pos, n, F,
                                                                            level, feat_mask, rows, F, hist);
      }
      ++s.hist_launches;
    }
    gbdt_split_kernel<<<nn, kGbdtThreads, 0, e.stream>>>(hist, d_heap, level, F, feat_mask, d_cuts, d_offsets,
                                                         p.lambda, p.min_child_weight, p.eta);
    if (n > 0) gbdt_route_kernel<<<row_blocks(n), kGbdtThreads, 0, e.stream>>>(d_bins, d_pos, n, F, d_heap, level);
  }
  FD_HIP(hipGetLastError());
}

void upload_cuts(Engine& e, const float* cuts, const int32_t* offsets, int F) {
  GbdtScratch& s = e.gbdt;
  const size_t nc = (size_t)offsets[F];
  s.cuts.ensure(std::max<size_t>(nc * 4, 4));
  s.offsets.ensure((size_t)(F + 1) * 4);
  if (nc) FD_HIP(hipMemcpyAsync(s.cuts.ptr, cuts, nc * 4, hipMemcpyHostToDevice, e.stream));
  FD_HIP(hipMemcpyAsync(s.offsets.ptr, offsets, (size_t)(F + 1) * 4, hipMemcpyHostToDevice, e.stream));
}

void check_offsets(const int32_t* offsets, int F) {
  FD_REQUIRE(offsets && offsets[0] == 0, FD_ERR_INVALID_ARG, "gbdt: cut offsets must start at 0");
  for (int f = 0; f < F; ++f)
    FD_REQUIRE(offsets[f + 1] >= offsets[f] && offsets[f + 1] - offsets[f] <= kGbdtMaxCuts, FD_ERR_INVALID_ARG,
               "gbdt: a feature has a negative number of cuts or more than 254");
}

}  // namespace

void gbdt_grow_tree_device(Engine& e, const uint8_t* d_bins, int64_t n, int32_t F, const float* cuts,
                           const int32_t* offsets, const int32_t* d_g, const int32_t* d_h, const uint8_t* d_row_mask,
                           uint64_t feature_mask, const fd_gbdt_params& p, const fd_gbdt_model& out, int64_t* n_nodes) {
  gbdt_check_params(p, n, F, false);
  check_model(out);
  check_offsets(offsets, F);
  feature_mask &= all_features(F);
  FD_REQUIRE(feature_mask != 0, FD_ERR_INVALID_ARG, "gbdt: the feature mask keeps no feature");
  GbdtScratch& s = e.gbdt;
  const int NH = heap_nodes(p.max_depth);
  upload_cuts(e, cuts, offsets, F);
  s.pos.ensure(std::max<size_t>((size_t)n * 4, 4));
  s.nodes.ensure((size_t)NH * sizeof(GbdtNode));
  s.hist.ensure((size_t)(1 << (p.max_depth - 1)) * F * kGbdtBins * 16);
  FD_HIP(hipMemsetAsync(s.pos.ptr, 0, std::max<size_t>((size_t)n * 4, 4), e.stream));
  FD_HIP(hipMemsetAsync(s.nodes.ptr, 0, (size_t)NH * sizeof(GbdtNode), e.stream));
  launch_tree(e, d_bins, n, F, s.cuts.as<float>(), s.offsets.as<int32_t>(), d_g, d_h, d_row_mask, feature_mask, p,
              s.pos.as<int32_t>(), s.nodes.as<GbdtNode>());
  std::vector<GbdtNode> heap((size_t)NH);
  FD_HIP(hipMemcpyAsync(heap.data(), s.nodes.ptr, (size_t)NH * sizeof(GbdtNode), hipMemcpyDeviceToHost, e.stream));
  FD_HIP(hipStreamSynchronize(e.stream));
  const_cast<int64_t*>(out.trees->tree_offsets)[0] = 0;
  int64_t split = 0;
  const int64_t m = emit_tree(heap.data(), out, 0, 0, &split);
  ++s.trees;
  s.nodes_split += (unsigned long long)split;
  if (n_nodes) *n_nodes = m;
}

namespace {

// The eval buffers of a fit (or of fd_gbdt_metric_host) for ne rows; the temporary storage of the sort and of the
// scan is asked for once here and kept
void ensure_eval(Engine& e, int64_t ne, int F, int n_rounds, bool auc) {
  GbdtScratch& s = e.gbdt;
  const size_t m = (size_t)std::max<int64_t>(ne, 1);
  s.ebins.ensure(m * (size_t)std::max(F, 1));
  s.emargin.ensure(m * 4);
  s.curve.ensure((size_t)std::max(n_rounds, 1) * 8);
  s.state.ensure(sizeof(GbdtEvalState));
  s.eval_tmp_bytes = 0;
  if (!auc) return;
  s.words.ensure(m * 16);
  s.neg_before.ensure(m * 4);
  auto* w = s.words.as<uint64_t>();
  size_t sort_b = 0, scan_b = 0;
  FD_HIP(rocprim::radix_sort_keys(nullptr, sort_b, w, w + m, m, 0, kGbdtSortBits, e.stream));
  FD_HIP(rocprim::exclusive_scan(nullptr, scan_b, rocprim::make_transform_iterator(w + m, EvalNegFlag()),
                                 s.neg_before.as<uint32_t>(), 0u, m, rocprim::plus<uint32_t>(), e.stream));
  s.eval_tmp_bytes = std::max<size_t>(std::max(sort_b, scan_b), 16);
  s.eval_tmp.ensure(s.eval_tmp_bytes);
}

// One round's evaluation on e.stream: the walk (heap: the round's tree; null: d_margin as it is), for AUC the sort,
// the scan and the count, and the state kernel. d_margin: ne f32, read and written.
void launch_eval(Engine& e, const uint8_t* d_ebins, const uint8_t* d_ey, int64_t ne, int F, const GbdtNode* d_heap,
                 int max_depth, bool first, float base, float* d_margin, int metric, int round, int k) {
  GbdtScratch& s = e.gbdt;
  auto* es = s.state.as<GbdtEvalState>();
  const GbdtStopState* st = &es->stop;
  auto* words = s.words.as<uint64_t>();
  auto* sorted = words ? words + ne : nullptr;
  auto* neg_before = s.neg_before.as<uint32_t>();
  if (metric == FD_GBDT_METRIC_AUC) {
    gbeval_walk_kernel<true><<<row_blocks(ne), kGbdtThreads, 0, e.stream>>>(
        d_ebins, d_ey, ne, F, d_heap, max_depth, first ? 1 : 0, base, d_margin, words, &es->acc, st);
    size_t tb = s.eval_tmp_bytes;
    FD_HIP(rocprim::radix_sort_keys(s.eval_tmp.ptr, tb, words, sorted, (size_t)ne, 0, kGbdtSortBits, e.stream));
    tb = s.eval_tmp_bytes;
    FD_HIP(rocprim::exclusive_scan(s.eval_tmp.ptr, tb, rocprim::make_transform_iterator(sorted, EvalNegFlag()),
                                   neg_before, 0u, (size_t)ne, rocprim::plus<uint32_t>(), e.stream));
    gbeval_count_kernel<<<std::min<unsigned>(row_blocks(ne), 4096u), kGbdtThreads, 0, e.stream>>>(
        sorted, neg_before, ne, &es->acc, st);
  } else {
    gbeval_walk_kernel<false><<<row_blocks(ne), kGbdtThreads, 0, e.stream>>>(
        d_ebins, d_ey, ne, F, d_heap, max_depth, first ? 1 : 0, base, d_margin, nullptr, &es->acc, st);
  }
  gbeval_state_kernel<<<1, 64, 0, e.stream>>>(es, sorted, neg_before, ne, metric, round, k, s.curve.as<double>());
  FD_HIP(hipGetLastError());
}

}  // namespace

double gbdt_metric_device(Engine& e, const float* d_margin, const uint8_t* d_y, int64_t n, int32_t metric) {
  GbdtScratch& s = e.gbdt;
  ensure_eval(e, n, 1, 1, metric == FD_GBDT_METRIC_AUC);
  FD_HIP(hipMemsetAsync(s.state.ptr, 0, sizeof(GbdtEvalState), e.stream));
  launch_eval(e, nullptr, d_y, n, 1, nullptr, 0, false, 0.0f, const_cast<float*>(d_margin), metric, 0, 0);
  double v = 0.0;
  FD_HIP(hipMemcpyAsync(&v, s.curve.ptr, 8, hipMemcpyDeviceToHost, e.stream));
  FD_HIP(hipStreamSynchronize(e.stream));
  return v;
}

// h_X: the matrix on the host when the caller has it (else it is copied back once, for the cuts). ev: null, or the
// watched fit's arguments with device pointers (X, y, margins, best_margins) and a host metric_out.
static void fit_device(Engine& e, const float* d_X, const float* h_X, const uint8_t* d_y, int64_t n, int32_t ld,
                       int32_t F, const fd_gbdt_params& p, const fd_gbdt_model& out, int64_t* n_nodes,
                       float* d_margins, fd_gbdt_eval* ev = nullptr) {
  gbdt_check_params(p, n, F, true);
  check_model(out);
  const bool watched = ev && gbdt_check_eval(*ev, n, F, false);
  GbdtScratch& s = e.gbdt;
  std::vector<float> back;
  if (!h_X && n > 0) {
    back.resize((size_t)n * ld);
    FD_HIP(hipMemcpyAsync(back.data(), d_X, back.size() * 4, hipMemcpyDeviceToHost, e.stream));
    FD_HIP(hipStreamSynchronize(e.stream));
    h_X = back.data();
  }
  std::vector<float> cuts;
  std::vector<int32_t> offsets;
  gbdt_cuts_host(h_X, n, ld, F, p.max_bin, cuts, offsets, kCutThreads);
  std::vector<float>().swap(back);
  cuts.push_back(0.0f);
  upload_cuts(e, cuts.data(), offsets.data(), F);
  const int NH = heap_nodes(p.max_depth);
  const size_t nn = std::max<size_t>((size_t)n, 1);
  s.bins.ensure(nn * F);
  s.gh.ensure(nn * 8);
  s.mask.ensure(nn);
  s.pos.ensure(nn * 4);
  s.margin.ensure(nn * 4);
  s.nodes.ensure((size_t)p.n_rounds * NH * sizeof(GbdtNode));
  s.hist.ensure((size_t)(1 << (p.max_depth - 1)) * F * kGbdtBins * 16);
  auto* bins = s.bins.as<uint8_t>();
  auto* g = s.gh.as<int32_t>();
  auto* h = g + nn;
  auto* mask = s.mask.as<uint8_t>();
  auto* pos = s.pos.as<int32_t>();
  auto* margin = s.margin.as<float>();
  auto* nodes = s.nodes.as<GbdtNode>();
  launch_gbdt_bin(e, d_X, n, ld, F, s.cuts.as<float>(), s.offsets.as<int32_t>(), bins);
  FD_HIP(hipMemsetAsync(nodes, 0, (size_t)p.n_rounds * NH * sizeof(GbdtNode), e.stream));
  const RowSample rs = row_sample(p.subsample);
  const float base = xgb_base_margin(p.base_score);
  // the watched fit: the eval rows binned with the training cuts, the stop state zeroed; the per-level kernels read
  // the stop flag only when the fit can stop
  const int64_t ne = watched ? ev->n : 0;
  const int k = watched ? ev->early_stopping_rounds : 0;
  const GbdtStopState* st = nullptr;
  float* best_margin = nullptr;
  if (watched) {
    ensure_eval(e, ne, F, p.n_rounds, ev->metric == FD_GBDT_METRIC_AUC);
    s.best_margin.ensure(nn * 4);
    best_margin = s.best_margin.as<float>();
    st = &s.state.as<GbdtEvalState>()->stop;
    FD_HIP(hipMemsetAsync(s.state.ptr, 0, sizeof(GbdtEvalState), e.stream));
    launch_gbdt_bin(e, ev->X, ne, ev->ld, F, s.cuts.as<float>(), s.offsets.as<int32_t>(), s.ebins.as<uint8_t>());
  }
  const unsigned long long hist0 = s.hist_launches;
  for (int t = 0; t <= p.n_rounds; ++t) {  // the last pass only applies the last tree
    const bool grow = t < p.n_rounds;
    const GbdtNode* prev = t ? nodes + (size_t)(t - 1) * NH : nullptr;
    if (n > 0 && !ev)
      gbdt_round_kernel<<<row_blocks(n), kGbdtThreads, 0, e.stream>>>(margin, d_y, n, prev, base, pos, g, h, mask,
                                                                      p.seed, (uint32_t)t, rs.threshold,
                                                                      rs.all ? 1 : 0, grow ? 1 : 0);
    else if (n > 0)
      gbeval_round_kernel<<<row_blocks(n), kGbdtThreads, 0, e.stream>>>(
          margin, d_y, n, prev, base, pos, g, h, mask, p.seed, (uint32_t)t, rs.threshold, rs.all ? 1 : 0,
          grow ? 1 : 0, ev->scale_pos_weight, st, best_margin);
    if (!grow) break;
    launch_tree(e, bins, n, F, s.cuts.as<float>(), s.offsets.as<int32_t>(), g, h, mask,
                round_feature_mask(p.seed, (uint32_t)t, F, p.colsample_bytree), p, pos, nodes + (size_t)t * NH,
                k > 0 ? st : nullptr);
    if (watched)
      launch_eval(e, s.ebins.as<uint8_t>(), ev->y, ne, F, nodes + (size_t)t * NH, p.max_depth, t == 0, base,
                  s.emargin.as<float>(), ev->metric, t, k);
  }
  FD_HIP(hipGetLastError());
  std::vector<GbdtNode> heaps((size_t)p.n_rounds * NH);
  FD_HIP(hipMemcpyAsync(heaps.data(), nodes, heaps.size() * sizeof(GbdtNode), hipMemcpyDeviceToHost, e.stream));
  if (d_margins && n > 0)
    FD_HIP(hipMemcpyAsync(d_margins, margin, (size_t)n * 4, hipMemcpyDeviceToDevice, e.stream));
  GbdtEvalState es{};
  std::vector<double> curve;
  if (watched) {
    curve.resize((size_t)p.n_rounds);
    FD_HIP(hipMemcpyAsync(&es, s.state.ptr, sizeof(es), hipMemcpyDeviceToHost, e.stream));
    FD_HIP(hipMemcpyAsync(curve.data(), s.curve.ptr, curve.size() * 8, hipMemcpyDeviceToHost, e.stream));
    if (ev->margins)
      FD_HIP(hipMemcpyAsync(ev->margins, s.emargin.ptr, (size_t)ne * 4, hipMemcpyDeviceToDevice, e.stream));
    if (ev->best_margins && n > 0)
      FD_HIP(hipMemcpyAsync(ev->best_margins, best_margin, (size_t)n * 4, hipMemcpyDeviceToDevice, e.stream));
  }
  FD_HIP(hipStreamSynchronize(e.stream));
  const int rounds_run = watched ? es.stop.rounds_run : p.n_rounds;
  if (ev) {
    ev->rounds_run = rounds_run;
    ev->best_iteration = watched ? es.stop.best_round : -1;
    if (watched && ev->metric_out) std::copy(curve.begin(), curve.begin() + rounds_run, ev->metric_out);
  }
  const_cast<int64_t*>(out.trees->tree_offsets)[0] = 0;
  int64_t base_node = 0, split = 0;
  for (int t = 0; t < rounds_run; ++t) base_node += emit_tree(heaps.data() + (size_t)t * NH, out, base_node, t, &split);
  // the launches of the rounds after a stop returned at the flag: they are not counted
  if (n > 0) s.hist_launches = hist0 + (unsigned long long)rounds_run * (unsigned long long)p.max_depth;
  s.trees += (unsigned long long)rounds_run;
  s.rounds_run += (unsigned long long)rounds_run;
  if (watched) s.eval_launches += (unsigned long long)rounds_run;
  s.nodes_split += (unsigned long long)split;
  if (n_nodes) *n_nodes = base_node;
}

void gbdt_fit_eval_device(Engine& e, const float* d_X, const float* h_X, const uint8_t* d_y, int64_t n, int32_t ld,
                          int32_t F, const fd_gbdt_params& p, fd_gbdt_eval& ev, const fd_gbdt_model& out,
                          int64_t* n_nodes, float* d_margins) {
  fit_device(e, d_X, h_X, d_y, n, ld, F, p, out, n_nodes, d_margins, &ev);
}

void gbdt_fit_device(Engine& e, const float* d_X, const uint8_t* d_y, int64_t n, int32_t ld, int32_t F,
                     const fd_gbdt_params& p, const fd_gbdt_model& out, int64_t* n_nodes, float* d_margins) {
  fit_device(e, d_X, nullptr, d_y, n, ld, F, p, out, n_nodes, d_margins);
}

void gbdt_fit_staged(Engine& e, const float* d_X, const float* h_X, const uint8_t* d_y, int64_t n, int32_t ld,
                     int32_t F, const fd_gbdt_params& p, const fd_gbdt_model& out, int64_t* n_nodes,
                     float* d_margins) {
  fit_device(e, d_X, h_X, d_y, n, ld, F, p, out, n_nodes, d_margins);
}

}  // namespace fd
