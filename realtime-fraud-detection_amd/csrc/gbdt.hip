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
#include <algorithm>
#include <cmath>
#include <exception>
#include <numeric>

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

// kLds: grid (row blocks, feature tiles of ft features), nodes * ft <= kHistPairs; else grid (row blocks, 1)
template <bool kLds>
__global__ void __launch_bounds__(kGbdtThreads) gbdt_hist_kernel(const uint8_t* __restrict__ bins,
                                                                 const int32_t* __restrict__ g,
                                                                 const int32_t* __restrict__ h,
                                                                 const uint8_t* __restrict__ mask,
                                                                 const int32_t* __restrict__ pos, int64_t n, int F,
                                                                 int level, uint64_t feat_mask, int rows_per_wg,
                                                                 int ft, unsigned long long* __restrict__ hist) {
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

// grid: the level's nodes. hist: the level's histograms; heap: the tree's nodes
__global__ void __launch_bounds__(kGbdtThreads) gbdt_split_kernel(const unsigned long long* __restrict__ hist,
                                                                  GbdtNode* __restrict__ heap, int level, int F,
                                                                  uint64_t feat_mask, const float* __restrict__ cuts,
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

__global__ void __launch_bounds__(kGbdtThreads) gbdt_route_kernel(const uint8_t* __restrict__ bins,
                                                                  int32_t* __restrict__ pos, int64_t n, int F,
                                                                  const GbdtNode* __restrict__ heap, int level) {
  const int64_t i = (int64_t)blockIdx.x * kGbdtThreads + threadIdx.x;
  if (i >= n) return;
  const int p = pos[i];
  if (p < (1 << level) - 1) return;
  const GbdtNode nd = heap[p];
  if (nd.state != kGbdtSplit) return;
  pos[i] = 2 * p + (gbdt_goes_left(nd, bins[i * F + nd.feature]) ? 1 : 2);
}

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

void gbdt_fit_ref_host(const float* X, const uint8_t* y, int64_t n, int32_t ld, int32_t F, const fd_gbdt_params& p,
                       const fd_gbdt_model& out, int64_t* n_nodes, float* margins) {
  gbdt_check_params(p, n, F, true);
  check_model(out);
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
  for (int t = 0; t < p.n_rounds; ++t) {
    for (int64_t i = 0; i < n; ++i) {
      gbdt_grad(margin[i], y[i], g[i], h[i]);
      mask[i] = gbdt_row_sampled(p.seed, (uint32_t)t, (uint64_t)i, rs.threshold, rs.all) ? 1 : 0;
    }
    const uint64_t fm = round_feature_mask(p.seed, (uint32_t)t, F, p.colsample_bytree);
    grow_heap_ref(bins.data(), n, F, cuts.data(), offsets.data(), g.data(), h.data(), mask.data(), fm, p, pos, heap);
    for (int64_t i = 0; i < n; ++i) margin[i] = margin[i] + heap[pos[i]].leaf;
    base += emit_tree(heap.data(), out, base, t, nullptr);
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
                 const fd_gbdt_params& p, int32_t* d_pos, GbdtNode* d_heap) {
  GbdtScratch& s = e.gbdt;
  auto* hist = s.hist.as<unsigned long long>();
  const int rows = s.hist_rows;
  const unsigned gx = (unsigned)((n + rows - 1) / rows);
  for (int level = 0; level < p.max_depth; ++level) {
    const int nn = 1 << level;
    FD_HIP(hipMemsetAsync(hist, 0, (size_t)nn * F * kGbdtBins * 16, e.stream));
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

// h_X: the matrix on the host when the caller has it (else it is copied back once, for the cuts)
static void fit_device(Engine& e, const float* d_X, const float* h_X, const uint8_t* d_y, int64_t n, int32_t ld,
                       int32_t F, const fd_gbdt_params& p, const fd_gbdt_model& out, int64_t* n_nodes,
                       float* d_margins) {
  gbdt_check_params(p, n, F, true);
  check_model(out);
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
  for (int t = 0; t <= p.n_rounds; ++t) {  // the last pass only applies the last tree
    const bool grow = t < p.n_rounds;
    if (n > 0)
      gbdt_round_kernel<<<row_blocks(n), kGbdtThreads, 0, e.stream>>>(
          margin, d_y, n, t ? nodes + (size_t)(t - 1) * NH : nullptr, base, pos, g, h, mask, p.seed, (uint32_t)t,
          rs.threshold, rs.all ? 1 : 0, grow ? 1 : 0);
    if (grow)
      launch_tree(e, bins, n, F, s.cuts.as<float>(), s.offsets.as<int32_t>(), g, h, mask,
                  round_feature_mask(p.seed, (uint32_t)t, F, p.colsample_bytree), p, pos, nodes + (size_t)t * NH);
  }
  FD_HIP(hipGetLastError());
  std::vector<GbdtNode> heaps((size_t)p.n_rounds * NH);
  FD_HIP(hipMemcpyAsync(heaps.data(), nodes, heaps.size() * sizeof(GbdtNode), hipMemcpyDeviceToHost, e.stream));
  if (d_margins && n > 0)
    FD_HIP(hipMemcpyAsync(d_margins, margin, (size_t)n * 4, hipMemcpyDeviceToDevice, e.stream));
  FD_HIP(hipStreamSynchronize(e.stream));
  const_cast<int64_t*>(out.trees->tree_offsets)[0] = 0;
  int64_t base_node = 0, split = 0;
  for (int t = 0; t < p.n_rounds; ++t) base_node += emit_tree(heaps.data() + (size_t)t * NH, out, base_node, t, &split);
  s.trees += (unsigned long long)p.n_rounds;
  s.nodes_split += (unsigned long long)split;
  if (n_nodes) *n_nodes = base_node;
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
