// iforest_fit.hip — the IsolationForest fit (ModelTrainer.train_isolation_forest's fit, ml/training/
// model_trainer.py:235-276): kernels, the offset pass and the single-threaded host reference. The arithmetic is
// iforest_fit_row.h, compiled by both; the semantics are declared in include/fdengine.h ("training: IsolationForest")
// and DESIGN §4.15.
//
// A fit is two launches and one copy back, whatever the number of trees:
//   iforest_fit_sample_kernel  a thread per (tree, j): the row id perm_t(j), [tree][psi] int32.
//   iforest_fit_grow_kernel    a workgroup per tree. The tree's psi rows are gathered once into LDS, row-major with an
//                              odd stride (a wave reading one row is conflict-free, and so is a wave reading one
//                              feature of 64 rows), when they fit beside the bookkeeping; else every read goes to the
//                              row of X itself, one coalesced read of F floats (the rows of a tree are the same 4 F psi
//                              bytes either way, and a level rereads them out of the cache). Bookkeeping in LDS: a u16
//                              permutation of the sample slots kept partitioned by node (ping-pong between levels) and
//                              (start, count) per heap slot. Per level a wave takes one node at a time: lane = feature,
//                              every lane keeps its feature's min and max over the node's segment in registers (no
//                              atomics, no LDS arrays), a ballot of max > min is the set of non-constant features, the
//                              chosen lane's min and max are shuffled out, and the wave partitions the segment 64 slots
//                              at a time by ballot and prefix count (left from the front, right from the back). Lane 0
//                              writes the node's {threshold, feature, count} to the tree's heap in global memory.
// The heaps of all trees come back in one copy and are renumbered breadth-first on the host, where the leaf term
// depth + c(count) is added from one table of c (the device takes no logarithm).
// The offset (contamination > 0): the grown forest is packed as fd_load_forest packs it (into a forest of the fit's
// own, no slot), the fit rows are scored by the serving kernels (f64 path-length sums in tree order: the same bits for
// any batch), the sums sorted by rocPRIM's radix sort, and the two order statistics around contamination (n - 1) are
// the 16 bytes that come back.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <numeric>
#include <vector>

#include <rocprim/rocprim.hpp>

#include "fd_internal.h"
#include "iforest_fit_row.h"

namespace fd {
namespace {

constexpr int kIfThreads = 256;
constexpr int kIfWaves = kIfThreads / 64;
constexpr size_t kIfSampleLds = 128 * 1024;  // the gathered rows' share of a CU's 160 KiB (16 KiB of bookkeeping)

inline int heap_nodes(int D) { return (1 << (D + 1)) - 1; }
inline uint64_t all_features(int F) { return F >= 64 ? ~0ull : (1ull << F) - 1ull; }
FD_HD int sample_stride(int F) { return F | 1; }

// ------------------------------------------------------------------------------------------------ kernels

// grid: ceil(T * psi / 256); rows[t * psi + j] = perm_{tree0 + t}(j)
__global__ void __launch_bounds__(kIfThreads) iforest_fit_sample_kernel(uint64_t key, uint32_t tree0, int T, int psi,
                                                                        int64_t n, int half_bits,
                                                                        int32_t* __restrict__ rows) {
  const int64_t i = (int64_t)blockIdx.x * kIfThreads + threadIdx.x;
  if (i >= (int64_t)T * psi) return;
  const uint32_t t = (uint32_t)(i / psi);
  rows[i] = (int32_t)iforest_perm(key, tree0 + t, n, half_bits, i - (int64_t)t * psi);
}

// grid: T workgroups; rows: [T][psi] ids in [0, n); masks: [T] kept features; heaps: [T][2^(D + 1) - 1], zeroed
template <bool kLds>
__global__ void __launch_bounds__(kIfThreads) iforest_fit_grow_kernel(const float* __restrict__ X, int32_t ld, int F,
                                                                      const int32_t* __restrict__ rows, int psi, int D,
                                                                      const uint64_t* __restrict__ masks, uint64_t key,
                                                                      uint32_t tree0, IfNode* __restrict__ heaps) {
  extern __shared__ float s_samples[];  // kLds: [psi][F | 1]
  __shared__ int32_t s_rows[kIfMaxSamples];
  __shared__ uint16_t s_perm[2][kIfMaxSamples];
  __shared__ uint16_t s_start[kIfHeapMax + 1], s_count[kIfHeapMax + 1];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const uint32_t tree = tree0 + blockIdx.x;
  const int NH = (1 << (D + 1)) - 1;
  IfNode* heap = heaps + (size_t)blockIdx.x * NH;
  const uint64_t fmask = masks[blockIdx.x];
  const int stride = sample_stride(F);
  for (int j = tid; j < psi; j += kIfThreads) {
    s_rows[j] = rows[(size_t)blockIdx.x * psi + j];
    s_perm[0][j] = (uint16_t)j;
  }
  for (int i = tid; i < NH; i += kIfThreads) s_count[i] = 0;
  __syncthreads();
  if (tid == 0) {
    s_start[0] = 0;
    s_count[0] = (uint16_t)psi;
  }
  if (kLds) {
    for (int p = wave; p < psi; p += kIfWaves)
      if (lane < F) s_samples[p * stride + lane] = X[(int64_t)s_rows[p] * ld + lane];
  }
  __syncthreads();
  const bool kept = lane < F && ((fmask >> lane) & 1ull);
  int cur = 0;
  for (int d = 0; d <= D; ++d) {
    const int first = (1 << d) - 1, nn = 1 << d;
    const uint16_t* pc = s_perm[cur];
    uint16_t* pn = s_perm[cur ^ 1];
    for (int k = wave; k < nn; k += kIfWaves) {  // (every condition below is the same for the whole wave)
      const int idx = first + k;
      const int m = s_count[idx];
      if (m == 0) continue;
      const int st = s_start[idx];
      int feature = -1;
      double thr = 0.0;
      if (m > 1 && d < D) {
        float mn = __builtin_huge_valf(), mx = -__builtin_huge_valf();
        if (kept) {
          for (int i = 0; i < m; ++i) {
            const int p = pc[st + i];
            const float x = kLds ? s_samples[p * stride + lane] : X[(int64_t)s_rows[p] * ld + lane];
            iforest_minmax(x, mn, mx);
          }
        }
        const uint64_t varying = __ballot(kept && mx > mn);
        const int c = __popcll(varying);
        if (c > 0) {
          feature = iforest_nth_bit(varying, iforest_pick(iforest_hash(key, tree, (uint32_t)idx, kIfTagFeature), c));
          const float fmn = __shfl(mn, feature), fmx = __shfl(mx, feature);
          thr = iforest_threshold(fmn, fmx, iforest_hash(key, tree, (uint32_t)idx, kIfTagThreshold));
          const uint64_t below = (1ull << lane) - 1ull;
          int nl = 0, nr = 0;
          for (int base = 0; base < m; base += 64) {
            const int i = base + lane;
            const bool in = i < m;
            int p = 0;
            bool left = false;
            if (in) {
              p = pc[st + i];
              const float x = kLds ? s_samples[p * stride + feature] : X[(int64_t)s_rows[p] * ld + feature];
              left = iforest_goes_left(x, thr);
            }
            const uint64_t bl = __ballot(in && left), br = __ballot(in && !left);
            if (in) {
              if (left) pn[st + nl + __popcll(bl & below)] = (uint16_t)p;
              else pn[st + m - 1 - (nr + __popcll(br & below))] = (uint16_t)p;
            }
            nl += __popcll(bl);
            nr += __popcll(br);
          }
          if (lane == 0) {
            s_start[2 * idx + 1] = (uint16_t)st;
            s_count[2 * idx + 1] = (uint16_t)nl;
            s_start[2 * idx + 2] = (uint16_t)(st + nl);
            s_count[2 * idx + 2] = (uint16_t)nr;
          }
        }
      }
      if (lane == 0) heap[idx] = IfNode{thr, feature, m};
    }
    __syncthreads();
    cur ^= 1;
  }
}

// ------------------------------------------------------------------------------------------------ host pieces

// c[0 .. psi]: scikit-learn's _average_path_length; the only logarithms of a fit
std::vector<double> path_length_table(int psi) {
#pragma clang fp contract(off)
  std::vector<double> c((size_t)psi + 1, 0.0);
  for (int m = 2; m <= psi; ++m) {
    const double v = (double)m;
    c[m] = m == 2 ? 1.0 : 2.0 * (std::log(v - 1.0) + 0.5772156649015329) - 2.0 * (v - 1.0) / v;
  }
  return c;
}

// max_features: the max(1, floor(c F)) features with the smallest hash, ties to the lower index
uint64_t tree_feature_mask(uint64_t key, uint32_t tree, int F, double max_features) {
  const int keep = std::max(1, (int)std::floor(max_features * (double)F));
  if (keep >= F) return all_features(F);
  std::vector<int> order(F);
  std::iota(order.begin(), order.end(), 0);
  std::vector<uint64_t> hash(F);
  for (int f = 0; f < F; ++f) hash[f] = iforest_hash(key, tree, (uint32_t)f, kIfTagSubset);
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return hash[a] < hash[b]; });
  uint64_t m = 0;
  for (int k = 0; k < keep; ++k) m |= 1ull << order[k];
  return m;
}

void check_out(const fd_tree_arrays& t) {
  FD_REQUIRE(t.tree_offsets && t.left && t.right && t.feature && t.threshold && t.leaf_value, FD_ERR_INVALID_ARG,
             "iforest_fit: null output arrays");
}

// a tree's heap appended to the caller's arrays in breadth-first numbering -> its node count
int64_t emit_tree(const IfNode* heap, const std::vector<double>& c, const fd_tree_arrays& t, double* n_node_samples,
                  int64_t base, int tree, int64_t* n_split) {
#pragma clang fp contract(off)
  auto* left = const_cast<int32_t*>(t.left) + base;
  auto* right = const_cast<int32_t*>(t.right) + base;
  auto* feature = const_cast<int32_t*>(t.feature) + base;
  auto* threshold = const_cast<double*>(t.threshold) + base;
  auto* dleft = t.default_left ? const_cast<uint8_t*>(t.default_left) + base : nullptr;
  auto* leaf = const_cast<double*>(t.leaf_value) + base;
  std::vector<int> queue{0}, depth{0};
  for (size_t q = 0; q < queue.size(); ++q) {  // a split node's children take the next two numbers
    const IfNode& nd = heap[queue[q]];
    const bool split = nd.feature >= 0;
    if (split) {
      left[q] = (int32_t)queue.size();
      right[q] = (int32_t)queue.size() + 1;
      for (int s = 1; s <= 2; ++s) {
        queue.push_back(2 * queue[q] + s);
        depth.push_back(depth[q] + 1);
      }
      if (n_split) ++*n_split;
    } else {
      left[q] = right[q] = -1;
    }
    feature[q] = split ? nd.feature : 0;
    threshold[q] = split ? nd.threshold : 0.0;
    if (dleft) dleft[q] = 0;
    // (depth + 1) + c(count) - 1, in the order the scikit-learn loader adds its two per-node arrays
    leaf[q] = split ? 0.0 : ((double)(depth[q] + 1) + c[(size_t)nd.count]) - 1.0;
    if (n_node_samples) n_node_samples[base + q] = (double)nd.count;
  }
  const_cast<int64_t*>(t.tree_offsets)[tree + 1] = base + (int64_t)queue.size();
  return (int64_t)queue.size();
}

// one tree on the host from its row ids: heap (heap_nodes(D) entries) is written
void grow_heap_ref(const float* X, int32_t ld, int F, const int32_t* rows, int psi, int D, uint64_t fmask, uint64_t key,
                   uint32_t tree, std::vector<IfNode>& heap) {
  const int NH = heap_nodes(D);
  heap.assign((size_t)NH, IfNode{0.0, -1, 0});
  std::vector<int> start((size_t)NH, 0);
  std::vector<int> perm((size_t)psi), next((size_t)psi);
  std::iota(perm.begin(), perm.end(), 0);
  heap[0].count = psi;
  for (int d = 0; d <= D; ++d) {
    for (int idx = (1 << d) - 1; idx < (1 << (d + 1)) - 1; ++idx) {
      const int m = heap[idx].count, st = start[idx];
      if (m <= 1 || d == D) continue;
      uint64_t varying = 0;
      std::vector<float> mn((size_t)F), mx((size_t)F);
      for (int f = 0; f < F; ++f) {
        if (!((fmask >> f) & 1ull)) continue;
        mn[f] = __builtin_huge_valf();
        mx[f] = -__builtin_huge_valf();
        for (int i = 0; i < m; ++i) iforest_minmax(X[(int64_t)rows[perm[st + i]] * ld + f], mn[f], mx[f]);
        if (mx[f] > mn[f]) varying |= 1ull << f;
      }
      const int c = __builtin_popcountll(varying);
      if (c == 0) continue;
      const int feature = iforest_nth_bit(varying, iforest_pick(iforest_hash(key, tree, (uint32_t)idx, kIfTagFeature),
                                                                (uint32_t)c));
      const double thr = iforest_threshold(mn[feature], mx[feature],
                                           iforest_hash(key, tree, (uint32_t)idx, kIfTagThreshold));
      int nl = 0, nr = 0;
      for (int i = 0; i < m; ++i) {
        const int p = perm[st + i];
        if (iforest_goes_left(X[(int64_t)rows[p] * ld + feature], thr)) next[st + nl++] = p;
        else next[st + m - 1 - nr++] = p;
      }
      heap[idx].feature = feature;
      heap[idx].threshold = thr;
      start[2 * idx + 1] = st;
      heap[2 * idx + 1].count = nl;
      start[2 * idx + 2] = st + nl;
      heap[2 * idx + 2].count = nr;
    }
    perm.swap(next);
  }
}

// numpy.percentile's linear method on score_samples = -2^(-raw / denominator), from the two raw order statistics
// around pos = contamination (n - 1) and the weight g = pos - floor(pos)
double offset_from_order_stats(double raw_lo, double raw_hi, double g, double denominator) {
#pragma clang fp contract(off)
  const double a = -std::pow(2.0, -(raw_lo / denominator)), b = -std::pow(2.0, -(raw_hi / denominator));
  const double diff = b - a;
  return g >= 0.5 ? b - diff * (1.0 - g) : a + diff * g;
}

struct OrderStat {
  int64_t lo, hi;
  double g;
};
OrderStat order_stat(double contamination, int64_t n) {
#pragma clang fp contract(off)
  const double pos = contamination * (double)(n - 1);
  const double fl = std::floor(pos);
  OrderStat o;
  o.lo = std::min<int64_t>((int64_t)fl, n - 1);
  o.hi = std::min<int64_t>(o.lo + 1, n - 1);
  o.g = pos - fl;
  return o;
}

void fill_forest(fd_forest_params& forest, int F, int T, const std::vector<double>& c, int psi) {
#pragma clang fp contract(off)
  forest.kind = FD_FOREST_SKLEARN_IFOREST;
  forest.num_feature = F;
  forest.base_score = 0.5;
  forest.if_offset = -0.5;
  forest.if_denominator = (double)T * c[(size_t)psi];
}

void check_rows(const int32_t* rows, int32_t m, int64_t n) {
  FD_REQUIRE(rows && m >= 1 && m <= kIfMaxSamples, FD_ERR_INVALID_ARG, "iforest_fit: 1..1024 row ids");
  for (int i = 0; i < m; ++i)
    FD_REQUIRE(rows[i] >= 0 && (int64_t)rows[i] < n, FD_ERR_INVALID_ARG, "iforest_fit: a row id outside [0, n)");
}

void launch_grow(Engine& e, const float* d_X, int32_t ld, int F, const int32_t* d_rows, int psi, int D,
                 const uint64_t* d_masks, uint64_t key, uint32_t tree0, int T, IfNode* d_heaps) {
  const size_t lds = (size_t)psi * sample_stride(F) * sizeof(float);
  FD_HIP(hipMemsetAsync(d_heaps, 0, (size_t)T * heap_nodes(D) * sizeof(IfNode), e.stream));
  if (lds <= kIfSampleLds) {
    FD_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(iforest_fit_grow_kernel<true>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)kIfSampleLds));
    iforest_fit_grow_kernel<true><<<T, kIfThreads, lds, e.stream>>>(d_X, ld, F, d_rows, psi, D, d_masks, key, tree0,
                                                                    d_heaps);
  } else {
    iforest_fit_grow_kernel<false><<<T, kIfThreads, 0, e.stream>>>(d_X, ld, F, d_rows, psi, D, d_masks, key, tree0,
                                                                   d_heaps);
  }
  FD_HIP(hipGetLastError());
}

}  // namespace

// ------------------------------------------------------------------------------------------------ host API

int iforest_fit_psi(const fd_iforest_fit_params& p, int64_t n) {
  return (int)std::min<int64_t>(p.max_samples == 0 ? 256 : p.max_samples, n);
}

void iforest_fit_check(const fd_iforest_fit_params& p, int64_t n, int32_t ld, int32_t F) {
  FD_REQUIRE(n <= 2147483647ll, FD_ERR_UNSUPPORTED, "iforest_fit: more than 2^31 - 1 rows");
  FD_REQUIRE(n >= 2, FD_ERR_INVALID_ARG, "iforest_fit: n must be at least 2");
  FD_REQUIRE(F >= 1 && F <= 64 && ld >= F, FD_ERR_INVALID_ARG, "iforest_fit: F must be in 1..64 and ld >= F");
  FD_REQUIRE(p.n_estimators >= 1 && p.n_estimators <= 65536, FD_ERR_INVALID_ARG,
             "iforest_fit: n_estimators must be in 1..65536");
  FD_REQUIRE(p.max_samples == 0 || (p.max_samples >= 2 && p.max_samples <= kIfMaxSamples), FD_ERR_INVALID_ARG,
             "iforest_fit: max_samples must be 0 or in 2..1024");
  FD_REQUIRE(p.max_features > 0.0 && p.max_features <= 1.0, FD_ERR_INVALID_ARG,
             "iforest_fit: max_features must be in (0, 1]");
  FD_REQUIRE(p.contamination == 0.0 || (p.contamination > 0.0 && p.contamination <= 0.5), FD_ERR_INVALID_ARG,
             "iforest_fit: contamination must be 0 or in (0, 0.5]");
}

int64_t iforest_fit_capacity(const fd_iforest_fit_params& p, int64_t n) {
  return (int64_t)p.n_estimators * heap_nodes(iforest_depth_cap(iforest_fit_psi(p, n)));
}

void iforest_fit_check_finite(const float* X, int64_t n, int32_t ld, int32_t F) {
  for (int64_t r = 0; r < n; ++r)
    for (int f = 0; f < F; ++f)
      FD_REQUIRE(std::isfinite(X[r * ld + f]), FD_ERR_INVALID_ARG, "iforest_fit: a non-finite value in X");
}

void iforest_fit_sample_ref_host(int64_t n, const fd_iforest_fit_params& p, int32_t tree, int32_t* rows,
                                 int32_t* psi) {
  const int m = iforest_fit_psi(p, n);
  const uint64_t key = iforest_key(p.seed);
  const int b = iforest_half_bits(n);
  for (int j = 0; j < m; ++j) rows[j] = (int32_t)iforest_perm(key, (uint32_t)tree, n, b, j);
  if (psi) *psi = m;
}

void iforest_fit_grow_tree_ref_host(const float* X, int64_t n, int32_t ld, int32_t F, const int32_t* rows, int32_t m,
                                    uint64_t feature_mask, const fd_iforest_fit_params& p, int32_t tree,
                                    fd_tree_arrays& out, double* n_node_samples, int64_t* n_nodes) {
  check_out(out);
  check_rows(rows, m, n);
  feature_mask &= all_features(F);
  FD_REQUIRE(feature_mask != 0, FD_ERR_INVALID_ARG, "iforest_fit: the feature mask keeps no feature");
  const int D = iforest_depth_cap(m);
  std::vector<IfNode> heap;
  grow_heap_ref(X, ld, F, rows, m, D, feature_mask, iforest_key(p.seed), (uint32_t)tree, heap);
  const_cast<int64_t*>(out.tree_offsets)[0] = 0;
  const int64_t nn = emit_tree(heap.data(), path_length_table(m), out, n_node_samples, 0, 0, nullptr);
  if (n_nodes) *n_nodes = nn;
}

void iforest_fit_ref_host(const float* X, int64_t n, int32_t ld, int32_t F, const fd_iforest_fit_params& p,
                          fd_tree_arrays& out, double* n_node_samples, fd_forest_params& forest, int64_t* n_nodes) {
  iforest_fit_check(p, n, ld, F);
  check_out(out);
  iforest_fit_check_finite(X, n, ld, F);
  const int psi = iforest_fit_psi(p, n), D = iforest_depth_cap(psi), T = p.n_estimators;
  const uint64_t key = iforest_key(p.seed);
  const std::vector<double> c = path_length_table(psi);
  const int b = iforest_half_bits(n);
  std::vector<int32_t> rows((size_t)psi);
  std::vector<IfNode> heap;
  const_cast<int64_t*>(out.tree_offsets)[0] = 0;
  int64_t base = 0;
  for (int t = 0; t < T; ++t) {
    for (int j = 0; j < psi; ++j) rows[j] = (int32_t)iforest_perm(key, (uint32_t)t, n, b, j);
    grow_heap_ref(X, ld, F, rows.data(), psi, D, tree_feature_mask(key, (uint32_t)t, F, p.max_features), key,
                  (uint32_t)t, heap);
    base += emit_tree(heap.data(), c, out, n_node_samples, base, t, nullptr);
  }
  out.n_trees = T;
  if (n_nodes) *n_nodes = base;
  fill_forest(forest, F, T, c, psi);
  if (p.contamination == 0.0) return;
  // the fit rows' raw sums: the leaf values in tree order, f64, as the serving kernels add them
  std::vector<double> raw((size_t)n);
  for (int64_t r = 0; r < n; ++r) {
    double s = 0.0;
    for (int t = 0; t < T; ++t) {
      const int64_t o = out.tree_offsets[t];
      int32_t node = 0;
      while (out.left[o + node] != -1)
        node = iforest_goes_left(X[r * ld + out.feature[o + node]], out.threshold[o + node]) ? out.left[o + node]
                                                                                              : out.right[o + node];
      s += out.leaf_value[o + node];
    }
    raw[(size_t)r] = s;
  }
  std::sort(raw.begin(), raw.end());
  const OrderStat os = order_stat(p.contamination, n);
  forest.if_offset = offset_from_order_stats(raw[(size_t)os.lo], raw[(size_t)os.hi], os.g, forest.if_denominator);
}

// ------------------------------------------------------------------------------------------------ device API

void iforest_fit_sample_device(Engine& e, int64_t n, const fd_iforest_fit_params& p, int32_t tree, int32_t* rows,
                               int32_t* psi) {
  IForestFitScratch& s = e.iforest;
  const int m = iforest_fit_psi(p, n);
  s.rows.ensure((size_t)m * 4);
  iforest_fit_sample_kernel<<<(m + kIfThreads - 1) / kIfThreads, kIfThreads, 0, e.stream>>>(
      iforest_key(p.seed), (uint32_t)tree, 1, m, n, iforest_half_bits(n), s.rows.as<int32_t>());
  FD_HIP(hipGetLastError());
  FD_HIP(hipMemcpyAsync(rows, s.rows.ptr, (size_t)m * 4, hipMemcpyDeviceToHost, e.stream));
  FD_HIP(hipStreamSynchronize(e.stream));
  if (psi) *psi = m;
}

void iforest_fit_grow_tree_device(Engine& e, const float* d_X, int64_t n, int32_t ld, int32_t F, const int32_t* rows,
                                  int32_t m, uint64_t feature_mask, const fd_iforest_fit_params& p, int32_t tree,
                                  fd_tree_arrays& out, double* n_node_samples, int64_t* n_nodes) {
  check_out(out);
  check_rows(rows, m, n);
  feature_mask &= all_features(F);
  FD_REQUIRE(feature_mask != 0, FD_ERR_INVALID_ARG, "iforest_fit: the feature mask keeps no feature");
  IForestFitScratch& s = e.iforest;
  const int D = iforest_depth_cap(m), NH = heap_nodes(D);
  s.rows.ensure((size_t)m * 4);
  s.masks.ensure(8);
  s.heaps.ensure((size_t)NH * sizeof(IfNode));
  FD_HIP(hipMemcpyAsync(s.rows.ptr, rows, (size_t)m * 4, hipMemcpyHostToDevice, e.stream));
  FD_HIP(hipMemcpyAsync(s.masks.ptr, &feature_mask, 8, hipMemcpyHostToDevice, e.stream));
  launch_grow(e, d_X, ld, F, s.rows.as<int32_t>(), m, D, s.masks.as<uint64_t>(), iforest_key(p.seed), (uint32_t)tree, 1,
              s.heaps.as<IfNode>());
  std::vector<IfNode> heap((size_t)NH);
  FD_HIP(hipMemcpyAsync(heap.data(), s.heaps.ptr, (size_t)NH * sizeof(IfNode), hipMemcpyDeviceToHost, e.stream));
  FD_HIP(hipStreamSynchronize(e.stream));
  const_cast<int64_t*>(out.tree_offsets)[0] = 0;
  int64_t split = 0;
  const int64_t nn = emit_tree(heap.data(), path_length_table(m), out, n_node_samples, 0, 0, &split);
  ++s.trees;
  s.nodes_split += (unsigned long long)split;
  if (n_nodes) *n_nodes = nn;
}

void iforest_fit_device(Engine& e, const float* d_X, int64_t n, int32_t ld, int32_t F, const fd_iforest_fit_params& p,
                        fd_tree_arrays& out, double* n_node_samples, fd_forest_params& forest, int64_t* n_nodes) {
  iforest_fit_check(p, n, ld, F);
  check_out(out);
  IForestFitScratch& s = e.iforest;
  const int psi = iforest_fit_psi(p, n), D = iforest_depth_cap(psi), NH = heap_nodes(D), T = p.n_estimators;
  const uint64_t key = iforest_key(p.seed);
  const std::vector<double> c = path_length_table(psi);
  std::vector<uint64_t> masks((size_t)T);
  for (int t = 0; t < T; ++t) masks[t] = tree_feature_mask(key, (uint32_t)t, F, p.max_features);
  s.rows.ensure((size_t)T * psi * 4);
  s.masks.ensure((size_t)T * 8);
  s.heaps.ensure((size_t)T * NH * sizeof(IfNode));
  FD_HIP(hipMemcpyAsync(s.masks.ptr, masks.data(), (size_t)T * 8, hipMemcpyHostToDevice, e.stream));
  const int64_t ids = (int64_t)T * psi;
  iforest_fit_sample_kernel<<<(unsigned)((ids + kIfThreads - 1) / kIfThreads), kIfThreads, 0, e.stream>>>(
      key, 0u, T, psi, n, iforest_half_bits(n), s.rows.as<int32_t>());
  launch_grow(e, d_X, ld, F, s.rows.as<int32_t>(), psi, D, s.masks.as<uint64_t>(), key, 0u, T, s.heaps.as<IfNode>());
  std::vector<IfNode> heaps((size_t)T * NH);
  FD_HIP(hipMemcpyAsync(heaps.data(), s.heaps.ptr, heaps.size() * sizeof(IfNode), hipMemcpyDeviceToHost, e.stream));
  FD_HIP(hipStreamSynchronize(e.stream));  // (masks is read by the copy above until here)
  const_cast<int64_t*>(out.tree_offsets)[0] = 0;
  int64_t base = 0, split = 0;
  for (int t = 0; t < T; ++t) base += emit_tree(heaps.data() + (size_t)t * NH, c, out, n_node_samples, base, t, &split);
  out.n_trees = T;
  s.trees += (unsigned long long)T;
  s.nodes_split += (unsigned long long)split;
  if (n_nodes) *n_nodes = base;
  fill_forest(forest, F, T, c, psi);
  if (p.contamination == 0.0) return;

  // the offset: score the fit rows with the grown forest through the serving kernels, sort the raw sums, read two
  PackedForest& pf = s.scorer;
  pf.loaded = false;
  shap_forget(pf);
  repack_forest(pf, forest, out);
  s.raw.ensure((size_t)n * 8);
  s.prob.ensure((size_t)n * 8);
  s.sorted.ensure((size_t)n * 8);
  launch_forest(e, pf, d_X, n, ld, s.prob.as<double>(), s.raw.as<double>(), nullptr);
  size_t tb = 0;
  FD_HIP(rocprim::radix_sort_keys(nullptr, tb, s.raw.as<double>(), s.sorted.as<double>(), (size_t)n, 0, 64, e.stream));
  s.sort_tmp.ensure(std::max<size_t>(tb, 16));
  FD_HIP(rocprim::radix_sort_keys(s.sort_tmp.ptr, tb, s.raw.as<double>(), s.sorted.as<double>(), (size_t)n, 0, 64,
                                  e.stream));
  const OrderStat os = order_stat(p.contamination, n);
  double stat[2];
  FD_HIP(hipMemcpyAsync(&stat[0], s.sorted.as<double>() + os.lo, 8, hipMemcpyDeviceToHost, e.stream));
  FD_HIP(hipMemcpyAsync(&stat[1], s.sorted.as<double>() + os.hi, 8, hipMemcpyDeviceToHost, e.stream));
  FD_HIP(hipStreamSynchronize(e.stream));
  forest.if_offset = offset_from_order_stats(stat[0], stat[1], os.g, forest.if_denominator);
  // the scorer's host copy of the trees has served; its device buffers stay for the next fit
  pf.loaded = false;
  for (auto* v : {&pf.t_left, &pf.t_right, &pf.t_feature}) std::vector<int32_t>().swap(*v);
  for (auto* v : {&pf.t_threshold, &pf.t_leaf}) std::vector<double>().swap(*v);
}

}  // namespace fd
