// forest_sparse.hip — the sparse (pointer) forest layout and its kernel: trees of ANY depth, unpadded.
//
// The heap layouts of forest.hip pad every tree to a perfect depth-D tree (D <= 10). scikit-learn's forest
// classifiers grow until the leaves are pure (depth 20-46 on the bench's 3,000-row sets), an IsolationForest with
// max_samples > 1024 or an XGBoost model with max_depth > 10 exceed D too: their 2^D heaps do not exist. Here a tree
// keeps its shape.
//
// Layout (pack_forest_sparse_host; include/fdengine.h fd_pack_forest_sparse_host documents the same words):
//   nodes      n_nodes records {f32 t, u32 meta}, go left <=> x < t. Records 0 .. T-1 are the T roots (a tree's
//              root index IS its tree index: no root table), then each tree's other nodes breadth-first, a node's two
//              children adjacent (one child index serves both).
//              internal: meta = left child's record index (24 bits, forest-global) | feature << 24 | default_left << 30
//              leaf:     meta = 1 << 31 | leaf ordinal (forest-global: tree by tree, a tree's root first, then
//                        its other records in order)
//   leaf_val   [n_leaves] f32 (XGBoost) / f64 (IsolationForest, predict_proba), by ordinal
//   leaf_ids   [n_leaves] original node ids, by ordinal
//
// forest_sparse_kernel: 1024 threads on a tile of 256 transactions, the feature tile in LDS as [f][256] f32 like
// the other forest kernels (any feature read of a wave hits 64 consecutive words: conflict-free). Wave w walks, for
// the 64 transactions of txn group w & 3, kSpK trees of tree group w >> 2 per round; a round is 4 x kSpK = 16 trees.
// Nodes are read from global memory (8-byte loads; a 100-tree forest is a few MB: L2-resident); the kSpK walks of
// a lane are interleaved so their dependent loads overlap, and 16 waves per CU hide the rest. A tree ends where
// its leaf is, so the walk loop runs until no lane of the WAVE is on an internal node — not to a fixed depth (the
// deepest path of such a forest is about three times its mean path). Leaf values go to LDS and the round's owner
// tree group adds them per transaction in tree order, seeded by the XGBoost base margin: the f32 margin, the f64
// path-length sum and the f64 probability sum are the reference's sequential sums, bit for bit, as for the heap
// kernels.
//
// Not here (follow-ups; tools/forest_sparse_bench.py is the measurement to start from): the top levels of each tree
// staged in LDS, and a tree-split variant for latency batches (a 1 k batch is 4 tiles = 4 CUs).
#include <algorithm>
#include <cmath>
#include <cstring>

#include "fd_internal.h"
#include "walk_common.h"

namespace fd {

// ------------------------------------------------------------------------------------------------
// host-side repack

namespace {

constexpr uint32_t kSpLeaf = 1u << 31;
constexpr uint32_t kSpDefaultLeft = 1u << 30;
constexpr int kSpFeatureShift = 24;
constexpr uint32_t kSpChildMask = (1u << kSpFeatureShift) - 1u;
static_assert((int64_t)kSpChildMask + 1 == kSparseMaxNodes, "the child field indexes kSparseMaxNodes records");
static_assert(kMaxFeatures <= 64, "the feature field is 6 bits");

bool arrays_complete(const fd_tree_arrays& t) {
  return t.n_trees > 0 && t.tree_offsets && t.left && t.right && t.feature && t.threshold && t.leaf_value;
}

}  // namespace

int forest_depth_probe(const fd_tree_arrays& t) {
  if (!arrays_complete(t)) return -1;
  int maxd = 0;
  std::vector<std::pair<int32_t, int>> st;
  for (int i = 0; i < t.n_trees; ++i) {
    const int64_t a = t.tree_offsets[i], m = t.tree_offsets[i + 1] - a;
    if (m <= 0) return -1;
    const int32_t* L = t.left + a;
    const int32_t* R = t.right + a;
    int64_t visited = 0;
    st.assign(1, {0, 0});
    while (!st.empty()) {
      const auto [o, d] = st.back();
      st.pop_back();
      if (o < 0 || o >= m || ++visited > m) return -1;
      if (L[o] < 0) {
        maxd = std::max(maxd, d);
      } else {
        st.push_back({L[o], d + 1});
        st.push_back({R[o], d + 1});
      }
    }
  }
  return maxd;
}

SparsePack pack_forest_sparse_host(const fd_forest_params& p, const fd_tree_arrays& t) {
  FD_REQUIRE(p.kind == FD_FOREST_XGB_BINARY_LOGISTIC || p.kind == FD_FOREST_SKLEARN_IFOREST ||
                 p.kind == FD_FOREST_SKLEARN_PROBA,
             FD_ERR_INVALID_ARG, "unknown forest kind");
  FD_REQUIRE(arrays_complete(t), FD_ERR_INVALID_ARG, "incomplete tree arrays");
  FD_REQUIRE(p.num_feature > 0 && p.num_feature <= kMaxFeatures, FD_ERR_UNSUPPORTED,
             "num_feature must be in [1, 64] (the sparse layout's 6-bit feature field and the LDS feature tile)");
  const bool xgb = p.kind == FD_FOREST_XGB_BINARY_LOGISTIC;
  const int T = t.n_trees, nf = p.num_feature;
  const char* too_many = "the sparse layout indexes at most 2^24 nodes per forest (24-bit child field)";
  FD_REQUIRE(t.tree_offsets[T] <= kSparseMaxNodes, FD_ERR_UNSUPPORTED, too_many);

  SparsePack sp;
  sp.kind = p.kind;
  sp.n_trees = T;
  sp.num_feature = nf;
  sp.leaf_bytes = xgb ? 4 : 8;
  sp.nodes.assign((size_t)2 * T, 0u);  // the roots, then each tree's other nodes as the walk below appends them
  // record r of the image holds original node src[r] of its tree, at depth dep[r]
  std::vector<int32_t> src((size_t)T), dep((size_t)T, 0);
  for (int i = 0; i < T; ++i) {
    FD_REQUIRE(t.tree_offsets[i + 1] > t.tree_offsets[i], FD_ERR_INVALID_ARG, "empty tree");
    src[i] = 0;
  }
  auto emit = [&](int64_t a, int64_t r) {  // fill record r from its original node; a = the tree's offset
    const int32_t o = src[r];
    if (t.left[a + o] < 0) {
      const int64_t ord = sp.n_leaves++;
      sp.nodes[2 * r] = 0u;
      sp.nodes[2 * r + 1] = kSpLeaf | (uint32_t)ord;
      sp.leaf_ids.push_back(o);
      if (xgb) {
        const float v = (float)t.leaf_value[a + o];
        sp.leaf_val.insert(sp.leaf_val.end(), reinterpret_cast<const char*>(&v), reinterpret_cast<const char*>(&v) + 4);
      } else {
        const double v = t.leaf_value[a + o];
        sp.leaf_val.insert(sp.leaf_val.end(), reinterpret_cast<const char*>(&v), reinterpret_cast<const char*>(&v) + 8);
      }
      sp.depth = std::max(sp.depth, dep[r]);
      return;
    }
    const int32_t f = t.feature[a + o];
    FD_REQUIRE(f >= 0 && f < nf, FD_ERR_INVALID_ARG, "split feature outside [0, num_feature)");
    const float thr = xgb ? (float)t.threshold[a + o] : sklearn_threshold_to_lt(t.threshold[a + o]);
    uint32_t tb;
    std::memcpy(&tb, &thr, 4);
    const int64_t child = (int64_t)src.size();  // the two children: the next two records
    FD_REQUIRE(child + 2 <= kSparseMaxNodes, FD_ERR_UNSUPPORTED, too_many);
    const uint32_t dl = (t.default_left && t.default_left[a + o]) ? kSpDefaultLeft : 0u;
    sp.nodes[2 * r] = tb;
    sp.nodes[2 * r + 1] = (uint32_t)child | (uint32_t)f << kSpFeatureShift | dl;
    src.push_back(t.left[a + o]);
    src.push_back(t.right[a + o]);
    dep.push_back(dep[r] + 1);
    dep.push_back(dep[r] + 1);
    sp.nodes.resize(sp.nodes.size() + 4, 0u);
  };
  // leaf ordinals follow record order within a tree, trees in order: the roots' records are emitted with their tree
  for (int i = 0; i < T; ++i) {
    const int64_t a = t.tree_offsets[i], m = t.tree_offsets[i + 1] - a;
    int64_t visited = 0;
    const int64_t first = (int64_t)src.size();
    // breadth-first: the root, then the records this tree appends (src grows while the loop runs)
    for (int64_t r = i; r < (int64_t)src.size(); r = (r == i ? first : r + 1)) {
      const int32_t o = src[r];
      FD_REQUIRE(o >= 0 && o < m, FD_ERR_INVALID_ARG, "tree child index out of range");
      FD_REQUIRE(++visited <= m, FD_ERR_INVALID_ARG, "tree is not a tree (node visited twice)");
      emit(a, r);
    }
  }
  sp.n_nodes = (int64_t)src.size();
  if (xgb) {  // as pack_forest_host: RegLossObj::ProbToMargin in f32
    const float bs = (float)p.base_score;
    sp.base_margin = -logf(1.0f / bs - 1.0f);
  }
  return sp;
}

namespace {

void upload_sparse(SparseImage& im, const SparsePack& sp, uint64_t gen) {
  auto up = [](DeviceBuffer& d, const void* h, size_t bytes) {
    d.ensure(std::max<size_t>(bytes, 8));
    if (bytes) FD_HIP(hipMemcpy(d.ptr, h, bytes, hipMemcpyHostToDevice));
  };
  up(im.nodes, sp.nodes.data(), sp.nodes.size() * sizeof(uint32_t));
  up(im.leaf_val, sp.leaf_val.data(), sp.leaf_val.size());
  up(im.leaf_ids, sp.leaf_ids.data(), sp.leaf_ids.size() * sizeof(int32_t));
  im.n_nodes = sp.n_nodes;
  im.n_leaves = sp.n_leaves;
  im.gen = gen;
}

}  // namespace

void load_forest_sparse(PackedForest& pf, const fd_forest_params& p, const fd_tree_arrays& t) {
  const SparsePack sp = pack_forest_sparse_host(p, t);
  forest_loaded(pf, p, t);
  upload_sparse(pf.sp, sp, pf.gen);
  pf.sparse_only = true;
  pf.kind = sp.kind;
  pf.n_trees = sp.n_trees;
  pf.depth = sp.depth;
  pf.num_feature = sp.num_feature;
  pf.base_margin = sp.base_margin;
  pf.if_offset = p.if_offset;
  pf.if_denominator = p.kind == FD_FOREST_SKLEARN_PROBA ? (double)sp.n_trees : p.if_denominator;
  // no heap, no binned layout: the paths that read them test these
  pf.binned = false;
  pf.chunk = pf.n_chunks = pf.b_chunk = pf.b_n_chunks = pf.n_chunk = pf.n_n_chunks = pf.bin_steps = pf.b_n_thr = 0;
  pf.tree_bytes = pf.chunk_stride = pf.b_tree_bytes = pf.b_chunk_stride = pf.n_chunk_stride = 0;
  pf.loaded = true;
}

// ------------------------------------------------------------------------------------------------
// device side

namespace {

constexpr int kSpWG = 1024;
constexpr int kSpK = 4;               // trees one lane walks interleaved
constexpr int kSpRound = 4 * kSpK;    // trees per round: 4 tree groups x kSpK

// LDS: Xs[nf][256] f32 | lv[2][kSpRound][256] LeafT | acc[256] LeafT | 16 wave flags
size_t lds_bytes_sparse(int nf, size_t leaf_sz) {
  return (size_t)nf * kTile * 4 + 2 * (size_t)kSpRound * kTile * leaf_sz + kTile * leaf_sz + 64;
}

// The kSpK trees t0 .. t0 + kSpK - 1 (those below n_trees) for this lane's transaction: ord[j] = the leaf ordinal
// reached (0 for a walk that does not exist: a row past n, a tree past n_trees — it starts on a leaf word). Every
// iteration steps each walk that is on an internal node. The step is branch-free: a walk that is done reads feature 0
// and record 0 (both always exist; the done lanes of a wave share the one line) and keeps its words by a select, so
// the iteration issues its kSpK LDS reads together and then its kSpK node loads together, and waits for each only
// where the next iteration uses it. (With the step inside `if (internal)` the compiler ends every divergent block on
// s_waitcnt vmcnt(0): the lane's walks ran one after the other.) The loop ends when no lane of the wave stepped.
template <bool NAN_AWARE>
__device__ __forceinline__ void walk_sparse(const uint2* __restrict__ nodes, int t0, int n_trees, bool active,
                                            const float* xlane, uint32_t (&ord)[kSpK]) {
  uint32_t thr[kSpK], meta[kSpK];
  uint2 nd[kSpK];
#pragma unroll
  for (int j = 0; j < kSpK; ++j) {
    const bool on = active && t0 + j < n_trees;
    nd[j] = nodes[on ? t0 + j : 0];  // the root of tree t is record t
    thr[j] = nd[j].x;
    meta[j] = on ? nd[j].y : kSpLeaf;
  }
  for (;;) {
    bool stepped = false;
    float x[kSpK];
#pragma unroll
    for (int j = 0; j < kSpK; ++j) x[j] = xlane[((meta[j] >> kSpFeatureShift) & 63u) * kTile];  // a leaf word: feature 0
    uint32_t next[kSpK];
#pragma unroll
    for (int j = 0; j < kSpK; ++j) {
      const bool internal = (int32_t)meta[j] >= 0;
      bool right = !(x[j] < __uint_as_float(thr[j]));
      if (NAN_AWARE) {
        if (x[j] != x[j]) right = (meta[j] & kSpDefaultLeft) == 0u;  // missing: default direction
      }
      next[j] = internal ? (meta[j] & kSpChildMask) + (right ? 1u : 0u) : 0u;
      stepped |= internal;
    }
#pragma unroll
    for (int j = 0; j < kSpK; ++j) nd[j] = nodes[next[j]];
#pragma unroll
    for (int j = 0; j < kSpK; ++j) {
      const bool internal = (int32_t)meta[j] >= 0;
      thr[j] = internal ? nd[j].x : thr[j];
      meta[j] = internal ? nd[j].y : meta[j];
    }
    if (__ballot(stepped) == 0ull) break;  // wave-uniform
  }
#pragma unroll
  for (int j = 0; j < kSpK; ++j) ord[j] = meta[j] & ~kSpLeaf;
}

template <typename LeafT, int KIND>
__global__ void __launch_bounds__(kSpWG)
forest_sparse_kernel(const float* __restrict__ X, int64_t n, int ld, int nf, const uint2* __restrict__ nodes,
                     const LeafT* __restrict__ leaf_val, const int32_t* __restrict__ leaf_ids, int n_trees,
                     float base_margin, double if_offset, double if_denom, double* __restrict__ out_prob,
                     double* __restrict__ out_raw, int32_t* __restrict__ out_leaf) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* Xs = reinterpret_cast<float*>(smem);                              // [nf][kTile]
  LeafT* lv = reinterpret_cast<LeafT*>(smem + (size_t)nf * kTile * 4);      // [2][kSpRound][kTile]
  LeafT* accL = lv + 2 * kSpRound * kTile;                                 // [kTile]
  uint32_t* flags = reinterpret_cast<uint32_t*>(accL + kTile);             // [16]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int gg = wave >> 2;                  // tree group
  const int txn = ((wave & 3) << 6) + lane;  // 0..255 within the tile
  const int64_t row = (int64_t)blockIdx.x * kTile + txn;
  const bool valid = row < n;

  // the tile: the four threads sharing `txn` take every 4th column (as the threshold-layout tile kernel does)
  int anynan = 0;
  const int ncopy = ld < nf ? ld : nf;
  if (valid) {
    const float* xr = X + row * (int64_t)ld;
    for (int f = gg; f < ncopy; f += 4) {
      const float v = xr[f];
      Xs[f * kTile + txn] = v;
      anynan |= (v != v);
    }
    for (int f = ncopy + gg; f < nf; f += 4) Xs[f * kTile + txn] = __builtin_nanf("");  // DMatrix: missing
    anynan |= (ncopy < nf);
  } else {
    for (int f = gg; f < nf; f += 4) Xs[f * kTile + txn] = 0.f;
  }
  if (gg == 0) accL[txn] = (KIND == FD_FOREST_XGB_BINARY_LOGISTIC) ? (LeafT)base_margin : (LeafT)0;
  const bool tile_nan = tile_any(anynan, flags, kSpWG / 64);

  const float* xlane = Xs + txn;
  const int rounds = (n_trees + kSpRound - 1) / kSpRound;
  for (int k = 0; k < rounds; ++k) {
    if (k > 0 && gg == ((k - 1) & 3)) {  // owner of round k-1 adds its leaf values in tree order
      const LeafT* b = lv + ((k - 1) & 1) * kSpRound * kTile;
      LeafT acc = accL[txn];
#pragma unroll
      for (int c = 0; c < kSpRound; ++c) acc += b[c * kTile + txn];  // a round before the last is full
      accL[txn] = acc;
    }
    const int t0 = k * kSpRound + gg * kSpK;
    uint32_t ord[kSpK];
    if (tile_nan)
      walk_sparse<true>(nodes, t0, n_trees, valid, xlane, ord);
    else
      walk_sparse<false>(nodes, t0, n_trees, valid, xlane, ord);
    LeafT lval[kSpK];  // (a walk that does not exist reached ordinal 0: the loads below need no guard)
#pragma unroll
    for (int j = 0; j < kSpK; ++j) lval[j] = leaf_val[ord[j]];
    LeafT* b = lv + (k & 1) * kSpRound * kTile;
#pragma unroll
    for (int j = 0; j < kSpK; ++j) b[(gg * kSpK + j) * kTile + txn] = (valid && t0 + j < n_trees) ? lval[j] : (LeafT)0;
    if (out_leaf != nullptr) {
      int32_t lid[kSpK];
#pragma unroll
      for (int j = 0; j < kSpK; ++j) lid[j] = leaf_ids[ord[j]];
#pragma unroll
      for (int j = 0; j < kSpK; ++j)
        if (valid && t0 + j < n_trees) out_leaf[row * n_trees + t0 + j] = lid[j];
    }
    __syncthreads();  // lv[k & 1] complete; the owner of round k-1 is done with lv[(k-1) & 1]
  }
  const int last = rounds - 1;
  if (gg != (last & 3)) return;
  LeafT acc = accL[txn];
  const LeafT* b = lv + (last & 1) * kSpRound * kTile;
  const int cnt = n_trees - last * kSpRound;  // only the trees that exist: no padding term enters the sum
  for (int c = 0; c < cnt; ++c) acc += b[c * kTile + txn];
  if (valid) write_outputs<KIND, LeafT>(acc, row, if_offset, if_denom, out_prob, out_raw);
}

template <typename LeafT, int KIND>
void launch_sparse_kind(Engine& e, const PackedForest& pf, const float* d_X, int64_t n, int32_t ld, double* d_prob,
                        double* d_raw, int32_t* d_leaf, hipStream_t st) {
  auto* fn = forest_sparse_kernel<LeafT, KIND>;
  const size_t lds = lds_bytes_sparse(pf.num_feature, sizeof(LeafT));
  FD_REQUIRE(lds <= kLdsBudget, FD_ERR_UNSUPPORTED, "sparse forest kernel exceeds the LDS budget");
  FD_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  const int64_t blocks = (n + kTile - 1) / kTile;
  Engine::Timed* ev =
      e.timing ? e.next_event_pair(KIND == FD_FOREST_XGB_BINARY_LOGISTIC ? FD_TIMING_XGB : FD_TIMING_IFOREST) : nullptr;
  if (ev) FD_HIP(hipEventRecord(ev->a, st));
  hipLaunchKernelGGL(fn, dim3((unsigned)blocks), dim3(kSpWG), lds, st, d_X, n, (int)ld, pf.num_feature,
                     pf.sp.nodes.as<const uint2>(), pf.sp.leaf_val.as<const LeafT>(), pf.sp.leaf_ids.as<const int32_t>(),
                     pf.n_trees, pf.base_margin, pf.if_offset, pf.if_denominator, d_prob, d_raw, d_leaf);
  FD_HIP(hipGetLastError());
  if (ev) FD_HIP(hipEventRecord(ev->b, st));
  ++e.sparse_total;
}

}  // namespace

void launch_forest_sparse(Engine& e, const PackedForest& pf, const float* d_X, int64_t n, int32_t ld, double* d_prob,
                          double* d_raw, int32_t* d_leaf, hipStream_t st) {
  if (pf.sp.gen != pf.gen || pf.gen == 0) {
    // a forest with the heap layouts under option 11: its sparse image from the trees as loaded (forest_loaded's copy)
    FD_REQUIRE(!pf.sparse_only && !pf.t_off.empty(), FD_ERR_NOT_LOADED, "forest has no sparse image");
    fd_tree_arrays t{};
    t.n_trees = pf.n_trees;
    t.tree_offsets = pf.t_off.data();
    t.left = pf.t_left.data();
    t.right = pf.t_right.data();
    t.feature = pf.t_feature.data();
    t.threshold = pf.t_threshold.data();
    t.default_left = pf.t_dleft.data();
    t.leaf_value = pf.t_leaf.data();
    upload_sparse(pf.sp, pack_forest_sparse_host(pf.params, t), pf.gen);
  }
  switch (pf.kind) {
    case FD_FOREST_XGB_BINARY_LOGISTIC:
      launch_sparse_kind<float, FD_FOREST_XGB_BINARY_LOGISTIC>(e, pf, d_X, n, ld, d_prob, d_raw, d_leaf, st);
      break;
    case FD_FOREST_SKLEARN_IFOREST:
      launch_sparse_kind<double, FD_FOREST_SKLEARN_IFOREST>(e, pf, d_X, n, ld, d_prob, d_raw, d_leaf, st);
      break;
    case FD_FOREST_SKLEARN_PROBA:
      launch_sparse_kind<double, FD_FOREST_SKLEARN_PROBA>(e, pf, d_X, n, ld, d_prob, d_raw, d_leaf, st);
      break;
    default:
      FD_REQUIRE(false, FD_ERR_INVALID_ARG, "unknown forest kind");
  }
}

}  // namespace fd
