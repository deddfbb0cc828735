// ensemble_plan.hip — the host planner of the fused ensemble kernel (ensemble.hip), run when a model is loaded or a
// plan is first needed: the host copy of a loaded forest (forest_loaded), its contraction against the compact vector's
// constant slots (contract_forest_host), and the joint plan of a pair of forests (build_plan) — merged per-feature
// threshold tables, the full chunks, the contracted chunks (padded 1 KiB blocks, or the dense chunk stream of
// dense_layout_host), the constant slots' bins and the binning passes. Host code only; ensemble_layout.h holds what it
// shares with the kernel.
#include <algorithm>
#include <atomic>
#include <cstring>

#include "ensemble_layout.h"

namespace fd {

static std::atomic<uint64_t> g_forest_gen{0};

void forest_loaded(PackedForest& pf, const fd_forest_params& p, const fd_tree_arrays& t) {
  pf.gen = ++g_forest_gen;
  pf.params = p;
  const int64_t m = t.tree_offsets[t.n_trees];
  pf.t_off.assign(t.tree_offsets, t.tree_offsets + t.n_trees + 1);
  pf.t_left.assign(t.left, t.left + m);
  pf.t_right.assign(t.right, t.right + m);
  pf.t_feature.assign(t.feature, t.feature + m);
  pf.t_threshold.assign(t.threshold, t.threshold + m);
  pf.t_leaf.assign(t.leaf_value, t.leaf_value + m);
  if (t.default_left)
    pf.t_dleft.assign(t.default_left, t.default_left + m);
  else
    pf.t_dleft.assign((size_t)m, 0);
}

// Every split on a constant slot of the compact scoring vector decided here, once: the pipelined stream's rows
// carry 0.5 in slots 12, 24, 25, 33, 34 and 0 in the other 37 that are not among the 22 varying ones (compact_src),
// so such a node sends every transaction the same way — left iff value < threshold in f32, pack_forest_host's
// comparison (the constants are never NaN: default_left plays no part) — and it is replaced by that child. Nodes are
// renumbered in pre-order; leaf values and the tree order are untouched. A tree that resolves to one leaf becomes a
// root over two leaves of that value (slot 0 against 0, never looked at); a tree that was a lone leaf stays one.
ContractedForest contract_forest_host(const fd_forest_params& p, const fd_tree_arrays& t) {
  FD_REQUIRE(p.kind == FD_FOREST_XGB_BINARY_LOGISTIC || p.kind == FD_FOREST_SKLEARN_IFOREST, FD_ERR_INVALID_ARG,
             "contraction: XGBoost binary:logistic or IsolationForest trees");
  FD_REQUIRE(p.num_feature > 0 && p.num_feature <= kMaxFeatures, FD_ERR_UNSUPPORTED, "num_feature must be in [1, 64]");
  FD_REQUIRE(forest_depth_probe(t) >= 0, FD_ERR_INVALID_ARG, "incomplete tree arrays or a tree that is not a tree");
  const bool xgb = p.kind == FD_FOREST_XGB_BINARY_LOGISTIC;
  ContractedForest c;
  c.off.push_back(0);
  struct Item {
    int32_t o, lo, ro;  // node, its children after resolution (original ids)
    int depth;
  };
  std::vector<Item> st, keep;
  std::vector<int32_t> remap;
  for (int i = 0; i < t.n_trees; ++i) {
    const int64_t a = t.tree_offsets[i], m = t.tree_offsets[i + 1] - a;
    const int32_t *L = t.left + a, *R = t.right + a, *F = t.feature + a;
    auto resolve = [&](int32_t o) {  // down through the constant splits
      while (L[o] >= 0) {
        FD_REQUIRE(F[o] >= 0 && F[o] < p.num_feature, FD_ERR_INVALID_ARG, "split feature outside [0, num_feature)");
        const int src = compact_src(F[o]);
        if (src >= 0) break;
        const float val = src == -2 ? 0.5f : 0.0f;
        const float thr = xgb ? (float)t.threshold[a + o] : sklearn_threshold_to_lt(t.threshold[a + o]);
        o = val < thr ? L[o] : R[o];
      }
      return o;
    };
    const int64_t base = (int64_t)c.left.size();
    auto emit = [&](int32_t l, int32_t r, int32_t f, double thr, uint8_t dl, double leaf) {
      c.left.push_back(l);
      c.right.push_back(r);
      c.feature.push_back(f);
      c.threshold.push_back(thr);
      c.dleft.push_back(dl);
      c.leaf.push_back(leaf);
      return (int32_t)((int64_t)c.left.size() - 1 - base);
    };
    int64_t splits_in = 0, splits_out = 0;
    for (int64_t o = 0; o < m; ++o) splits_in += L[o] >= 0 ? 1 : 0;
    int depth = 0;
    const int32_t root = resolve(0);
    if (L[root] < 0 && L[0] >= 0) {  // resolved entirely
      emit(1, 2, 0, 0.0, 0, 0.0);
      emit(-1, -1, 0, 0.0, 0, t.leaf_value[a + root]);
      emit(-1, -1, 0, 0.0, 0, t.leaf_value[a + root]);
      depth = 1;
    } else {
      // the surviving nodes keep their relative order (the root first), so a tree with nothing to resolve comes back
      // as it went in
      st.clear();
      st.push_back({root, 0, 0});
      keep.clear();
      while (!st.empty()) {
        Item it = st.back();
        st.pop_back();
        depth = std::max(depth, it.depth);
        if (L[it.o] >= 0) {
          it.lo = resolve(L[it.o]);
          it.ro = resolve(R[it.o]);
          st.push_back({it.ro, 0, 0, it.depth + 1});
          st.push_back({it.lo, 0, 0, it.depth + 1});
        }
        keep.push_back(it);
      }
      std::sort(keep.begin() + 1, keep.end(), [](const Item& x, const Item& y) { return x.o < y.o; });
      remap.assign((size_t)m, -1);
      for (size_t k = 0; k < keep.size(); ++k) remap[(size_t)keep[k].o] = (int32_t)k;
      for (const Item& it : keep) {
        const int32_t o = it.o;
        if (L[o] < 0) {
          emit(-1, -1, F[o], t.threshold[a + o], t.default_left ? t.default_left[a + o] : 0, t.leaf_value[a + o]);
        } else {
          ++splits_out;
          emit(remap[(size_t)it.lo], remap[(size_t)it.ro], F[o], t.threshold[a + o],
               t.default_left ? t.default_left[a + o] : 0, t.leaf_value[a + o]);
        }
      }
    }
    c.pruned += splits_in - splits_out;
    c.depth.push_back(std::max(depth, 1));
    c.off.push_back((int64_t)c.left.size());
  }
  return c;
}

namespace {

using Tables = std::vector<std::vector<float>>;  // [feature]: its ascending distinct thresholds (f32)

fd_tree_arrays arrays_of(const PackedForest& f) {
  fd_tree_arrays t{};
  t.n_trees = f.n_trees;
  t.tree_offsets = f.t_off.data();
  t.left = f.t_left.data();
  t.right = f.t_right.data();
  t.feature = f.t_feature.data();
  t.threshold = f.t_threshold.data();
  t.default_left = f.t_dleft.data();
  t.leaf_value = f.t_leaf.data();
  return t;
}

// Tree i of a contracted forest as a perfect heap of depth dw (at least its own): node words at dst[1 .. 2^dw), a leaf
// above depth dw a pad node that both ways leave for the same leaf, every threshold as its index in its feature's
// table; then the 2^dw leaf values at `leaves`, f32 (xgb) or f64. slot_of(feature): the bin tile's index of the value
// a node tests, the node word's slot.
template <class SlotOf>
void expand_heap(const ContractedForest& c, int i, bool xgb, const Tables& tables, int dw, uint32_t* dst, char* leaves,
                 SlotOf slot_of) {
  const int nl = 1 << dw;
  const int64_t a = c.off[i];
  int32_t cur[2 * 256];  // the contracted node at each heap slot
  cur[1] = 0;
  for (int s = 1; s < nl; ++s) {
    const int32_t o = cur[s];
    const uint32_t link = ens_link(s, nl);
    if (c.left[a + o] < 0) {
      dst[s] = ens_node_word(0, 0, link, false);
      cur[2 * s] = cur[2 * s + 1] = o;
      continue;
    }
    const int f = c.feature[a + o];
    const uint32_t slot = slot_of(f);
    const float thr = xgb ? (float)c.threshold[a + o] : sklearn_threshold_to_lt(c.threshold[a + o]);
    const std::vector<float>& tb = tables[(size_t)f];
    const uint32_t jm = (uint32_t)(std::lower_bound(tb.begin(), tb.end(), thr) - tb.begin());
    // (the root of a tree that resolved to one leaf tests slot 0 against 0, which no table need hold: both ways
    // reach the same value; a plan's merged tables hold at most kMaxBins thresholds, the host export's any number)
    FD_REQUIRE(jm <= 0xFFFFu, FD_ERR_UNSUPPORTED, "ensemble layout: threshold index beyond 16 bits");
    dst[s] = ens_node_word(jm, slot, link, c.dleft[a + o] != 0);
    cur[2 * s] = c.left[a + o];
    cur[2 * s + 1] = c.right[a + o];
  }
  for (int s = 0; s < nl; ++s) {
    const double v = c.leaf[a + cur[nl + s]];
    if (xgb) {
      const float vf = (float)v;
      std::memcpy(leaves + (size_t)s * 4, &vf, 4);
    } else {
      std::memcpy(leaves + (size_t)s * 8, &v, 8);
    }
  }
}

// Binning passes over the tables (thr, off): consecutive features whose padded tables fit the staging area (bufA +
// bufB + the tiles), a larger table alone, searched in global memory; each staged pass's image (element g of the
// pass at word thr_pad(g), 1 KiB pieces) appended to img. The staging area is sized by the padded layout for the dense
// kernel too: a plan's passes serve both (64-wide rows keep the padded kernels), and the dense kernel's area behind its
// 11 KiB tile is the larger (133,120 B against 114,688 B wide), so a pass that fits here fits there.
void plan_passes(const std::vector<float>& thr, const std::vector<int32_t>& off, int nf, bool wide, EnsPassSet& ps,
                 std::vector<float>& img) {
  const size_t stage_floats = (2 * (size_t)ens_buf(wide) + 2 * (size_t)kEnsTile) / 4;
  ps = EnsPassSet{};
  ps.f.push_back(0);
  ps.img_off.push_back((int)(img.size() * 4));
  int f = 0;
  while (f < nf) {
    int g = f;
    while (g < nf && (size_t)(off[g + 1] - off[f]) + (size_t)(off[g + 1] - off[f]) / 32 + 1 <= stage_floats) ++g;
    const int np = (int)ps.f.size() - 1;
    FD_REQUIRE(np < kMaxPass, FD_ERR_UNSUPPORTED, "ensemble binning plan too long");
    if (g == f) {  // one feature's table exceeds the LDS space
      ps.glob |= 1ull << np;
      g = f + 1;
    } else {
      const int cnt = off[g] - off[f];
      const size_t words = cnt > 0 ? (size_t)thr_pad(cnt - 1) + 1 : 0;
      const size_t base = img.size();
      img.resize(base + (words + 255) / 256 * 256, 0.f);
      for (int i = 0; i < cnt; ++i) img[base + (size_t)thr_pad(i)] = thr[(size_t)off[f] + i];
    }
    ps.f.push_back(g);
    ps.img_off.push_back((int)(img.size() * 4));
    f = g;
  }
}

// build_plan step 1 — the merged per-feature tables: the distinct thresholds of the forests present; false when a
// feature has more than the binned layout holds
bool merge_tables(const HostPack* const (&hp)[2], int nf, Tables& merged) {
  merged.assign((size_t)nf, {});
  for (int f = 0; f < nf; ++f) {
    for (const HostPack* h : hp) {
      if (!h) continue;
      merged[f].insert(merged[f].end(), h->b_thr.begin() + h->b_thr_off[f], h->b_thr.begin() + h->b_thr_off[f + 1]);
    }
    std::sort(merged[f].begin(), merged[f].end());
    merged[f].erase(std::unique(merged[f].begin(), merged[f].end()), merged[f].end());
    if (merged[f].size() > (size_t)kMaxBins) return false;
  }
  return true;
}

// build_plan step 2 — a forest's full chunks: ch node blocks of 1 KiB (walk_ens link addressing), then the ch trees'
// leaf values [ch][NL] of lsz bytes; padding trees (a partial last chunk) keep zero nodes and zero leaves. The node
// words are the binned layout's (pack_forest_host), their thresholds re-indexed in the merged tables.
std::vector<char> pack_full_chunks(const HostPack& h, const Tables& merged, int ch, int NL, size_t lsz, size_t stride) {
  const int T = h.n_trees, nc = (T + ch - 1) / ch;
  std::vector<char> blob((size_t)nc * stride, 0);
  for (int i = 0; i < T; ++i) {
    const char* src = h.b_blob.data() + (size_t)(i / h.b_chunk) * h.b_chunk_stride + (size_t)(i % h.b_chunk) *
                                                                                        h.b_tree_bytes;
    char* chunk = blob.data() + (size_t)(i / ch) * stride;
    uint32_t* dst = reinterpret_cast<uint32_t*>(chunk + (size_t)(i % ch) * 1024);
    for (int s = 1; s < NL; ++s) {
      uint32_t w;
      std::memcpy(&w, src + (size_t)s * 4, 4);
      const uint32_t f = (w >> 10) & 63u;
      uint32_t j = w >> 16;
      if (!h.pad[(size_t)i * NL + s]) {  // real split: its threshold's index in the merged table
        const float t = h.b_thr[h.b_thr_off[f] + j];
        j = (uint32_t)(std::lower_bound(merged[f].begin(), merged[f].end(), t) - merged[f].begin());
      }
      dst[s] = ens_node_word(j, f, ens_link(s, NL), (w & 1u) != 0);
    }
    std::memcpy(chunk + (size_t)ch * 1024 + (size_t)(i % ch) * NL * lsz, src + (size_t)NL * 4, (size_t)NL * lsz);
  }
  return blob;
}

// build_plan step 3, contract 1 / 2 — the contracted forest (contract_forest_host) in the full chunks' geometry (nc
// chunks of ch trees, NL = 2^D leaf values per row): tree i a perfect heap of depth dw <= D — the deepest of its
// wave's ch / 4 trees (contract 1) or its own depth d_i (contract 2) — in its 1 KiB node block, the last split level's link
// s - 2^(dw - 1), dw in heap slot 0 (it arrives with the chunk's DMA), its 2^dw leaves at the start of its leaf row.
// Padding trees of a partial last chunk: pad nodes and zero leaves (contract 2: depth 1). Thresholds are looked up in
// the same merged tables (the contracted trees' are a subset). steps: the sum of the forest's own trees' dw.
std::vector<char> pack_contracted_chunks(const ContractedForest& c, bool xgb, const Tables& merged, int nc, int ch,
                                         size_t stride, int D, int contract, long long& steps) {
  const int T = (int)c.off.size() - 1, tpg = ch / 4, NL = 1 << D;
  const size_t nb = (size_t)nc * ch, lsz = xgb ? 4 : 8;
  std::vector<int> dw(nb, 1);
  for (int i = 0; i < T; ++i) dw[i] = std::min(c.depth[i], D);
  if (contract == 1)
    for (size_t g0 = 0; g0 < nb; g0 += tpg) {
      const int mx = *std::max_element(dw.begin() + g0, dw.begin() + g0 + tpg);
      std::fill(dw.begin() + g0, dw.begin() + g0 + tpg, mx);
    }
  std::vector<char> blob((size_t)nc * stride, 0);
  for (size_t i = 0; i < nb; ++i) {
    char* chunk = blob.data() + (i / ch) * stride;
    uint32_t* dst = reinterpret_cast<uint32_t*>(chunk + (i % ch) * 1024);
    dst[0] = (uint32_t)dw[i];
    if ((int)i >= T) {  // a padding tree: pad nodes with their links (a zero word would link to heap slot 0)
      const int nl = 1 << dw[i];
      for (int s = 1; s < nl; ++s) dst[s] = ens_node_word(0, 0, ens_link(s, nl), false);
      continue;
    }
    steps += dw[i];
    expand_heap(c, (int)i, xgb, merged, dw[i], dst, chunk + (size_t)ch * 1024 + (i % ch) * NL * lsz,
                [](int f) { return (uint32_t)f; });
  }
  return blob;
}

void upload(DeviceBuffer& d, const std::vector<char>& blob) {
  d.ensure(blob.size());
  FD_HIP(hipMemcpy(d.ptr, blob.data(), blob.size(), hipMemcpyHostToDevice));
}

}  // namespace

// The dense chunk stream of one contracted forest (include/fdengine.h fd_dense_layout_host: the layout, the chunk
// table and the node word): build_plan's chunks under ensemble_contract 3 / 4 and the host export, one function.
DenseLayout dense_layout_host(const ContractedForest& c, bool xgb, const std::vector<std::vector<float>>& tables,
                              bool wide, int mode, int owner_bias) {
  FD_REQUIRE(mode == 3 || mode == 4, FD_ERR_INVALID_ARG, "dense layout: mode 3 or 4");
  FD_REQUIRE(owner_bias >= 0 && owner_bias <= 64, FD_ERR_INVALID_ARG, "dense layout: owner_bias in [0, 64]");
  DenseLayout L;
  const int T = (int)c.off.size() - 1;
  const int tpg = ens_chunk_trees(wide, xgb ? 0 : 1) / 4;
  const size_t lsz = xgb ? 4 : 8;
  L.tpg = tpg;
  L.buf = ens_buf(wide);
  L.tree.assign((size_t)T, fd_dense_tree{});
  for (int i = 0; i < T; ++i)
    FD_REQUIRE(c.depth[i] >= 1 && c.depth[i] <= 8, FD_ERR_UNSUPPORTED, "dense layout: a tree deeper than 8 levels");
  struct Bundle {
    std::vector<int> trees;  // forest indices, in place order
    int depth = 1;
  };
  // trees [i0, i0 + n) as bundles, and the data bytes they take
  auto bundle_up = [&](int i0, int n, std::vector<Bundle>& B) {
    std::vector<int> order(n);
    for (int k = 0; k < n; ++k) order[k] = i0 + k;
    if (mode == 4)
      std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return c.depth[x] > c.depth[y]; });
    B.clear();
    size_t bytes = 0;
    // a partial bundle (the forest's last chunk): in mode 3 the forest's last trees; in mode 4 at the place in the
    // sorted order where the sum of the walked depths is least (the last such place) — some place is optimal for these
    // bundle sizes, so mode 4 never walks more levels than mode 3
    const int nbund = (n + tpg - 1) / tpg, part = n % tpg;
    int where = nbund - 1;
    if (mode == 4 && part) {
      long long best = -1;
      for (int w = 0; w < nbund; ++w) {
        long long cost = 0;
        for (int q = 0, k = 0; q < nbund; ++q) {
          const int sz = q == w ? part : tpg;
          cost += (long long)sz * c.depth[order[k]];  // sorted: the bundle's first tree is its deepest
          k += sz;
        }
        if (best < 0 || cost <= best) best = cost, where = w;
      }
    }
    for (int q = 0, k = 0; q < nbund; ++q) {
      const int sz = (part && q == where) ? part : tpg;
      Bundle b;
      b.trees.assign(order.begin() + k, order.begin() + k + sz);
      k += sz;
      for (int t : b.trees) b.depth = std::max(b.depth, (int)c.depth[t]);
      bytes += b.trees.size() * ((4 + lsz) << b.depth);
      B.push_back(std::move(b));
    }
    return bytes;
  };
  // the node word's slot: the feature's compact index (the dense bin tile holds the varying slots only)
  auto compact_slot = [&](int f) {
    FD_REQUIRE(f >= 0 && f < (int)tables.size() && compact_src(f) >= 0, FD_ERR_UNSUPPORTED,
               "dense layout: a split on a constant slot");
    return (uint32_t)compact_src(f);
  };
  std::vector<Bundle> B, cand;
  int i0 = 0;
  while (i0 < T) {
    int n = 0;
    for (int m = tpg;; m += tpg) {  // grow by a bundle's worth of trees while the caps hold
      const int me = std::min(m, T - i0);
      const size_t bytes = bundle_up(i0, me, cand);
      if ((int)cand.size() > kDenseSMax || bytes > L.buf) break;
      n = me;
      B = cand;
      if (i0 + m >= T) break;
    }
    FD_REQUIRE(n > 0, FD_ERR_UNSUPPORTED, "dense layout: one bundle exceeds the chunk buffer");
    const int nb = (int)B.size(), ci = (int)L.chunk_off.size();
    // blocks: the node blocks by size (every block aligned to its own size), then the leaf rows in forest order
    std::vector<int> by_size;
    std::vector<int> bundle_of(n), place_of(n);
    for (int b = 0; b < nb; ++b)
      for (size_t j = 0; j < B[b].trees.size(); ++j) {
        bundle_of[B[b].trees[j] - i0] = b;
        place_of[B[b].trees[j] - i0] = (int)j;
      }
    for (int k = 0; k < n; ++k) by_size.push_back(k);
    std::stable_sort(by_size.begin(), by_size.end(),
                     [&](int x, int y) { return B[bundle_of[x]].depth > B[bundle_of[y]].depth; });
    size_t at = 0;
    for (int k : by_size) {
      L.tree[i0 + k].node_offset = (int32_t)at;
      at += (size_t)4 << B[bundle_of[k]].depth;
    }
    for (int k = 0; k < n; ++k) {
      L.tree[i0 + k].leaf_offset = (int32_t)at;
      at += lsz << B[bundle_of[k]].depth;
    }
    FD_REQUIRE(at <= L.buf, FD_ERR_UNSUPPORTED, "dense layout: chunk data exceed the buffer");
    const size_t data = (at + 1023) / 1024 * 1024, base = L.blob.size();
    L.blob.resize(base + data + kDenseTab, 0);
    L.chunk_off.push_back((int64_t)base);
    L.chunk_len.push_back((int32_t)(data + kDenseTab));
    char* chunk = L.blob.data() + base;
    // deal the bundles to the tree groups: deepest first, each to the least loaded group
    std::vector<int> deal(nb);
    for (int b = 0; b < nb; ++b) deal[b] = b;
    std::stable_sort(deal.begin(), deal.end(), [&](int x, int y) { return B[x].depth > B[y].depth; });
    long long load[4] = {(long long)owner_bias * n, 0, 0, 0};  // sixteenths of a level
    std::vector<int> group_of(nb);
    std::vector<std::vector<int>> of_group(4);
    for (int b : deal) {
      int g = 0;
      for (int q = 1; q < 4; ++q)
        if (load[q] < load[g]) g = q;
      load[g] += 16ll * B[b].depth;
      group_of[b] = g;
      of_group[g].push_back(b);
    }
    // the trees
    for (int k = 0; k < n; ++k) {
      const int i = i0 + k, dw = B[bundle_of[k]].depth;
      fd_dense_tree& t = L.tree[i];
      t.chunk = ci;
      t.bundle = bundle_of[k];
      t.group = group_of[bundle_of[k]];
      t.depth = dw;
      L.steps += dw;
      expand_heap(c, i, xgb, tables, dw, reinterpret_cast<uint32_t*>(chunk + t.node_offset), chunk + t.leaf_offset,
                  compact_slot);
    }
    // the chunk table
    uint32_t* tab = reinterpret_cast<uint32_t*>(chunk + data);
    tab[0] = (uint32_t)n | ((uint32_t)nb << 8);
    if (ci > 0) {  // the previous chunk's table names this one
      uint32_t* prev =
          reinterpret_cast<uint32_t*>(L.blob.data() + L.chunk_off[ci - 1] + L.chunk_len[ci - 1] - kDenseTab);
      prev[1] = (uint32_t)(base >> 10);
      prev[2] = (uint32_t)((data + kDenseTab) >> 10);
    }
    for (int g = 0; g < 4; ++g) {
      tab[3] |= (uint32_t)of_group[g].size() << (8 * g);
      for (size_t s = 0; s < of_group[g].size(); ++s) {
        const int b = of_group[g][s];
        uint32_t* e = tab + (kDenseGroupTab + kDenseGroupStride * g + kDenseBundleEnt * s) / 4;
        e[0] = (uint32_t)B[b].depth | ((uint32_t)b << 8) | ((uint32_t)g << 16);
        for (int j = 0; j < 6; ++j) {
          const int t = B[b].trees[(size_t)j < B[b].trees.size() ? j : 0];
          e[1 + j / 2] |= (uint32_t)L.tree[t].node_offset << (16 * (j & 1));
        }
      }
    }
    for (int k = 0; k < n; ++k)
      tab[kDenseTreeTab / 4 + k] =
          (uint32_t)(kDenseTileRow * bundle_of[k] + place_of[k]) | ((uint32_t)L.tree[i0 + k].leaf_offset << 16);
    i0 += n;
  }
  return L;
}

// joint repack of forest A (XGBoost, slot sa) and B (IsolationForest, slot sb) into plan P; either slot may be -1
// (a single forest: the kernel walks only the other one); false when not possible (the per-model path runs)
// contract (option ensemble_contract; 0 for the single-forest plans, whose rows are 64-wide): also pack nodes_c[]
bool build_plan(Engine& e, EnsemblePlan& P, int sa, int sb, bool wide, int contract) {
  P.valid = false;
  const PackedForest* F[2] = {sa >= 0 ? &e.forests[sa] : nullptr, sb >= 0 ? &e.forests[sb] : nullptr};
  if (!F[0] && !F[1]) return false;
  int D = 0, nf = -1;
  for (const PackedForest* f : F) {
    if (!f) continue;
    // (a sparse-only forest — predict_proba kind or deeper than the heaps — has no binned layout: per-model path)
    if (f->sparse_only || !f->binned || f->t_off.empty() || (nf >= 0 && f->num_feature != nf)) return false;
    nf = f->num_feature;
    D = std::max(D, f->depth);
  }
  if (D > 8) return false;
  if (ens_lds(nf, wide) > kLdsBudget) return false;
  HostPack hp[2];
  const HostPack* present[2] = {nullptr, nullptr};
  for (int k = 0; k < 2; ++k) {
    if (!F[k]) continue;
    hp[k] = pack_forest_host(F[k]->params, arrays_of(*F[k]), D);
    if (!hp[k].binned || hp[k].depth != D) return false;
    present[k] = &hp[k];
  }
  // 1. the merged per-feature tables, and their flat copy for the device
  Tables merged;
  if (!merge_tables(present, nf, merged)) return false;
  std::vector<float> thr;
  std::vector<int32_t> off(nf + 1, 0);
  int maxc = 0;
  for (int f = 0; f < nf; ++f) {
    thr.insert(thr.end(), merged[f].begin(), merged[f].end());
    off[f + 1] = (int32_t)thr.size();
    maxc = std::max(maxc, (int)merged[f].size());
  }
  // 2. the full chunks
  const int NL = 1 << D;
  const size_t leaf_sz[2] = {sizeof(float), sizeof(double)};
  for (int k = 0; k < 2; ++k) {
    const int ch = ens_chunk_trees(wide, k);
    P.CH[k] = ch;
    if (!F[k]) {
      P.n_trees[k] = P.n_chunks[k] = 0;
      P.stride[k] = 0;
      continue;
    }
    const size_t stride = ((size_t)ch * 1024 + (size_t)ch * NL * leaf_sz[k] + 1023) / 1024 * 1024;
    FD_REQUIRE(stride <= ens_buf(wide), FD_ERR_UNSUPPORTED, "ensemble chunk exceeds its LDS buffer");
    upload(P.nodes[k], pack_full_chunks(hp[k], merged, ch, NL, leaf_sz[k], stride));
    P.n_trees[k] = hp[k].n_trees;
    P.n_chunks[k] = (hp[k].n_trees + ch - 1) / ch;
    P.stride[k] = stride;
  }
  // 3. the contracted chunks: the dense chunk stream (contract 3 / 4, the VD 3 kernel) or the padded 1 KiB blocks
  P.contract = contract;
  P.contracted = false;
  P.nodes_pruned = 0;
  P.steps_full = P.steps_c = 0;
  P.dense_len0[0] = P.dense_len0[1] = P.dense_chunks[0] = P.dense_chunks[1] = 0;
  for (int k = 0; k < 2 && contract; ++k) {
    if (!F[k]) continue;
    const bool xgb = F[k]->params.kind == FD_FOREST_XGB_BINARY_LOGISTIC;
    const ContractedForest c = contract_forest_host(F[k]->params, arrays_of(*F[k]));
    if (contract >= 3) {
      FD_REQUIRE(ens_lds_dense(wide) <= ens_lds(kMaxFeatures, wide), FD_ERR_UNSUPPORTED,
                 "dense layout: more LDS than the padded layout");
      const DenseLayout L = dense_layout_host(c, xgb, merged, wide, contract, kDenseOwnerBias);
      upload(P.nodes_c[k], L.blob);
      P.dense_len0[k] = L.chunk_len.empty() ? 0 : L.chunk_len[0];
      P.dense_chunks[k] = (int)L.chunk_len.size();
      P.steps_c += L.steps;
    } else {
      upload(P.nodes_c[k],
             pack_contracted_chunks(c, xgb, merged, P.n_chunks[k], P.CH[k], P.stride[k], D, contract, P.steps_c));
    }
    P.nodes_pruned += c.pruned;
  }
  for (int k = 0; k < 2; ++k) P.steps_full += F[k] ? (long long)hp[k].n_trees * D : 0;
  P.contracted = contract != 0 && P.steps_c < P.steps_full;
  P.thr.ensure(std::max<size_t>(4, thr.size() * sizeof(float)));
  if (!thr.empty()) FD_HIP(hipMemcpy(P.thr.ptr, thr.data(), thr.size() * sizeof(float), hipMemcpyHostToDevice));
  P.h_thr_off = off;
  // 4. the bins of the compact vector's constant slots (0 or 0.5): #{t <= value} in the feature's merged table; and
  // of the small-integer compact slots' values 0 .. kLutN - 1
  P.h_cbin.assign(kMaxFeatures, 0);
  for (int f = 0; f < nf && f < kMaxFeatures; ++f) {
    const int src = compact_src(f);
    if (src >= 0) continue;
    const float val = src == -2 ? 0.5f : 0.0f;
    P.h_cbin[f] = (uint16_t)(std::upper_bound(merged[f].begin(), merged[f].end(), val) - merged[f].begin());
  }
  P.h_lut.assign((size_t)kIntSlots * kLutN, 0);
  for (int k = 0; k < kIntSlots; ++k) {
    const int f = kCompactSlot[kIntCompact[k]];
    if (f >= nf) continue;
    for (int x = 0; x < kLutN; ++x)
      P.h_lut[(size_t)k * kLutN + x] =
          (uint16_t)(std::upper_bound(merged[f].begin(), merged[f].end(), (float)x) - merged[f].begin());
  }
  // 5. the binning passes and their table images
  {
    std::vector<float> img;
    plan_passes(thr, off, nf, wide, P.passes, img);
    P.img.ensure(std::max<size_t>(1024, img.size() * sizeof(float)));
    if (!img.empty()) FD_HIP(hipMemcpy(P.img.ptr, img.data(), img.size() * sizeof(float), hipMemcpyHostToDevice));
  }
  P.max_feature_thr = maxc;
  P.slot[0] = sa;
  P.slot[1] = sb;
  P.gen[0] = F[0] ? F[0]->gen : 0;
  P.gen[1] = F[1] ? F[1]->gen : 0;
  P.n_forests = (F[0] ? 1 : 0) + (F[1] ? 1 : 0);
  P.D = D;
  P.nf = nf;
  P.wide = wide;
  P.kind[0] = FD_FOREST_XGB_BINARY_LOGISTIC;
  P.kind[1] = FD_FOREST_SKLEARN_IFOREST;
  P.base_margin = F[0] ? hp[0].base_margin : 0.f;
  P.if_offset = F[1] ? F[1]->if_offset : 0.0;
  P.if_denominator = F[1] ? F[1]->if_denominator : 0.0;
  P.valid = true;
  return true;
}

bool plan_current(const Engine& e, const EnsemblePlan& P, int sa, int sb, bool wide, int contract) {
  return P.valid && P.wide == wide && P.contract == contract && P.slot[0] == sa && P.slot[1] == sb &&
         P.gen[0] == (sa >= 0 ? e.forests[sa].gen : 0) && P.gen[1] == (sb >= 0 ? e.forests[sb].gen : 0);
}

// the chunk layout for this engine: option "ensemble_chunks" 1 wide / 2 compact, 0 (auto) compact once the engine
// has RCCL communicators (its sharded step's exchanges co-run with the scoring), else wide
bool want_wide(const Engine& e) { return e.ens_chunks == 1 || (e.ens_chunks == 0 && !e.comm.ready); }

}  // namespace fd
