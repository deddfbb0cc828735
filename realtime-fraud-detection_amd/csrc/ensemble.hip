// ensemble.hip — the fused scoring kernel of the hot path: the XGBoost primary classifier
// (ml/models/model_manager.py:309-311) and the IsolationForest (:338-346) walked over ONE binned feature
// tile per 256-transaction tile, then the ensemble epilogue (ensemble_predictor.py:185-369: clamp,
// confidence, weighted / voting / stacking blend, decision, risk), in one launch — instead of a forest
// kernel per model (each binning the same vectors in its own prologue) plus a blend kernel.
//
// Joint repack (host, ensemble_plan.hip build_plan, cached per pair of loaded forests): both forests padded to one
// depth D <= 8 and their node words rewritten against the MERGED per-feature table of distinct thresholds (union
// of the two), so one bin word per (feature, transaction) serves both: "x < t" is "bin_merged(x) <= index of t in
// the merged table" for every threshold of either forest. Leaf ids are not produced on this path (the per-model
// kernels keep the leaf-id outputs).
//
// Kernel: 1024 threads = 16 waves per tile (tree group gg = wave >> 2, transaction group wave & 3). Prologue:
// each thread loads 16 features of its row into registers; the merged table is staged in LDS in feature
// ranges (passes) that fit the chunk buffers + leaf-index tiles (dead until chunk 0 is staged) and every
// value is binned into the u16 tile (two features per 1 KiB row, 32 KiB for 64 features). Then the chunk
// stream is XGBoost's 24-tree chunks followed by the IsolationForest's 16-tree chunks (the compact layout: 20 /
// 12, see EnsCfg) (1 KiB node block per tree + the chunk's leaf values, double-buffered by LDS-DMA); per chunk
// each wave walks its TPG trees (6 / 4; 5 / 3) for its 64 transactions (walk_ens: 4 VALU + 2 LDS reads per node
// step) and stores the packed leaf
// indices to the chunk's index tile; the owner tree group (0) then adds each transaction's leaf values of
// that chunk, read from LDS, in tree order into the f32 margin (XGBoost) or the f64 path-length sum
// (IsolationForest): both the reference's sequential sums, bit for bit. Epilogue (tree group 0, one thread
// per transaction): sigmoid / IsolationForest transform, blend_row, outputs (columns, or the 24-B route
// result records of the owner GPU).
//
// Compact / split rows (the pipelined stream) hold 42 constant slots: the plan also packs the forests with every
// split on such a slot decided (contract_forest_host); 64-wide rows keep the full forests and the kernels above.
// Engine option ensemble_contract chooses how the contracted forests are laid out and walked on those rows:
//   4 (default), 3 — the dense chunk stream (dense_layout_host; include/fdengine.h documents it), the VD 3 kernel.
//     A bundle is TPG trees walked by one wave, each a perfect heap of the bundle's depth in a node block of its own
//     size (4 * 2^d bytes) with a leaf row of 2^d values; node words name the 22 varying slots, and the bin tile holds
//     only those (11 KiB: no constant bins are written). A chunk is a run of consecutive trees, up to kDenseSMax = 8
//     bundles that fit the chunk buffer, closed by a 1 KiB chunk table that the DMA puts at a fixed place behind the
//     buffer: per tree group its bundles (depth, tile row, block offsets), per tree its leaf-index byte and leaf row,
//     and the next chunk's offset and length. Between two barriers a wave walks every bundle of its group with the
//     fixed-depth walk_ens_at (walk_dense), the bundles dealt to the groups deepest first so the four end together;
//     the owner adds the chunk's leaf values in forest order (owner_sum_dense). 4 sorts a chunk's trees by depth
//     before cutting bundles, 3 keeps consecutive trees.
//   1 — the padded 1 KiB-block chunks, each wave's trees walked to the deepest of them (walk_pack_var, VD 2);
//   2 — the same chunks, each tree to its own depth (walk_ens_var, VD 1); 0 — the full forests.
//
// This file: the kernel and its launchers. The plans they run — the joint repack, the contraction, the chunk packers
// and the binning passes — are built on the host by ensemble_plan.hip; ensemble_layout.h holds what the two share
// (chunk geometry, LDS layout, node word, the dense chunk table).
#include "blend_row.h"
#include "ensemble_layout.h"
#include "walk_common.h"

namespace fd {

namespace {

constexpr int kEnsWG = 1024;

struct EnsArgs {
  // Field order: what a wave reads before its first LDS-DMA goes out (rows, pass 0's table image, chunk 0) and the
  // other scalars first, packed into the first few 64-B scalar-cache lines; the per-feature / per-pass tables after
  // them (round 6: the prologue's kernel-argument round trips)
  const float* X;
  int64_t n;
  int ld, nf;
  const float* thr;
  int vec4;                       // rows 16-B aligned (ld % 4 == 0, aligned X): float4 row loads
  int compact;                    // 1: X rows are the compact 64-B rows (fd_internal.h), binned here; 2: split rows
                                  // (RowA [n] at X, RowB [n] after it, 32 B each: features.hip, load_split)
  int owner_fixed;                // chunk owner: tree group 0 (the oldest waves: highest issue priority), else rotating
  int prio;                       // issue priority 2 above the co-running feature kernels (engine option ensemble_prio)
  int n_pass;
  int ldepth;                      // variable-depth walk (VD kernels): the plan's depth D, leaf rows of 2^D values
  unsigned long long pass_global;  // bit p: pass p bins from global memory (its table does not fit LDS)
  const char* img;                 // the passes' padded table images (thr_pad layout), 1 KiB pieces
  const char* nodes[2];
  int n_chunks[2];
  int stride[2];
  float base_margin;
  int pad1;
  double if_offset, if_denom;
  int pos[2];   // blend position (present-model order) of forest A / B
  int mcol[2];  // model-probability column (caller's model index) of forest A / B
  double* mp;
  double* fp;
  double* conf;
  uint8_t* dec;
  uint8_t* risk;
  const RouteRecord* rec;
  ResultRecord* res;
  int pass_f[kMaxPass + 1];
  int img_off[kMaxPass + 1];       // pass p's image: bytes [img_off[p], img_off[p + 1]) of img
  int thr_off[kMaxFeatures + 1];  // per-feature table offsets into thr (kernel arguments: scalar loads)
  uint16_t cbin[kMaxFeatures];    // compact mode: the bins of the constant slots (0 or 0.5), per plan
  // dense kernel: compact slot c's table, elements [cthr[2 c], cthr[2 c + 1]) of thr — the same numbers as thr_off's.
  // A compiler reason, not an algorithmic one: with thr_off the dense instantiations merge the constant-index reads
  // into 4- and 8-dword argument loads that the register allocator first spills and then re-loads instead, and the
  // dead 16-32 B spill slot stays in the frame: a kernel with a private segment (tests/test_kernel_budget.py holds
  // the hot kernels to none). Read from cthr they compile to 0 B of scratch, at 65 / 54 VGPRs as the other kernels.
  int cthr[2 * kCompactSlots];
  alignas(4) uint16_t lut[8 * 32];  // compact mode: [kIntSlots][kLutN] bins of the small-integer slots' values 0..31
  BlendConsts blend;
#ifdef FD_FOREST_PROFILE
  int prof_slot;  // which of the kEprofSlots profile buffers this launch writes (launch count mod kEprofSlots)
  int clk_slot;   // this launch's record in g_eclk (launch count mod kEclkSlots)
#endif
};

// The walk of TPG trees over D levels, one step 4 VALU + 2 LDS reads (the node word: ensemble_layout.h).
// tb[j]: the LDS address of tree j's node block, aligned to the block's 4 * 2^D bytes (the link OR is exact)
template <int D, int TPG, bool NAN_AWARE>
__device__ __forceinline__ void walk_ens_at(uint32_t (&tb)[TPG], uint32_t lane4, uint32_t (&leaf)[TPG]) {
  uint32_t node[TPG], kl[TPG], kr[TPG], xw[TPG];
#pragma unroll
  for (int j = 0; j < TPG; ++j) {
    // in a VGPR: v_and_or_b32 takes one scalar operand on gfx9 (the mask literal), else it splits in two
    asm volatile("" : "+v"(tb[j]));
    node[j] = lds_load<uint32_t>(tb[j] + 4u);
  }
#pragma unroll
  for (int j = 0; j < TPG; ++j) {
    xw[j] = lds_load<uint16_t>((node[j] & 0xFC02u) | lane4);
    if (D > 1) {
      const u32x2 k = lds_load<u32x2>(tb[j] + 8u);
      kl[j] = k.x;
      kr[j] = k.y;
    }
  }
#pragma unroll
  for (int l = 0; l < D; ++l) {
#pragma unroll
    for (int j = 0; j < TPG; ++j) {
      bool right = xw[j] > (node[j] >> 16);  // bin > j  <=>  !(x < t_j)
      if (NAN_AWARE) {
        if (xw[j] == 0xFFFFu) right = (node[j] & 1u) == 0u;  // missing: default direction
      }
      if (l + 1 < D) {
        uint32_t a = kl[j], b = kr[j];
        asm volatile("" : "+v"(a), "+v"(b));
        node[j] = right ? b : a;
        xw[j] = lds_load<uint16_t>((node[j] & 0xFC02u) | lane4);
        if (l + 2 < D) {
          const u32x2 k = lds_load<u32x2>((node[j] & kLinkMask) | tb[j]);
          kl[j] = k.x;
          kr[j] = k.y;
        }
      } else {
        leaf[j] = ((node[j] & kLinkMask) >> 2) + (right ? 1u : 0u);
      }
    }
  }
}

// the padded chunks: tree t0 + j in the 1 KiB block t0 + j of the chunk at buf
template <int D, int TPG, bool NAN_AWARE>
__device__ __forceinline__ void walk_ens(uint32_t buf, int t0, uint32_t lane4, uint32_t (&leaf)[TPG]) {
  uint32_t tb[TPG];
#pragma unroll
  for (int j = 0; j < TPG; ++j) tb[j] = buf + (uint32_t)(t0 + j) * 1024u;
  walk_ens_at<D, TPG, NAN_AWARE>(tb, lane4, leaf);
}

// a wave's TPG leaf indices (< 2^D <= 256) as one u64, a byte per tree in tree order
template <int TPG>
__device__ __forceinline__ unsigned long long pack_leaf_bytes(const uint32_t (&leaf)[TPG]) {
  static_assert(TPG <= 8, "a byte per tree in a u64");
  uint32_t lo = 0, hi = 0;
#pragma unroll
  for (int j = 0; j < TPG; ++j) {
    if (j < 4) lo |= leaf[j] << (8 * j);
    else hi |= leaf[j] << (8 * (j - 4));
  }
  return ((unsigned long long)hi << 32) | lo;
}

// Walk this wave's TPG trees of the chunk at `cur` (trees gg*TPG ...) for its 64 transactions; the leaf
// indices (< 2^D <= 256) packed a byte per tree, in tree order, stored as one u64 per (tree group, txn).
// (Measured: byte-per-tree stores of a [txn][16] tile cost ~5 us more per 64k batch; skewing the split
// towards tree group 0 was slower still.)
template <int D, int TPG>
__device__ __forceinline__ unsigned long long walk_pack(uint32_t cur, int gg, uint32_t lane4, bool tile_nan) {
  uint32_t leaf[TPG];
  if (tile_nan)
    walk_ens<D, TPG, true>(cur, gg * TPG, lane4, leaf);
  else
    walk_ens<D, TPG, false>(cur, gg * TPG, lane4, leaf);
  return pack_leaf_bytes<TPG>(leaf);
}

// The walk over contracted trees (build_plan: every split on a constant slot of the compact vector resolved on the
// host), tree j a perfect heap of its own depth d[j] <= 8, the depths wave-uniform (SGPRs). Level-synchronous: the
// selects of all chains first (VALU only; a finished chain's select is dead), then the reads of the chains that go on
// — chain j issues its bin read only while l + 1 < d[j] and its pair read while l + 2 < d[j] — so the uniform branches
// stand between whole phases and not inside a chain's step. The leaf index is formed at level d[j] - 1.
template <int TPG, bool NAN_AWARE>
__device__ __forceinline__ void walk_ens_var(uint32_t buf, int t0, uint32_t lane4, const int (&d)[TPG],
                                             uint32_t (&leaf)[TPG]) {
  uint32_t tb[TPG], node[TPG], kl[TPG], kr[TPG], xw[TPG];
  int dw = 1;
#pragma unroll
  for (int j = 0; j < TPG; ++j) {
    tb[j] = buf + (uint32_t)(t0 + j) * 1024u;
    asm volatile("" : "+v"(tb[j]));
    node[j] = lds_load<uint32_t>(tb[j] + 4u);
    dw = max(dw, d[j]);
    leaf[j] = 0u;
  }
#pragma unroll
  for (int j = 0; j < TPG; ++j) {
    xw[j] = lds_load<uint16_t>((node[j] & 0xFC02u) | lane4);
    const u32x2 k = lds_load<u32x2>(tb[j] + 8u);  // (a depth-1 tree's: inside its block, unused)
    kl[j] = k.x;
    kr[j] = k.y;
  }
#pragma unroll
  for (int l = 0; l < 8; ++l) {
    if (l >= dw) break;
#pragma unroll
    for (int j = 0; j < TPG; ++j) {
      bool right = xw[j] > (node[j] >> 16);
      if (NAN_AWARE) {
        if (xw[j] == 0xFFFFu) right = (node[j] & 1u) == 0u;
      }
      const uint32_t at = ((node[j] & kLinkMask) >> 2) + (right ? 1u : 0u);
      leaf[j] = (l + 1 == d[j]) ? at : leaf[j];
      node[j] = right ? kr[j] : kl[j];
    }
    if (l + 1 >= dw) break;
#pragma unroll
    for (int j = 0; j < TPG; ++j) {
      if (l + 1 < d[j]) {
        xw[j] = lds_load<uint16_t>((node[j] & 0xFC02u) | lane4);
        if (l + 2 < d[j]) {
          const u32x2 k = lds_load<u32x2>((node[j] & kLinkMask) | tb[j]);
          kl[j] = k.x;
          kr[j] = k.y;
        }
      }
    }
  }
}

// walk_pack over a chunk of contracted trees: the wave's TPG depths from heap slot 0 of its trees' node blocks (one
// broadcast read each, kept scalar). VD 1: every tree to its own depth (walk_ens_var); VD 2: the host padded the
// wave's trees to the deepest of them, and that depth selects a fixed-depth walk_ens.
template <int VD, int TPG>
__device__ __forceinline__ unsigned long long walk_pack_var(uint32_t cur, int gg, uint32_t lane4, bool tile_nan) {
  uint32_t leaf[TPG];
  int d[TPG];
#pragma unroll
  for (int j = 0; j < TPG; ++j)
    d[j] = __builtin_amdgcn_readfirstlane((int)lds_load<uint32_t>(cur + (uint32_t)(gg * TPG + j) * 1024u)) & 0xFF;
  if (VD == 1) {
    if (tile_nan)
      walk_ens_var<TPG, true>(cur, gg * TPG, lane4, d, leaf);
    else
      walk_ens_var<TPG, false>(cur, gg * TPG, lane4, d, leaf);
  } else {
#define FD_WALK_DEPTH(K)                                          \
  case K:                                                         \
    if (tile_nan)                                                 \
      walk_ens<K, TPG, true>(cur, gg * TPG, lane4, leaf);         \
    else                                                          \
      walk_ens<K, TPG, false>(cur, gg * TPG, lane4, leaf);        \
    break;
    switch (d[0]) {
      FD_WALK_DEPTH(1)
      FD_WALK_DEPTH(2)
      FD_WALK_DEPTH(3)
      FD_WALK_DEPTH(4)
      FD_WALK_DEPTH(5)
      FD_WALK_DEPTH(6)
      FD_WALK_DEPTH(7)
      default:
        if (tile_nan)
          walk_ens<8, TPG, true>(cur, gg * TPG, lane4, leaf);
        else
          walk_ens<8, TPG, false>(cur, gg * TPG, lane4, leaf);
        break;
    }
#undef FD_WALK_DEPTH
  }
  return pack_leaf_bytes<TPG>(leaf);
}

// walk_ens_at, the leaf indices packed a byte per tree as walk_pack's (written out, not pack_leaf_bytes: through the
// call the dense kernels' instructions come out in another order)
template <int D, int TPG, bool NAN_AWARE>
__device__ __forceinline__ unsigned long long walk_pack_at(uint32_t (&tb)[TPG], uint32_t lane4) {
  uint32_t leaf[TPG];
  walk_ens_at<D, TPG, NAN_AWARE>(tb, lane4, leaf);
  uint32_t lo = 0, hi = 0;
#pragma unroll
  for (int j = 0; j < TPG; ++j) {
    if (j < 4) lo |= leaf[j] << (8 * j);
    else hi |= leaf[j] << (8 * (j - 4));
  }
  return ((unsigned long long)hi << 32) | lo;
}

// The dense chunk at `cur`, its table at `tab` (dense_layout_host): this wave walks every bundle the table gives its
// tree group, deepest first — depth, tile row and the trees' node-block offsets from the bundle's 16-B entry (one
// broadcast read, depth and row kept scalar; the next entry is read before the walk) — and stores each bundle's leaf bytes to
// tile[bundle][txn]. counts: word 3 of the table, the groups' bundle counts.
template <int TPG>
__device__ __forceinline__ void walk_dense(uint32_t cur, uint32_t tab, uint32_t tw, int gg, int txn, uint32_t lane4,
                                           bool tile_nan, uint32_t counts) {
  static_assert(TPG <= 6, "six block offsets per bundle entry");
  const int nb = (int)((counts >> (8 * gg)) & 0xFFu);
  const uint32_t ent = tab + kDenseGroupTab + (uint32_t)gg * kDenseGroupStride;
  u32x4 e = lds_load<u32x4>(ent);
  for (int s = 0; s < nb; ++s) {
    // (the offsets stay in VGPRs, where the block addresses are wanted: only the depth and the tile row are scalar)
    const uint32_t e0 = __builtin_amdgcn_readfirstlane(e.x);
    const uint32_t off[6] = {e.y & 0xFFFFu, e.y >> 16, e.z & 0xFFFFu, e.z >> 16, e.w & 0xFFFFu, e.w >> 16};
    // (past the group's last entry: still inside the table)
    e = lds_load<u32x4>(ent + (uint32_t)(s + 1) * kDenseBundleEnt);
    uint32_t tb[TPG];
#pragma unroll
    for (int j = 0; j < TPG; ++j) tb[j] = cur + off[j];
    // (packed inside each case: merged after the switch, the TPG leaf indices become one <TPG x i32> value that the
    // compiler legalises through a stack slot)
    unsigned long long w;
#define FD_WALK_DEPTH(K)                                                                                        \
  case K:                                                                                                       \
    w = tile_nan ? walk_pack_at<K, TPG, true>(tb, lane4) : walk_pack_at<K, TPG, false>(tb, lane4);              \
    break;
    switch (e0 & 0xFFu) {
      FD_WALK_DEPTH(1)
      FD_WALK_DEPTH(2)
      FD_WALK_DEPTH(3)
      FD_WALK_DEPTH(4)
      FD_WALK_DEPTH(5)
      FD_WALK_DEPTH(6)
      FD_WALK_DEPTH(7)
      default:
        w = tile_nan ? walk_pack_at<8, TPG, true>(tb, lane4) : walk_pack_at<8, TPG, false>(tb, lane4);
        break;
    }
#undef FD_WALK_DEPTH
    lds_store<unsigned long long>(tw + (((e0 >> 8) & 0xFFu) * (uint32_t)kTile + (uint32_t)txn) * 8u,
                                  w);
  }
}

// owner_sum over a dense chunk: the chunk's trees in forest order, tree k's leaf index from the tile byte its table
// entry names and its value from its leaf row, eight trees at a time — the entries two batches ahead and the indices
// one batch ahead of the values, so the three dependent reads of a tree overlap its neighbours'. Entries past the
// chunk's last tree are zero (reads inside the buffer, values not added).
template <typename LeafT>
__device__ __forceinline__ void owner_sum_dense(uint32_t buf, uint32_t tab, uint32_t tile, uint32_t acc, int txn) {
  const int n = (int)(__builtin_amdgcn_readfirstlane(lds_load<uint32_t>(tab)) & 0xFFu);
  const uint32_t tx = tile + (uint32_t)txn * 8u, ent = tab + kDenseTreeTab;
  // (entries as two u32x4 per batch, unrolled component reads: no array the compiler could leave on the stack)
  u32x4 ea = lds_load<u32x4>(ent), eb = lds_load<u32x4>(ent + 16u);
  u32x4 na = lds_load<u32x4>(ent + 32u), nb = lds_load<u32x4>(ent + 48u);
  uint32_t i0 = lds_load<uint8_t>(tx + (ea.x & 0xFFFFu)), i1 = lds_load<uint8_t>(tx + (ea.y & 0xFFFFu)),
           i2 = lds_load<uint8_t>(tx + (ea.z & 0xFFFFu)), i3 = lds_load<uint8_t>(tx + (ea.w & 0xFFFFu)),
           i4 = lds_load<uint8_t>(tx + (eb.x & 0xFFFFu)), i5 = lds_load<uint8_t>(tx + (eb.y & 0xFFFFu)),
           i6 = lds_load<uint8_t>(tx + (eb.z & 0xFFFFu)), i7 = lds_load<uint8_t>(tx + (eb.w & 0xFFFFu));
  LeafT s = lds_load<LeafT>(acc + (uint32_t)txn * (uint32_t)sizeof(LeafT));
  constexpr uint32_t LS = (uint32_t)sizeof(LeafT);
  for (int b = 0; b < n; b += 8) {
    const LeafT v0 = lds_load<LeafT>(buf + (ea.x >> 16) + i0 * LS), v1 = lds_load<LeafT>(buf + (ea.y >> 16) + i1 * LS),
                v2 = lds_load<LeafT>(buf + (ea.z >> 16) + i2 * LS), v3 = lds_load<LeafT>(buf + (ea.w >> 16) + i3 * LS),
                v4 = lds_load<LeafT>(buf + (eb.x >> 16) + i4 * LS), v5 = lds_load<LeafT>(buf + (eb.y >> 16) + i5 * LS),
                v6 = lds_load<LeafT>(buf + (eb.z >> 16) + i6 * LS), v7 = lds_load<LeafT>(buf + (eb.w >> 16) + i7 * LS);
    ea = na;
    eb = nb;
    i0 = lds_load<uint8_t>(tx + (ea.x & 0xFFFFu));
    i1 = lds_load<uint8_t>(tx + (ea.y & 0xFFFFu));
    i2 = lds_load<uint8_t>(tx + (ea.z & 0xFFFFu));
    i3 = lds_load<uint8_t>(tx + (ea.w & 0xFFFFu));
    i4 = lds_load<uint8_t>(tx + (eb.x & 0xFFFFu));
    i5 = lds_load<uint8_t>(tx + (eb.y & 0xFFFFu));
    i6 = lds_load<uint8_t>(tx + (eb.z & 0xFFFFu));
    i7 = lds_load<uint8_t>(tx + (eb.w & 0xFFFFu));
    na = lds_load<u32x4>(ent + (uint32_t)(b + 16) * 4u);
    nb = lds_load<u32x4>(ent + (uint32_t)(b + 16) * 4u + 16u);
    s = b + 0 < n ? s + v0 : s;
    s = b + 1 < n ? s + v1 : s;
    s = b + 2 < n ? s + v2 : s;
    s = b + 3 < n ? s + v3 : s;
    s = b + 4 < n ? s + v4 : s;
    s = b + 5 < n ? s + v5 : s;
    s = b + 6 < n ? s + v6 : s;
    s = b + 7 < n ? s + v7 : s;
  }
  lds_store<LeafT>(acc + (uint32_t)txn * (uint32_t)sizeof(LeafT), s);
}

// One transaction's share of a finished chunk: its CH leaf values (indices from the tile, values from the
// chunk's leaf block in LDS) added in tree order to the forest's running sum — the reference's sequential
// f32 margin / f64 path-length sum, bit for bit.
template <int D, int TPG, int CH, typename LeafT>
__device__ __forceinline__ void owner_sum(uint32_t buf, uint32_t tile, uint32_t acc, int txn, const int NL = 1 << D) {
  unsigned long long w[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) w[q] = lds_load<unsigned long long>(tile + (uint32_t)(q * kTile + txn) * 8u);
  LeafT v[CH];
#pragma unroll
  for (int t = 0; t < CH; ++t) {
    const uint32_t idx = (uint32_t)(w[t / TPG] >> (8 * (t % TPG))) & 0xFFu;
    v[t] = lds_load<LeafT>(buf + (uint32_t)(CH * 1024) + ((uint32_t)(t * NL) + idx) * (uint32_t)sizeof(LeafT));
  }
  LeafT s = lds_load<LeafT>(acc + (uint32_t)txn * (uint32_t)sizeof(LeafT));
#pragma unroll
  for (int t = 0; t < CH; ++t) s += v[t];
  lds_store<LeafT>(acc + (uint32_t)txn * (uint32_t)sizeof(LeafT), s);
}

#ifdef FD_FOREST_PROFILE
// per (workgroup < 256, wave): cycles in prologue, loop top (leaf stores, DMA issue, owner add), walk + leaf
// loads, DMA wait + barrier, epilogue (s_memtime; read by fd_debug_ens_profile)
constexpr int kEprofSlots = 4;  // the last 4 launches (the pipelined stream: launches beside the next features)
__device__ unsigned long long g_eprof[kEprofSlots * 256 * 16 * 16];
static int g_eprof_next = 0;
// per launch, the clocks of wave 0 of workgroups 0, 64, 128, 192: {s_memtime start, end, s_memrealtime start, end}
// (shader clock = memtime cycles / realtime ticks x 100 MHz; tools/clock_ramp.py)
constexpr int kEclkSlots = 1024;
__device__ unsigned long long g_eclk[kEclkSlots * 4 * 4];
static int g_eclk_next = 0;
#define FD_ESTAMP(var) const unsigned long long var = __builtin_amdgcn_s_memtime()
#else
#define FD_ESTAMP(var)
#endif

// bin = #{t <= v} by binary lifting, as bin_of, for L values in lockstep: branch-free (clamped index + select), so
// the L reads of a step issue back to back; tables staged in LDS at tl (element g at thr_pad(g)) or, glob, in global
template <int L>
__device__ __forceinline__ void search_lockstep(const float (&vv)[L], const int (&o)[L], const int (&cnt)[L],
                                                int (&pos)[L], int steps, bool glob, uint32_t tl, int o0,
                                                const float* __restrict__ thr) {
  if (!glob) {
    for (int st = steps; st > 0; st >>= 1) {
      float t[L];
#pragma unroll
      for (int k = 0; k < L; ++k) {
        const int np = pos[k] + st;
        const int idx = np <= cnt[k] ? np - 1 : 0;
        t[k] = lds_load<float>(tl + (uint32_t)thr_pad(o[k] - o0 + idx) * 4u);
      }
#pragma unroll
      for (int k = 0; k < L; ++k) {
        const int np = pos[k] + st;
        pos[k] = (np <= cnt[k] && t[k] <= vv[k]) ? np : pos[k];
      }
    }
  } else {
    for (int st = steps; st > 0; st >>= 1) {
      float t[L];
#pragma unroll
      for (int k = 0; k < L; ++k) {
        const int np = pos[k] + st;
        t[k] = thr[o[k] + (np <= cnt[k] ? np - 1 : 0)];
      }
#pragma unroll
      for (int k = 0; k < L; ++k) {
        const int np = pos[k] + st;
        pos[k] = (np <= cnt[k] && t[k] <= vv[k]) ? np : pos[k];
      }
    }
  }
}

// Compact rows (the pipeline): the 42 constant slots' bins are the plan's (a.cbin), written without a search —
// thread Q of a transaction writes the bin-tile dwords (feature pairs) Q, Q + 4, ... — and the 22 varying slots are
// dealt round-robin to the four threads of the transaction (compact slots Q, Q + 4, ...: 6, 6, 5, 5 searches instead
// of up to 16 per thread over the 64-wide row)
template <int Q>
__device__ __forceinline__ void bin_compact_constants(const EnsArgs& a, uint16_t* Xs, int txn) {
  uint32_t* X32 = reinterpret_cast<uint32_t*>(Xs);
#pragma unroll
  for (int j = Q; j < kMaxFeatures / 2; j += 4) {
    const int f = 2 * j;
    const bool c0 = compact_src(f) < 0 && f < a.nf, c1 = compact_src(f + 1) < 0 && f + 1 < a.nf;
    if (c0 && c1)
      X32[j * 256 + txn] = (uint32_t)a.cbin[f] | ((uint32_t)a.cbin[f + 1] << 16);
    else if (c0)
      Xs[j * 512 + txn * 2] = a.cbin[f];
    else if (c1)
      Xs[j * 512 + txn * 2 + 1] = a.cbin[f + 1];
  }
}

// The compact slots whose values are always small integers — hour, day of week, weekend, the 1 h / 24 h / 5 min
// counts and the account age (each clip10 of an integer), the new-device flag (features.hip write_vector) — are
// binned by one lookup in a per-plan table of the bins of 0..31 (staged in LDS), not searched: each thread keeps 3-4
// searches of its 5-6 (one lockstep group instead of two). A value outside 0..31 or not integral (never, from the
// engine's own feature kernel) takes its own search, so the bins stay #{t <= v} for any input.
// (kLutN: ensemble_layout.h; kIntSlots, kIntCompact, int_slot: fd_internal.h, the compact row's byte slots)
static_assert(kIntSlots * kLutN == 8 * 32, "EnsArgs::lut");
// thread Q's compact indices Q + 4 i: the LUT row of each small-integer one (-1: searched), and the searched i's
constexpr int kIntOf[4][6] = {{-1, 2, -1, 6, -1, -1}, {-1, 3, 5, -1, -1, -1}, {0, 4, -1, -1, -1, -1},
                              {1, -1, -1, 7, -1, -1}};
constexpr int kNSearched[4] = {4, 4, 3, 3};
constexpr int kSearched[4][4] = {{0, 2, 4, 5}, {0, 3, 4, 5}, {2, 3, 4, 0}, {1, 2, 4, 0}};
constexpr bool int_tables_agree() {
  for (int q = 0; q < 4; ++q) {
    int ns = 0;
    for (int i = 0; i < 6; ++i) {
      const int ci = q + 4 * i;
      const int want = ci < kCompactSlots ? int_slot(ci) : -1;
      if (kIntOf[q][i] != want) return false;
      if (ci < kCompactSlots && want < 0) {
        if (ns >= 4 || kSearched[q][ns] != i) return false;
        ++ns;
      }
    }
    if (ns != kNSearched[q]) return false;
  }
  return true;
}
static_assert(int_tables_agree(), "kIntOf / kSearched must follow kIntCompact and kCompactSlot");

// thread Q's share of a compact row (fd_internal.h: 14 f32 words, then 8 byte slots): compact slots Q, Q + 4, ...
// into v[0..5], the byte slots as the f32 of their integer (exactly the value the feature kernel computed)
template <int Q>
__device__ __forceinline__ void load_compact(const float* __restrict__ xr, float (&v)[16]) {
  const unsigned long long ib = *reinterpret_cast<const unsigned long long*>(xr + 14);
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    const int ci = Q + 4 * i;
    if (ci >= kCompactSlots) {
      v[i] = 0.f;
    } else if (int_slot(ci) >= 0) {
      v[i] = (float)(unsigned)((ib >> (8 * int_slot(ci))) & 0xFFull);
    } else {
      v[i] = xr[compact_word(ci)];
    }
  }
}

// Split rows (features.hip Prep32 / RowA / RowB): thread Q's compact slots Q, Q + 4, ... from the slot pass's RowA
// (card-independent) and the bucket pass's RowB (card-dependent). The derived features' positions 41..46 follow
// FeatureProcessor's conditional order (feature_processor.py:330-363, write_vector): [amount_sqrt if amount > 0,
// amount / user average if that average > 0, hourly velocity ratio if the 24 h count > 0, combined device-IP risk,
// business hours, late night], the k-th present one at 41 + k, zero after. The values are RowA / RowB's f32 as stored.
template <int Q>
__device__ __forceinline__ void load_split(const uint4* __restrict__ ra, const uint4* __restrict__ rb,
                                           float (&v)[16]) {
  const uint4 a0 = ra[0], a1 = ra[1], b0 = rb[0], b1 = rb[1];
  const unsigned fa = a1.w >> 24;                   // RowA flags
  const int na = (fa & 1u) ? 1 : 0;                 // amount > 0
  const int nu = ((b1.z >> 8) & 1u) ? 1 : 0;        // user average > 0
  const int nc = ((b1.y >> 8) & 0xFFu) ? 1 : 0;     // 24 h count > 0 (its byte: clip10 of an integer)
  const int n2 = na + nu + nc;
  auto byte = [](unsigned w, int k) { return (float)((w >> (8 * k)) & 0xFFu); };
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    const int ci = Q + 4 * i;
    float x = 0.f;
    switch (ci) {  // compile-time per unrolled i (fd_internal.h kCompactSlot order)
      case 0: x = __uint_as_float(a0.x); break;   // 0 amount
      case 1: x = __uint_as_float(a0.y); break;   // 1 amount_log
      case 2: x = byte(a1.w, 0); break;           // 5 hour
      case 3: x = byte(a1.w, 1); break;           // 6 day of week
      case 4: x = byte(a1.w, 2); break;           // 7 weekend
      case 5: x = byte(b1.y, 0); break;           // 14 1 h count
      case 6: x = byte(b1.y, 1); break;           // 15 24 h count
      case 7: x = __uint_as_float(b0.x); break;   // 16 24 h amount
      case 8: x = __uint_as_float(b0.y); break;   // 17 user average
      case 9: x = byte(b1.y, 2); break;           // 19 account age
      case 10: x = __uint_as_float(a0.w); break;  // 21 merchant fraud rate
      case 11: x = __uint_as_float(a1.x); break;  // 23 merchant risk
      case 12: x = byte(b1.y, 3); break;          // 26 new device
      case 13: x = __uint_as_float(a1.y); break;  // 27 IP risk
      case 14: x = __uint_as_float(b0.z); break;  // 31 1 h amount
      case 15: x = byte(b1.z, 0); break;          // 32 5 min count
      default:
        if (ci < kCompactSlots) {  // 41 + k: the k-th present derived feature
          const int k = ci - 16;
          const float first = (na && k == 0) ? __uint_as_float(a0.z)
                                             : ((nu && k == na) ? __uint_as_float(b0.w) : __uint_as_float(b1.x));
          const int t = k - n2;  // past the conditional three: combined risk, business, late night
          x = k < n2 ? first
                     : (t == 0 ? __uint_as_float(a1.z)
                               : (t == 1 ? ((fa & 2u) ? 1.f : 0.f) : (t == 2 ? ((fa & 4u) ? 1.f : 0.f) : 0.f)));
        }
        break;
    }
    v[i] = x;
  }
}

// CS: the bin tile holds the varying slots only, slot Q + 4 i at its compact index (the dense layout's node words name
// it), else every feature at its own index
template <int Q, int L, bool CS = false>
__device__ __forceinline__ void bin_compact_pass(const EnsArgs& a, const float (&v)[16], uint16_t* Xs,
                                                 int txn, int f0, int f1, bool glob, uint32_t tl, int o0,
                                                 int& anynan, uint32_t lut) {
  constexpr int NV = (kCompactSlots - Q + 3) / 4;  // compact slots Q, Q + 4, ... below kCompactSlots
  constexpr int NS = kNSearched[Q];
  // the small-integer slots: one LDS lookup each
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int ks = kIntOf[Q][i];
    if (ks < 0) continue;
    const int f = kCompactSlot[Q + 4 * i];
    if (!(f >= f0 && f < f1 && f < a.nf)) continue;  // wave-uniform
    const float x = v[i];
    uint16_t bin;
    if (x != x) {
      anynan = 1;
      bin = (uint16_t)0xFFFFu;
    } else if (x >= 0.f && x < (float)kLutN && x == truncf(x)) {
      bin = lds_load<uint16_t>(lut + (uint32_t)(ks * kLutN + (int)x) * 2u);
    } else {  // #{t <= x} over the feature's merged table in global memory: binary lifting with a fixed trip count
      // (tables hold < 2^16 thresholds), straight-line code, so this loop over i stays unrolled and v[] in registers
      // (CS: the slot's bounds from cthr as below — EnsArgs::cthr says why)
      const int o = CS ? a.cthr[2 * (Q + 4 * i)] : a.thr_off[f];
      const int cnt = (CS ? a.cthr[2 * (Q + 4 * i) + 1] : a.thr_off[f + 1]) - o;
      int pos = 0;
#pragma unroll
      for (int st = 1 << 15; st > 0; st >>= 1)
        if (pos + st <= cnt && a.thr[o + pos + st - 1] <= x) pos += st;
      bin = (uint16_t)pos;
    }
    const int at = CS ? Q + 4 * i : f;
    Xs[(at >> 1) * 512 + txn * 2 + (at & 1)] = bin;
  }
  // the others: binary lifting in lockstep groups of L
#pragma unroll
  for (int g0 = 0; g0 < NS; g0 += L) {
    float vv[L];
    int o[L], cnt[L], pos[L];
    bool act[L];
    int steps = 0;
#pragma unroll
    for (int k = 0; k < L; ++k) {
      const int i = kSearched[Q][g0 + k < NS ? g0 + k : 0];
      const int f = kCompactSlot[Q + 4 * i];
      act[k] = g0 + k < NS && f >= f0 && f < f1 && f < a.nf;
      vv[k] = act[k] ? v[i] : 0.f;  // v[i]: compact slot Q + 4 i of the row
      o[k] = act[k] ? (CS ? a.cthr[2 * (Q + 4 * i)] : a.thr_off[f]) : o0;
      cnt[k] = act[k] ? (CS ? a.cthr[2 * (Q + 4 * i) + 1] : a.thr_off[f + 1]) - o[k] : 0;
      pos[k] = 0;
      steps = max(steps, lift_steps(cnt[k]));
    }
    search_lockstep<L>(vv, o, cnt, pos, steps, glob, tl, o0, a.thr);
#pragma unroll
    for (int k = 0; k < L; ++k) {
      const int i = kSearched[Q][g0 + k < NS ? g0 + k : 0];
      const int f = kCompactSlot[Q + 4 * i];
      if (act[k]) {
        const bool nan = vv[k] != vv[k];
        anynan |= nan ? 1 : 0;
        const int at = CS ? Q + 4 * i : f;
        Xs[(at >> 1) * 512 + txn * 2 + (at & 1)] = nan ? (uint16_t)0xFFFFu : (uint16_t)pos[k];
      }
    }
  }
}

// VD != 0 (D = 8): the chunks hold contracted trees of their own depths (walk_pack_var), leaf rows of 2^a.ldepth
template <int D, int OUT, bool WIDE, bool LUT = true, int VD = 0>
__global__ void __launch_bounds__(kEnsWG) ensemble_kernel(EnsArgs a) {
  // LUT: the small-integer slots binned through their table, the only form left since the option without it went
  // (DESIGN §3). The parameter stays: the benchmark and the committed counter profiles name the kernels by their
  // symbols, fd::(anonymous namespace)::ensemble_kernel<8, OUT, WIDE, true> among them.
  static_assert(LUT, "ensemble_kernel: only the small-integer table's instantiations exist");
  constexpr int kCHA = EnsCfg<WIDE>::CHA, kCHB = EnsCfg<WIDE>::CHB;
  constexpr uint32_t kEnsBuf = EnsCfg<WIDE>::BUF;
  constexpr int TPGA = kCHA / 4, TPGB = kCHB / 4;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const uint32_t sdyn = (uint32_t)(size_t)((lds_char*)smem);
  const uint32_t s0 = (sdyn + 1023u) & ~1023u;
  char* const lbase = smem + (s0 - sdyn);
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int gg = __builtin_amdgcn_readfirstlane(wave >> 2);  // wave-uniform: scalar addressing
  const int txn = ((wave & 3) << 6) + lane;
  const uint32_t lane4 = s0 + (uint32_t)txn * 4u;
  // VD 3 (dense chunks): the 22-slot bin tile, a chunk table behind each buffer, tiles of kDenseSMax bundles
  constexpr bool DENSE = VD == 3;
  constexpr uint32_t kBufStep = kEnsBuf + (DENSE ? kDenseTab : 0u), kTileBytes = DENSE ? kDenseTile : kEnsTile;
  const uint32_t bufA = s0 + (DENSE ? ens_xs_bytes(kCompactSlots) : ens_xs_bytes(a.nf)), bufB = bufA + kBufStep;
  const uint32_t tile0 = bufB + kBufStep, tile1 = tile0 + kTileBytes;
  const uint32_t accA = tile1 + kTileBytes, accB = accA + kTile * 4;
  const uint32_t flags = accB + kTile * 8, owner_cnt = flags + 64;
  const int64_t row = (int64_t)blockIdx.x * kTile + txn;
  const bool valid = row < a.n;
  const int nA = a.n_chunks[0], G = nA + a.n_chunks[1];
  const int NL = VD ? 1 << a.ldepth : 1 << D;  // leaf values per tree row

#ifdef FD_FOREST_PROFILE
  unsigned long long pr_top = 0, pr_walk = 0, pr_sync = 0, pr_dma = 0, pr_st[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#endif
  FD_ESTAMP(pr_t0);
#ifdef FD_FOREST_PROFILE
  const unsigned long long pr_rt0 = __builtin_amdgcn_s_memrealtime();  // 100 MHz, one clock for the whole GPU
#endif
  // every kernel argument the prologue branches on or addresses with, in ONE round of scalar loads: left to itself
  // the compiler issues them lazily, one dependent kernel-argument round trip per branch (five before the row loads
  // went out). The empty asm needs them all in SGPRs at this point; later reads of the same fields reuse them.
  {
    const int k_prio = a.prio, k_compact = a.compact, k_npass = a.n_pass, k_vec4 = a.vec4, k_ld = a.ld;
    const unsigned long long k_pg = a.pass_global;
    const float* k_x = a.X;
    const char* k_img = a.img;
    const int k_i0 = a.img_off[0], k_i1 = a.img_off[1], k_f1 = a.pass_f[1];
    asm volatile("" ::"s"(k_prio), "s"(k_compact), "s"(k_npass), "s"(k_vec4), "s"(k_ld), "s"(k_pg), "s"(k_x),
                 "s"(k_img), "s"(k_i0), "s"(k_i1), "s"(k_f1), "s"(nA), "s"(G), "s"(a.n));
  }
  // above the feature kernels of the next micro-batch that share the CU in the pipelined stream (priority 0):
  // this kernel is the stream's critical path, theirs is latency-bound with slack
  if (a.prio) __builtin_amdgcn_s_setprio(2);
  int anynan = 0;
  const bool early0 = G > 0 && a.n_pass == 1 && (a.pass_global & 1ull) != 0;
  {
    uint16_t* Xs = reinterpret_cast<uint16_t*>(lbase);
    const int q = __builtin_amdgcn_readfirstlane(tid >> 8);  // wave-uniform: the four threads sharing `txn`
    const int fq = q * 16;
    // (1) raw values: thread (q, txn) loads features [16 q, 16 q + 16) of its row in one go (all loads in
    // flight together) and keeps them in registers until they are binned
    // compact mode: thread q's share of the pipeline's compact row, slots q, q + 4, ... (6, 6, 5, 5 of the 22) in
    // v[0..5] — the same registers as the full row's 16 (one value array live through the passes, not two: 54
    // VGPRs, the bucket kernel's wave fits beside the ensemble's four per SIMD); the constant slots' bins straight
    // away
    float v[16];
    if (valid && a.compact == 2) {  // split rows: RowA [n], then RowB [n]
      const uint4* ra = reinterpret_cast<const uint4*>(a.X) + 2 * row;
      const uint4* rb = reinterpret_cast<const uint4*>(a.X) + 2 * (a.n + row);
      switch (q) {  // wave-uniform
        case 0: load_split<0>(ra, rb, v); if (!DENSE) bin_compact_constants<0>(a, Xs, txn); break;
        case 1: load_split<1>(ra, rb, v); if (!DENSE) bin_compact_constants<1>(a, Xs, txn); break;
        case 2: load_split<2>(ra, rb, v); if (!DENSE) bin_compact_constants<2>(a, Xs, txn); break;
        default: load_split<3>(ra, rb, v); if (!DENSE) bin_compact_constants<3>(a, Xs, txn); break;
      }
    } else if (valid && a.compact) {
      const float* xr = a.X + row * (int64_t)kCompactWidth;
      switch (q) {  // wave-uniform
        case 0: load_compact<0>(xr, v); if (!DENSE) bin_compact_constants<0>(a, Xs, txn); break;
        case 1: load_compact<1>(xr, v); if (!DENSE) bin_compact_constants<1>(a, Xs, txn); break;
        case 2: load_compact<2>(xr, v); if (!DENSE) bin_compact_constants<2>(a, Xs, txn); break;
        default: load_compact<3>(xr, v); if (!DENSE) bin_compact_constants<3>(a, Xs, txn); break;
      }
    } else if (!DENSE && valid) {  // (the dense kernel's rows are compact or split: its tile has no 64 slots)
      const float* xr = a.X + row * (int64_t)a.ld;
      const int ncopy = a.ld < a.nf ? a.ld : a.nf;
      if (a.vec4 && fq + 16 <= ncopy) {
        const float4* x4 = reinterpret_cast<const float4*>(xr + fq);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const float4 t = x4[k];
          v[4 * k] = t.x;
          v[4 * k + 1] = t.y;
          v[4 * k + 2] = t.z;
          v[4 * k + 3] = t.w;
        }
      } else {
#pragma unroll
        for (int k = 0; k < 16; ++k) v[k] = fq + k < ncopy ? xr[fq + k] : __builtin_nanf("");  // missing: NaN
      }
    }
    // pass 0's table image goes out by LDS-DMA now, beside the row loads (it lands while they are in flight); every
    // search in global memory instead (engine option ensemble_bin_global): nothing staged, so chunk 0's DMA goes out
    if (a.n_pass > 0 && !(a.pass_global & 1ull))
      stage_pieces(a.img + a.img_off[0], bufA, a.img_off[1] - a.img_off[0], kEnsWG / 64, wave);
    if (early0)
      stage_pieces<DENSE>(nA > 0 ? a.nodes[0] : a.nodes[1], bufA, nA > 0 ? a.stride[0] : a.stride[1], kEnsWG / 64, wave,
                          bufA + kEnsBuf);
#ifdef FD_FOREST_PROFILE
    pr_st[0] = __builtin_amdgcn_s_memtime();
#endif
    // compact mode: the small-integer slots' bin table into the accumulator area (unused until the chunk loop)
    // (published by the first pass's staging barrier: no barrier of its own)
    if (a.compact && tid < kIntSlots * kLutN / 2)
      lds_store<uint32_t>(accA + (uint32_t)tid * 4u, reinterpret_cast<const uint32_t*>(a.lut)[tid]);
    // (2) per pass: stage its tables, then bin this thread's features of the pass kLock at a time (independent
    // searches in lockstep, so kLock LDS reads are in flight per step) into the u16 tile
    constexpr int kLock = 4;  // 8 measured slower (bank conflicts of the diverging searches, not latency)
    for (int p = 0; p < a.n_pass; ++p) {
      const int f0 = a.pass_f[p], f1 = a.pass_f[p + 1];
      const bool glob = (a.pass_global >> p) & 1ull;
      const int o0 = a.thr_off[f0];
      const uint32_t tl = bufA;  // this pass's tables: bufA + bufB + the tiles (free until chunk 0 is staged)
      if (!glob) {  // the pass's image (element g at word g + g / 32, thr_pad) in LDS: DMA, then publish
        if (p > 0)
          stage_pieces(a.img + a.img_off[p], bufA, a.img_off[p + 1] - a.img_off[p], kEnsWG / 64, wave);
        dma_wait();
        __syncthreads();
      } else if (a.compact && p == 0) {
        __syncthreads();  // the small-integer table
      }
#ifdef FD_FOREST_PROFILE
      if (p < 3) pr_st[1 + 2 * p] = __builtin_amdgcn_s_memtime();
#endif
      if (valid && a.compact) {
        switch (q) {
          case 0: bin_compact_pass<0, kLock, DENSE>(a, v, Xs, txn, f0, f1, glob, tl, o0, anynan, accA); break;
          case 1: bin_compact_pass<1, kLock, DENSE>(a, v, Xs, txn, f0, f1, glob, tl, o0, anynan, accA); break;
          case 2: bin_compact_pass<2, kLock, DENSE>(a, v, Xs, txn, f0, f1, glob, tl, o0, anynan, accA); break;
          default: bin_compact_pass<3, kLock, DENSE>(a, v, Xs, txn, f0, f1, glob, tl, o0, anynan, accA); break;
        }
      } else if (!DENSE && valid) {
#pragma unroll
        for (int kk = 0; kk < 16; kk += kLock) {
          const int fb = fq + kk;
          if (fb + kLock - 1 < f0 || fb >= f1) continue;  // wave-uniform
          float vv[kLock];
          int o[kLock], cnt[kLock], pos[kLock];
          bool act[kLock];
          int steps = 0;
#pragma unroll
          for (int k = 0; k < kLock; ++k) {
            const int f = fb + k;
            act[k] = f >= f0 && f < f1;
            vv[k] = act[k] ? v[kk + k] : 0.f;
            o[k] = act[k] ? a.thr_off[f] : o0;
            cnt[k] = act[k] ? a.thr_off[f + 1] - o[k] : 0;
            pos[k] = 0;
            steps = max(steps, lift_steps(cnt[k]));
          }
          // bin = #{t <= v} by binary lifting, as bin_of; branch-free (clamped index + select), so the four
          // reads of a step issue back to back
          if (!glob) {
            for (int st = steps; st > 0; st >>= 1) {
              float t[kLock];
#pragma unroll
              for (int k = 0; k < kLock; ++k) {
                const int np = pos[k] + st;
                const int idx = np <= cnt[k] ? np - 1 : 0;
                t[k] = lds_load<float>(tl + (uint32_t)thr_pad(o[k] - o0 + idx) * 4u);
              }
#pragma unroll
              for (int k = 0; k < kLock; ++k) {
                const int np = pos[k] + st;
                pos[k] = (np <= cnt[k] && t[k] <= vv[k]) ? np : pos[k];
              }
            }
          } else {
            for (int st = steps; st > 0; st >>= 1) {
              float t[kLock];
#pragma unroll
              for (int k = 0; k < kLock; ++k) {
                const int np = pos[k] + st;
                t[k] = a.thr[o[k] + (np <= cnt[k] ? np - 1 : 0)];
              }
#pragma unroll
              for (int k = 0; k < kLock; ++k) {
                const int np = pos[k] + st;
                pos[k] = (np <= cnt[k] && t[k] <= vv[k]) ? np : pos[k];
              }
            }
          }
#pragma unroll
          for (int k = 0; k < kLock; ++k) {
            const int f = fb + k;
            if (act[k]) {
              const bool nan = vv[k] != vv[k];
              anynan |= nan ? 1 : 0;
              Xs[(f >> 1) * 512 + txn * 2 + (f & 1)] = nan ? (uint16_t)0xFFFFu : (uint16_t)pos[k];
            }
          }
        }
      }
      __syncthreads();  // the staged tables are overwritten by the next pass / chunk 1
#ifdef FD_FOREST_PROFILE
      if (p < 3) pr_st[2 + 2 * p] = __builtin_amdgcn_s_memtime();
#endif
    }
  }
  // chunk 0 (the tables are dead): forest A's first, or B's when A is absent (dense: stride is its length)
  if (G > 0 && !early0)
    stage_pieces<DENSE>(nA > 0 ? a.nodes[0] : a.nodes[1], bufA, nA > 0 ? a.stride[0] : a.stride[1], kEnsWG / 64, wave,
                        bufA + kEnsBuf);
  if (gg == 0) {
    lds_store<float>(accA + txn * 4, a.base_margin);
    lds_store<double>(accB + txn * 8, 0.0);
  }
  if (tid == 0) lds_store<uint32_t>(owner_cnt, 0u);
  dma_wait();  // chunk 0 (published by tile_any's barrier)
  const bool tile_nan = tile_any(anynan, reinterpret_cast<uint32_t*>(lbase + (flags - s0)), kEnsWG / 64);

  // Iteration g: the owner tree group (0, or (g - 1) & 3 with the rotating schedule) sums chunk g-1 (leaf indices from tile[(g-1)&1], values
  // from its LDS buffer), waits until all four of its waves are done reading that buffer (LDS counter),
  // then stages chunk g+1 into it; every wave walks chunk g and stores its packed leaf indices to
  // tile[g&1]; the owners complete their DMA; the barrier publishes chunk g+1 and tile[g&1].
  FD_ESTAMP(pr_t1);
  for (int g = 0; g < G; ++g) {
    FD_ESTAMP(q0);
    const bool owner = gg == (a.owner_fixed ? 0 : ((g - 1) & 3));
    const uint32_t cur = (g & 1) ? bufB : bufA, tw = (g & 1) ? tile1 : tile0;
    // dense: words 0..3 of this chunk's table — its tree and bundle counts, the next chunk's offset and length in
    // KiB, the groups' bundle counts — in SGPRs
    uint32_t th1 = 0, th2 = 0, th3 = 0;
    if (DENSE) {
      const u32x4 h = lds_load<u32x4>(cur + kEnsBuf);
      th1 = __builtin_amdgcn_readfirstlane(h.y);
      th2 = __builtin_amdgcn_readfirstlane(h.z);
      th3 = __builtin_amdgcn_readfirstlane(h.w);
    }
    if (owner) {
      if (g > 0) {
        const int c = g - 1;
        const uint32_t bp = (c & 1) ? bufB : bufA, tp = (c & 1) ? tile1 : tile0;
        if (DENSE) {
          if (c < nA) owner_sum_dense<float>(bp, bp + kEnsBuf, tp, accA, txn);
          else owner_sum_dense<double>(bp, bp + kEnsBuf, tp, accB, txn);
        } else if (c < nA) owner_sum<D, TPGA, kCHA, float>(bp, tp, accA, txn, NL);
        else owner_sum<D, TPGB, kCHB, double>(bp, tp, accB, txn, NL);
        // the leaf reads of all four owner waves are complete before any of them overwrites the buffer
        if (lane == 0)
          __hip_atomic_fetch_add(reinterpret_cast<uint32_t*>(lbase + (owner_cnt - s0)), 1u, __ATOMIC_RELAXED,
                                 __HIP_MEMORY_SCOPE_WORKGROUP);
        while (__hip_atomic_load(reinterpret_cast<uint32_t*>(lbase + (owner_cnt - s0)), __ATOMIC_RELAXED,
                                 __HIP_MEMORY_SCOPE_WORKGROUP) < 4u * (uint32_t)g)
          __builtin_amdgcn_s_sleep(1);
      }
      if (g + 1 < G) {
        const int h = g + 1, fb = h >= nA ? 1 : 0;
        const uint32_t nb = (g & 1) ? bufA : bufB;
        if (DENSE) {  // forest B's first chunk by the arguments, any other by this chunk's table
          if (h == nA) stage_pieces<true>(a.nodes[1], nb, a.stride[1], 4, wave & 3, nb + kEnsBuf);
          else stage_pieces<true>(a.nodes[fb] + ((size_t)th1 << 10), nb, (int)(th2 << 10), 4, wave & 3, nb + kEnsBuf);
        } else {
          stage_pieces(a.nodes[fb] + (size_t)(fb ? h - nA : h) * a.stride[fb], nb, a.stride[fb], 4, wave & 3);
        }
      }
    }
    FD_ESTAMP(q1);
    if (DENSE) {
      if (g < nA) walk_dense<TPGA>(cur, cur + kEnsBuf, tw, gg, txn, lane4, tile_nan, th3);
      else walk_dense<TPGB>(cur, cur + kEnsBuf, tw, gg, txn, lane4, tile_nan, th3);
    } else {
      unsigned long long w;
      if (VD)
        w = g < nA ? walk_pack_var<VD, TPGA>(cur, gg, lane4, tile_nan)
                   : walk_pack_var<VD, TPGB>(cur, gg, lane4, tile_nan);
      else
        w = g < nA ? walk_pack<D, TPGA>(cur, gg, lane4, tile_nan) : walk_pack<D, TPGB>(cur, gg, lane4, tile_nan);
      lds_store<unsigned long long>(tw + (uint32_t)(gg * kTile + txn) * 8u, w);
    }
    FD_ESTAMP(q2);
    if (owner) dma_wait();
#ifdef FD_FOREST_PROFILE
    const unsigned long long q2d = __builtin_amdgcn_s_memtime();
#endif
    __syncthreads();
#ifdef FD_FOREST_PROFILE
    const unsigned long long q3 = __builtin_amdgcn_s_memtime();
    pr_top += q1 - q0;
    pr_walk += q2 - q1;
    pr_dma += q2d - q2;
    pr_sync += q3 - q2;
#endif
  }
  if (G > 0 && gg == (a.owner_fixed ? 0 : ((G - 1) & 3))) {
    const int c = G - 1;
    const uint32_t bp = (c & 1) ? bufB : bufA, tp = (c & 1) ? tile1 : tile0;
    if (DENSE) {
      if (c < nA) owner_sum_dense<float>(bp, bp + kEnsBuf, tp, accA, txn);
      else owner_sum_dense<double>(bp, bp + kEnsBuf, tp, accB, txn);
    } else if (c < nA) owner_sum<D, TPGA, kCHA, float>(bp, tp, accA, txn, NL);
    else owner_sum<D, TPGB, kCHB, double>(bp, tp, accB, txn, NL);
  }
  __syncthreads();
#ifdef FD_FOREST_PROFILE
  if (lane == 0 && blockIdx.x < 256) {
    unsigned long long* o = g_eprof + (size_t)a.prof_slot * 256 * 16 * 16 + ((size_t)blockIdx.x * 16 + wave) * 16;
    for (int k = 0; k < 7; ++k) o[6 + k] = pr_st[k] ? pr_st[k] - pr_t0 : 0;
    o[0] = pr_t1 - pr_t0;
    o[1] = pr_top;
    o[2] = pr_walk;
    o[3] = pr_sync;
    o[13] = pr_dma;  // of pr_sync: the owner waves' wait for their chunk DMA (0 for the other waves)
    o[4] = pr_t0;
    o[5] = __builtin_amdgcn_s_memtime();
    o[14] = pr_rt0;
    o[15] = __builtin_amdgcn_s_memrealtime();
    if (wave == 0 && (blockIdx.x & 63) == 0) {
      unsigned long long* c = g_eclk + ((size_t)a.clk_slot * 4 + (blockIdx.x >> 6)) * 4;
      c[0] = pr_t0;
      c[1] = o[5];
      c[2] = pr_rt0;
      c[3] = o[15];
    }
  }
#endif
  if (gg != 0 || !valid) return;

  // epilogue: the two models' probabilities, then the blend (blend_row.h)
  double pa, pb;
  {
    const float mg = lds_load<float>(accA + txn * 4);  // XGBoost common::Sigmoid in f32
    const float xm = fminf(-mg, 88.7f);
    const float denom = expf(xm) + 1.0f + 1e-16f;
    pa = (double)(1.0f / denom);
  }
  {
    const double d = lds_load<double>(accB + txn * 8);  // sklearn score -> decision -> 1/(1+exp(s))
    const double qd = (a.if_denom != 0.0) ? d / a.if_denom : 1.0;
    const double score = pow(2.0, -qd);
    const double decision = -score - a.if_offset;
    pb = 1.0 / (1.0 + exp(decision));
  }
  if (OUT == 2) {  // one forest: its probability (forest_predict semantics) and, when asked, its raw score
    a.fp[row] = nA > 0 ? pa : pb;
    if (a.mp) a.mp[row] = nA > 0 ? (double)lds_load<float>(accA + txn * 4) : lds_load<double>(accB + txn * 8);
    return;
  }
  double raw[FD_MAX_MODELS];  // the two present models at their blend positions (selects: no scratch)
#pragma unroll
  for (int m = 0; m < FD_MAX_MODELS; ++m) raw[m] = m == a.pos[0] ? pa : (m == a.pos[1] ? pb : 0.0);
  if (a.mp) {
    a.mp[(size_t)a.mcol[0] * a.n + row] = pa;
    a.mp[(size_t)a.mcol[1] * a.n + row] = pb;
  }
  double fp, conf;
  uint8_t dec, risk;
  blend_row(a.blend, raw, fp, conf, dec, risk);
  if (OUT == 0) {
    a.fp[row] = fp;
    if (a.conf) a.conf[row] = conf;
    if (a.dec) a.dec[row] = dec;
    if (a.risk) a.risk[row] = risk;
  } else {
    ResultRecord r;
    r.fraud_prob = fp;
    r.confidence = conf;
    r.seq = a.rec[row].seq;
    r.decision = dec;
    r.risk = risk;
    r.pad = 0;
    a.res[row] = r;
  }
}

template <int OUT, bool WIDE>
const void* pick_ensemble(int D) {
  switch (D) {
    case 1: return (const void*)ensemble_kernel<1, OUT, WIDE>;
    case 2: return (const void*)ensemble_kernel<2, OUT, WIDE>;
    case 3: return (const void*)ensemble_kernel<3, OUT, WIDE>;
    case 4: return (const void*)ensemble_kernel<4, OUT, WIDE>;
    case 5: return (const void*)ensemble_kernel<5, OUT, WIDE>;
    case 6: return (const void*)ensemble_kernel<6, OUT, WIDE>;
    case 7: return (const void*)ensemble_kernel<7, OUT, WIDE>;
    case 8: return (const void*)ensemble_kernel<8, OUT, WIDE>;
    default: return nullptr;
  }
}

// (the instantiations without the small-integer table, round 5's A/B, were removed with the option: DESIGN §3)
const void* pick_ensemble(int out, bool wide, int D) {
  if (wide) return out == 1 ? pick_ensemble<1, true>(D) : out == 2 ? pick_ensemble<2, true>(D) : pick_ensemble<0, true>(D);
  return out == 1 ? pick_ensemble<1, false>(D) : out == 2 ? pick_ensemble<2, false>(D) : pick_ensemble<0, false>(D);
}

// the variable-depth instantiations (contracted chunks; blended columns or route records only: compact rows are the
// pipelined stream's), the kernel's VD: 1 per tree / 2 per wave (walk_pack_var), 3 the dense chunk stream
template <int VD>
const void* pick_ensemble_var(int out, bool wide) {
  if (wide)
    return out == 1 ? (const void*)ensemble_kernel<8, 1, true, true, VD>
                    : (const void*)ensemble_kernel<8, 0, true, true, VD>;
  return out == 1 ? (const void*)ensemble_kernel<8, 1, false, true, VD>
                  : (const void*)ensemble_kernel<8, 0, false, true, VD>;
}
const void* pick_ensemble_var(int out, bool wide, int vd) {
  return vd == 2 ? pick_ensemble_var<2>(out, wide)
                 : vd == 3 ? pick_ensemble_var<3>(out, wide) : pick_ensemble_var<1>(out, wide);
}

}  // namespace

#ifdef FD_FOREST_PROFILE
// n words from the start of the buffers: slot k's profile at word k * 256 * 16 * 16; *next_slot (if given) = the slot
// the next launch writes (so the most recent launch wrote (next_slot + kEprofSlots - 1) % kEprofSlots)
extern "C" __attribute__((visibility("default"))) int fd_debug_ens_profile(unsigned long long* out, int n) {
  return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_eprof), sizeof(unsigned long long) * (size_t)n);
}
extern "C" __attribute__((visibility("default"))) int fd_debug_ens_profile_next(void) { return g_eprof_next; }
extern "C" __attribute__((visibility("default"))) int fd_debug_ens_clock(unsigned long long* out, int n) {
  return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_eclk), sizeof(unsigned long long) * (size_t)n);
}
extern "C" __attribute__((visibility("default"))) int fd_debug_ens_clock_next(void) { return g_eclk_next; }
#endif

namespace {
struct Pair {
  int sa = -1, sb = -1, pa = -1, pb = -1, ma = -1, mb = -1;
};

// The fused kernel applies (and its joint plan is built) when the batch is large and the present models are
// exactly one XGBoost and one IsolationForest in engine slots.
bool select_pair(Engine& e, const ModelSet& ms, int64_t n, Pair& q) {
  if (!e.ensemble_on || e.forest_variant != 0 || n <= 0) return false;
  if ((n + kTile - 1) / kTile < kSplitTiles) return false;  // latency batches: the tree-split path
  int k = 0;
  for (int m = 0; m < ms.n_models(); ++m) {
    if (!ms.has(m)) continue;
    const int s = ms.slots[m];
    if (s < 0 || s >= kMaxSlots || !e.forests[s].loaded || e.forests[s].sparse_only) return false;
    const int kind = e.forests[s].kind;
    if (kind == FD_FOREST_XGB_BINARY_LOGISTIC && q.sa < 0) {
      q.sa = s;
      q.pa = k;
      q.ma = m;
    } else if (kind == FD_FOREST_SKLEARN_IFOREST && q.sb < 0) {
      q.sb = s;
      q.pb = k;
      q.mb = m;
    } else {
      return false;
    }
    ++k;
  }
  if (q.sa < 0 || q.sb < 0) return false;
  const bool wide = want_wide(e);
  if (!plan_current(e, e.ens, q.sa, q.sb, wide, e.ens_contract) &&
      !build_plan(e, e.ens, q.sa, q.sb, wide, e.ens_contract))
    return false;
  return true;
}

void plan_args(const EnsemblePlan& P, const float* dX, int64_t n, int32_t ld, bool owner_fixed, EnsArgs& a) {
  a.X = dX;
  a.n = n;
  a.ld = ld;
  a.nf = P.nf;
  a.thr = P.thr.as<const float>();
  FD_REQUIRE(P.nf <= kMaxFeatures, FD_ERR_UNSUPPORTED, "ensemble: more than 64 features");
  for (int f = 0; f <= P.nf; ++f) a.thr_off[f] = P.h_thr_off[f];
  a.owner_fixed = owner_fixed ? 1 : 0;
  for (int f = 0; f < kMaxFeatures; ++f) a.cbin[f] = f < (int)P.h_cbin.size() ? P.h_cbin[f] : 0;
  for (int c = 0; c < kCompactSlots; ++c) {
    const int f = kCompactSlot[c];
    a.cthr[2 * c] = f < P.nf ? P.h_thr_off[f] : 0;
    a.cthr[2 * c + 1] = f < P.nf ? P.h_thr_off[f + 1] : 0;
  }
  for (size_t k = 0; k < P.h_lut.size() && k < sizeof(a.lut) / sizeof(a.lut[0]); ++k) a.lut[k] = P.h_lut[k];
  a.vec4 = (ld % 4 == 0 && (reinterpret_cast<uintptr_t>(dX) & 15u) == 0) ? 1 : 0;
  const EnsPassSet& ps = P.passes;  // plan_passes
  a.n_pass = (int)ps.f.size() - 1;
  for (int p = 0; p <= a.n_pass; ++p) {
    a.pass_f[p] = ps.f[p];
    a.img_off[p] = ps.img_off[p];
  }
  a.pass_global = ps.glob;
  a.img = P.img.as<const char>();
  for (int q = 0; q < 2; ++q) {
    a.nodes[q] = P.nodes[q].as<const char>();
    a.n_chunks[q] = P.n_chunks[q];
    a.stride[q] = (int)P.stride[q];
  }
  a.base_margin = P.base_margin;
  a.if_offset = P.if_offset;
  a.if_denom = P.if_denominator;
}

// out: 0 blended columns, 1 route result records, 2 the single forest's probability column (a.fp)
bool run_plan(Engine& e, const EnsemblePlan& P, EnsArgs& a, int out, int timing_kind, int vd = 0) {
  const void* fn = vd && out != 2 ? pick_ensemble_var(out, P.wide, vd) : pick_ensemble(out, P.wide, P.D);
  if (!fn) return false;
  const size_t lds = vd == 3 ? ens_lds_dense(P.wide) : ens_lds(P.nf, P.wide);
  FD_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  const int64_t blocks = (a.n + kTile - 1) / kTile;
  Engine::Timed* ev = e.timing ? e.next_event_pair(timing_kind) : nullptr;
  if (ev) FD_HIP(hipEventRecord(ev->a, e.stream));
#ifdef FD_FOREST_PROFILE
  a.prof_slot = g_eprof_next;
  g_eprof_next = (g_eprof_next + 1) % kEprofSlots;
  a.clk_slot = g_eclk_next;
  g_eclk_next = (g_eclk_next + 1) % kEclkSlots;
#endif
  void* args[] = {&a};
  FD_HIP(hipLaunchKernel(fn, dim3((unsigned)blocks), dim3(kEnsWG), args, lds, e.stream));
  if (ev) FD_HIP(hipEventRecord(ev->b, e.stream));
  return true;
}
}  // namespace

bool ensemble_applies(Engine& e, const ModelSet& ms, int64_t n) {
  Pair q;
  return select_pair(e, ms, n, q);
}

bool launch_ensemble(Engine& e, const ModelSet& ms, const ScoreRows& rows, const ScoreOut& out_cols) {
  Pair q;
  if (!select_pair(e, ms, rows.n, q)) return false;
  const int pa = q.pa, pb = q.pb, ma = q.ma, mb = q.mb;
  const int compact = rows.compact;
  EnsArgs a{};
  plan_args(e.ens, rows.X, rows.n, compact ? kCompactWidth : rows.ld, e.ens_owner_fixed, a);
  a.compact = compact;
  if (compact && e.ens_bin_global) {  // one pass, every table searched where it lies (L2), nothing staged
    a.n_pass = 1;
    a.pass_f[0] = 0;
    a.pass_f[1] = e.ens.nf;
    a.pass_global = 1ull;
  }
  a.prio = e.ens_prio ? 1 : 0;
  a.pos[0] = pa;
  a.pos[1] = pb;
  a.mcol[0] = ma;
  a.mcol[1] = mb;
  a.blend = blend_consts(ms);
  a.mp = out_cols.mp;
  a.fp = out_cols.fp;
  a.conf = out_cols.conf;
  a.dec = out_cols.dec;
  a.risk = out_cols.risk;
  a.rec = rows.records;
  a.res = rows.results;
  const int out = rows.results ? 1 : 0;
  FD_REQUIRE(out == 1 || out_cols.fp != nullptr, FD_ERR_INVALID_ARG, "null output");
  // compact / split rows carry the constant slots' values by construction: the contracted chunks and the
  // variable-depth walk, when the contraction shortened any tree; 64-wide rows keep nodes[] and the fixed-depth kernels
  // (the kernel's VD: 1 per tree, 2 per wave, 3 the dense chunk stream of ensemble_contract 3 / 4)
  const int vd = (compact && e.ens.contracted) ? (e.ens.contract >= 3 ? 3 : e.ens.contract == 1 ? 2 : 1) : 0;
  if (vd) {
    for (int k = 0; k < 2; ++k) a.nodes[k] = e.ens.nodes_c[k].as<const char>();
    a.ldepth = e.ens.D;
  }
  if (vd == 3)
    for (int k = 0; k < 2; ++k) {
      a.n_chunks[k] = e.ens.dense_chunks[k];
      a.stride[k] = e.ens.dense_len0[k];  // the first chunk's length: the others' come with the tables
    }
  if (!run_plan(e, e.ens, a, out, FD_TIMING_ENSEMBLE, vd)) return false;
  if (vd) ++e.ens_contract_total;
  e.ens_steps_last = vd ? e.ens.steps_c : e.ens.steps_full;
  e.ens_dense_chunks_last = vd == 3 ? e.ens.dense_chunks[0] + e.ens.dense_chunks[1] : 0;
  return true;
}

bool launch_ensemble_single(Engine& e, int slot, const float* dX, int64_t n, int32_t ld, double* dprob,
                            double* draw, hipStream_t stream) {
  if (!e.ensemble_on || e.forest_variant != 0 || n <= 0) return false;
  if ((n + kTile - 1) / kTile < kSplitTiles) return false;
  if (slot < 0 || slot >= kMaxSlots || !e.forests[slot].loaded || e.forests[slot].sparse_only) return false;
  const bool xgb = e.forests[slot].kind == FD_FOREST_XGB_BINARY_LOGISTIC;
  const int sa = xgb ? slot : -1, sb = xgb ? -1 : slot;
  EnsemblePlan& P = e.ens1[slot];
  const bool wide = want_wide(e);
  if (!plan_current(e, P, sa, sb, wide) && !build_plan(e, P, sa, sb, wide)) return false;
  EnsArgs a{};
  plan_args(P, dX, n, ld, e.ens_owner_fixed, a);
  a.prio = e.ens_prio ? 1 : 0;
  a.fp = dprob;
  a.mp = draw;  // one forest: its raw score (XGBoost f32 margin, IsolationForest f64 path-length sum) or null
  const hipStream_t saved = e.stream;
  if (stream) e.stream = stream;
  bool ok = false;
  try {
    ok = run_plan(e, P, a, 2, xgb ? FD_TIMING_XGB : FD_TIMING_IFOREST);
  } catch (...) {
    e.stream = saved;
    throw;
  }
  e.stream = saved;
  if (ok) ++e.ens_single_total;
  return ok;
}

}  // namespace fd
