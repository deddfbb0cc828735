// ensemble_layout.h — what the fused ensemble kernel (ensemble.hip) and its host planner (ensemble_plan.hip) must
// agree on: the chunk geometry, the kernel's LDS layout, the padded threshold images, the ensemble node word and
// the dense chunk table's fields.
#pragma once

#include "fd_internal.h"

namespace fd {

constexpr int kMaxPass = 64;  // binning passes of a plan at most (EnsArgs::pass_f)
constexpr int kLutN = 32;     // the small-integer compact slots' bin table: the bins of the values 0 .. kLutN - 1

// Trees per chunk, by layout: wide 24 XGBoost (TPG 6) / 16 IsolationForest (TPG 4) trees in 48 KiB chunk
// buffers; compact 20 (TPG 5) / 12 (TPG 3) in 40 KiB, which leaves the CU the ~20 KiB of LDS an RCCL kernel
// needs beside the scoring (the sharded step's exchanges co-run with it: with the wide layout they waited for a
// whole scoring launch to end). A chunk in LDS: CH node blocks of 1 KiB (walk_ens link addressing), then the CH
// trees' leaf values [CH][2^D]; its buffer is sized for depth 8: max(CHA x (1 KiB + 1 KiB f32), CHB x (1 KiB +
// 2 KiB f64)).
template <bool WIDE>
struct EnsCfg {
  static constexpr int CHA = WIDE ? 24 : 20;
  static constexpr int CHB = WIDE ? 16 : 12;
  static constexpr uint32_t BUF = (uint32_t)(CHA * (1024 + 256 * 4) > CHB * (1024 + 256 * 8) ? CHA * (1024 + 256 * 4)
                                                                                             : CHB * (1024 + 256 * 8));
};
inline uint32_t ens_buf(bool wide) { return wide ? EnsCfg<true>::BUF : EnsCfg<false>::BUF; }
// trees per chunk of forest k (0: A, the XGBoost model; 1: B, the IsolationForest); a wave walks a quarter of them
inline int ens_chunk_trees(bool wide, int k) {
  return k == 0 ? (wide ? EnsCfg<true>::CHA : EnsCfg<false>::CHA) : (wide ? EnsCfg<true>::CHB : EnsCfg<false>::CHB);
}
constexpr uint32_t kEnsTile = 4u * kTile * 8u;  // leaf indices of one chunk: [tree group][txn] u64, a byte per tree

// The bin tile: u16 bins, two features per 1 KiB row — feature f of transaction t at byte
// (f >> 1) * 1024 + 4 t + 2 (f & 1) — so a node word's bits [15:10] = f >> 1 and bit 1 = f & 1 address it
// with one AND-OR, and the 64 lanes of a read hit 64 distinct banks whatever features they ask for.
__host__ __device__ constexpr uint32_t ens_xs_bytes(int nf) { return (uint32_t)((nf + 1) / 2) * 1024u; }

// LDS bytes of the kernel: Xs | bufA | bufB | tile0 | tile1 | accA (f32) | accB (f64) | flags + owner counter,
// + 1 KiB alignment
inline size_t ens_lds(int nf, bool wide) {
  return (size_t)ens_xs_bytes(nf) + 2 * (size_t)ens_buf(wide) + 2 * (size_t)kEnsTile + kTile * 4 + kTile * 8 + 128 +
         1024;
}

// The dense layout (VD 3: contracted forests on compact / split rows, dense_layout_host): the bin tile holds the 22
// varying slots at their compact indices (11 KiB), each chunk buffer is BUF data bytes + the chunk's 1 KiB table at a
// fixed place behind them, and a leaf-index tile holds kDenseSMax bundles. Xs | bufA + table | bufB + table | tile0 |
// tile1 | accA | accB | flags + owner counter, + 1 KiB alignment: 148,608 B wide, 132,224 B compact, 3 KiB under the
// padded layout's (kDenseSMax 9 would leave 1 KiB, and the two tables take 2).
constexpr uint32_t kDenseTile = (uint32_t)kDenseSMax * kTile * 8u;
// The chunk table (include/fdengine.h fd_dense_layout_host), kDenseTab bytes. Words 0..3: trees | bundles << 8, the
// next chunk's offset and its length in KiB, the four tree groups' bundle counts (a byte each). From kDenseGroupTab:
// per tree group kDenseGroupStride bytes, a kDenseBundleEnt-byte entry per bundle (depth | tile row << 8 | group
// << 16, then six u16 node-block offsets). From kDenseTreeTab: a word per tree, forest order — its leaf-index byte in
// the tile (kDenseTileRow per bundle + its place) | its leaf row's offset << 16.
constexpr uint32_t kDenseTab = 1024, kDenseGroupTab = 64, kDenseTreeTab = 576;
constexpr uint32_t kDenseGroupStride = 128, kDenseBundleEnt = 16, kDenseTileRow = kTile * 8u;
static_assert(kDenseGroupTab + 4 * kDenseGroupStride == kDenseTreeTab &&
                  kDenseSMax * kDenseBundleEnt <= kDenseGroupStride,
              "the groups' bundle entries end where the tree entries begin");
constexpr int kDenseOwnerBias = 0;  // dense_layout_host's owner_bias in the engine's plans
inline size_t ens_lds_dense(bool wide) {
  return (size_t)ens_xs_bytes(kCompactSlots) + 2 * ((size_t)ens_buf(wide) + kDenseTab) + 2 * (size_t)kDenseTile +
         kTile * 4 + kTile * 8 + 128 + 1024;
}

// Staged threshold tables hold element g at word g + g / 32: the binary search's power-of-two strides would
// otherwise put every lane of a step on one LDS bank (up to 32-way conflicts); one pad word per 32 spreads them.
__host__ __device__ __forceinline__ int thr_pad(int g) { return g + (g >> 5); }

// Ensemble node word: j << 16 | (slot >> 1) << 10 | link << 3 | (slot & 1) << 1 | default_left; slot is the bin
// tile's index of the value the node tests (the feature, or its compact index in the dense layout). `link`
// makes the next pair address one AND-OR: for a node at heap slot i above the last split level, link = i (its
// children pair is at byte 8 i of the tree's node block); at the last split level link = i - 2^(D-1), so the
// leaf is 2 link + right. One step is then v_cmp (u16 bin against the word's high half: SDWA) + v_cndmask
// (child) + v_and_or (bin address) + v_and_or (pair address): 4 VALU, 2 LDS reads.
constexpr uint32_t kLinkMask = 0x3F8u;
// heap slot s of a tree with nl = 2^depth leaves
inline uint32_t ens_link(int s, int nl) { return (uint32_t)(s < (nl >> 1) ? s : s - (nl >> 1)); }
inline uint32_t ens_node_word(uint32_t j, uint32_t slot, uint32_t link, bool dleft) {
  return (j << 16) | ((slot >> 1) << 10) | (link << 3) | ((slot & 1u) << 1) | (dleft ? 1u : 0u);
}

}  // namespace fd
