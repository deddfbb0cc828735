// mlp_fit_row.h — the counter-based rules of the MLP fit (mlp_fit.hip): the key of an epoch's row order
// and the dropout mask. The kernels and the single-threaded host reference (fd_mlp_fit_ref_host, fd_mlp_fit_batch_host)
// compile these same functions, so both train on the same batches under the same masks, bit for bit. Everything is a
// function of (seed, counter) through key_hash.h's fmix64: nothing depends on a launch shape or on a stream of draws.
#pragma once

#include <cstdint>

#include "key_hash.h"

namespace fd {

constexpr int kMlpFitRows = 16;    // batch rows per tile (the MFMA's 16 columns) = one chunk of the gradient sum
constexpr int kMlpFitWidth = 64;   // the widest layer; the unit stride of a mask array

FD_HD uint64_t mlp_fit_key(uint64_t seed) { return fmix64(seed + 0x9e3779b97f4a7c15ULL); }

// Epoch `epoch`'s sort key of row `row`: the epoch's order is the stable ascending sort of the rows by this key
// (fmix64 is a bijection, so the keys of one epoch are distinct; stable all the same).
FD_HD uint64_t mlp_fit_order_key(uint64_t key, uint32_t epoch, uint32_t row) {
  return fmix64(key ^ (((uint64_t)epoch << 32) | row));
}

// p in [0, 1) -> the threshold a unit's 32-bit draw must reach to be kept: floor(p 2^32); 0 keeps everything
inline uint32_t mlp_fit_threshold(double p) { return (uint32_t)(uint64_t)(p * 4294967296.0); }

// the part of the mask hash that a (global step, hidden layer) pair fixes
FD_HD uint64_t mlp_fit_mask_layer(uint64_t key, uint32_t step, uint32_t layer) {
  return fmix64(~key ^ (((uint64_t)step << 3) | layer));
}
// keep unit `unit` of the batch's row `row` (its position in the batch, not its row id)?
FD_HD bool mlp_fit_keep(uint64_t layer_key, uint32_t row, uint32_t unit, uint32_t thr) {
  return (uint32_t)(fmix64(layer_key ^ (((uint64_t)row << 6) | unit)) >> 32) >= thr;
}

}  // namespace fd
