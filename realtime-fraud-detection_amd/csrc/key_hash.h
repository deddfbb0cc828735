// key_hash.h — the one definition of the 64-bit key finaliser and of card ownership. Every table that is probed by
// a card, merchant or aggregate key (features.hip, sink.hip, ingest.hip, snapshot.hip) and the routing of a card to
// its owner GPU (route.hip, snapshot.hip) go through these two functions: a snapshot restored by one and routed by
// another copy would silently drop cards. oracle/route_ref.py restates them independently for the tests.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define FD_HD __host__ __device__ __forceinline__
#else
#define FD_HD inline
#endif

namespace fd {

// murmur3's fmix64
FD_HD uint64_t fmix64(uint64_t k) {
  k ^= k >> 33;
  k *= 0xff51afd7ed558ccdULL;
  k ^= k >> 33;
  k *= 0xc4ceb9fe1a85ec53ULL;
  k ^= k >> 33;
  return k;
}

// Owner GPU of a card among G: the high 32 bits of the mix (the card table's home slot uses the low bits, so the
// owned keys still spread over every slot of the owner's table), multiply-shift range reduction. Key 0 counts as 1,
// the card table's key normalisation (card_slot).
FD_HD unsigned shard_of(uint64_t key, unsigned G) {
  if (key == 0) key = 1;
  return (unsigned)(((fmix64(key) >> 32) * (uint64_t)G) >> 32);
}

}  // namespace fd
