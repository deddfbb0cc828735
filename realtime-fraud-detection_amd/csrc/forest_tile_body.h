// forest_tile_body.h — the body of the tile kernels forest_kernel3 / 4 / 6 (forest.hip), written once. No include
// guard: forest.hip includes it INSIDE each of the three kernels, after `constexpr Layout LAY = ...`, with the
// kernel's parameters (X, n, ld, nf, blob, n_chunks, chunk_stride, leaf_ids, n_trees, thr, thr_off, base_margin,
// if_offset, if_denom, out_prob, out_raw, out_leaf, leaves; a kernel without one of thr / thr_off / leaves declares
// it as a null constant) and template parameters (D, CH, LeafT, KIND) in scope. LDS map and schedule: forest.hip.
//
// The layouts differ in three places, each an `if constexpr` below:
//   prologue  kThreshold copies the raw f32 columns into the tile. The binned layouts replace every value by its
//             bin: the count of the feature's distinct split thresholds that are <= x (branchless binary lifting
//             over the sorted table, staged in LDS when it fits), stored as the u32 word bin << 16 (missing/NaN:
//             0xFFFF << 16). A binned node word is j << 16 | feature * 1024 | default_left, so "x < t_j" is
//             "bin <= j" is ONE unsigned compare word(x) <= node, the feature-row address is
//             (node & 0xFC00) | lane, and a node's two children are one 8-byte pair read: per level one
//             ds_read_b32 (feature) and one ds_read_b64 (children).
//   walk      walk3 / walk4 / walk4 over node-only trees.
//   leaves    from the staged chunk, or (kNodeOnly) from the global [tree][2^D] array `leaves` (L2-resident:
//             0.5 MiB for 500 x depth 8) with all TPG loads in flight together.
// kNodeOnly stages only the CH trees' node words (1 KiB per depth-8 tree instead of 2-3 KiB with the leaves), so
// the same LDS budget stages more trees per chunk: CH = 24 for XGBoost (TPG = 6 independent walks per wave instead
// of 4) and 16 for the f64-leaf IsolationForest (instead of 8). The walk is bound by the LDS round-trip latency of
// its dependent chains, not by LDS cycles (PMC: LDS array ~50 % busy, VALU ~35 %), so more chains per wave is the
// lever.
  constexpr bool kBins = LAY != Layout::kThreshold;
  constexpr bool kNodesOnly = LAY == Layout::kNodeOnly;
  constexpr int TPG = CH / 4;
  constexpr int NL = 1 << D;
  constexpr uint32_t kNodeBytes = kBins ? 4u : 8u;
  constexpr uint32_t TB = (kNodeBytes + (uint32_t)sizeof(LeafT)) << D;  // tree stride when the chunk holds leaves
  extern __shared__ __attribute__((aligned(16))) char smem[];
  // 1 KiB-aligned base: no static LDS in these kernels (so the base is 0); 1 KiB slack reserved anyway
  const uint32_t sdyn = (uint32_t)(size_t)((lds_char*)smem);
  const uint32_t s0 = (sdyn + 1023u) & ~1023u;
  char* const lbase = smem + (s0 - sdyn);
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int gg = wave >> 2;                  // tree group
  const int txn = ((wave & 3) << 6) + lane;  // 0..255 within the tile
  const uint32_t lane4 = s0 + (uint32_t)txn * 4u;
  const uint32_t xbytes = (uint32_t)nf * 1024u;
  const uint32_t bufA = s0 + xbytes, bufB = bufA + (uint32_t)chunk_stride;
  const uint32_t lvA = bufB + (uint32_t)chunk_stride;
  const uint32_t lvB = lvA + CH * kTile * sizeof(LeafT);
  const uint32_t accL = lvB + CH * kTile * sizeof(LeafT);
  const int64_t row = (int64_t)blockIdx.x * kTile + txn;
  const bool valid = row < n;
#ifdef FD_FOREST_PROFILE
  unsigned long long p_walk = 0, p_leaf = 0, p_own = 0, p_sync = 0;
#endif
  FD_PROF_T(p_t0);

  stage_chunk_asm(blob, bufA, chunk_stride, kWG3 / 64);  // chunk 0 lands while the tile is loaded / binned
  [[maybe_unused]] bool tbl_lds = false;
  if constexpr (kBins) {
    // threshold tables: into LDS over bufB + lv (dead until chunk 1 / the first leaf store) if they fit
    const int n_thr = thr_off[nf];
    tbl_lds = (uint32_t)n_thr * 4u <= accL - bufB;
    if (tbl_lds) {
      float* tl = reinterpret_cast<float*>(lbase + (bufB - s0));
      for (int i = tid; i < n_thr; i += kWG3) tl[i] = thr[i];
      __syncthreads();
    }
  }
  int anynan = 0;
  const int ncopy = ld < nf ? ld : nf;
  const int q = tid >> 8;  // the four threads sharing `txn` take every 4th column
  if constexpr (kBins) {
    uint32_t* Xs = reinterpret_cast<uint32_t*>(lbase);
    const float* xr = X + row * (int64_t)ld;
    for (int f = q; f < nf; f += 4) {
      uint32_t w = 0;
      if (valid) {
        const float v = f < ncopy ? xr[f] : __builtin_nanf("");  // DMatrix: missing column = NaN
        if (v != v) {
          w = 0xFFFF0000u;
          anynan = 1;
        } else {
          const int o = thr_off[f], cnt = thr_off[f + 1] - o;
          const uint32_t b = tbl_lds ? bin_of<true>(v, nullptr, bufB + (uint32_t)o * 4u, cnt, lift_steps(cnt))
                                     : bin_of<false>(v, thr + o, 0u, cnt, lift_steps(cnt));
          w = b << 16;
        }
      }
      Xs[f * kTile + txn] = w;
    }
  } else {
    float* Xs = reinterpret_cast<float*>(lbase);
    if (valid) {
      const float* xr = X + row * (int64_t)ld;
      for (int f = q; f < ncopy; f += 4) {
        const float v = xr[f];
        Xs[f * kTile + txn] = v;
        anynan |= (v != v);
      }
      for (int f = ncopy + q; f < nf; f += 4) Xs[f * kTile + txn] = __builtin_nanf("");
      anynan |= (ncopy < nf);
    } else {
      for (int f = q; f < nf; f += 4) Xs[f * kTile + txn] = 0.f;
    }
  }
  if (gg == 0)
    lds_store<LeafT>(accL + txn * sizeof(LeafT),
                     (KIND == FD_FOREST_XGB_BINARY_LOGISTIC) ? (LeafT)base_margin : (LeafT)0);
  dma_wait();  // chunk 0 (published by tile_any's barrier)
  const bool tile_nan =
      tile_any(anynan, reinterpret_cast<uint32_t*>(lbase + (accL - s0) + kTile * sizeof(LeafT)), kWG3 / 64);
  FD_PROF_T(p_t1);

  for (int k = 0; k < n_chunks; ++k) {
    FD_PROF_T(q0);
    const uint32_t cur = (k & 1) ? bufB : bufA;
    if (k + 1 < n_chunks)
      stage_chunk_asm(blob + (size_t)(k + 1) * chunk_stride, (k & 1) ? bufA : bufB, chunk_stride, kWG3 / 64);
    if (k > 0 && gg == ((k - 1) & 3)) {  // owner of chunk k-1 adds its leaf values in tree order
      const uint32_t lv = ((k - 1) & 1) ? lvB : lvA;
      LeafT acc = lds_load<LeafT>(accL + txn * sizeof(LeafT));
#pragma unroll
      for (int c = 0; c < CH; ++c) acc += lds_load<LeafT>(lv + (c * kTile + txn) * sizeof(LeafT));
      lds_store<LeafT>(accL + txn * sizeof(LeafT), acc);
    }
    FD_PROF_T(q1);
    uint32_t slots[TPG];
    if constexpr (kBins) {
      if (tile_nan)
        walk4<D, TPG, LeafT, true, kNodesOnly>(cur, gg, lane4, slots);
      else
        walk4<D, TPG, LeafT, false, kNodesOnly>(cur, gg, lane4, slots);
    } else {
      if (tile_nan)
        walk3<D, TPG, LeafT, true>(cur, gg, lane4, slots);
      else
        walk3<D, TPG, LeafT, false>(cur, gg, lane4, slots);
    }
#ifdef FD_FOREST_PROFILE
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#endif
    FD_PROF_T(q2);
    const uint32_t lv = (k & 1) ? lvB : lvA;
    [[maybe_unused]] LeafT lval[TPG];
    if constexpr (kNodesOnly) {
#pragma unroll
      for (int j = 0; j < TPG; ++j) lval[j] = leaves[((size_t)k * CH + gg * TPG + j) * NL + slots[j]];
    }
#pragma unroll
    for (int j = 0; j < TPG; ++j) {
      const int c = gg * TPG + j;
      if constexpr (kNodesOnly) {
        lds_store<LeafT>(lv + (c * kTile + txn) * sizeof(LeafT), lval[j]);
      } else {
        const uint32_t tb = cur + (uint32_t)c * TB;
        lds_store<LeafT>(lv + (c * kTile + txn) * sizeof(LeafT),
                         lds_load<LeafT>(tb + NL * kNodeBytes + slots[j] * sizeof(LeafT)));
      }
      if (out_leaf != nullptr && valid) {
        const int tg = k * CH + c;
        if (tg < n_trees) out_leaf[row * n_trees + tg] = leaf_ids[(size_t)tg * NL + slots[j]];
      }
    }
    FD_PROF_T(q3);
    dma_wait();
    __syncthreads();  // chunk k+1 landed; lv[k&1] complete; owner of k-1 done with lv[(k-1)&1]
    FD_PROF_T(q4);
    FD_PROF_ADD(p_own, q0, q1);
    FD_PROF_ADD(p_walk, q1, q2);
    FD_PROF_ADD(p_leaf, q2, q3);
    FD_PROF_ADD(p_sync, q3, q4);
  }
#ifdef FD_FOREST_PROFILE
  if (lane == 0 && blockIdx.x < 256) {
    FD_PROF_T(p_t2);
    unsigned long long* o = g_prof + ((size_t)blockIdx.x * 16 + wave) * 8;
    o[0] = p_t1 - p_t0; o[1] = p_walk; o[2] = p_leaf; o[3] = p_own; o[4] = p_sync; o[5] = p_t2 - p_t0;
    o[6] = p_t0; o[7] = 0;
  }
#endif
  const int last = n_chunks - 1;
  if (gg != (last & 3)) return;
  LeafT acc = lds_load<LeafT>(accL + txn * sizeof(LeafT));
  {
    const uint32_t lv = (last & 1) ? lvB : lvA;
#pragma unroll
    for (int c = 0; c < CH; ++c) acc += lds_load<LeafT>(lv + (c * kTile + txn) * sizeof(LeafT));
  }
  if (valid) write_outputs<KIND, LeafT>(acc, row, if_offset, if_denom, out_prob, out_raw);
