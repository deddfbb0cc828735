// graph.hip — the graph detector's transaction-network features (GraphFraudDetector._calculate_network_features,
// ml/models/graph_neural_network.py:338-392) over a device-resident log of recent transactions.
//
// The reference keeps a Python list of up to max_history_size dicts, cut to its newer half whenever it is full, and
// rescans it several times per transaction. Here the log is four device arrays (card_key u64, cents i64, merchant i32,
// dist i32) holding the entries from s(next g) on — at most H - 1 of them, the carried tail — followed by the chunk
// being processed; graph_row.h has the window rule s(g) and the f64 epilogue. dist is k - prev(k), the distance to the
// latest earlier entry with the same (card_key, merchant) pair, 0 for none: entry k is a first occurrence for a window
// starting at s exactly when dist == 0 or k - dist < s, and the value does not move when the tail is carried forward.
// A match further back than the log holds is before s(k) <= s(g) of every later window, so searching the log is exact.
//
// Per chunk of at most kGraphChunk transactions (temporaries stay at chunk + H), all on the caller's stream:
//   graph_move_kernel     only when s() stepped since the last chunk: the tail to the front of the other log buffer
//   graph_append_kernel   the chunk's three input columns behind the tail
//   (chunks of kGraphSmall transactions or more:)
//   graph_prev_kernel     64 new entries per workgroup; it stages their shared range of (card_key, merchant) through LDS
//                         tiles, its 16 waves each take a 16th of a tile (every lane of a wave reads the same
//                         address: broadcasts) and each entry keeps its latest match
//   graph_scan_kernel     64 transactions per workgroup; it stages the union of their windows the same way; each lane
//                         masks to its own [s(g), g] and counts cntU, S, dM, dU; writes four columns and dM
//   (smaller chunks: graph_prev_small_kernel / graph_scan_small_kernel, the same counts with one workgroup per
//   transaction striding over its window)
//   graph_cluster_kernel  one workgroup per transaction, gone at once when dM < 2; gathers the user's first-occurrence
//                         merchants into an LDS list (kGraphList at a time: the lists of one user are disjoint sets,
//                         so their counts add), sorts a list of more than kGraphLinear in LDS, then strides over
//                         the window's first occurrences and counts members (binary search, or a linear probe): T
// The host keeps the running index and passes it with the launch: nothing is read back.
#include <algorithm>

#include "fd_internal.h"
#include "graph_row.h"

namespace fd {
namespace {

constexpr int kScanThreads = 256;  // threads per workgroup of the per-transaction kernels (small forms, cluster)
constexpr int kTxnPerWg = 64;      // transactions per workgroup of the tile kernels (one per lane, the waves split the tile)
constexpr int kTileWaves = 16;     // waves per workgroup of the tile kernels
constexpr int kTileThreads = 64 * kTileWaves;
constexpr int kGraphTile = 1024;   // log entries per LDS tile of the prev / scan kernels
constexpr int kGraphList = 1024;   // merchants per LDS list of the cluster kernel
constexpr int kGraphLinear = 32;   // cluster lists up to this long are probed linearly, longer ones sorted and searched
constexpr int kGraphSortMin = 64;  // the smallest sort
constexpr int kGraphSmall = 512;   // calls (chunks) below this many transactions: a workgroup per transaction

struct GraphLog {
  uint64_t* key;
  int64_t* cents;
  int32_t* merch;
  int32_t* dist;
};

GraphLog log_of(const GraphState& g, int which) {
  char* b = g.log[which].as<char>();
  const size_t cap = (size_t)g.cap;
  return GraphLog{reinterpret_cast<uint64_t*>(b), reinterpret_cast<int64_t*>(b + cap * 8),
                  reinterpret_cast<int32_t*>(b + cap * 16), reinterpret_cast<int32_t*>(b + cap * 20)};
}

__global__ void __launch_bounds__(256) graph_move_kernel(GraphLog src, GraphLog dst, int from, int count) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= count) return;
  dst.key[i] = src.key[from + i];
  dst.cents[i] = src.cents[from + i];
  dst.merch[i] = src.merch[from + i];
  dst.dist[i] = src.dist[from + i];
}

__global__ void __launch_bounds__(256) graph_append_kernel(GraphLog log, int off, const uint64_t* __restrict__ key,
                                                           const int32_t* __restrict__ merch,
                                                           const int64_t* __restrict__ cents, int c) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= c) return;
  log.key[off + i] = key[i];
  log.merch[off + i] = merch[i];
  log.cents[off + i] = cents[i];
}

// The tile kernels: a workgroup of kTileWaves = 16 waves takes kTxnPerWg = 64 consecutive transactions, lane l of every
// wave the l-th of them; wave w takes the tile's entries w, w + 16, ... (one address per wave and read: broadcasts),
// and the 16 partial results of a transaction meet in LDS at the end. (A wave's pass over its share of H entries is a
// serial chain: the more waves share a window, the shorter it is and the more of them a SIMD has to switch between.)

// dist of the c new entries at positions [off, off + c); base: the global index of position 0
__global__ void __launch_bounds__(kTileThreads) graph_prev_kernel(GraphLog log, int off, int c, int64_t base, int H) {
  __shared__ uint64_t skey[kGraphTile];
  __shared__ int32_t smer[kGraphTile];
  __shared__ int sbest[kTileThreads];
  const int tid = threadIdx.x, w = tid >> 6, l = tid & 63;
  const int p0 = off + blockIdx.x * kTxnPerWg;                    // the workgroup's first position
  const int pend = min(off + c, p0 + kTxnPerWg);                  // one past its last
  const int p = p0 + l;
  const bool live = p < pend;
  const uint64_t u = live ? log.key[p] : 0;
  const int32_t m = live ? log.merch[p] : 0;
  const int lo = max(0, (int)(graph_window_start(base + p0, H) - base));
  int best = -1;
  for (int t0 = lo; t0 < pend - 1; t0 += kGraphTile) {
    const int cnt = min(kGraphTile, pend - 1 - t0);  // candidates j < p <= pend - 1
    for (int j = tid; j < cnt; j += kTileThreads) {
      skey[j] = log.key[t0 + j];
      smer[j] = log.merch[t0 + j];
    }
    __syncthreads();
    const int lim = live ? p - t0 : 0;  // this lane's candidates of the tile: j < lim
#pragma unroll 4
    for (int j = w; j < cnt; j += kTileWaves)
      if (j < lim && skey[j] == u && smer[j] == m) best = t0 + j;  // (ascending per wave)
    __syncthreads();
  }
  sbest[tid] = best;
  __syncthreads();
  if (w != 0 || !live) return;
  for (int k = 1; k < kTileWaves; ++k) best = max(best, sbest[l + 64 * k]);
  log.dist[p] = best >= 0 ? p - best : 0;
}

// columns 0, 1, 3, 4 (2 zeroed) and dM of the c transactions at positions [off, off + c)
__global__ void __launch_bounds__(kTileThreads) graph_scan_kernel(GraphLog log, int off, int c, int64_t base, int H,
                                                                  double* __restrict__ out, int32_t* __restrict__ dm) {
  struct KeyCents {
    uint64_t key;
    long long cents;
  };
  __shared__ __attribute__((aligned(16))) KeyCents skc[kGraphTile];
  __shared__ int2 smd[kGraphTile];  // merchant, dist
  __shared__ long long sS[kTileThreads];
  __shared__ int scnt[3][kTileThreads];
  const int tid = threadIdx.x, w = tid >> 6, l = tid & 63;
  const int p0 = off + blockIdx.x * kTxnPerWg;
  const int pend = min(off + c, p0 + kTxnPerWg);
  const int p = p0 + l;
  const bool live = p < pend;
  const uint64_t u = live ? log.key[p] : 0;
  const int32_t m = live ? log.merch[p] : -1;
  const int lo = max(0, (int)(graph_window_start(base + p0, H) - base));  // s() never decreases: the union's start
  const int lo_own = live ? max(0, (int)(graph_window_start(base + p, H) - base)) : 0;
  const bool null_row = u == 0 || m < 0;
  const int hi_own = (live && !null_row) ? p : -1;  // a null row counts nothing
  int cntU = 0, dM = 0, dU = 0;
  long long S = 0;
  for (int t0 = lo; t0 < pend; t0 += kGraphTile) {
    const int cnt = min(kGraphTile, pend - t0);
    for (int j = tid; j < cnt; j += kTileThreads) {
      skc[j] = KeyCents{log.key[t0 + j], (long long)log.cents[t0 + j]};
      smd[j] = make_int2(log.merch[t0 + j], log.dist[t0 + j]);
    }
    __syncthreads();
#pragma unroll 4
    for (int j = w; j < cnt; j += kTileWaves) {
      const int jj = t0 + j;
      const KeyCents kc = skc[j];
      const int2 md = smd[j];
      const bool in = jj >= lo_own && jj <= hi_own;
      const bool first = md.y == 0 || jj - md.y < lo_own;
      const bool mine = in && kc.key == u;
      cntU += mine ? 1 : 0;
      S += mine ? kc.cents : 0ll;
      dM += (mine && first && md.x >= 0) ? 1 : 0;
      dU += (in && first && md.x == m && kc.key != 0) ? 1 : 0;
    }
    __syncthreads();
  }
  sS[tid] = S;
  scnt[0][tid] = cntU;
  scnt[1][tid] = dM;
  scnt[2][tid] = dU;
  __syncthreads();
  if (w != 0 || !live) return;
  for (int k = 1; k < kTileWaves; ++k) {
    S += sS[l + 64 * k];
    cntU += scnt[0][l + 64 * k];
    dM += scnt[1][l + 64 * k];
    dU += scnt[2][l + 64 * k];
  }
  const int32_t d = log.dist[p];
  const int i = p - off;
  graph_row(null_row, cntU, S, dM, dU, log.cents[p], d == 0 || p - d < lo_own, out + (int64_t)i * FD_GRAPH_COLS);
  dm[i] = null_row ? 0 : dM;
}

// Sums of the workgroup's four waves: shuffles inside a wave, then one LDS slot per wave. Every thread gets the total.
template <class T>
__device__ __forceinline__ T graph_block_sum(T v, T* slots) {
  for (int s = 32; s > 0; s >>= 1) v += __shfl_down(v, s, 64);
  __syncthreads();  // (the slots' previous use)
  if ((threadIdx.x & 63) == 0) slots[threadIdx.x >> 6] = v;
  __syncthreads();
  return slots[0] + slots[1] + slots[2] + slots[3];
}

// Calls of fewer than kGraphSmall transactions: one workgroup per transaction, its threads striding over the window
// with coalesced loads (the tile kernels would leave most of a workgroup's lanes idle behind a serial pass over H
// entries). The counts are integers, so both forms give the same bits.
__global__ void __launch_bounds__(kScanThreads) graph_prev_small_kernel(GraphLog log, int off, int64_t base, int H) {
  __shared__ int slots[4];
  const int tid = threadIdx.x;
  const int p = off + blockIdx.x;
  const uint64_t u = log.key[p];
  const int32_t m = log.merch[p];
  const int lo = max(0, (int)(graph_window_start(base + p, H) - base));
  int best = -1;
  for (int j = lo + tid; j < p; j += kScanThreads)
    if (log.key[j] == u && log.merch[j] == m) best = j;  // (ascending per thread)
  for (int s = 32; s > 0; s >>= 1) best = max(best, __shfl_down(best, s, 64));
  if ((tid & 63) == 0) slots[tid >> 6] = best;
  __syncthreads();
  if (tid == 0) {
    best = max(max(slots[0], slots[1]), max(slots[2], slots[3]));
    log.dist[p] = best >= 0 ? p - best : 0;
  }
}

__global__ void __launch_bounds__(kScanThreads) graph_scan_small_kernel(GraphLog log, int off, int64_t base, int H,
                                                                        double* __restrict__ out,
                                                                        int32_t* __restrict__ dm) {
  __shared__ long long slots[4];
  const int tid = threadIdx.x;
  const int i = blockIdx.x;
  const int p = off + i;
  const uint64_t u = log.key[p];
  const int32_t m = log.merch[p];
  const int lo_own = max(0, (int)(graph_window_start(base + p, H) - base));
  const bool null_row = u == 0 || m < 0;  // (the whole workgroup)
  int cntU = 0, dM = 0, dU = 0;
  long long S = 0;
  if (!null_row)
    for (int jj = lo_own + tid; jj <= p; jj += kScanThreads) {
      const uint64_t kj = log.key[jj];
      const int32_t mj = log.merch[jj];
      const int32_t dj = log.dist[jj];
      const bool first = dj == 0 || jj - dj < lo_own;
      const bool mine = kj == u;
      cntU += mine ? 1 : 0;
      S += mine ? (long long)log.cents[jj] : 0ll;
      dM += (mine && first && mj >= 0) ? 1 : 0;
      dU += (first && mj == m && kj != 0) ? 1 : 0;
    }
  // three counts of at most 65536 each in one word beside the sum
  const long long packed = graph_block_sum<long long>((long long)cntU | ((long long)dM << 20) | ((long long)dU << 40),
                                                      slots);
  S = graph_block_sum<long long>(S, slots);
  if (tid != 0) return;
  cntU = (int)(packed & 0xfffff);
  dM = (int)((packed >> 20) & 0xfffff);
  dU = (int)(packed >> 40);
  const int32_t d = log.dist[p];
  graph_row(null_row, cntU, S, dM, dU, log.cents[p], d == 0 || p - d < lo_own, out + (int64_t)i * FD_GRAPH_COLS);
  dm[i] = null_row ? 0 : dM;
}

// list[0, len) ascending, by a bitonic sort of the next power of two (the tail padded with INT_MAX, which sorts behind
// or beside every merchant: the first len entries are the list's own). All threads; ends on a barrier.
__device__ __forceinline__ void graph_sort_list(int32_t* list, int len, int tid) {
  int n2 = kGraphSortMin;
  while (n2 < len) n2 <<= 1;
  for (int q = len + tid; q < n2; q += kScanThreads) list[q] = 0x7fffffff;
  __syncthreads();
  for (int k = 2; k <= n2; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < (n2 >> 1); t += kScanThreads) {
        const int a = ((t & ~(j - 1)) << 1) | (t & (j - 1)), b = a | j;
        const int32_t x = list[a], y = list[b];
        if ((x > y) == ((a & k) == 0)) {
          list[a] = y;
          list[b] = x;
        }
      }
      __syncthreads();
    }
}

// members of list[0, len) among the window's first occurrences, this thread's share. sorted: the list is ascending
// (a binary search per entry); otherwise it is short and padded to a multiple of 4 with -1 (a linear probe).
__device__ __forceinline__ int graph_count_members(const GraphLog& log, const int32_t* list, int len, bool sorted,
                                                   int lo_own, int p, int tid) {
  int T = 0;
  for (int b = lo_own; b <= p; b += kScanThreads) {
    const int jj = b + tid;
    const bool valid = jj <= p;
    const int32_t mj = valid ? log.merch[jj] : -1;
    const int32_t dj = valid ? log.dist[jj] : 0;
    const bool f = valid && mj >= 0 && (dj == 0 || jj - dj < lo_own);
    if (__ballot(f) == 0) continue;  // (this wave)
    bool hit = false;
    if (sorted) {
      int a = 0, n = len;  // lower bound of mj in list[0, len)
      while (n > 0) {
        const int h = n >> 1;
        const bool right = list[a + h] < mj;
        a = right ? a + h + 1 : a;
        n = right ? n - h - 1 : h;
      }
      hit = a < len && list[a] == mj;
    } else {
      for (int q = 0; q < len; q += 4) {
        const int4 v = *reinterpret_cast<const int4*>(list + q);
        hit = hit || v.x == mj || v.y == mj || v.z == mj || v.w == mj;
      }
    }
    T += (f && hit) ? 1 : 0;
  }
  return T;
}

// the list is complete: T's share of it. All threads; the list may be rewritten afterwards.
__device__ __forceinline__ int graph_list_members(const GraphLog& log, int32_t* list, int len, int lo_own, int p,
                                                  int tid) {
  const bool sorted = len > kGraphLinear;
  __syncthreads();  // the appends
  if (sorted) {
    graph_sort_list(list, len, tid);
  } else {
    if (tid < 4) list[len + tid] = -1;
    __syncthreads();
  }
  const int T = graph_count_members(log, list, len, sorted, lo_own, p, tid);
  __syncthreads();
  return T;
}

// column 2 of the transactions with dM >= 2: one workgroup each
__global__ void __launch_bounds__(kScanThreads) graph_cluster_kernel(GraphLog log, int off, int64_t base, int H,
                                                                     double* __restrict__ out,
                                                                     const int32_t* __restrict__ dm) {
  __shared__ __attribute__((aligned(16))) int32_t list[kGraphList + 4];
  __shared__ int s_len;
  __shared__ int slots[4];
  const int i = blockIdx.x;
  const int dM = dm[i];
  if (dM < 2) return;  // (the whole workgroup)
  const int tid = threadIdx.x;
  const int p = off + i;
  const int lo_own = max(0, (int)(graph_window_start(base + p, H) - base));
  const uint64_t u = log.key[p];
  if (tid == 0) s_len = 0;
  int len = 0, T = 0;  // len: s_len as every thread knows it
  for (int b = lo_own; b <= p; b += kScanThreads) {
    const int jj = b + tid;
    const bool valid = jj <= p;
    const uint64_t kj = valid ? log.key[jj] : 0;
    const int32_t mj = valid ? log.merch[jj] : -1;
    const int32_t dj = valid ? log.dist[jj] : 0;
    const bool cand = valid && kj == u && mj >= 0 && (dj == 0 || jj - dj < lo_own);
    const int cnt = __syncthreads_count(cand);  // (also orders the appends before it and s_len's reset)
    if (len + cnt > kGraphList) {  // these would not fit: count the list's members, start the next list
      T += graph_list_members(log, list, len, lo_own, p, tid);
      if (tid == 0) s_len = 0;
      len = 0;
      __syncthreads();
    }
    if (cand) list[atomicAdd(&s_len, 1)] = mj;  // the order inside a list does not matter
    len += cnt;
  }
  T += graph_list_members(log, list, len, lo_own, p, tid);
  T = graph_block_sum<int>(T, slots);
  if (tid == 0) out[(int64_t)i * FD_GRAPH_COLS + 2] = graph_cluster_value(T, dM);
}

}  // namespace

void graph_init(Engine& e, const fd_graph_params& p) {
  FD_REQUIRE(p.max_history >= kGraphMinHistory && p.max_history <= kGraphMaxHistory, FD_ERR_INVALID_ARG,
             "graph max_history must be in [2, 65536], got " + std::to_string(p.max_history));
  GraphState& g = e.graph;
  g.ready = false;
  g.H = p.max_history;
  g.cap = g.H + kGraphChunk;
  for (DeviceBuffer& b : g.log) b.ensure((size_t)g.cap * 24);
  g.dm.ensure((size_t)kGraphChunk * 4);
  g.total = 0;
  g.base = 0;
  g.cur = 0;
  g.ready = true;
}

void graph_clear(Engine& e) {
  GraphState& g = e.graph;
  FD_REQUIRE(g.ready, FD_ERR_NOT_LOADED, "graph log not initialised (fd_graph_init)");
  g.total = 0;
  g.base = 0;
}

void graph_info(Engine& e, int64_t* total, int64_t* held) {
  const GraphState& g = e.graph;
  FD_REQUIRE(g.ready, FD_ERR_NOT_LOADED, "graph log not initialised (fd_graph_init)");
  if (total) *total = g.total;
  if (held) *held = g.total == 0 ? 0 : g.total - graph_window_start(g.total - 1, g.H);
}

void graph_step(Engine& e, const fd_txn_batch& t, int64_t n, double* d_out) {
  GraphState& g = e.graph;
  FD_REQUIRE(g.ready, FD_ERR_NOT_LOADED, "graph log not initialised (fd_graph_init)");
  FD_REQUIRE(n >= 0 && n < (1ll << 31), FD_ERR_INVALID_ARG, "batch size out of range");
  if (n == 0) return;
  FD_REQUIRE(t.card_key && t.merchant && t.amount_cents && d_out, FD_ERR_INVALID_ARG,
             "null card_key / merchant / amount_cents / output");
  hipStream_t st = e.stream;
  Engine::Timed* ev = e.timing ? e.next_event_pair(FD_TIMING_GRAPH) : nullptr;
  if (ev) FD_HIP(hipEventRecord(ev->a, st));
  for (int64_t a = 0; a < n; a += kGraphChunk) {
    const int c = (int)std::min<int64_t>(kGraphChunk, n - a);
    const int64_t s0 = graph_window_start(g.total, g.H);  // the earliest index this chunk's windows reach
    if (s0 > g.base) {  // carry the tail [s0, total) to the front of the other buffer
      const int from = (int)(s0 - g.base), count = (int)(g.total - s0);
      if (count > 0)
        hipLaunchKernelGGL(graph_move_kernel, dim3((count + 255) / 256), dim3(256), 0, st, log_of(g, g.cur),
                           log_of(g, g.cur ^ 1), from, count);
      g.cur ^= 1;
      g.base = s0;
    }
    const int off = (int)(g.total - g.base);
    FD_REQUIRE(off >= 0 && off + c <= g.cap, FD_ERR_UNSUPPORTED, "internal: graph log overflow");
    const GraphLog log = log_of(g, g.cur);
    double* out = d_out + a * FD_GRAPH_COLS;
    hipLaunchKernelGGL(graph_append_kernel, dim3((c + 255) / 256), dim3(256), 0, st, log, off, t.card_key + a,
                       t.merchant + a, t.amount_cents + a, c);
    if (c < kGraphSmall) {
      hipLaunchKernelGGL(graph_prev_small_kernel, dim3((unsigned)c), dim3(kScanThreads), 0, st, log, off, g.base, g.H);
      hipLaunchKernelGGL(graph_scan_small_kernel, dim3((unsigned)c), dim3(kScanThreads), 0, st, log, off, g.base, g.H,
                         out, g.dm.as<int32_t>());
    } else {
      const unsigned wgs = (unsigned)((c + kTxnPerWg - 1) / kTxnPerWg);
      hipLaunchKernelGGL(graph_prev_kernel, dim3(wgs), dim3(kTileThreads), 0, st, log, off, c, g.base, g.H);
      hipLaunchKernelGGL(graph_scan_kernel, dim3(wgs), dim3(kTileThreads), 0, st, log, off, c, g.base, g.H, out,
                         g.dm.as<int32_t>());
    }
    hipLaunchKernelGGL(graph_cluster_kernel, dim3((unsigned)c), dim3(kScanThreads), 0, st, log, off, g.base, g.H,
                       out, g.dm.as<int32_t>());
    FD_HIP(hipGetLastError());
    g.total += c;
  }
  ++g.steps;
  if (ev) FD_HIP(hipEventRecord(ev->b, st));
}

}  // namespace fd
