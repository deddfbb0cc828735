// fd_internal.h — engine internals shared by the HIP translation units of libfdengine.so.
// Not part of the ABI (see include/fdengine.h).
#pragma once

#include <hip/hip_runtime.h>

#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstddef>
#include <cstdint>
#include <mutex>
#include <stdexcept>
#include <string>
#include <thread>
#include <type_traits>
#include <utility>
#include <vector>

#include "fdengine.h"
#include "key_hash.h"
#include "metrics_row.h"

namespace fd {

constexpr int kMaxSlots = 8;      // forest slots per engine
constexpr int kTile = 256;        // transactions per workgroup in the forest kernel (one per thread)
constexpr int kGatherBatchMax = 4096;  // largest batch the gather bucket kernel takes (features.hip kChunkCap)
constexpr int kMaxFeatures = 64;  // model columns held in LDS ([feature][kTile] f32 = 64 KiB max)
// The compact scoring vector of the fused pipeline (features.hip write_vector -> ensemble.hip prologue): of the 64
// slots of the engine's vector (FeatureProcessor's 41 definitions + derived features + pad, _prepare_features) only
// these 22 vary per transaction; slots 12, 24, 25, 33, 34 are always 0.5 (defaults with no bridged source) and the
// rest 0. The pipelined stream writes a 64-B row per transaction instead of 64 floats (256 B) when nothing else reads
// the vectors, and the ensemble kernel expands it: the 14 slots with arbitrary values as f32 in words
// 0..13 (compact-index order), the 8 that are always small integers — hour, day of week, weekend, the 1 h / 24 h /
// 5 min counts, the account age (each clip10 of an integer), the new-device flag — as bytes 56..63.
constexpr int kCompactWidth = 16;  // row stride in 4-B words
constexpr int kCompactSlots = 22;
constexpr int kCompactSlot[kCompactSlots] = {0, 1, 5, 6, 7, 14, 15, 16, 17, 19, 21, 23,
                                             26, 27, 31, 32, 41, 42, 43, 44, 45, 46};
constexpr int kIntSlots = 8;
constexpr int kIntCompact[kIntSlots] = {2, 3, 4, 5, 6, 9, 12, 15};  // compact indices (features 5 6 7 14 15 19 26 32)
// the byte (0..7) of a small-integer compact slot, -1 for the others
__host__ __device__ constexpr int int_slot(int ci) {
  for (int k = 0; k < kIntSlots; ++k)
    if (kIntCompact[k] == ci) return k;
  return -1;
}
// the f32 word (0..13) of a compact slot with arbitrary values, -1 for the small-integer ones
__host__ __device__ constexpr int compact_word(int ci) {
  if (int_slot(ci) >= 0) return -1;
  int w = 0;
  for (int k = 0; k < ci; ++k) w += int_slot(k) < 0 ? 1 : 0;
  return w;
}
static_assert(compact_word(kCompactSlots - 1) == kCompactSlots - kIntSlots - 1 && kCompactSlots - kIntSlots <= 14,
              "14 f32 words, then the 8 bytes");
// the slot's place in the compact row, -2 for the constant 0.5, -1 for the constant 0
__host__ __device__ constexpr int compact_src(int f) {
  for (int k = 0; k < kCompactSlots; ++k)
    if (kCompactSlot[k] == f) return k;
  return (f == 12 || f == 24 || f == 25 || f == 33 || f == 34) ? -2 : -1;
}
constexpr int kMaxDepth = 10;     // deepest tree the heap repacker accepts (deeper forests: the sparse layout)
// Sparse (pointer) layout, forest_sparse.hip: a node's meta word holds a 24-bit forest-global node index (the left
// child; the right child is the next record) or leaf ordinal, and a 6-bit feature
constexpr int64_t kSparseMaxNodes = 1ll << 24;
constexpr size_t kLdsBudget = 160 * 1024;  // LDS per CU (one workgroup per CU at 64k batches)
constexpr int kMaxBins = 65534;   // distinct thresholds per feature in the binned layout
constexpr int kSplitTiles = 128;  // below this many 256-txn tiles the forest runs the tree-split path
constexpr int kSeqInput = 16;     // LSTM per-event input width (the bridged raw features)
constexpr unsigned long long kSeqMaterialized = 1ull << 63;  // sequence descriptor: row i of the sequence buffer
constexpr int kLstmHidden = 128;  // lstm_sequential hidden_units (ml/utils/config.py:152-156)

#ifdef FD_FOREST_PROFILE
// Latency-path timeline (profiling build only; tools/c5_phases.py): per (kernel id, linear workgroup < 1024)
// {start, mark 1, mark 2, end} of thread 0 in the GPU-wide 100 MHz clock. Each translation unit keeps its own buffer
// (FD_TL_BUF) and exports it (fd_debug_tl_<unit>); the last launch of each kernel id wins.
constexpr int kTlKernels = 8;
#define FD_TL_BUF(name) __device__ unsigned long long name[fd::kTlKernels * 1024 * 4]
#define FD_TL(buf, kid, k)                                                                            \
  do {                                                                                                \
    const unsigned tl_b = blockIdx.x + blockIdx.y * gridDim.x;                                        \
    if (threadIdx.x == 0 && tl_b < 1024u) buf[((kid) * 1024 + tl_b) * 4 + (k)] = __builtin_amdgcn_s_memrealtime(); \
  } while (0)
#else
#define FD_TL(buf, kid, k) \
  do {                     \
  } while (0)
#endif

struct Error : std::runtime_error {
  int code;
  Error(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};

void set_error(const std::string& msg);

#define FD_HIP(call)                                                                       \
  do {                                                                                     \
    hipError_t _e = (call);                                                                \
    if (_e != hipSuccess)                                                                  \
      throw ::fd::Error(FD_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(_e));    \
  } while (0)

#define FD_REQUIRE(cond, code, msg)              \
  do {                                           \
    if (!(cond)) throw ::fd::Error((code), (msg)); \
  } while (0)

// bytes held through DeviceBuffer in this process, every engine together (counter "device_bytes_live")
inline std::atomic<long long> g_device_bytes_live{0};

// A device allocation and its owner: grows, never shrinks, freed when the owner goes (a member with its struct, a
// local at scope exit — an exception's included). Moves, never copies. The only hipMalloc / hipFree of the library.
struct DeviceBuffer {
  void* ptr = nullptr;
  size_t bytes = 0;
  DeviceBuffer() = default;
  DeviceBuffer(const DeviceBuffer&) = delete;
  DeviceBuffer& operator=(const DeviceBuffer&) = delete;
  DeviceBuffer(DeviceBuffer&& o) noexcept { swap(o); }
  DeviceBuffer& operator=(DeviceBuffer&& o) noexcept {
    if (this != &o) {
      release();
      swap(o);
    }
    return *this;
  }
  ~DeviceBuffer() { release(); }
  void swap(DeviceBuffer& o) noexcept {
    std::swap(ptr, o.ptr);
    std::swap(bytes, o.bytes);
  }
  void ensure(size_t need) {
    if (need <= bytes) return;
    release();
    FD_HIP(hipMalloc(&ptr, need));
    bytes = need;
    g_device_bytes_live.fetch_add((long long)need, std::memory_order_relaxed);
  }
  // grow by a quarter more than asked: buffers sized per batch by a count that wanders (a shard's inbox) then
  // reallocate O(log) times instead of at every new maximum (hipFree waits for the device)
  void ensure_headroom(size_t need) {
    if (need > bytes) ensure(need + need / 4);
  }
  void release() {
    if (ptr) (void)hipFree(ptr);
    g_device_bytes_live.fetch_sub((long long)bytes, std::memory_order_relaxed);
    ptr = nullptr;
    bytes = 0;
  }
  // drop the allocation without freeing it: a deliberate leak of memory the device may still touch (it stays counted)
  void abandon() {
    ptr = nullptr;
    bytes = 0;
  }
  template <class T>
  T* as() const { return static_cast<T*>(ptr); }
};
static_assert(!std::is_copy_constructible_v<DeviceBuffer> && std::is_nothrow_move_constructible_v<DeviceBuffer>);

// small-batch tree-split scratch of one forest (forest.hip launch_split)
struct SplitScratch {
  DeviceBuffer bins, nan, leaves;  // nan: per-tile "holds a NaN" flags, cleared by the step's sum kernel
};

// Latency batches, option "latency_prebin": the tree-split binning of the XGBoost / IsolationForest pair done by
// workgroups of the LSTM head's launch, ahead of its own (lstm.hip lstm_kernel4), so the pair's binning launch and its
// queue gap go (forest.hip launch_forest_pair_blend). Filled by forest_pair_prebin before the LSTM launch (score_matrix);
// `done` set by the LSTM launch that binned (these vectors), consumed by the pair launch.
struct PreBin {
  const float* thr[2] = {};        // [0] XGBoost, [1] IsolationForest: distinct thresholds, feature-major
  const int32_t* thr_off[2] = {};
  uint32_t* bins[2] = {};          // [feature][n_pad]
  uint32_t* nan[2] = {};           // per-tile NaN flags
  int nf[2] = {};
  int64_t n = 0, n_pad = 0;
  int ld = 0;
  int steps[2] = {};               // each forest's largest lifting step (PackedForest::bin_steps)
  bool thr_nonempty = false;       // both tables hold a threshold (the inline searches read clamped positions)
  const void* fx = nullptr;        // the forests and the vectors the bins are for
  const void* ff = nullptr;
  const float* X = nullptr;
  bool want = false, done = false;
};

// The sparse image of a forest on the device (forest_sparse.hip): node records, then the two arrays indexed by leaf
// ordinal. gen: the PackedForest::gen it was built for (0 = none).
struct SparseImage {
  DeviceBuffer nodes, leaf_val, leaf_ids;
  int64_t n_nodes = 0, n_leaves = 0;
  uint64_t gen = 0;
};

// gbdt.hip: device buffers of a fit (they grow and stay), the histogram kernel's rows per workgroup (option
// "gbdt_hist_rows") and the counters "gbdt_hist_launches" / "gbdt_trees" / "gbdt_nodes_split"; of a watched fit
// (fd_gbdt_fit_eval_*) the eval rows' bins and margins, their sort words (unsorted, then sorted), the negatives'
// prefix counts, rocPRIM's temporary storage (asked for once per fit), the stop state, the metric curve and the
// training margins after the best round; counters "gbdt_eval_launches" / "gbdt_rounds_run"
struct GbdtScratch {
  DeviceBuffer bins, gh, mask, pos, margin, hist, nodes, cuts, offsets;
  DeviceBuffer ebins, emargin, words, neg_before, eval_tmp, state, curve, best_margin;
  size_t eval_tmp_bytes = 0;
  int hist_rows = 4096;
  unsigned long long hist_launches = 0, trees = 0, nodes_split = 0, eval_launches = 0, rounds_run = 0;
};

// The TreeSHAP path table of a forest on the device (shap.hip): built on the first explain call, for the
// PackedForest::gen it was built for (0 = none)
struct ShapImage {
  DeviceBuffer paths, elems;
  int64_t n_paths = 0, chunk_paths = 0;
  int n_chunks = 0;
  double bias = 0.0;
  uint64_t gen = 0;
};

// A forest repacked into perfect depth-D trees stored as 1-based heaps (see forest.hip header and
// DESIGN.md "Forest layout"): per tree 2^D node records {f32 thr, u32 meta} (slot 0 unused; children
// of slot s are 2s / 2s+1) then 2^D leaf values (f32 XGBoost, f64 Isolation Forest); chunks of
// `chunk` trees, each `chunk_stride` bytes (1 KiB multiple, LDS-DMA staging).
//   meta = feature * kTile * 4 (byte offset of the feature row in the LDS tile) | default_left << 31.
struct PackedForest {
  bool loaded = false;
  // kind FD_FOREST_SKLEARN_PROBA or deeper than kMaxDepth: only the sparse image exists (no heap, no binned layout;
  // chunk / b_chunk / n_chunk are 0 and their buffers are not read), every launch goes to forest_sparse_kernel
  bool sparse_only = false;
  mutable SparseImage sp;  // built at load for a sparse-only forest, else on the first launch under option 11
  int kind = 0;
  int n_trees = 0;
  int n_chunks = 0;
  int chunk = 0;
  int depth = 0;
  int num_feature = 0;
  size_t tree_bytes = 0;
  size_t chunk_stride = 0;
  float base_margin = 0.f;  // XGB: -logf(1/base_score - 1)
  double if_offset = 0.0;
  double if_denominator = 0.0;
  DeviceBuffer blob;      // n_chunks * chunk_stride
  DeviceBuffer leaf_ids;  // n_trees_padded * 2^D original node ids (parity output)
  // binned layout (forest_kernel4), present when every feature has <= 65534 distinct thresholds
  bool binned = false;
  int b_chunk = 0, b_n_chunks = 0, bin_steps = 0;
  size_t b_tree_bytes = 0, b_chunk_stride = 0;
  DeviceBuffer b_blob;     // b_n_chunks * b_chunk_stride
  DeviceBuffer b_thr;      // distinct thresholds, feature-major ascending (f32)
  DeviceBuffer b_thr_off;  // num_feature + 1 offsets (int32)
  int b_n_thr = 0;         // distinct thresholds in b_thr
  // node-only chunks of the binned layout (forest_kernel6): CH trees' node words per chunk, leaf
  // values in a separate [tree][2^D] array read from global memory
  int n_chunk = 0, n_n_chunks = 0;
  size_t n_chunk_stride = 0;
  DeviceBuffer n_blob;    // n_n_chunks * n_chunk_stride
  DeviceBuffer n_leaves;  // n_n_chunks * n_chunk * 2^D leaf values (f32 XGBoost / f64 IsolationForest)
  mutable SplitScratch split;
  // the model as loaded (host copy): the fused ensemble kernel repacks it jointly with the other forest
  uint64_t gen = 0;  // changes on every load / unload (ensemble plan cache key)
  fd_forest_params params{};
  std::vector<int64_t> t_off;
  std::vector<int32_t> t_left, t_right, t_feature;
  std::vector<double> t_threshold, t_leaf;
  std::vector<uint8_t> t_dleft;
  // attribution (shap.hip): the covers fd_forest_set_cover / fd_load_xgboost_json attached (empty: none) and the path
  // table built from them; both go with the forest (shap_forget)
  std::vector<double> t_cover;
  mutable ShapImage shap;
  // every device image of the forest freed (unload); the host copy of the trees stays
  void drop_device() {
    for (DeviceBuffer* b : {&blob, &leaf_ids, &b_blob, &b_thr, &b_thr_off, &n_blob, &n_leaves, &split.bins, &split.nan,
                            &split.leaves, &sp.nodes, &sp.leaf_val, &sp.leaf_ids, &shap.paths, &shap.elems})
      b->release();
    sp.gen = shap.gen = 0;
  }
};

// iforest_fit.hip: device buffers of a fit (they grow and stay), the grown forest packed for the offset's scoring pass
// (never in a slot) and the counters "iforest_fit_trees" / "iforest_fit_nodes_split"
struct IForestFitScratch {
  DeviceBuffer rows, masks, heaps, raw, prob, sorted, sort_tmp;
  PackedForest scorer;
  unsigned long long trees = 0, nodes_split = 0;
};

// mlp_fit.hip: device buffers of a fit (they grow and stay) — the shape words, the forward and transposed operand
// blobs, the flat master parameters and the optimiser's two moments, the chunk partials with their loss / weight sums,
// every epoch's index array, the epochs' f64 loss sums, a step's masks (fd_mlp_fit_batch_device) — the option
// "mlp_fit_chunks_per_wg" (0: a chunk per workgroup) and the counters "mlp_fit_steps" / "mlp_fit_launches"
struct MlpFitScratch {
  DeviceBuffer shape, fwd, bwd, w, m, v, partial, lossw, idx, loss, masks;
  int chunks_per_wg = 0;
  unsigned long long steps = 0, launches = 0;
};

// The fused ensemble kernel's joint repack of one XGBoost and/or one IsolationForest (ensemble_plan.hip build_plan):
// both padded to one depth D, node words rewritten against the MERGED per-feature threshold tables, so one bin
// tile serves both forests; chunks of CH[k] node-only trees, leaf values [tree][2^D] per forest.
// binning passes of one row form (ensemble_plan.hip plan_passes): pass p covers features [f[p], f[p + 1]); bit p of
// glob: searched in global memory (a table larger than the staging area); img_off[p] .. img_off[p + 1]: pass p's
// padded LDS image
struct EnsPassSet {
  std::vector<int> f, img_off;
  unsigned long long glob = 0;
};

struct EnsemblePlan {
  bool valid = false;
  bool wide = true;  // chunk layout: 24 / 16 trees (wide) or 20 / 12 (compact: LDS room for an RCCL kernel beside)
  int slot[2] = {-1, -1};   // forest A = the XGBoost model (or the only forest), forest B = the IsolationForest
  uint64_t gen[2] = {0, 0};
  int n_forests = 0, D = 0, nf = 0;
  int kind[2] = {0, 0}, n_trees[2] = {0, 0}, CH[2] = {0, 0}, n_chunks[2] = {0, 0};
  size_t stride[2] = {0, 0};
  float base_margin = 0.f;
  double if_offset = 0.0, if_denominator = 0.0;
  DeviceBuffer nodes[2], thr;  // per forest: chunk blobs (node blocks + leaf values); merged threshold tables
  std::vector<int32_t> h_thr_off;  // merged table offsets (host copy: binning pass plan)
  // (ensemble_plan.hip build_plan / plan_passes)
  std::vector<uint16_t> h_cbin;    // bins of the compact vector's constant slots
  std::vector<uint16_t> h_lut;     // bins of the small-integer compact slots' values 0..31
  DeviceBuffer img;    // every staged binning pass's padded table image, LDS-DMA source
  EnsPassSet passes;
  int max_feature_thr = 0;
  // the forests contracted against the compact vector's constant slots (ensemble_plan.hip contract_forest_host): the
  // same chunk geometry, tree t a perfect heap of its own depth d_t (heap slot 0 of its node block holds d_t), its
  // 2^d_t leaves at the start of its leaf row. contract: the mode the plan was built for (option ensemble_contract:
  // 0 none, 1 every tree padded to the deepest of its wave's trees, 2 every tree its own depth); contracted: some tree
  // is walked over fewer than D levels (else the launches keep nodes[])
  DeviceBuffer nodes_c[2];
  int contract = 0;
  bool contracted = false;
  long long nodes_pruned = 0;           // splits of the loaded forests that the contracted ones no longer hold
  long long steps_full = 0, steps_c = 0;  // node steps per transaction: n_trees x D over both forests / sum of d_t
  // contract 3 / 4: nodes_c[] hold the dense chunk stream (ensemble_plan.hip dense_layout_host) — chunks of their own
  // lengths, each closed by its 1 KiB chunk table; the first chunk's length and the chunk count per forest
  int dense_len0[2] = {0, 0}, dense_chunks[2] = {0, 0};
};

// A forest with every split on a constant slot of the compact scoring vector (compact_src(f) < 0: the value 0.5 or 0)
// replaced by the child that value takes — left iff value < threshold in f32, the packer's comparison
// (ensemble_plan.hip contract_forest_host)
struct ContractedForest {
  std::vector<int64_t> off;
  std::vector<int32_t> left, right, feature, depth;  // depth: per tree, >= 1 (a lone leaf walks one pad level)
  std::vector<double> threshold, leaf;
  std::vector<uint8_t> dleft;
  long long pruned = 0;
  fd_tree_arrays arrays() const {
    fd_tree_arrays t{};
    t.n_trees = (int32_t)off.size() - 1;
    t.tree_offsets = off.data();
    t.left = left.data();
    t.right = right.data();
    t.feature = feature.data();
    t.threshold = threshold.data();
    t.default_left = dleft.data();
    t.leaf_value = leaf.data();
    return t;
  }
};
ContractedForest contract_forest_host(const fd_forest_params& p, const fd_tree_arrays& t);

// The dense chunk layout of a contracted forest (ensemble_plan.hip dense_layout_host; include/fdengine.h
// fd_dense_layout_host documents the chunk table and the node word): what ensemble_kernel's VD 3 instantiation walks.
constexpr int kDenseSMax = 8;  // bundles per chunk at most: the leaf-index tiles are kDenseSMax x 2 KiB, twice
struct DenseLayout {
  std::vector<char> blob;           // the chunks, back to back
  std::vector<int64_t> chunk_off;   // per chunk: byte offset in blob
  std::vector<int32_t> chunk_len;   // per chunk: bytes (data rounded up to 1 KiB + the 1 KiB table)
  std::vector<fd_dense_tree> tree;  // per tree, forest order
  int tpg = 0;                      // trees per bundle
  uint32_t buf = 0;                 // the chunk buffer's data bytes (EnsCfg::BUF)
  long long steps = 0;              // sum of the walked depths of the forest's own trees
};
// tables[f]: feature f's ascending distinct thresholds (f32) that node words index; mode 3 consecutive bundles, 4 the
// chunk's trees sorted by depth; owner_bias: sixteenths of a level per tree of the chunk charged to tree group 0
DenseLayout dense_layout_host(const ContractedForest& c, bool xgb, const std::vector<std::vector<float>>& tables,
                              bool wide, int mode, int owner_bias);
// The planner's part of the fused path (ensemble_plan.hip), called by ensemble.hip's launchers. build_plan: the joint
// repack of forest A (XGBoost, slot sa) and B (IsolationForest, slot sb; either may be -1) into P, false when not
// possible; plan_current: P was built for these slots' forests as loaded now; want_wide: the engine's chunk layout.
struct Engine;
bool build_plan(Engine& e, EnsemblePlan& P, int sa, int sb, bool wide, int contract = 0);
bool plan_current(const Engine& e, const EnsemblePlan& P, int sa, int sb, bool wide, int contract = 0);
bool want_wide(const Engine& e);

// card-hash routing records (route.hip): one transaction (48 B) / one result (24 B)
struct __attribute__((aligned(16))) RouteRecord {
  unsigned long long key;
  long long ts;
  long long cents;
  unsigned long long dfp;
  int merchant;
  unsigned seq;  // index in the ingest rank's micro-batch
  unsigned char ipc, hour, wk;
  unsigned char pm;  // payment-method code for the owner's windows (255 = null)
  unsigned flags;    // bit 0: Transaction.isFraud (owner's windows / sink)
};
struct __attribute__((aligned(8))) ResultRecord {
  double fraud_prob;
  double confidence;
  unsigned seq;
  unsigned char decision, risk;
  unsigned short pad;
};

// LSTM head (lstm.hip): B operands packed per wave/gate/k-step/lane, summed biases, dense head
struct LstmModel {
  bool loaded = false;
  int input_size = 0, n_out = 0;
  DeviceBuffer wpk, wpk4, bias, wout, bout;  // wpk: 16-row kernel's B operands; wpk4: the 4-row kernel's
  bool hh_finite = false;  // every W_hh weight finite: W_hh h_{-1} = W_hh 0 adds only zeros (lstm_kernel4 skips it)
};

// Transaction-network features (graph.hip): the device log of recent transactions. Each of the two buffers holds the
// four columns (card_key u64, cents i64, merchant i32, dist i32) at `cap` entries; the live one holds the global
// indices [base, total). The tail is carried to the other buffer when the window start steps.
constexpr int kGraphChunk = 16384;  // transactions per pass of the graph kernels (temporaries stay at chunk + H)
struct GraphState {
  bool ready = false;
  int H = 0;    // max_history
  int cap = 0;  // entries per column: H + kGraphChunk
  int cur = 0;  // the live buffer
  int64_t total = 0;  // transactions since init / clear: the next global index
  int64_t base = 0;   // global index of the live buffer's position 0
  DeviceBuffer log[2];
  DeviceBuffer dm;  // per transaction of a chunk: dM, the scan kernel's count for the cluster kernel
  unsigned long long steps = 0;  // counter "graph_steps"
};

// Text patterns and features (text.hip): per-row accumulators of one chunk, and the device-side counter behind
// "text_nonascii_rows" (nothing is read back per call)
constexpr int kTextChunk = 65536;  // rows per pass of the text kernels (the accumulators stay at chunk x 48 B)
struct TextState {
  DeviceBuffer acc;
  DeviceBuffer count;
  unsigned long long calls = 0;  // counter "text_calls"
};

// A/B tests (abtest.hip): the tests' parameters on the host, their accumulators on the device
struct AbTest {
  bool live = false;
  uint64_t salt = 0;
  double threshold = 0.0;
};
struct AbState {
  AbTest tests[FD_AB_MAX_TESTS];
  DeviceBuffer state;     // fd_ab_state per test id
  DeviceBuffer partials;  // one fd_ab_state per workgroup of the record kernel, then its ticket
  DeviceBuffer part;      // partition: control rows per workgroup, scanned in place
  DeviceBuffer index;     // fd_ab_score_matrix_* (score.hip ab_score_matrix): the partition's index, its two counts, the variants
  DeviceBuffer rows;      // ... and the batch in partition order with its results
};
// Prediction metrics (metrics.hip): the collector's state on the device, the ring's header on the host
struct MetricsCollector {
  bool live = false;
  MetricsHeader h{};
  DeviceBuffer state;     // MetricsState (its header unused)
  DeviceBuffer partials;  // one MetricsPart per workgroup of the record kernel, then its ticket
  DeviceBuffer summary;   // the query kernel's fd_metrics_summary
};
// ab_scatter_results: partition-order results (p_*) back to arrival order; a null output is skipped
struct AbScatter {
  const int32_t* idx;
  int64_t n;
  int64_t count[2];  // rows per variant
  int models[2];     // n_models per variant
  int m_max;
  const double *p_fp, *p_conf;
  const uint8_t *p_dec, *p_risk;
  const double* p_mp[2];  // models[v] x count[v], column-major
  double *fp, *conf;
  uint8_t *dec, *risk;
  double* mp;  // m_max x n
};

// MLP head (mlp.hip): the packed model (header, per layer the A operands in the chained k order, padded biases)
struct MlpModel {
  bool loaded = false;
  bool hot = false;  // the reference shape's kernel form: 3 layers, every padded width 64
  int n_layers = 0;
  int dims[9] = {};
  int words = 0;     // 4-B words of the blob (= the kernel's LDS image)
  int cus = 0, occ_ref = 1, occ_lds = 1;  // CUs; workgroups of each kernel form that fit a CU beside each other
  DeviceBuffer blob;
};

// One card's keyed state header (features.hip): 128 B = one L2 line, so a transaction's state read touches one
// line. Bytes 0-63 hold everything a transaction rewrites (last time, ring cursor, window counts / sums / oldest
// times, the redis_compat session, the LSTM history cursor in flags), bytes 64-127 what only an insert or a profile
// load writes (key, profile, device fingerprints): a transaction's write-back dirties half the line (round 5; the
// oldest times are stored as 32-bit offsets below last_ts to fit — exact, a window spans < 2^32 ms).
struct __attribute__((aligned(128))) CardHeader {
  long long last_ts;               // time of the card's last event (sliding: last appended; redis: last write)
  unsigned char ring_n, ring_head; // sliding: events held (<= K), next write position
  unsigned char unsorted;          // sliding: appends left before the ring is time-sorted again (0 = sorted)
  unsigned char pad0;
  unsigned char wc[3], pad1;       // sliding: events of the ring's newest suffix inside the 5m / 1h / 24h window
  unsigned flags;                  // bit 0 user profile; bit 1 redis session live; bits 8-15 LSTM events held;
                                   // bits 16-23 LSTM history write position
  int rc_cnt;                      // redis_compat: session count
  long long ws[3];                 // sliding: window sums (cents); redis_compat: ws[0] is the session amount
  unsigned wod[3];                 // sliding: last_ts - time of the oldest in-window event (valid when wc > 0)
  unsigned pad2;
  unsigned long long key;          // 0 = empty slot
  double avg;                      // profile: avg_transaction_amount (NaN = null)
  int age;                         // profile: account_age_days
  int pad3;
  unsigned long long fp[3];        // profile: device fingerprints (0 = none)
  long long pad4[2];
};
static_assert(sizeof(CardHeader) == 128, "CardHeader must be one 128-B line");
static_assert(offsetof(CardHeader, key) == 64 && offsetof(CardHeader, wod) + sizeof(unsigned) * 3 <= 64,
              "the mutable fields in bytes 0-63, the key at 64 (snapshot.hip reads it there)");
constexpr int kCardHeaderBytes = (int)sizeof(CardHeader);

// one event of a card's ring (sliding windows): time and cents
struct __attribute__((aligned(16))) RingEvent {
  long long ts;
  long long cents;
};

// The card table's state pages: slot s owns bytes [s * stride, (s + 1) * stride) of one allocation — its
// 128-B header, then (sliding mode) its K ring events of 16 B. A transaction's state (header and the ring
// entries it evicts / appends) lies in one contiguous page: one address translation per card instead of one
// per array (round 4; before, headers and rings were two arrays of their own).
struct CardPages {
  char* base;
  long long stride;  // bytes per slot: 128 + 16 K (sliding), 128 (redis_compat)
  __host__ __device__ __forceinline__ CardHeader* hdr(long long s) const {
    return reinterpret_cast<CardHeader*>(base + s * stride);
  }
  __host__ __device__ __forceinline__ RingEvent* ring(long long s) const {
    return reinterpret_cast<RingEvent*>(base + s * stride + kCardHeaderBytes);
  }
};

#ifdef __HIP_DEVICE_COMPILE__
#define FD_CARD_SLOT_QUAL __device__ __forceinline__
#else
#define FD_CARD_SLOT_QUAL __device__ inline
#endif
// Card-table probe (murmur3 fmix64 home slot, linear probing) over the compact key array `keys` (8 B per slot,
// CardStore::keys): the probes' random accesses stay inside 8 x capacity bytes, a range the GPU's TLBs reach,
// instead of the 128-B headers. The probe sequence is read as aligned groups of 8 keys (64 B, four 16-B loads in
// flight): at the bench's load factor (~0.75, where a linear probe runs ~2.5 slots on a hit and ~8 on a miss) one
// dependent load round instead of one per slot. A key seen as 0 is claimed by CAS, whose result also corrects a
// stale read (another CU's insert): it returns the key that is there. An insert mirrors the key into the slot's
// header (snapshots and occupancy read it there). Returns the slot, -1 when the table is full.
FD_CARD_SLOT_QUAL long long card_slot(unsigned long long* keys, CardPages pg, long long mask, unsigned long long key) {
  if (key == 0ull) key = 1ull;  // 0 marks an empty slot
  long long h = (long long)(fmix64(key) & (unsigned long long)mask);
  if (mask >= 7) {
    long long g = h & ~7ll;
    int j0 = (int)(h & 7);
    for (long long p = 0; p <= mask + 8; p += 8) {  // the first group twice: its slots before j0 come last
      const uint4* q = reinterpret_cast<const uint4*>(keys + g);
      uint4 w[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) w[u] = q[u];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        if (j < j0) continue;
        const uint4 v = w[j >> 1];
        const unsigned long long k = (j & 1) ? (((unsigned long long)v.w << 32) | v.z)
                                             : (((unsigned long long)v.y << 32) | v.x);
        if (k == key) return g + j;
        if (k == 0ull) {
          const unsigned long long old = atomicCAS(&keys[g + j], 0ull, key);
          if (old == 0ull) {
            pg.hdr(g + j)->key = key;
            return g + j;
          }
          if (old == key) return g + j;
        }
      }
      j0 = 0;
      g = (g + 8) & mask;
    }
    return -1;
  }
  for (long long p = 0; p <= mask; ++p) {
    const unsigned long long k = __hip_atomic_load(&keys[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (k == key) return h;
    if (k == 0ull) {
      const unsigned long long old = atomicCAS(&keys[h], 0ull, key);
      if (old == 0ull) {
        pg.hdr(h)->key = key;
        return h;
      }
      if (old == key) return h;
    }
    h = (h + 1) & mask;
  }
  return -1;
}

// HBM-resident keyed card state (features.hip)
struct CardStore {
  bool ready = false;
  int64_t cap = 0;   // slots (power of two)
  int mode = 0;      // fd_window_mode
  int K = 1;         // ring events per card (sliding)
  int S = 0;         // LSTM history events per card (0 = off)
  int bucket_keys = 0;  // option "bucket_keys": transactions per bucket workgroup (0 auto, features.hip)
  bool bucket_spread = true;  // option "bucket_spread": a bucket's card segments dealt over all 4 waves
  // option "slot_gather": batches of <= 4096 transactions outside the pipelined stream find their card slots inside
  // the bucket kernel (each bucket workgroup takes the keys that hash to it), no slot launch (features.hip)
  bool slot_gather = true;
  // option "lean_group": how the lean bucket kernel groups a bucket's keys by card — 0 rank sort, 1 rank sort split
  // over every thread (rank_sort_split), 2 (default) LDS hash table (no sort)
  int lean_group = 2;
  bool slot_prio = false;  // option "slot_prio": the pipelined stream's slot kernel issues at priority 2
  bool feat_prio = false;  // option "feature_prio": the pipelined stream's lean bucket kernel issues at priority 2 (the
                           // default in round 5; off since round 6's split rows, engine.hip)
  int64_t n_merchants = 0;
  DeviceBuffer pages, keys, merchants, err, seq;  // pages: CardPages (header + ring per slot); keys: the compact
                                                  // key array card_slot probes
  long long page_bytes = kCardHeaderBytes;
  CardPages view() const { return CardPages{static_cast<char*>(pages.ptr), page_bytes}; }
  DeviceBuffer sat;  // u64: transactions whose 24 h window held K prior events (counter "window_saturated")
  // per-batch card grouping (feat_slot -> feat_bucket): per-txn slots, keys per bucket, [NB][C] bucket regions,
  // overflow counters by batch parity + the overflow list (key, bucket), prep records. Two sets: the pipelined
  // stream alternates them, so batch i+1's slot kernel runs while batch i's bucket kernel still reads its set.
  struct GroupScratch {
    DeviceBuffer slot, bucket_fill, pairs, ovf_cnt, ovf_key, ovf_b, prep;
    int batch_parity = 0;
  } gs[2];
  DeviceBuffer bucket_scr;  // lean bucket kernel: per-bucket global working set of its slow path
  DeviceBuffer uext, mext, vocab;  // extended profiles + vocabulary flags (feature map, rule scores)
  int64_t n_mext = 0;
  bool vocab_loaded = false;
  double tp_threshold = 0.7;  // JobConfig.fraudThreshold (fl/config/JobConfig.java:47)
};

// Flink window aggregates (windows.hip): device event logs (double-buffered for compaction), sort scratch
struct WindowState {
  bool ready = false;
  int64_t cap = 0, cand_cap = 0;
  int64_t ooo = 10000;                    // watermark lag (ms)
  int64_t wm = INT64_MIN;                 // current watermark
  int64_t min_seen = INT64_MAX;           // smallest event time added (bases the first firing's keys)
  int64_t max_seen = INT64_MIN;           // largest event time added (flush) or observed (sharded)
  bool observed = false;                  // fd_windows_observe since the last step: advance even with n == 0
  DeviceBuffer ulog[2], mlog[2];
  int ucur = 0, mcur = 0;
  int64_t ucount = 0, mcount = 0;
  DeviceBuffer keys, vals, sort_tmp, uout, mout, scalars;
};

// RedisTransactionSink bucket aggregates (sink.hip)
struct SinkState {
  bool ready = false;
  unsigned long long cap = 0, ucap = 0;
  DeviceBuffer table, users, err;
};

// JSON ingest codec lookup tables (ingest.hip): merchant ids and the three vocabularies, hash -> index
struct IngestTables {
  DeviceBuffer mkeys, mvals, vkeys[3], vvals[3];
  unsigned long long mmask = 0, vmask[3] = {0, 0, 0};
  bool mloaded = false, vloaded[3] = {false, false, false};
  int stop_after = 0;  // diagnostics option "ingest_stop_after"
};

// the engine's own RCCL communicators and buffers for the sharded step (comm.hip, sharded_step there);
// per-batch buffers in two slots (a step's batch and the next one, prefetched)
struct ShardComm {
  bool ready = false;
  // a step that timed out or failed on the device aborts both communicators (ncclCommAbort: RCCL's blocked
  // kernels exit) before it throws, so no stream is left parked on a peer; afterwards the engine refuses sharded
  // steps, and its syncs / fd_comm_destroy wait on the forward stream only up to comm_timeout_ms
  bool aborted = false;
  std::string abort_reason;
  int rank = 0, world = 1;
  const void* api = nullptr;  // the RcclApi (comm.hip) of the library fd_comm_init was given
  void* fwd = nullptr;   // ncclComm_t: counts + records, on x_fwd
  void* back = nullptr;  // ncclComm_t: results, on the engine stream
  hipStream_t x_fwd = nullptr;
  DeviceBuffer rec[2], cnt[2], back_buf;
  // received records: a ring of three inboxes, so a batch's records exchange waits for the scoring three batches
  // back (long done) instead of two (still running beside the pipeline) — x_fwd is then never parked on an inbox,
  // and the next batch's counts queued behind the records are not held up either (the process has 4 hardware
  // queues for 4+ streams: a parked stream stalls whatever shares its queue)
  static constexpr int kInbox = 3;
  DeviceBuffer inbox[kInbox];
  // the owner's result records, by inbox: the fused kernel writes them in place (round 6: no staging copy). Batch i's
  // scoring follows its records' arrival (in_ev), which followed x_fwd's wait for inbox_ev of batch i - 3 — recorded
  // after that batch's results exchange — so res[q] is free when batch i writes it, with no event of its own
  DeviceBuffer res[kInbox];
  hipEvent_t in_ev[kInbox] = {}, inbox_ev[kInbox] = {};  // records arrived / the engine stream passed their results
  bool inbox_live[kInbox] = {};
  int inbox_next = 0;                                     // the next batch's inbox
  int inbox_of[2] = {0, 0};                               // slot s's batch's inbox
  DeviceBuffer route_blk;                  // the partition's block counts (x_fwd)
  // coherent host-mapped memory per slot: send counts [G], receive counts [G] (FD_MAX_SHARDS each), then a u64
  // sequence word; count_publish_kernel writes the counts and then the sequence, the host polls the sequence
  int64_t* h_cnt[2] = {nullptr, nullptr};
  int64_t* d_hcnt[2] = {nullptr, nullptr};  // the same buffers' device addresses
  unsigned long long cnt_seq[2] = {0, 0};  // the sequence the slot's latest publish writes
  // the prefetched batch (fd_sharded_step's `next`): its caller-given id, size and count slot; its counts are in
  // flight on x_fwd. A later call names it by that id (never by its address: torch's allocator recycles them).
  bool pending = false;
  unsigned long long pending_id = 0;
  int64_t pending_n = 0;
  int pending_slot = 0, next_slot = 0;
  int64_t split[2][2 * FD_MAX_SHARDS] = {};  // a slot's checked split sizes, send [G] then recv [G]
  // Every communicator operation of a step is issued by the calling thread, in one fixed order on every rank
  // (counts of batch i+1, records of batch i on x_fwd; results of batch i on the engine stream): RCCL kernels block
  // on their peers, and ops of two communicators issued from two threads could reach a shared hardware queue in
  // opposite orders on two ranks. (Round 3 ran the next batch's forward half on a worker thread; it measured no
  // faster - 0.0932 vs 0.0943 ms per step, profiles/r03/route_overhead_stream_priority_p1.log - and had that hazard.)
  int64_t timeout_ms = 120000;  // option "comm_timeout_ms": the split-size wait gives up (FD_ERR_HIP) after this
  // option "count_exchange": 1 a batch's per-peer counts travel as ONE ncclAllGather of every rank's send vector
  // (cnt[s]: send [G], then the G x G matrix), issued right after the records group; 0 as 2G point-to-point
  // operations inside it (send [G], receive [G]); -1 (default) the all-gather from 4 ranks (a separate RCCL launch
  // costs ~2 us more host time than the world-1 group's two self operations; at 8 ranks it replaces 16)
  int count_mode = -1;
  bool count_gather = false;  // the form in use (count_mode, world)
  int device = 0;
  // host time inside fd_sharded_step by phase (ns, counters "sharded_host_ns_<phase>", kShardHostPhase order)
  static constexpr int kHostPhases = 8;
  std::atomic<unsigned long long> steps{0}, host_ns[kHostPhases] = {};
  std::atomic<unsigned long long> ops{0};  // RCCL operations issued (send, recv, all-gather; counter "rccl_ops")
};
// "wait": the split sizes; "partition", "counts", "count_copy": a batch's route kernels, count exchange and copy to
// the host; "records": the records exchange; "score": the owner's pipeline; "back", "scatter": results
inline const char* const kShardHostPhase[ShardComm::kHostPhases] = {
    "wait", "partition", "counts", "count_copy", "records", "score", "back", "scatter"};
// per-thread phase clock: lap(ph) adds the time since the previous lap to phase ph
struct HostLaps {
  ShardComm& c;
  std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
  void operator()(int ph) {
    const auto now = std::chrono::steady_clock::now();
    c.host_ns[ph].fetch_add((unsigned long long)std::chrono::duration_cast<std::chrono::nanoseconds>(now - t).count(),
                            std::memory_order_relaxed);
    t = now;
  }
};

inline int64_t floor_div_host(int64_t a, int64_t b) {
  int64_t q = a / b;
  if ((a % b != 0) && ((a < 0) != (b < 0))) --q;
  return q;
}

// ---- the arguments of the scoring schedulers (score.hip), named. Host side only: passed by const&, never a
// kernel's parameter (the launch sites hand the kernels the members).

// The models of one scoring call: blend parameters, slots[m] (a forest slot, FD_SLOT_LSTM, FD_SLOT_MLP, or < 0 for an
// external probability column ext[m]) and present[m] (null: all present). The public fd_ab_model_set's four members.
struct ModelSet {
  const fd_blend_params* params = nullptr;
  const int32_t* slots = nullptr;
  const double* const* ext = nullptr;
  const uint8_t* present = nullptr;
  ModelSet(const fd_blend_params* p, const int32_t* s, const double* const* x, const uint8_t* pr)
      : params(p), slots(s), ext(x), present(pr) {}
  explicit ModelSet(const fd_ab_model_set& s) : ModelSet(s.params, s.slots, s.ext_probs, s.present) {}
  int n_models() const { return params->n_models; }
  bool has(int m) const { return !(present && !present[m]); }
  // model m sits in a forest slot (present or not; the slot may still be out of range: slot_of checks)
  bool forest(int m) const { return slots[m] >= 0 && slots[m] != FD_SLOT_LSTM && slots[m] != FD_SLOT_MLP; }
  bool external(int m) const { return slots[m] < 0 && has(m); }  // present and scored by the caller: ext[m]
  bool wants_lstm() const {  // a present model is the LSTM head: the batch needs card-history sequences
    for (int m = 0; m < n_models() && m < FD_MAX_MODELS; ++m)
      if (slots && slots[m] == FD_SLOT_LSTM && has(m)) return true;
    return false;
  }
  bool all_in_slots() const {  // no present model is external (routed scoring has no place for a column)
    for (int m = 0; m < n_models() && m < FD_MAX_MODELS; ++m)
      if (external(m)) return false;
    return true;
  }
};
// one text per entry point ("n_models out of range" / "bad n_models"): the helper takes it
inline void require_model_count(const fd_blend_params& p, const char* text) {
  FD_REQUIRE(p.n_models > 0 && p.n_models <= FD_MAX_MODELS, FD_ERR_INVALID_ARG, text);
}
inline void require_all_in_slots(const ModelSet& ms) {
  FD_REQUIRE(ms.all_in_slots(), FD_ERR_INVALID_ARG,
             "routed scoring needs every present model in a forest slot, FD_SLOT_LSTM or FD_SLOT_MLP");
}

// The outputs of one scoring call: the per-model matrix (n_models x n, column-major; optional) and the four blended
// columns (fp required where columns are written at all; the others optional)
struct ScoreOut {
  double* mp = nullptr;
  double* fp = nullptr;
  double* conf = nullptr;
  uint8_t* dec = nullptr;
  uint8_t* risk = nullptr;
  // the same columns from row `first` on, nulls staying null; the matrix of those rows is the caller's to name
  ScoreOut rows_from(int64_t first, double* mp_rows = nullptr) const {
    return {mp_rows, fp ? fp + first : nullptr, conf ? conf + first : nullptr, dec ? dec + first : nullptr,
            risk ? risk + first : nullptr};
  }
};

// The rows score_matrix scores: the matrix, and what only some callers have — the LSTM head's sequences (n x T x 16,
// with the latency path's descriptors), the routed records with the result records to write, compact / split rows
struct ScoreRows {
  const float* X;
  int64_t n;
  int32_t ld;
  ScoreRows(const float* X_, int64_t n_, int32_t ld_) : X(X_), n(n_), ld(ld_) {}
  const float* seq = nullptr;
  int T = 0;
  const unsigned long long* seq_desc = nullptr;
  const RouteRecord* records = nullptr;
  ResultRecord* results = nullptr;
  int compact = 0;  // 1 / 2: X holds compact / split rows (launch_ensemble), the fused kernel only
};

// One micro-batch of the pipelined stream (pipe_step): transaction columns (txns) whose scores go to `out` (and the
// vectors to d_vectors), or routed 48-B records whose scores leave as 24-B result records in d_results
struct PipeBatch {
  const fd_txn_batch* txns = nullptr;
  const void* records = nullptr;
  int64_t n = 0;
  float* d_vectors = nullptr;
  ScoreOut out;
  void* d_results = nullptr;
  void* input_ready = nullptr;    // hipEvent_t: the inputs are complete
  bool results_in_place = false;  // d_results is the engine's own buffer: no staging copy (fd_sharded_step)
};

// score_matrix's side streams: [0] the LSTM head (and, small_streams 1, every forest after the first), [1] small
// batches under small_streams 2: the forests after the first. Created on first use.
struct SideStreams {
  hipStream_t st[2] = {};
  hipEvent_t fork_ev = nullptr, join_ev[2] = {};
  void fork(int k, hipStream_t from);  // st[k] after everything queued on `from` so far
  hipEvent_t mark(int k);              // an event recorded on st[k] now
  void join(int k, hipStream_t to);    // `to` after everything queued on st[k] so far
  void release();
};

// The pipelined stream (fd_score_batch_pipelined / fd_score_records_pipelined / fd_sharded_step; score.hip pipe_step):
// features and scoring of batch i on stream[i & 1] (no cross-stream wait between a batch's features and its forests;
// batch i-1's features waited for by event); vectors / LSTM sequences double-buffered by batch parity
struct Pipeline {
  static constexpr int kSlots = 2;
  hipStream_t stream[2] = {nullptr, nullptr};
  // batch i's scoring-done event is done_ev[i mod kDoneRing]: the engine stream, the next batch of a per-model
  // scoring path and — split rows — batch i + 4's slot pass (which rewrites the ring buffer batch i's fused kernel
  // read) wait on it
  static constexpr int kDoneRing = 4;
  hipEvent_t entry_ev = nullptr, feat_ev[kSlots] = {}, done_ev[kDoneRing] = {};
  bool feat_live[kSlots] = {}, done_live[kDoneRing] = {};
  bool dirty = true;  // another engine call since the last pipelined one: order after the engine stream first
  // option "slot_stream" (0 off, 1 high-priority stream, 2 low): batch i's slot pass on a stream of its own, so it
  // does not queue behind batch i-2's fused kernel on stream[i & 1]; its bucket pass waits for it by event.
  // -1 (default) auto: 2 when the card table has >= 2^26 slots, else 0. Config 4 (2^27 slots): 0.0915 -> 0.0897 ms
  // per step at 2 (1: 0.0906); config 3 (10 M cards): 0.0876 -> 0.0948
  int slot_mode = -1;
  hipStream_t slot_stream = nullptr;
  hipEvent_t slot_ev[kSlots] = {};
  // launch_grouped's slot pass goes to this stream (then an event the bucket pass's stream waits for) while set
  hipStream_t slot_pass_stream = nullptr;
  hipEvent_t slot_pass_ev = nullptr;
  unsigned long long iter = 0;
  unsigned long long iter_total = 0;         // counter "pipelined_batches"
  unsigned long long compact_total = 0;      // counter "pipelined_compact_batches": batches scored from compact vectors
  unsigned long long split_total = 0;        // counter "pipelined_split_batches": of those, split rows
  unsigned long long host_ns = 0;            // counter "pipelined_host_ns": host time inside fd_score_batch_pipelined
  unsigned long long slot_stream_total = 0;  // counter "pipelined_slot_stream_batches": slot pass on its own stream
  bool lean = true;    // "pipeline_lean" option: lean bucket kernel (fits beside the ensemble kernel)
  bool gather = true;  // "pipeline_gather" option: batches of <= kGatherBatchMax take the gather bucket kernel
  DeviceBuffer vec[kSlots], seq[kSlots];
  // split rows (compact_vectors 2): RowA | RowB of batch i in ring buffer i mod kSplitRing. With the slot pass on its
  // own stream, batch i's slot kernel writes RowA while batch i - 2's fused kernel (the same vec parity) may still
  // read its rows — the slot stream waits only for batch i - 2's bucket pass — so the split rows get a deeper ring,
  // and the slot pass waits for the fused kernel that last read its buffer (batch i - 4's done_ev: long done)
  static constexpr int kSplitRing = 4;
  static_assert(kSplitRing == kDoneRing, "the split-row ring's buffers are released by the done events");
  DeviceBuffer split[kSplitRing];
  // the scoring streams write a batch's outputs into out[slot]; one copy kernel on the engine stream moves them to
  // the caller's buffers, so the caller's memory is written only in the engine stream's order (torch's caching
  // allocator may hand batch i's freed outputs to batch i+1); batch i+2's scoring waits for copy_ev[slot]
  DeviceBuffer out[kSlots];
  hipEvent_t copy_ev[kSlots] = {};
  bool copy_live[kSlots] = {};
  bool copy_vec[kSlots] = {};  // that copy also read the slot's vectors (the slot's next features wait)
  // first use: the streams (option stream_priority) and events; slot_mode -1 resolved by the card table's size
  void create(int stream_prio, bool big_table);
  void release();  // streams drained and destroyed, events destroyed (~Engine)
  // stream s after the scoring of every pipelined batch so far (a new engine stream inherits the old one's order)
  void order_after_scoring(hipStream_t s);
};

struct Engine {
  int device = 0;
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;
  PackedForest forests[kMaxSlots];
  CardStore state;
  LstmModel lstm;
  MlpModel mlp;
  unsigned long long mlp_total = 0;  // counter "mlp_launches"
  GraphState graph;
  TextState text;
  AbState ab;
  MetricsCollector metrics;
  WindowState windows;
  IngestTables ingest;
  SinkState sink;
  SideStreams side;                            // score_matrix's side streams (score.hip)
  DeviceBuffer seq_buf;                        // per-txn LSTM input sequences of the fused path
  DeviceBuffer seq_desc;                       // latency path: per-txn sequence descriptors (kSeqMaterialized)
  DeviceBuffer feat_vec, feat_ext;  // feature vectors of the scoring entry points / extended-feature scratch
  Pipeline pipe;                               // the pipelined stream (score.hip pipe_step)
  unsigned long long sparse_total = 0;        // counter "forest_sparse_launches": launches of forest_sparse_kernel
  unsigned long long shap_total = 0;          // counter "forest_shap_launches": launches of shap_kernel
  DeviceBuffer shap_partial;                  // shap.hip: per-chunk sums of one row batch, [chunk][column][row]
  GbdtScratch gbdt;                           // gbdt.hip: the fit's device buffers and counters
  IForestFitScratch iforest;                  // iforest_fit.hip: the fit's device buffers and counters
  MlpFitScratch mlp_fit;                      // mlp_fit.hip: the fit's device buffers, option and counters
  unsigned long long ens_single_total = 0;    // counter "ensemble_single_launches": fd_forest_predict batches run by
                                              // the fused kernel over one forest (config 2's timed kernel)
  int small_streams = 0;  // score_matrix, latency batches: side streams for the LSTM / other forests (score.hip)
  bool latency_fused = true;  // "latency_fused": latency pair walk + sums + blend in 2 launches (forest.hip)
  bool seq_ring_lstm = true;  // "seq_ring_lstm": latency batches' LSTM reads card histories from the ring
  bool latency_prebin = true;  // "latency_prebin": the latency pair's binning in the LSTM head's launch (PreBin)
  int latency_prebin_mode = 3;  // its value: 1 the binning workgroups ahead of the LSTM's, 2 after them, 3 (default)
                                // the searches inside the LSTM's own workgroups (lstm.hip InlineSearch; 2 where a
                                // thread would take more than two)
  PreBin prebin;
  unsigned long long prebin_total = 0;  // counter "latency_prebinned_batches"
  bool ens_prio = true;   // "ensemble_prio": the fused kernel's waves issue at priority 2 (above the feature kernels;
                          // the default since round 6's split rows, score.hip pipe_step)
  bool ens_bin_global = false;  // "ensemble_bin_global": compact rows binned by searches in global memory (no staging)
  int compact_vectors = 2;      // "compact_vectors": the pipelined stream's scoring rows for the fused kernel when
                                // nobody asked for vectors: 0 the 64-wide vector, 1 compact 64-B rows, 2 split rows
                                // (card-independent half from the slot pass; score.hip pipe_step, features.hip Prep32)
  int stream_prio = 3;    // option "stream_priority": the pipeline / forward streams' HIP priorities (score.hip Pipeline::create, comm.hip)
  DeviceBuffer stage;          // the host (`_host`) entry points' staged inputs and outputs (engine.hip Stage)
  DeviceBuffer scratch_probs;  // score_matrix per-model columns
  DeviceBuffer route_blk, route_out, route_err;  // card-hash routing scratch (route.hip)
  DeviceBuffer route_blk_stream;                 // fd_route_partition_stream's block counts (its own stream)
  ShardComm comm;                                // card-hash sharding over RCCL (comm.hip)
  EnsemblePlan ens;                              // fused XGBoost + IsolationForest + blend (ensemble.hip)
  EnsemblePlan ens1[kMaxSlots];                  // the same kernel over one forest (forest predict), per slot
  bool route_err_live = false;
  // optional per-launch kernel timing (HIP events on the launch stream)
  int forest_variant = 0;  // "forest_kernel" option
  bool ens_owner_fixed = true;  // "ensemble_owner" option (A/B of the fused kernel's chunk-owner schedule)
  int ens_chunks = 0;           // "ensemble_chunks": 0 auto, 1 wide, 2 compact chunk layout (ensemble.hip)
  int ens_contract = 4;         // "ensemble_contract": compact / split rows walk the forests contracted against the
                                // constant slots: 0 no, 1 each tree to its wave's deepest, 2 to its own depth, 3 / 4
                                // the dense chunk stream (bundles of consecutive trees / 4, default: sorted by depth)
  unsigned long long ens_contract_total = 0;  // counter "ensemble_contracted_launches"
  int ens_dense_chunks_last = 0;  // counter "ensemble_dense_chunks": chunks of the last fused pair launch, if dense
  long long ens_steps_last = 0;  // counter "ensemble_node_steps_per_txn": node steps per transaction of the last fused launch
  int mlp_form = 0;        // "mlp_form" option: 0 auto, 1 the LDS form (mlp_lds_kernel) for the reference shape too
  int mlp_wgs_per_cu = 0;  // "mlp_wgs_per_cu" option: the MLP's persistent grid, workgroups per CU (0 auto: 2 where they fit)
  int lstm_rows = 0;  // "lstm_rows" option: transactions per LSTM workgroup tile (0 auto, 4 or 16)
  bool ensemble_on = true;  // "ensemble" option: the fused XGBoost + IsolationForest + blend kernel (auto)
  bool timing = false;
  int timing_every = 1;               // "timing_every" option: time one launch in N of each kind
  unsigned long long timing_seq[16] = {};
  struct Timed {
    hipEvent_t a, b;
    int kind;
    // a launch split over two streams (the pipelined slot pass on its own stream, then the bucket pass): its
    // second part is c..d, the launch's time the sum of both (the wait between them excluded)
    hipEvent_t c = nullptr, d = nullptr;
    bool split = false;
  };
  std::vector<Timed> events;  // pool
  size_t events_used = 0;
  void activate() const { FD_HIP(hipSetDevice(device)); }
  Timed* next_event_pair(int kind);
  ~Engine();  // engine.hip: the teardown whose order matters; the buffers then go with their owners
};

// forest.hip
struct HostPack {
  std::vector<char> blob;
  std::vector<int32_t> leaf_ids;
  int kind = 0, n_trees = 0, n_chunks = 0, chunk = 0, depth = 0, num_feature = 0;
  size_t tree_bytes = 0, chunk_stride = 0;
  float base_margin = 0.f;
  // binned layout
  bool binned = false;
  std::vector<char> b_blob;
  std::vector<float> b_thr;
  std::vector<int32_t> b_thr_off;
  int b_chunk = 0, b_n_chunks = 0, bin_steps = 0;
  size_t b_tree_bytes = 0, b_chunk_stride = 0;
  // node-only chunks (forest_kernel6); n_chunk == 0 when no supported chunk size fits
  std::vector<char> n_blob, n_leaves;
  int n_chunk = 0, n_n_chunks = 0;
  size_t n_chunk_stride = 0;
  std::vector<uint8_t> pad;  // [tree][2^D] heap slot is a pad node (a leaf above depth D): either way is right
};
// min_depth: pad every tree to at least this depth (the ensemble kernel's common depth)
HostPack pack_forest_host(const fd_forest_params& p, const fd_tree_arrays& t, int min_depth = 0);
void repack_forest(PackedForest& pf, const fd_forest_params& p, const fd_tree_arrays& t);
// sklearn's (double)x <= thr as the engine's f32 "x < t" (forest.hip)
float sklearn_threshold_to_lt(double thr);
// forest_sparse.hip: the sparse (pointer) layout for trees of any depth (include/fdengine.h fd_pack_forest_sparse_host)
struct SparsePack {
  std::vector<uint32_t> nodes;    // 2 words per node: f32 threshold bits, meta
  std::vector<char> leaf_val;     // n_leaves values: f32 XGBoost, f64 the sklearn kinds
  std::vector<int32_t> leaf_ids;  // n_leaves original node ids
  int kind = 0, n_trees = 0, depth = 0, num_feature = 0, leaf_bytes = 0;
  int64_t n_nodes = 0, n_leaves = 0;
  float base_margin = 0.f;
};
SparsePack pack_forest_sparse_host(const fd_forest_params& p, const fd_tree_arrays& t);
// the deepest leaf of a well-formed forest (root = 0), -1 when the arrays are incomplete or not trees
int forest_depth_probe(const fd_tree_arrays& t);
// fd_load_forest for a forest that takes the sparse layout only
void load_forest_sparse(PackedForest& pf, const fd_forest_params& p, const fd_tree_arrays& t);
// forest_sparse_kernel over the forest on `stream` (the image is built first when the forest has none yet)
void launch_forest_sparse(Engine& e, const PackedForest& pf, const float* d_X, int64_t n, int32_t ld, double* d_prob,
                          double* d_raw, int32_t* d_leaf, hipStream_t stream);
// two forests of a latency batch, one binning launch (forest.hip); false: not applicable, nothing launched
bool launch_forest_pair(Engine& e, const PackedForest& pa, const PackedForest& pb, const float* d_X, int64_t n,
                        int32_t ld, double* d_prob_a, double* d_prob_b);
void launch_forest(Engine& e, const PackedForest& pf, const float* d_X, int64_t n, int32_t ld,
                   double* d_prob, double* d_raw, int32_t* d_leaf, hipStream_t stream = nullptr);
// a latency batch's XGBoost + IsolationForest and the blend: bin (one launch), both walks (one launch), both
// sequential sums + blend_row over every present model (one launch); cols = the present models' probability columns
// in present order (the two forests' are written, the others read), pos1 / pos2 = p1's / p2's place in it.
// false: not applicable (not one of each kind on the split path at depth 8); nothing launched.
struct BlendConsts;
bool launch_forest_pair_blend(Engine& e, const PackedForest& p1, const PackedForest& p2, const float* d_X, int64_t n,
                              int32_t ld, const BlendConsts& bc, const double* const* cols, int pos1, int pos2,
                              const ScoreOut& out, hipEvent_t before_blend = nullptr);
// e.prebin for the pair launch_forest_pair_blend will run over d_X (n rows): false (e.prebin.want cleared) when it
// does not apply
bool forest_pair_prebin(Engine& e, const PackedForest& p1, const PackedForest& p2, const float* d_X, int64_t n,
                        int32_t ld);
// windows.hip
void windows_init(Engine& e, const fd_window_params& p);
void windows_step(Engine& e, const fd_txn_batch& t, const fd_window_inputs& in, int64_t n, bool flush,
                  fd_user_window* u_out, int64_t u_cap, int64_t* n_user, fd_merchant_window* m_out, int64_t m_cap,
                  int64_t* n_merch, bool timed = false);  // timed: an FD_TIMING_WINDOWS event pair around the step
void windows_observe(Engine& e, int64_t max_event_ts);
void merchant_windows_merge(const fd_merchant_window* p, int64_t n, fd_merchant_window* out, int64_t* n_out);
// ingest.hip
void ingest_set_vocab(Engine& e, int which, const uint8_t* bytes, const int64_t* offsets, int64_t n);
void ingest_set_merchants(Engine& e, const uint8_t* bytes, const int64_t* offsets, int64_t n);
void launch_ingest(Engine& e, const uint8_t* d_bytes, const int64_t* d_offsets, int64_t n, const fd_ingest_out& out);
// sink.hip
void sink_init(Engine& e, const fd_sink_params& p);
void sink_update(Engine& e, const fd_txn_batch& t, const fd_window_inputs& in, int64_t n);
void sink_query(Engine& e, int kind, const int64_t* bucket, const int32_t* merchant, int64_t n, fd_aggregate* out);
void sink_evict_before(Engine& e, int64_t hour, int64_t* kept_entries, int64_t* kept_users);
// snapshot.hip
void state_snapshot(Engine& e, const char* path, int shard, int n_shards, int64_t* bytes_written);
void state_restore(Engine& e, const char* path, int shard, int n_shards, int flags, int64_t* cards_restored);
// features.hip
void state_init(Engine& e, const fd_state_params& p);
void state_clear(Engine& e);
int64_t state_count(Engine& e);
void load_users(Engine& e, const fd_users& u);
void load_merchants(Engine& e, const fd_merchants& m);
// compact: 0 the 64-wide vector; 1 the fused pipeline's compact form (64-B rows: kCompactWidth words, fd_internal.h);
// 2 split rows (features.hip Prep32 / RowA / RowB: RowA [n] then RowB [n], 32 B each; lean bucket pass only)
void launch_features(Engine& e, const fd_txn_batch& t, int64_t n, float* d_vec, double* d_raw,
                     float* d_seq = nullptr, double* d_vel5 = nullptr, hipStream_t stream = nullptr,
                     bool lean = false, int set = 0, hipEvent_t before_buckets = nullptr, int compact = 0,
                     unsigned long long* d_seq_desc = nullptr);
// the same over received 48-B route records (route.hip), no unpack pass; also returns nothing else
void launch_features_records(Engine& e, const void* d_records, int64_t n, float* d_vec, float* d_seq,
                             hipStream_t stream = nullptr, bool lean = false, int set = 0,
                             hipEvent_t before_buckets = nullptr, int compact = 0);
void load_users_ext(Engine& e, const fd_users_ext& u);
void load_merchants_ext(Engine& e, const fd_merchants_ext& m);
void load_vocab(Engine& e, const uint8_t* pay_high_risk, const uint8_t* type_refund);
void launch_features_full(Engine& e, const fd_txn_batch& t, const fd_txn_context& c, int64_t n, float* d_vec,
                          double* d_raw, double* d_fmap, fd_rule_scores* d_rules);
void features_check(Engine& e);
// score.hip: the scoring schedulers behind fd_score_matrix_* / fd_score_batch_* / fd_score_records_* /
// fd_ab_score_matrix_* (device pointers; everything on e.stream unless said otherwise)
// a non-blocking stream at HIP priority level (+1 the greatest, -1 the least, 0 the default)
hipStream_t make_stream(int level);
PackedForest& slot_of(Engine& e, int slot);  // FD_ERR_INVALID_ARG when out of range
// every model of the set over the rows, then the blend. true: the route result records (rows.results) were written
// too (the fused ensemble kernel's epilogue); otherwise the caller packs them from the columns
bool score_matrix(Engine& e, const ModelSet& ms, const ScoreRows& rows, const ScoreOut& out);
// features (card state updated) -> score_matrix; d_vectors null: the vectors stay in engine scratch
void score_batch(Engine& e, const ModelSet& ms, const fd_txn_batch& t, int64_t n, float* d_vectors,
                 const ScoreOut& out);
// the same over routed 48-B records, the scores leaving as 24-B result records
void score_records(Engine& e, const ModelSet& ms, const void* d_records, int64_t n, void* d_results);
// score_matrix with one model set per A/B variant, results in arrival order (waits once, for the partition's counts)
void ab_score_matrix(Engine& e, int id, const fd_ab_model_set& c, const fd_ab_model_set& t, const float* dX,
                     const uint64_t* d_keys, int64_t n, int32_t ld, uint8_t* d_variant, const ScoreOut& out);
// one micro-batch of the pipelined stream: features and scoring on the pipeline's streams, outputs on e.stream
void pipe_step(Engine& e, const ModelSet& ms, const PipeBatch& b);
// route.hip
unsigned shard_of_host(unsigned long long key, unsigned G);
// stream / scratch: the launch stream and block-count scratch (default: the engine stream and route_blk)
void launch_route_partition(Engine& e, const fd_txn_batch& t, const fd_window_inputs* extra, int64_t n, int G,
                            void* d_records, int64_t* d_counts, hipStream_t stream = nullptr,
                            DeviceBuffer* scratch = nullptr, bool timed = true);
// the sharded step's split form of the partition: block counts + per-shard totals added into `totals` (zero on
// entry) first, so the count exchange can start; then the scan + record scatter (blk: the same scratch)
void launch_route_count(const fd_txn_batch& t, int64_t n, int G, int64_t* totals, hipStream_t st, DeviceBuffer& blk);
// the sharded step's split sizes to the host (comm.hip): cnt[0, 2G) -> host-mapped h, the send half zeroed for the
// next count, then the sequence word h_seq = seq (release); run by the scan kernel of launch_route_place
struct CountPublish {
  int64_t* cnt;
  int G;
  int gather_rank;  // >= 0: the receive counts are column gather_rank of the all-gathered matrix at cnt + G
  int64_t* h;
  unsigned long long* h_seq;
  unsigned long long seq;
};
void launch_route_place(const fd_txn_batch& t, int64_t n, int G, void* d_records, hipStream_t st, DeviceBuffer& blk,
                        const CountPublish* pub = nullptr);
void launch_route_unpack(Engine& e, const void* d_records, const void* d_results, int64_t n, const fd_txn_batch& out,
                         uint8_t* pm, uint8_t* fraud, double* score);
// the blended columns of `cols` (its matrix unused) into result records / result records back into columns
void launch_result_pack(Engine& e, const ScoreOut& cols, const RouteRecord* records, int64_t n, void* d_results);
void launch_result_scatter(Engine& e, const void* d_results, int64_t n, const ScoreOut& out);
void route_check(Engine& e);
// comm.hip
void comm_unique_id(const char* rccl_path, uint8_t* out);
void comm_init(Engine& e, const char* rccl_path, int rank, int world, const uint8_t* id_fwd, const uint8_t* id_back);
void comm_destroy(Engine& e);
// ncclCommAbort both communicators (idempotent); reason is kept for the errors of later calls
void comm_abort(Engine& e, const std::string& reason);
// hipStreamSynchronize, or for an aborted engine a poll bounded by comm_timeout_ms (false: still busy)
bool comm_sync_stream(Engine& e, hipStream_t st);
void comm_launch_counts(Engine& e, const fd_txn_batch& t, int64_t n, hipEvent_t ready, int slot, HostLaps& L);
void comm_wait_counts(Engine& e, int slot, int64_t n, HostLaps& L);  // host wait; split[slot] checked
// a batch as fd_sharded_step names it: its columns, its id (0: not prefetched) and the event its inputs wait for
struct ShardBatch {
  const fd_txn_batch* txns;
  int64_t n;
  uint64_t id;
  hipEvent_t ready;
};
// records exchange of `slot` behind its inbox slot, + the next batch's count exchange in the same group
void comm_forward_group(Engine& e, int slot, const ShardBatch* next, int next_slot, HostLaps& L);
// one sharded step: this batch's counts (unless prefetched: cur.id names the pending batch), records out, the
// owner's pipe_step, results back into `out` in arrival order; `next`: the batch to prefetch the counts of
void sharded_step(Engine& e, const ModelSet& ms, const ShardBatch& cur, const ShardBatch* next, const ScoreOut& out,
                  int64_t* split_sizes);
void comm_exchange(Engine& e, bool back, hipStream_t st, const void* sendbuf, const int64_t* send, void* recvbuf,
                   const int64_t* recv, size_t elem);
// lstm.hip
void load_lstm(Engine& e, const fd_lstm_params& p);
// d_desc (latency path): per transaction its sequence's place — the card's history ring or row i of d_seq
// (features.hip seq_step); null: every row of d_seq
void launch_lstm(Engine& e, hipStream_t stream, const float* d_seq, int64_t n, int T, double* d_prob,
                 const unsigned long long* d_desc = nullptr);
// mlp.hip
std::vector<uint32_t> pack_mlp_host(const fd_mlp_params& p);  // validates (no device), include/fdengine.h
void load_mlp(Engine& e, const fd_mlp_params& p);
void launch_mlp(Engine& e, hipStream_t stream, const float* d_X, int64_t n, int32_t ld, double* d_prob);
// graph.hip
void graph_init(Engine& e, const fd_graph_params& p);
void graph_clear(Engine& e);
void graph_info(Engine& e, int64_t* total, int64_t* held);
void graph_step(Engine& e, const fd_txn_batch& t, int64_t n, double* d_out);  // device pointers, on e.stream
// text.hip
int64_t text_nonascii_rows(Engine& e);  // waits for the engine stream
void text_features(Engine& e, const uint8_t* d_bytes, const int64_t* d_off, int64_t n, double* d_feat,
                   uint8_t* d_patterns, uint8_t* d_status);  // device pointers, on e.stream; outputs may be null
// abtest.hip (device pointers, on e.stream)
const AbTest& ab_test(Engine& e, int id);  // FD_ERR_NOT_LOADED unless created
void ab_create(Engine& e, int id, const fd_ab_params& p);
void ab_destroy(Engine& e, int id);
void ab_clear(Engine& e, int id);
void ab_assign(Engine& e, int id, const uint64_t* d_keys, int64_t n, uint8_t* d_variant);
void ab_partition(Engine& e, const uint8_t* d_variant, int64_t n, int32_t* d_idx, int64_t* d_counts);
void ab_gather_rows(Engine& e, const float* d_X, const int32_t* d_idx, int64_t n, int32_t ld, float* d_Xp);
void ab_gather_column(Engine& e, const double* d_col, const int32_t* d_idx, int64_t count, double* d_out);
void ab_scatter_results(Engine& e, const AbScatter& a);
void ab_record(Engine& e, int id, const uint8_t* d_variant, const double* d_prediction, const uint8_t* d_decision,
               const double* d_time_ms, double time_scalar, const uint8_t* d_label, int64_t n);
void ab_state_read(Engine& e, int id, fd_ab_state* out);  // waits for the engine stream
// metrics.hip (device pointers, on e.stream)
size_t metrics_state_bytes(int32_t slots);
void metrics_check_params(const fd_metrics_params& p);  // FD_ERR_INVALID_ARG
void metrics_live(Engine& e);                           // FD_ERR_NOT_LOADED before metrics_init
void metrics_init(Engine& e, const fd_metrics_params& p);
void metrics_clear(Engine& e);
void metrics_check_record(const MetricsHeader& h, const void* fraud_prob, const void* decision,
                          const void* model_probs, int32_t n_models, double timestamp, int64_t n);
void metrics_record(Engine& e, const double* d_fraud_prob, const uint8_t* d_decision, const double* d_model_probs,
                    int32_t n_models, const double* d_time_ms, double time_scalar, double timestamp, int64_t n);
void metrics_query(Engine& e, double now, fd_metrics_summary* out);  // waits for the engine stream
// model_io.hip: the unchanged XGBoost 2.0.3 JSON model file, flattened (fdengine/forest.py semantics)
struct XgbModel {
  int num_feature = 0;
  double base_score = 0.5;
  std::vector<int64_t> offsets;
  std::vector<int32_t> left, right, feature;
  std::vector<double> threshold, leaf_value;
  std::vector<uint8_t> default_left;
  std::vector<double> cover;  // sum_hessian per node; empty when a tree of the file has none
};
void read_xgboost_json(const char* path, XgbModel& out);
// learner_model_param.base_score is stored in probability space; the margin it seeds is RegLossObj::ProbToMargin =
// -logf(1 / base_score - 1) evaluated in f32. The loader (forest.hip) and the fit (gbdt.hip) both start from this one.
inline float xgb_base_margin(double base_score) {
  const float bs = (float)base_score;
  return -logf(1.0f / bs - 1.0f);
}
// gbdt.hip: the histogram GBDT fit (include/fdengine.h "training"; the rule is gbdt_row.h). Host pointers unless named
// d_*; the grown trees are written to `out` in breadth-first numbering.
// threads: host threads the features are split over (the cuts do not depend on it)
int64_t gbdt_cuts_host(const float* X, int64_t n, int32_t ld, int32_t F, int32_t max_bin, std::vector<float>& cuts,
                       std::vector<int32_t>& offsets, int threads = 1);
void gbdt_check_params(const fd_gbdt_params& p, int64_t n, int32_t F, bool fit);
void gbdt_bin_ref_host(const float* X, int64_t n, int32_t ld, int32_t F, const float* cuts, const int32_t* offsets,
                       uint8_t* bins);
void gbdt_grad_ref_host(const float* margin, const uint8_t* y, int64_t n, int32_t* g, int32_t* h);
void gbdt_grad_weighted_ref_host(const float* margin, const uint8_t* y, int64_t n, double w, int32_t* g, int32_t* h);
void gbdt_grow_tree_ref_host(const uint8_t* bins, int64_t n, int32_t F, const float* cuts, const int32_t* offsets,
                             const int32_t* g, const int32_t* h, const uint8_t* row_mask, uint64_t feature_mask,
                             const fd_gbdt_params& p, const fd_gbdt_model& out, int64_t* n_nodes);
// ev: null, or the watched fit's arguments (fd_gbdt_fit_eval_*): its outputs are written
void gbdt_fit_ref_host(const float* X, const uint8_t* y, int64_t n, int32_t ld, int32_t F, const fd_gbdt_params& p,
                       const fd_gbdt_model& out, int64_t* n_nodes, float* margins, fd_gbdt_eval* ev = nullptr);
// the limits of fd_gbdt_eval for a fit of n rows -> whether it holds an eval set; host_labels: ev.y is read
bool gbdt_check_eval(const fd_gbdt_eval& ev, int64_t n, int32_t F, bool host_labels);
void gbdt_check_metric_labels(const uint8_t* y, int64_t n, int32_t metric);
double gbdt_metric_ref_host(const float* margin, const uint8_t* y, int64_t n, int32_t metric);
double gbdt_metric_device(Engine& e, const float* d_margin, const uint8_t* d_y, int64_t n, int32_t metric);
// ev's X, y, margins and best_margins are device pointers, metric_out a host pointer; h_X may be null
void gbdt_fit_eval_device(Engine& e, const float* d_X, const float* h_X, const uint8_t* d_y, int64_t n, int32_t ld,
                          int32_t F, const fd_gbdt_params& p, fd_gbdt_eval& ev, const fd_gbdt_model& out,
                          int64_t* n_nodes, float* d_margins);
void launch_gbdt_bin(Engine& e, const float* d_X, int64_t n, int32_t ld, int32_t F, const float* d_cuts,
                     const int32_t* d_offsets, uint8_t* d_bins);
void launch_gbdt_grad(Engine& e, const float* d_margin, const uint8_t* d_y, int64_t n, int32_t* d_g, int32_t* d_h);
void gbdt_grow_tree_device(Engine& e, const uint8_t* d_bins, int64_t n, int32_t F, const float* cuts,
                           const int32_t* offsets, const int32_t* d_g, const int32_t* d_h, const uint8_t* d_row_mask,
                           uint64_t feature_mask, const fd_gbdt_params& p, const fd_gbdt_model& out, int64_t* n_nodes);
void gbdt_fit_device(Engine& e, const float* d_X, const uint8_t* d_y, int64_t n, int32_t ld, int32_t F,
                     const fd_gbdt_params& p, const fd_gbdt_model& out, int64_t* n_nodes, float* d_margins);
// the same with the matrix also on the host (h_X: the cuts are computed from it without a copy back)
void gbdt_fit_staged(Engine& e, const float* d_X, const float* h_X, const uint8_t* d_y, int64_t n, int32_t ld,
                     int32_t F, const fd_gbdt_params& p, const fd_gbdt_model& out, int64_t* n_nodes, float* d_margins);

// iforest_fit.hip: the IsolationForest fit (include/fdengine.h "training: IsolationForest"; the rule is
// iforest_fit_row.h). Host pointers unless named d_*; the outputs are host arrays.
void iforest_fit_check(const fd_iforest_fit_params& p, int64_t n, int32_t ld, int32_t F);
int iforest_fit_psi(const fd_iforest_fit_params& p, int64_t n);
int64_t iforest_fit_capacity(const fd_iforest_fit_params& p, int64_t n);
void iforest_fit_check_finite(const float* X, int64_t n, int32_t ld, int32_t F);
void iforest_fit_ref_host(const float* X, int64_t n, int32_t ld, int32_t F, const fd_iforest_fit_params& p,
                          fd_tree_arrays& out, double* n_node_samples, fd_forest_params& forest, int64_t* n_nodes);
void iforest_fit_device(Engine& e, const float* d_X, int64_t n, int32_t ld, int32_t F, const fd_iforest_fit_params& p,
                        fd_tree_arrays& out, double* n_node_samples, fd_forest_params& forest, int64_t* n_nodes);
void iforest_fit_sample_ref_host(int64_t n, const fd_iforest_fit_params& p, int32_t tree, int32_t* rows, int32_t* psi);
void iforest_fit_sample_device(Engine& e, int64_t n, const fd_iforest_fit_params& p, int32_t tree, int32_t* rows,
                               int32_t* psi);
void iforest_fit_grow_tree_ref_host(const float* X, int64_t n, int32_t ld, int32_t F, const int32_t* rows, int32_t m,
                                    uint64_t feature_mask, const fd_iforest_fit_params& p, int32_t tree,
                                    fd_tree_arrays& out, double* n_node_samples, int64_t* n_nodes);
// d_X: the matrix on the device; rows: host ids (checked by the caller)
void iforest_fit_grow_tree_device(Engine& e, const float* d_X, int64_t n, int32_t ld, int32_t F, const int32_t* rows,
                                  int32_t m, uint64_t feature_mask, const fd_iforest_fit_params& p, int32_t tree,
                                  fd_tree_arrays& out, double* n_node_samples, int64_t* n_nodes);
// mlp_fit.hip: the MLP member's fit (include/fdengine.h "training: the PyTorch MLP member"; the counter-based rules
// are mlp_fit_row.h). Host pointers unless named d_*; the outputs are host arrays. fit: the whole fit's limits (else a
// gradient call's).
void mlp_fit_check(const fd_mlp_fit_params& p, int64_t n, int32_t ld, bool fit);
void mlp_fit_check_inputs(const float* X, const uint8_t* y, int64_t n, int32_t ld, const fd_mlp_fit_params& p);
void mlp_fit_ref_host(const float* X, const uint8_t* y, int64_t n, int32_t ld, const fd_mlp_fit_params& p,
                      fd_mlp_fit_out& out);
void mlp_fit_device(Engine& e, const float* d_X, const uint8_t* d_y, int64_t n, int32_t ld,
                    const fd_mlp_fit_params& p, fd_mlp_fit_out& out);
void mlp_grad_ref_host(const float* X, const uint8_t* y, int64_t n, int32_t ld, const fd_mlp_fit_params& p,
                       const uint8_t* masks, fd_mlp_fit_out& out);
void mlp_grad_device(Engine& e, const float* d_X, const uint8_t* d_y, int64_t n, int32_t ld,
                     const fd_mlp_fit_params& p, const uint8_t* d_masks, fd_mlp_fit_out& out);
void mlp_fit_batch_ref_host(int64_t n, const fd_mlp_fit_params& p, int32_t epoch, int64_t step, int32_t* order,
                            uint8_t* masks, int32_t* rows);
void mlp_fit_batch_device(Engine& e, int64_t n, const fd_mlp_fit_params& p, int32_t epoch, int64_t step,
                          int32_t* order, uint8_t* masks, int32_t* rows);
// shap.hip: path-dependent TreeSHAP (include/fdengine.h "forest attribution")
struct ShapTable {
  std::vector<fd_shap_path> paths;
  std::vector<fd_shap_elem> elems;
  fd_shap_info info{};
};
// "" when every node reachable from a root has a finite cover > 0, else the message naming the first that has not
std::string shap_cover_problem(const fd_tree_arrays& t, const double* cover);
ShapTable shap_paths_host(const fd_forest_params& p, const fd_tree_arrays& t, const double* cover);
void shap_ref_host(const fd_forest_params& p, const fd_tree_arrays& t, const double* cover, const float* X, int64_t n,
                   int32_t ld, double* phi, int32_t ld_phi);
// the forest's covers and path table dropped (unload / reload)
void shap_forget(PackedForest& pf);
// device pointers, on e.stream; d_rows may be null (then n_rows = n)
void launch_forest_shap(Engine& e, const PackedForest& pf, const float* d_X, int64_t n, int32_t ld,
                        const int64_t* d_rows, int64_t n_rows, double* d_phi, int32_t ld_phi);
void launch_shap_topk(Engine& e, const double* d_phi, int64_t n, int32_t ld_phi, int32_t nf, int32_t k, bool by_abs,
                      int32_t* d_idx, double* d_val);
// ensemble.hip: the fused path when the present models are one XGBoost and/or one IsolationForest in engine
// slots and the batch is large (false: not applicable, the caller runs the per-model kernels + blend).
// results != nullptr: write route result records (seq from records[i]) instead of the columns.
bool ensemble_applies(Engine& e, const ModelSet& ms, int64_t n);
// one forest's probabilities through the fused kernel (large batches, no raw / leaf outputs); false: not applicable
bool launch_ensemble_single(Engine& e, int slot, const float* dX, int64_t n, int32_t ld, double* dprob,
                            double* draw, hipStream_t stream);
// rows.compact: 1 the rows are the compact vector (64-B rows of kCompactWidth words, ld ignored; the plan's features
// <= 64); 2 split rows (RowA [n] then RowB [n] at rows.X, features.hip)
bool launch_ensemble(Engine& e, const ModelSet& ms, const ScoreRows& rows, const ScoreOut& out);
// ensemble_plan.hip: the host copy of a loaded forest, which the joint plans are built from
void forest_loaded(PackedForest& pf, const fd_forest_params& p, const fd_tree_arrays& t);
// blend.hip
// d_probs[m]: model m's probability column (an absent model's may be null); ms.slots / ms.ext are not read
void launch_blend(Engine& e, const ModelSet& ms, int64_t n, const double* const* d_probs, const ScoreOut& out);

}  // namespace fd
