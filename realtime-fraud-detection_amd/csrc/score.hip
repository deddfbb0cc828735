// score.hip — the scoring schedulers: which kernels score a batch, on which streams, in what order.
//   score_matrix     every model of a set over one matrix, then the blend: the fused ensemble kernel, the latency
//                    pair / pair-blend paths, prebinning in the LSTM launch, side streams, the MLP head, external columns
//   score_batch / score_records   features (columns / routed records) -> score_matrix
//   ab_score_matrix  score_matrix once per A/B variant over the partitioned batch
//   pipe_step        one micro-batch of the pipelined stream: the whole event and stream protocol (fd::Pipeline)
// The C ABI's entry points (engine.hip) check their arguments and call one of these; fd_sharded_step's orchestration
// is comm.hip's sharded_step, which calls pipe_step. The arguments are named by fd_internal.h's ModelSet / ScoreRows /
// ScoreOut / PipeBatch.
#include <algorithm>
#include <string>

#include "blend_row.h"
#include "fd_internal.h"

// fd_score_batch_pipelined's outputs: engine staging -> the caller's buffers, on the engine stream (one thread per
// transaction; null destinations are skipped); result records (routed batches) as 8-byte words. C linkage: the
// profiling tools and the committed profiles select it by this unmangled name.
extern "C" __global__ void __launch_bounds__(256)
pipe_out_copy_kernel(const double* __restrict__ fp, const double* __restrict__ conf, const uint8_t* __restrict__ dec,
                     const uint8_t* __restrict__ risk, const double* __restrict__ mp, int n_mp, int64_t n,
                     double* __restrict__ o_fp, double* __restrict__ o_conf, uint8_t* __restrict__ o_dec,
                     uint8_t* __restrict__ o_risk, double* __restrict__ o_mp, const float4* __restrict__ vec,
                     float4* __restrict__ o_vec, const uint64_t* __restrict__ res, uint64_t* __restrict__ o_res) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  if (o_vec) {  // the vectors: 16 float4 per row, one float4 per thread over the whole grid
    const int64_t total = n * (FD_VECTOR_WIDTH / 4);
    for (int64_t q = i; q < total; q += stride) o_vec[q] = vec[q];
  }
  if (o_res) {
    const int64_t total = n * (int64_t)(sizeof(fd::ResultRecord) / 8);
    for (int64_t q = i; q < total; q += stride) o_res[q] = res[q];
  }
  if (i >= n) return;
  if (o_fp) o_fp[i] = fp[i];
  if (o_conf) o_conf[i] = conf[i];
  if (o_dec) o_dec[i] = dec[i];
  if (o_risk) o_risk[i] = risk[i];
  for (int m = 0; m < n_mp; ++m) o_mp[(size_t)m * n + i] = mp[(size_t)m * n + i];
}

namespace fd {

// Events that only order one device's streams: no system-scope release at record (that is an L2 writeback
// per record, several us of stream time between a kernel and its cross-stream dependents)
constexpr unsigned kStreamEventFlags = hipEventDisableTiming | hipEventDisableSystemFence;

hipStream_t make_stream(int level) {
  hipStream_t st = nullptr;
  if (level == 0) {
    FD_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    return st;
  }
  int least = 0, greatest = 0;
  FD_HIP(hipDeviceGetStreamPriorityRange(&least, &greatest));
  FD_HIP(hipStreamCreateWithPriority(&st, hipStreamNonBlocking, level > 0 ? greatest : least));
  return st;
}

PackedForest& slot_of(Engine& e, int slot) {
  FD_REQUIRE(slot >= 0 && slot < kMaxSlots, FD_ERR_INVALID_ARG, "slot out of range");
  return e.forests[slot];
}

// ---------------------------------------------------------------- score_matrix's side streams
void SideStreams::fork(int k, hipStream_t from) {
  if (!st[k]) {
    FD_HIP(hipStreamCreateWithFlags(&st[k], hipStreamNonBlocking));
    FD_HIP(hipEventCreateWithFlags(&join_ev[k], kStreamEventFlags));
  }
  if (!fork_ev) FD_HIP(hipEventCreateWithFlags(&fork_ev, kStreamEventFlags));
  FD_HIP(hipEventRecord(fork_ev, from));
  FD_HIP(hipStreamWaitEvent(st[k], fork_ev, 0));
}

hipEvent_t SideStreams::mark(int k) {
  FD_HIP(hipEventRecord(join_ev[k], st[k]));
  return join_ev[k];
}

void SideStreams::join(int k, hipStream_t to) { FD_HIP(hipStreamWaitEvent(to, mark(k), 0)); }

void SideStreams::release() {
  for (int k = 0; k < 2; ++k) {
    if (!st[k]) continue;
    (void)hipStreamSynchronize(st[k]);
    (void)hipStreamDestroy(st[k]);
    (void)hipEventDestroy(join_ev[k]);
  }
  if (fork_ev) (void)hipEventDestroy(fork_ev);
}

// ---------------------------------------------------------------- score_matrix
namespace {
// A latency batch with exactly two present forests: which models they are, and what the other present models are
struct LatencyPair {
  int fm[2] = {-1, -1};
  bool lstm = false;         // a present model is the LSTM head
  bool others_lstm = true;   // every present model beside the two forests is the LSTM head
};
LatencyPair latency_pair(const ModelSet& ms) {
  LatencyPair lp;
  int k = 0;
  for (int m = 0; m < ms.n_models(); ++m) {
    if (!ms.has(m)) continue;
    if (ms.forest(m)) {
      if (k < 2) lp.fm[k++] = m;
    } else if (ms.slots[m] == FD_SLOT_LSTM) {
      lp.lstm = true;
    } else {
      lp.others_lstm = false;
    }
  }
  return lp;
}
}  // namespace

// Score the same feature matrix with every forest model, then blend (all on e.stream). A model in slot
// FD_SLOT_LSTM runs the LSTM head over rows.seq (n x T x 16) on the auxiliary stream, forked after
// everything already queued on e.stream (the feature kernel that wrote the sequences) and joined before the blend. A
// model in slot FD_SLOT_MLP is the MLP head over the matrix (mlp.hip), on e.stream beside the forests.
// Returns true when the route result records were written too (the fused ensemble kernel writes them in its
// epilogue); otherwise the caller packs them from the columns.
bool score_matrix(Engine& e, const ModelSet& ms, const ScoreRows& rows, const ScoreOut& out) {
  const fd_blend_params& p = *ms.params;
  const int32_t* slots = ms.slots;
  const float* dX = rows.X;
  const int64_t n = rows.n;
  const int32_t ld = rows.ld;
  require_model_count(p, "n_models out of range");
  FD_REQUIRE(slots != nullptr && (out.fp != nullptr || rows.results != nullptr), FD_ERR_INVALID_ARG,
             "null slots/output");
  if (n == 0) return false;
  // one XGBoost + one IsolationForest, large batch: both forests and the blend in one kernel
  if (launch_ensemble(e, ms, rows, out)) return rows.results != nullptr;
  // compact vectors are written only when the fused kernel applies (pipe_step): any other path is a bug
  FD_REQUIRE(!rows.compact, FD_ERR_UNSUPPORTED, "internal: compact vectors without the fused ensemble kernel");
  FD_REQUIRE(out.fp != nullptr, FD_ERR_INVALID_ARG, "null output");
  const int M = p.n_models;
  double* dMP = out.mp;
  if (!dMP) {
    e.scratch_probs.ensure((size_t)n * M * sizeof(double));
    dMP = e.scratch_probs.as<double>();
  }
  const double* cols[FD_MAX_MODELS] = {};
  // small (latency) batches, small_streams: 0 (default) everything on e.stream — the kernels of a 1 k batch are
  // short and the cross-queue fork / join hops cost more than the overlap gains (config 5: 0.088 vs 0.095 ms);
  // 1 the LSTM and every forest after the first on side stream 0; 2 the LSTM on side stream 0, the other forests on
  // side stream 1 (forked after everything queued so far, i.e. the feature kernel). Large batches: the LSTM on side
  // stream 0.
  int n_forests = 0;
  for (int m = 0; m < M; ++m) n_forests += (ms.has(m) && ms.forest(m));
  const bool latency = (n + kTile - 1) / kTile < kSplitTiles;
  const int ss = latency ? e.small_streams : 2;
  const bool small = latency && n_forests > 1;
  SideStreams& side = e.side;
  bool aux_forked = false;
  auto fork_aux = [&]() {
    if (!aux_forked) side.fork(0, e.stream);
    aux_forked = true;
  };
  // the pair paths below: two present forests of a latency batch
  const bool two = small && n_forests == 2;
  const LatencyPair lp = two ? latency_pair(ms) : LatencyPair{};
  // option latency_prebin: when this call runs the pair path below on e.stream (two forests, every other present
  // model the LSTM head), the LSTM launch bins the vectors for the pair's walks in workgroups ahead of its own, and
  // the pair skips its binning launch (fd::PreBin; the bins are for this call only). A slot out of range is left to
  // the pair path, which raises it after the LSTM launch.
  struct PreBinReset {
    Engine& e;
    ~PreBinReset() { e.prebin.want = e.prebin.done = false; }
  } prebin_reset{e};
  e.prebin.want = e.prebin.done = false;
  if (e.latency_prebin && e.latency_fused && two && ss == 0 && lp.lstm && lp.others_lstm &&
      slots[lp.fm[0]] < kMaxSlots && slots[lp.fm[1]] < kMaxSlots) {
    const PackedForest& pa = e.forests[slots[lp.fm[0]]];
    const PackedForest& pb = e.forests[slots[lp.fm[1]]];
    if (pa.loaded && pb.loaded) forest_pair_prebin(e, pa, pb, dX, n, ld);
  }
  for (int m = 0; m < M; ++m) {  // the LSTM first, so it overlaps the forests
    if (!ms.has(m) || slots[m] != FD_SLOT_LSTM) continue;
    FD_REQUIRE(rows.seq != nullptr, FD_ERR_INVALID_ARG,
               "the LSTM head needs card-history sequences (fd_score_batch_device with seq_len > 0)");
    double* col = dMP + (size_t)m * n;
    if (ss == 0) {
      launch_lstm(e, e.stream, rows.seq, n, rows.T, col, rows.seq_desc);
    } else {
      fork_aux();
      launch_lstm(e, side.st[0], rows.seq, n, rows.T, col, rows.seq_desc);
    }
    cols[m] = col;
  }
  const bool use2 = small && ss == 2, use1 = small && ss == 1;
  if (use2) side.fork(1, e.stream);
  if (use1) fork_aux();
  // two forests, one stream: one binning launch for both (fd::launch_forest_pair); when every other present model
  // is the LSTM head (already queued above), both walks in one launch and both sums + the blend in another
  // (fd::launch_forest_pair_blend: 3 launches instead of 6)
  bool paired = false;
  if (two && (ss == 0 || (e.latency_fused && !use2))) {
    const int* fm = lp.fm;
    const PackedForest& pa = slot_of(e, slots[fm[0]]);
    const PackedForest& pb = slot_of(e, slots[fm[1]]);
    if (pa.loaded && pb.loaded) {
      double* ca = dMP + (size_t)fm[0] * n;
      double* cb = dMP + (size_t)fm[1] * n;
      if (lp.others_lstm && e.latency_fused) {
        const double* pc[FD_MAX_MODELS] = {};
        int q = 0, pos_a = -1, pos_b = -1;
        for (int m = 0; m < M; ++m) {
          if (!ms.has(m)) continue;
          if (m == fm[0]) pos_a = q;
          if (m == fm[1]) pos_b = q;
          pc[q++] = m == fm[0] ? ca : m == fm[1] ? cb : cols[m];
        }
        // the LSTM head on the side stream (small_streams 1): the blend launch waits for it
        const hipEvent_t lstm_done = aux_forked ? side.mark(0) : nullptr;
        if (launch_forest_pair_blend(e, pa, pb, dX, n, ld, blend_consts(ms), pc, pos_a, pos_b, out, lstm_done))
          return false;
      }
      if (ss == 0) {  // (with side streams the per-forest launches below)
        paired = launch_forest_pair(e, pa, pb, dX, n, ld, ca, cb);
        if (paired) {
          cols[fm[0]] = ca;
          cols[fm[1]] = cb;
        }
      }
    }
  }
  int forests_seen = 0;
  for (int m = 0; m < M; ++m) {
    if (!ms.has(m) || slots[m] == FD_SLOT_LSTM) continue;
    if (paired && ms.forest(m)) continue;
    double* col = dMP + (size_t)m * n;
    if (slots[m] == FD_SLOT_MLP) {
      launch_mlp(e, e.stream, dX, n, ld, col);
      cols[m] = col;
    } else if (slots[m] >= 0) {
      const PackedForest& pf = slot_of(e, slots[m]);
      FD_REQUIRE(pf.loaded, FD_ERR_NOT_LOADED, "Model in slot " + std::to_string(slots[m]) + " not loaded");
      const bool on_side = small && forests_seen++ > 0;
      const hipStream_t st = on_side && use2 ? side.st[1] : on_side && use1 ? side.st[0] : nullptr;
      launch_forest(e, pf, dX, n, ld, col, nullptr, nullptr, st);
      cols[m] = col;
    } else {
      FD_REQUIRE(ms.ext && ms.ext[m], FD_ERR_INVALID_ARG, "model without slot needs an external probability column");
      if (ms.ext[m] != col)
        FD_HIP(hipMemcpyAsync(col, ms.ext[m], (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, e.stream));
      cols[m] = col;
    }
  }
  if (aux_forked) side.join(0, e.stream);
  if (use2) side.join(1, e.stream);
  launch_blend(e, ms, n, cols, out);
  return false;
}

// fd_ab_score_matrix_*: score_matrix with one model set per variant (device pointers, on e.stream). The batch is
// assigned and partitioned, the two counts are read back (they size the launches: the one wait), then rows and
// external columns are gathered into partition order, each variant with rows is scored by score_matrix as a batch of
// its own, and the results are scattered back to arrival order.
void ab_score_matrix(Engine& e, int id, const fd_ab_model_set& c, const fd_ab_model_set& t, const float* dX,
                     const uint64_t* d_keys, int64_t n, int32_t ld, uint8_t* d_variant, const ScoreOut& out) {
  ab_test(e, id);
  const fd_ab_model_set* set[2] = {&c, &t};
  for (const fd_ab_model_set* s : set) {
    FD_REQUIRE(s->params && s->slots, FD_ERR_INVALID_ARG, "null blend params / slots");
    require_model_count(*s->params, "n_models out of range");
  }
  FD_REQUIRE(n >= 0 && n < (1ll << 31) && ld > 0, FD_ERR_INVALID_ARG, "bad batch size / row stride");
  if (n == 0) return;
  FD_REQUIRE(dX && d_keys && out.fp, FD_ERR_INVALID_ARG, "null X / keys / fraud_prob");
  const ModelSet ms[2] = {ModelSet(c), ModelSet(t)};
  auto pad = [](size_t b) { return (b + 255) / 256 * 256; };
  const size_t nn = (size_t)n;
  // before the counts are known: the index, the two counts, and the variant column when the caller wants none
  const size_t o_cnt = pad(nn * sizeof(int32_t)), o_var = o_cnt + 256;
  e.ab.index.ensure(o_var + (d_variant ? 0 : pad(nn)));
  char* b0 = e.ab.index.as<char>();
  int32_t* idx = reinterpret_cast<int32_t*>(b0);
  int64_t* d_counts = reinterpret_cast<int64_t*>(b0 + o_cnt);
  if (!d_variant) d_variant = reinterpret_cast<uint8_t*>(b0 + o_var);
  ab_assign(e, id, d_keys, n, d_variant);
  ab_partition(e, d_variant, n, idx, d_counts);
  AbScatter sc{};
  FD_HIP(hipMemcpyAsync(sc.count, d_counts, sizeof(sc.count), hipMemcpyDeviceToHost, e.stream));
  FD_HIP(hipStreamSynchronize(e.stream));
  FD_REQUIRE(sc.count[0] >= 0 && sc.count[1] >= 0 && sc.count[0] + sc.count[1] == n, FD_ERR_HIP,
             "internal: A/B partition counts do not add up");
  // the batch in partition order, in its own buffer (the index above stays where it is)
  size_t total = 0;
  auto take = [&](size_t bytes) {
    const size_t at = total;
    total += pad(bytes);
    return at;
  };
  const size_t o_x = take(nn * ld * sizeof(float)), o_fp = take(nn * 8), o_conf = take(nn * 8), o_dec = take(nn),
               o_risk = take(nn);
  size_t o_mp[2] = {}, o_ext[2][FD_MAX_MODELS] = {};
  for (int v = 0; v < 2; ++v) {
    sc.models[v] = ms[v].n_models();
    if (out.mp) o_mp[v] = take((size_t)sc.models[v] * sc.count[v] * 8);
    for (int m = 0; m < sc.models[v]; ++m)
      if (sc.count[v] && ms[v].external(m)) {
        FD_REQUIRE(ms[v].ext && ms[v].ext[m], FD_ERR_INVALID_ARG,
                   "model without slot needs an external probability column");
        o_ext[v][m] = take((size_t)sc.count[v] * 8);
      }
  }
  e.ab.rows.ensure(total);
  char* b = e.ab.rows.as<char>();
  float* Xp = reinterpret_cast<float*>(b + o_x);
  // the partition-order columns: the ones the caller asked for (the scatter skips the others)
  ScoreOut part;
  part.fp = reinterpret_cast<double*>(b + o_fp);
  part.conf = reinterpret_cast<double*>(b + o_conf);
  part.dec = reinterpret_cast<uint8_t*>(b + o_dec);
  part.risk = reinterpret_cast<uint8_t*>(b + o_risk);
  sc.p_fp = part.fp;
  sc.p_conf = part.conf;
  sc.p_dec = part.dec;
  sc.p_risk = part.risk;
  if (!out.conf) part.conf = nullptr;
  if (!out.dec) part.dec = nullptr;
  if (!out.risk) part.risk = nullptr;
  ab_gather_rows(e, dX, idx, n, ld, Xp);
  for (int v = 0; v < 2; ++v) {
    const int64_t first = v ? sc.count[0] : 0, cnt = sc.count[v];
    if (cnt == 0) continue;
    const double* ext[FD_MAX_MODELS] = {};
    for (int m = 0; m < sc.models[v]; ++m)
      if (ms[v].external(m)) {
        double* col = reinterpret_cast<double*>(b + o_ext[v][m]);
        ab_gather_column(e, ms[v].ext[m], idx + first, cnt, col);
        ext[m] = col;
      }
    double* mp = out.mp ? reinterpret_cast<double*>(b + o_mp[v]) : nullptr;
    sc.p_mp[v] = mp;
    score_matrix(e, ModelSet(ms[v].params, ms[v].slots, ext, ms[v].present), ScoreRows(Xp + first * ld, cnt, ld),
                 part.rows_from(first, mp));
  }
  sc.idx = idx;
  sc.n = n;
  sc.m_max = std::max(sc.models[0], sc.models[1]);
  sc.fp = out.fp;
  sc.conf = out.conf;
  sc.dec = out.dec;
  sc.risk = out.risk;
  sc.mp = out.mp;
  ab_scatter_results(e, sc);
}

// engine scratch for the serial paths' LSTM input sequences, when a present model is the LSTM head
static float* lstm_seq_buffer(Engine& e, const ModelSet& ms, int64_t n, DeviceBuffer& buf) {
  if (!ms.wants_lstm()) return nullptr;
  FD_REQUIRE(e.state.ready && e.state.S > 0, FD_ERR_INVALID_ARG,
             "the LSTM head needs card history: fd_state_params.seq_len > 0");
  buf.ensure((size_t)n * e.state.S * kSeqInput * sizeof(float));
  return buf.as<float>();
}

void score_batch(Engine& e, const ModelSet& ms, const fd_txn_batch& t, int64_t n, float* d_vectors,
                 const ScoreOut& out) {
  float* vec = d_vectors;
  if (!vec) {
    e.feat_vec.ensure((size_t)n * FD_VECTOR_WIDTH * 4);
    vec = e.feat_vec.as<float>();
  }
  float* seq = lstm_seq_buffer(e, ms, n, e.seq_buf);
  // latency batches: the LSTM (4-row kernel) reads each card's last transaction's sequence from the history ring,
  // which nothing rewrites before it runs (the next batch's features follow on this stream); the feature kernel
  // writes only the other rows
  unsigned long long* desc = nullptr;
  if (seq && e.seq_ring_lstm && n < 4096 && (e.lstm_rows == 0 || e.lstm_rows == 4)) {
    e.seq_desc.ensure((size_t)n * sizeof(unsigned long long));
    desc = e.seq_desc.as<unsigned long long>();
    // a transaction whose card probe fails (table full) gets no descriptor from the feature kernel: the gather
    // kernel writes kSeqMaterialized for it; the slot-kernel path starts from all-materialized (bit 63 set)
    if (!e.state.slot_gather) FD_HIP(hipMemsetAsync(desc, 0xff, (size_t)n * sizeof(unsigned long long), e.stream));
  }
  launch_features(e, t, n, vec, nullptr, seq, nullptr, nullptr, false, 0, nullptr, false, desc);
  ScoreRows rows(vec, n, FD_VECTOR_WIDTH);
  rows.seq = seq;
  rows.T = e.state.S;
  rows.seq_desc = desc;
  score_matrix(e, ms, rows, out);
}

void score_records(Engine& e, const ModelSet& ms, const void* d_records, int64_t n, void* d_results) {
  e.feat_vec.ensure((size_t)n * FD_VECTOR_WIDTH * 4);
  e.route_out.ensure((size_t)n * (2 * sizeof(double) + 2));
  ScoreOut cols;  // the four columns in engine scratch, packed into the result records
  cols.fp = e.route_out.as<double>();
  cols.conf = cols.fp + n;
  cols.dec = reinterpret_cast<uint8_t*>(cols.conf + n);
  cols.risk = cols.dec + n;
  ScoreRows rows(e.feat_vec.as<float>(), n, FD_VECTOR_WIDTH);
  float* seq = lstm_seq_buffer(e, ms, n, e.seq_buf);
  rows.seq = seq;
  rows.T = e.state.S;
  rows.records = static_cast<const RouteRecord*>(d_records);
  rows.results = static_cast<ResultRecord*>(d_results);
  launch_features_records(e, d_records, n, e.feat_vec.as<float>(), seq);  // reads the records in place
  if (!score_matrix(e, ms, rows, cols)) launch_result_pack(e, cols, rows.records, n, d_results);
}

// ---------------------------------------------------------------- the pipelined stream
void Pipeline::create(int stream_prio, bool big_table) {
  for (int k = 0; k < 2; ++k)
    if (!stream[k]) stream[k] = make_stream(stream_prio >= 1 ? 1 : 0);
  if (slot_mode < 0)  // auto: where the feature chain outlasts the fused kernel (random card traffic over a
    // large table), not where an earlier slot pass only adds contention beside it
    slot_mode = big_table ? 2 : 0;
  if (slot_mode && !slot_stream) {
    slot_stream = make_stream(slot_mode == 1 ? 1 : -1);
    for (int k = 0; k < kSlots; ++k) FD_HIP(hipEventCreateWithFlags(&slot_ev[k], kStreamEventFlags));
  }
  if (!entry_ev) {
    FD_HIP(hipEventCreateWithFlags(&entry_ev, kStreamEventFlags));
    for (int k = 0; k < kSlots; ++k) {
      FD_HIP(hipEventCreateWithFlags(&feat_ev[k], kStreamEventFlags));
      FD_HIP(hipEventCreateWithFlags(&copy_ev[k], kStreamEventFlags));
    }
    for (int k = 0; k < kDoneRing; ++k) FD_HIP(hipEventCreateWithFlags(&done_ev[k], kStreamEventFlags));
  }
}

void Pipeline::release() {
  for (hipStream_t st : {stream[0], stream[1], slot_stream})
    if (st) {
      (void)hipStreamSynchronize(st);
      (void)hipStreamDestroy(st);
    }
  if (entry_ev) (void)hipEventDestroy(entry_ev);
  for (int k = 0; k < kSlots; ++k)
    for (hipEvent_t ev : {slot_ev[k], feat_ev[k], copy_ev[k]})
      if (ev) (void)hipEventDestroy(ev);
  for (hipEvent_t ev : done_ev)
    if (ev) (void)hipEventDestroy(ev);
}

void Pipeline::order_after_scoring(hipStream_t s) {
  for (int k = 0; k < kDoneRing; ++k)
    if (done_live[k]) FD_HIP(hipStreamWaitEvent(s, done_ev[k], 0));
}

// One micro-batch of the pipelined stream: transaction columns (b.txns) or routed 48-B records (b.records, whose
// scores leave as 24-B result records in b.d_results). Shared by fd_score_batch_pipelined, fd_score_records_pipelined
// and fd_sharded_step.
void pipe_step(Engine& e, const ModelSet& ms, const PipeBatch& b) {
  Pipeline& P = e.pipe;
  const int64_t n = b.n;
  const void* records = b.records;
  P.create(e.stream_prio, e.state.ready && e.state.cap >= (1ll << 26));
  // Batch i: buffer slot s = i mod 2, its features and its scoring on Sc = stream[i & 1] (Sf: the same
  // stream). Card-state order: batch i's bucket pass after batch i-1's (an event). Buffer s is free once batch
  // i-2's scoring is done (the same queue). Outputs: the engine stream waits for batch i's scoring. (Measured and
  // dropped: one feature stream for every batch + two scoring streams, ring of three buffers — the third stream
  // shares a hardware queue with a scoring stream: 567 vs 742 M txn/s)
  constexpr int nbuf = Pipeline::kSlots;
  const int s = (int)(P.iter % (unsigned long long)nbuf);
  const int prev = s ^ 1;
  hipStream_t Sc = P.stream[P.iter & 1];
  hipStream_t Sf = Sc;
  // option slot_stream: the slot pass on Ss, after what it reads (the entry order, the inputs) and batch i-2's
  // bucket pass (scratch set s: its fill counts and keys are consumed and reset there); feat_slot_kernel only
  // finds / inserts card keys, which the bucket passes of earlier batches never change
  hipStream_t Ss = P.slot_stream;
  const hipEvent_t input_ready = static_cast<hipEvent_t>(b.input_ready);
  if (P.dirty) {  // work queued on e.stream by other calls (state loads, snapshots, ...) comes first
    FD_HIP(hipEventRecord(P.entry_ev, e.stream));
    FD_HIP(hipStreamWaitEvent(Sf, P.entry_ev, 0));
    if (Ss) FD_HIP(hipStreamWaitEvent(Ss, P.entry_ev, 0));
    P.dirty = false;
  }
  if (input_ready) FD_HIP(hipStreamWaitEvent(Sf, input_ready, 0));
  if (Ss && input_ready) FD_HIP(hipStreamWaitEvent(Ss, input_ready, 0));
  if (Ss && P.feat_live[s]) FD_HIP(hipStreamWaitEvent(Ss, P.feat_ev[s], 0));
  // the slot's vectors are rewritten below: after batch i-nbuf's output copy if that one read them
  if (P.copy_live[s] && P.copy_vec[s]) FD_HIP(hipStreamWaitEvent(Sf, P.copy_ev[s], 0));
  // mode 1: the slot pass (scratch set s & 1, untouched by batch i-1) runs at once; the bucket pass waits for
  // batch i-1's card updates
  hipEvent_t before_buckets = P.feat_live[prev] ? P.feat_ev[prev] : nullptr;
  // the fused kernel alone reads the vectors and nobody asked for them: the compact form (64 instead of 256 B per
  // transaction written here and read by the ensemble kernel, fd_internal.h kCompactSlot), or split rows
  // (compact 2: the slot pass writes the card-independent half, the bucket pass reads 32-B instead of 64-B prep
  // records; the lean bucket pass only, and not with LSTM history in the card state)
  int compact = (e.compact_vectors && b.d_vectors == nullptr && ensemble_applies(e, ms, n)) ? e.compact_vectors : 0;
  const int sr = (int)(P.iter % (unsigned long long)Pipeline::kSplitRing);  // split rows: this batch's ring buffer
  const bool want_seq = ms.wants_lstm();
  float* seq = lstm_seq_buffer(e, ms, n, P.seq[s]);
  // latency-sized batches: the gather kernel (slot pass inside the bucket launch) instead of the slot + lean pair,
  // whose two launches cost 39 us per 1 k batch against its 18; it waits for batch i-1's card updates
  // (before_buckets) like the lean pass
  const bool lean = P.lean && !(P.gather && e.state.slot_gather && n <= kGatherBatchMax && !Ss);
  if (compact == 2 && (!lean || want_seq || e.state.S > 0)) compact = 1;
  float* vec = nullptr;
  if (compact == 2) {  // RowA | RowB in the ring; the slot pass (which writes RowA) after the last fused kernel that
    // read this buffer — on the slot stream that is an explicit wait, on the batch's own stream the stream order
    P.split[sr].ensure((size_t)n * 64);
    vec = P.split[sr].as<float>();
    if (Ss && P.done_live[sr]) FD_HIP(hipStreamWaitEvent(Ss, P.done_ev[sr], 0));  // batch i - 4's
  } else {  // the 64-wide vectors or compact rows: the slot's own buffer (split-row batches never touch it)
    P.vec[s].ensure((size_t)n * FD_VECTOR_WIDTH * 4);
    vec = P.vec[s].as<float>();
  }
  {
    struct SlotPass {  // launch_grouped reads these for this call only
      Pipeline& P;
      ~SlotPass() { P.slot_pass_stream = nullptr, P.slot_pass_ev = nullptr; }
    } slot_pass{P};
    P.slot_pass_stream = Ss;
    P.slot_pass_ev = Ss ? P.slot_ev[s] : nullptr;
    if (records)
      launch_features_records(e, records, n, vec, seq, Sf, lean, s, before_buckets, compact);
    else
      launch_features(e, *b.txns, n, vec, nullptr, seq, nullptr, Sf, lean, s, before_buckets, compact);
  }
  FD_HIP(hipEventRecord(P.feat_ev[s], Sf));
  P.feat_live[s] = true;
  // scoring paths other than the fused kernel share engine scratch (per-model columns, tree-split and LSTM
  // buffers): those batches also wait for the previous batch's scoring
  const int pr = (sr + Pipeline::kDoneRing - 1) % Pipeline::kDoneRing;  // batch i - 1's done event
  if (P.done_live[pr] && !compact && !ensemble_applies(e, ms, n)) FD_HIP(hipStreamWaitEvent(Sc, P.done_ev[pr], 0));
  // this slot's output staging: free once batch i-nbuf's copy to its caller (on e.stream) is done. Routed batches
  // always stage the four columns (the result records are packed from them when the fused kernel does not apply).
  const int n_mp = b.out.mp ? ms.n_models() : 0;
  const size_t n8 = (size_t)n * 8, a8 = ((size_t)n + 7) & ~(size_t)7;
  // results_in_place (fd_sharded_step: d_results is the engine's own res[q], free by the step's event order, see
  // ShardComm::res): the scoring writes the result records there, no staging copy; otherwise they are staged and
  // copied on the engine stream like the columns (a caller's buffer is written only in the engine stream's order)
  const bool in_place = records && b.results_in_place;
  const size_t rbytes = records && !in_place ? (size_t)n * sizeof(ResultRecord) : 0;
  P.out[s].ensure((2 + (size_t)n_mp) * n8 + 2 * a8 + rbytes);
  char* so = P.out[s].as<char>();
  ScoreOut st;  // the staged columns: the ones the caller asked for; all four for routed batches
  st.fp = reinterpret_cast<double*>(so);
  st.conf = (b.out.conf || records) ? reinterpret_cast<double*>(so + n8) : nullptr;
  st.mp = n_mp ? reinterpret_cast<double*>(so + 2 * n8) : nullptr;
  st.dec = (b.out.dec || records) ? reinterpret_cast<uint8_t*>(so + (2 + (size_t)n_mp) * n8) : nullptr;
  st.risk = (b.out.risk || records) ? reinterpret_cast<uint8_t*>(so + (2 + (size_t)n_mp) * n8 + a8) : nullptr;
  auto* s_res = !records ? nullptr
                         : in_place ? static_cast<ResultRecord*>(b.d_results)
                                    : reinterpret_cast<ResultRecord*>(so + (2 + (size_t)n_mp) * n8 + 2 * a8);
  if (P.copy_live[s]) FD_HIP(hipStreamWaitEvent(Sc, P.copy_ev[s], 0));
  ++P.iter;
  ++P.iter_total;
  P.compact_total += compact != 0;
  P.split_total += compact == 2;
  P.slot_stream_total += Ss != nullptr;
  {  // the scoring launches go on Sc: score_matrix launches on e.stream
    struct Swap {
      Engine& e;
      hipStream_t saved;
      ~Swap() { e.stream = saved; }
    } swap{e, e.stream};
    e.stream = Sc;
    ScoreRows rows(vec, n, FD_VECTOR_WIDTH);
    rows.seq = seq;
    rows.T = e.state.S;
    rows.records = static_cast<const RouteRecord*>(records);
    rows.results = s_res;
    rows.compact = compact;
    if (!score_matrix(e, ms, rows, st) && records) launch_result_pack(e, st, rows.records, n, s_res);
  }
  // (split rows: this event also releases ring buffer sr to batch i + 4's slot pass — no event of its own, which
  // cost a record per step on the engine stream; recorded on Sc beside the fused kernel it cost 4 % in round 6)
  FD_HIP(hipEventRecord(P.done_ev[sr], Sc));
  P.done_live[sr] = true;
  FD_HIP(hipStreamWaitEvent(e.stream, P.done_ev[sr], 0));
  if (in_place) {  // nothing to copy: the next use of staging slot s (batch i + 2) is on this batch's stream Sc
    P.copy_live[s] = false;
    return;
  }
  hipLaunchKernelGGL(pipe_out_copy_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, e.stream, st.fp, st.conf,
                     st.dec, st.risk, st.mp, n_mp, n, records ? nullptr : b.out.fp, b.out.conf, b.out.dec, b.out.risk,
                     b.out.mp, reinterpret_cast<const float4*>(vec), reinterpret_cast<float4*>(b.d_vectors),
                     reinterpret_cast<const uint64_t*>(s_res), static_cast<uint64_t*>(b.d_results));
  FD_HIP(hipGetLastError());
  FD_HIP(hipEventRecord(P.copy_ev[s], e.stream));
  P.copy_live[s] = true;
  P.copy_vec[s] = b.d_vectors != nullptr;
}

}  // namespace fd
