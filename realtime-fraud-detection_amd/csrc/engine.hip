// engine.hip — C-ABI surface of libfdengine.so (declared in include/fdengine.h), and nothing else: an entry point
// locks the engine, checks its arguments, stages host arrays where it takes them, and makes one call into the
// translation unit that does the work (the scoring schedulers: score.hip; the sharded step: comm.hip).
// Device memory is not released here by name: fd_engine_destroy deletes the engine, ~Engine (below) does the teardown
// whose order matters, and every DeviceBuffer goes with the struct or the scope that owns it (fd_internal.h).
// Every entry point catches everything: status codes + a thread-local message cross the ABI,
// exceptions never do (mirrors the reference's log-and-raise contract, ml/models/model_manager.py:302-307,
// with the raise done by the Python shim).
#include <algorithm>
#include <chrono>
#include <mutex>
#include <cstring>
#include <string>

#include "blend_row.h"
#include "abtest_row.h"
#include "fd_internal.h"
#include "graph_row.h"
#include "host_stage.h"
#include "ingest_parse.h"
#include "text_row.h"

namespace fd {

static thread_local std::string g_last_error;

void set_error(const std::string& msg) { g_last_error = msg; }

Engine::Timed* Engine::next_event_pair(int kind) {
  if (timing_every > 1 && kind >= 0 && kind < 16 && (timing_seq[kind]++ % (unsigned)timing_every) != 0)
    return nullptr;  // sampled timing: this launch runs without event records
  if (events_used == events.size()) {
    // timing events only: no system-scope fence at record (a fenced record costs ~4 us of stream time)
    hipEvent_t a, b;
    FD_HIP(hipEventCreateWithFlags(&a, hipEventDisableSystemFence));
    FD_HIP(hipEventCreateWithFlags(&b, hipEventDisableSystemFence));
    events.push_back({a, b, 0});
  }
  Timed* t = &events[events_used++];
  t->kind = kind;
  t->split = false;
  return t;
}

// Only what has an order: the communicators go while every buffer is still there (comm_destroy decides which of them
// an undrained exchange may still touch, and abandons those), the streams are drained before they are destroyed, and
// all of it before the members' destructors free the device memory. Nothing here throws.
Engine::~Engine() {
  if (stream) (void)hipStreamSynchronize(stream);
  try {
    comm_destroy(*this);
  } catch (...) {
  }
  pipe.release();
  side.release();
  for (auto& ev : events)
    for (hipEvent_t h : {ev.a, ev.b, ev.c, ev.d})
      if (h) (void)hipEventDestroy(h);
  if (own_stream) (void)hipStreamDestroy(own_stream);
}

}  // namespace fd

using fd::Engine;
using fd::Stage;

#define FD_API_BEGIN try {
#define FD_API_END                    \
  return FD_OK;                       \
  }                                   \
  catch (const fd::Error& e) {        \
    fd::set_error(e.what());          \
    return e.code;                    \
  }                                   \
  catch (const std::bad_alloc&) {     \
    fd::set_error("out of memory");   \
    return FD_ERR_OOM;                \
  }                                   \
  catch (const std::exception& e) {   \
    fd::set_error(e.what());          \
    return FD_ERR_INVALID_ARG;        \
  }

struct fd_engine {
  Engine e;
  // every entry point on this engine holds it (FD_ENGINE_LOCK): calls from several host threads are serialised
  // per engine (e.g. ModelManager.predict in an executor thread beside a reload on the event loop's thread);
  // recursive so an entry point may call another
  std::recursive_mutex mu;
};

static std::recursive_mutex& lock_of(fd_engine* p) {
  static std::recursive_mutex none;  // null engine: E() reports it
  return p ? p->mu : none;
}
#define FD_ENGINE_LOCK(p) std::lock_guard<std::recursive_mutex> fd_engine_guard_(lock_of(p))

// Engine of an entry point that may queue work on e.stream: the next fd_score_batch_pipelined orders its
// feature stream after e.stream again (Pipeline::dirty).
static Engine& E(fd_engine* p) {
  FD_REQUIRE(p != nullptr, FD_ERR_INVALID_ARG, "null engine");
  p->e.activate();
  p->e.pipe.dirty = true;
  return p->e;
}

// Engine of an entry point that queues no device work touching engine state (options, timing reads)
static Engine& E_quiet(fd_engine* p) {
  FD_REQUIRE(p != nullptr, FD_ERR_INVALID_ARG, "null engine");
  p->e.activate();
  return p->e;
}

using fd::ModelSet;
using fd::ScoreOut;
using fd::slot_of;

extern "C" {

const char* fd_last_error(void) { return fd::g_last_error.c_str(); }

int fd_abi_version(void) { return FD_ABI_VERSION; }

int fd_device_count(int* out) {
  FD_API_BEGIN
  FD_REQUIRE(out, FD_ERR_INVALID_ARG, "null out");
  int c = 0;
  FD_HIP(hipGetDeviceCount(&c));
  *out = c;
  FD_API_END
}

int fd_engine_create(int device, fd_engine** out) {
  FD_API_BEGIN
  FD_REQUIRE(out, FD_ERR_INVALID_ARG, "null out");
  *out = nullptr;
  int c = 0;
  FD_HIP(hipGetDeviceCount(&c));
  FD_REQUIRE(device >= 0 && device < c, FD_ERR_INVALID_ARG,
             "device " + std::to_string(device) + " not present (" + std::to_string(c) + " visible)");
  auto* p = new fd_engine();
  p->e.device = device;
  try {
    FD_HIP(hipSetDevice(device));
    FD_HIP(hipStreamCreateWithFlags(&p->e.own_stream, hipStreamNonBlocking));
    p->e.stream = p->e.own_stream;
  } catch (...) {
    delete p;
    throw;
  }
  *out = p;
  FD_API_END
}

int fd_engine_destroy(fd_engine* eng) {
  FD_API_BEGIN
  if (!eng) return FD_OK;
  { FD_ENGINE_LOCK(eng); }  // wait for a call in flight on another thread (destroying while in use is the caller's bug)
  Engine& e = E(eng);
  if (e.comm.aborted) {  // an aborted exchange: every stream gets a bounded wait; one that never drains leaks the engine
    bool ok = fd::comm_sync_stream(e, e.comm.x_fwd);
    ok = fd::comm_sync_stream(e, e.stream) && ok;
    for (hipStream_t st : e.pipe.stream) ok = fd::comm_sync_stream(e, st) && ok;
    ok = fd::comm_sync_stream(e, e.pipe.slot_stream) && ok;
    FD_REQUIRE(ok, FD_ERR_HIP, "engine leaked: streams still busy " + std::to_string(e.comm.timeout_ms) +
                                   " ms after the communicators were aborted (" + e.comm.abort_reason + ")");
  }
  delete eng;  // ~Engine: the ordered teardown, then every buffer with its owner
  FD_API_END
}

// the new engine stream inherits the order of the old one over pipelined batches: their scoring is complete
// before anything queued on it (fd_score_batch_pipelined's outputs stay ordered on the engine stream)
static void rebind_stream(Engine& e, hipStream_t s) {
  if (s != e.stream) e.pipe.order_after_scoring(s);
  e.stream = s;
}

int fd_engine_set_stream(fd_engine* eng, void* hip_stream) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E(eng);
  rebind_stream(e, static_cast<hipStream_t>(hip_stream));
  FD_API_END
}

int fd_engine_reset_stream(fd_engine* eng) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E(eng);
  rebind_stream(e, e.own_stream);
  FD_API_END
}

int fd_engine_sync(fd_engine* eng) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E(eng);
  if (e.comm.aborted) {  // streams behind an aborted exchange: bounded waits, then the abort's reason
    bool ok = fd::comm_sync_stream(e, e.comm.x_fwd);
    ok = fd::comm_sync_stream(e, e.stream) && ok;
    for (hipStream_t st : e.pipe.stream) ok = fd::comm_sync_stream(e, st) && ok;
    // the slot pass and the side streams can be queued behind an aborted inbox event too (as fd_engine_destroy)
    for (hipStream_t st : {e.pipe.slot_stream, e.side.st[0], e.side.st[1]}) ok = fd::comm_sync_stream(e, st) && ok;
    FD_REQUIRE(ok, FD_ERR_HIP, "streams still busy " + std::to_string(e.comm.timeout_ms) +
                                   " ms after the communicators were aborted (" + e.comm.abort_reason + ")");
  }
  FD_HIP(hipStreamSynchronize(e.stream));
  if (e.comm.x_fwd) FD_HIP(hipStreamSynchronize(e.comm.x_fwd));
  for (hipStream_t st : {e.pipe.stream[0], e.pipe.stream[1], e.pipe.slot_stream, e.side.st[0], e.side.st[1]})
    if (st) FD_HIP(hipStreamSynchronize(st));
  fd::route_check(e);
  FD_API_END
}

int fd_engine_set_timing(fd_engine* eng, int enable) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E_quiet(eng);
  e.timing = enable != 0;
  FD_API_END
}

int fd_engine_get_counter(fd_engine* eng, const char* key, int64_t* value) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E_quiet(eng);
  FD_REQUIRE(key && value, FD_ERR_INVALID_ARG, "null key/value");
  const std::string k(key);
  if (k == "pipelined_batches") {  // fd_score_batch_pipelined / fd_score_records_pipelined batches so far
    *value = (int64_t)e.pipe.iter_total;
  } else if (k == "ensemble_single_launches") {  // fd_forest_predict batches scored by the fused kernel over one
    // forest (probabilities, optionally raw scores; no leaf ids): config 2's timed kernel, ensemble_kernel<8,2>
    *value = (int64_t)e.ens_single_total;
  } else if (k == "ensemble_contracted_launches") {  // fused launches over the contracted forests (compact / split rows,
    // option ensemble_contract, a plan the contraction shortened)
    *value = (int64_t)e.ens_contract_total;
  } else if (k == "ensemble_nodes_pruned") {  // the current pair plan: splits on constant slots resolved at load, and
    // the splits of the subtrees that went with them
    *value = e.ens.valid ? (int64_t)e.ens.nodes_pruned : 0;
  } else if (k == "ensemble_node_steps_per_txn") {  // the last fused pair launch: tree levels walked per transaction
    // over both forests (the sum of the depths as walked; n_trees x D on the uncontracted path)
    *value = (int64_t)e.ens_steps_last;
  } else if (k == "ensemble_dense_chunks") {  // the last fused pair launch: chunks over both forests when it walked the
    // dense chunk stream (ensemble_contract 3 / 4), else 0
    *value = (int64_t)e.ens_dense_chunks_last;
  } else if (k == "forest_sparse_launches") {  // launches of forest_sparse_kernel: predict_proba forests, forests
    // deeper than 10 levels, and any forest under option forest_kernel = 11
    *value = (int64_t)e.sparse_total;
  } else if (k == "forest_shap_launches") {  // launches of shap_kernel (fd_forest_shap_*: one per batch of 4096 rows)
    *value = (int64_t)e.shap_total;
  } else if (k == "gbdt_hist_launches") {  // launches of gbdt_hist_kernel (one per tree level with rows)
    *value = (int64_t)e.gbdt.hist_launches;
  } else if (k == "gbdt_trees") {  // trees grown on the device (fd_gbdt_fit_* / fd_gbdt_grow_tree_device / _host)
    *value = (int64_t)e.gbdt.trees;
  } else if (k == "gbdt_nodes_split") {  // split nodes of those trees
    *value = (int64_t)e.gbdt.nodes_split;
  } else if (k == "gbdt_eval_launches") {  // launches of the eval kernel that walked a tree (a watched fit's rounds)
    *value = (int64_t)e.gbdt.eval_launches;
  } else if (k == "gbdt_rounds_run") {  // rounds the device fits ran (launches that returned at the stop flag excluded)
    *value = (int64_t)e.gbdt.rounds_run;
  } else if (k == "iforest_fit_trees") {  // IsolationForest trees grown on the device (fd_iforest_fit_*)
    *value = (int64_t)e.iforest.trees;
  } else if (k == "iforest_fit_nodes_split") {  // split nodes of those trees
    *value = (int64_t)e.iforest.nodes_split;
  } else if (k == "mlp_fit_steps") {  // optimiser steps of the MLP fits (fd_mlp_fit_device / _host)
    *value = (int64_t)e.mlp_fit.steps;
  } else if (k == "mlp_fit_launches") {  // launches of mlp_fit_step_kernel and mlp_fit_update_kernel: 2 per step, 2 per
    // fd_mlp_grad_device / _host call
    *value = (int64_t)e.mlp_fit.launches;
  } else if (k == "mlp_launches") {  // launches of the MLP head's kernel (fd_mlp_predict_*, FD_SLOT_MLP models)
    *value = (int64_t)e.mlp_total;
  } else if (k == "graph_steps") {  // fd_graph_step_* calls that appended transactions
    *value = (int64_t)e.graph.steps;
  } else if (k == "text_calls") {  // fd_text_features_* calls with n > 0
    *value = (int64_t)e.text.calls;
  } else if (k == "text_nonascii_rows") {  // rows those calls flagged FD_TEXT_NONASCII (waits for the engine stream)
    *value = fd::text_nonascii_rows(e);
  } else if (k == "latency_prebinned_batches") {  // latency pair launches that used the feature kernel's bins
    *value = (int64_t)e.prebin_total;
  } else if (k == "pipelined_split_batches") {  // of the compact ones: split rows (compact_vectors 2)
    *value = (int64_t)e.pipe.split_total;
  } else if (k == "pipelined_compact_batches") {  // of those: scored by the fused kernel from the compact 64-B
    // rows (no vectors requested), the variant the config-3/4 bench times
    *value = (int64_t)e.pipe.compact_total;
  } else if (k == "pipelined_host_ns") {  // host nanoseconds inside fd_score_batch_pipelined (HIP launches, event
    // records and waits of the pipelined step)
    *value = (int64_t)e.pipe.host_ns;
  } else if (k == "pipelined_slot_stream_batches") {  // of those: the slot pass on its own stream (slot_stream)
    *value = (int64_t)e.pipe.slot_stream_total;
  } else if (k == "device_bytes_live") {  // bytes of device memory the library holds now, over every engine of the
    // process (DeviceBuffer; memory abandoned behind an undrained exchange stays counted)
    *value = (int64_t)fd::g_device_bytes_live.load();
  } else if (k == "window_saturated") {  // sliding windows: transactions whose 24 h window held K prior events
    // (its count may be truncated at the ring capacity); synchronises the engine's streams
    FD_REQUIRE(e.state.ready, FD_ERR_NOT_LOADED, "card state not initialised (fd_state_init)");
    FD_HIP(hipStreamSynchronize(e.stream));
    for (hipStream_t st : e.pipe.stream)
      if (st) FD_HIP(hipStreamSynchronize(st));
    unsigned long long v = 0;
    FD_HIP(hipMemcpy(&v, e.state.sat.ptr, 8, hipMemcpyDeviceToHost));
    *value = (int64_t)v;
  } else if (k == "sharded_steps") {  // fd_sharded_step calls so far
    *value = (int64_t)e.comm.steps.load();
  } else if (k == "rccl_ops") {  // RCCL operations issued by the engine's exchanges (send, recv, all-gather)
    *value = (int64_t)e.comm.ops.load();
  } else if (k.rfind("sharded_host_ns_", 0) == 0) {  // host time inside fd_sharded_step by phase
    int i = 0;
    while (i < fd::ShardComm::kHostPhases && k.compare(16, std::string::npos, fd::kShardHostPhase[i]) != 0) ++i;
    FD_REQUIRE(i < fd::ShardComm::kHostPhases, FD_ERR_INVALID_ARG, "unknown counter: " + k);
    *value = (int64_t)e.comm.host_ns[i].load();
  } else {
    FD_REQUIRE(false, FD_ERR_INVALID_ARG, "unknown counter: " + k);
  }
  FD_API_END
}

int fd_engine_set_option(fd_engine* eng, const char* key, int64_t value) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E_quiet(eng);
  FD_REQUIRE(key, FD_ERR_INVALID_ARG, "null key");
  const std::string k(key);
  if (k == "forest_kernel") {
    // 0 auto; 1 / 2 / 3 / 8 force kernel 1 / 3 / 4 / 6; 6 the tree-split path; 11 the sparse-layout kernel
    // (forest.hip launch_forest)
    FD_REQUIRE(value == 0 || value == 1 || value == 2 || value == 3 || value == 6 || value == 8 || value == 11,
               FD_ERR_INVALID_ARG, "forest_kernel must be 0, 1, 2, 3, 6, 8 or 11");
    e.forest_variant = (int)value;
  } else if (k == "ensemble") {  // 1 (default): fused forests + blend when applicable; 0: per-model kernels
    FD_REQUIRE(value == 0 || value == 1, FD_ERR_INVALID_ARG, "ensemble must be 0 or 1");
    e.ensemble_on = value != 0;
  } else if (k == "ensemble_owner") {  // fused kernel: 0 owner tree group rotates per chunk; 1 always group 0
    FD_REQUIRE(value == 0 || value == 1, FD_ERR_INVALID_ARG, "ensemble_owner must be 0 or 1");
    e.ens_owner_fixed = value != 0;
  } else if (k == "ensemble_prio") {  // fused kernel: 1 (default since round 6) its waves issue above the co-running
    // feature kernels' (s_setprio 2); 0 the same priority. Round 4 measured 1 slower (0.0929 vs 0.0908-0.0918 ms,
    // profiles/r04/prio); with round 6's split rows the feature chain is 20 us shorter than the fused kernel beside it
    // and the critical path is the fused kernel: with feature_prio 0, the driver's command 0.0944 -> 0.0897 ms and 200
    // steps 0.0826 -> 0.0812 (profiles/r06/prio)
    FD_REQUIRE(value == 0 || value == 1, FD_ERR_INVALID_ARG, "ensemble_prio must be 0 or 1");
    e.ens_prio = value != 0;
  } else if (k == "ensemble_chunks") {  // fused kernel's chunk layout: 0 auto (compact once the engine has RCCL
    // communicators, else wide), 1 wide (24 / 16 trees), 2 compact (20 / 12: LDS room for an RCCL kernel beside)
    FD_REQUIRE(value >= 0 && value <= 2, FD_ERR_INVALID_ARG, "ensemble_chunks must be 0, 1 or 2");
    e.ens_chunks = (int)value;
  } else if (k == "ensemble_contract") {  // fused kernel on compact / split rows: the forests contracted against the
    // rows' constant slots (ensemble_plan.hip contract_forest_host). 4 (default) / 3: the contracted trees packed
    // densely, up to eight bundles per chunk and barrier (dense_layout_host), bundles of the chunk's trees sorted by
    // depth / of consecutive trees; 1 the padded chunks, each tree walked to the deepest of its wave's trees (a fixed-depth walk
    // chosen per wave and chunk); 2 each tree's own depth (uniform branches inside the walk: measured slower, DESIGN
    // §3); 0 the full forests at the common depth. Outputs are identical in every mode. A change rebuilds the plan's
    // chunks: the device is idle first
    FD_REQUIRE(value >= 0 && value <= 4, FD_ERR_INVALID_ARG, "ensemble_contract must be 0 .. 4");
    if ((int)value != e.ens_contract) {
      e.activate();
      FD_HIP(hipDeviceSynchronize());
    }
    e.ens_contract = (int)value;
  } else if (k == "compact_vectors") {  // pipelined stream, the fused kernel's batches when nobody asked for the
    // vectors: 2 (default) split rows — the card-independent half finished by the slot pass, the bucket pass reads
    // 32-B prep records and writes the card half (features.hip Prep32 / RowA / RowB); 1 the compact 64-B row; 0 the
    // 64-wide vector (outputs identical in every mode)
    FD_REQUIRE(value >= 0 && value <= 2, FD_ERR_INVALID_ARG, "compact_vectors must be 0, 1 or 2");
    e.compact_vectors = (int)value;
  } else if (k == "latency_fused") {  // latency batches: 1 (default) both forests' walks in one launch and their
    // sums + the blend in another (fd::launch_forest_pair_blend); 0 the per-forest walk + sum launches + blend
    FD_REQUIRE(value == 0 || value == 1, FD_ERR_INVALID_ARG, "latency_fused must be 0 or 1");
    e.latency_fused = value != 0;
  } else if (k == "pipeline_lean") {  // fd_score_batch_pipelined's bucket pass: 1 (default) lean + deferred
    FD_REQUIRE(value == 0 || value == 1, FD_ERR_INVALID_ARG, "pipeline_lean must be 0 or 1");
    e.pipe.lean = value != 0;
  } else if (k == "pipeline_gather") {  // fd_score_batch_pipelined, batches of <= 4096 transactions (slot_gather on,
    // no slot stream): 1 (default) the gather bucket kernel (card slots found inside it, one feature launch), 0 the
    // slot + lean bucket pair of the large batches
    FD_REQUIRE(value == 0 || value == 1, FD_ERR_INVALID_ARG, "pipeline_gather must be 0 or 1");
    e.pipe.gather = value != 0;
  } else if (k == "latency_prebin") {  // latency batches with the LSTM head: the XGBoost + IsolationForest pair's
    // tree-split binning in the LSTM launch: 3 (default) inside the LSTM's own workgroups (a lifting level per
    // recurrence step; 2 where a thread would have more than two searches), 2 in extra workgroups after the LSTM's
    // own (they fill the CUs the LSTM's workgroups leave as they finish), 1 ahead of them; 0 the pair's own binning
    // launch
    FD_REQUIRE(value >= 0 && value <= 3, FD_ERR_INVALID_ARG, "latency_prebin must be 0, 1, 2 or 3");
    e.latency_prebin = value != 0;
    if (value) e.latency_prebin_mode = (int)value;
  } else if (k == "small_streams") {  // latency batches: 2 LSTM | other forests on two side streams, 1 one, 0 none
    FD_REQUIRE(value >= 0 && value <= 2, FD_ERR_INVALID_ARG, "small_streams must be 0, 1 or 2");
    e.small_streams = (int)value;
  } else if (k == "count_exchange") {  // fd_sharded_step's per-peer counts: 1 one ncclAllGather per batch, 0 2G
    // point-to-point operations in the records group, -1 (default) the all-gather from 4 ranks; set before
    // fd_comm_init or between steps with no batch prefetched (every rank the same)
    FD_REQUIRE(value >= -1 && value <= 1, FD_ERR_INVALID_ARG, "count_exchange must be -1, 0 or 1");
    FD_REQUIRE(!e.comm.pending, FD_ERR_INVALID_ARG, "count_exchange: a prefetched batch's counts are in flight");
    e.comm.count_mode = (int)value;
    e.comm.count_gather = value == 1 || (value < 0 && e.comm.world >= 4);
  } else if (k == "comm_timeout_ms") {  // fd_sharded_step: the split-size wait gives up (FD_ERR_HIP) after this
    FD_REQUIRE(value >= 1, FD_ERR_INVALID_ARG, "comm_timeout_ms must be >= 1");
    e.comm.timeout_ms = value;
  } else if (k == "stream_priority") {  // HIP stream priorities (ROCm keeps a hardware-queue pool per priority):
    // 0 all default; 1 the two pipeline streams high; 2 + the sharded step's forward stream low; 3 (default) + it
    // high. Set before the first pipelined call / fd_comm_init (the streams are created then). With every stream
    // at the default priority the process's 4 hardware queues are shared by the engine stream, the two pipeline
    // streams, the forward stream and RCCL's own: the engine stream's output copy (waiting for batch i's
    // forests) then sat in front of batch i+1's feature kernels in one queue — the native sharded step measured
    // 0.137 ms per 64 k batch at 0, 0.093 at 2 / 3 (the direct step 0.089 either way).
    FD_REQUIRE(value >= 0 && value <= 3, FD_ERR_INVALID_ARG, "stream_priority must be in 0..3");
    FD_REQUIRE(!e.pipe.stream[0] && !e.comm.x_fwd, FD_ERR_INVALID_ARG,
               "stream_priority: set before the first pipelined call and fd_comm_init");
    e.stream_prio = (int)value;
  } else if (k == "bucket_keys") {  // feature bucket pass: transactions per bucket workgroup, 0 auto (8 up to
    // 2048 transactions, 16 below 8192, else 128), else a power of two in 8..512
    FD_REQUIRE(value == 0 || (value >= 8 && value <= 512 && (value & (value - 1)) == 0), FD_ERR_INVALID_ARG,
               "bucket_keys must be 0 or a power of two in 8..512");
    e.state.bucket_keys = (int)value;
  } else if (k == "ensemble_bin_global") {  // the fused kernel's compact rows: 1 binned by searches of the merged
    // tables where they lie (L2), chunk 0's DMA issued at once; 0 the tables staged in LDS first
    FD_REQUIRE(value == 0 || value == 1, FD_ERR_INVALID_ARG, "ensemble_bin_global must be 0 or 1");
    e.ens_bin_global = value != 0;
  } else if (k == "lean_group") {  // pipelined stream: the lean bucket kernel's grouping of a bucket's keys by card,
    // 0 rank sort (first m threads, whole list each), 1 rank sort split over all threads, 2 (default) LDS hash table
    FD_REQUIRE(value >= 0 && value <= 2, FD_ERR_INVALID_ARG, "lean_group must be 0, 1 or 2");
    e.state.lean_group = (int)value;
  } else if (k == "slot_gather") {  // batches of <= 4096 transactions outside the pipelined stream: card slots found
    // inside the bucket kernel, no slot launch (1, default) / the slot kernel first (0)
    FD_REQUIRE(value == 0 || value == 1, FD_ERR_INVALID_ARG, "slot_gather must be 0 or 1");
    e.state.slot_gather = value != 0;
  } else if (k == "slot_stream") {  // fd_score_batch_pipelined: batch i's slot pass on a stream of its own (1 high
    // priority, 2 low; 0 on pipe_stream[i & 1] behind batch i-2's fused kernel; -1 auto by the card table's size),
    // set before the first pipelined call
    FD_REQUIRE(value >= -1 && value <= 2, FD_ERR_INVALID_ARG, "slot_stream must be -1, 0, 1 or 2");
    FD_REQUIRE(!e.pipe.slot_stream || (int)value == e.pipe.slot_mode, FD_ERR_INVALID_ARG,
               "slot_stream: set before the first pipelined call");
    e.pipe.slot_mode = (int)value;
  } else if (k == "slot_prio") {  // pipelined stream: 1 the slot kernel's waves issue at priority 2, 0 (default) not
    FD_REQUIRE(value == 0 || value == 1, FD_ERR_INVALID_ARG, "slot_prio must be 0 or 1");
    e.state.slot_prio = value != 0;
  } else if (k == "feature_prio") {  // pipelined stream: 1 the lean bucket kernel's waves issue at priority 2 (round 5's
    // default: DESIGN §3, 0.0857 -> 0.0843 ms per config-4 step at 200 steps), 0 (default since round 6) at the
    // default priority, below the fused kernel (ensemble_prio)
    FD_REQUIRE(value == 0 || value == 1, FD_ERR_INVALID_ARG, "feature_prio must be 0 or 1");
    e.state.feat_prio = value != 0;
  } else if (k == "bucket_spread") {  // feature bucket pass, >= 8 k transactions: 1 (default) card segments
    // round-robin over the 4 waves
    FD_REQUIRE(value == 0 || value == 1, FD_ERR_INVALID_ARG, "bucket_spread must be 0 or 1");
    e.state.bucket_spread = value != 0;
  } else if (k == "timing_every") {  // kernel timing (fd_timing_*): HIP events on one launch in N of each kind
    FD_REQUIRE(value >= 1 && value <= 1000000, FD_ERR_INVALID_ARG, "timing_every must be >= 1");
    e.timing_every = (int)value;
    for (auto& q : e.timing_seq) q = 0;  // the next launch of every kind is a timed one
  } else if (k == "seq_ring_lstm") {  // latency batches: 1 (default) the LSTM reads card histories from the ring
    FD_REQUIRE(value == 0 || value == 1, FD_ERR_INVALID_ARG, "seq_ring_lstm must be 0 or 1");
    e.seq_ring_lstm = value != 0;
  } else if (k == "gbdt_hist_rows") {  // gbdt.hip: rows a workgroup of the histogram kernel takes (the grid follows);
    // the sums are integers, so every value gives the same trees
    FD_REQUIRE(value >= 64 && value <= (1 << 20), FD_ERR_INVALID_ARG, "gbdt_hist_rows must be in 64..1048576");
    e.gbdt.hist_rows = (int)value;
  } else if (k == "lstm_rows") {  // LSTM tile: 0 auto (4 below 4096 transactions, else 16), 4 or 16
    FD_REQUIRE(value == 0 || value == 4 || value == 16, FD_ERR_INVALID_ARG, "lstm_rows must be 0, 4 or 16");
    e.lstm_rows = (int)value;
  } else if (k == "mlp_form") {  // MLP head: 0 auto (the reference shape's register form), 1 the LDS form always
    FD_REQUIRE(value == 0 || value == 1, FD_ERR_INVALID_ARG, "mlp_form must be 0 or 1");
    e.mlp_form = (int)value;
  } else if (k == "mlp_wgs_per_cu") {  // MLP head's persistent grid: workgroups per CU, 0 auto (2 where they fit)
    FD_REQUIRE(value >= 0 && value <= 8, FD_ERR_INVALID_ARG, "mlp_wgs_per_cu must be in 0..8");
    e.mlp_wgs_per_cu = (int)value;
  } else if (k == "mlp_fit_chunks_per_wg") {  // mlp_fit.hip: chunks (16-row tiles of the batch) a workgroup of the step
    // kernel takes in turn (the grid follows), 0 (default) one each; a chunk's partial depends on the batch alone, so
    // every value gives the same bits
    FD_REQUIRE(value >= 0 && value <= (1 << 30), FD_ERR_INVALID_ARG, "mlp_fit_chunks_per_wg must be in 0..2^30");
    e.mlp_fit.chunks_per_wg = (int)value;
  } else if (k == "ingest_stop_after") {  // diagnostics: 0 full; 1 stage; 2 + structure; 3 + members
    FD_REQUIRE(value >= 0 && value <= 3, FD_ERR_INVALID_ARG, "ingest_stop_after must be in 0..3");
    e.ingest.stop_after = (int)value;
  } else if (k == "rule_fraud_threshold_permille") {  // JobConfig.fraudThreshold x 1000
    FD_REQUIRE(value >= 0 && value <= 1000, FD_ERR_INVALID_ARG, "rule_fraud_threshold_permille must be in 0..1000");
    e.state.tp_threshold = (double)value / 1000.0;
  } else {
    throw fd::Error(FD_ERR_INVALID_ARG, "unknown option: " + k);
  }
  FD_API_END
}

int fd_timing_read(fd_engine* eng, int kind, double* total_ms, int64_t* launches) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E_quiet(eng);
  double tot = 0.0;
  int64_t cnt = 0;
  for (size_t i = 0; i < e.events_used; ++i) {
    if (kind >= 0 && e.events[i].kind != kind) continue;
    FD_HIP(hipEventSynchronize(e.events[i].b));
    float ms = 0.f;
    FD_HIP(hipEventElapsedTime(&ms, e.events[i].a, e.events[i].b));
    tot += ms;
    if (e.events[i].split) {
      FD_HIP(hipEventSynchronize(e.events[i].d));
      FD_HIP(hipEventElapsedTime(&ms, e.events[i].c, e.events[i].d));
      tot += ms;
    }
    ++cnt;
  }
  if (total_ms) *total_ms = tot;
  if (launches) *launches = cnt;
  FD_API_END
}

int fd_timing_reset(fd_engine* eng) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E_quiet(eng);
  for (size_t i = 0; i < e.events_used; ++i) {  // pairs on 2+ streams
    FD_HIP(hipEventSynchronize(e.events[i].b));
    if (e.events[i].split) FD_HIP(hipEventSynchronize(e.events[i].d));
  }
  e.events_used = 0;
  FD_API_END
}

int fd_load_forest(fd_engine* eng, int slot, const fd_forest_params* params, const fd_tree_arrays* trees) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E(eng);
  FD_REQUIRE(params && trees, FD_ERR_INVALID_ARG, "null params/trees");
  fd::PackedForest& pf = slot_of(e, slot);
  FD_HIP(hipStreamSynchronize(e.stream));  // a reload must not race an in-flight predict
  pf.loaded = false;
  fd::shap_forget(pf);  // covers and path table belong to the forest that leaves
  fd::repack_forest(pf, *params, *trees);
  FD_API_END
}

int fd_pack_forest_host(const fd_forest_params* params, const fd_tree_arrays* trees, void* blob,
                        int64_t blob_cap, int32_t* leaf_ids, int64_t ids_cap, fd_pack_info* info) {
  FD_API_BEGIN
  FD_REQUIRE(params && trees && info, FD_ERR_INVALID_ARG, "null params/trees/info");
  const fd::HostPack hp = fd::pack_forest_host(*params, *trees);
  info->n_trees = hp.n_trees;
  info->n_chunks = hp.n_chunks;
  info->chunk = hp.chunk;
  info->depth = hp.depth;
  info->tree_bytes = (int64_t)hp.tree_bytes;
  info->chunk_stride = (int64_t)hp.chunk_stride;
  info->blob_bytes = (int64_t)hp.blob.size();
  info->n_leaf_ids = (int64_t)hp.leaf_ids.size();
  info->base_margin = hp.base_margin;
  info->layout = 0;
  info->n_thresholds = (int64_t)hp.b_thr.size();
  info->bin_steps = hp.bin_steps;
  if (blob) {
    FD_REQUIRE(blob_cap >= (int64_t)hp.blob.size(), FD_ERR_INVALID_ARG, "blob buffer too small");
    std::memcpy(blob, hp.blob.data(), hp.blob.size());
  }
  if (leaf_ids) {
    FD_REQUIRE(ids_cap >= (int64_t)hp.leaf_ids.size(), FD_ERR_INVALID_ARG, "leaf id buffer too small");
    std::memcpy(leaf_ids, hp.leaf_ids.data(), hp.leaf_ids.size() * sizeof(int32_t));
  }
  FD_API_END
}

int fd_contract_forest_host(const fd_forest_params* params, const fd_tree_arrays* trees, int64_t* n_nodes,
                            fd_tree_arrays* out, int32_t* depths, int64_t* n_pruned) {
  FD_API_BEGIN
  FD_REQUIRE(params && trees, FD_ERR_INVALID_ARG, "null params/trees");
  const fd::ContractedForest c = fd::contract_forest_host(*params, *trees);
  const int32_t T = (int32_t)c.off.size() - 1;
  const int64_t M = (int64_t)c.left.size();
  if (n_nodes) *n_nodes = M;
  if (n_pruned) *n_pruned = (int64_t)c.pruned;
  if (depths) std::memcpy(depths, c.depth.data(), (size_t)T * 4);
  if (out) {
    FD_REQUIRE(out->tree_offsets && out->left && out->right && out->feature && out->threshold && out->default_left &&
                   out->leaf_value,
               FD_ERR_INVALID_ARG, "incomplete output arrays");
    out->n_trees = T;
    std::memcpy(const_cast<int64_t*>(out->tree_offsets), c.off.data(), (size_t)(T + 1) * 8);
    std::memcpy(const_cast<int32_t*>(out->left), c.left.data(), (size_t)M * 4);
    std::memcpy(const_cast<int32_t*>(out->right), c.right.data(), (size_t)M * 4);
    std::memcpy(const_cast<int32_t*>(out->feature), c.feature.data(), (size_t)M * 4);
    std::memcpy(const_cast<double*>(out->threshold), c.threshold.data(), (size_t)M * 8);
    std::memcpy(const_cast<uint8_t*>(out->default_left), c.dleft.data(), (size_t)M);
    std::memcpy(const_cast<double*>(out->leaf_value), c.leaf.data(), (size_t)M * 8);
  }
  FD_API_END
}

int fd_dense_layout_host(const fd_forest_params* params, const fd_tree_arrays* trees, int32_t wide, int32_t mode,
                         int32_t owner_bias, fd_dense_info* info, void* blob, int64_t* chunk_offsets,
                         int32_t* chunk_lengths, fd_dense_tree* tree_info, float* thresholds, int32_t* thr_offsets) {
  FD_API_BEGIN
  FD_REQUIRE(params && trees && info, FD_ERR_INVALID_ARG, "null params/trees/info");
  const fd::ContractedForest c = fd::contract_forest_host(*params, *trees);
  const bool xgb = params->kind == FD_FOREST_XGB_BINARY_LOGISTIC;
  // the forest's own tables: the distinct f32 thresholds of the contracted splits, per feature, ascending
  std::vector<std::vector<float>> tables((size_t)params->num_feature);
  for (size_t o = 0; o < c.left.size(); ++o)
    if (c.left[o] >= 0)
      tables[(size_t)c.feature[o]].push_back(xgb ? (float)c.threshold[o] : fd::sklearn_threshold_to_lt(c.threshold[o]));
  int64_t n_thr = 0;
  for (std::vector<float>& t : tables) {
    std::sort(t.begin(), t.end());
    t.erase(std::unique(t.begin(), t.end()), t.end());
    n_thr += (int64_t)t.size();
  }
  const fd::DenseLayout L = fd::dense_layout_host(c, xgb, tables, wide != 0, mode, owner_bias);
  info->n_chunks = (int32_t)L.chunk_len.size();
  info->s_max = fd::kDenseSMax;
  info->trees_per_bundle = L.tpg;
  info->buf_bytes = (int32_t)L.buf;
  info->blob_bytes = (int64_t)L.blob.size();
  info->n_thresholds = n_thr;
  info->node_steps = L.steps;
  if (blob) std::memcpy(blob, L.blob.data(), L.blob.size());
  if (chunk_offsets) std::memcpy(chunk_offsets, L.chunk_off.data(), L.chunk_off.size() * 8);
  if (chunk_lengths) std::memcpy(chunk_lengths, L.chunk_len.data(), L.chunk_len.size() * 4);
  if (tree_info) std::memcpy(tree_info, L.tree.data(), L.tree.size() * sizeof(fd_dense_tree));
  if (thr_offsets) thr_offsets[0] = 0;
  int64_t at = 0;
  for (size_t f = 0; f < tables.size(); ++f) {
    if (thresholds) std::memcpy(thresholds + at, tables[f].data(), tables[f].size() * 4);
    at += (int64_t)tables[f].size();
    if (thr_offsets) thr_offsets[f + 1] = (int32_t)at;
  }
  FD_API_END
}

int fd_pack_forest_binned_host(const fd_forest_params* params, const fd_tree_arrays* trees, void* blob,
                               int64_t blob_cap, float* thresholds, int64_t thr_cap, int32_t* offsets,
                               fd_pack_info* info) {
  FD_API_BEGIN
  FD_REQUIRE(params && trees && info, FD_ERR_INVALID_ARG, "null params/trees/info");
  const fd::HostPack hp = fd::pack_forest_host(*params, *trees);
  FD_REQUIRE(hp.binned, FD_ERR_UNSUPPORTED,
             "forest has no binned layout (depth > 8 or > 65534 distinct thresholds in a feature)");
  info->n_trees = hp.n_trees;
  info->n_chunks = hp.b_n_chunks;
  info->chunk = hp.b_chunk;
  info->depth = hp.depth;
  info->tree_bytes = (int64_t)hp.b_tree_bytes;
  info->chunk_stride = (int64_t)hp.b_chunk_stride;
  info->blob_bytes = (int64_t)hp.b_blob.size();
  info->n_leaf_ids = (int64_t)hp.leaf_ids.size();
  info->base_margin = hp.base_margin;
  info->layout = 1;
  info->n_thresholds = (int64_t)hp.b_thr.size();
  info->bin_steps = hp.bin_steps;
  if (blob) {
    FD_REQUIRE(blob_cap >= (int64_t)hp.b_blob.size(), FD_ERR_INVALID_ARG, "blob buffer too small");
    std::memcpy(blob, hp.b_blob.data(), hp.b_blob.size());
  }
  if (thresholds) {
    FD_REQUIRE(thr_cap >= (int64_t)hp.b_thr.size(), FD_ERR_INVALID_ARG, "threshold buffer too small");
    std::memcpy(thresholds, hp.b_thr.data(), hp.b_thr.size() * sizeof(float));
  }
  if (offsets) std::memcpy(offsets, hp.b_thr_off.data(), hp.b_thr_off.size() * sizeof(int32_t));
  FD_API_END
}

int fd_pack_forest_sparse_host(const fd_forest_params* params, const fd_tree_arrays* trees, void* nodes,
                               int64_t nodes_cap, void* leaf_values, int64_t values_cap, int32_t* leaf_ids,
                               int64_t ids_cap, fd_sparse_info* info) {
  FD_API_BEGIN
  FD_REQUIRE(params && trees && info, FD_ERR_INVALID_ARG, "null params/trees/info");
  const fd::SparsePack sp = fd::pack_forest_sparse_host(*params, *trees);
  *info = fd_sparse_info{};
  info->kind = sp.kind;
  info->n_trees = sp.n_trees;
  info->depth = sp.depth;
  info->leaf_bytes = sp.leaf_bytes;
  info->n_nodes = sp.n_nodes;
  info->n_leaves = sp.n_leaves;
  info->base_margin = sp.base_margin;
  if (nodes) {
    FD_REQUIRE(nodes_cap >= sp.n_nodes, FD_ERR_INVALID_ARG, "node buffer too small");
    std::memcpy(nodes, sp.nodes.data(), sp.nodes.size() * sizeof(uint32_t));
  }
  if (leaf_values) {
    FD_REQUIRE(values_cap >= sp.n_leaves, FD_ERR_INVALID_ARG, "leaf value buffer too small");
    std::memcpy(leaf_values, sp.leaf_val.data(), sp.leaf_val.size());
  }
  if (leaf_ids) {
    FD_REQUIRE(ids_cap >= sp.n_leaves, FD_ERR_INVALID_ARG, "leaf id buffer too small");
    std::memcpy(leaf_ids, sp.leaf_ids.data(), sp.leaf_ids.size() * sizeof(int32_t));
  }
  FD_API_END
}

int fd_load_xgboost_json(fd_engine* eng, int slot, const char* path) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E(eng);
  fd::PackedForest& pf = slot_of(e, slot);
  fd::XgbModel m;
  fd::read_xgboost_json(path, m);
  fd_forest_params p{};
  p.kind = FD_FOREST_XGB_BINARY_LOGISTIC;
  p.num_feature = m.num_feature;
  p.base_score = m.base_score;
  fd_tree_arrays t{};
  t.n_trees = (int32_t)(m.offsets.size() - 1);
  t.tree_offsets = m.offsets.data();
  t.left = m.left.data();
  t.right = m.right.data();
  t.feature = m.feature.data();
  t.threshold = m.threshold.data();
  t.default_left = m.default_left.data();
  t.leaf_value = m.leaf_value.data();
  FD_REQUIRE(t.n_trees > 0, FD_ERR_INVALID_ARG, "xgboost json: no trees");
  FD_HIP(hipStreamSynchronize(e.stream));  // a reload must not race an in-flight predict
  pf.loaded = false;
  fd::shap_forget(pf);
  fd::repack_forest(pf, p, t);
  // the file's sum_hessian as covers, when every reachable node has a usable one (else the slot has none)
  if (m.cover.size() == m.left.size() && fd::shap_cover_problem(t, m.cover.data()).empty()) pf.t_cover = m.cover;
  FD_API_END
}

int fd_xgboost_json_read(const char* path, fd_forest_params* params, int32_t* n_trees, int64_t* n_nodes,
                         fd_tree_arrays* trees) {
  FD_API_BEGIN
  fd::XgbModel m;
  fd::read_xgboost_json(path, m);
  const int32_t T = (int32_t)(m.offsets.size() - 1);
  const int64_t M = (int64_t)m.left.size();
  if (params) {
    *params = fd_forest_params{};
    params->kind = FD_FOREST_XGB_BINARY_LOGISTIC;
    params->num_feature = m.num_feature;
    params->base_score = m.base_score;
  }
  if (n_trees) *n_trees = T;
  if (n_nodes) *n_nodes = M;
  if (trees) {
    FD_REQUIRE(trees->tree_offsets && trees->left && trees->right && trees->feature && trees->threshold &&
                   trees->default_left && trees->leaf_value,
               FD_ERR_INVALID_ARG, "incomplete output arrays");
    trees->n_trees = T;
    std::memcpy(const_cast<int64_t*>(trees->tree_offsets), m.offsets.data(), (size_t)(T + 1) * 8);
    std::memcpy(const_cast<int32_t*>(trees->left), m.left.data(), (size_t)M * 4);
    std::memcpy(const_cast<int32_t*>(trees->right), m.right.data(), (size_t)M * 4);
    std::memcpy(const_cast<int32_t*>(trees->feature), m.feature.data(), (size_t)M * 4);
    std::memcpy(const_cast<double*>(trees->threshold), m.threshold.data(), (size_t)M * 8);
    std::memcpy(const_cast<uint8_t*>(trees->default_left), m.default_left.data(), (size_t)M);
    std::memcpy(const_cast<double*>(trees->leaf_value), m.leaf_value.data(), (size_t)M * 8);
  }
  FD_API_END
}

int fd_unload_forest(fd_engine* eng, int slot) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E(eng);
  fd::PackedForest& pf = slot_of(e, slot);
  FD_HIP(hipStreamSynchronize(e.stream));
  pf.drop_device();
  fd::shap_forget(pf);  // the covers
  pf.sparse_only = false;
  pf.binned = false;
  pf.loaded = false;
  pf.gen = 0;  // any ensemble plan built over this slot is stale
  FD_API_END
}

int fd_forest_info(fd_engine* eng, int slot, int32_t* n_trees, int32_t* depth, int32_t* num_feature) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E(eng);
  fd::PackedForest& pf = slot_of(e, slot);
  FD_REQUIRE(pf.loaded, FD_ERR_NOT_LOADED, "Model in slot " + std::to_string(slot) + " not loaded");
  if (n_trees) *n_trees = pf.n_trees;
  if (depth) *depth = pf.depth;
  if (num_feature) *num_feature = pf.num_feature;
  FD_API_END
}

int fd_forest_predict_device(fd_engine* eng, int slot, const float* d_X, int64_t n, int32_t ld,
                             double* d_prob, double* d_raw, int32_t* d_leaf) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E(eng);
  fd::PackedForest& pf = slot_of(e, slot);
  FD_REQUIRE(pf.loaded, FD_ERR_NOT_LOADED, "Model in slot " + std::to_string(slot) + " not loaded");
  FD_REQUIRE(n >= 0, FD_ERR_INVALID_ARG, "negative n");
  fd::launch_forest(e, pf, d_X, n, ld, d_prob, d_raw, d_leaf);
  FD_API_END
}

int fd_forest_predict_host(fd_engine* eng, int slot, const float* X, int64_t n, int32_t ld, double* prob,
                           double* raw, int32_t* leaf) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E(eng);
  fd::PackedForest& pf = slot_of(e, slot);
  FD_REQUIRE(pf.loaded, FD_ERR_NOT_LOADED, "Model in slot " + std::to_string(slot) + " not loaded");
  FD_REQUIRE(n >= 0 && ld > 0 && X && prob, FD_ERR_INVALID_ARG, "bad arguments");
  if (n == 0) return FD_OK;
  Stage st(e);
  const float* dX;
  double *dprob, *draw;
  int32_t* dleaf;
  st.in(dX, X, (size_t)n * ld);
  st.out(dprob, prob, (size_t)n);
  st.out(draw, raw, (size_t)n);
  st.out(dleaf, leaf, (size_t)n * pf.n_trees);
  st.upload();
  fd::launch_forest(e, pf, dX, n, ld, dprob, draw, dleaf);
  st.download();
  FD_API_END
}

// ---------------------------------------------------------------- forest attribution (shap.hip)

static fd_tree_arrays tree_arrays_of(const fd::PackedForest& pf) {
  fd_tree_arrays t{};
  t.n_trees = (int32_t)pf.t_off.size() - 1;
  t.tree_offsets = pf.t_off.data();
  t.left = pf.t_left.data();
  t.right = pf.t_right.data();
  t.feature = pf.t_feature.data();
  t.threshold = pf.t_threshold.data();
  t.default_left = pf.t_dleft.data();
  t.leaf_value = pf.t_leaf.data();
  return t;
}

int fd_forest_set_cover(fd_engine* eng, int slot, const double* cover, int64_t n_nodes) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E(eng);
  fd::PackedForest& pf = slot_of(e, slot);
  FD_REQUIRE(pf.loaded && !pf.t_off.empty(), FD_ERR_NOT_LOADED, "Model in slot " + std::to_string(slot) + " not loaded");
  FD_REQUIRE(cover != nullptr && n_nodes == pf.t_off.back(), FD_ERR_INVALID_ARG,
             "cover: one value per node of the forest (" + std::to_string(pf.t_off.back()) + ")");
  const std::string bad = fd::shap_cover_problem(tree_arrays_of(pf), cover);
  FD_REQUIRE(bad.empty(), FD_ERR_INVALID_ARG, bad);
  FD_HIP(hipStreamSynchronize(e.stream));  // an explain call in flight reads the table these covers replace
  fd::shap_forget(pf);
  pf.t_cover.assign(cover, cover + n_nodes);
  FD_API_END
}

int fd_xgboost_json_read_cover(const char* path, double* cover, int64_t cap, int64_t* n_nodes) {
  FD_API_BEGIN
  fd::XgbModel m;
  fd::read_xgboost_json(path, m);
  const int64_t M = (int64_t)m.left.size();
  if (n_nodes) *n_nodes = M;
  if (cover) {
    FD_REQUIRE((int64_t)m.cover.size() == M, FD_ERR_INVALID_ARG, "xgboost json: a tree without sum_hessian");
    FD_REQUIRE(cap >= M, FD_ERR_INVALID_ARG, "cover buffer too small");
    std::memcpy(cover, m.cover.data(), (size_t)M * 8);
  }
  FD_API_END
}

int fd_shap_paths_host(const fd_forest_params* params, const fd_tree_arrays* trees, const double* cover,
                       fd_shap_path* paths, int64_t paths_cap, fd_shap_elem* elems, int64_t elems_cap,
                       fd_shap_info* info) {
  FD_API_BEGIN
  FD_REQUIRE(params && trees && info, FD_ERR_INVALID_ARG, "null params/trees/info");
  const fd::ShapTable tb = fd::shap_paths_host(*params, *trees, cover);
  *info = tb.info;
  if (paths) {
    FD_REQUIRE(paths_cap >= tb.info.n_paths, FD_ERR_INVALID_ARG, "path buffer too small");
    std::memcpy(paths, tb.paths.data(), tb.paths.size() * sizeof(fd_shap_path));
  }
  if (elems) {
    FD_REQUIRE(elems_cap >= tb.info.n_elems, FD_ERR_INVALID_ARG, "element buffer too small");
    std::memcpy(elems, tb.elems.data(), tb.elems.size() * sizeof(fd_shap_elem));
  }
  FD_API_END
}

int fd_forest_shap_ref_host(const fd_forest_params* params, const fd_tree_arrays* trees, const double* cover,
                            const float* X, int64_t n, int32_t ld, double* phi, int32_t ld_phi) {
  FD_API_BEGIN
  FD_REQUIRE(params && trees, FD_ERR_INVALID_ARG, "null params/trees");
  fd::shap_ref_host(*params, *trees, cover, X, n, ld, phi, ld_phi);
  FD_API_END
}

int fd_forest_shap_device(fd_engine* eng, int slot, const float* d_X, int64_t n, int32_t ld, const int64_t* d_rows,
                          int64_t n_rows, double* d_phi, int32_t ld_phi) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E(eng);
  fd::PackedForest& pf = slot_of(e, slot);
  FD_REQUIRE(pf.loaded, FD_ERR_NOT_LOADED, "Model in slot " + std::to_string(slot) + " not loaded");
  FD_REQUIRE(n >= 0 && (!d_rows || n_rows >= 0), FD_ERR_INVALID_ARG, "negative n");
  fd::launch_forest_shap(e, pf, d_X, n, ld, d_rows, n_rows, d_phi, ld_phi);
  FD_API_END
}

int fd_forest_shap_host(fd_engine* eng, int slot, const float* X, int64_t n, int32_t ld, const int64_t* rows,
                        int64_t n_rows, double* phi, int32_t ld_phi) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E(eng);
  fd::PackedForest& pf = slot_of(e, slot);
  FD_REQUIRE(pf.loaded, FD_ERR_NOT_LOADED, "Model in slot " + std::to_string(slot) + " not loaded");
  FD_REQUIRE(n >= 0 && ld > 0 && (!rows || n_rows >= 0), FD_ERR_INVALID_ARG, "bad arguments");
  const int64_t total = rows ? n_rows : n;
  for (int64_t j = 0; rows && j < n_rows; ++j)
    FD_REQUIRE(rows[j] >= 0 && rows[j] < n, FD_ERR_INVALID_ARG,
               "rows[" + std::to_string(j) + "] = " + std::to_string(rows[j]) + " is outside [0, n)");
  if (total == 0 || n == 0) {  // nothing to stage; the argument and cover checks still run
    fd::launch_forest_shap(e, pf, nullptr, n, ld, rows, 0, nullptr, ld_phi);
    return FD_OK;
  }
  FD_REQUIRE(X && phi, FD_ERR_INVALID_ARG, "null X / phi");
  Stage st(e);
  const float* dX;
  const int64_t* drows;
  double* dphi;
  st.in(dX, X, (size_t)n * ld);
  st.in(drows, rows, (size_t)(rows ? n_rows : 0));
  st.out(dphi, phi, (size_t)total * ld_phi);
  st.upload();
  if (ld_phi > pf.num_feature + 1)  // the staged rows come back whole: columns past the bias as zeros
    FD_HIP(hipMemsetAsync(dphi, 0, (size_t)total * ld_phi * sizeof(double), e.stream));
  fd::launch_forest_shap(e, pf, dX, n, ld, drows, n_rows, dphi, ld_phi);
  st.download();
  FD_API_END
}

int fd_shap_topk_device(fd_engine* eng, const double* d_phi, int64_t n, int32_t ld_phi, int32_t num_feature, int32_t k,
                        int32_t by_abs, int32_t* d_idx, double* d_val) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E(eng);
  fd::launch_shap_topk(e, d_phi, n, ld_phi, num_feature, k, by_abs != 0, d_idx, d_val);
  FD_API_END
}

int fd_shap_topk_host(fd_engine* eng, const double* phi, int64_t n, int32_t ld_phi, int32_t num_feature, int32_t k,
                      int32_t by_abs, int32_t* idx, double* val) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E(eng);
  FD_REQUIRE(n >= 0 && ld_phi > 0 && k >= 1 && k <= FD_SHAP_MAX_TOPK, FD_ERR_INVALID_ARG,
             "bad arguments (k must be in [1, 16])");
  if (n == 0) return FD_OK;
  FD_REQUIRE(phi && idx && val, FD_ERR_INVALID_ARG, "null phi / idx / val");
  Stage st(e);
  const double* dphi;
  int32_t* didx;
  double* dval;
  st.in(dphi, phi, (size_t)n * ld_phi);
  st.out(didx, idx, (size_t)n * k);
  st.out(dval, val, (size_t)n * k);
  st.upload();
  fd::launch_shap_topk(e, dphi, n, ld_phi, num_feature, k, by_abs != 0, didx, dval);
  st.download();
  FD_API_END
}

// ---------------------------------------------------------------- training: histogram GBDT (gbdt.hip)

int fd_gbdt_cuts_host(const float* X, int64_t n, int32_t ld, int32_t F, int32_t max_bin, float* cuts,
                      int32_t* offsets, int64_t* n_cuts) {
  FD_API_BEGIN
  std::vector<float> c;
  std::vector<int32_t> o;
  const int64_t total = fd::gbdt_cuts_host(X, n, ld, F, max_bin, c, o, 16);
  if (n_cuts) *n_cuts = total;
  if (cuts && offsets) {
    std::memcpy(offsets, o.data(), o.size() * sizeof(int32_t));
    if (total) std::memcpy(cuts, c.data(), (size_t)total * sizeof(float));
  }
  FD_API_END
}

int fd_gbdt_bin_ref_host(const float* X, int64_t n, int32_t ld, int32_t F, const float* cuts, const int32_t* offsets,
                         uint8_t* bins) {
  FD_API_BEGIN
  FD_REQUIRE(F >= 1 && F <= 64 && ld >= F && n >= 0 && offsets, FD_ERR_INVALID_ARG, "gbdt: bad arguments");
  FD_REQUIRE(n == 0 || (X && bins), FD_ERR_INVALID_ARG, "gbdt: null X / bins");
  fd::gbdt_bin_ref_host(X, n, ld, F, cuts, offsets, bins);
  FD_API_END
}

int fd_gbdt_bin_device(fd_engine* eng, const float* d_X, int64_t n, int32_t ld, int32_t F, const float* d_cuts,
                       const int32_t* d_offsets, uint8_t* d_bins) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E(eng);
  fd::launch_gbdt_bin(e, d_X, n, ld, F, d_cuts, d_offsets, d_bins);
  FD_API_END
}

int fd_gbdt_bin_host(fd_engine* eng, const float* X, int64_t n, int32_t ld, int32_t F, const float* cuts,
                     const int32_t* offsets, uint8_t* bins) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E(eng);
  FD_REQUIRE(F >= 1 && F <= 64 && ld >= F && n >= 0 && offsets && offsets[0] == 0, FD_ERR_INVALID_ARG,
             "gbdt: bad arguments");
  for (int f = 0; f < F; ++f)
    FD_REQUIRE(offsets[f + 1] >= offsets[f], FD_ERR_INVALID_ARG, "gbdt: decreasing cut offsets");
  if (n == 0) return FD_OK;
  FD_REQUIRE(X && bins, FD_ERR_INVALID_ARG, "gbdt: null X / bins");
  const float none = 0.0f;
  const size_t nc = (size_t)offsets[F];
  Stage st(e);
  const float *dX, *dcuts;
  const int32_t* doff;
  uint8_t* dbins;
  st.in(dX, X, (size_t)n * ld);
  st.in(dcuts, nc ? cuts : &none, std::max<size_t>(nc, 1));
  st.in(doff, offsets, (size_t)F + 1);
  st.out(dbins, bins, (size_t)n * F);
  st.upload();
  fd::launch_gbdt_bin(e, dX, n, ld, F, dcuts, doff, dbins);
  st.download();
  FD_API_END
}

int fd_gbdt_grad_ref_host(const float* margin, const uint8_t* y, int64_t n, int32_t* g, int32_t* h) {
  FD_API_BEGIN
  FD_REQUIRE(n >= 0 && (n == 0 || (margin && y && g && h)), FD_ERR_INVALID_ARG, "gbdt: null margin / y / g / h");
  for (int64_t i = 0; i < n; ++i) FD_REQUIRE(y[i] <= 1, FD_ERR_INVALID_ARG, "gbdt: labels must be 0 or 1");
  fd::gbdt_grad_ref_host(margin, y, n, g, h);
  FD_API_END
}

int fd_gbdt_grad_host(fd_engine* eng, const float* margin, const uint8_t* y, int64_t n, int32_t* g, int32_t* h) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E(eng);
  FD_REQUIRE(n >= 0 && (n == 0 || (margin && y && g && h)), FD_ERR_INVALID_ARG, "gbdt: null margin / y / g / h");
  for (int64_t i = 0; i < n; ++i) FD_REQUIRE(y[i] <= 1, FD_ERR_INVALID_ARG, "gbdt: labels must be 0 or 1");
  if (n == 0) return FD_OK;
  Stage st(e);
  const float* dm;
  const uint8_t* dy;
  int32_t *dg, *dh;
  st.in(dm, margin, (size_t)n);
  st.in(dy, y, (size_t)n);
  st.out(dg, g, (size_t)n);
  st.out(dh, h, (size_t)n);
  st.upload();
  fd::launch_gbdt_grad(e, dm, dy, n, dg, dh);
  st.download();
  FD_API_END
}

int fd_gbdt_grow_tree_ref_host(const uint8_t* bins, int64_t n, int32_t F, const float* cuts, const int32_t* offsets,
                               const int32_t* g, const int32_t* h, const uint8_t* row_mask, uint64_t feature_mask,
                               const fd_gbdt_params* params, fd_gbdt_model* out, int64_t* n_nodes) {
  FD_API_BEGIN
  FD_REQUIRE(params && out && offsets && (n == 0 || (bins && g && h)), FD_ERR_INVALID_ARG, "gbdt: null argument");
  fd::gbdt_grow_tree_ref_host(bins, n, F, cuts, offsets, g, h, row_mask, feature_mask, *params, *out, n_nodes);
  FD_API_END
}

int fd_gbdt_grow_tree_device(fd_engine* eng, const uint8_t* d_bins, int64_t n, int32_t F, const float* cuts,
                             const int32_t* offsets, const int32_t* d_g, const int32_t* d_h, const uint8_t* d_row_mask,
                             uint64_t feature_mask, const fd_gbdt_params* params, fd_gbdt_model* out,
                             int64_t* n_nodes) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E(eng);
  FD_REQUIRE(params && out && offsets && (n == 0 || (d_bins && d_g && d_h)), FD_ERR_INVALID_ARG,
             "gbdt: null argument");
  fd::gbdt_grow_tree_device(e, d_bins, n, F, cuts, offsets, d_g, d_h, d_row_mask, feature_mask, *params, *out,
                            n_nodes);
  FD_API_END
}

int fd_gbdt_grow_tree_host(fd_engine* eng, const uint8_t* bins, int64_t n, int32_t F, const float* cuts,
                           const int32_t* offsets, const int32_t* g, const int32_t* h, const uint8_t* row_mask,
                           uint64_t feature_mask, const fd_gbdt_params* params, fd_gbdt_model* out, int64_t* n_nodes) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E(eng);
  FD_REQUIRE(params && out && offsets && (n == 0 || (bins && g && h)), FD_ERR_INVALID_ARG, "gbdt: null argument");
  fd::gbdt_check_params(*params, n, F, false);
  const uint8_t none = 0;
  const int32_t zero = 0;
  Stage st(e);
  const uint8_t *dbins, *dmask;
  const int32_t *dg, *dh;
  st.in(dbins, n ? bins : &none, std::max<size_t>((size_t)n * F, 1));
  st.in(dg, n ? g : &zero, std::max<size_t>((size_t)n, 1));
  st.in(dh, n ? h : &zero, std::max<size_t>((size_t)n, 1));
  st.in(dmask, row_mask, (size_t)n);
  st.upload();
  fd::gbdt_grow_tree_device(e, dbins, n, F, cuts, offsets, dg, dh, n ? dmask : nullptr, feature_mask, *params, *out,
                            n_nodes);
  FD_API_END
}

static void gbdt_capacity(const fd_gbdt_params& p, int64_t n, int32_t F, int64_t* n_nodes) {
  fd::gbdt_check_params(p, n, F, true);
  FD_REQUIRE(n_nodes, FD_ERR_INVALID_ARG, "gbdt: null n_nodes");
  *n_nodes = (int64_t)p.n_rounds * ((1ll << (p.max_depth + 1)) - 1);
}

int fd_gbdt_fit_ref_host(const float* X, const uint8_t* y, int64_t n, int32_t ld, int32_t F,
                         const fd_gbdt_params* params, fd_gbdt_model* out, int64_t* n_nodes, float* margins) {
  FD_API_BEGIN
  FD_REQUIRE(params, FD_ERR_INVALID_ARG, "gbdt: null params");
  if (!out) {
    gbdt_capacity(*params, n, F, n_nodes);
    return FD_OK;
  }
  FD_REQUIRE(n == 0 || (X && y), FD_ERR_INVALID_ARG, "gbdt: null X / y");
  fd::gbdt_fit_ref_host(X, y, n, ld, F, *params, *out, n_nodes, margins);
  FD_API_END
}

int fd_gbdt_fit_device(fd_engine* eng, const float* d_X, const uint8_t* d_y, int64_t n, int32_t ld, int32_t F,
                       const fd_gbdt_params* params, fd_gbdt_model* out, int64_t* n_nodes, float* d_margins) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E(eng);
  FD_REQUIRE(params, FD_ERR_INVALID_ARG, "gbdt: null params");
  if (!out) {
    gbdt_capacity(*params, n, F, n_nodes);
    return FD_OK;
  }
  FD_REQUIRE(n == 0 || (d_X && d_y), FD_ERR_INVALID_ARG, "gbdt: null X / y");
  fd::gbdt_fit_device(e, d_X, d_y, n, ld, F, *params, *out, n_nodes, d_margins);
  FD_API_END
}

int fd_gbdt_fit_host(fd_engine* eng, const float* X, const uint8_t* y, int64_t n, int32_t ld, int32_t F,
                     const fd_gbdt_params* params, fd_gbdt_model* out, int64_t* n_nodes, float* margins) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E(eng);
  FD_REQUIRE(params, FD_ERR_INVALID_ARG, "gbdt: null params");
  if (!out) {
    gbdt_capacity(*params, n, F, n_nodes);
    return FD_OK;
  }
  fd::gbdt_check_params(*params, n, F, true);
  FD_REQUIRE(n == 0 || (X && y), FD_ERR_INVALID_ARG, "gbdt: null X / y");
  FD_REQUIRE(ld >= F, FD_ERR_INVALID_ARG, "gbdt: ld < F");
  for (int64_t i = 0; i < n; ++i) FD_REQUIRE(y[i] <= 1, FD_ERR_INVALID_ARG, "gbdt: labels must be 0 or 1");
  const float none = 0.0f;
  const uint8_t zero = 0;
  Stage st(e);
  const float* dX;
  const uint8_t* dy;
  float* dm;
  st.in(dX, n ? X : &none, std::max<size_t>((size_t)n * ld, 1));
  st.in(dy, n ? y : &zero, std::max<size_t>((size_t)n, 1));
  st.out(dm, margins, (size_t)n);
  st.upload();
  fd::gbdt_fit_staged(e, dX, n ? X : &none, dy, n, ld, F, *params, *out, n_nodes, dm);
  st.download();
  FD_API_END
}

int fd_gbdt_fit_eval_ref_host(const float* X, const uint8_t* y, int64_t n, int32_t ld, int32_t F,
                              const fd_gbdt_params* params, fd_gbdt_eval* eval, fd_gbdt_model* out, int64_t* n_nodes,
                              float* margins) {
  FD_API_BEGIN
  FD_REQUIRE(params, FD_ERR_INVALID_ARG, "gbdt: null params");
  if (!out) {
    gbdt_capacity(*params, n, F, n_nodes);
    return FD_OK;
  }
  FD_REQUIRE(eval, FD_ERR_INVALID_ARG, "gbdt: null eval");
  FD_REQUIRE(n == 0 || (X && y), FD_ERR_INVALID_ARG, "gbdt: null X / y");
  fd::gbdt_fit_ref_host(X, y, n, ld, F, *params, *out, n_nodes, margins, eval);
  FD_API_END
}

int fd_gbdt_fit_eval_device(fd_engine* eng, const float* d_X, const uint8_t* d_y, int64_t n, int32_t ld, int32_t F,
                            const fd_gbdt_params* params, fd_gbdt_eval* eval, fd_gbdt_model* out, int64_t* n_nodes,
                            float* d_margins) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E(eng);
  FD_REQUIRE(params, FD_ERR_INVALID_ARG, "gbdt: null params");
  if (!out) {
    gbdt_capacity(*params, n, F, n_nodes);
    return FD_OK;
  }
  FD_REQUIRE(eval, FD_ERR_INVALID_ARG, "gbdt: null eval");
  FD_REQUIRE(n == 0 || (d_X && d_y), FD_ERR_INVALID_ARG, "gbdt: null X / y");
  fd::gbdt_fit_eval_device(e, d_X, nullptr, d_y, n, ld, F, *params, *eval, *out, n_nodes, d_margins);
  FD_API_END
}

int fd_gbdt_fit_eval_host(fd_engine* eng, const float* X, const uint8_t* y, int64_t n, int32_t ld, int32_t F,
                          const fd_gbdt_params* params, fd_gbdt_eval* eval, fd_gbdt_model* out, int64_t* n_nodes,
                          float* margins) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E(eng);
  FD_REQUIRE(params, FD_ERR_INVALID_ARG, "gbdt: null params");
  if (!out) {
    gbdt_capacity(*params, n, F, n_nodes);
    return FD_OK;
  }
  FD_REQUIRE(eval, FD_ERR_INVALID_ARG, "gbdt: null eval");
  fd::gbdt_check_params(*params, n, F, true);
  FD_REQUIRE(n == 0 || (X && y), FD_ERR_INVALID_ARG, "gbdt: null X / y");
  FD_REQUIRE(ld >= F, FD_ERR_INVALID_ARG, "gbdt: ld < F");
  const bool watched = fd::gbdt_check_eval(*eval, n, F, true);
  for (int64_t i = 0; i < n; ++i) FD_REQUIRE(y[i] <= 1, FD_ERR_INVALID_ARG, "gbdt: labels must be 0 or 1");
  const float none = 0.0f;
  const uint8_t zero = 0;
  Stage st(e);
  const float *dX, *deX = nullptr;
  const uint8_t *dy, *dey = nullptr;
  float *dm, *dem = nullptr, *dbm = nullptr;
  st.in(dX, n ? X : &none, std::max<size_t>((size_t)n * ld, 1));
  st.in(dy, n ? y : &zero, std::max<size_t>((size_t)n, 1));
  st.out(dm, margins, (size_t)n);
  if (watched) {
    st.in(deX, eval->X, (size_t)eval->n * eval->ld);
    st.in(dey, eval->y, (size_t)eval->n);
    st.out(dem, eval->margins, (size_t)eval->n);
    st.out(dbm, eval->best_margins, (size_t)n);
  }
  st.upload();
  fd_gbdt_eval dev = *eval;  // the same arguments with the staged pointers
  dev.X = deX;
  dev.y = dey;
  dev.margins = dem;
  dev.best_margins = dbm;
  fd::gbdt_fit_eval_device(e, dX, n ? X : &none, dy, n, ld, F, *params, dev, *out, n_nodes, dm);
  st.download();
  eval->rounds_run = dev.rounds_run;
  eval->best_iteration = dev.best_iteration;
  FD_API_END
}

int fd_gbdt_metric_ref_host(const float* margins, const uint8_t* y, int64_t n, int32_t metric, double* out) {
  FD_API_BEGIN
  FD_REQUIRE(n >= 1 && margins && y && out, FD_ERR_INVALID_ARG, "gbdt: the metric needs margins, labels and n >= 1");
  FD_REQUIRE(metric == FD_GBDT_METRIC_AUC || metric == FD_GBDT_METRIC_ERROR, FD_ERR_INVALID_ARG,
             "gbdt: unknown eval metric");
  FD_REQUIRE(n <= (1ll << 28), FD_ERR_UNSUPPORTED, "gbdt: more than 2^28 eval rows");
  fd::gbdt_check_metric_labels(y, n, metric);
  *out = fd::gbdt_metric_ref_host(margins, y, n, metric);
  FD_API_END
}

int fd_gbdt_grad_weighted_ref_host(const float* margin, const uint8_t* y, int64_t n, double scale_pos_weight,
                                   int32_t* g, int32_t* h) {
  FD_API_BEGIN
  FD_REQUIRE(n >= 0 && (n == 0 || (margin && y && g && h)), FD_ERR_INVALID_ARG, "gbdt: null margin / y / g / h");
  FD_REQUIRE(scale_pos_weight > 0.0 && scale_pos_weight <= 64.0, FD_ERR_INVALID_ARG,
             "gbdt: scale_pos_weight must be in (0, 64]");
  for (int64_t i = 0; i < n; ++i) FD_REQUIRE(y[i] <= 1, FD_ERR_INVALID_ARG, "gbdt: labels must be 0 or 1");
  fd::gbdt_grad_weighted_ref_host(margin, y, n, scale_pos_weight, g, h);
  FD_API_END
}

int fd_gbdt_metric_host(fd_engine* eng, const float* margins, const uint8_t* y, int64_t n, int32_t metric,
                        double* out) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E(eng);
  FD_REQUIRE(n >= 1 && margins && y && out, FD_ERR_INVALID_ARG, "gbdt: the metric needs margins, labels and n >= 1");
  FD_REQUIRE(metric == FD_GBDT_METRIC_AUC || metric == FD_GBDT_METRIC_ERROR, FD_ERR_INVALID_ARG,
             "gbdt: unknown eval metric");
  FD_REQUIRE(n <= (1ll << 28), FD_ERR_UNSUPPORTED, "gbdt: more than 2^28 eval rows");
  fd::gbdt_check_metric_labels(y, n, metric);
  Stage st(e);
  const float* dm;
  const uint8_t* dy;
  st.in(dm, margins, (size_t)n);
  st.in(dy, y, (size_t)n);
  st.upload();
  *out = fd::gbdt_metric_device(e, dm, dy, n, metric);
  FD_API_END
}

// ---------------------------------------------------------------- training: IsolationForest (iforest_fit.hip)

// the first of the two calls: only the node capacity
static void iforest_fit_capacity(const fd_iforest_fit_params& p, int64_t n, int32_t ld, int32_t F, int64_t* n_nodes) {
  fd::iforest_fit_check(p, n, ld, F);
  FD_REQUIRE(n_nodes, FD_ERR_INVALID_ARG, "iforest_fit: null n_nodes");
  *n_nodes = fd::iforest_fit_capacity(p, n);
}

int fd_iforest_fit_ref_host(const float* X, int64_t n, int32_t ld, int32_t F, const fd_iforest_fit_params* params,
                            fd_tree_arrays* out, double* n_node_samples, fd_forest_params* forest, int64_t* n_nodes) {
  FD_API_BEGIN
  FD_REQUIRE(params, FD_ERR_INVALID_ARG, "iforest_fit: null params");
  if (!out) {
    iforest_fit_capacity(*params, n, ld, F, n_nodes);
    return FD_OK;
  }
  FD_REQUIRE(X && forest, FD_ERR_INVALID_ARG, "iforest_fit: null X / forest");
  fd::iforest_fit_ref_host(X, n, ld, F, *params, *out, n_node_samples, *forest, n_nodes);
  FD_API_END
}

int fd_iforest_fit_device(fd_engine* eng, const float* d_X, int64_t n, int32_t ld, int32_t F,
                          const fd_iforest_fit_params* params, fd_tree_arrays* out, double* n_node_samples,
                          fd_forest_params* forest, int64_t* n_nodes) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E(eng);
  FD_REQUIRE(params, FD_ERR_INVALID_ARG, "iforest_fit: null params");
  if (!out) {
    iforest_fit_capacity(*params, n, ld, F, n_nodes);
    return FD_OK;
  }
  FD_REQUIRE(d_X && forest, FD_ERR_INVALID_ARG, "iforest_fit: null X / forest");
  fd::iforest_fit_device(e, d_X, n, ld, F, *params, *out, n_node_samples, *forest, n_nodes);
  FD_API_END
}

int fd_iforest_fit_host(fd_engine* eng, const float* X, int64_t n, int32_t ld, int32_t F,
                        const fd_iforest_fit_params* params, fd_tree_arrays* out, double* n_node_samples,
                        fd_forest_params* forest, int64_t* n_nodes) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E(eng);
  FD_REQUIRE(params, FD_ERR_INVALID_ARG, "iforest_fit: null params");
  if (!out) {
    iforest_fit_capacity(*params, n, ld, F, n_nodes);
    return FD_OK;
  }
  fd::iforest_fit_check(*params, n, ld, F);
  FD_REQUIRE(X && forest, FD_ERR_INVALID_ARG, "iforest_fit: null X / forest");
  fd::iforest_fit_check_finite(X, n, ld, F);
  Stage st(e);
  const float* dX;
  st.in(dX, X, (size_t)n * ld);
  st.upload();
  fd::iforest_fit_device(e, dX, n, ld, F, *params, *out, n_node_samples, *forest, n_nodes);
  FD_API_END
}

// what the two sample seams check before a row id is computed
static void iforest_sample_check(int64_t n, const fd_iforest_fit_params* params, int32_t tree, const int32_t* rows) {
  FD_REQUIRE(params && rows, FD_ERR_INVALID_ARG, "iforest_fit: null params / rows");
  fd::iforest_fit_check(*params, n, 1, 1);
  FD_REQUIRE(tree >= 0 && tree < 65536, FD_ERR_INVALID_ARG, "iforest_fit: tree must be in 0..65535");
}

int fd_iforest_fit_sample_ref_host(int64_t n, const fd_iforest_fit_params* params, int32_t tree, int32_t* rows,
                                   int32_t* psi) {
  FD_API_BEGIN
  iforest_sample_check(n, params, tree, rows);
  fd::iforest_fit_sample_ref_host(n, *params, tree, rows, psi);
  FD_API_END
}

int fd_iforest_fit_sample_host(fd_engine* eng, int64_t n, const fd_iforest_fit_params* params, int32_t tree,
                               int32_t* rows, int32_t* psi) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E(eng);
  iforest_sample_check(n, params, tree, rows);
  fd::iforest_fit_sample_device(e, n, *params, tree, rows, psi);
  FD_API_END
}

static void iforest_grow_check(const float* X, int64_t n, int32_t ld, int32_t F, const fd_iforest_fit_params* params,
                               int32_t tree, const fd_tree_arrays* out) {
  FD_REQUIRE(params && out && X, FD_ERR_INVALID_ARG, "iforest_fit: null params / out / X");
  FD_REQUIRE(n >= 1 && n <= 2147483647ll && F >= 1 && F <= 64 && ld >= F, FD_ERR_INVALID_ARG,
             "iforest_fit: n must be in 1..2^31 - 1, F in 1..64 and ld >= F");
  FD_REQUIRE(tree >= 0 && tree < 65536, FD_ERR_INVALID_ARG, "iforest_fit: tree must be in 0..65535");
}

int fd_iforest_fit_grow_tree_ref_host(const float* X, int64_t n, int32_t ld, int32_t F, const int32_t* rows,
                                      int32_t m, uint64_t feature_mask, const fd_iforest_fit_params* params,
                                      int32_t tree, fd_tree_arrays* out, double* n_node_samples, int64_t* n_nodes) {
  FD_API_BEGIN
  iforest_grow_check(X, n, ld, F, params, tree, out);
  fd::iforest_fit_grow_tree_ref_host(X, n, ld, F, rows, m, feature_mask, *params, tree, *out, n_node_samples, n_nodes);
  FD_API_END
}

int fd_iforest_fit_grow_tree_host(fd_engine* eng, const float* X, int64_t n, int32_t ld, int32_t F,
                                  const int32_t* rows, int32_t m, uint64_t feature_mask,
                                  const fd_iforest_fit_params* params, int32_t tree, fd_tree_arrays* out,
                                  double* n_node_samples, int64_t* n_nodes) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E(eng);
  iforest_grow_check(X, n, ld, F, params, tree, out);
  Stage st(e);
  const float* dX;
  st.in(dX, X, (size_t)n * ld);
  st.upload();
  fd::iforest_fit_grow_tree_device(e, dX, n, ld, F, rows, m, feature_mask, *params, tree, *out, n_node_samples,
                                   n_nodes);
  FD_API_END
}

// ---------------------------------------------------------------- training: the PyTorch MLP member (mlp_fit.hip)

int fd_mlp_fit_ref_host(const float* X, const uint8_t* y, int64_t n, int32_t ld, const fd_mlp_fit_params* params,
                        fd_mlp_fit_out* out) {
  FD_API_BEGIN
  FD_REQUIRE(params && out, FD_ERR_INVALID_ARG, "mlp_fit: null params / out");
  fd::mlp_fit_ref_host(X, y, n, ld, *params, *out);
  FD_API_END
}

int fd_mlp_fit_device(fd_engine* eng, const float* d_X, const uint8_t* d_y, int64_t n, int32_t ld,
                      const fd_mlp_fit_params* params, fd_mlp_fit_out* out) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E(eng);
  FD_REQUIRE(params && out, FD_ERR_INVALID_ARG, "mlp_fit: null params / out");
  fd::mlp_fit_device(e, d_X, d_y, n, ld, *params, *out);
  FD_API_END
}

int fd_mlp_fit_host(fd_engine* eng, const float* X, const uint8_t* y, int64_t n, int32_t ld,
                    const fd_mlp_fit_params* params, fd_mlp_fit_out* out) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E(eng);
  FD_REQUIRE(params && out, FD_ERR_INVALID_ARG, "mlp_fit: null params / out");
  fd::mlp_fit_check(*params, n, ld, true);
  fd::mlp_fit_check_inputs(X, y, n, ld, *params);
  Stage st(e);
  const float* dX;
  const uint8_t* dy;
  st.in(dX, X, (size_t)n * ld);
  st.in(dy, y, (size_t)n);
  st.upload();
  fd::mlp_fit_device(e, dX, dy, n, ld, *params, *out);
  FD_API_END
}

int fd_mlp_grad_ref_host(const float* X, const uint8_t* y, int64_t n, int32_t ld, const fd_mlp_fit_params* params,
                         const uint8_t* masks, fd_mlp_fit_out* out) {
  FD_API_BEGIN
  FD_REQUIRE(params && out, FD_ERR_INVALID_ARG, "mlp_grad: null params / out");
  fd::mlp_grad_ref_host(X, y, n, ld, *params, masks, *out);
  FD_API_END
}

int fd_mlp_grad_device(fd_engine* eng, const float* d_X, const uint8_t* d_y, int64_t n, int32_t ld,
                       const fd_mlp_fit_params* params, const uint8_t* d_masks, fd_mlp_fit_out* out) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E(eng);
  FD_REQUIRE(params && out, FD_ERR_INVALID_ARG, "mlp_grad: null params / out");
  fd::mlp_grad_device(e, d_X, d_y, n, ld, *params, d_masks, *out);
  FD_API_END
}

int fd_mlp_grad_host(fd_engine* eng, const float* X, const uint8_t* y, int64_t n, int32_t ld,
                     const fd_mlp_fit_params* params, const uint8_t* masks, fd_mlp_fit_out* out) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E(eng);
  FD_REQUIRE(params && out, FD_ERR_INVALID_ARG, "mlp_grad: null params / out");
  fd::mlp_fit_check(*params, n, ld, false);
  fd::mlp_fit_check_inputs(X, y, n, ld, *params);
  Stage st(e);
  const float* dX;
  const uint8_t* dy;
  const uint8_t* dm;
  st.in(dX, X, (size_t)n * ld);
  st.in(dy, y, (size_t)n);
  st.in(dm, masks, (size_t)(params->n_layers - 1) * n * 64);
  st.upload();
  fd::mlp_grad_device(e, dX, dy, n, ld, *params, dm, *out);
  FD_API_END
}

// what the two batch seams check before an order or a mask is computed (no weights are read)
static void mlp_batch_check(int64_t n, const fd_mlp_fit_params* params) {
  FD_REQUIRE(params, FD_ERR_INVALID_ARG, "mlp_fit: null params");
  FD_REQUIRE(params->n_layers >= 2 && params->n_layers <= 8, FD_ERR_UNSUPPORTED, "MLP n_layers must be in [2, 8]");
  FD_REQUIRE(n >= 1 && n <= 2147483647ll, FD_ERR_INVALID_ARG, "mlp_fit: n must be in 1..2^31 - 1");
  FD_REQUIRE(params->epochs >= 1 && params->batch_size >= 1 && params->batch_size <= 65536, FD_ERR_INVALID_ARG,
             "mlp_fit: epochs must be at least 1 and batch_size in 1..65536");
  FD_REQUIRE(params->dropout >= 0.0 && params->dropout < 1.0, FD_ERR_INVALID_ARG, "mlp_fit: dropout must be in [0, 1)");
}

int fd_mlp_fit_batch_host(int64_t n, const fd_mlp_fit_params* params, int32_t epoch, int64_t step, int32_t* order,
                          uint8_t* masks, int32_t* rows) {
  FD_API_BEGIN
  mlp_batch_check(n, params);
  fd::mlp_fit_batch_ref_host(n, *params, epoch, step, order, masks, rows);
  FD_API_END
}

int fd_mlp_fit_batch_device(fd_engine* eng, int64_t n, const fd_mlp_fit_params* params, int32_t epoch, int64_t step,
                            int32_t* order, uint8_t* masks, int32_t* rows) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E(eng);
  mlp_batch_check(n, params);
  fd::mlp_fit_batch_device(e, n, *params, epoch, step, order, masks, rows);
  FD_API_END
}

int fd_state_init(fd_engine* eng, const fd_state_params* params) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E(eng);
  FD_REQUIRE(params, FD_ERR_INVALID_ARG, "null params");
  FD_HIP(hipStreamSynchronize(e.stream));
  fd::state_init(e, *params);
  FD_API_END
}

int fd_state_clear(fd_engine* eng) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E(eng);
  fd::state_clear(e);
  FD_API_END
}

int fd_state_info(fd_engine* eng, int64_t* capacity, int64_t* cards) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E(eng);
  fd::features_check(e);
  if (capacity) *capacity = e.state.cap;
  if (cards) *cards = fd::state_count(e);
  FD_API_END
}

int fd_state_load_users_host(fd_engine* eng, const fd_users* users) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E(eng);
  FD_REQUIRE(users, FD_ERR_INVALID_ARG, "null users");
  fd::load_users(e, *users);
  FD_API_END
}

int fd_load_merchants_host(fd_engine* eng, const fd_merchants* merchants) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E(eng);
  FD_REQUIRE(merchants, FD_ERR_INVALID_ARG, "null merchants");
  FD_HIP(hipStreamSynchronize(e.stream));
  fd::load_merchants(e, *merchants);
  FD_API_END
}

int fd_features_device(fd_engine* eng, const fd_txn_batch* txns, int64_t n, float* d_vectors, double* d_raw) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E(eng);
  FD_REQUIRE(txns, FD_ERR_INVALID_ARG, "null txns");
  fd::launch_features(e, *txns, n, d_vectors, d_raw);
  FD_API_END
}

int fd_features_host(fd_engine* eng, const fd_txn_batch* txns, int64_t n, float* vectors, double* raw) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E(eng);
  FD_REQUIRE(txns && vectors && n >= 0, FD_ERR_INVALID_ARG, "bad arguments");
  if (n == 0) return FD_OK;
  FD_REQUIRE(txns->card_key && txns->ts_ms && txns->amount_cents && txns->device_fp && txns->merchant &&
                 txns->ip_class && txns->hour && txns->weekend,
             FD_ERR_INVALID_ARG, "incomplete transaction batch");
  Stage st(e);
  fd_txn_batch d{};
  float* dv;
  double* dr;
  stage_txns(st, d, *txns, n, fd::kTxnAll);
  st.out(dv, vectors, (size_t)n * FD_VECTOR_WIDTH);
  st.out(dr, raw, (size_t)n * FD_RAW_FEATURES);
  st.upload();
  fd::launch_features(e, d, n, dv, dr);
  st.download(/*wait=*/false);
  fd::features_check(e);  // synchronises
  FD_API_END
}

int fd_score_matrix_device(fd_engine* eng, const fd_blend_params* params, const int32_t* slots,
                           const double* const* ext_probs, const uint8_t* present, const float* d_X,
                           int64_t n, int32_t ld, double* d_model_probs, double* d_fraud_prob,
                           double* d_confidence, uint8_t* d_decision, uint8_t* d_risk) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E(eng);
  FD_REQUIRE(params && d_X && ld > 0 && n >= 0, FD_ERR_INVALID_ARG, "bad arguments");
  fd::score_matrix(e, ModelSet(params, slots, ext_probs, present), fd::ScoreRows(d_X, n, ld),
                   ScoreOut{d_model_probs, d_fraud_prob, d_confidence, d_decision, d_risk});
  FD_API_END
}

int fd_score_matrix_host(fd_engine* eng, const fd_blend_params* params, const int32_t* slots,
                         const double* const* ext_probs, const uint8_t* present, const float* X, int64_t n,
                         int32_t ld, double* model_probs, double* fraud_prob, double* confidence,
                         uint8_t* decision, uint8_t* risk) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E(eng);
  FD_REQUIRE(params && slots && X && fraud_prob && ld > 0 && n >= 0, FD_ERR_INVALID_ARG, "bad arguments");
  fd::require_model_count(*params, "n_models out of range");
  if (n == 0) return FD_OK;
  const int M = params->n_models;
  const ModelSet host(params, slots, ext_probs, present);
  Stage st(e);
  fd::ScoreRows rows(nullptr, n, ld);
  const double* dext[FD_MAX_MODELS] = {};
  ScoreOut out;
  st.in(rows.X, X, (size_t)n * ld);
  for (int m = 0; m < M; ++m) {  // the external columns; score_matrix copies each into its place in the matrix
    if (!host.external(m)) continue;
    FD_REQUIRE(ext_probs && ext_probs[m], FD_ERR_INVALID_ARG, "model without slot needs an external probability column");
    st.in(dext[m], ext_probs[m], (size_t)n);
  }
  st.out(out.mp, model_probs, (size_t)n * M);  // absent: score_matrix keeps the matrix in its own scratch
  st.out(out.fp, fraud_prob, (size_t)n);
  st.out(out.conf, confidence, (size_t)n);
  st.out(out.dec, decision, (size_t)n);
  st.out(out.risk, risk, (size_t)n);
  st.upload();
  fd::score_matrix(e, ModelSet(params, slots, dext, present), rows, out);
  st.download();
  FD_API_END
}

int fd_score_batch_device(fd_engine* eng, const fd_blend_params* params, const int32_t* slots,
                          const double* const* ext_probs, const uint8_t* present, const fd_txn_batch* txns,
                          int64_t n, float* d_vectors, double* d_model_probs, double* d_fraud_prob,
                          double* d_confidence, uint8_t* d_decision, uint8_t* d_risk) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E(eng);
  FD_REQUIRE(params && txns && n >= 0, FD_ERR_INVALID_ARG, "bad arguments");
  if (n == 0) return FD_OK;
  FD_REQUIRE(slots != nullptr && d_fraud_prob != nullptr, FD_ERR_INVALID_ARG, "null slots/output");
  fd::score_batch(e, ModelSet(params, slots, ext_probs, present), *txns, n, d_vectors,
                  ScoreOut{d_model_probs, d_fraud_prob, d_confidence, d_decision, d_risk});
  FD_API_END
}

int fd_score_batch_pipelined(fd_engine* eng, const fd_blend_params* params, const int32_t* slots,
                             const double* const* ext_probs, const uint8_t* present, const fd_txn_batch* txns,
                             int64_t n, float* d_vectors, double* d_model_probs, double* d_fraud_prob,
                             double* d_confidence, uint8_t* d_decision, uint8_t* d_risk, void* input_ready) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E_quiet(eng);
  FD_REQUIRE(params && txns && n >= 0, FD_ERR_INVALID_ARG, "bad arguments");
  if (n == 0) return FD_OK;
  FD_REQUIRE(d_fraud_prob != nullptr, FD_ERR_INVALID_ARG, "null fraud_prob output");
  fd::require_model_count(*params, "bad n_models");
  fd::PipeBatch b;
  b.txns = txns;
  b.n = n;
  b.d_vectors = d_vectors;
  b.out = ScoreOut{d_model_probs, d_fraud_prob, d_confidence, d_decision, d_risk};
  b.input_ready = input_ready;
  const auto t0 = std::chrono::steady_clock::now();
  fd::pipe_step(e, ModelSet(params, slots, ext_probs, present), b);
  e.pipe.host_ns += (unsigned long long)std::chrono::duration_cast<std::chrono::nanoseconds>(
                        std::chrono::steady_clock::now() - t0).count();
  FD_API_END
}

int fd_score_records_pipelined(fd_engine* eng, const fd_blend_params* params, const int32_t* slots,
                               const uint8_t* present, const void* d_records, int64_t n, void* d_results,
                               void* input_ready) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E_quiet(eng);
  FD_REQUIRE(params && slots && n >= 0, FD_ERR_INVALID_ARG, "bad arguments");
  fd::require_model_count(*params, "bad n_models");
  const ModelSet ms(params, slots, nullptr, present);
  fd::require_all_in_slots(ms);
  if (n == 0) return FD_OK;
  FD_REQUIRE(d_records != nullptr && d_results != nullptr, FD_ERR_INVALID_ARG, "null records / results");
  fd::PipeBatch b;
  b.records = d_records;
  b.n = n;
  b.d_results = d_results;
  b.input_ready = input_ready;
  fd::pipe_step(e, ms, b);
  FD_API_END
}

// ---------------------------------------------------------------- card-hash sharded step over RCCL (comm.hip)
int fd_comm_unique_id(const char* rccl_path, uint8_t* id_out) {
  FD_API_BEGIN
  FD_REQUIRE(id_out, FD_ERR_INVALID_ARG, "null id");
  fd::comm_unique_id(rccl_path, id_out);
  FD_API_END
}

int fd_comm_init(fd_engine* eng, const char* rccl_path, int32_t rank, int32_t world, const uint8_t* id_fwd,
                 const uint8_t* id_back) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E_quiet(eng);
  fd::comm_init(e, rccl_path, rank, world, id_fwd, id_back);
  FD_API_END
}

int fd_comm_destroy(fd_engine* eng) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E_quiet(eng);
  fd::comm_destroy(e);
  FD_API_END
}

int fd_sharded_step(fd_engine* eng, const fd_blend_params* params, const int32_t* slots, const uint8_t* present,
                    const fd_txn_batch* txns, int64_t n, uint64_t batch_id, void* input_ready,
                    const fd_txn_batch* next, int64_t next_n, uint64_t next_id, void* next_ready,
                    double* d_fraud_prob, double* d_confidence, uint8_t* d_decision, uint8_t* d_risk,
                    int64_t* split_sizes) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E_quiet(eng);
  fd::ShardComm& c = e.comm;
  FD_REQUIRE(c.ready, FD_ERR_NOT_LOADED, "no communicators (fd_comm_init)");
  FD_REQUIRE(!c.aborted, FD_ERR_HIP, "communicators aborted (" + c.abort_reason + "): fd_comm_destroy, then fd_comm_init");
  FD_REQUIRE(params && slots && txns && n >= 0 && (!next || next_n >= 0), FD_ERR_INVALID_ARG, "bad arguments");
  FD_REQUIRE(!next || next_id != 0, FD_ERR_INVALID_ARG, "a prefetched batch needs a nonzero next_id");
  fd::require_model_count(*params, "bad n_models");
  const ModelSet ms(params, slots, nullptr, present);
  fd::require_all_in_slots(ms);
  FD_REQUIRE(n == 0 || d_fraud_prob, FD_ERR_INVALID_ARG, "null fraud_prob output");
  const fd::ShardBatch cur{txns, n, batch_id, static_cast<hipEvent_t>(input_ready)};
  const fd::ShardBatch nxt{next, next_n, next_id, static_cast<hipEvent_t>(next_ready)};
  fd::sharded_step(e, ms, cur, next ? &nxt : nullptr, ScoreOut{nullptr, d_fraud_prob, d_confidence, d_decision, d_risk},
                   split_sizes);
  FD_API_END
}

int fd_state_load_users_ext_host(fd_engine* eng, const fd_users_ext* users) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E(eng);
  FD_REQUIRE(users, FD_ERR_INVALID_ARG, "null users");
  fd::load_users_ext(e, *users);
  FD_API_END
}

int fd_load_merchants_ext_host(fd_engine* eng, const fd_merchants_ext* merchants) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E(eng);
  FD_REQUIRE(merchants, FD_ERR_INVALID_ARG, "null merchants");
  FD_HIP(hipStreamSynchronize(e.stream));
  fd::load_merchants_ext(e, *merchants);
  FD_API_END
}

int fd_load_vocab_host(fd_engine* eng, const uint8_t* payment_high_risk, const uint8_t* type_is_refund) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E(eng);
  FD_HIP(hipStreamSynchronize(e.stream));
  fd::load_vocab(e, payment_high_risk, type_is_refund);
  FD_API_END
}

int fd_features_full_device(fd_engine* eng, const fd_txn_batch* txns, const fd_txn_context* ctx, int64_t n,
                            float* d_vectors, double* d_raw, double* d_fmap, fd_rule_scores* d_rules) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E(eng);
  FD_REQUIRE(txns, FD_ERR_INVALID_ARG, "null txns");
  const fd_txn_context none{};
  fd::launch_features_full(e, *txns, ctx ? *ctx : none, n, d_vectors, d_raw, d_fmap, d_rules);
  FD_API_END
}

int fd_windows_init(fd_engine* eng, const fd_window_params* params) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E(eng);
  FD_REQUIRE(params, FD_ERR_INVALID_ARG, "null params");
  FD_HIP(hipStreamSynchronize(e.stream));
  fd::windows_init(e, *params);
  FD_API_END
}

int fd_windows_step_device(fd_engine* eng, const fd_txn_batch* txns, const fd_window_inputs* in, int64_t n,
                           int flush, fd_user_window* user_out, int64_t user_cap, int64_t* n_user,
                           fd_merchant_window* merchant_out, int64_t merchant_cap, int64_t* n_merchant) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E(eng);
  FD_REQUIRE(n_user && n_merchant, FD_ERR_INVALID_ARG, "null result counts");
  const fd_txn_batch none_t{};
  const fd_window_inputs none_in{};
  FD_REQUIRE(txns || n == 0, FD_ERR_INVALID_ARG, "null txns");
  fd::windows_step(e, txns ? *txns : none_t, in ? *in : none_in, n, flush != 0, user_out, user_cap, n_user,
                   merchant_out, merchant_cap, n_merchant, /*timed=*/true);
  FD_API_END
}

int fd_windows_step_host(fd_engine* eng, const fd_txn_batch* txns, const fd_window_inputs* in, int64_t n, int flush,
                         fd_user_window* user_out, int64_t user_cap, int64_t* n_user,
                         fd_merchant_window* merchant_out, int64_t merchant_cap, int64_t* n_merchant) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E(eng);
  FD_REQUIRE(n_user && n_merchant, FD_ERR_INVALID_ARG, "null result counts");
  FD_REQUIRE(n >= 0 && (txns || n == 0), FD_ERR_INVALID_ARG, "bad batch");
  fd_txn_batch dt{};
  fd_window_inputs di{};
  if (n > 0) {
    FD_REQUIRE(txns->card_key && txns->ts_ms && txns->amount_cents && txns->merchant, FD_ERR_INVALID_ARG,
               "batch needs card_key, ts_ms, amount_cents and merchant");
    const fd_window_inputs hi = in ? *in : fd_window_inputs{};
    Stage st(e);
    stage_txns(st, dt, *txns, n, fd::kTxnKey | fd::kTxnTs | fd::kTxnCents | fd::kTxnMerchant);
    st.in(di.payment_method, hi.payment_method, (size_t)n);
    st.in(di.is_fraud, hi.is_fraud, (size_t)n);
    st.in(di.fraud_score, hi.fraud_score, (size_t)n);
    st.upload();
  }
  fd::windows_step(e, dt, di, n, flush != 0, user_out, user_cap, n_user, merchant_out, merchant_cap, n_merchant);
  FD_API_END
}

int fd_windows_stats(fd_engine* eng, int64_t* watermark, int64_t* user_events, int64_t* merchant_events) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E(eng);
  FD_REQUIRE(e.windows.ready, FD_ERR_NOT_LOADED, "windows not initialised (fd_windows_init)");
  if (watermark) *watermark = e.windows.wm;
  if (user_events) *user_events = e.windows.ucount;
  if (merchant_events) *merchant_events = e.windows.mcount;
  FD_API_END
}

int fd_windows_observe(fd_engine* eng, int64_t max_event_ts) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  fd::windows_observe(E(eng), max_event_ts);
  FD_API_END
}

int fd_merchant_windows_merge(const fd_merchant_window* parts, int64_t n, fd_merchant_window* out, int64_t* n_out) {
  FD_API_BEGIN
  fd::merchant_windows_merge(parts, n, out, n_out);
  FD_API_END
}

int fd_sink_init(fd_engine* eng, const fd_sink_params* params) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E(eng);
  FD_REQUIRE(params, FD_ERR_INVALID_ARG, "null params");
  FD_HIP(hipStreamSynchronize(e.stream));
  fd::sink_init(e, *params);
  FD_API_END
}

int fd_sink_update_device(fd_engine* eng, const fd_txn_batch* txns, const fd_window_inputs* in, int64_t n) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E(eng);
  FD_REQUIRE(txns, FD_ERR_INVALID_ARG, "null batch");
  const fd_window_inputs none{nullptr, nullptr, nullptr};
  fd::sink_update(e, *txns, in ? *in : none, n);
  FD_API_END
}

int fd_sink_update_host(fd_engine* eng, const fd_txn_batch* txns, const fd_window_inputs* in, int64_t n) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E(eng);
  FD_REQUIRE(txns && n >= 0, FD_ERR_INVALID_ARG, "bad arguments");
  if (n == 0) return FD_OK;
  FD_REQUIRE(txns->card_key && txns->ts_ms && txns->amount_cents && txns->merchant, FD_ERR_INVALID_ARG,
             "batch needs card_key, ts_ms, amount_cents and merchant");
  Stage st(e);
  fd_txn_batch d{};
  fd_window_inputs din{};  // (the sink does not read payment_method)
  stage_txns(st, d, *txns, n, fd::kTxnKey | fd::kTxnTs | fd::kTxnCents | fd::kTxnMerchant);
  st.in(din.is_fraud, in ? in->is_fraud : nullptr, (size_t)n);
  st.in(din.fraud_score, in ? in->fraud_score : nullptr, (size_t)n);
  st.upload();
  fd::sink_update(e, d, din, n);  // no wait here: the next call on e.stream is ordered behind it
  FD_API_END
}

int fd_sink_query_host(fd_engine* eng, int32_t kind, const int64_t* bucket, const int32_t* merchant, int64_t n,
                       fd_aggregate* out) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E(eng);
  fd::sink_query(e, kind, bucket, merchant, n, out);
  FD_API_END
}

int fd_sink_evict_before(fd_engine* eng, int64_t hour_key, int64_t* kept_entries, int64_t* kept_users) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E(eng);
  fd::sink_evict_before(e, hour_key, kept_entries, kept_users);
  FD_API_END
}

int fd_hash64(const uint8_t* bytes, int64_t n, uint64_t* out) {
  FD_API_BEGIN
  FD_REQUIRE(out && n >= 0 && (n == 0 || bytes), FD_ERR_INVALID_ARG, "bad arguments");
  *out = fd::hash_bytes(bytes, n);
  FD_API_END
}

int fd_ingest_set_vocab(fd_engine* eng, int32_t which, const uint8_t* bytes, const int64_t* offsets, int64_t n) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E(eng);
  fd::ingest_set_vocab(e, which, bytes, offsets, n);
  FD_API_END
}

int fd_ingest_set_merchants(fd_engine* eng, const uint8_t* bytes, const int64_t* offsets, int64_t n) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E(eng);
  fd::ingest_set_merchants(e, bytes, offsets, n);
  FD_API_END
}

int fd_ingest_json_device(fd_engine* eng, const uint8_t* d_bytes, const int64_t* d_offsets, int64_t n,
                          const fd_ingest_out* d_out) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E(eng);
  FD_REQUIRE(d_out, FD_ERR_INVALID_ARG, "null outputs");
  fd::launch_ingest(e, d_bytes, d_offsets, n, *d_out);
  FD_API_END
}

int fd_ingest_json_host(fd_engine* eng, const uint8_t* bytes, const int64_t* offsets, int64_t n,
                        const fd_ingest_out* out) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E(eng);
  FD_REQUIRE(out && offsets && n >= 0, FD_ERR_INVALID_ARG, "bad arguments");
  if (n == 0) return FD_OK;
  FD_REQUIRE(offsets[0] == 0 && offsets[n] >= 0, FD_ERR_INVALID_ARG, "offsets must start at 0");
  const size_t nb = (size_t)offsets[n];
  Stage st(e);
  const uint8_t* d_bytes;
  const int64_t* d_offsets;
  static const uint8_t no_bytes = 0;  // nb == 0: the kernel still gets a byte pointer, and `bytes` may be null
  st.in(d_bytes, nb ? bytes : &no_bytes, nb);
  st.in(d_offsets, offsets, (size_t)n + 1);
  fd_ingest_out d{};
  auto col = [&](auto member) { st.out(d.*member, out->*member, (size_t)n); };
  col(&fd_ingest_out::card_key);
  col(&fd_ingest_out::ts_ms);
  col(&fd_ingest_out::amount_cents);
  col(&fd_ingest_out::merchant);
  col(&fd_ingest_out::device_fp);
  col(&fd_ingest_out::ip_class);
  col(&fd_ingest_out::hour);
  col(&fd_ingest_out::weekend);
  col(&fd_ingest_out::geo_lat);
  col(&fd_ingest_out::geo_lon);
  col(&fd_ingest_out::merchant_lat);
  col(&fd_ingest_out::merchant_lon);
  col(&fd_ingest_out::payment_method);
  col(&fd_ingest_out::transaction_type);
  col(&fd_ingest_out::card_type);
  col(&fd_ingest_out::user_agent_flag);
  col(&fd_ingest_out::fraud_score);
  col(&fd_ingest_out::is_fraud);
  col(&fd_ingest_out::txn_hash);
  col(&fd_ingest_out::status);
  st.upload();
  fd::launch_ingest(e, d_bytes, d_offsets, n, d);
  st.download();
  FD_API_END
}

int fd_ingest_scalar_host(int32_t kind, const uint8_t* text, int32_t n, double* f64_out, int64_t* i64_out,
                          int32_t* flags_out) {
  FD_API_BEGIN
  FD_REQUIRE(text && n >= 0 && flags_out, FD_ERR_INVALID_ARG, "bad arguments");
  *flags_out = 0;
  if (kind == 0 || kind == 1) {
    fd::Decimal d;
    const int end = fd::scan_number(text, 0, n, d);
    if (end != n) {
      *flags_out = 1;
      return FD_OK;
    }
    if (kind == 0) {
      bool amb = false;
      const double v = fd::decimal_to_double(d.w, d.q, d.neg, d.many, &amb);
      if (f64_out) *f64_out = v;
      if (amb) *flags_out |= 2;
    } else {
      bool inexact = false;
      int64_t c = 0;
      if (!fd::decimal_to_cents(d, &c, &inexact)) *flags_out |= 1;
      if (inexact) *flags_out |= 2;
      if (i64_out) *i64_out = c;
    }
  } else if (kind == 2) {
    int64_t ms = 0;
    if (!fd::parse_iso_instant(text, 0, n, &ms)) *flags_out = 1;
    if (i64_out) *i64_out = ms;
  } else {
    throw fd::Error(FD_ERR_INVALID_ARG, "unknown scalar kind");
  }
  FD_API_END
}

int fd_state_snapshot(fd_engine* eng, const char* path, int32_t shard, int32_t n_shards, int64_t* bytes_written) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E(eng);
  fd::features_check(e);
  fd::state_snapshot(e, path, shard, n_shards, bytes_written);
  FD_API_END
}

int fd_state_restore(fd_engine* eng, const char* path, int32_t shard, int32_t n_shards, int32_t flags,
                     int64_t* cards_restored) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E(eng);
  fd::features_check(e);
  fd::state_restore(e, path, shard, n_shards, flags, cards_restored);
  FD_API_END
}

int fd_load_lstm(fd_engine* eng, const fd_lstm_params* params) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E(eng);
  FD_REQUIRE(params, FD_ERR_INVALID_ARG, "null params");
  FD_HIP(hipStreamSynchronize(e.stream));
  if (e.side.st[0]) FD_HIP(hipStreamSynchronize(e.side.st[0]));
  fd::load_lstm(e, *params);
  FD_API_END
}

int fd_unload_lstm(fd_engine* eng) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E(eng);
  FD_HIP(hipStreamSynchronize(e.stream));
  if (e.side.st[0]) FD_HIP(hipStreamSynchronize(e.side.st[0]));
  for (auto* b : {&e.lstm.wpk, &e.lstm.wpk4, &e.lstm.bias, &e.lstm.wout, &e.lstm.bout}) b->release();
  e.lstm.loaded = false;
  FD_API_END
}

int fd_lstm_predict_device(fd_engine* eng, const float* d_seq, int64_t n, int32_t T, double* d_prob) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E(eng);
  fd::launch_lstm(e, e.stream, d_seq, n, T, d_prob);
  FD_API_END
}

int fd_lstm_predict_host(fd_engine* eng, const float* seq, int64_t n, int32_t T, double* prob) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E(eng);
  FD_REQUIRE(n >= 0 && T >= 1 && T <= FD_MAX_SEQ_LEN, FD_ERR_INVALID_ARG, "bad arguments");
  if (n == 0) return FD_OK;
  FD_REQUIRE(seq && prob, FD_ERR_INVALID_ARG, "null sequence / output");
  Stage st(e);
  const float* dseq;
  double* dprob;
  st.in(dseq, seq, (size_t)n * T * fd::kSeqInput);
  st.out(dprob, prob, (size_t)n);
  st.upload();
  fd::launch_lstm(e, e.stream, dseq, n, T, dprob);
  st.download();
  FD_API_END
}

int fd_pack_mlp_host(const fd_mlp_params* params, void* blob, int64_t cap, int64_t* bytes) {
  FD_API_BEGIN
  FD_REQUIRE(params && bytes, FD_ERR_INVALID_ARG, "null params/bytes");
  const std::vector<uint32_t> pk = fd::pack_mlp_host(*params);
  *bytes = (int64_t)pk.size() * 4;
  if (blob) {
    FD_REQUIRE(cap >= *bytes, FD_ERR_INVALID_ARG, "blob buffer too small");
    std::memcpy(blob, pk.data(), pk.size() * 4);
  }
  FD_API_END
}

// every stream a scoring call may have put the MLP's launches on
static void mlp_quiesce(Engine& e) {
  FD_HIP(hipStreamSynchronize(e.stream));
  for (hipStream_t st : e.pipe.stream)
    if (st) FD_HIP(hipStreamSynchronize(st));
}

int fd_load_mlp(fd_engine* eng, const fd_mlp_params* params) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E(eng);
  FD_REQUIRE(params, FD_ERR_INVALID_ARG, "null params");
  mlp_quiesce(e);  // a reload must not race an in-flight predict
  fd::load_mlp(e, *params);
  FD_API_END
}

int fd_unload_mlp(fd_engine* eng) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E(eng);
  mlp_quiesce(e);
  e.mlp.blob.release();
  e.mlp.loaded = false;
  FD_API_END
}

int fd_mlp_info(fd_engine* eng, int32_t* n_layers, int32_t* in_dim, int32_t* hidden) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E_quiet(eng);
  FD_REQUIRE(e.mlp.loaded, FD_ERR_NOT_LOADED, "Model graph_neural (MLP) not loaded");
  if (n_layers) *n_layers = e.mlp.n_layers;
  if (in_dim) *in_dim = e.mlp.dims[0];
  if (hidden) *hidden = e.mlp.dims[1];
  FD_API_END
}

int fd_mlp_predict_device(fd_engine* eng, const float* d_X, int64_t n, int32_t ld, double* d_prob) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E(eng);
  fd::launch_mlp(e, e.stream, d_X, n, ld, d_prob);
  FD_API_END
}

int fd_mlp_predict_host(fd_engine* eng, const float* X, int64_t n, int32_t ld, double* prob) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E(eng);
  FD_REQUIRE(e.mlp.loaded, FD_ERR_NOT_LOADED, "Model graph_neural (MLP) not loaded");
  FD_REQUIRE(n >= 0 && n < (1ll << 31), FD_ERR_INVALID_ARG, "batch size out of range");
  FD_REQUIRE(ld >= e.mlp.dims[0], FD_ERR_INVALID_ARG,
             "row stride " + std::to_string(ld) + " is below the MLP's in_dim " + std::to_string(e.mlp.dims[0]));
  if (n == 0) return FD_OK;
  FD_REQUIRE(X && prob, FD_ERR_INVALID_ARG, "null vectors / output");
  Stage st(e);
  const float* dX;
  double* dprob;
  st.in(dX, X, (size_t)n * ld);
  st.out(dprob, prob, (size_t)n);
  st.upload();
  fd::launch_mlp(e, e.stream, dX, n, ld, dprob);
  st.download();
  FD_API_END
}

int fd_graph_init(fd_engine* eng, const fd_graph_params* params) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E(eng);
  FD_REQUIRE(params, FD_ERR_INVALID_ARG, "null params");
  FD_HIP(hipStreamSynchronize(e.stream));  // a step in flight may still read the log this replaces
  fd::graph_init(e, *params);
  FD_API_END
}

int fd_graph_clear(fd_engine* eng) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E(eng);
  fd::graph_clear(e);
  FD_API_END
}

int fd_graph_info(fd_engine* eng, int64_t* total, int64_t* held) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E_quiet(eng);
  fd::graph_info(e, total, held);
  FD_API_END
}

int fd_graph_step_device(fd_engine* eng, const fd_txn_batch* txns, int64_t n, double* d_out) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E(eng);
  FD_REQUIRE(txns, FD_ERR_INVALID_ARG, "null txns");
  fd::graph_step(e, *txns, n, d_out);
  FD_API_END
}

int fd_graph_step_host(fd_engine* eng, const fd_txn_batch* txns, int64_t n, double* out) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E(eng);
  FD_REQUIRE(txns, FD_ERR_INVALID_ARG, "null txns");
  FD_REQUIRE(e.graph.ready, FD_ERR_NOT_LOADED, "graph log not initialised (fd_graph_init)");
  FD_REQUIRE(n >= 0 && n < (1ll << 31), FD_ERR_INVALID_ARG, "batch size out of range");
  if (n == 0) return FD_OK;
  FD_REQUIRE(txns->card_key && txns->merchant && txns->amount_cents && out, FD_ERR_INVALID_ARG,
             "null card_key / merchant / amount_cents / output");
  Stage st(e);
  fd_txn_batch d{};
  double* dout;
  stage_txns(st, d, *txns, n, fd::kTxnKey | fd::kTxnCents | fd::kTxnMerchant);
  st.out(dout, out, (size_t)n * FD_GRAPH_FEATURES);
  st.upload();
  fd::graph_step(e, d, n, dout);
  st.download();
  FD_API_END
}

int fd_graph_features_host(const uint64_t* card_key, const int32_t* merchant, const int64_t* amount_cents, int64_t n,
                           int32_t max_history, double* out) {
  FD_API_BEGIN
  FD_REQUIRE(max_history >= fd::kGraphMinHistory && max_history <= fd::kGraphMaxHistory, FD_ERR_INVALID_ARG,
             "graph max_history must be in [2, 65536], got " + std::to_string(max_history));
  FD_REQUIRE(n >= 0, FD_ERR_INVALID_ARG, "negative n");
  if (n == 0) return FD_OK;
  FD_REQUIRE(card_key && merchant && amount_cents && out, FD_ERR_INVALID_ARG,
             "null card_key / merchant / amount_cents / output");
  fd::graph_features_stream_host(card_key, merchant, amount_cents, n, max_history, out);
  FD_API_END
}

int fd_text_features_device(fd_engine* eng, const fd_text_batch* d, int64_t n, double* d_feat, uint8_t* d_patterns,
                            uint8_t* d_status) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E(eng);
  FD_REQUIRE(d, FD_ERR_INVALID_ARG, "null text batch");
  fd::text_features(e, d->bytes, d->off, n, d_feat, d_patterns, d_status);
  FD_API_END
}

int fd_text_features_host(fd_engine* eng, const fd_text_batch* t, int64_t n, double* feat, uint8_t* patterns,
                          uint8_t* status) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E(eng);
  FD_REQUIRE(t, FD_ERR_INVALID_ARG, "null text batch");
  FD_REQUIRE(n >= 0 && n < (1ll << 31), FD_ERR_INVALID_ARG, "batch size out of range");
  if (n == 0) return FD_OK;
  FD_REQUIRE(t->off, FD_ERR_INVALID_ARG, "null text offsets");
  FD_REQUIRE(fd::text_offsets_valid(t->off, n), FD_ERR_INVALID_ARG,
             "text offsets must start at 0 and never decrease");
  const int64_t total = t->off[4 * n];
  FD_REQUIRE(total == 0 || t->bytes, FD_ERR_INVALID_ARG, "null text bytes");
  Stage st(e);
  fd_text_batch d{};
  double* dfeat;
  uint8_t *dpat, *dstatus;
  st.in(d.off, t->off, (size_t)(4 * n + 1));
  st.in(d.bytes, t->bytes, (size_t)total);
  st.out(dfeat, feat, (size_t)n * FD_TEXT_FEATURES);
  st.out(dpat, patterns, (size_t)n);
  st.out(dstatus, status, (size_t)n);
  st.upload();
  fd::text_features(e, d.bytes, d.off, n, dfeat, dpat, dstatus);
  st.download();
  FD_API_END
}

int fd_text_features_ref_host(const uint8_t* bytes, const int64_t* off, int64_t n, double* feat, uint8_t* patterns,
                              uint8_t* status) {
  FD_API_BEGIN
  FD_REQUIRE(n >= 0, FD_ERR_INVALID_ARG, "negative n");
  if (n == 0) return FD_OK;
  FD_REQUIRE(off, FD_ERR_INVALID_ARG, "null text offsets");
  FD_REQUIRE(fd::text_offsets_valid(off, n), FD_ERR_INVALID_ARG, "text offsets must start at 0 and never decrease");
  FD_REQUIRE(off[4 * n] == 0 || bytes, FD_ERR_INVALID_ARG, "null text bytes");
  fd::text_features_rows_host(bytes, off, n, feat, patterns, status);
  FD_API_END
}

int fd_ab_create(fd_engine* eng, int32_t test_id, const fd_ab_params* params) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E(eng);
  FD_REQUIRE(params, FD_ERR_INVALID_ARG, "null A/B params");
  fd::ab_create(e, test_id, *params);
  FD_API_END
}

int fd_ab_destroy(fd_engine* eng, int32_t test_id) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  fd::ab_destroy(E(eng), test_id);
  FD_API_END
}

int fd_ab_clear(fd_engine* eng, int32_t test_id) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  fd::ab_clear(E(eng), test_id);
  FD_API_END
}

int fd_ab_assign_device(fd_engine* eng, int32_t test_id, const uint64_t* d_keys, int64_t n, uint8_t* d_variant) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  fd::ab_assign(E(eng), test_id, d_keys, n, d_variant);
  FD_API_END
}

int fd_ab_assign_host(fd_engine* eng, int32_t test_id, const uint64_t* keys, int64_t n, uint8_t* variant) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E(eng);
  fd::ab_test(e, test_id);
  FD_REQUIRE(n >= 0 && n < (1ll << 31), FD_ERR_INVALID_ARG, "batch size out of range");
  if (n == 0) return FD_OK;
  FD_REQUIRE(keys && variant, FD_ERR_INVALID_ARG, "null keys / variant");
  Stage st(e);
  const uint64_t* dk;
  uint8_t* dv;
  st.in(dk, keys, (size_t)n);
  st.out(dv, variant, (size_t)n);
  st.upload();
  fd::ab_assign(e, test_id, dk, n, dv);
  st.download();
  FD_API_END
}

int fd_ab_partition_device(fd_engine* eng, const uint8_t* d_variant, int64_t n, int32_t* d_idx, int64_t* d_counts) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  fd::ab_partition(E(eng), d_variant, n, d_idx, d_counts);
  FD_API_END
}

int fd_ab_partition_host(fd_engine* eng, const uint8_t* variant, int64_t n, int32_t* idx, int64_t* counts) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E(eng);
  FD_REQUIRE(n >= 0 && n < (1ll << 31) && counts, FD_ERR_INVALID_ARG, "bad batch size / null counts");
  FD_REQUIRE(n == 0 || (variant && idx), FD_ERR_INVALID_ARG, "null variant / index");
  Stage st(e);
  const uint8_t* dv;
  int32_t* di;
  int64_t* dc;
  st.in(dv, variant, (size_t)n);
  st.out(di, idx, (size_t)n);
  st.out(dc, counts, 2);
  st.upload();
  fd::ab_partition(e, dv, n, di, dc);
  st.download();
  FD_API_END
}

int fd_ab_score_matrix_device(fd_engine* eng, int32_t test_id, const fd_ab_model_set* control,
                              const fd_ab_model_set* treatment, const float* d_X, const uint64_t* d_keys, int64_t n,
                              int32_t ld, uint8_t* d_variant, double* d_model_probs, double* d_fraud_prob,
                              double* d_confidence, uint8_t* d_decision, uint8_t* d_risk) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E(eng);
  FD_REQUIRE(control && treatment, FD_ERR_INVALID_ARG, "null model set");
  fd::ab_score_matrix(e, test_id, *control, *treatment, d_X, d_keys, n, ld, d_variant,
                      ScoreOut{d_model_probs, d_fraud_prob, d_confidence, d_decision, d_risk});
  FD_API_END
}

int fd_ab_score_matrix_host(fd_engine* eng, int32_t test_id, const fd_ab_model_set* control,
                            const fd_ab_model_set* treatment, const float* X, const uint64_t* keys, int64_t n,
                            int32_t ld, uint8_t* variant, double* model_probs, double* fraud_prob, double* confidence,
                            uint8_t* decision, uint8_t* risk) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E(eng);
  FD_REQUIRE(control && treatment, FD_ERR_INVALID_ARG, "null model set");
  FD_REQUIRE(n >= 0 && n < (1ll << 31) && ld > 0, FD_ERR_INVALID_ARG, "bad batch size / row stride");
  fd::ab_test(e, test_id);
  if (n == 0) return FD_OK;
  FD_REQUIRE(X && keys && fraud_prob, FD_ERR_INVALID_ARG, "null X / keys / fraud_prob");
  Stage st(e);
  const float* dX;
  const uint64_t* dk;
  const double* dext[2][FD_MAX_MODELS] = {};
  fd_ab_model_set dset[2] = {*control, *treatment};
  int m_max = 0;
  st.in(dX, X, (size_t)n * ld);
  st.in(dk, keys, (size_t)n);
  for (int v = 0; v < 2; ++v) {  // the external columns, n-long in arrival order
    const fd_ab_model_set& s = dset[v];
    FD_REQUIRE(s.params && s.slots, FD_ERR_INVALID_ARG, "null blend params / slots");
    fd::require_model_count(*s.params, "n_models out of range");
    const int M = s.params->n_models;
    m_max = std::max(m_max, M);
    for (int m = 0; m < M; ++m) {
      if (!ModelSet(s).external(m)) continue;
      FD_REQUIRE(s.ext_probs && s.ext_probs[m], FD_ERR_INVALID_ARG,
                 "model without slot needs an external probability column");
      st.in(dext[v][m], s.ext_probs[m], (size_t)n);
    }
    dset[v].ext_probs = dext[v];
  }
  uint8_t* dvar;
  ScoreOut out;
  st.out(dvar, variant, (size_t)n);
  st.out(out.mp, model_probs, (size_t)n * m_max);
  st.out(out.fp, fraud_prob, (size_t)n);
  st.out(out.conf, confidence, (size_t)n);
  st.out(out.dec, decision, (size_t)n);
  st.out(out.risk, risk, (size_t)n);
  st.upload();
  fd::ab_score_matrix(e, test_id, dset[0], dset[1], dX, dk, n, ld, dvar, out);
  st.download();
  FD_API_END
}

int fd_ab_record_device(fd_engine* eng, int32_t test_id, const uint8_t* d_variant, const double* d_prediction,
                        const uint8_t* d_decision, const double* d_processing_time_ms, double time_scalar,
                        const uint8_t* d_actual_fraud, int64_t n) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  fd::ab_record(E(eng), test_id, d_variant, d_prediction, d_decision, d_processing_time_ms, time_scalar,
                d_actual_fraud, n);
  FD_API_END
}

int fd_ab_record_host(fd_engine* eng, int32_t test_id, const uint8_t* variant, const double* prediction,
                      const uint8_t* decision, const double* processing_time_ms, double time_scalar,
                      const uint8_t* actual_fraud, int64_t n) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E(eng);
  fd::ab_test(e, test_id);
  FD_REQUIRE(n >= 0, FD_ERR_INVALID_ARG, "negative n");
  if (n == 0) return FD_OK;
  FD_REQUIRE(variant && prediction && decision, FD_ERR_INVALID_ARG, "null variant / prediction / decision");
  Stage st(e);
  const uint8_t *dv, *dd, *dl;
  const double *dp, *dt;
  st.in(dv, variant, (size_t)n);
  st.in(dp, prediction, (size_t)n);
  st.in(dd, decision, (size_t)n);
  st.in(dt, processing_time_ms, (size_t)n);
  st.in(dl, actual_fraud, (size_t)n);
  st.upload();
  // No wait, as in fd_sink_update_host: fd_ab_state_host is ordered behind the kernel on e.stream. The caller may
  // reuse its columns at once only because a copy from pageable memory has read its source when hipMemcpyAsync
  // returns; columns in pinned memory are read later, and must stay as they are until the stream has passed this call
  // (include/fdengine.h says so).
  fd::ab_record(e, test_id, dv, dp, dd, dt, time_scalar, dl, n);
  FD_API_END
}

int fd_ab_state_host(fd_engine* eng, int32_t test_id, fd_ab_state* out) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  fd::ab_state_read(E(eng), test_id, out);
  FD_API_END
}

int fd_ab_state_merge_host(const fd_ab_state* a, const fd_ab_state* b, fd_ab_state* out) {
  FD_API_BEGIN
  FD_REQUIRE(a && b && out, FD_ERR_INVALID_ARG, "null state");
  fd_ab_state r = *a;
  for (int v = 0; v < 2; ++v) fd::ab_merge(r.variant[v], b->variant[v]);
  *out = r;
  FD_API_END
}

int fd_ab_bucket_host(const uint64_t* keys, int64_t n, uint64_t salt, uint8_t* bucket_out) {
  FD_API_BEGIN
  FD_REQUIRE(n >= 0 && (n == 0 || (keys && bucket_out)), FD_ERR_INVALID_ARG, "bad arguments");
  for (int64_t i = 0; i < n; ++i) bucket_out[i] = (uint8_t)fd::ab_bucket(keys[i], salt);
  FD_API_END
}

int fd_ab_record_ref_host(const uint8_t* variant, const double* prediction, const uint8_t* decision,
                          const double* processing_time_ms, double time_scalar, const uint8_t* actual_fraud, int64_t n,
                          fd_ab_state* state) {
  FD_API_BEGIN
  FD_REQUIRE(n >= 0 && state && (n == 0 || (variant && prediction && decision)), FD_ERR_INVALID_ARG, "bad arguments");
  for (int64_t i = 0; i < n; ++i)
    fd::ab_add_row(state->variant[variant[i] ? 1 : 0], prediction[i], decision[i],
                   processing_time_ms ? processing_time_ms[i] : time_scalar,
                   actual_fraud ? actual_fraud[i] : (uint8_t)FD_AB_NO_LABEL);
  FD_API_END
}

int fd_metrics_init(fd_engine* eng, const fd_metrics_params* params) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E(eng);
  FD_REQUIRE(params, FD_ERR_INVALID_ARG, "null metrics params");
  fd::metrics_init(e, *params);
  FD_API_END
}

int fd_metrics_clear(fd_engine* eng) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  fd::metrics_clear(E(eng));
  FD_API_END
}

int fd_metrics_record_device(fd_engine* eng, const double* d_fraud_prob, const uint8_t* d_decision,
                             const double* d_model_probs, int32_t n_models, const double* d_time_ms,
                             double time_scalar, double timestamp, int64_t n) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  fd::metrics_record(E(eng), d_fraud_prob, d_decision, d_model_probs, n_models, d_time_ms, time_scalar, timestamp, n);
  FD_API_END
}

int fd_metrics_record_host(fd_engine* eng, const double* fraud_prob, const uint8_t* decision,
                           const double* model_probs, int32_t n_models, const double* time_ms, double time_scalar,
                           double timestamp, int64_t n) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E(eng);
  fd::metrics_live(e);
  fd::metrics_check_record(e.metrics.h, fraud_prob, decision, model_probs, n_models, timestamp, n);
  if (n == 0) return FD_OK;
  Stage st(e);
  const double *dp, *dm, *dt;
  const uint8_t* dd;
  st.in(dp, fraud_prob, (size_t)n);
  st.in(dd, decision, (size_t)n);
  st.in(dm, n_models ? model_probs : nullptr, (size_t)n * n_models);
  st.in(dt, time_ms, (size_t)n);
  st.upload();
  // No wait, as in fd_ab_record_host: fd_metrics_query_host is ordered behind the kernel on e.stream; pageable
  // columns have been read when hipMemcpyAsync returns, pinned ones must stay until the stream has passed this call.
  fd::metrics_record(e, dp, dd, dm, n_models, dt, time_scalar, timestamp, n);
  FD_API_END
}

int fd_metrics_query_host(fd_engine* eng, double now, fd_metrics_summary* out) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  fd::metrics_query(E(eng), now, out);
  FD_API_END
}

int64_t fd_metrics_state_bytes(int32_t slots) {
  return slots >= 1 && slots <= 65536 ? (int64_t)fd::metrics_state_bytes(slots) : 0;
}

int fd_metrics_state_init_host(void* state, const fd_metrics_params* params) {
  FD_API_BEGIN
  FD_REQUIRE(state && params, FD_ERR_INVALID_ARG, "null state / params");
  fd::metrics_check_params(*params);
  std::memset(state, 0, fd::metrics_state_bytes(params->slots));
  static_cast<fd::MetricsState*>(state)->h = fd::MetricsHeader{params->slots, params->n_models, 0, 0, 0, 0.0};
  FD_API_END
}

int fd_metrics_record_ref_host(void* state, const double* fraud_prob, const uint8_t* decision,
                               const double* model_probs, int32_t n_models, const double* time_ms, double time_scalar,
                               double timestamp, int64_t n) {
  FD_API_BEGIN
  FD_REQUIRE(state, FD_ERR_INVALID_ARG, "null state");
  fd::MetricsState& s = *static_cast<fd::MetricsState*>(state);
  FD_REQUIRE(s.h.slots > 0, FD_ERR_NOT_LOADED, "metrics state not initialised (fd_metrics_state_init_host)");
  fd::metrics_check_record(s.h, fraud_prob, decision, model_probs, n_models, timestamp, n);
  if (n == 0) return FD_OK;
  bool fresh;
  fd::MetricsSlot& slot = s.ring[fd::metrics_ring_advance(s.h, timestamp, fresh)];
  if (fresh) {
    std::memset(&slot, 0, sizeof(slot));
    slot.ts = timestamp;
    fd::metrics_window_floats_open(slot.w);
  }
  int64_t cnt[fd::kMcCount] = {};
  fd::MetricsPart part;
  fd::metrics_rows_host(fraud_prob, decision, model_probs, n_models, time_ms, time_scalar, n, cnt, part);
  for (int k = 0; k < fd::kMcCount; ++k) {
    if (cnt[k] == 0) continue;
    *fd::metrics_counter_ptr(&s.cum, &slot.w, k) += cnt[k];
    const int sr = fd::metrics_counter_series(k);
    if (sr >= 0) s.cum.series[sr].last_timestamp = timestamp;
  }
  fd::metrics_apply(s.cum, slot.w, part);
  FD_API_END
}

int fd_metrics_query_ref_host(const void* state, double now, fd_metrics_summary* out) {
  FD_API_BEGIN
  FD_REQUIRE(state && out, FD_ERR_INVALID_ARG, "null state / out");
  const fd::MetricsState& s = *static_cast<const fd::MetricsState*>(state);
  FD_REQUIRE(s.h.slots > 0, FD_ERR_NOT_LOADED, "metrics state not initialised (fd_metrics_state_init_host)");
  std::memset(out, 0, sizeof(*out));
  out->total = s.cum;
  for (int g = 0; g <= FD_METRICS_MAX_MODELS; ++g) {
    fd::metrics_window_reduce_group(s.ring, s.h.slots, s.h.head, s.h.used, now, 3600.0, g, out->hour);
    fd::metrics_window_reduce_group(s.ring, s.h.slots, s.h.head, s.h.used, now, 60.0, g, out->minute);
  }
  out->evictions = s.h.evictions;
  out->slots_used = s.h.used;
  out->newest = s.h.used ? s.h.newest : 0.0;
  FD_API_END
}

// b's window into a's: metrics_window_merge_group with the "no rows: min = max = 0" form of a summary
static void metrics_summary_window_merge(fd_metrics_window& a, const fd_metrics_window& b) {
  fd::metrics_window_merge_group(a, b, 0);
  for (int m = 0; m < FD_METRICS_MAX_MODELS; ++m) {
    fd_metrics_window_model& am = a.model[m];
    const fd_metrics_window_model& bm = b.model[m];
    if (bm.rows == 0) continue;
    if (am.rows == 0) {
      am = bm;
      continue;
    }
    fd::metrics_window_merge_group(a, b, 1 + m);
  }
}

int fd_metrics_summary_merge_host(const fd_metrics_summary* a, const fd_metrics_summary* b, fd_metrics_summary* out) {
  FD_API_BEGIN
  FD_REQUIRE(a && b && out, FD_ERR_INVALID_ARG, "null summary");
  fd_metrics_summary r = *a;
  const fd_metrics_summary& o = *b;
  for (int k = 0; k < fd::kMcCumCount; ++k) (&r.total.predictions)[k] += (&o.total.predictions)[k];
  fd::metrics_sum_merge(r.total.score_sum, o.total.score_sum);
  for (int s = 0; s < FD_METRICS_SERIES; ++s) {
    fd_metrics_series& rs = r.total.series[s];
    const fd_metrics_series& os = o.total.series[s];
    if (os.rows == 0) continue;
    rs.last_timestamp = rs.rows == 0 ? os.last_timestamp : fd::metrics_max(rs.last_timestamp, os.last_timestamp);
    for (int k = 0; k < fd::kMcSeriesCount; ++k) (&rs.rows)[k] += (&os.rows)[k];
    fd::metrics_sum_merge(rs.time_ms, os.time_ms);
    fd::metrics_sum_merge(rs.seconds, os.seconds);
  }
  metrics_summary_window_merge(r.hour, o.hour);
  metrics_summary_window_merge(r.minute, o.minute);
  r.evictions += o.evictions;
  r.slots_used += o.slots_used;
  r.newest = a->slots_used == 0 ? o.newest : o.slots_used == 0 ? r.newest : fd::metrics_max(r.newest, o.newest);
  *out = r;
  FD_API_END
}

int fd_features_seq_device(fd_engine* eng, const fd_txn_batch* txns, int64_t n, float* d_vectors, double* d_raw,
                           float* d_seq) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E(eng);
  FD_REQUIRE(txns, FD_ERR_INVALID_ARG, "null txns");
  fd::launch_features(e, *txns, n, d_vectors, d_raw, d_seq);
  FD_API_END
}

int fd_shard_of_host(const uint64_t* keys, int64_t n, int32_t n_shards, int32_t* out) {
  FD_API_BEGIN
  FD_REQUIRE(n >= 0 && (n == 0 || (keys && out)), FD_ERR_INVALID_ARG, "bad arguments");
  FD_REQUIRE(n_shards >= 1 && n_shards <= FD_MAX_SHARDS, FD_ERR_INVALID_ARG, "n_shards must be in [1, 64]");
  for (int64_t i = 0; i < n; ++i) out[i] = (int32_t)fd::shard_of_host(keys[i], (unsigned)n_shards);
  FD_API_END
}

int fd_route_partition_device(fd_engine* eng, const fd_txn_batch* txns, int64_t n, int32_t n_shards,
                              void* d_records, int64_t* d_counts) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E(eng);
  FD_REQUIRE(txns, FD_ERR_INVALID_ARG, "null txns");
  fd::launch_route_partition(e, *txns, nullptr, n, n_shards, d_records, d_counts);
  FD_API_END
}

int fd_route_partition_ex_device(fd_engine* eng, const fd_txn_batch* txns, const fd_window_inputs* extra, int64_t n,
                                 int32_t n_shards, void* d_records, int64_t* d_counts) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E(eng);
  FD_REQUIRE(txns, FD_ERR_INVALID_ARG, "null txns");
  fd::launch_route_partition(e, *txns, extra, n, n_shards, d_records, d_counts);
  FD_API_END
}

int fd_route_partition_stream(fd_engine* eng, const fd_txn_batch* txns, const fd_window_inputs* extra, int64_t n,
                              int32_t n_shards, void* d_records, int64_t* d_counts, void* stream) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E_quiet(eng);  // touches no card state: the pipelined stream stays undisturbed
  FD_REQUIRE(txns, FD_ERR_INVALID_ARG, "null txns");
  fd::launch_route_partition(e, *txns, extra, n, n_shards, d_records, d_counts, static_cast<hipStream_t>(stream),
                             &e.route_blk_stream);
  FD_API_END
}

int fd_route_unpack_device(fd_engine* eng, const void* d_records, const void* d_results, int64_t n,
                           const fd_txn_batch* out, uint8_t* d_payment_method, uint8_t* d_is_fraud,
                           double* d_fraud_score) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E(eng);
  FD_REQUIRE(out, FD_ERR_INVALID_ARG, "null output columns");
  fd::launch_route_unpack(e, d_records, d_results, n, *out, d_payment_method, d_is_fraud, d_fraud_score);
  FD_API_END
}

int fd_score_records_device(fd_engine* eng, const fd_blend_params* params, const int32_t* slots,
                            const uint8_t* present, const void* d_records, int64_t n, void* d_results) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E(eng);
  FD_REQUIRE(params && slots && n >= 0, FD_ERR_INVALID_ARG, "bad arguments");
  const ModelSet ms(params, slots, nullptr, present);
  fd::require_all_in_slots(ms);
  if (n == 0) return FD_OK;
  fd::score_records(e, ms, d_records, n, d_results);
  FD_API_END
}

int fd_route_scatter_results_device(fd_engine* eng, const void* d_results, int64_t n, double* d_fraud_prob,
                                    double* d_confidence, uint8_t* d_decision, uint8_t* d_risk) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E(eng);
  fd::launch_result_scatter(e, d_results, n, ScoreOut{nullptr, d_fraud_prob, d_confidence, d_decision, d_risk});
  FD_API_END
}

int fd_blend_device(fd_engine* eng, const fd_blend_params* params, int64_t n, const double* const* d_probs,
                    const uint8_t* present, double* d_fraud_prob, double* d_confidence, uint8_t* d_decision,
                    uint8_t* d_risk) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E(eng);
  FD_REQUIRE(params, FD_ERR_INVALID_ARG, "null params");
  fd::launch_blend(e, ModelSet(params, nullptr, nullptr, present), n, d_probs,
                   ScoreOut{nullptr, d_fraud_prob, d_confidence, d_decision, d_risk});
  FD_API_END
}

int fd_blend_host(fd_engine* eng, const fd_blend_params* params, int64_t n, const double* const* probs,
                  const uint8_t* present, double* fraud_prob, double* confidence, uint8_t* decision,
                  uint8_t* risk) {
  FD_API_BEGIN
  FD_ENGINE_LOCK(eng);
  Engine& e = E(eng);
  FD_REQUIRE(params && probs && fraud_prob, FD_ERR_INVALID_ARG, "bad arguments");
  FD_REQUIRE(params->n_models >= 0 && params->n_models <= FD_MAX_MODELS, FD_ERR_INVALID_ARG,
             "n_models out of range");
  if (n == 0) return FD_OK;
  const int M = params->n_models;
  Stage st(e);
  const ModelSet ms(params, nullptr, nullptr, present);
  const double* dcols[FD_MAX_MODELS] = {};
  ScoreOut out;
  for (int m = 0; m < M; ++m) {  // (an absent model's column stays null: launch_blend skips it)
    if (!ms.has(m)) continue;
    FD_REQUIRE(probs[m], FD_ERR_INVALID_ARG, "null probability column");
    st.in(dcols[m], probs[m], (size_t)n);
  }
  st.out(out.fp, fraud_prob, (size_t)n);
  st.out(out.conf, confidence, (size_t)n);
  st.out(out.dec, decision, (size_t)n);
  st.out(out.risk, risk, (size_t)n);
  st.upload();
  fd::launch_blend(e, ms, n, dcols, out);
  st.download();
  FD_API_END
}

}  // extern "C"
