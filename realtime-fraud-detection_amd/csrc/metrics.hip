// metrics.hip — the kernels of the prediction metrics (MetricsCollector, ml/monitoring/metrics.py): one streaming pass
// over the columns a scoring call left on the device, and the query that reduces the windows. The per-row rule, the
// accumulators and the ring are metrics_row.h; the numbers are declared in include/fdengine.h.
//
// State (one allocation, MetricsState): the cumulative part, then a ring of time slots, each a timestamp and the
// window accumulators of the rows recorded under it. Which slot a call goes to is decided on the host (the engine
// keeps the ring's header there: metrics_ring_advance), so a record call waits for nothing; a slot that is opened is
// zeroed by a memset ahead of the launch.
//
// Record. Lanes stride over the rows.
//   Integer counters (kMcCount = 208: totals, two histograms, risk levels, nine series of 17, the slot's counts): per
//   workgroup in LDS, one 32-bit LDS atomic add per increment; after the rows the nonzero ones go to the state with
//   64-bit integer global atomic adds. Integer adds are order-free: the counts are exact whatever the schedule. A
//   workgroup that adds rows to a series also stores the call's timestamp as the series' last one (every such store
//   of a call writes the same value).
//   Float sums, min and max (MetricsPart, 70 doubles): in the lane's registers, then ab_record_kernel's scheme: a wave
//   reduces by shuffles, the four waves through LDS in wave order, one partial per workgroup, an agent-scope fence,
//   an integer ticket, and the last workgroup reduces the partials by the same tree and applies the result to the
//   cumulative part and the slot. The grid depends on n alone, so the same calls on the same state give the same
//   bits. No float atomic is used anywhere in this file.
// LDS per workgroup: kMetricsWaves MetricsParts (2240 B), kMcCount counters (832 B), one flag.
//
// Query. One workgroup. Lane (window, group) for the 2 windows x 9 groups (the window's own numbers, one per model)
// walks the ring's used slots oldest to newest and merges those inside the window, in LDS; the workgroup then writes
// one fd_metrics_summary, which is all the host reads back.
#include <algorithm>
#include <cstddef>

#include "fd_internal.h"
#include "metrics_row.h"

namespace fd {
namespace {

static_assert(offsetof(fd_metrics_cumulative, risk_detected) == 8 * (kMcRisk - kMcCum), "cumulative counters in order");
static_assert(offsetof(fd_metrics_cumulative, score_sum) == 8 * kMcCumCount, "cumulative counters are contiguous");
static_assert(offsetof(fd_metrics_series, time_hist) == 8 * 5 && offsetof(fd_metrics_series, time_ms) == 8 * kMcSeriesCount, "");
static_assert(offsetof(fd_metrics_window, time_ms) == 8 * 3 && offsetof(fd_metrics_window_model, time_ms) == 8 * 4, "");
static_assert(sizeof(MetricsPart) == 8 * (6 + 8 * FD_METRICS_MAX_MODELS), "MetricsPart is 70 doubles");

__device__ __forceinline__ fd_metrics_sum metrics_shfl_down(const fd_metrics_sum& s, int d) {
  return fd_metrics_sum{__shfl_down(s.hi, d), __shfl_down(s.lo, d)};
}

// The workgroup's accumulators merged in lane order; the result is thread 0's return value. The merge is
// metrics_part_merge, taken a component at a time so that only one component's partner is live at once.
__device__ __forceinline__ MetricsPart metrics_block_reduce(MetricsPart acc, MetricsPart* s_part) {
#pragma unroll 1
  for (int d = 32; d > 0; d >>= 1) {  // (lanes whose partner is past the wave merge their own value: unused)
    metrics_sum_merge(acc.ms, metrics_shfl_down(acc.ms, d));
    metrics_sum_merge(acc.sec, metrics_shfl_down(acc.sec, d));
    metrics_sum_merge(acc.p, metrics_shfl_down(acc.p, d));
#pragma unroll
    for (int m = 0; m < FD_METRICS_MAX_MODELS; ++m) {
      MetricsModelPart& a = acc.model[m];
      metrics_sum_merge(a.ms, metrics_shfl_down(a.ms, d));
      metrics_sum_merge(a.sec, metrics_shfl_down(a.sec, d));
      metrics_sum_merge(a.pred, metrics_shfl_down(a.pred, d));
      a.min_ms = metrics_min(a.min_ms, __shfl_down(a.min_ms, d));
      a.max_ms = metrics_max(a.max_ms, __shfl_down(a.max_ms, d));
    }
  }
  __syncthreads();  // s_part may still be read from the round before
  if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll 1
    for (int w = 1; w < kMetricsWaves; ++w) metrics_part_merge(acc, s_part[w]);
  }
  return acc;
}

__global__ void __launch_bounds__(kMetricsThreads) metrics_record_kernel(
    const double* __restrict__ fraud_prob, const uint8_t* __restrict__ decision,
    const double* __restrict__ model_probs, int n_models, const double* __restrict__ time_ms, double time_scalar,
    double ts, int fresh, int64_t n, MetricsPart* partials, unsigned* ticket, fd_metrics_cumulative* cum,
    MetricsSlot* slot) {
  __shared__ MetricsPart s_part[kMetricsWaves];
  __shared__ unsigned s_cnt[kMcCount];
  __shared__ int s_last;
  for (int k = threadIdx.x; k < kMcCount; k += kMetricsThreads) s_cnt[k] = 0;
  __syncthreads();
  auto add = [&](int k) { atomicAdd(&s_cnt[k], 1u); };  // k < kMcCount by construction (metrics_count_*)
  MetricsPart acc = metrics_part_empty();
  const int64_t stride = (int64_t)gridDim.x * kMetricsThreads;
#pragma unroll 1
  for (int64_t i = (int64_t)blockIdx.x * kMetricsThreads + threadIdx.x; i < n; i += stride) {
    const double p = fraud_prob[i];
    const double ms = time_ms ? time_ms[i] : time_scalar;
    const double sec = metrics_seconds(ms);
    const uint8_t dec = decision[i];
    const int tb = metrics_time_bucket(sec);
    metrics_count_row(add, p, dec, tb);
    metrics_part_add_row(acc, p, ms, sec);
#pragma unroll
    for (int m = 0; m < FD_METRICS_MAX_MODELS; ++m) {  // (unrolled: acc.model[m] stays in registers)
      if (m >= n_models) break;
      const double q = model_probs[(int64_t)m * n + i];
      if (!metrics_has_model(q)) continue;
      metrics_count_model(add, m, q, dec, tb);
      metrics_part_add_model(acc.model[m], q, ms, sec);
    }
  }
  __syncthreads();
  for (int k = threadIdx.x; k < kMcCount; k += kMetricsThreads) {
    const unsigned v = s_cnt[k];
    if (v == 0) continue;
    atomicAdd(reinterpret_cast<unsigned long long*>(metrics_counter_ptr(cum, &slot->w, k)), (unsigned long long)v);
    const int s = metrics_counter_series(k);
    if (s >= 0) cum->series[s].last_timestamp = ts;
  }
  acc = metrics_block_reduce(acc, s_part);
  if (threadIdx.x == 0) {
    partials[blockIdx.x] = acc;
    __threadfence();  // release at agent scope: the partial's stores are written back and waited for before the ticket
    const unsigned t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s_last = t == gridDim.x - 1;
  }
  __syncthreads();
  if (!s_last) return;
  __threadfence();  // acquire: the loads below see every workgroup's partial
  MetricsPart mine = metrics_part_empty();
  if (threadIdx.x < gridDim.x) mine = partials[threadIdx.x];
  mine = metrics_block_reduce(mine, s_part);
  if (threadIdx.x == 0) {  // the only writer of the state's float fields
    if (fresh) {
      slot->ts = ts;
      metrics_window_floats_open(slot->w);
    }
    metrics_apply(*cum, slot->w, mine);
  }
}

constexpr int kQueryGroups = 1 + FD_METRICS_MAX_MODELS;

__global__ void __launch_bounds__(kMetricsThreads) metrics_query_kernel(const fd_metrics_cumulative* __restrict__ cum,
                                                                        const MetricsSlot* __restrict__ ring,
                                                                        int64_t slots, int64_t head, int64_t used,
                                                                        int64_t evictions, double newest, double now,
                                                                        fd_metrics_summary* out) {
  __shared__ fd_metrics_window s_win[2];  // hour, minute
  constexpr int kCumWords = sizeof(fd_metrics_cumulative) / 8, kWinWords = 2 * sizeof(fd_metrics_window) / 8;
  static_assert(kCumWords <= kMetricsThreads && kWinWords <= kMetricsThreads, "one word per lane");
  const int t = threadIdx.x;
  if (t < kCumWords) reinterpret_cast<uint64_t*>(&out->total)[t] = reinterpret_cast<const uint64_t*>(cum)[t];
  if (t < kWinWords) reinterpret_cast<uint64_t*>(s_win)[t] = 0;
  __syncthreads();
  if (t < 2 * kQueryGroups) {
    const int w = t / kQueryGroups;
    metrics_window_reduce_group(ring, slots, head, used, now, w == 0 ? 3600.0 : 60.0, t - w * kQueryGroups, s_win[w]);
  }
  __syncthreads();
  if (t < kWinWords) reinterpret_cast<uint64_t*>(&out->hour)[t] = reinterpret_cast<const uint64_t*>(s_win)[t];
  if (t == 0) {
    out->evictions = evictions;
    out->slots_used = used;
    out->newest = newest;
  }
}

MetricsState* dev_state(Engine& e) { return e.metrics.state.as<MetricsState>(); }
fd_metrics_cumulative* dev_cum(Engine& e) {
  return reinterpret_cast<fd_metrics_cumulative*>(e.metrics.state.as<char>() + offsetof(MetricsState, cum));
}
MetricsSlot* dev_ring(Engine& e) {
  return reinterpret_cast<MetricsSlot*>(e.metrics.state.as<char>() + offsetof(MetricsState, ring));
}

}  // namespace

static_assert(offsetof(fd_metrics_summary, minute) == offsetof(fd_metrics_summary, hour) + sizeof(fd_metrics_window), "");

size_t metrics_state_bytes(int32_t slots) { return offsetof(MetricsState, ring) + (size_t)slots * sizeof(MetricsSlot); }

void metrics_live(Engine& e) {
  FD_REQUIRE(e.metrics.live, FD_ERR_NOT_LOADED, "metrics collector not initialised (fd_metrics_init)");
}

void metrics_check_params(const fd_metrics_params& p) {
  FD_REQUIRE(p.n_models >= 0 && p.n_models <= FD_METRICS_MAX_MODELS, FD_ERR_INVALID_ARG,
             "metrics n_models outside 0..8");
  FD_REQUIRE(p.slots >= 1 && p.slots <= 65536, FD_ERR_INVALID_ARG, "metrics slots outside 1..65536");
}

void metrics_init(Engine& e, const fd_metrics_params& p) {
  metrics_check_params(p);
  e.metrics.state.ensure(metrics_state_bytes(p.slots));
  e.metrics.partials.ensure(kMetricsGrid * sizeof(MetricsPart) + sizeof(unsigned));
  e.metrics.summary.ensure(sizeof(fd_metrics_summary));
  e.metrics.h = MetricsHeader{p.slots, p.n_models, 0, 0, 0, 0.0};
  e.metrics.live = true;
  metrics_clear(e);
}

void metrics_clear(Engine& e) {
  metrics_live(e);
  MetricsHeader& h = e.metrics.h;
  h.head = h.used = h.evictions = 0;
  h.newest = 0.0;
  FD_HIP(hipMemsetAsync(dev_state(e), 0, metrics_state_bytes(h.slots), e.stream));
}

// the checks every form of a record call makes before anything is queued or staged
void metrics_check_record(const MetricsHeader& h, const void* fraud_prob, const void* decision,
                          const void* model_probs, int32_t n_models, double timestamp, int64_t n) {
  FD_REQUIRE(n >= 0 && n < (1ll << 31), FD_ERR_INVALID_ARG, "batch size out of range");
  FD_REQUIRE(n_models >= 0 && n_models <= h.n_models, FD_ERR_INVALID_ARG,
             "n_models above the collector's (fd_metrics_params.n_models)");
  if (n == 0) return;
  FD_REQUIRE(fraud_prob && decision && (n_models == 0 || model_probs), FD_ERR_INVALID_ARG,
             "null fraud_prob / decision / model_probs");
  FD_REQUIRE(timestamp == timestamp && (h.used == 0 || timestamp >= h.newest), FD_ERR_INVALID_ARG,
             "metrics timestamp is before the newest recorded one (or NaN)");
}

void metrics_record(Engine& e, const double* d_fraud_prob, const uint8_t* d_decision, const double* d_model_probs,
                    int32_t n_models, const double* d_time_ms, double time_scalar, double timestamp, int64_t n) {
  metrics_live(e);
  metrics_check_record(e.metrics.h, d_fraud_prob, d_decision, d_model_probs, n_models, timestamp, n);
  if (n == 0) return;
  bool fresh;
  const int64_t idx = metrics_ring_advance(e.metrics.h, timestamp, fresh);  // (>= 0: checked above)
  MetricsSlot* slot = dev_ring(e) + idx;
  MetricsPart* partials = e.metrics.partials.as<MetricsPart>();
  unsigned* ticket = reinterpret_cast<unsigned*>(partials + kMetricsGrid);
  if (fresh) FD_HIP(hipMemsetAsync(slot, 0, sizeof(MetricsSlot), e.stream));
  FD_HIP(hipMemsetAsync(ticket, 0, sizeof(unsigned), e.stream));
  hipLaunchKernelGGL(metrics_record_kernel, dim3(metrics_grid(n)), dim3(kMetricsThreads), 0, e.stream, d_fraud_prob,
                     d_decision, d_model_probs, (int)n_models, d_time_ms, time_scalar, timestamp, (int)fresh, n,
                     partials, ticket, dev_cum(e), slot);
  FD_HIP(hipGetLastError());
}

void metrics_query(Engine& e, double now, fd_metrics_summary* out) {
  metrics_live(e);
  FD_REQUIRE(out, FD_ERR_INVALID_ARG, "null out");
  const MetricsHeader& h = e.metrics.h;
  fd_metrics_summary* d_out = e.metrics.summary.as<fd_metrics_summary>();
  hipLaunchKernelGGL(metrics_query_kernel, dim3(1), dim3(kMetricsThreads), 0, e.stream, dev_cum(e), dev_ring(e),
                     (int64_t)h.slots, h.head, h.used, h.evictions, h.used ? h.newest : 0.0, now, d_out);
  FD_HIP(hipGetLastError());
  FD_HIP(hipMemcpyAsync(out, d_out, sizeof(fd_metrics_summary), hipMemcpyDeviceToHost, e.stream));
  FD_HIP(hipStreamSynchronize(e.stream));
}

}  // namespace fd
