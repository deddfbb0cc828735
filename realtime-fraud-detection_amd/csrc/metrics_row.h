// metrics_row.h — the per-row rule of the prediction metrics (metrics.hip, and the host forms in engine.hip): the
// classification of a row (score bucket, duration bucket, risk level, a model's three-way distribution, the > 0.5 and
// > 0.8 predicates), the integer counters it increments, the float accumulators it enters, how two accumulators merge,
// the ring of time slots and the reduction of a window. Host and device compile these same functions, so
// fd_metrics_record_ref_host, the kernels' lanes and fd_metrics_summary_merge_host cannot drift apart. The numbers are
// declared in include/fdengine.h (fd_metrics_summary), each beside its line of ml/monitoring/metrics.py.
//
// Every compare is an f64 compare against the literal the reference compares with; the duration is the f64 quotient
// ms / 1000.0, formed before it is compared (0.3 * 10 style products of bounds are never formed: 0.1 * 3 is not 0.3).
// Float sums are unevaluated pairs hi + lo kept by abtest_row.h's error-free addition. No expression here may be
// contracted into an fma or reassociated (the pragmas below; the library is not built with fast-math).
#pragma once

#include <cstdint>
#include <vector>

#include "abtest_row.h"  // ab_pair_add, FD_HD

namespace fd {

constexpr int kMetricsThreads = 256;
constexpr int kMetricsWaves = kMetricsThreads / 64;
constexpr int kMetricsGrid = kMetricsThreads;  // at most one partial per lane of the last workgroup
constexpr int kMetricsRowsPerLane = 4;         // rows a lane takes before the grid reaches kMetricsGrid

// The integer counters of one record call, in the order a workgroup keeps them in LDS. Each range is a run of
// consecutive int64 fields of the public structs (metrics_counter_ptr), which is why those structs begin with them.
constexpr int kMcCum = 0;  // predictions, fraud_detections, declined, score_hist[12], risk_detected[5]
constexpr int kMcScore = kMcCum + 3;
constexpr int kMcRisk = kMcScore + FD_METRICS_SCORE_BUCKETS;
constexpr int kMcCumCount = 3 + FD_METRICS_SCORE_BUCKETS + FD_METRICS_RISK_LEVELS;
constexpr int kMcSeries = kMcCum + kMcCumCount;  // per series: rows, decisions[4], time_hist[12]
constexpr int kMcSeriesCount = 1 + 4 + FD_METRICS_TIME_BUCKETS;
constexpr int kMcWindow = kMcSeries + FD_METRICS_SERIES * kMcSeriesCount;  // rows, fraud, high_risk
constexpr int kMcWModel = kMcWindow + 3;                                   // per model: rows, dist[3]
constexpr int kMcCount = kMcWModel + FD_METRICS_MAX_MODELS * 4;            // 208

struct MetricsSlot {
  double ts;
  fd_metrics_window w;
};
struct MetricsHeader {
  int32_t slots, n_models;  // slots == 0: not initialised
  int64_t head, used, evictions;  // head: the newest slot's index (with used > 0)
  double newest;
};
// The collector in one allocation. On the device the header is unused: the engine keeps it on the host.
struct MetricsState {
  MetricsHeader h;
  fd_metrics_cumulative cum;
  MetricsSlot ring[1];  // h.slots of them
};

static_assert(sizeof(fd_metrics_series) == 8 * kMcSeriesCount + 40, "series: counters first, no padding");
static_assert(sizeof(fd_metrics_window_model) == 80 && sizeof(fd_metrics_window) == 40 + 8 * 80, "window layout");

FD_HD int metrics_score_bucket(double p) {  // the first bound with p <= bound, counted without a branch
  int b = 0;
  b += !(p <= 0.0);
  b += !(p <= 0.1);
  b += !(p <= 0.2);
  b += !(p <= 0.3);
  b += !(p <= 0.4);
  b += !(p <= 0.5);
  b += !(p <= 0.6);
  b += !(p <= 0.7);
  b += !(p <= 0.8);
  b += !(p <= 0.9);
  b += !(p <= 1.0);
  return b;  // 11: +Inf
}

FD_HD double metrics_seconds(double ms) {
#pragma clang fp contract(off)
  return ms / 1000.0;
}

FD_HD int metrics_time_bucket(double sec) {
  int b = 0;
  b += !(sec <= 0.001);
  b += !(sec <= 0.005);
  b += !(sec <= 0.01);
  b += !(sec <= 0.025);
  b += !(sec <= 0.05);
  b += !(sec <= 0.1);
  b += !(sec <= 0.25);
  b += !(sec <= 0.5);
  b += !(sec <= 1.0);
  b += !(sec <= 2.5);
  b += !(sec <= 5.0);
  return b;
}

FD_HD int metrics_risk(double p) {  // enum fd_risk, _get_risk_level :310-321
  return p >= 0.95 ? FD_CRITICAL : p >= 0.8 ? FD_HIGH : p >= 0.6 ? FD_MEDIUM : p >= 0.3 ? FD_LOW : FD_VERY_LOW;
}

FD_HD int metrics_dist(double q) { return q < 0.3 ? 0 : q < 0.7 ? 1 : 2; }  // q is not NaN: NaN is "no such model"

FD_HD bool metrics_has_model(double q) { return q == q; }

// The counters of one row without its models; add(k) increments counter k. tb: the row's duration bucket.
template <class Add>
FD_HD void metrics_count_row(Add&& add, double p, uint8_t decision, int tb) {
  add(kMcCum + 0);
  add(kMcWindow + 0);
  if (p > 0.5) {
    add(kMcCum + 1);
    add(kMcRisk + metrics_risk(p));
    add(kMcWindow + 1);
  }
  if (p > 0.8) add(kMcWindow + 2);
  if (decision == FD_DECLINE) add(kMcCum + 2);
  add(kMcScore + metrics_score_bucket(p));
  add(kMcSeries + 0);
  if (decision < 4) add(kMcSeries + 1 + decision);
  add(kMcSeries + 5 + tb);
}

// ... and of one model the row carries (q: the model's own prediction)
template <class Add>
FD_HD void metrics_count_model(Add&& add, int m, double q, uint8_t decision, int tb) {
  const int s = kMcSeries + (1 + m) * kMcSeriesCount;
  add(s);
  if (decision < 4) add(s + 1 + decision);
  add(s + 5 + tb);
  add(kMcWModel + 4 * m);
  add(kMcWModel + 4 * m + 1 + metrics_dist(q));
}

// where counter k lives: in the cumulative part or in the call's slot
FD_HD int64_t* metrics_counter_ptr(fd_metrics_cumulative* cum, fd_metrics_window* w, int k) {
  if (k < kMcSeries) return &cum->predictions + k;
  if (k < kMcWindow) {
    const int s = (k - kMcSeries) / kMcSeriesCount;
    return &cum->series[s].rows + (k - kMcSeries - s * kMcSeriesCount);
  }
  if (k < kMcWModel) return &w->rows + (k - kMcWindow);
  const int m = (k - kMcWModel) / 4;
  return &w->model[m].rows + (k - kMcWModel - 4 * m);
}
// the series whose `rows` counter k is, or -1 (a call that adds rows to a series stamps its last_timestamp)
FD_HD int metrics_counter_series(int k) {
  if (k < kMcSeries || k >= kMcWindow) return -1;
  const int s = (k - kMcSeries) / kMcSeriesCount;
  return k - kMcSeries - s * kMcSeriesCount == 0 ? s : -1;
}

// ------------------------------------------------------------------------------------------ float accumulators
FD_HD void metrics_sum_add(fd_metrics_sum& s, double x) { ab_pair_add(s.hi, s.lo, x); }

FD_HD void metrics_sum_merge(fd_metrics_sum& a, const fd_metrics_sum& b) {
#pragma clang fp contract(off)
  ab_pair_add(a.hi, a.lo, b.hi);
  a.lo = a.lo + b.lo;
}

FD_HD double metrics_min(double a, double b) { return b < a ? b : a; }
FD_HD double metrics_max(double a, double b) { return b > a ? b : a; }
FD_HD double metrics_inf() { return __builtin_huge_val(); }

// The float part of one record call: what a lane accumulates, a workgroup reduces and the last workgroup applies
struct MetricsModelPart {
  fd_metrics_sum ms, sec, pred;
  double min_ms, max_ms;  // +inf / -inf without rows
};
struct MetricsPart {
  fd_metrics_sum ms, sec, p;
  MetricsModelPart model[FD_METRICS_MAX_MODELS];
};

FD_HD MetricsPart metrics_part_empty() {
  MetricsPart a{};
  for (int m = 0; m < FD_METRICS_MAX_MODELS; ++m) {
    a.model[m].min_ms = metrics_inf();
    a.model[m].max_ms = -metrics_inf();
  }
  return a;
}

FD_HD void metrics_part_add_row(MetricsPart& a, double p, double ms, double sec) {
  metrics_sum_add(a.ms, ms);
  metrics_sum_add(a.sec, sec);
  metrics_sum_add(a.p, p);
}

FD_HD void metrics_part_add_model(MetricsModelPart& a, double q, double ms, double sec) {
  metrics_sum_add(a.ms, ms);
  metrics_sum_add(a.sec, sec);
  metrics_sum_add(a.pred, q);
  a.min_ms = metrics_min(a.min_ms, ms);
  a.max_ms = metrics_max(a.max_ms, ms);
}

FD_HD void metrics_part_merge(MetricsPart& a, const MetricsPart& b) {
  metrics_sum_merge(a.ms, b.ms);
  metrics_sum_merge(a.sec, b.sec);
  metrics_sum_merge(a.p, b.p);
  for (int m = 0; m < FD_METRICS_MAX_MODELS; ++m) {
    metrics_sum_merge(a.model[m].ms, b.model[m].ms);
    metrics_sum_merge(a.model[m].sec, b.model[m].sec);
    metrics_sum_merge(a.model[m].pred, b.model[m].pred);
    a.model[m].min_ms = metrics_min(a.model[m].min_ms, b.model[m].min_ms);
    a.model[m].max_ms = metrics_max(a.model[m].max_ms, b.model[m].max_ms);
  }
}

// an empty window: zero counts and sums, min / max at their identities (a slot as it is opened)
FD_HD void metrics_window_floats_open(fd_metrics_window& w) {
  for (int m = 0; m < FD_METRICS_MAX_MODELS; ++m) {
    w.model[m].min_time_ms = metrics_inf();
    w.model[m].max_time_ms = -metrics_inf();
  }
}

// a call's reduced float part into the cumulative part and the call's slot (the counters went in on their own)
FD_HD void metrics_apply(fd_metrics_cumulative& cum, fd_metrics_window& w, const MetricsPart& part) {
  metrics_sum_merge(cum.score_sum, part.p);
  metrics_sum_merge(cum.series[0].time_ms, part.ms);
  metrics_sum_merge(cum.series[0].seconds, part.sec);
  metrics_sum_merge(w.time_ms, part.ms);
  for (int m = 0; m < FD_METRICS_MAX_MODELS; ++m) {
    const MetricsModelPart& pm = part.model[m];
    metrics_sum_merge(cum.series[1 + m].time_ms, pm.ms);
    metrics_sum_merge(cum.series[1 + m].seconds, pm.sec);
    metrics_sum_merge(w.model[m].time_ms, pm.ms);
    metrics_sum_merge(w.model[m].prediction, pm.pred);
    w.model[m].min_time_ms = metrics_min(w.model[m].min_time_ms, pm.min_ms);
    w.model[m].max_time_ms = metrics_max(w.model[m].max_time_ms, pm.max_ms);
  }
}

// ------------------------------------------------------------------------------------------ windows
// Group g of a window: 0 its own numbers, 1 + m model m's. One lane of the query kernel reduces one group of one
// window over the ring, oldest slot to newest, and so does the host form.
FD_HD void metrics_window_merge_group(fd_metrics_window& a, const fd_metrics_window& b, int g) {
  if (g == 0) {
    a.rows += b.rows;
    a.fraud += b.fraud;
    a.high_risk += b.high_risk;
    metrics_sum_merge(a.time_ms, b.time_ms);
    return;
  }
  fd_metrics_window_model& am = a.model[g - 1];
  const fd_metrics_window_model& bm = b.model[g - 1];
  am.rows += bm.rows;
  for (int k = 0; k < 3; ++k) am.dist[k] += bm.dist[k];
  metrics_sum_merge(am.time_ms, bm.time_ms);
  metrics_sum_merge(am.prediction, bm.prediction);
  am.min_time_ms = metrics_min(am.min_time_ms, bm.min_time_ms);
  am.max_time_ms = metrics_max(am.max_time_ms, bm.max_time_ms);
}

// out's group g = the slots with now - ts <= limit (the reference's predicate, :233 / :247), oldest to newest.
// out's group must be empty (zero; min / max are set here). A model without rows reports min = max = 0.
FD_HD void metrics_window_reduce_group(const MetricsSlot* ring, int64_t slots, int64_t head, int64_t used, double now,
                                       double limit, int g, fd_metrics_window& out) {
#pragma clang fp contract(off)
  if (g > 0) {
    out.model[g - 1].min_time_ms = metrics_inf();
    out.model[g - 1].max_time_ms = -metrics_inf();
  }
  for (int64_t k = 0; k < used; ++k) {
    const MetricsSlot& s = ring[(head + slots - (used - 1) + k) % slots];
    if (now - s.ts <= limit) metrics_window_merge_group(out, s.w, g);
  }
  if (g > 0 && out.model[g - 1].rows == 0) out.model[g - 1].min_time_ms = out.model[g - 1].max_time_ms = 0.0;
}

// ------------------------------------------------------------------------------------------ host only
// The slot a call stamped ts goes to: the newest when ts equals its stamp, else the next one (fresh; the oldest is
// evicted from a full ring). -1: ts is before the newest stamp or not a number (the clock may not run backwards).
inline int64_t metrics_ring_advance(MetricsHeader& h, double ts, bool& fresh) {
  fresh = false;
  if (!(ts == ts)) return -1;
  if (h.used > 0) {
    if (ts < h.newest) return -1;
    if (ts == h.newest) return h.head;
  }
  fresh = true;
  h.head = h.used == 0 ? 0 : (h.head + 1) % h.slots;
  if (h.used == h.slots) h.evictions += 1;
  else h.used += 1;
  h.newest = ts;
  return h.head;
}

inline int metrics_grid(int64_t n) {
  const int64_t per_block = (int64_t)kMetricsThreads * kMetricsRowsPerLane;
  const int64_t g = (n + per_block - 1) / per_block;
  return (int)(g < kMetricsGrid ? g : kMetricsGrid);
}

// kMetricsThreads accumulators reduced as a workgroup reduces its lanes': every wave by the shuffle-down tree (lane l
// takes lane l + d for d = 32 .. 1), then the waves in order. The result is lane[0].
inline void metrics_tree_host(MetricsPart* lane) {
  for (int w = 0; w < kMetricsWaves; ++w)
    for (int d = 32; d > 0; d >>= 1)
      for (int l = 0; l < d; ++l) metrics_part_merge(lane[w * 64 + l], lane[w * 64 + l + d]);
  for (int w = 1; w < kMetricsWaves; ++w) metrics_part_merge(lane[0], lane[w * 64]);
}

// One record call's rows: counters into cnt[kMcCount] (added to), the float part into `out` in the record kernel's
// order: the kernel's grid for n, lanes striding over the rows, the workgroups' partials reduced by one more tree.
inline void metrics_rows_host(const double* fraud_prob, const uint8_t* decision, const double* model_probs,
                              int n_models, const double* time_ms, double time_scalar, int64_t n, int64_t* cnt,
                              MetricsPart& out) {
  const int grid = metrics_grid(n);
  auto add = [cnt](int k) { cnt[k] += 1; };
  std::vector<MetricsPart> partial(kMetricsGrid, metrics_part_empty()), lane(kMetricsThreads);
  const int64_t stride = (int64_t)grid * kMetricsThreads;
  for (int b = 0; b < grid; ++b) {
    for (int t = 0; t < kMetricsThreads; ++t) {
      MetricsPart acc = metrics_part_empty();
      for (int64_t i = (int64_t)b * kMetricsThreads + t; i < n; i += stride) {
        const double p = fraud_prob[i], ms = time_ms ? time_ms[i] : time_scalar, sec = metrics_seconds(ms);
        const int tb = metrics_time_bucket(sec);
        metrics_count_row(add, p, decision[i], tb);
        metrics_part_add_row(acc, p, ms, sec);
        for (int m = 0; m < n_models; ++m) {
          const double q = model_probs[(int64_t)m * n + i];
          if (!metrics_has_model(q)) continue;
          metrics_count_model(add, m, q, decision[i], tb);
          metrics_part_add_model(acc.model[m], q, ms, sec);
        }
      }
      lane[t] = acc;
    }
    metrics_tree_host(lane.data());
    partial[b] = lane[0];
  }
  metrics_tree_host(partial.data());
  out = partial[0];
}
}  // namespace fd
