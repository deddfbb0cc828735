// abtest_row.h — the per-row rule of the A/B tests (abtest.hip, and the host forms in engine.hip): the bucket of a
// user key, the variant of a bucket, the decision classes, one variant's accumulator, how a row enters it and how two
// accumulators merge. Host and device compile these same functions, so fd_ab_record_ref_host, the kernel's lanes and
// fd_ab_state_merge_host cannot drift apart. The numbers are declared in include/fdengine.h (fd_ab_variant_state).
//
// Moments. A float column (prediction, processing_time_ms) is held as its sum and its M2 = sum (x - mean)^2, each as
// an unevaluated pair hi + lo kept by error-free additions (two_sum). M2 merges by Chan's pairwise formula
//   M2 = M2a + M2b + (mean_b - mean_a)^2 * na * nb / (na + nb).
// Why pairs and not a bare (mean, M2): the summary's effect size and improvement are ratios of mean_t - mean_c, which
// cancels; a running mean that rounds once per row drifts by about 0.3 sqrt(n) ulp, against the log n of the
// reference's pairwise np.mean, and the cancellation multiplies that. With the pairs the mean is (hi + lo) / n, within
// an ulp for any order of rows and merges.
// No expression here may be contracted into an fma or reassociated: two_sum relies on it, and the host and the
// device would otherwise round differently (the pragma below; the library is not built with fast-math).
#pragma once

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>  // FD_HD's attributes
#endif

#include <cstdint>

#include "fdengine.h"
#include "key_hash.h"

namespace fd {

FD_HD uint32_t ab_bucket(uint64_t key, uint64_t salt) {
  if (key == 0) key = 1;  // the card table's key normalisation (shard_of)
  return (uint32_t)(fmix64(key ^ salt) % 100u);
}

// threshold: the f64 the host computed as traffic_split * 100 (0.07 * 100 = 7.000000000000001: 8 buckets)
FD_HD uint8_t ab_variant(uint32_t bucket, double threshold) { return (double)bucket < threshold ? 1 : 0; }

// DECLINE and REVIEW flag a transaction, APPROVE and APPROVE_WITH_MONITORING pass it; any other code is neither
FD_HD bool ab_flagged(uint8_t decision) { return decision == FD_DECLINE || decision == FD_REVIEW; }
FD_HD bool ab_passed(uint8_t decision) { return decision == FD_APPROVE || decision == FD_APPROVE_WITH_MONITORING; }

// hi + lo += x, exactly up to the rounding of lo
FD_HD void ab_pair_add(double& hi, double& lo, double x) {
#pragma clang fp contract(off)
  const double s = hi + x;
  const double b = s - hi;
  const double err = (hi - (s - b)) + (x - b);
  hi = s;
  lo = lo + err;
}

FD_HD double ab_mean(const fd_ab_moments& m, int64_t n) {
#pragma clang fp contract(off)
  return (m.sum_hi + m.sum_lo) / (double)n;
}

// b (nb rows) into a (na rows); either may be empty
FD_HD void ab_moments_merge(fd_ab_moments& a, int64_t na, const fd_ab_moments& b, int64_t nb) {
#pragma clang fp contract(off)
  if (nb == 0) return;
  if (na == 0) {
    a = b;
    return;
  }
  const double delta = ab_mean(b, nb) - ab_mean(a, na);
  const double w = ((double)na * (double)nb) / (double)(na + nb);
  ab_pair_add(a.m2_hi, a.m2_lo, b.m2_hi);
  ab_pair_add(a.m2_hi, a.m2_lo, (delta * delta) * w);
  a.m2_lo = a.m2_lo + b.m2_lo;
  ab_pair_add(a.sum_hi, a.sum_lo, b.sum_hi);
  a.sum_lo = a.sum_lo + b.sum_lo;
}

// one value into a (na rows before it): the merge above with b = {x}
FD_HD void ab_moments_add(fd_ab_moments& a, int64_t na, double x) {
#pragma clang fp contract(off)
  if (na > 0) {
    const double delta = x - ab_mean(a, na);
    ab_pair_add(a.m2_hi, a.m2_lo, (delta * delta) * ((double)na / (double)(na + 1)));
  }
  ab_pair_add(a.sum_hi, a.sum_lo, x);
}

// label: 0 not fraud, 1 fraud, FD_AB_NO_LABEL (the reference's None)
FD_HD void ab_add_row(fd_ab_variant_state& s, double prediction, uint8_t decision, double time_ms, uint8_t label) {
  ab_moments_add(s.prediction, s.rows, prediction);
  ab_moments_add(s.time_ms, s.rows, time_ms);
  s.rows += 1;
  for (int d = 0; d < 4; ++d) s.decisions[d] += decision == d;  // (no indexing by the row's value: registers)
  if (label != FD_AB_NO_LABEL) {
    const bool fraud = label != 0, flag = ab_flagged(decision), pass = ab_passed(decision);
    s.labeled += 1;
    s.tp += fraud && flag;
    s.fp += !fraud && flag;
    s.tn += !fraud && pass;
    s.fn += fraud && pass;
  }
}

FD_HD void ab_merge(fd_ab_variant_state& a, const fd_ab_variant_state& b) {
  ab_moments_merge(a.prediction, a.rows, b.prediction, b.rows);
  ab_moments_merge(a.time_ms, a.rows, b.time_ms, b.rows);
  a.rows += b.rows;
  for (int d = 0; d < 4; ++d) a.decisions[d] += b.decisions[d];
  a.labeled += b.labeled;
  a.tp += b.tp;
  a.fp += b.fp;
  a.tn += b.tn;
  a.fn += b.fn;
}

}  // namespace fd
