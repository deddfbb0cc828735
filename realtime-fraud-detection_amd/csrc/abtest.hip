// abtest.hip — the kernels of the A/B tests (ABTestManager, ml/testing/ab_testing.py): assign users to a variant,
// partition a batch by variant for routed scoring, and reduce recorded results per variant. The per-row rule is
// abtest_row.h; the routed scoring itself is ab_score_matrix in score.hip (fd_ab_score_matrix_*), which calls
// score_matrix once per variant.
//
// Partition (stable: control rows in arrival order, then treatment rows in arrival order; no atomic places a row).
// A workgroup of kAbThreads takes kAbThreads consecutive rows, one per lane. Three launches:
//   ab_partition_count_kernel    control rows per workgroup: a wave64 ballot and popcount per wave, the four wave
//                                counts summed through LDS
//   ab_partition_offsets_kernel  one workgroup: exclusive scan of those counts in place, kAbThreads at a time with a
//                                carry; writes the two totals
//   ab_partition_kernel          the ballot again; a control row's place is its workgroup's offset + the control
//                                count of the lower waves (LDS) + that of the lower lanes (ballot & lower-lane mask);
//                                a treatment row i goes to n_control + (i - the control rows before i)
// LDS: kAbWaves ints per workgroup, one writer each, read after a barrier.
//
// Record. Every lane strides over the rows and keeps both variants' accumulators (fd_ab_variant_state, 144 B each) in
// registers; a wave reduces them by shuffles, the workgroup's four waves through LDS in wave order, and each workgroup
// writes one partial. The last workgroup to take a ticket reads the partials, one per lane, reduces them the same way
// (a fixed tree over workgroup order) and merges the result into the test's state. The grid depends on n alone, so
// the same call on the same state gives the same bits. Hand-off: the partial's writer fences (agent scope, which
// writes its stores back and waits for them) before the relaxed ticket add; the last workgroup fences before it
// reads, with per-lane (vector) loads. The ticket is zeroed by a memset ahead of each launch.
#include <algorithm>

#include "abtest_row.h"
#include "fd_internal.h"

namespace fd {
namespace {

constexpr int kAbThreads = 256;
constexpr int kAbWaves = kAbThreads / 64;
constexpr int kAbRecordGrid = kAbThreads;  // at most one partial per lane of the last workgroup
constexpr int kAbRowsPerLane = 4;          // rows a lane takes before the grid reaches kAbRecordGrid

__global__ void __launch_bounds__(kAbThreads) ab_assign_kernel(const uint64_t* __restrict__ keys, int64_t n,
                                                               uint64_t salt, double threshold,
                                                               uint8_t* __restrict__ variant) {
  const int64_t i = (int64_t)blockIdx.x * kAbThreads + threadIdx.x;
  if (i < n) variant[i] = ab_variant(ab_bucket(keys[i], salt), threshold);
}

// control rows of this wave (every lane gets it) and, in `below`, those in the lanes under this one
__device__ __forceinline__ int ab_wave_controls(bool control, int& below) {
  const unsigned long long mask = __ballot(control);
  const unsigned lane = threadIdx.x & 63u;
  below = __popcll(mask & ((1ull << lane) - 1ull));
  return __popcll(mask);
}

__global__ void __launch_bounds__(kAbThreads) ab_partition_count_kernel(const uint8_t* __restrict__ variant, int64_t n,
                                                                        int32_t* __restrict__ blk) {
  __shared__ int s_wave[kAbWaves];
  const int64_t i = (int64_t)blockIdx.x * kAbThreads + threadIdx.x;
  int below;
  const int c = ab_wave_controls(i < n && variant[i] == 0, below);
  if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    int t = 0;
    for (int w = 0; w < kAbWaves; ++w) t += s_wave[w];
    blk[blockIdx.x] = t;
  }
}

__global__ void __launch_bounds__(kAbThreads) ab_partition_offsets_kernel(int32_t* __restrict__ blk, int32_t nblk,
                                                                          int64_t n, int64_t* __restrict__ counts) {
  __shared__ int s_wave[kAbWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int carry = 0;
  for (int base = 0; base < nblk; base += kAbThreads) {
    const int k = base + tid;
    const int x = k < nblk ? blk[k] : 0;
    int incl = x;  // inclusive scan inside the wave
    for (int d = 1; d < 64; d <<= 1) {
      const int up = __shfl_up(incl, d);
      if (lane >= d) incl += up;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    int before = 0, total = 0;
    for (int w = 0; w < kAbWaves; ++w) {
      const int t = s_wave[w];
      if (w < wave) before += t;
      total += t;
    }
    if (k < nblk) blk[k] = carry + before + incl - x;
    carry += total;
    __syncthreads();  // s_wave is rewritten by the next round
  }
  if (tid == 0) {
    counts[0] = carry;
    counts[1] = n - carry;
  }
}

__global__ void __launch_bounds__(kAbThreads) ab_partition_kernel(const uint8_t* __restrict__ variant, int64_t n,
                                                                  const int32_t* __restrict__ blk,
                                                                  const int64_t* __restrict__ counts,
                                                                  int32_t* __restrict__ idx) {
  __shared__ int s_wave[kAbWaves];
  const int64_t i = (int64_t)blockIdx.x * kAbThreads + threadIdx.x;
  const bool valid = i < n;
  const bool control = valid && variant[i] == 0;
  int below;
  const int c = ab_wave_controls(control, below);
  if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = c;
  __syncthreads();
  if (!valid) return;
  int64_t before = (int64_t)blk[blockIdx.x] + below;  // control rows ahead of row i
  for (int w = 0; w < (int)(threadIdx.x >> 6); ++w) before += s_wave[w];
  const int64_t pos = control ? before : counts[0] + (i - before);  // < n: before <= i, and i - before < n_treatment
  idx[pos] = (int32_t)i;
}

// Xp[j, :] = X[idx[j], :], V floats at a time (V = 4 needs ld % 4 == 0 and 16-byte aligned bases)
template <int V>
__global__ void __launch_bounds__(kAbThreads) ab_gather_rows_kernel(const float* __restrict__ X,
                                                                    const int32_t* __restrict__ idx, int64_t n,
                                                                    int32_t ld, float* __restrict__ Xp) {
  const int64_t per_row = ld / V;
  const int64_t g = (int64_t)blockIdx.x * kAbThreads + threadIdx.x;
  if (g >= n * per_row) return;
  const int64_t j = g / per_row, c = (g - j * per_row) * V;
  const float* src = X + (int64_t)idx[j] * ld + c;
  float* dst = Xp + j * ld + c;
  if constexpr (V == 4) *reinterpret_cast<float4*>(dst) = *reinterpret_cast<const float4*>(src);
  else *dst = *src;
}

// an external probability column into partition order: out[j] = col[idx[j]]
__global__ void __launch_bounds__(kAbThreads) ab_gather_column_kernel(const double* __restrict__ col,
                                                                      const int32_t* __restrict__ idx, int64_t count,
                                                                      double* __restrict__ out) {
  const int64_t j = (int64_t)blockIdx.x * kAbThreads + threadIdx.x;
  if (j < count) out[j] = col[idx[j]];
}

__global__ void __launch_bounds__(kAbThreads) ab_scatter_results_kernel(AbScatter a) {
  const int64_t j = (int64_t)blockIdx.x * kAbThreads + threadIdx.x;
  if (j >= a.n) return;
  const int64_t i = a.idx[j];
  if (a.fp) a.fp[i] = a.p_fp[j];
  if (a.conf) a.conf[i] = a.p_conf[j];
  if (a.dec) a.dec[i] = a.p_dec[j];
  if (a.risk) a.risk[i] = a.p_risk[j];
  if (a.mp) {
    const int v = j >= a.count[0];
    const int64_t jj = v ? j - a.count[0] : j;
    for (int m = 0; m < a.m_max; ++m)
      a.mp[(int64_t)m * a.n + i] = m < a.models[v] ? a.p_mp[v][(int64_t)m * a.count[v] + jj] : __longlong_as_double(0x7ff8000000000000ll);
  }
}

// ---------------------------------------------------------------------------------------------------------- record

__device__ __forceinline__ fd_ab_moments ab_shfl_down(const fd_ab_moments& m, int d) {
  return fd_ab_moments{__shfl_down(m.sum_hi, d), __shfl_down(m.sum_lo, d), __shfl_down(m.m2_hi, d),
                       __shfl_down(m.m2_lo, d)};
}

__device__ __forceinline__ fd_ab_variant_state ab_shfl_down(const fd_ab_variant_state& s, int d) {
  fd_ab_variant_state r;
  r.rows = __shfl_down((long long)s.rows, d);
#pragma unroll
  for (int k = 0; k < 4; ++k) r.decisions[k] = __shfl_down((long long)s.decisions[k], d);
  r.labeled = __shfl_down((long long)s.labeled, d);
  r.tp = __shfl_down((long long)s.tp, d);
  r.fp = __shfl_down((long long)s.fp, d);
  r.tn = __shfl_down((long long)s.tn, d);
  r.fn = __shfl_down((long long)s.fn, d);
  r.prediction = ab_shfl_down(s.prediction, d);
  r.time_ms = ab_shfl_down(s.time_ms, d);
  return r;
}

// The workgroup's accumulators merged in lane order; the result is thread 0's return value. s_part: kAbWaves states.
__device__ __forceinline__ fd_ab_state ab_block_reduce(fd_ab_state acc, fd_ab_state* s_part) {
#pragma unroll 1
  for (int d = 32; d > 0; d >>= 1)
#pragma unroll
    for (int v = 0; v < 2; ++v) {
      const fd_ab_variant_state other = ab_shfl_down(acc.variant[v], d);
      ab_merge(acc.variant[v], other);  // (lanes whose partner is past the wave merge their own value: unused)
    }
  __syncthreads();  // s_part may still be read from the round before
  if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0)
    for (int w = 1; w < kAbWaves; ++w) {
      ab_merge(acc.variant[0], s_part[w].variant[0]);
      ab_merge(acc.variant[1], s_part[w].variant[1]);
    }
  return acc;
}

__global__ void __launch_bounds__(kAbThreads) ab_record_kernel(const uint8_t* __restrict__ variant,
                                                               const double* __restrict__ prediction,
                                                               const uint8_t* __restrict__ decision,
                                                               const double* __restrict__ time_ms, double time_scalar,
                                                               const uint8_t* __restrict__ label, int64_t n,
                                                               fd_ab_state* partials, unsigned* ticket,
                                                               fd_ab_state* state) {
  __shared__ fd_ab_state s_part[kAbWaves];
  __shared__ int s_last;
  fd_ab_state acc{};
  const int64_t stride = (int64_t)gridDim.x * kAbThreads;
  for (int64_t i = (int64_t)blockIdx.x * kAbThreads + threadIdx.x; i < n; i += stride) {
    const double t = time_ms ? time_ms[i] : time_scalar;
    const uint8_t lab = label ? label[i] : (uint8_t)FD_AB_NO_LABEL;
    if (variant[i]) ab_add_row(acc.variant[1], prediction[i], decision[i], t, lab);
    else ab_add_row(acc.variant[0], prediction[i], decision[i], t, lab);
  }
  acc = ab_block_reduce(acc, s_part);
  if (threadIdx.x == 0) {
    partials[blockIdx.x] = acc;
    __threadfence();  // release at agent scope: the partial's stores are written back and waited for before the ticket
    const unsigned t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s_last = t == gridDim.x - 1;
  }
  __syncthreads();
  if (!s_last) return;
  __threadfence();  // acquire: the loads below see every workgroup's partial
  fd_ab_state mine{};
  if (threadIdx.x < gridDim.x) mine = partials[threadIdx.x];
  mine = ab_block_reduce(mine, s_part);
  if (threadIdx.x == 0) {
    fd_ab_state s = *state;
    ab_merge(s.variant[0], mine.variant[0]);
    ab_merge(s.variant[1], mine.variant[1]);
    *state = s;
  }
}

fd_ab_state* state_of(Engine& e, int id) { return e.ab.state.as<fd_ab_state>() + id; }

struct AbTimed {  // one FD_TIMING_ABTEST entry around a step
  Engine& e;
  Engine::Timed* ev;
  explicit AbTimed(Engine& en) : e(en), ev(en.timing ? en.next_event_pair(FD_TIMING_ABTEST) : nullptr) {
    if (ev) FD_HIP(hipEventRecord(ev->a, e.stream));
  }
  void done() {
    FD_HIP(hipGetLastError());
    if (ev) FD_HIP(hipEventRecord(ev->b, e.stream));
  }
};

unsigned blocks_for(int64_t work) { return (unsigned)((work + kAbThreads - 1) / kAbThreads); }

}  // namespace

const AbTest& ab_test(Engine& e, int id) {
  FD_REQUIRE(id >= 0 && id < FD_AB_MAX_TESTS, FD_ERR_INVALID_ARG, "A/B test id out of range");
  FD_REQUIRE(e.ab.tests[id].live, FD_ERR_NOT_LOADED, "A/B test " + std::to_string(id) + " not created");
  return e.ab.tests[id];
}

void ab_create(Engine& e, int id, const fd_ab_params& p) {
  FD_REQUIRE(id >= 0 && id < FD_AB_MAX_TESTS, FD_ERR_INVALID_ARG, "A/B test id out of range");
  FD_REQUIRE(!e.ab.tests[id].live, FD_ERR_INVALID_ARG, "A/B test " + std::to_string(id) + " already exists");
  FD_REQUIRE(p.threshold >= 0.0 && p.threshold <= 100.0, FD_ERR_INVALID_ARG, "A/B threshold outside [0, 100]");
  e.ab.state.ensure(FD_AB_MAX_TESTS * sizeof(fd_ab_state));
  e.ab.partials.ensure(kAbRecordGrid * sizeof(fd_ab_state) + sizeof(unsigned));
  e.ab.tests[id] = AbTest{true, p.salt, p.threshold};
  ab_clear(e, id);
}

void ab_destroy(Engine& e, int id) {
  ab_test(e, id);
  e.ab.tests[id].live = false;
}

void ab_clear(Engine& e, int id) {
  ab_test(e, id);
  FD_HIP(hipMemsetAsync(state_of(e, id), 0, sizeof(fd_ab_state), e.stream));
}

void ab_assign(Engine& e, int id, const uint64_t* d_keys, int64_t n, uint8_t* d_variant) {
  const AbTest& t = ab_test(e, id);
  FD_REQUIRE(n >= 0 && n < (1ll << 31), FD_ERR_INVALID_ARG, "batch size out of range");
  if (n == 0) return;
  FD_REQUIRE(d_keys && d_variant, FD_ERR_INVALID_ARG, "null keys / variant");
  AbTimed tm(e);
  hipLaunchKernelGGL(ab_assign_kernel, dim3(blocks_for(n)), dim3(kAbThreads), 0, e.stream, d_keys, n, t.salt,
                     t.threshold, d_variant);
  tm.done();
}

void ab_partition(Engine& e, const uint8_t* d_variant, int64_t n, int32_t* d_idx, int64_t* d_counts) {
  FD_REQUIRE(n >= 0 && n < (1ll << 31), FD_ERR_INVALID_ARG, "batch size out of range");
  FD_REQUIRE(d_counts, FD_ERR_INVALID_ARG, "null counts");
  if (n == 0) {
    FD_HIP(hipMemsetAsync(d_counts, 0, 2 * sizeof(int64_t), e.stream));
    return;
  }
  FD_REQUIRE(d_variant && d_idx, FD_ERR_INVALID_ARG, "null variant / index");
  const unsigned nblk = blocks_for(n);
  e.ab.part.ensure((size_t)nblk * sizeof(int32_t));
  int32_t* blk = e.ab.part.as<int32_t>();
  AbTimed tm(e);
  hipLaunchKernelGGL(ab_partition_count_kernel, dim3(nblk), dim3(kAbThreads), 0, e.stream, d_variant, n, blk);
  hipLaunchKernelGGL(ab_partition_offsets_kernel, dim3(1), dim3(kAbThreads), 0, e.stream, blk, (int32_t)nblk, n,
                     d_counts);
  hipLaunchKernelGGL(ab_partition_kernel, dim3(nblk), dim3(kAbThreads), 0, e.stream, d_variant, n, blk, d_counts,
                     d_idx);
  tm.done();
}

void ab_gather_rows(Engine& e, const float* d_X, const int32_t* d_idx, int64_t n, int32_t ld, float* d_Xp) {
  if (n == 0) return;
  AbTimed tm(e);
  const bool vec = ld % 4 == 0 && ((uintptr_t)d_X | (uintptr_t)d_Xp) % 16 == 0;
  if (vec)
    hipLaunchKernelGGL(ab_gather_rows_kernel<4>, dim3(blocks_for(n * (ld / 4))), dim3(kAbThreads), 0, e.stream, d_X,
                       d_idx, n, ld, d_Xp);
  else
    hipLaunchKernelGGL(ab_gather_rows_kernel<1>, dim3(blocks_for(n * ld)), dim3(kAbThreads), 0, e.stream, d_X, d_idx,
                       n, ld, d_Xp);
  tm.done();
}

void ab_gather_column(Engine& e, const double* d_col, const int32_t* d_idx, int64_t count, double* d_out) {
  if (count == 0) return;
  AbTimed tm(e);
  hipLaunchKernelGGL(ab_gather_column_kernel, dim3(blocks_for(count)), dim3(kAbThreads), 0, e.stream, d_col, d_idx,
                     count, d_out);
  tm.done();
}

void ab_scatter_results(Engine& e, const AbScatter& a) {
  if (a.n == 0) return;
  AbTimed tm(e);
  hipLaunchKernelGGL(ab_scatter_results_kernel, dim3(blocks_for(a.n)), dim3(kAbThreads), 0, e.stream, a);
  tm.done();
}

void ab_record(Engine& e, int id, const uint8_t* d_variant, const double* d_prediction, const uint8_t* d_decision,
               const double* d_time_ms, double time_scalar, const uint8_t* d_label, int64_t n) {
  ab_test(e, id);
  FD_REQUIRE(n >= 0, FD_ERR_INVALID_ARG, "negative n");
  if (n == 0) return;
  FD_REQUIRE(d_variant && d_prediction && d_decision, FD_ERR_INVALID_ARG, "null variant / prediction / decision");
  const int64_t per_block = (int64_t)kAbThreads * kAbRowsPerLane;
  const unsigned grid = (unsigned)std::min<int64_t>(kAbRecordGrid, (n + per_block - 1) / per_block);
  fd_ab_state* partials = e.ab.partials.as<fd_ab_state>();
  unsigned* ticket = reinterpret_cast<unsigned*>(partials + kAbRecordGrid);
  AbTimed tm(e);
  FD_HIP(hipMemsetAsync(ticket, 0, sizeof(unsigned), e.stream));
  hipLaunchKernelGGL(ab_record_kernel, dim3(grid), dim3(kAbThreads), 0, e.stream, d_variant, d_prediction, d_decision,
                     d_time_ms, time_scalar, d_label, n, partials, ticket, state_of(e, id));
  tm.done();
}

void ab_state_read(Engine& e, int id, fd_ab_state* out) {
  ab_test(e, id);
  FD_REQUIRE(out, FD_ERR_INVALID_ARG, "null out");
  FD_HIP(hipMemcpyAsync(out, state_of(e, id), sizeof(fd_ab_state), hipMemcpyDeviceToHost, e.stream));
  FD_HIP(hipStreamSynchronize(e.stream));
}

}  // namespace fd
