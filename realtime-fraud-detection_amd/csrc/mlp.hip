// mlp.hip — the PyTorch member of the ensemble (graph_neural, model_type "pytorch") on the CDNA4 matrix cores.
//
// Reference: ModelManager._create_pytorch_model_architecture / _load_pytorch_model / _predict_pytorch
// (ml/models/model_manager.py:202-242, 168-179, 321-330): num_layers nn.Linear layers of width hidden_channels over
// the 64-wide scoring vector (defaults 64 -> 64 -> 64 -> 2), ReLU after every layer but the last, dropout the identity
// in eval(), softmax(dim=1)[:, 1]. Everything is f32, the reference's dtype.
//
// Kernel: each wave takes 16-row tiles and carries them through every layer on v_mfma_f32_16x16x4_f32 (exact f32 fma
// chains, no bf16) with no exchange between waves. It computes H^T = W X^T: the weights are the A operand (16 output
// units per tile), the rows' activations the B operand (k on the lane group, the row on lane & 15). With the C/D
// layout (col = lane & 15 = row of the batch, row = 4 (lane >> 4) + reg = output unit) lane group g, register r of
// output block b holds hidden unit 16 b + 4 g + r of its batch row — which is exactly a B operand of the next layer
// when k-step (b, r) sums over the units {16 b + 4 g + r : g = 0..3}. The host packs every weight matrix in that k
// order (pack_mlp_host), so a layer's D registers feed the next layer's MFMAs directly: no LDS transpose between
// layers, no barrier after the preload. The input rows are loaded in the same order (lane (g, row) takes the float4
// at columns 16 b + 4 g), so layer 0 needs no other packing.
// Weights stay resident while a workgroup's four waves loop over tiles (persistent grid). Zero padding to multiples
// of 16 is exact (a padded unit is relu(0 + 0) = 0 and meets zero weights downstream).
//   mlp_ref_kernel  the reference shape's form (3 layers, every padded width 64): each lane holds its A operands of
//                   all three layers and the bias blocks in registers (36 + 9 float4, loaded from the packed blob
//                   with coalesced 16-B loads, all in flight at once; the blob is 36.6 KB and stays in L2); no LDS,
//                   no barrier; one wave per SIMD, the next tile's rows in flight behind the MFMAs.
//   mlp_lds_kernel  every other shape (up to 8 layers of 64: 129 KB packed): the blob is staged once per workgroup
//                   into LDS; a lane reads the A operands of four k-steps with one ds_read_b128; the layer count and
//                   the block counts come from the blob's header.
// Per 16-row tile of the reference shape: 64 + 64 + 16 = 144 MFMAs = 4608 matrix-pipe cycles per wave.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "fd_internal.h"

namespace fd {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kMlpHeader = 32;          // header words of the packed blob (pack_mlp_host)
constexpr uint32_t kMlpMagic = 0x31504c4du;  // "MLP1"
constexpr int kRows = 16;               // batch rows per tile (the MFMA's 16 columns)
constexpr int kWaves = 4;               // waves per workgroup, a tile each

__host__ __device__ constexpr int blocks16(int d) { return (d + 15) >> 4; }

// torch.relu: max(v, 0) that keeps a NaN (v_max_f32 / fmaxf would return 0 for it)
__device__ __forceinline__ float relu_nan(float v) { return v < 0.f ? 0.f : v; }

// The tile's rows in the B-operand order: lane (g = lane >> 4, c = lane & 15) takes columns 16 b + 4 g .. + 3 of row
// 16 tile + c. vec: 16-B loads (ld, in_dim multiples of 4, X 16-B aligned); rows >= n and columns >= in_dim are
// never read (ld may exceed in_dim: what lies there is not the model's input).
template <bool HOT>
__device__ __forceinline__ void load_rows(const float* __restrict__ X, int64_t n, int ld, int in_dim, int kb0,
                                          bool vec, int64_t tile, int g, int c, f32x4 (&x)[4]) {
  const int64_t row = tile * kRows + c;
  const float* p = X + row * (int64_t)ld;
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    x[b] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (!HOT && b >= kb0) continue;
    const int col = 16 * b + 4 * g;
    if (row >= n) continue;
    if (vec) {
      if (col < in_dim) x[b] = *reinterpret_cast<const f32x4*>(p + col);
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (col + r < in_dim) x[b][r] = p[col + r];
    }
  }
}

// softmax([z0, z1])[1], the row maximum subtracted, as the f64 of the f32 value
__device__ __forceinline__ double softmax1(float z0, float z1) {
  const float m = fmaxf(z0, z1);
  const float e0 = expf(z0 - m), e1 = expf(z1 - m);
  return (double)(e1 / (e0 + e1));
}

__global__ void __launch_bounds__(64 * kWaves) mlp_ref_kernel(const float* __restrict__ X, int64_t n, int ld,
                                                              const uint32_t* __restrict__ blob, int vec,
                                                              double* __restrict__ prob) {
#pragma clang fp contract(off)
  const int tid = threadIdx.x;
  const int* hd = reinterpret_cast<const int*>(blob);  // uniform reads of the header (scalar loads)
  const int in_dim = hd[2];
  const int w = tid >> 6, l = tid & 63, g = l >> 4, c = l & 15;
  const int64_t ntiles = (n + kRows - 1) / kRows;
  const int64_t stride = (int64_t)gridDim.x * kWaves;
  int64_t tile = (int64_t)blockIdx.x * kWaves + w;
  if (tile >= ntiles) return;  // (whole waves: no barrier below)
  f32x4 xn[4];
  load_rows<true>(X, n, ld, in_dim, 4, vec != 0, tile, g, c, xn);
  // this lane's A operands [layer][out block t][k block b] and bias blocks, for the whole kernel (offsets are
  // multiples of 4 words: pack_mlp_host)
  const f32x4* gw = reinterpret_cast<const f32x4*>(blob);
  f32x4 wa[2][4][4], ba[2][4], wz[4];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const f32x4* wp = gw + hd[11 + i] / 4;
    const f32x4* bp = gw + hd[19 + i] / 4;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
#pragma unroll
      for (int b = 0; b < 4; ++b) wa[i][t][b] = wp[(t * 4 + b) * 64 + l];
      ba[i][t] = bp[4 * t + g];
    }
  }
#pragma unroll
  for (int b = 0; b < 4; ++b) wz[b] = gw[hd[13] / 4 + b * 64 + l];
  const f32x4 bz = gw[hd[21] / 4 + g];
  for (; tile < ntiles; tile += stride) {
    f32x4 h[4] = {xn[0], xn[1], xn[2], xn[3]};
    if (tile + stride < ntiles)  // the next tile's rows, in flight behind this tile's MFMAs
      load_rows<true>(X, n, ld, in_dim, 4, vec != 0, tile + stride, g, c, xn);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      f32x4 acc[4] = {ba[i][0], ba[i][1], ba[i][2], ba[i][3]};
#pragma unroll
      for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int t = 0; t < 4; ++t)  // four independent accumulators back to back
            acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[i][t][b][r], h[b][r], acc[t], 0, 0, 0);
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) h[t][r] = relu_nan(acc[t][r]);
    }
    // the output layer: one block of 16 padded units, the two logits in lane group 0's registers 0 and 1; two
    // accumulators (k blocks 0, 1 and 2, 3) so the 16 dependent k-steps do not wait on each other's latency
    f32x4 z0 = bz, z1 = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        z0 = __builtin_amdgcn_mfma_f32_16x16x4f32(wz[b][r], h[b][r], z0, 0, 0, 0);
        z1 = __builtin_amdgcn_mfma_f32_16x16x4f32(wz[b + 2][r], h[b + 2][r], z1, 0, 0, 0);
      }
    const int64_t row = tile * kRows + c;
    if (g == 0 && row < n) prob[row] = softmax1(z0[0] + z1[0], z0[1] + z1[1]);
  }
}

// one layer from LDS: acc[t] = bias block t + sum over k-steps (b, r) of W-operand x h[b][r], for t < ot, b < kb
__device__ __forceinline__ void layer_lds(const float* __restrict__ wp, const float* __restrict__ bp, int kb, int ot,
                                          int l, const f32x4 (&h)[4], f32x4 (&acc)[4]) {
  const int g = l >> 4;
#pragma unroll
  for (int t = 0; t < 4; ++t)
    acc[t] = t < ot ? *reinterpret_cast<const f32x4*>(bp + 16 * t + 4 * g) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    if (b >= kb) break;
    f32x4 a[4];
#pragma unroll
    for (int t = 0; t < 4; ++t)
      if (t < ot) a[t] = *reinterpret_cast<const f32x4*>(wp + ((t * kb + b) * 64 + l) * 4);
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int t = 0; t < 4; ++t)
        if (t < ot) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t][r], h[b][r], acc[t], 0, 0, 0);
  }
}

__global__ void __launch_bounds__(64 * kWaves) mlp_lds_kernel(const float* __restrict__ X, int64_t n, int ld,
                                                              const uint32_t* __restrict__ blob, int vec,
                                                              double* __restrict__ prob) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int tid = threadIdx.x;
  const int* hd = reinterpret_cast<const int*>(blob);  // uniform reads of the header (scalar loads)
  const int nvec = hd[27] / 4;
  const int L = hd[1];
  const int in_dim = hd[2];
  const int kb0 = blocks16(in_dim);
  const int w = tid >> 6, l = tid & 63, g = l >> 4, c = l & 15;
  const int64_t ntiles = (n + kRows - 1) / kRows;
  const int64_t stride = (int64_t)gridDim.x * kWaves;
  int64_t tile = (int64_t)blockIdx.x * kWaves + w;
  f32x4 xn[4];
  load_rows<false>(X, n, ld, in_dim, kb0, vec != 0, tile, g, c, xn);  // (a tile >= ntiles reads nothing: rows >= n)
  // the packed model -> LDS, eight 16-B loads per thread in flight
  for (int base = 0; base < nvec; base += 8 * 64 * kWaves) {
    f32x4 v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int idx = base + j * 64 * kWaves + tid;
      v[j] = idx < nvec ? reinterpret_cast<const f32x4*>(blob)[idx] : f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int idx = base + j * 64 * kWaves + tid;
      if (idx < nvec) reinterpret_cast<f32x4*>(sm)[idx] = v[j];
    }
  }
  __syncthreads();
  for (; tile < ntiles; tile += stride) {
    f32x4 h[4] = {xn[0], xn[1], xn[2], xn[3]};
    if (tile + stride < ntiles)  // the next tile's rows, in flight behind this tile's MFMAs
      load_rows<false>(X, n, ld, in_dim, kb0, vec != 0, tile + stride, g, c, xn);
    f32x4 acc[4];
    for (int i = 0; i + 1 < L; ++i) {
      layer_lds(sm + hd[11 + i], sm + hd[19 + i], blocks16(hd[2 + i]), blocks16(hd[3 + i]), l, h, acc);
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) h[t][r] = relu_nan(acc[t][r]);
    }
    // the output layer: one block of 16 padded units, the two logits in lane group 0's registers 0 and 1
    layer_lds(sm + hd[11 + L - 1], sm + hd[19 + L - 1], blocks16(hd[2 + L - 1]), 1, l, h, acc);
    const int64_t row = tile * kRows + c;
    if (g == 0 && row < n) prob[row] = softmax1(acc[0][0], acc[0][1]);
  }
}

}  // namespace

// Validates and packs: header (kMlpHeader words: magic, n_layers, dims[9], weight offsets[8], bias offsets[8], total
// words), then per layer its A operands [out block t][k block b][lane][r] = W[16 t + (lane & 15)][16 b + 4 (lane >> 4)
// + r] (zero beyond the layer's shape) and its bias padded to the block.
std::vector<uint32_t> pack_mlp_host(const fd_mlp_params& p) {
  FD_REQUIRE(p.n_layers >= 2 && p.n_layers <= 8, FD_ERR_UNSUPPORTED,
             "MLP n_layers must be in [2, 8], got " + std::to_string(p.n_layers));
  const int L = p.n_layers;
  for (int i = L + 1; i < 9; ++i)
    FD_REQUIRE(p.dims[i] == 0, FD_ERR_INVALID_ARG,
               "MLP dims inconsistent with n_layers: dims[" + std::to_string(i) + "] set beyond layer " +
                   std::to_string(L - 1));
  FD_REQUIRE(p.dims[0] >= 1 && p.dims[0] <= 64, FD_ERR_UNSUPPORTED,
             "MLP in_dim must be in [1, 64], got " + std::to_string(p.dims[0]));
  for (int i = 1; i < L; ++i)
    FD_REQUIRE(p.dims[i] >= 1 && p.dims[i] <= 64, FD_ERR_UNSUPPORTED,
               "MLP hidden width must be in [1, 64], got " + std::to_string(p.dims[i]) + " (layer " +
                   std::to_string(i - 1) + ")");
  FD_REQUIRE(p.dims[L] == 2, FD_ERR_UNSUPPORTED,
             "MLP output layer must have exactly 2 outputs, got " + std::to_string(p.dims[L]));
  for (int i = 0; i < L; ++i) FD_REQUIRE(p.weight[i] != nullptr, FD_ERR_INVALID_ARG, "null MLP weight");
  size_t words = kMlpHeader;
  uint32_t hd[kMlpHeader] = {};
  hd[0] = kMlpMagic;
  hd[1] = (uint32_t)L;
  for (int i = 0; i <= L; ++i) hd[2 + i] = (uint32_t)p.dims[i];
  for (int i = 0; i < L; ++i) {
    const int kb = blocks16(p.dims[i]), ot = blocks16(p.dims[i + 1]);
    hd[11 + i] = (uint32_t)words;
    words += (size_t)ot * kb * 256;
    hd[19 + i] = (uint32_t)words;
    words += (size_t)ot * 16;
  }
  hd[27] = (uint32_t)words;
  std::vector<uint32_t> out(words, 0u);
  std::memcpy(out.data(), hd, sizeof(hd));
  for (int i = 0; i < L; ++i) {
    const int K = p.dims[i], O = p.dims[i + 1], kb = blocks16(K), ot = blocks16(O);
    float* wp = reinterpret_cast<float*>(out.data()) + hd[11 + i];
    float* bp = reinterpret_cast<float*>(out.data()) + hd[19 + i];
    for (int t = 0; t < ot; ++t)
      for (int b = 0; b < kb; ++b)
        for (int l = 0; l < 64; ++l)
          for (int r = 0; r < 4; ++r) {
            const int o = 16 * t + (l & 15), k = 16 * b + 4 * (l >> 4) + r;
            wp[((t * kb + b) * 64 + l) * 4 + r] = (o < O && k < K) ? p.weight[i][(size_t)o * K + k] : 0.f;
          }
    for (int o = 0; o < O; ++o) bp[o] = p.bias[i] ? p.bias[i][o] : 0.f;
  }
  return out;
}

void load_mlp(Engine& e, const fd_mlp_params& p) {
  const std::vector<uint32_t> blob = pack_mlp_host(p);
  MlpModel& m = e.mlp;
  m.loaded = false;
  m.blob.ensure(blob.size() * 4);
  FD_HIP(hipMemcpy(m.blob.ptr, blob.data(), blob.size() * 4, hipMemcpyHostToDevice));
  m.n_layers = p.n_layers;
  for (int i = 0; i < 9; ++i) m.dims[i] = i <= p.n_layers ? p.dims[i] : 0;
  m.words = (int)blob.size();
  m.hot = p.n_layers == 3 && blocks16(p.dims[0]) == 4 && blocks16(p.dims[1]) == 4 && blocks16(p.dims[2]) == 4;
  int cus = 0;
  FD_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, e.device));
  m.cus = cus > 0 ? cus : 256;
  const size_t lds = (size_t)m.words * 4;
  FD_REQUIRE(lds <= kLdsBudget, FD_ERR_UNSUPPORTED, "internal: packed MLP exceeds the LDS budget");
  // (the cap, not the model's size: another engine on this device may hold a larger model)
  FD_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(mlp_lds_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                             (int)kLdsBudget));
  // persistent workgroups: as many as stay resident beside each other, two per CU at the most (the reference shape's
  // form runs one wave per SIMD)
  int occ = 1;
  FD_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, reinterpret_cast<const void*>(mlp_lds_kernel), 64 * kWaves,
                                                      lds));
  m.occ_lds = std::max(1, occ);
  FD_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, reinterpret_cast<const void*>(mlp_ref_kernel), 64 * kWaves,
                                                      0));
  m.occ_ref = std::max(1, occ);
  m.loaded = true;
}

void launch_mlp(Engine& e, hipStream_t stream, const float* d_X, int64_t n, int32_t ld, double* d_prob) {
  const MlpModel& m = e.mlp;
  FD_REQUIRE(m.loaded, FD_ERR_NOT_LOADED, "Model graph_neural (MLP) not loaded");
  FD_REQUIRE(n >= 0 && n < (1ll << 31), FD_ERR_INVALID_ARG, "batch size out of range");
  FD_REQUIRE(ld >= m.dims[0], FD_ERR_INVALID_ARG,
             "row stride " + std::to_string(ld) + " is below the MLP's in_dim " + std::to_string(m.dims[0]));
  if (n == 0) return;
  FD_REQUIRE(d_X && d_prob, FD_ERR_INVALID_ARG, "null vectors / output");
  Engine::Timed* ev = e.timing ? e.next_event_pair(FD_TIMING_MLP) : nullptr;
  if (ev) FD_HIP(hipEventRecord(ev->a, stream));
  const size_t lds = (size_t)m.words * 4;
  const int64_t tiles = (n + kRows - 1) / kRows;
  const bool ref = m.hot && e.mlp_form == 0;  // option "mlp_form": 1 the LDS form for the reference shape too
  const int occ = ref ? m.occ_ref : m.occ_lds;
  const int per_cu = std::min(occ, e.mlp_wgs_per_cu ? e.mlp_wgs_per_cu : 2);  // option "mlp_wgs_per_cu"
  const unsigned grid = (unsigned)std::min<int64_t>((tiles + kWaves - 1) / kWaves, (int64_t)m.cus * per_cu);
  const int vec = (ld % 4 == 0 && m.dims[0] % 4 == 0 && (reinterpret_cast<uintptr_t>(d_X) & 15) == 0) ? 1 : 0;
  if (ref)
    hipLaunchKernelGGL(mlp_ref_kernel, dim3(grid), dim3(64 * kWaves), 0, stream, d_X, n, (int)ld,
                       m.blob.as<const uint32_t>(), vec, d_prob);
  else
    hipLaunchKernelGGL(mlp_lds_kernel, dim3(grid), dim3(64 * kWaves), lds, stream, d_X, n, (int)ld,
                       m.blob.as<const uint32_t>(), vec, d_prob);
  FD_HIP(hipGetLastError());
  ++e.mlp_total;
  if (ev) FD_HIP(hipEventRecord(ev->b, stream));
}

}  // namespace fd
