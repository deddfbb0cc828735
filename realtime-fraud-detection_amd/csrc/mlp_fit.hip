// mlp_fit.hip — minibatch training of the PyTorch member (graph_neural) on the CDNA4 matrix cores: the fit that
// produces what mlp.hip serves. The semantics are declared in include/fdengine.h ("training: the PyTorch MLP member")
// and DESIGN §4.16; the counter-based rules (row order, dropout mask) are mlp_fit_row.h, compiled by the kernels and by
// the host reference alike.
//
// A step is two launches, and a fit is a stream of them with nothing copied or waited for in between:
//   mlp_fit_step_kernel    one wave per chunk (= one 16-row tile of the batch). Forward as mlp.hip: H^T = W X^T on
//                          v_mfma_f32_16x16x4_f32, weights the A operand read from the packed blob (it stays in L2), a
//                          layer's D registers the next layer's B operand; the rows are gathered through the epoch's
//                          index array. Every layer's input is also written to LDS transposed (unit-major, the row on
//                          the k index), and 16 sign bits per hidden layer stay in registers (unit > 0 after ReLU and
//                          dropout). The two-class softmax and the CE gradient in f32 on lane group 0. Backward per layer:
//                            db  = the sum of dZ over the 16 lanes of a lane group (xor tree);
//                            dW  = dZ H^T, the batch rows as k: both operands read back from the transposed LDS images
//                                  (the C/D layout has the batch row on the lane, the MFMA wants it on k);
//                            dH  = W^T dZ: the A operand is the transposed pack of W (kept beside the forward one), dZ
//                                  in the D layout is the B operand as it stands; then the sign bits and the scale.
//                          The chunk's dW, db, loss sum and weight sum are written once to the chunk's partial: no
//                          atomics, no read-modify-write.
//   mlp_fit_update_kernel  a thread per parameter: the f32 partials added in ascending chunk order in an f64
//                          accumulator, divided there by the batch's weight sum, rounded once; Adam or SGD in f32, the new weight written to the flat master copy and to its
//                          two places in the operand blobs. Thread 0 adds the batch's loss to the epoch's f64 sum.
// Which workgroup computes a chunk is the launch's business only (option "mlp_fit_chunks_per_wg"): a chunk's partial
// depends on the batch alone, so the fit's bits do not depend on the grid.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "fd_internal.h"
#include "mlp_fit_row.h"

namespace fd {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kTileWords = kMlpFitRows * kMlpFitWidth;  // one transposed activation image (4 KiB)
constexpr int kUpdThreads = 256;

__host__ __device__ constexpr int blocks16(int d) { return (d + 15) >> 4; }

// The fit's shape on the device, read by uniform (scalar) loads: n_layers, dims[9], and per layer the word offsets of
// its A operands and bias in the forward blob, of its transposed A operands, and of its weights / bias in the flat
// parameter vector (PyTorch layout, layer after layer: weight [O x K] then bias [O]); last the parameter count.
enum { SH_L = 0, SH_DIMS = 1, SH_W = 10, SH_B = 18, SH_WT = 26, SH_P = 34, SH_PB = 42, SH_NP = 50, SH_WORDS = 52 };

struct StepArgs {
  const float* X;
  const uint8_t* y;
  const int32_t* idx;    // the batch's row ids (null: row b of the batch is row b of X)
  const uint8_t* masks;  // explicit masks [layer][row][64] (fd_mlp_grad_*), null: the hash
  const float* fwd;
  const float* bwd;
  const int* shape;
  float* partial;        // [chunk][n_params]
  float* lossw;          // [chunk][2]: loss sum, weight sum
  uint64_t key;
  uint32_t step, thr;
  float scale, pos_weight;
  int ld, nb, nchunks, cpw, vec;
};

// one layer: acc[t] = (bias block t | 0) + sum over k-steps (b, r) of A(t, b, r) x h[b][r], t < ot, b < kb. A operands
// from global memory, one 16-B load per four k-steps (coalesced: lane l takes the l-th float4 of the block).
__device__ __forceinline__ void layer_glb(const float* __restrict__ wp, const float* __restrict__ bp, int kb, int ot,
                                          int l, const f32x4 (&h)[4], f32x4 (&acc)[4]) {
  const int g = l >> 4;
#pragma unroll
  for (int t = 0; t < 4; ++t)
    acc[t] = (bp && t < ot) ? *reinterpret_cast<const f32x4*>(bp + 16 * t + 4 * g) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    if (b >= kb) break;
    f32x4 a[4];
#pragma unroll
    for (int t = 0; t < 4; ++t)
      a[t] = t < ot ? *reinterpret_cast<const f32x4*>(wp + ((t * kb + b) * 64 + l) * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int t = 0; t < 4; ++t)
        if (t < ot) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t][r], h[b][r], acc[t], 0, 0, 0);
  }
}

// The D-layout registers (block t, lane group g, register r = unit 16 t + 4 g + r of batch row c) -> the transposed
// image: unit-major, a unit's 16 rows in the order (row & 3) * 4 + (row >> 2), so that lane (m = lane & 15,
// kk = lane >> 4) reads rows kk, 4 + kk, 8 + kk, 12 + kk of unit 16 blk + m — its operand of four k-steps over the
// batch rows — as one 16-B read at ((16 blk + m) * 4 + kk) * 4. 64 lanes write 64 distinct banks.
__device__ __forceinline__ void store_transposed(float* __restrict__ img, const f32x4 (&v)[4], int nblk, int g, int c) {
  const int pos = (c & 3) * 4 + (c >> 2);
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    if (t >= nblk) break;
#pragma unroll
    for (int r = 0; r < 4; ++r) img[(16 * t + 4 * g + r) * 16 + pos] = v[t][r];
  }
}

__device__ __forceinline__ float group_sum16(float v) {  // over the 16 lanes of a lane group, a fixed xor tree
  v += __shfl_xor(v, 8, 16);
  v += __shfl_xor(v, 4, 16);
  v += __shfl_xor(v, 2, 16);
  v += __shfl_xor(v, 1, 16);
  return v;
}

__global__ void __launch_bounds__(64) mlp_fit_step_kernel(const StepArgs a) {
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) float sh_h[8 * kTileWords];  // layer i's input, transposed
  __shared__ __attribute__((aligned(16))) float sh_dz[kTileWords];     // the current layer's dZ, transposed
  const int* __restrict__ sp = a.shape;
  const int L = sp[SH_L], NP = sp[SH_NP];
  const int in_dim = sp[SH_DIMS];
  const int l = threadIdx.x, g = l >> 4, c = l & 15;
  for (int q = 0; q < a.cpw; ++q) {
    const long long chunk_ll = (long long)blockIdx.x * a.cpw + q;
    if (chunk_ll >= a.nchunks) break;
    const int chunk = (int)chunk_ll;
    float* __restrict__ part = a.partial + (size_t)chunk * NP;
    const int rb = chunk * kMlpFitRows + c;  // the lane's row of the batch
    const bool live = rb < a.nb;
    const int64_t rid = live ? (a.idx ? (int64_t)a.idx[rb] : (int64_t)rb) : 0;
    const int yv = live ? (a.y[rid] != 0) : 0;
    const float wr = live ? (yv ? a.pos_weight : 1.f) : 0.f;
    f32x4 h[4], acc[4];
    {  // the row in the B-operand order (mlp.hip load_rows); a dead row is zeros
      const float* p = a.X + rid * (int64_t)a.ld;
      const int kb0 = blocks16(in_dim);
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        h[b] = f32x4{0.f, 0.f, 0.f, 0.f};
        const int col = 16 * b + 4 * g;
        if (!live || b >= kb0) continue;
        if (a.vec) {
          if (col < in_dim) h[b] = *reinterpret_cast<const f32x4*>(p + col);
        } else {
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (col + r < in_dim) h[b][r] = p[col + r];
        }
      }
    }
    unsigned long long bits_lo = 0ull, bits_hi = 0ull;  // hidden layer i's 16 sign bits at 16 (i & 3) of lo (i < 4) / hi
    // ---- forward
    for (int i = 0; i + 1 < L; ++i) {
      const int kb = blocks16(sp[SH_DIMS + i]), ot = blocks16(sp[SH_DIMS + i + 1]);
      store_transposed(sh_h + i * kTileWords, h, kb, g, c);
      layer_glb(a.fwd + sp[SH_W + i], a.fwd + sp[SH_B + i], kb, ot, l, h, acc);
      const uint64_t lk = mlp_fit_mask_layer(a.key, a.step, (uint32_t)i);
      const uint8_t* mrow = a.masks ? a.masks + ((size_t)i * a.nb + (live ? rb : 0)) * kMlpFitWidth : nullptr;
      unsigned bits = 0u;
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float v = 0.f;
          if (t < ot) {
            const int u = 16 * t + 4 * g + r;
            v = acc[t][r] > 0.f ? acc[t][r] : 0.f;
            const bool keep = mrow ? mrow[u] != 0 : (a.thr == 0u || mlp_fit_keep(lk, (uint32_t)rb, (uint32_t)u, a.thr));
            v = keep ? v * a.scale : 0.f;
          }
          h[t][r] = v;
          bits |= (v > 0.f ? 1u : 0u) << (4 * t + r);
        }
      if (i < 4)
        bits_lo |= (unsigned long long)bits << (16 * i);
      else
        bits_hi |= (unsigned long long)bits << (16 * (i - 4));
    }
    const int kbl = blocks16(sp[SH_DIMS + L - 1]);
    store_transposed(sh_h + (L - 1) * kTileWords, h, kbl, g, c);
    layer_glb(a.fwd + sp[SH_W + L - 1], a.fwd + sp[SH_B + L - 1], kbl, 1, l, h, acc);
    // ---- loss and its gradient: lane group 0 holds the two logits of row c in registers 0 and 1
    f32x4 dz[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) dz[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    float lossr = 0.f, wsum = 0.f;
    if (g == 0 && live) {
      // two classes: with d = z_other - z_y the row's loss is softplus(d) and its gradient +-sigmoid(d), the other
      // class's probability — formed without the cancellation of softmax - onehot (p_y - 1 = -p_other exactly)
      const float d = yv ? acc[0][0] - acc[0][1] : acc[0][1] - acc[0][0];
      const float t = expf(-fabsf(d));
      const float po = (d >= 0.f ? 1.f : t) / (1.f + t);
      lossr = wr * ((d > 0.f ? d : 0.f) + log1pf(t));
      dz[0][yv ? 0 : 1] = wr * po;
      dz[0][yv ? 1 : 0] = -(wr * po);
      wsum = wr;
    }
    lossr = group_sum16(lossr);
    wsum = group_sum16(wsum);
    if (l == 0) {
      a.lossw[2 * chunk] = lossr;
      a.lossw[2 * chunk + 1] = wsum;
    }
    // ---- backward
    for (int i = L - 1; i >= 0; --i) {
      const int K = sp[SH_DIMS + i], O = sp[SH_DIMS + i + 1];
      const int kb = blocks16(K), ot = blocks16(O);
      float* __restrict__ pw = part + sp[SH_P + i];
      float* __restrict__ pb = part + sp[SH_PB + i];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        if (t >= ot) break;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float s = group_sum16(dz[t][r]);
          const int u = 16 * t + 4 * g + r;
          if (c == 0 && u < O) pb[u] = s;
        }
      }
      __syncthreads();  // the layer before's reads of sh_dz are over (and every write of sh_h, the first time)
      store_transposed(sh_dz, dz, ot, g, c);
      __syncthreads();
      const float* hi = sh_h + i * kTileWords;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        if (t >= ot) break;
        const f32x4 za = *reinterpret_cast<const f32x4*>(sh_dz + ((16 * t + c) * 4 + g) * 4);
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          if (b >= kb) break;
          const f32x4 hb = *reinterpret_cast<const f32x4*>(hi + ((16 * b + c) * 4 + g) * 4);
          f32x4 w = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int s = 0; s < 4; ++s) w = __builtin_amdgcn_mfma_f32_16x16x4f32(za[s], hb[s], w, 0, 0, 0);
          const int k = 16 * b + c;  // D layout: lane (g, c), register r = dW[16 t + 4 g + r][16 b + c]
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int o = 16 * t + 4 * g + r;
            if (o < O && k < K) pw[o * K + k] = w[r];
          }
        }
      }
      if (i > 0) {
        layer_glb(a.bwd + sp[SH_WT + i], nullptr, ot, kb, l, dz, acc);
        const int hl = i - 1;  // the hidden layer whose output this layer read
        const unsigned bits =
            (unsigned)((hl < 4 ? bits_lo >> (16 * hl) : bits_hi >> (16 * (hl - 4))) & 0xffffull);
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            dz[t][r] = (t < kb && ((bits >> (4 * t + r)) & 1u)) ? acc[t][r] * a.scale : 0.f;
      }
    }
    __syncthreads();  // the next chunk rewrites the images
  }
}

struct UpdateArgs {
  const int* shape;
  const float* partial;
  const float* lossw;
  float* w;       // flat master parameters
  float* m;       // Adam: exp_avg; SGD: momentum buffer
  float* v;       // Adam: exp_avg_sq
  float* fwd;
  float* bwd;
  float* grad;    // mode 0: the gradient out
  double* loss;   // mode 0: the loss out (=); else the epoch's sum (+=)
  int nchunks, mode;  // 0 gradient only, 1 Adam, 2 SGD
  float lr, beta1, beta2, eps, wd, momentum;
  float omb1, omb2;           // 1 - beta1, 1 - beta2, formed in f64 (torch hands lerp_ / addcmul_ the f64 scalars)
  float step_size, bc2_sqrt;  // Adam: lr / (1 - beta1^t), sqrt(1 - beta2^t), computed in f64 on the host
};

__global__ void __launch_bounds__(kUpdThreads) mlp_fit_update_kernel(const UpdateArgs a) {
#pragma clang fp contract(off)
  const int* __restrict__ sp = a.shape;
  const int L = sp[SH_L], NP = sp[SH_NP];
  const int j = blockIdx.x * kUpdThreads + threadIdx.x;
  // the chunks' f32 partials, added in ascending chunk order in an f64 accumulator, divided there by the batch's weight
  // sum and rounded to f32 once
  double Wd = 0.0;
  for (int c = 0; c < a.nchunks; ++c) Wd += (double)a.lossw[2 * c + 1];
  if (j == 0) {
    double ls = 0.0;
    for (int c = 0; c < a.nchunks; ++c) ls += (double)a.lossw[2 * c];
    const double bl = ls / Wd;  // (the loss stays f64: loss_curve is)
    *a.loss = a.mode == 0 ? bl : *a.loss + bl;
  }
  if (j >= NP) return;
  double s = 0.0;
  for (int c = 0; c < a.nchunks; ++c) s += (double)a.partial[(size_t)c * NP + j];
  float gr = (float)(s / Wd);  // one rounding
  if (a.mode == 0) {
    a.grad[j] = gr;
    return;
  }
  float p = a.w[j];
  if (a.wd != 0.f) gr = gr + a.wd * p;
  if (a.mode == 1) {  // torch.optim.Adam's single-tensor step
    float m = a.m[j], v = a.v[j];
    m = m + (gr - m) * a.omb1;                               // exp_avg.lerp_(grad, 1 - beta1)
    v = v * a.beta2 + (a.omb2 * gr) * gr;                  // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, 1 - beta2)
    const float denom = sqrtf(v) / a.bc2_sqrt + a.eps;
    p = p + (-a.step_size) * (m / denom);                   // param.addcdiv_(exp_avg, denom, value=-step_size)
    a.m[j] = m;
    a.v[j] = v;
  } else {            // torch.optim.SGD: buf = momentum buf + grad (buf starts at 0 = the first step's clone)
    if (a.momentum != 0.f) {
      const float buf = a.momentum * a.m[j] + gr;
      a.m[j] = buf;
      gr = buf;
    }
    p = p + (-a.lr) * gr;
  }
  a.w[j] = p;
  // the parameter's places in the operand blobs
  for (int i = 0; i < L; ++i) {
    const int K = sp[SH_DIMS + i], O = sp[SH_DIMS + i + 1];
    const int jw = j - sp[SH_P + i];
    if (jw < 0) break;
    if (jw < O * K) {
      const int o = jw / K, k = jw - o * K;
      const int kb = blocks16(K), ot = blocks16(O);
      // forward: [out block][k block][lane = (k & 15) >> 2 << 4 | o & 15][k & 3]
      a.fwd[sp[SH_W + i] + (((o >> 4) * kb + (k >> 4)) * 64 + (((k & 15) >> 2) << 4 | (o & 15))) * 4 + (k & 3)] = p;
      // transposed: the same pack of W^T
      a.bwd[sp[SH_WT + i] + (((k >> 4) * ot + (o >> 4)) * 64 + (((o & 15) >> 2) << 4 | (k & 15))) * 4 + (o & 3)] = p;
      break;
    }
    if (jw < O * K + O) {
      a.fwd[sp[SH_B + i] + (jw - O * K)] = p;
      break;
    }
  }
}

// the masks of one step as bytes [layer][row][64], by the step kernel's hash
__global__ void __launch_bounds__(kUpdThreads) mlp_fit_mask_kernel(uint64_t key, uint32_t step, uint32_t thr,
                                                                   int hidden_layers, int rows, uint8_t* out) {
  const int64_t total = (int64_t)hidden_layers * rows * kMlpFitWidth;
  const int64_t j = (int64_t)blockIdx.x * kUpdThreads + threadIdx.x;
  if (j >= total) return;
  const int u = (int)(j % kMlpFitWidth);
  const int64_t lr = j / kMlpFitWidth;
  const int row = (int)(lr % rows), layer = (int)(lr / rows);
  out[j] = (thr == 0u || mlp_fit_keep(mlp_fit_mask_layer(key, step, (uint32_t)layer), (uint32_t)row, (uint32_t)u, thr))
               ? 1 : 0;
}

// ---------------------------------------------------------------- host side

struct Shape {
  int w[SH_WORDS] = {};
  int L() const { return w[SH_L]; }
  int dim(int i) const { return w[SH_DIMS + i]; }
  int np() const { return w[SH_NP]; }
  int fwd_words = 0, bwd_words = 0;
};

fd_mlp_params as_mlp_params(const fd_mlp_fit_params& p) {
  fd_mlp_params q{};
  q.n_layers = p.n_layers;
  for (int i = 0; i < 9; ++i) q.dims[i] = p.dims[i];
  for (int i = 0; i < 8; ++i) {
    q.weight[i] = p.init_weight[i];
    q.bias[i] = p.init_bias[i];
  }
  return q;
}

// the shape, the forward blob (pack_mlp_host: its limits and messages) and the transposed one, the flat parameters
Shape build_model(const fd_mlp_fit_params& p, std::vector<uint32_t>& fwd, std::vector<float>& bwd,
                  std::vector<float>& flat) {
  fwd = pack_mlp_host(as_mlp_params(p));
  Shape s;
  const int L = p.n_layers;
  s.w[SH_L] = L;
  for (int i = 0; i <= L; ++i) s.w[SH_DIMS + i] = p.dims[i];
  int np = 0, wt = 0;
  for (int i = 0; i < L; ++i) {
    const int K = p.dims[i], O = p.dims[i + 1];
    s.w[SH_W + i] = (int)fwd[11 + i];
    s.w[SH_B + i] = (int)fwd[19 + i];
    s.w[SH_WT + i] = wt;
    wt += blocks16(K) * blocks16(O) * 256;
    s.w[SH_P + i] = np;
    s.w[SH_PB + i] = np + O * K;
    np += O * K + O;
  }
  s.w[SH_NP] = np;
  s.fwd_words = (int)fwd.size();
  s.bwd_words = wt;
  bwd.assign((size_t)wt, 0.f);
  flat.assign((size_t)np, 0.f);
  for (int i = 0; i < L; ++i) {
    const int K = p.dims[i], O = p.dims[i + 1], ot = blocks16(O);
    for (int o = 0; o < O; ++o) {
      for (int k = 0; k < K; ++k) {
        const float v = p.init_weight[i][(size_t)o * K + k];
        flat[(size_t)s.w[SH_P + i] + (size_t)o * K + k] = v;
        bwd[(size_t)s.w[SH_WT + i] +
            (size_t)((((k >> 4) * ot + (o >> 4)) * 64 + (((o & 15) >> 2) << 4 | (k & 15))) * 4 + (o & 3))] = v;
      }
      flat[(size_t)s.w[SH_PB + i] + o] = p.init_bias[i] ? p.init_bias[i][o] : 0.f;
    }
  }
  return s;
}

void unflatten(const Shape& s, const std::vector<float>& flat, const fd_mlp_fit_out& out) {
  for (int i = 0; i < s.L(); ++i) {
    const int K = s.dim(i), O = s.dim(i + 1);
    if (out.weight[i]) std::memcpy(out.weight[i], flat.data() + s.w[SH_P + i], sizeof(float) * O * K);
    if (out.bias[i]) std::memcpy(out.bias[i], flat.data() + s.w[SH_PB + i], sizeof(float) * O);
  }
}

bool unit_interval(double v) { return v >= 0.0 && v < 1.0; }  // (false for a NaN)

int64_t steps_per_epoch(const fd_mlp_fit_params& p, int64_t n) { return (n + p.batch_size - 1) / p.batch_size; }

std::vector<int32_t> epoch_order(uint64_t key, int32_t epoch, int64_t n) {
  std::vector<std::pair<uint64_t, int32_t>> kv((size_t)n);
  for (int64_t r = 0; r < n; ++r) kv[(size_t)r] = {mlp_fit_order_key(key, (uint32_t)epoch, (uint32_t)r), (int32_t)r};
  std::stable_sort(kv.begin(), kv.end(), [](const auto& x, const auto& y) { return x.first < y.first; });
  std::vector<int32_t> out((size_t)n);
  for (int64_t r = 0; r < n; ++r) out[(size_t)r] = kv[(size_t)r].second;
  return out;
}

void fill_masks_host(uint64_t key, uint32_t step, uint32_t thr, int hidden_layers, int rows, uint8_t* out) {
  for (int i = 0; i < hidden_layers; ++i) {
    const uint64_t lk = mlp_fit_mask_layer(key, step, (uint32_t)i);
    for (int b = 0; b < rows; ++b)
      for (int u = 0; u < kMlpFitWidth; ++u)
        out[((size_t)i * rows + b) * kMlpFitWidth + u] =
            (thr == 0u || mlp_fit_keep(lk, (uint32_t)b, (uint32_t)u, thr)) ? 1 : 0;
  }
}

// ---- the host reference: loss and gradients of one batch at flat parameters w, plain f32 loops
// rows: the batch's row ids (null: 0 .. nb - 1); masks as fd_mlp_grad_* (null: all kept)
double ref_grad(const Shape& s, const float* w, const float* X, const uint8_t* y, int32_t ld, const int32_t* rows,
               int nb, const uint8_t* masks, float scale, float pos_weight, float* grad) {
#pragma clang fp contract(off)
  const int L = s.L(), np = s.np();
  // as the kernels: f32 sums over the rows of a chunk (ascending), the chunks' sums added in ascending order in f64
  std::vector<double> total((size_t)np, 0.0);
  std::vector<float> cg((size_t)np);
  double Wd = 0.0, lossd = 0.0;
  std::vector<float> act((size_t)(L + 1) * kMlpFitWidth), d(kMlpFitWidth), dn(kMlpFitWidth);
  for (int b0 = 0; b0 < nb; b0 += kMlpFitRows) {
    std::fill(cg.begin(), cg.end(), 0.f);
    float closs = 0.f, cw = 0.f;
    for (int b = b0; b < std::min(nb, b0 + kMlpFitRows); ++b) {
      const int64_t rid = rows ? rows[b] : b;
      const float* x = X + rid * (int64_t)ld;
      const int yv = y[rid] != 0;
      const float wr = yv ? pos_weight : 1.f;
      for (int k = 0; k < s.dim(0); ++k) act[k] = x[k];
      for (int i = 0; i < L; ++i) {
        const int K = s.dim(i), O = s.dim(i + 1);
        const float* wi = w + s.w[SH_P + i];
        const float* bi = w + s.w[SH_PB + i];
        const float* hin = act.data() + (size_t)i * kMlpFitWidth;
        float* hout = act.data() + (size_t)(i + 1) * kMlpFitWidth;
        for (int o = 0; o < O; ++o) {
          float z = bi[o];
          for (int k = 0; k < K; ++k) z += wi[(size_t)o * K + k] * hin[k];
          if (i + 1 < L) {
            z = z > 0.f ? z : 0.f;
            const bool keep = !masks || masks[((size_t)i * nb + b) * kMlpFitWidth + o] != 0;
            z = keep ? z * scale : 0.f;
          }
          hout[o] = z;
        }
      }
      const float* z = act.data() + (size_t)L * kMlpFitWidth;
      const float dl = z[1 - yv] - z[yv];  // the kernel's form: loss = softplus(dl), gradient +-sigmoid(dl)
      const float t = std::exp(-std::fabs(dl));
      const float po = (dl >= 0.f ? 1.f : t) / (1.f + t);
      closs += wr * ((dl > 0.f ? dl : 0.f) + std::log1p(t));
      cw += wr;
      std::fill(d.begin(), d.end(), 0.f);
      d[1 - yv] = wr * po;
      d[yv] = -(wr * po);
      for (int i = L - 1; i >= 0; --i) {
        const int K = s.dim(i), O = s.dim(i + 1);
        const float* wi = w + s.w[SH_P + i];
        float* gw = cg.data() + s.w[SH_P + i];
        float* gb = cg.data() + s.w[SH_PB + i];
        const float* hin = act.data() + (size_t)i * kMlpFitWidth;
        for (int o = 0; o < O; ++o) {
          gb[o] += d[o];
          for (int k = 0; k < K; ++k) gw[(size_t)o * K + k] += d[o] * hin[k];
        }
        if (i > 0) {
          for (int k = 0; k < K; ++k) {
            float v = 0.f;
            for (int o = 0; o < O; ++o) v += wi[(size_t)o * K + k] * d[o];
            dn[k] = hin[k] > 0.f ? v * scale : 0.f;  // hin > 0: past its ReLU and kept
          }
          std::copy(dn.begin(), dn.begin() + K, d.begin());
        }
      }
    }
    for (int q = 0; q < np; ++q) total[(size_t)q] += (double)cg[(size_t)q];
    lossd += (double)closs;
    Wd += (double)cw;
  }
  for (int q = 0; q < np; ++q) grad[q] = (float)(total[(size_t)q] / Wd);
  return lossd / Wd;
}

void check_inputs_host(const float* X, const uint8_t* y, int64_t n, int32_t ld, int in_dim) {
  FD_REQUIRE(X && y, FD_ERR_INVALID_ARG, "mlp_fit: null X / y");
  for (int64_t r = 0; r < n; ++r) {
    FD_REQUIRE(y[r] <= 1, FD_ERR_INVALID_ARG,
               "mlp_fit: label " + std::to_string((int)y[r]) + " at row " + std::to_string(r) + " is outside {0, 1}");
    for (int k = 0; k < in_dim; ++k)
      FD_REQUIRE(std::isfinite(X[r * (int64_t)ld + k]), FD_ERR_INVALID_ARG,
                 "mlp_fit: a non-finite value in X at row " + std::to_string(r));
  }
}

struct AdamScalars {
  float step_size, bc2_sqrt;
};
AdamScalars adam_scalars(const fd_mlp_fit_params& p, int64_t t) {  // t: 1-based step, torch's f64 arithmetic
  const double bc1 = 1.0 - std::pow(p.beta1, (double)t), bc2 = 1.0 - std::pow(p.beta2, (double)t);
  return {(float)(p.lr / bc1), (float)std::sqrt(bc2)};
}

int vec_ok(const float* d_X, int32_t ld, int in_dim) {
  return (ld % 4 == 0 && in_dim % 4 == 0 && (reinterpret_cast<uintptr_t>(d_X) & 15) == 0) ? 1 : 0;
}

// the step launch: chunks dealt to workgroups cpw at a time (option "mlp_fit_chunks_per_wg"; 0: a chunk each)
void launch_step(Engine& e, StepArgs a) {
  const int64_t want = e.mlp_fit.chunks_per_wg > 0 ? e.mlp_fit.chunks_per_wg : 1;
  a.cpw = (int)std::min<int64_t>(want, a.nchunks);
  const unsigned grid = (unsigned)((a.nchunks + a.cpw - 1) / a.cpw);
  hipLaunchKernelGGL(mlp_fit_step_kernel, dim3(grid), dim3(64), 0, e.stream, a);
  FD_HIP(hipGetLastError());
  ++e.mlp_fit.launches;
}
void launch_update(Engine& e, const UpdateArgs& a, int np) {
  hipLaunchKernelGGL(mlp_fit_update_kernel, dim3((unsigned)((np + kUpdThreads - 1) / kUpdThreads)), dim3(kUpdThreads), 0,
                     e.stream, a);
  FD_HIP(hipGetLastError());
  ++e.mlp_fit.launches;
}

// model buffers of a fit / a gradient call on the device; nchunks: of the largest batch
Shape upload_model(Engine& e, const fd_mlp_fit_params& p, int nchunks) {
  MlpFitScratch& s = e.mlp_fit;
  std::vector<uint32_t> fwd;
  std::vector<float> bwd, flat;
  const Shape sh = build_model(p, fwd, bwd, flat);
  const size_t pbytes = (size_t)nchunks * sh.np() * sizeof(float);
  FD_REQUIRE(pbytes <= (1ull << 30), FD_ERR_UNSUPPORTED, "mlp_fit: the batch's chunk partials exceed 1 GiB");
  s.shape.ensure(sizeof(sh.w));
  s.fwd.ensure(fwd.size() * 4);
  s.bwd.ensure(bwd.size() * 4);
  s.w.ensure(flat.size() * 4);
  s.m.ensure(flat.size() * 4);
  s.v.ensure(flat.size() * 4);
  s.partial.ensure(pbytes);
  s.lossw.ensure((size_t)nchunks * 2 * sizeof(float));
  FD_HIP(hipMemcpyAsync(s.shape.ptr, sh.w, sizeof(sh.w), hipMemcpyHostToDevice, e.stream));
  FD_HIP(hipMemcpyAsync(s.fwd.ptr, fwd.data(), fwd.size() * 4, hipMemcpyHostToDevice, e.stream));
  FD_HIP(hipMemcpyAsync(s.bwd.ptr, bwd.data(), bwd.size() * 4, hipMemcpyHostToDevice, e.stream));
  FD_HIP(hipMemcpyAsync(s.w.ptr, flat.data(), flat.size() * 4, hipMemcpyHostToDevice, e.stream));
  FD_HIP(hipMemsetAsync(s.m.ptr, 0, flat.size() * 4, e.stream));
  FD_HIP(hipMemsetAsync(s.v.ptr, 0, flat.size() * 4, e.stream));
  FD_HIP(hipStreamSynchronize(e.stream));  // (the host vectors go out of scope)
  return sh;
}

}  // namespace

void mlp_fit_check(const fd_mlp_fit_params& p, int64_t n, int32_t ld, bool fit) {
  // (the shape's limits are pack_mlp_host's, restated so that they are named before a weight is read)
  FD_REQUIRE(p.n_layers >= 2 && p.n_layers <= 8, FD_ERR_UNSUPPORTED,
             "MLP n_layers must be in [2, 8], got " + std::to_string(p.n_layers));
  for (int i = 0; i < p.n_layers; ++i)
    FD_REQUIRE(p.dims[i] >= 1 && p.dims[i] <= 64, FD_ERR_UNSUPPORTED,
               "MLP width must be in [1, 64], got " + std::to_string(p.dims[i]) + " (dims[" + std::to_string(i) + "])");
  FD_REQUIRE(p.dims[p.n_layers] == 2, FD_ERR_UNSUPPORTED,
             "MLP output layer must have exactly 2 outputs, got " + std::to_string(p.dims[p.n_layers]));
  for (int i = 0; i < p.n_layers; ++i)
    FD_REQUIRE(p.init_weight[i] != nullptr, FD_ERR_INVALID_ARG, "mlp_fit: null initial weight");
  FD_REQUIRE(n >= 1, FD_ERR_INVALID_ARG, "mlp_fit: n must be at least 1");
  FD_REQUIRE(n <= 2147483647ll, FD_ERR_UNSUPPORTED, "mlp_fit: more than 2^31 - 1 rows");
  FD_REQUIRE(ld >= p.dims[0], FD_ERR_INVALID_ARG,
             "mlp_fit: row stride " + std::to_string(ld) + " is below in_dim " + std::to_string(p.dims[0]));
  FD_REQUIRE(unit_interval(p.dropout), FD_ERR_INVALID_ARG, "mlp_fit: dropout must be in [0, 1)");
  FD_REQUIRE(std::isfinite(p.pos_weight) && p.pos_weight > 0.0, FD_ERR_INVALID_ARG,
             "mlp_fit: pos_weight must be finite and > 0");
  if (!fit) {
    FD_REQUIRE(n <= 65536, FD_ERR_UNSUPPORTED, "mlp_grad: a batch holds at most 65536 rows");
    return;
  }
  FD_REQUIRE(p.epochs >= 1, FD_ERR_INVALID_ARG, "mlp_fit: epochs must be at least 1");
  FD_REQUIRE(p.batch_size >= 1, FD_ERR_INVALID_ARG,
             "mlp_fit: batch_size must be at least 1, got " + std::to_string(p.batch_size));
  FD_REQUIRE(p.batch_size <= 65536, FD_ERR_UNSUPPORTED, "mlp_fit: batch_size above 65536");
  FD_REQUIRE((int64_t)p.epochs * n <= (1ll << 29), FD_ERR_UNSUPPORTED,
             "mlp_fit: epochs * n exceeds 2^29 (every epoch's index array is built once)");
  FD_REQUIRE(p.optimizer == FD_MLP_OPT_ADAM || p.optimizer == FD_MLP_OPT_SGD, FD_ERR_INVALID_ARG,
             "mlp_fit: optimizer must be FD_MLP_OPT_ADAM or FD_MLP_OPT_SGD");
  FD_REQUIRE(std::isfinite(p.lr) && p.lr > 0.0, FD_ERR_INVALID_ARG, "mlp_fit: lr must be finite and > 0");
  FD_REQUIRE(std::isfinite(p.weight_decay) && p.weight_decay >= 0.0, FD_ERR_INVALID_ARG,
             "mlp_fit: weight_decay must be finite and >= 0");
  if (p.optimizer == FD_MLP_OPT_ADAM) {
    FD_REQUIRE(unit_interval(p.beta1) && unit_interval(p.beta2), FD_ERR_INVALID_ARG, "mlp_fit: betas must be in [0, 1)");
    FD_REQUIRE(std::isfinite(p.eps) && p.eps > 0.0, FD_ERR_INVALID_ARG, "mlp_fit: eps must be finite and > 0");
  } else {
    FD_REQUIRE(unit_interval(p.momentum), FD_ERR_INVALID_ARG, "mlp_fit: momentum must be in [0, 1)");
  }
}

void mlp_fit_check_inputs(const float* X, const uint8_t* y, int64_t n, int32_t ld, const fd_mlp_fit_params& p) {
  check_inputs_host(X, y, n, ld, p.dims[0]);
}

int32_t mlp_fit_batch_rows(const fd_mlp_fit_params& p, int64_t n, int64_t step) {
  const int64_t spe = steps_per_epoch(p, n);
  FD_REQUIRE(step >= 0 && step < spe * p.epochs, FD_ERR_INVALID_ARG, "mlp_fit: step outside the fit");
  const int64_t j = step % spe;
  return (int32_t)std::min<int64_t>(p.batch_size, n - j * p.batch_size);
}

void mlp_fit_batch_ref_host(int64_t n, const fd_mlp_fit_params& p, int32_t epoch, int64_t step, int32_t* order,
                            uint8_t* masks, int32_t* rows) {
  FD_REQUIRE(epoch >= 0 && epoch < p.epochs, FD_ERR_INVALID_ARG, "mlp_fit: epoch outside the fit");
  const uint64_t key = mlp_fit_key(p.seed);
  const int32_t nb = mlp_fit_batch_rows(p, n, step);
  if (rows) *rows = nb;
  if (order) {
    const std::vector<int32_t> o = epoch_order(key, epoch, n);
    std::memcpy(order, o.data(), sizeof(int32_t) * (size_t)n);
  }
  if (masks) fill_masks_host(key, (uint32_t)step, mlp_fit_threshold(p.dropout), p.n_layers - 1, nb, masks);
}

void mlp_fit_batch_device(Engine& e, int64_t n, const fd_mlp_fit_params& p, int32_t epoch, int64_t step,
                          int32_t* order, uint8_t* masks, int32_t* rows) {
  FD_REQUIRE(epoch >= 0 && epoch < p.epochs, FD_ERR_INVALID_ARG, "mlp_fit: epoch outside the fit");
  MlpFitScratch& s = e.mlp_fit;
  const uint64_t key = mlp_fit_key(p.seed);
  const int32_t nb = mlp_fit_batch_rows(p, n, step);
  if (rows) *rows = nb;
  if (order) {
    const std::vector<int32_t> o = epoch_order(key, epoch, n);
    s.idx.ensure(sizeof(int32_t) * (size_t)n);
    FD_HIP(hipMemcpyAsync(s.idx.ptr, o.data(), sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, e.stream));
    FD_HIP(hipMemcpyAsync(order, s.idx.ptr, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, e.stream));
    FD_HIP(hipStreamSynchronize(e.stream));
  }
  if (masks) {
    const int64_t total = (int64_t)(p.n_layers - 1) * nb * kMlpFitWidth;
    s.masks.ensure((size_t)total);
    hipLaunchKernelGGL(mlp_fit_mask_kernel, dim3((unsigned)((total + kUpdThreads - 1) / kUpdThreads)),
                       dim3(kUpdThreads), 0, e.stream, key, (uint32_t)step, mlp_fit_threshold(p.dropout),
                       p.n_layers - 1, (int)nb, s.masks.as<uint8_t>());
    FD_HIP(hipGetLastError());
    FD_HIP(hipMemcpyAsync(masks, s.masks.ptr, (size_t)total, hipMemcpyDeviceToHost, e.stream));
    FD_HIP(hipStreamSynchronize(e.stream));
  }
}

void mlp_grad_ref_host(const float* X, const uint8_t* y, int64_t n, int32_t ld, const fd_mlp_fit_params& p,
                       const uint8_t* masks, fd_mlp_fit_out& out) {
  mlp_fit_check(p, n, ld, false);
  check_inputs_host(X, y, n, ld, p.dims[0]);
  std::vector<uint32_t> fwd;
  std::vector<float> bwd, flat;
  const Shape sh = build_model(p, fwd, bwd, flat);
  std::vector<float> grad((size_t)sh.np());
  const double loss = ref_grad(sh, flat.data(), X, y, ld, nullptr, (int)n, masks, (float)(1.0 / (1.0 - p.dropout)),
                              (float)p.pos_weight, grad.data());
  unflatten(sh, grad, out);
  if (out.loss_curve) out.loss_curve[0] = loss;
  out.steps = 0;
}

void mlp_fit_ref_host(const float* X, const uint8_t* y, int64_t n, int32_t ld, const fd_mlp_fit_params& p,
                      fd_mlp_fit_out& out) {
#pragma clang fp contract(off)
  mlp_fit_check(p, n, ld, true);
  check_inputs_host(X, y, n, ld, p.dims[0]);
  std::vector<uint32_t> fwd;
  std::vector<float> bwd, w;
  const Shape sh = build_model(p, fwd, bwd, w);
  const int np = sh.np();
  std::vector<float> grad((size_t)np), m((size_t)np, 0.f), v((size_t)np, 0.f);
  const uint64_t key = mlp_fit_key(p.seed);
  const uint32_t thr = mlp_fit_threshold(p.dropout);
  const float scale = (float)(1.0 / (1.0 - p.dropout));
  const int64_t spe = steps_per_epoch(p, n);
  const int HL = p.n_layers - 1;
  std::vector<uint8_t> masks(thr ? (size_t)HL * p.batch_size * kMlpFitWidth : 0);
  const float lr = (float)p.lr, b2 = (float)p.beta2, eps = (float)p.eps, wd = (float)p.weight_decay,
              mom = (float)p.momentum, omb1 = (float)(1.0 - p.beta1), omb2 = (float)(1.0 - p.beta2);
  int64_t step = 0;
  for (int ep = 0; ep < p.epochs; ++ep) {
    const std::vector<int32_t> order = epoch_order(key, ep, n);
    double acc = 0.0;
    for (int64_t j = 0; j < spe; ++j, ++step) {
      const int nb = (int)std::min<int64_t>(p.batch_size, n - j * p.batch_size);
      if (thr) fill_masks_host(key, (uint32_t)step, thr, HL, nb, masks.data());
      acc += ref_grad(sh, w.data(), X, y, ld, order.data() + j * p.batch_size, nb, thr ? masks.data() : nullptr,
                              scale, (float)p.pos_weight, grad.data());
      const AdamScalars as = adam_scalars(p, step + 1);
      for (int q = 0; q < np; ++q) {
        float g = grad[q], pw = w[q];
        if (wd != 0.f) g = g + wd * pw;
        if (p.optimizer == FD_MLP_OPT_ADAM) {
          m[q] = m[q] + (g - m[q]) * omb1;
          v[q] = v[q] * b2 + (omb2 * g) * g;
          const float denom = std::sqrt(v[q]) / as.bc2_sqrt + eps;
          pw = pw + (-as.step_size) * (m[q] / denom);
        } else {
          if (mom != 0.f) {
            m[q] = mom * m[q] + g;
            g = m[q];
          }
          pw = pw + (-lr) * g;
        }
        w[q] = pw;
      }
    }
    if (out.loss_curve) out.loss_curve[ep] = acc / (double)spe;
  }
  unflatten(sh, w, out);
  out.steps = step;
}

void mlp_grad_device(Engine& e, const float* d_X, const uint8_t* d_y, int64_t n, int32_t ld,
                     const fd_mlp_fit_params& p, const uint8_t* d_masks, fd_mlp_fit_out& out) {
  mlp_fit_check(p, n, ld, false);
  FD_REQUIRE(d_X && d_y, FD_ERR_INVALID_ARG, "mlp_grad: null X / y");
  MlpFitScratch& s = e.mlp_fit;
  const int nchunks = (int)((n + kMlpFitRows - 1) / kMlpFitRows);
  const Shape sh = upload_model(e, p, nchunks);
  s.loss.ensure(sizeof(double));
  StepArgs a{};
  a.X = d_X;
  a.y = d_y;
  a.idx = nullptr;
  a.masks = d_masks;
  a.fwd = s.fwd.as<float>();
  a.bwd = s.bwd.as<float>();
  a.shape = s.shape.as<int>();
  a.partial = s.partial.as<float>();
  a.lossw = s.lossw.as<float>();
  a.key = 0;
  a.step = 0;
  a.thr = 0;  // (no mask array: every unit kept)
  a.scale = (float)(1.0 / (1.0 - p.dropout));
  a.pos_weight = (float)p.pos_weight;
  a.ld = ld;
  a.nb = (int)n;
  a.nchunks = nchunks;
  a.vec = vec_ok(d_X, ld, p.dims[0]);
  launch_step(e, a);
  UpdateArgs u{};
  u.shape = a.shape;
  u.partial = a.partial;
  u.lossw = a.lossw;
  u.grad = s.m.as<float>();  // (the moment buffer is free in a gradient call)
  u.loss = s.loss.as<double>();
  u.nchunks = nchunks;
  u.mode = 0;
  launch_update(e, u, sh.np());
  std::vector<float> grad((size_t)sh.np());
  double loss = 0.0;
  FD_HIP(hipMemcpyAsync(grad.data(), s.m.ptr, grad.size() * 4, hipMemcpyDeviceToHost, e.stream));
  FD_HIP(hipMemcpyAsync(&loss, s.loss.ptr, sizeof(double), hipMemcpyDeviceToHost, e.stream));
  FD_HIP(hipStreamSynchronize(e.stream));
  unflatten(sh, grad, out);
  if (out.loss_curve) out.loss_curve[0] = loss;
  out.steps = 0;
}

void mlp_fit_device(Engine& e, const float* d_X, const uint8_t* d_y, int64_t n, int32_t ld,
                    const fd_mlp_fit_params& p, fd_mlp_fit_out& out) {
  mlp_fit_check(p, n, ld, true);
  FD_REQUIRE(d_X && d_y, FD_ERR_INVALID_ARG, "mlp_fit: null X / y");
  MlpFitScratch& s = e.mlp_fit;
  const int64_t spe = steps_per_epoch(p, n);
  const int max_nb = (int)std::min<int64_t>(p.batch_size, n);
  const int max_chunks = (max_nb + kMlpFitRows - 1) / kMlpFitRows;
  const Shape sh = upload_model(e, p, max_chunks);
  // every epoch's row order, built and uploaded once
  const uint64_t key = mlp_fit_key(p.seed);
  s.idx.ensure(sizeof(int32_t) * (size_t)n * p.epochs);
  s.loss.ensure(sizeof(double) * (size_t)p.epochs);
  {
    std::vector<int32_t> all((size_t)n * p.epochs);
    for (int ep = 0; ep < p.epochs; ++ep) {
      const std::vector<int32_t> o = epoch_order(key, ep, n);
      std::memcpy(all.data() + (size_t)ep * n, o.data(), sizeof(int32_t) * (size_t)n);
    }
    FD_HIP(hipMemcpyAsync(s.idx.ptr, all.data(), all.size() * sizeof(int32_t), hipMemcpyHostToDevice, e.stream));
    FD_HIP(hipMemsetAsync(s.loss.ptr, 0, sizeof(double) * (size_t)p.epochs, e.stream));
    FD_HIP(hipStreamSynchronize(e.stream));
  }
  StepArgs a{};
  a.X = d_X;
  a.y = d_y;
  a.masks = nullptr;
  a.fwd = s.fwd.as<float>();
  a.bwd = s.bwd.as<float>();
  a.shape = s.shape.as<int>();
  a.partial = s.partial.as<float>();
  a.lossw = s.lossw.as<float>();
  a.key = key;
  a.thr = mlp_fit_threshold(p.dropout);
  a.scale = (float)(1.0 / (1.0 - p.dropout));
  a.pos_weight = (float)p.pos_weight;
  a.ld = ld;
  a.vec = vec_ok(d_X, ld, p.dims[0]);
  UpdateArgs u{};
  u.shape = a.shape;
  u.partial = a.partial;
  u.lossw = a.lossw;
  u.w = s.w.as<float>();
  u.m = s.m.as<float>();
  u.v = s.v.as<float>();
  u.fwd = s.fwd.as<float>();
  u.bwd = s.bwd.as<float>();
  u.mode = p.optimizer == FD_MLP_OPT_ADAM ? 1 : 2;
  u.lr = (float)p.lr;
  u.beta1 = (float)p.beta1;
  u.beta2 = (float)p.beta2;
  u.omb1 = (float)(1.0 - p.beta1);
  u.omb2 = (float)(1.0 - p.beta2);
  u.eps = (float)p.eps;
  u.wd = (float)p.weight_decay;
  u.momentum = (float)p.momentum;
  int64_t step = 0;
  for (int ep = 0; ep < p.epochs; ++ep) {
    for (int64_t j = 0; j < spe; ++j, ++step) {
      const int nb = (int)std::min<int64_t>(p.batch_size, n - j * p.batch_size);
      a.idx = s.idx.as<int32_t>() + (size_t)ep * n + (size_t)j * p.batch_size;
      a.nb = nb;
      a.nchunks = (nb + kMlpFitRows - 1) / kMlpFitRows;
      a.step = (uint32_t)step;
      launch_step(e, a);
      const AdamScalars as = adam_scalars(p, step + 1);
      u.step_size = as.step_size;
      u.bc2_sqrt = as.bc2_sqrt;
      u.nchunks = a.nchunks;
      u.loss = s.loss.as<double>() + ep;
      launch_update(e, u, sh.np());
    }
  }
  s.steps += (unsigned long long)step;
  std::vector<float> w((size_t)sh.np());
  std::vector<double> sums((size_t)p.epochs);
  FD_HIP(hipMemcpyAsync(w.data(), s.w.ptr, w.size() * 4, hipMemcpyDeviceToHost, e.stream));
  FD_HIP(hipMemcpyAsync(sums.data(), s.loss.ptr, sums.size() * sizeof(double), hipMemcpyDeviceToHost, e.stream));
  FD_HIP(hipStreamSynchronize(e.stream));
  unflatten(sh, w, out);
  if (out.loss_curve)
    for (int ep = 0; ep < p.epochs; ++ep) out.loss_curve[ep] = sums[(size_t)ep] / (double)spe;
  out.steps = step;
}

}  // namespace fd
