// shap.hip — path-dependent TreeSHAP of a loaded forest's raw output (include/fdengine.h "forest attribution").
//
// Host side: the path table (shap_paths_host) and the recursive reference (shap_ref_host, Algorithm 2 of Lundberg et
// al. 2018, on the trees themselves). Device side: shap_kernel, shap_reduce_kernel, shap_topk_kernel.
//
// The path form. A root-to-leaf path with leaf value v and m unique features; element j has z_j (the share of the
// training weight that follows the path's edges on that feature) and, for a row, o_j in {0, 1} (the row itself
// follows them). With c_k the coefficient of t^k in P(t) = prod_j (z_j + o_j t) and W_m[k] = k! (m-1-k)! / m!,
//   phi_i += v (o_i - z_i) sum_k q_k W_m[k],   q = P / (z_i + o_i t).
// Because o is 0 or 1 no division is left: for o_i = 0, z_i q = P, so the term is -v sum_k c_k W_m[k], the same for
// every such element of the path; for o_i = 1 the divisor is monic and q comes from the top by
// q_{k-1} = c_k - z_i q_k (the direction in which an error shrinks by z_i <= 1 per step).
//
// shap_kernel: one lane per row, one wave per workgroup. The wave streams the paths of its chunk of the table: a
// path's length, features, intervals and z are wave-uniform, only o differs per lane, and the recurrences are
// unrolled against the length (one instantiation per length 1 .. FD_SHAP_MAX_PATH: every private array is indexed
// statically). The row's feature values sit in LDS as [f][64] f32 and its sums as [f][64] f64, so a wave-uniform f
// touches 64 consecutive words. blockIdx.y is the chunk: the table's split into chunks depends on the forest alone, a
// chunk's sums are formed path by path, and shap_reduce_kernel adds the chunks' sums in chunk order — a row's bits
// do not depend on the batch around it, and nothing is added atomically.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>

#include "fd_internal.h"

namespace fd {

namespace {

constexpr int kShapDepthMax = 4096;  // recursion bound of the host routines (a tree deeper than this is refused)

bool arrays_complete(const fd_tree_arrays& t) {
  return t.n_trees > 0 && t.tree_offsets && t.left && t.right && t.feature && t.threshold && t.leaf_value;
}

// the walk's comparison: go left <=> x < t in f32
float split_lt(bool xgb, double thr) { return xgb ? (float)thr : sklearn_threshold_to_lt(thr); }

double xgb_base_margin(const fd_forest_params& p) {
  const float bs = (float)p.base_score;
  return (double)(-logf(1.0f / bs - 1.0f));  // as pack_forest_host: RegLossObj::ProbToMargin in f32
}

int check_forest(const fd_forest_params& p, const fd_tree_arrays& t, const double* cover) {
  FD_REQUIRE(p.kind == FD_FOREST_XGB_BINARY_LOGISTIC || p.kind == FD_FOREST_SKLEARN_IFOREST ||
                 p.kind == FD_FOREST_SKLEARN_PROBA,
             FD_ERR_INVALID_ARG, "unknown forest kind");
  FD_REQUIRE(arrays_complete(t), FD_ERR_INVALID_ARG, "incomplete tree arrays");
  FD_REQUIRE(p.num_feature > 0, FD_ERR_INVALID_ARG, "num_feature must be positive");
  FD_REQUIRE(cover != nullptr, FD_ERR_INVALID_ARG, "null cover");
  const int depth = forest_depth_probe(t);
  FD_REQUIRE(depth >= 0, FD_ERR_INVALID_ARG, "incomplete tree arrays or a tree that is not a tree");
  FD_REQUIRE(depth <= kShapDepthMax, FD_ERR_UNSUPPORTED, "attribution: a tree deeper than 4096 levels");
  const int64_t m = t.tree_offsets[t.n_trees];
  for (int64_t o = 0; o < m; ++o)
    if (t.left[o] >= 0)
      FD_REQUIRE(t.feature[o] >= 0 && t.feature[o] < p.num_feature, FD_ERR_INVALID_ARG,
                 "split feature outside [0, num_feature)");
  const std::string bad = shap_cover_problem(t, cover);
  FD_REQUIRE(bad.empty(), FD_ERR_INVALID_ARG, bad);
  return depth;
}

struct Edge {
  int32_t f;
  float thr;
  bool left, dflt;
  double z;
};

struct PathBuilder {
  const fd_tree_arrays& t;
  const double* cover;
  bool xgb;
  ShapTable& out;
  int tree = 0;
  int64_t a = 0;
  std::vector<Edge> edges;

  void leaf(int32_t o) {
    fd_shap_elem el[FD_SHAP_MAX_PATH];
    int m = 0;
    for (const Edge& e : edges) {
      int j = 0;
      while (j < m && el[j].feature != e.f) ++j;
      if (j == m) {
        FD_REQUIRE(m < FD_SHAP_MAX_PATH, FD_ERR_UNSUPPORTED,
                   "attribution: tree " + std::to_string(tree) + " has a path with more than " +
                       std::to_string(FD_SHAP_MAX_PATH) + " unique features");
        el[m] = fd_shap_elem{};
        el[m].feature = e.f;
        el[m].lo = -std::numeric_limits<float>::infinity();
        el[m].hi = std::numeric_limits<float>::infinity();
        el[m].nan_follows = 1;
        el[m].z = 1.0;
        ++m;
      }
      if (e.left) {
        el[j].hi = el[j].has_hi ? std::min(el[j].hi, e.thr) : e.thr;
        el[j].has_hi = 1;
      } else {
        el[j].lo = std::max(el[j].lo, e.thr);
      }
      if (!e.dflt) el[j].nan_follows = 0;
      el[j].z *= e.z;
    }
    fd_shap_path p{};
    p.elem_offset = (int64_t)out.elems.size();
    p.len = m;
    p.tree = tree;
    p.value = xgb ? (double)(float)t.leaf_value[a + o] : t.leaf_value[a + o];
    p.pz = 1.0;
    for (int j = 0; j < m; ++j) p.pz *= el[j].z;
    out.elems.insert(out.elems.end(), el, el + m);
    out.paths.push_back(p);
    out.info.max_len = std::max(out.info.max_len, m);
    out.info.bias += p.value * p.pz;
  }

  void walk(int32_t o) {
    if (t.left[a + o] < 0) return leaf(o);
    const int32_t kids[2] = {t.left[a + o], t.right[a + o]};
    const bool dl = t.default_left && t.default_left[a + o];
    for (int s = 0; s < 2; ++s) {
      Edge e;
      e.f = t.feature[a + o];
      e.thr = split_lt(xgb, t.threshold[a + o]);
      e.left = s == 0;
      e.dflt = e.left == dl;
      e.z = cover[a + kids[s]] / cover[a + o];
      edges.push_back(e);
      walk(kids[s]);
      edges.pop_back();
    }
  }
};

}  // namespace

std::string shap_cover_problem(const fd_tree_arrays& t, const double* cover) {
  std::vector<int32_t> st;
  for (int i = 0; i < t.n_trees; ++i) {
    const int64_t a = t.tree_offsets[i];
    st.assign(1, 0);
    while (!st.empty()) {
      const int32_t o = st.back();
      st.pop_back();
      const double c = cover[a + o];
      if (!(std::isfinite(c) && c > 0.0))
        return "cover of tree " + std::to_string(i) + " node " + std::to_string(o) + " is not a finite number > 0";
      if (t.left[a + o] >= 0) {
        st.push_back(t.right[a + o]);
        st.push_back(t.left[a + o]);
      }
    }
  }
  return std::string();
}

ShapTable shap_paths_host(const fd_forest_params& p, const fd_tree_arrays& t, const double* cover) {
  check_forest(p, t, cover);
  ShapTable out;
  PathBuilder b{t, cover, p.kind == FD_FOREST_XGB_BINARY_LOGISTIC, out};
  for (int i = 0; i < t.n_trees; ++i) {
    b.tree = i;
    b.a = t.tree_offsets[i];
    b.walk(0);
  }
  if (b.xgb) out.info.bias += xgb_base_margin(p);
  out.info.n_paths = (int64_t)out.paths.size();
  out.info.n_elems = (int64_t)out.elems.size();
  // the kernel's split: a function of the table alone (a row's bits must not depend on the batch)
  const int64_t chunks = std::min<int64_t>(32, std::max<int64_t>(1, (out.info.n_paths + 63) / 64));
  out.info.chunk_paths = (out.info.n_paths + chunks - 1) / chunks;
  out.info.n_chunks = (int32_t)((out.info.n_paths + out.info.chunk_paths - 1) / out.info.chunk_paths);
  return out;
}

// ------------------------------------------------------------------------------------------------
// the recursive reference

namespace {

struct PathEl {
  int d;
  double z, o, w;
};

void extend_path(PathEl* m, int u, double pz, double po, int pi) {
  m[u].d = pi;
  m[u].z = pz;
  m[u].o = po;
  m[u].w = u == 0 ? 1.0 : 0.0;
  for (int i = u - 1; i >= 0; --i) {
    m[i + 1].w += po * m[i].w * (i + 1) / (double)(u + 1);
    m[i].w = pz * m[i].w * (u - i) / (double)(u + 1);
  }
}

void unwind_path(PathEl* m, int u, int k) {
  const double o = m[k].o, z = m[k].z;
  double nxt = m[u].w;
  for (int j = u - 1; j >= 0; --j) {
    if (o != 0.0) {
      const double tmp = m[j].w;
      m[j].w = nxt * (u + 1) / ((j + 1) * o);
      nxt = tmp - m[j].w * z * (u - j) / (double)(u + 1);
    } else {
      m[j].w = m[j].w * (u + 1) / (z * (u - j));
    }
  }
  for (int j = k; j < u; ++j) {
    m[j].d = m[j + 1].d;
    m[j].z = m[j + 1].z;
    m[j].o = m[j + 1].o;
  }
}

double unwound_sum(const PathEl* m, int u, int k) {
  const double o = m[k].o, z = m[k].z;
  double nxt = m[u].w, total = 0.0;
  for (int j = u - 1; j >= 0; --j) {
    if (o != 0.0) {
      const double tmp = nxt * (u + 1) / ((j + 1) * o);
      total += tmp;
      nxt = m[j].w - tmp * z * (u - j) / (double)(u + 1);
    } else {
      total += m[j].w / z / ((u - j) / (double)(u + 1));
    }
  }
  return total;
}

struct RefWalk {
  const fd_tree_arrays& t;
  const double* cover;
  bool xgb;
  int64_t a = 0;
  const float* x = nullptr;
  int ld = 0;
  double* phi = nullptr;

  void go(int32_t o, const PathEl* parent, int u, double pz, double po, int pi) {
    PathEl* m = const_cast<PathEl*>(parent) + u + 1;
    std::copy(parent, parent + u, m);
    extend_path(m, u, pz, po, pi);
    if (t.left[a + o] < 0) {
      const double v = xgb ? (double)(float)t.leaf_value[a + o] : t.leaf_value[a + o];
      for (int i = 1; i <= u; ++i) phi[m[i].d] += unwound_sum(m, u, i) * (m[i].o - m[i].z) * v;
      return;
    }
    const int32_t f = t.feature[a + o];
    const bool missing = f >= ld || x[f] != x[f];
    const bool dl = t.default_left && t.default_left[a + o];
    const bool left = missing ? dl : x[f] < split_lt(xgb, t.threshold[a + o]);
    const int32_t hot = left ? t.left[a + o] : t.right[a + o];
    const int32_t cold = left ? t.right[a + o] : t.left[a + o];
    double iz = 1.0, io = 1.0;
    int k = 1;
    while (k <= u && m[k].d != f) ++k;
    if (k <= u) {
      iz = m[k].z;
      io = m[k].o;
      unwind_path(m, u, k);
      --u;
    }
    go(hot, m, u + 1, iz * cover[a + hot] / cover[a + o], io, f);
    go(cold, m, u + 1, iz * cover[a + cold] / cover[a + o], 0.0, f);
  }

  double mean(int32_t o) const {
    if (t.left[a + o] < 0) return xgb ? (double)(float)t.leaf_value[a + o] : t.leaf_value[a + o];
    const int32_t l = t.left[a + o], r = t.right[a + o];
    return (cover[a + l] * mean(l) + cover[a + r] * mean(r)) / cover[a + o];
  }
};

}  // namespace

void shap_ref_host(const fd_forest_params& p, const fd_tree_arrays& t, const double* cover, const float* X, int64_t n,
                   int32_t ld, double* phi, int32_t ld_phi) {
  const int depth = check_forest(p, t, cover);
  FD_REQUIRE(n >= 0 && ld > 0 && ld_phi >= p.num_feature + 1, FD_ERR_INVALID_ARG,
             "bad arguments (ld > 0, ld_phi >= num_feature + 1)");
  FD_REQUIRE(n == 0 || (X && phi), FD_ERR_INVALID_ARG, "null X / phi");
  const int nf = p.num_feature;
  RefWalk w{t, cover, p.kind == FD_FOREST_XGB_BINARY_LOGISTIC};
  double bias = 0.0;
  for (int i = 0; i < t.n_trees; ++i) {
    w.a = t.tree_offsets[i];
    bias += w.mean(0);
  }
  if (w.xgb) bias += xgb_base_margin(p);
  // level l of the recursion holds at most min(l, nf) + 1 elements behind its parent's
  std::vector<PathEl> arena((size_t)(depth + 3) * (size_t)(std::min(depth, nf) + 3));
  for (int64_t r = 0; r < n; ++r) {
    w.x = X + r * (int64_t)ld;
    w.ld = ld;
    w.phi = phi + r * (int64_t)ld_phi;
    std::fill(w.phi, w.phi + nf, 0.0);
    for (int i = 0; i < t.n_trees; ++i) {
      w.a = t.tree_offsets[i];
      w.go(0, arena.data(), 0, 1.0, 1.0, -1);
    }
    w.phi[nf] = bias;
  }
}

void shap_forget(PackedForest& pf) {
  pf.t_cover.clear();
  pf.t_cover.shrink_to_fit();
  pf.shap.paths.release();
  pf.shap.elems.release();
  pf.shap.gen = 0;
}

// ------------------------------------------------------------------------------------------------
// device side

namespace {

constexpr int kShapRows = 64;     // rows per workgroup: one wave, one lane per row
constexpr int kShapBatch = 4096;  // rows per launch: bounds the per-chunk sums (n_chunks x num_feature x 4096 f64)

// W_m[k] = k! (m-1-k)! / m!
__host__ __device__ constexpr double shap_weight(int m, int k) {
  double w = 1.0 / m;
  for (int j = 1; j <= k; ++j) w = w * j / (m - j);
  return w;
}

// One path of M unique features for this lane's row. el: the path's elements (wave-uniform); xl / al: this lane's
// column of the feature tile / of the sums.
template <int M>
__device__ __forceinline__ void shap_path(const fd_shap_elem* __restrict__ el, double v, const float* xl, double* al) {
  double z[M];
  bool o[M];
  int f[M];
#pragma unroll
  for (int j = 0; j < M; ++j) {
    const fd_shap_elem e = el[j];
    f[j] = e.feature;
    z[j] = e.z;
    const float x = xl[e.feature * kShapRows];
    const bool in = !(x < e.lo) && (e.has_hi ? x < e.hi : true);
    o[j] = (x != x) ? e.nan_follows != 0 : in;
  }
  // c_k of prod_j (z_j + o_j t)
  double c[M + 1];
  c[0] = 1.0;
#pragma unroll
  for (int k = 1; k <= M; ++k) c[k] = 0.0;
#pragma unroll
  for (int j = 0; j < M; ++j) {
#pragma unroll
    for (int k = j + 1; k >= 1; --k) c[k] = z[j] * c[k] + (o[j] ? c[k - 1] : 0.0);
    c[0] *= z[j];
  }
  double d0 = 0.0;
#pragma unroll
  for (int k = 0; k < M; ++k) d0 += c[k] * shap_weight(M, k);
  const double zero_term = -v * d0;
#pragma unroll
  for (int i = 0; i < M; ++i) {
    double term = zero_term;
    if (__ballot(o[i]) != 0ull) {  // some row of the wave follows this feature's edges
      double q = c[M];
      double d1 = q * shap_weight(M, M - 1);
#pragma unroll
      for (int k = M - 1; k >= 1; --k) {
        q = c[k] - z[i] * q;
        d1 += q * shap_weight(M, k - 1);
      }
      if (o[i]) term = v * (1.0 - z[i]) * d1;
    }
    al[f[i] * kShapRows] += term;
  }
}

// grid (row blocks of the batch, chunks). rows: the batch's row indices into X (null: row0 + j). partial:
// [chunk][feature][pstride] sums of this batch.
__global__ void __launch_bounds__(kShapRows)
shap_kernel(const float* __restrict__ X, int64_t n, int ld, int nf, const int64_t* __restrict__ rows, int64_t row0,
            int64_t count, const fd_shap_path* __restrict__ paths, const fd_shap_elem* __restrict__ elems,
            int64_t n_paths, int64_t chunk_paths, double* __restrict__ partial, int64_t pstride) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double* acc = reinterpret_cast<double*>(smem);                    // [nf][64]
  float* xs = reinterpret_cast<float*>(acc + (size_t)nf * kShapRows);  // [nf][64]
  const int lane = threadIdx.x;
  const int64_t j = (int64_t)blockIdx.x * kShapRows + lane;
  const bool valid = j < count;
  const int64_t r = valid ? (rows ? rows[row0 + j] : row0 + j) : -1;
  const bool in_range = r >= 0 && r < n;
  const int ncopy = ld < nf ? ld : nf;
  for (int f = 0; f < nf; ++f) {
    float v = 0.f;
    if (in_range) v = f < ncopy ? X[r * (int64_t)ld + f] : __builtin_nanf("");  // a column >= ld: missing
    xs[f * kShapRows + lane] = v;
    acc[f * kShapRows + lane] = 0.0;
  }
  // (one wave, and a lane reads only its own column: no barrier)
  const int64_t p0 = (int64_t)blockIdx.y * chunk_paths;
  const int64_t p1 = p0 + chunk_paths < n_paths ? p0 + chunk_paths : n_paths;
  const float* xl = xs + lane;
  double* al = acc + lane;
  for (int64_t p = p0; p < p1; ++p) {
    const fd_shap_path ph = paths[p];
    const int len = __builtin_amdgcn_readfirstlane(ph.len);
    const fd_shap_elem* el = elems + ph.elem_offset;
    switch (len) {
#define FD_SHAP_CASE(M) \
  case M:               \
    shap_path<M>(el, ph.value, xl, al); \
    break;
      FD_SHAP_CASE(1) FD_SHAP_CASE(2) FD_SHAP_CASE(3) FD_SHAP_CASE(4) FD_SHAP_CASE(5) FD_SHAP_CASE(6)
      FD_SHAP_CASE(7) FD_SHAP_CASE(8) FD_SHAP_CASE(9) FD_SHAP_CASE(10) FD_SHAP_CASE(11) FD_SHAP_CASE(12)
      FD_SHAP_CASE(13) FD_SHAP_CASE(14) FD_SHAP_CASE(15) FD_SHAP_CASE(16)
#undef FD_SHAP_CASE
      default:  // a lone leaf: the bias only
        break;
    }
  }
  static_assert(FD_SHAP_MAX_PATH == 16, "one case per path length");
  if (!valid) return;
  double* out = partial + (int64_t)blockIdx.y * nf * pstride + j;
  for (int f = 0; f < nf; ++f) out[(int64_t)f * pstride] = acc[f * kShapRows + lane];
}

// phi[row0 + j, f] = the chunks' sums in chunk order; column nf = bias. Thread <-> (f, j), j fastest.
__global__ void __launch_bounds__(256)
shap_reduce_kernel(const double* __restrict__ partial, int n_chunks, int nf, int64_t pstride, int64_t count,
                   int64_t row0, const int64_t* __restrict__ rows, int64_t n, double bias, double* __restrict__ phi,
                   int ld_phi) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= count * (nf + 1)) return;
  const int f = (int)(idx / count);
  const int64_t j = idx - (int64_t)f * count;
  const int64_t r = rows ? rows[row0 + j] : row0 + j;
  double s;
  if (!(r >= 0 && r < n)) {
    s = __builtin_nan("");
  } else if (f == nf) {
    s = bias;
  } else {
    s = partial[(int64_t)f * pstride + j];
    for (int c = 1; c < n_chunks; ++c) s += partial[((int64_t)c * nf + f) * pstride + j];
  }
  phi[(row0 + j) * (int64_t)ld_phi + f] = s;
}

// One wave per row. Place t is the candidate that comes next after place t - 1 in (key descending, column ascending)
// order: every lane scans its columns (lane, lane + 64, ...) for its best such candidate, the wave reduces.
__global__ void __launch_bounds__(256)
shap_topk_kernel(const double* __restrict__ phi, int64_t n, int ld_phi, int nf, int k, int by_abs,
                 int32_t* __restrict__ idx, double* __restrict__ val) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n) return;  // wave-uniform
  const double* p = phi + row * (int64_t)ld_phi;
  constexpr int kNone = 0x7fffffff;
  double pk = __builtin_inf();
  int pi = -1;
  int t = 0;
  for (; t < k; ++t) {
    double bk = 0.0, bv = 0.0;
    int bi = kNone;
    for (int f = lane; f < nf; f += 64) {
      const double v = p[f];
      if (v == 0.0 || v != v) continue;
      const double key = by_abs ? fabs(v) : v;
      const bool after = key < pk || (key == pk && f > pi);
      if (after && (bi == kNone || key > bk)) {  // (f ascends: an equal key keeps the lower column)
        bk = key;
        bv = v;
        bi = f;
      }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      const double ok = __shfl_xor(bk, off, 64), ov = __shfl_xor(bv, off, 64);
      const int oi = __shfl_xor(bi, off, 64);
      if (oi != kNone && (bi == kNone || ok > bk || (ok == bk && oi < bi))) {
        bk = ok;
        bv = ov;
        bi = oi;
      }
    }
    if (bi == kNone) break;  // wave-uniform: every lane holds the wave's result
    if (lane == 0) {
      idx[row * k + t] = bi;
      val[row * k + t] = bv;
    }
    pk = bk;
    pi = bi;
  }
  for (int u = t + lane; u < k; u += 64) {
    idx[row * k + u] = -1;
    val[row * k + u] = 0.0;
  }
}

fd_tree_arrays tree_view(const PackedForest& pf) {
  fd_tree_arrays t{};
  t.n_trees = pf.n_trees;
  t.tree_offsets = pf.t_off.data();
  t.left = pf.t_left.data();
  t.right = pf.t_right.data();
  t.feature = pf.t_feature.data();
  t.threshold = pf.t_threshold.data();
  t.default_left = pf.t_dleft.data();
  t.leaf_value = pf.t_leaf.data();
  return t;
}

void build_image(const PackedForest& pf) {
  FD_REQUIRE(!pf.t_off.empty(), FD_ERR_NOT_LOADED, "forest has no host copy of its trees");
  FD_REQUIRE(pf.num_feature <= kMaxFeatures, FD_ERR_UNSUPPORTED, "attribution: num_feature must be <= 64");
  const ShapTable tb = shap_paths_host(pf.params, tree_view(pf), pf.t_cover.data());
  ShapImage& im = pf.shap;
  auto up = [](DeviceBuffer& d, const void* h, size_t bytes) {
    d.ensure(std::max<size_t>(bytes, 8));
    if (bytes) FD_HIP(hipMemcpy(d.ptr, h, bytes, hipMemcpyHostToDevice));
  };
  up(im.paths, tb.paths.data(), tb.paths.size() * sizeof(fd_shap_path));
  up(im.elems, tb.elems.data(), tb.elems.size() * sizeof(fd_shap_elem));
  im.n_paths = tb.info.n_paths;
  im.chunk_paths = tb.info.chunk_paths;
  im.n_chunks = tb.info.n_chunks;
  im.bias = tb.info.bias;
  im.gen = pf.gen;
}

}  // namespace

void launch_forest_shap(Engine& e, const PackedForest& pf, const float* d_X, int64_t n, int32_t ld,
                        const int64_t* d_rows, int64_t n_rows, double* d_phi, int32_t ld_phi) {
  FD_REQUIRE(!pf.t_cover.empty(), FD_ERR_NOT_LOADED,
             "forest has no covers: attribution needs fd_forest_set_cover (or a model file with sum_hessian)");
  FD_REQUIRE(ld > 0 && ld_phi >= pf.num_feature + 1, FD_ERR_INVALID_ARG,
             "bad arguments (ld > 0, ld_phi >= num_feature + 1)");
  if (pf.shap.gen != pf.gen || pf.gen == 0) build_image(pf);
  const int64_t total = d_rows ? n_rows : n;
  if (total <= 0) return;
  FD_REQUIRE(d_X && d_phi, FD_ERR_INVALID_ARG, "null X / phi");
  const ShapImage& im = pf.shap;
  const int nf = pf.num_feature;
  const size_t lds = (size_t)nf * kShapRows * (sizeof(double) + sizeof(float));
  const int64_t pstride = std::min<int64_t>(kShapBatch, (total + kShapRows - 1) / kShapRows * kShapRows);
  e.shap_partial.ensure((size_t)im.n_chunks * nf * pstride * sizeof(double));
  hipStream_t st = e.stream;
  for (int64_t row0 = 0; row0 < total; row0 += kShapBatch) {
    const int64_t count = std::min<int64_t>(kShapBatch, total - row0);
    const dim3 grid((unsigned)((count + kShapRows - 1) / kShapRows), (unsigned)im.n_chunks);
    hipLaunchKernelGGL(shap_kernel, grid, dim3(kShapRows), lds, st, d_X, n, (int)ld, nf, d_rows, row0, count,
                       im.paths.as<const fd_shap_path>(), im.elems.as<const fd_shap_elem>(), im.n_paths,
                       im.chunk_paths, e.shap_partial.as<double>(), pstride);
    FD_HIP(hipGetLastError());
    const int64_t cells = count * (nf + 1);
    hipLaunchKernelGGL(shap_reduce_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, st,
                       e.shap_partial.as<const double>(), im.n_chunks, nf, pstride, count, row0, d_rows, n, im.bias,
                       d_phi, (int)ld_phi);
    FD_HIP(hipGetLastError());
    ++e.shap_total;
  }
}

void launch_shap_topk(Engine& e, const double* d_phi, int64_t n, int32_t ld_phi, int32_t nf, int32_t k, bool by_abs,
                      int32_t* d_idx, double* d_val) {
  FD_REQUIRE(n >= 0 && nf > 0 && ld_phi >= nf, FD_ERR_INVALID_ARG, "bad arguments (num_feature > 0, ld_phi >= num_feature)");
  FD_REQUIRE(k >= 1 && k <= FD_SHAP_MAX_TOPK, FD_ERR_INVALID_ARG, "k must be in [1, 16]");
  if (n == 0) return;
  FD_REQUIRE(d_phi && d_idx && d_val, FD_ERR_INVALID_ARG, "null phi / idx / val");
  hipLaunchKernelGGL(shap_topk_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, e.stream, d_phi, n, (int)ld_phi,
                     (int)nf, (int)k, by_abs ? 1 : 0, d_idx, d_val);
  FD_HIP(hipGetLastError());
}

}  // namespace fd
