// gbdt_sanitize.cpp — a stand-alone CPU program (its own main) that drives the host reference of the histogram GBDT
// fit (csrc/gbdt.hip over csrc/gbdt_row.h) under AddressSanitizer + UBSan. It is compiled together with gbdt.hip by
// the command in DESIGN §6, runs on the CPU only, is never loaded into Python and uses no device.
//
// It grows the smallest and the largest shape of the split-search cases (1 row x 1 feature, max_bin 2, depth 1, and
// 4,099 rows x 64 features with NaNs, max_bin 256, depth 10: most of the heap stays empty), with and without a row
// mask, then runs a whole fit with row and column sampling, and checks the invariants a memory error would break:
// node counts inside the capacity, children inside the tree, covers that add up.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "fd_internal.h"

namespace {

struct Lcg {
  uint64_t s;
  double next() {  // [0, 1)
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(s >> 11) * (1.0 / 9007199254740992.0);
  }
};

struct Model {
  std::vector<int64_t> off;
  std::vector<int32_t> left, right, feature;
  std::vector<double> thr, leaf, sh, lc, bw;
  std::vector<uint8_t> dl;
  fd_tree_arrays trees{};
  fd_gbdt_model model{};
  Model(int n_trees, int64_t cap)
      : off(n_trees + 1), left(cap), right(cap), feature(cap), thr(cap), leaf(cap), sh(cap), lc(cap), bw(cap), dl(cap) {
    trees = fd_tree_arrays{n_trees, off.data(), left.data(), right.data(), feature.data(), thr.data(), dl.data(),
                           leaf.data()};
    model = fd_gbdt_model{&trees, sh.data(), lc.data(), bw.data()};
  }
};

int failures = 0;
#define CHECK(c)                                              \
  do {                                                        \
    if (!(c)) {                                               \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
      ++failures;                                             \
    }                                                         \
  } while (0)

void check_forest(const Model& m, int n_trees, int64_t n_nodes, int F) {
  CHECK(m.off[0] == 0 && m.off[n_trees] == n_nodes);
  for (int t = 0; t < n_trees; ++t) {
    const int64_t o = m.off[t], size = m.off[t + 1] - o;
    CHECK(size >= 1);
    for (int64_t i = 0; i < size; ++i) {
      if (m.left[o + i] == -1) continue;
      CHECK(m.left[o + i] > i && m.left[o + i] < size && m.right[o + i] == m.left[o + i] + 1 && m.right[o + i] < size);
      CHECK(m.feature[o + i] >= 0 && m.feature[o + i] < F && m.lc[o + i] > 1e-6);
      CHECK(m.sh[o + i] == m.sh[o + m.left[o + i]] + m.sh[o + m.right[o + i]]);
    }
  }
}

void make_data(Lcg& rng, int64_t n, int F, double nan_frac, std::vector<float>& X, std::vector<uint8_t>& y) {
  X.resize((size_t)n * F);
  y.resize((size_t)n);
  for (int64_t r = 0; r < n; ++r) {
    for (int f = 0; f < F; ++f) {
      const double u = rng.next();
      float v = f % 3 == 1 ? (float)std::floor(u * 7.0) : (float)(u * 4.0 - 2.0);
      if (rng.next() < nan_frac) v = std::numeric_limits<float>::quiet_NaN();
      X[(size_t)r * F + f] = v;
    }
    const float x0 = X[(size_t)r * F];
    y[r] = ((x0 == x0 ? x0 : 0.0f) + (float)(rng.next() - 0.5) > 0.0f) ? 1 : 0;
  }
}

void grow_case(int64_t n, int F, int max_bin, int depth, double mcw, double nan_frac, bool masked) {
  Lcg rng{0x9e3779b97f4a7c15ull + (uint64_t)n};
  std::vector<float> X, cuts, margin((size_t)n);
  std::vector<uint8_t> y, bins((size_t)n * F), mask((size_t)n);
  std::vector<int32_t> offsets, g((size_t)n), h((size_t)n);
  make_data(rng, n, F, nan_frac, X, y);
  fd::gbdt_cuts_host(X.data(), n, F, F, max_bin, cuts, offsets);
  cuts.push_back(0.0f);
  fd::gbdt_bin_ref_host(X.data(), n, F, F, cuts.data(), offsets.data(), bins.data());
  for (int64_t i = 0; i < n; ++i) {
    margin[i] = (float)(rng.next() * 2.0 - 1.0);
    mask[i] = rng.next() < 0.5 ? 1 : 0;
  }
  fd::gbdt_grad_ref_host(margin.data(), y.data(), n, g.data(), h.data());
  fd_gbdt_params p{};
  p.max_depth = depth;
  p.eta = 0.1;
  p.lambda = 1.0;
  p.min_child_weight = mcw;
  const int64_t cap = (1ll << (depth + 1)) - 1;
  Model m(1, cap);
  int64_t n_nodes = -1;
  fd::gbdt_grow_tree_ref_host(bins.data(), n, F, cuts.data(), offsets.data(), g.data(), h.data(),
                              masked ? mask.data() : nullptr, ~0ull, p, m.model, &n_nodes);
  CHECK(n_nodes >= 1 && n_nodes <= cap);
  check_forest(m, 1, n_nodes, F);
  std::printf("grow %lld x %d, max_bin %d, depth %d%s: %lld nodes\n", (long long)n, F, max_bin, depth,
              masked ? ", row mask" : "", (long long)n_nodes);
}

void fit_case() {
  const int64_t n = 257;
  const int F = 64;
  Lcg rng{12345};
  std::vector<float> X, margins((size_t)n);
  std::vector<uint8_t> y;
  make_data(rng, n, F, 0.1, X, y);
  fd_gbdt_params p{};
  p.n_rounds = 5;
  p.max_depth = 6;
  p.max_bin = 256;
  p.eta = 0.1;
  p.lambda = 1.0;
  p.min_child_weight = 0.1;
  p.subsample = 0.5;
  p.colsample_bytree = 0.3;
  p.base_score = 0.5;
  p.seed = 3;
  const int64_t cap = (int64_t)p.n_rounds * ((1ll << (p.max_depth + 1)) - 1);
  Model m(p.n_rounds, cap);
  int64_t n_nodes = -1;
  fd::gbdt_fit_ref_host(X.data(), y.data(), n, F, F, p, m.model, &n_nodes, margins.data());
  CHECK(n_nodes >= p.n_rounds && n_nodes <= cap);
  check_forest(m, p.n_rounds, n_nodes, F);
  for (float v : margins) CHECK(std::isfinite(v));
  std::printf("fit %lld x %d, %d rounds: %lld nodes\n", (long long)n, F, p.n_rounds, (long long)n_nodes);
}

}  // namespace

int main() {
  grow_case(1, 1, 2, 1, 1.0, 0.0, false);
  grow_case(4099, 64, 256, 10, 0.1, 0.05, false);
  grow_case(4099, 64, 256, 10, 0.1, 0.05, true);
  fit_case();
  std::printf(failures ? "%d check(s) FAILED\n" : "all checks passed\n", failures);
  return failures ? 1 : 0;
}
