// iforest_fit_sanitize.cpp — a stand-alone CPU program (its own main) that drives the host reference of the
// IsolationForest fit (csrc/iforest_fit.hip over csrc/iforest_fit_row.h) under AddressSanitizer + UBSan. It is
// compiled together with iforest_fit.hip by the command in DESIGN §6, runs on the CPU only, is never loaded into
// Python and uses no device.
//
// It fits the smallest and the largest shape of tests/iforest_fit_cases.py (2 rows x 1 feature with psi 2, and 5,000
// rows x 64 features with psi 1024: depth 10, most of each heap empty), a matrix whose row stride is wider than the
// model with a per-tree feature subset and heavy ties, the sampler at both ends of its range and one tree from
// explicit rows with repeats, and checks the invariants a memory error would break: node counts inside the capacity,
// children inside the tree, counts that add up, distinct row ids inside [0, n), a finite offset.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <vector>

#include "fd_internal.h"

// The device path of iforest_fit.hip scores the fit rows through the serving kernels of forest.hip and shap.hip, which
// this program does not link. The host reference never reaches them: these stand-ins only close the link.
namespace fd {
void repack_forest(PackedForest&, const fd_forest_params&, const fd_tree_arrays&) { std::abort(); }
void launch_forest(Engine&, const PackedForest&, const float*, int64_t, int32_t, double*, double*, int32_t*,
                   hipStream_t) {
  std::abort();
}
void shap_forget(PackedForest&) { std::abort(); }
}  // namespace fd

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
  std::vector<double> thr, leaf, count;
  std::vector<uint8_t> dl;
  fd_tree_arrays trees{};
  Model(int n_trees, int64_t cap)
      : off(n_trees + 1), left(cap), right(cap), feature(cap), thr(cap), leaf(cap), count(cap), dl(cap) {
    trees = fd_tree_arrays{n_trees, off.data(), left.data(), right.data(), feature.data(), thr.data(), dl.data(),
                           leaf.data()};
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

void check_forest(const Model& m, int n_trees, int64_t n_nodes, int F, int psi) {
  CHECK(m.off[0] == 0 && m.off[n_trees] == n_nodes);
  for (int t = 0; t < n_trees; ++t) {
    const int64_t o = m.off[t], size = m.off[t + 1] - o;
    CHECK(size >= 1 && m.count[o] == (double)psi);
    for (int64_t i = 0; i < size; ++i) {
      if (m.left[o + i] == -1) {
        CHECK(m.right[o + i] == -1 && m.leaf[o + i] >= 0.0 && std::isfinite(m.leaf[o + i]));
        continue;
      }
      CHECK(m.left[o + i] > i && m.left[o + i] < size && m.right[o + i] == m.left[o + i] + 1 && m.right[o + i] < size);
      CHECK(m.feature[o + i] >= 0 && m.feature[o + i] < F && std::isfinite(m.thr[o + i]));
      CHECK(m.count[o + i] == m.count[o + m.left[o + i]] + m.count[o + m.right[o + i]]);
      CHECK(m.count[o + m.left[o + i]] >= 1.0 && m.count[o + m.right[o + i]] >= 1.0);
    }
  }
}

std::vector<float> make_data(Lcg& rng, int64_t n, int ld, int F) {
  std::vector<float> X((size_t)n * ld, 1e30f);  // (the columns past F are never read into a tree)
  for (int64_t r = 0; r < n; ++r)
    for (int f = 0; f < F; ++f) {
      const double u = rng.next();
      X[(size_t)r * ld + f] = f % 3 == 1 ? (float)std::floor(u * 3.0) : f % 7 == 5 ? 2.5f : (float)(u * 4.0 - 2.0);
    }
  return X;
}

void fit_case(int64_t n, int ld, int F, int trees, int max_samples, double max_features, double contamination) {
  Lcg rng{0x9e3779b97f4a7c15ull + (uint64_t)n};
  const std::vector<float> X = make_data(rng, n, ld, F);
  fd_iforest_fit_params p{};
  p.n_estimators = trees;
  p.max_samples = max_samples;
  p.max_features = max_features;
  p.contamination = contamination;
  p.seed = 7;
  fd::iforest_fit_check(p, n, ld, F);
  const int64_t cap = fd::iforest_fit_capacity(p, n);
  const int psi = fd::iforest_fit_psi(p, n);
  Model m(trees, cap);
  fd_forest_params forest{};
  int64_t n_nodes = -1;
  fd::iforest_fit_ref_host(X.data(), n, ld, F, p, m.trees, m.count.data(), forest, &n_nodes);
  CHECK(n_nodes >= trees && n_nodes <= cap);
  check_forest(m, trees, n_nodes, F, psi);
  CHECK(forest.kind == FD_FOREST_SKLEARN_IFOREST && forest.num_feature == F && forest.if_denominator > 0.0);
  CHECK(std::isfinite(forest.if_offset) && forest.if_offset < 0.0 && forest.if_offset > -1.0);
  if (contamination == 0.0) CHECK(forest.if_offset == -0.5);
  std::printf("fit %lld x %d (ld %d), %d trees, psi %d: %lld nodes of %lld, offset %.17g\n", (long long)n, F, ld, trees,
              psi, (long long)n_nodes, (long long)cap, forest.if_offset);
}

void sample_case(int64_t n, int max_samples, int tree) {
  fd_iforest_fit_params p{};
  p.n_estimators = 1;
  p.max_samples = max_samples;
  p.max_features = 1.0;
  p.seed = 0xffffffffffffffffull;
  std::vector<int32_t> rows(1024, -1);
  int32_t psi = 0;
  fd::iforest_fit_sample_ref_host(n, p, tree, rows.data(), &psi);
  CHECK(psi == fd::iforest_fit_psi(p, n));
  std::set<int32_t> seen;
  for (int j = 0; j < psi; ++j) {
    CHECK(rows[j] >= 0 && (int64_t)rows[j] < n);
    seen.insert(rows[j]);
  }
  CHECK((int)seen.size() == psi);
  std::printf("sample n %lld, tree %d: %d distinct rows\n", (long long)n, tree, psi);
}

void grow_case() {
  const int64_t n = 300;
  const int F = 5;
  Lcg rng{99};
  const std::vector<float> X = make_data(rng, n, F, F);
  std::vector<int32_t> rows(1024);
  for (int i = 0; i < 1024; ++i) rows[i] = i % 300;  // every row three or four times
  fd_iforest_fit_params p{};
  p.seed = 5;
  Model m(1, 2047);
  int64_t n_nodes = -1;
  fd::iforest_fit_grow_tree_ref_host(X.data(), n, F, F, rows.data(), 1024, 0x15, p, 3, m.trees, m.count.data(),
                                     &n_nodes);
  CHECK(n_nodes >= 1 && n_nodes <= 2047);
  check_forest(m, 1, n_nodes, F, 1024);
  for (int64_t i = 0; i < n_nodes; ++i)
    if (m.left[i] != -1) CHECK(m.feature[i] == 0 || m.feature[i] == 2 || m.feature[i] == 4);
  std::printf("grow 1024 rows with repeats, features {0, 2, 4}: %lld nodes\n", (long long)n_nodes);
}

}  // namespace

int main() {
  fit_case(2, 1, 1, 3, 0, 1.0, 0.5);
  fit_case(5000, 64, 64, 4, 1024, 1.0, 0.05);
  fit_case(700, 40, 33, 5, 0, 0.5, 0.1);
  fit_case(100, 6, 6, 300, 16, 1.0, 0.0);
  sample_case(2, 0, 0);
  sample_case(2147483647ll, 1024, 65535);
  grow_case();
  std::printf(failures ? "%d check(s) FAILED\n" : "all checks passed\n", failures);
  return failures ? 1 : 0;
}
