// gbdt_eval_sanitize.cpp — a stand-alone CPU program (its own main) that drives the host reference of the watched GBDT
// fit (what fd_gbdt_fit_eval_ref_host and fd_gbdt_metric_ref_host call: fd::gbdt_fit_ref_host with an fd_gbdt_eval and
// fd::gbdt_metric_ref_host, csrc/gbdt.hip over csrc/gbdt_row.h; the two entry points themselves live in engine.hip
// with the rest of the C ABI, and are restated below in their few lines) under AddressSanitizer + UBSan. It is
// compiled together with gbdt.hip by the command in DESIGN §6, runs on the CPU only, is never loaded into Python and
// uses no device.
//
// It runs the metric on 2 rows and on 4,099 + 5,000 rows with one large tie group, signed zeros, infinities and NaNs,
// and watched fits at the smallest and the largest shape of the tests (65 x 1 with a 2-row eval set; 4,099 x 33 with
// 1,025 eval rows, 40 rounds, a class weight, both metrics, with and without early stopping), and checks what a
// memory error would break: curve entries inside [0, 1], rounds_run = best_iteration + k + 1 after a stop, tree
// offsets written for exactly the rounds that ran.
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
      : off(n_trees + 1, -1), left(cap), right(cap), feature(cap), thr(cap), leaf(cap), sh(cap), lc(cap), bw(cap),
        dl(cap) {
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

// the bodies of the two entry points (engine.hip), without the engine
int fit_eval_ref_host(const float* X, const uint8_t* y, int64_t n, int32_t ld, int32_t F, const fd_gbdt_params* p,
                      fd_gbdt_eval* ev, fd_gbdt_model* out, int64_t* n_nodes, float* margins) {
  try {
    if (!out) {
      fd::gbdt_check_params(*p, n, F, true);
      *n_nodes = (int64_t)p->n_rounds * ((1ll << (p->max_depth + 1)) - 1);
      return FD_OK;
    }
    fd::gbdt_fit_ref_host(X, y, n, ld, F, *p, *out, n_nodes, margins, ev);
    return FD_OK;
  } catch (const fd::Error& e) {
    return e.code;
  }
}

int metric_ref_host(const float* margins, const uint8_t* y, int64_t n, int32_t metric, double* out) {
  try {
    fd::gbdt_check_metric_labels(y, n, metric);
    *out = fd::gbdt_metric_ref_host(margins, y, n, metric);
    return FD_OK;
  } catch (const fd::Error& e) {
    return e.code;
  }
}

void make_data(Lcg& rng, int64_t n, int F, std::vector<float>& X, std::vector<uint8_t>& y) {
  X.resize((size_t)n * F);
  y.resize((size_t)n);
  for (int64_t r = 0; r < n; ++r) {
    for (int f = 0; f < F; ++f) {
      const double u = rng.next();
      float v = f % 3 == 1 ? (float)std::floor(u * 7.0) : (float)(u * 4.0 - 2.0);
      if (F > 1 && rng.next() < 0.03) v = std::numeric_limits<float>::quiet_NaN();
      X[(size_t)r * F + f] = v;
    }
    const float x0 = X[(size_t)r * F];
    y[r] = ((x0 == x0 ? x0 : 0.0f) + (float)(rng.next() - 0.5) > 0.0f) ? 1 : 0;
  }
  y[0] = 0;  // both classes, whatever was drawn
  y[(size_t)n - 1] = 1;
}

void metric_case(int64_t n_other) {
  Lcg rng{77 + (uint64_t)n_other};
  std::vector<float> m;
  std::vector<uint8_t> y;
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  const float special[] = {0.0f, -0.0f, inf, -inf, nan, -nan, 1e-45f, -1e-45f};
  for (int64_t i = 0; i < n_other; ++i) m.push_back(i < 8 ? special[i] : (float)(rng.next() * 6.0 - 3.0));
  if (n_other > 2) m.insert(m.end(), 5000, 0.125f);
  for (size_t i = 0; i < m.size(); ++i) y.push_back(rng.next() < 0.4 ? 1 : 0);
  y[0] = 0;
  y[1] = 1;
  for (int metric : {FD_GBDT_METRIC_AUC, FD_GBDT_METRIC_ERROR}) {
    double v = -1.0;
    CHECK(metric_ref_host(m.data(), y.data(), (int64_t)m.size(), metric, &v) == FD_OK);
    CHECK(v >= 0.0 && v <= 1.0);
    std::printf("metric %d over %zu rows: %.6f\n", metric, m.size(), v);
  }
  double v;
  std::vector<uint8_t> ones(m.size(), 1);
  CHECK(metric_ref_host(m.data(), ones.data(), (int64_t)m.size(), FD_GBDT_METRIC_AUC, &v) ==
        FD_ERR_INVALID_ARG);
}

void fit_case(int64_t n, int F, int depth, int64_t n_eval, int rounds, int metric, int k, double w) {
  Lcg rng{12345 + (uint64_t)n};
  std::vector<float> X, Xe, margins((size_t)n), best((size_t)n), emargins((size_t)n_eval);
  std::vector<uint8_t> y, ye;
  make_data(rng, n, F, X, y);
  make_data(rng, n_eval, F, Xe, ye);
  fd_gbdt_params p{};
  p.n_rounds = rounds;
  p.max_depth = depth;
  p.max_bin = 256;
  p.eta = 0.3;
  p.lambda = 1.0;
  p.min_child_weight = 0.1;
  p.subsample = 0.8;
  p.colsample_bytree = 0.8;
  p.base_score = 0.5;
  p.seed = 3;
  std::vector<double> curve((size_t)rounds, -1.0);
  fd_gbdt_eval ev{};
  ev.X = Xe.data();
  ev.y = ye.data();
  ev.n = n_eval;
  ev.ld = F;
  ev.metric = metric;
  ev.early_stopping_rounds = k;
  ev.scale_pos_weight = w;
  ev.metric_out = curve.data();
  ev.margins = emargins.data();
  ev.best_margins = best.data();
  int64_t cap = -1;
  CHECK(fit_eval_ref_host(X.data(), y.data(), n, F, F, &p, nullptr, nullptr, &cap, nullptr) == FD_OK);
  CHECK(cap == (int64_t)rounds * ((1ll << (depth + 1)) - 1));
  Model m(rounds, cap);
  int64_t n_nodes = -1;
  CHECK(fit_eval_ref_host(X.data(), y.data(), n, F, F, &p, &ev, &m.model, &n_nodes, margins.data()) == FD_OK);
  const int run = ev.rounds_run, bi = ev.best_iteration;
  CHECK(run >= 1 && run <= rounds && bi >= 0 && bi < run);
  CHECK(run == rounds || (k > 0 && run == bi + k + 1));
  CHECK(m.off[0] == 0 && m.off[run] == n_nodes && n_nodes <= cap);
  for (int t = run + 1; t <= rounds; ++t) CHECK(m.off[t] == -1);  // nothing written past the rounds that ran
  for (int t = 0; t < rounds; ++t) CHECK(t < run ? (curve[t] >= 0.0 && curve[t] <= 1.0) : curve[t] == -1.0);
  for (float v : margins) CHECK(std::isfinite(v));
  for (float v : emargins) CHECK(std::isfinite(v));
  for (float v : best) CHECK(std::isfinite(v));
  std::printf("fit %lld x %d, %lld eval rows, metric %d, k %d, w %g: %d of %d rounds, best %d, %lld nodes\n",
              (long long)n, F, (long long)n_eval, metric, k, w, run, rounds, bi, (long long)n_nodes);
}

void argument_cases() {
  std::vector<float> X(8, 0.5f);
  std::vector<uint8_t> y{0, 1, 0, 1, 0, 1, 0, 1};
  fd_gbdt_params p{};
  p.n_rounds = 2;
  p.max_depth = 2;
  p.max_bin = 16;
  p.eta = 0.1;
  p.lambda = 1.0;
  p.min_child_weight = 1.0;
  p.subsample = p.colsample_bytree = 1.0;
  p.base_score = 0.5;
  Model m(2, 14);
  int64_t nn = 0;
  fd_gbdt_eval ev{};
  ev.scale_pos_weight = 1.0;
  ev.early_stopping_rounds = 2;  // without an eval set
  CHECK(fit_eval_ref_host(X.data(), y.data(), 8, 1, 1, &p, &ev, &m.model, &nn, nullptr) == FD_ERR_INVALID_ARG);
  ev.early_stopping_rounds = 0;
  ev.scale_pos_weight = 65.0;
  CHECK(fit_eval_ref_host(X.data(), y.data(), 8, 1, 1, &p, &ev, &m.model, &nn, nullptr) == FD_ERR_INVALID_ARG);
  ev.scale_pos_weight = 2.0;  // the weight alone
  CHECK(fit_eval_ref_host(X.data(), y.data(), 8, 1, 1, &p, &ev, &m.model, &nn, nullptr) == FD_OK);
  CHECK(ev.rounds_run == 2 && ev.best_iteration == -1);
}

}  // namespace

int main() {
  metric_case(2);
  metric_case(4099);
  fit_case(65, 1, 10, 2, 3, FD_GBDT_METRIC_AUC, 0, 1.0);
  fit_case(65, 1, 10, 2, 3, FD_GBDT_METRIC_ERROR, 1, 0.25);
  fit_case(4099, 33, 6, 1025, 40, FD_GBDT_METRIC_AUC, 0, 19.0);
  fit_case(4099, 33, 6, 1025, 40, FD_GBDT_METRIC_AUC, 2, 64.0);
  fit_case(4099, 33, 6, 1025, 40, FD_GBDT_METRIC_ERROR, 2, 1.0);
  argument_cases();
  std::printf(failures ? "%d check(s) FAILED\n" : "all checks passed\n", failures);
  return failures ? 1 : 0;
}
