// graph_row.h — the transaction-network features' window rule and f64 epilogue, shared by the kernels (graph.hip) and
// the pure host form (fd_graph_features_host). Self-contained (no HIP, no engine headers) so the host form also
// compiles into a stand-alone program.
// Reference: GraphFraudDetector (ml/models/graph_neural_network.py)
//   _add_transaction_to_history   :228-242   truncate to history[-H//2:] when len >= H, then append
//   _calculate_network_features   :338-392   the five features over the history, the new transaction included
// Declared rule (DESIGN.md "Transaction-network features"): transaction g (0-based since init / clear) sees the
// inclusive index range [s(g), g]; prev(k) is the latest earlier entry with k's (card_key, merchant) pair; entry k is
// "first for s" when prev(k) < s. Over the window: cntU / S = count / cents of the user's entries, dM = first entries
// of the user with a merchant, dU = first entries at the merchant with a user, T = first entries whose merchant is one
// of the user's. Arithmetic is f64 with FP contraction off and the reference's operation order.
#pragma once

#include <cstdint>
#include <unordered_map>
#include <vector>

#if defined(__HIPCC__)
#define FD_GRAPH_HD __host__ __device__ __forceinline__
#else
#define FD_GRAPH_HD inline
#endif

#define FD_GRAPH_COLS 5  // user_centrality, merchant_centrality, clustering_coefficient, path_length_anomaly,
                         // community_anomaly (FD_GRAPH_FEATURES)

namespace fd {

constexpr int kGraphMinHistory = 2;       // H = 1 keeps ceil(1/2) = 1 = H entries: the period H - keep is 0
constexpr int kGraphMaxHistory = 65536;

// s(g): the first index transaction g still sees. keep = ceil(H/2) entries survive a truncation, which happens every
// P = H - keep appends once the history has reached H.
FD_GRAPH_HD int64_t graph_window_start(int64_t g, int64_t H) {
  if (g < H) return 0;
  const int64_t keep = (H + 1) / 2, P = H - keep;
  return H + (g - H) / P * P - keep;
}

// Python's min(a, b): a unless b < a
FD_GRAPH_HD double graph_py_min(double a, double b) { return (b < a) ? b : a; }

// Columns 0, 1, 3, 4 of one row (column 2 is graph_cluster_value). null_row: the user or the merchant is null.
FD_GRAPH_HD void graph_row(bool null_row, int64_t cntU, int64_t S, int64_t dM, int64_t dU, int64_t cents,
                           bool first, double* out) {
#pragma clang fp contract(off)
  out[0] = out[1] = out[2] = out[3] = out[4] = 0.0;
  if (null_row) return;
  out[0] = graph_py_min((double)dM / 10.0, 1.0);
  out[1] = graph_py_min((double)dU / 100.0, 1.0);
  const double avg = ((double)S / 100.0) / (double)cntU;  // cntU >= 1: the window holds the transaction itself
  if (avg > 0) {
    const double d = (double)cents / 100.0 - avg;
    out[3] = graph_py_min((d < 0 ? -d : d) / avg, 1.0);
  }
  out[4] = first ? 1.0 : 0.0;
}

// clustering_coefficient from T and dM (dM > 1)
FD_GRAPH_HD double graph_cluster_value(int64_t T, int64_t dM) {
#pragma clang fp contract(off)
  return graph_py_min((double)(T - dM) / (double)(dM * 10), 1.0);
}

// A whole stream from index 0 on the host: the declared rule by direct scans of each window (O(n H)).
inline void graph_features_stream_host(const uint64_t* key, const int32_t* merchant, const int64_t* cents, int64_t n,
                                       int64_t H, double* out) {
  struct PairHash {
    size_t operator()(const std::pair<uint64_t, int32_t>& p) const {
      uint64_t x = p.first * 0x9e3779b97f4a7c15ull ^ ((uint64_t)(uint32_t)p.second * 0xc2b2ae3d27d4eb4full);
      x ^= x >> 29;
      return (size_t)x;
    }
  };
  std::unordered_map<std::pair<uint64_t, int32_t>, int64_t, PairHash> last;  // pair -> its latest index
  std::unordered_map<int32_t, int64_t> mark;                                // merchant -> the row it was marked for
  std::vector<int64_t> prev((size_t)n);
  last.reserve((size_t)n);
  for (int64_t g = 0; g < n; ++g) {
    const auto pr = std::make_pair(key[g], merchant[g]);
    auto it = last.find(pr);
    prev[(size_t)g] = it == last.end() ? -1 : it->second;
    last[pr] = g;
    const int64_t s = graph_window_start(g, H);
    const uint64_t u = key[g];
    const int32_t m = merchant[g];
    double* row = out + g * FD_GRAPH_COLS;
    const bool null_row = u == 0 || m < 0;
    int64_t cntU = 0, S = 0, dM = 0, dU = 0;
    if (!null_row)
      for (int64_t k = s; k <= g; ++k) {
        const bool first = prev[(size_t)k] < s;
        if (key[k] == u) {
          ++cntU;
          S += cents[k];
          if (first && merchant[k] >= 0) {
            ++dM;
            mark[merchant[k]] = g;
          }
        }
        if (merchant[k] == m && first && key[k] != 0) ++dU;
      }
    graph_row(null_row, cntU, S, dM, dU, cents[g], prev[(size_t)g] < s, row);
    if (!null_row && dM > 1) {
      int64_t T = 0;
      for (int64_t k = s; k <= g; ++k)
        if (prev[(size_t)k] < s && merchant[k] >= 0) {
          auto mk = mark.find(merchant[k]);
          if (mk != mark.end() && mk->second == g) ++T;
        }
      row[2] = graph_cluster_value(T, dM);
    }
  }
}

}  // namespace fd
