// Micro-benchmark: steady-state time per 16-row tile and wave of the MLP head's reference-shape kernel
// (csrc/mlp.hip mlp_ref_kernel, included as source), with the rows in HBM (ld 64) and with every row read from the
// same 256 bytes (ld 0: no memory traffic), at 1 / 4 / 16 / 32 tiles per wave on a 256-workgroup grid; HIP events,
// the best of 5 launches. The slope over tiles per wave is the per-tile cost (DESIGN §3 "The MLP head").
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -Iinclude -Irealtime-fraud-detection_amd/csrc \
//       tools/micro/mlp_tiles.hip -o tools/micro/mlp_tiles && ./tools/micro/mlp_tiles
#include "../../realtime-fraud-detection_amd/csrc/mlp.hip"

#include <cstdio>

namespace fd {
Engine::Timed* Engine::next_event_pair(int) { return nullptr; }  // engine.hip defines it in the library; unused here
}  // namespace fd
using namespace fd;

#define CK(call)                                                 \
  do {                                                           \
    if ((call) != hipSuccess) {                                  \
      printf("%s failed\n", #call);                              \
      return 1;                                                  \
    }                                                            \
  } while (0)

int main() {
  fd_mlp_params p{};
  p.n_layers = 3;
  p.dims[0] = p.dims[1] = p.dims[2] = 64;
  p.dims[3] = 2;
  std::vector<float> w0(4096, 0.01f), w1(4096, 0.02f), w2(128, 0.03f), b(64, 0.1f);
  p.weight[0] = w0.data();
  p.weight[1] = w1.data();
  p.weight[2] = w2.data();
  p.bias[0] = p.bias[1] = p.bias[2] = b.data();
  const std::vector<uint32_t> blob = pack_mlp_host(p);
  uint32_t* dblob;
  CK(hipMalloc(&dblob, blob.size() * 4));
  CK(hipMemcpy(dblob, blob.data(), blob.size() * 4, hipMemcpyHostToDevice));
  const int64_t nmax = 16ll * 1024 * 32;  // 1024 waves x 32 tiles of 16 rows
  float* dX;
  double* dp;
  CK(hipMalloc(&dX, nmax * 64 * 4));
  CK(hipMemset(dX, 0, nmax * 64 * 4));
  CK(hipMalloc(&dp, nmax * 8));
  hipEvent_t a, e;
  CK(hipEventCreate(&a));
  CK(hipEventCreate(&e));
  for (int ld : {64, 0})
    for (int T : {1, 4, 16, 32}) {
      const int64_t n = 16ll * 1024 * T;
      float best = 1e9f;
      for (int rep = 0; rep < 6; ++rep) {
        CK(hipEventRecord(a, 0));
        hipLaunchKernelGGL(mlp_ref_kernel, dim3(256), dim3(256), 0, 0, dX, n, ld, dblob, 1, dp);
        CK(hipEventRecord(e, 0));
        CK(hipEventSynchronize(e));
        float ms;
        CK(hipEventElapsedTime(&ms, a, e));
        if (rep && ms < best) best = ms;
      }
      printf("ld %2d tiles/wave %2d: %.2f us\n", ld, T, best * 1e3);
    }
  CK(hipDeviceSynchronize());
  return 0;
}
