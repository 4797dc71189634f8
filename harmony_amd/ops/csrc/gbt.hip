// K10 — GBT level-wise histogram build.
//
// Replaces the torch scatter_add pair in the tree builder (reference
// GBTTrainer.java:244+ does per-value exact scans on the CPU; the GPU
// histogram method is the standard redesign). One workgroup owns a
// (sample-tile, feature-chunk) and accumulates (count, residual-sum)
// histograms for ALL of the level's nodes in LDS with fp32 LDS atomics,
// then merges once into the global [n_nodes, F, num_bins] arrays. The
// feature chunk is sized so the per-WG LDS stays <= 64 KB (deeper levels ->
// narrower chunks, more grid.y), down to one feature at n_nodes * nb = 8192;
// wider levels go to K10w (gbt_hist_wide.hip), which groups the rows by node.
//
// Why LDS privatization: the torch path's scatter_add issues B*F global
// atomics into HBM; here each WG's collisions resolve in LDS (~100x the
// atomic throughput) and HBM sees one atomicAdd per non-empty LDS entry.

#include "hip_common.h"

namespace {

constexpr int HIST_THREADS = 256;
constexpr int LDS_ENTRIES = 8192;  // (cnt,sum) pairs -> 64 KB LDS

__global__ void gbt_hist_kernel(
    const int* __restrict__ bins,    // [B, F]
    const float* __restrict__ resid, // [B]
    const int* __restrict__ node,    // [B] level-local node idx
    float* __restrict__ cnt,         // [n_nodes, F, nb]
    float* __restrict__ sum,         // [n_nodes, F, nb]
    int B, int F, int nb, int n_nodes, int fc, int tile) {
  extern __shared__ float lds[];
  const int f0 = blockIdx.y * fc;
  const int fcw = min(fc, F - f0);          // chunk width at the tail
  const int nent = n_nodes * fcw * nb;
  float* lcnt = lds;
  float* lsum = lds + nent;
  for (int i = threadIdx.x; i < 2 * nent; i += blockDim.x) lds[i] = 0.f;
  __syncthreads();

  const int start = blockIdx.x * tile;
  const int end = min(B, start + tile);
  for (int i = start + threadIdx.x; i < end; i += blockDim.x) {
    const int nd = node[i];
    const float r = resid[i];
    const int* row = bins + (long)i * F + f0;
    const int base = nd * fcw * nb;
    for (int j = 0; j < fcw; ++j) {
      const int b = row[j];
      atomicAdd(&lcnt[base + j * nb + b], 1.f);
      atomicAdd(&lsum[base + j * nb + b], r);
    }
  }
  __syncthreads();

  for (int i = threadIdx.x; i < nent; i += blockDim.x) {
    const float c = lcnt[i];
    if (c == 0.f) continue;
    const int nd = i / (fcw * nb);
    const int rem = i - nd * fcw * nb;
    const long g = ((long)nd * F + f0 + rem / nb) * nb + (rem % nb);
    atomicAdd(&cnt[g], c);
    atomicAdd(&sum[g], lsum[i]);
  }
}

}  // namespace

// K10w (gbt_hist_wide.hip): the same histogram for n_nodes * nb > 8192.
void gbt_hist_wide_launch(const char* op, const torch::Tensor& bins,
                          const torch::Tensor& resid,
                          const torch::Tensor& node, torch::Tensor& cnt,
                          torch::Tensor& sum);

void gbt_hist(torch::Tensor bins, torch::Tensor resid, torch::Tensor node,
              torch::Tensor cnt, torch::Tensor sum) {
  check_tensor(__func__, bins, "bins", torch::kInt32, {-1, -1});
  const int B = bins.size(0), F = bins.size(1);
  check_tensor(__func__, resid, "resid", torch::kFloat32, {B});
  check_tensor(__func__, node, "node", torch::kInt32, {B});
  check_tensor(__func__, cnt, "cnt", torch::kFloat32, {-1, F, -1});
  const int n_nodes = cnt.size(0), nb = cnt.size(2);
  check_tensor(__func__, sum, "sum", torch::kFloat32, {n_nodes, F, nb});
  check_below_2_31(__func__, {{"B", bins.size(0)}, {"F", bins.size(1)}});
  TORCH_CHECK(n_nodes >= 1 && nb >= 1, __func__,
              ": cnt needs n_nodes, nb >= 1");
  TORCH_CHECK(nb <= LDS_ENTRIES, __func__, ": more than ", LDS_ENTRIES,
              " bins, a node too wide for LDS (use torch fallback)");
  check_below_2_31(__func__, {{"n_nodes", cnt.size(0)}});
  check_on_device(__func__, {bins, resid, node, cnt, sum});
  if (B == 0 || F == 0) return;
  if ((long)n_nodes * nb > LDS_ENTRIES) {
    // the level's nodes do not fit one workgroup's LDS together: K10w
    gbt_hist_wide_launch(__func__, bins, resid, node, cnt, sum);
    return;
  }
  const int fc = std::min((long)F, (long)(LDS_ENTRIES / (n_nodes * nb)));
  const int n_chunks = (F + fc - 1) / fc;
  // enough sample tiles to fill the chip once chunks are counted in
  const int want = std::max(1, 512 / n_chunks);
  const int tile = std::max((B + want - 1) / want, HIST_THREADS);
  const int tiles = (B + tile - 1) / tile;
  const size_t lds = (size_t)2 * n_nodes * fc * nb * sizeof(float);
  hipLaunchKernelGGL(gbt_hist_kernel, dim3(tiles, n_chunks),
                     dim3(HIST_THREADS), lds, current_stream(),
                     bins.data_ptr<int>(), resid.data_ptr<float>(),
                     node.data_ptr<int>(), cnt.data_ptr<float>(),
                     sum.data_ptr<float>(), B, F, nb, n_nodes, fc, tile);
}
