// K10s — GBT level histogram over a binned SPARSE batch (SparseBins).
//
// Reference: GBTETDataParser builds every sample with createSparse, so the
// reference GBT trains on sparse vectors. Dense K10 (gbt.hip) walks all
// B * F cells of a batch at every tree level; here a level costs the batch's
// non-zeros plus one [n_nodes, nb] slab per feature PRESENT in the batch.
//
// Shape: K10's LDS privatisation turned from sample tiles to column ranges.
// One workgroup owns fc = LDS_ENTRIES / (n_nodes * nb) consecutive present
// features. The column side of SparseBins stores the entries grouped by
// feature, so the workgroup's entries are ONE contiguous range
// feat_ptr[f0] .. feat_ptr[f0 + fcw]: row, bin and compact feature index are
// read coalesced, node[row] and resid[row] are gathered, and the entry is
// added into the (node, feature, bin) cell in LDS with LDS atomics.
//
// The implied zeros are never visited. After the barrier, for every
// (node, feature) the workgroup sums the cells it holds and adds
// node_cnt - sum_cnt and node_sum - sum_s, the share of the samples that have
// no entry in that column, into the feature's zero bin (the bin the value 0.0
// falls in; 0 for a categorical feature). node_cnt / node_sum are the
// per-node totals of the level, one tiny scatter done by the caller.
//
// The workgroup is the only writer of its features, so the slab goes to
// global memory with plain stores (16 bytes per lane when nb % 4 == 0): no
// global atomics, and the output needs no zero fill.
//
// LDS layout [node][feature][bin], cnt then sum: a node's cells of the
// workgroup's features are contiguous in LDS AND in the output
// [n_nodes, nf, nb], so the write-out is a straight copy per node. The
// fix-up walks the nb bins of one (node, feature) per lane, starting at a
// lane-dependent bin: with nb a multiple of 32 the lanes of a half-wave then
// sit on 32 different banks, where a common start would put them all on one.
//
// Malformed indices (row outside [0, B), bin outside [0, nb), node outside
// [0, n_nodes), feature index outside the workgroup's range, bounds outside
// [0, nnz]) are skipped or clamped, never dereferenced.

#include "hip_common.h"

namespace {

constexpr int HS_THREADS = 256;
constexpr int HS_LDS_ENTRIES = 8192;  // (cnt,sum) pairs -> 64 KB LDS, as K10
constexpr int HS_UNROLL = 4;          // entries in flight per thread

template <bool VEC4>
__global__ __launch_bounds__(HS_THREADS) void gbt_hist_sparse_kernel(
    const int64_t* __restrict__ feat_ptr,  // [nf+1]
    const int* __restrict__ feat_row,      // [nnz]
    const int* __restrict__ feat_bin,      // [nnz]
    const int* __restrict__ feat_idx,      // [nnz] compact feature index
    const int* __restrict__ zero_bin,      // [nf]
    const float* __restrict__ resid,       // [B]
    const int* __restrict__ node,          // [B] level-local node idx
    const float* __restrict__ node_cnt,    // [n_nodes]
    const float* __restrict__ node_sum,    // [n_nodes]
    float* __restrict__ cnt,               // [n_nodes, nf, nb]
    float* __restrict__ sum,               // [n_nodes, nf, nb]
    int B, int nf, int nb, int n_nodes, int fc, int64_t nnz) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x;
  const int f0 = blockIdx.x * fc;
  const int fcw = min(fc, nf - f0);     // chunk width at the tail
  const int slab = fcw * nb;            // one node's cells
  const int nent = n_nodes * slab;      // <= HS_LDS_ENTRIES
  float* lcnt = lds;
  float* lsum = lds + nent;
  if (VEC4) {
    float4* z = reinterpret_cast<float4*>(lds);
    for (int i = tid; i < nent / 2; i += HS_THREADS)
      z[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  } else {
    for (int i = tid; i < 2 * nent; i += HS_THREADS) lds[i] = 0.f;
  }
  __syncthreads();

  int64_t e0 = feat_ptr[f0], e1 = feat_ptr[f0 + fcw];
  e0 = e0 < 0 ? 0 : (e0 > nnz ? nnz : e0);
  e1 = e1 < 0 ? 0 : (e1 > nnz ? nnz : e1);
  // HS_UNROLL entries per thread and trip: the coalesced loads of all of
  // them, then the gathers they address, then the LDS atomics, so a long
  // entry range does not pay one global round trip per entry
  for (int64_t e = e0 + tid; e < e1; e += HS_THREADS * HS_UNROLL) {
    int row[HS_UNROLL], cell[HS_UNROLL], nd[HS_UNROLL];
    float r[HS_UNROLL];
#pragma unroll
    for (int u = 0; u < HS_UNROLL; ++u) {
      const int64_t eu = e + (int64_t)u * HS_THREADS;
      const bool in = eu < e1;
      row[u] = in ? feat_row[eu] : -1;
      const int b = in ? feat_bin[eu] : 0;
      const int j = in ? feat_idx[eu] - f0 : 0;
      if ((unsigned)row[u] >= (unsigned)B || (unsigned)b >= (unsigned)nb ||
          (unsigned)j >= (unsigned)fcw)
        row[u] = -1;
      cell[u] = j * nb + b;
    }
#pragma unroll
    for (int u = 0; u < HS_UNROLL; ++u) {
      nd[u] = node[row[u] < 0 ? 0 : row[u]];
      r[u] = resid[row[u] < 0 ? 0 : row[u]];
    }
#pragma unroll
    for (int u = 0; u < HS_UNROLL; ++u) {
      if (row[u] >= 0 && (unsigned)nd[u] < (unsigned)n_nodes) {
        const int c = nd[u] * slab + cell[u];
        atomicAdd(&lcnt[c], 1.f);
        atomicAdd(&lsum[c], r[u]);
      }
    }
  }
  __syncthreads();

  // implied zeros: what the node holds minus what the column's entries gave
  const int npair = n_nodes * fcw;
  for (int p = tid; p < npair; p += HS_THREADS) {
    const int nd = p / fcw;
    const int j = p - nd * fcw;
    float* c = lcnt + p * nb;
    float* s = lsum + p * nb;
    float sc = 0.f, ss = 0.f;
    int b = p % nb;
    for (int q = 0; q < nb; ++q) {
      sc += c[b];
      ss += s[b];
      if (++b == nb) b = 0;
    }
    int zb = zero_bin[f0 + j];
    zb = zb < 0 ? 0 : (zb >= nb ? nb - 1 : zb);
    c[zb] += node_cnt[nd] - sc;
    s[zb] += node_sum[nd] - ss;
  }
  __syncthreads();

  if (VEC4) {
    // nb % 4 == 0: slab and every output offset are multiples of 4 floats
    for (int i = tid * 4; i < nent; i += HS_THREADS * 4) {
      const int nd = i / slab;
      const int64_t g = ((int64_t)nd * nf + f0) * nb + (i - nd * slab);
      *reinterpret_cast<float4*>(cnt + g) =
          *reinterpret_cast<const float4*>(lcnt + i);
      *reinterpret_cast<float4*>(sum + g) =
          *reinterpret_cast<const float4*>(lsum + i);
    }
  } else {
    for (int i = tid; i < nent; i += HS_THREADS) {
      const int nd = i / slab;
      const int64_t g = ((int64_t)nd * nf + f0) * nb + (i - nd * slab);
      cnt[g] = lcnt[i];
      sum[g] = lsum[i];
    }
  }
}

constexpr int64_t kI31 = (int64_t)1 << 31;

}  // namespace

// The widest level (n_nodes * nb) K10s keeps in LDS.
int64_t gbt_hist_sparse_max_cells() { return HS_LDS_ENTRIES; }

// One tree level's histograms over the present features of a SparseBins.
// Returns {cnt, sum}, each float32 [n_nodes, nf, nb], in feat_ids order.
std::vector<torch::Tensor> gbt_hist_sparse(
    torch::Tensor feat_ptr, torch::Tensor feat_row, torch::Tensor feat_bin,
    torch::Tensor feat_idx, torch::Tensor zero_bin, torch::Tensor resid,
    torch::Tensor node, torch::Tensor node_cnt, torch::Tensor node_sum,
    int64_t nb) {
  CHECK_IN(feat_ptr); CHECK_IN(feat_row); CHECK_IN(feat_bin);
  CHECK_IN(feat_idx); CHECK_IN(zero_bin); CHECK_IN(resid); CHECK_IN(node);
  CHECK_IN(node_cnt); CHECK_IN(node_sum);
  TORCH_CHECK(feat_ptr.dtype() == torch::kInt64 && feat_ptr.dim() == 1 &&
              feat_ptr.numel() >= 1, "feat_ptr must be int64 [nf+1]");
  const int64_t nf = feat_ptr.numel() - 1, nnz = feat_row.numel();
  const int64_t B = resid.numel(), n_nodes = node_cnt.numel();
  TORCH_CHECK(feat_row.dtype() == torch::kInt32 && feat_row.dim() == 1 &&
              feat_bin.dtype() == torch::kInt32 && feat_bin.dim() == 1 &&
              feat_idx.dtype() == torch::kInt32 && feat_idx.dim() == 1 &&
              feat_bin.numel() == nnz && feat_idx.numel() == nnz,
              "feat_row, feat_bin, feat_idx must be int32 [nnz]");
  TORCH_CHECK(zero_bin.dtype() == torch::kInt32 && zero_bin.dim() == 1 &&
              zero_bin.numel() == nf, "zero_bin must be int32 [nf]");
  TORCH_CHECK(resid.dtype() == torch::kFloat32 && resid.dim() == 1,
              "resid must be float32 [B]");
  TORCH_CHECK(node.dtype() == torch::kInt32 && node.dim() == 1 &&
              node.numel() == B, "node must be int32 [B]");
  TORCH_CHECK(node_cnt.dtype() == torch::kFloat32 && node_cnt.dim() == 1 &&
              node_sum.dtype() == torch::kFloat32 && node_sum.dim() == 1 &&
              node_sum.numel() == n_nodes,
              "node_cnt and node_sum must be float32 [n_nodes]");
  TORCH_CHECK(nb >= 1 && n_nodes >= 1, "gbt_hist_sparse: nb, n_nodes >= 1");
  TORCH_CHECK(n_nodes * nb <= HS_LDS_ENTRIES,
              "level too wide for LDS histogram (use the torch path)");
  TORCH_CHECK(B < kI31 && nf < kI31 && nnz < kI31 * 4,
              "gbt_hist_sparse: B and nf must be below 2^31, nnz below 2^33");
  auto opt = resid.options();
  torch::Tensor cnt = torch::empty({n_nodes, nf, nb}, opt);
  torch::Tensor sum = torch::empty({n_nodes, nf, nb}, opt);
  if (nf == 0) return {cnt, sum};
  TORCH_CHECK(B >= 1, "gbt_hist_sparse: entries but no rows");
  const int fc = (int)std::min(nf, HS_LDS_ENTRIES / (n_nodes * nb));
  const int64_t n_wg = (nf + fc - 1) / fc;
  const size_t lds = (size_t)2 * n_nodes * fc * nb * sizeof(float);
  const bool vec4 = nb % 4 == 0 &&
                    reinterpret_cast<uintptr_t>(cnt.data_ptr<float>()) % 16 == 0 &&
                    reinterpret_cast<uintptr_t>(sum.data_ptr<float>()) % 16 == 0;
  hipStream_t st = current_stream();
#define GO(V)                                                                \
  hipLaunchKernelGGL((gbt_hist_sparse_kernel<V>), dim3((unsigned)n_wg),      \
                     dim3(HS_THREADS), lds, st,                              \
                     feat_ptr.data_ptr<int64_t>(), feat_row.data_ptr<int>(), \
                     feat_bin.data_ptr<int>(), feat_idx.data_ptr<int>(),     \
                     zero_bin.data_ptr<int>(), resid.data_ptr<float>(),      \
                     node.data_ptr<int>(), node_cnt.data_ptr<float>(),       \
                     node_sum.data_ptr<float>(), cnt.data_ptr<float>(),      \
                     sum.data_ptr<float>(), (int)B, (int)nf, (int)nb,        \
                     (int)n_nodes, fc, nnz)
  if (vec4) GO(true); else GO(false);
#undef GO
  return {cnt, sum};
}
