// K10p — GBT forest prediction in one launch.
//
// Reference: GBTTrainer.java predictByTree / the forest sum of evaluateModel.
// The torch path (GBTree.predict_bins once per tree) costs about six tensor
// ops per tree level and one host-to-device copy per tree; here the whole
// forest is applied to a block of binned rows by one kernel.
//
// Input: the packed forest of gbt.encode_trees, int32 [T, row]:
//   [key | feature[ni] | threshold[ni] | leaf bits[2^d] | mask lo[ni] |
//    mask hi[ni]]        ni = 2^d - 1, the two mask ranges optional.
// For a SparseBins batch the caller appends ni words per tree, the zero bin of
// every node's feature (0 for a feature absent from the batch): it depends on
// (tree, node) only, so it is found by ONE searchsorted over the whole packed
// forest before the launch, not per row. The compact feature index is not
// needed: a lane looks its (row, feature) up among the keys of its own row.
//
// Choices:
//   * one row per lane; the lane walks the trees in forest order and does
//     pred = pred + step * leaf with one rounded multiply and one rounded add
//     (contraction is turned off in the kernel body: v_mul_f32 and v_add_f32,
//     never a fused multiply-add), so the sum order is the torch loop's and
//     the result is bit-identical to it. No atomics.
//   * the trees are staged in LDS in groups of PR_LDS_WORDS / row words (a
//     depth-4 tree with masks is 77 words: 106 trees per group); every lane
//     of the workgroup reads the same group.
//   * routing one tree is a chain of d dependent gathers. The trees of a
//     group are independent until their leaves are summed, so a lane routes
//     PR_UNROLL trees at a time, level by level, and adds the leaves in order
//     afterwards: PR_UNROLL gathers are in flight instead of one.
//   * sparse rows: row bounds come from searchsorted(keys, arange(B+1) * F);
//     a lane binary-searches only its own row's keys. Keys are int64
//     (row * F + feature passes 2^32 at F = 2^20).
//
// Routing is gbt._route_right: t >= 0 right iff bin > t; t == -1 left;
// t == -2 right iff bin < 64 and bit clamp(bin, 0, 63) of the node's 64-bit
// mask is set. A forest packed without masks has mask 0 everywhere.
//
// Nothing a malformed forest or batch holds is dereferenced unchecked: a
// feature outside [0, F) reads feature 0 (the wrapper refuses such a forest
// before the launch), row bounds are clamped to [0, nnz], the leaf index is
// below 2^d by construction.

#include "hip_common.h"

namespace {

constexpr int PR_THREADS = 256;
constexpr int PR_LDS_WORDS = 8192;   // 32 KiB of staged trees
constexpr int PR_UNROLL = 4;         // trees routed at a time by a lane
constexpr int PR_MAX_DEPTH = 8;

template <bool SPARSE>
__global__ __launch_bounds__(PR_THREADS) void gbt_predict_kernel(
    const int64_t* __restrict__ bins,     // dense: [B, F]
    const int64_t* __restrict__ keys,     // sparse: [nnz] row * F + feature
    const int* __restrict__ key_bin,      // sparse: [nnz]
    const int64_t* __restrict__ row_ptr,  // sparse: [B+1] bounds into keys
    const int* __restrict__ forest,       // [T, row_len]
    float* __restrict__ out,              // [B]
    int B, int64_t F, int T, int depth, int row_len, int mask_off, int zb_off,
    int group, int64_t nnz, float step) {
  // no fused multiply-add in this body. __fmul_rn / __fadd_rn would not do:
  // in the HIP headers they are a plain * and + compiled under the default
  // -ffp-contract=fast, and were fused into v_fmac_f32 after inlining
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) int lds[];
  const int tid = threadIdx.x;
  const int64_t row = (int64_t)blockIdx.x * PR_THREADS + tid;
  const bool live = row < B;
  const int ni = (1 << depth) - 1;
  int64_t lo = 0, hi = 0;
  if (SPARSE && live) {
    lo = row_ptr[row];
    hi = row_ptr[row + 1];
    lo = lo < 0 ? 0 : (lo > nnz ? nnz : lo);
    hi = hi < lo ? lo : (hi > nnz ? nnz : hi);
  }
  const int64_t* brow = SPARSE ? nullptr : bins + (live ? row : 0) * F;
  float pred = 0.f;
  for (int t0 = 0; t0 < T; t0 += group) {
    const int nt = min(group, T - t0);
    const int nw = nt * row_len;
    const int* src = forest + (int64_t)t0 * row_len;
    __syncthreads();                  // the previous group is consumed
    for (int i = tid; i < nw; i += PR_THREADS) lds[i] = src[i];
    __syncthreads();
    if (!live) continue;
    for (int u0 = 0; u0 < nt; u0 += PR_UNROLL) {
      int local[PR_UNROLL];
      int tr[PR_UNROLL];                // the tree's first word in lds
#pragma unroll
      for (int u = 0; u < PR_UNROLL; ++u) {
        local[u] = 0;
        // past the group's end: the last tree again, its leaf is not added
        tr[u] = min(u0 + u, nt - 1) * row_len;
      }
      for (int level = 0; level < depth; ++level) {
        const int first = (1 << level) - 1;
#pragma unroll
        for (int u = 0; u < PR_UNROLL; ++u) {
          const int n = first + local[u];
          int feat = lds[tr[u] + 1 + n];
          const int thr = lds[tr[u] + 1 + ni + n];
          if ((int64_t)feat < 0 || (int64_t)feat >= F) feat = 0;
          int64_t b;
          if (SPARSE) {
            const int64_t want = row * F + feat;
            int64_t a = lo, z = hi;
            while (a < z) {           // lower bound among the row's keys
              const int64_t m = a + ((z - a) >> 1);
              if (keys[m] < want) a = m + 1; else z = m;
            }
            b = lds[tr[u] + zb_off + n];
            if (a < hi && keys[a] == want) b = key_bin[a];
          } else {
            b = brow[feat];
          }
          bool right;
          if (thr >= 0) {
            right = b > (int64_t)thr;
          } else {
            unsigned long long mask = 0;
            if (mask_off > 0) {       // the low and the high mask word
              const unsigned ml = (unsigned)lds[tr[u] + mask_off + n];
              const unsigned mh = (unsigned)lds[tr[u] + mask_off + ni + n];
              mask = (unsigned long long)ml | ((unsigned long long)mh << 32);
            }
            const int sh = b < 0 ? 0 : (b > 63 ? 63 : (int)b);
            right = thr == -2 && b < 64 && ((mask >> sh) & 1ull);
          }
          local[u] = 2 * local[u] + (right ? 1 : 0);
        }
      }
#pragma unroll
      for (int u = 0; u < PR_UNROLL; ++u) {
        if (u0 + u < nt) {
          const float leaf =
              __int_as_float(lds[tr[u] + 1 + 2 * ni + local[u]]);
          const float scaled = step * leaf;   // rounded, then a rounded add
          pred = pred + scaled;
        }
      }
    }
  }
  if (live) out[row] = pred;
}

constexpr int64_t kI31 = (int64_t)1 << 31;

}  // namespace

// The deepest tree K10p takes, and the words of staged trees per LDS group
// (a group holds gbt_predict_lds_words() / row trees).
int64_t gbt_predict_max_depth() { return PR_MAX_DEPTH; }
int64_t gbt_predict_lds_words() { return PR_LDS_WORDS; }

// step_size * the forest's prediction, float32 [B], summed in forest order.
// Dense: bins int64 [B, F]. Sparse: keys int64 [nnz] sorted, key_bin int32
// [nnz], row_ptr int64 [B+1], and forest rows extended by the ni zero-bin
// words (see the header). F is the number of features of the batch.
torch::Tensor gbt_forest_predict(
    c10::optional<torch::Tensor> bins, torch::Tensor forest, int64_t depth,
    double step_size, int64_t F, c10::optional<torch::Tensor> keys,
    c10::optional<torch::Tensor> key_bin,
    c10::optional<torch::Tensor> row_ptr) {
  CHECK_IN(forest);
  TORCH_CHECK(depth >= 1, "gbt_forest_predict: depth must be at least 1");
  TORCH_CHECK(depth <= PR_MAX_DEPTH,
              "gbt_forest_predict: tree too deep (use the torch path)");
  TORCH_CHECK(forest.dtype() == torch::kInt32 && forest.dim() == 2,
              "forest must be int32 [T, row]");
  const bool sparse = !bins.has_value();
  const int64_t ni = ((int64_t)1 << depth) - 1;
  const int64_t base = 1 + 2 * ni + ((int64_t)1 << depth);
  const int64_t extra = sparse ? ni : 0;
  const int64_t T = forest.size(0), row_len = forest.size(1);
  TORCH_CHECK(row_len == base + extra || row_len == base + 2 * ni + extra,
              "gbt_forest_predict: forest row length does not fit depth");
  const bool with_masks = row_len == base + 2 * ni + extra;
  TORCH_CHECK(F >= 1 && T < kI31, "gbt_forest_predict: F >= 1, T < 2^31");
  int64_t B = 0, nnz = 0;
  if (sparse) {
    TORCH_CHECK(keys.has_value() && key_bin.has_value() && row_ptr.has_value(),
                "sparse input needs keys, key_bin and row_ptr");
    CHECK_IN(*keys); CHECK_IN(*key_bin); CHECK_IN(*row_ptr);
    nnz = keys->numel();
    TORCH_CHECK(keys->dtype() == torch::kInt64 && keys->dim() == 1,
                "keys must be int64 [nnz]");
    TORCH_CHECK(key_bin->dtype() == torch::kInt32 && key_bin->dim() == 1 &&
                key_bin->numel() == nnz, "key_bin must be int32 [nnz]");
    TORCH_CHECK(row_ptr->dtype() == torch::kInt64 && row_ptr->dim() == 1 &&
                row_ptr->numel() >= 1, "row_ptr must be int64 [B+1]");
    B = row_ptr->numel() - 1;
  } else {
    CHECK_IN(*bins);
    TORCH_CHECK(bins->dtype() == torch::kInt64 && bins->dim() == 2 &&
                bins->size(1) == F, "bins must be int64 [B, F]");
    B = bins->size(0);
  }
  TORCH_CHECK(B < kI31, "gbt_forest_predict: B must be below 2^31");
  torch::Tensor out = torch::zeros(
      {B}, forest.options().dtype(torch::kFloat32));
  if (B == 0 || T == 0) return out;
  const int group = (int)(PR_LDS_WORDS / row_len);
  TORCH_CHECK(group >= 1, "gbt_forest_predict: a tree does not fit in LDS");
  const size_t lds = (size_t)group * row_len * sizeof(int);
  const int64_t n_wg = (B + PR_THREADS - 1) / PR_THREADS;
  const int mask_off = with_masks ? (int)base : 0;
  const int zb_off = sparse ? (int)(row_len - ni) : 0;
  hipStream_t st = current_stream();
  if (sparse) {
    hipLaunchKernelGGL((gbt_predict_kernel<true>), dim3((unsigned)n_wg),
                       dim3(PR_THREADS), lds, st, nullptr,
                       keys->data_ptr<int64_t>(), key_bin->data_ptr<int>(),
                       row_ptr->data_ptr<int64_t>(), forest.data_ptr<int>(),
                       out.data_ptr<float>(), (int)B, F, (int)T, (int)depth,
                       (int)row_len, mask_off, zb_off, group, nnz,
                       (float)step_size);
  } else {
    hipLaunchKernelGGL((gbt_predict_kernel<false>), dim3((unsigned)n_wg),
                       dim3(PR_THREADS), lds, st, bins->data_ptr<int64_t>(),
                       nullptr, nullptr, nullptr, forest.data_ptr<int>(),
                       out.data_ptr<float>(), (int)B, F, (int)T, (int)depth,
                       (int)row_len, mask_off, zb_off, group, nnz,
                       (float)step_size);
  }
  return out;
}
