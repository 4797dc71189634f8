// K4s: sparse MLR — the forward logits and the gradient of one mini-batch
// as gather-reduces over the batch's non-zeros, for libsvm-style inputs
// whose feature space is far wider than a row is long.
//
// Reference semantics: MLRTrainer.java:374-398 walks only a sample's
// non-zeros (the data is SparseVector, MLRETDataParser.createSparse). The
// dense path here (X @ W^T, P^T @ X) costs B*F*C; these cost nnz*C.
//
//   mlr_sparse_fwd   logits[r, c] = sum_e val[e] * Wt[col[e], c]
//                    over the CSR entries e of row r
//   mlr_sparse_grad  G[c, f] = sum_e feat_val[e] * P[feat_row[e], c]
//                    over the entries e of present feature f, through the
//                    static per-batch column index (CSC over present
//                    features, rows ascending within a feature)
//
// Both are the same computation — out[segment, :] = sum over the segment's
// entries of value * table[index, :] — so one kernel serves both; only the
// output addressing differs (logits rows are contiguous in c; G is [C, F],
// so a feature's classes are F floats apart and its position is feat_ids[s]).
//
// Layout: CSR-vector, as K13 (pregel.hip). G = 2^k lanes (1..64, chosen on
// the host from the mean segment length) cooperate on one segment; lanes
// read consecutive entries (coalesced index/value loads), stride by G over
// longer segments, and reduce with a width-G xor butterfly. Each lane keeps
// up to 16 class partials in registers; C > 16 walks the segment once per
// tile of 16 classes. A table row is fetched as contiguous 16-byte loads:
// Wt is the model transposed and padded to [F, Cp], Cp = C rounded up to 4,
// so a non-zero costs one Cp-float fetch instead of C cache lines of [C, F].
// P rows are read the same way, so P's row stride is a multiple of 4 floats
// too (the caller pads it: measured up to 2.3x faster than scalar loads of
// an unpadded [B, C] and never slower, the pad copy included —
// profiles/mlr_sparse_ab.md).
//
// No atomics: one lane writes each output element, and for a fixed G the
// summation order is fixed by the data, so the result is bitwise identical
// from run to run. The gradient's scatter is the "store pass + per-
// destination sum pass" form with the store pass folded away: the column
// index is built once per batch at load time.
//
// Accepted for this version: one very long segment (a bias feature present
// in every row gives a column of B entries) is walked by its one group
// alone and holds up that group's workgroup; splitting long columns over
// several groups is left to a later change.

#include "hip_common.h"

namespace {

constexpr int kBlock = 256;
constexpr int kTile = 16;        // class partials per lane per sweep

template <int G>
__global__ __launch_bounds__(kBlock) void mlr_sparse_gather_kernel(
    const int64_t* __restrict__ seg_ptr,     // [S+1]
    const int* __restrict__ idx,             // [nnz] row of `table`
    const float* __restrict__ val,           // [nnz]
    const int* __restrict__ seg_ids,         // nullable: segment s writes s
    const float* __restrict__ table, int64_t n_rows, int64_t ld,
    float* __restrict__ out, int64_t n_out, int64_t out_seg_stride,
    int64_t out_cls_stride, int64_t S, int64_t nnz, int C) {
  constexpr int kSegs = kBlock / G;          // segments per workgroup sweep
  const int lane = threadIdx.x & (G - 1);
  const int64_t stride = (int64_t)gridDim.x * kSegs;
  // all G lanes of a group share `s`, so the group takes every branch below
  // together and the width-G shuffles only ever read live lanes
  for (int64_t s = (int64_t)blockIdx.x * kSegs + threadIdx.x / G; s < S;
       s += stride) {
    const int64_t o = seg_ids != nullptr ? (int64_t)seg_ids[s] : s;
    if (o < 0 || o >= n_out) continue;       // malformed index: write nothing
    int64_t beg = seg_ptr[s], end = seg_ptr[s + 1];
    // a malformed index must not read out of bounds
    beg = beg < 0 ? 0 : beg;
    end = end > nnz ? nnz : end;
    for (int c0 = 0; c0 < C; c0 += kTile) {
      const int nc = (C - c0) < kTile ? (C - c0) : kTile;
      float acc[kTile];
#pragma unroll
      for (int k = 0; k < kTile; ++k) acc[k] = 0.f;
      for (int64_t e = beg + lane; e < end; e += G) {
        const int t = idx[e];
        if ((unsigned)t >= (unsigned)n_rows) continue;
        const float v = val[e];
        const float* p = table + (int64_t)t * ld + c0;
        // ld is a multiple of 4 and >= C rounded up to 4, so the quad that
        // holds class c0 + nc - 1 lies inside the row
#pragma unroll
        for (int q = 0; q < kTile / 4; ++q)
          if (4 * q < nc) {
            const float4 w = *reinterpret_cast<const float4*>(p + 4 * q);
            acc[4 * q + 0] += v * w.x;
            acc[4 * q + 1] += v * w.y;
            acc[4 * q + 2] += v * w.z;
            acc[4 * q + 3] += v * w.w;
          }
      }
#pragma unroll
      for (int k = 0; k < kTile; ++k)
        if (k < nc) {
#pragma unroll
          for (int m = G >> 1; m > 0; m >>= 1)
            acc[k] += __shfl_xor(acc[k], m, G);
        }
      if (lane == 0) {
        float* dst = out + o * out_seg_stride + (int64_t)c0 * out_cls_stride;
#pragma unroll
        for (int k = 0; k < kTile; ++k)
          if (k < nc) dst[(int64_t)k * out_cls_stride] = acc[k];
      }
    }
  }
}

struct GatherArgs {
  const int64_t* seg_ptr;
  const int* idx;
  const float* val;
  const int* seg_ids;
  const float* table;
  int64_t n_rows, ld;
  float* out;
  int64_t n_out, out_seg_stride, out_cls_stride, S, nnz;
  int C;
};

template <int G>
void launch(dim3 grid, hipStream_t st, const GatherArgs& a) {
  hipLaunchKernelGGL((mlr_sparse_gather_kernel<G>), grid, dim3(kBlock), 0, st,
                     a.seg_ptr, a.idx, a.val, a.seg_ids, a.table, a.n_rows,
                     a.ld, a.out, a.n_out, a.out_seg_stride, a.out_cls_stride,
                     a.S, a.nnz, a.C);
}

void run(int64_t group, const GatherArgs& a) {
  TORCH_CHECK(group >= 1 && group <= 64 && (group & (group - 1)) == 0,
              "group must be a power of two in 1..64");
  const int64_t segs_per_block = kBlock / group;
  const int64_t want = (a.S + segs_per_block - 1) / segs_per_block;
  // memory-bound: cap the grid and let the groups stride over the rest
  dim3 grid((unsigned)std::min<int64_t>(want, 256 * 8 * 4));
  hipStream_t st = current_stream();
#define GO(GV) case GV: launch<GV>(grid, st, a); break
  switch (group) {
    GO(1); GO(2); GO(4); GO(8); GO(16); GO(32); GO(64);
  }
#undef GO
}

constexpr int64_t kI31 = (int64_t)1 << 31;

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

// logits [B, C] of a CSR batch against the transposed, padded model
// Wt [F, Cp] (Cp a multiple of 4, >= C; pad columns are never written out).
// group: lanes per row, a power of two in 1..64.
torch::Tensor mlr_sparse_fwd(torch::Tensor row_ptr, torch::Tensor col,
                             torch::Tensor val, torch::Tensor Wt, int64_t C,
                             int64_t group) {
  CHECK_IN(row_ptr); CHECK_IN(col); CHECK_IN(val); CHECK_IN(Wt);
  TORCH_CHECK(row_ptr.dtype() == torch::kInt64 && row_ptr.dim() == 1 &&
              row_ptr.numel() >= 1, "row_ptr must be int64 [B+1]");
  TORCH_CHECK(col.dtype() == torch::kInt32 && col.dim() == 1,
              "col must be int32 [nnz]");
  TORCH_CHECK(val.dtype() == torch::kFloat32 && val.dim() == 1 &&
              val.numel() == col.numel(), "val must be float32 [nnz]");
  TORCH_CHECK(Wt.dtype() == torch::kFloat32 && Wt.dim() == 2,
              "Wt must be float32 [F, Cp]");
  const int64_t B = row_ptr.numel() - 1, nnz = col.numel();
  const int64_t F = Wt.size(0), Cp = Wt.size(1);
  TORCH_CHECK(C >= 1 && Cp % 4 == 0 && Cp >= C && Cp - C < 4,
              "Wt must be [F, C rounded up to a multiple of 4]");
  TORCH_CHECK(nnz < kI31 && B < kI31 && F < kI31,
              "mlr_sparse_fwd: nnz, B and F must be below 2^31");
  TORCH_CHECK(aligned16(Wt.data_ptr<float>()), "Wt must be 16-byte aligned");
  auto logits = torch::empty({B, C}, Wt.options());
  if (B == 0) return logits;
  GatherArgs a{row_ptr.data_ptr<int64_t>(), col.data_ptr<int>(),
               val.data_ptr<float>(), nullptr, Wt.data_ptr<float>(), F, Cp,
               logits.data_ptr<float>(), B, C, 1, B, nnz, (int)C};
  run(group, a);
  return logits;
}

// G [C, F] = P^T @ X through the batch's column index. P is [B, C] with
// unit class stride and a row stride that is a multiple of 4 floats and at
// least C rounded up to 4: a padded [B, Cp] buffer viewed as P[:, :C] (or P
// itself when C is a multiple of 4). group: lanes per present feature.
torch::Tensor mlr_sparse_grad(torch::Tensor feat_ids, torch::Tensor feat_ptr,
                              torch::Tensor feat_row, torch::Tensor feat_val,
                              torch::Tensor P, int64_t F, int64_t group) {
  CHECK_IN(feat_ids); CHECK_IN(feat_ptr); CHECK_IN(feat_row);
  CHECK_IN(feat_val);
  TORCH_CHECK(P.is_cuda() && P.dtype() == torch::kFloat32 && P.dim() == 2,
              "P must be float32 [B, C] on device");
  TORCH_CHECK(feat_ids.dtype() == torch::kInt32 && feat_ids.dim() == 1,
              "feat_ids must be int32 [nf]");
  TORCH_CHECK(feat_ptr.dtype() == torch::kInt64 && feat_ptr.dim() == 1 &&
              feat_ptr.numel() == feat_ids.numel() + 1,
              "feat_ptr must be int64 [nf+1]");
  TORCH_CHECK(feat_row.dtype() == torch::kInt32 && feat_row.dim() == 1,
              "feat_row must be int32 [nnz]");
  TORCH_CHECK(feat_val.dtype() == torch::kFloat32 && feat_val.dim() == 1 &&
              feat_val.numel() == feat_row.numel(),
              "feat_val must be float32 [nnz]");
  const int64_t nf = feat_ids.numel(), nnz = feat_row.numel();
  const int64_t B = P.size(0), C = P.size(1);
  TORCH_CHECK(C >= 1 && F >= 0, "mlr_sparse_grad: need C >= 1, F >= 0");
  TORCH_CHECK(nnz < kI31 && B < kI31 && F < kI31,
              "mlr_sparse_grad: nnz, B and F must be below 2^31");
  auto G = torch::zeros({C, F}, P.options());
  if (nf == 0 || B == 0 || F == 0) return G;
  // 16-byte row loads need every quad of a row inside the row's stride
  const int64_t ld = P.stride(0);
  TORCH_CHECK(P.stride(1) == 1 && ld % 4 == 0 && ld >= (C + 3) / 4 * 4 &&
              aligned16(P.data_ptr<float>()),
              "P must be a 16-byte aligned [B, C] view with unit class "
              "stride and a row stride that is a multiple of 4 and >= C "
              "rounded up to 4");
  GatherArgs a{feat_ptr.data_ptr<int64_t>(), feat_row.data_ptr<int>(),
               feat_val.data_ptr<float>(), feat_ids.data_ptr<int>(),
               P.data_ptr<float>(), B, ld, G.data_ptr<float>(), F, 1, F, nf,
               nnz, (int)C};
  run(group, a);
  return G;
}
