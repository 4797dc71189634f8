// K11s — Lasso cyclic coordinate descent over a sparse batch: one launch
// does one full sweep over the features PRESENT in the batch, through the
// batch's static column index (SparseBatch: feat_ids / feat_ptr / feat_row /
// feat_val, rows distinct within a feature).
//
// Reference: LassoTrainer.java builds the batch matrix from SparseVectors
// (horzcatVecSparse, :273-283) and skips a column that has no mass in the
// batch (:199-208). Dense K11 (lasso.hip) walks all B rows of all F columns;
// here a coordinate costs its own entries only, and a feature the batch does
// not hold is never touched.
//
// Shape. Coordinate descent is sequential across coordinates, so this is one
// workgroup with the residual in LDS, as K11. What decides the speed is the
// fixed cost per coordinate, not bandwidth: at tens of non-zeros per row and
// F = 2^20 nearly every present column has one or two entries and there are
// tens of thousands of columns. So:
//   * the thread count T is a launch parameter (64, 256, 1024; the host rule
//     is ops.lasso_sparse_threads). At T = 64 the workgroup is one wave: the
//     reduction is the in-register wave sum alone and every __syncthreads()
//     below is just the LDS write -> read ordering inside that wave;
//   * a column whose weight does not move (the common case: w stays 0) skips
//     its scatter and the barrier after it. Every thread computes the same
//     new weight from the same partials, so the branch is uniform;
//   * per-column scalars (id, col_sq, w, segment bounds) are loaded 64 columns
//     at a time, one column per lane, a batch ahead, and handed out with
//     v_readlane, and a moved weight goes back into its lane and is stored
//     once per 64 columns; column k+1's first (row, val) entries are loaded
//     before column k's reduce / threshold / scatter. Neither depends on r,
//     so the global-load latency sits behind the LDS chain;
//   * a zero weight that thresholds to zero again leaves the column before
//     the divide.
//
// Hazards. Column k+1's gather reads r[] cells that OTHER lanes scattered in
// column k (consecutive columns share rows but map entries to different
// lanes), so a moved weight is followed by a barrier. Within a column the
// scatter follows the barrier of the reduction (one wave: its own in-order
// LDS queue), so every gather of the column is done before any scatter. The
// cross-wave partials are double-buffered by the parity of the column count,
// which puts a barrier between a read of one buffer and its next write.
//
// Prologue. r = y - X w is built here, not by a torch index_add_: r = y, then
// for each present feature in order with w != 0, r[row] -= val * w, one
// column at a time with a barrier between columns, so the summation order
// depends on the data alone and no atomics are used. The columns with a
// non-zero weight are found kScan * T at a time (ballot masks in LDS); the
// lane that looked at such a column hands its weight, bounds and first entry
// to the workgroup through a double-buffered LDS slot.
//
// No atomics anywhere: results are bitwise reproducible for a given T.
// Malformed indices (row outside [0, B), feature outside [0, F), bounds
// outside [0, nnz]) are skipped, never dereferenced.

#include "hip_common.h"

namespace {

constexpr float kZeroThreshold = 1e-9f;   // LassoTrainer.java:61
constexpr int kMaxWaves = 16;
constexpr int kScan = 4;                  // prologue columns per thread/chunk
// LDS carve-up, in floats; every offset is a multiple of 4 (16 bytes)
constexpr int kPartialOff = 0;                            // [2][kMaxWaves]
constexpr int kSlotOff = kPartialOff + 2 * kMaxWaves;     // [2][8]
constexpr int kMaskOff = kSlotOff + 16;                   // [kScan*waves][2]
constexpr int kResidOff = kMaskOff + 2 * kScan * kMaxWaves;
constexpr int64_t kLdsBytes = 64 * 1024;
constexpr int64_t kMaxRows = kLdsBytes / 4 - kResidOff;

__device__ __forceinline__ int lane_i(int v, int l) {
  return __builtin_amdgcn_readlane(v, l);
}
__device__ __forceinline__ float lane_f(float v, int l) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}

// Wave sum that leaves the same bits in every lane, without the LDS crossbar
// a __shfl_xor butterfly goes through (six dependent ds_bpermute round trips
// were most of a short column's time): four DPP steps inside each 16-lane
// row (xor 1, xor 2, half mirror, mirror; each pair of lanes adds the same
// two values, so a row's lanes agree), then the four row sums by v_readlane.
// Needs all 64 lanes active.
template <int CTRL>
__device__ __forceinline__ float dpp_add(float v) {
  return v + __int_as_float(__builtin_amdgcn_update_dpp(
                 0, __float_as_int(v), CTRL, 0xF, 0xF, true));
}
__device__ __forceinline__ float wave_sum_uniform(float v) {
  v = dpp_add<0xB1>(v);    // quad_perm [1,0,3,2]
  v = dpp_add<0x4E>(v);    // quad_perm [2,3,0,1]
  v = dpp_add<0x141>(v);   // row_half_mirror
  v = dpp_add<0x140>(v);   // row_mirror
  return (lane_f(v, 0) + lane_f(v, 16)) + (lane_f(v, 32) + lane_f(v, 48));
}

// One column per lane: the scalars of columns k0 .. k0+63.
struct ColBatch {
  int id;        // feature, -1 where there is no (valid) column
  float cs, wi;
  int beg, end;  // clamped to [0, nnz]; beg >= end: nothing to do
};

__device__ __forceinline__ ColBatch load_cols(
    int k0, int lane, const int* __restrict__ feat_ids,
    const int64_t* __restrict__ feat_ptr, const float* w,
    const float* __restrict__ col_sq, int F, int nf, int nnz) {
  ColBatch c{-1, 0.f, 0.f, 0, 0};
  const int k = k0 + lane;
  if (k < nf) {
    const int f = feat_ids[k];
    const int64_t b = feat_ptr[k], e = feat_ptr[k + 1];
    c.cs = col_sq[k];
    if ((unsigned)f < (unsigned)F) {
      c.id = f;
      c.wi = w[f];
      c.beg = (int)(b < 0 ? 0 : (b > nnz ? nnz : b));
      c.end = (int)(e < 0 ? 0 : (e > nnz ? nnz : e));
    }
  }
  return c;
}

template <int T>
__global__ __launch_bounds__(T) void lasso_cd_sparse_kernel(
    const int* __restrict__ feat_ids, const int64_t* __restrict__ feat_ptr,
    const int* __restrict__ feat_row, const float* __restrict__ feat_val,
    const float* __restrict__ y, float* w, const float* __restrict__ col_sq,
    float lam_n, float* __restrict__ r_g, int B, int F, int nf, int nnz) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int NW = T / WAVE;
  float* partial = lds + kPartialOff;
  float* slot = lds + kSlotOff;
  unsigned* masks = reinterpret_cast<unsigned*>(lds + kMaskOff);
  float* r = lds + kResidOff;
  const int tid = threadIdx.x, wid = tid / WAVE, lane = tid % WAVE;

  for (int i = tid; i < B; i += T) r[i] = y[i];
  __syncthreads();

  // ---- prologue: r -= X w over the columns whose weight is not zero
  // the column's first entry (frow, fval) comes with the slot; the rest is
  // read here
  auto subtract = [&](float wf, int beg, int end, int frow, float fval) {
    if (tid == 0 && beg < end && (unsigned)frow < (unsigned)B)
      r[frow] -= fval * wf;
    for (int e = beg + 1 + tid; e < end; e += T) {
      const int row = feat_row[e];
      const float v = feat_val[e];
      if ((unsigned)row < (unsigned)B) r[row] -= v * wf;
    }
  };
  for (int k0 = 0; k0 < nf; k0 += kScan * T) {
    ColBatch own[kScan];
#pragma unroll
    for (int u = 0; u < kScan; ++u)
      own[u] = load_cols(k0 + u * T + wid * WAVE, lane, feat_ids, feat_ptr,
                         w, col_sq, F, nf, nnz);
    // first entry of every column with a weight: loaded here, kScan * T
    // columns at once, so a column of one entry (the usual one when the
    // feature space is wide) costs the walk below no global load at all
    int ofr[kScan];
    float ofv[kScan];
#pragma unroll
    for (int u = 0; u < kScan; ++u) {
      ofr[u] = -1;
      ofv[u] = 0.f;
      if (own[u].id >= 0 && own[u].wi != 0.f && own[u].beg < own[u].end) {
        ofr[u] = feat_row[own[u].beg];
        ofv[u] = feat_val[own[u].beg];
      }
    }
#pragma unroll
    for (int u = 0; u < kScan; ++u) {
      const unsigned long long m =
          __ballot(own[u].id >= 0 && own[u].wi != 0.f);
      if (lane == 0) {
        masks[2 * (u * NW + wid)] = (unsigned)m;
        masks[2 * (u * NW + wid) + 1] = (unsigned)(m >> 32);
      }
    }
    __syncthreads();
    // Walk the set bits in column order. The owner lane publishes column
    // j's (w, beg, end, first entry) into slot[p] while the workgroup still subtracts
    // the column before it; one barrier per column orders both.
    int p = 0;
    bool have = false;
    float cw = 0.f, cv = 0.f;
    int cb = 0, ce = 0, cr = -1;
#pragma unroll
    for (int u = 0; u < kScan; ++u) {
      for (int ww = 0; ww < NW; ++ww) {
        unsigned long long m =
            ((unsigned long long)__builtin_amdgcn_readfirstlane(
                 masks[2 * (u * NW + ww) + 1]) << 32) |
            __builtin_amdgcn_readfirstlane(masks[2 * (u * NW + ww)]);
        while (m) {
          const int b = __ffsll((long long)m) - 1;
          m &= m - 1;
          if (wid == ww && lane == b) {
            slot[8 * p] = own[u].wi;
            slot[8 * p + 1] = __int_as_float(own[u].beg);
            slot[8 * p + 2] = __int_as_float(own[u].end);
            slot[8 * p + 3] = __int_as_float(ofr[u]);
            slot[8 * p + 4] = ofv[u];
          }
          if (have) subtract(cw, cb, ce, cr, cv);
          __syncthreads();
          cw = slot[8 * p];
          cb = __float_as_int(slot[8 * p + 1]);
          ce = __float_as_int(slot[8 * p + 2]);
          cr = __float_as_int(slot[8 * p + 3]);
          cv = slot[8 * p + 4];
          have = true;
          p ^= 1;
        }
      }
    }
    if (have) subtract(cw, cb, ce, cr, cv);
    __syncthreads();     // last column done; masks and slots free again
  }

  // ---- sweep
  ColBatch cur = load_cols(0, lane, feat_ids, feat_ptr, w, col_sq, F, nf,
                           nnz);
  int row0 = 0;
  float val0 = 0.f;
  {
    const int e = lane_i(cur.beg, 0) + tid;
    if (e < lane_i(cur.end, 0)) {
      row0 = feat_row[e];
      val0 = feat_val[e];
    }
  }
  int par = 0;
  for (int kb = 0; kb < nf; kb += WAVE) {
    const ColBatch nxt = load_cols(kb + WAVE, lane, feat_ids, feat_ptr, w,
                                   col_sq, F, nf, nnz);
    const int cnt = nf - kb < WAVE ? nf - kb : WAVE;
    bool dirty = false;
    for (int j = 0; j < cnt; ++j) {
      const bool live = lane_i(cur.id, j) >= 0;
      const float cs = lane_f(cur.cs, j);
      const float wi = lane_f(cur.wi, j);
      const int beg = lane_i(cur.beg, j), end = lane_i(cur.end, j);
      // the next column's first entries: no dependence on r, so their
      // latency hides behind this column's LDS chain. (Handing a one-entry
      // column its entry from the batch registers instead, with no load at
      // all, measured 10 % slower: the chain, not the load, is the cost.)
      int nrow = 0;
      float nval = 0.f;
      {
        const bool in = j + 1 < WAVE;
        const int jn = in ? j + 1 : 0;
        const int nb = in ? lane_i(cur.beg, jn) : lane_i(nxt.beg, 0);
        const int ne = in ? lane_i(cur.end, jn) : lane_i(nxt.end, 0);
        const int e = nb + tid;
        if (e < ne) {
          nrow = feat_row[e];
          nval = feat_val[e];
        }
      }
      // an absent or massless column keeps its weight (upstream: continue)
      if (live && end > beg && cs > kZeroThreshold) {
        float acc = 0.f;
        int e = beg + tid;
        if (e < end && (unsigned)row0 < (unsigned)B) acc = val0 * r[row0];
        for (e += T; e < end; e += T) {
          const int row = feat_row[e];
          const float v = feat_val[e];
          const bool ok = (unsigned)row < (unsigned)B;
          const float rv = r[ok ? row : 0];
          acc += ok ? v * rv : 0.f;
        }
        float c = wave_sum_uniform(acc);
        if (NW > 1) {
          float* pp = partial + par * kMaxWaves;
          if (lane == 0) pp[wid] = c;
          __syncthreads();
          c = 0.f;
#pragma unroll
          for (int q = 0; q < NW; ++q) c += pp[q];
          par ^= 1;
        }
        c += wi * cs;
        const float sgn = (c > 0.f) ? 1.f : ((c < 0.f) ? -1.f : 0.f);
        // a zero weight thresholded to zero again (the usual outcome) is
        // done here: wn = 0 * sgn / cs is a zero, and so is d
        const float t = fmaxf(fabsf(c) - lam_n, 0.f) * sgn;
        if (t == 0.f && wi == 0.f) {
          row0 = nrow;
          val0 = nval;
          continue;
        }
        const float wn = t / cs;
        const float d = wi - wn;
        if (d != 0.f) {
          if (lane == j) {
            cur.wi = wn;
            dirty = true;
          }
          e = beg + tid;
          if (e < end && (unsigned)row0 < (unsigned)B) r[row0] += val0 * d;
          for (e += T; e < end; e += T) {
            const int row = feat_row[e];
            const float v = feat_val[e];
            if ((unsigned)row < (unsigned)B) r[row] += v * d;
          }
          __syncthreads();
        }
      }
      row0 = nrow;
      val0 = nval;
    }
    // The moved weights of these 64 columns go out in one store here: a
    // store per column would sit in the same in-order memory counter as the
    // next column's prefetched entries and put its latency on every column.
    if (wid == 0 && dirty) w[cur.id] = cur.wi;
    cur = nxt;
  }

  __syncthreads();
  for (int i = tid; i < B; i += T) r_g[i] = r[i];
}

constexpr int64_t kI31 = (int64_t)1 << 31;

}  // namespace

// The largest batch the LDS-resident residual admits.
int64_t lasso_cd_sparse_max_rows() { return kMaxRows; }

// One cyclic sweep over the present features. w [F] is updated in place,
// r_out [B] receives y - X w_new. threads: 64, 256 or 1024.
void lasso_cd_sparse(torch::Tensor feat_ids, torch::Tensor feat_ptr,
                     torch::Tensor feat_row, torch::Tensor feat_val,
                     torch::Tensor y, torch::Tensor w, torch::Tensor col_sq,
                     double lam_n, torch::Tensor r_out, int64_t threads) {
  CHECK_IN(feat_ids); CHECK_IN(feat_ptr); CHECK_IN(feat_row);
  CHECK_IN(feat_val); CHECK_IN(y); CHECK_IN(w); CHECK_IN(col_sq);
  CHECK_IN(r_out);
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
  TORCH_CHECK(y.dtype() == torch::kFloat32 && y.dim() == 1 &&
              r_out.dtype() == torch::kFloat32 && r_out.dim() == 1 &&
              r_out.numel() == y.numel(),
              "y and r_out must be float32 [B]");
  TORCH_CHECK(w.dtype() == torch::kFloat32 && w.dim() == 1,
              "w must be float32 [F]");
  TORCH_CHECK(col_sq.dtype() == torch::kFloat32 && col_sq.dim() == 1 &&
              col_sq.numel() == feat_ids.numel(),
              "col_sq must be float32 [nf]");
  const int64_t nf = feat_ids.numel(), nnz = feat_row.numel();
  const int64_t B = y.numel(), F = w.numel();
  TORCH_CHECK(nf >= 1 && B >= 1, "lasso_cd_sparse: empty batch");
  TORCH_CHECK(B <= kMaxRows,
              "batch too large for LDS-resident residual (max ", kMaxRows,
              " rows)");
  TORCH_CHECK(nnz < kI31 && F < kI31 && nf < kI31 - 4 * 1024 * kScan,
              "lasso_cd_sparse: nnz, F and nf must be below 2^31");
  const size_t lds = (size_t)(kResidOff + B) * sizeof(float);
  hipStream_t st = current_stream();
#define GO(TV)                                                              \
  case TV:                                                                  \
    hipLaunchKernelGGL((lasso_cd_sparse_kernel<TV>), dim3(1), dim3(TV),     \
                       lds, st, feat_ids.data_ptr<int>(),                   \
                       feat_ptr.data_ptr<int64_t>(),                        \
                       feat_row.data_ptr<int>(),                            \
                       feat_val.data_ptr<float>(), y.data_ptr<float>(),     \
                       w.data_ptr<float>(), col_sq.data_ptr<float>(),       \
                       (float)lam_n, r_out.data_ptr<float>(), (int)B,       \
                       (int)F, (int)nf, (int)nnz);                          \
    break
  switch (threads) {
    GO(64); GO(256); GO(1024);
    default:
      TORCH_CHECK(false, "threads must be 64, 256 or 1024");
  }
#undef GO
}
