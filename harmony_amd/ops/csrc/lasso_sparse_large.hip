// K11sL — the sparse Lasso sweep (K11s, lasso_sparse.hip) for batches whose
// residual does not fit K11s's 64 KiB of LDS: 16209 to 40928 rows, the
// residual fp32 in up to 160 KiB of dynamic LDS (a gfx950 CU's whole LDS:
// 40960 floats, less the 32 floats of cross-wave partials below).
//
// Shape. One workgroup of T = 64, 256 or 1024 threads, NW = T / 64 waves. At
// these row counts a wide feature space gives hundreds of thousands of
// present columns of a handful of entries each, and what a column costs is
// one wave's dependent chain (gather, wave sum, threshold, scatter), not
// bandwidth. K11s runs these chains one after the other. Here the present
// columns are cut into windows of NW consecutive columns, window i holding
// columns i*NW .. i*NW+NW-1, and the host marks a window clean when its
// columns pairwise share no row and none is longer than a limit
// (ops.lasso_sparse_windows). Row-disjoint columns commute exactly in
// coordinate descent: each reads and writes residual cells no other column
// of the window touches, so sweeping them at the same time gives the values
// of sweeping them in order.
//   * clean window: wave v takes column i*NW+v alone: 64 entries per pass,
//     the in-register wave sum, threshold, scatter; no cross-wave partials
//     and no barrier inside the window. One __syncthreads() ends it: columns
//     of different windows may share rows, and that barrier is what orders
//     one window's scatter and the next one's gather;
//   * dirty window: its columns go one at a time with all waves on the
//     column, K11s's scheme: cross-wave partials double-buffered by parity, a
//     barrier after a moved weight, the scatter skipped when it does not
//     move;
//   * without a table every window is dirty, and with T = 64 a window is one
//     column, both kinds are the same code and the kernel is the sequential
//     sweep.
// From K11s: the per-column scalars are loaded 64 columns at a time, one
// column per lane, a batch ahead (every wave holds the whole batch, so a
// window's wave reads its own column's lane); the first entries of whatever
// runs next (the next window's columns, one per wave, or the next dirty
// column, across the workgroup) are loaded before the current LDS chain; a
// zero weight that thresholds to zero again leaves before the divide; moved
// weights are stored once per batch of 64 columns, each by the wave that
// owns the column (column j belongs to wave j % NW in both kinds of window),
// which keeps the store off the memory counter the prefetch waits on.
//
// Prologue. r = y, then r -= X w over the same windows: in a clean window
// each wave subtracts its own column if its weight is not zero, one barrier
// per window; in a dirty one column by column with a barrier between
// columns. A window none of whose columns has a weight is passed without a
// barrier, and the first entry of every weighted column comes with the batch
// load, so a one-entry column costs no load of its own.
//
// No atomics, and the order of every sum is fixed by (T, table): results are
// bitwise reproducible. The table is trusted (the wrapper is its only
// producer); a wrong one gives wrong sums, never a wild access: malformed
// indices (row outside [0, B), feature outside [0, F), bounds outside
// [0, nnz]) are skipped, never dereferenced.

#include "hip_common.h"

namespace {

constexpr float kZeroThreshold = 1e-9f;   // LassoTrainer.java:61
constexpr int kMaxWaves = 16;
// LDS carve-up, in floats
constexpr int kPartialOff = 0;                            // [2][kMaxWaves]
constexpr int kResidOff = kPartialOff + 2 * kMaxWaves;
constexpr int64_t kLdsBytes = 160 * 1024;                 // one gfx950 CU
constexpr int64_t kMaxRows = kLdsBytes / 4 - kResidOff;   // 40928

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

// Clean flags of the windows of columns k0 .. k0+63, one window per lane.
template <int NW>
__device__ __forceinline__ int load_flags(
    int k0, int lane, const unsigned char* __restrict__ win, int nwin) {
  if (NW == 1 || win == nullptr) return 0;
  const int i = k0 / NW + lane;
  return (lane < WAVE / NW && i < nwin) ? (int)win[i] : 0;
}

template <int T>
__global__ __launch_bounds__(T) void lasso_cd_sparse_large_kernel(
    const int* __restrict__ feat_ids, const int64_t* __restrict__ feat_ptr,
    const int* __restrict__ feat_row, const float* __restrict__ feat_val,
    const float* __restrict__ y, float* w, const float* __restrict__ col_sq,
    const unsigned char* __restrict__ win, float lam_n,
    float* __restrict__ r_g, int B, int F, int nf, int nnz) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int NW = T / WAVE;
  constexpr int WPB = WAVE / NW;          // windows per batch of 64 columns
  float* partial = lds + kPartialOff;
  float* r = lds + kResidOff;
  const int tid = threadIdx.x, lane = tid % WAVE;
  const int wid = __builtin_amdgcn_readfirstlane(tid / WAVE);
  const int nwin = (nf + NW - 1) / NW;

  for (int i = tid; i < B; i += T) r[i] = y[i];
  __syncthreads();

  // ---- prologue: r -= X w, window by window
  {
    // the first entry of each weighted column of the batch, one per lane
    auto load_first = [&](const ColBatch& c, int& fr, float& fv) {
      fr = -1;
      fv = 0.f;
      if (c.id >= 0 && c.wi != 0.f && c.beg < c.end) {
        fr = feat_row[c.beg];
        fv = feat_val[c.beg];
      }
    };
    ColBatch cur = load_cols(0, lane, feat_ids, feat_ptr, w, col_sq, F, nf,
                             nnz);
    int cflag = load_flags<NW>(0, lane, win, nwin);
    int cfr;
    float cfv;
    load_first(cur, cfr, cfv);
    for (int kb = 0; kb < nf; kb += WAVE) {
      const ColBatch nxt = load_cols(kb + WAVE, lane, feat_ids, feat_ptr, w,
                                     col_sq, F, nf, nnz);
      const int nflag = load_flags<NW>(kb + WAVE, lane, win, nwin);
      int nfr;
      float nfv;
      load_first(nxt, nfr, nfv);
      // columns of the batch that have something to subtract
      const unsigned long long live =
          __ballot(cur.id >= 0 && cur.wi != 0.f && cur.beg < cur.end);
      // column j with `step` threads from thread `off` on
      auto subtract = [&](int j, int off, int step) {
        const float wf = lane_f(cur.wi, j);
        const int beg = lane_i(cur.beg, j), end = lane_i(cur.end, j);
        const int frow = lane_i(cfr, j);
        const float fval = lane_f(cfv, j);
        if (off == 0 && (unsigned)frow < (unsigned)B) r[frow] -= fval * wf;
        for (int e = beg + 1 + off; e < end; e += step) {
          const int row = feat_row[e];
          const float v = feat_val[e];
          if ((unsigned)row < (unsigned)B) r[row] -= v * wf;
        }
      };
      for (int q = 0; q < WPB && kb + q * NW < nf; ++q) {
        const unsigned m = (unsigned)(live >> (q * NW)) & ((1u << NW) - 1u);
        if (m == 0) continue;
        if (NW > 1 && lane_i(cflag, q)) {
          if ((m >> wid) & 1u) subtract(q * NW + wid, lane, WAVE);
          __syncthreads();
        } else {
          for (int v = 0; v < NW; ++v) {
            if (!((m >> v) & 1u)) continue;
            subtract(q * NW + v, tid, T);
            __syncthreads();
          }
        }
      }
      cur = nxt;
      cflag = nflag;
      cfr = nfr;
      cfv = nfv;
    }
  }

  // ---- sweep
  ColBatch cur = load_cols(0, lane, feat_ids, feat_ptr, w, col_sq, F, nf,
                           nnz);
  int cflag = load_flags<NW>(0, lane, win, nwin);
  ColBatch nxt = cur;
  int nflag = 0;
  bool moved = false;       // this lane's column of the batch, in this wave
  int par = 0;

  // The first entries of what runs after window q (or, inside a dirty
  // window, after a column that is not its last): if that is a clean window,
  // this wave's column of it, one entry per lane; if a dirty one, its first
  // column, one entry per thread.
  auto fetch = [&](const ColBatch& c, int j, bool solo, int& row,
                   float& val) {
    row = 0;
    val = 0.f;
    const int e = lane_i(c.beg, j) + (solo ? lane : tid);
    if (e < lane_i(c.end, j)) {
      row = feat_row[e];
      val = feat_val[e];
    }
  };
  auto fetch_window = [&](int q, int& row, float& val) {
    const bool in = q < WPB;              // else: window 0 of the next batch
    const int qq = in ? q : 0;
    const bool solo = NW > 1 && lane_i(in ? cflag : nflag, qq);
    fetch(in ? cur : nxt, qq * NW + (solo ? wid : 0), solo, row, val);
  };
  // One coordinate. solo: this wave alone, 64 entries per pass; otherwise
  // the whole workgroup, with the cross-wave sum and the barrier after a
  // moved weight. (row0, val0) is the thread's first entry, fetched earlier.
  auto column = [&](int j, auto solo_t, int row0, float val0) {
    constexpr bool solo = decltype(solo_t)::value;
    const int off = solo ? lane : tid;
    constexpr int step = solo ? WAVE : T;
    const bool live = lane_i(cur.id, j) >= 0;
    const float cs = lane_f(cur.cs, j);
    const float wi = lane_f(cur.wi, j);
    const int beg = lane_i(cur.beg, j), end = lane_i(cur.end, j);
    // an absent or massless column keeps its weight (upstream: continue)
    if (!(live && end > beg && cs > kZeroThreshold)) return;
    float acc = 0.f;
    int e = beg + off;
    if (e < end && (unsigned)row0 < (unsigned)B) acc = val0 * r[row0];
    for (e += step; e < end; e += step) {
      const int row = feat_row[e];
      const float v = feat_val[e];
      const bool ok = (unsigned)row < (unsigned)B;
      const float rv = r[ok ? row : 0];
      acc += ok ? v * rv : 0.f;
    }
    float c = wave_sum_uniform(acc);
    if (!solo && NW > 1) {
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
    const float t = fmaxf(fabsf(c) - lam_n, 0.f) * sgn;
    // a zero weight thresholded to zero again (the usual outcome) is done
    if (t == 0.f && wi == 0.f) return;
    const float wn = t / cs;
    const float d = wi - wn;
    if (d == 0.f) return;
    if (lane == j && wid == j % NW) {
      cur.wi = wn;
      moved = true;
    }
    e = beg + off;
    if (e < end && (unsigned)row0 < (unsigned)B) r[row0] += val0 * d;
    for (e += step; e < end; e += step) {
      const int row = feat_row[e];
      const float v = feat_val[e];
      if ((unsigned)row < (unsigned)B) r[row] += v * d;
    }
    if (!solo) __syncthreads();
  };

  int row0, nrow;
  float val0, nval;
  {
    const bool solo = NW > 1 && lane_i(cflag, 0);
    fetch(cur, solo ? wid : 0, solo, row0, val0);
  }
  for (int kb = 0; kb < nf; kb += WAVE) {
    nxt = load_cols(kb + WAVE, lane, feat_ids, feat_ptr, w, col_sq, F, nf,
                    nnz);
    nflag = load_flags<NW>(kb + WAVE, lane, win, nwin);
    for (int q = 0; q < WPB && kb + q * NW < nf; ++q) {
      if (NW > 1 && lane_i(cflag, q)) {
        fetch_window(q + 1, nrow, nval);
        column(q * NW + wid, std::true_type{}, row0, val0);
        __syncthreads();
        row0 = nrow;
        val0 = nval;
      } else {
        for (int v = 0; v < NW; ++v) {
          if (v + 1 < NW) fetch(cur, q * NW + v + 1, false, nrow, nval);
          else fetch_window(q + 1, nrow, nval);
          column(q * NW + v, std::false_type{}, row0, val0);
          row0 = nrow;
          val0 = nval;
        }
      }
    }
    // the moved weights of these 64 columns go out here, not column by
    // column: a store per column would sit in the in-order memory counter
    // the next column's prefetched entries are waited on
    if (moved) w[cur.id] = cur.wi;
    moved = false;
    cur = nxt;
    cflag = nflag;
  }

  __syncthreads();
  for (int i = tid; i < B; i += T) r_g[i] = r[i];
}

}  // namespace

// The largest batch the LDS-resident residual admits: 40928 rows.
int64_t lasso_cd_sparse_large_max_rows() { return kMaxRows; }

// Launches K11sL; the caller (lasso_cd_sparse, lasso_sparse.hip) has checked
// every tensor. win: clean flags of the windows of threads / 64 columns, or
// nullptr for none (every window dirty).
void lasso_cd_sparse_large_launch(
    const char* op, const int* feat_ids, const int64_t* feat_ptr,
    const int* feat_row, const float* feat_val, const float* y, float* w,
    const float* col_sq, const unsigned char* win, float lam_n, float* r_out,
    int64_t B, int64_t F, int64_t nf, int64_t nnz, int64_t threads) {
  TORCH_CHECK(B <= kMaxRows, op, ": batch too large for LDS-resident "
              "residual (max ", kMaxRows, " rows)");
  const size_t lds = (size_t)(kResidOff + B) * sizeof(float);
  dispatch_pow2<64, 1024, 4>(op, "threads", threads, [&](auto t) {
    auto kern = lasso_cd_sparse_large_kernel<t.value>;
    // more than the 64 KiB a kernel gets by default: admitted once per kernel
    static const hipError_t admitted = hipFuncSetAttribute(
        reinterpret_cast<const void*>(kern),
        hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsBytes);
    check_hip(op, admitted, "admitting 160 KiB of dynamic LDS");
    hipLaunchKernelGGL(kern, dim3(1), dim3(t.value), lds, current_stream(),
                       feat_ids, feat_ptr, feat_row, feat_val, y, w, col_sq,
                       win, lam_n, r_out, (int)B, (int)F, (int)nf, (int)nnz);
    check_hip(op, hipGetLastError(), "launching K11sL");
  });
}
