// K10w — GBT level histogram for levels wider than K10's LDS.
//
// K10 (gbt.hip) keeps the (count, sum) cells of ALL nodes of a level in one
// workgroup's 64 KiB, because a tile of rows holds arbitrary nodes; that ends
// at n_nodes * nb = 8192, the ninth level with 64 bins. K10w serves the
// levels past it (nb <= 8192) by grouping the rows by node first:
//
//   * The launch function sorts `node` (stable, a tensor op: B small keys
//     against the B * F bins the kernel walks). The kernel reads the sorted
//     node ids and the permutation, and gathers resid through it.
//   * A workgroup owns a SLICE of 1024 consecutive sorted rows and a range of
//     features (grid.y, only as far as needed for about 512 workgroups, and
//     so that a range has at most 64 features: one lane per feature).
//     Wave w owns rows 256 w .. 256 w + 255 of the slice; lane l keeps the
//     permutation, node and residual of rows l, l + 64, l + 128, l + 192 of
//     them in registers for the workgroup's lifetime.
//   * The slice is walked in PASSES over node sub-ranges. A pass starts at
//     the node `a` of the first row not yet taken and takes the rows with
//     node - a < G = 8192 / nb, so empty nodes cost nothing however far apart
//     the populated ones lie. With span = last taken node - a + 1 it holds
//     span * nb cells per feature, and so covers fc = 8192 / (span * nb)
//     features at a time: a slice inside one or two big nodes takes its whole
//     feature range at once, a level of tiny nodes degrades to fc = 1.
//   * Inside a pass a wave maps its lanes to (row, feature), feature fastest
//     and lw = fc rounded up to a power of two lanes wide, so the
//     lanes of a row load one contiguous run bins[order[i], f0 : f0 + fc].
//     The row's registers reach those lanes by __shfl; the four register rows
//     of a lane give four independent loads in flight. Every entry is two
//     fp32 LDS atomics into cell (node - a, j, b); a bin outside [0, nb) is
//     skipped. Then every cell with cnt != 0 goes to the global arrays with
//     atomicAdd (neighbouring slices and feature chunks of other workgroups
//     share nodes), and only the span * fc * nb cells in use are zeroed.
//   * DIRECT passes: a pass with fewer rows than cells (a last level with
//     a handful of rows per node: 512 rows against 8192 cells, per feature)
//     would spend its time zeroing and scanning LDS. Such a pass adds its
//     entries to the global arrays directly, over the workgroup's whole
//     feature range at once. kDirectRatio sets the switch; the measurement
//     is in profiles/gbt_hist_wide_ab.md.
//
// The pass bounds come from one small reduction over the registers (count,
// last node, next node; LDS integer atomics on three words that the cells
// reuse afterwards), so nothing is read twice from global memory.
//
// Node ids outside [0, n_nodes) and bins outside [0, nb) are skipped, never
// dereferenced. Counts are exact (integers below 2^24); a sum is a float32
// sum of its cell's residuals in an order the atomics decide.

#include <climits>
#include <cstdlib>

#include "hip_common.h"

namespace {

constexpr int HW_THREADS = 256;
constexpr int HW_SLICE = 1024;                    // sorted rows per workgroup
constexpr int HW_ROWS = HW_SLICE / HW_THREADS;    // register rows per lane
constexpr int HW_WAVE_ROWS = HW_ROWS * WAVE;      // rows a wave owns
constexpr int HW_CELLS = 8192;   // (cnt,sum) pairs -> 64 KB LDS, two WGs a CU
constexpr int HW_FEATS = WAVE;   // widest feature range of a workgroup
// A pass goes to global memory directly when rows * kDirectRatio < its cells
// per feature (span * nb). With fewer rows than cells few entries meet in a
// cell, so the flush would issue nearly as many global atomics as the
// entries themselves, after zeroing and scanning the cells for nothing.
constexpr int kDirectRatio = 2;

// This wave's share of one pass: the entries (row, f0 + j), j < fcw, of its
// rows with node in [a, a + width). DIRECT adds to the global arrays, else to
// the LDS cells [span][fcw][nb] at lcnt / lsum. Called by whole waves only.
template <bool DIRECT>
__device__ __forceinline__ void hw_accumulate(
    const int* __restrict__ bins, const int (&ord)[HW_ROWS],
    const int (&nd)[HW_ROWS], const float (&res)[HW_ROWS], int a, int width,
    int F, int nb, int f0, int fcw, float* lcnt, float* lsum,
    float* __restrict__ cnt, float* __restrict__ sum) {
  unsigned long long mask[HW_ROWS], any = 0;
#pragma unroll
  for (int k = 0; k < HW_ROWS; ++k) {
    mask[k] = __ballot(nd[k] >= a && nd[k] - a < width);
    any |= mask[k];
  }
  if (any == 0) return;
  int lwl = 0;                       // log2 of the lanes per row
  while ((1 << lwl) < fcw) ++lwl;    // fcw <= HW_FEATS = WAVE
  const int lw = 1 << lwl, rps = WAVE >> lwl;     // rows per step
  const int lane = threadIdx.x & (WAVE - 1);
  const int r = lane >> lwl, j = lane & (lw - 1);
  for (int s = 0; s < lw; ++s) {
    const int src = s * rps + r;     // the lane that holds this lane's row
    const unsigned long long rows = (rps == WAVE ? ~0ull : (1ull << rps) - 1)
                                    << (s * rps);
    if ((any & rows) == 0) continue;                 // wave-uniform
    bool act[HW_ROWS];
    int o[HW_ROWS], n[HW_ROWS];
    float rr[HW_ROWS];
#pragma unroll
    for (int k = 0; k < HW_ROWS; ++k) {
      act[k] = (mask[k] >> src) & 1;
      o[k] = __shfl(ord[k], src, WAVE);
      n[k] = __shfl(nd[k], src, WAVE);
      rr[k] = __shfl(res[k], src, WAVE);
    }
    int b[HW_ROWS];
#pragma unroll
    for (int k = 0; k < HW_ROWS; ++k)
      b[k] = act[k] && j < fcw ? bins[(int64_t)o[k] * F + f0 + j] : -1;
#pragma unroll
    for (int k = 0; k < HW_ROWS; ++k) {
      if ((unsigned)b[k] >= (unsigned)nb) continue;
      if (DIRECT) {
        const int64_t g = ((int64_t)n[k] * F + f0 + j) * nb + b[k];
        atomicAdd(&cnt[g], 1.f);
        atomicAdd(&sum[g], rr[k]);
      } else {
        const int c = ((n[k] - a) * fcw + j) * nb + b[k];
        atomicAdd(&lcnt[c], 1.f);
        atomicAdd(&lsum[c], rr[k]);
      }
    }
  }
}

__global__ __launch_bounds__(HW_THREADS) void gbt_hist_wide_kernel(
    const int* __restrict__ bins,       // [B, F]
    const int64_t* __restrict__ order,  // [B] rows in node order
    const int* __restrict__ snode,      // [B] node[order], ascending
    const float* __restrict__ resid,    // [B]
    float* __restrict__ cnt,            // [n_nodes, F, nb]
    float* __restrict__ sum,            // [n_nodes, F, nb]
    int B, int F, int nb, int n_nodes, int fper, int direct_ratio) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  int* hdr = reinterpret_cast<int*>(lds);  // pass bounds, before the cells
  const int tid = threadIdx.x;
  const int fbeg = blockIdx.y * fper, fend = min(F, fbeg + fper);
  const int G = HW_CELLS / nb;             // nodes a pass can hold, >= 1

  int ord[HW_ROWS], nd[HW_ROWS];
  float res[HW_ROWS];
  const int64_t w0 = (int64_t)blockIdx.x * HW_SLICE +
                     (tid / WAVE) * HW_WAVE_ROWS + (tid & (WAVE - 1));
#pragma unroll
  for (int k = 0; k < HW_ROWS; ++k) {
    const int64_t i = w0 + k * WAVE;
    const bool in = i < B;
    const int64_t o = in ? order[i] : 0;
    const int n = in ? snode[i] : -1;
    const bool ok = in && (uint64_t)o < (uint64_t)B &&
                    (unsigned)n < (unsigned)n_nodes;
    ord[k] = ok ? (int)o : 0;
    nd[k] = ok ? n : -1;                   // -1: never taken by a pass
    res[k] = resid[ord[k]];
  }

  // The first round (width 0) takes nothing and finds the slice's first node.
  int a = 0, width = 0;
  for (;;) {
    if (tid == 0) { hdr[0] = 0; hdr[1] = a; hdr[2] = INT_MAX; }
    __syncthreads();
    int c = 0, mx = a, mn = INT_MAX;
#pragma unroll
    for (int k = 0; k < HW_ROWS; ++k) {
      if (nd[k] < a) continue;
      if (nd[k] - a < width) { ++c; mx = max(mx, nd[k]); }
      else mn = min(mn, nd[k]);
    }
    if (c) { atomicAdd(&hdr[0], c); atomicMax(&hdr[1], mx); }
    if (mn != INT_MAX) atomicMin(&hdr[2], mn);
    __syncthreads();
    const int rows = hdr[0], span = hdr[1] - a + 1, next = hdr[2];
    __syncthreads();                       // hdr is read; the cells may go in

    if (rows > 0) {
      const int cells1 = span * nb;        // cells per feature, <= HW_CELLS
      if (direct_ratio > 0 && (int64_t)rows * direct_ratio < cells1) {
        hw_accumulate<true>(bins, ord, nd, res, a, width, F, nb, fbeg,
                            fend - fbeg, nullptr, nullptr, cnt, sum);
      } else {
        const int fc = HW_CELLS / cells1;
        for (int f0 = fbeg; f0 < fend; f0 += fc) {
          const int fcw = min(fc, fend - f0);
          const int ncell = cells1 * fcw;
          float* lcnt = lds;
          float* lsum = lds + ncell;
          float4* z = reinterpret_cast<float4*>(lds);
          for (int i = tid; i < ncell / 2; i += HW_THREADS)
            z[i] = make_float4(0.f, 0.f, 0.f, 0.f);
          if (tid < 2 && (ncell & 1)) lds[2 * ncell - 1 - tid] = 0.f;
          __syncthreads();
          hw_accumulate<false>(bins, ord, nd, res, a, width, F, nb, f0, fcw,
                               lcnt, lsum, cnt, sum);
          __syncthreads();
          for (int i = tid; i < ncell; i += HW_THREADS) {
            const float cc = lcnt[i];
            if (cc == 0.f) continue;
            const int n = i / (fcw * nb);
            const int rem = i - n * fcw * nb;
            const int j = rem / nb;
            const int64_t g =
                ((int64_t)(a + n) * F + f0 + j) * nb + (rem - j * nb);
            atomicAdd(&cnt[g], cc);
            atomicAdd(&sum[g], lsum[i]);
          }
          __syncthreads();
        }
      }
    }
    if (next == INT_MAX) break;
    a = next;
    width = G;
  }
}

}  // namespace

// Launches K10w; the caller (gbt_hist, gbt.hip) has checked every tensor,
// that B, F >= 1 and that 1 <= nb <= 8192. cnt and sum are zeroed
// [n_nodes, F, nb].
void gbt_hist_wide_launch(const char* op, const torch::Tensor& bins,
                          const torch::Tensor& resid,
                          const torch::Tensor& node, torch::Tensor& cnt,
                          torch::Tensor& sum) {
  const int64_t B = bins.size(0), F = bins.size(1);
  const int64_t n_nodes = cnt.size(0), nb = cnt.size(2);
  static_assert(HW_CELLS == 8192, "gbt_hist admits nb <= 8192");
  // rows grouped by node: [sorted node ids, permutation]
  auto sorted = torch::sort(node, /*stable=*/true, /*dim=*/0,
                            /*descending=*/false);
  const torch::Tensor snode = std::get<0>(sorted).contiguous();
  const torch::Tensor order = std::get<1>(sorted).contiguous();
  const int64_t slices = (B + HW_SLICE - 1) / HW_SLICE;
  // feature ranges only as far as needed to fill the chip (~512 workgroups)
  const int64_t want = std::min(F, std::max<int64_t>(1, 512 / slices));
  const int64_t fper = std::min<int64_t>((F + want - 1) / want, HW_FEATS);
  const int64_t franges = (F + fper - 1) / fper;
  // HARMONY_GBT_HIST_DIRECT=0 keeps every pass in LDS (measurement only)
  const char* env = std::getenv("HARMONY_GBT_HIST_DIRECT");
  const int ratio = env != nullptr && env[0] == '0' ? 0 : kDirectRatio;
  hipLaunchKernelGGL(gbt_hist_wide_kernel,
                     dim3((unsigned)slices, (unsigned)franges),
                     dim3(HW_THREADS), (size_t)2 * HW_CELLS * sizeof(float),
                     current_stream(), bins.data_ptr<int>(),
                     order.data_ptr<int64_t>(), snode.data_ptr<int>(),
                     resid.data_ptr<float>(), cnt.data_ptr<float>(),
                     sum.data_ptr<float>(), (int)B, (int)F, (int)nb,
                     (int)n_nodes, (int)fper, ratio);
  check_hip(op, hipGetLastError(), "launching K10w");
}
