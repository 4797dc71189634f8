// K11L — Lasso cyclic coordinate descent for batches past K11's LDS limit:
// 16368 to 65536 rows, one whole sweep in one launch. Reached through the
// lasso_cd binding (lasso.hip), which keeps K11 for every batch K11 takes.
//
// Coordinate descent is sequential across coordinates, so this is still one
// workgroup of 1024 threads. What differs from K11 is where the residual
// lives and how often a column is read:
//   * thread t owns rows t, t + 1024, ... and keeps the first R of them
//     (R = 16 or 32: up to 32768 rows) in registers for the whole sweep;
//     rows from 32768 up live in LDS (LdsPart, 128 KiB), each cell read and
//     written by its owner alone. So the residual needs no barrier at all;
//   * the register rows' column values are read once and serve both the dot
//     product and the update. The first P of them are loaded a coordinate
//     ahead, before the reduce and the soft-threshold of the coordinate
//     before: they do not depend on r, so their latency sits behind the
//     reduction. P = 16, or 8 beside an LDS part: a second whole column of
//     32 would not fit the 128 VGPRs a wave has at 1024 threads, and the
//     rest is loaded first thing in its own coordinate. The LDS rows' values
//     do not fit beside them either and are read again for the update,
//     kLdsChunk at a time;
//   * the dot product is a wave sum plus 16 cross-wave partials in LDS,
//     double-buffered by the parity of the coordinate, which puts a barrier
//     between a read of one buffer and its next write: one barrier per
//     coordinate. Every thread adds the same partials in the same order and
//     computes the same new weight, so there is no broadcast slot and the
//     d == 0 skip is uniform.
//
// The update is K11's, which is the loop at the bottom of ops.lasso_cd:
//   c = x.r + w[f] col_sq[f];  wn = sign(c) max(|c| - lam_n, 0) / col_sq[f];
//   r += x (w[f] - wn).
// No atomics: the summation order depends on (B, F) alone, so two runs give
// the same bits. A row index at or past B is never dereferenced; such a
// thread slot holds x = r = 0.

#include "hip_common.h"

namespace {

constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / WAVE;
constexpr int kLdsRows = 32 * kThreads;       // rows 32768 .. 65535
constexpr int kLdsChunk = 8;                  // LDS rows per thread per step
constexpr int64_t kMaxRows = 32 * kThreads + kLdsRows;

// This thread's value of the kThreads rows that start at the (uniform) row
// `row` of the column x; 0 past the batch. (Loads made unconditional, by
// clamping the index or by reading the last chunk from the batch's last
// kThreads rows, leave so many loop-invariant indices and masks in registers
// that the R = 32 kernels spill; under a predicate they do not.)
__device__ __forceinline__ float col_at(const float* __restrict__ x, int row,
                                        int tid, int B) {
  return tid < B - row ? (x + row)[tid] : 0.f;
}

template <int R, bool LdsPart>
__global__ __launch_bounds__(kThreads) void lasso_cd_large_kernel(
    const float* __restrict__ Xt, float* __restrict__ r_g, float* w,
    const float* __restrict__ col_sq, float lam_n, int B, int F) {
  constexpr int P = LdsPart ? 8 : 16;      // column values held ahead
  constexpr int kRegRows = R * kThreads;
  __shared__ float partial[2][kWaves];
  __shared__ float rl[LdsPart ? kLdsRows : 1];
  const int tid = threadIdx.x, wid = tid / WAVE, lane = tid % WAVE;
  if (F == 0) return;

  float r[R];
#pragma unroll
  for (int k = 0; k < R; ++k) r[k] = col_at(r_g, k * kThreads, tid, B);
  // chunks of kLdsChunk * kThreads LDS rows that hold a row of the batch
  const int lds_steps =
      LdsPart ? (B - kRegRows + kLdsChunk * kThreads - 1) /
                    (kLdsChunk * kThreads)
              : 0;
  if (LdsPart) {
    for (int k = 0; k < kLdsRows / kThreads; ++k)
      rl[tid + k * kThreads] =
          col_at(r_g, kRegRows + k * kThreads, tid, B);
  }

  float xn[P];
#pragma unroll
  for (int k = 0; k < P; ++k) xn[k] = col_at(Xt, k * kThreads, tid, B);
  float wi_n = w[0], cs_n = col_sq[0];

  for (int f = 0; f < F; ++f) {
    const float* __restrict__ x = Xt + (long)f * B;
    const float wi = wi_n, cs = cs_n;
    float xc[R];
#pragma unroll
    for (int k = P; k < R; ++k) xc[k] = col_at(x, k * kThreads, tid, B);
#pragma unroll
    for (int k = 0; k < P; ++k) xc[k] = xn[k];
    if (f + 1 < F) {
#pragma unroll
      for (int k = 0; k < P; ++k)
        xn[k] = col_at(x + B, k * kThreads, tid, B);
      wi_n = w[f + 1];
      cs_n = col_sq[f + 1];
    }

    float a[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < R; ++k) a[k & 3] += xc[k] * r[k];
    if (LdsPart) {
      for (int s = 0; s < lds_steps; ++s) {
        const int j0 = tid + s * kLdsChunk * kThreads;
        float xv[kLdsChunk];
#pragma unroll
        for (int u = 0; u < kLdsChunk; ++u)
          xv[u] = col_at(x, kRegRows + j0 - tid + u * kThreads, tid, B);
#pragma unroll
        for (int u = 0; u < kLdsChunk; ++u)
          a[u & 3] += xv[u] * rl[j0 + u * kThreads];
      }
    }
    float c = wave_sum_uniform((a[0] + a[1]) + (a[2] + a[3]));
    float* pp = partial[f & 1];
    if (lane == 0) pp[wid] = c;
    __syncthreads();
    c = 0.f;
#pragma unroll
    for (int q = 0; q < kWaves; ++q) c += pp[q];

    c += wi * cs;
    const float sgn = (c > 0.f) ? 1.f : ((c < 0.f) ? -1.f : 0.f);
    const float wn = fmaxf(fabsf(c) - lam_n, 0.f) * sgn / cs;
    const float d = wi - wn;
    if (tid == 0) w[f] = wn;
    if (d != 0.f) {
#pragma unroll
      for (int k = 0; k < R; ++k) r[k] += xc[k] * d;
      if (LdsPart) {
        for (int s = 0; s < lds_steps; ++s) {
          const int j0 = tid + s * kLdsChunk * kThreads;
          float xv[kLdsChunk];
#pragma unroll
          for (int u = 0; u < kLdsChunk; ++u)
            xv[u] = col_at(x, kRegRows + j0 - tid + u * kThreads, tid, B);
#pragma unroll
          for (int u = 0; u < kLdsChunk; ++u)
            rl[j0 + u * kThreads] += xv[u] * d;
        }
      }
    }
  }

#pragma unroll
  for (int k = 0; k < R; ++k) {
    const int i = tid + k * kThreads;
    if (i < B) r_g[i] = r[k];
  }
  if (LdsPart) {
    for (int i = kRegRows + tid; i < B; i += kThreads)
      r_g[i] = rl[i - kRegRows];
  }
}

}  // namespace

// The largest batch lasso_cd takes.
int64_t lasso_cd_max_rows() { return kMaxRows; }

// One sweep by K11L; lasso_cd has checked the arguments and that
// B <= lasso_cd_max_rows().
void lasso_cd_large_launch(const float* Xt, float* r, float* w,
                           const float* col_sq, float lam_n, int B, int F,
                           hipStream_t stream) {
  const int regs = B <= 16 * kThreads ? 16 : 32;
  dispatch_pow2<16, 32>("lasso_cd", "rows per thread", regs, [&](auto R) {
    dispatch_bool(B > R.value * kThreads, [&](auto lds_part) {
      // an LDS part goes with 32 register rows only
      if constexpr (R.value == 32 || !lds_part.value) {
        hipLaunchKernelGGL(
            (lasso_cd_large_kernel<R.value, lds_part.value>), dim3(1),
            dim3(kThreads), 0, stream, Xt, r, w, col_sq, lam_n, B, F);
      }
    });
  });
}
