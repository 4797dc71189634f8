// K4-BF16: the MLR step on bf16 training data (app arg data_dtype=bfloat16),
// v_mfma_f32_16x16x32_bf16 on gfx950, wave64.
//
// X [B, F] is stored as bf16 and is exact. The float32 multiplicands (W in
// the forward, P = softmax - onehot in the gradient) are split into three
// bf16 terms h = bf16(v), m = bf16(v - h), l = bf16(v - h - m) with
// h + m + l == v; a bf16 x bf16 product is exact in float32, so one X
// fragment feeds three MFMAs into float32 accumulators and the result
// differs from the exact dot product of the float32 values by float32
// accumulation rounding alone. The model, P, the gradient and the push stay
// float32. No atomics: split-F and split-B partials go to scratch and are
// summed in a fixed order, so every output is bit-identical run to run.
//
//   split_wt   Wt [F][16] f32 -> planes [3][16][F] bf16 (1.5 MiB at
//              F = 16384, L2-resident): the forward's B fragment (class c,
//              8 consecutive f) is one 16-byte load.
//   fwd        a wave owns 64 rows = 4 MFMA row tiles and walks its f-range
//              64 at a time; the A fragment is 16 bytes straight from X's
//              row, no LDS. Lane group g = lane / 16 takes f0 + 16 g .. + 15
//              for both operands (a k-permutation common to A and B), so a
//              wave's loads cover 128 contiguous bytes of every row, and the
//              W fragments are reused by the 4 row tiles from registers.
//              8 independent accumulator chains per wave.
//   softmax    sums the split-F partials in order; softmax - onehot with
//              the log-sum-exp guard of mlr_softmax_pad_kernel; P f32
//              [B][16] with classes >= C zero; per-row cross entropy and hit
//              flag; P's three bf16 planes transposed [3][16][Bp], so the
//              gradient's A fragment (class c, 8 consecutive b) is one
//              16-byte load.
//   grad       gradT[c][f] = sum_b P[b][c] X[b][f], k = b. A workgroup owns
//              128 f and streams 64 rows per stage: coalesced 16-byte loads
//              of whole 256-byte row pieces, prefetched in registers while
//              the previous stage computes. X's fragment is a column walk:
//              rows are staged in LDS 66 dwords apart and a lane reads the
//              dword of columns (2j, 2j + 1) in 8 consecutive rows, which
//              yields the fragments of two f-tiles (even and odd columns;
//              the store interleaves them back). The 66-dword stride puts
//              lane groups g and g + 1 on opposite halves of the 32 banks.
//              P planes are staged next to it and read 16 bytes per lane.
//              Rows outside the split's range are zeroed on load.
//   reduce     split-B partials [splitb][16][F] summed in order.
//
// Shapes: C <= 16, F % 32 == 0, any B and any row window. Measured A/B
// against the float32 rocBLAS pair: scripts/mlr_bf16_ab.py,
// profiles/mlr_bf16_ab.md.

#include "hip_common.h"

namespace {

using f32x4 = __attribute__((ext_vector_type(4))) float;
using u32x4 = __attribute__((ext_vector_type(4))) unsigned int;
using u32x2 = __attribute__((ext_vector_type(2))) unsigned int;
using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
typedef unsigned short bf16_t;      // raw bits

constexpr int CPAD = 16;            // class dim padded to one MFMA tile
constexpr int FW_ROWS = 256;        // forward: rows per workgroup, 4 waves x 64
constexpr int GT_F = 128;           // gradient: f per workgroup, 4 waves x 32
constexpr int GT_B = 64;            // gradient: rows per LDS stage, 2 k-steps
constexpr int XS_LD = GT_F / 2 + 2; // dwords between staged X rows
constexpr int PS_LD = GT_B + 8;     // bf16 between staged P plane rows

// No packed fp32 arithmetic in these kernels: the three-term split has to be
// exact and the outputs bit-identical, and nothing here is bound by the VALU.
#if defined(__HIP_DEVICE_COMPILE__)
#define MLR_BF16_KERNEL __attribute__((target("no-packed-fp32-ops")))
#else
#define MLR_BF16_KERNEL
#endif

// float32 -> bf16 bits, round to nearest even (torch's .to(bfloat16)).
__device__ __forceinline__ unsigned bf16_rne(float v) {
  const unsigned u = __float_as_uint(v);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (u >> 16) | 0x40u;   // NaN
  return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}

__device__ __forceinline__ void split3(float v, unsigned (&t)[3]) {
  t[0] = bf16_rne(v);
  float r = v - __uint_as_float(t[0] << 16);
  t[1] = bf16_rne(r);
  r -= __uint_as_float(t[1] << 16);
  t[2] = bf16_rne(r);
}

__device__ __forceinline__ f32x4 mfma_bf16(u32x4 a, u32x4 b, f32x4 acc) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(
      __builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), acc, 0, 0,
      0);
}

__device__ __forceinline__ u32x4 load16(const bf16_t* p) {
  return *reinterpret_cast<const u32x4*>(p);
}

__device__ __forceinline__ long lmin(long a, long b) { return a < b ? a : b; }

// ------------------------------------------------------------ W^T planes
// One thread per (c, f): planes[p][c][f], writes coalesced along f.
__global__ MLR_BF16_KERNEL
void mlr_bf16_split_wt_kernel(const float* __restrict__ Wt,    // [F][16]
                              bf16_t* __restrict__ planes,     // [3][16][F]
                              long F) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= CPAD * F) return;
  const long c = idx / F, f = idx - c * F;
  unsigned t[3];
  split3(Wt[f * CPAD + c], t);
#pragma unroll
  for (int p = 0; p < 3; ++p) planes[(p * CPAD + c) * F + f] = (bf16_t)t[p];
}

// ---------------------------------------------------------------- forward
// grid.x = ceil(n / 256), grid.y = splitf; block = 4 independent waves.
// X points at the window's first row; part is [splitf][n][16].
__global__ __launch_bounds__(256) MLR_BF16_KERNEL
void mlr_bf16_fwd_kernel(const bf16_t* __restrict__ X,
                         const bf16_t* __restrict__ Wp,        // [3][16][F]
                         float* __restrict__ part, int n, long F) {
  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int i = lane & 15;           // fragment row (A) / class (B)
  const int g = lane >> 4;           // fragment k group
  const long row0 = ((long)blockIdx.x * 4 + wave) * 64;
  if (row0 >= n) return;             // no barrier in this kernel
  const long f_per = F / gridDim.y;
  const long f_lo = (long)blockIdx.y * f_per;
  const long f_hi = f_lo + f_per;

  // rows past the window are clamped to its last row and never stored
  const bf16_t* xrow[4];
#pragma unroll
  for (int t = 0; t < 4; ++t)
    xrow[t] = X + lmin(row0 + t * 16 + i, (long)n - 1) * F;
  const bf16_t* wrow[3];
#pragma unroll
  for (int p = 0; p < 3; ++p) wrow[p] = Wp + (long)(p * CPAD + i) * F;

  f32x4 acc[4][2];
#pragma unroll
  for (int t = 0; t < 4; ++t)
    acc[t][0] = acc[t][1] = f32x4{0.f, 0.f, 0.f, 0.f};

  long f = f_lo;
  for (; f + 64 <= f_hi; f += 64) {
    const long fo = f + 16 * g;      // this lane group's 16 f of the 64
    u32x4 a[4][2], b[3][2];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      a[t][0] = load16(xrow[t] + fo);
      a[t][1] = load16(xrow[t] + fo + 8);
    }
#pragma unroll
    for (int p = 0; p < 3; ++p) {
      b[p][0] = load16(wrow[p] + fo);
      b[p][1] = load16(wrow[p] + fo + 8);
    }
#pragma unroll
    for (int p = 0; p < 3; ++p)
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        acc[t][0] = mfma_bf16(a[t][0], b[p][0], acc[t][0]);
        acc[t][1] = mfma_bf16(a[t][1], b[p][1], acc[t][1]);
      }
  }
  if (f < f_hi) {                    // the f-range is a multiple of 32
    const long fo = f + 8 * g;
    u32x4 a[4], b[3];
#pragma unroll
    for (int t = 0; t < 4; ++t) a[t] = load16(xrow[t] + fo);
#pragma unroll
    for (int p = 0; p < 3; ++p) b[p] = load16(wrow[p] + fo);
#pragma unroll
    for (int p = 0; p < 3; ++p)
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[t][0] = mfma_bf16(a[t], b[p], acc[t][0]);
  }
  // D: lane holds class i of rows 4 g + q
  float* dst = part + (long)blockIdx.y * n * CPAD;
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const long r = row0 + t * 16 + 4 * g + q;
      if (r < n) dst[r * CPAD + i] = acc[t][0][q] + acc[t][1][q];
    }
}

// Sum of the split-F partials of one row, in order.
__device__ __forceinline__ void sum_partials(const float* __restrict__ part,
                                             int splitf, int n, int row,
                                             float (&z)[CPAD]) {
#pragma unroll
  for (int j = 0; j < CPAD; ++j) z[j] = 0.f;
  for (int s = 0; s < splitf; ++s) {
    const float4* src = reinterpret_cast<const float4*>(
        part + ((long)s * n + row) * CPAD);
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const float4 x = src[v];
      z[4 * v + 0] += x.x; z[4 * v + 1] += x.y;
      z[4 * v + 2] += x.z; z[4 * v + 3] += x.w;
    }
  }
}

// mlr_fwd_mfma_part with splitf > 1: logits of the window into P.
__global__ MLR_BF16_KERNEL
void mlr_bf16_logit_reduce_kernel(const float* __restrict__ part, int splitf,
                                  float* __restrict__ P, int n) {
  const int row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= n) return;
  float z[CPAD];
  sum_partials(part, splitf, n, row, z);
  float4* dst = reinterpret_cast<float4*>(P + (long)row * CPAD);
#pragma unroll
  for (int v = 0; v < 4; ++v)
    dst[v] = make_float4(z[4 * v], z[4 * v + 1], z[4 * v + 2], z[4 * v + 3]);
}

// Row `row` of P^T's planes [3][16][Bp]: consecutive threads write
// consecutive bf16 of each plane row.
__device__ __forceinline__ void store_planes(bf16_t* __restrict__ PT, int Bp,
                                             int row, const float (&p)[CPAD]) {
#pragma unroll
  for (int j = 0; j < CPAD; ++j) {
    unsigned t[3];
    split3(p[j], t);
#pragma unroll
    for (int k = 0; k < 3; ++k)
      PT[(long)(k * CPAD + j) * Bp + row] = (bf16_t)t[k];
  }
}

// ------------------------------------------------- softmax epilogue, step
// One thread per row of Bp = n rounded up to 8; rows >= n zero the planes.
__global__ MLR_BF16_KERNEL
void mlr_bf16_softmax_kernel(const float* __restrict__ part, int splitf,
                             const int64_t* __restrict__ labels,
                             float* __restrict__ P,            // [n][16]
                             float* __restrict__ ce, int* __restrict__ hit,
                             bf16_t* __restrict__ PT, int n, int Bp, int C) {
  const int row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= Bp) return;
  float z[CPAD];
  if (row >= n) {
#pragma unroll
    for (int j = 0; j < CPAD; ++j) z[j] = 0.f;
    store_planes(PT, Bp, row, z);
    return;
  }
  sum_partials(part, splitf, n, row, z);
  const int lab = (int)labels[row];
  float m = -1e30f, zlab = 0.f;
  int argmax = 0;
#pragma unroll
  for (int j = 0; j < CPAD; ++j) {
    if (j < C && z[j] > m) { m = z[j]; argmax = j; }
    if (j == lab) zlab = z[j];
  }
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < CPAD; ++j) {
    z[j] = j < C ? __expf(z[j] - m) : 0.f;
    s += z[j];
  }
  const float inv = 1.f / s;
#pragma unroll
  for (int j = 0; j < CPAD; ++j)
    z[j] = j < C ? z[j] * inv - (j == lab ? 1.f : 0.f) : 0.f;
  ce[row] = m + __logf(s) - zlab;
  hit[row] = argmax == lab ? 1 : 0;
  float4* dst = reinterpret_cast<float4*>(P + (long)row * CPAD);
#pragma unroll
  for (int v = 0; v < 4; ++v)
    dst[v] = make_float4(z[4 * v], z[4 * v + 1], z[4 * v + 2], z[4 * v + 3]);
  store_planes(PT, Bp, row, z);
}

// mlr_grad_mfma_part: the window's rows of a float32 P into planes.
__global__ MLR_BF16_KERNEL
void mlr_bf16_split_p_kernel(const float* __restrict__ P,      // window rows
                             bf16_t* __restrict__ PT, int n, int Bp) {
  const int row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= Bp) return;
  float z[CPAD];
#pragma unroll
  for (int j = 0; j < CPAD; ++j) z[j] = 0.f;
  if (row < n) {
    const float4* src = reinterpret_cast<const float4*>(P + (long)row * CPAD);
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const float4 x = src[v];
      z[4 * v] = x.x; z[4 * v + 1] = x.y; z[4 * v + 2] = x.z;
      z[4 * v + 3] = x.w;
    }
  }
  store_planes(PT, Bp, row, z);
}

// One stage's loads of the gradient into registers: 4 row pieces of X and
// up to 2 pieces of the P planes per thread, zero outside [.., b_hi).
__device__ __forceinline__ void grad_load_stage(
    const bf16_t* __restrict__ xsrc, const bf16_t* __restrict__ PT, long F,
    int Bp, long b0, long b_hi, bool fvalid, int tid, u32x4 (&xr)[4],
    u32x4 (&pr)[2]) {
  const u32x4 zero4 = {0u, 0u, 0u, 0u};
  const int srow = tid >> 4;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const long b = b0 + srow + 16 * u;
    xr[u] = fvalid && b < b_hi ? load16(xsrc + b * F) : zero4;
  }
#pragma unroll
  for (int v = 0; v < 2; ++v) {
    const int piece = tid + 256 * v;
    const long b = b0 + 8 * (piece & 7);
    pr[v] = piece < 3 * CPAD * 8 && b < b_hi
                ? load16(PT + (long)(piece >> 3) * Bp + b) : zero4;
  }
}

// ---------------------------------------------------------------- gradient
// grid.x = ceil(F / 128), grid.y = splitb; block = 256. Split s owns rows
// [s * per, min((s + 1) * per, n)), per % 32 == 0; gpart is [splitb][16][F].
__global__ __launch_bounds__(256) MLR_BF16_KERNEL
void mlr_bf16_grad_kernel(const bf16_t* __restrict__ X,        // window rows
                          const bf16_t* __restrict__ PT,       // [3][16][Bp]
                          float* __restrict__ gpart, int n, int Bp, long F,
                          int per) {
  __shared__ unsigned int xs[GT_B * XS_LD];
  __shared__ __attribute__((aligned(16))) bf16_t ps[3 * CPAD * PS_LD];
  const int tid = threadIdx.x;
  const int wave = tid >> 6;
  const int lane = tid & 63;
  const int j = lane & 15;           // class (A) / column pair (B)
  const int g = lane >> 4;           // fragment k group
  const long fblk = (long)blockIdx.x * GT_F;
  const long b_lo = (long)blockIdx.y * per;
  const long b_hi = lmin(b_lo + per, (long)n);
  const int nstage = b_hi > b_lo ? (int)((b_hi - b_lo + GT_B - 1) / GT_B) : 0;

  // staging: thread -> row srow + 16 u of the stage, 8 columns from 8 sc;
  // P planes: 48 plane rows x 8 pieces of 8 b, 384 pieces over 256 threads
  const int srow = tid >> 4;
  const int sc = tid & 15;
  const bool fvalid = fblk + 8 * sc < F;
  const bf16_t* xsrc = X + fblk + 8 * sc;
  u32x4 xr[4], pr[2];

  f32x4 acc[2][2];
#pragma unroll
  for (int t = 0; t < 2; ++t)
    acc[t][0] = acc[t][1] = f32x4{0.f, 0.f, 0.f, 0.f};

  if (nstage > 0)
    grad_load_stage(xsrc, PT, F, Bp, b_lo, b_hi, fvalid, tid, xr, pr);
  for (int st = 0; st < nstage; ++st) {
    __syncthreads();                 // the previous stage has been read
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      u32x2* dst = reinterpret_cast<u32x2*>(
          &xs[(srow + 16 * u) * XS_LD + 4 * sc]);
      dst[0] = u32x2{xr[u].x, xr[u].y};
      dst[1] = u32x2{xr[u].z, xr[u].w};
    }
#pragma unroll
    for (int v = 0; v < 2; ++v) {
      const int piece = tid + 256 * v;
      if (piece < 3 * CPAD * 8)
        *reinterpret_cast<u32x4*>(
            &ps[(piece >> 3) * PS_LD + 8 * (piece & 7)]) = pr[v];
    }
    __syncthreads();
    if (st + 1 < nstage)
      grad_load_stage(xsrc, PT, F, Bp, b_lo + (long)(st + 1) * GT_B, b_hi,
                      fvalid, tid, xr, pr);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      // dword (columns 2 j, 2 j + 1) of rows 32 ks + 8 g .. + 7
      unsigned d[8];
#pragma unroll
      for (int kk = 0; kk < 8; ++kk)
        d[kk] = xs[(32 * ks + 8 * g + kk) * XS_LD + wave * 16 + j];
      u32x4 even, odd;
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        even[w] = (d[2 * w] & 0xffffu) | (d[2 * w + 1] << 16);
        odd[w] = (d[2 * w] >> 16) | (d[2 * w + 1] & 0xffff0000u);
      }
#pragma unroll
      for (int p = 0; p < 3; ++p) {
        const u32x4 a = *reinterpret_cast<const u32x4*>(
            &ps[(p * CPAD + j) * PS_LD + 32 * ks + 8 * g]);
        acc[0][ks] = mfma_bf16(a, even, acc[0][ks]);
        acc[1][ks] = mfma_bf16(a, odd, acc[1][ks]);
      }
    }
  }
  // D: lane holds column pair j of classes 4 g + q
  const long f = fblk + wave * 32 + 2 * j;
  if (f < F) {
    const f32x4 even = acc[0][0] + acc[0][1], odd = acc[1][0] + acc[1][1];
    float* dst = gpart + ((long)blockIdx.y * CPAD + 4 * g) * F + f;
    *reinterpret_cast<float2*>(dst) = make_float2(even.x, odd.x);
    *reinterpret_cast<float2*>(dst + F) = make_float2(even.y, odd.y);
    *reinterpret_cast<float2*>(dst + 2 * F) = make_float2(even.z, odd.z);
    *reinterpret_cast<float2*>(dst + 3 * F) = make_float2(even.w, odd.w);
  }
}

// gradT[c][f] += sum over the splits, in order.
__global__ MLR_BF16_KERNEL
void mlr_bf16_grad_reduce_kernel(const float* __restrict__ gpart, int splitb,
                                 float* __restrict__ gradT, long F) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= CPAD * F) return;
  float s = gradT[idx];
  for (int k = 0; k < splitb; ++k) s += gpart[(long)k * CPAD * F + idx];
  gradT[idx] = s;
}

// -------------------------------------------------------- checks, launches

struct Shape { int64_t B, F; };

// X bf16 [B, F] for the 16-byte fragment loads.
Shape check_x(const char* op, const torch::Tensor& X) {
  check_tensor(op, X, "X", torch::kBFloat16, {-1, -1});
  return {X.size(0), X.size(1)};
}

void check_x_layout(const char* op, const torch::Tensor& X) {
  TORCH_CHECK(X.size(1) >= 32 && X.size(1) % 32 == 0, op,
              ": X must be bfloat16 with F % 32 == 0, got F = ", X.size(1));
  TORCH_CHECK(aligned16(X.data_ptr()), op,
              ": X must be 16-byte aligned, got ", X.data_ptr());
}

void check_rows(const char* op, int64_t off, int64_t n, int64_t B) {
  TORCH_CHECK(off >= 0 && n >= 1 && off + n <= B, op,
              ": rows [off, off + n) must lie inside the batch of ", B,
              ", got off = ", off, ", n = ", n);
  check_below_2_31(op, {{"n", n}});
}

void check_splits(const char* op, int64_t F, int64_t splitf, int64_t splitb) {
  TORCH_CHECK(splitf >= 1 && splitf <= 65535 && F % (32 * splitf) == 0, op,
              ": splitf must be in 1..65535 with F % (32 * splitf) == 0, got ",
              splitf, " for F = ", F);
  TORCH_CHECK(splitb >= 1 && splitb <= 65535, op,
              ": splitb must be in 1..65535, got ", splitb);
}

const bf16_t* bf16_ptr(const torch::Tensor& t) {
  return reinterpret_cast<const bf16_t*>(t.data_ptr());
}

bf16_t* bf16_ptr(torch::Tensor& t) {
  return reinterpret_cast<bf16_t*>(t.data_ptr());
}

torch::Tensor split_wt(const torch::Tensor& Wt) {
  const int64_t F = Wt.size(0);
  auto planes = torch::empty({3, CPAD, F}, Wt.options().dtype(torch::kBFloat16));
  hipLaunchKernelGGL(mlr_bf16_split_wt_kernel, dim3((CPAD * F + 255) / 256),
                     dim3(256), 0, current_stream(), Wt.data_ptr<float>(),
                     bf16_ptr(planes), (long)F);
  return planes;
}

// Partial logits of rows [off, off + n) into part [splitf][n][16].
void launch_fwd(const torch::Tensor& X, const torch::Tensor& planes,
                float* part, int64_t off, int64_t n, int64_t splitf) {
  const int64_t F = X.size(1);
  hipLaunchKernelGGL(mlr_bf16_fwd_kernel,
                     dim3((n + FW_ROWS - 1) / FW_ROWS, splitf), dim3(256), 0,
                     current_stream(), bf16_ptr(X) + off * F, bf16_ptr(planes),
                     part, (int)n, (long)F);
}

// gradT += P^T X over rows [off, off + n), P as planes [3][16][Bp].
void launch_grad(const torch::Tensor& X, const torch::Tensor& PT,
                 torch::Tensor& gradT, int64_t off, int64_t n,
                 int64_t splitb) {
  const int64_t F = X.size(1), Bp = PT.size(2);
  // rows per split: a multiple of the MFMA k-step
  const int64_t per = ((n + splitb - 1) / splitb + 31) / 32 * 32;
  auto gpart = torch::empty({splitb, CPAD, F}, gradT.options());
  hipLaunchKernelGGL(mlr_bf16_grad_kernel,
                     dim3((F + GT_F - 1) / GT_F, splitb), dim3(256), 0,
                     current_stream(), bf16_ptr(X) + off * F, bf16_ptr(PT),
                     gpart.data_ptr<float>(), (int)n, (int)Bp, (long)F,
                     (int)per);
  hipLaunchKernelGGL(mlr_bf16_grad_reduce_kernel,
                     dim3((CPAD * F + 255) / 256), dim3(256), 0,
                     current_stream(), gpart.data_ptr<float>(), (int)splitb,
                     gradT.data_ptr<float>(), (long)F);
}

}  // namespace

// The bf16 branches of mlr_fwd_mfma_part, mlr_grad_mfma_part and
// mlr_step_mfma (mlr_mfma.hip dispatches on X's dtype); `op` is the entry's
// name for the messages.

void mlr_bf16_fwd_part(const char* op, torch::Tensor X, torch::Tensor Wt,
                       torch::Tensor P, int64_t off, int64_t n,
                       int64_t splitf) {
  const Shape s = check_x(op, X);
  check_tensor(op, Wt, "Wt", torch::kFloat32, {s.F, CPAD});
  check_tensor(op, P, "P", torch::kFloat32, {s.B, CPAD});
  check_x_layout(op, X);
  check_rows(op, off, n, s.B);
  check_splits(op, s.F, splitf, 1);
  check_on_device(op, {X, Wt, P});
  auto planes = split_wt(Wt);
  float* rows = P.data_ptr<float>() + off * CPAD;
  if (splitf == 1) {
    launch_fwd(X, planes, rows, off, n, 1);
    return;
  }
  auto part = torch::empty({splitf, n, CPAD}, P.options());
  launch_fwd(X, planes, part.data_ptr<float>(), off, n, splitf);
  hipLaunchKernelGGL(mlr_bf16_logit_reduce_kernel, dim3((n + 255) / 256),
                     dim3(256), 0, current_stream(), part.data_ptr<float>(),
                     (int)splitf, rows, (int)n);
}

void mlr_bf16_grad_part(const char* op, torch::Tensor P, torch::Tensor X,
                        torch::Tensor gradT, int64_t off, int64_t n,
                        int64_t splitb) {
  const Shape s = check_x(op, X);
  check_tensor(op, P, "P", torch::kFloat32, {s.B, CPAD});
  check_tensor(op, gradT, "gradT", torch::kFloat32, {CPAD, s.F});
  check_x_layout(op, X);
  check_rows(op, off, n, s.B);
  check_splits(op, s.F, 1, splitb);
  check_on_device(op, {P, X, gradT});
  const int64_t Bp = (n + 7) / 8 * 8;
  auto PT = torch::empty({3, CPAD, Bp}, X.options());
  hipLaunchKernelGGL(mlr_bf16_split_p_kernel, dim3((Bp + 255) / 256),
                     dim3(256), 0, current_stream(),
                     P.data_ptr<float>() + off * CPAD, bf16_ptr(PT), (int)n,
                     (int)Bp);
  launch_grad(X, PT, gradT, off, n, splitb);
}

std::vector<torch::Tensor> mlr_bf16_step(const char* op, torch::Tensor X,
                                         torch::Tensor Wt,
                                         torch::Tensor labels,
                                         int64_t row_block, int64_t C,
                                         int64_t splitf, int64_t splitb) {
  const Shape s = check_x(op, X);
  check_tensor(op, Wt, "Wt", torch::kFloat32, {s.F, CPAD});
  check_tensor(op, labels, "labels", torch::kInt64, {s.B});
  check_x_layout(op, X);
  check_rows(op, 0, s.B, s.B);
  TORCH_CHECK(row_block == 0, op, ": row_block must be 0 for bfloat16 X "
              "(no row-blocked variant), got ", row_block);
  TORCH_CHECK(C >= 1 && C <= CPAD, op, ": C must be in 1..16, got ", C);
  check_splits(op, s.F, splitf, splitb);
  check_on_device(op, {X, Wt, labels});
  const int64_t B = s.B, Bp = (B + 7) / 8 * 8;
  auto f32 = Wt.options();
  auto planes = split_wt(Wt);
  auto part = torch::empty({splitf, B, CPAD}, f32);
  launch_fwd(X, planes, part.data_ptr<float>(), 0, B, splitf);
  auto P = torch::empty({B, CPAD}, f32);
  auto ce = torch::empty({B}, f32);
  auto hit = torch::empty({B}, f32.dtype(torch::kInt32));
  auto PT = torch::empty({3, CPAD, Bp}, X.options());
  hipLaunchKernelGGL(mlr_bf16_softmax_kernel, dim3((Bp + 255) / 256),
                     dim3(256), 0, current_stream(), part.data_ptr<float>(),
                     (int)splitf, labels.data_ptr<int64_t>(),
                     P.data_ptr<float>(), ce.data_ptr<float>(),
                     hit.data_ptr<int>(), bf16_ptr(PT), (int)B, (int)Bp,
                     (int)C);
  auto gradT = torch::zeros({(int64_t)CPAD, s.F}, f32);
  launch_grad(X, PT, gradT, 0, B, splitb);
  return {gradT, ce.sum().reshape({1}),
          hit.sum().to(torch::kInt32).reshape({1})};
}
