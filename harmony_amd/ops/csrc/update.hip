// K3/K9: fused owner-side update application — the "server" compute.
// Reference semantics: BlockImpl.update via per-app UpdateFunction
// (NMFETModelUpdateFunction.java:48-52 axpy+clamp,
// MLRETModelUpdateFunction.java:60-62 add,
// LDAETModelUpdateFunction.java:43-64 count merge with clamp>=0).
// Here the aggregated deltas arriving from the push all-to-all are applied
// in ONE gather-modify-scatter kernel per table (vs 3+ torch launches).

#include "hip_common.h"

namespace {

enum Mode { ADD = 0, ASSIGN = 1, NMF_SGD = 2, LDA_COUNTS = 3 };

template <typename T>
__device__ __forceinline__ T apply_one(T v, T d, int mode, float step,
                                       float maxval) {
  switch (mode) {
    case ADD: return v + d;
    case ASSIGN: return d;
    case NMF_SGD: {
      float x = (float)v - step * (float)d;
      x = fminf(fmaxf(x, 0.f), maxval);
      return (T)x;
    }
    case LDA_COUNTS: {
      T x = v + d;
      return x < (T)0 ? (T)0 : x;
    }
  }
  return v;
}

// One lane group (G lanes, a power of two) per row: the row index is read
// once per group, then the row is swept in 16-byte pieces (VEC: vd % 4 == 0
// and 16-byte aligned bases) or element by element. No per-element divide.
template <typename T>
struct alignas(16) Vec4 { T v[4]; };

template <typename T, bool VEC>
__global__ void scatter_apply_kernel(T* __restrict__ shard,
                                     const int64_t* __restrict__ rows,
                                     const T* __restrict__ deltas,
                                     int64_t n, int vd, int log2g, int mode,
                                     float step, float maxval) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t i = t >> log2g;
  if (i >= n) return;
  const int lane = (int)(t & ((1 << log2g) - 1));
  const int g = 1 << log2g;
  T* dst = shard + rows[i] * vd;
  const T* src = deltas + i * vd;
  if (VEC) {
    for (int c = lane * 4; c < vd; c += g * 4) {
      Vec4<T> v = *reinterpret_cast<const Vec4<T>*>(dst + c);
      const Vec4<T> d = *reinterpret_cast<const Vec4<T>*>(src + c);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        v.v[j] = apply_one(v.v[j], d.v[j], mode, step, maxval);
      *reinterpret_cast<Vec4<T>*>(dst + c) = v;
    }
  } else {
    for (int c = lane; c < vd; c += g)
      dst[c] = apply_one(dst[c], src[c], mode, step, maxval);
  }
}

template <typename T>
__global__ void dense_apply_kernel(T* __restrict__ shard,
                                   const T* __restrict__ delta, int64_t n,
                                   int mode, float step, float maxval) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  shard[i] = apply_one(shard[i], delta[i], mode, step, maxval);
}

}  // namespace

template <typename T>
static void launch_scatter_apply(torch::Tensor& shard, torch::Tensor& rows,
                                 torch::Tensor& deltas, int64_t n, int vd,
                                 int mode, float step, float maxval) {
  T* sp = shard.data_ptr<T>();
  const T* dp = deltas.data_ptr<T>();
  const bool vec = vd % 4 == 0 &&
                   ((reinterpret_cast<uintptr_t>(sp) |
                     reinterpret_cast<uintptr_t>(dp)) & 15) == 0;
  const int units = vec ? vd / 4 : vd;   // accesses per row
  int log2g = 0;
  while (log2g < 6 && (1 << log2g) < units) ++log2g;
  const int64_t threads = n << log2g;
  dim3 blk(256), grid((unsigned)((threads + 255) / 256));
  if (vec)
    hipLaunchKernelGGL((scatter_apply_kernel<T, true>), grid, blk, 0,
                       current_stream(), sp, rows.data_ptr<int64_t>(), dp, n,
                       vd, log2g, mode, step, maxval);
  else
    hipLaunchKernelGGL((scatter_apply_kernel<T, false>), grid, blk, 0,
                       current_stream(), sp, rows.data_ptr<int64_t>(), dp, n,
                       vd, log2g, mode, step, maxval);
}

void scatter_apply(torch::Tensor shard, torch::Tensor rows,
                   torch::Tensor deltas, int64_t mode, double step,
                   double maxval) {
  CHECK_IN(shard); CHECK_IN(rows); CHECK_IN(deltas);
  const int64_t n = rows.size(0);
  const int vd = shard.size(1);
  if (n == 0 || vd == 0) return;
  if (shard.dtype() == torch::kFloat32) {
    launch_scatter_apply<float>(shard, rows, deltas, n, vd, (int)mode,
                                (float)step, (float)maxval);
  } else if (shard.dtype() == torch::kInt32) {
    launch_scatter_apply<int>(shard, rows, deltas, n, vd, (int)mode,
                              (float)step, (float)maxval);
  } else {
    TORCH_CHECK(false, "scatter_apply: unsupported dtype");
  }
}

void dense_apply(torch::Tensor shard, torch::Tensor delta, int64_t mode,
                 double step, double maxval) {
  CHECK_IN(shard); CHECK_IN(delta);
  const int64_t total = shard.numel();
  TORCH_CHECK(delta.numel() == total, "size mismatch");
  if (total == 0) return;
  dim3 blk(256), grid((unsigned)((total + 255) / 256));
  if (shard.dtype() == torch::kFloat32) {
    hipLaunchKernelGGL(dense_apply_kernel<float>, grid, blk, 0,
                       current_stream(), shard.data_ptr<float>(),
                       delta.data_ptr<float>(), total, (int)mode, (float)step,
                       (float)maxval);
  } else if (shard.dtype() == torch::kInt32) {
    hipLaunchKernelGGL(dense_apply_kernel<int>, grid, blk, 0,
                       current_stream(), shard.data_ptr<int>(),
                       delta.data_ptr<int>(), total, (int)mode, (float)step,
                       (float)maxval);
  } else {
    TORCH_CHECK(false, "dense_apply: unsupported dtype");
  }
}
