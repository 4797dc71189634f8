// K11 — Lasso cyclic coordinate descent, whole sweep in one launch.
//
// Reference LassoTrainer.java:164-190 does the closed-form per-coordinate
// update on the CPU. The torch device path queues ~8 tiny kernels per
// coordinate (dot, soft-threshold, axpy) — F=256 coordinates => ~2000
// launches per batch, pure launch-bound. This persistent kernel runs the
// entire cyclic sweep in ONE workgroup with the residual resident in LDS:
// per coordinate, a block-wide dot(x_f, r), the thread-0 soft-threshold,
// and the LDS axpy. CD is inherently sequential across coordinates, so one
// WG is the right shape — the op is latency-bound, not throughput-bound.
//
// X is passed transposed ([F, B] contiguous) so each coordinate's column
// is a coalesced stream. B is capped by LDS (<= 16367 samples); the binding
// hands larger batches, up to lasso_cd_max_rows(), to K11L (lasso_large.hip).

#include "hip_common.h"

namespace {

constexpr int CD_THREADS = 1024;

__global__ void lasso_cd_kernel(const float* __restrict__ Xt,
                                float* __restrict__ r_g,
                                float* __restrict__ w,
                                const float* __restrict__ col_sq,
                                float lam_n, int B, int F) {
  extern __shared__ float lds[];
  float* r = lds;                          // [B]
  float* partial = lds + B;                // [CD_THREADS / WAVE]
  float* bc = partial + CD_THREADS / WAVE; // broadcast slot
  const int wid = threadIdx.x / WAVE;
  const int lane = threadIdx.x % WAVE;

  for (int i = threadIdx.x; i < B; i += blockDim.x) r[i] = r_g[i];
  __syncthreads();

  for (int f = 0; f < F; ++f) {
    const float* x = Xt + (long)f * B;
    float acc = 0.f;
    for (int i = threadIdx.x; i < B; i += blockDim.x) acc += x[i] * r[i];
    acc = wave_reduce_sum(acc);
    if (lane == 0) partial[wid] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
      float c = 0.f;
      for (int k = 0; k < CD_THREADS / WAVE; ++k) c += partial[k];
      const float cs = col_sq[f];
      const float wi = w[f];
      c += wi * cs;
      const float sgn = (c > 0.f) ? 1.f : ((c < 0.f) ? -1.f : 0.f);
      const float wn = fmaxf(fabsf(c) - lam_n, 0.f) * sgn / cs;
      bc[0] = wi - wn;
      w[f] = wn;
    }
    __syncthreads();
    const float d = bc[0];
    if (d != 0.f) {
      for (int i = threadIdx.x; i < B; i += blockDim.x) r[i] += x[i] * d;
    }
    __syncthreads();
  }

  for (int i = threadIdx.x; i < B; i += blockDim.x) r_g[i] = r[i];
}

}  // namespace

int64_t lasso_cd_max_rows();
void lasso_cd_large_launch(const float* Xt, float* r, float* w,
                           const float* col_sq, float lam_n, int B, int F,
                           hipStream_t stream);

void lasso_cd(torch::Tensor Xt, torch::Tensor r, torch::Tensor w,
              torch::Tensor col_sq, double lam_n) {
  check_tensor(__func__, Xt, "Xt", torch::kFloat32, {-1, -1});
  const int F = Xt.size(0), B = Xt.size(1);
  check_tensor(__func__, r, "r", torch::kFloat32, {B});
  check_tensor(__func__, w, "w", torch::kFloat32, {F});
  check_tensor(__func__, col_sq, "col_sq", torch::kFloat32, {F});
  check_below_2_31(__func__, {{"F", Xt.size(0)}});
  const size_t lds = (Xt.size(1) + CD_THREADS / WAVE + 1) * sizeof(float);
  TORCH_CHECK(Xt.size(1) <= lasso_cd_max_rows(), __func__,
              ": batch too large for a residual kept on chip (max ",
              lasso_cd_max_rows(), " rows)");
  check_on_device(__func__, {Xt, r, w, col_sq});
  if (lds > 64 * 1024) {
    lasso_cd_large_launch(Xt.data_ptr<float>(), r.data_ptr<float>(),
                          w.data_ptr<float>(), col_sq.data_ptr<float>(),
                          (float)lam_n, B, F, current_stream());
    return;
  }
  hipLaunchKernelGGL(lasso_cd_kernel, dim3(1), dim3(CD_THREADS), lds,
                     current_stream(), Xt.data_ptr<float>(),
                     r.data_ptr<float>(), w.data_ptr<float>(),
                     col_sq.data_ptr<float>(), (float)lam_n, B, F);
}
