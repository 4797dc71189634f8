// Shared CDNA4 device helpers (gfx950: wave64, 4x SIMD-32 per CU).
#pragma once

#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>

#include "binding.h"

#define WAVE 64

// The HIP stream torch has current for this thread (per-job streams are set
// from python with torch.cuda.stream(...)).
inline hipStream_t current_stream() {
  return c10::hip::getCurrentHIPStream().stream();
}

// A runtime call or a launch (hipGetLastError()) that must have succeeded.
inline void check_hip(const char* op, hipError_t status, const char* what) {
  TORCH_CHECK(status == hipSuccess, op, ": ", what, " failed: ",
              hipGetErrorString(status));
}

// The server's nmf_sgd on one element: clamp(v - step * d, 0, maxval), the
// product and the difference rounded once, together (what the compiler has
// always made of that expression in scatter_apply; spelled out so that
// every kernel that applies the update gets the same bits). Compares, not
// fminf/fmaxf: those return the other operand for a NaN, and a NaN must stay
// one as under torch's clamp_.
__device__ __forceinline__ float nmf_sgd_one(float v, float d, float step,
                                             float maxval) {
  float x = __fmaf_rn(-step, d, v);
  x = x < 0.f ? 0.f : x;
  x = x > maxval ? maxval : x;
  return x;
}

// Full-wave sum: butterfly over 64 lanes; every lane ends with the total.
__device__ __forceinline__ float wave_reduce_sum(float v) {
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m, WAVE);
  return v;
}

__device__ __forceinline__ int lane_i(int v, int l) {
  return __builtin_amdgcn_readlane(v, l);
}
__device__ __forceinline__ float lane_f(float v, int l) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}

// Wave sum that leaves the same bits in every lane, without the LDS crossbar
// a __shfl_xor butterfly goes through (six dependent ds_bpermute round trips
// were most of a short Lasso column's time): four DPP steps inside each
// 16-lane row (xor 1, xor 2, half mirror, mirror; each pair of lanes adds the
// same two values, so a row's lanes agree), then the four row sums by
// v_readlane. Needs all 64 lanes active.
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

// Inclusive prefix sum across 64 lanes (Hillis-Steele via shfl_up).
__device__ __forceinline__ float wave_inclusive_scan(float v) {
#pragma unroll
  for (int d = 1; d < WAVE; d <<= 1) {
    float o = __shfl_up(v, d, WAVE);
    if ((threadIdx.x & (WAVE - 1)) >= d) v += o;
  }
  return v;
}

// Counter-based RNG: two murmur3 finalizer rounds over (seed, ctr).
// Deterministic and reproduced bit-exactly by the torch reference
// (harmony_amd/ops/rng.py) so CPU<->GPU numerics tests can compare samples.
__device__ __forceinline__ unsigned int rng_u32(unsigned int seed,
                                                unsigned int ctr) {
  unsigned int h = seed ^ (ctr * 2654435761u);
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    h ^= h >> 16; h *= 0x85ebca6bu;
    h ^= h >> 13; h *= 0xc2b2ae35u;
    h ^= h >> 16;
  }
  return h;
}

__device__ __forceinline__ float rng_uniform(unsigned int seed,
                                             unsigned int ctr) {
  return (rng_u32(seed, ctr) + 0.5f) * 2.3283064365386963e-10f;  // 2^-32
}
