// K13: Pregel pull — "send + combine" of one superstep as a CSR
// gather-reduce over a static inverted edge index (for each destination row,
// the list of its local source vertices).
//
// Reference semantics: ComputationCallable.java:36 calls compute() per
// vertex, each sendMessage goes through MessageManager.addMessage with the
// app's MessageCombiner (sum for pagerank, min for shortestpath). The graph
// is static for the life of a job, so the combine needs neither atomics nor
// a per-superstep sort: the edge list is inverted once at load time
// (pregel/engine.py build_pull_index) and every superstep is one pass that
// reads the per-vertex message through the index, SpMV-style.
//
// Layout: CSR-vector. G = 2^k lanes (1..64, chosen on the host from the
// graph's mean in-degree) cooperate on one row; the lanes of a group read
// consecutive in_src entries (coalesced), stride by G over longer rows and
// reduce with a width-G xor butterfly. One lane writes out[row]/flag[row].
// No atomics: for a fixed G the summation order is fixed, so the result for
// a given graph and input is bitwise identical from run to run.
//
// Accepted for this version: a skewed row (one very long in-list) is walked
// by its one group alone and holds up that group's workgroup; splitting long
// rows over several groups is left to a later change. msg_dim == 1 only.

#include "hip_common.h"

#include <limits>

namespace {

constexpr int kBlock = 256;

template <int G, bool MIN, bool ADDW>
__global__ __launch_bounds__(kBlock) void pregel_pull_kernel(
    const int64_t* __restrict__ in_ptr, const int* __restrict__ in_src,
    const float* __restrict__ in_w,          // nullable: use w_const
    float w_const, const float* __restrict__ vert_msg,
    const uint8_t* __restrict__ send_mask,   // nullable: every source sends
    float* __restrict__ out, uint8_t* __restrict__ flag, int64_t R,
    int64_t n_local, int64_t n_edges) {
  constexpr int kRows = kBlock / G;          // rows per workgroup per sweep
  const int lane = threadIdx.x & (G - 1);
  const int64_t stride = (int64_t)gridDim.x * kRows;
  // all G lanes of a group share `row`, so the group leaves the loop
  // together and the width-G shuffles below only ever read live lanes
  for (int64_t row = (int64_t)blockIdx.x * kRows + threadIdx.x / G; row < R;
       row += stride) {
    int64_t beg = in_ptr[row], end = in_ptr[row + 1];
    // a malformed index must not read out of bounds
    beg = beg < 0 ? 0 : beg;
    end = end > n_edges ? n_edges : end;
    float acc = MIN ? std::numeric_limits<float>::infinity() : 0.f;
    int any = 0;
    for (int64_t e = beg + lane; e < end; e += G) {
      const int s = in_src[e];
      if ((unsigned)s >= (unsigned)n_local) continue;
      if (send_mask != nullptr && send_mask[s] == 0) continue;
      float v = vert_msg[s];
      if (ADDW) v += (in_w != nullptr) ? in_w[e] : w_const;
      acc = MIN ? fminf(acc, v) : acc + v;
      any = 1;
    }
#pragma unroll
    for (int m = G >> 1; m > 0; m >>= 1) {
      const float o = __shfl_xor(acc, m, G);
      acc = MIN ? fminf(acc, o) : acc + o;
      any |= __shfl_xor(any, m, G);
    }
    if (lane == 0) {
      out[row] = acc;
      flag[row] = (uint8_t)any;
    }
  }
}

}  // namespace

// combiner: 0 = add, 1 = min. group: lanes per row, a power of two in 1..64.
std::vector<torch::Tensor> pregel_pull(
    torch::Tensor in_ptr, torch::Tensor in_src,
    c10::optional<torch::Tensor> in_w, double w_const, torch::Tensor vert_msg,
    c10::optional<torch::Tensor> send_mask, int64_t combiner, bool add_weight,
    int64_t group) {
  check_tensor(__func__, in_ptr, "in_ptr", torch::kInt64, {-1});
  check_tensor(__func__, in_src, "in_src", torch::kInt32, {-1});
  check_tensor(__func__, vert_msg, "vert_msg", torch::kFloat32, {-1});  // 1-D
  const int64_t R = in_ptr.numel() - 1;
  const int64_t n_edges = in_src.numel();
  const int64_t n_local = vert_msg.numel();
  const float* wp = check_tensor<float>(__func__, in_w, "in_w", {n_edges});
  const uint8_t* mp =
      check_tensor<uint8_t>(__func__, send_mask, "send_mask", {n_local});
  TORCH_CHECK(combiner == 0 || combiner == 1, __func__,
              ": combiner: 0 add, 1 min");
  check_pow2<1, 64>(__func__, "group", group);
  check_below_2_31(__func__,
                   {{"R", R}, {"n_local", n_local}, {"Ein", n_edges}});
  check_on_device(__func__, {in_ptr, in_src, vert_msg, in_w, send_mask});
  auto out = torch::empty({R}, vert_msg.options());
  auto flag = torch::empty({R}, vert_msg.options().dtype(torch::kUInt8));
  if (R == 0) return {out, flag};
  const int64_t rows_per_block = kBlock / group;
  const dim3 grid = strided_grid((R + rows_per_block - 1) / rows_per_block);
  hipStream_t st = current_stream();
  dispatch_pow2<1, 64>(__func__, "group", group, [&](auto g) {
    constexpr int G = decltype(g)::value;
    dispatch_bool(combiner == 1, [&](auto is_min) {
      dispatch_bool(add_weight, [&](auto addw) {
        hipLaunchKernelGGL(
            (pregel_pull_kernel<G, decltype(is_min)::value,
                                decltype(addw)::value>),
            grid, dim3(kBlock), 0, st, in_ptr.data_ptr<int64_t>(),
            in_src.data_ptr<int>(), wp, (float)w_const,
            vert_msg.data_ptr<float>(), mp, out.data_ptr<float>(),
            flag.data_ptr<uint8_t>(), R, n_local, n_edges);
      });
    });
  });
  return {out, flag};
}
