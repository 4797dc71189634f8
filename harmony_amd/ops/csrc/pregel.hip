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

template <int G>
void launch(bool is_min, bool addw, dim3 grid, hipStream_t st,
            const int64_t* in_ptr, const int* in_src, const float* in_w,
            float w_const, const float* vert_msg, const uint8_t* mask,
            float* out, uint8_t* flag, int64_t R, int64_t n_local,
            int64_t n_edges) {
#define PULL(MINV, ADDV)                                                     \
  hipLaunchKernelGGL((pregel_pull_kernel<G, MINV, ADDV>), grid, dim3(kBlock), \
                     0, st, in_ptr, in_src, in_w, w_const, vert_msg, mask,   \
                     out, flag, R, n_local, n_edges)
  if (is_min) {
    if (addw) PULL(true, true); else PULL(true, false);
  } else {
    if (addw) PULL(false, true); else PULL(false, false);
  }
#undef PULL
}

}  // namespace

// combiner: 0 = add, 1 = min. group: lanes per row, a power of two in 1..64.
std::vector<torch::Tensor> pregel_pull(
    torch::Tensor in_ptr, torch::Tensor in_src,
    c10::optional<torch::Tensor> in_w, double w_const, torch::Tensor vert_msg,
    c10::optional<torch::Tensor> send_mask, int64_t combiner, bool add_weight,
    int64_t group) {
  CHECK_IN(in_ptr); CHECK_IN(in_src); CHECK_IN(vert_msg);
  TORCH_CHECK(in_ptr.dtype() == torch::kInt64 && in_ptr.dim() == 1 &&
              in_ptr.numel() >= 1, "in_ptr must be int64 [R+1]");
  TORCH_CHECK(in_src.dtype() == torch::kInt32 && in_src.dim() == 1,
              "in_src must be int32 [Ein]");
  TORCH_CHECK(vert_msg.dtype() == torch::kFloat32 && vert_msg.dim() == 1,
              "vert_msg must be float32 [n_local] (msg_dim == 1 only)");
  TORCH_CHECK(combiner == 0 || combiner == 1, "combiner: 0 add, 1 min");
  TORCH_CHECK(group >= 1 && group <= 64 && (group & (group - 1)) == 0,
              "group must be a power of two in 1..64");
  const int64_t R = in_ptr.numel() - 1;
  const int64_t n_edges = in_src.numel();
  const int64_t n_local = vert_msg.numel();
  TORCH_CHECK(n_local < (int64_t)1 << 31 && n_edges < (int64_t)1 << 31,
              "pregel_pull: n_local and Ein must be below 2^31");
  const float* wp = nullptr;
  if (in_w.has_value()) {
    CHECK_IN(*in_w);
    TORCH_CHECK(in_w->dtype() == torch::kFloat32 &&
                in_w->numel() == n_edges, "in_w must be float32 [Ein]");
    wp = in_w->data_ptr<float>();
  }
  const uint8_t* mp = nullptr;
  if (send_mask.has_value()) {
    CHECK_IN(*send_mask);
    TORCH_CHECK(send_mask->dtype() == torch::kUInt8 &&
                send_mask->numel() == n_local,
                "send_mask must be uint8 [n_local]");
    mp = send_mask->data_ptr<uint8_t>();
  }
  auto out = torch::empty({R}, vert_msg.options());
  auto flag = torch::empty({R}, vert_msg.options().dtype(torch::kUInt8));
  if (R == 0) return {out, flag};
  const int64_t rows_per_block = kBlock / group;
  const int64_t want = (R + rows_per_block - 1) / rows_per_block;
  // memory-bound: cap the grid and let the groups stride over the rest
  dim3 grid((unsigned)std::min<int64_t>(want, 256 * 8 * 4));
  hipStream_t st = current_stream();
#define GO(GV)                                                               \
  case GV:                                                                   \
    launch<GV>(combiner == 1, add_weight, grid, st,                          \
               in_ptr.data_ptr<int64_t>(), in_src.data_ptr<int>(), wp,       \
               (float)w_const, vert_msg.data_ptr<float>(), mp,               \
               out.data_ptr<float>(), flag.data_ptr<uint8_t>(), R, n_local,  \
               n_edges);                                                     \
    break
  switch (group) {
    GO(1); GO(2); GO(4); GO(8); GO(16); GO(32); GO(64);
  }
#undef GO
  return {out, flag};
}
