// K13p: Pregel push — "send + combine" of one superstep along the OUT-edges
// of the few vertices that send (the frontier), for the min combiner.
//
// K13 (pregel.hip) walks every in-edge of every row each superstep and skips
// the sources that do not send one edge at a time; its cost is the whole
// graph however small the frontier. The reference's per-vertex compute()
// touches only the vertices that received a message ("vertices vote to
// halt"). K13p is that direction: it reads only the out-lists of the
// frontier and combines into the destination rows with atomics.
//
// Work is assigned per frontier EDGE, not per frontier vertex. A pre-pass
// (push_degrees) writes the clamped out-degree of every frontier entry, the
// host op turns them into the exclusive prefix sum fptr[nf+1], and lane p of
// a grid-strided launch handles frontier-edge position p: it finds its
// vertex by binary search in fptr (largest i with fptr[i] <= p), so
// consecutive lanes inside one vertex read consecutive out_row / out_w
// entries, and one hub with 10^6 out-edges spreads over the whole chip.
//
// Combine: min over float32 values through integer atomics on the float's
// bits. out is pre-filled with +inf. A value with the sign bit clear does a
// signed atomicMin on the int32 view (non-negative floats order like their
// bits; a negative float already stored is a negative int and stays). A
// value with the sign bit set does an unsigned atomicMax on the uint32 view
// (any negative float's bits exceed every non-negative one's, and among
// negatives the larger bits are the smaller float). Both are no-return,
// device-scope integer atomics: the result does not depend on arrival order,
// so two runs agree bit for bit. No float atomics. NaN messages are
// unspecified (K13's fminf drops them; here their bits take part in the
// integer order).
//
// flag[row] = 1 is a plain byte store by every lane that delivers; all
// writers store the same value. Nothing malformed is dereferenced: a frontier
// id outside [0, n_local) has degree 0, edge ranges are clamped to [0, E], a
// row outside [0, R) is skipped. msg_dim == 1 only.

#include "hip_common.h"

#include <limits>

namespace {

constexpr int kBlock = 256;
constexpr int64_t kMaxGrid = 2048;

// The pre-pass, one launch over max(nf, R) positions: fills out with +inf
// and flag with 0 (the push kernel runs after it on the same stream), and
// writes deg[0] = 0, deg[i + 1] = clamped out-degree of frontier[i], or 0
// when send_mask says that the vertex does not send; the inclusive cumsum of
// deg is the exclusive prefix sum fptr[nf + 1].
__global__ __launch_bounds__(kBlock) void push_degrees_kernel(
    const int64_t* __restrict__ out_ptr, const int* __restrict__ frontier,
    const uint8_t* __restrict__ send_mask,   // nullable: every entry sends
    int64_t* __restrict__ deg, float* __restrict__ out,
    uint8_t* __restrict__ flag, int64_t nf, int64_t R, int64_t n_local,
    int64_t n_edges) {
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  const int64_t span = nf > R ? nf : R;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < span;
       i += stride) {
    if (i < R) {
      out[i] = std::numeric_limits<float>::infinity();
      flag[i] = 0;
    }
    if (i >= nf) continue;
    if (i == 0) deg[0] = 0;
    const int v = frontier[i];
    int64_t d = 0;
    if ((unsigned)v < (unsigned)n_local &&
        (send_mask == nullptr || send_mask[v] != 0)) {
      int64_t beg = out_ptr[v], end = out_ptr[v + 1];
      beg = beg < 0 ? 0 : beg;
      end = end > n_edges ? n_edges : end;
      d = end > beg ? end - beg : 0;
    }
    deg[i + 1] = d;
  }
}

template <bool ADDW>
__global__ __launch_bounds__(kBlock) void pregel_push_kernel(
    const int64_t* __restrict__ out_ptr, const int* __restrict__ out_row,
    const float* __restrict__ out_w,         // nullable: use w_const
    float w_const, const float* __restrict__ vert_msg,
    const int* __restrict__ frontier, const int64_t* __restrict__ fptr,
    int* __restrict__ out_bits, uint8_t* __restrict__ flag, int64_t nf,
    int64_t R, int64_t n_local, int64_t n_edges) {
  const int64_t total = fptr[nf];
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x; p < total;
       p += stride) {
    // largest i in [0, nf) with fptr[i] <= p; fptr[0] = 0 <= p < fptr[nf],
    // and entries of degree 0 (fptr[i] == fptr[i+1]) are stepped over
    int64_t lo = 0, hi = nf;
    while (hi - lo > 1) {
      const int64_t mid = (lo + hi) >> 1;
      if (fptr[mid] <= p) lo = mid; else hi = mid;
    }
    const int v = frontier[lo];
    // fptr gave this entry a non-zero degree, so v passed the range check of
    // the pre-pass; checked again so that no caller-built fptr can matter
    if ((unsigned)v >= (unsigned)n_local) continue;
    int64_t beg = out_ptr[v];
    beg = beg < 0 ? 0 : beg;
    const int64_t e = beg + (p - fptr[lo]);
    if (e < 0 || e >= n_edges) continue;
    const int row = out_row[e];
    if ((unsigned)row >= (unsigned)R) continue;
    float val = vert_msg[v];
    if (ADDW) val += (out_w != nullptr) ? out_w[e] : w_const;
    const int bits = __float_as_int(val);
    if (bits >= 0) {
      atomicMin(out_bits + row, bits);
    } else {
      atomicMax(reinterpret_cast<unsigned int*>(out_bits) + row,
                (unsigned int)bits);
    }
    flag[row] = 1;
  }
}

}  // namespace

// The min combiner only. send_mask (uint8 [n_local], optional) narrows the
// frontier to the entries whose vertex it marks, so that a caller with a mask
// on the device passes frontier = all vertices and needs no compaction (and
// no host read of its size). edges_hint >= 0 is the caller's count of
// frontier edges and only sizes the grid; the kernel's loop bound is
// fptr[nf].
std::vector<torch::Tensor> pregel_push(
    torch::Tensor out_ptr, torch::Tensor out_row,
    c10::optional<torch::Tensor> out_w, double w_const,
    torch::Tensor vert_msg, torch::Tensor frontier,
    c10::optional<torch::Tensor> send_mask, int64_t num_rows,
    bool add_weight, int64_t edges_hint) {
  CHECK_IN(out_ptr); CHECK_IN(out_row); CHECK_IN(vert_msg);
  CHECK_IN(frontier);
  TORCH_CHECK(out_ptr.dtype() == torch::kInt64 && out_ptr.dim() == 1 &&
              out_ptr.numel() >= 1, "out_ptr must be int64 [n_local+1]");
  TORCH_CHECK(out_row.dtype() == torch::kInt32 && out_row.dim() == 1,
              "out_row must be int32 [E]");
  TORCH_CHECK(vert_msg.dtype() == torch::kFloat32 && vert_msg.dim() == 1,
              "vert_msg must be float32 [n_local] (msg_dim == 1 only)");
  TORCH_CHECK(frontier.dtype() == torch::kInt32 && frontier.dim() == 1,
              "frontier must be int32 [nf]");
  const int64_t n_local = out_ptr.numel() - 1;
  const int64_t n_edges = out_row.numel();
  const int64_t nf = frontier.numel();
  const int64_t R = num_rows;
  TORCH_CHECK(vert_msg.numel() == n_local,
              "vert_msg must have one entry per local vertex");
  TORCH_CHECK(R >= 0 && R < (int64_t)1 << 31 &&
              n_local < (int64_t)1 << 31 && n_edges < (int64_t)1 << 31,
              "pregel_push: num_rows, n_local and E must be below 2^31");
  const float* wp = nullptr;
  if (out_w.has_value()) {
    CHECK_IN(*out_w);
    TORCH_CHECK(out_w->dtype() == torch::kFloat32 &&
                out_w->numel() == n_edges, "out_w must be float32 [E]");
    wp = out_w->data_ptr<float>();
  }
  const uint8_t* mp = nullptr;
  if (send_mask.has_value()) {
    CHECK_IN(*send_mask);
    TORCH_CHECK(send_mask->dtype() == torch::kUInt8 &&
                send_mask->numel() == n_local,
                "send_mask must be uint8 [n_local]");
    mp = send_mask->data_ptr<uint8_t>();
  }
  if (nf == 0 || R == 0 || n_edges == 0) {
    return {torch::full({R}, std::numeric_limits<float>::infinity(),
                        vert_msg.options()),
            torch::zeros({R}, vert_msg.options().dtype(torch::kUInt8))};
  }
  auto out = torch::empty({R}, vert_msg.options());
  auto flag = torch::empty({R}, vert_msg.options().dtype(torch::kUInt8));
  hipStream_t st = current_stream();
  auto deg = torch::empty({nf + 1}, out_ptr.options());
  const int64_t dgrid = std::min<int64_t>(
      (std::max(nf, R) + kBlock - 1) / kBlock, kMaxGrid);
  hipLaunchKernelGGL(push_degrees_kernel, dim3((unsigned)dgrid), dim3(kBlock),
                     0, st, out_ptr.data_ptr<int64_t>(),
                     frontier.data_ptr<int>(), mp, deg.data_ptr<int64_t>(),
                     out.data_ptr<float>(), flag.data_ptr<uint8_t>(), nf, R,
                     n_local, n_edges);
  auto fptr = at::cumsum(deg, 0);
  // without a hint the frontier's edge count is only known on the device:
  // size the grid for a full chip and let idle workgroups leave at once
  int64_t want = kMaxGrid;
  if (edges_hint >= 0) want = (edges_hint + kBlock - 1) / kBlock;
  const int64_t grid =
      std::max<int64_t>(1, std::min<int64_t>(want, kMaxGrid));
#define PUSH(ADDV)                                                           \
  hipLaunchKernelGGL((pregel_push_kernel<ADDV>), dim3((unsigned)grid),       \
                     dim3(kBlock), 0, st, out_ptr.data_ptr<int64_t>(),       \
                     out_row.data_ptr<int>(), wp, (float)w_const,            \
                     vert_msg.data_ptr<float>(), frontier.data_ptr<int>(),   \
                     fptr.data_ptr<int64_t>(),                               \
                     reinterpret_cast<int*>(out.data_ptr<float>()),          \
                     flag.data_ptr<uint8_t>(), nf, R, n_local, n_edges)
  if (add_weight) PUSH(true); else PUSH(false);
#undef PUSH
  return {out, flag};
}
