// K10b — GBT split search over one level's K10 histograms.
//
// Reference: GBTTrainer.java picks, per tree node, the best split over all
// features: a threshold for a continuous feature (bestSplitRealFeature) and a
// SUBSET of the categories for a categorical one (bestSplitLabelFeature,
// exhaustive by Gray code up to 10 labels). Here the histograms of a level
// are already on the device ([n_nodes, F, nb] counts and residual sums, K10),
// and with nb <= 64 one (node, feature) histogram is one wavefront, one lane
// per bin or category. Replaces the torch chain of build_tree (two cumsums,
// about ten elementwise ops over [n_nodes, F, nb], an argmax, three host
// syncs), which cannot express a subset search.
//
// Pass 1, one wave per (node, feature), four features of a node per
// 256-thread workgroup:
//   continuous   inclusive scan of (cnt, s) over the bins; lane b holds the
//                candidate "left = bins <= b".
//   categorical  the live categories (cnt > 0) are put in (mean, id) order,
//                mean = s / cnt by IEEE division: each lane counts the live
//                lanes that sort before it (one uniform broadcast per live
//                lane), dead lanes go behind the live ones in id order, so
//                the ranks are a permutation of 0..63; (cnt, s) move to rank
//                order with one ds_permute, and the same scan follows. Lane
//                p holds the candidate "left = the first p + 1 categories of
//                the order". For lam = 0 the optimum over all subsets is one
//                of these (Fisher 1958); for lam > 0 none better was found
//                by exhaustive search (docs/ROADMAP.md).
//   both         gain = sl^2/(cl+lam) + sr^2/(cr+lam) - stot^2/(ctot+lam),
//                valid iff cl > 0 and cr > 0 (lanes >= nb - 1 never are: the
//                lanes >= nb hold empty bins), wave arg-max that keeps the
//                lower lane on equal gain. A categorical winner's mask is one
//                ballot over the original lanes: live and rank > p.
//   Lane 0 writes (gain, candidate, mask) to a [n_nodes, F] scratch.
// Pass 2, one wave per node: arg-max over the F scratch entries, the lower
// feature on equal gain, and the four outputs.
//
// No LDS, no atomics, no cross-workgroup protocol: two plain launches on the
// current stream, so the result is bitwise reproducible.

#include "hip_common.h"

namespace {

constexpr int SPLIT_THREADS = 256;
constexpr int WAVES = SPLIT_THREADS / WAVE;
constexpr float kNoCandidate = -1e30f;   // build_tree's invalid-gain value
constexpr float kMinGain = 1e-12f;       // build_tree's has_split constant

// The gain is written as torch evaluates it: every product, quotient and sum
// rounded on its own.
__device__ __forceinline__ float split_gain(float sl, float cl, float sr,
                                            float cr, float stot, float ctot,
                                            float lam) {
#pragma clang fp contract(off)
  const float a = sl * sl / (cl + lam);
  const float b = sr * sr / (cr + lam);
  const float c = stot * stot / (ctot + lam);
  return a + b - c;
}

// Wave arg-max of (g, i): the largest g, the smallest i among equal g. Every
// lane ends with the winner.
__device__ __forceinline__ void wave_argmax(float& g, int& i) {
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) {
    const float og = __shfl_xor(g, m, WAVE);
    const int oi = __shfl_xor(i, m, WAVE);
    if (og > g || (og == g && oi < i)) {
      g = og;
      i = oi;
    }
  }
}

__global__ __launch_bounds__(SPLIT_THREADS) void gbt_split_feature_kernel(
    const float* __restrict__ cnt,    // [n_nodes, F, nb]
    const float* __restrict__ sum,    // [n_nodes, F, nb]
    const int* __restrict__ ftype,    // [F] 0 = continuous
    float* __restrict__ sgain,        // [n_nodes, F]
    int* __restrict__ scand,          // [n_nodes, F]
    long long* __restrict__ smask,    // [n_nodes, F]
    int n_nodes, int F, int nb, int fblocks, float lam) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x / WAVE;
  const int nd = blockIdx.x / fblocks;
  const int f = (blockIdx.x - nd * fblocks) * WAVES + wid;
  if (nd >= n_nodes || f >= F) return;          // wave-uniform
  const long nf = (long)nd * F + f;

  float c = 0.f, s = 0.f;
  if (lane < nb) {
    c = cnt[nf * nb + lane];
    s = sum[nf * nb + lane];
  }
  const bool categorical = ftype[f] != 0;       // wave-uniform
  const bool live = c > 0.f;
  int rank = lane;
  if (categorical) {
    const unsigned long long lm = __ballot(live);
    const float mean = live ? s / c : 0.f;
    if (live) {
      rank = 0;
      unsigned long long m = lm;
      while (m) {                               // uniform: lm is a scalar
        const int j = __builtin_amdgcn_readfirstlane(__ffsll((long long)m) - 1);
        m &= m - 1;
        const float mj = __int_as_float(
            __builtin_amdgcn_readlane(__float_as_int(mean), j));
        rank += (mj < mean || (mj == mean && j < lane)) ? 1 : 0;
      }
    } else {
      // dead lanes follow the live ones, in id order
      const unsigned long long below = (1ull << lane) - 1ull;
      rank = __popcll(lm) + __popcll(~lm & below);
    }
    // push (cnt, s) to rank order; the ranks are a permutation of 0..63
    c = __int_as_float(
        __builtin_amdgcn_ds_permute(rank * 4, __float_as_int(c)));
    s = __int_as_float(
        __builtin_amdgcn_ds_permute(rank * 4, __float_as_int(s)));
  }
  const float cl = wave_inclusive_scan(c);
  const float sl = wave_inclusive_scan(s);
  const float ctot = __shfl(cl, WAVE - 1, WAVE);
  const float stot = __shfl(sl, WAVE - 1, WAVE);
  const float cr = ctot - cl, sr = stot - sl;
  float g = (cl > 0.f && cr > 0.f)
                ? split_gain(sl, cl, sr, cr, stot, ctot, lam)
                : kNoCandidate;
  int p = lane;
  wave_argmax(g, p);
  const unsigned long long right =
      __ballot(categorical && live && rank > p);
  if (lane == 0) {
    sgain[nf] = g;
    scand[nf] = p;
    smask[nf] = (long long)right;
  }
}

__global__ __launch_bounds__(WAVE) void gbt_split_node_kernel(
    const float* __restrict__ sgain, const int* __restrict__ scand,
    const long long* __restrict__ smask, const int* __restrict__ ftype,
    int* __restrict__ feature, int* __restrict__ threshold,
    long long* __restrict__ mask, float* __restrict__ gain, int n_nodes,
    int F) {
  const int nd = blockIdx.x;
  const int lane = threadIdx.x;
  if (nd >= n_nodes) return;
  float g = kNoCandidate;
  int f = 0x7fffffff;
  for (int i = lane; i < F; i += WAVE) {        // ascending: first max stays
    const float gi = sgain[(long)nd * F + i];
    if (gi > g) {
      g = gi;
      f = i;
    }
  }
  wave_argmax(g, f);
  if (lane == 0) {
    const bool split = f < F && g > kMinGain;
    const bool cat = split && ftype[f] != 0;
    feature[nd] = split ? f : 0;
    threshold[nd] = split ? (cat ? -2 : scand[(long)nd * F + f]) : -1;
    mask[nd] = cat ? smask[(long)nd * F + f] : 0ll;
    gain[nd] = split ? g : 0.f;
  }
}

}  // namespace

// Best split per node of one level. cnt, s: float32 [n_nodes, F, nb] with
// nb <= 64; ftype: int32 [F]. Returns (feature int32, threshold int32,
// mask int64, gain float32), each [n_nodes].
std::vector<torch::Tensor> gbt_best_split(torch::Tensor cnt, torch::Tensor s,
                                          torch::Tensor ftype, double lam) {
  CHECK_IN(cnt); CHECK_IN(s); CHECK_IN(ftype);
  TORCH_CHECK(cnt.dtype() == torch::kFloat32 && cnt.dim() == 3 &&
              s.dtype() == torch::kFloat32 && s.sizes() == cnt.sizes(),
              "cnt and s must be float32 [n_nodes, F, nb]");
  const int64_t n_nodes = cnt.size(0), F = cnt.size(1), nb = cnt.size(2);
  TORCH_CHECK(ftype.dtype() == torch::kInt32 && ftype.dim() == 1 &&
              ftype.numel() == F, "ftype must be int32 [F]");
  TORCH_CHECK(nb >= 1 && nb <= WAVE, "gbt_best_split: nb must be in 1..64");
  TORCH_CHECK(n_nodes >= 1 && F >= 1, "gbt_best_split: empty level");
  const int64_t fblocks = (F + WAVES - 1) / WAVES;
  TORCH_CHECK(n_nodes * fblocks < ((int64_t)1 << 31) &&
              n_nodes * F * nb < ((int64_t)1 << 40),
              "gbt_best_split: level too large");
  auto dev = cnt.device();
  auto i32 = torch::TensorOptions().dtype(torch::kInt32).device(dev);
  auto i64 = torch::TensorOptions().dtype(torch::kInt64).device(dev);
  auto f32 = torch::TensorOptions().dtype(torch::kFloat32).device(dev);
  auto sgain = torch::empty({n_nodes, F}, f32);
  auto scand = torch::empty({n_nodes, F}, i32);
  auto smask = torch::empty({n_nodes, F}, i64);
  auto feature = torch::empty({n_nodes}, i32);
  auto threshold = torch::empty({n_nodes}, i32);
  auto mask = torch::empty({n_nodes}, i64);
  auto gain = torch::empty({n_nodes}, f32);
  hipStream_t st = current_stream();
  hipLaunchKernelGGL(gbt_split_feature_kernel,
                     dim3((unsigned)(n_nodes * fblocks)), dim3(SPLIT_THREADS),
                     0, st, cnt.data_ptr<float>(), s.data_ptr<float>(),
                     ftype.data_ptr<int>(), sgain.data_ptr<float>(),
                     scand.data_ptr<int>(),
                     reinterpret_cast<long long*>(smask.data_ptr<int64_t>()),
                     (int)n_nodes, (int)F, (int)nb, (int)fblocks, (float)lam);
  hipLaunchKernelGGL(gbt_split_node_kernel, dim3((unsigned)n_nodes),
                     dim3(WAVE), 0, st, sgain.data_ptr<float>(),
                     scand.data_ptr<int>(),
                     reinterpret_cast<const long long*>(
                         smask.data_ptr<int64_t>()),
                     ftype.data_ptr<int>(), feature.data_ptr<int>(),
                     threshold.data_ptr<int>(),
                     reinterpret_cast<long long*>(mask.data_ptr<int64_t>()),
                     gain.data_ptr<float>(), (int)n_nodes, (int)F);
  return {feature, threshold, mask, gain};
}
