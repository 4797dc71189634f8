// K7e: LDA held-out fold-in (document completion) — one lane group per
// document, shaped like K7 (lda.hip).
//
// Each held-out document comes as two lists of (word, count) pairs sorted by
// word id: the observed half and the scored half. Against the FROZEN model
//   phi[w,k] = (n_wk + beta) / (n_k + V beta)
// the group runs `iters` EM steps on the document's topic mixture,
//   theta_k <- (alpha + sum_pairs c theta_k phi[w,k] / sum_j theta_j phi[w,j])
//              / (N_obs + K alpha),        theta^0 = 1/K,
// and then scores  ll = sum_scored c log sum_k theta_k phi[w,k].
//
// Per lane, K/G chunks of ti = theta * invden and of the step's accumulator m
// live in registers; invden[k] = 1/(n_k + V beta) is built once per
// workgroup in LDS and folded into theta once per step. A pair costs one
// coalesced int32 row read, a few flops per topic and one group butterfly.
// The (word, count) pairs are fetched G at a time, one per lane, and handed
// round by shuffles, so that no row address waits for an index load of its
// own. Nothing is written but theta[doc] and ll[doc], with plain stores: no
// atomics and no coupling between documents, so a document's result does not
// depend on its place in the batch.
//
// Arithmetic: float32, pairs in their stored order, IEEE division and libm
// logf (no fast-math), and no contraction into fma, so that a pair's terms
// are the same bits in whichever of the loops below it is processed.
//
// Pairs in flight: PF = 2 issues the row loads of two pairs before the
// arithmetic of the first (the same operations in the same order: the
// results are bit-identical to PF = 1). profiles/lda_foldin_ab.md has the
// timings behind the default.

#include "hip_common.h"
#include <cstdlib>

#pragma clang fp contract(off)

namespace {

constexpr int MAXC = 16;           // K <= 64 * MAXC
constexpr int BLOCK_THREADS = 256;

template <int G>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
  for (int m = G / 2; m > 0; m >>= 1) v += __shfl_xor(v, m, G);
  return v;
}

// One row of the frozen table for this lane: chunk c is topic c*G + lane.
// FULL: K == NC * G, every chunk is whole. Otherwise a lane past K re-reads
// topic K - 1, whose term ti = 0 then drops: a load under `idx < K` becomes
// a branch with a wait of its own per chunk, which serialises the row's
// loads (measured, profiles/lda_foldin_ab.md).
template <int G, int NC, bool FULL>
__device__ __forceinline__ void load_row(const int* __restrict__ word_topic,
                                         int w, int K, int lane,
                                         int (&n)[NC]) {
  const int* row = word_topic + (int64_t)w * K;      // 64-bit row offset
#pragma unroll
  for (int c = 0; c < NC; ++c)
    n[c] = row[FULL ? c * G + lane : min(c * G + lane, K - 1)];
}

// sum_k theta_k phi[w,k] for one pair; val[c] keeps this lane's terms.
// ti = theta * invden is 0 past K, so a padded chunk adds exactly 0.
template <int G, int NC>
__device__ __forceinline__ float pair_total(const int (&n)[NC],
                                            const float (&ti)[NC], float beta,
                                            float (&val)[NC]) {
  float part = 0.f;
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    val[c] = ti[c] * ((float)n[c] + beta);
    part += val[c];
  }
  return group_sum<G>(part);
}

// m_k += c theta_k phi[w,k] / total for one observed pair
template <int G, int NC>
__device__ __forceinline__ void fold_pair(const int (&n)[NC],
                                          const float (&ti)[NC], float beta,
                                          float cnt, float (&m)[NC]) {
  float val[NC];
  const float scale = cnt / pair_total<G, NC>(n, ti, beta, val);
#pragma unroll
  for (int c = 0; c < NC; ++c) m[c] += val[c] * scale;
}

template <int G, int NC, int PF, bool FULL>
__global__ void __launch_bounds__(BLOCK_THREADS)
lda_foldin_kernel(const int* __restrict__ word_topic,
                  const int* __restrict__ topic_sum,
                  const int64_t* __restrict__ obs_ptr,
                  const int64_t* __restrict__ obs_word,
                  const int* __restrict__ obs_cnt,
                  const int64_t* __restrict__ sc_ptr,
                  const int64_t* __restrict__ sc_word,
                  const int* __restrict__ sc_cnt,
                  float* __restrict__ theta_out, float* __restrict__ ll_out,
                  float alpha, float beta, float vbeta, int n_docs, int K,
                  int iters) {
  constexpr int GROUPS = BLOCK_THREADS / G;
  extern __shared__ float invden[];                       // [K]
  const int group = threadIdx.x / G;
  const int lane = threadIdx.x % G;

  for (int idx = threadIdx.x; idx < K; idx += blockDim.x)
    invden[idx] = 1.0f / ((float)topic_sum[idx] + vbeta);
  __syncthreads();

  const int doc = blockIdx.x * GROUPS + group;
  if (doc >= n_docs) return;                              // whole group

  const int64_t o0 = obs_ptr[doc], o1 = obs_ptr[doc + 1];
  const int64_t s0 = sc_ptr[doc], s1 = sc_ptr[doc + 1];
  float* theta_row = theta_out + (int64_t)doc * K;

  int n_obs = 0;
  for (int64_t p = o0 + lane; p < o1; p += G) n_obs += obs_cnt[p];
#pragma unroll
  for (int m = G / 2; m > 0; m >>= 1) n_obs += __shfl_xor(n_obs, m, G);
  const float den = (float)n_obs + (float)K * alpha;

  float ti[NC], m[NC];
  const float uniform = 1.0f / (float)K;
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const int idx = c * G + lane;
    ti[c] = (idx < K) ? uniform * invden[idx] : 0.f;
    if (iters == 0 && idx < K) theta_row[idx] = uniform;
  }

  for (int it = 0; it < iters; ++it) {
#pragma unroll
    for (int c = 0; c < NC; ++c) m[c] = 0.f;

    for (int64_t base = o0; base < o1; base += G) {
      // G pairs, one per lane; word ids are below num_vocabs < 2^31
      const bool have = base + lane < o1;
      const int wv = have ? (int)obs_word[base + lane] : 0;
      const int cv = have ? obs_cnt[base + lane] : 0;
      const int nb = (o1 - base < G) ? (int)(o1 - base) : G;
      int j = 0;
      if (PF == 2) {
        for (; j + 1 < nb; j += 2) {
          int na[NC], nb2[NC];
          load_row<G, NC, FULL>(word_topic, __shfl(wv, j, G), K, lane, na);
          load_row<G, NC, FULL>(word_topic, __shfl(wv, j + 1, G), K, lane, nb2);
          fold_pair<G, NC>(na, ti, beta, (float)__shfl(cv, j, G), m);
          fold_pair<G, NC>(nb2, ti, beta, (float)__shfl(cv, j + 1, G), m);
        }
      }
      for (; j < nb; ++j) {
        int na[NC];
        load_row<G, NC, FULL>(word_topic, __shfl(wv, j, G), K, lane, na);
        fold_pair<G, NC>(na, ti, beta, (float)__shfl(cv, j, G), m);
      }
    }

#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const int idx = c * G + lane;
      const float th = (m[c] + alpha) / den;
      if (idx < K) {
        if (it == iters - 1) theta_row[idx] = th;
        ti[c] = th * invden[idx];
      }
    }
  }

  // every lane of the group holds the same total, so the same ll
  float ll = 0.f;
  for (int64_t base = s0; base < s1; base += G) {
    const bool have = base + lane < s1;
    const int wv = have ? (int)sc_word[base + lane] : 0;
    const int cv = have ? sc_cnt[base + lane] : 0;
    const int nb = (s1 - base < G) ? (int)(s1 - base) : G;
    for (int j = 0; j < nb; ++j) {
      int na[NC];
      float val[NC];
      load_row<G, NC, FULL>(word_topic, __shfl(wv, j, G), K, lane, na);
      ll += (float)__shfl(cv, j, G) *
            logf(pair_total<G, NC>(na, ti, beta, val));
    }
  }
  if (lane == 0) ll_out[doc] = ll;
}

template <int G, int NC, int PF, bool FULL>
void launch(const torch::Tensor& word_topic, const torch::Tensor& topic_sum,
            const torch::Tensor& obs_ptr, const torch::Tensor& obs_word,
            const torch::Tensor& obs_cnt, const torch::Tensor& sc_ptr,
            const torch::Tensor& sc_word, const torch::Tensor& sc_cnt,
            torch::Tensor& theta, torch::Tensor& ll, float alpha, float beta,
            float vbeta, int D, int K, int iters) {
  constexpr int GROUPS = BLOCK_THREADS / G;
  dim3 blk(BLOCK_THREADS), grid((D + GROUPS - 1) / GROUPS);
  hipLaunchKernelGGL((lda_foldin_kernel<G, NC, PF, FULL>), grid, blk,
                     (size_t)K * sizeof(float), current_stream(),
                     word_topic.data_ptr<int>(), topic_sum.data_ptr<int>(),
                     obs_ptr.data_ptr<int64_t>(),
                     obs_word.data_ptr<int64_t>(), obs_cnt.data_ptr<int>(),
                     sc_ptr.data_ptr<int64_t>(), sc_word.data_ptr<int64_t>(),
                     sc_cnt.data_ptr<int>(), theta.data_ptr<float>(),
                     ll.data_ptr<float>(), alpha, beta, vbeta, D, K, iters);
}

}  // namespace

int64_t lda_foldin_max_topics() { return WAVE * MAXC; }

// The caller (ops.lda_foldin) has checked that every word id is in
// [0, num_vocabs) and that the pair arrays have the lengths the ptr arrays
// end at; here only shapes and dtypes.
std::vector<torch::Tensor> lda_foldin(
    torch::Tensor word_topic, torch::Tensor topic_sum, torch::Tensor obs_ptr,
    torch::Tensor obs_word, torch::Tensor obs_cnt, torch::Tensor sc_ptr,
    torch::Tensor sc_word, torch::Tensor sc_cnt, double alpha, double beta,
    int64_t num_vocabs, int64_t iters) {
  CHECK_IN(word_topic); CHECK_IN(topic_sum); CHECK_IN(obs_ptr);
  CHECK_IN(obs_word); CHECK_IN(obs_cnt); CHECK_IN(sc_ptr); CHECK_IN(sc_word);
  CHECK_IN(sc_cnt);
  TORCH_CHECK(word_topic.dtype() == torch::kInt32 && word_topic.dim() == 2);
  TORCH_CHECK(topic_sum.dtype() == torch::kInt32);
  TORCH_CHECK(obs_ptr.dtype() == torch::kInt64 &&
              sc_ptr.dtype() == torch::kInt64);
  TORCH_CHECK(obs_word.dtype() == torch::kInt64 &&
              sc_word.dtype() == torch::kInt64);
  TORCH_CHECK(obs_cnt.dtype() == torch::kInt32 &&
              sc_cnt.dtype() == torch::kInt32);
  const int64_t K = word_topic.size(1);
  TORCH_CHECK(K >= 1 && K <= WAVE * MAXC, "num_topics > ", WAVE * MAXC,
              " unsupported");
  TORCH_CHECK(topic_sum.numel() == K, "topic_sum must hold num_topics counts");
  TORCH_CHECK(num_vocabs >= 1 && num_vocabs < ((int64_t)1 << 31) &&
              word_topic.size(0) >= num_vocabs,
              "word_topic has fewer than num_vocabs rows");
  TORCH_CHECK(obs_ptr.dim() == 1 && obs_ptr.size(0) >= 1 &&
              sc_ptr.dim() == 1 && sc_ptr.size(0) == obs_ptr.size(0),
              "obs_ptr and sc_ptr must both be [D + 1]");
  TORCH_CHECK(obs_cnt.numel() == obs_word.numel() &&
              sc_cnt.numel() == sc_word.numel());
  TORCH_CHECK(iters >= 0 && iters < (1 << 30));
  const int64_t D = obs_ptr.size(0) - 1;
  TORCH_CHECK(D < (int64_t)1 << 31);
  auto fopt = word_topic.options().dtype(torch::kFloat32);
  auto theta = torch::empty({D, K}, fopt);
  auto ll = torch::empty({D}, fopt);
  if (D == 0) return {theta, ll};

  const int G = (K <= 32 * MAXC) ? 32 : 64;
  const int nchunk = (int)((K + G - 1) / G);
  int nc = 1;
  while (nc < nchunk) nc <<= 1;
  int pf = 2;
  const char* env = getenv("HARMONY_LDA_FOLDIN_PF");      // A/B override
  if (env && atoi(env) == 1) pf = 1;
  if (env && atoi(env) == 2) pf = 2;

#define FOLDIN_LAUNCH(G_, NC_, PF_, FULL_)                                   \
  launch<G_, NC_, PF_, FULL_>(                                               \
      word_topic, topic_sum, obs_ptr, obs_word, obs_cnt, sc_ptr, sc_word,    \
      sc_cnt, theta, ll, (float)alpha, (float)beta,                          \
      (float)(num_vocabs * beta), (int)D, (int)K, (int)iters)
#define FOLDIN_FULL(G_, NC_, PF_)                                            \
  do {                                                                       \
    if (K == (NC_) * (G_)) FOLDIN_LAUNCH(G_, NC_, PF_, true);                \
    else FOLDIN_LAUNCH(G_, NC_, PF_, false);                                 \
  } while (0)
#define FOLDIN_PF(G_, NC_)                                                   \
  do {                                                                       \
    if (pf == 2) FOLDIN_FULL(G_, NC_, 2); else FOLDIN_FULL(G_, NC_, 1);      \
  } while (0)
#define FOLDIN_NC(G_)                                                        \
  switch (nc) {                                                              \
    case 1: FOLDIN_PF(G_, 1); break;                                         \
    case 2: FOLDIN_PF(G_, 2); break;                                         \
    case 4: FOLDIN_PF(G_, 4); break;                                         \
    case 8: FOLDIN_PF(G_, 8); break;                                         \
    default: FOLDIN_PF(G_, 16); break;                                       \
  }
  if (G == 32) { FOLDIN_NC(32) } else { FOLDIN_PF(64, 16); }   // K > 512
#undef FOLDIN_NC
#undef FOLDIN_PF
#undef FOLDIN_FULL
#undef FOLDIN_LAUNCH
  return {theta, ll};
}
