// K7b/K7c/K7d: Metropolis-Hastings alias LDA sampler (LightLDA-style).
//
// The exact dense sampler (lda.hip) costs O(K) per token. With the
// word-topic snapshot batch-stale (which it already is — see mlapps/lda.py),
// a 2-proposal MH step per token has the SAME stationary distribution at
// O(1) per token:
//   word proposal  t1 ~ q_w(k) ∝ (n_wk + b)/(n_k + Vb)  via a per-word
//                  TWO-LEVEL alias table built once per refresh; the
//                  acceptance uses the CURRENT snapshot for pi and the
//                  density qv the (possibly older) table encodes for q.
//   doc proposal   t2 ~ q_d(k) ∝ n~_dk + a  (n~ includes the current token)
//                  drawn in O(1): with prob aK/(aK+L_d) a uniform topic,
//                  else the topic of a uniformly chosen token of the doc;
//                  acceptance carries the full ratio with the doc-proposal
//                  correction.
//
// Two-level alias (exact): the row's K probabilities split into 64 lane
// segments of S = K/64; a 64-entry TOP alias selects the segment
// (mass-proportional), a per-segment alias selects the entry:
// P(k) = mass(g)/sum * p(k)/mass(g) = p(k)/sum. All 64 segment tables build
// CONCURRENTLY (one lane each, S serial steps) and only the 64-entry top
// table is a serial chain.
//
// The file has ONE token step, ONE table-row build and three kernel shapes:
//   mh_token_step<Tables, Counts>  the MH step. `Tables` says where the stale
//       tables live (LegacyTables: five arrays, run-time K; PackedTables<S>:
//       one 16*S-byte record per (word, segment) plus 8-byte top pairs),
//       `Counts` how the doc-topic row in LDS is updated (U8Counts: private
//       row, plain ops; AtomicCounts: row shared by a wave). RNG: counter
//       hash (hip_common.h) at ctr = token*8 + draw, mirrored by the torch
//       reference for sample-exact CPU/GPU tests.
//   alias_build_row<CS>            one row's tables in LDS (CS = compile-time
//       S, or 0 for any K % 64 == 0). alias_build_kernel writes six arrays,
//       alias_build_packed_kernel<S> packed records — the same bits.
//   lda_mh_kernel<PF>              K7b, thread per doc, u8 rows, exact vs the
//       CPU oracle; PF prefetches the next token's top entry.
//   lda_mh_wave_kernel<Tables, FUSED>  K7c/K7d, wave per doc, lanes take
//       tokens round-robin and share the row through LDS atomics. With
//       PackedTables it is the benchmark's kernel; FUSED also applies the
//       +/-1 of every moved token to the table shard.

#include "hip_common.h"
#include <cstdlib>
#include <algorithm>

namespace {

constexpr int ALIAS_THREADS = 64;   // same-box interleaved A/B: 64 beats 128
                                    // (isolated 0.59 vs 0.655 ms; 3-job bench
                                    // 1.59/1.62 vs 1.63/1.66 ms/step) — the
                                    // earlier '64 = 1.74 ms' was cross-box noise
constexpr int BUILD_WAVES = 4;

// ---------------------------------------------------------------- layout --
// K7d packed tables. The legacy layout keeps [rows][K] / [rows][64] arrays
// and a token touches ~9 different 128-byte lines of them. The stale tables
// of one (word, lane segment) pair live here in ONE record of 16*S bytes:
//   rec[row][seg] = { reserved[S] | prob[S] | qv[S] | alias[S] } (int32 bits)
//   top[row][seg] = { top_prob, top_alias }                      (8 bytes)
// t1 is drawn inside segment g, so prob/alias/qv[t1] are one record and
// qv[s] is record s/S. The counts stay in the dense pulled snapshot: a
// per-step refresh of a count slot inside every record (the reserved slot)
// was measured and lost, see profiles/r04_lda_step.md. That leaves about
// six lines per token: top, rec(g), rec(s/S) and count[s], count[t1],
// count[t2].

// S consecutive ints at a 4*S-byte aligned address, widest access <= 16 B
template <int S>
__device__ __forceinline__ void ld_slot(const int* __restrict__ p,
                                        int (&v)[S]) {
  if constexpr (S == 1) {
    v[0] = p[0];
  } else if constexpr (S == 2) {
    const int2 t = *reinterpret_cast<const int2*>(p);
    v[0] = t.x; v[1] = t.y;
  } else {
#pragma unroll
    for (int i = 0; i < S / 4; ++i) {
      const int4 t = reinterpret_cast<const int4*>(p)[i];
      v[4 * i] = t.x; v[4 * i + 1] = t.y; v[4 * i + 2] = t.z;
      v[4 * i + 3] = t.w;
    }
  }
}

template <int S>
__device__ __forceinline__ void st_slot(int* __restrict__ p,
                                        const int (&v)[S]) {
  if constexpr (S == 1) {
    p[0] = v[0];
  } else if constexpr (S == 2) {
    *reinterpret_cast<int2*>(p) = make_int2(v[0], v[1]);
  } else {
#pragma unroll
    for (int i = 0; i < S / 4; ++i)
      reinterpret_cast<int4*>(p)[i] =
          make_int4(v[4 * i], v[4 * i + 1], v[4 * i + 2], v[4 * i + 3]);
  }
}

// One whole record in registers, fields picked by compare/select. Each
// field is kept as its own 4-wide pieces: one 4*S-wide array indexed by a
// lane-varying value is put in scratch memory by the compiler.
__device__ __forceinline__ int sel4(const int4& v, int i) {
  return (i == 0) ? v.x : (i == 1) ? v.y : (i == 2) ? v.z : v.w;
}

template <int S> struct SegRecord;

template <> struct SegRecord<1> {
  int4 t;
  __device__ __forceinline__ explicit SegRecord(const int* p)
      : t(*reinterpret_cast<const int4*>(p)) {}
  __device__ __forceinline__ int field(int f, int) const { return sel4(t, f); }
};

template <> struct SegRecord<2> {
  int4 a, b;                       // {c0 c1 p0 p1} {q0 q1 a0 a1}
  __device__ __forceinline__ explicit SegRecord(const int* p)
      : a(reinterpret_cast<const int4*>(p)[0]),
        b(reinterpret_cast<const int4*>(p)[1]) {}
  __device__ __forceinline__ int field(int f, int i) const {
    return sel4(f < 2 ? a : b, (f & 1) * 2 + i);
  }
};

template <> struct SegRecord<4> {
  int4 t[4];
  __device__ __forceinline__ explicit SegRecord(const int* p) {
#pragma unroll
    for (int f = 0; f < 4; ++f) t[f] = reinterpret_cast<const int4*>(p)[f];
  }
  __device__ __forceinline__ int field(int f, int i) const {
    return sel4(t[f], i);
  }
};

template <> struct SegRecord<8> {
  int4 t[8];
  __device__ __forceinline__ explicit SegRecord(const int* p) {
#pragma unroll
    for (int f = 0; f < 8; ++f) t[f] = reinterpret_cast<const int4*>(p)[f];
  }
  __device__ __forceinline__ int field(int f, int i) const {
    const int lo = sel4(t[2 * f], i & 3), hi = sel4(t[2 * f + 1], i & 3);
    return (i < 4) ? lo : hi;
  }
};

// ----------------------------------------------------------- table build --

// In-LDS serial Vose over n entries at pr[0..n), links lk, output al.
// Deterministic order (descending init so pops ascend) — the torch
// reference replicates it exactly.
__device__ void vose_serial(float* pr, int* al, int* lk, int n) {
  int small_top = -1, large_top = -1;
  for (int k = n - 1; k >= 0; --k) {
    if (pr[k] < 1.f) { lk[k] = small_top; small_top = k; }
    else             { lk[k] = large_top; large_top = k; }
  }
  while (small_top >= 0 && large_top >= 0) {
    const int sm = small_top; small_top = lk[sm];
    const int lg = large_top;
    al[sm] = lg;
    const float rem = (pr[lg] + pr[sm]) - 1.f;
    pr[lg] = rem;
    large_top = lk[lg];
    if (rem < 1.f) { lk[lg] = small_top; small_top = lg; }
    else           { lk[lg] = large_top; large_top = lg; }
  }
  while (large_top >= 0) { const int lg = large_top; large_top = lk[lg];
                           pr[lg] = 1.f; al[lg] = lg; }
  while (small_top >= 0) { const int sm = small_top; small_top = lk[sm];
                           pr[sm] = 1.f; al[sm] = sm; }
}

// One wave's LDS scratch for a row:
// pr[K] f32 | al[K] i32 | lk[K] i32 | tp[64] f32 | ta[64] i32 | tl[64] i32
struct BuildLds {
  float* pr; int* al; int* lk; float* tp; int* ta; int* tl;
  __device__ __forceinline__ BuildLds(float* smem, int wave, int K) {
    pr = smem + (size_t)wave * (3 * (size_t)K + 3 * WAVE);
    al = (int*)(pr + K);
    lk = al + K;
    tp = (float*)(lk + K);
    ta = (int*)(tp + WAVE);
    tl = ta + WAVE;
  }
};

// One row of alias tables, built by one wave. Lane `lane` owns the segment
// [lane*S, (lane+1)*S): it reads its S counts at cnt_p and writes the S
// proposal densities qv = p/total (what the tables encode; the stale-table
// acceptance needs it) at qv_p. On return the LDS holds the entry tables
// (l.pr, l.al) and the top table (l.tp, l.ta), visible to every lane; the
// row's total mass is returned on every lane. CS > 0 fixes S at compile
// time (16-byte accesses, unrolled), CS == 0 takes any S_rt.
template <int CS>
__device__ __forceinline__ float alias_build_row(
    const BuildLds& l, int lane, int S_rt, const int* __restrict__ cnt_p,
    const float* __restrict__ invden, float beta, int* __restrict__ qv_p) {
  constexpr int N = CS > 0 ? CS : 1;
  const int S = CS > 0 ? CS : S_rt;
  float* pr = l.pr + lane * S;
  const float* inv = invden + lane * S;
  int v[N];
  if constexpr (CS > 0) ld_slot<N>(cnt_p, v);
  float seg_mass = 0.f;
  for (int i = 0; i < S; ++i) {
    int n;
    if constexpr (CS > 0) n = v[i]; else n = cnt_p[i];
    const float c = (float)n + beta;
    pr[i] = c * inv[i];
    // the stored p is rounded, the mass takes the product unrounded: a
    // fused multiply-add, written out so that the compiler's contraction
    // choice cannot change the last bit of the mass (and with it qsum, qv
    // and every table entry)
    seg_mass = __fmaf_rn(c, inv[i], seg_mass);
  }
  const float total = wave_reduce_sum(seg_mass);
  const float inv_total = 1.f / total;
  if constexpr (CS > 0) {
    for (int i = 0; i < S; ++i) v[i] = __float_as_int(pr[i] * inv_total);
    st_slot<N>(qv_p, v);
  } else {
    for (int i = 0; i < S; ++i) qv_p[i] = __float_as_int(pr[i] * inv_total);
  }
  // per-segment alias: normalize within segment to mean 1 (concurrent
  // across all 64 lanes; each runs a tiny S-entry serial Vose)
  const float sscale = (seg_mass > 0.f) ? (float)S / seg_mass : 0.f;
  for (int i = 0; i < S; ++i) pr[i] *= sscale;
  vose_serial(pr, l.al + lane * S, l.lk + lane * S, S);
  // top alias over segment masses (normalized to mean 1 across 64)
  l.tp[lane] = seg_mass * (float)WAVE / total;
  if (lane == 0) vose_serial(l.tp, l.ta, l.tl, WAVE);
  // lanes 1..63 read what lane 0 just wrote to tp/ta (and the dense
  // write-back reads other lanes' segments): without the fence the
  // compiler forwards each lane's own earlier store of tp[lane]
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  return total;
}

// Dense rows in, six arrays out; any K % 64 == 0.
__global__ void alias_build_kernel(const int* __restrict__ word_topic,
                                   const float* __restrict__ invden,
                                   float beta,
                                   float* __restrict__ prob,     // [rows][K]
                                   int* __restrict__ alias,      // [rows][K]
                                   float* __restrict__ top_prob, // [rows][64]
                                   int* __restrict__ top_alias,  // [rows][64]
                                   float* __restrict__ qv,       // [rows][K]
                                   float* __restrict__ qsum,     // [rows]
                                   int rows, int K) {
  extern __shared__ float smem_f[];
  const int wave = threadIdx.x / WAVE;
  const int lane = threadIdx.x % WAVE;
  const BuildLds l(smem_f, wave, K);
  const int S = K / WAVE;                  // entries per lane segment
  const int waves_wg = blockDim.x / WAVE;
  for (int row = blockIdx.x * waves_wg + wave; row < rows;
       row += gridDim.x * waves_wg) {
    const int64_t base = (int64_t)row * K;
    const float total = alias_build_row<0>(
        l, lane, S, word_topic + base + lane * S, invden, beta,
        reinterpret_cast<int*>(qv) + base + lane * S);
    if (lane == 0) qsum[row] = total;
    // coalesced write-back
    for (int c = 0; c < S; ++c) {
      const int k = c * WAVE + lane;
      prob[base + k] = l.pr[k];
      alias[base + k] = l.al[k];
    }
    top_prob[(int64_t)row * WAVE + lane] = l.tp[lane];
    top_alias[(int64_t)row * WAVE + lane] = l.ta[lane];
  }
}

// The row read through src_rows (the table shard in place) or densely, and
// the tables written as packed records; S in {1, 2, 4, 8}.
template <int S>
__global__ void alias_build_packed_kernel(const int* __restrict__ src,
                                          const int* __restrict__ src_rows,
                                          const float* __restrict__ invden,
                                          float beta,
                                          int* __restrict__ rec,   // [rows][64][4S]
                                          int2* __restrict__ top,  // [rows][64]
                                          float* __restrict__ qsum,
                                          int rows) {
  constexpr int K = S * WAVE;
  extern __shared__ float smem_f[];
  const int wave = threadIdx.x / WAVE;
  const int lane = threadIdx.x % WAVE;
  const BuildLds l(smem_f, wave, K);
  const int waves_wg = blockDim.x / WAVE;
  for (int row = blockIdx.x * waves_wg + wave; row < rows;
       row += gridDim.x * waves_wg) {
    const int64_t base = (int64_t)(src_rows ? src_rows[row] : row) * K;
    int* r = rec + ((int64_t)row * WAVE + lane) * (4 * S);
    const float total = alias_build_row<S>(l, lane, S, src + base + lane * S,
                                           invden, beta, r + 2 * S);   // qv
    if (lane == 0) qsum[row] = total;
    int out[S];
#pragma unroll
    for (int i = 0; i < S; ++i) out[i] = __float_as_int(l.pr[lane * S + i]);
    st_slot<S>(r + S, out);                             // prob
#pragma unroll
    for (int i = 0; i < S; ++i) out[i] = l.al[lane * S + i];
    st_slot<S>(r + 3 * S, out);                         // alias
    top[(int64_t)row * WAVE + lane] =
        make_int2(__float_as_int(l.tp[lane]), l.ta[lane]);
  }
}

// ------------------------------------------------------------ token step --

struct TopEntry { float prob; int alias; };
struct SegEntry { int lt; float qv_t; };     // topic within segment, its qv

// Tables view over the legacy arrays; K and S are run-time.
struct LegacyTables {
  using word_t = int64_t;
  const float* prob;       // [rows][K] entry alias prob
  const int* alias;        // [rows][K] entry alias index
  const float* top_prob;   // [rows][64]
  const int* top_alias;    // [rows][64]
  const float* qv_;        // [rows][K] proposal density
  int K, S;
  __device__ __forceinline__ TopEntry top(int64_t w, int gb) const {
    const int64_t i = w * WAVE + gb;
    return {top_prob[i], top_alias[i]};
  }
  __device__ __forceinline__ SegEntry entry(int64_t w, int g, float frac,
                                            int eb) const {
    const int64_t ebase = w * K + g * S;
    const int lt = (frac < prob[ebase + eb]) ? eb : alias[ebase + eb];
    return {lt, qv_[ebase + lt]};
  }
  __device__ __forceinline__ float qv(int64_t w, int k) const {
    return qv_[w * K + k];
  }
};

// Tables view over the packed records: rec(g) is loaded whole (S x 16
// bytes) and prob[eb]/alias[eb], then qv[t1], are selected in registers.
template <int S_>
struct PackedTables {
  using word_t = int;
  static constexpr int S = S_, K = S_ * WAVE;
  static constexpr int R = 4 * S_;             // ints per record
  const int* rec;          // [rows][64][R]
  const int2* tops;        // [rows][64]
  __device__ __forceinline__ const int* word(int w) const {
    return rec + (int64_t)w * (WAVE * R);
  }
  __device__ __forceinline__ TopEntry top(int w, int gb) const {
    const int2 t = tops[(int64_t)w * WAVE + gb];
    return {__int_as_float(t.x), t.y};
  }
  __device__ __forceinline__ SegEntry entry(int w, int g, float frac,
                                            int eb) const {
    const SegRecord<S> rg(word(w) + g * R);
    const int lt = (frac < __int_as_float(rg.field(1, eb)))
                       ? eb : rg.field(3, eb);
    return {lt, __int_as_float(rg.field(2, lt))};
  }
  __device__ __forceinline__ float qv(int w, int k) const {
    return __int_as_float(word(w)[(k / S) * R + 2 * S + (k % S)]);
  }
};

// Doc-topic row private to one thread (counts <= doc length <= 255).
struct U8Counts {
  unsigned char* nd;
  __device__ __forceinline__ int take(int k) const { return nd[k] -= 1; }
  __device__ __forceinline__ int get(int k) const { return nd[k]; }
  __device__ __forceinline__ void put(int k) const { nd[k] += 1; }
};

// Doc-topic row shared by the lanes of a wave. take() is the value after MY
// decrement; other lanes race, so get() reads approximately-current counts
// (standard GPU-LDA relaxation, validated by scripts/lda_convergence.py).
struct AtomicCounts {
  int* nd;
  __device__ __forceinline__ int take(int k) const {
    return atomicAdd(&nd[k], -1) - 1;
  }
  __device__ __forceinline__ int get(int k) const { return nd[k]; }
  __device__ __forceinline__ void put(int k) const { atomicAdd(&nd[k], 1); }
};

// The tokens [p0, p1) of one doc and what the doc proposal needs of them.
struct DocSpan {
  int64_t p0, p1;
  float Ld, p_uniform;
  // inactive tail docs get an empty span: their threads skip the token
  // loop but still reach the block-wide barriers
  __device__ __forceinline__ DocSpan(const int64_t* __restrict__ doc_offsets,
                                     int doc, int n_docs, float alpha, int K) {
    const bool active = doc < n_docs;
    p0 = active ? doc_offsets[doc] : 0;
    p1 = active ? doc_offsets[doc + 1] : 0;
    Ld = (float)(p1 - p0);
    const float aK = alpha * (float)K;
    p_uniform = aK / (aK + Ld);
  }
};

// First-level draw of token p's word proposal: it depends only on
// (seed, p, word), so a caller may issue it ahead of the token's step.
struct SegDraw { float u1; int gb; TopEntry top; };

template <class Tables>
__device__ __forceinline__ SegDraw draw_segment(const Tables& tv,
                                                unsigned int seed, int64_t p,
                                                typename Tables::word_t w) {
  const float u1 = rng_uniform(seed, (unsigned int)(p * 8)) * (float)WAVE;
  int gb = (int)u1;
  if (gb >= WAVE) gb = WAVE - 1;
  return {u1, gb, tv.top(w, gb)};
}

// One MH step of token p (word w, current topic s): removes the token from
// the doc row, runs the word and the doc proposal, puts the token back under
// its new topic and returns that topic. wcnt is the word's row of the pulled
// snapshot, read-only during a sweep. Draws use counters p*8 + 0..6 (0 is
// draw_segment's).
template <class Tables, class Counts>
__device__ __forceinline__ int mh_token_step(
    const Tables& tv, const Counts& nd, const int* __restrict__ wcnt,
    const float* __restrict__ invden, const int* z,
    typename Tables::word_t w, int64_t p, const DocSpan& d, float alpha,
    float beta, unsigned int seed, int s, const SegDraw& sd) {
  const int K = tv.K, S = tv.S;
  // both loads are issued before the LDS update of take()
  int cnt_s = wcnt[s];
  const float qv_s = tv.qv(w, s);
  const int nds0 = nd.take(s);                 // exclude the token
  const unsigned int c0 = (unsigned int)(p * 8);
  // ---- word proposal (two-level alias) ----
  {
    const int g = (sd.u1 - (float)sd.gb < sd.top.prob) ? sd.gb : sd.top.alias;
    const float u2 = rng_uniform(seed, c0 + 6) * (float)S;
    int eb = (int)u2;
    if (eb >= S) eb = S - 1;
    const SegEntry e = tv.entry(w, g, u2 - (float)eb, eb);
    const int t1 = g * S + e.lt;
    const int cnt_t = wcnt[t1];
    // acceptance: pi uses the CURRENT snapshot, q the (possibly older)
    // table's encoded density — with a fresh table the word factors
    // cancel mathematically; the explicit form stays correct when the
    // tables are reused across several pulls (alias_refresh)
    const float pi_s = ((float)nds0 + alpha) *
        ((float)cnt_s + beta) * invden[s];
    const float pi_t = ((float)nd.get(t1) + alpha) *
        ((float)cnt_t + beta) * invden[t1];
    const float a1 = (pi_t * qv_s) / (pi_s * e.qv_t);
    if (rng_uniform(seed, c0 + 1) < a1) { s = t1; cnt_s = cnt_t; }
  }
  // ---- doc proposal: q_d ∝ n~_dk + a (n~ includes current token) ----
  {
    int t2;
    if (rng_uniform(seed, c0 + 2) < d.p_uniform) {
      t2 = (int)(rng_uniform(seed, c0 + 3) * (float)K);
      if (t2 >= K) t2 = K - 1;
    } else {
      int64_t j = d.p0 + (int64_t)(rng_uniform(seed, c0 + 4) * d.Ld);
      if (j >= d.p1) j = d.p1 - 1;
      t2 = (j == p) ? s : z[j];
    }
    const int cnt_t2 = wcnt[t2];
    const float nds = (float)nd.get(s), ndt = (float)nd.get(t2);
    // n~ (proposal counts) include the current assignment s
    const float qs = nds + 1.f + alpha;
    const float qt = ndt + (t2 == s ? 1.f : 0.f) + alpha;
    const float pis = (nds + alpha) *
        ((float)cnt_s + beta) * invden[s];
    const float pit = (ndt + alpha) *
        ((float)cnt_t2 + beta) * invden[t2];
    const float a2 = (pit * qs) / (pis * qt);
    if (rng_uniform(seed, c0 + 5) < a2) s = t2;
  }
  nd.put(s);
  return s;
}

// ---------------------------------------------------------------- sweeps --

// K7b: ONE THREAD PER DOCUMENT (per-token work is scalar), the doc-topic
// counts as a u8 LDS row, tokens serial per doc. Sample-exact vs the CPU
// oracle but parallelism-starved: each token's acceptance chain is a
// dependent global-load sequence with too few waves to hide it.
template <bool PF>
__global__ __launch_bounds__(256)
void lda_mh_kernel(int* __restrict__ doc_topic,        // [D][K] int32
                   const int* __restrict__ word_topic, // [rows][K] (fresh)
                   const float* __restrict__ invden,   // [K]
                   const LegacyTables tv,
                   const int64_t* __restrict__ doc_offsets,
                   const int64_t* __restrict__ word_ids,
                   int* __restrict__ z,
                   float alpha, float beta,
                   int n_docs, unsigned int seed) {
  extern __shared__ unsigned char nd8[];               // [THREADS][K] u8
  const int K = tv.K;
  const int doc = blockIdx.x * blockDim.x + threadIdx.x;
  const U8Counts nd{nd8 + (size_t)threadIdx.x * K};
  const int64_t gbase = (int64_t)blockIdx.x * blockDim.x * K;
  const int ndocs_wg =
      min((int)blockDim.x, n_docs - (int)(blockIdx.x * blockDim.x));
  // coalesced block-wide row staging: the WG's docs are contiguous, so the
  // [docs x K] slice loads as one flat stream (thread-private loops would
  // put adjacent lanes 1 KB apart — every 4 B load its own cacheline)
  for (int i = threadIdx.x; i < ndocs_wg * K; i += blockDim.x)
    nd8[i] = (unsigned char)doc_topic[gbase + i];
  __syncthreads();
  const DocSpan d(doc_offsets, doc, n_docs, alpha, K);
  // software-prefetched first-level draw: token p+1's two top-table loads
  // are issued before token p's dependent acceptance chain
  SegDraw next{};
  if (PF && d.p0 < d.p1) next = draw_segment(tv, seed, d.p0, word_ids[d.p0]);
  for (int64_t p = d.p0; p < d.p1; ++p) {
    const int64_t w = word_ids[p];
    SegDraw cur = next;
    if (!PF) cur = draw_segment(tv, seed, p, w);
    else if (p + 1 < d.p1) next = draw_segment(tv, seed, p + 1, word_ids[p + 1]);
    z[p] = mh_token_step(tv, nd, word_topic + w * K, invden, z, w, p, d,
                         alpha, beta, seed, z[p], cur);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < ndocs_wg * K; i += blockDim.x)
    doc_topic[gbase + i] = (int)nd8[i];
}

// K7c/K7d: wave-per-doc MH sweep. A FULL WAVE cooperates on one doc: lanes
// take tokens round-robin and share the doc-topic row in LDS via atomics —
// within-doc token updates become approximately parallel. The legacy and the
// packed tables give bit-identical samples under the same LDS interleaving.
// FUSED: the kernel holds (word, old topic, new topic) of every token and
// samples from the pulled snapshot, never from the shard, so it applies the
// +/-1 to the shard row itself; the scattered atomics overlap the sampler's
// own load latency instead of running as a pass of their own. Summary-row
// deltas stage through an LDS histogram per workgroup (see
// lda_apply_all_kernel for why not per-token global atomics).
template <class Tables, bool FUSED>
__global__ __launch_bounds__(256)
void lda_mh_wave_kernel(int* __restrict__ doc_topic,
                        const int* __restrict__ word_topic,
                        const float* __restrict__ invden,
                        const Tables tv,
                        const int64_t* __restrict__ doc_offsets,
                        const typename Tables::word_t* __restrict__ word_ids,
                        int* __restrict__ z,
                        int* __restrict__ shard,
                        const int* __restrict__ row_of_local,
                        int64_t summary_row,
                        float alpha, float beta,
                        int n_docs, unsigned int seed) {
  extern __shared__ int ndw[];                 // [waves_wg][K] (+ [K] FUSED)
  const int K = tv.K;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int waves_wg = blockDim.x >> 6;
  const int doc = blockIdx.x * waves_wg + wave;
  const AtomicCounts nd{ndw + (size_t)wave * K};
  int* ssum = ndw + (size_t)waves_wg * K;
  const int64_t gbase = (int64_t)blockIdx.x * waves_wg * K;
  const int ndocs_wg = min(waves_wg, n_docs - blockIdx.x * waves_wg);
  for (int i = tid; i < ndocs_wg * K; i += blockDim.x)
    ndw[i] = doc_topic[gbase + i];
  if (FUSED)
    for (int k = tid; k < K; k += blockDim.x) ssum[k] = 0;
  __syncthreads();
  const DocSpan d(doc_offsets, doc, n_docs, alpha, K);
  for (int64_t p = d.p0 + lane; p < d.p1; p += WAVE) {
    const typename Tables::word_t w = word_ids[p];
    const int s_old = z[p];
    const int s = mh_token_step(tv, nd, word_topic + (int64_t)w * K, invden,
                                z, w, p, d, alpha, beta, seed, s_old,
                                draw_segment(tv, seed, p, w));
    z[p] = s;
    if (FUSED && s != s_old) {
      int* srow = shard + (int64_t)row_of_local[w] * K;
      atomicSub(&srow[s_old], 1);
      atomicAdd(&srow[s], 1);
      atomicSub(&ssum[s_old], 1);
      atomicAdd(&ssum[s], 1);
    }
  }
  __syncthreads();
  for (int i = tid; i < ndocs_wg * K; i += blockDim.x)
    doc_topic[gbase + i] = ndw[i];
  if (FUSED)
    for (int k = tid; k < K; k += blockDim.x) {
      const int v = ssum[k];
      if (v != 0) atomicAdd(&shard[summary_row * K + k], v);
    }
}

// ------------------------------------------------------------------ host --

// 1 / (n_k + V*beta), the per-topic factor both builds and samplers share
torch::Tensor build_invden(const torch::Tensor& topic_sum, double beta,
                           int64_t num_vocabs) {
  auto invden = 1.0 / (topic_sum.to(torch::kFloat32)
                       + (double)num_vocabs * beta);
  return invden.contiguous();
}

// One wave per row, grid-strided; LDS as laid out by BuildLds.
struct BuildLaunch {
  dim3 grid, blk;
  size_t shmem;
  BuildLaunch(int rows, int K, int waves)
      : grid(std::min((rows + waves - 1) / waves, 8192)), blk(WAVE * waves),
        shmem((size_t)waves * (3 * K + 3 * WAVE) * 4) {}
};

// lda_mh and lda_mh_wave: the same arguments over the legacy arrays, thread
// per doc or wave per doc.
torch::Tensor launch_legacy_mh(bool wave, torch::Tensor doc_topic,
                               torch::Tensor word_topic, torch::Tensor invden,
                               torch::Tensor prob, torch::Tensor alias,
                               torch::Tensor top_prob, torch::Tensor top_alias,
                               torch::Tensor qv, torch::Tensor doc_offsets,
                               torch::Tensor word_ids,
                               torch::Tensor assignments,
                               double alpha, double beta, int64_t seed) {
  CHECK_IN(doc_topic); CHECK_IN(word_topic); CHECK_IN(invden);
  CHECK_IN(prob); CHECK_IN(alias); CHECK_IN(top_prob); CHECK_IN(top_alias);
  CHECK_IN(qv); CHECK_IN(doc_offsets); CHECK_IN(word_ids);
  CHECK_IN(assignments);
  const int D = doc_topic.size(0), K = doc_topic.size(1);
  if (D == 0) return assignments;
  const LegacyTables tv{prob.data_ptr<float>(), alias.data_ptr<int>(),
                        top_prob.data_ptr<float>(), top_alias.data_ptr<int>(),
                        qv.data_ptr<float>(), K, K / WAVE};
  const unsigned int seed32 = (unsigned int)(seed & 0xffffffff);
  if (wave) {
    int waves_wg = 4;                    // 256 threads, 4 docs per block
    const char* we = getenv("HARMONY_LDA_WAVE_WG");   // occupancy A/B
    if (we) { int v = atoi(we); if (v >= 1 && v <= 4) waves_wg = v; }  // <=4: 256-thread launch bound
    dim3 blk(WAVE * waves_wg), grid((D + waves_wg - 1) / waves_wg);
    const size_t shmem = (size_t)waves_wg * K * 4;
    hipLaunchKernelGGL((lda_mh_wave_kernel<LegacyTables, false>), grid, blk,
                       shmem, current_stream(), doc_topic.data_ptr<int>(),
                       word_topic.data_ptr<int>(), invden.data_ptr<float>(),
                       tv, doc_offsets.data_ptr<int64_t>(),
                       word_ids.data_ptr<int64_t>(),
                       assignments.data_ptr<int>(), (int*)nullptr,
                       (const int*)nullptr, (int64_t)0,
                       (float)alpha, (float)beta, D, seed32);
    return assignments;
  }
  int threads = ALIAS_THREADS;    // HARMONY_LDA_MH_THREADS: fill/LDS A/B
  const char* te = getenv("HARMONY_LDA_MH_THREADS");
  if (te) { int t = atoi(te); if (t==64 || t==128 || t==256) threads = t; }
  dim3 blk(threads), grid((D + threads - 1) / threads);
  const size_t shmem = (size_t)threads * K;           // u8 rows
  TORCH_CHECK(shmem <= 160 * 1024, "K too large for u8 LDS rows");
  const char* pe = getenv("HARMONY_LDA_MH_PREFETCH");
  const bool pf = !(pe && atoi(pe) == 0);   // default: prefetch on
  auto kern = pf ? lda_mh_kernel<true> : lda_mh_kernel<false>;
  hipLaunchKernelGGL(kern, grid, blk, shmem, current_stream(),
                     doc_topic.data_ptr<int>(), word_topic.data_ptr<int>(),
                     invden.data_ptr<float>(), tv,
                     doc_offsets.data_ptr<int64_t>(),
                     word_ids.data_ptr<int64_t>(),
                     assignments.data_ptr<int>(),
                     (float)alpha, (float)beta, D, seed32);
  return assignments;
}

}  // namespace

std::vector<torch::Tensor> lda_alias_build(torch::Tensor word_topic,
                                           torch::Tensor topic_sum,
                                           double beta, int64_t num_vocabs) {
  CHECK_IN(word_topic); CHECK_IN(topic_sum);
  TORCH_CHECK(word_topic.dtype() == torch::kInt32);
  const int rows = word_topic.size(0), K = word_topic.size(1);
  TORCH_CHECK(K % WAVE == 0, "alias sampler requires K % 64 == 0");
  auto invden = build_invden(topic_sum, beta, num_vocabs);
  auto prob = torch::empty({rows, K},
                           word_topic.options().dtype(torch::kFloat32));
  auto alias = torch::empty({rows, K}, word_topic.options());
  auto top_prob = torch::empty({rows, WAVE},
                               word_topic.options().dtype(torch::kFloat32));
  auto top_alias = torch::empty({rows, WAVE}, word_topic.options());
  auto qv = torch::empty({rows, K},
                         word_topic.options().dtype(torch::kFloat32));
  auto qsum = torch::empty({rows}, prob.options());
  if (rows > 0) {
    int waves = BUILD_WAVES;       // HARMONY_LDA_BUILD_WAVES: occupancy A/B
    const char* bw = getenv("HARMONY_LDA_BUILD_WAVES");
    if (bw) { int w = atoi(bw); if (w >= 1 && w <= 8) waves = w; }
    const BuildLaunch L(rows, K, waves);
    hipLaunchKernelGGL(alias_build_kernel, L.grid, L.blk, L.shmem,
                       current_stream(),
                       word_topic.data_ptr<int>(), invden.data_ptr<float>(),
                       (float)beta, prob.data_ptr<float>(),
                       alias.data_ptr<int>(), top_prob.data_ptr<float>(),
                       top_alias.data_ptr<int>(), qv.data_ptr<float>(),
                       qsum.data_ptr<float>(), rows, K);
  }
  return {prob, alias, top_prob, top_alias, qv, qsum, invden};
}

torch::Tensor lda_mh(torch::Tensor doc_topic, torch::Tensor word_topic,
                     torch::Tensor invden, torch::Tensor prob,
                     torch::Tensor alias, torch::Tensor top_prob,
                     torch::Tensor top_alias, torch::Tensor qv,
                     torch::Tensor doc_offsets,
                     torch::Tensor word_ids, torch::Tensor assignments,
                     double alpha, double beta, int64_t seed) {
  return launch_legacy_mh(false, doc_topic, word_topic, invden, prob, alias,
                          top_prob, top_alias, qv, doc_offsets, word_ids,
                          assignments, alpha, beta, seed);
}

torch::Tensor lda_mh_wave(torch::Tensor doc_topic, torch::Tensor word_topic,
                          torch::Tensor invden, torch::Tensor prob,
                          torch::Tensor alias, torch::Tensor top_prob,
                          torch::Tensor top_alias, torch::Tensor qv,
                          torch::Tensor doc_offsets,
                          torch::Tensor word_ids,
                          torch::Tensor assignments,
                          double alpha, double beta, int64_t seed) {
  return launch_legacy_mh(true, doc_topic, word_topic, invden, prob, alias,
                          top_prob, top_alias, qv, doc_offsets, word_ids,
                          assignments, alpha, beta, seed);
}

// ---- K7d host entries: packed tables ----

#define LDA_DISPATCH_S(S_, ...)                                     \
  switch (S_) {                                                     \
    case 1: { constexpr int S = 1; __VA_ARGS__; break; }            \
    case 2: { constexpr int S = 2; __VA_ARGS__; break; }            \
    case 4: { constexpr int S = 4; __VA_ARGS__; break; }            \
    case 8: { constexpr int S = 8; __VA_ARGS__; break; }            \
    default: TORCH_CHECK(false, "packed LDA tables need K/64 in {1,2,4,8}"); \
  }

static int packed_S(const torch::Tensor& rec, const torch::Tensor& top) {
  CHECK_IN(rec); CHECK_IN(top);
  TORCH_CHECK(rec.dtype() == torch::kInt32 && top.dtype() == torch::kInt32);
  TORCH_CHECK(rec.dim() == 3 && rec.size(1) == WAVE && rec.size(2) % 4 == 0,
              "rec must be [rows][64][4*S] int32");
  TORCH_CHECK(top.dim() == 3 && top.size(0) == rec.size(0) &&
              top.size(1) == WAVE && top.size(2) == 2,
              "top must be [rows][64][2] int32");
  return (int)(rec.size(2) / 4);
}

static const int* check_rows(const c10::optional<torch::Tensor>& src_rows,
                             const torch::Tensor& src, int64_t rows, int K) {
  CHECK_IN(src);
  TORCH_CHECK(src.dtype() == torch::kInt32 && src.dim() == 2 &&
              src.size(1) == K, "src must be [n][K] int32");
  if (!src_rows.has_value()) {
    TORCH_CHECK(src.size(0) >= rows, "src has fewer rows than rec");
    return nullptr;
  }
  const torch::Tensor& r = *src_rows;
  CHECK_IN(r);
  TORCH_CHECK(r.dtype() == torch::kInt32 && r.dim() == 1 &&
              r.size(0) == rows, "src_rows must be [rows] int32");
  return r.data_ptr<int>();
}

std::vector<torch::Tensor> lda_alias_build_packed(
    torch::Tensor src, c10::optional<torch::Tensor> src_rows,
    torch::Tensor topic_sum, double beta, int64_t num_vocabs,
    torch::Tensor rec, torch::Tensor top) {
  CHECK_IN(topic_sum);
  const int S_ = packed_S(rec, top);
  const int rows = rec.size(0), K = S_ * WAVE;
  TORCH_CHECK(topic_sum.numel() == K);
  const int* rows_p = check_rows(src_rows, src, rows, K);
  auto invden = build_invden(topic_sum, beta, num_vocabs);
  auto qsum = torch::empty({rows}, invden.options());
  if (rows > 0) {
    const BuildLaunch L(rows, K, BUILD_WAVES);
    LDA_DISPATCH_S(S_, hipLaunchKernelGGL(
        alias_build_packed_kernel<S>, L.grid, L.blk, L.shmem,
        current_stream(),
        src.data_ptr<int>(), rows_p, invden.data_ptr<float>(), (float)beta,
        rec.data_ptr<int>(), reinterpret_cast<int2*>(top.data_ptr<int>()),
        qsum.data_ptr<float>(), rows));
  }
  return {invden, qsum};
}

torch::Tensor lda_mh_wave_packed(torch::Tensor doc_topic,
                                 torch::Tensor word_topic, torch::Tensor rec,
                                 torch::Tensor top, torch::Tensor invden,
                                 torch::Tensor doc_offsets,
                                 torch::Tensor word_ids,
                                 torch::Tensor assignments,
                                 double alpha, double beta, int64_t seed,
                                 c10::optional<torch::Tensor> shard,
                                 c10::optional<torch::Tensor> row_of_local,
                                 int64_t summary_row) {
  CHECK_IN(doc_topic); CHECK_IN(word_topic); CHECK_IN(invden); CHECK_IN(doc_offsets);
  CHECK_IN(word_ids); CHECK_IN(assignments);
  const int S_ = packed_S(rec, top);
  const int D = doc_topic.size(0), K = doc_topic.size(1);
  TORCH_CHECK(K == S_ * WAVE, "doc_topic width does not match rec");
  TORCH_CHECK(doc_topic.dtype() == torch::kInt32 &&
              assignments.dtype() == torch::kInt32 &&
              word_ids.dtype() == torch::kInt32 &&
              doc_offsets.dtype() == torch::kInt64 &&
              invden.dtype() == torch::kFloat32 && invden.numel() == K);
  TORCH_CHECK(doc_offsets.numel() == D + 1 &&
              word_ids.numel() == assignments.numel());
  const bool fused = shard.has_value();
  int* shard_p = nullptr; const int* rol_p = nullptr;
  if (fused) {
    TORCH_CHECK(row_of_local.has_value(), "fused apply needs row_of_local");
    CHECK_IN(*shard); CHECK_IN(*row_of_local);
    TORCH_CHECK(shard->dtype() == torch::kInt32 && shard->dim() == 2 &&
                shard->size(1) == K);
    TORCH_CHECK(row_of_local->dtype() == torch::kInt32 &&
                row_of_local->numel() == rec.size(0));
    TORCH_CHECK(summary_row >= 0 && summary_row < shard->size(0));
    shard_p = shard->data_ptr<int>();
    rol_p = row_of_local->data_ptr<int>();
  }
  TORCH_CHECK(word_topic.dtype() == torch::kInt32 &&
              word_topic.dim() == 2 && word_topic.size(1) == K &&
              word_topic.size(0) >= rec.size(0),
              "word_topic must be [>= rec rows][K] int32");
  if (D == 0) return assignments;
  const int waves_wg = 4;              // 256 threads, 4 docs per block
  dim3 blk(WAVE * waves_wg), grid((D + waves_wg - 1) / waves_wg);
  const size_t shmem = ((size_t)waves_wg + (fused ? 1 : 0)) * K * 4;
#define LDA_LAUNCH_PACKED(F)                                              \
  hipLaunchKernelGGL((lda_mh_wave_kernel<PackedTables<S>, F>), grid, blk, \
                     shmem, current_stream(), doc_topic.data_ptr<int>(),  \
                     word_topic.data_ptr<int>(), invden.data_ptr<float>(),\
                     PackedTables<S>{rec.data_ptr<int>(),                 \
                         reinterpret_cast<const int2*>(top.data_ptr<int>())},\
                     doc_offsets.data_ptr<int64_t>(),                     \
                     word_ids.data_ptr<int>(),                            \
                     assignments.data_ptr<int>(), shard_p, rol_p,         \
                     summary_row, (float)alpha, (float)beta, D,           \
                     (unsigned int)(seed & 0xffffffff))
  LDA_DISPATCH_S(S_, if (fused) LDA_LAUNCH_PACKED(true);
                     else LDA_LAUNCH_PACKED(false));
#undef LDA_LAUNCH_PACKED
  return assignments;
}
