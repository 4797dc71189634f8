// K1+K2: NMF gradient over a sparse batch.
// Reference hot loop NMFTrainer.java:328-367 (per nonzero (i,j,v):
// e = L_i.R_j - v; lGrad += 2e R_j + L2; rGrad_j += 2e L_i + L2) and the
// per-thread gradient-map merge :375-406.
//
// CDNA4 design: one WAVE per L-row (CSR). The row's L vector lives in
// registers (rank <= 256 -> <=4 f32 per lane), its lGrad accumulates in
// registers across all of the row's nonzeros and is written once —
// no atomics on the L side (this replaces the reference's per-thread
// hashmap merge). rGrad contributions scatter with atomicAdd: distinct rows
// rarely collide on a column within a cycle, and f32 atomicAdd on HBM/L2 is
// cheap on gfx950. The rank-dot is a 64-lane butterfly reduction.

#include "hip_common.h"
#include <cstdlib>

namespace {

constexpr int MAXC = 4;  // supports rank <= 4*64 = 256

__global__ void nmf_grad_kernel(const float* __restrict__ L,
                                const float* __restrict__ R,
                                const int64_t* __restrict__ row_ptr,
                                const int64_t* __restrict__ col_idx,
                                const float* __restrict__ vals,
                                float* __restrict__ lgrad,
                                float* __restrict__ rgrad,
                                float* __restrict__ sqerr,
                                int n_rows, int k, float lam2) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int row = (blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
  if (row >= n_rows) return;
  const int nchunk = (k + WAVE - 1) / WAVE;

  float l[MAXC], lg[MAXC];
#pragma unroll
  for (int c = 0; c < MAXC; ++c) {
    int idx = c * WAVE + lane;
    l[c] = (c < nchunk && idx < k) ? L[(int64_t)row * k + idx] : 0.f;
    lg[c] = 0.f;
  }

  float sq = 0.f;
  const int64_t p0 = row_ptr[row], p1 = row_ptr[row + 1];
  for (int64_t p = p0; p < p1; ++p) {
    const int64_t j = col_idx[p];
    float r[MAXC];
    float part = 0.f;
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
      int idx = c * WAVE + lane;
      r[c] = (c < nchunk && idx < k) ? R[j * k + idx] : 0.f;
      part += l[c] * r[c];
    }
    const float e = wave_reduce_sum(part) - vals[p];
    const float ge = 2.f * e;
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
      int idx = c * WAVE + lane;
      if (c < nchunk && idx < k) {
        lg[c] += ge * r[c] + lam2 * l[c];
        atomicAdd(&rgrad[j * k + idx], ge * l[c] + lam2 * r[c]);
      }
    }
    sq += (lane == 0) ? e * e : 0.f;
  }

#pragma unroll
  for (int c = 0; c < MAXC; ++c) {
    int idx = c * WAVE + lane;
    if (c < nchunk && idx < k) lgrad[(int64_t)row * k + idx] = lg[c];
  }
  if (lane == 0 && sq != 0.f) atomicAdd(sqerr, sq);
}

// Two-pass variant (no atomics): the batch's nonzeros are ALSO indexed by a
// static column-sorted permutation (precomputed once per data block, like
// the reference's per-feature pre-sort in GBT). Pass A (row-major) computes
// e[p] + lgrad with L/lgrad in registers; pass B walks each column's
// segment, accumulates rgrad_j in registers and writes it once. This
// replaces the reference's per-thread gradient hashmap + merge
// (NMFTrainer.aggregateGradient:375-406) with a segmented reduction and
// removes 200M+ HBM/L2 atomics per batch.

template <int G>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
  for (int m = G / 2; m > 0; m >>= 1) v += __shfl_xor(v, m, G);
  return v;
}

template <int G>
__global__ void nmf_grad_e_kernel(const float* __restrict__ L,
                                  const float* __restrict__ R,
                                  const int64_t* __restrict__ row_ptr,
                                  const int64_t* __restrict__ col_idx,
                                  const float* __restrict__ vals,
                                  float* __restrict__ lgrad,
                                  float* __restrict__ e_out,
                                  float* __restrict__ sqerr,
                                  int n_rows, int k, float lam2) {
  const int lane = threadIdx.x & (G - 1);
  const int row = (blockIdx.x * blockDim.x + threadIdx.x) / G;
  if (row >= n_rows) return;
  const int nchunk = (k + G - 1) / G;
  float l[MAXC], lg[MAXC];
#pragma unroll
  for (int c = 0; c < MAXC; ++c) {
    int idx = c * G + lane;
    l[c] = (c < nchunk && idx < k) ? L[(int64_t)row * k + idx] : 0.f;
    lg[c] = 0.f;
  }
  float sq = 0.f;
  const int64_t p0 = row_ptr[row], p1 = row_ptr[row + 1];
  // software-pipelined 2-deep: issue the NEXT nonzero's R-row loads before
  // the current dot's butterfly reduce — the serial per-nonzero chain
  // (load R_j -> dot -> reduce) is latency-bound otherwise
  float r[MAXC], rn[MAXC];
  if (p0 < p1) {
    const int64_t j0 = col_idx[p0];
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
      int idx = c * G + lane;
      r[c] = (c < nchunk && idx < k) ? R[j0 * k + idx] : 0.f;
    }
  }
  for (int64_t p = p0; p < p1; ++p) {
    if (p + 1 < p1) {
      const int64_t jn = col_idx[p + 1];
#pragma unroll
      for (int c = 0; c < MAXC; ++c) {
        int idx = c * G + lane;
        rn[c] = (c < nchunk && idx < k) ? R[jn * k + idx] : 0.f;
      }
    }
    float part = 0.f;
#pragma unroll
    for (int c = 0; c < MAXC; ++c) part += l[c] * r[c];
    const float e = group_sum<G>(part) - vals[p];
    const float ge = 2.f * e;
#pragma unroll
    for (int c = 0; c < MAXC; ++c) lg[c] += ge * r[c] + lam2 * l[c];
    if (lane == 0) e_out[p] = e;
    sq += (lane == 0) ? e * e : 0.f;
#pragma unroll
    for (int c = 0; c < MAXC; ++c) r[c] = rn[c];
  }
#pragma unroll
  for (int c = 0; c < MAXC; ++c) {
    int idx = c * G + lane;
    if (c < nchunk && idx < k) lgrad[(int64_t)row * k + idx] = lg[c];
  }
  if (lane == 0 && sq != 0.f) atomicAdd(sqerr, sq);
}

template <int G>
__global__ void nmf_rgrad_kernel(const float* __restrict__ L,
                                 const float* __restrict__ R,
                                 const float* __restrict__ e_in,
                                 const int64_t* __restrict__ perm,
                                 const int64_t* __restrict__ seg_ptr,
                                 const int64_t* __restrict__ row_sorted,
                                 float* __restrict__ rgrad,
                                 int n_cols, int k, float lam2) {
  const int lane = threadIdx.x & (G - 1);
  const int col = (blockIdx.x * blockDim.x + threadIdx.x) / G;
  if (col >= n_cols) return;
  const int nchunk = (k + G - 1) / G;
  float acc[MAXC];
#pragma unroll
  for (int c = 0; c < MAXC; ++c) acc[c] = 0.f;
  const int64_t p0 = seg_ptr[col], p1 = seg_ptr[col + 1];
  // 2-deep pipeline over the segment's (e, L-row) loads
  float lv[MAXC], lvn[MAXC];
  float ge = 0.f, gen = 0.f;
  if (p0 < p1) {
    ge = 2.f * e_in[perm[p0]];
    const int64_t i0 = row_sorted[p0];
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
      int idx = c * G + lane;
      lv[c] = (c < nchunk && idx < k) ? L[i0 * k + idx] : 0.f;
    }
  }
  for (int64_t p = p0; p < p1; ++p) {
    if (p + 1 < p1) {
      gen = 2.f * e_in[perm[p + 1]];
      const int64_t in_ = row_sorted[p + 1];
#pragma unroll
      for (int c = 0; c < MAXC; ++c) {
        int idx = c * G + lane;
        lvn[c] = (c < nchunk && idx < k) ? L[in_ * k + idx] : 0.f;
      }
    }
#pragma unroll
    for (int c = 0; c < MAXC; ++c) acc[c] += ge * lv[c];
#pragma unroll
    for (int c = 0; c < MAXC; ++c) lv[c] = lvn[c];
    ge = gen;
  }
  // L2 term: lam2 * (#nonzeros in this column) * R_j
  const float nl = lam2 * (float)(p1 - p0);
#pragma unroll
  for (int c = 0; c < MAXC; ++c) {
    int idx = c * G + lane;
    if (c < nchunk && idx < k)
      rgrad[(int64_t)col * k + idx] = acc[c] + nl * R[(int64_t)col * k + idx];
  }
}

}  // namespace

std::vector<torch::Tensor> nmf_grad_twopass(
    torch::Tensor L, torch::Tensor R, torch::Tensor row_ptr,
    torch::Tensor col_idx, torch::Tensor vals, torch::Tensor perm,
    torch::Tensor seg_ptr, torch::Tensor row_sorted, double lam) {
  CHECK_IN(L); CHECK_IN(R); CHECK_IN(row_ptr); CHECK_IN(col_idx);
  CHECK_IN(vals); CHECK_IN(perm); CHECK_IN(seg_ptr); CHECK_IN(row_sorted);
  const int n = L.size(0), k = L.size(1), m = R.size(0);
  TORCH_CHECK(k <= 64 * MAXC);
  TORCH_CHECK(seg_ptr.numel() == m + 1, "seg_ptr must cover all R rows");
  auto lgrad = torch::empty_like(L);
  auto rgrad = torch::empty_like(R);
  auto e = torch::empty_like(vals);
  auto sqerr = torch::zeros({}, L.options());
  // lane-group width: 32 (2 rows/wave) when the rank fits 32*MAXC —
  // same co-scheduling reasoning as the LDA sampler; HARMONY_NMF_G overrides
  int G = (k <= 32 * MAXC) ? 32 : 64;
  const char* env = getenv("HARMONY_NMF_G");
  if (env && atoi(env) == 64) G = 64;
  if (env && atoi(env) == 32 && k <= 32 * MAXC) G = 32;
  int threads = 256;   // HARMONY_NMF_THREADS: occupancy A/B knob
  const char* te = getenv("HARMONY_NMF_THREADS");
  if (te) { int t = atoi(te); if (t == 128 || t == 256 || t == 512 || t == 1024) threads = t; }
  if (n > 0) {
    dim3 grid((n + threads / G - 1) / (threads / G));
    if (G == 32)
      hipLaunchKernelGGL(nmf_grad_e_kernel<32>, grid, dim3(threads), 0,
                         current_stream(),
                         L.data_ptr<float>(), R.data_ptr<float>(),
                         row_ptr.data_ptr<int64_t>(),
                         col_idx.data_ptr<int64_t>(),
                         vals.data_ptr<float>(), lgrad.data_ptr<float>(),
                         e.data_ptr<float>(), sqerr.data_ptr<float>(),
                         n, k, 2.f * (float)lam);
    else
      hipLaunchKernelGGL(nmf_grad_e_kernel<64>, grid, dim3(threads), 0,
                         current_stream(),
                         L.data_ptr<float>(), R.data_ptr<float>(),
                         row_ptr.data_ptr<int64_t>(),
                         col_idx.data_ptr<int64_t>(),
                         vals.data_ptr<float>(), lgrad.data_ptr<float>(),
                         e.data_ptr<float>(), sqerr.data_ptr<float>(),
                         n, k, 2.f * (float)lam);
  }
  if (m > 0) {
    dim3 grid((m + threads / G - 1) / (threads / G));
    if (G == 32)
      hipLaunchKernelGGL(nmf_rgrad_kernel<32>, grid, dim3(threads), 0,
                         current_stream(),
                         L.data_ptr<float>(), R.data_ptr<float>(),
                         e.data_ptr<float>(), perm.data_ptr<int64_t>(),
                         seg_ptr.data_ptr<int64_t>(),
                         row_sorted.data_ptr<int64_t>(),
                         rgrad.data_ptr<float>(), m, k, 2.f * (float)lam);
    else
      hipLaunchKernelGGL(nmf_rgrad_kernel<64>, grid, dim3(threads), 0,
                         current_stream(),
                         L.data_ptr<float>(), R.data_ptr<float>(),
                         e.data_ptr<float>(), perm.data_ptr<int64_t>(),
                         seg_ptr.data_ptr<int64_t>(),
                         row_sorted.data_ptr<int64_t>(),
                         rgrad.data_ptr<float>(), m, k, 2.f * (float)lam);
  }
  return {lgrad, rgrad, sqerr};
}

std::vector<torch::Tensor> nmf_grad(torch::Tensor L, torch::Tensor R,
                                    torch::Tensor row_ptr,
                                    torch::Tensor col_idx, torch::Tensor vals,
                                    double lam) {
  CHECK_IN(L); CHECK_IN(R); CHECK_IN(row_ptr); CHECK_IN(col_idx); CHECK_IN(vals);
  TORCH_CHECK(L.dtype() == torch::kFloat32 && R.dtype() == torch::kFloat32);
  TORCH_CHECK(L.size(1) == R.size(1), "rank mismatch");
  TORCH_CHECK(L.size(1) <= 64 * MAXC, "rank > ", 64 * MAXC, " unsupported");
  const int n = L.size(0), k = L.size(1);
  TORCH_CHECK(row_ptr.numel() == n + 1, "row_ptr size");
  auto lgrad = torch::empty_like(L);
  auto rgrad = torch::zeros_like(R);
  auto sqerr = torch::zeros({}, L.options());
  if (n > 0) {
    const int waves_per_block = 4;                 // 256 threads
    dim3 blk(WAVE * waves_per_block);
    dim3 grid((n + waves_per_block - 1) / waves_per_block);
    hipLaunchKernelGGL(nmf_grad_kernel, grid, blk, 0, current_stream(),
                       L.data_ptr<float>(), R.data_ptr<float>(),
                       row_ptr.data_ptr<int64_t>(), col_idx.data_ptr<int64_t>(),
                       vals.data_ptr<float>(), lgrad.data_ptr<float>(),
                       rgrad.data_ptr<float>(), sqerr.data_ptr<float>(),
                       n, k, 2.f * (float)lam);
  }
  return {lgrad, rgrad, sqerr};
}

// ---------------------------------------------------------------------------
// nmf_step: pipelined two-pass gradient with the local L update fused in.
//
// Same split as nmf_grad_twopass (pass A per L row -> e, lgrad; pass B per
// unique column -> rgrad), rebuilt around what bounds it: random 4*k-byte row
// gathers served from the Infinity Cache. Each lane group
//   * fetches a row as one 16-byte load per lane (scalar path: 4 dwords);
//   * loads indices / vals lane-parallel (one coalesced load per G entries)
//     and broadcasts the per-nonzero value with a shuffle;
//   * keeps a ring of D rows in flight: prologue fills it, the steady loop
//     consumes slot s and refills it with row i+D in straight-line code (no
//     branch between loads, so the compiler's counted waits leave the rest
//     of the ring outstanding), the epilogue drains it under guards;
//   * pass A reduces U dots at a time so the butterfly chains overlap, and
//     stores e with one coalesced store per G nonzeros.
// Pass A also writes L_new = clamp(L - step*lgrad, 0, max_val) (mul then
// sub, uncontracted: the torch chain's roundings) to a scratch tensor —
// pass B still reads the old L. Indices are int32. R rows are addressed
// through the caller's index (col -> row of R_src), so R_src may be a
// gathered [n_uniq, k] tensor or a whole table.
// ---------------------------------------------------------------------------

namespace {

struct Row4 { float v[4]; };

// VEC: lane owns columns 4*lane..4*lane+3 (one 16-byte access).
// scalar: lane owns columns c*G+lane, c = 0..3 (four 4-byte accesses).
// Elements past k are read from column 0 of the same row (a valid address)
// and never stored; callers zero their multiplier.
template <int G, bool VEC>
struct RowIO {
  int off[4];
  bool ok[4];
  __device__ __forceinline__ RowIO(int lane, int k) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int idx = VEC ? 4 * lane + c : c * G + lane;
      ok[c] = idx < k;
      off[c] = ok[c] ? idx : (VEC ? c : 0);
    }
  }
  __device__ __forceinline__ Row4 load(const float* __restrict__ p) const {
    Row4 r;
    if (VEC) {
      const float4 t = *reinterpret_cast<const float4*>(p + off[0]);
      r.v[0] = t.x; r.v[1] = t.y; r.v[2] = t.z; r.v[3] = t.w;
    } else {
#pragma unroll
      for (int c = 0; c < 4; ++c) r.v[c] = p[off[c]];
    }
    return r;
  }
  __device__ __forceinline__ void store(float* __restrict__ p,
                                        const Row4& r) const {
    if (VEC) {
      if (ok[0])
        *reinterpret_cast<float4*>(p + off[0]) =
            make_float4(r.v[0], r.v[1], r.v[2], r.v[3]);
    } else {
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (ok[c]) p[off[c]] = r.v[c];
    }
  }
};

// a - s*g with the product rounded before the subtraction, as the torch
// chain L - step*lgrad rounds it (the default contraction would fuse them)
__device__ __forceinline__ float mul_then_sub(float a, float s, float g) {
#pragma clang fp contract(off)
  const float p = s * g;
  return a - p;
}

// Entry i (0 <= i < 4*G) of a lane-parallel 4-register index chunk:
// register c, lane t holds entry c*G + t. i is uniform over the group, so
// the register choice costs scalar branches, no vector work.
template <int G, typename T>
__device__ __forceinline__ T chunk_get(const T (&reg)[4], int i) {
  const int c = i / G;
  const T sel = c == 0 ? reg[0] : c == 1 ? reg[1] : c == 2 ? reg[2] : reg[3];
  return __shfl(sel, i & (G - 1), G);
}

template <int G, int D, int U, bool VEC>
__global__ void __launch_bounds__(256)
nmf_step_a_kernel(const float* __restrict__ L,      // batch rows [n, k]
                  const float* __restrict__ Rsrc,
                  const int* __restrict__ row_ptr,
                  const int* __restrict__ col,      // row of Rsrc per nonzero
                  const float* __restrict__ vals,
                  const float* __restrict__ step_p,
                  float* __restrict__ e_out,
                  float* __restrict__ L_new,
                  float* __restrict__ lgrad,        // may be null
                  float* __restrict__ sqerr,
                  int n_rows, int k, float lam2, float max_val) {
  static_assert(D % U == 0 && D <= G, "ring shape");
  constexpr int SC = 4 * G;   // nonzeros per index chunk
  const int lane = threadIdx.x & (G - 1);
  const int row = (blockIdx.x * blockDim.x + threadIdx.x) / G;
  if (row >= n_rows) return;
  const RowIO<G, VEC> io(lane, k);
  const Row4 lraw = io.load(L + (size_t)row * k);
  Row4 l, lg;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    l.v[c] = io.ok[c] ? lraw.v[c] : 0.f;
    lg.v[c] = 0.f;
  }
  float sq = 0.f;
  const int p0 = row_ptr[row], p1 = row_ptr[row + 1];

  for (int base = p0; base < p1; base += SC) {
    const int cnt = min(SC, p1 - base);
    int colv[4];
    float valv[4], ev[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int q = c * G + lane;
      const bool in = q < cnt;
      colv[c] = col[base + (in ? q : 0)];
      valv[c] = vals[base + (in ? q : 0)];
      ev[c] = 0.f;
    }
    Row4 ring[D];
    // prologue: unconditional, index clamped to the chunk's last entry
#pragma unroll
    for (int d = 0; d < D; ++d) {
      const int j = chunk_get<G>(colv, min(d, cnt - 1));
      ring[d] = io.load(Rsrc + (size_t)j * k);
    }

    // consume slots s..s+U-1 holding nonzeros i..i+U-1 of this chunk
    auto consume = [&](const int s, const int i, const bool guarded) {
      float part[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const Row4& r = ring[s + u];
        part[u] = l.v[0] * r.v[0] + l.v[1] * r.v[1] + l.v[2] * r.v[2] +
                  l.v[3] * r.v[3];
      }
#pragma unroll
      for (int m = G / 2; m > 0; m >>= 1)
#pragma unroll
        for (int u = 0; u < U; ++u) part[u] += __shfl_xor(part[u], m, G);
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int q = i + u;
        const bool valid = !guarded || q < cnt;
        const int qc = valid ? q : 0;
        const float e = part[u] - chunk_get<G>(valv, qc);
        const float ge = 2.f * e;
        const Row4& r = ring[s + u];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const float t = lg.v[c] + (ge * r.v[c] + lam2 * l.v[c]);
          lg.v[c] = valid ? t : lg.v[c];
        }
        sq = valid ? sq + e * e : sq;
        const bool mine = valid && (qc & (G - 1)) == lane;
        const int cc = qc / G;
#pragma unroll
        for (int c = 0; c < 4; ++c) ev[c] = (mine && cc == c) ? e : ev[c];
      }
    };

    int i = 0;
    // steady state: every refill is in range, loads are unconditional
    for (; i + 2 * D <= cnt; i += D) {
#pragma unroll
      for (int s = 0; s < D; s += U) {
        consume(s, i + s, false);
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int j = chunk_get<G>(colv, i + s + u + D);
          ring[s + u] = io.load(Rsrc + (size_t)j * k);
        }
      }
    }
    // epilogue: fewer than 2*D nonzeros left, the ring holds i..i+D-1
#pragma unroll
    for (int s = 0; s < D; s += U) {
      if (i + s < cnt) consume(s, i + s, true);
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int q = i + s + u + D;
        if (q < cnt) {
          const int j = chunk_get<G>(colv, q);
          ring[s + u] = io.load(Rsrc + (size_t)j * k);
        }
      }
    }
    i += D;
#pragma unroll
    for (int s = 0; s < D; s += U)
      if (i + s < cnt) consume(s, i + s, true);

#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int q = c * G + lane;
      if (q < cnt) e_out[base + q] = ev[c];
    }
  }

  const float step = *step_p;
  Row4 ln;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    ln.v[c] = fminf(fmaxf(mul_then_sub(lraw.v[c], step, lg.v[c]), 0.f),
                    max_val);
  }
  io.store(L_new + (size_t)row * k, ln);
  if (lgrad) io.store(lgrad + (size_t)row * k, lg);
  if (lane == 0 && sq != 0.f) atomicAdd(sqerr, sq);
}

template <int G, int D, bool VEC>
__global__ void __launch_bounds__(256)
nmf_step_b_kernel(const float* __restrict__ L,      // batch rows [n, k]
                  const float* __restrict__ Rsrc,
                  const float* __restrict__ e_in,
                  const int* __restrict__ perm,
                  const int* __restrict__ seg_ptr,
                  const int* __restrict__ row_sorted,
                  const int* __restrict__ rsrc_of,  // null: identity
                  float* __restrict__ rgrad,
                  int n_cols, int k, float lam2) {
  static_assert(D <= G, "ring shape");
  const int lane = threadIdx.x & (G - 1);
  const int colid = (blockIdx.x * blockDim.x + threadIdx.x) / G;
  if (colid >= n_cols) return;
  const RowIO<G, VEC> io(lane, k);
  Row4 acc;
#pragma unroll
  for (int c = 0; c < 4; ++c) acc.v[c] = 0.f;
  const int p0 = seg_ptr[colid], p1 = seg_ptr[colid + 1];

  for (int base = p0; base < p1; base += G) {
    const int cnt = min(G, p1 - base);
    const int q = lane < cnt ? lane : 0;
    const int rowv = row_sorted[base + q];
    const float gev = 2.f * e_in[perm[base + q]];   // G independent loads
    Row4 ring[D];
#pragma unroll
    for (int d = 0; d < D; ++d) {
      const int r = __shfl(rowv, min(d, cnt - 1), G);
      ring[d] = io.load(L + (size_t)r * k);
    }
    // same per-column order and arithmetic as nmf_rgrad_kernel
    auto consume = [&](const int s, const int i, const bool guarded) {
      const bool valid = !guarded || i < cnt;
      const float ge = __shfl(gev, valid ? i : 0, G);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const float t = acc.v[c] + ge * ring[s].v[c];
        acc.v[c] = valid ? t : acc.v[c];
      }
    };
    int i = 0;
    for (; i + 2 * D <= cnt; i += D) {
#pragma unroll
      for (int s = 0; s < D; ++s) {
        consume(s, i + s, false);
        const int r = __shfl(rowv, i + s + D, G);
        ring[s] = io.load(L + (size_t)r * k);
      }
    }
#pragma unroll
    for (int s = 0; s < D; ++s) {
      consume(s, i + s, true);
      if (i + s + D < cnt) {
        const int r = __shfl(rowv, i + s + D, G);
        ring[s] = io.load(L + (size_t)r * k);
      }
    }
    i += D;
#pragma unroll
    for (int s = 0; s < D; ++s) consume(s, i + s, true);
  }

  // L2 term: lam2 * (#nonzeros in this column) * R_j
  const float nl = lam2 * (float)(p1 - p0);
  const int rs = rsrc_of ? rsrc_of[colid] : colid;
  const Row4 rr = io.load(Rsrc + (size_t)rs * k);
  Row4 out;
#pragma unroll
  for (int c = 0; c < 4; ++c) out.v[c] = acc.v[c] + nl * rr.v[c];
  io.store(rgrad + (size_t)colid * k, out);
}

inline bool aligned16(const void* p) {
  return (reinterpret_cast<uintptr_t>(p) & 15) == 0;
}

template <int G, int D, int U, bool VEC>
void launch_nmf_step(const float* L, const float* Rsrc, const int* row_ptr,
                     const int* col, const float* vals, const float* step,
                     const int* perm, const int* seg_ptr,
                     const int* row_sorted, const int* rsrc_of, float* e,
                     float* L_new, float* lgrad, float* rgrad, float* sqerr,
                     int n, int m, int k, float lam2, float max_val) {
  constexpr int threads = 256, per = threads / G;
  if (n > 0)
    hipLaunchKernelGGL((nmf_step_a_kernel<G, D, U, VEC>),
                       dim3((n + per - 1) / per), dim3(threads), 0,
                       current_stream(), L, Rsrc, row_ptr, col, vals, step,
                       e, L_new, lgrad, sqerr, n, k, lam2, max_val);
  if (m > 0)
    hipLaunchKernelGGL((nmf_step_b_kernel<G, D, VEC>),
                       dim3((m + per - 1) / per), dim3(threads), 0,
                       current_stream(), L, Rsrc, e, perm, seg_ptr,
                       row_sorted, rsrc_of, rgrad, m, k, lam2);
}

}  // namespace

// L: [NL, k], the batch is rows l_lo..l_lo+n. col indexes rows of R_src;
// seg_ptr has one segment per rgrad row (n_uniq); rsrc_of maps an rgrad row
// to its R_src row (undefined tensor: identity). step: 0-dim device float.
// Returns {L_new [n,k], rgrad [n_uniq,k], sq_err[, lgrad [n,k]]}.
std::vector<torch::Tensor> nmf_step(
    torch::Tensor L, int64_t l_lo, int64_t n, torch::Tensor R_src,
    torch::Tensor row_ptr, torch::Tensor col, torch::Tensor vals,
    torch::Tensor perm, torch::Tensor seg_ptr, torch::Tensor row_sorted,
    c10::optional<torch::Tensor> rsrc_of, torch::Tensor step, double lam,
    double max_val, bool want_lgrad) {
  CHECK_IN(L); CHECK_IN(R_src); CHECK_IN(row_ptr); CHECK_IN(col);
  CHECK_IN(vals); CHECK_IN(perm); CHECK_IN(seg_ptr); CHECK_IN(row_sorted);
  CHECK_IN(step);
  TORCH_CHECK(L.dtype() == torch::kFloat32 && R_src.dtype() == torch::kFloat32
              && vals.dtype() == torch::kFloat32
              && step.dtype() == torch::kFloat32 && step.numel() == 1);
  for (const auto& t : {row_ptr, col, perm, seg_ptr, row_sorted})
    TORCH_CHECK(t.dtype() == torch::kInt32, "nmf_step takes int32 indices");
  const int k = L.size(1);
  TORCH_CHECK(R_src.size(1) == k, "rank mismatch");
  TORCH_CHECK(k >= 1 && k <= 64 * MAXC, "rank > ", 64 * MAXC, " unsupported");
  TORCH_CHECK(l_lo >= 0 && n >= 0 && l_lo + n <= L.size(0), "L range");
  TORCH_CHECK(row_ptr.numel() == n + 1, "row_ptr size");
  const int64_t nnz = col.numel();
  TORCH_CHECK(vals.numel() == nnz && perm.numel() == nnz &&
              row_sorted.numel() == nnz, "nnz mismatch");
  TORCH_CHECK(nnz < (int64_t{1} << 31), "nmf_step: nnz must fit int32");
  const int m = seg_ptr.numel() - 1;
  TORCH_CHECK(m >= 0, "seg_ptr size");
  const int* rsrc_p = nullptr;
  if (rsrc_of.has_value()) {
    CHECK_IN(*rsrc_of);
    TORCH_CHECK(rsrc_of->dtype() == torch::kInt32 && rsrc_of->numel() == m,
                "rsrc_of: one int32 per rgrad row");
    rsrc_p = rsrc_of->data_ptr<int>();
  } else {
    TORCH_CHECK(R_src.size(0) >= m, "R_src rows < seg_ptr segments");
  }
  auto L_new = torch::empty({n, k}, L.options());
  auto rgrad = torch::empty({m, k}, L.options());
  auto e = torch::empty({nnz}, L.options());
  auto sqerr = torch::zeros({}, L.options());
  torch::Tensor lgrad;
  if (want_lgrad) lgrad = torch::empty({n, k}, L.options());
  const float* Lp = L.data_ptr<float>() + l_lo * k;
  const float* Rp = R_src.data_ptr<float>();
  const bool vec = k % 4 == 0 && aligned16(Lp) && aligned16(Rp);
  const bool wide = k > 4 * 32;   // four floats per lane: G=32 holds 128
#define NMF_STEP_LAUNCH(G, D, U, VEC)                                        \
  launch_nmf_step<G, D, U, VEC>(                                             \
      Lp, Rp, row_ptr.data_ptr<int>(), col.data_ptr<int>(),                  \
      vals.data_ptr<float>(), step.data_ptr<float>(), perm.data_ptr<int>(),  \
      seg_ptr.data_ptr<int>(), row_sorted.data_ptr<int>(), rsrc_p,           \
      e.data_ptr<float>(), L_new.data_ptr<float>(),                          \
      want_lgrad ? lgrad.data_ptr<float>() : nullptr,                        \
      rgrad.data_ptr<float>(), sqerr.data_ptr<float>(), (int)n, m, k,        \
      2.f * (float)lam, (float)max_val)
  // ring depth 4 with dots reduced in pairs: measured best of D = 2, 4, 8 on
  // MI355X at the bench shape (profiles/r03_nmf_step.md)
  if (vec && !wide) NMF_STEP_LAUNCH(32, 4, 2, true);
  else if (vec) NMF_STEP_LAUNCH(64, 4, 2, true);
  else if (!wide) NMF_STEP_LAUNCH(32, 4, 2, false);
  else NMF_STEP_LAUNCH(64, 4, 2, false);
#undef NMF_STEP_LAUNCH
  if (want_lgrad) return {L_new, rgrad, sqerr, lgrad};
  return {L_new, rgrad, sqerr};
}
