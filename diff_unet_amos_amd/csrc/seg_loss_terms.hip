// The fused segmentation loss with the terms beyond mse / bce / dice: "ce", "dice_ce" and "generalized_dice" of
// losses/loss.py:40-54, forward and backward, for any subset of the six gradient-carrying names (plus the multi_neighbor
// partials of csrc/multi_neighbor.hip in the tail).  The contract -- the formulas, the label assumptions (none: one-hot,
// all-zero and soft voxels alike, nothing assumes sum_c y_c = 1), the buffers -- is in include/dua_hip.h at
// dua_seg_loss_terms_*; csrc/seg_loss.hip keeps the three-term kernels as they are and is what a name set within
// mse / bce / dice / multi_neighbor still runs.
//
//   reduce : one pass over logits and labels.  A thread owns a voxel and walks its row in groups of eight channels (one 16-byte
//            read per group on the fp16 path, labels coalesced per channel): per channel s = sigmoid(p) feeds I = sum s y,
//            S = sum s, Y = sum y and the squared-error and BCE sums; across the groups a running maximum m and
//            l = sum exp(p - m) (rescaled by exp(m_old - m) when the maximum moves) give lse = m + log l after ONE read of the
//            row, and the voxel adds Y_v lse - sum_c y_c p_c to the cross-entropy sum.  exp only ever sees p - m <= 0: a
//            logit of +-200 neither overflows nor cancels.  The 3 C per-channel accumulators are registers: the kernel is
//            instantiated per number of channel groups NG (1, 2, 3, 4, 8), so every index is a compile-time constant
//            (C = 16: 48 accumulators; C = 64: 192, one wave per SIMD -- still a streaming pass, and not the shipped shape).
//            Each workgroup WRITES its fp64 partials; a second small kernel adds them in workgroup order.  No floating-point
//            atomics: the same inputs give the same bits (the rule of csrc/augment_intensity.hip).
//   finish : the scalar tail.  Terms, combine, dcomb as seg_loss_finish_kernel; the generalized-Dice weights (once, here) and
//            per (n, c) the two fp32 constants of the gradient's Dice-shaped part, formed in fp64 and rounded once.
//   grad   : one pass.  The row (logits and labels) is held in registers, so softmax needs no second read;
//            dp = g [ mse' + bce' + (k0 y + k1) s (1 - s) + ce' ], each part behind a branch on its use flag.
// Streaming passes and a one-wave tail: no LDS tiling, no MFMA, no host read (graph-capturable).
#include "common.hpp"
#include "../../include/dua_hip.h"

namespace dua {

constexpr int LT_MAXC = 64;              // = LOSS_MAXC of seg_loss.hip
constexpr int LT_REDUCE_BLOCKS = 512;    // workgroups per sample of the reduce pass (at most): the scratch rows per sample
constexpr int LT_GRAD_BLOCKS = 4096;

__host__ __device__ inline int lt_width(int C) { return 3 * C + 3; }     // (I, S, Y) per channel, then mse, bce, ce
inline long lt_reduce_blocks(long V) {
  const long b = (V + 255) / 256;
  return b > LT_REDUCE_BLOCKS ? LT_REDUCE_BLOCKS : b;
}

// A group's channels past C ("dead", only where C % 8 != 0) are computed like the others, on a logit of LT_DEAD and a label of 0,
// so that the eight channels of a group are straight-line code the scheduler can interleave (a branch per channel made every
// sigmoid / softplus chain wait for the one before it).  Such a channel adds exact zeros: s = 1 / (1 + inf) = 0, s y = 0, d = 0,
// max(p, 0) - p * 0 + log1p(0) = 0, e^(p - m) = 0, and max(m, p) = m for every logit a network can produce.  Its accumulators
// are never stored, its gradient never written.
constexpr float LT_DEAD = -1e30f;

// eight channels of a row from c0 on: one 16-byte read (vec: fp16, all eight inside C, row 16-byte aligned) or scalar reads of
// the nch >= 1 live ones (the dead ones re-read the last live address: no read outside the C channels)
template <typename T>
__device__ __forceinline__ void lt_load8(const T* __restrict__ row, bool vec, int nch, float out[8]) {
  if constexpr (sizeof(T) == 2) {
    if (vec) {
      const f16x8 v = *(const f16x8*)row;
#pragma unroll
      for (int e = 0; e < 8; ++e) out[e] = (float)v[e];
      return;
    }
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float x = (float)row[e < nch ? e : nch - 1];
    out[e] = e < nch ? x : LT_DEAD;
  }
}

// the eight labels of voxel v from channel c0 on (col = y + (n C + c0) V + v), coalesced per channel; dead ones are 0
__device__ __forceinline__ void lt_labels8(const float* __restrict__ col, long V, int nch, float out[8]) {
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float t = col[(long)(e < nch ? e : nch - 1) * V];
    out[e] = e < nch ? t : 0.f;
  }
}

__device__ __forceinline__ float lt_wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ double lt_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ double lt_wave_max(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
  return v;
}

// partials: fp64 [N][gridDim.x][3 C + 3], WRITTEN
template <typename T, int NG>
__global__ __launch_bounds__(256) void seg_loss_terms_reduce_kernel(const T* __restrict__ p, int p_stride,
                                                                    const float* __restrict__ y, int C, long V,
                                                                    double* __restrict__ partials, int vec) {
  __shared__ float red[4][3 * LT_MAXC + 3];
  const int n = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float I[NG][8], S[NG][8], Y[NG][8];
#pragma unroll
  for (int g = 0; g < NG; ++g)
#pragma unroll
    for (int e = 0; e < 8; ++e) { I[g][e] = 0.f; S[g][e] = 0.f; Y[g][e] = 0.f; }
  float mse = 0.f, bce = 0.f, ce = 0.f;
  for (long v = blockIdx.x * 256L + threadIdx.x; v < V; v += (long)gridDim.x * 256) {
    const T* pr = p + ((long)n * V + v) * p_stride;
    const float* yr = y + (long)n * C * V + v;
    float m = -INFINITY, l = 0.f, Yv = 0.f, dot = 0.f;
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      const int c0 = 8 * g;
      if (c0 < C) {                                        // uniform
        const int nch = min(8, C - c0);
        float pv[8], yv[8];
        lt_load8(pr + c0, vec != 0, nch, pv);
        lt_labels8(yr + (long)c0 * V, V, nch, yv);
        float gm = m;
#pragma unroll
        for (int e = 0; e < 8; ++e) gm = fmaxf(gm, pv[e]);
        l *= __expf(m - gm);                               // first group: m = -inf, exp -> 0, l = 0 stays 0
        m = gm;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float s = 1.f / (1.f + __expf(-pv[e]));
          I[g][e] += s * yv[e]; S[g][e] += s; Y[g][e] += yv[e];
          const float d = s - yv[e];
          mse += d * d;
          bce += fmaxf(pv[e], 0.f) - pv[e] * yv[e] + log1pf(__expf(-fabsf(pv[e])));
          l += __expf(pv[e] - m);
          Yv += yv[e];
          dot += pv[e] * yv[e];
        }
      }
    }
    ce += Yv * (m + logf(l)) - dot;
  }
#pragma unroll
  for (int g = 0; g < NG; ++g) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int c = 8 * g + e;
      if (c < C) {                                         // uniform
        const float a = lt_wave_sum(I[g][e]), b = lt_wave_sum(S[g][e]), cc = lt_wave_sum(Y[g][e]);
        if (lane == 0) { red[wave][3 * c] = a; red[wave][3 * c + 1] = b; red[wave][3 * c + 2] = cc; }
      }
    }
  }
  mse = lt_wave_sum(mse); bce = lt_wave_sum(bce); ce = lt_wave_sum(ce);
  if (lane == 0) { red[wave][3 * LT_MAXC] = mse; red[wave][3 * LT_MAXC + 1] = bce; red[wave][3 * LT_MAXC + 2] = ce; }
  __syncthreads();
  const int W = lt_width(C);
  double* out = partials + ((long)n * gridDim.x + blockIdx.x) * W;
  for (int i = threadIdx.x; i < W; i += 256) {
    const int j = i < 3 * C ? i : 3 * LT_MAXC + (i - 3 * C);
    out[i] = (((double)red[0][j] + (double)red[1][j]) + (double)red[2][j]) + (double)red[3][j];
  }
}

// sums (fp64 [N C 4 + 3], WRITTEN): block (i, n), one wave: lane j adds the partials of workgroups j, j + 64, .. in that order,
// then the xor tree -- a fixed order.  The three whole-batch sums (i >= 3 C) are formed by the blocks of n = 0 over all samples.
__global__ __launch_bounds__(64) void seg_loss_terms_sum_kernel(const double* __restrict__ partials, int G, int N, int C,
                                                                double* __restrict__ sums) {
  const int i = blockIdx.x, n = blockIdx.y, W = lt_width(C);
  const bool whole = i >= 3 * C;
  if (whole && n != 0) return;
  const double* q = partials + (whole ? 0L : (long)n * G * W) + i;
  const long rows = whole ? (long)N * G : G;
  double acc = 0.0;
  for (long r = threadIdx.x; r < rows; r += 64) acc += q[r * W];
  acc = lt_wave_sum(acc);
  if (threadIdx.x != 0) return;
  if (whole) { sums[(long)N * C * 4 + (i - 3 * C)] = acc; return; }
  double* o = sums + ((long)n * C + i / 3) * 4;
  o[i % 3] = acc;
  if (i % 3 == 2) o[3] = 0.0;
}

// One wave; lane c owns channel c.  consts: fp32 [N][C][2] = (k0, k1) of the gradient's (k0 y + k1) s (1 - s):
//   Dice, counted nd = use_dice + use_dice_ce times:   k0 = -2 nd / (De N C),  k1 = nd Ie / (De^2 N C)
//   generalized Dice:                                  k0 += -2 w / (B N),     k1 += A w / (B^2 N)
// each sum formed in fp64 and rounded once.
__global__ __launch_bounds__(64) void seg_loss_terms_finish_kernel(int N, int C, double V, int use_mse, int use_bce, int use_dice,
                                                                   int use_ce, int use_dice_ce, int use_gdice, int combine,
                                                                   const double* __restrict__ sums, float* loss, float* dcomb,
                                                                   float* __restrict__ consts, const double* __restrict__ mn,
                                                                   int mn_K) {
  const int c = threadIdx.x;
  const bool on = c < C;
  const int nd = use_dice + use_dice_ce, nce = use_ce + use_dice_ce;
  const double e = 1e-5, NC = (double)N * (double)C;
  double dice = 0.0, gd = 0.0;
  for (int n = 0; n < N; ++n) {
    // sums may be NULL when only the multi_neighbor term is asked for: the per-(n, c) sums are read for a Dice-shaped name only
    double I = 0.0, S = 0.0, Y = 0.0;
    if (on && (nd || use_gdice)) {
      const double* q = sums + ((long)n * C + c) * 4;
      I = q[0]; S = q[1]; Y = q[2];
    }
    double k0 = 0.0, k1 = 0.0;
    if (nd) {
      const double De = S + Y + e, Ie = 2.0 * I + e;
      if (on) dice += 1.0 - Ie / De;
      k0 = -2.0 * nd / (De * NC);
      k1 = nd * Ie / (De * De * NC);
    }
    if (use_gdice) {
      double w = on ? 1.0 / (Y * Y) : 0.0;
      const bool inf = isinf(w);
      if (inf) w = 0.0;
      const double wmax = lt_wave_max(w);                // weights are >= 0; lanes past C hold 0
      if (inf) w = wmax;
      const double A = 2.0 * lt_wave_sum(w * I) + e, B = lt_wave_sum(w * (S + Y)) + e;
      gd += 1.0 - A / B;                                 // the same on every lane
      k0 += -2.0 * w / (B * (double)N);
      k1 += A * w / (B * B * (double)N);
    }
    if (on && (nd || use_gdice)) {
      consts[((long)n * C + c) * 2] = (float)k0;
      consts[((long)n * C + c) * 2 + 1] = (float)k1;
    }
  }
  dice = lt_wave_sum(dice);
  if (threadIdx.x != 0) return;
  double total = 0.0;
  int count = 0;
  if (use_mse) { total += sums[4L * N * C] / (NC * V); ++count; }
  if (use_bce) { total += sums[4L * N * C + 1] / (NC * V); ++count; }
  if (nd) { total += nd * (dice / NC); count += use_dice; }
  if (nce) { total += nce * (sums[4L * N * C + 2] / ((double)N * V)); count += use_ce; }
  count += use_dice_ce;                                  // dice_ce is ONE term: its two parts are in total already
  if (use_gdice) { total += gd / (double)N; ++count; }
  if (mn) {
    double sq = 0.0, entries = 0.0;
    for (int n = 0; n < N; ++n) {
      const double* r = mn + (long)n * (mn_K + 1);
      for (int a = 0; a < mn_K; ++a) sq += r[a];
      entries += r[mn_K];
    }
    total += sq / entries;
    ++count;
  }
  double L = total, dc = 1.0;
  if (count > 1 && combine == 1) { L = total / count; dc = 1.0 / count; }
  else if (count > 1 && combine == 2) { L = log(1.0 + total); dc = 1.0 / (1.0 + total); }
  loss[0] = (float)L;
  dcomb[0] = (float)dc;
}

// The voxel loop of the gradient kernel.  WITH_B: the boundary term's part rides in the same pass, gb * phi * s (1 - s) * a_bnd
// (phi fp32 [N][C][V] like the labels), added in fp32 to gs * [named terms] before the ONE rounding to T.
template <typename T, int NG, bool WITH_B>
__device__ __forceinline__ void lt_grad_rows(const T* __restrict__ p, int p_stride, const float* __restrict__ y, int C, long V,
                                             int n, const float* k0, const float* k1, float gs, float a_mse, float a_bce,
                                             float a_ce, int use_mse, int use_bce, int use_k, int use_ce, T* __restrict__ dp,
                                             int dp_stride, int vec_in, int vec_out, const float* __restrict__ phi, float gb,
                                             float a_bnd) {
  for (long v = blockIdx.x * 256L + threadIdx.x; v < V; v += (long)gridDim.x * 256) {
    const T* pr = p + ((long)n * V + v) * p_stride;
    const float* yr = y + (long)n * C * V + v;
    T* dr = dp + ((long)n * V + v) * dp_stride;
    float pv[NG][8], yv[NG][8];
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      const int c0 = 8 * g, nch = min(8, C - c0);
      if (c0 < C) {
        lt_load8(pr + c0, vec_in != 0, nch, pv[g]);
        lt_labels8(yr + (long)c0 * V, V, nch, yv[g]);
      }
    }
    float m = -INFINITY, rl = 0.f;
    if (use_ce) {                                          // uniform
      float l = 0.f, Yv = 0.f;
#pragma unroll
      for (int g = 0; g < NG; ++g)
        if (8 * g < C) {
#pragma unroll
          for (int e = 0; e < 8; ++e) m = fmaxf(m, pv[g][e]);
        }
#pragma unroll
      for (int g = 0; g < NG; ++g)
        if (8 * g < C) {
#pragma unroll
          for (int e = 0; e < 8; ++e) { l += __expf(pv[g][e] - m); Yv += yv[g][e]; }
        }
      rl = Yv / l;
    }
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      const int c0 = 8 * g;
      if (c0 < C) {
        float o[8];
        [[maybe_unused]] float fv[8];
        if constexpr (WITH_B) lt_labels8(phi + ((long)n * C + c0) * V + v, V, min(8, C - c0), fv);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float x = pv[g][e], t = yv[g][e];
          const float s = 1.f / (1.f + __expf(-x));
          const float ds = s * (1.f - s), d = s - t;
          float acc = 0.f;
          if (use_mse) acc += a_mse * d * ds;
          if (use_bce) acc += a_bce * d;
          if (use_k) acc += (k0[c0 + e] * t + k1[c0 + e]) * ds;          // k0, k1 hold LT_MAXC entries, 0 past C
          if (use_ce) acc += a_ce * (rl * __expf(x - m) - t);
          o[e] = gs * acc;
          if constexpr (WITH_B) o[e] += gb * (fv[e] * ds * a_bnd);
        }
        if constexpr (sizeof(T) == 2) {
          if (vec_out) {
            f16x8 w;
#pragma unroll
            for (int e = 0; e < 8; ++e) w[e] = (f16)o[e];
            *(f16x8*)(dr + c0) = w;
            continue;
          }
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) if (c0 + e < C) dr[c0 + e] = (T)o[e];
      }
    }
  }
}

// BND: the form dua_seg_loss_terms_boundary_grad launches, gb = *bscale.  gb == 0 (a schedule that starts at alpha = 0) runs the
// loop without the term and does not read phi: there the compiler may round gs * acc straight to fp16 (v_fma_mixlo_f16, which it
// does for one element of eight), and alpha = 0 must give the bits of the step without a boundary weight.  BND = false is the
// kernel as it was.
template <typename T, int NG, bool BND = false>
__global__ __launch_bounds__(256) void seg_loss_terms_grad_kernel(const T* __restrict__ p, int p_stride,
                                                                  const float* __restrict__ y, int C, long V,
                                                                  const float* __restrict__ consts,
                                                                  const float* __restrict__ gscale, float a_mse, float a_bce,
                                                                  float a_ce, int use_mse, int use_bce, int use_k, int use_ce,
                                                                  T* __restrict__ dp, int dp_stride, int vec_in, int vec_out,
                                                                  const float* __restrict__ phi = nullptr,
                                                                  const float* __restrict__ bscale = nullptr, float a_bnd = 0.f) {
  __shared__ float k0[LT_MAXC], k1[LT_MAXC];
  const int n = blockIdx.y;
  const float gs = gscale ? *gscale : 1.f;
  if (threadIdx.x < LT_MAXC) {
    const bool have = use_k && threadIdx.x < C;
    k0[threadIdx.x] = have ? consts[((long)n * C + threadIdx.x) * 2] : 0.f;
    k1[threadIdx.x] = have ? consts[((long)n * C + threadIdx.x) * 2 + 1] : 0.f;
  }
  __syncthreads();
  if constexpr (BND) {
    const float gb = *bscale;
    if (gb != 0.f) {                                       // uniform
      lt_grad_rows<T, NG, true>(p, p_stride, y, C, V, n, k0, k1, gs, a_mse, a_bce, a_ce, use_mse, use_bce, use_k, use_ce, dp,
                                dp_stride, vec_in, vec_out, phi, gb, a_bnd);
      return;
    }
  }
  lt_grad_rows<T, NG, false>(p, p_stride, y, C, V, n, k0, k1, gs, a_mse, a_bce, a_ce, use_mse, use_bce, use_k, use_ce, dp,
                             dp_stride, vec_in, vec_out, nullptr, 0.f, 0.f);
}

// The boundary term's sum, sum_{c,v} sigmoid(p) phi, as a pass of its own (the named reduce above keeps its code): a thread owns
// a voxel and walks its row like the reduce does, adds s * phi in fp32, and the workgroup WRITES one fp64 partial.
// partials: fp64 [N][gridDim.x].
template <typename T>
__global__ __launch_bounds__(256) void seg_loss_boundary_reduce_kernel(const T* __restrict__ p, int p_stride,
                                                                       const float* __restrict__ phi, int C, long V,
                                                                       double* __restrict__ partials, int vec) {
  __shared__ float red[4];
  const int n = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float acc = 0.f;
  for (long v = blockIdx.x * 256L + threadIdx.x; v < V; v += (long)gridDim.x * 256) {
    const T* pr = p + ((long)n * V + v) * p_stride;
    const float* fr = phi + (long)n * C * V + v;
    for (int c0 = 0; c0 < C; c0 += 8) {
      const int nch = min(8, C - c0);
      float pv[8], fv[8];
      lt_load8(pr + c0, vec != 0, nch, pv);
      lt_labels8(fr + (long)c0 * V, V, nch, fv);
#pragma unroll
      for (int e = 0; e < 8; ++e) acc += (1.f / (1.f + __expf(-pv[e]))) * fv[e];
    }
  }
  acc = lt_wave_sum(acc);
  if (lane == 0) red[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0)
    partials[(long)n * gridDim.x + blockIdx.x] = (((double)red[0] + (double)red[1]) + (double)red[2]) + (double)red[3];
}

// One wave: lane j adds the partials j, j + 64, .. in that order, then the xor tree -- a fixed order.  B = sum / (N C V);
// bterm[0] = B and loss[0] (holding L_named, as dua_seg_loss_terms_finish left it) becomes L_named + alpha B, formed in fp64
// and rounded once.  alpha = 0 leaves loss[0] as it is, whatever B is.
__global__ __launch_bounds__(64) void seg_loss_boundary_finish_kernel(const double* __restrict__ partials, long rows, double M,
                                                                      const float* __restrict__ alpha, float* loss,
                                                                      float* __restrict__ bterm) {
  double acc = 0.0;
  for (long r = threadIdx.x; r < rows; r += 64) acc += partials[r];
  acc = lt_wave_sum(acc);
  if (threadIdx.x != 0) return;
  const double B = acc / M;
  const float a = alpha[0];
  bterm[0] = (float)B;
  if (a != 0.f) loss[0] = (float)((double)loss[0] + (double)a * B);      // 0 * (an inf or NaN B) would turn L_named into NaN
}

inline bool lt_dims_ok(int N, int C, long voxels) {
  return N > 0 && N <= 65535 && C > 0 && C <= LT_MAXC && voxels > 0;
}

}  // namespace dua

extern "C" {

long dua_seg_loss_terms_scratch_bytes(int N, int C, long voxels) {
  if (!dua::lt_dims_ok(N, C, voxels)) return DUA_ERR_ARG;
  return (long)N * dua::lt_reduce_blocks(voxels) * dua::lt_width(C) * (long)sizeof(double);
}

#define LT_BY_GROUPS(LAUNCH, T)              \
  do {                                       \
    if (C <= 8) LAUNCH(T, 1);                \
    else if (C <= 16) LAUNCH(T, 2);          \
    else if (C <= 24) LAUNCH(T, 3);          \
    else if (C <= 32) LAUNCH(T, 4);          \
    else LAUNCH(T, 8);                       \
  } while (0)

int dua_seg_loss_terms_reduce(int dtype, int N, int C, long voxels, const void* logits, int logits_stride, const float* labels,
                              double* sums, void* scratch, long scratch_bytes, void* stream) {
  if (!logits || !labels || !sums || !scratch || !dua::lt_dims_ok(N, C, voxels) || logits_stride < C ||
      (dtype != DUA_F16 && dtype != DUA_F32) || scratch_bytes < dua_seg_loss_terms_scratch_bytes(N, C, voxels))
    return DUA_ERR_ARG;
  const int G = (int)dua::lt_reduce_blocks(voxels);
  const dim3 grid(G, N);
  const int vec = dtype == DUA_F16 && C % 8 == 0 && logits_stride % 8 == 0 && ((size_t)logits & 15) == 0;
  hipStream_t s = (hipStream_t)stream;
#define LT_REDUCE(T, NG)                                                                                                   \
  hipLaunchKernelGGL((dua::seg_loss_terms_reduce_kernel<T, NG>), grid, dim3(256), 0, s, (const T*)logits, logits_stride, labels, \
                     C, voxels, (double*)scratch, vec)
  if (dtype == DUA_F16) LT_BY_GROUPS(LT_REDUCE, dua::f16); else LT_BY_GROUPS(LT_REDUCE, float);
#undef LT_REDUCE
  hipLaunchKernelGGL(dua::seg_loss_terms_sum_kernel, dim3(dua::lt_width(C), N), dim3(64), 0, s, (const double*)scratch, G, N, C,
                     sums);
  return (int)hipGetLastError();
}

int dua_seg_loss_terms_finish(int N, int C, long voxels, int use_mse, int use_bce, int use_dice, int use_ce, int use_dice_ce,
                              int use_gdice, int K, const double* mn_partials, int combine, const double* sums, float* loss,
                              float* dcomb, float* consts, void* stream) {
  const int flags[6] = {use_mse, use_bce, use_dice, use_ce, use_dice_ce, use_gdice};
  int any = 0;
  for (int f : flags) {
    if (f != 0 && f != 1) return DUA_ERR_ARG;
    any |= f;
  }
  if (!dua::lt_dims_ok(N, C, voxels) || !loss || !dcomb || combine < 0 || combine > 2 || (!any && !mn_partials) ||
      (any && !sums) || ((use_dice || use_dice_ce || use_gdice) && !consts) || (mn_partials && (K <= 0 || K > dua::LT_MAXC)))
    return DUA_ERR_ARG;
  hipLaunchKernelGGL(dua::seg_loss_terms_finish_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, N, C, (double)voxels, use_mse,
                     use_bce, use_dice, use_ce, use_dice_ce, use_gdice, combine, sums, loss, dcomb, consts, mn_partials, K);
  return (int)hipGetLastError();
}

}  // extern "C"

// dua_seg_loss_terms_grad (phi == NULL: a term must be selected) and dua_seg_loss_terms_boundary_grad (phi, bscale: the named part may
// be empty)
static int lt_grad_launch(int dtype, int N, int C, long voxels, const void* logits, int logits_stride, const float* labels,
                          const float* consts, const float* gscale, int use_mse, int use_bce, int use_dice, int use_ce,
                          int use_dice_ce, int use_gdice, const float* phi, const float* bscale, void* dlogits,
                          int dlogits_stride, void* stream) {
  const int flags[6] = {use_mse, use_bce, use_dice, use_ce, use_dice_ce, use_gdice};
  int any = 0;
  for (int f : flags) {
    if (f != 0 && f != 1) return DUA_ERR_ARG;
    any |= f;
  }
  const int use_k = use_dice || use_dice_ce || use_gdice, nce = use_ce + use_dice_ce;
  if (!logits || !labels || !dlogits || !dua::lt_dims_ok(N, C, voxels) || logits_stride < C || dlogits_stride < C ||
      (!any && !phi) || (use_k && !consts) || (dtype != DUA_F16 && dtype != DUA_F32))
    return DUA_ERR_ARG;
  const double M = (double)N * (double)C * (double)voxels;
  const float a_mse = (float)(2.0 / M), a_bce = (float)(1.0 / M), a_ce = (float)((double)nce / ((double)N * (double)voxels));
  const float a_bnd = (float)(1.0 / M);
  long b = (voxels + 255) / 256;
  const dim3 grid((unsigned)(b > dua::LT_GRAD_BLOCKS ? dua::LT_GRAD_BLOCKS : b), N);
  const int f16v = dtype == DUA_F16 && C % 8 == 0;
  const int vec_in = f16v && logits_stride % 8 == 0 && ((size_t)logits & 15) == 0;
  const int vec_out = f16v && dlogits_stride % 8 == 0 && ((size_t)dlogits & 15) == 0;
  hipStream_t s = (hipStream_t)stream;
#define LT_GRAD(T, NG)                                                                                                          \
  do {                                                                                                                          \
    if (phi)                                                                                                                    \
      hipLaunchKernelGGL((dua::seg_loss_terms_grad_kernel<T, NG, true>), grid, dim3(256), 0, s, (const T*)logits, logits_stride, \
                         labels, C, voxels, consts, gscale, a_mse, a_bce, a_ce, use_mse, use_bce, use_k, nce != 0, (T*)dlogits, \
                         dlogits_stride, vec_in, vec_out, phi, bscale, a_bnd);                                                  \
    else                                                                                                                        \
      hipLaunchKernelGGL((dua::seg_loss_terms_grad_kernel<T, NG>), grid, dim3(256), 0, s, (const T*)logits, logits_stride,      \
                         labels, C, voxels, consts, gscale, a_mse, a_bce, a_ce, use_mse, use_bce, use_k, nce != 0, (T*)dlogits, \
                         dlogits_stride, vec_in, vec_out, (const float*)nullptr, (const float*)nullptr, 0.f);                   \
  } while (0)
  if (dtype == DUA_F16) LT_BY_GROUPS(LT_GRAD, dua::f16); else LT_BY_GROUPS(LT_GRAD, float);
#undef LT_GRAD
  return (int)hipGetLastError();
}

extern "C" {

int dua_seg_loss_terms_grad(int dtype, int N, int C, long voxels, const void* logits, int logits_stride, const float* labels,
                            const float* consts, const float* gscale, int use_mse, int use_bce, int use_dice, int use_ce,
                            int use_dice_ce, int use_gdice, void* dlogits, int dlogits_stride, void* stream) {
  return lt_grad_launch(dtype, N, C, voxels, logits, logits_stride, labels, consts, gscale, use_mse, use_bce, use_dice, use_ce,
                        use_dice_ce, use_gdice, nullptr, nullptr, dlogits, dlogits_stride, stream);
}

long dua_seg_loss_boundary_scratch_bytes(int N, int C, long voxels) {
  if (!dua::lt_dims_ok(N, C, voxels)) return DUA_ERR_ARG;
  return (long)N * dua::lt_reduce_blocks(voxels) * (long)sizeof(double);
}

int dua_seg_loss_boundary_reduce(int dtype, int N, int C, long voxels, const void* logits, int logits_stride, const float* phi,
                                 const float* alpha, float* loss, float* bterm, void* scratch, long scratch_bytes,
                                 void* stream) {
  if (!logits || !phi || !alpha || !loss || !bterm || !scratch || !dua::lt_dims_ok(N, C, voxels) || logits_stride < C ||
      (dtype != DUA_F16 && dtype != DUA_F32) || scratch_bytes < dua_seg_loss_boundary_scratch_bytes(N, C, voxels))
    return DUA_ERR_ARG;
  const int G = (int)dua::lt_reduce_blocks(voxels);
  const int vec = dtype == DUA_F16 && C % 8 == 0 && logits_stride % 8 == 0 && ((size_t)logits & 15) == 0;
  hipStream_t s = (hipStream_t)stream;
  if (dtype == DUA_F16)
    hipLaunchKernelGGL(dua::seg_loss_boundary_reduce_kernel<dua::f16>, dim3(G, N), dim3(256), 0, s, (const dua::f16*)logits,
                       logits_stride, phi, C, voxels, (double*)scratch, vec);
  else
    hipLaunchKernelGGL(dua::seg_loss_boundary_reduce_kernel<float>, dim3(G, N), dim3(256), 0, s, (const float*)logits,
                       logits_stride, phi, C, voxels, (double*)scratch, vec);
  hipLaunchKernelGGL(dua::seg_loss_boundary_finish_kernel, dim3(1), dim3(64), 0, s, (const double*)scratch, (long)N * G,
                     (double)N * (double)C * (double)voxels, alpha, loss, bterm);
  return (int)hipGetLastError();
}

int dua_seg_loss_terms_boundary_grad(int dtype, int N, int C, long voxels, const void* logits, int logits_stride,
                                     const float* labels, const float* consts, const float* gscale, int use_mse, int use_bce,
                                     int use_dice, int use_ce, int use_dice_ce, int use_gdice, const float* phi,
                                     const float* bscale, void* dlogits, int dlogits_stride, void* stream) {
  if (!phi || !bscale) return DUA_ERR_ARG;
  return lt_grad_launch(dtype, N, C, voxels, logits, logits_stride, labels, consts, gscale, use_mse, use_bce, use_dice, use_ce,
                        use_dice_ce, use_gdice, phi, bscale, dlogits, dlogits_stride, stream);
}

#undef LT_BY_GROUPS

}  // extern "C"
