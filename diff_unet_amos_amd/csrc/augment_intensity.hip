// Intensity augmentation of a training batch on the device: Gaussian noise, Gaussian blur, multiplicative brightness, contrast
// and gamma (with and without inversion), the intensity half of nnU-Net's default recipe, as a stage after the batch producer's
// apply.  The contract (which random word decides what, the row layout, the order of the fp32 operations, how the statistics
// are taken) is written down in include/dua_hip.h ("training input: intensity augmentation"); this file only says how it is
// computed.
//
//   draw        : ONE workgroup, one wave per sample, the counter protocol of dua_aug_draw (augment.hip): every wave reads the
//                 call counter, a workgroup barrier, one lane moves it on.  Three Philox blocks per sample, tagged 0x40000000 + j.
//   noise, blur : one pass, images -> scratch.  A workgroup owns an 8 x 8 x 16 tile of the output and stages the tile plus a halo
//                 of 4 voxels (16 x 16 x 24) in LDS; the noise of a halo voxel is regenerated from its counter, not exchanged
//                 (a Philox block and one Box-Muller pair per 4 voxels), and the boundary is reflected when the tile is loaded, so
//                 the three separable passes (w, h, d) read LDS without a bounds test.  40 KB of static LDS: 864 workgroups per
//                 96^3 sample, 3 - 4 per CU.  Out of place, because a tile reads voxels its neighbours write.
//   pointwise   : four passes over the patch, separated by the statistics the next one needs.  Each pass writes one 32-byte
//                 partial (sum, sum of squares, minimum, maximum; fp64) per workgroup; the next pass reduces the partials of its
//                 sample in a fixed order in every workgroup (a wave takes them 64 apart, then a butterfly), so no atomic is
//                 involved and the bits do not depend on the order of arrival.
//                   brightness : source (scratch after noise / blur, else images) -> out, x *= f; statistics of the result
//                   contrast   : in place; statistics of the result for gamma
//                   gamma 1    : in place, y = t^gamma (hi - lo) + lo; mean and deviation of y
//                   gamma 2    : in place, the rescaling to the mean and deviation gamma 1 started from
//                 A sample without the event of a pass leaves that pass with its first instruction after the row is read.
// -ffp-contract=off (csrc/Makefile) keeps every fp32 operation of the contract separately rounded; the pragma below says so for
// this file whatever the command line.
#include "common.hpp"
#include "philox.hpp"
#include "../../include/dua_hip.h"

#pragma clang fp contract(off)

namespace dua {

constexpr int AI_THREADS = 256;
constexpr int AI_DRAW_WAVES = 16;
constexpr int AI_MAX_PARTS = 256;                         // workgroups (and partials) per sample of a pointwise pass
constexpr int AI_HALO = 4;                                // DUA_AUG_INTENSITY_MAX_RADIUS
constexpr int AI_TD = 8, AI_TH = 8, AI_TW = 16;           // the output tile of a workgroup
constexpr int AI_LD = AI_TD + 2 * AI_HALO, AI_LH = AI_TH + 2 * AI_HALO, AI_LW = AI_TW + 2 * AI_HALO;
constexpr uint32_t AI_DRAW_TAG = 0x40000000u, AI_NOISE_TAG = 0x80000000u;
static_assert(AI_TD * AI_TH * AI_TW == 4 * AI_THREADS, "a lane stores 4 voxels of the tile");
static_assert(AI_HALO == DUA_AUG_INTENSITY_MAX_RADIUS && AI_LW % 4 == 0 && AI_TW % 4 == 0, "16-byte rows in the staged tile");
static_assert((AI_LD * AI_LH * AI_LW + AI_LD * AI_LH * AI_TW) * 4 <= 64 * 1024, "static LDS: nothing for dua_prepare to raise");

struct AiStats { double sum, sq, mn, mx; };               // one partial, or the reduced statistics of a sample
static_assert(sizeof(AiStats) == 32, "a partial is 32 bytes");

__device__ __forceinline__ float ai_unit(uint32_t x) { return (float)(x >> 8) * 5.9604644775390625e-8f; }       // 2^-24: exact
__device__ __forceinline__ float ai_between(float lo, float span, uint32_t x) {
  const float t = span * ai_unit(x);
  return t + lo;
}

__global__ void __launch_bounds__(AI_DRAW_WAVES * 64) aug_intensity_draw_kernel(dua_aug_intensity_config cfg, int B,
                                                                                unsigned long long seed,
                                                                                unsigned long long* counter, int use_counter,
                                                                                unsigned long long counter_value,
                                                                                float* __restrict__ rows) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long call = use_counter ? counter_value : *counter;
  __syncthreads();                                        // every wave holds the call counter before one lane moves it on
  if (!use_counter && threadIdx.x == 0) *counter = call + 1;
  if (lane != 0) return;                                  // the decisions of a sample are one lane's arithmetic
  for (int b = wave; b < B; b += AI_DRAW_WAVES) {
    uint32_t w[3][4];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      w[j][0] = (uint32_t)call; w[j][1] = (uint32_t)(call >> 32); w[j][2] = (uint32_t)b; w[j][3] = AI_DRAW_TAG + (uint32_t)j;
      philox4x32_10(w[j], (uint32_t)seed, (uint32_t)(seed >> 32));
    }
    int mask = 0;
    float std = 0.f, sigma = 0.f, bright = 1.f, contrast = 1.f, gamma = 1.f;
    if (ai_unit(w[0][0]) < cfg.noise_prob) { mask |= DUA_AUG_INTENSITY_NOISE; std = ai_between(cfg.noise_std_min, cfg.noise_std_span, w[0][1]); }
    if (ai_unit(w[0][2]) < cfg.blur_prob) { mask |= DUA_AUG_INTENSITY_BLUR; sigma = ai_between(cfg.blur_sigma_min, cfg.blur_sigma_span, w[0][3]); }
    if (ai_unit(w[1][0]) < cfg.brightness_prob) { mask |= DUA_AUG_INTENSITY_BRIGHTNESS; bright = ai_between(cfg.brightness_min, cfg.brightness_span, w[1][1]); }
    if (ai_unit(w[1][2]) < cfg.contrast_prob) { mask |= DUA_AUG_INTENSITY_CONTRAST; contrast = ai_between(cfg.contrast_min, cfg.contrast_span, w[1][3]); }
    if (ai_unit(w[2][0]) < cfg.gamma_prob) {
      mask |= DUA_AUG_INTENSITY_GAMMA;
      const bool below = ai_unit(w[2][1]) < 0.5f && cfg.gamma_min < 1.f;
      gamma = below ? ai_between(cfg.gamma_min, cfg.gamma_span_below, w[2][2])
                    : ai_between(fmaxf(cfg.gamma_min, 1.f), cfg.gamma_span_above, w[2][2]);
      if (ai_unit(w[2][3]) < cfg.gamma_invert_prob) mask |= DUA_AUG_INTENSITY_INVERT;
    }
    float* row = rows + (long)b * DUA_AUG_INTENSITY_WORDS;
    row[DUA_AUG_INTENSITY_EVENTS] = __int_as_float(mask);
    row[DUA_AUG_INTENSITY_STD] = std;
    row[DUA_AUG_INTENSITY_SIGMA] = sigma;
    row[DUA_AUG_INTENSITY_BRIGHT] = bright;
    row[DUA_AUG_INTENSITY_CONTRAST_F] = contrast;
    row[DUA_AUG_INTENSITY_GAMMA_V] = gamma;
    row[DUA_AUG_INTENSITY_CALL_LO] = __int_as_float((int)(uint32_t)call);
    row[DUA_AUG_INTENSITY_CALL_HI] = __int_as_float((int)(uint32_t)(call >> 32));
    row[DUA_AUG_INTENSITY_SAMPLE] = __int_as_float(b);
#pragma unroll
    for (int j = DUA_AUG_INTENSITY_SAMPLE + 1; j < DUA_AUG_INTENSITY_WORDS; ++j) row[j] = 0.f;
  }
}

__device__ __forceinline__ int ai_events(const float* __restrict__ row) { return __float_as_int(row[DUA_AUG_INTENSITY_EVENTS]); }

// scipy's mode="reflect" for one step over either end (extents are at least the radius), then clamped: an index further out
// only feeds outputs that lie outside the patch and are never stored, and must still be an address inside it
__device__ __forceinline__ int ai_reflect(int i, int n) {
  i = i < 0 ? -1 - i : i;
  i = i >= n ? 2 * n - 1 - i : i;
  return min(max(i, 0), n - 1);
}

// the four normals of noise block q (voxels 4q .. 4q + 3 of sample `sample` in call `call`)
__device__ __forceinline__ void ai_normals(uint32_t call_lo, uint32_t call_hi, uint32_t sample, uint32_t q, uint32_t k0, uint32_t k1,
                                           float z[4]) {
  uint32_t c[4] = {call_lo, call_hi, sample, AI_NOISE_TAG + q};
  philox4x32_10(c, k0, k1);
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const float u1 = (float)((c[2 * p] >> 8) + 1u) * 5.9604644775390625e-8f;         // (0, 1]
    const float u2 = (float)(c[2 * p + 1] >> 8) * 5.9604644775390625e-8f;            // [0, 1)
    const float r = sqrtf(-2.f * logf(u1));
    float sn, cs;
    sincosf(6.28318530717958647692f * u2, &sn, &cs);
    z[2 * p] = r * cs;
    z[2 * p + 1] = r * sn;
  }
}

// V = 4: roi_w is a multiple of 4 and every pointer 16-byte aligned, so a group of 4 voxels along w never crosses a row, is one
// noise block, and reflects onto one whole group (reversed); V = 1: voxel by voxel.
template <int V>
__global__ void __launch_bounds__(AI_THREADS) aug_intensity_noise_blur_kernel(const float* __restrict__ images,
                                                                             const float* __restrict__ rows, int Rd, int Rh, int Rw,
                                                                             unsigned long long seed, float* __restrict__ tmp) {
  __shared__ __attribute__((aligned(16))) float A[AI_LD * AI_LH * AI_LW];      // the staged tile; after the w pass, the h pass's output
  __shared__ __attribute__((aligned(16))) float Bs[AI_LD * AI_LH * AI_TW];     // the w pass's output
  const int b = blockIdx.y, tid = threadIdx.x;
  const float* row = rows + (long)b * DUA_AUG_INTENSITY_WORDS;
  const int mask = ai_events(row);
  if (!(mask & (DUA_AUG_INTENSITY_NOISE | DUA_AUG_INTENSITY_BLUR))) return;
  const bool noisy = (mask & DUA_AUG_INTENSITY_NOISE) != 0;
  const float std = row[DUA_AUG_INTENSITY_STD];
  const uint32_t call_lo = (uint32_t)__float_as_int(row[DUA_AUG_INTENSITY_CALL_LO]);
  const uint32_t call_hi = (uint32_t)__float_as_int(row[DUA_AUG_INTENSITY_CALL_HI]);
  const uint32_t sample = (uint32_t)__float_as_int(row[DUA_AUG_INTENSITY_SAMPLE]);
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  int R = 0;
  float t0 = 1.f, t1 = 0.f, t2 = 0.f, t3 = 0.f, t4 = 0.f;
  if (mask & DUA_AUG_INTENSITY_BLUR) {
    const float sigma = row[DUA_AUG_INTENSITY_SIGMA];
    R = (int)fminf(fmaxf(floorf(4.f * sigma + 0.5f), 0.f), (float)AI_HALO);       // a NaN becomes 0
    if (R > 0) {                                          // taps in fp64 from the fp32 sigma, each rounded to fp32 once
      const double s2 = 2.0 * (double)sigma * (double)sigma;
      double e[AI_HALO + 1], sum = 1.0;
#pragma unroll
      for (int i = 1; i <= AI_HALO; ++i) {
        e[i] = i <= R ? exp(-(double)(i * i) / s2) : 0.0;
        sum += 2.0 * e[i];
      }
      t0 = (float)(1.0 / sum); t1 = (float)(e[1] / sum); t2 = (float)(e[2] / sum); t3 = (float)(e[3] / sum); t4 = (float)(e[4] / sum);
    }
  }
  const int tiles_w = (Rw + AI_TW - 1) / AI_TW, tiles_h = (Rh + AI_TH - 1) / AI_TH;
  const int tw = blockIdx.x % tiles_w, trow = blockIdx.x / tiles_w, th = trow % tiles_h, td = trow / tiles_h;
  const int d0 = td * AI_TD, h0 = th * AI_TH, w0 = tw * AI_TW;
  const long vox = (long)Rd * Rh * Rw;
  const float* src = images + (long)b * vox;
  const int lo_l = AI_HALO - R, hi_d = AI_HALO + AI_TD + R, hi_h = AI_HALO + AI_TH + R;      // staged planes / rows the passes read

  // stage the tile: reflected at the patch boundary, noise added where it is read
  if constexpr (V == 4) {
    constexpr int GW = AI_LW / 4;
    for (int g = tid; g < AI_LD * AI_LH * GW; g += AI_THREADS) {
      const int lg = g % GW, lh = (g / GW) % AI_LH, ld = g / (GW * AI_LH);
      if (ld < lo_l || ld >= hi_d || lh < lo_l || lh >= hi_h || 4 * lg + 3 < lo_l || 4 * lg >= AI_HALO + AI_TW + R) continue;
      const int gd = ai_reflect(d0 - AI_HALO + ld, Rd), gh = ai_reflect(h0 - AI_HALO + lh, Rh);
      int gw = w0 - AI_HALO + 4 * lg;                     // a multiple of 4
      bool rev = false;
      if (gw < 0) { gw = -4 - gw; rev = true; }
      else if (gw >= Rw) { gw = 2 * Rw - 4 - gw; rev = true; }
      gw = min(max(gw, 0), Rw - 4);
      const long i = ((long)gd * Rh + gh) * Rw + gw;
      f32x4 v = *reinterpret_cast<const f32x4*>(src + i);
      if (noisy) {
        float z[4];
        ai_normals(call_lo, call_hi, sample, (uint32_t)(i >> 2), k0, k1, z);
#pragma unroll
        for (int e = 0; e < 4; ++e) { const float t = std * z[e]; v[e] = v[e] + t; }
      }
      if (rev) { const f32x4 r = {v[3], v[2], v[1], v[0]}; v = r; }
      *reinterpret_cast<f32x4*>(&A[(ld * AI_LH + lh) * AI_LW + 4 * lg]) = v;
    }
  } else {
    for (int g = tid; g < AI_LD * AI_LH * AI_LW; g += AI_THREADS) {
      const int lw = g % AI_LW, lh = (g / AI_LW) % AI_LH, ld = g / (AI_LW * AI_LH);
      if (ld < lo_l || ld >= hi_d || lh < lo_l || lh >= hi_h || lw < lo_l || lw >= AI_HALO + AI_TW + R) continue;
      const int gd = ai_reflect(d0 - AI_HALO + ld, Rd), gh = ai_reflect(h0 - AI_HALO + lh, Rh), gw = ai_reflect(w0 - AI_HALO + lw, Rw);
      const long i = ((long)gd * Rh + gh) * Rw + gw;
      float v = src[i];
      if (noisy) {
        float z[4];
        ai_normals(call_lo, call_hi, sample, (uint32_t)(i >> 2), k0, k1, z);
        const int e = (int)(i & 3);
        const float t = std * (e == 0 ? z[0] : e == 1 ? z[1] : e == 2 ? z[2] : z[3]);
        v = v + t;
      }
      A[g] = v;
    }
  }
  __syncthreads();
  // along w: Bs[ld][lh][w] from A[ld][lh][w + 4 +- t]
  for (int o = tid; o < AI_LD * AI_LH * AI_TW; o += AI_THREADS) {
    const int w = o % AI_TW, lh = (o / AI_TW) % AI_LH, ld = o / (AI_TW * AI_LH);
    if (ld < lo_l || ld >= hi_d || lh < lo_l || lh >= hi_h) continue;
    const float* p = &A[(ld * AI_LH + lh) * AI_LW + w + AI_HALO];
    float acc = t0 * p[0];
    if (R >= 1) { acc += t1 * p[-1]; acc += t1 * p[1]; }
    if (R >= 2) { acc += t2 * p[-2]; acc += t2 * p[2]; }
    if (R >= 3) { acc += t3 * p[-3]; acc += t3 * p[3]; }
    if (R >= 4) { acc += t4 * p[-4]; acc += t4 * p[4]; }
    Bs[o] = acc;
  }
  __syncthreads();
  // along h: C[ld][h][w] (in A's storage) from Bs[ld][h + 4 +- t][w]
  float* Cs = A;
  for (int o = tid; o < AI_LD * AI_TH * AI_TW; o += AI_THREADS) {
    const int w = o % AI_TW, h = (o / AI_TW) % AI_TH, ld = o / (AI_TW * AI_TH);
    if (ld < lo_l || ld >= hi_d) continue;
    const float* p = &Bs[(ld * AI_LH + h + AI_HALO) * AI_TW + w];
    float acc = t0 * p[0];
    if (R >= 1) { acc += t1 * p[-1 * AI_TW]; acc += t1 * p[1 * AI_TW]; }
    if (R >= 2) { acc += t2 * p[-2 * AI_TW]; acc += t2 * p[2 * AI_TW]; }
    if (R >= 3) { acc += t3 * p[-3 * AI_TW]; acc += t3 * p[3 * AI_TW]; }
    if (R >= 4) { acc += t4 * p[-4 * AI_TW]; acc += t4 * p[4 * AI_TW]; }
    Cs[o] = acc;
  }
  __syncthreads();
  // along d, 4 voxels of a row per lane, and out
  {
    constexpr int PL = AI_TH * AI_TW;                     // one plane of Cs
    const int wq = tid % (AI_TW / 4), h = (tid / (AI_TW / 4)) % AI_TH, d = tid / (AI_TW / 4 * AI_TH);
    const int gd = d0 + d, gh = h0 + h, gw = w0 + 4 * wq;
    if (gd >= Rd || gh >= Rh || gw >= Rw) return;
    float acc[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float* p = &Cs[((d + AI_HALO) * AI_TH + h) * AI_TW + 4 * wq + e];
      float a = t0 * p[0];
      if (R >= 1) { a += t1 * p[-1 * PL]; a += t1 * p[1 * PL]; }
      if (R >= 2) { a += t2 * p[-2 * PL]; a += t2 * p[2 * PL]; }
      if (R >= 3) { a += t3 * p[-3 * PL]; a += t3 * p[3 * PL]; }
      if (R >= 4) { a += t4 * p[-4 * PL]; a += t4 * p[4 * PL]; }
      acc[e] = a;
    }
    float* dst = tmp + (long)b * vox + ((long)gd * Rh + gh) * Rw + gw;
    if constexpr (V == 4) {
      const f32x4 v = {acc[0], acc[1], acc[2], acc[3]};
      *reinterpret_cast<f32x4*>(dst) = v;                 // roi_w is a multiple of 4: all four inside
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (gw + e < Rw) dst[e] = acc[e];
    }
  }
}

// ---- the pointwise chain ----

__device__ __forceinline__ void ai_merge(AiStats& a, const AiStats& o) {
  a.sum += o.sum; a.sq += o.sq; a.mn = fmin(a.mn, o.mn); a.mx = fmax(a.mx, o.mx);
}
__device__ __forceinline__ AiStats ai_wave_reduce(AiStats a) {      // a butterfly: every lane ends with the same bits
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) {
    AiStats o;
    o.sum = __shfl_xor(a.sum, m); o.sq = __shfl_xor(a.sq, m); o.mn = __shfl_xor(a.mn, m); o.mx = __shfl_xor(a.mx, m);
    ai_merge(a, o);
  }
  return a;
}
constexpr double AI_INF = __builtin_huge_val();

// the workgroup's partial: waves by butterfly, then the waves in index order
__device__ __forceinline__ void ai_write_partial(AiStats a, AiStats* sh, AiStats* __restrict__ dst) {
  a = ai_wave_reduce(a);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = a;
  __syncthreads();
  if (threadIdx.x == 0) {
    AiStats t = sh[0];
    for (int w = 1; w < AI_THREADS / 64; ++w) ai_merge(t, sh[w]);
    *dst = t;
  }
}

// the statistics of a sample from its partials, the same bits in every workgroup: lane l of the first wave takes partials
// l, l + 64, .. in that order, then the butterfly
__device__ __forceinline__ AiStats ai_sample_stats(const AiStats* __restrict__ parts, int nparts, AiStats* sh) {
  if (threadIdx.x < 64) {
    AiStats a = {0.0, 0.0, AI_INF, -AI_INF};
    for (int p = threadIdx.x; p < nparts; p += 64) ai_merge(a, parts[p]);
    a = ai_wave_reduce(a);
    if (threadIdx.x == 0) *sh = a;
  }
  __syncthreads();
  return *sh;
}
// mean, population deviation, minimum, maximum: each rounded to fp32 once
struct AiMoments { float mean, dev, lo, hi; };
__device__ __forceinline__ AiMoments ai_moments(const AiStats& s, long n) {
  const double m = s.sum / (double)n, var = s.sq / (double)n - m * m;
  return AiMoments{(float)m, (float)sqrt(var > 0.0 ? var : 0.0), (float)s.mn, (float)s.mx};
}

template <int V> struct AiVec;
template <> struct AiVec<4> { using T = f32x4; };
template <> struct AiVec<1> { using T = float; };
template <int V> __device__ __forceinline__ void ai_load(const float* p, float x[V]) {
  if constexpr (V == 4) { const f32x4 v = *reinterpret_cast<const f32x4*>(p); x[0] = v[0]; x[1] = v[1]; x[2] = v[2]; x[3] = v[3]; }
  else x[0] = *p;
}
template <int V> __device__ __forceinline__ void ai_store(float* p, const float x[V]) {
  if constexpr (V == 4) { const f32x4 v = {x[0], x[1], x[2], x[3]}; *reinterpret_cast<f32x4*>(p) = v; }
  else *p = x[0];
}
__device__ __forceinline__ void ai_take(AiStats& a, float x) {
  const double d = (double)x;
  a.sum += d; a.sq += d * d; a.mn = fmin(a.mn, d); a.mx = fmax(a.mx, d);
}

enum { AI_BRIGHT = 0, AI_CONTRAST = 1, AI_GAMMA1 = 2, AI_GAMMA2 = 3 };

// One pass of the chain over sample blockIdx.y; gridDim.x workgroups stride over its groups of V voxels.  parts: [3][B][gridDim.x]
// partials -- 0: after brightness, 1: after contrast, 2: of gamma's y.
template <int V, int PASS>
__global__ void __launch_bounds__(AI_THREADS) aug_intensity_point_kernel(const float* images, const float* __restrict__ tmp,
                                                                        const float* __restrict__ rows, long vox, int B, float* out,
                                                                        AiStats* __restrict__ parts) {
  __shared__ AiStats sh[AI_THREADS / 64];
  __shared__ AiStats whole[2];
  const int b = blockIdx.y, np = gridDim.x;
  const float* row = rows + (long)b * DUA_AUG_INTENSITY_WORDS;
  const int mask = ai_events(row);
  const bool invert = (mask & DUA_AUG_INTENSITY_INVERT) != 0;
  AiStats* p0 = parts + ((long)0 * B + b) * np;
  AiStats* p1 = parts + ((long)1 * B + b) * np;
  AiStats* p2 = parts + ((long)2 * B + b) * np;
  float* dst = out + (long)b * vox;
  const long first = ((long)blockIdx.x * AI_THREADS + threadIdx.x) * V, step = (long)np * AI_THREADS * V;
  AiStats acc = {0.0, 0.0, AI_INF, -AI_INF};
  if constexpr (PASS == AI_BRIGHT) {
    const float* src = (mask & (DUA_AUG_INTENSITY_NOISE | DUA_AUG_INTENSITY_BLUR)) ? tmp + (long)b * vox : images + (long)b * vox;
    const bool mul = (mask & DUA_AUG_INTENSITY_BRIGHTNESS) != 0;
    const bool stats = (mask & (DUA_AUG_INTENSITY_CONTRAST | DUA_AUG_INTENSITY_GAMMA)) != 0;
    if (src == dst && !mul && !stats) return;
    const float f = row[DUA_AUG_INTENSITY_BRIGHT];
    for (long i = first; i < vox; i += step) {
      float x[V];
      ai_load<V>(src + i, x);
#pragma unroll
      for (int e = 0; e < V; ++e) {
        if (mul) x[e] = x[e] * f;
        ai_take(acc, x[e]);
      }
      if (src != dst || mul) ai_store<V>(dst + i, x);
    }
    if (stats) ai_write_partial(acc, sh, p0 + blockIdx.x);
  } else if constexpr (PASS == AI_CONTRAST) {
    if (!(mask & DUA_AUG_INTENSITY_CONTRAST)) return;
    const AiMoments s = ai_moments(ai_sample_stats(p0, np, &whole[0]), vox);
    const float f = row[DUA_AUG_INTENSITY_CONTRAST_F];
    const bool stats = (mask & DUA_AUG_INTENSITY_GAMMA) != 0;
    for (long i = first; i < vox; i += step) {
      float x[V];
      ai_load<V>(dst + i, x);
#pragma unroll
      for (int e = 0; e < V; ++e) {
        const float c = x[e] - s.mean, t = c * f, v = t + s.mean;
        x[e] = fminf(fmaxf(v, s.lo), s.hi);
        ai_take(acc, x[e]);
      }
      ai_store<V>(dst + i, x);
    }
    if (stats) ai_write_partial(acc, sh, p1 + blockIdx.x);
  } else {
    if (!(mask & DUA_AUG_INTENSITY_GAMMA)) return;
    const AiMoments s = ai_moments(ai_sample_stats((mask & DUA_AUG_INTENSITY_CONTRAST) ? p1 : p0, np, &whole[0]), vox);
    // the statistics of -x from those of x: exact
    const float mean = invert ? -s.mean : s.mean, lo = invert ? -s.hi : s.lo, hi = invert ? -s.lo : s.hi;
    if constexpr (PASS == AI_GAMMA1) {
      const float g = row[DUA_AUG_INTENSITY_GAMMA_V], range = hi - lo, den = range + 1e-7f;
      for (long i = first; i < vox; i += step) {
        float x[V];
        ai_load<V>(dst + i, x);
#pragma unroll
        for (int e = 0; e < V; ++e) {
          const float v = invert ? -x[e] : x[e];
          const float a = v - lo, t = a / den, p = powf(t, g), q = p * range;
          x[e] = q + lo;
          ai_take(acc, x[e]);
        }
        ai_store<V>(dst + i, x);
      }
      ai_write_partial(acc, sh, p2 + blockIdx.x);
    } else {
      const AiMoments y = ai_moments(ai_sample_stats(p2, np, &whole[1]), vox);
      const float den = y.dev + 1e-8f;
      for (long i = first; i < vox; i += step) {
        float x[V];
        ai_load<V>(dst + i, x);
#pragma unroll
        for (int e = 0; e < V; ++e) {
          const float c = x[e] - y.mean, q = c / den, r = q * s.dev, v = r + mean;
          x[e] = invert ? -v : v;
        }
        ai_store<V>(dst + i, x);
      }
    }
  }
}

static bool ai_prob_ok(float p) { return p >= 0.f && p <= 1.f; }
static bool ai_finite(float x) { return x >= -3.0e38f && x <= 3.0e38f; }      // false for a NaN
static long ai_parts(long vox, bool wide) {
  const long groups = wide ? vox / 4 : vox, blocks = (groups + AI_THREADS - 1) / AI_THREADS;
  return blocks < AI_MAX_PARTS ? blocks : AI_MAX_PARTS;
}
static long ai_tmp_bytes(int B, long vox) { return ((long)B * vox * 4 + 255) / 256 * 256; }

}  // namespace dua

extern "C" {

long dua_aug_intensity_scratch_bytes(int B, int roi_d, int roi_h, int roi_w) {
  if (B < 1 || B > 65535 || roi_d < 4 || roi_h < 4 || roi_w < 4) return DUA_ERR_ARG;
  const long vox = (long)roi_d * roi_h;                   // two factors below 2^31
  if (vox >= (1L << 31) || vox * roi_w >= (1L << 31)) return DUA_ERR_ARG;
  return dua::ai_tmp_bytes(B, vox * roi_w) + 3L * B * dua::AI_MAX_PARTS * (long)sizeof(dua::AiStats);
}

int dua_aug_intensity_draw(const dua_aug_intensity_config* cfg, int B, unsigned long long seed, unsigned long long* counter,
                           int use_counter, unsigned long long counter_value, float* rows, void* stream) {
  if (!cfg || B < 1 || !rows || (!use_counter && !counter)) return DUA_ERR_ARG;
  const dua_aug_intensity_config c = *cfg;
  if (!dua::ai_prob_ok(c.noise_prob) || !dua::ai_prob_ok(c.blur_prob) || !dua::ai_prob_ok(c.brightness_prob) ||
      !dua::ai_prob_ok(c.contrast_prob) || !dua::ai_prob_ok(c.gamma_prob) || !dua::ai_prob_ok(c.gamma_invert_prob))
    return DUA_ERR_ARG;
  // every comparison is false for a NaN
  if (!(c.noise_std_min >= 0.f && dua::ai_finite(c.noise_std_min)) || !(c.noise_std_span >= 0.f && dua::ai_finite(c.noise_std_span)) ||
      !(c.blur_sigma_min > 0.f) || !(c.blur_sigma_span >= 0.f) ||
      !(floorf(4.f * (c.blur_sigma_min + c.blur_sigma_span) + 0.5f) <= (float)DUA_AUG_INTENSITY_MAX_RADIUS) ||
      !(c.brightness_min > 0.f && dua::ai_finite(c.brightness_min)) || !(c.brightness_span >= 0.f && dua::ai_finite(c.brightness_span)) ||
      !(c.contrast_min > 0.f && dua::ai_finite(c.contrast_min)) || !(c.contrast_span >= 0.f && dua::ai_finite(c.contrast_span)) ||
      !(c.gamma_min > 0.f && dua::ai_finite(c.gamma_min)) || !dua::ai_finite(c.gamma_span_below) || !dua::ai_finite(c.gamma_span_above) ||
      !(c.gamma_min + c.gamma_span_below > 0.f) || !((c.gamma_min > 1.f ? c.gamma_min : 1.f) + c.gamma_span_above > 0.f))
    return DUA_ERR_ARG;
  const int waves = B < dua::AI_DRAW_WAVES ? B : dua::AI_DRAW_WAVES;
  hipLaunchKernelGGL(dua::aug_intensity_draw_kernel, dim3(1), dim3(waves * 64), 0, (hipStream_t)stream, c, B, seed, counter,
                     use_counter, counter_value, rows);
  return (int)hipGetLastError();
}

int dua_aug_intensity_apply(const float* images, const float* rows, int B, int roi_d, int roi_h, int roi_w,
                            unsigned long long seed, float* out, void* scratch, long scratch_bytes, void* stream) {
  if (!images || !rows || !out || !scratch || ((size_t)scratch & 15)) return DUA_ERR_ARG;
  const long need = dua_aug_intensity_scratch_bytes(B, roi_d, roi_h, roi_w);
  if (need < 0 || scratch_bytes < need) return DUA_ERR_ARG;
  const long vox = (long)roi_d * roi_h * roi_w;
  float* tmp = (float*)scratch;
  dua::AiStats* parts = (dua::AiStats*)((char*)scratch + dua::ai_tmp_bytes(B, vox));
  // 16-byte accesses need every sample and every row to start on a 16-byte boundary
  const bool wide = roi_w % 4 == 0 && ((size_t)images & 15) == 0 && ((size_t)out & 15) == 0;
  hipStream_t s = (hipStream_t)stream;
  const long tiles = (long)((roi_d + dua::AI_TD - 1) / dua::AI_TD) * ((roi_h + dua::AI_TH - 1) / dua::AI_TH) *
                     ((roi_w + dua::AI_TW - 1) / dua::AI_TW);            // at most vox / 64 + ..: below 2^31
  const dim3 tgrid((unsigned)tiles, B), pgrid((unsigned)dua::ai_parts(vox, wide), B), block(dua::AI_THREADS);
#define DUA_AI_POINT(V, PASS) \
  hipLaunchKernelGGL((dua::aug_intensity_point_kernel<V, PASS>), pgrid, block, 0, s, images, (const float*)tmp, rows, vox, B, out, parts)
  if (wide) {
    hipLaunchKernelGGL(dua::aug_intensity_noise_blur_kernel<4>, tgrid, block, 0, s, images, rows, roi_d, roi_h, roi_w, seed, tmp);
    DUA_AI_POINT(4, dua::AI_BRIGHT); DUA_AI_POINT(4, dua::AI_CONTRAST); DUA_AI_POINT(4, dua::AI_GAMMA1); DUA_AI_POINT(4, dua::AI_GAMMA2);
  } else {
    hipLaunchKernelGGL(dua::aug_intensity_noise_blur_kernel<1>, tgrid, block, 0, s, images, rows, roi_d, roi_h, roi_w, seed, tmp);
    DUA_AI_POINT(1, dua::AI_BRIGHT); DUA_AI_POINT(1, dua::AI_CONTRAST); DUA_AI_POINT(1, dua::AI_GAMMA1); DUA_AI_POINT(1, dua::AI_GAMMA2);
  }
#undef DUA_AI_POINT
  return (int)hipGetLastError();
}

}  // extern "C"
