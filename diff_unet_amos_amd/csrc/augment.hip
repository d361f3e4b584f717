// Augmented training batches from device-resident volumes: the random tail of the reference's training transforms
// (utils.py:143-160: RandCropByPosNegLabeld, three RandFlipd, RandRotate90d, RandScaleIntensityd, RandShiftIntensityd) and the
// one-hot expansion of Engine.convert_labels (engine.py:157-165).  The contract (which random word decides what, the index
// maps, the order of the fp32 operations) is written down in include/dua_hip.h; this file only says how it is computed.
//
//   count  : once per volume.  One block per chunk of DUA_AUG_CHUNK voxels counts both candidate sets (ballot + popcount, no
//            atomics); a single block then turns the per-chunk counts into exclusive prefix tables in place.
//   draw   : ONE workgroup per call, one wave per sample (samples beyond the workgroup's waves in further rounds).  The
//            decisions are wave-uniform arithmetic on three Philox blocks.  "The r-th candidate" is a 64-ary search of the
//            prefix table (every lane probes one entry, a ballot picks the segment: three dependent loads for 5 000 chunks
//            where a binary search takes thirteen) and a ballot / popcount scan of the one chunk found; the lane that holds
//            the candidate writes the row.  One workgroup, because the call counter is read by every sample and advanced by
//            one lane of the same launch: a workgroup barrier orders the two, which no grid of independent workgroups could.
//   apply  : a pure store-bandwidth kernel (per voxel: 4 + 1 bytes read, 4 (1 + C) written).  The rotation is in the (d, h)
//            plane, so an output row along w is always one source row, forwards or backwards: a lane owns 4 consecutive
//            output voxels, reads their 4 floats and 4 label bytes and writes one 16-byte store into the image plane and
//            into each of the C label planes; a wave-instruction covers 1 KiB of one plane.
// -ffp-contract=off (csrc/Makefile) keeps the three fp32 operations of the intensity transform, and the two of each drawn
// value, separately rounded; the pragma below says so for this file whatever the command line.
#include "common.hpp"
#include "philox.hpp"
#include "../../include/dua_hip.h"

#pragma clang fp contract(off)

namespace dua {

constexpr int AUG_THREADS = 256;
constexpr int AUG_DRAW_WAVES = 16;
static_assert(DUA_AUG_CHUNK == 4 * AUG_THREADS, "the counting block takes 4 voxels per thread");
static_assert(sizeof(dua_aug_volume) == 64, "dua_aug_volume is a 64-byte row");

__device__ __forceinline__ bool is_candidate(bool fg, unsigned char l, float v, float thr) {
  return fg ? (l > 0) : (l == 0 && v > thr);
}

// counts[0][c], counts[1][c] = candidates of either kind in chunk c (entry nchunks is left to the scan)
__global__ void __launch_bounds__(AUG_THREADS) aug_chunk_counts_kernel(const float* __restrict__ image,
                                                                       const unsigned char* __restrict__ label, long voxels,
                                                                       float thr, int nchunks, unsigned* __restrict__ prefix) {
  __shared__ unsigned part[2][AUG_THREADS / 64];
  const int c = blockIdx.x, tid = threadIdx.x;
  unsigned fg = 0, bg = 0;
#pragma unroll
  for (int j = 0; j < DUA_AUG_CHUNK / AUG_THREADS; ++j) {
    const long i = (long)c * DUA_AUG_CHUNK + j * AUG_THREADS + tid;
    const bool in = i < voxels;
    const unsigned char l = in ? label[i] : 0;
    const float v = in ? image[i] : 0.f;
    fg += __popcll(__ballot(in && is_candidate(true, l, v, thr)));
    bg += __popcll(__ballot(in && is_candidate(false, l, v, thr)));
  }
  if ((tid & 63) == 0) { part[0][tid >> 6] = fg; part[1][tid >> 6] = bg; }
  __syncthreads();
  if (tid < 2) {
    unsigned s = 0;
    for (int w = 0; w < AUG_THREADS / 64; ++w) s += part[tid][w];
    prefix[(long)tid * (nchunks + 1) + c] = s;
  }
}

// in place, per row: counts [nchunks] -> exclusive prefix [nchunks + 1] (the last entry is the total).  One block per row;
// every thread owns a contiguous segment.
__global__ void __launch_bounds__(AUG_THREADS) aug_prefix_scan_kernel(int nchunks, unsigned* __restrict__ prefix) {
  __shared__ unsigned seg[AUG_THREADS];
  unsigned* row = prefix + (long)blockIdx.x * (nchunks + 1);
  const int tid = threadIdx.x, per = (nchunks + AUG_THREADS - 1) / AUG_THREADS;
  const int lo = min(tid * per, nchunks), hi = min(lo + per, nchunks);
  unsigned s = 0;
  for (int i = lo; i < hi; ++i) s += row[i];
  seg[tid] = s;
  __syncthreads();
  unsigned base = 0;
  for (int t = 0; t < tid; ++t) base += seg[t];
  for (int i = lo; i < hi; ++i) {
    const unsigned n = row[i];
    row[i] = base;
    base += n;
  }
  if (tid == AUG_THREADS - 1) row[nchunks] = base;       // the last thread's running sum has passed every chunk
}

__device__ __forceinline__ float unit_float(uint32_t x) { return (float)(x >> 8) * 5.9604644775390625e-8f; }   // 2^-24: exact
__device__ __forceinline__ uint32_t below(uint32_t x, uint32_t n) { return __umulhi(x, n); }
__device__ __forceinline__ float symmetric(float half_width, uint32_t x) {
  const float t = (2.f * half_width) * unit_float(x);
  return t + (-half_width);
}

__global__ void __launch_bounds__(AUG_DRAW_WAVES * 64) aug_draw_kernel(const dua_aug_volume* __restrict__ table, int nvol,
                                                                      const int* __restrict__ ids, int B, dua_aug_config cfg,
                                                                      unsigned long long seed, unsigned long long* counter,
                                                                      int use_counter, unsigned long long counter_value,
                                                                      int* __restrict__ params, int* status) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long call = use_counter ? counter_value : *counter;
  __syncthreads();                                        // every wave holds the call counter before one lane moves it on
  if (!use_counter && threadIdx.x == 0) *counter = call + 1;
  for (int b = wave; b < B; b += AUG_DRAW_WAVES) {
    int* row = params + (long)b * DUA_AUG_PARAM_WORDS;
    const int vid = ids[b];
    if (vid < 0 || vid >= nvol) {
      if (lane == 0) {
        row[DUA_AUG_VOLUME] = -1;
        for (int j = 1; j < DUA_AUG_PARAM_WORDS; ++j) row[j] = 0;
        if (status) *status = 1;
      }
      continue;
    }
    const dua_aug_volume vol = table[vid];
    uint32_t w[3][4];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      w[j][0] = (uint32_t)call; w[j][1] = (uint32_t)(call >> 32); w[j][2] = (uint32_t)b; w[j][3] = (uint32_t)j;
      philox4x32_10(w[j], (uint32_t)seed, (uint32_t)(seed >> 32));
    }
    const bool fg = vol.fg_count > 0 && (vol.bg_count == 0 || unit_float(w[0][0]) < cfg.pos_fraction);
    const uint32_t count = fg ? vol.fg_count : vol.bg_count;
    const unsigned* prefix = fg ? vol.fg_prefix : vol.bg_prefix;
    const uint32_t r = below(w[0][1], count);
    int flip = 0;
    flip |= unit_float(w[0][2]) < cfg.flip_prob ? 1 : 0;
    flip |= unit_float(w[0][3]) < cfg.flip_prob ? 2 : 0;
    flip |= unit_float(w[1][0]) < cfg.flip_prob ? 4 : 0;
    const int k = unit_float(w[1][1]) < cfg.rot90_prob ? 1 + (int)below(w[1][2], (uint32_t)cfg.max_k) : 0;
    const float scale = unit_float(w[1][3]) < cfg.scale_prob ? symmetric(cfg.scale_factors, w[2][0]) : 0.f;
    const float shift = unit_float(w[2][1]) < cfg.shift_prob ? symmetric(cfg.shift_offsets, w[2][2]) : 0.f;
    if (count == 0) {                                     // a table row the host should never have built
      if (lane == 0) {
        row[DUA_AUG_VOLUME] = -1;
        for (int j = 1; j < DUA_AUG_PARAM_WORDS; ++j) row[j] = 0;
        if (status) *status = 1;
      }
      continue;
    }
    // the chunk c with prefix[c] <= r < prefix[c + 1]: prefix is non-decreasing, prefix[0] = 0 <= r < total = prefix[nchunks]
    int lo = 0, hi = vol.nchunks;
    while (hi - lo > 1) {
      const int step = (hi - lo + 63) >> 6;
      const long idx = (long)lo + (long)lane * step;
      const unsigned v = idx < hi ? prefix[idx] : 0xFFFFFFFFu;
      const int seg = __popcll(__ballot(idx < hi && v <= r)) - 1;      // lane 0 probes prefix[lo] <= r: seg >= 0
      lo += max(seg, 0) * step;
      hi = min(lo + step, hi);
    }
    uint32_t rem = r - prefix[lo];
    const long voxels = (long)vol.D * vol.H * vol.W;
    bool written = false;
    for (int j = 0; j < DUA_AUG_CHUNK / 64; ++j) {
      const long i = (long)lo * DUA_AUG_CHUNK + j * 64 + lane;
      const bool in = i < voxels;
      const bool cand = in && is_candidate(fg, vol.label[in ? i : 0], vol.image[in ? i : 0], vol.image_threshold);
      const unsigned long long m = __ballot(cand);
      const uint32_t n = __popcll(m);
      if (rem < n) {
        const uint32_t rank = __popcll(m & ((1ull << lane) - 1ull));
        if (cand && rank == rem) {
          const unsigned line = (unsigned)i / (unsigned)vol.W;                  // voxels < 2^31
          const int cw = (int)((unsigned)i - line * (unsigned)vol.W), cd = (int)(line / (unsigned)vol.H);
          const int ch = (int)(line - (unsigned)cd * (unsigned)vol.H);
          row[DUA_AUG_VOLUME] = vid;
          row[DUA_AUG_START_D] = min(max(cd - cfg.roi[0] / 2, 0), vol.D - cfg.roi[0]);
          row[DUA_AUG_START_H] = min(max(ch - cfg.roi[1] / 2, 0), vol.H - cfg.roi[1]);
          row[DUA_AUG_START_W] = min(max(cw - cfg.roi[2] / 2, 0), vol.W - cfg.roi[2]);
          row[DUA_AUG_FLIP] = flip;
          row[DUA_AUG_K] = k;
          row[DUA_AUG_SCALE] = __float_as_int(scale);
          row[DUA_AUG_SHIFT] = __float_as_int(shift);
        }
        written = true;
        break;
      }
      rem -= n;
    }
    if (!written && lane == 0) {                          // the prefix table and the volume disagree
      row[DUA_AUG_VOLUME] = -1;
      for (int j = 1; j < DUA_AUG_PARAM_WORDS; ++j) row[j] = 0;
      if (status) *status = 1;
    }
  }
}

template <int V> struct OutVec;
template <> struct OutVec<4> { using T = f32x4; };
template <> struct OutVec<1> { using T = float; };

// V output voxels per lane (4: roi_w is a multiple of 4, so a group never crosses a row and every store is 16-byte aligned)
template <int V>
__global__ void __launch_bounds__(AUG_THREADS) aug_apply_kernel(const dua_aug_volume* __restrict__ table, int nvol,
                                                               const int* __restrict__ params, int Rd, int Rh, int Rw,
                                                               const unsigned char* __restrict__ class_ids, int C,
                                                               float* __restrict__ images, float* __restrict__ labels,
                                                               int* status) {
  using Vec = typename OutVec<V>::T;
  const int b = blockIdx.y;
  const int* row = params + (long)b * DUA_AUG_PARAM_WORDS;
  const int vid = row[DUA_AUG_VOLUME], sd0 = row[DUA_AUG_START_D], sh0 = row[DUA_AUG_START_H], sw0 = row[DUA_AUG_START_W];
  const int flip = row[DUA_AUG_FLIP], k = row[DUA_AUG_K];
  bool ok = vid >= 0 && vid < nvol && (unsigned)flip < 8u && (unsigned)k < 4u && (!(k & 1) || Rd == Rh);
  dua_aug_volume vol = {};
  if (ok) {
    vol = table[vid];
    ok = sd0 >= 0 && sh0 >= 0 && sw0 >= 0 && sd0 <= vol.D - Rd && sh0 <= vol.H - Rh && sw0 <= vol.W - Rw;
  }
  if (!ok) {                                              // block-uniform: nothing is read, nothing is written
    if (status && blockIdx.x == 0 && threadIdx.x == 0) *status = 1;
    return;
  }
  const long vox = (long)Rd * Rh * Rw;
  const unsigned o = (blockIdx.x * (unsigned)AUG_THREADS + threadIdx.x) * V;   // first output voxel of this lane (vox < 2^31)
  if (o >= vox) return;
  const unsigned orow = o / (unsigned)Rw;
  const int ow = (int)(o - orow * (unsigned)Rw), od = (int)(orow / (unsigned)Rh), oh = (int)(orow - (unsigned)od * (unsigned)Rh);
  // inverse of rot90(., k, (0, 1)): k = 1: out[i][j] = x[j][n - 1 - i]; k = 2: x[n0 - 1 - i][n1 - 1 - j]; k = 3: x[n - 1 - j][i]
  int a, c;
  switch (k) {
    case 1: a = oh; c = Rh - 1 - od; break;
    case 2: a = Rd - 1 - od; c = Rh - 1 - oh; break;
    case 3: a = Rd - 1 - oh; c = od; break;
    default: a = od; c = oh; break;
  }
  if (flip & 1) a = Rd - 1 - a;
  if (flip & 2) c = Rh - 1 - c;
  const bool fw = (flip & 4) != 0;
  const long src = ((long)(sd0 + a) * vol.H + (sh0 + c)) * vol.W + sw0;     // start of the source row's window
  const float factor = 1.f + __int_as_float(row[DUA_AUG_SCALE]);
  const float shift = __int_as_float(row[DUA_AUG_SHIFT]);
  float px[V];
  unsigned char lb[V];
#pragma unroll
  for (int e = 0; e < V; ++e) {
    const int sw = fw ? Rw - 1 - (ow + e) : ow + e;
    px[e] = vol.image[src + sw];
    lb[e] = vol.label[src + sw];
  }
  Vec v;
  if constexpr (V == 4) {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = px[e] * factor + shift;
  } else {
    v = px[0] * factor + shift;
  }
  *reinterpret_cast<Vec*>(images + (long)b * vox + o) = v;
  float* lab = labels + (long)b * C * vox + o;
#pragma unroll 4
  for (int ch = 0; ch < C; ++ch) {
    const unsigned char id = class_ids[ch];
    Vec m;
    if constexpr (V == 4) {
#pragma unroll
      for (int e = 0; e < 4; ++e) m[e] = lb[e] == id ? 1.f : 0.f;
    } else {
      m = lb[0] == id ? 1.f : 0.f;
    }
    *reinterpret_cast<Vec*>(lab + (long)ch * vox) = m;
  }
}

static bool prob_ok(float p) { return p >= 0.f && p <= 1.f; }

}  // namespace dua

extern "C" {

int dua_aug_count_candidates(const float* image, const unsigned char* label, long voxels, float image_threshold,
                             unsigned* prefix, void* stream) {
  if (!image || !label || !prefix || voxels <= 0 || voxels >= (1L << 31) || image_threshold != image_threshold)
    return DUA_ERR_ARG;
  const int nchunks = (int)((voxels + DUA_AUG_CHUNK - 1) / DUA_AUG_CHUNK);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(dua::aug_chunk_counts_kernel, dim3(nchunks), dim3(dua::AUG_THREADS), 0, s, image, label, voxels,
                     image_threshold, nchunks, prefix);
  hipLaunchKernelGGL(dua::aug_prefix_scan_kernel, dim3(2), dim3(dua::AUG_THREADS), 0, s, nchunks, prefix);
  return (int)hipGetLastError();
}

int dua_aug_draw(const dua_aug_volume* table, int nvol, const int* ids, int B, const dua_aug_config* cfg,
                 unsigned long long seed, unsigned long long* counter, int use_counter, unsigned long long counter_value,
                 int* params, int* status, void* stream) {
  if (!table || nvol < 1 || !ids || B < 1 || !cfg || !params || (!use_counter && !counter)) return DUA_ERR_ARG;
  if (cfg->roi[0] < 1 || cfg->roi[1] < 1 || cfg->roi[2] < 1 || cfg->max_k < 1 || cfg->max_k > 3) return DUA_ERR_ARG;
  if (!dua::prob_ok(cfg->pos_fraction) || !dua::prob_ok(cfg->flip_prob) || !dua::prob_ok(cfg->rot90_prob) ||
      !dua::prob_ok(cfg->scale_prob) || !dua::prob_ok(cfg->shift_prob) || !(cfg->scale_factors >= 0.f) ||
      !(cfg->shift_offsets >= 0.f) || (cfg->rot90_prob > 0.f && cfg->roi[0] != cfg->roi[1]))
    return DUA_ERR_ARG;
  const int waves = B < dua::AUG_DRAW_WAVES ? B : dua::AUG_DRAW_WAVES;
  hipLaunchKernelGGL(dua::aug_draw_kernel, dim3(1), dim3(waves * 64), 0, (hipStream_t)stream, table, nvol, ids, B, *cfg, seed,
                     counter, use_counter, counter_value, params, status);
  return (int)hipGetLastError();
}

int dua_aug_apply(const dua_aug_volume* table, int nvol, const int* params, int B, int roi_d, int roi_h, int roi_w,
                  const unsigned char* class_ids, int C, float* images, float* labels, int* status, void* stream) {
  if (!table || nvol < 1 || !params || B < 1 || B > 65535 || roi_d < 1 || roi_h < 1 || roi_w < 1 || !class_ids || C < 1 ||
      C > DUA_AUG_MAX_CLASSES || !images || !labels)
    return DUA_ERR_ARG;
  const long vox = (long)roi_d * roi_h * roi_w;
  if (vox >= (1L << 31)) return DUA_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  // 16-byte stores need every plane and every row to start on a 16-byte boundary
  const bool wide = roi_w % 4 == 0 && ((size_t)images & 15) == 0 && ((size_t)labels & 15) == 0;
  if (wide) {
    const dim3 grid((unsigned)((vox / 4 + dua::AUG_THREADS - 1) / dua::AUG_THREADS), B);
    hipLaunchKernelGGL(dua::aug_apply_kernel<4>, grid, dim3(dua::AUG_THREADS), 0, s, table, nvol, params, roi_d, roi_h, roi_w,
                       class_ids, C, images, labels, status);
  } else {
    const dim3 grid((unsigned)((vox + dua::AUG_THREADS - 1) / dua::AUG_THREADS), B);
    hipLaunchKernelGGL(dua::aug_apply_kernel<1>, grid, dim3(dua::AUG_THREADS), 0, s, table, nvol, params, roi_d, roi_h, roi_w,
                       class_ids, C, images, labels, status);
  }
  return (int)hipGetLastError();
}

}  // extern "C"
