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
//   centroids : once per volume, for label smoothing (dataset/cache_dataset.py:105-153).  One pass over the label map, 16 bytes
//            per thread and step; count and index sums per class as 64-bit integers, LDS atomics inside a workgroup, one
//            global integer atomic per class and workgroup: exact, so identical between runs.  A finish launch divides in fp64.
//   smoothed apply : the apply kernel with another body for the label planes (template parameter MODE): the same index code
//            gives the source index of a lane's 4 voxels, the centroids of the row's volume sit in LDS (one broadcast read per
//            channel), and a channel costs 4 x (sub, fma, sqrt, add, rcp, mul, sub, min) before its 16-byte store.
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

// what the smoothed forms need beyond the one-hot apply (unused by SMOOTH_NONE)
struct AugSmooth {
  const float* centroids;                                 // fp32 [nvol][K][3]
  int K;
  float alpha, order, epsilon, max_value;
};
enum { SMOOTH_NONE = 0, SMOOTH_ORDER1 = 1, SMOOTH_POW = 2 };

// V output voxels per lane (4: roi_w is a multiple of 4, so a group never crosses a row and every store is 16-byte aligned).
// MODE: what a label plane holds -- SMOOTH_NONE: the one-hot channel; SMOOTH_ORDER1 / SMOOTH_POW: the centroid-distance
// smoothed channel (order == 1 without pow), evaluated at the source index that the index code, shared by all, finds.
template <int V, int MODE>
__global__ void __launch_bounds__(AUG_THREADS) aug_apply_kernel(const dua_aug_volume* __restrict__ table, int nvol,
                                                               const int* __restrict__ params, int Rd, int Rh, int Rw,
                                                               const unsigned char* __restrict__ class_ids, int C,
                                                               float* __restrict__ images, float* __restrict__ labels,
                                                               int* status, AugSmooth sm) {
  using Vec = typename OutVec<V>::T;
  __shared__ float cen[MODE == SMOOTH_NONE ? 1 : DUA_AUG_MAX_CLASSES][4];      // centroid of class_ids[ch] in the row's volume
  __shared__ int bad_id;
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
  if constexpr (MODE != SMOOTH_NONE) {
    if (threadIdx.x == 0) bad_id = 0;
    __syncthreads();
    if ((int)threadIdx.x < C) {                           // C <= DUA_AUG_MAX_CLASSES < AUG_THREADS
      const int id = class_ids[threadIdx.x];
      if (id < sm.K) {
        const float* c3 = sm.centroids + ((long)vid * sm.K + id) * 3;
        cen[threadIdx.x][0] = c3[0]; cen[threadIdx.x][1] = c3[1]; cen[threadIdx.x][2] = c3[2];
      } else {
        bad_id = 1;
      }
    }
    __syncthreads();
    if (bad_id) {                                         // block-uniform again: a class id without a centroid row
      if (status && blockIdx.x == 0 && threadIdx.x == 0) *status = 1;
      return;
    }
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
  if constexpr (MODE == SMOOTH_NONE) {
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
  } else {
    // the source index of the lane's voxels is (sd0 + a, sh0 + c, sw0 + sw_e); fp32 holds it exactly for extents up to 2^24
    const float fd = (float)(sd0 + a), fh = (float)(sh0 + c);
    float fx[V];
#pragma unroll
    for (int e = 0; e < V; ++e) fx[e] = (float)(sw0 + (fw ? Rw - 1 - (ow + e) : ow + e));
#pragma unroll 2
    for (int ch = 0; ch < C; ++ch) {
      const unsigned char id = class_ids[ch];
      const float dd = fd - cen[ch][0], dh = fh - cen[ch][1], cw = cen[ch][2];
      const float t = dd * dd + dh * dh;
      float m[V];
#pragma unroll
      for (int e = 0; e < V; ++e) {
        const float dw = fx[e] - cw;
        const float dist = __builtin_amdgcn_sqrtf(__builtin_fmaf(dw, dw, t));
        const float p = MODE == SMOOTH_POW ? powf(dist, sm.order) : dist;
        const float s = __builtin_amdgcn_rcpf(p + sm.epsilon) * sm.alpha;
        m[e] = fminf(fabsf((lb[e] == id ? 1.f : 0.f) - s), sm.max_value);
      }
      if constexpr (V == 4) {
        Vec mv;
#pragma unroll
        for (int e = 0; e < 4; ++e) mv[e] = m[e];
        *reinterpret_cast<Vec*>(lab + (long)ch * vox) = mv;
      } else {
        *(lab + (long)ch * vox) = m[0];
      }
    }
  }
}

constexpr int CEN_THREADS = 256;
constexpr int CEN_RUN = 16;                               // label bytes per thread and step: one 16-byte load
constexpr int CEN_MAX_BLOCKS = 2048;
constexpr int CEN_MAX_CLASSES = 256;                      // every value of a uint8 label map

// sums[k] += (count, sum d, sum h, sum w) of the voxels of class k (row K: ids >= K).  A thread takes 16 consecutive voxels and
// adds to the workgroup's LDS table once per run of equal ids (label maps are piecewise constant: mostly one run); the
// workgroup adds its non-zero entries to the global table once.  64-bit integer atomics at both levels: the sums are exact
// and do not depend on the order of arrival.
__global__ void __launch_bounds__(CEN_THREADS) aug_class_sums_kernel(const unsigned char* __restrict__ label, long voxels, int H,
                                                                    int W, int K, unsigned long long* __restrict__ sums) {
  __shared__ unsigned long long part[(CEN_MAX_CLASSES + 1) * 4];
  for (int i = threadIdx.x; i < (K + 1) * 4; i += CEN_THREADS) part[i] = 0;
  __syncthreads();
  const long groups = (voxels + CEN_RUN - 1) / CEN_RUN;
  for (long g = (long)blockIdx.x * CEN_THREADS + threadIdx.x; g < groups; g += (long)gridDim.x * CEN_THREADS) {
    const long i0 = g * CEN_RUN;
    const int n = (int)min((long)CEN_RUN, voxels - i0);
    unsigned char lb[CEN_RUN];
    if (n == CEN_RUN) {                                   // label is 16-byte aligned (checked by the launcher)
      const uint4 q = *reinterpret_cast<const uint4*>(label + i0);
      const unsigned wd[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
      for (int e = 0; e < CEN_RUN; ++e) lb[e] = (unsigned char)(wd[e >> 2] >> (8 * (e & 3)));
    } else {
#pragma unroll
      for (int e = 0; e < CEN_RUN; ++e) lb[e] = e < n ? label[i0 + e] : 0;
    }
    const unsigned line = (unsigned)i0 / (unsigned)W;     // voxels < 2^31
    int w = (int)((unsigned)i0 - line * (unsigned)W), d = (int)(line / (unsigned)H), h = (int)(line - (unsigned)d * (unsigned)H);
    int cur = min((int)lb[0], K);
    unsigned long long cnt = 0, sd = 0, sh = 0, sw = 0;
#pragma unroll
    for (int e = 0; e < CEN_RUN; ++e) {
      if (e < n) {
        const int id = min((int)lb[e], K);
        if (id != cur) {
          atomicAdd(&part[cur * 4 + 0], cnt); atomicAdd(&part[cur * 4 + 1], sd);
          atomicAdd(&part[cur * 4 + 2], sh); atomicAdd(&part[cur * 4 + 3], sw);
          cur = id; cnt = sd = sh = sw = 0;
        }
        cnt += 1; sd += (unsigned)d; sh += (unsigned)h; sw += (unsigned)w;
        if (++w == W) { w = 0; if (++h == H) { h = 0; ++d; } }
      }
    }
    atomicAdd(&part[cur * 4 + 0], cnt); atomicAdd(&part[cur * 4 + 1], sd);
    atomicAdd(&part[cur * 4 + 2], sh); atomicAdd(&part[cur * 4 + 3], sw);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < (K + 1) * 4; i += CEN_THREADS)
    if (part[i]) atomicAdd(&sums[i], part[i]);
}

// centroids[k] = fp32(sum / count), the division in fp64 on exact operands (below 2^53); zeros for an absent class
__global__ void aug_centroid_finish_kernel(int K, const unsigned long long* __restrict__ sums, float* __restrict__ centroids) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= K) return;
  const unsigned long long n = sums[k * 4];
#pragma unroll
  for (int j = 0; j < 3; ++j) centroids[k * 3 + j] = n ? (float)((double)sums[k * 4 + 1 + j] / (double)n) : 0.f;
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
    hipLaunchKernelGGL((dua::aug_apply_kernel<4, dua::SMOOTH_NONE>), grid, dim3(dua::AUG_THREADS), 0, s, table, nvol, params,
                       roi_d, roi_h, roi_w, class_ids, C, images, labels, status, dua::AugSmooth{});
  } else {
    const dim3 grid((unsigned)((vox + dua::AUG_THREADS - 1) / dua::AUG_THREADS), B);
    hipLaunchKernelGGL((dua::aug_apply_kernel<1, dua::SMOOTH_NONE>), grid, dim3(dua::AUG_THREADS), 0, s, table, nvol, params,
                       roi_d, roi_h, roi_w, class_ids, C, images, labels, status, dua::AugSmooth{});
  }
  return (int)hipGetLastError();
}

int dua_aug_class_centroids(const unsigned char* label, int D, int H, int W, int num_classes, unsigned long long* sums,
                            float* centroids, void* stream) {
  if (!label || ((size_t)label & 15) || D < 1 || H < 1 || W < 1 || num_classes < 1 || num_classes > dua::CEN_MAX_CLASSES ||
      !sums || !centroids)
    return DUA_ERR_ARG;
  const long voxels = (long)D * H * W;                    // three factors below 2^31: cannot wrap before the test below
  const long longest = D > H ? (D > W ? D : W) : (H > W ? H : W);
  if ((long)D * H >= (1L << 31) || voxels >= (1L << 31) || voxels * longest >= (1L << 53)) return DUA_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  const hipError_t e = hipMemsetAsync(sums, 0, sizeof(unsigned long long) * 4 * (num_classes + 1), s);
  if (e != hipSuccess) return (int)e;
  const long per_block = (long)dua::CEN_RUN * dua::CEN_THREADS;
  const long blocks = (voxels + per_block - 1) / per_block;
  hipLaunchKernelGGL(dua::aug_class_sums_kernel, dim3((unsigned)(blocks < dua::CEN_MAX_BLOCKS ? blocks : dua::CEN_MAX_BLOCKS)),
                     dim3(dua::CEN_THREADS), 0, s, label, voxels, H, W, num_classes, sums);
  hipLaunchKernelGGL(dua::aug_centroid_finish_kernel, dim3((num_classes + 63) / 64), dim3(64), 0, s, num_classes, sums, centroids);
  return (int)hipGetLastError();
}

int dua_aug_apply_smoothed(const dua_aug_volume* table, int nvol, const float* centroids, int num_classes,
                           const dua_aug_smoothing* smoothing, const int* params, int B, int roi_d, int roi_h, int roi_w,
                           const unsigned char* class_ids, int C, float* images, float* labels, int* status, void* stream) {
  if (!table || nvol < 1 || !params || B < 1 || B > 65535 || roi_d < 1 || roi_h < 1 || roi_w < 1 || !class_ids || C < 1 ||
      C > DUA_AUG_MAX_CLASSES || !images || !labels || !centroids || num_classes < 1 || num_classes > dua::CEN_MAX_CLASSES ||
      !smoothing)
    return DUA_ERR_ARG;
  const dua_aug_smoothing p = *smoothing;
  // every comparison is false for a NaN.  epsilon is a normal number, so that 1 / (dist^order + epsilon) stays finite and
  // alpha = 0 gives exactly 0
  if (!(p.alpha >= 0.f && p.alpha <= 3.0e38f) || !(p.order > 0.f && p.order <= 3.0e38f) ||
      !(p.epsilon >= 1.17549435e-38f && p.epsilon <= 3.0e38f) || !(p.max_value > 0.f))
    return DUA_ERR_ARG;
  const long vox = (long)roi_d * roi_h * roi_w;
  if (vox >= (1L << 31)) return DUA_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  const dua::AugSmooth sm{centroids, num_classes, p.alpha, p.order, p.epsilon, p.max_value};
  const bool wide = roi_w % 4 == 0 && ((size_t)images & 15) == 0 && ((size_t)labels & 15) == 0;
  const bool pw = p.order != 1.f;
  const dim3 grid((unsigned)(((wide ? vox / 4 : vox) + dua::AUG_THREADS - 1) / dua::AUG_THREADS), B);
#define DUA_AUG_SMOOTHED(V, MODE)                                                                                              \
  hipLaunchKernelGGL((dua::aug_apply_kernel<V, MODE>), grid, dim3(dua::AUG_THREADS), 0, s, table, nvol, params, roi_d, roi_h, \
                     roi_w, class_ids, C, images, labels, status, sm)
  if (wide && !pw) DUA_AUG_SMOOTHED(4, dua::SMOOTH_ORDER1);
  else if (wide) DUA_AUG_SMOOTHED(4, dua::SMOOTH_POW);
  else if (!pw) DUA_AUG_SMOOTHED(1, dua::SMOOTH_ORDER1);
  else DUA_AUG_SMOOTHED(1, dua::SMOOTH_POW);
#undef DUA_AUG_SMOOTHED
  return (int)hipGetLastError();
}

}  // extern "C"
