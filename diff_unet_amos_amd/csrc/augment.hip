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
//   apply  : ONE kernel template, aug_apply_kernel<V, MODE, AFFINE>, behind every apply entry point; one host launcher holds the
//            argument checks and chooses the instantiation.  All forms share the store side: a lane owns 4 consecutive output
//            voxels along w (1 where roi_w or an output pointer rules out 16-byte stores) and writes one 16-byte store into the
//            image plane and into each of the C label planes; a wave-instruction covers 1 KiB of one plane.  The flip / rot90
//            index code, the row checks and the smoothed channel are device functions.  Two read sides (AFFINE):
//            rows   : a pure store-bandwidth kernel (per voxel: 4 + 1 bytes read, 4 (1 + C) written).  The rotation by k is in the
//                     (d, h) plane, so an output row along w is always one source row, forwards or backwards: a lane reads the
//                     4 floats and 4 label bytes of its voxels.
//            gather : random rotation and zoom, through the affine rows of the draw.  8 image loads and 1 label byte per voxel
//                     from a source region of a few MB that neighbouring lanes share.  A workgroup covers a compact 4 x 8 x 32
//                     tile of the output (a wave one 8 x 32 piece of a plane, a 128-byte line per row and store), not a run of
//                     1 024 voxels: under a rotation an output row crosses a source line every few voxels, and it is the rows
//                     beside, above and below it that use the rest of those lines (measured: DESIGN.md 10c-1).
//            Three label bodies (MODE): the one-hot channel, or the centroid-distance smoothed channel with or without pow.  The
//            read side leaves the source position of each voxel; the centroids of the row's volume sit in LDS (one broadcast
//            read per channel), and a channel costs 4 x (sub, fma, sqrt, add, rcp, mul, sub, min) before its 16-byte store.
//   centroids : once per volume, for label smoothing (dataset/cache_dataset.py:105-153).  One pass over the label map, 16 bytes
//            per thread and step; count and index sums per class as 64-bit integers, LDS atomics inside a workgroup, one
//            global integer atomic per class and workgroup: exact, so identical between runs.  A finish launch divides in fp64.
//   class count : once per volume, when crop centres are drawn by class: the same chunks, one prefix row per class, one pass.
//   class draw : the draw kernel's CLASSES form: a ballot over cum picks the class, the same search runs on that class's row.
//   affine draw : the draw kernel's AFFINE form takes two more Philox blocks and writes, beside the params row, the matrix
//            M = R / z from half-angle tangents in fp64 (no sine, no cosine: a numpy restatement has its bits).
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

__device__ __forceinline__ bool is_class_candidate(int k, unsigned char l, float v, float thr) {
  return (int)l == k && (k != 0 || v > thr);
}

// counts[k][c] = candidates of class k in chunk c, all K rows from one pass over label and image.  Ballots, but over the ids
// a wave actually holds, not over all K: the lowest lane still to be counted names an id, one ballot finds every lane with
// that id, its popcount goes to the workgroup's LDS row in ONE integer add from that lane.  A label map is piecewise constant,
// so 64 consecutive voxels hold one to three ids and a step costs that many ballots, where a ballot per class would cost K = 64
// of them for every 64 voxels; a per-lane LDS histogram would send the 64 adds of a wave to the same word (same-address LDS
// atomics are taken one after another).  Integer adds: the counts do not depend on the order of arrival.
__global__ void __launch_bounds__(AUG_THREADS) aug_class_chunk_counts_kernel(const float* __restrict__ image,
                                                                             const unsigned char* __restrict__ label, long voxels,
                                                                             float thr, int nchunks, int K,
                                                                             unsigned* __restrict__ prefix) {
  __shared__ unsigned hist[DUA_AUG_MAX_CLASSES];
  const int c = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  if (tid < K) hist[tid] = 0;                             // K <= DUA_AUG_MAX_CLASSES < AUG_THREADS
  __syncthreads();
#pragma unroll
  for (int j = 0; j < DUA_AUG_CHUNK / AUG_THREADS; ++j) {
    const long i = (long)c * DUA_AUG_CHUNK + j * AUG_THREADS + tid;
    int id = i < voxels ? (int)label[i] : -1;             // -1: in no set
    if (id == 0 && !(image[i] > thr)) id = -1;
    if (id >= K) id = -1;
    unsigned long long todo = __ballot(id >= 0);
    while (todo) {                                        // wave-uniform
      const int leader = __ffsll((long long)todo) - 1;
      const int cur = __shfl(id, leader);
      const unsigned long long same = __ballot(id == cur);
      if (lane == leader) atomicAdd(&hist[cur], (unsigned)__popcll(same));       // 0 <= cur < K
      todo &= ~same;
    }
  }
  __syncthreads();
  if (tid < K) prefix[(long)tid * (nchunks + 1) + c] = hist[tid];
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

// one row of dua_aug_draw_affine's second output: M = R_d R_h R_w / z from the half-angle tangents, every operation one IEEE
// fp64 operation in the order include/dua_hip.h writes them (this file compiles without contraction), rounded once to fp32
__device__ void aug_affine_row(float* __restrict__ dst, const float t[3], float z, int events, float pad) {
  double c[3], s[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double td = (double)t[a], q = td * td, n = 1.0 + q;
    c[a] = (1.0 - q) / n;
    s[a] = (td + td) / n;
  }
  const double cd = c[0], ch = c[1], cw = c[2], sd = s[0], sh = s[1], sw = s[2];
  const double R[9] = {ch * cw, 0.0 - (ch * sw), sh,
                       (cd * sw) + (sd * (sh * cw)), (cd * cw) - (sd * (sh * sw)), 0.0 - (sd * ch),
                       (sd * sw) - (cd * (sh * cw)), (sd * cw) + (cd * (sh * sw)), cd * ch};
  const double g = 1.0 / (double)z;
#pragma unroll
  for (int j = 0; j < 9; ++j) dst[DUA_AUG_AFFINE_M + j] = (float)(R[j] * g);
#pragma unroll
  for (int a = 0; a < 3; ++a) dst[DUA_AUG_AFFINE_T + a] = t[a];
  dst[DUA_AUG_AFFINE_ZOOM] = z;
  reinterpret_cast<int*>(dst)[DUA_AUG_AFFINE_EVENTS] = events;
  dst[DUA_AUG_AFFINE_PAD] = pad;
  dst[DUA_AUG_AFFINE_PAD + 1] = 0.f;
}

// what dua_aug_draw_classes adds to a draw (unread by the other entries)
struct AugClassDraw {
  const dua_aug_class_volume* classes;                    // may be NULL: the pos / neg rule
  int K;
  float uniform_prob;
  int* chosen;                                            // [B], may be NULL
  unsigned long long* tally;                              // [K + 1], may be NULL
};

// a row that cannot be drawn: volume -1, zeros, *status
__device__ __forceinline__ void aug_bad_row(int* __restrict__ row, int* status) {
  row[DUA_AUG_VOLUME] = -1;
  for (int j = 1; j < DUA_AUG_PARAM_WORDS; ++j) row[j] = 0;
  if (status) *status = 1;
}

// the params row of a sample whose centre is the voxel with linear index i of its volume
__device__ __forceinline__ void aug_write_row(int* __restrict__ row, int vid, long i, const dua_aug_volume& vol,
                                              const dua_aug_config& cfg, int flip, int k, float scale, float shift) {
  const unsigned line = (unsigned)i / (unsigned)vol.W;    // voxels < 2^31
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

// AFFINE: dua_aug_draw_affine -- two more Philox blocks per sample and the affine row beside the params row, which keeps its bits
// CLASSES: dua_aug_draw_classes -- word 2.3 decides the uniform event (a voxel of the whole volume, no table), otherwise the
// candidate set is a class: lane k holds cum[k], one ballot of u < cum[k] and its lowest bit give the class, and the search below
// runs on row k of the volume's class table.  Every branch on these is wave-uniform.  Without a class table the set is the pos /
// neg one, and with uniform_prob = 0 besides, the row has the bits of the CLASSES = false form.
template <bool AFFINE, bool CLASSES>
__global__ void __launch_bounds__(AUG_DRAW_WAVES * 64) aug_draw_kernel(const dua_aug_volume* __restrict__ table, int nvol,
                                                                      const int* __restrict__ ids, int B, dua_aug_config cfg,
                                                                      unsigned long long seed, unsigned long long* counter,
                                                                      int use_counter, unsigned long long counter_value,
                                                                      int* __restrict__ params, int* status,
                                                                      dua_aug_affine_config acfg, float* __restrict__ affine,
                                                                      AugClassDraw cls) {
  const float no_turn[3] = {0.f, 0.f, 0.f};
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long call = use_counter ? counter_value : *counter;
  __syncthreads();                                        // every wave holds the call counter before one lane moves it on
  if (!use_counter && threadIdx.x == 0) *counter = call + 1;
  for (int b = wave; b < B; b += AUG_DRAW_WAVES) {
    int* row = params + (long)b * DUA_AUG_PARAM_WORDS;
    const int vid = ids[b];
    float* arow = AFFINE ? affine + (long)b * DUA_AUG_AFFINE_WORDS : nullptr;
    if (vid < 0 || vid >= nvol) {
      if (lane == 0) {
        aug_bad_row(row, status);
        if constexpr (AFFINE) aug_affine_row(arow, no_turn, 1.f, 0, acfg.pad_value);
        if constexpr (CLASSES) if (cls.chosen) cls.chosen[b] = -2;
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
    uint32_t count = fg ? vol.fg_count : vol.bg_count;
    const unsigned* prefix = fg ? vol.fg_prefix : vol.bg_prefix;
    int cclass = -1;                                      // the chosen class; -1: the pos / neg set
    bool uniform = false;
    if constexpr (CLASSES) {
      uniform = unit_float(w[2][3]) < cls.uniform_prob;
      if (!uniform && cls.classes) {
        const dua_aug_class_volume cv = cls.classes[vid];
        const float u = unit_float(w[0][0]);
        const bool below_cum = lane < cls.K && u < cv.cum[lane < cls.K ? lane : 0];      // K <= 64: a lane per class
        const unsigned long long m = __ballot(below_cum);
        cclass = m ? __ffsll((long long)m) - 1 : cls.K;   // K: a cum that chooses nothing
        prefix = cv.prefix + (long)min(cclass, cls.K - 1) * (vol.nchunks + 1);
        count = cclass < cls.K ? prefix[vol.nchunks] : 0u;
      }
    }
    const long voxels = (long)vol.D * vol.H * vol.W;
    const uint32_t r = below(w[0][1], uniform ? (uint32_t)voxels : count);
    int flip = 0;
    flip |= unit_float(w[0][2]) < cfg.flip_prob ? 1 : 0;
    flip |= unit_float(w[0][3]) < cfg.flip_prob ? 2 : 0;
    flip |= unit_float(w[1][0]) < cfg.flip_prob ? 4 : 0;
    const int k = unit_float(w[1][1]) < cfg.rot90_prob ? 1 + (int)below(w[1][2], (uint32_t)cfg.max_k) : 0;
    const float scale = unit_float(w[1][3]) < cfg.scale_prob ? symmetric(cfg.scale_factors, w[2][0]) : 0.f;
    const float shift = unit_float(w[2][1]) < cfg.shift_prob ? symmetric(cfg.shift_offsets, w[2][2]) : 0.f;
    float turn[3] = {0.f, 0.f, 0.f}, zoom = 1.f;
    int events = 0;
    if constexpr (AFFINE) {
      uint32_t x[2][4];
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        x[j][0] = (uint32_t)call; x[j][1] = (uint32_t)(call >> 32); x[j][2] = (uint32_t)b; x[j][3] = (uint32_t)(3 + j);
        philox4x32_10(x[j], (uint32_t)seed, (uint32_t)(seed >> 32));
      }
      if (unit_float(x[0][0]) < acfg.rotate_prob) {
        events |= 1;
#pragma unroll
        for (int a = 0; a < 3; ++a) turn[a] = symmetric(acfg.rotate_tan_half[a], x[0][1 + a]);
      }
      if (unit_float(x[1][0]) < acfg.zoom_prob) {
        events |= 2;
        const float t = acfg.zoom_span * unit_float(x[1][1]);
        zoom = t + acfg.zoom_min;
      }
    }
    bool written = false;
    if (uniform) {                                        // voxel number r of the whole volume: no table, no scan
      if (lane == 0) aug_write_row(row, vid, (long)r, vol, cfg, flip, k, scale, shift);
      written = true;
    } else if (count > 0) {                               // count == 0: a table row the host should never have built
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
      for (int j = 0; j < DUA_AUG_CHUNK / 64; ++j) {
        const long i = (long)lo * DUA_AUG_CHUNK + j * 64 + lane;
        const bool in = i < voxels;
        const unsigned char l = vol.label[in ? i : 0];
        const float v = vol.image[in ? i : 0];
        const bool cand = in && (CLASSES && cclass >= 0 ? is_class_candidate(cclass, l, v, vol.image_threshold)
                                                        : is_candidate(fg, l, v, vol.image_threshold));
        const unsigned long long m = __ballot(cand);
        const uint32_t n = __popcll(m);
        if (rem < n) {
          const uint32_t rank = __popcll(m & ((1ull << lane) - 1ull));
          if (cand && rank == rem) aug_write_row(row, vid, i, vol, cfg, flip, k, scale, shift);
          written = true;
          break;
        }
        rem -= n;
      }
    }
    if (lane == 0) {
      if (!written) aug_bad_row(row, status);             // an empty set, or the prefix table and the volume disagree
      if constexpr (AFFINE) {
        if (written) aug_affine_row(arow, turn, zoom, events, acfg.pad_value);
        else aug_affine_row(arow, no_turn, 1.f, 0, acfg.pad_value);
      }
      if constexpr (CLASSES) {
        if (cls.chosen) cls.chosen[b] = !written ? -2 : uniform ? -1 : cclass;
        if (cls.tally && written && (uniform || cclass >= 0)) atomicAdd(&cls.tally[uniform ? cls.K : cclass], 1ull);
      }
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

// what every apply kernel checks of its params row before it reads or writes anything (block-uniform); vol = the row's volume
__device__ __forceinline__ bool aug_row_ok(const dua_aug_volume* __restrict__ table, int nvol, const int* __restrict__ row, int Rd,
                                           int Rh, int Rw, dua_aug_volume& vol) {
  const int vid = row[DUA_AUG_VOLUME], sd0 = row[DUA_AUG_START_D], sh0 = row[DUA_AUG_START_H], sw0 = row[DUA_AUG_START_W];
  const int flip = row[DUA_AUG_FLIP], k = row[DUA_AUG_K];
  bool ok = vid >= 0 && vid < nvol && (unsigned)flip < 8u && (unsigned)k < 4u && (!(k & 1) || Rd == Rh);
  if (ok) {
    vol = table[vid];
    ok = sd0 >= 0 && sh0 >= 0 && sw0 >= 0 && sd0 <= vol.D - Rd && sh0 <= vol.H - Rh && sw0 <= vol.W - Rw;
  }
  return ok;
}

// the smoothed forms: the centroid of class_ids[ch] in volume vid into cen[ch]; false (block-uniform) for an id without a row
__device__ __forceinline__ bool aug_stage_centroids(float (*cen)[4], int* bad_id, int vid, const unsigned char* __restrict__ class_ids,
                                                    int C, const AugSmooth& sm) {
  if (threadIdx.x == 0) *bad_id = 0;
  __syncthreads();
  if ((int)threadIdx.x < C) {                             // C <= DUA_AUG_MAX_CLASSES < AUG_THREADS
    const int id = class_ids[threadIdx.x];
    if (id < sm.K) {
      const float* c3 = sm.centroids + ((long)vid * sm.K + id) * 3;
      cen[threadIdx.x][0] = c3[0]; cen[threadIdx.x][1] = c3[1]; cen[threadIdx.x][2] = c3[2];
    } else {
      *bad_id = 1;
    }
  }
  __syncthreads();
  return *bad_id == 0;
}

// linear output voxel o -> its position (od, oh, ow)
__device__ __forceinline__ void aug_output_position(unsigned o, int Rh, int Rw, int& od, int& oh, int& ow) {
  const unsigned orow = o / (unsigned)Rw;
  ow = (int)(o - orow * (unsigned)Rw); od = (int)(orow / (unsigned)Rh); oh = (int)(orow - (unsigned)od * (unsigned)Rh);
}

// output row (od, oh) -> the window indices (a, c) along d and h of the source row it comes from, for every (flip, k); along w the
// row runs forwards, or backwards with flip bit 2.  The one copy of the flip / rot90 index code.
__device__ __forceinline__ void aug_window_row(int od, int oh, int k, int flip, int Rd, int Rh, int& a, int& c) {
  // inverse of rot90(., k, (0, 1)): k = 1: out[i][j] = x[j][n - 1 - i]; k = 2: x[n0 - 1 - i][n1 - 1 - j]; k = 3: x[n - 1 - j][i]
  switch (k) {
    case 1: a = oh; c = Rh - 1 - od; break;
    case 2: a = Rd - 1 - od; c = Rh - 1 - oh; break;
    case 3: a = Rd - 1 - oh; c = od; break;
    default: a = od; c = oh; break;
  }
  if (flip & 1) a = Rd - 1 - a;
  if (flip & 2) c = Rh - 1 - c;
}

// one smoothed label value: onehot = [label == class], (dw, t) = the w difference and dd^2 + dh^2 against the class centroid
template <int MODE>
__device__ __forceinline__ float aug_smoothed(float onehot, float dw, float t, const AugSmooth& sm) {
  const float dist = __builtin_amdgcn_sqrtf(__builtin_fmaf(dw, dw, t));
  const float p = MODE == SMOOTH_POW ? powf(dist, sm.order) : dist;
  const float s = __builtin_amdgcn_rcpf(p + sm.epsilon) * sm.alpha;
  return fminf(fabsf(onehot - s), sm.max_value);
}

constexpr int AFF_TILE_D = 4, AFF_TILE_H = 8, AFF_TILE_W = 32;
static_assert(AFF_TILE_D * AFF_TILE_H * AFF_TILE_W == 4 * AUG_THREADS && AFF_TILE_W % 4 == 0, "one tile per workgroup, 4 voxels per lane");

// floorf(s) as an index that can be compared and incremented: clamped to [-2, 2^31 - 128] first, where the clamp only moves an
// index that lies outside every volume to another one that does (a NaN becomes -2)
__device__ __forceinline__ int aug_floor_index(float fl) { return (int)fminf(fmaxf(fl, -2.f), 2147483520.f); }

// The one apply kernel.  A lane owns V consecutive output voxels of a row along w (4: roi_w is a multiple of 4, so a group never
// crosses a row and every store is 16-byte aligned) and writes one store into the image plane and into each label plane.
// MODE: what a label plane holds -- SMOOTH_NONE: the one-hot channel; SMOOTH_ORDER1 / SMOOTH_POW: the centroid-distance
// smoothed channel (order == 1 without pow), evaluated at the source position (jd, jh, jw) of each voxel.
// AFFINE: how an output voxel finds its source values.  false: the index code gives the source row, 1 float and 1 label byte per
// voxel, forwards or backwards along it; `affine` is unread.  true: a gather -- per voxel the 8 corners of the trilinear cell
// around s = M r + c and the label byte at the nearest voxel.  The window index p of an output voxel comes from the same index
// code, so flips and k apply after the resampling.  The products with r_d and r_h and their sum are the same numbers for the V
// voxels of a lane: computed once, they are the bits each voxel would get from scratch; nothing is carried along the row.
template <int V, int MODE, bool AFFINE>
__global__ void __launch_bounds__(AUG_THREADS) aug_apply_kernel(const dua_aug_volume* __restrict__ table, int nvol,
                                                               const int* __restrict__ params, const float* __restrict__ affine,
                                                               int Rd, int Rh, int Rw, const unsigned char* __restrict__ class_ids,
                                                               int C, float* __restrict__ images, float* __restrict__ labels,
                                                               int* status, AugSmooth sm) {
  using Vec = typename OutVec<V>::T;
  __shared__ float cen[MODE == SMOOTH_NONE ? 1 : DUA_AUG_MAX_CLASSES][4];      // centroid of class_ids[ch] in the row's volume
  __shared__ int bad_id;
  const int b = blockIdx.y;
  const int* row = params + (long)b * DUA_AUG_PARAM_WORDS;
  const int vid = row[DUA_AUG_VOLUME], sd0 = row[DUA_AUG_START_D], sh0 = row[DUA_AUG_START_H], sw0 = row[DUA_AUG_START_W];
  const int flip = row[DUA_AUG_FLIP], k = row[DUA_AUG_K];
  dua_aug_volume vol = {};
  if (!aug_row_ok(table, nvol, row, Rd, Rh, Rw, vol)) {   // block-uniform: nothing is read, nothing is written
    if (status && blockIdx.x == 0 && threadIdx.x == 0) *status = 1;
    return;
  }
  if constexpr (MODE != SMOOTH_NONE) {
    if (!aug_stage_centroids(cen, &bad_id, vid, class_ids, C, sm)) {       // block-uniform again: a class id without a centroid row
      if (status && blockIdx.x == 0 && threadIdx.x == 0) *status = 1;
      return;
    }
  }
  const long vox = (long)Rd * Rh * Rw;
  int od, oh, ow, a, c;
  unsigned o;                                             // first output voxel of this lane (vox < 2^31)
  if constexpr (AFFINE && V == 4) {
    // a workgroup covers a compact AFF_TILE_D x AFF_TILE_H x AFF_TILE_W tile of the output, a wave one 8 x 32 piece of a plane:
    // under a rotation the rows of a tile read neighbouring source lines, which the CU's L1 then holds for all of them
    const unsigned tiles_w = (Rw + AFF_TILE_W - 1) / AFF_TILE_W, tiles_h = (Rh + AFF_TILE_H - 1) / AFF_TILE_H;
    const unsigned tw = blockIdx.x % tiles_w, trow = blockIdx.x / tiles_w, th = trow % tiles_h, td = trow / tiles_h;
    const unsigned lw = threadIdx.x % (AFF_TILE_W / 4), lrow = threadIdx.x / (AFF_TILE_W / 4);
    ow = (int)(tw * AFF_TILE_W + lw * 4); oh = (int)(th * AFF_TILE_H + lrow % AFF_TILE_H); od = (int)(td * AFF_TILE_D + lrow / AFF_TILE_H);
    if (od >= Rd || oh >= Rh || ow >= Rw) return;          // roi_w is a multiple of 4: a lane's voxels are all inside or all outside
    o = ((unsigned)od * (unsigned)Rh + (unsigned)oh) * (unsigned)Rw + (unsigned)ow;
  } else {
    o = (blockIdx.x * (unsigned)AUG_THREADS + threadIdx.x) * V;
    if (o >= vox) return;
    aug_output_position(o, Rh, Rw, od, oh, ow);
  }
  aug_window_row(od, oh, k, flip, Rd, Rh, a, c);
  const bool fw = (flip & 4) != 0;
  const float factor = 1.f + __int_as_float(row[DUA_AUG_SCALE]);
  const float shift = __int_as_float(row[DUA_AUG_SHIFT]);
  float px[V], jd[V], jh[V], jw[V];                       // the source value and the position the smoothed forms take
  unsigned char lb[V];
  if constexpr (AFFINE) {
    const float* arow = affine + (long)b * DUA_AUG_AFFINE_WORDS;
    float m[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) m[j] = arow[DUA_AUG_AFFINE_M + j];
    const float pad = arow[DUA_AUG_AFFINE_PAD];
    const float hd = 0.5f * (float)(Rd - 1), hh = 0.5f * (float)(Rh - 1), hw = 0.5f * (float)(Rw - 1);      // exact
    const float cd = (float)sd0 + hd, chh = (float)sh0 + hh, cw = (float)sw0 + hw;
    const float rd = (float)a - hd, rh = (float)c - hh;
    const float qd = m[0] * rd + m[1] * rh, qh = m[3] * rd + m[4] * rh, qw = m[6] * rd + m[7] * rh;
    const unsigned D = (unsigned)vol.D, H = (unsigned)vol.H, W = (unsigned)vol.W;
#pragma unroll
    for (int e = 0; e < V; ++e) {
      const float rw = (float)(fw ? Rw - 1 - (ow + e) : ow + e) - hw;
      const float s0 = (qd + m[2] * rw) + cd, s1 = (qh + m[5] * rw) + chh, s2 = (qw + m[8] * rw) + cw;
      const float l0 = floorf(s0), l1 = floorf(s1), l2 = floorf(s2);
      const float f0 = s0 - l0, f1 = s1 - l1, f2 = s2 - l2;
      const int i0 = aug_floor_index(l0), i1 = aug_floor_index(l1), i2 = aug_floor_index(l2);
      float cor[2][2][2];
#pragma unroll
      for (int ed = 0; ed < 2; ++ed)
#pragma unroll
        for (int eh = 0; eh < 2; ++eh)
#pragma unroll
          for (int ew = 0; ew < 2; ++ew) {
            const unsigned d = (unsigned)(i0 + ed), h = (unsigned)(i1 + eh), w = (unsigned)(i2 + ew);
            const bool in = d < D && h < H && w < W;      // a negative index is a huge unsigned one
            cor[ed][eh][ew] = in ? vol.image[((long)d * vol.H + h) * vol.W + w] : pad;
          }
      float y[2];
#pragma unroll
      for (int ed = 0; ed < 2; ++ed) {
        const float x0 = __builtin_fmaf(f2, cor[ed][0][1] - cor[ed][0][0], cor[ed][0][0]);
        const float x1 = __builtin_fmaf(f2, cor[ed][1][1] - cor[ed][1][0], cor[ed][1][0]);
        y[ed] = __builtin_fmaf(f1, x1 - x0, x0);
      }
      px[e] = __builtin_fmaf(f0, y[1] - y[0], y[0]);
      const int n0 = f0 >= 0.5f ? 1 : 0, n1 = f1 >= 0.5f ? 1 : 0, n2 = f2 >= 0.5f ? 1 : 0;
      const unsigned d = (unsigned)(i0 + n0), h = (unsigned)(i1 + n1), w = (unsigned)(i2 + n2);
      lb[e] = (d < D && h < H && w < W) ? vol.label[((long)d * vol.H + h) * vol.W + w] : (unsigned char)0;
      jd[e] = l0 + (float)n0; jh[e] = l1 + (float)n1; jw[e] = l2 + (float)n2;      // the nearest voxel, unclamped
    }
  } else {
    const long src = ((long)(sd0 + a) * vol.H + (sh0 + c)) * vol.W + sw0;   // start of the source row's window
#pragma unroll
    for (int e = 0; e < V; ++e) {
      const int sw = fw ? Rw - 1 - (ow + e) : ow + e;
      px[e] = vol.image[src + sw];
      lb[e] = vol.label[src + sw];
      // the source index (sd0 + a, sh0 + c, sw0 + sw); fp32 holds it exactly for extents up to 2^24
      jd[e] = (float)(sd0 + a); jh[e] = (float)(sh0 + c); jw[e] = (float)(sw0 + sw);
    }
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
  constexpr int PLANES_UNROLL = MODE == SMOOTH_NONE && !AFFINE ? 4 : 2;
#pragma unroll PLANES_UNROLL
  for (int ch = 0; ch < C; ++ch) {
    const unsigned char id = class_ids[ch];
    float mv[V];
#pragma unroll
    for (int e = 0; e < V; ++e) {
      const float onehot = lb[e] == id ? 1.f : 0.f;
      if constexpr (MODE == SMOOTH_NONE) {
        mv[e] = onehot;
      } else {
        const float dd = jd[e] - cen[ch][0], dh = jh[e] - cen[ch][1];
        mv[e] = aug_smoothed<MODE>(onehot, jw[e] - cen[ch][2], dd * dd + dh * dh, sm);
      }
    }
    if constexpr (V == 4) {
      Vec out;
#pragma unroll
      for (int e = 0; e < 4; ++e) out[e] = mv[e];
      *reinterpret_cast<Vec*>(lab + (long)ch * vox) = out;
    } else {
      *(lab + (long)ch * vox) = mv[0];
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

// dua_aug_draw (affine_cfg == NULL and affine == NULL), dua_aug_draw_affine (both given) and, with cls, dua_aug_draw_classes
// (either)
static int aug_draw_launch(const dua_aug_volume* table, int nvol, const int* ids, int B, const dua_aug_config* cfg,
                           const dua_aug_affine_config* affine_cfg, unsigned long long seed, unsigned long long* counter,
                           int use_counter, unsigned long long counter_value, int* params, float* affine, int* status,
                           const dua::AugClassDraw* cls, void* stream) {
  if (!table || nvol < 1 || !ids || B < 1 || !cfg || !params || (!use_counter && !counter)) return DUA_ERR_ARG;
  if (cfg->roi[0] < 1 || cfg->roi[1] < 1 || cfg->roi[2] < 1 || cfg->max_k < 1 || cfg->max_k > 3) return DUA_ERR_ARG;
  if (!dua::prob_ok(cfg->pos_fraction) || !dua::prob_ok(cfg->flip_prob) || !dua::prob_ok(cfg->rot90_prob) ||
      !dua::prob_ok(cfg->scale_prob) || !dua::prob_ok(cfg->shift_prob) || !(cfg->scale_factors >= 0.f) ||
      !(cfg->shift_offsets >= 0.f) || (cfg->rot90_prob > 0.f && cfg->roi[0] != cfg->roi[1]))
    return DUA_ERR_ARG;
  dua_aug_affine_config a{};
  if (affine_cfg) {
    a = *affine_cfg;
    // every comparison is false for a NaN
    if (!dua::prob_ok(a.rotate_prob) || !dua::prob_ok(a.zoom_prob) || !(a.zoom_min > 0.f && a.zoom_min <= 3.0e38f) ||
        !(a.zoom_span >= 0.f && a.zoom_span <= 3.0e38f) || !(a.pad_value >= -3.0e38f && a.pad_value <= 3.0e38f))
      return DUA_ERR_ARG;
    for (int i = 0; i < 3; ++i)
      if (!(a.rotate_tan_half[i] >= 0.f && a.rotate_tan_half[i] <= 1.f)) return DUA_ERR_ARG;
  }
  const int waves = B < dua::AUG_DRAW_WAVES ? B : dua::AUG_DRAW_WAVES;
  const auto kernel = cls ? (affine_cfg ? dua::aug_draw_kernel<true, true> : dua::aug_draw_kernel<false, true>)
                          : (affine_cfg ? dua::aug_draw_kernel<true, false> : dua::aug_draw_kernel<false, false>);
  hipLaunchKernelGGL(kernel, dim3(1), dim3(waves * 64), 0, (hipStream_t)stream, table, nvol, ids, B, *cfg, seed, counter,
                     use_counter, counter_value, params, status, a, affine, cls ? *cls : dua::AugClassDraw{});
  return (int)hipGetLastError();
}

// every apply entry point: affine == NULL reads whole source rows, otherwise through the affine rows; smoothing == NULL gives
// one-hot label planes, otherwise the smoothed ones from centroids
static int aug_apply_launch(const dua_aug_volume* table, int nvol, const float* centroids, int num_classes,
                            const dua_aug_smoothing* smoothing, const int* params, const float* affine, int B, int roi_d,
                            int roi_h, int roi_w, const unsigned char* class_ids, int C, float* images, float* labels,
                            int* status, void* stream) {
  if (!table || nvol < 1 || !params || B < 1 || B > 65535 || roi_d < 1 || roi_h < 1 || roi_w < 1 || !class_ids || C < 1 ||
      C > DUA_AUG_MAX_CLASSES || !images || !labels)
    return DUA_ERR_ARG;
  dua::AugSmooth sm{};
  int mode = dua::SMOOTH_NONE;
  if (smoothing) {
    const dua_aug_smoothing p = *smoothing;
    // every comparison is false for a NaN.  epsilon is a normal number, so that 1 / (dist^order + epsilon) stays finite and
    // alpha = 0 gives exactly 0
    if (num_classes < 1 || num_classes > dua::CEN_MAX_CLASSES || !(p.alpha >= 0.f && p.alpha <= 3.0e38f) ||
        !(p.order > 0.f && p.order <= 3.0e38f) || !(p.epsilon >= 1.17549435e-38f && p.epsilon <= 3.0e38f) || !(p.max_value > 0.f))
      return DUA_ERR_ARG;
    sm = dua::AugSmooth{centroids, num_classes, p.alpha, p.order, p.epsilon, p.max_value};
    mode = p.order != 1.f ? dua::SMOOTH_POW : dua::SMOOTH_ORDER1;
  }
  const long vox = (long)roi_d * roi_h * roi_w;
  if (vox >= (1L << 31)) return DUA_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  // 16-byte stores need every plane and every row to start on a 16-byte boundary
  const bool wide = roi_w % 4 == 0 && ((size_t)images & 15) == 0 && ((size_t)labels & 15) == 0;
  long blocks = ((wide ? vox / 4 : vox) + dua::AUG_THREADS - 1) / dua::AUG_THREADS;     // a lane per 4 (1) voxels in linear order
  if (wide && affine)                                     // a tile per workgroup: at most vox, which is below 2^31
    blocks = (long)((roi_d + dua::AFF_TILE_D - 1) / dua::AFF_TILE_D) * ((roi_h + dua::AFF_TILE_H - 1) / dua::AFF_TILE_H) *
             ((roi_w + dua::AFF_TILE_W - 1) / dua::AFF_TILE_W);
  const dim3 grid((unsigned)blocks, B);
#define DUA_AUG_APPLY(V, MODE, AFFINE)                                                                                          \
  hipLaunchKernelGGL((dua::aug_apply_kernel<V, MODE, AFFINE>), grid, dim3(dua::AUG_THREADS), 0, s, table, nvol, params, affine, \
                     roi_d, roi_h, roi_w, class_ids, C, images, labels, status, sm)
#define DUA_AUG_APPLY_A(V, MODE) if (affine) DUA_AUG_APPLY(V, MODE, true); else DUA_AUG_APPLY(V, MODE, false)
#define DUA_AUG_APPLY_V(MODE) if (wide) { DUA_AUG_APPLY_A(4, MODE); } else { DUA_AUG_APPLY_A(1, MODE); }
  switch (mode) {
    case dua::SMOOTH_NONE: DUA_AUG_APPLY_V(dua::SMOOTH_NONE) break;
    case dua::SMOOTH_ORDER1: DUA_AUG_APPLY_V(dua::SMOOTH_ORDER1) break;
    default: DUA_AUG_APPLY_V(dua::SMOOTH_POW) break;
  }
#undef DUA_AUG_APPLY_V
#undef DUA_AUG_APPLY_A
#undef DUA_AUG_APPLY
  return (int)hipGetLastError();
}

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
  return aug_draw_launch(table, nvol, ids, B, cfg, nullptr, seed, counter, use_counter, counter_value, params, nullptr, status,
                         nullptr, stream);
}

int dua_aug_apply(const dua_aug_volume* table, int nvol, const int* params, int B, int roi_d, int roi_h, int roi_w,
                  const unsigned char* class_ids, int C, float* images, float* labels, int* status, void* stream) {
  return aug_apply_launch(table, nvol, nullptr, 0, nullptr, params, nullptr, B, roi_d, roi_h, roi_w, class_ids, C, images, labels,
                          status, stream);
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
  if (!centroids || !smoothing) return DUA_ERR_ARG;
  return aug_apply_launch(table, nvol, centroids, num_classes, smoothing, params, nullptr, B, roi_d, roi_h, roi_w, class_ids, C,
                          images, labels, status, stream);
}

int dua_aug_draw_affine(const dua_aug_volume* table, int nvol, const int* ids, int B, const dua_aug_config* cfg,
                        const dua_aug_affine_config* affine_cfg, unsigned long long seed, unsigned long long* counter,
                        int use_counter, unsigned long long counter_value, int* params, float* affine, int* status,
                        void* stream) {
  if (!affine_cfg || !affine) return DUA_ERR_ARG;
  return aug_draw_launch(table, nvol, ids, B, cfg, affine_cfg, seed, counter, use_counter, counter_value, params, affine, status,
                         nullptr, stream);
}

int dua_aug_apply_affine(const dua_aug_volume* table, int nvol, const float* centroids, int num_classes,
                         const dua_aug_smoothing* smoothing, const int* params, const float* affine, int B, int roi_d,
                         int roi_h, int roi_w, const unsigned char* class_ids, int C, float* images, float* labels,
                         int* status, void* stream) {
  constexpr int max_extent = 1 << 22;                     // r and c of the contract are exact in fp32
  if (!affine || roi_d > max_extent || roi_h > max_extent || roi_w > max_extent || (centroids == nullptr) != (smoothing == nullptr))
    return DUA_ERR_ARG;
  return aug_apply_launch(table, nvol, centroids, num_classes, smoothing, params, affine, B, roi_d, roi_h, roi_w, class_ids, C,
                          images, labels, status, stream);
}

int dua_aug_count_class_candidates(const float* image, const unsigned char* label, long voxels, float image_threshold,
                                   int num_classes, unsigned* prefix, void* stream) {
  if (!image || !label || !prefix || voxels <= 0 || voxels >= (1L << 31) || image_threshold != image_threshold ||
      num_classes < 1 || num_classes > DUA_AUG_MAX_CLASSES)
    return DUA_ERR_ARG;
  const int nchunks = (int)((voxels + DUA_AUG_CHUNK - 1) / DUA_AUG_CHUNK);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(dua::aug_class_chunk_counts_kernel, dim3(nchunks), dim3(dua::AUG_THREADS), 0, s, image, label, voxels,
                     image_threshold, nchunks, num_classes, prefix);
  hipLaunchKernelGGL(dua::aug_prefix_scan_kernel, dim3(num_classes), dim3(dua::AUG_THREADS), 0, s, nchunks, prefix);
  return (int)hipGetLastError();
}

int dua_aug_draw_classes(const dua_aug_volume* table, int nvol, const int* ids, int B, const dua_aug_config* cfg,
                         const dua_aug_affine_config* affine_cfg, unsigned long long seed, unsigned long long* counter,
                         int use_counter, unsigned long long counter_value, int* params, float* affine, int* status,
                         const dua_aug_class_volume* classes, int num_classes, float uniform_prob, int* chosen,
                         unsigned long long* tally, void* stream) {
  if ((affine_cfg == nullptr) != (affine == nullptr) || !dua::prob_ok(uniform_prob)) return DUA_ERR_ARG;
  if (classes ? (num_classes < 1 || num_classes > DUA_AUG_MAX_CLASSES) : (chosen || tally)) return DUA_ERR_ARG;
  const dua::AugClassDraw cls{classes, classes ? num_classes : 0, uniform_prob, chosen, tally};
  return aug_draw_launch(table, nvol, ids, B, cfg, affine_cfg, seed, counter, use_counter, counter_value, params, affine, status,
                         &cls, stream);
}

}  // extern "C"
