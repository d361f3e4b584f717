// Signed distance maps of a label batch for the boundary loss (Kervadec et al., "Boundary loss for highly unbalanced
// segmentation"): per volume (n, c) the exact Euclidean distance transform of the mask { y > threshold } AND of its complement,
// unit spacing, as phi = sqrt(d2) outside and 1 - sqrt(d2) inside.  The contract is in include/dua_hip.h at dua_sdf_maps.
//
// One signed 32-bit word per voxel carries both transforms.  At every stage a voxel's partial distance to its OWN set is 0, so
// only the distance to the other set needs storing: the sign is the membership (negative = inside the mask), the magnitude the
// partial squared distance to the nearest voxel of the other set (>= 1: the voxel itself is not in it), or SDF_NONE when no such
// voxel has been seen yet.  Seen from a voxel of membership m, a line entry of the other membership is at partial distance 0
// and an entry of the same membership is at its own magnitude (its "other set" is the same set), hence
//   out(l) = min over l' of [ sign(l') != sign(l) ? 0 : mag(l') ] + (l - l')^2,
// the separable squared-distance recursion (W, then H, then D), exact in integers.
//
//   rows : W pass.  Reads the labels, thresholds, and finds the nearest entry of the other membership in the row by an outward
//          search over the row staged in LDS.  Writes the word.
//   cols : H pass and D pass, in place.  A workgroup stages whole lines of SDF_TW neighbouring columns ([L][TW] words, at most
//          32 KB), every thread searches outward from its entry and stops at k^2 >= best, as edt_cols_kernel of
//          csrc/surface.hip does in fp64.  The D pass converts: a magnitude still at SDF_NONE means the other set is empty in
//          the whole volume (phi = 0, d2 = 0); anything else is d2 < 2^24, exact in fp32.
//   A row or column that holds one membership and no distance yet has no candidate and keeps its words: it is not searched.
//   In a class's volume that is most lines (the class is a blob somewhere else), and each entry of one would walk to both ends.
// SDF_NONE = 2^30: SDF_NONE + 511^2 < 2^31, so a candidate built on it cannot wrap, and it is >= SDF_NONE, so the running
// minimum (which starts at the entry's own magnitude <= SDF_NONE) never rises above SDF_NONE.  A line is addressed inside its
// own volume only.  Integer minima: no atomics, no order dependence, the same inputs give the same bits; no host read.
#include "common.hpp"
#include "../../include/dua_hip.h"

namespace dua {

constexpr int SDF_NONE = 1 << 30;
constexpr int SDF_MAX_EXTENT = 512;
constexpr int SDF_ROW_WORDS = 1024;      // words of rows a workgroup of the W pass stages (whole rows; one row when W is larger)
constexpr int SDF_TILE_WORDS = 8192;     // words of lines a workgroup of the H / D pass stages: 32 KB
constexpr long SDF_MAX_GRID = 1L << 20;

__device__ __forceinline__ int sdf_mag(int w) { return w < 0 ? -w : w; }

// words: int32 [rows][W], WRITTEN.  A workgroup takes `rpb` consecutive rows (a contiguous piece of memory) at a time.
__global__ __launch_bounds__(256) void sdf_rows_kernel(const float* __restrict__ y, float threshold, long rows, int W, int rpb,
                                                       int* __restrict__ words) {
  __shared__ int in[SDF_ROW_WORDS];      // 1 inside the mask, 0 outside
  __shared__ int mixed[SDF_ROW_WORDS];   // per row: 1 when it holds both memberships (most rows of a class volume do not)
  const long groups = (rows + rpb - 1) / rpb;
  for (long g = blockIdx.x; g < groups; g += gridDim.x) {
    const long r0 = g * rpb;
    const int nr = (int)(rows - r0 < rpb ? rows - r0 : rpb), n = nr * W;
    const float* src = y + r0 * W;
    for (int i = threadIdx.x; i < n; i += 256) in[i] = src[i] > threshold;
    for (int i = threadIdx.x; i < nr; i += 256) mixed[i] = 0;
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += 256) {
      const int r = i / W;
      if (in[i] != in[r * W]) mixed[r] = 1;           // every writer stores the same value
    }
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += 256) {
      const int r = i / W, x = i - r * W;
      const int* row = in + r * W;
      const int m = row[x];
      int best = SDF_NONE;
      for (int k = 1; mixed[r] && k < W; ++k) {
        const bool lo = x >= k, hi = x + k < W;
        if (!lo && !hi) break;
        if ((lo && row[x - k] != m) || (hi && row[x + k] != m)) { best = k * k; break; }
      }
      words[r0 * W + i] = m ? -best : best;
    }
    __syncthreads();
  }
}

// One pass along an axis of extent L and stride lstride.  The lines of one "outer" slab start at ncols consecutive words
// (outer * ostride + j, j < ncols); a workgroup takes TW neighbouring columns, all L entries of each.  LAST: write phi (and
// d2 when asked) instead of the word.
template <bool LAST>
__global__ __launch_bounds__(256) void sdf_cols_kernel(int* __restrict__ words, long outer, int L, long lstride, long ostride,
                                                       long ncols, int TW, float* __restrict__ phi, int* __restrict__ d2) {
  extern __shared__ int f[];             // [L][TW]
  __shared__ int open[64];               // per column: 1 when a search can find something (TW <= 64)
  const long tpo = (ncols + TW - 1) / TW, tiles = outer * tpo;
  const int n = L * TW;
  for (long t = blockIdx.x; t < tiles; t += gridDim.x) {
    const long o = t / tpo, j0 = (t - o * tpo) * TW;
    const long base = o * ostride + j0;
    const int live = (int)(ncols - j0 < TW ? ncols - j0 : TW);
    for (int i = threadIdx.x; i < n; i += 256) {
      const int l = i / TW, j = i - l * TW;
      f[i] = j < live ? words[base + (long)l * lstride + j] : SDF_NONE;
    }
    if (threadIdx.x < 64) open[threadIdx.x] = 0;
    __syncthreads();
    // A column whose entries all have one membership and no distance yet stays as it is: no candidate exists.  Far from a
    // class's blob that is most columns, and each would cost every entry a search to both ends of the line.
    for (int i = threadIdx.x; i < n; i += 256) {
      const int j = i % TW, w = f[i];
      if (sdf_mag(w) < SDF_NONE || (w < 0) != (f[j] < 0)) open[j] = 1;      // every writer stores the same value
    }
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += 256) {
      const int l = i / TW, j = i - l * TW;
      if (j >= live) continue;
      const int w = f[i];
      const bool inside = w < 0;
      int best = sdf_mag(w);
      for (int k = 1; open[j] && k < L; ++k) {
        const int kk = k * k;
        if (kk >= best) break;
        if (l >= k) {
          const int u = f[i - k * TW];
          best = min(best, ((u < 0) != inside ? 0 : sdf_mag(u)) + kk);
        }
        if (l + k < L) {
          const int u = f[i + k * TW];
          best = min(best, ((u < 0) != inside ? 0 : sdf_mag(u)) + kk);
        }
      }
      const long at = base + (long)l * lstride + j;
      if constexpr (LAST) {
        const bool none = best >= SDF_NONE;
        const float r = sqrtf((float)best);
        phi[at] = none ? 0.f : (inside ? 1.f - r : r);
        if (d2) d2[at] = none ? 0 : best;
      } else {
        words[at] = inside ? -best : best;
      }
    }
    __syncthreads();
  }
}

inline bool sdf_dims_ok(int N, int C, int D, int H, int W) {
  return N > 0 && C > 0 && (long)N * C <= 65535 && D >= 1 && D <= SDF_MAX_EXTENT && H >= 1 && H <= SDF_MAX_EXTENT && W >= 1 &&
         W <= SDF_MAX_EXTENT;
}

// columns per tile: as many as 32 KB of whole lines hold, at most one wave's worth, a power of two (16 at L = 512)
inline int sdf_tile_cols(int L) {
  int tw = 64;
  while (tw * L > SDF_TILE_WORDS) tw >>= 1;
  return tw;
}

inline unsigned sdf_grid(long blocks) { return (unsigned)(blocks > SDF_MAX_GRID ? SDF_MAX_GRID : blocks); }

}  // namespace dua

extern "C" {

long dua_sdf_scratch_bytes(int N, int C, int D, int H, int W) {
  if (!dua::sdf_dims_ok(N, C, D, H, W)) return DUA_ERR_ARG;
  return (long)N * C * D * H * W * (long)sizeof(int);
}

int dua_sdf_maps(int N, int C, int D, int H, int W, const float* labels, float threshold, float* phi, int* d2_out, void* scratch,
                 long scratch_bytes, void* stream) {
  if (!dua::sdf_dims_ok(N, C, D, H, W) || !labels || !phi || !scratch || !(threshold == threshold) ||
      scratch_bytes < dua_sdf_scratch_bytes(N, C, D, H, W))
    return DUA_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  int* words = (int*)scratch;
  const long vols = (long)N * C, rows = vols * D * H;
  const int rpb = W >= dua::SDF_ROW_WORDS ? 1 : dua::SDF_ROW_WORDS / W;
  hipLaunchKernelGGL(dua::sdf_rows_kernel, dim3(dua::sdf_grid((rows + rpb - 1) / rpb)), dim3(256), 0, s, labels, threshold, rows,
                     W, rpb, words);
  {
    const int tw = dua::sdf_tile_cols(H);
    const long outer = vols * D, tiles = outer * ((W + tw - 1) / tw);
    hipLaunchKernelGGL(dua::sdf_cols_kernel<false>, dim3(dua::sdf_grid(tiles)), dim3(256), (size_t)H * tw * sizeof(int), s, words,
                       outer, H, (long)W, (long)H * W, (long)W, tw, (float*)nullptr, (int*)nullptr);
  }
  {
    const int tw = dua::sdf_tile_cols(D);
    const long hw = (long)H * W, tiles = vols * ((hw + tw - 1) / tw);
    hipLaunchKernelGGL(dua::sdf_cols_kernel<true>, dim3(dua::sdf_grid(tiles)), dim3(256), (size_t)D * tw * sizeof(int), s, words,
                       vols, D, hw, (long)D * hw, hw, tw, phi, d2_out);
  }
  return (int)hipGetLastError();
}

}  // extern "C"
