// Surface-distance metrics of light_training/evaluation/metric.py:314-390 (medpy.metric.binary hd / hd95 / asd / assd behind
// the reference's wrappers) for a batch of V = N * C binary volumes [D][H][W], on the device.
//
//   masks  : one pass over A (test) and B (reference): border(X) = X & ~erode(X), the erosion with
//            generate_binary_structure(3, connectivity) and border_value 0 (outside the volume is background), written as one
//            byte per voxel (bit 0 = border(A), bit 1 = border(B)), and the integer counts |A|, |B|, |A & B|, |border A|,
//            |border B| per volume (64-bit integer atomics, one per block: order-independent)
//   EDT    : exact squared Euclidean distance to the nearest seed voxel, separable.  W pass: one thread per row staged in LDS,
//            a forward and a backward scan give the integer distance g along the row (then sw^2 g^2 in fp64).  H and D passes:
//            lanes along W (a tile of WC consecutive columns, all of the line in LDS), each output is the minimum over the
//            line of f(l') + s^2 (l - l')^2, searched outwards from l and stopped once s^2 k^2 reaches the best value found
//            (an exact minimum: every candidate further out is larger).  All distances in fp64.  The D pass of the metric
//            table evaluates only the query surface voxels and writes nothing else ("gather" form); it also leaves each
//            block's sum of distances (fixed order, written, not accumulated) and the maximum (integer atomicMax on the
//            bits of a non-negative double: order-independent).
//   select : hd95 = np.percentile(concat(sds(A,B), sds(B,A)), 95), linear: the order statistics at floor and floor + 1 of
//            0.95 (n - 1) by an exact radix select over the uint64 bit patterns of the squared distances (8 passes of 8 bits:
//            per-volume 256-bin integer histograms, then one step that fixes the digit), and one pass for the smallest
//            value above the selected one.  sqrt is monotone, so selecting on squared distances selects the distances.
//   finish : per volume, the block sums in a fixed order, the wrapper rule (A or B empty or full -> NaN / 0) and the table.
//   dice   : normalized surface Dice in the voxel-count form: one pass over the surface bytes counts, per direction and
//            tolerance, the surface voxels with d^2 <= tau^2 (integer atomics), one thread per (volume, tolerance) divides.  It
//            needs distances up to the largest tolerance only, so its transform is band-limited (BOUNDED): values above
//            cap2 = tau_max^2 become +inf in every pass and no search goes past them; every value <= cap2 keeps its bits.
// Every sum is taken in a fixed order and every atomic is an integer one, so two runs on the same masks agree bit for bit.
#include "common.hpp"
#include "../../include/dua_hip.h"

#include <math.h>

namespace dua {

constexpr int SURF_THREADS = 256;
constexpr int SURF_PER_THREAD = 16;                     // masks: voxels per thread, 4096 per block
constexpr int SURF_BLOCK_VOX = SURF_THREADS * SURF_PER_THREAD;
constexpr int SEL_GROUPS = 4;                           // select passes: 16-byte groups per thread, 16 KiB of bytes per block
constexpr int ROWS_THREADS = 64;                        // W pass: one wave, one row per lane
constexpr int ROWS_LDS = 32768;
constexpr int COLS_LDS = 48 * 1024;
constexpr unsigned short ROW_NONE = 0xFFFF;             // no seed on the row (extents are <= DUA_SURFACE_MAX_EXTENT)

__device__ __forceinline__ bool fg_at(const float* p, size_t i) { return p[i] != 0.f; }
__device__ __forceinline__ bool fg_at(const unsigned char* p, size_t i) { return p[i] != 0; }

// border(X) at a foreground voxel: on a face of the volume (a face neighbour lies outside, border_value 0), or some neighbour
// of the footprint (offsets with at most `conn` non-zero components) is background
// `fg(offset)` says whether the voxel `offset` elements away is foreground; sd / sh are the element strides of a step along D / H
template <typename F>
__device__ __forceinline__ bool is_border_of(F fg, int d, int h, int w, int D, int H, int W, ptrdiff_t sd, ptrdiff_t sh, int conn) {
  if (d == 0 || h == 0 || w == 0 || d == D - 1 || h == H - 1 || w == W - 1) return true;
#pragma unroll
  for (int dz = -1; dz <= 1; ++dz)
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
      for (int dx = -1; dx <= 1; ++dx) {
        const int nnz = (dz != 0) + (dy != 0) + (dx != 0);
        if (nnz == 0 || nnz > conn) continue;
        if (!fg((ptrdiff_t)dz * sd + (ptrdiff_t)dy * sh + dx)) return true;
      }
  return false;
}

template <typename T>
__device__ __forceinline__ bool is_border(const T* __restrict__ x, size_t p, int d, int h, int w, int D, int H, int W, int conn) {
  return is_border_of([&](ptrdiff_t off) { return fg_at(x, p + off); }, d, h, w, D, H, W, (ptrdiff_t)H * W, (ptrdiff_t)W, conn);
}

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// the five per-thread counts of a masks block into counts[0..5): shuffles across the wave, LDS across the block, one 64-bit
// integer atomic per non-zero counter
__device__ __forceinline__ void masks_block_counts(int na, int nb, int ntp, int nba, int nbb, unsigned long long* __restrict__ counts) {
  __shared__ int red[SURF_THREADS / 64][5];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  na = wave_sum(na); nb = wave_sum(nb); ntp = wave_sum(ntp); nba = wave_sum(nba); nbb = wave_sum(nbb);
  if (lane == 0) { red[wv][0] = na; red[wv][1] = nb; red[wv][2] = ntp; red[wv][3] = nba; red[wv][4] = nbb; }
  __syncthreads();
  if (threadIdx.x < 5) {
    long long t = 0;
    for (int k = 0; k < SURF_THREADS / 64; ++k) t += red[k][threadIdx.x];
    if (t) atomicAdd(&counts[threadIdx.x], (unsigned long long)t);
  }
}

// grid (blocks over [0, svs), V).  surf: [V][svs] bytes, the bytes in [vox, svs) written 0.  counts: [V][5], pre-zeroed.
template <typename TA, typename TB>
__global__ __launch_bounds__(SURF_THREADS) void surface_masks_kernel(const TA* __restrict__ a, long a_vs, const TB* __restrict__ b,
                                                                     long b_vs, int D, int H, int W, int conn,
                                                                     unsigned char* __restrict__ surf, long svs,
                                                                     unsigned long long* __restrict__ counts) {
  const int v = blockIdx.y;
  const long vox = (long)D * H * W;
  const TA* av = a + (size_t)v * a_vs;
  const TB* bv = b + (size_t)v * b_vs;
  int na = 0, nb = 0, ntp = 0, nba = 0, nbb = 0;
  for (int j = 0; j < SURF_PER_THREAD; ++j) {
    const long p = (long)blockIdx.x * SURF_BLOCK_VOX + (long)j * SURF_THREADS + threadIdx.x;
    if (p >= svs) break;
    unsigned char s = 0;
    if (p < vox) {
      const int w = (int)(p % W), h = (int)((p / W) % H), d = (int)(p / ((long)W * H));
      const bool fa = fg_at(av, (size_t)p), fb = fg_at(bv, (size_t)p);
      const bool ba = fa && is_border(av, (size_t)p, d, h, w, D, H, W, conn);
      const bool bb = fb && is_border(bv, (size_t)p, d, h, w, D, H, W, conn);
      na += fa; nb += fb; ntp += fa && fb; nba += ba; nbb += bb;
      s = (unsigned char)(ba | (bb << 1));
    }
    surf[(size_t)v * svs + p] = s;
  }
  masks_block_counts(na, nb, ntp, nba, nbb, counts + (size_t)v * 5);
}

// The label-map form, one (map pair, class) per launch: the mask of the test is (a == cls), that of the reference (b == cls), read
// from the two maps [..][H][W] themselves, and the pass covers the box of extents (Db, Hb, Wb) at origin (od, oh, ow) only.  The
// box is the class's bounding box in both maps grown by one voxel per side and clamped to the volume, so a foreground voxel on
// a face of the box lies on a face of the volume: the face rule of is_border_of on the box is that of the full volume, and an
// inner voxel's neighbours lie in the box.  surf: [svs] bytes on the box grid [Db][Hb][Wb]; counts: [5], pre-zeroed.
__global__ __launch_bounds__(SURF_THREADS) void surface_map_masks_kernel(const unsigned char* __restrict__ a,
                                                                         const unsigned char* __restrict__ b, int cls, int H, int W,
                                                                         int od, int oh, int ow, int Db, int Hb, int Wb, int conn,
                                                                         unsigned char* __restrict__ surf, long svs,
                                                                         unsigned long long* __restrict__ counts) {
  const long vox = (long)Db * Hb * Wb;
  const ptrdiff_t sd = (ptrdiff_t)H * W, sh = (ptrdiff_t)W;
  int na = 0, nb = 0, ntp = 0, nba = 0, nbb = 0;
  for (int j = 0; j < SURF_PER_THREAD; ++j) {
    const long p = (long)blockIdx.x * SURF_BLOCK_VOX + (long)j * SURF_THREADS + threadIdx.x;
    if (p >= svs) break;
    unsigned char s = 0;
    if (p < vox) {
      const int w = (int)(p % Wb), h = (int)((p / Wb) % Hb), d = (int)(p / ((long)Wb * Hb));
      const size_t q = (size_t)(od + d) * (size_t)sd + (size_t)(oh + h) * (size_t)sh + (size_t)(ow + w);
      const bool fa = a[q] == cls, fb = b[q] == cls;
      const bool ba = fa && is_border_of([&](ptrdiff_t off) { return a[q + off] == cls; }, d, h, w, Db, Hb, Wb, sd, sh, conn);
      const bool bb = fb && is_border_of([&](ptrdiff_t off) { return b[q + off] == cls; }, d, h, w, Db, Hb, Wb, sd, sh, conn);
      na += fa; nb += fb; ntp += fa && fb; nba += ba; nbb += bb;
      s = (unsigned char)(ba | (bb << 1));
    }
    surf[p] = s;
  }
  masks_block_counts(na, nb, ntp, nba, nbb, counts);
}

// The bounding boxes of every value below C in a pair of label maps: boxes[n][c] = (d0, h0, w0, d1, h1, w1), half-open, of
// (a[n] == c) | (b[n] == c); pre-set to (INT_MAX x 3, 0 x 3), which is what an absent class keeps.  grid (blocks, N).  A wave takes
// 64 consecutive voxels of ONE row at a time (d and h are wave-uniform), finds the distinct values among its lanes and one
// lane per value folds the run's extent into the block's LDS table; the block then folds its table into boxes.  Integer min /
// max only: the result does not depend on any order.
constexpr int BOX_ITER = 16;                            // wave tiles per wave
__global__ void surface_box_init_kernel(int n, int* __restrict__ boxes) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) boxes[i] = i % 6 < 3 ? 0x7fffffff : 0;
}

__global__ __launch_bounds__(SURF_THREADS) void surface_boxes_kernel(const unsigned char* __restrict__ a, long a_vs,
                                                                     const unsigned char* __restrict__ b, long b_vs, int D, int H,
                                                                     int W, int C, int* __restrict__ boxes) {
  __shared__ int lo[DUA_BLEND_MAX_CLASSES * 3], hi[DUA_BLEND_MAX_CLASSES * 3];
  for (int i = threadIdx.x; i < 3 * C; i += SURF_THREADS) { lo[i] = 0x7fffffff; hi[i] = 0; }
  __syncthreads();
  const int n = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int tpr = (W + 63) / 64;                        // wave tiles per row
  const long tiles = (long)D * H * tpr;
  const unsigned char* maps[2] = {a + (size_t)n * a_vs, b + (size_t)n * b_vs};
  for (int j = 0; j < BOX_ITER; ++j) {
    const long t = ((long)blockIdx.x * BOX_ITER + j) * (SURF_THREADS / 64) + wave;
    if (t >= tiles) break;                              // wave-uniform
    const long row = t / tpr;
    const int w0 = (int)(t - row * tpr) * 64, w = w0 + lane;
    const int h = (int)(row % H), d = (int)(row / H);
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      const int val = w < W ? maps[m][(size_t)row * W + w] : 255;
      const bool valid = val < C;
      unsigned long long todo = __ballot(valid);        // wave-uniform: every lane runs the same iterations
      while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const int ll = __shfl(val, leader, 64);
        const unsigned long long same = __ballot(valid && val == ll);
        if (lane == leader) {
          atomicMin(&lo[3 * ll + 0], d); atomicMin(&lo[3 * ll + 1], h); atomicMin(&lo[3 * ll + 2], w0 + __ffsll((long long)same) - 1);
          atomicMax(&hi[3 * ll + 0], d + 1); atomicMax(&hi[3 * ll + 1], h + 1);
          atomicMax(&hi[3 * ll + 2], w0 + 64 - __clzll((long long)same));
        }
        todo &= ~same;                                  // `same` holds the leader's bit
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 3 * C; i += SURF_THREADS) {
    if (hi[i] == 0) continue;
    int* row = boxes + ((size_t)n * C + i / 3) * 6;
    atomicMin(row + i % 3, lo[i]);
    atomicMax(row + 3 + i % 3, hi[i]);
  }
}

// W pass.  grid (ceil(D*H / R), V, dirs), 64 threads, R rows of S u16 in LDS (S even, S / 2 odd: lanes on different rows hit
// different banks).  Direction z: seed where (seeds & mask_z) != 0; out + z * out_dir = sw2 * g^2, +inf on a row without seeds.
// BOUNDED (the band-limited transform): a value above cap2 is written as +inf.
template <bool BOUNDED>
__global__ __launch_bounds__(ROWS_THREADS) void edt_rows_kernel(const unsigned char* __restrict__ seeds, long seeds_vs, int mask0,
                                                                int mask1, int D, int H, int W, int R, int S, double sw2,
                                                                double* __restrict__ out, long out_dir, double cap2) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned short* row = (unsigned short*)smem;
  const int v = blockIdx.y, z = blockIdx.z;
  const int mask = z == 0 ? mask0 : mask1;
  const long rows = (long)D * H, vox = rows * W;
  const long r0 = (long)blockIdx.x * R;
  const int nr = (int)(rows - r0 < R ? rows - r0 : R);
  const unsigned char* src = seeds + (size_t)v * seeds_vs + (size_t)r0 * W;
  for (int i = threadIdx.x; i < nr * W; i += ROWS_THREADS) {
    const int r = i / W, x = i - r * W;
    row[r * S + x] = (src[i] & mask) ? 0 : ROW_NONE;
  }
  __syncthreads();
  if ((int)threadIdx.x < nr) {
    unsigned short* q = row + threadIdx.x * S;
    int last = -1;
    for (int x = 0; x < W; ++x) {
      if (q[x] == 0) last = x;
      q[x] = last < 0 ? ROW_NONE : (unsigned short)(x - last);
    }
    int next = -1;
    for (int x = W - 1; x >= 0; --x) {
      if (q[x] == 0) next = x;
      if (next >= 0 && next - x < q[x]) q[x] = (unsigned short)(next - x);
    }
  }
  __syncthreads();
  double* dst = out + (size_t)z * out_dir + (size_t)v * vox + (size_t)r0 * W;
  for (int i = threadIdx.x; i < nr * W; i += ROWS_THREADS) {
    const int r = i / W, x = i - r * W;
    const unsigned g = row[r * S + x];
    double val = g == ROW_NONE ? (double)INFINITY : sw2 * (double)(g * g);
    if constexpr (BOUNDED) {
      if (val > cap2) val = (double)INFINITY;
    }
    dst[i] = val;
  }
}

// H or D pass, in place.  The line axis has L entries at stride lstride; `outer` indexes the other non-W axis (stride ostride).
// grid (outer_n * nwc, V, dirs), 256 threads; a block owns columns [w0, w0 + WC) of one outer index over the whole line.
// GATHER = false: every voxel of a column with a finite value is rewritten.  GATHER = true (the last pass of the metric table):
// only voxels whose surface byte has qmask_z set are evaluated; their squared distance is written in place, the block's sum of
// distances goes to partial[(z V + v) P + blockIdx.x] and its largest squared distance into maxbits[z V + v] (atomicMax);
// STATS = false (surface Dice, which counts and never sums) leaves both out.
// BOUNDED (the band-limited transform, inputs already +inf above cap2): the outward search also stops once s^2 k^2 > cap2 and
// a result above cap2 is written as +inf.  A sum of two non-negative terms is at least each of them (rounding is monotone), so
// a candidate dropped here exceeds cap2 in the unbounded search too; every result <= cap2 is the minimum of the same sums as
// there, hence the same bits.  A column (GATHER = false) or a query (GATHER = true) whose whole neighbourhood is +inf costs at
// most sqrt(cap2) / s steps, and a column whose inputs are all +inf is skipped through colflag as before.
template <bool GATHER, bool BOUNDED, bool STATS>
__global__ __launch_bounds__(256) void edt_cols_kernel(double* __restrict__ buf, long vox, int L, long lstride, long ostride,
                                                       int W, int WC, int nwc, double s2, const unsigned char* __restrict__ surf,
                                                       long svs, int qmask0, int qmask1, double* __restrict__ partial, int P,
                                                       unsigned long long* __restrict__ maxbits, double cap2) {
  static_assert(GATHER || !STATS, "the sums and the maximum belong to the gather form");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  double* red = (double*)smem;                                         // [256]
  double* f = (double*)(smem + 256 * sizeof(double));                  // [L][WC]
  const size_t fbytes = ((size_t)L * WC * sizeof(double) + 15) & ~(size_t)15;
  unsigned char* qs = smem + 256 * sizeof(double) + fbytes;            // [L][WC]   (GATHER)
  const size_t qbytes = GATHER ? (((size_t)L * WC + 15) & ~(size_t)15) : 0;
  int* colflag = (int*)(qs + qbytes);                                  // [WC]
  const int v = blockIdx.y, z = blockIdx.z, V = gridDim.y;
  const int outer = blockIdx.x / nwc, w0 = (blockIdx.x - outer * nwc) * WC;
  const int qmask = z == 0 ? qmask0 : qmask1;
  double* col = buf + ((size_t)z * V + v) * vox + (size_t)outer * ostride + w0;
  const unsigned char* qcol = GATHER ? surf + (size_t)v * svs + (size_t)outer * ostride + w0 : nullptr;
  const int n = L * WC;
  for (int i = threadIdx.x; i < n; i += 256) {
    const int l = i / WC, w = i - l * WC;
    const bool in = w0 + w < W;
    f[i] = in ? col[(size_t)l * lstride + w] : (double)INFINITY;
    if constexpr (GATHER) qs[i] = in ? (qcol[(size_t)l * lstride + w] & qmask) != 0 : 0;
  }
  __syncthreads();
  if ((int)threadIdx.x < WC) {
    int flag = 0;
    for (int l = 0; l < L; ++l) {
      if constexpr (GATHER) flag |= qs[l * WC + threadIdx.x];
      else flag |= f[l * WC + threadIdx.x] < (double)INFINITY;
    }
    colflag[threadIdx.x] = flag;
  }
  __syncthreads();
  const int w = threadIdx.x % WC, G = 256 / WC;
  double sum = 0.0, mx = 0.0;
  if ((int)threadIdx.x < G * WC && w0 + w < W && colflag[w]) {
    for (int l = threadIdx.x / WC; l < L; l += G) {
      if constexpr (GATHER) {
        if (!qs[l * WC + w]) continue;
      }
      double best = f[l * WC + w];
      for (int k = 1; k < L; ++k) {
        const double ck = s2 * (double)((long)k * k);
        if (!(ck < best)) break;
        if constexpr (BOUNDED) {
          if (ck > cap2) break;
        }
        if (l >= k) best = fmin(best, f[(l - k) * WC + w] + ck);
        if (l + k < L) best = fmin(best, f[(l + k) * WC + w] + ck);
      }
      if constexpr (BOUNDED) {
        if (best > cap2) best = (double)INFINITY;
      }
      col[(size_t)l * lstride + w] = best;
      if constexpr (STATS) {
        sum += sqrt(best);
        mx = fmax(mx, best);
      }
    }
  }
  if constexpr (STATS) {
    red[threadIdx.x] = sum;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
      if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
      __syncthreads();
    }
    if (threadIdx.x == 0) partial[((size_t)z * V + v) * P + blockIdx.x] = red[0];
    __syncthreads();
    red[threadIdx.x] = mx;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
      if ((int)threadIdx.x < s) red[threadIdx.x] = fmax(red[threadIdx.x], red[threadIdx.x + s]);
      __syncthreads();
    }
    if (threadIdx.x == 0 && red[0] > 0.0)
      atomicMax(&maxbits[(size_t)z * V + v], (unsigned long long)__double_as_longlong(red[0]));
  }
}

// sel: [V][4] u64 = (prefix, rank still to find inside the prefix, count of the last digit's bin, rank sought)
__device__ __forceinline__ unsigned long long hd95_rank(unsigned long long n) {
  return n ? (unsigned long long)floor((double)(n - 1) * 0.95) : 0ull;
}

__global__ void select_init_kernel(int V, const unsigned long long* __restrict__ counts, unsigned long long* __restrict__ sel) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= V) return;
  const unsigned long long k = hd95_rank(counts[(size_t)v * 5 + 3] + counts[(size_t)v * 5 + 4]);
  sel[(size_t)v * 4 + 0] = 0; sel[(size_t)v * 4 + 1] = k; sel[(size_t)v * 4 + 2] = 0; sel[(size_t)v * 4 + 3] = k;
}

// The surface voxels of volume v with their keys (the squared distance's bits): bit 0 reads direction 0, bit 1 direction 1
// (a voxel on both surfaces counts once in each, at distance 0).  MODE 0: histogram of the digit at `shift` among keys inside the
// prefix; MODE 1: the smallest key above the selected one.
template <int MODE>
__global__ __launch_bounds__(SURF_THREADS) void select_pass_kernel(const unsigned char* __restrict__ surf, long svs,
                                                                   const double* __restrict__ dist, long vox, int shift,
                                                                   const unsigned long long* __restrict__ sel,
                                                                   unsigned* __restrict__ hist, unsigned long long* __restrict__ nextmin) {
  __shared__ unsigned lh[256];
  __shared__ unsigned long long lm[SURF_THREADS];
  const int v = blockIdx.y, V = gridDim.y;
  if (MODE == 0) lh[threadIdx.x] = 0;
  __syncthreads();
  const unsigned long long prefix = sel[(size_t)v * 4];
  const int hs = shift + 8;
  unsigned long long best = ~0ull;
  const uint4* s16 = (const uint4*)(surf + (size_t)v * svs);
  const long groups = svs / 16;
  const double* d0 = dist + (size_t)v * vox;
  const double* d1 = dist + ((size_t)V + v) * vox;
  for (int j = 0; j < SEL_GROUPS; ++j) {
    const long g = ((long)blockIdx.x * SEL_GROUPS + j) * SURF_THREADS + threadIdx.x;
    if (g >= groups) break;
    const uint4 q = s16[g];
    if ((q.x | q.y | q.z | q.w) == 0) continue;
    const unsigned words[4] = {q.x, q.y, q.z, q.w};
    for (int e = 0; e < 16; ++e) {
      const unsigned s = (words[e >> 2] >> ((e & 3) * 8)) & 3u;
      if (!s) continue;
      const size_t p = (size_t)g * 16 + e;
      for (int side = 0; side < 2; ++side) {           // a voxel on both surfaces is in both directions' sets
        if (!(s & (1u << side))) continue;
        const unsigned long long key = (unsigned long long)__double_as_longlong(side == 0 ? d0[p] : d1[p]);
        if (MODE == 0) {
          if (hs >= 64 || (key >> hs) == (prefix >> hs)) atomicAdd(&lh[(key >> shift) & 255], 1u);
        } else if (key > prefix && key < best) {
          best = key;
        }
      }
    }
  }
  if (MODE == 0) {
    __syncthreads();
    if (lh[threadIdx.x]) atomicAdd(&hist[(size_t)v * 256 + threadIdx.x], lh[threadIdx.x]);
  } else {
    lm[threadIdx.x] = best;
    __syncthreads();
    for (int s = SURF_THREADS / 2; s > 0; s >>= 1) {
      if ((int)threadIdx.x < s && lm[threadIdx.x + s] < lm[threadIdx.x]) lm[threadIdx.x] = lm[threadIdx.x + s];
      __syncthreads();
    }
    if (threadIdx.x == 0 && lm[0] != ~0ull) atomicMin(&nextmin[v], lm[0]);
  }
}

// one block of 256 per volume: fix the digit at `shift`, then clear the histogram for the next pass
__global__ __launch_bounds__(256) void select_step_kernel(int shift, unsigned long long* __restrict__ sel, unsigned* __restrict__ hist) {
  __shared__ unsigned h[256];
  const int v = blockIdx.x;
  h[threadIdx.x] = hist[(size_t)v * 256 + threadIdx.x];
  __syncthreads();
  hist[(size_t)v * 256 + threadIdx.x] = 0;
  if (threadIdx.x == 0) {
    unsigned long long k = sel[(size_t)v * 4 + 1], below = 0;
    for (int dgt = 0; dgt < 256; ++dgt) {
      if (k < below + h[dgt]) {
        sel[(size_t)v * 4 + 0] |= (unsigned long long)dgt << shift;
        sel[(size_t)v * 4 + 1] = k - below;
        sel[(size_t)v * 4 + 2] = h[dgt];
        break;
      }
      below += h[dgt];
    }
  }
}

// one block of 256 per volume: out[v][DUA_SURFACE_FIELDS]
__global__ __launch_bounds__(256) void surface_finish_kernel(int V, long vox, const unsigned long long* __restrict__ counts,
                                                             const double* __restrict__ partial, int P,
                                                             const unsigned long long* __restrict__ maxbits,
                                                             const unsigned long long* __restrict__ sel,
                                                             const unsigned long long* __restrict__ nextmin, int nan_for_nonexisting,
                                                             double* __restrict__ out) {
  __shared__ double red[2][256];
  const int v = blockIdx.x;
  for (int z = 0; z < 2; ++z) {
    const double* pz = partial + ((size_t)z * V + v) * P;
    double s = 0.0;
    for (int i = threadIdx.x; i < P; i += 256) s += pz[i];
    red[z][threadIdx.x] = s;
  }
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      red[0][threadIdx.x] += red[0][threadIdx.x + s];
      red[1][threadIdx.x] += red[1][threadIdx.x + s];
    }
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  const unsigned long long* c = counts + (size_t)v * 5;
  const unsigned long long na = c[0], nb = c[1], tp = c[2], sa = c[3], sb = c[4];
  double* o = out + (size_t)v * DUA_SURFACE_FIELDS;
  o[DUA_SURFACE_TP] = (double)tp;
  o[DUA_SURFACE_FP] = (double)(na - tp);
  o[DUA_SURFACE_FN] = (double)(nb - tp);
  o[DUA_SURFACE_TN] = (double)((unsigned long long)vox - na - nb + tp);
  o[DUA_SURFACE_NSURF] = (double)(sa + sb);
  const bool exists = na > 0 && nb > 0 && na < (unsigned long long)vox && nb < (unsigned long long)vox;
  if (!exists) {
    const double r = nan_for_nonexisting ? (double)NAN : 0.0;
    o[DUA_SURFACE_HD] = o[DUA_SURFACE_HD95] = o[DUA_SURFACE_ASD] = o[DUA_SURFACE_ASSD] = r;
    o[DUA_SURFACE_HD95_LO] = o[DUA_SURFACE_HD95_HI] = o[DUA_SURFACE_ASD_BA] = r;
    return;
  }
  const double asd = red[0][0] / (double)sa, asd_ba = red[1][0] / (double)sb;
  o[DUA_SURFACE_HD] = sqrt(fmax(__longlong_as_double((long long)maxbits[v]), __longlong_as_double((long long)maxbits[V + v])));
  o[DUA_SURFACE_ASD] = asd;
  o[DUA_SURFACE_ASD_BA] = asd_ba;
  o[DUA_SURFACE_ASSD] = (asd + asd_ba) / 2.0;
  // np.percentile(x, 95), method "linear": virtual index (n - 1) * 0.95, numpy's _lerp between its floor and floor + 1
  const unsigned long long n = sa + sb, kl = sel[(size_t)v * 4 + 3];
  const unsigned long long prefix = sel[(size_t)v * 4], less = kl - sel[(size_t)v * 4 + 1], eq = sel[(size_t)v * 4 + 2];
  unsigned long long hi_key = prefix;
  if (kl + 1 < n && kl + 1 >= less + eq) hi_key = nextmin[v];
  const double lo = sqrt(__longlong_as_double((long long)prefix)), hi = sqrt(__longlong_as_double((long long)hi_key));
  const double idx = (double)(n - 1) * 0.95;
  const double t = idx - floor(idx);
  const double diff = hi - lo;
  o[DUA_SURFACE_HD95] = t >= 0.5 ? hi - diff * (1.0 - t) : lo + diff * t;
  o[DUA_SURFACE_HD95_LO] = lo;
  o[DUA_SURFACE_HD95_HI] = hi;
}

// ---- surface Dice (normalized surface Dice, voxel-count form) -----------------------------------------------------------------
// The squared tolerances of the call, [classes][T] row-major, by value in the kernel arguments (at most 1 KiB): nothing is
// copied to the device and nothing waits for a copy.  Volume v reads row v % classes.
struct SurfaceTolerances {
  double t2[DUA_SURFACE_MAX_TOLERANCE_ENTRIES];
};

// The surface voxels of volume v as in select_pass_kernel (16-byte groups of surface bytes, dist read only where a bit is set):
// within[v][t][side] += #{surface voxels of side with d^2 <= tau_t^2}, side 0 = border(A) against border(B).  Per-thread integer
// counts, shuffles across the wave, LDS across the block, one 64-bit integer atomic per block and (side, t).  within pre-zeroed.
__global__ __launch_bounds__(SURF_THREADS) void surface_count_kernel(const unsigned char* __restrict__ surf, long svs,
                                                                     const double* __restrict__ dist, long vox, int classes, int T,
                                                                     const SurfaceTolerances tol,
                                                                     unsigned long long* __restrict__ within) {
  constexpr int MT = DUA_SURFACE_MAX_TOLERANCES;
  __shared__ int red[SURF_THREADS / 64][2 * MT];
  const int v = blockIdx.y, V = gridDim.y;
  const double* row = tol.t2 + (size_t)(v % classes) * T;
  double t2[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) t2[t] = t < T ? row[t] : -1.0;          // d^2 >= 0 is never within an unused slot
  int cnt[2][MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) cnt[0][t] = cnt[1][t] = 0;
  const uint4* s16 = (const uint4*)(surf + (size_t)v * svs);
  const long groups = svs / 16;
  const double* d0 = dist + (size_t)v * vox;
  const double* d1 = dist + ((size_t)V + v) * vox;
  for (int j = 0; j < SEL_GROUPS; ++j) {
    const long g = ((long)blockIdx.x * SEL_GROUPS + j) * SURF_THREADS + threadIdx.x;
    if (g >= groups) break;
    const uint4 q = s16[g];
    if ((q.x | q.y | q.z | q.w) == 0) continue;
    const unsigned words[4] = {q.x, q.y, q.z, q.w};
    for (int e = 0; e < 16; ++e) {
      const unsigned s = (words[e >> 2] >> ((e & 3) * 8)) & 3u;
      if (!s) continue;
      const size_t p = (size_t)g * 16 + e;
      if (s & 1u) {
        const double d2 = d0[p];
#pragma unroll
        for (int t = 0; t < MT; ++t) cnt[0][t] += d2 <= t2[t];
      }
      if (s & 2u) {
        const double d2 = d1[p];
#pragma unroll
        for (int t = 0; t < MT; ++t) cnt[1][t] += d2 <= t2[t];
      }
    }
  }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int side = 0; side < 2; ++side)
#pragma unroll
    for (int t = 0; t < MT; ++t) {
      const int c = wave_sum(cnt[side][t]);
      if (lane == 0) red[wv][side * MT + t] = c;
    }
  __syncthreads();
  if (threadIdx.x < 2 * MT) {
    const int side = threadIdx.x / MT, t = threadIdx.x % MT;
    long long total = 0;
    for (int k = 0; k < SURF_THREADS / 64; ++k) total += red[k][threadIdx.x];
    if (t < T && total) atomicAdd(&within[((size_t)v * T + t) * 2 + side], (unsigned long long)total);
  }
}

// one thread per (v, t): nsd = (within_AB + within_BA) / (|border A| + |border B|), one fp64 division of two integers; no
// surface voxel at all -> NaN (0 with nan_for_nonexisting = 0).  One empty border gives 0 by itself (nothing lies within).
__global__ void surface_dice_finish_kernel(int V, int T, const unsigned long long* __restrict__ counts,
                                           const unsigned long long* __restrict__ within, int nan_for_nonexisting,
                                           double* __restrict__ nsd) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= V * T) return;
  const int v = i / T;
  const unsigned long long den = counts[(size_t)v * 5 + 3] + counts[(size_t)v * 5 + 4];
  const unsigned long long num = within[(size_t)i * 2] + within[(size_t)i * 2 + 1];
  nsd[i] = den ? (double)num / (double)den : (nan_for_nonexisting ? (double)NAN : 0.0);
}

// ---- host side ----------------------------------------------------------------------------------------------------------

static long align256(long x) { return (x + 255) & ~255L; }

static bool extents_ok(int V, int D, int H, int W) {
  return V >= 1 && V <= 65535 && D >= 1 && H >= 1 && W >= 1 && D <= DUA_SURFACE_MAX_EXTENT && H <= DUA_SURFACE_MAX_EXTENT &&
         W <= DUA_SURFACE_MAX_EXTENT;
}

static bool spacing_ok(double s) { return s > 0.0 && isfinite(s); }

static int rows_stride(int W) {             // u16 entries per LDS row: even, with an odd number of dwords
  int S = (W + 1) & ~1;
  if ((S / 2) % 2 == 0) S += 2;
  return S;
}

static size_t cols_lds(int L, int WC, bool gather) {
  const size_t f = ((size_t)L * WC * 8 + 15) & ~(size_t)15;
  const size_t q = gather ? (((size_t)L * WC + 15) & ~(size_t)15) : 0;
  return 256 * 8 + f + q + (size_t)WC * 4;
}

static int cols_wc(int L, int W, bool gather) {
  int wc = 64;
  while (wc > 1 && cols_lds(L, wc, gather) > (size_t)COLS_LDS) wc >>= 1;
  while (wc > 1 && wc / 2 >= W) wc >>= 1;
  return wc;
}

// the three EDT passes over dirs (1 or 2) directions: seeds [V][seeds_vs] bytes; out: dirs x [V][vox] fp64.
// surf: the D pass in gather form (queries = the surface bytes' bits 1 | 2); partial and maxbits: with its sums and maxima.
// bounded: the band-limited transform (exact up to cap2, +inf above); its gather form has no sums (no caller asks for both).
static int edt_launch(int V, int D, int H, int W, const unsigned char* seeds, long seeds_vs, int smask0, int smask1, int dirs,
                      double sd, double sh, double sw, double* out, const unsigned char* surf, long svs, double* partial,
                      unsigned long long* maxbits, bool bounded, double cap2, hipStream_t s) {
  const long vox = (long)D * H * W, dir_stride = (long)V * vox;
  const int S = rows_stride(W);
  int R = ROWS_LDS / (S * 2);
  if (R > ROWS_THREADS) R = ROWS_THREADS;
  const long rows = (long)D * H;
  const dim3 rgrid((unsigned)((rows + R - 1) / R), V, dirs);
  if (bounded)
    hipLaunchKernelGGL(edt_rows_kernel<true>, rgrid, dim3(ROWS_THREADS), (size_t)R * S * 2, s, seeds, seeds_vs, smask0, smask1, D,
                       H, W, R, S, sw * sw, out, dir_stride, cap2);
  else
    hipLaunchKernelGGL(edt_rows_kernel<false>, rgrid, dim3(ROWS_THREADS), (size_t)R * S * 2, s, seeds, seeds_vs, smask0, smask1,
                       D, H, W, R, S, sw * sw, out, dir_stride, 0.0);
#define COLS_LAUNCH(G, B, ST, grid, lds, L, ls, os, wc, nwc, s2, P)                                                          \
  hipLaunchKernelGGL((edt_cols_kernel<G, B, ST>), grid, dim3(256), lds, s, out, vox, L, ls, os, W, wc, nwc, s2,               \
                     G ? surf : nullptr, G ? svs : 0L, G ? 1 : 0, G ? 2 : 0, ST ? partial : nullptr, P, ST ? maxbits : nullptr, \
                     B ? cap2 : 0.0)
  // H pass: line along H (stride W), outer index d (stride H W)
  int wc = cols_wc(H, W, false), nwc = (W + wc - 1) / wc;
  const dim3 hgrid((unsigned)((long)D * nwc), V, dirs);
  if (bounded) COLS_LAUNCH(false, true, false, hgrid, cols_lds(H, wc, false), H, (long)W, (long)H * W, wc, nwc, sh * sh, 0);
  else COLS_LAUNCH(false, false, false, hgrid, cols_lds(H, wc, false), H, (long)W, (long)H * W, wc, nwc, sh * sh, 0);
  // D pass: line along D (stride H W), outer index h (stride W)
  const bool gather = surf != nullptr, stats = partial != nullptr;
  wc = cols_wc(D, W, gather);
  nwc = (W + wc - 1) / wc;
  const dim3 grid((unsigned)((long)H * nwc), V, dirs);
  const size_t lds = cols_lds(D, wc, gather);
  if (gather && stats && !bounded) COLS_LAUNCH(true, false, true, grid, lds, D, (long)H * W, (long)W, wc, nwc, sd * sd, H * nwc);
  else if (gather && !bounded) COLS_LAUNCH(true, false, false, grid, lds, D, (long)H * W, (long)W, wc, nwc, sd * sd, 0);
  else if (gather) COLS_LAUNCH(true, true, false, grid, lds, D, (long)H * W, (long)W, wc, nwc, sd * sd, 0);
  else if (bounded) COLS_LAUNCH(false, true, false, grid, lds, D, (long)H * W, (long)W, wc, nwc, sd * sd, 0);
  else COLS_LAUNCH(false, false, false, grid, lds, D, (long)H * W, (long)W, wc, nwc, sd * sd, 0);
#undef COLS_LAUNCH
  return (int)hipGetLastError();
}

static int masks_launch(int V, int D, int H, int W, const void* a, int a_dtype, long a_vs, const void* b, int b_dtype, long b_vs,
                        int conn, unsigned char* surf, long svs, unsigned long long* counts, hipStream_t s) {
  hipError_t e = hipMemsetAsync(counts, 0, (size_t)V * 5 * sizeof(unsigned long long), s);
  if (e != hipSuccess) return (int)e;
  const dim3 grid((unsigned)((svs + SURF_BLOCK_VOX - 1) / SURF_BLOCK_VOX), V);
#define SM_LAUNCH(TA, TB)                                                                                                  \
  hipLaunchKernelGGL((surface_masks_kernel<TA, TB>), grid, dim3(SURF_THREADS), 0, s, (const TA*)a, a_vs, (const TB*)b, b_vs, D, \
                     H, W, conn, surf, svs, counts)
  if (a_dtype == DUA_F32 && b_dtype == DUA_F32) SM_LAUNCH(float, float);
  else if (a_dtype == DUA_F32) SM_LAUNCH(float, unsigned char);
  else if (b_dtype == DUA_F32) SM_LAUNCH(unsigned char, float);
  else SM_LAUNCH(unsigned char, unsigned char);
#undef SM_LAUNCH
  return (int)hipGetLastError();
}

struct SurfaceScratch {
  long surf, dist, partial, maxbits, hist, sel, nextmin, total;
};

static SurfaceScratch scratch_layout(int V, int D, int H, int W) {
  SurfaceScratch L;
  const long vox = (long)D * H * W, svs = align256(vox);
  const int wc = cols_wc(D, W, true), P = H * ((W + wc - 1) / wc);
  L.surf = 0;
  L.dist = align256(L.surf + (long)V * svs);
  L.partial = align256(L.dist + 2L * V * vox * 8);
  L.maxbits = align256(L.partial + 2L * V * P * 8);
  L.hist = align256(L.maxbits + 2L * V * 8);
  L.sel = align256(L.hist + (long)V * 256 * 4);
  L.nextmin = align256(L.sel + (long)V * 4 * 8);
  L.total = align256(L.nextmin + (long)V * 8);
  return L;
}

static bool mask_dtype_ok(int t) { return t == DUA_F32 || t == DUA_U8; }

// surface Dice alone: the surface bytes and the two distance volumes
struct DiceScratch {
  long surf, dist, total;
};

static DiceScratch dice_layout(int V, int D, int H, int W) {
  DiceScratch L;
  const long vox = (long)D * H * W;
  L.surf = 0;
  L.dist = align256((long)V * align256(vox));
  L.total = align256(L.dist + 2L * V * vox * 8);
  return L;
}

// the [classes][T] table of a call: squared (tau * tau, rounded once) into tol, the largest square into cap2
static bool tolerances_ok(int V, int classes, int T, const double* tolerances, SurfaceTolerances& tol, double& cap2) {
  if (!tolerances || classes < 1 || V % classes != 0 || T < 1 || T > DUA_SURFACE_MAX_TOLERANCES ||
      (long)classes * T > DUA_SURFACE_MAX_TOLERANCE_ENTRIES)
    return false;
  cap2 = 0.0;
  for (int i = 0; i < DUA_SURFACE_MAX_TOLERANCE_ENTRIES; ++i) tol.t2[i] = -1.0;
  for (int i = 0; i < classes * T; ++i) {
    const double t = tolerances[i];
    if (!isfinite(t) || t < 0.0) return false;
    tol.t2[i] = t * t;
    if (tol.t2[i] > cap2) cap2 = tol.t2[i];
  }
  return true;
}

// count and finish on a gathered dist buffer (both directions): within [V][T][2], nsd [V][T]
static int dice_launch(int V, long vox, const unsigned char* surf, long svs, const double* dist, int classes, int T,
                       const SurfaceTolerances& tol, const unsigned long long* counts, int nan_for_nonexisting,
                       unsigned long long* within, double* nsd, hipStream_t s) {
  hipError_t e = hipMemsetAsync(within, 0, (size_t)V * T * 2 * sizeof(unsigned long long), s);
  if (e != hipSuccess) return (int)e;
  const dim3 grid((unsigned)((svs / 16 + SURF_THREADS * SEL_GROUPS - 1) / (SURF_THREADS * SEL_GROUPS)), V);
  hipLaunchKernelGGL(surface_count_kernel, grid, dim3(SURF_THREADS), 0, s, surf, svs, dist, vox, classes, T, tol, within);
  hipLaunchKernelGGL(surface_dice_finish_kernel, dim3((V * T + 255) / 256), dim3(256), 0, s, V, T, counts, within,
                     nan_for_nonexisting, nsd);
  return (int)hipGetLastError();
}

}  // namespace dua

// Everything behind the surface bytes (workspace + L.surf, on the grid [V][D][H][W]) and counts: transform, select, finish and,
// with tol, the surface Dice.  full_vox: the voxels of the volume the masks live in -- tn and the "mask is full" rule count
// against it; it is D H W unless the grid is a box of a larger volume (dua_surface_map_report).
static int surface_table_tail(int V, int D, int H, int W, long full_vox, double sd, double sh, double sw, int nan_for_nonexisting,
                              unsigned long long* counts, double* out, unsigned char* ws, const dua::SurfaceScratch& L, int classes,
                              int T, const dua::SurfaceTolerances* tol, unsigned long long* within, double* nsd, hipStream_t s) {
  const long vox = (long)D * H * W, svs = dua::align256(vox);
  unsigned char* surf = ws + L.surf;
  double* dist = (double*)(ws + L.dist);
  double* partial = (double*)(ws + L.partial);
  unsigned long long* maxbits = (unsigned long long*)(ws + L.maxbits);
  unsigned* hist = (unsigned*)(ws + L.hist);
  unsigned long long* sel = (unsigned long long*)(ws + L.sel);
  unsigned long long* nextmin = (unsigned long long*)(ws + L.nextmin);
  hipError_t e = hipMemsetAsync(maxbits, 0, (size_t)2 * V * 8, s);
  if (e == hipSuccess) e = hipMemsetAsync(hist, 0, (size_t)V * 256 * 4, s);
  if (e == hipSuccess) e = hipMemsetAsync(nextmin, 0xFF, (size_t)V * 8, s);
  if (e != hipSuccess) return (int)e;
  // direction 0: seeds border(B) (bit 1), read at border(A) (bit 0); direction 1 the other way round
  const int rc = dua::edt_launch(V, D, H, W, surf, svs, 2, 1, 2, sd, sh, sw, dist, surf, svs, partial, maxbits, false, 0.0, s);
  if (rc) return rc;
  hipLaunchKernelGGL(dua::select_init_kernel, dim3((V + 255) / 256), dim3(256), 0, s, V, counts, sel);
  const dim3 sgrid((unsigned)((svs / 16 + dua::SURF_THREADS * dua::SEL_GROUPS - 1) / (dua::SURF_THREADS * dua::SEL_GROUPS)), V);
  for (int shift = 56; shift >= 0; shift -= 8) {
    hipLaunchKernelGGL(dua::select_pass_kernel<0>, sgrid, dim3(dua::SURF_THREADS), 0, s, surf, svs, dist, vox, shift, sel, hist,
                       nextmin);
    hipLaunchKernelGGL(dua::select_step_kernel, dim3(V), dim3(256), 0, s, shift, sel, hist);
  }
  hipLaunchKernelGGL(dua::select_pass_kernel<1>, sgrid, dim3(dua::SURF_THREADS), 0, s, surf, svs, dist, vox, 0, sel, hist, nextmin);
  const int wc = dua::cols_wc(D, W, true);
  hipLaunchKernelGGL(dua::surface_finish_kernel, dim3(V), dim3(256), 0, s, V, full_vox, counts, partial, H * ((W + wc - 1) / wc),
                     maxbits, sel, nextmin, nan_for_nonexisting, out);
  if (tol) return dua::dice_launch(V, vox, surf, svs, dist, classes, T, *tol, counts, nan_for_nonexisting, within, nsd, s);
  return (int)hipGetLastError();
}

// the distance table; with tol, the surface Dice outputs too, counted on the same dist buffer (dua_surface_report)
static int surface_table(int V, int D, int H, int W, const void* test, int test_dtype, long test_vstride, const void* reference,
                         int reference_dtype, long reference_vstride, int connectivity, double sd, double sh, double sw,
                         int nan_for_nonexisting, unsigned long long* counts, double* out, void* workspace, long workspace_bytes,
                         int classes, int T, const dua::SurfaceTolerances* tol, unsigned long long* within, double* nsd,
                         void* stream) {
  const long vox = (long)D * H * W;
  if (!dua::extents_ok(V, D, H, W) || !test || !reference || !counts || !out || !workspace || connectivity < 1 ||
      connectivity > 3 || !dua::mask_dtype_ok(test_dtype) || !dua::mask_dtype_ok(reference_dtype) || test_vstride < vox ||
      reference_vstride < vox || !dua::spacing_ok(sd) || !dua::spacing_ok(sh) || !dua::spacing_ok(sw))
    return DUA_ERR_ARG;
  const dua::SurfaceScratch L = dua::scratch_layout(V, D, H, W);
  if (workspace_bytes < L.total || ((size_t)workspace & 255) != 0) return DUA_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  unsigned char* ws = (unsigned char*)workspace;
  unsigned char* surf = ws + L.surf;
  const long svs = dua::align256(vox);
  int rc = dua::masks_launch(V, D, H, W, test, test_dtype, test_vstride, reference, reference_dtype, reference_vstride,
                             connectivity, surf, svs, counts, s);
  if (rc) return rc;
  return surface_table_tail(V, D, H, W, vox, sd, sh, sw, nan_for_nonexisting, counts, out, ws, L, classes, T, tol, within, nsd, s);
}


extern "C" {

long dua_surface_scratch_bytes(int V, int D, int H, int W) {
  if (!dua::extents_ok(V, D, H, W)) return DUA_ERR_ARG;
  return dua::scratch_layout(V, D, H, W).total;
}

int dua_surface_masks(int V, int D, int H, int W, const void* test, int test_dtype, long test_vstride, const void* reference,
                      int reference_dtype, long reference_vstride, int connectivity, unsigned char* surf, long surf_vstride,
                      unsigned long long* counts, void* stream) {
  const long vox = (long)D * H * W;
  if (!dua::extents_ok(V, D, H, W) || !test || !reference || !surf || !counts || connectivity < 1 || connectivity > 3 ||
      !dua::mask_dtype_ok(test_dtype) || !dua::mask_dtype_ok(reference_dtype) || test_vstride < vox ||
      reference_vstride < vox || surf_vstride < vox)
    return DUA_ERR_ARG;
  return dua::masks_launch(V, D, H, W, test, test_dtype, test_vstride, reference, reference_dtype, reference_vstride, connectivity,
                           surf, surf_vstride, counts, (hipStream_t)stream);
}

int dua_surface_edt_sq(int V, int D, int H, int W, const unsigned char* seeds, long seeds_vstride, int seed_mask, double sd,
                       double sh, double sw, double* out, void* stream) {
  const long vox = (long)D * H * W;
  if (!dua::extents_ok(V, D, H, W) || !seeds || !out || seeds_vstride < vox || (seed_mask & 255) == 0 ||
      !dua::spacing_ok(sd) || !dua::spacing_ok(sh) || !dua::spacing_ok(sw))
    return DUA_ERR_ARG;
  return dua::edt_launch(V, D, H, W, seeds, seeds_vstride, seed_mask, seed_mask, 1, sd, sh, sw, out, nullptr, 0, nullptr, nullptr,
                         false, 0.0, (hipStream_t)stream);
}

int dua_surface_edt_sq_bounded(int V, int D, int H, int W, const unsigned char* seeds, long seeds_vstride, int seed_mask,
                               double sd, double sh, double sw, double max_distance, double* out, void* stream) {
  const long vox = (long)D * H * W;
  if (!dua::extents_ok(V, D, H, W) || !seeds || !out || seeds_vstride < vox || (seed_mask & 255) == 0 ||
      !dua::spacing_ok(sd) || !dua::spacing_ok(sh) || !dua::spacing_ok(sw) || !(max_distance >= 0.0))
    return DUA_ERR_ARG;
  return dua::edt_launch(V, D, H, W, seeds, seeds_vstride, seed_mask, seed_mask, 1, sd, sh, sw, out, nullptr, 0, nullptr, nullptr,
                         true, max_distance * max_distance, (hipStream_t)stream);
}


int dua_surface_distance_table(int V, int D, int H, int W, const void* test, int test_dtype, long test_vstride,
                               const void* reference, int reference_dtype, long reference_vstride, int connectivity, double sd,
                               double sh, double sw, int nan_for_nonexisting, unsigned long long* counts, double* out,
                               void* workspace, long workspace_bytes, void* stream) {
  return surface_table(V, D, H, W, test, test_dtype, test_vstride, reference, reference_dtype, reference_vstride, connectivity,
                       sd, sh, sw, nan_for_nonexisting, counts, out, workspace, workspace_bytes, 0, 0, nullptr, nullptr, nullptr,
                       stream);
}

long dua_surface_dice_scratch_bytes(int V, int D, int H, int W) {
  if (!dua::extents_ok(V, D, H, W)) return DUA_ERR_ARG;
  return dua::dice_layout(V, D, H, W).total;
}

int dua_surface_dice_table(int V, int D, int H, int W, const void* test, int test_dtype, long test_vstride,
                           const void* reference, int reference_dtype, long reference_vstride, int connectivity, double sd,
                           double sh, double sw, int classes, int T, const double* tolerances, int nan_for_nonexisting,
                           int bounded, unsigned long long* counts, unsigned long long* within, double* nsd, void* workspace,
                           long workspace_bytes, void* stream) {
  const long vox = (long)D * H * W;
  dua::SurfaceTolerances tol;
  double cap2 = 0.0;
  if (!dua::extents_ok(V, D, H, W) || !test || !reference || !counts || !within || !nsd || !workspace || connectivity < 1 ||
      connectivity > 3 || !dua::mask_dtype_ok(test_dtype) || !dua::mask_dtype_ok(reference_dtype) || test_vstride < vox ||
      reference_vstride < vox || !dua::spacing_ok(sd) || !dua::spacing_ok(sh) || !dua::spacing_ok(sw) ||
      !dua::tolerances_ok(V, classes, T, tolerances, tol, cap2))
    return DUA_ERR_ARG;
  const dua::DiceScratch L = dua::dice_layout(V, D, H, W);
  if (workspace_bytes < L.total || ((size_t)workspace & 255) != 0) return DUA_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  unsigned char* surf = (unsigned char*)workspace + L.surf;
  double* dist = (double*)((unsigned char*)workspace + L.dist);
  const long svs = dua::align256(vox);
  int rc = dua::masks_launch(V, D, H, W, test, test_dtype, test_vstride, reference, reference_dtype, reference_vstride,
                             connectivity, surf, svs, counts, s);
  if (rc) return rc;
  // direction 0: seeds border(B) (bit 1), read at border(A) (bit 0); direction 1 the other way round
  rc = dua::edt_launch(V, D, H, W, surf, svs, 2, 1, 2, sd, sh, sw, dist, surf, svs, nullptr, nullptr, bounded != 0, cap2, s);
  if (rc) return rc;
  return dua::dice_launch(V, vox, surf, svs, dist, classes, T, tol, counts, nan_for_nonexisting, within, nsd, s);
}

int dua_surface_report(int V, int D, int H, int W, const void* test, int test_dtype, long test_vstride, const void* reference,
                       int reference_dtype, long reference_vstride, int connectivity, double sd, double sh, double sw, int classes,
                       int T, const double* tolerances, int nan_for_nonexisting, unsigned long long* counts, double* out,
                       unsigned long long* within, double* nsd, void* workspace, long workspace_bytes, void* stream) {
  dua::SurfaceTolerances tol;
  double cap2 = 0.0;
  if (!within || !nsd || !dua::extents_ok(V, D, H, W) || !dua::tolerances_ok(V, classes, T, tolerances, tol, cap2))
    return DUA_ERR_ARG;
  return surface_table(V, D, H, W, test, test_dtype, test_vstride, reference, reference_dtype, reference_vstride, connectivity,
                       sd, sh, sw, nan_for_nonexisting, counts, out, workspace, workspace_bytes, classes, T, &tol, within, nsd,
                       stream);
}

// ---- the report of two label maps, per class, inside the class's box ---------------------------------------------------------

// a row of the box table, grown by one voxel per side and clamped: origin and extents.  false: the class is absent (d1 == 0).
// A row that is neither absent nor a non-empty box inside the volume is refused by the callers.
static bool map_box_ok(const int* b, int D, int H, int W) {
  if (b[3] == 0) return true;
  return b[0] >= 0 && b[0] < b[3] && b[3] <= D && b[1] >= 0 && b[1] < b[4] && b[4] <= H && b[2] >= 0 && b[2] < b[5] && b[5] <= W;
}

static bool map_box_grow(const int* b, int D, int H, int W, int o[3], int n[3]) {
  if (b[3] == 0) return false;
  const int ext[3] = {D, H, W};
  for (int i = 0; i < 3; ++i) {
    o[i] = b[i] > 0 ? b[i] - 1 : 0;
    const int hi = b[3 + i] < ext[i] ? b[3 + i] + 1 : ext[i];
    n[i] = hi - o[i];
  }
  return true;
}

long dua_surface_map_scratch_bytes(int D, int H, int W, int rows, const int* boxes) {
  if (!dua::extents_ok(1, D, H, W) || rows < 1 || rows > 65535 || !boxes) return DUA_ERR_ARG;
  long largest = 0;                                    // the rows run one after the other on one stream and share one region
  for (int r = 0; r < rows; ++r) {
    int o[3], n[3];
    if (!map_box_ok(boxes + 6 * r, D, H, W)) return DUA_ERR_ARG;
    if (map_box_grow(boxes + 6 * r, D, H, W, o, n)) {
      const long need = dua::scratch_layout(1, n[0], n[1], n[2]).total;
      if (need > largest) largest = need;
    }
  }
  return largest;
}

int dua_surface_map_boxes(int N, int D, int H, int W, const unsigned char* test, long test_vstride, const unsigned char* reference,
                          long reference_vstride, int C, int* boxes, void* stream) {
  const long vox = (long)D * H * W;
  if (!dua::extents_ok(N, D, H, W) || !test || !reference || !boxes || C < 1 || C > DUA_BLEND_MAX_CLASSES ||
      (long)N * C > 65535 || test_vstride < vox || reference_vstride < vox || ((size_t)boxes & 3) != 0)
    return DUA_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  const int n = N * C * 6;
  hipLaunchKernelGGL(dua::surface_box_init_kernel, dim3((n + 255) / 256), dim3(256), 0, s, n, boxes);
  const long tiles = (long)D * H * ((W + 63) / 64), per_block = (long)dua::BOX_ITER * (dua::SURF_THREADS / 64);
  hipLaunchKernelGGL(dua::surface_boxes_kernel, dim3((unsigned)((tiles + per_block - 1) / per_block), N), dim3(dua::SURF_THREADS),
                     0, s, test, test_vstride, reference, reference_vstride, D, H, W, C, boxes);
  return (int)hipGetLastError();
}

int dua_surface_map_report(int N, int D, int H, int W, const unsigned char* test, long test_vstride,
                           const unsigned char* reference, long reference_vstride, int K, const int* class_ids, const int* boxes,
                           int connectivity, double sd, double sh, double sw, int T, const double* tolerances,
                           int nan_for_nonexisting, unsigned long long* counts, double* out, unsigned long long* within,
                           double* nsd, void* workspace, long workspace_bytes, void* stream) {
  const long vox = (long)D * H * W;
  dua::SurfaceTolerances all;
  double cap2 = 0.0;
  if (!dua::extents_ok(N, D, H, W) || !test || !reference || !class_ids || !boxes || !counts || !out || !within || !nsd ||
      K < 1 || (long)N * K > 65535 || connectivity < 1 || connectivity > 3 || test_vstride < vox || reference_vstride < vox ||
      !dua::spacing_ok(sd) || !dua::spacing_ok(sh) || !dua::spacing_ok(sw) || !dua::tolerances_ok(K, K, T, tolerances, all, cap2))
    return DUA_ERR_ARG;
  for (int k = 0; k < K; ++k)
    if (class_ids[k] < 0 || class_ids[k] > 255) return DUA_ERR_ARG;
  const long need = dua_surface_map_scratch_bytes(D, H, W, N * K, boxes);
  if (need < 0 || workspace_bytes < need || (need > 0 && (!workspace || ((size_t)workspace & 255) != 0))) return DUA_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  unsigned char* ws = (unsigned char*)workspace;
  for (int r = 0; r < N * K; ++r) {
    const int n = r / K, k = r % K;
    unsigned long long* counts_r = counts + (size_t)r * 5;
    double* out_r = out + (size_t)r * DUA_SURFACE_FIELDS;
    unsigned long long* within_r = within + (size_t)r * T * 2;
    double* nsd_r = nsd + (size_t)r * T;
    hipError_t e = hipMemsetAsync(counts_r, 0, 5 * sizeof(unsigned long long), s);
    if (e != hipSuccess) return (int)e;
    int o[3], b[3];
    if (!map_box_grow(boxes + 6 * r, D, H, W, o, b)) {
      // absent from both maps: the rows a pair of empty masks gets, without a border pass or a transform
      e = hipMemsetAsync(within_r, 0, (size_t)T * 2 * sizeof(unsigned long long), s);
      if (e != hipSuccess) return (int)e;
      hipLaunchKernelGGL(dua::surface_finish_kernel, dim3(1), dim3(256), 0, s, 1, vox, counts_r, (const double*)nullptr, 0,
                         (const unsigned long long*)nullptr, (const unsigned long long*)nullptr,
                         (const unsigned long long*)nullptr, nan_for_nonexisting, out_r);
      hipLaunchKernelGGL(dua::surface_dice_finish_kernel, dim3((T + 255) / 256), dim3(256), 0, s, 1, T, counts_r, within_r,
                         nan_for_nonexisting, nsd_r);
      continue;
    }
    const dua::SurfaceScratch L = dua::scratch_layout(1, b[0], b[1], b[2]);
    const long svs = dua::align256((long)b[0] * b[1] * b[2]);
    hipLaunchKernelGGL(dua::surface_map_masks_kernel, dim3((unsigned)((svs + dua::SURF_BLOCK_VOX - 1) / dua::SURF_BLOCK_VOX)),
                       dim3(dua::SURF_THREADS), 0, s, test + (size_t)n * test_vstride, reference + (size_t)n * reference_vstride,
                       class_ids[k], H, W, o[0], o[1], o[2], b[0], b[1], b[2], connectivity, ws + L.surf, svs, counts_r);
    dua::SurfaceTolerances tol;
    for (int i = 0; i < DUA_SURFACE_MAX_TOLERANCE_ENTRIES; ++i) tol.t2[i] = i < T ? all.t2[(size_t)k * T + i] : -1.0;
    const int rc = surface_table_tail(1, b[0], b[1], b[2], vox, sd, sh, sw, nan_for_nonexisting, counts_r, out_r, ws, L, 1, T, &tol,
                                      within_r, nsd_r, s);
    if (rc) return rc;
  }
  return (int)hipGetLastError();
}

}  // extern "C"
