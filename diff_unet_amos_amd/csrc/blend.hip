// Streamed sliding-window blend (Engine.infer, engine.py:167-182; Tester, test.py:119-159; metric.py:37-49): window outputs
// are added into a device-resident fp32 sum volume as soon as a predictor call returns, and one pass afterwards divides by the
// window count, crops the padding away, binarises and tallies Dice.  The contract is written down in include/dua_hip.h; this
// file only says how it is computed.
//
//   accumulate : ONE GRID PER WINDOW, enqueued in window-index order inside the call.  Windows of one predictor call overlap
//            each other (scan interval 19 at roi 96, overlap 0.8), so two windows' additions into one voxel need an order; the
//            stream gives it, no atomics, and every voxel sees the fp32 additions of a slice-add per window in index order.
//            A kernel boundary costs 1.5-2 us against >= 30 us of traffic for a 16 x 96^3 window (window read, volume read,
//            volume written: 170 MB), and a call holds sw_batch_size (1..4) windows.
//            The volume side is the read-modify-write side, so the lanes are laid along the VOLUME's 16-byte groups: a window
//            row starts `shift` = (element offset of its first voxel) mod 4 elements into a group, lane g of a row owns group g
//            and does one aligned 16-byte load and store there; the two groups a row only partly covers are done by element.
//            The window side is read at whatever alignment that leaves it (one 16-byte load when shift == 0 and the row is
//            aligned, four dword loads otherwise: reads of one cache line by neighbouring lanes).  A volume whose base is not
//            16-byte aligned takes the one-element-per-lane form.
//            Every lane reads the table row (a wave-uniform load) and clamps it into the volume before forming an address.
//            There is ONE kernel, blend_accumulate_kernel<T, WIDE, WEIGHTED, MIRROR>; the four entry points differ only in its
//            two last flags, and a flag that is off leaves its arguments unread.
//            WEIGHTED (mode="gaussian"): the importance map is never stored.  It is an outer product of three per-axis
//            vectors, clamped from below, so a lane rebuilds w = max((g0[z] g1[y]) g2[x], floor) per voxel from the vectors (a
//            few hundred bytes, cache resident) -- g2 is indexed by the window x of each element, i.e. the group's x0 + j in
//            the shifted wide form.  Every product and sum is a single rounded fp32 operation (__fmul_rn / __fadd_rn): the
//            bits of `out[slice] += w * o`.
//            MIRROR (mirror test-time augmentation): the un-flip of a window predicted under axis flips is a different READ
//            ORDER of the window side.  The lanes still own the volume's 16-byte groups; a flip of D or H only changes which
//            window row a lane reads, and a flip of W means the four volume elements at window x0 .. x0 + 3 come from window
//            elements rw-1-x0-3 .. rw-1-x0: one vector load where that address is aligned (as often as in the unmirrored form
//            when rw is a multiple of 4), reversed in registers.  The importance weight stays indexed by the volume-side
//            (z, y, x): it multiplies the un-flipped output.
//   finish : grid = (blocks, B C): a workgroup stays inside one channel plane, so its Dice tallies are three counters.  When
//            nothing is cropped and a plane is a multiple of 4 voxels, a lane takes 4 consecutive voxels (16-byte load of the
//            sums, 16-byte store of q, 4-byte store of the mask, 16- or 4-byte load of the labels); otherwise one voxel.
//            Counters: per lane -> wave shuffle -> LDS -> one 64-bit integer atomic per counter and workgroup.
//   weight_sum, weighted finish : weight_sum rebuilds the summed weights of the whole volume from the plan's per-axis starts (a
//            voxel loops over the starts that cover it, D-major = window-index order, `cnt[slice] += w` in single rounded
//            additions), and finish divides by that volume instead of the product of three counts, same kernel body.
#include "common.hpp"
#include "../../include/dua_hip.h"

#pragma clang fp contract(off)

namespace dua {

constexpr int BLEND_THREADS = 256;
constexpr int BLEND_FINISH_BLOCKS = 256;      // per channel plane; grid-stride beyond

enum { LABELS_NONE = 0, LABELS_ONEHOT_F32 = 1, LABELS_ONEHOT_U8 = 2, LABELS_MAP_U8 = 3 };

__device__ __forceinline__ int clamp_flag(int v, int hi, bool& bad) {       // into [0, hi]
  if (v < 0) { bad = true; return 0; }
  if (v > hi) { bad = true; return hi; }
  return v;
}

__device__ __forceinline__ f32x4 load4(const float* p) {
  if (((size_t)p & 15) == 0) return *reinterpret_cast<const f32x4*>(p);
  return f32x4{p[0], p[1], p[2], p[3]};
}
__device__ __forceinline__ f32x4 load4(const f16* p) {
  if (((size_t)p & 7) == 0) {
    const f16x4 v = *reinterpret_cast<const f16x4*>(p);
    return f32x4{(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
  }
  return f32x4{(float)p[0], (float)p[1], (float)p[2], (float)p[3]};
}

__device__ __forceinline__ f32x4 reversed(f32x4 v) { return f32x4{v[3], v[2], v[1], v[0]}; }

// w of one voxel from the row's g0[z] g1[y] product: the outer-product order of the map, every product rounded, then the floor
__device__ __forceinline__ float window_weight(float gzy, float gx, float floor_w) { return fmaxf(__fmul_rn(gzy, gx), floor_w); }

// the new sum value: v + o, or v + w o with every operation rounded once
template <bool WEIGHTED>
__device__ __forceinline__ float blend_add(float v, float o, float gzy, float gx, float floor_w) {
  if constexpr (WEIGHTED) return __fadd_rn(v, __fmul_rn(window_weight(gzy, gx, floor_w), o));
  else return v + o;
}

// one window [C][rd][rh][rw] at `win`, its position in `row` (b, d, h, w); grid = (ceil(rh G / threads), rd, C).
// WEIGHTED: sum += w * window with w = max((g0[z] g1[y]) g2[x], floor_w); otherwise g0, g1, g2 and floor_w are not read.
// MIRROR: the window is read un-flipped, sum[.., d + z, h + y, w + x] += win[c, m0(z), m1(y), m2(x)], m_a(i) = r_a - 1 - i when bit
// a of `flip` is set, else i; otherwise `flip` is not read
template <typename T, bool WIDE, bool WEIGHTED, bool MIRROR>
__global__ void __launch_bounds__(BLEND_THREADS)
blend_accumulate_kernel(const T* __restrict__ win, const int* __restrict__ row, float* __restrict__ sum,
                        const float* __restrict__ g0, const float* __restrict__ g1, const float* __restrict__ g2, float floor_w,
                        int B, int C, int rd, int rh, int rw, int Dp, int Hp, int Wp, int G, int* err, int flip) {
  bool bad = false;
  const int b = clamp_flag(row[0], B - 1, bad), d = clamp_flag(row[1], Dp - rd, bad), h = clamp_flag(row[2], Hp - rh, bad),
            w = clamp_flag(row[3], Wp - rw, bad);
  if (bad && err && blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0 && threadIdx.x == 0) *err = 1;
  const int c = blockIdx.z, z = blockIdx.y;
  const int it = blockIdx.x * BLEND_THREADS + threadIdx.x;
  if (it >= rh * G) return;
  const int y = it / G, g = it - y * G;
  const long vrow = ((((long)b * C + c) * Dp + (d + z)) * Hp + (h + y)) * Wp + w;      // volume element of the row's x = 0
  const int wz = MIRROR && (flip & 1) ? rd - 1 - z : z, wy = MIRROR && (flip & 2) ? rh - 1 - y : y;      // the window row read
  const T* wrow = win + (((long)c * rd + wz) * rh + wy) * rw;
  const bool fx = MIRROR && (flip & 4);             // W reversed: volume x reads window rw - 1 - x
  const float gzy = WEIGHTED ? __fmul_rn(g0[z], g1[y]) : 0.f;
  if (WIDE) {
    const int shift = (int)(vrow & 3);
    const int x0 = 4 * g - shift;                   // window x of the group's first element: the index into g2 as well
    if (x0 >= rw) return;
    float* vp = sum + (vrow + x0);                  // 16-byte aligned
    if (x0 >= 0 && x0 + 4 <= rw) {
      f32x4 v = *reinterpret_cast<f32x4*>(vp);
      f32x4 o = load4(wrow + (fx ? rw - 4 - x0 : x0));          // one load either way: the address is selected, not the path
      const f32x4 gx = WEIGHTED ? load4(g2 + x0) : f32x4{};
      if (fx) o = reversed(o);
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = blend_add<WEIGHTED>(v[j], o[j], gzy, gx[j], floor_w);
      *reinterpret_cast<f32x4*>(vp) = v;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int x = x0 + j;
        if (x >= 0 && x < rw)
          vp[j] = blend_add<WEIGHTED>(vp[j], (float)wrow[fx ? rw - 1 - x : x], gzy, WEIGHTED ? g2[x] : 0.f, floor_w);
      }
    }
  } else {
    if (g < rw)
      sum[vrow + g] = blend_add<WEIGHTED>(sum[vrow + g], (float)wrow[fx ? rw - 1 - g : g], gzy, WEIGHTED ? g2[g] : 0.f, floor_w);
  }
}

// wsum [Dp][Hp][Wp]: one voxel per lane, the weights of the windows over it added in window-index order (the window grid is
// the product of the three ascending start lists, D slowest).  A start is only compared with the voxel's coordinate, and the
// vectors are indexed by coordinate - start inside [0, roi): no start value can lead outside them.
__global__ void __launch_bounds__(BLEND_THREADS)
blend_weight_sum_kernel(const int* __restrict__ sd, int nsd, const int* __restrict__ sh, int nsh, const int* __restrict__ sw,
                        int nsw, int rd, int rh, int rw, const float* __restrict__ g0, const float* __restrict__ g1,
                        const float* __restrict__ g2, float floor_w, float* __restrict__ wsum, int Hp, int Wp, unsigned V) {
  const unsigned i = blockIdx.x * BLEND_THREADS + threadIdx.x;             // V < 2^31: no wrap
  if (i >= V) return;
  const int x = (int)(i % (unsigned)Wp);
  const unsigned r = i / (unsigned)Wp;
  const int y = (int)(r % (unsigned)Hp), z = (int)(r / (unsigned)Hp);
  float acc = 0.f;
  for (int a = 0; a < nsd; ++a) {
    const int dz = z - sd[a];
    if (dz < 0 || dz >= rd) continue;
    const float gz = g0[dz];
    for (int k = 0; k < nsh; ++k) {
      const int dy = y - sh[k];
      if (dy < 0 || dy >= rh) continue;
      const float gzy = __fmul_rn(gz, g1[dy]);
      for (int m = 0; m < nsw; ++m) {
        const int dx = x - sw[m];
        if (dx < 0 || dx >= rw) continue;
        acc = __fadd_rn(acc, window_weight(gzy, g2[dx], floor_w));
      }
    }
  }
  wsum[i] = acc;
}

__device__ __forceinline__ bool sigmoid_above_half(float q) { return 1.f / (1.f + expf(-q)) > 0.5f; }

// WEIGHTED: the divisor is wsum [Dp][Hp][Wp] (blend_weight_sum_kernel) and nd, nh, nw are not read; otherwise the count
// nd[z] nh[y] nw[x] and wsum is not read
template <int VEC, bool WEIGHTED>
__global__ void __launch_bounds__(BLEND_THREADS) blend_finish_kernel(const float* __restrict__ sum, int C, int Dp, int Hp, int Wp,
                                                                     const int* __restrict__ nd, const int* __restrict__ nh,
                                                                     const int* __restrict__ nw, const float* __restrict__ wsum,
                                                                     int od, int oh, int ow, int D,
                                                                     int H, int W, float* __restrict__ q_out,
                                                                     unsigned char* __restrict__ mask_out,
                                                                     const void* __restrict__ labels, int label_kind,
                                                                     unsigned long long* __restrict__ tallies) {
  __shared__ unsigned part[3][BLEND_THREADS / 64];
  const int plane = blockIdx.y, c = plane % C, b = plane / C;
  const long V = (long)D * H * W;
  const long obase = (long)plane * V;                         // q, mask and one-hot labels: [B][C][D][H][W]
  const long lbase = label_kind == LABELS_MAP_U8 ? (long)b * V : obase;
  const float* lf = reinterpret_cast<const float*>(labels);
  const unsigned char* lu = reinterpret_cast<const unsigned char*>(labels);
  unsigned t_and = 0, t_a = 0, t_b = 0;
  for (long i = ((long)blockIdx.x * BLEND_THREADS + threadIdx.x) * VEC; i < V; i += (long)gridDim.x * BLEND_THREADS * VEC) {
    int x = (int)(i % W);
    const long r = i / W;
    int y = (int)(r % H), z = (int)(r / H);
    float s[VEC], den[VEC] = {};
    bool lab[VEC] = {};
    if constexpr (VEC == 4) {                                 // nothing cropped: the sum plane has the output's layout
      const f32x4 v = *reinterpret_cast<const f32x4*>(sum + obase + i);
      s[0] = v[0]; s[1] = v[1]; s[2] = v[2]; s[3] = v[3];
      if constexpr (WEIGHTED) {
        const f32x4 t = *reinterpret_cast<const f32x4*>(wsum + i);
        den[0] = t[0]; den[1] = t[1]; den[2] = t[2]; den[3] = t[3];
      }
      if (label_kind == LABELS_ONEHOT_F32) {
        const f32x4 l = *reinterpret_cast<const f32x4*>(lf + lbase + i);
#pragma unroll
        for (int j = 0; j < VEC; ++j) lab[j] = l[j] != 0.f;
      } else if (label_kind != LABELS_NONE) {
        const unsigned l = *reinterpret_cast<const unsigned*>(lu + lbase + i);
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
          const unsigned byte = (l >> (8 * j)) & 255u;
          lab[j] = label_kind == LABELS_MAP_U8 ? byte == (unsigned)c : byte != 0;
        }
      }
    } else {
      s[0] = sum[(((long)plane * Dp + (od + z)) * Hp + (oh + y)) * Wp + (ow + x)];
      if constexpr (WEIGHTED) den[0] = wsum[((long)(od + z) * Hp + (oh + y)) * Wp + (ow + x)];
      if (label_kind == LABELS_ONEHOT_F32) lab[0] = lf[lbase + i] != 0.f;
      else if (label_kind == LABELS_ONEHOT_U8) lab[0] = lu[lbase + i] != 0;
      else if (label_kind == LABELS_MAP_U8) lab[0] = lu[lbase + i] == (unsigned)c;
    }
    float q[VEC];
    unsigned m = 0;
    int ndh = 0;
    if constexpr (!WEIGHTED) ndh = nd[od + z] * nh[oh + y];
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      if constexpr (WEIGHTED) q[j] = s[j] / den[j];
      else q[j] = s[j] / (float)(ndh * nw[ow + x]);
      const bool a = sigmoid_above_half(q[j]);
      m |= (unsigned)a << (8 * j);
      if (label_kind != LABELS_NONE) {
        t_a += a;
        t_b += lab[j];
        t_and += a && lab[j];
      }
      if (j + 1 < VEC && ++x == W) {                          // the next voxel starts a row
        x = 0;
        if (++y == H) { y = 0; ++z; }
        if constexpr (!WEIGHTED) ndh = nd[od + z] * nh[oh + y];
      }
    }
    if constexpr (VEC == 4) {
      if (q_out) *reinterpret_cast<f32x4*>(q_out + obase + i) = f32x4{q[0], q[1], q[2], q[3]};
      if (mask_out) *reinterpret_cast<unsigned*>(mask_out + obase + i) = m;
    } else {
      if (q_out) q_out[obase + i] = q[0];
      if (mask_out) mask_out[obase + i] = (unsigned char)m;
    }
  }
  if (label_kind == LABELS_NONE) return;                      // uniform over the grid
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    t_and += __shfl_down(t_and, off, 64);
    t_a += __shfl_down(t_a, off, 64);
    t_b += __shfl_down(t_b, off, 64);
  }
  const int tid = threadIdx.x;
  if ((tid & 63) == 0) { part[0][tid >> 6] = t_and; part[1][tid >> 6] = t_a; part[2][tid >> 6] = t_b; }
  __syncthreads();
  if (tid < 3) {
    unsigned long long v = 0;
#pragma unroll
    for (int k = 0; k < BLEND_THREADS / 64; ++k) v += part[tid][k];
    if (v) atomicAdd(&tallies[c * 3 + tid], v);
  }
}

}  // namespace dua

// the four accumulate entry points: `weighted` says whether g0, g1, g2, floor_w are given, flip == 0 launches the unmirrored
// instantiation
static int blend_accumulate_launch(int dtype, int nb, int C, int rd, int rh, int rw, const void* windows, const int* table,
                                   int table_rows, int table_off, int table_stride, int flip, bool weighted, const float* g0,
                                   const float* g1, const float* g2, float floor_w, float* sum, int B, int Dp, int Hp, int Wp,
                                   int* err_word, void* stream) {
  if ((dtype != DUA_F32 && dtype != DUA_F16) || nb < 1 || C < 1 || C > DUA_BLEND_MAX_CLASSES || !windows || !table || !sum)
    return DUA_ERR_ARG;
  if (rd < 1 || rh < 1 || rw < 1 || B < 1 || Dp < rd || Hp < rh || Wp < rw || rd > 65535) return DUA_ERR_ARG;
  if (table_rows < 1 || table_off < 0 || table_stride < 1 || (long)table_off + (long)(nb - 1) * table_stride >= table_rows)
    return DUA_ERR_ARG;
  if ((long)Dp * Hp * Wp >= (1L << 31) || (long)rd * rh * rw >= (1L << 31)) return DUA_ERR_ARG;
  if (((size_t)windows & (dtype == DUA_F16 ? 1 : 3)) || ((size_t)sum & 3) || ((size_t)table & 3)) return DUA_ERR_ARG;
  if (weighted && (!g0 || !g1 || !g2 || (((size_t)g0 | (size_t)g1 | (size_t)g2) & 3) || !(floor_w > 0.f))) return DUA_ERR_ARG;
  if (flip < 0 || flip > 7) return DUA_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  const bool wide = ((size_t)sum & 15) == 0;
  const int G = wide ? (rw + 3) / 4 + 1 : rw;                // groups a row can touch at any shift
  const dim3 grid((unsigned)(((long)rh * G + dua::BLEND_THREADS - 1) / dua::BLEND_THREADS), rd, C);
  const long wvox = (long)C * rd * rh * rw;
  for (int k = 0; k < nb; ++k) {                              // stream order = window-index order
    const int* row = table + 4 * ((long)table_off + (long)k * table_stride);
#define DUA_BLEND_ACC(T, WIDE, WEIGHTED, MIRROR)                                                                            \
  hipLaunchKernelGGL((dua::blend_accumulate_kernel<T, WIDE, WEIGHTED, MIRROR>), grid, dim3(dua::BLEND_THREADS), 0, s,       \
                     reinterpret_cast<const T*>(windows) + k * wvox, row, sum, g0, g1, g2, floor_w, B, C, rd, rh, rw, Dp, Hp, Wp, \
                     G, err_word, flip)
#define DUA_BLEND_ACC_M(T, WIDE, WEIGHTED)                                                                                  \
  if (flip) DUA_BLEND_ACC(T, WIDE, WEIGHTED, true); else DUA_BLEND_ACC(T, WIDE, WEIGHTED, false)
#define DUA_BLEND_ACC_W(T, WIDE) if (weighted) { DUA_BLEND_ACC_M(T, WIDE, true); } else { DUA_BLEND_ACC_M(T, WIDE, false); }
#define DUA_BLEND_ACC_T(T) if (wide) { DUA_BLEND_ACC_W(T, true) } else { DUA_BLEND_ACC_W(T, false) }
    if (dtype == DUA_F32) { DUA_BLEND_ACC_T(float) } else { DUA_BLEND_ACC_T(dua::f16) }
#undef DUA_BLEND_ACC_T
#undef DUA_BLEND_ACC_W
#undef DUA_BLEND_ACC_M
#undef DUA_BLEND_ACC
  }
  return (int)hipGetLastError();
}

int dua_blend_accumulate(int dtype, int nb, int C, int rd, int rh, int rw, const void* windows, const int* table, int table_rows,
                         int table_off, int table_stride, float* sum, int B, int Dp, int Hp, int Wp, int* err_word,
                         void* stream) {
  return blend_accumulate_launch(dtype, nb, C, rd, rh, rw, windows, table, table_rows, table_off, table_stride, 0, false, nullptr,
                                 nullptr, nullptr, 0.f, sum, B, Dp, Hp, Wp, err_word, stream);
}

int dua_blend_accumulate_mirrored(int dtype, int nb, int C, int rd, int rh, int rw, const void* windows, const int* table,
                                  int table_rows, int table_off, int table_stride, int flip, float* sum, int B, int Dp, int Hp,
                                  int Wp, int* err_word, void* stream) {
  return blend_accumulate_launch(dtype, nb, C, rd, rh, rw, windows, table, table_rows, table_off, table_stride, flip, false,
                                 nullptr, nullptr, nullptr, 0.f, sum, B, Dp, Hp, Wp, err_word, stream);
}

int dua_blend_accumulate_weighted(int dtype, int nb, int C, int rd, int rh, int rw, const void* windows, const int* table,
                                  int table_rows, int table_off, int table_stride, const float* g0, const float* g1,
                                  const float* g2, float floor_w, float* sum, int B, int Dp, int Hp, int Wp, int* err_word,
                                  void* stream) {
  return blend_accumulate_launch(dtype, nb, C, rd, rh, rw, windows, table, table_rows, table_off, table_stride, 0, true, g0, g1,
                                 g2, floor_w, sum, B, Dp, Hp, Wp, err_word, stream);
}

int dua_blend_accumulate_weighted_mirrored(int dtype, int nb, int C, int rd, int rh, int rw, const void* windows, const int* table,
                                           int table_rows, int table_off, int table_stride, int flip, const float* g0,
                                           const float* g1, const float* g2, float floor_w, float* sum, int B, int Dp, int Hp,
                                           int Wp, int* err_word, void* stream) {
  return blend_accumulate_launch(dtype, nb, C, rd, rh, rw, windows, table, table_rows, table_off, table_stride, flip, true, g0, g1,
                                 g2, floor_w, sum, B, Dp, Hp, Wp, err_word, stream);
}

int dua_blend_weight_sum(const int* starts_d, int nd, const int* starts_h, int nh, const int* starts_w, int nw, int rd, int rh,
                         int rw, const float* g0, const float* g1, const float* g2, float floor_w, float* wsum, int Dp, int Hp,
                         int Wp, void* stream) {
  if (!starts_d || !starts_h || !starts_w || !g0 || !g1 || !g2 || !wsum || nd < 1 || nh < 1 || nw < 1) return DUA_ERR_ARG;
  if (rd < 1 || rh < 1 || rw < 1 || Dp < rd || Hp < rh || Wp < rw || (long)Dp * Hp * Wp >= (1L << 31)) return DUA_ERR_ARG;
  if ((((size_t)starts_d | (size_t)starts_h | (size_t)starts_w | (size_t)g0 | (size_t)g1 | (size_t)g2 | (size_t)wsum) & 3) ||
      !(floor_w > 0.f))
    return DUA_ERR_ARG;
  const long V = (long)Dp * Hp * Wp;
  hipLaunchKernelGGL(dua::blend_weight_sum_kernel, dim3((unsigned)((V + dua::BLEND_THREADS - 1) / dua::BLEND_THREADS)),
                     dim3(dua::BLEND_THREADS), 0, (hipStream_t)stream, starts_d, nd, starts_h, nh, starts_w, nw, rd, rh, rw, g0, g1,
                     g2, floor_w, wsum, Hp, Wp, (unsigned)V);
  return (int)hipGetLastError();
}

// dua_blend_finish (wsum == nullptr: the count vectors) and dua_blend_finish_weighted (wsum, no count vectors)
static int blend_finish_launch(const float* sum, int B, int C, int Dp, int Hp, int Wp, const int* nd, const int* nh, const int* nw,
                               const float* wsum, int od, int oh, int ow, int D, int H, int W, float* q_out,
                               unsigned char* mask_out, const void* labels, int labels_dtype, int label_map,
                               unsigned long long* tallies, void* stream) {
  if (!sum || ((size_t)wsum & 3) || B < 1 || C < 1 || C > DUA_BLEND_MAX_CLASSES || (long)B * C > 65535) return DUA_ERR_ARG;
  if (D < 1 || H < 1 || W < 1 || od < 0 || oh < 0 || ow < 0 || od > Dp - D || oh > Hp - H || ow > Wp - W) return DUA_ERR_ARG;
  if ((long)Dp * Hp * Wp >= (1L << 31)) return DUA_ERR_ARG;
  if (!q_out && !mask_out && !tallies) return DUA_ERR_ARG;
  if ((labels != nullptr) != (tallies != nullptr)) return DUA_ERR_ARG;
  int kind = dua::LABELS_NONE;
  if (labels) {
    if (label_map) {
      if (labels_dtype != DUA_U8) return DUA_ERR_ARG;
      kind = dua::LABELS_MAP_U8;
    } else if (labels_dtype == DUA_F32) kind = dua::LABELS_ONEHOT_F32;
    else if (labels_dtype == DUA_U8) kind = dua::LABELS_ONEHOT_U8;
    else return DUA_ERR_ARG;
  }
  if (((size_t)sum & 3) || ((size_t)q_out & 3) || (kind == dua::LABELS_ONEHOT_F32 && ((size_t)labels & 3)) || ((size_t)tallies & 7))
    return DUA_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  if (tallies) {
    const hipError_t e = hipMemsetAsync(tallies, 0, sizeof(unsigned long long) * 3 * C, s);
    if (e != hipSuccess) return (int)e;
  }
  const long V = (long)D * H * W;
  const bool wide = D == Dp && H == Hp && W == Wp && V % 4 == 0 && ((size_t)sum & 15) == 0 && ((size_t)q_out & 15) == 0 &&
                    ((size_t)mask_out & 3) == 0 && ((size_t)labels & (kind == dua::LABELS_ONEHOT_F32 ? 15 : 3)) == 0 &&
                    ((size_t)wsum & 15) == 0;
  const long items = wide ? V / 4 : V;
  long blocks = (items + dua::BLEND_THREADS - 1) / dua::BLEND_THREADS;
  if (blocks > dua::BLEND_FINISH_BLOCKS) blocks = dua::BLEND_FINISH_BLOCKS;
  const dim3 grid((unsigned)blocks, (unsigned)(B * C));
#define DUA_BLEND_FINISH(VEC, WEIGHTED)                                                                                     \
  hipLaunchKernelGGL((dua::blend_finish_kernel<VEC, WEIGHTED>), grid, dim3(dua::BLEND_THREADS), 0, s, sum, C, Dp, Hp, Wp, nd, nh, \
                     nw, wsum, od, oh, ow, D, H, W, q_out, mask_out, labels, kind, tallies)
  if (wsum) { if (wide) DUA_BLEND_FINISH(4, true); else DUA_BLEND_FINISH(1, true); }
  else { if (wide) DUA_BLEND_FINISH(4, false); else DUA_BLEND_FINISH(1, false); }
#undef DUA_BLEND_FINISH
  return (int)hipGetLastError();
}

int dua_blend_finish(const float* sum, int B, int C, int Dp, int Hp, int Wp, const int* nd, const int* nh, const int* nw, int od,
                     int oh, int ow, int D, int H, int W, float* q_out, unsigned char* mask_out, const void* labels,
                     int labels_dtype, int label_map, unsigned long long* tallies, void* stream) {
  if (!nd || !nh || !nw) return DUA_ERR_ARG;
  return blend_finish_launch(sum, B, C, Dp, Hp, Wp, nd, nh, nw, nullptr, od, oh, ow, D, H, W, q_out, mask_out, labels,
                             labels_dtype, label_map, tallies, stream);
}

int dua_blend_finish_weighted(const float* sum, int B, int C, int Dp, int Hp, int Wp, const float* wsum, int od, int oh, int ow,
                              int D, int H, int W, float* q_out, unsigned char* mask_out, const void* labels, int labels_dtype,
                              int label_map, unsigned long long* tallies, void* stream) {
  if (!wsum) return DUA_ERR_ARG;
  return blend_finish_launch(sum, B, C, Dp, Hp, Wp, nullptr, nullptr, nullptr, wsum, od, oh, ow, D, H, W, q_out, mask_out, labels,
                             labels_dtype, label_map, tallies, stream);
}
