// Case preparation on the device: the deterministic front of the reference's transform chain (utils.py:125-136, :168-177:
// ScaleIntensityRanged, CropForegroundd, Orientationd, Spacingd) as one box pass and one fused gather, and the nearest gather
// back to the grid of the scan.  The contract (window, box, orientation rule, coordinates, lerp order) is written down in
// include/dua_hip.h ("case preparation"); this file only says how it is computed.
//
//   box      : one streaming pass, 8 voxels per thread and step (one 16-byte load of int16, two of fp32).  Most of a CT scan is
//              air: a run without a voxel above a_min costs the loads and a compare, and only a run with foreground pays for
//              its (x0, x1, x2).  Six extrema and a count per thread, combined across the wave with shuffles, across the
//              workgroup with LDS integer atomics and across the grid with one global integer atomic per word and workgroup:
//              order-independent, so identical between runs.
//   resample : the direct gather.  A thread owns 4 consecutive prepared voxels of one row along W: the D and H table entries
//              are read once, the W entries per voxel; 8 source elements and one label byte per voxel straight from global
//              memory (orientation is three signed strides, so every one of the 48 is this code), the window applied to each
//              source element, seven lerps, one 16-byte image store and one 4-byte label store when the row length is a
//              multiple of 4 (element stores otherwise).  The kernel computes no coordinate: the tables come from the host.
//   restore  : the nearest gather in the other direction, the same thread shape over the source grid, C channels per thread.
// -ffp-contract=off (csrc/Makefile) and the pragma below keep b - a rounded on its own before the explicit fmaf of a lerp.
#include <limits.h>

#include "common.hpp"
#include "../../include/dua_hip.h"

#pragma clang fp contract(off)

namespace dua {

constexpr int PREP_THREADS = 256;
constexpr int PREP_RUN = 8;                               // source voxels per thread and step of the box pass
constexpr int PREP_MAX_BLOCKS = 4096;
constexpr int PREP_VEC = 4;                               // prepared voxels per thread of the gathers

__device__ __forceinline__ float prep_window(float v, float a_min, float range) {
  return fminf(fmaxf((v - a_min) / range, 0.f), 1.f);     // fmaxf(NaN, 0) = 0
}

// bit e of the result: element e of the run at p is above a_min (n < PREP_RUN elements exist at the end of the volume)
__device__ __forceinline__ unsigned prep_fg_mask(const short* p, bool wide, int n, float a_min) {
  unsigned m = 0;
  if (wide && n == PREP_RUN) {
    const uint4 q = *reinterpret_cast<const uint4*>(p);
    const unsigned wd[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int e = 0; e < PREP_RUN; ++e) m |= ((float)(short)(wd[e >> 1] >> (16 * (e & 1))) > a_min ? 1u : 0u) << e;
  } else {
#pragma unroll
    for (int e = 0; e < PREP_RUN; ++e) m |= (e < n && (float)p[e] > a_min ? 1u : 0u) << e;
  }
  return m;
}
__device__ __forceinline__ unsigned prep_fg_mask(const float* p, bool wide, int n, float a_min) {
  unsigned m = 0;
  if (wide && n == PREP_RUN) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) m |= (a[e] > a_min ? 1u : 0u) << e | (b[e] > a_min ? 1u : 0u) << (e + 4);
  } else {
#pragma unroll
    for (int e = 0; e < PREP_RUN; ++e) m |= (e < n && p[e] > a_min ? 1u : 0u) << e;
  }
  return m;
}

__global__ void prep_box_init_kernel(int* __restrict__ result) {
  if (threadIdx.x < 8) result[threadIdx.x] = threadIdx.x < 3 ? INT_MAX : (threadIdx.x < 6 ? -1 : 0);
}

// result[0..2] = min, result[3..5] = max index per source axis, result[6] = count over the voxels above a_min
template <typename T>
__global__ void __launch_bounds__(PREP_THREADS) prep_box_kernel(const T* __restrict__ src, long voxels, int X1, int X2, float a_min,
                                                                bool wide, int* __restrict__ result) {
  __shared__ int part[8];
  const int tid = threadIdx.x;
  if (tid < 8) part[tid] = tid < 3 ? INT_MAX : (tid < 6 ? -1 : 0);
  __syncthreads();
  int mn[3] = {INT_MAX, INT_MAX, INT_MAX}, mx[3] = {-1, -1, -1}, cnt = 0;
  const long groups = (voxels + PREP_RUN - 1) / PREP_RUN;
  for (long g = (long)blockIdx.x * PREP_THREADS + tid; g < groups; g += (long)gridDim.x * PREP_THREADS) {
    const long i0 = g * PREP_RUN;
    const int n = (int)min((long)PREP_RUN, voxels - i0);
    const unsigned m = prep_fg_mask(src + i0, wide, n, a_min);
    if (m == 0) continue;
    const unsigned line = (unsigned)i0 / (unsigned)X2;    // voxels < 2^31
    int c = (int)((unsigned)i0 - line * (unsigned)X2), a = (int)(line / (unsigned)X1), b = (int)(line - (unsigned)a * (unsigned)X1);
    cnt += __popc(m);
    if (c + PREP_RUN <= X2) {                             // the run lies in one row
      mn[0] = min(mn[0], a); mx[0] = max(mx[0], a);
      mn[1] = min(mn[1], b); mx[1] = max(mx[1], b);
      mn[2] = min(mn[2], c + (__ffs(m) - 1)); mx[2] = max(mx[2], c + (31 - __clz(m)));
    } else {
#pragma unroll
      for (int e = 0; e < PREP_RUN; ++e) {
        if (m >> e & 1) {
          mn[0] = min(mn[0], a); mx[0] = max(mx[0], a);
          mn[1] = min(mn[1], b); mx[1] = max(mx[1], b);
          mn[2] = min(mn[2], c); mx[2] = max(mx[2], c);
        }
        if (++c == X2) { c = 0; if (++b == X1) { b = 0; ++a; } }
      }
    }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      mn[j] = min(mn[j], __shfl_xor(mn[j], off));
      mx[j] = max(mx[j], __shfl_xor(mx[j], off));
    }
    cnt += __shfl_xor(cnt, off);
  }
  if ((tid & 63) == 0 && cnt) {
#pragma unroll
    for (int j = 0; j < 3; ++j) { atomicMin(&part[j], mn[j]); atomicMax(&part[3 + j], mx[j]); }
    atomicAdd(&part[6], cnt);
  }
  __syncthreads();
  if (part[6] == 0) return;                               // workgroup-uniform: nothing above a_min here
  // the extrema only ever move one way, so a workgroup that cannot improve the word it reads (however stale) cannot improve the
  // current one either and skips its atomic: after the first few workgroups only the count is still added by everyone
  if (tid < 6) {
    const int seen = __hip_atomic_load(&result[tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (tid < 3 ? part[tid] < seen : part[tid] > seen) {
      if (tid < 3) atomicMin(&result[tid], part[tid]);
      else atomicMax(&result[tid], part[tid]);
    }
  } else if (tid == 6) {
    atomicAdd(&result[6], part[6]);
  }
}

struct PrepArgs {
  int n_in[3], n_out[3];
  int st[3], base;                                        // element strides and base offset: |.| < 2^31 (checked by the launcher)
  const int* lo;
  const float* wt;
  const int* nr;
  float a_min, range;
};

__device__ __forceinline__ float prep_lerp(float a, float b, float w) { return __builtin_fmaf(w, b - a, a); }

// wide: rows of the prepared volume are a multiple of 4 long and both outputs are aligned for their vector store
template <typename T, bool LABEL>
__global__ void __launch_bounds__(PREP_THREADS) prep_resample_kernel(const T* __restrict__ src,
                                                                     const unsigned char* __restrict__ src_label, PrepArgs p,
                                                                     bool wide, float* __restrict__ image,
                                                                     unsigned char* __restrict__ label) {
  const int N1 = p.n_out[1], N2 = p.n_out[2];
  const unsigned G = (unsigned)(N2 + PREP_VEC - 1) / PREP_VEC;
  const unsigned t = blockIdx.x * (unsigned)PREP_THREADS + threadIdx.x;      // rows x G < 2^31
  const unsigned row = t / G;
  if (row >= (unsigned)p.n_out[0] * (unsigned)N1) return;
  const int i2 = (int)(t - row * G) * PREP_VEC;
  const int i0 = (int)(row / (unsigned)N1), i1 = (int)(row - (unsigned)i0 * (unsigned)N1);
  const int n = min(PREP_VEC, N2 - i2);
  const int t1 = p.n_out[0] + i1, t2 = p.n_out[0] + N1 + i2;                // table rows of axes 1 and 2
  // D and H: one table entry each for the whole run
  const int l0 = min(max(p.lo[i0], 0), p.n_in[0] - 1), h0 = min(l0 + 1, p.n_in[0] - 1);
  const int l1 = min(max(p.lo[t1], 0), p.n_in[1] - 1), h1 = min(l1 + 1, p.n_in[1] - 1);
  const float w0 = p.wt[i0], w1 = p.wt[t1];
  const int corner[2][2] = {{p.base + l0 * p.st[0] + l1 * p.st[1], p.base + l0 * p.st[0] + h1 * p.st[1]},
                            {p.base + h0 * p.st[0] + l1 * p.st[1], p.base + h0 * p.st[0] + h1 * p.st[1]}};
  int lab_row = 0;
  if constexpr (LABEL) {
    const int n0 = min(max(p.nr[i0], 0), p.n_in[0] - 1), n1 = min(max(p.nr[t1], 0), p.n_in[1] - 1);
    lab_row = p.base + n0 * p.st[0] + n1 * p.st[1];
  }
  float raw[PREP_VEC][2][2][2], w2[PREP_VEC];
  unsigned char lb[PREP_VEC];
#pragma unroll
  for (int e = 0; e < PREP_VEC; ++e) {
    const int q = t2 + min(e, n - 1);                     // a lane past the end of the row repeats the last voxel
    const int l2 = min(max(p.lo[q], 0), p.n_in[2] - 1), h2 = min(l2 + 1, p.n_in[2] - 1);
    w2[e] = p.wt[q];
#pragma unroll
    for (int dz = 0; dz < 2; ++dz)
#pragma unroll
      for (int hy = 0; hy < 2; ++hy) {
        raw[e][dz][hy][0] = (float)src[corner[dz][hy] + l2 * p.st[2]];
        raw[e][dz][hy][1] = (float)src[corner[dz][hy] + h2 * p.st[2]];
      }
    if constexpr (LABEL) lb[e] = src_label[lab_row + min(max(p.nr[q], 0), p.n_in[2] - 1) * p.st[2]];
  }
  float out[PREP_VEC];
#pragma unroll
  for (int e = 0; e < PREP_VEC; ++e) {
    float s[2];
#pragma unroll
    for (int dz = 0; dz < 2; ++dz) {
      float r[2];
#pragma unroll
      for (int hy = 0; hy < 2; ++hy)                      // W first
        r[hy] = prep_lerp(prep_window(raw[e][dz][hy][0], p.a_min, p.range), prep_window(raw[e][dz][hy][1], p.a_min, p.range), w2[e]);
      s[dz] = prep_lerp(r[0], r[1], w1);                  // then H
    }
    out[e] = prep_lerp(s[0], s[1], w0);                   // then D
  }
  const long o = (long)row * N2 + i2;
  if (wide) {                                             // n == 4 for every thread
    f32x4 v;
#pragma unroll
    for (int e = 0; e < PREP_VEC; ++e) v[e] = out[e];
    *reinterpret_cast<f32x4*>(image + o) = v;
    if constexpr (LABEL)
      *reinterpret_cast<unsigned*>(label + o) = (unsigned)lb[0] | (unsigned)lb[1] << 8 | (unsigned)lb[2] << 16 | (unsigned)lb[3] << 24;
  } else {
#pragma unroll
    for (int e = 0; e < PREP_VEC; ++e)
      if (e < n) {
        image[o + e] = out[e];
        if constexpr (LABEL) label[o + e] = lb[e];
      }
  }
}

// out[c][x0][x1][x2] = mask[c][tab0[x0] + tab1[x1] + tab2[x2]], 0 where a table entry is negative
__global__ void __launch_bounds__(PREP_THREADS) prep_restore_kernel(const unsigned char* __restrict__ mask, long pv, int C, int X0,
                                                                    int X1, int X2, const int* __restrict__ tab0,
                                                                    const int* __restrict__ tab1, const int* __restrict__ tab2,
                                                                    bool wide, unsigned char* __restrict__ out) {
  const unsigned G = (unsigned)(X2 + PREP_VEC - 1) / PREP_VEC;
  const unsigned t = blockIdx.x * (unsigned)PREP_THREADS + threadIdx.x;
  const unsigned row = t / G;
  if (row >= (unsigned)X0 * (unsigned)X1) return;
  const int x2 = (int)(t - row * G) * PREP_VEC;
  const int x0 = (int)(row / (unsigned)X1), x1 = (int)(row - (unsigned)x0 * (unsigned)X1);
  const int n = min(PREP_VEC, X2 - x2);
  const int a = tab0[x0], b = tab1[x1];
  long off[PREP_VEC];
#pragma unroll
  for (int e = 0; e < PREP_VEC; ++e) {
    const int c = tab2[x2 + min(e, n - 1)];
    const long s = (long)a + b + c;
    off[e] = (a | b | c) >= 0 && s < pv ? s : -1;
  }
  const long sv = (long)X0 * X1 * X2, o = (long)row * X2 + x2;
  for (int ch = 0; ch < C; ++ch) {
    const unsigned char* m = mask + (long)ch * pv;
    unsigned char v[PREP_VEC];
#pragma unroll
    for (int e = 0; e < PREP_VEC; ++e) v[e] = off[e] >= 0 ? m[off[e]] : (unsigned char)0;
    unsigned char* dst = out + (long)ch * sv + o;
    if (wide) {
      *reinterpret_cast<unsigned*>(dst) = (unsigned)v[0] | (unsigned)v[1] << 8 | (unsigned)v[2] << 16 | (unsigned)v[3] << 24;
    } else {
#pragma unroll
      for (int e = 0; e < PREP_VEC; ++e)
        if (e < n) dst[e] = v[e];
    }
  }
}

static bool extents_ok(long a, long b, long c) {          // three positive extents whose product is below 2^31
  return a >= 1 && b >= 1 && c >= 1 && a < (1L << 31) && b < (1L << 31) && c < (1L << 31) && a * b < (1L << 31) &&
         a * b * c < (1L << 31);
}

}  // namespace dua

extern "C" {

int dua_prep_foreground_box(int dtype, const void* src, int X0, int X1, int X2, float a_min, int* result, void* stream) {
  if ((dtype != DUA_I16 && dtype != DUA_F32) || !src || !result || !dua::extents_ok(X0, X1, X2) || !(a_min - a_min == 0.f))
    return DUA_ERR_ARG;
  const long voxels = (long)X0 * X1 * X2;
  hipStream_t s = (hipStream_t)stream;
  const long per_block = (long)dua::PREP_RUN * dua::PREP_THREADS;
  const long blocks = (voxels + per_block - 1) / per_block;
  const dim3 grid((unsigned)(blocks < dua::PREP_MAX_BLOCKS ? blocks : dua::PREP_MAX_BLOCKS));
  const bool wide = ((size_t)src & 15) == 0;
  hipLaunchKernelGGL(dua::prep_box_init_kernel, dim3(1), dim3(64), 0, s, result);
  if (dtype == DUA_I16)
    hipLaunchKernelGGL(dua::prep_box_kernel<short>, grid, dim3(dua::PREP_THREADS), 0, s, (const short*)src, voxels, X1, X2, a_min,
                       wide, result);
  else
    hipLaunchKernelGGL(dua::prep_box_kernel<float>, grid, dim3(dua::PREP_THREADS), 0, s, (const float*)src, voxels, X1, X2, a_min,
                       wide, result);
  return (int)hipGetLastError();
}

int dua_prep_resample(int dtype, const void* src, const unsigned char* src_label, const dua_prep_geom* geom, const int* lo,
                      const float* weight, const int* nearest, float a_min, float range, float* image, unsigned char* label,
                      void* stream) {
  if ((dtype != DUA_I16 && dtype != DUA_F32) || !src || !geom || !lo || !weight || !nearest || !image ||
      (src_label == nullptr) != (label == nullptr))
    return DUA_ERR_ARG;
  if (!(a_min - a_min == 0.f) || !(range > 0.f && range <= 3.0e38f)) return DUA_ERR_ARG;
  const dua_prep_geom g = *geom;
  if (!dua::extents_ok(g.n_in[0], g.n_in[1], g.n_in[2]) || !dua::extents_ok(g.n_out[0], g.n_out[1], g.n_out[2]) ||
      g.src_voxels < 1 || g.src_voxels >= (1L << 31) || g.base < 0 || g.base >= g.src_voxels)
    return DUA_ERR_ARG;
  // every corner of the oriented box inside the source: with table entries clamped into [0, n_in - 1], no read leaves it
  long lowest = g.base, highest = g.base;
  for (int j = 0; j < 3; ++j) {
    if (g.stride[j] <= -(1L << 31) || g.stride[j] >= (1L << 31)) return DUA_ERR_ARG;
    const long span = (long)(g.n_in[j] - 1) * g.stride[j];               // below 2^62
    if (span < 0) lowest += span; else highest += span;
  }
  if (lowest < 0 || highest >= g.src_voxels) return DUA_ERR_ARG;
  dua::PrepArgs p;
  for (int j = 0; j < 3; ++j) { p.n_in[j] = g.n_in[j]; p.n_out[j] = g.n_out[j]; p.st[j] = (int)g.stride[j]; }
  p.base = (int)g.base; p.lo = lo; p.wt = weight; p.nr = nearest; p.a_min = a_min; p.range = range;
  const long rows = (long)g.n_out[0] * g.n_out[1], groups = rows * ((g.n_out[2] + dua::PREP_VEC - 1) / dua::PREP_VEC);
  const dim3 grid((unsigned)((groups + dua::PREP_THREADS - 1) / dua::PREP_THREADS));
  const bool wide = g.n_out[2] % dua::PREP_VEC == 0 && ((size_t)image & 15) == 0 && ((size_t)label & 3) == 0;
  hipStream_t s = (hipStream_t)stream;
#define DUA_PREP_RESAMPLE(T, LABEL)                                                                                         \
  hipLaunchKernelGGL((dua::prep_resample_kernel<T, LABEL>), grid, dim3(dua::PREP_THREADS), 0, s, (const T*)src, src_label, p, \
                     wide, image, label)
  if (dtype == DUA_I16 && label) DUA_PREP_RESAMPLE(short, true);
  else if (dtype == DUA_I16) DUA_PREP_RESAMPLE(short, false);
  else if (label) DUA_PREP_RESAMPLE(float, true);
  else DUA_PREP_RESAMPLE(float, false);
#undef DUA_PREP_RESAMPLE
  return (int)hipGetLastError();
}

int dua_prep_restore(const unsigned char* mask, long prepared_voxels, int C, int X0, int X1, int X2, const int* tab0,
                     const int* tab1, const int* tab2, unsigned char* out, void* stream) {
  if (!mask || prepared_voxels < 1 || prepared_voxels >= (1L << 31) || C < 1 || C > 65535 || !dua::extents_ok(X0, X1, X2) ||
      !tab0 || !tab1 || !tab2 || !out)
    return DUA_ERR_ARG;
  const long groups = (long)X0 * X1 * ((X2 + dua::PREP_VEC - 1) / dua::PREP_VEC);
  const dim3 grid((unsigned)((groups + dua::PREP_THREADS - 1) / dua::PREP_THREADS));
  const bool wide = X2 % dua::PREP_VEC == 0 && ((size_t)out & 3) == 0;    // X2 % 4 == 0: every channel starts on a 4-byte boundary
  hipLaunchKernelGGL(dua::prep_restore_kernel, grid, dim3(dua::PREP_THREADS), 0, (hipStream_t)stream, mask, prepared_voxels, C,
                     X0, X1, X2, tab0, tab1, tab2, wide, out);
  return (int)hipGetLastError();
}

}  // extern "C"
