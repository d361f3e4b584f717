// Label map on the grid of the scan, straight from the blended sum volume (the deliverable behind Engine.infer, engine.py:167-182:
// one organ per voxel of the scan; the usual export resamples the class probabilities to the scan's grid and takes the arg-max
// there).  The contract (tables, corner logits, sigmoid, lerp order, tie and threshold rules, tallies) is written down in
// include/dua_hip.h ("label map on the grid of the scan"); this file only says how it is computed.
//
//   one launch : the thread shape of prep_restore_kernel over the SOURCE grid -- a thread owns 4 consecutive voxels of one row
//            along X2 and walks further runs in a grid-stride loop (the grid is capped, so the tallies cost a bounded number of
//            global atomics).  The table entries of source axes 0 and 1 are read once per run, those of axis 2 per voxel.  A
//            voxel with a negative entry is outside the foreground box: label 0, nothing else read.
//   per voxel  : the three (lower index, upper index, weight) triples are sorted from source-axis order into prepared-axis
//            order with wave-uniform selects (the permutation is a launch argument), which fixes the 8 corner offsets into a
//            channel plane of the sum volume and the 8 divisors once; then c walks the channels: 8 loads, 8 IEEE divisions,
//            8 sigmoids, 7 lerps and one strict compare against the running best (p, c), both in registers.  No
//            [C][source] tensor exists anywhere.  Neighbouring source voxels read the same or neighbouring corners (the scan is
//            usually the finer grid), so the 8 C loads per voxel are cache hits after the first; the pass is bound by the
//            8 C exponentials and 16 C divisions per voxel inside the box.
//   tallies    : LDS integer atomics per voxel into 3 C words per workgroup, then one 64-bit global integer atomic per non-zero
//            word and workgroup: exact and independent of the order of arrival.
// A table entry is divided by its prepared stride and clamped into the prepared extent before any address is formed: no table
// can make the kernel read outside the sum volume.
// -ffp-contract=off (csrc/Makefile) and the pragma below keep b - a rounded on its own before the explicit fmaf of a lerp.
#include "common.hpp"
#include "../../include/dua_hip.h"

#pragma clang fp contract(off)

namespace dua {

constexpr int LM_THREADS = 256;
constexpr int LM_VEC = 4;                                 // source voxels per thread and step
constexpr int LM_MAX_BLOCKS = 8192;

struct LabelmapArgs {
  const float* sum;                                       // [C][Dp][Hp][Wp]
  const int* cnt[3];                                      // nd, nh, nw (count form)
  const float* wsum;                                      // [Dp][Hp][Wp] (weighted form)
  const int* lo[3];                                       // per SOURCE axis
  const float* wt[3];
  long plane;                                             // Dp Hp Wp
  int C;
  int pstride[3];                                         // element strides of the padded volume: Hp Wp, Wp, 1
  int off[3];                                             // crop offsets od, oh, ow
  int n[3];                                               // prepared extents D, H, W
  int tstride[3];                                         // strides the table entries are multiplied by: H W, W, 1
  int X[3];                                               // source extents
  int axis[3];                                            // prepared axis of source axis 0, 1, 2
  float min_prob;
};

__device__ __forceinline__ float lm_lerp(float a, float b, float w) { return __builtin_fmaf(w, b - a, a); }

// prepared axis j takes the value of the source axis that maps to it (a0, a1: the prepared axes of source axes 0 and 1)
template <typename T>
__device__ __forceinline__ T lm_pick(int j, int a0, int a1, T v0, T v1, T v2) { return a0 == j ? v0 : (a1 == j ? v1 : v2); }

// one table entry of source axis p: lower / upper coordinate along prepared axis axis[p], inside [0, n - 1] whatever it holds
struct LmAxis { int lo, hi; float w; bool inside; };
__device__ __forceinline__ LmAxis lm_axis(const LabelmapArgs& a, int p, int x) {
  const int e = a.lo[p][x], j = a.axis[p];
  LmAxis r;
  r.inside = e >= 0;
  r.lo = min((int)((unsigned)max(e, 0) / (unsigned)a.tstride[j]), a.n[j] - 1);
  r.hi = min(r.lo + 1, a.n[j] - 1);
  r.w = a.wt[p][x];
  return r;
}

template <bool WEIGHTED, bool TALLY>
__global__ void __launch_bounds__(LM_THREADS) labelmap_kernel(LabelmapArgs a, bool wide, unsigned char* __restrict__ out,
                                                              const unsigned char* __restrict__ ref,
                                                              unsigned long long* __restrict__ tallies) {
  __shared__ unsigned part[3 * DUA_BLEND_MAX_CLASSES];
  const int tid = threadIdx.x;
  if constexpr (TALLY) {
    for (int k = tid; k < 3 * a.C; k += LM_THREADS) part[k] = 0;
    __syncthreads();
  }
  const int X1 = a.X[1], X2 = a.X[2], a0 = a.axis[0], a1 = a.axis[1];
  const unsigned G = (unsigned)(X2 + LM_VEC - 1) / LM_VEC;
  const unsigned groups = (unsigned)a.X[0] * (unsigned)X1 * G;              // below 2^31
  for (unsigned t = blockIdx.x * (unsigned)LM_THREADS + tid; t < groups; t += gridDim.x * (unsigned)LM_THREADS) {
    const unsigned row = t / G;
    const int x2 = (int)(t - row * G) * LM_VEC;
    const int x0 = (int)(row / (unsigned)X1), x1 = (int)(row - (unsigned)x0 * (unsigned)X1);
    const int n = min(LM_VEC, X2 - x2);
    const long o = (long)row * X2 + x2;
    const LmAxis s0 = lm_axis(a, 0, x0), s1 = lm_axis(a, 1, x1);
    unsigned packed = 0, refw = 0;
    if constexpr (TALLY) {
      if (wide) refw = *reinterpret_cast<const unsigned*>(ref + o);
    }
#pragma unroll
    for (int e = 0; e < LM_VEC; ++e) {
      if (e >= n) break;
      const LmAxis s2 = lm_axis(a, 2, x2 + e);
      int label = 0;
      if (s0.inside && s1.inside && s2.inside) {
        int off[3][2];                                    // per PREPARED axis: element offset of the lower / upper coordinate
        float w[3];
        int cnt[3][2];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          const int l = lm_pick(j, a0, a1, s0.lo, s1.lo, s2.lo) + a.off[j], h = lm_pick(j, a0, a1, s0.hi, s1.hi, s2.hi) + a.off[j];
          off[j][0] = l * a.pstride[j];
          off[j][1] = h * a.pstride[j];
          w[j] = lm_pick(j, a0, a1, s0.w, s1.w, s2.w);
          if constexpr (!WEIGHTED) { cnt[j][0] = a.cnt[j][l]; cnt[j][1] = a.cnt[j][h]; }
        }
        int corner[2][2][2];
        float den[2][2][2];
#pragma unroll
        for (int bz = 0; bz < 2; ++bz)
#pragma unroll
          for (int by = 0; by < 2; ++by)
#pragma unroll
            for (int bx = 0; bx < 2; ++bx) {
              corner[bz][by][bx] = off[0][bz] + off[1][by] + off[2][bx];
              if constexpr (WEIGHTED) den[bz][by][bx] = a.wsum[corner[bz][by][bx]];
              else den[bz][by][bx] = (float)(cnt[0][bz] * cnt[1][by] * cnt[2][bx]);
            }
        float best = -1.f;                                // below every probability: channel 0 wins unless it is NaN
        const float* sc = a.sum;
        for (int c = 0; c < a.C; ++c) {
          float s[2];
#pragma unroll
          for (int bz = 0; bz < 2; ++bz) {
            float r[2];
#pragma unroll
            for (int by = 0; by < 2; ++by) {
              float p[2];
#pragma unroll
              for (int bx = 0; bx < 2; ++bx) {
                const float q = sc[corner[bz][by][bx]] / den[bz][by][bx];
                p[bx] = 1.f / (1.f + __expf(-q));
              }
              r[by] = lm_lerp(p[0], p[1], w[2]);          // prepared axis 2 first
            }
            s[bz] = lm_lerp(r[0], r[1], w[1]);            // then axis 1
          }
          const float v = lm_lerp(s[0], s[1], w[0]);      // then axis 0
          if (v > best) { best = v; label = c; }          // strict: the lowest channel keeps a tie; NaN > x is false
          sc += a.plane;
        }
        if (best < a.min_prob) label = 0;
      }
      packed |= (unsigned)label << (8 * e);
      if constexpr (TALLY) {
        const unsigned r = wide ? (refw >> (8 * e)) & 255u : ref[o + e];
        atomicAdd(&part[3 * label + 1], 1u);
        if (r < (unsigned)a.C) {
          atomicAdd(&part[3 * r + 2], 1u);
          if (r == (unsigned)label) atomicAdd(&part[3 * r], 1u);
        }
      }
    }
    if (wide) {
      *reinterpret_cast<unsigned*>(out + o) = packed;
    } else {
#pragma unroll
      for (int e = 0; e < LM_VEC; ++e)
        if (e < n) out[o + e] = (unsigned char)(packed >> (8 * e));
    }
  }
  if constexpr (TALLY) {
    __syncthreads();
    for (int k = tid; k < 3 * a.C; k += LM_THREADS) {
      const unsigned v = part[k];
      if (v) atomicAdd(&tallies[k], (unsigned long long)v);
    }
  }
}

static bool lm_extents_ok(long a, long b, long c) {       // three positive extents whose product is below 2^31
  return a >= 1 && b >= 1 && c >= 1 && a < (1L << 31) && b < (1L << 31) && c < (1L << 31) && a * b < (1L << 31) &&
         a * b * c < (1L << 31);
}

}  // namespace dua

extern "C" int dua_blend_finish_labelmap(const float* sum, int C, int Dp, int Hp, int Wp, const int* nd, const int* nh,
                                         const int* nw, const float* wsum, int od, int oh, int ow, int D, int H, int W, int X0,
                                         int X1, int X2, const int* lo0, const int* lo1, const int* lo2, const float* w0,
                                         const float* w1, const float* w2, int axis0, int axis1, int axis2, float min_prob,
                                         unsigned char* label_out, const unsigned char* reference, unsigned long long* tallies,
                                         void* stream) {
  if (!sum || !label_out || !lo0 || !lo1 || !lo2 || !w0 || !w1 || !w2) return DUA_ERR_ARG;
  const bool counts = nd && nh && nw;
  if (counts == (wsum != nullptr) || (!counts && (nd || nh || nw))) return DUA_ERR_ARG;       // exactly one divisor form
  if ((reference != nullptr) != (tallies != nullptr)) return DUA_ERR_ARG;
  if (C < 1 || C > DUA_BLEND_MAX_CLASSES || C > 255) return DUA_ERR_ARG;
  if (!dua::lm_extents_ok(Dp, Hp, Wp) || !dua::lm_extents_ok(D, H, W) || !dua::lm_extents_ok(X0, X1, X2)) return DUA_ERR_ARG;
  if (od < 0 || oh < 0 || ow < 0 || od > Dp - D || oh > Hp - H || ow > Wp - W) return DUA_ERR_ARG;
  if (axis0 < 0 || axis1 < 0 || axis2 < 0 || (1 << axis0 | 1 << axis1 | 1 << axis2) != 7) return DUA_ERR_ARG;   // a permutation
  if (!(min_prob >= 0.f && min_prob <= 1.f)) return DUA_ERR_ARG;                              // NaN fails both
  if ((((size_t)sum | (size_t)wsum | (size_t)nd | (size_t)nh | (size_t)nw | (size_t)lo0 | (size_t)lo1 | (size_t)lo2 | (size_t)w0 |
        (size_t)w1 | (size_t)w2) & 3) || ((size_t)tallies & 7))
    return DUA_ERR_ARG;
  dua::LabelmapArgs a;
  a.sum = sum; a.wsum = wsum; a.C = C; a.min_prob = min_prob;
  a.plane = (long)Dp * Hp * Wp;
  a.cnt[0] = nd; a.cnt[1] = nh; a.cnt[2] = nw;
  a.lo[0] = lo0; a.lo[1] = lo1; a.lo[2] = lo2;
  a.wt[0] = w0; a.wt[1] = w1; a.wt[2] = w2;
  a.pstride[0] = Hp * Wp; a.pstride[1] = Wp; a.pstride[2] = 1;
  a.off[0] = od; a.off[1] = oh; a.off[2] = ow;
  a.n[0] = D; a.n[1] = H; a.n[2] = W;
  a.tstride[0] = H * W; a.tstride[1] = W; a.tstride[2] = 1;
  a.X[0] = X0; a.X[1] = X1; a.X[2] = X2;
  a.axis[0] = axis0; a.axis[1] = axis1; a.axis[2] = axis2;
  hipStream_t s = (hipStream_t)stream;
  if (tallies) {
    const hipError_t e = hipMemsetAsync(tallies, 0, sizeof(unsigned long long) * 3 * C, s);
    if (e != hipSuccess) return (int)e;
  }
  const long groups = (long)X0 * X1 * ((X2 + dua::LM_VEC - 1) / dua::LM_VEC);
  long blocks = (groups + dua::LM_THREADS - 1) / dua::LM_THREADS;
  if (blocks > dua::LM_MAX_BLOCKS) blocks = dua::LM_MAX_BLOCKS;
  const bool wide = X2 % dua::LM_VEC == 0 && ((size_t)label_out & 3) == 0 && ((size_t)reference & 3) == 0;
#define DUA_LABELMAP(WEIGHTED, TALLY)                                                                                       \
  hipLaunchKernelGGL((dua::labelmap_kernel<WEIGHTED, TALLY>), dim3((unsigned)blocks), dim3(dua::LM_THREADS), 0, s, a, wide, \
                     label_out, reference, tallies)
  if (wsum) { if (tallies) DUA_LABELMAP(true, true); else DUA_LABELMAP(true, false); }
  else { if (tallies) DUA_LABELMAP(false, true); else DUA_LABELMAP(false, false); }
#undef DUA_LABELMAP
  return (int)hipGetLastError();
}
