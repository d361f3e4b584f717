// The "multi_neighbor" term of the training loss: losses/loss.py:234-301 (MultiNeighborLoss, reduction "mean"), combined
// with the other terms by Loss.__call__ (:64-86, csrc/train_glue.hip's loss tail).  For each sample i the reference takes
// x = labels[i] and x = sigmoid(preds[i]), both [C, D, H, W], and
//   t = argmax(x, dim=1)                     -- over DEPTH, not over classes (a quirk of the reference, reproduced as it is):
//                                               t is [C, H, W] and holds depth indices; ties and NaN as torch.argmax (the
//                                               first maximum wins, NaN counts as the maximum)
//   centroid_k = fp32 mean of the (c, h, w) index triples with t == k, k < K (num_classes); k is valid when it occurs in
//                the LABEL map; a valid class absent from the prediction keeps the centroid (0, 0, 0)
//   the Kv valid centroids in class order: Kv < 2 -> one entry 0; else n[a][b] = (c_a - c_b) / (|c_a - c_b|' + 1e-6)
//                (|.|' = the norm with 0 replaced by 1), angle[a][b][e] = acos(clamp(n[a][b] . n[a][e], -1+1e-6, 1-1e-6))
//                for b < e: Kv * Kv (Kv - 1) / 2 entries
//   loss = mean over the entries of ALL samples together of (angle_pred - angle_label)^2, fp32 throughout.
// argmax cuts the graph: the term has no gradient.  It changes the loss value and, under "mean" / "log", the combine's
// derivative (dcomb) only.
//
//   columns: one thread per (n, 8 channels, h, w) and quarter of D; both argmaxes of each of its columns, combined across the
//            quarters in LDS; (sum c, sum h, sum w, count) per (n, side, class) in integers: LDS atomics per block, then one
//            64-bit global atomic per block and non-zero field (deterministic: integer adds only)
//   angles : one block per (row a, sample n): centroids, the normalised rows n[a][*] of both sides, sum over b < e of the
//            squared angle difference in double, written (not accumulated) to partials[n][a]; row 0 also writes the
//            sample's entry count to partials[n][K]
#include "common.hpp"
#include "../../include/dua_hip.h"

namespace dua {

constexpr int MN_MAXK = 64;      // = LOSS_MAXC of seg_loss.hip
constexpr int MN_ITEMS = 64;     // column groups (8 channels at one (h, w)) per block
constexpr int MN_SLICES = 4;     // depth quarters per column group: 256 threads

// torch.argmax's order: v replaces the running maximum when larger, or when v is NaN and the maximum is not
__device__ __forceinline__ bool mn_takes(float v, float best) { return v > best || (v != v && best == best); }

// sigmoid as torch computes it in fp32: the accurate expf (not __expf), so that saturation to 1.0 -- and the ties it
// makes -- falls on the same logits
__device__ __forceinline__ float mn_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

template <typename T, bool VEC>
__device__ __forceinline__ void mn_load8(const T* __restrict__ row, int nch, float out[8]) {
  if constexpr (VEC && sizeof(T) == 2) {
    const f16x8 v = *(const f16x8*)row;
#pragma unroll
    for (int e = 0; e < 8; ++e) out[e] = (float)v[e];
  } else if constexpr (VEC) {
    const f32x4 a = *(const f32x4*)row, b = *(const f32x4*)(row + 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) { out[e] = a[e]; out[4 + e] = b[e]; }
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e) out[e] = e < nch ? (float)row[e] : 0.f;
  }
}

// p: channels-last [N][D][H][W][p_stride] (first C channels), y: NCDHW fp32 [N][C][D][H][W];
// csums: [N][2][K][4] u64 (side 0 = labels, 1 = prediction; sum c, sum h, sum w, count), pre-zeroed.
// VEC: p_stride % 8 == 0 and p 16-byte aligned (a group's 8 channels lie inside the row even where c0 + 8 > C).
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void multi_neighbor_columns_kernel(const T* __restrict__ p, int p_stride,
                                                                     const float* __restrict__ y, int C, int K, int D, int H,
                                                                     int W, unsigned long long* __restrict__ csums) {
  __shared__ float bv[MN_SLICES][2][8][MN_ITEMS];
  __shared__ int bi[MN_SLICES][2][8][MN_ITEMS];
  __shared__ unsigned hist[2][MN_MAXK][4];
  const int n = blockIdx.y, item = threadIdx.x % MN_ITEMS, slice = threadIdx.x / MN_ITEMS;
  const int G = (C + 7) / 8;
  const long HW = (long)H * W;
  const long it = (long)blockIdx.x * MN_ITEMS + item;          // (hw, g), g fastest: a wave reads whole logits rows
  const bool live = it < HW * G;
  const int g = live ? (int)(it % G) : 0;
  const long hw = live ? it / G : 0;
  const int c0 = 8 * g, nch = min(8, C - c0);
  for (int i = threadIdx.x; i < 2 * MN_MAXK * 4; i += 256) (&hist[0][0][0])[i] = 0u;

  const int chunk = (D + MN_SLICES - 1) / MN_SLICES;
  const int d0 = slice * chunk, d1 = min(D, d0 + chunk);
  float lv[8], pv[8];
  int li[8], pi[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) { lv[e] = 0.f; pv[e] = 0.f; li[e] = -1; pi[e] = -1; }
  if (live) {
    const float* yc = y + ((long)n * C + c0) * D * HW + hw;                 // labels: coalesced over w
    const T* pc = p + (long)n * D * HW * p_stride + hw * p_stride + c0;     // logits: one run of 8 channels per voxel
#pragma unroll 2
    for (int d = d0; d < d1; ++d) {
      float xl[8], xp[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) xl[e] = e < nch ? yc[((long)e * D + d) * HW] : 0.f;
      mn_load8<T, VEC>(pc + (long)d * HW * p_stride, nch, xp);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float s = mn_sigmoid(xp[e]);
        if (li[e] < 0 || mn_takes(xl[e], lv[e])) { lv[e] = xl[e]; li[e] = d; }
        if (pi[e] < 0 || mn_takes(s, pv[e])) { pv[e] = s; pi[e] = d; }
      }
    }
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    bv[slice][0][e][item] = lv[e]; bi[slice][0][e][item] = li[e];
    bv[slice][1][e][item] = pv[e]; bi[slice][1][e][item] = pi[e];
  }
  __syncthreads();
  // the quarters in depth order (each holds its first maximum): thread (slice s, item) finishes channels 2s, 2s+1 of its item
  if (live) {
    const int h = (int)(hw / W), w = (int)(hw % W);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int e = 2 * slice + j;
      if (e >= nch) continue;
#pragma unroll
      for (int side = 0; side < 2; ++side) {
        float best = 0.f;
        int k = -1;
        for (int s = 0; s < MN_SLICES; ++s) {
          const int i = bi[s][side][e][item];
          if (i >= 0 && (k < 0 || mn_takes(bv[s][side][e][item], best))) { best = bv[s][side][e][item]; k = i; }
        }
        if (k < K) {
          atomicAdd(&hist[side][k][0], (unsigned)(c0 + e));
          atomicAdd(&hist[side][k][1], (unsigned)h);
          atomicAdd(&hist[side][k][2], (unsigned)w);
          atomicAdd(&hist[side][k][3], 1u);
        }
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 2 * K * 4; i += 256) {
    const int side = i / (4 * K), k = (i / 4) % K, f = i % 4;
    const unsigned v = hist[side][k][f];
    if (v) atomicAdd(csums + (((long)n * 2 + side) * K + k) * 4 + f, (unsigned long long)v);
  }
}

__global__ __launch_bounds__(256) void multi_neighbor_angles_kernel(int K, const unsigned long long* __restrict__ csums,
                                                                    double* __restrict__ partials) {
  __shared__ float cen[2][MN_MAXK][3];   // the valid centroids in class order (labels, prediction)
  __shared__ float nv[2][MN_MAXK][3];    // n[a][b] of this block's row a
  __shared__ double red[4];
  __shared__ int kv_s;
  const int a = blockIdx.x, n = blockIdx.y;
  const unsigned long long* q = csums + (long)n * 2 * K * 4;
  if (threadIdx.x == 0) {
    int kv = 0;
    for (int k = 0; k < K; ++k) {
      if (q[k * 4 + 3] == 0) continue;
      for (int side = 0; side < 2; ++side) {
        const unsigned long long* r = q + (side * K + k) * 4;
        const float cnt = (float)r[3];
        for (int j = 0; j < 3; ++j) cen[side][kv][j] = r[3] ? (float)r[j] / cnt : 0.f;
      }
      ++kv;
    }
    kv_s = kv;
  }
  __syncthreads();
  const int kv = kv_s;
  double* out = partials + (long)n * (K + 1);
  if (a == 0 && threadIdx.x == 0) out[K] = kv < 2 ? 1.0 : 0.5 * (double)kv * (double)kv * (double)(kv - 1);
  if (kv < 2 || a >= kv) {
    if (threadIdx.x == 0) out[a] = 0.0;
    return;
  }
  for (int i = threadIdx.x; i < 2 * kv; i += 256) {
    const int side = i / kv, b = i % kv;
    const float dx = cen[side][a][0] - cen[side][b][0], dy = cen[side][a][1] - cen[side][b][1],
                dz = cen[side][a][2] - cen[side][b][2];
    float nrm = sqrtf(dx * dx + dy * dy + dz * dz);
    nrm = nrm > 0.f ? nrm : 1.f;
    const float den = nrm + 1e-6f;
    nv[side][b][0] = dx / den; nv[side][b][1] = dy / den; nv[side][b][2] = dz / den;
  }
  __syncthreads();
  double acc = 0.0;
  for (int i = threadIdx.x; i < kv * kv; i += 256) {
    const int b = i / kv, e = i % kv;
    if (b >= e) continue;
    float ang[2];
#pragma unroll
    for (int side = 0; side < 2; ++side) {
      float dot = nv[side][b][0] * nv[side][e][0] + nv[side][b][1] * nv[side][e][1] + nv[side][b][2] * nv[side][e][2];
      dot = fminf(fmaxf(dot, -1.f + 1e-6f), 1.f - 1e-6f);
      ang[side] = acosf(dot);
    }
    const float dlt = ang[1] - ang[0];
    acc += (double)(dlt * dlt);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) out[a] = ((red[0] + red[1]) + red[2]) + red[3];
}

}  // namespace dua

extern "C" {

int dua_multi_neighbor_columns(int dtype, int N, int C, int K, int D, int H, int W, const void* logits, int logits_stride,
                               const float* labels, unsigned long long* csums, void* stream) {
  if (!logits || !labels || !csums || N <= 0 || N > 65535 || C <= 0 || K <= 0 || K > dua::MN_MAXK || D <= 0 || H <= 0 ||
      W <= 0 || logits_stride < C)
    return DUA_ERR_ARG;
  const long items = (long)H * W * ((C + 7) / 8);
  const long blocks = (items + dua::MN_ITEMS - 1) / dua::MN_ITEMS;
  if (blocks > 0x7fffffffL) return DUA_ERR_ARG;
  const dim3 grid((unsigned)blocks, N);
  const bool aligned = ((size_t)logits & 15) == 0 && logits_stride % 8 == 0;
  hipStream_t s = (hipStream_t)stream;
#define MN_LAUNCH(T, V)                                                                                             \
  hipLaunchKernelGGL((dua::multi_neighbor_columns_kernel<T, V>), grid, dim3(256), 0, s, (const T*)logits, logits_stride, \
                     labels, C, K, D, H, W, csums)
  if (dtype == DUA_F16) {
    if (aligned) MN_LAUNCH(dua::f16, true); else MN_LAUNCH(dua::f16, false);
  } else if (dtype == DUA_F32) {
    if (aligned) MN_LAUNCH(float, true); else MN_LAUNCH(float, false);
  } else {
    return DUA_ERR_ARG;
  }
#undef MN_LAUNCH
  return (int)hipGetLastError();
}

int dua_multi_neighbor_angles(int N, int K, const unsigned long long* csums, double* partials, void* stream) {
  if (!csums || !partials || N <= 0 || N > 65535 || K <= 0 || K > dua::MN_MAXK) return DUA_ERR_ARG;
  hipLaunchKernelGGL(dua::multi_neighbor_angles_kernel, dim3(K, N), dim3(256), 0, (hipStream_t)stream, K, csums, partials);
  return (int)hipGetLastError();
}

}  // extern "C"
