// Step-Uncertainty Fusion of R DDIM runs of one window, folded into the sampling step (include/dua_hip.h, "Step-Uncertainty
// Fusion"): the runs of group g are batch rows g R .. g R + R - 1 of the step that has just run, so after the tail wrote the
// step's fp32 logits [G R][C][vox] one streaming pass adds the step's weighted predictions into acc [G][C][vox]:
//   m = (l_0 + .. + l_{R-1}) / R;  p = max(sigmoid(m), 0.001);  u = -p log(p);  w = exp(a_k (1 - u));
//   acc += w (clamp(l_0, -1, 1) + .. + clamp(l_{R-1}, -1, 1))
// Within a group a (class, voxel) plane is one contiguous run of P = C vox floats in acc and in every run's logits, so the
// kernel walks j in [0, P): one thread owns an element of acc (a float4 of them on the vector path), reads its R logits in run
// order and writes once.  No atomics, no cross-thread sums: the result does not depend on the grid.  HBM bound: (R + 2) P 4
// bytes per group against ~25 flops and three transcendental calls per element.
// x0^ is the clamp of the same fp32 logit the tail clamps (sampler.hip, sampler_update): bit-equal to the tail's xstart output.
#include "common.hpp"
#include "../../include/dua_hip.h"

namespace dua {

// the step index of this launch: the device word dua_step_begin wrote (clamped into the table, the offence reported), or the
// host's (checked by the launcher)
__device__ __forceinline__ int suf_step(const int* step_word, int step, int nsteps, int* err_word) {
  if (!step_word) return step;
  int k = *step_word;
  if (k < 0 || k >= nsteps) {
    if (err_word && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) *err_word = 1;
    k = k < 0 ? 0 : nsteps - 1;
  }
  return k;
}

// sl = sum of the runs' logits, sx = sum of their clamped values -> the weighted term of this step.
// sigmoid in the form seg_loss.hip uses.  A very negative m makes __expf(-m) overflow to +inf and p = 1 / inf = 0; the max
// then gives 0.001, which is also what the exact sigmoid (below 2^-126 there) is clamped to.  logf / expf are library calls.
__device__ __forceinline__ float suf_term(float sl, float sx, float rcount, float a) {
  const float m = sl / rcount;
  float p = 1.f / (1.f + __expf(-m));
  p = fmaxf(p, 0.001f);
  const float u = -p * logf(p);
  const float w = expf(a * (1.f - u));
  return w * sx;
}

__device__ __forceinline__ float clamp1(float x) { return fminf(fmaxf(x, -1.f), 1.f); }

// grid (x, G): workgroup row g walks the P / 4 float4 of its group
__global__ __launch_bounds__(256) void suf_accumulate_vec4(int R, long P4, const f32x4* __restrict__ logits,
                                                           const float* __restrict__ step_coef, int nsteps,
                                                           const int* __restrict__ step_word, int step, int* err_word,
                                                           f32x4* __restrict__ acc) {
  const float a = step_coef[suf_step(step_word, step, nsteps, err_word)];
  const float rcount = (float)R;
  const long g = blockIdx.y;
  const f32x4* lg = logits + g * R * P4;
  f32x4* ag = acc + g * P4;
  for (long j = blockIdx.x * 256L + threadIdx.x; j < P4; j += (long)gridDim.x * 256) {
    f32x4 l = lg[j];
    f32x4 sl = l, sx;
#pragma unroll
    for (int e = 0; e < 4; ++e) sx[e] = clamp1(l[e]);
    for (int r = 1; r < R; ++r) {
      l = lg[r * P4 + j];
#pragma unroll
      for (int e = 0; e < 4; ++e) { sl[e] += l[e]; sx[e] += clamp1(l[e]); }
    }
    f32x4 o = ag[j];
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = o[e] + suf_term(sl[e], sx[e], rcount, a);
    ag[j] = o;
  }
}

__global__ __launch_bounds__(256) void suf_accumulate_scalar(int R, long P, const float* __restrict__ logits,
                                                             const float* __restrict__ step_coef, int nsteps,
                                                             const int* __restrict__ step_word, int step, int* err_word,
                                                             float* __restrict__ acc) {
  const float a = step_coef[suf_step(step_word, step, nsteps, err_word)];
  const float rcount = (float)R;
  const long g = blockIdx.y;
  const float* lg = logits + g * R * P;
  float* ag = acc + g * P;
  for (long j = blockIdx.x * 256L + threadIdx.x; j < P; j += (long)gridDim.x * 256) {
    float l = lg[j];
    float sl = l, sx = clamp1(l);
    for (int r = 1; r < R; ++r) {
      l = lg[r * P + j];
      sl += l;
      sx += clamp1(l);
    }
    ag[j] = ag[j] + suf_term(sl, sx, rcount, a);
  }
}

}  // namespace dua

extern "C" int dua_suf_accumulate(int G, int R, int C, long voxels, const float* logits, const float* step_coef, int nsteps,
                                  const int* step_word, int step, int* err_word, float* acc, void* stream) {
  if (!logits || !step_coef || !acc || G <= 0 || G > 65535 || R <= 0 || R > DUA_SUF_MAX_RUNS || C <= 0 || voxels <= 0 ||
      nsteps <= 0)
    return DUA_ERR_ARG;
  if (!step_word && (step < 0 || step >= nsteps)) return DUA_ERR_ARG;
  if (voxels > (1L << 40) / C) return DUA_ERR_ARG;          // C voxels R G stays far inside a long
  const long P = (long)C * voxels;
  const bool vec = voxels % 4 == 0 && (((size_t)logits | (size_t)acc) & 15) == 0;
  // memory bound: at most ~2048 workgroups of 256 in all (8 per CU), the rest of a group's plane by grid stride
  const long items = vec ? P / 4 : P;
  long gx = (items + 255) / 256;
  const long cap = 2048 / G > 0 ? 2048 / G : 1;
  if (gx > cap) gx = cap;
  const dim3 grid((unsigned)gx, (unsigned)G);
  if (vec)
    hipLaunchKernelGGL(dua::suf_accumulate_vec4, grid, dim3(256), 0, (hipStream_t)stream, R, P / 4, (const dua::f32x4*)logits,
                       step_coef, nsteps, step_word, step, err_word, (dua::f32x4*)acc);
  else
    hipLaunchKernelGGL(dua::suf_accumulate_scalar, grid, dim3(256), 0, (hipStream_t)stream, R, P, logits, step_coef, nsteps,
                       step_word, step, err_word, acc);
  return (int)hipGetLastError();
}
