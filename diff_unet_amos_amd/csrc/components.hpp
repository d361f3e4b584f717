// The pieces of the union-find of components.hip that fill_holes.hip runs as well, in one definition: the constants, the
// lock-free find / union, the run start the inits write, the Dice tallies of the filter and fill passes (map form and one-hot
// form), the host checks of extents, dtypes and the reference, the head of the workspace layout, and the two launches (merge,
// flatten) that only need "parent >= 0 = a voxel of the set that is being joined" -- whichever set that is.
#pragma once
#include "common.hpp"

namespace dua {

constexpr int CC_THREADS = 256;
constexpr int CC_PER_THREAD = 4;
constexpr int CC_SCAN_BLOCK = CC_THREADS * CC_PER_THREAD;      // voxels per block of the numbering scan (and of sizes / filter)
constexpr int CC_WAVES = CC_THREADS / 64;
constexpr int CC_BG = -1;                                      // parent of a voxel outside the set that is being joined
enum : int { CC_REF_NONE = 0, CC_REF_ONEHOT_F32, CC_REF_ONEHOT_U8, CC_REF_MAP };

__device__ __forceinline__ bool cc_fg(const void* m, int is_f32, size_t i) {
  return is_f32 ? reinterpret_cast<const float*>(m)[i] != 0.f : reinterpret_cast<const unsigned char*>(m)[i] != 0;
}

__device__ __forceinline__ int cc_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ int cc_wave_sum(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// THE INVARIANT of every loop below: parent[i] <= i for every foreground voxel, at all times, and a slot only ever decreases
// (init writes the start of the voxel's run, merge writes with atomicMin a root smaller than the slot's index, flatten writes
// the root).  So the chain i, parent[i], parent[parent[i]], ... strictly decreases until it meets a slot with parent[i] == i:
// find terminates, whatever other threads store meanwhile (a value read late is an older, larger ancestor of the same set).
__device__ __forceinline__ int cc_find(const int* parent, int i) {
  int p = cc_load(parent + i);
  while (p != i) {                    // p < i
    i = p;
    p = cc_load(parent + i);
  }
  return i;
}

// Lock-free union.  hi > lo are the two roots found; atomicMin writes lo into hi's slot and returns what the slot held.
//   old == hi : the slot was still a root when written -- hi's set now hangs below lo, done.
//   old <  hi : another thread had linked hi below old first.  The slot now holds min(old, lo), so hi stays attached to one of
//               them and the link that remains to be made is old ~ lo: repeat with their roots.
// Both new roots are < hi (find(old) <= old < hi, find(lo) <= lo < hi), so max(a, b) strictly decreases from one iteration to
// the next and the loop ends, at the latest with both roots equal.
__device__ __forceinline__ void cc_union(int* parent, int a, int b) {
  a = cc_find(parent, a);
  b = cc_find(parent, b);
  while (a != b) {
    const int hi = a > b ? a : b, lo = a > b ? b : a;
    const int old = __hip_atomic_fetch_min(parent + hi, lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (old == hi) break;
    a = cc_find(parent, old);
    b = cc_find(parent, lo);
  }
}

// the parent the init writes: the first voxel of the lane's run inside its wave (`starts` has a bit per run start), CC_BG for
// background
__device__ __forceinline__ int cc_run_parent(bool fg, unsigned long long starts, int lane, long p) {
  if (!fg) return CC_BG;
  const unsigned long long below = starts & (~0ull >> (63 - lane));         // bits 0 .. lane: never empty for a foreground lane
  return (int)p - (lane - (63 - __clzll((long long)below)));
}

// ---- the Dice tallies of the filter and fill passes: (|A & B|, |A|, |B|) per class, A = the pass's output, B = the reference ----

// The map form (cc_filter_map_kernel<true>, fh_fill_map_kernel<true>): A and B are label maps.  Class 0, the bulk of a scan, is
// counted in registers; the other classes in the LDS words part[3 * class + counter]; a value >= C counts nowhere.  The kernel
// declares the LDS (part: 3 * DUA_BLEND_MAX_CLASSES words, red: one row per wave) and places the two barriers: one between
// zero() and the first add(), one between reduce() and flush().
struct CcMapTally {
  unsigned* part;
  int (*red)[3];
  int z[3] = {0, 0, 0};

  __device__ __forceinline__ void zero(int C) {
    for (int i = threadIdx.x; i < 3 * C; i += CC_THREADS) part[i] = 0;
  }
  __device__ __forceinline__ void add(int o, int r, int C) {
    if (o == 0) ++z[1];
    else if (o < C) atomicAdd(&part[3 * o + 1], 1u);
    if (r == 0) {
      ++z[2];
      z[0] += o == 0;
    } else if (r < C) {
      atomicAdd(&part[3 * r + 2], 1u);
      if (r == o) atomicAdd(&part[3 * r], 1u);
    }
  }
  __device__ __forceinline__ void reduce() {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const int t = cc_wave_sum(z[i]);
      if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][i] = t;
    }
  }
  // one 64-bit integer atomic per non-zero word
  __device__ __forceinline__ void flush(int C, unsigned long long* tallies) {
    for (int i = threadIdx.x; i < 3 * C; i += CC_THREADS) {
      unsigned long long t = part[i];
      if (i < 3)
        for (int k = 0; k < CC_WAVES; ++k) t += (unsigned long long)red[k][i];
      if (t) atomicAdd(&tallies[i], t);
    }
  }
};

// The one-hot form (cc_filter_kernel, fh_fill_mask_kernel): volume v = b * C + c is class c of sample b.  The reference voxel p
// of that volume, for the three kinds of reference:
__device__ __forceinline__ bool cc_ref_fg(const void* ref, int kind, int v, int b, int c, int vox, long p) {
  if (kind == CC_REF_MAP) return reinterpret_cast<const unsigned char*>(ref)[(size_t)b * (size_t)vox + (size_t)p] == c;
  return cc_fg(ref, kind == CC_REF_ONEHOT_F32, (size_t)v * (size_t)vox + (size_t)p);
}

__device__ __forceinline__ void cc_onehot_add(int* n, bool a, bool r) {
  n[0] += a && r; n[1] += a; n[2] += r;
}

// The block's total of each of N per-thread counters, returned to thread i < N for counter i: wave sums, one LDS row per wave,
// one barrier.  The counters below `first` (kernel-uniform) are known to be zero in every thread and are not summed.
template <int N>
__device__ __forceinline__ unsigned long long cc_block_totals(int (&n)[N], int (*red)[N], int first) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)                         // cc_wave_sum of the N counters, side by side
#pragma unroll
    for (int i = 0; i < N; ++i)
      if (i >= first) n[i] += __shfl_xor(n[i], off, 64);
  if ((threadIdx.x & 63) == 0)
#pragma unroll
    for (int i = 0; i < N; ++i) red[threadIdx.x >> 6][i] = n[i];
  __syncthreads();
  unsigned long long t = 0;
  if (threadIdx.x < N)
    for (int k = 0; k < CC_WAVES; ++k) t += (unsigned long long)red[k][threadIdx.x];
  return t;
}

// thread i < 3 holds the block's total of counter i: one 64-bit integer atomic per non-zero counter of class c
__device__ __forceinline__ void cc_onehot_flush(unsigned long long t, int c, unsigned long long* tallies) {
  if (threadIdx.x < 3 && t) atomicAdd(&tallies[(size_t)c * 3 + threadIdx.x], t);
}

inline long cc_align256(long x) { return (x + 255) & ~255L; }

inline bool cc_extents_ok(int V, int D, int H, int W) {
  if (V < 1 || V > 65535 || D < 1 || H < 1 || W < 1) return false;
  return (long)D * H <= 0x7fffffffL / W && (long)D * H * W < 0x7fffffffL;       // linear indices are int32
}

inline bool cc_mask_dtype_ok(int t) { return t == DUA_F32 || t == DUA_U8; }

// The reference of a one-hot tallying pass over V volumes (dua_cc_filter, dua_fill_holes_mask) as a CC_REF_* kind; DUA_ERR_ARG
// for a reference without tallies or the reverse, classes that do not divide V, a dtype the kind does not take or a
// misaligned pointer.
inline int cc_reference_kind(const void* reference, int reference_dtype, int label_map, int C, int V,
                             const unsigned long long* tallies, int* kind) {
  *kind = CC_REF_NONE;
  if ((reference != nullptr) != (tallies != nullptr)) return DUA_ERR_ARG;
  if (!reference) return 0;
  if (C < 1 || C > DUA_BLEND_MAX_CLASSES || V % C != 0 || ((size_t)tallies & 7) != 0) return DUA_ERR_ARG;
  if (label_map) {
    if (reference_dtype != DUA_U8) return DUA_ERR_ARG;
    *kind = CC_REF_MAP;
  } else if (reference_dtype == DUA_F32) {
    if (((size_t)reference & 3) != 0) return DUA_ERR_ARG;
    *kind = CC_REF_ONEHOT_F32;
  } else if (reference_dtype == DUA_U8) {
    *kind = CC_REF_ONEHOT_U8;
  } else {
    return DUA_ERR_ARG;
  }
  return 0;
}

// The head of every workspace here: the parents and the block counts of the numbering scan; `end` is where the rest begins.
struct CcPrefix {
  long pvs, nb;                      // parent elements per volume, scan blocks per volume
  long parent, blocksum, end;
};

inline CcPrefix cc_layout_prefix(int V, int D, int H, int W) {
  CcPrefix L;
  const long vox = (long)D * H * W;
  L.pvs = (vox + 63) & ~63L;
  L.nb = (vox + CC_SCAN_BLOCK - 1) / CC_SCAN_BLOCK;
  L.parent = 0;
  L.blocksum = cc_align256(L.parent + (long)V * L.pvs * 4);
  L.end = cc_align256(L.blocksum + (long)V * L.nb * 4);
  return L;
}

// Defined in components.hip.  parent: int32 [V][pvs], as an init left it (>= 0 inside the set, CC_BG outside).
//   merge   : the unions of every voxel of the set with the backward half of its neighbourhood (cc_merge_kernel<false>);
//   flatten : parent[p] = find(p), and blocksum[v][block] = the roots in each block of CC_SCAN_BLOCK voxels (nb per volume).
void cc_launch_merge(hipStream_t s, int V, int D, int H, int W, int connectivity, int* parent, long pvs);
void cc_launch_flatten(hipStream_t s, int V, long vox, int* parent, long pvs, int* blocksum, long nb);

}  // namespace dua
