// The pieces of the union-find of components.hip that fill_holes.hip runs as well, in one definition: the constants, the
// lock-free find / union, the run start the inits write, the host checks of extents and dtypes, and the two launches (merge,
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

inline long cc_align256(long x) { return (x + 255) & ~255L; }

inline bool cc_extents_ok(int V, int D, int H, int W) {
  if (V < 1 || V > 65535 || D < 1 || H < 1 || W < 1) return false;
  return (long)D * H <= 0x7fffffffL / W && (long)D * H * W < 0x7fffffffL;       // linear indices are int32
}

inline bool cc_mask_dtype_ok(int t) { return t == DUA_F32 || t == DUA_U8; }

// Defined in components.hip.  parent: int32 [V][pvs], as an init left it (>= 0 inside the set, CC_BG outside).
//   merge   : the unions of every voxel of the set with the backward half of its neighbourhood (cc_merge_kernel<false>);
//   flatten : parent[p] = find(p), and blocksum[v][block] = the roots in each block of CC_SCAN_BLOCK voxels (nb per volume).
void cc_launch_merge(hipStream_t s, int V, int D, int H, int W, int connectivity, int* parent, long pvs);
void cc_launch_flatten(hipStream_t s, int V, long vox, int* parent, long pvs, int* blocksum, long nb);

}  // namespace dua
