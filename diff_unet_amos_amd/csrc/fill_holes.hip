// Filling of enclosed holes in V binary volumes [D][H][W] (the mask form) and in V uint8 label maps (the map form), on the
// device.  The contract is written down in include/dua_hip.h ("evaluation: fill holes"): the mask form is
// scipy.ndimage.binary_fill_holes(mask, generate_binary_structure(3, connectivity)) per volume; the map form fills a
// background component that touches no face and is bordered by ONE selectable class with that class.
//
// The union-find is that of components.hip (components.hpp), run on the BACKGROUND: the voxels with mask == 0 / map == 0.
//   init       : parent[p] = the start of p's run of background along W inside its wave, CC_BG for every other voxel.
//   merge      : cc_launch_merge -- the unions with the backward half of the neighbourhood (connectivity 1 / 2 / 3).
//   flatten    : cc_launch_flatten -- parent[p] = the root of p's background component = its smallest linear index.
//   border     : one thread per voxel of the six faces; a background voxel there stores border[root] = 1 (a byte, every writer
//                the same value: no atomic).  The passes below read the flags after this launch has ended.
//   neighbours : (map form) every background voxel of a root WITHOUT a border flag collects the values of its non-zero
//                neighbours as a 64-bit set -- bit c for a selectable class c, bit 0 for a value >= C or a class that is not
//                selected -- and the set is OR-ed into set[root].  Roots with a border flag are skipped: the background around
//                the body, the one component that holds most voxels of a scan, costs no atomic at all.  The other lanes are
//                reduced per wave first: one atomicOr per distinct root per wave, and none when the word holds the bits already.
//   fill       : a background voxel whose root has no border flag becomes 1 (mask form) or the class c when set[root] is the
//                single bit c >= 1 (map form); every other voxel is copied.  The filled counts and, with a reference, the Dice
//                tallies are summed per workgroup and added with 64-bit integer atomics.
// Integer work throughout (atomicMin, atomicOr, integer atomicAdd): every output is exact and equal between runs.  Nothing is
// read back: the chain can be captured into a graph.  LDS is static and small; nothing is registered with dua_prepare.
#include <type_traits>

#include "components.hpp"

namespace dua {

constexpr int FH_MAX_CLASSES = DUA_BLEND_MAX_CLASSES;            // the width of the neighbour set
static_assert(FH_MAX_CLASSES == 64, "one bit of an unsigned long long per class");

// grid (ceil(vox / 256), V).  MAP: src is V uint8 maps, a voxel is seeded when its value is 0.  Otherwise src is V masks (fp32
// or uint8), a voxel is seeded when the mask is 0 there and the volume is selected (select[v] != 0 or no select): a volume
// that is not selected has no seed, so nothing of it is ever filled.  A wave holds 64 consecutive voxels.
template <bool MAP>
__global__ __launch_bounds__(CC_THREADS) void fh_init_kernel(const void* __restrict__ src, int is_f32, long svs,
                                                             const unsigned char* __restrict__ select, int vox, int W,
                                                             int* __restrict__ parent, long pvs) {
  const int v = blockIdx.y;
  const long p = (long)blockIdx.x * CC_THREADS + threadIdx.x;
  bool bg = false;
  if (p < vox) {
    if constexpr (MAP) bg = reinterpret_cast<const unsigned char*>(src)[(size_t)v * svs + (size_t)p] == 0;
    else bg = (!select || select[v] != 0) && !cc_fg(src, is_f32, (size_t)v * svs + (size_t)p);
  }
  const int lane = threadIdx.x & 63;
  const unsigned long long f = __ballot(bg);
  const unsigned long long row0 = __ballot(bg && p % W == 0);
  const unsigned long long starts = f & (~(f << 1) | row0);      // as cc_init_kernel: lane 0, after a non-member, or a new row
  if (p >= vox) return;
  parent[(size_t)v * pvs + (size_t)p] = cc_run_parent(bg, starts, lane, p);
}

// grid (ceil(F / 256), V), F = 2 (H W + D W + D H): thread t is one voxel of one face (an edge voxel is visited by two or three
// threads, which store the same byte).  parent is flattened: parent[p] >= 0 is p's root.
__global__ __launch_bounds__(CC_THREADS) void fh_border_kernel(const int* __restrict__ parent_all, long pvs,
                                                               unsigned char* __restrict__ border_all, int D, int H, int W) {
  const long HW = (long)H * W, DW = (long)D * W, DH = (long)D * H;
  long t = (long)blockIdx.x * CC_THREADS + threadIdx.x;
  long d, h, w;
  if (t < 2 * HW) {
    d = t < HW ? 0 : D - 1;
    t %= HW;
    h = t / W; w = t % W;
  } else if (t < 2 * HW + 2 * DW) {
    t -= 2 * HW;
    h = t < DW ? 0 : H - 1;
    t %= DW;
    d = t / W; w = t % W;
  } else if (t < 2 * HW + 2 * DW + 2 * DH) {
    t -= 2 * HW + 2 * DW;
    w = t < DH ? 0 : W - 1;
    t %= DH;
    d = t / H; h = t % H;
  } else {
    return;
  }
  const long p = (d * H + h) * W + w;                            // < D H W
  const int r = parent_all[(size_t)blockIdx.y * pvs + (size_t)p];
  if (r >= 0) border_all[(size_t)blockIdx.y * pvs + (size_t)r] = 1;
}

__device__ __forceinline__ unsigned long long fh_wave_or(unsigned long long b) {
  unsigned lo = (unsigned)b, hi = (unsigned)(b >> 32);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    lo |= (unsigned)__shfl_xor((int)lo, off, 64);
    hi |= (unsigned)__shfl_xor((int)hi, off, 64);
  }
  return ((unsigned long long)hi << 32) | lo;
}

// grid (ceil(vox / 256), V), one voxel per thread, every lane takes part in the ballots.  class_mask: bit c set = class c may
// fill (1 <= c < C).
__global__ __launch_bounds__(CC_THREADS) void fh_neighbours_kernel(const int* __restrict__ parent_all, long pvs,
                                                                   const unsigned char* __restrict__ border_all,
                                                                   unsigned long long* __restrict__ set_all,
                                                                   const unsigned char* __restrict__ map_all, long mvs, int D,
                                                                   int H, int W, int conn, int C, unsigned long long class_mask) {
  const int* parent = parent_all + (size_t)blockIdx.y * pvs;
  const unsigned char* border = border_all + (size_t)blockIdx.y * pvs;
  unsigned long long* set = set_all + (size_t)blockIdx.y * pvs;
  const unsigned char* map = map_all + (size_t)blockIdx.y * mvs;
  const long vox = (long)D * H * W;
  const long pl = (long)blockIdx.x * CC_THREADS + threadIdx.x;
  int r = -1;
  unsigned long long bits = 0;
  if (pl < vox) {
    const int p = (int)pl;
    const int x = parent[p];
    if (x >= 0 && border[x] == 0) {
      r = x;
      const int HW = H * W;
      const int w = p % W, h = (p / W) % H, d = p / HW;
#pragma unroll
      for (int dz = -1; dz <= 1; ++dz) {
        const int zz = d + dz;
        if (zz < 0 || zz >= D) continue;
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy) {
          const int yy = h + dy;
          if (yy < 0 || yy >= H) continue;
#pragma unroll
          for (int dx = -1; dx <= 1; ++dx) {
            const int nnz = (dz != 0) + (dy != 0) + (dx != 0);
            if (nnz == 0 || nnz > conn) continue;
            const int xx = w + dx;
            if (xx < 0 || xx >= W) continue;
            const int val = map[p + dz * HW + dy * W + dx];
            if (val == 0) continue;                              // a voxel of the component itself (adjacent zeros are joined)
            bits |= (val < C && (class_mask >> val & 1ull)) ? 1ull << val : 1ull;
          }
        }
      }
    }
  }
  const int lane = threadIdx.x & 63;
  const bool valid = bits != 0;
  unsigned long long todo = __ballot(valid);                     // wave-uniform: every lane runs the same iterations
  while (todo) {
    const int leader = __ffsll((long long)todo) - 1;
    const int rr = __shfl(r, leader, 64);
    const bool mine = valid && r == rr;
    const unsigned long long same = __ballot(mine);
    const unsigned long long b = fh_wave_or(mine ? bits : 0ull);
    if (lane == leader) {
      const unsigned long long cur = __hip_atomic_load(set + rr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if ((cur & b) != b) atomicOr(set + rr, b);                 // a word only gains bits: a stale read costs an atomic, no bit
    }
    todo &= ~same;                                               // `same` holds the leader's bit: todo shrinks every time
  }
}

// grid (nb, V): the mask form's fill.  out has the mask's dtype: the mask's value where the voxel is foreground, 1 where it is
// a hole, 0 elsewhere.  filled[v] += the holes' voxels; with a reference, (|A & B|, |A|, |B|) of A = (out != 0) go to
// tallies[c = v % C] as in cc_filter_kernel.
template <bool F32>
__global__ __launch_bounds__(CC_THREADS) void fh_fill_mask_kernel(const int* __restrict__ parent_all, long pvs,
                                                                  const unsigned char* __restrict__ border_all,
                                                                  const void* __restrict__ mask, long mvs, int vox,
                                                                  void* __restrict__ out, unsigned long long* __restrict__ filled,
                                                                  const void* __restrict__ ref, int ref_kind, int C,
                                                                  unsigned long long* __restrict__ tallies) {
  using T = typename std::conditional<F32, float, unsigned char>::type;
  const int v = blockIdx.y;
  const int* parent = parent_all + (size_t)v * pvs;
  const unsigned char* border = border_all + (size_t)v * pvs;
  const T* m = reinterpret_cast<const T*>(mask) + (size_t)v * mvs;
  T* o = reinterpret_cast<T*>(out) + (size_t)v * (size_t)vox;
  const int c = v % C, b = v / C;
  int n[4] = {0, 0, 0, 0};                                       // |A & B|, |A|, |B|, filled
#pragma unroll
  for (int j = 0; j < CC_PER_THREAD; ++j) {
    const long p = (long)blockIdx.x * CC_SCAN_BLOCK + j * CC_THREADS + threadIdx.x;
    if (p >= vox) continue;
    const int x = parent[p];
    T val = m[p];                                                // x >= 0 says val == 0
    if (x >= 0 && border[x] == 0) {
      val = (T)1;
      ++n[3];
    }
    o[p] = val;
    if (ref_kind != CC_REF_NONE) cc_onehot_add(n, val != (T)0, cc_ref_fg(ref, ref_kind, v, b, c, vox, p));
  }
  __shared__ int red[CC_WAVES][4];
  const bool tally = ref_kind != CC_REF_NONE;                    // kernel-uniform; without it the three counts are 0 everywhere
  const unsigned long long t = cc_block_totals<4>(n, red, tally ? 0 : 3);
  if (threadIdx.x == 3 && t) atomicAdd(&filled[v], t);
  if (tally) cc_onehot_flush(t, c, tallies);
}

// grid (nb, V): the map form's fill.  out[v][p] = map[v][p] unless the value is 0, the root of p has no border flag and its
// neighbour set is one bit c >= 1: then c.  filled[c] += the voxels that became c.  TALLY: the tallies of cc_filter_map_kernel,
// for the filled map.
template <bool TALLY>
__global__ __launch_bounds__(CC_THREADS) void fh_fill_map_kernel(const int* __restrict__ parent_all, long pvs,
                                                                 const unsigned char* __restrict__ border_all,
                                                                 const unsigned long long* __restrict__ set_all,
                                                                 const unsigned char* __restrict__ map, long mvs, int vox, int C,
                                                                 unsigned char* __restrict__ out,
                                                                 unsigned long long* __restrict__ filled,
                                                                 const unsigned char* __restrict__ ref,
                                                                 unsigned long long* __restrict__ tallies) {
  __shared__ unsigned fpart[FH_MAX_CLASSES];
  __shared__ unsigned part[TALLY ? 3 * FH_MAX_CLASSES : 1];
  __shared__ int red[TALLY ? CC_WAVES : 1][3];
  const int v = blockIdx.y;
  const int* parent = parent_all + (size_t)v * pvs;
  const unsigned char* border = border_all + (size_t)v * pvs;
  const unsigned long long* set = set_all + (size_t)v * pvs;
  CcMapTally tally{part, red};
  for (int i = threadIdx.x; i < C; i += CC_THREADS) fpart[i] = 0;
  if constexpr (TALLY) tally.zero(C);
  __syncthreads();
#pragma unroll
  for (int j = 0; j < CC_PER_THREAD; ++j) {
    const long p = (long)blockIdx.x * CC_SCAN_BLOCK + j * CC_THREADS + threadIdx.x;
    if (p >= vox) continue;
    int o = map[(size_t)v * mvs + (size_t)p];
    if (o == 0) {
      const int x = parent[p];                                   // >= 0: every zero voxel was seeded
      if (border[x] == 0) {
        const unsigned long long s = set[x];
        if (s > 1ull && (s & (s - 1ull)) == 0ull) {              // one bit, and not bit 0; the bit is below C by construction
          o = __ffsll((long long)s) - 1;
          atomicAdd(&fpart[o], 1u);
        }
      }
    }
    out[(size_t)v * (size_t)vox + (size_t)p] = (unsigned char)o;
    if constexpr (TALLY) tally.add(o, ref[(size_t)v * (size_t)vox + (size_t)p], C);
  }
  if constexpr (TALLY) tally.reduce();
  __syncthreads();
  for (int i = threadIdx.x; i < C; i += CC_THREADS)
    if (fpart[i]) atomicAdd(&filled[i], (unsigned long long)fpart[i]);
  if constexpr (TALLY) tally.flush(C, tallies);
}

// ---- host side ----------------------------------------------------------------------------------------------------------

struct FhScratch : CcPrefix {
  long border, total_mask;
  long set, total_map;               // the map form: one 64-bit neighbour set per voxel index, behind the border flags
};

static FhScratch fh_layout(int V, int D, int H, int W) {
  FhScratch L{cc_layout_prefix(V, D, H, W)};
  L.border = L.end;
  L.total_mask = cc_align256(L.border + (long)V * L.pvs);
  L.set = L.total_mask;
  L.total_map = cc_align256(L.set + (long)V * L.pvs * 8);
  return L;
}

// the launches both forms share, after the init: merge, flatten, border
static void fh_components(hipStream_t s, int V, int D, int H, int W, int connectivity, void* workspace, const FhScratch& L) {
  int* parent = (int*)((unsigned char*)workspace + L.parent);
  int* blocksum = (int*)((unsigned char*)workspace + L.blocksum);
  unsigned char* border = (unsigned char*)workspace + L.border;
  cc_launch_merge(s, V, D, H, W, connectivity, parent, L.pvs);
  cc_launch_flatten(s, V, (long)D * H * W, parent, L.pvs, blocksum, L.nb);
  const long faces = 2 * ((long)H * W + (long)D * W + (long)D * H);
  hipLaunchKernelGGL(fh_border_kernel, dim3((unsigned)((faces + CC_THREADS - 1) / CC_THREADS), V), dim3(CC_THREADS), 0, s, parent,
                     L.pvs, border, D, H, W);
}

}  // namespace dua

extern "C" {

long dua_fill_holes_scratch_bytes(int V, int D, int H, int W, int label_map) {
  if (!dua::cc_extents_ok(V, D, H, W)) return DUA_ERR_ARG;
  const dua::FhScratch L = dua::fh_layout(V, D, H, W);
  return label_map ? L.total_map : L.total_mask;
}

int dua_fill_holes_mask(int V, int D, int H, int W, const void* mask, int mask_dtype, long mask_vstride, int connectivity,
                        const unsigned char* select, void* out, unsigned long long* filled, const void* reference,
                        int reference_dtype, int label_map, int C, unsigned long long* tallies, void* workspace,
                        long workspace_bytes, void* stream) {
  if (!dua::cc_extents_ok(V, D, H, W) || !mask || !out || !filled || !workspace || connectivity < 1 || connectivity > 3 ||
      !dua::cc_mask_dtype_ok(mask_dtype))
    return DUA_ERR_ARG;
  const long vox = (long)D * H * W;
  const bool f32 = mask_dtype == DUA_F32;
  if (mask_vstride < vox || ((size_t)filled & 7) != 0 || (f32 && ((((size_t)mask) | ((size_t)out)) & 3) != 0)) return DUA_ERR_ARG;
  int kind;
  if (dua::cc_reference_kind(reference, reference_dtype, label_map, C, V, tallies, &kind) != 0) return DUA_ERR_ARG;
  const dua::FhScratch L = dua::fh_layout(V, D, H, W);
  if (workspace_bytes < L.total_mask || ((size_t)workspace & 255) != 0) return DUA_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  int* parent = (int*)((unsigned char*)workspace + L.parent);
  unsigned char* border = (unsigned char*)workspace + L.border;
  hipError_t e = hipMemsetAsync(border, 0, (size_t)V * L.pvs, s);
  if (e == hipSuccess) e = hipMemsetAsync(filled, 0, sizeof(unsigned long long) * V, s);
  if (e == hipSuccess && tallies) e = hipMemsetAsync(tallies, 0, sizeof(unsigned long long) * 3 * C, s);
  if (e != hipSuccess) return (int)e;
  const dim3 threads(dua::CC_THREADS);
  const dim3 gvox((unsigned)((vox + dua::CC_THREADS - 1) / dua::CC_THREADS), V), gscan((unsigned)L.nb, V);
  hipLaunchKernelGGL(dua::fh_init_kernel<false>, gvox, threads, 0, s, mask, (int)f32, mask_vstride, select, (int)vox, W, parent,
                     L.pvs);
  dua::fh_components(s, V, D, H, W, connectivity, workspace, L);
  const int Cn = reference ? C : 1;
  if (f32)
    hipLaunchKernelGGL(dua::fh_fill_mask_kernel<true>, gscan, threads, 0, s, parent, L.pvs, border, mask, mask_vstride, (int)vox, out,
                       filled, reference, kind, Cn, tallies);
  else
    hipLaunchKernelGGL(dua::fh_fill_mask_kernel<false>, gscan, threads, 0, s, parent, L.pvs, border, mask, mask_vstride, (int)vox, out,
                       filled, reference, kind, Cn, tallies);
  return (int)hipGetLastError();
}

int dua_fill_holes_map(int V, int D, int H, int W, const unsigned char* map, long map_vstride, int C, int connectivity,
                       unsigned long long class_mask, unsigned char* out, unsigned long long* filled,
                       const unsigned char* reference, unsigned long long* tallies, void* workspace, long workspace_bytes,
                       void* stream) {
  if (!dua::cc_extents_ok(V, D, H, W) || !map || !out || !filled || !workspace || connectivity < 1 || connectivity > 3 || C < 1 ||
      C > DUA_BLEND_MAX_CLASSES)
    return DUA_ERR_ARG;
  const long vox = (long)D * H * W;
  // the classes that may fill are among 1 .. C - 1
  const unsigned long long allowed = (C == 64 ? ~0ull : (1ull << C) - 1ull) & ~1ull;
  if ((class_mask & ~allowed) != 0 || map_vstride < vox || (reference != nullptr) != (tallies != nullptr) ||
      ((size_t)filled & 7) != 0 || ((size_t)tallies & 7) != 0)
    return DUA_ERR_ARG;
  const dua::FhScratch L = dua::fh_layout(V, D, H, W);
  if (workspace_bytes < L.total_map || ((size_t)workspace & 255) != 0) return DUA_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  int* parent = (int*)((unsigned char*)workspace + L.parent);
  unsigned char* border = (unsigned char*)workspace + L.border;
  unsigned long long* set = (unsigned long long*)((unsigned char*)workspace + L.set);
  hipError_t e = hipMemsetAsync(border, 0, (size_t)(L.total_map - L.border), s);         // the flags and the sets behind them
  if (e == hipSuccess) e = hipMemsetAsync(filled, 0, sizeof(unsigned long long) * C, s);
  if (e == hipSuccess && tallies) e = hipMemsetAsync(tallies, 0, sizeof(unsigned long long) * 3 * C, s);
  if (e != hipSuccess) return (int)e;
  const dim3 threads(dua::CC_THREADS);
  const dim3 gvox((unsigned)((vox + dua::CC_THREADS - 1) / dua::CC_THREADS), V), gscan((unsigned)L.nb, V);
  hipLaunchKernelGGL(dua::fh_init_kernel<true>, gvox, threads, 0, s, (const void*)map, 0, map_vstride,
                     (const unsigned char*)nullptr, (int)vox, W, parent, L.pvs);
  dua::fh_components(s, V, D, H, W, connectivity, workspace, L);
  hipLaunchKernelGGL(dua::fh_neighbours_kernel, gvox, threads, 0, s, parent, L.pvs, border, set, map, map_vstride, D, H, W,
                     connectivity, C, class_mask);
  if (tallies)
    hipLaunchKernelGGL(dua::fh_fill_map_kernel<true>, gscan, threads, 0, s, parent, L.pvs, border, set, map, map_vstride, (int)vox, C,
                       out, filled, reference, tallies);
  else
    hipLaunchKernelGGL(dua::fh_fill_map_kernel<false>, gscan, threads, 0, s, parent, L.pvs, border, set, map, map_vstride, (int)vox,
                       C, out, filled, reference, tallies);
  return (int)hipGetLastError();
}

}  // extern "C"
