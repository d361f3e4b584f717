// Connected-component labelling of V = N * C binary volumes [D][H][W] and the keep-largest / minimum-size filter built on it,
// on the device.  The contract is written down in include/dua_hip.h ("evaluation: connected components"): per volume the
// labels are those of scipy.ndimage.label(mask, generate_binary_structure(3, connectivity)).
//
//   init    : union-find over the voxels of a volume, in global memory.  parent[p] = p for foreground (p = the linear index in
//             the volume, int32), CC_BG for background -- but along W by run: a voxel starts at the first voxel of its x-run
//             inside the 64 lanes of its wave (one ballot, one bit scan), so most unions along x never happen.
//   merge   : every foreground voxel unions itself with the backward half of its neighbourhood (3 / 9 / 13 offsets for
//             connectivity 1 / 2 / 3), so every adjacent pair is visited once.  The -x union is left to the wave's lane 0 (the
//             run init covered the rest), and a union is skipped where the voxel one step down the row proves it redundant.
//   flatten : parent[p] = find(p); a finished component's root is its smallest linear index.  The same pass counts the roots
//             of each block of CC_SCAN_BLOCK voxels.
//   number  : an exclusive prefix sum of the root flags per volume (block counts, one scan of the block counts, apply), so
//             label = 1 + the rank of the root = components numbered by their first voxel in raster order; background 0.
//   sizes   : integer atomic adds into int32 [V][cap], one per distinct label per wave (lanes sharing a label are combined
//             first).  Labels above cap are not tallied.
//   filter  : per volume the k largest labels (ties to the smaller label) and / or those of at least min_size voxels are kept;
//             one pass writes the uint8 mask and, with a reference, the three Dice counts per class.
// Integer work throughout: results are exact and do not depend on the order in which workgroups run.
// The find / union, the run start of the inits, the Dice tallies of the filter passes, the check of the reference, the head of
// the workspace layout and the merge and flatten launches are shared with fill_holes.hip through components.hpp.
#include "components.hpp"

namespace dua {

// grid (ceil(vox / 256), V).  A wave holds 64 consecutive voxels: every lane takes part in the ballots.  A volume with
// select[v] == 0 is all background to everything that follows.
__global__ __launch_bounds__(CC_THREADS) void cc_init_kernel(const void* __restrict__ mask, int is_f32, long mvs,
                                                             const unsigned char* __restrict__ select, int vox, int W,
                                                             int* __restrict__ parent, long pvs) {
  const int v = blockIdx.y;
  const long p = (long)blockIdx.x * CC_THREADS + threadIdx.x;
  const bool on = !select || select[v] != 0;
  const bool fg = on && p < vox && cc_fg(mask, is_f32, (size_t)v * mvs + (size_t)p);
  const int lane = threadIdx.x & 63;
  const unsigned long long f = __ballot(fg);
  const unsigned long long row0 = __ballot(fg && p % W == 0);
  // a run starts at a foreground lane that is lane 0, follows a background lane, or is the first voxel of a row
  const unsigned long long starts = f & (~(f << 1) | row0);
  if (p >= vox) return;
  parent[(size_t)v * pvs + (size_t)p] = cc_run_parent(fg, starts, lane, p);
}

// The label-map form of the init: grid as above, V = N maps.  A voxel is foreground when its value lies in 1 .. C - 1, and a run
// also starts where the value changes: a run holds one value, so the unions the init stands for are all between equal values.
__global__ __launch_bounds__(CC_THREADS) void cc_init_map_kernel(const unsigned char* __restrict__ map, long mvs, int C, int vox,
                                                                 int W, int* __restrict__ parent, long pvs) {
  const int v = blockIdx.y;
  const long p = (long)blockIdx.x * CC_THREADS + threadIdx.x;
  const int val = p < vox ? map[(size_t)v * mvs + (size_t)p] : 0;
  const bool fg = val >= 1 && val < C;
  const int lane = threadIdx.x & 63;
  const int prev = __shfl_up(val, 1, 64);                        // every lane takes part; lane 0 starts a run anyway
  const unsigned long long f = __ballot(fg);
  const unsigned long long row0 = __ballot(fg && p % W == 0);
  const unsigned long long change = __ballot(fg && lane > 0 && prev != val);
  const unsigned long long starts = f & (~(f << 1) | row0 | change);
  if (p >= vox) return;
  parent[(size_t)v * pvs + (size_t)p] = cc_run_parent(fg, starts, lane, p);
}

// grid (ceil(vox / 256), V), one voxel per thread.  MAP (the label-map form): two voxels are joined only when they carry the same
// value, so "q is foreground" reads "q carries p's value" everywhere below; the redundancy arguments hold word for word with
// that reading, because every voxel they name then carries p's value.
template <bool MAP>
__global__ __launch_bounds__(CC_THREADS) void cc_merge_kernel(int* __restrict__ parent_all, long pvs, int D, int H, int W,
                                                              int conn, const unsigned char* __restrict__ map_all, long mvs) {
  int* parent = parent_all + (size_t)blockIdx.y * pvs;
  const long vox = (long)D * H * W;
  const long pl = (long)blockIdx.x * CC_THREADS + threadIdx.x;
  if (pl >= vox) return;
  const int p = (int)pl;
  if (parent[p] < 0) return;                                    // the sign of a slot never changes
  const unsigned char* map = MAP ? map_all + (size_t)blockIdx.y * mvs : nullptr;
  const int val = MAP ? map[p] : 0;
  auto joined = [&](int i) {                                    // i is foreground (of p's class)
    if constexpr (MAP) return map[i] == val;
    else return parent[i] >= 0;
  };
  const int HW = H * W;
  const int w = p % W, h = (p / W) % H, d = p / HW;
  const bool left = w > 0 && joined(p - 1);
  // -x: lanes 1..63 were joined to their run by the init; lane 0 joins the run that ends in the wave before
  if (left && (threadIdx.x & 63) == 0) cc_union(parent, p, p - 1);
#pragma unroll
  for (int dz = -1; dz <= 0; ++dz)
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy) {
      if (!(dz < 0 || dy < 0)) continue;                        // the backward half: (dz, dy) before (0, 0)
      const int zz = d + dz, yy = h + dy;
      if (zz < 0 || yy < 0 || yy >= H) continue;
#pragma unroll
      for (int dx = -1; dx <= 1; ++dx) {
        const int nnz = (dz != 0) + (dy != 0) + (dx != 0);
        if (nnz > conn) continue;
        const int xx = w + dx;
        if (xx < 0 || xx >= W) continue;
        const int q = p + dz * HW + dy * W + dx;
        if (!joined(q)) continue;
        if (dx == 0) {
          // p - 1 and q - 1 are both foreground: p ~ p - 1 and q ~ q - 1 along x, and p - 1 makes (or skips for the same
          // reason, down to the start of the run) this union with q - 1
          if (left && joined(q - 1)) continue;
        } else {
          // r = p + (dz, dy, 0) is foreground: q ~ r along x, and p ~ r is this voxel's own union at dx == 0 (an offset with
          // one non-zero component fewer, so inside the footprint)
          if (joined(q - dx)) continue;
        }
        cc_union(parent, p, q);
      }
    }
}

// grid (nb = ceil(vox / CC_SCAN_BLOCK), V): parent[p] = find(p), and blocksum[v][block] = the roots in the block
__global__ __launch_bounds__(CC_THREADS) void cc_flatten_kernel(int* __restrict__ parent_all, long pvs, int vox,
                                                                int* __restrict__ blocksum, int nb) {
  int* parent = parent_all + (size_t)blockIdx.y * pvs;
  int n = 0;
#pragma unroll
  for (int j = 0; j < CC_PER_THREAD; ++j) {
    const long p = (long)blockIdx.x * CC_SCAN_BLOCK + j * CC_THREADS + threadIdx.x;
    if (p >= vox) continue;
    const int x = parent[p];
    if (x < 0) continue;
    const int r = cc_find(parent, (int)p);
    if (r != x) __hip_atomic_store(parent + p, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    n += r == (int)p;
  }
  __shared__ int red[CC_WAVES];
  n = cc_wave_sum(n);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = n;
  __syncthreads();
  if (threadIdx.x == 0) {
    int t = 0;
    for (int k = 0; k < CC_WAVES; ++k) t += red[k];
    blocksum[(size_t)blockIdx.y * nb + blockIdx.x] = t;
  }
}

// grid (V), 256 threads: blocksum[v][0 .. nb) becomes its exclusive prefix sum, counts[v] the total (fixed order: deterministic)
__global__ __launch_bounds__(CC_THREADS) void cc_scan_blocks_kernel(int* __restrict__ blocksum, int nb, int* __restrict__ counts) {
  __shared__ int s[CC_THREADS];
  int* bs = blocksum + (size_t)blockIdx.x * nb;
  int carry = 0;
  for (int base = 0; base < nb; base += CC_THREADS) {            // uniform trip count
    const int i = base + threadIdx.x;
    const int x = i < nb ? bs[i] : 0;
    s[threadIdx.x] = x;
    __syncthreads();
    for (int off = 1; off < CC_THREADS; off <<= 1) {
      const int y = (int)threadIdx.x >= off ? s[threadIdx.x - off] : 0;
      __syncthreads();
      s[threadIdx.x] += y;
      __syncthreads();
    }
    if (i < nb) bs[i] = carry + s[threadIdx.x] - x;
    carry += s[CC_THREADS - 1];
    __syncthreads();
  }
  if (threadIdx.x == 0) counts[blockIdx.x] = carry;
}

// grid (nb, V): label of a root = 1 + (roots before its block) + (roots before it inside the block); background 0; the other
// foreground voxels are left to cc_propagate_kernel.  Order inside the block: j-major, then wave, then lane = the voxel index.
__global__ __launch_bounds__(CC_THREADS) void cc_rank_kernel(const int* __restrict__ parent_all, long pvs, int vox,
                                                             const int* __restrict__ blockpre, int nb, int* __restrict__ labels) {
  const int* parent = parent_all + (size_t)blockIdx.y * pvs;
  int* lab = labels + (size_t)blockIdx.y * (size_t)vox;
  __shared__ int wt[CC_PER_THREAD * CC_WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int within[CC_PER_THREAD], kind[CC_PER_THREAD];                // kind: 0 outside / non-root foreground, 1 background, 2 root
#pragma unroll
  for (int j = 0; j < CC_PER_THREAD; ++j) {
    const long p = (long)blockIdx.x * CC_SCAN_BLOCK + j * CC_THREADS + threadIdx.x;
    int x = 0;
    kind[j] = 0;
    if (p < vox) {
      x = parent[p];
      kind[j] = x < 0 ? 1 : (x == (int)p ? 2 : 0);
    }
    const unsigned long long roots = __ballot(kind[j] == 2);
    within[j] = __popcll(roots & ((1ull << lane) - 1ull));
    if (lane == 0) wt[j * CC_WAVES + wave] = __popcll(roots);
  }
  __syncthreads();
  const int base = 1 + blockpre[(size_t)blockIdx.y * nb + blockIdx.x];
#pragma unroll
  for (int j = 0; j < CC_PER_THREAD; ++j) {
    const long p = (long)blockIdx.x * CC_SCAN_BLOCK + j * CC_THREADS + threadIdx.x;
    int before = 0;
    for (int k = 0; k < j * CC_WAVES + wave; ++k) before += wt[k];
    if (kind[j] == 2) lab[p] = base + before + within[j];
    else if (kind[j] == 1) lab[p] = 0;
  }
}

// grid (nb, V): a non-root foreground voxel takes the label of its root (written by the launch before; roots are not
// written here)
__global__ __launch_bounds__(CC_THREADS) void cc_propagate_kernel(const int* __restrict__ parent_all, long pvs, int vox,
                                                                  int* __restrict__ labels) {
  const int* parent = parent_all + (size_t)blockIdx.y * pvs;
  int* lab = labels + (size_t)blockIdx.y * (size_t)vox;
#pragma unroll
  for (int j = 0; j < CC_PER_THREAD; ++j) {
    const long p = (long)blockIdx.x * CC_SCAN_BLOCK + j * CC_THREADS + threadIdx.x;
    if (p >= vox) continue;
    const int x = parent[p];
    if (x >= 0 && x != (int)p) lab[p] = lab[x];
  }
}

// grid (nb, V): sizes[v][l - 1] += the voxels of label l, 1 <= l <= cap.  Per wave, the lanes that share a label are counted
// with one ballot and ONE lane adds: one atomic per distinct label per wave (raster neighbours mostly share theirs).
__global__ __launch_bounds__(CC_THREADS) void cc_sizes_kernel(const int* __restrict__ labels, int vox, int cap,
                                                              int* __restrict__ sizes) {
  const int* lab = labels + (size_t)blockIdx.y * (size_t)vox;
  int* sz = sizes + (size_t)blockIdx.y * cap;
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int j = 0; j < CC_PER_THREAD; ++j) {
    const long p = (long)blockIdx.x * CC_SCAN_BLOCK + j * CC_THREADS + threadIdx.x;
    const int l = p < vox ? lab[p] : 0;
    const bool valid = l >= 1 && l <= cap;
    unsigned long long todo = __ballot(valid);                   // wave-uniform: every lane runs the same iterations
    while (todo) {
      const int leader = __ffsll((long long)todo) - 1;
      const int ll = __shfl(l, leader, 64);
      const unsigned long long same = __ballot(valid && l == ll);
      if (lane == leader) atomicAdd(sz + (ll - 1), __popcll(same));
      todo &= ~same;                                             // `same` holds the leader's bit: todo shrinks every time
    }
  }
}

// grid (ceil(cap / 256), V): keep[v][l - 1] for the labels 1 .. n = min(counts[v], cap).  The position of label l in
// np.argsort(-sizes, kind="stable") is the number of labels that are larger, or equal and smaller in number; l is kept when
// that position is below k (k == 0: no limit on the number) and its size is at least min_size.
// MAP (the label-map form): cls[v][l - 1] is the class of label l, and the position is taken among the labels of l's class.
template <bool MAP>
__global__ __launch_bounds__(CC_THREADS) void cc_select_kernel(const int* __restrict__ sizes, const int* __restrict__ counts,
                                                               int cap, int k, int min_size, unsigned char* __restrict__ keep,
                                                               const unsigned char* __restrict__ cls_all) {
  __shared__ int tile[CC_THREADS];
  __shared__ unsigned char ctile[MAP ? CC_THREADS : 1];
  const unsigned char* cls = MAP ? cls_all + (size_t)blockIdx.y * cap : nullptr;
  const int v = blockIdx.y;
  const int* sz = sizes + (size_t)v * cap;
  int n = counts[v];
  n = n < 0 ? 0 : (n > cap ? cap : n);
  const int l = blockIdx.x * CC_THREADS + threadIdx.x;           // label l + 1
  const int mine = l < n ? sz[l] : 0;
  const int myc = MAP && l < n ? cls[l] : 0;
  int pos = 0;
  if (k > 0 && (int)(blockIdx.x * CC_THREADS) < n) {             // block-uniform
    for (int base = 0; base < n; base += CC_THREADS) {
      __syncthreads();
      tile[threadIdx.x] = base + (int)threadIdx.x < n ? sz[base + threadIdx.x] : -1;
      if constexpr (MAP) ctile[threadIdx.x] = base + (int)threadIdx.x < n ? cls[base + threadIdx.x] : 0;
      __syncthreads();
      const int m = n - base < CC_THREADS ? n - base : CC_THREADS;
      for (int t = 0; t < m; ++t) {
        const int s = tile[t];
        pos += (!MAP || ctile[t] == myc) && ((s > mine) || (s == mine && base + t < l));
      }
    }
  }
  if (l < cap) keep[(size_t)v * cap + l] = l < n && (k == 0 || pos < k) && mine >= min_size;
}

// grid (nb, V): out[v][p] = the voxel's component is kept (apply[v] != 0 or no apply), else the mask itself; with a reference,
// the block's (|A & B|, |A|, |B|) go to tallies[c = v % C] with one integer atomic per counter.
__global__ __launch_bounds__(CC_THREADS) void cc_filter_kernel(const int* __restrict__ labels, int vox, int cap,
                                                               const unsigned char* __restrict__ keep,
                                                               const unsigned char* __restrict__ apply,
                                                               const void* __restrict__ mask, int mask_f32, long mvs,
                                                               unsigned char* __restrict__ out, const void* __restrict__ ref,
                                                               int ref_kind, int C, unsigned long long* __restrict__ tallies) {
  const int v = blockIdx.y;
  const int* lab = labels + (size_t)v * (size_t)vox;
  const unsigned char* kp = keep + (size_t)v * cap;
  const bool on = !apply || apply[v] != 0;
  const int c = v % C, b = v / C;
  int n[3] = {0, 0, 0};                                          // |A & B|, |A|, |B|
#pragma unroll
  for (int j = 0; j < CC_PER_THREAD; ++j) {
    const long p = (long)blockIdx.x * CC_SCAN_BLOCK + j * CC_THREADS + threadIdx.x;
    if (p >= vox) continue;
    bool a;
    if (on) {
      const int l = lab[p];
      a = l >= 1 && l <= cap && kp[l - 1] != 0;
    } else {
      a = cc_fg(mask, mask_f32, (size_t)v * mvs + (size_t)p);
    }
    out[(size_t)v * (size_t)vox + (size_t)p] = a ? 1 : 0;
    if (ref_kind != CC_REF_NONE) cc_onehot_add(n, a, cc_ref_fg(ref, ref_kind, v, b, c, vox, p));
  }
  if (ref_kind == CC_REF_NONE) return;                           // kernel-uniform
  __shared__ int red[CC_WAVES][3];
  cc_onehot_flush(cc_block_totals<3>(n, red, 0), c, tallies);
}

// ---- the label-map form of the filter ------------------------------------------------------------------------------------

// grid (nb, V): cls[v][l - 1] = the class of label l, 1 <= l <= cap.  A component carries one value, the value at its root; every
// voxel that starts a run of its label along W stores that same byte (identical stores: the order does not matter).
__global__ __launch_bounds__(CC_THREADS) void cc_class_kernel(const int* __restrict__ labels, const unsigned char* __restrict__ map,
                                                              long mvs, int vox, int W, int cap, unsigned char* __restrict__ cls) {
  const int v = blockIdx.y;
  const int* lab = labels + (size_t)v * (size_t)vox;
#pragma unroll
  for (int j = 0; j < CC_PER_THREAD; ++j) {
    const long p = (long)blockIdx.x * CC_SCAN_BLOCK + j * CC_THREADS + threadIdx.x;
    if (p >= vox) continue;
    const int l = lab[p];
    if (l < 1 || l > cap) continue;
    if (p % W != 0 && lab[p - 1] == l) continue;
    cls[(size_t)v * cap + (l - 1)] = map[(size_t)v * mvs + (size_t)p];
  }
}

// grid (nb, V): out[v][p] = map[v][p] where the value is 0 or >= C, where its class is passed through (apply[value] == 0) or
// where the voxel's component is kept; 0 otherwise.  TALLY: (|A & B|, |A|, |B|) of A = out, B = ref per class (CcMapTally).
template <bool TALLY>
__global__ __launch_bounds__(CC_THREADS) void cc_filter_map_kernel(const int* __restrict__ labels, int vox, int cap,
                                                                   const unsigned char* __restrict__ keep,
                                                                   const unsigned char* __restrict__ apply,
                                                                   const unsigned char* __restrict__ map, long mvs, int C,
                                                                   unsigned char* __restrict__ out,
                                                                   const unsigned char* __restrict__ ref,
                                                                   unsigned long long* __restrict__ tallies) {
  __shared__ unsigned part[TALLY ? 3 * DUA_BLEND_MAX_CLASSES : 1];
  __shared__ int red[TALLY ? CC_WAVES : 1][3];
  const int v = blockIdx.y;
  const int* lab = labels + (size_t)v * (size_t)vox;
  const unsigned char* kp = keep + (size_t)v * cap;
  CcMapTally tally{part, red};
  if constexpr (TALLY) {
    tally.zero(C);
    __syncthreads();
  }
#pragma unroll
  for (int j = 0; j < CC_PER_THREAD; ++j) {
    const long p = (long)blockIdx.x * CC_SCAN_BLOCK + j * CC_THREADS + threadIdx.x;
    if (p >= vox) continue;
    const int val = map[(size_t)v * mvs + (size_t)p];
    int o = val;
    if (val >= 1 && val < C && (!apply || apply[val] != 0)) {
      const int l = lab[p];
      if (!(l >= 1 && l <= cap && kp[l - 1] != 0)) o = 0;
    }
    out[(size_t)v * (size_t)vox + (size_t)p] = (unsigned char)o;
    if constexpr (TALLY) tally.add(o, ref[(size_t)v * (size_t)vox + (size_t)p], C);
  }
  if constexpr (TALLY) {
    tally.reduce();
    __syncthreads();
    tally.flush(C, tallies);
  }
}

// ---- host side ----------------------------------------------------------------------------------------------------------

void cc_launch_merge(hipStream_t s, int V, int D, int H, int W, int connectivity, int* parent, long pvs) {
  const long vox = (long)D * H * W;
  hipLaunchKernelGGL(cc_merge_kernel<false>, dim3((unsigned)((vox + CC_THREADS - 1) / CC_THREADS), V), dim3(CC_THREADS), 0, s,
                     parent, pvs, D, H, W, connectivity, (const unsigned char*)nullptr, 0L);
}

void cc_launch_flatten(hipStream_t s, int V, long vox, int* parent, long pvs, int* blocksum, long nb) {
  hipLaunchKernelGGL(cc_flatten_kernel, dim3((unsigned)nb, V), dim3(CC_THREADS), 0, s, parent, pvs, (int)vox, blocksum, (int)nb);
}

// the numbering both label entry points run on the parents an init and a merge left: flatten, scan of the block counts, rank,
// propagate
static void cc_launch_number(hipStream_t s, int V, long vox, int* parent, long pvs, int* blocksum, long nb, int* counts,
                             int* labels) {
  const dim3 threads(CC_THREADS), gscan((unsigned)nb, V);
  cc_launch_flatten(s, V, vox, parent, pvs, blocksum, nb);
  hipLaunchKernelGGL(cc_scan_blocks_kernel, dim3(V), threads, 0, s, blocksum, (int)nb, counts);
  hipLaunchKernelGGL(cc_rank_kernel, gscan, threads, 0, s, parent, pvs, (int)vox, blocksum, (int)nb, labels);
  hipLaunchKernelGGL(cc_propagate_kernel, gscan, threads, 0, s, parent, pvs, (int)vox, labels);
}

struct CcScratch : CcPrefix {
  long keep, total;
  long cls, total_map;               // the label-map form: the class table behind the keep table
};

static CcScratch cc_layout(int V, int D, int H, int W, int cap) {
  CcScratch L{cc_layout_prefix(V, D, H, W)};
  L.keep = L.end;
  L.total = cc_align256(L.keep + (long)V * cap);
  L.cls = L.total;
  L.total_map = cc_align256(L.cls + (long)V * cap);
  return L;
}

}  // namespace dua

extern "C" {

long dua_cc_scratch_bytes(int V, int D, int H, int W, int cap) {
  if (!dua::cc_extents_ok(V, D, H, W) || cap < 1 || cap > DUA_CC_MAX_CAP) return DUA_ERR_ARG;
  return dua::cc_layout(V, D, H, W, cap).total;
}

int dua_cc_label(int V, int D, int H, int W, const void* mask, int mask_dtype, long mask_vstride, int connectivity,
                 const unsigned char* select, int* labels, int* counts, void* workspace, long workspace_bytes, void* stream) {
  if (!dua::cc_extents_ok(V, D, H, W) || !mask || !labels || !counts || !workspace || connectivity < 1 || connectivity > 3 ||
      !dua::cc_mask_dtype_ok(mask_dtype))
    return DUA_ERR_ARG;
  const long vox = (long)D * H * W;
  const dua::CcScratch L = dua::cc_layout(V, D, H, W, 1);         // the labelling part of the layout does not depend on cap
  if (mask_vstride < vox || workspace_bytes < L.keep || ((size_t)workspace & 255) != 0 || ((size_t)labels & 3) != 0 ||
      ((size_t)counts & 3) != 0 || (mask_dtype == DUA_F32 && ((size_t)mask & 3) != 0))
    return DUA_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  int* parent = (int*)((unsigned char*)workspace + L.parent);
  int* blocksum = (int*)((unsigned char*)workspace + L.blocksum);
  const dim3 threads(dua::CC_THREADS), gvox((unsigned)((vox + dua::CC_THREADS - 1) / dua::CC_THREADS), V);
  const int is_f32 = mask_dtype == DUA_F32;
  hipLaunchKernelGGL(dua::cc_init_kernel, gvox, threads, 0, s, mask, is_f32, mask_vstride, select, (int)vox, W, parent, L.pvs);
  dua::cc_launch_merge(s, V, D, H, W, connectivity, parent, L.pvs);
  dua::cc_launch_number(s, V, vox, parent, L.pvs, blocksum, L.nb, counts, labels);
  return (int)hipGetLastError();
}

int dua_cc_sizes(int V, int D, int H, int W, const int* labels, int cap, int* sizes, void* stream) {
  if (!dua::cc_extents_ok(V, D, H, W) || !labels || !sizes || cap < 1 || cap > DUA_CC_MAX_CAP || ((size_t)labels & 3) != 0 ||
      ((size_t)sizes & 3) != 0)
    return DUA_ERR_ARG;
  const long vox = (long)D * H * W;
  hipStream_t s = (hipStream_t)stream;
  const hipError_t e = hipMemsetAsync(sizes, 0, (size_t)V * cap * sizeof(int), s);
  if (e != hipSuccess) return (int)e;
  const dim3 grid((unsigned)((vox + dua::CC_SCAN_BLOCK - 1) / dua::CC_SCAN_BLOCK), V);
  hipLaunchKernelGGL(dua::cc_sizes_kernel, grid, dim3(dua::CC_THREADS), 0, s, labels, (int)vox, cap, sizes);
  return (int)hipGetLastError();
}

int dua_cc_filter(int V, int D, int H, int W, const int* labels, const int* counts, const int* sizes, int cap, int k,
                  int min_size, const unsigned char* apply, const void* mask, int mask_dtype, long mask_vstride,
                  unsigned char* out, const void* reference, int reference_dtype, int label_map, int C,
                  unsigned long long* tallies, void* workspace, long workspace_bytes, void* stream) {
  if (!dua::cc_extents_ok(V, D, H, W) || !labels || !counts || !sizes || !out || !workspace || cap < 1 || cap > DUA_CC_MAX_CAP ||
      k < 0 || ((size_t)labels & 3) != 0 || ((size_t)counts & 3) != 0 || ((size_t)sizes & 3) != 0)
    return DUA_ERR_ARG;
  const long vox = (long)D * H * W;
  if (apply && !mask) return DUA_ERR_ARG;                        // a volume passed through is copied from its mask
  if (mask && (!dua::cc_mask_dtype_ok(mask_dtype) || mask_vstride < vox || (mask_dtype == DUA_F32 && ((size_t)mask & 3) != 0)))
    return DUA_ERR_ARG;
  int kind;
  if (dua::cc_reference_kind(reference, reference_dtype, label_map, C, V, tallies, &kind) != 0) return DUA_ERR_ARG;
  const dua::CcScratch L = dua::cc_layout(V, D, H, W, cap);
  if (workspace_bytes < L.total || ((size_t)workspace & 255) != 0) return DUA_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  unsigned char* keep = (unsigned char*)workspace + L.keep;
  if (tallies) {
    const hipError_t e = hipMemsetAsync(tallies, 0, sizeof(unsigned long long) * 3 * C, s);
    if (e != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL(dua::cc_select_kernel<false>, dim3((unsigned)((cap + dua::CC_THREADS - 1) / dua::CC_THREADS), V),
                     dim3(dua::CC_THREADS), 0, s, sizes, counts, cap, k, min_size, keep, (const unsigned char*)nullptr);
  hipLaunchKernelGGL(dua::cc_filter_kernel, dim3((unsigned)L.nb, V), dim3(dua::CC_THREADS), 0, s, labels, (int)vox, cap, keep,
                     apply, mask, mask_dtype == DUA_F32, mask_vstride, out, reference, kind, reference ? C : 1, tallies);
  return (int)hipGetLastError();
}

long dua_cc_map_scratch_bytes(int V, int D, int H, int W, int cap) {
  if (!dua::cc_extents_ok(V, D, H, W) || cap < 1 || cap > DUA_CC_MAX_CAP) return DUA_ERR_ARG;
  return dua::cc_layout(V, D, H, W, cap).total_map;
}

int dua_cc_label_map(int V, int D, int H, int W, const unsigned char* map, long map_vstride, int C, int connectivity, int* labels,
                     int* counts, void* workspace, long workspace_bytes, void* stream) {
  if (!dua::cc_extents_ok(V, D, H, W) || !map || !labels || !counts || !workspace || connectivity < 1 || connectivity > 3 ||
      C < 1 || C > DUA_BLEND_MAX_CLASSES)
    return DUA_ERR_ARG;
  const long vox = (long)D * H * W;
  const dua::CcScratch L = dua::cc_layout(V, D, H, W, 1);         // the labelling part of the layout does not depend on cap
  if (map_vstride < vox || workspace_bytes < L.keep || ((size_t)workspace & 255) != 0 || ((size_t)labels & 3) != 0 ||
      ((size_t)counts & 3) != 0)
    return DUA_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  int* parent = (int*)((unsigned char*)workspace + L.parent);
  int* blocksum = (int*)((unsigned char*)workspace + L.blocksum);
  const dim3 threads(dua::CC_THREADS), gvox((unsigned)((vox + dua::CC_THREADS - 1) / dua::CC_THREADS), V);
  hipLaunchKernelGGL(dua::cc_init_map_kernel, gvox, threads, 0, s, map, map_vstride, C, (int)vox, W, parent, L.pvs);
  hipLaunchKernelGGL(dua::cc_merge_kernel<true>, gvox, threads, 0, s, parent, L.pvs, D, H, W, connectivity, map, map_vstride);
  dua::cc_launch_number(s, V, vox, parent, L.pvs, blocksum, L.nb, counts, labels);
  return (int)hipGetLastError();
}

int dua_cc_filter_map(int V, int D, int H, int W, const unsigned char* map, long map_vstride, int C, const int* labels,
                      const int* counts, const int* sizes, int cap, int k, int min_size, const unsigned char* apply,
                      unsigned char* out, const unsigned char* reference, unsigned long long* tallies, void* workspace,
                      long workspace_bytes, void* stream) {
  if (!dua::cc_extents_ok(V, D, H, W) || !map || !labels || !counts || !sizes || !out || !workspace || cap < 1 ||
      cap > DUA_CC_MAX_CAP || k < 0 || C < 1 || C > DUA_BLEND_MAX_CLASSES || ((size_t)labels & 3) != 0 ||
      ((size_t)counts & 3) != 0 || ((size_t)sizes & 3) != 0)
    return DUA_ERR_ARG;
  const long vox = (long)D * H * W;
  if (map_vstride < vox || (reference != nullptr) != (tallies != nullptr) || ((size_t)tallies & 7) != 0) return DUA_ERR_ARG;
  const dua::CcScratch L = dua::cc_layout(V, D, H, W, cap);
  if (workspace_bytes < L.total_map || ((size_t)workspace & 255) != 0) return DUA_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  unsigned char* keep = (unsigned char*)workspace + L.keep;
  unsigned char* cls = (unsigned char*)workspace + L.cls;
  if (tallies) {
    const hipError_t e = hipMemsetAsync(tallies, 0, sizeof(unsigned long long) * 3 * C, s);
    if (e != hipSuccess) return (int)e;
  }
  const dim3 threads(dua::CC_THREADS), gscan((unsigned)L.nb, V);
  hipLaunchKernelGGL(dua::cc_class_kernel, gscan, threads, 0, s, labels, map, map_vstride, (int)vox, W, cap, cls);
  hipLaunchKernelGGL(dua::cc_select_kernel<true>, dim3((unsigned)((cap + dua::CC_THREADS - 1) / dua::CC_THREADS), V), threads, 0,
                     s, sizes, counts, cap, k, min_size, keep, (const unsigned char*)cls);
  if (tallies)
    hipLaunchKernelGGL(dua::cc_filter_map_kernel<true>, gscan, threads, 0, s, labels, (int)vox, cap, keep, apply, map, map_vstride,
                       C, out, reference, tallies);
  else
    hipLaunchKernelGGL(dua::cc_filter_map_kernel<false>, gscan, threads, 0, s, labels, (int)vox, cap, keep, apply, map,
                       map_vstride, C, out, reference, tallies);
  return (int)hipGetLastError();
}

}  // extern "C"
