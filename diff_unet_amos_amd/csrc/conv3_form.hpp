// Which kernel, tile, split, grid and LDS size a 3x3x3 convolution or a transposed convolution launch takes: decided HERE, in
// pure host code (no HIP call, no allocation), once.  The launchers (conv3d_igemm.hip, conv3d_wide.hip, deconv.hip) switch over
// the form this gives them; the exported queries (dua_conv3d_k3_form, dua_conv3d_k3_kernel_kind, dua_conv3d_k3_workspace,
// dua_conv3d_k3_dgrad_reduce_supported, dua_deconv_k2s2_form, dua_deconv_k2s2_kernel_kind) are projections of the same form.
// The tile and LDS constants of the kernels live here too, so that the LDS bytes of a form and the limits registered for
// dua_prepare() (kConvLdsAttrs, kWideLdsAttrs, kDeconvLdsAttrs) come from the same names.
#pragma once
#include "../../include/dua_hip.h"
#include <algorithm>
#include <initializer_list>

namespace dua {

// ---- tile and LDS constants of the kernels ------------------------------------------------------------------------------
namespace c3 {
constexpr int TD = 4, TH = 8, TW = 8;
constexpr int HD = TD + 2, HH = TH + 2, HW = TW + 2;
constexpr int KG = 4;                      // k-groups (16 B) per chunk
constexpr int VS = KG * 16;                // 64 B per halo voxel per chunk
constexpr int RS = HW * VS + 16;           // 656: halo row stride, padded (bank-conflict free)
constexpr int PS = HH * RS;                // 6560: halo plane stride
constexpr int HALO_BYTES = HD * PS;        // 39360
constexpr int BN = 64;                     // output channels per workgroup
}  // namespace c3

namespace c3v2 {
using namespace c3;
constexpr int SLAB = 3 * KG * BN * 16;             // 12288
constexpr int LDS_MAIN = HALO_BYTES + 2 * SLAB;    // 63936
}  // namespace c3v2

// Halo image: 32 B per voxel (the 16 ordinary channels; the image channel goes to an fp16 array of its own), 12 voxel slots
// per row (10 used), and the two 16-byte halves of a voxel swapped on odd halo rows: with that the four 16-lane groups of
// every ds_read_b128 fragment read cover all 64 banks once (rows r>>3 = 0..3 of a 32-voxel block land on 16-byte slots
// {0,2,4,6}+8k / {1,3,5,7}+8k).
namespace c3f {
using namespace c3;
constexpr int VSF = 32, RSF = 12 * VSF, PSF = HH * RSF;      // 384-byte rows, 3840-byte planes
constexpr int HALO_F = HD * PSF;                              // 23040
constexpr int WRES = 27 * 2 * BN * 16;                        // 55296: [tap][k-half][64 couts][16 B]
constexpr int IMG_F = 1216;                                   // 600 fp16 of the image halo (+ pad)
constexpr int LDS_F = WRES + HALO_F + IMG_F;                  // 79552: two workgroups per CU
constexpr int NV = HD * HH * HW;                              // 600 halo voxels
}  // namespace c3f

namespace c3w {
constexpr int TH = 8, TW = 8, HH = TH + 2, HW = TW + 2;
constexpr int VSF = 32, RSF = 12 * VSF, PSF = HH * RSF;      // 384-byte rows, 3840-byte planes
constexpr int BN = 64;
constexpr int WPLANE = 18 * 1024;                              // [9 taps][2 k-groups][64 couts][16 B]
constexpr int HALO_MAX = 10 * PSF;                             // 38400: the 8-deep tile
constexpr int LDS_FIXED = HALO_MAX + 2 * WPLANE;               // 75264
constexpr int SLAB = 3 * 4 * BN * 16;                          // 12288: one (kd, kh) slab of the packed weights (32-channel chunk)
}  // namespace c3w

namespace dc {
constexpr int TM = 256, BN = 64, KG = 4;
constexpr int VS = KG * 16 + 16;          // 80 B per voxel: conflict-free for 32 consecutive rows
constexpr int A_BYTES = TM * VS;          // 20480
constexpr int W_BYTES = KG * BN * 16;     // 4096
}  // namespace dc

namespace dcs {
constexpr int TMS = 64, MC = 4;
constexpr int STAGE = TMS * dc::VS + dc::W_BYTES;            // 5120 + 4096 per wave
constexpr int RS = dc::BN * 4 + 16;                          // fp32 partial row: 272 B
constexpr int RED = 4 * TMS * RS;                            // 69632: the staging rows live inside it
}  // namespace dcs

// ---- dynamic LDS: what a launch asks for, and the limit registered for its kernel -------------------------------------------
constexpr int LDS_CU = 160 * 1024;            // the whole LDS of a CU: the one-workgroup-per-CU kernels register all of it
constexpr int MAX_PACKED_CIN = 1024;          // packed input channels a launch may have (the transform tables are sized for it)
// scale / shift / add tables (fp32) of a fused producer transform, behind the tiles
constexpr int xf_lds(int packed_cin) { return 3 * 4 * packed_cin; }
constexpr int XF_LDS_MAX = xf_lds(MAX_PACKED_CIN);
// A background launch (dua_conv3_desc.background) runs on a second stream UNDER other launches: it asks for enough
// extra LDS that only ONE of its workgroups fits a CU, so that every CU keeps 64 KB and half its wave slots free for the
// main stream's workgroups (two of them per CU leave no room: the co-running launches then wait for retiring workgroups).
constexpr int PARTIAL_LDS_PAD = 36 * 1024;
constexpr int TAP_LDS = c3v2::LDS_MAIN + 4096;                                // the tap forms: + the [voxel][32] tap tile
constexpr int FIRST_LDS = c3f::LDS_F + 2048;                                  // + the statistics exchange
constexpr int V2_TD2_LDS = 4 * c3::HH * c3::RS + 2 * c3v2::SLAB;             // 2x8x8 tiles: a 4-plane halo
constexpr int V2_TD2_KD_LDS = 4 * c3::HH * c3::RS + 9 * c3v2::SLAB;          // ... with a ring of three kd planes
constexpr int V2_TD4_KD_LDS = c3::HALO_BYTES + 9 * c3v2::SLAB;
constexpr int WIDE_LDS_LIMIT = 80 * 1024;                                     // two workgroups per CU
constexpr int WIDE_BWD_LDS = 1024;                                            // exchange of the backward-sums epilogue

constexpr int conv3_lds_limit(int kernel) {
  switch (kernel) {
    case DUA_CONV3_FIRST: return FIRST_LDS + PARTIAL_LDS_PAD;
    case DUA_CONV3_TAP0: case DUA_CONV3_TAP1: return TAP_LDS + PARTIAL_LDS_PAD;
    case DUA_CONV3_WIDE: case DUA_CONV3_WIDE_BWD: return WIDE_LDS_LIMIT;
    case DUA_CONV3_V2_4: case DUA_CONV3_V2_4_HALF: return c3v2::LDS_MAIN + XF_LDS_MAX + PARTIAL_LDS_PAD;
    case DUA_CONV3_V2_2: return c3v2::LDS_MAIN + XF_LDS_MAX;
    default: return LDS_CU;                                                   // the kd-plane forms
  }
}

template <int ELEM_BYTES> constexpr int deconv_one_tap_lds() {                // staging tiles or the output tile, whichever is larger
  constexpr int OS = dc::BN * ELEM_BYTES + 16;
  return dc::TM * OS > dc::A_BYTES + dc::W_BYTES ? dc::TM * OS : dc::A_BYTES + dc::W_BYTES;
}
constexpr int deconv_alltaps_lds(int tm, int nchunks, int elem_bytes) {
  return tm * (nchunks * 64 + 16) + 4 * nchunks * dc::W_BYTES + 2 * tm * (32 * elem_bytes + 16);
}
constexpr int deconv_lds_limit(int kernel, int elem_bytes) {
  switch (kernel) {
    case DUA_DECONV_ONE_TAP: return (elem_bytes == 2 ? deconv_one_tap_lds<2>() : deconv_one_tap_lds<4>()) + XF_LDS_MAX;
    case DUA_DECONV_KSPLIT: return dcs::RED + XF_LDS_MAX;
    default: return LDS_CU;
  }
}

// ---- dua_conv3_desc.policy, decoded once --------------------------------------------------------------------------------
// The only place that knows the hand-set values (include/dua_hip.h lists them); everything else reads the flags.
struct Conv3Policy {
  bool wide = false;            // the wide-tile form where the layer qualifies
  bool kd_plane = false;        // kd planes by LDS-DMA for the launches that cannot put two workgroups on every CU
  bool automatic = false;       // split-K and 2x8x8 tiles by the size of the layer
  int split_target = 0;         // split-K: workgroups aimed at
  int split_max_base = 0;       // split-K: only layers of at most this many 4x8x8 workgroups
  bool td2 = false;             // 2x8x8 tiles whatever the size
  bool first = false;           // the resident-weight first-layer kernel for the 16 + 1 channel tap form
  bool no_finish = false;       // DUA_POLICY_NO_FINISH
};
constexpr int SLAB_SPLIT_TARGET = 320, KD_SPLIT_TARGET = 256, SPLIT_MAX_BASE = 64;

inline int decode_conv3_policy(int policy, Conv3Policy* out) {
  Conv3Policy p;
  if (policy & ~(0xff | DUA_POLICY_NO_FINISH)) return DUA_ERR_ARG;
  p.no_finish = (policy & DUA_POLICY_NO_FINISH) != 0;
  auto automatic = [&p](bool kd) {
    p.automatic = true; p.kd_plane = kd;
    p.split_target = kd ? KD_SPLIT_TARGET : SLAB_SPLIT_TARGET; p.split_max_base = SPLIT_MAX_BASE;
  };
  switch (policy & 0xff) {
    case 0: automatic(true); p.wide = p.first = true; break;
    case 2: automatic(true); p.split_target = 512; p.split_max_base = 256; break;   // A/B: K split up to 256 base workgroups
    case 3: p.td2 = true; break;
    case 6: automatic(false); break;
    case 7: automatic(true); break;
    default: return DUA_ERR_ARG;
  }
  *out = p;
  return 0;
}

// dua_deconv_k2s2_fwd: 0, or 6 = no k-split kernel
struct DeconvPolicy {
  bool ksplit = true;           // Cin chunks split over the waves where the layer qualifies
};
inline int decode_deconv_policy(int policy, DeconvPolicy* out) {
  switch (policy) {
    case 0: *out = DeconvPolicy{}; return 0;
    case 6: *out = DeconvPolicy{false}; return 0;
    default: return DUA_ERR_ARG;
  }
}

// ---- split-K --------------------------------------------------------------------------------------------------------------
// (Cin chunk, kd) units over `want` workgroups per base workgroup: about one workgroup per CU, each keeping a few units.
inline void choose_split(int base_wgs, int units, int* ksplit, int* ups, int target, int max_base) {
  *ksplit = 1; *ups = units;
  if (base_wgs > max_base || units <= 1) return;  // 24^3 and up: the partial-tile round trip costs more than it buys
  int want = target == SLAB_SPLIT_TARGET ? (target + base_wgs - 1) / base_wgs : target / base_wgs;   // the slab form rounds up
  if (want < 1) want = 1;
  if (want > units) want = units;
  *ups = (units + want - 1) / want;
  *ksplit = (units + *ups - 1) / *ups;
}

// ---- the form of a convolution launch ---------------------------------------------------------------------------------------
struct Conv3Form : dua_conv3_form {
  int nchunks, ntiles, tiles_h, tiles_w, nct, cout_pad;    // geometry the kernels take (Conv3Args)
  int tap_ch;                                              // packed index of the tap channel, or -1
  int items;                                               // first-layer kernel: (sample, tile) items its workgroups walk
  int fin_G, fin_VL, fin_ITER;                             // finish launch: channel groups per pass, voxel lanes, voxels per lane
  unsigned fin_grid_x, fin_grid_y;
};

inline int conv3_chunk_elems(int dtype) { return c3::KG * (dtype == DUA_F16 ? 8 : 4); }

// bytes of fp32 partial tiles a split into ks parts needs
inline long conv3_split_bytes(const dua_conv3_desc* d, int ks, int cout_pad) {
  return ks > 1 ? (long)ks * d->N * d->D * d->H * d->W * cout_pad * 4 : 0;
}

// cus: compute units of the device (the first-layer kernel's grid; <= 0 is an error for that form only).
inline int conv3_form(const dua_conv3_desc* d, const Conv3Policy& p, bool fused, bool backward_sums, long workspace_bytes, int cus,
                      Conv3Form* f) {
  using namespace c3;
  if (d->dtype != DUA_F16 && d->dtype != DUA_F32) return DUA_ERR_ARG;
  const bool half = d->dtype == DUA_F16;
  const int CK = conv3_chunk_elems(d->dtype);
  *f = Conv3Form{};
  f->nchunks = (d->Cin + CK - 1) / CK;
  if (f->nchunks * CK > MAX_PACKED_CIN) return DUA_ERR_ARG;
  f->tiles_h = (d->H + TH - 1) / TH; f->tiles_w = (d->W + TW - 1) / TW;
  f->ntiles = ((d->D + TD - 1) / TD) * f->tiles_h * f->tiles_w;
  f->nct = (d->Cout + BN - 1) / BN;
  f->cout_pad = f->nct * BN;
  f->tile_depth = TD;
  f->ksplit = 1; f->units_per_split = f->nchunks * 3;
  f->tap_ch = d->tap_channel_plus1 > 0 ? d->tap_channel_plus1 - 1 : -1;
  const long vox = (long)d->D * d->H * d->W;
  const long base = (long)f->ntiles * f->nct * d->N;                 // workgroups of 4x8x8 tiles
  const int xf = fused ? xf_lds(f->nchunks * CK) : 0;
  const int bg_pad = d->background ? PARTIAL_LDS_PAD : 0;             // one workgroup per CU, see PARTIAL_LDS_PAD
  const bool in_blk = d->layout & DUA_IN_BLOCKED, out_blk = d->layout & DUA_OUT_BLOCKED;
  f->grid_x = f->ntiles; f->grid_y = f->nct; f->grid_z = d->N;

  if (f->tap_ch >= 0 && half) {
    // single-channel tap form (see the kernel): fp16, one Cin chunk, no fused input transform, 16 * NKS ordinary
    // channels in front of the tap channel, zero padding behind it; weights from dua_pack_conv3_weights_tap
    f->kernel = f->tap_ch == 16 ? (p.first ? DUA_CONV3_FIRST : DUA_CONV3_TAP1) : DUA_CONV3_TAP0;
  } else if (half && p.wide && !d->background && base >= 1024 && d->D % 8 == 0 && d->H % 8 == 0 && d->W % 8 == 0 && d->Cin % 16 == 0 &&
             d->Cin <= (fused ? 256 : 384) && vox * d->Cin_stride < 0x7fffffffL) {
    // fp16 layers with tiles to spare (96^3): one 8x8x8 tile per workgroup
    f->kernel = backward_sums ? DUA_CONV3_WIDE_BWD : DUA_CONV3_WIDE;
  } else {
    f->kernel = DUA_CONV3_V2_4;                                        // refined below
  }
  const bool is_wide = f->kernel == DUA_CONV3_WIDE || f->kernel == DUA_CONV3_WIDE_BWD;
  // 16-channel-blocked buffers: read by the wide-tile form only, written by it and by the first-layer kernel only
  if ((in_blk && !is_wide) || (out_blk && !is_wide && f->kernel != DUA_CONV3_FIRST)) return DUA_ERR_ARG;
  if ((in_blk && (d->Cin_off % 16 || d->Cin_stride % 16)) || (out_blk && (d->Cout_off % 16 || d->Cout_stride % 16))) return DUA_ERR_ARG;
  // only the shipped wide-tile form has the backward-sums epilogue (channels-last)
  if (backward_sums && (f->kernel != DUA_CONV3_WIDE_BWD || in_blk || out_blk)) return DUA_ERR_ARG;

  if (f->tap_ch >= 0) {
    if (!half || f->nchunks != 1 || fused || (f->tap_ch != 0 && f->tap_ch != 16) || d->Cin != f->tap_ch + 8) return DUA_ERR_ARG;
    if (f->kernel == DUA_CONV3_FIRST) {
      // two persistent workgroups per CU walk the (sample, tile) items; a background launch takes one per CU (and the LDS
      // pad that keeps a second one off the CU)
      if (cus <= 0) return DUA_ERR_ARG;
      f->items = f->ntiles * d->N;
      f->grid_x = std::min(f->items, std::max(1, (bg_pad ? 1 : 2) * cus / f->nct)); f->grid_z = 1;
      f->lds_bytes = FIRST_LDS + bg_pad;
    } else {
      f->lds_bytes = TAP_LDS + bg_pad;
    }
  } else if (is_wide) {
    f->tile_depth = 8;
    f->tiles_h = d->H / 8; f->tiles_w = d->W / 8;
    f->ntiles = (d->D / 8) * f->tiles_h * f->tiles_w;
    f->grid_x = f->ntiles;
    f->lds_bytes = c3w::LDS_FIXED + (fused ? xf_lds(d->Cin) : 0) + (backward_sums ? WIDE_BWD_LDS : 0);
    if (f->lds_bytes > WIDE_LDS_LIMIT) return DUA_ERR_ARG;
  } else {
    if (p.automatic) {
      int ks, ups;
      choose_split((int)base, f->nchunks * 3, &ks, &ups, p.split_target, p.split_max_base);
      f->workspace_needed = conv3_split_bytes(d, ks, f->cout_pad);
      if (ks > 1 && f->workspace_needed <= workspace_bytes) { f->ksplit = ks; f->units_per_split = ups; }
    }
    if (f->ksplit > 1) {
      f->kernel = p.kd_plane ? DUA_CONV3_V2_4_KD : DUA_CONV3_V2_4;
      f->grid_z = d->N * f->ksplit;
      f->lds_bytes = (p.kd_plane ? V2_TD4_KD_LDS : c3v2::LDS_MAIN) + xf;
      f->finish = !p.no_finish;
      if (f->finish) {
        if (f->cout_pad / 4 > 256) return DUA_ERR_ARG;
        f->fin_G = f->cout_pad / 4;                                // channel groups handled per block pass
        f->fin_VL = 256 / f->fin_G;
        f->fin_ITER = 8;
        auto blocks = [&] { return (vox + (long)f->fin_VL * f->fin_ITER - 1) / ((long)f->fin_VL * f->fin_ITER); };
        while (f->fin_ITER > 1 && blocks() < 128) f->fin_ITER >>= 1;   // >= ~128 blocks; every block ends with 16 atomic
                                                                       // instructions (measured: 432 blocks 14.8 us, 216 blocks
                                                                       // 10.9 us at 12^3)
        f->fin_grid_x = (unsigned)blocks(); f->fin_grid_y = d->N;
      }
    } else if (p.td2 || (p.automatic && base < 200 && base > 64)) {
      // 24^3-sized layers (too few 4x8x8 tiles for 256 CUs, too big for split-K to pay): 2x8x8 tiles, twice the workgroups.
      // The kd-plane form (nine slabs resident: one workgroup per CU) only while every workgroup has a CU of its own; with more of
      // them (12^3 at batch 4: 384) two slab-pipeline workgroups per CU are faster (64.3 vs 79.8 us on 256 -> 256, tools/bench_conv.py)
      f->tile_depth = 2;
      f->ntiles = ((d->D + 1) / 2) * f->tiles_h * f->tiles_w;
      f->grid_x = f->ntiles;
      const bool kd = p.kd_plane && (long)f->ntiles * f->nct * d->N <= 256;
      f->kernel = kd ? DUA_CONV3_V2_2_KD : DUA_CONV3_V2_2;
      f->lds_bytes = (kd ? V2_TD2_KD_LDS : V2_TD2_LDS) + xf;
    } else {
      if (half && d->Cin - (f->nchunks - 1) * CK <= CK / 2) f->kernel = DUA_CONV3_V2_4_HALF;   // e.g. Cin = 48: the last chunk is half padding
      f->lds_bytes = c3v2::LDS_MAIN + xf + bg_pad;
    }
  }
  f->lds_limit = conv3_lds_limit(f->kernel);
  return 0;
}

inline int conv3_form(const dua_conv3_desc* d, bool fused, bool backward_sums, long workspace_bytes, int cus, Conv3Form* f) {
  Conv3Policy p;
  if (!d || decode_conv3_policy(d->policy, &p)) return DUA_ERR_ARG;
  return conv3_form(d, p, fused, backward_sums, workspace_bytes, cus, f);
}

// dua_conv3d_k3_workspace: the split of the SLAB policy for the plain channels-last launch of d's shape.  Its target rounds up
// where the kd-plane targets round down, and ksplit grows with the workgroups aimed at, so this is never smaller than what any
// policy a plan runs with (0, 6, 7) splits into: a workspace of this size enables the split under each of them
// (tests/test_conv3_form.py holds the inequality).
inline long conv3_workspace_bytes(const dua_conv3_desc* d) {
  Conv3Policy slab;
  slab.automatic = true; slab.split_target = SLAB_SPLIT_TARGET; slab.split_max_base = SPLIT_MAX_BASE;
  dua_conv3_desc plain = *d;
  plain.tap_channel_plus1 = plain.background = plain.layout = 0;
  Conv3Form f;
  if (int e = conv3_form(&plain, slab, false, false, 0, 0, &f)) return e;
  return f.workspace_needed;
}

// dua_conv3d_k3_kernel_kind of a form: 0 = conv3d_k3_v2_kernel in any instantiation, 1 = first-layer, 2 = wide-tile
inline int conv3_kind_of(const Conv3Form& f) {
  if (f.kernel == DUA_CONV3_FIRST) return 1;
  return f.kernel == DUA_CONV3_WIDE || f.kernel == DUA_CONV3_WIDE_BWD ? 2 : 0;
}

// ---- the form of a transposed-convolution launch ----------------------------------------------------------------------------
struct DeconvForm : dua_deconv_form {
  int nchunks, nct;
  int Do, Ho, Wo, pad;            // output extents (2 x input, or one more: replicate pad) and whether any is odd
  int lds_base;                   // one-tap kernel: where its transform tables start
};

inline int deconv_form(const dua_conv3_desc* d, bool fused, int Do, int Ho, int Wo, DeconvForm* f) {
  DeconvPolicy p;
  if (!d || (d->dtype != DUA_F16 && d->dtype != DUA_F32) || decode_deconv_policy(d->policy, &p)) return DUA_ERR_ARG;
  const int eb = d->dtype == DUA_F16 ? 2 : 4;
  const int CK = dc::KG * 16 / eb;
  *f = DeconvForm{};
  f->nchunks = (d->Cin + CK - 1) / CK;
  f->nct = (d->Cout + dc::BN - 1) / dc::BN;
  f->Do = Do ? Do : 2 * d->D; f->Ho = Ho ? Ho : 2 * d->H; f->Wo = Wo ? Wo : 2 * d->W;
  f->pad = (f->Do | f->Ho | f->Wo) & 1;
  const long vox = (long)d->D * d->H * d->W;
  const int xf = fused ? xf_lds(f->nchunks * CK) : 0;
  f->grid_y = 8 * f->nct; f->grid_z = d->N;                         // one tap per workgroup, unless all taps below
  if (vox >= 256L * 128 && f->nchunks <= 4) {
    // enough tiles to fill the chip with one workgroup per 8 taps.  128-voxel tiles: two workgroups per CU up to 64 input
    // channels (70 KB each), one's pixel-shuffle stores under the other's loads
    f->kernel = DUA_DECONV_ALLTAPS_128;
    f->tile_voxels = 128;
    f->lds_bytes = deconv_alltaps_lds(f->tile_voxels, f->nchunks, eb) + xf;
    f->grid_y = f->nct;
  } else if (f->nchunks >= 8 && f->nchunks <= 4 * dcs::MC && p.ksplit) {   // Cin >= 256: waves split the Cin chunks
    f->kernel = DUA_DECONV_KSPLIT;
    f->tile_voxels = dcs::TMS;
    f->lds_bytes = dcs::RED + xf;
  } else {
    f->kernel = DUA_DECONV_ONE_TAP;
    f->tile_voxels = dc::TM;
    f->lds_base = eb == 2 ? deconv_one_tap_lds<2>() : deconv_one_tap_lds<4>();
    f->lds_bytes = f->lds_base + xf;
  }
  f->grid_x = (int)((vox + f->tile_voxels - 1) / f->tile_voxels);
  f->lds_limit = deconv_lds_limit(f->kernel, eb);
  // 16-channel blocks: never read; written by the all-taps kernel only
  if (d->layout & DUA_IN_BLOCKED) return DUA_ERR_ARG;
  if ((d->layout & DUA_OUT_BLOCKED) && (f->kernel < DUA_DECONV_ALLTAPS_128 || d->Cout_off % 16 || d->Cout_stride % 16 ||
                                        (long)f->Do * f->Ho * f->Wo * 16 >= 0x7fffffffL)) return DUA_ERR_ARG;
  if (f->lds_bytes > f->lds_limit || f->nchunks * CK > MAX_PACKED_CIN) return DUA_ERR_ARG;
  return 0;
}

// dua_deconv_k2s2_kernel_kind of a form: 0 = one tap per workgroup, 1 = ksplit, 2 = all taps
inline int deconv_kind_of(const DeconvForm& f) { return std::min(f.kernel, (int)DUA_DECONV_ALLTAPS_128); }

// ---- argument checks shared by the entry points -------------------------------------------------------------------------------
// A producer descriptor whose statistics are given must be complete (the fp16 kernels apply the slope as max(t, slope t)).
inline bool producer_ok(const dua_in_norm* in, int channels) {
  return in->gamma && in->beta && in->c_pad >= channels && in->count > 0 && in->slope >= 0.f && in->slope <= 1.f;
}
// descriptor and pointers present, channel counts / strides / offsets multiples of 8 (16-byte accesses), producer complete
inline bool conv_call_ok(const dua_conv3_desc* d, std::initializer_list<const void*> required, const dua_in_norm* in) {
  if (!d) return false;
  for (const void* p : required) if (!p) return false;
  if (d->Cin % 8 || d->Cout % 8 || d->Cin_stride % 8 || d->Cout_stride % 8 || d->Cin_off % 8 || d->Cout_off % 8) return false;
  return !(in && in->stats) || producer_ok(in, d->Cin);
}

}  // namespace dua
