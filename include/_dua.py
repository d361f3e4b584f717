# models/basic_unet/_dua.py  (new file in the reference; shipped here as include/_dua.py and executed by
# tests/test_integration_stub.py, so it cannot drift from include/dua_hip.h)
"""Kernel-level binding of libdua_hip.so for a maintainer of aarchiiive/diff-unet-amos: nn.Conv3d(k3, s1, p1) of MONAI's
Convolution block (models/basic_unet/denoiser.py:56-59) on the MI355X kernel, from channels-last fp16 tensors.
Needs nothing from the diff_unet_amos_amd Python package -- only the shared library."""
import ctypes as C
import os

import torch          # first: the library binds to the libamdhip64 torch has already mapped (one HIP runtime, shared streams)

DUA_ABI_VERSION = 8   # of the include/dua_hip.h this file was written against
_L = C.CDLL(os.environ.get("DUA_HIP_SO", "/path/to/diff_unet_amos_amd/libdua_hip.so"))
_L.dua_abi_version.restype = C.c_int
if _L.dua_abi_version() != DUA_ABI_VERSION:      # struct layouts differ between ABI versions: refuse, never reinterpret
    raise ImportError(f"libdua_hip.so has ABI {_L.dua_abi_version()}, this binding was written for {DUA_ABI_VERSION}")


class Conv3Desc(C.Structure):                    # dua_conv3_desc: 15 ints
    _fields_ = [(n, C.c_int) for n in ("dtype", "N", "D", "H", "W", "Cin", "Cin_stride", "Cin_off",
                                       "Cout", "Cout_stride", "Cout_off", "tap_channel_plus1", "background",
                                       "layout", "policy")]


class InNorm(C.Structure):                       # dua_in_norm: the producer's InstanceNorm + LeakyReLU, fused into the consumer
    _fields_ = [("stats", C.c_void_p), ("gamma", C.c_void_p), ("beta", C.c_void_p), ("add", C.c_void_p),
                ("add_stride", C.c_int), ("c_pad", C.c_int), ("count", C.c_longlong), ("eps", C.c_float),
                ("slope", C.c_float)]


_L.dua_prepare.restype = C.c_int
_L.dua_pack_conv3_weights.restype = C.c_long
_L.dua_pack_conv3_weights.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
_L.dua_conv3d_k3_fwd.restype = C.c_int
_L.dua_conv3d_k3_fwd.argtypes = [C.POINTER(Conv3Desc), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(InNorm),
                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_long, C.c_void_p]
DUA_F16 = 1
# mirror test-time augmentation of the streamed blend: dua_blend_accumulate[_weighted] with the un-flip of a window predicted
# under axis flips folded into the read of the window (flip: bit a set = spatial axis a reversed; the contract is in dua_hip.h)
_L.dua_blend_accumulate_mirrored.restype = C.c_int
_L.dua_blend_accumulate_mirrored.argtypes = ([C.c_int] * 6 + [C.c_void_p, C.c_void_p] + [C.c_int] * 4 + [C.c_void_p] +
                                             [C.c_int] * 4 + [C.c_void_p, C.c_void_p])
_L.dua_blend_accumulate_weighted_mirrored.restype = C.c_int
_L.dua_blend_accumulate_weighted_mirrored.argtypes = ([C.c_int] * 6 + [C.c_void_p, C.c_void_p] + [C.c_int] * 4 +
                                                      [C.c_void_p] * 3 + [C.c_float, C.c_void_p] + [C.c_int] * 4 +
                                                      [C.c_void_p, C.c_void_p])
# the uint8 label map on the grid of the scan straight from the sum volume of the streamed blend (corner logits, sigmoid,
# trilinear interpolation by per-axis tables, arg-max, optional tallies against the scan's label; the contract is in dua_hip.h)
_L.dua_blend_finish_labelmap.restype = C.c_int
_L.dua_blend_finish_labelmap.argtypes = ([C.c_void_p] + [C.c_int] * 4 + [C.c_void_p] * 4 + [C.c_int] * 9 + [C.c_void_p] * 6 +
                                         [C.c_int] * 3 + [C.c_float] + [C.c_void_p] * 4)

# random rotation and zoom in the device batch producer: dua_aug_draw_affine draws, beside the params rows of dua_aug_draw (the
# same bits), one affine row per sample; dua_aug_apply_affine resamples the patch through it (trilinear image, nearest label, the
# row's pad value outside the volume; centroids / smoothing None = one-hot labels).  The contract is in dua_hip.h
class AugConfig(C.Structure):                    # dua_aug_config
    _fields_ = [("roi", C.c_int * 3), ("max_k", C.c_int), ("pos_fraction", C.c_float), ("flip_prob", C.c_float),
                ("rot90_prob", C.c_float), ("scale_prob", C.c_float), ("scale_factors", C.c_float), ("shift_prob", C.c_float),
                ("shift_offsets", C.c_float), ("reserved", C.c_int)]


class AugAffineConfig(C.Structure):              # dua_aug_affine_config: tan(max angle / 2) per axis, fp32(zoom_max - zoom_min)
    _fields_ = [("rotate_prob", C.c_float), ("rotate_tan_half", C.c_float * 3), ("zoom_prob", C.c_float), ("zoom_min", C.c_float),
                ("zoom_span", C.c_float), ("pad_value", C.c_float), ("reserved", C.c_int)]


_L.dua_aug_draw_affine.restype = C.c_int
_L.dua_aug_draw_affine.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.POINTER(AugConfig), C.POINTER(AugAffineConfig),
                                   C.c_ulonglong, C.c_void_p, C.c_int, C.c_ulonglong, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
_L.dua_aug_apply_affine.restype = C.c_int
_L.dua_aug_apply_affine.argtypes = ([C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_int] * 4 +
                                    [C.c_void_p, C.c_int] + [C.c_void_p] * 4)
# class-balanced crop centres: dua_aug_count_class_candidates builds, once per volume, one prefix row per class;
# dua_aug_draw_classes is dua_aug_draw_affine (affine_cfg / affine may both be None) with the centre drawn from a class chosen by
# the volume's cum row, or, with probability uniform_prob, from the whole volume.  The contract is in dua_hip.h
class AugClassVolume(C.Structure):               # dua_aug_class_volume: device pointers to the class prefix table and to cum
    _fields_ = [("prefix", C.c_void_p), ("cum", C.c_void_p)]


_L.dua_aug_count_class_candidates.restype = C.c_int
_L.dua_aug_count_class_candidates.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_float, C.c_int, C.c_void_p, C.c_void_p]
_L.dua_aug_draw_classes.restype = C.c_int
_L.dua_aug_draw_classes.argtypes = ([C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.POINTER(AugConfig), C.POINTER(AugAffineConfig),
                                     C.c_ulonglong, C.c_void_p, C.c_int, C.c_ulonglong] + [C.c_void_p] * 4 +
                                    [C.c_int, C.c_float] + [C.c_void_p] * 3)

# gradient-norm clipping and an EMA of the weights in the AdamW launch: dua_grads_sumsq writes one fp64 partial per 4096-element
# chunk (dua_adamw_blocks of them per list), dua_grad_norm_finish turns them into the norm and clip_grad_norm_'s coefficient and
# raises the overflow flag, dua_adamw_step_ex is dua_adamw_step with that coefficient and  e += w (p - e),  w = (float)(1.0 - rate)
# formed in double.  Lists of <= 64 tensors go in by value.  The contract is in dua_hip.h
DUA_ADAMW_MAX_TENSORS, DUA_ADAMW_CHUNK = 64, 4096


class AdamWList(C.Structure):                    # dua_adamw_list: device pointers of parameters, gradients and the two moments
    _fields_ = [("count", C.c_int), ("numel", C.c_long * DUA_ADAMW_MAX_TENSORS)] + [(n, C.c_void_p * DUA_ADAMW_MAX_TENSORS)
                                                                                      for n in ("p", "g", "m", "v")]


class AdamWEma(C.Structure):                     # dua_adamw_ema: one EMA tensor per entry of the list
    _fields_ = [("e", C.c_void_p * DUA_ADAMW_MAX_TENSORS)]


_L.dua_adamw_blocks.restype = C.c_long
_L.dua_adamw_blocks.argtypes = [C.POINTER(AdamWList)]
_L.dua_grads_sumsq.restype = C.c_int
_L.dua_grads_sumsq.argtypes = [C.POINTER(AdamWList), C.c_void_p, C.c_void_p]
_L.dua_grad_norm_finish.restype = C.c_int
_L.dua_grad_norm_finish.argtypes = [C.c_void_p, C.c_long, C.c_void_p, C.c_float] + [C.c_void_p] * 4
_L.dua_adamw_step_ex.restype = C.c_int
_L.dua_adamw_step_ex.argtypes = ([C.POINTER(AdamWList), C.c_float, C.c_void_p] + [C.c_float] * 4 + [C.c_void_p] * 3 +
                                 [C.c_int, C.c_void_p, C.POINTER(AdamWEma), C.c_float, C.c_void_p])

# filling of enclosed holes after keep-largest: dua_fill_holes_mask is scipy.ndimage.binary_fill_holes per (sample, class)
# volume; dua_fill_holes_map fills a background component of a uint8 label map that touches no face and is bordered by one
# selectable class (class_mask: bit c = class c may fill) with that class.  Both write the filled voxel counts and, with a
# reference, the Dice tallies; the workspace comes from dua_fill_holes_scratch_bytes.  The contract is in dua_hip.h
_L.dua_fill_holes_scratch_bytes.restype = C.c_long
_L.dua_fill_holes_scratch_bytes.argtypes = [C.c_int] * 5
_L.dua_fill_holes_mask.restype = C.c_int
_L.dua_fill_holes_mask.argtypes = ([C.c_int] * 4 + [C.c_void_p, C.c_int, C.c_long, C.c_int] + [C.c_void_p] * 4 + [C.c_int] * 3 +
                                   [C.c_void_p, C.c_void_p, C.c_long, C.c_void_p])
_L.dua_fill_holes_map.restype = C.c_int
_L.dua_fill_holes_map.argtypes = ([C.c_int] * 4 + [C.c_void_p, C.c_long, C.c_int, C.c_int, C.c_ulonglong] + [C.c_void_p] * 5 +
                                  [C.c_long, C.c_void_p])


def _stream():
    return torch.cuda.current_stream().cuda_stream


def pack(conv):
    """nn.Conv3d(k3) parameters -> (packed fp16 weights, fp32 bias padded to a multiple of 64); once per weight update."""
    w = conv.weight.detach().float().contiguous()
    cout, cin = w.shape[:2]
    assert cin % 8 == 0 and cout % 8 == 0, "channel counts must be multiples of 8 (pad the buffers)"
    nbytes = _L.dua_pack_conv3_weights(DUA_F16, cout, cin, cin, None, None, None, None)
    buf = torch.empty(nbytes, dtype=torch.uint8, device=w.device)
    if _L.dua_pack_conv3_weights(DUA_F16, cout, cin, cin, w.data_ptr(), None, buf.data_ptr(), _stream()) != nbytes:
        raise RuntimeError("dua_pack_conv3_weights failed")
    bias = torch.zeros(-(-cout // 64) * 64, dtype=torch.float32, device=w.device)
    if conv.bias is not None:
        bias[:cout] = conv.bias.detach().float()
    return buf, bias


def new_stats(N, cout, device):
    """Zeroed InstanceNorm sums the convolution accumulates into: dua_stat_word [N][8][4][ceil(cout / 64) * 64]."""
    return torch.zeros((N, 8, 4, -(-cout // 64) * 64), dtype=torch.int64, device=device)


def producer(stats, norm, voxels, slope=0.1):
    """dua_in_norm of a raw convolution output: its sums + the nn.InstanceNorm3d(affine=True) that follows it."""
    return InNorm(stats.data_ptr(), norm.weight.data_ptr(), norm.bias.data_ptr(), None, 0, stats.shape[3], int(voxels),
                  float(norm.eps), float(slope))


def conv3(x_cl, w_packed, bias_pad, y_cl, stats, producer=None):
    """x_cl / y_cl: channels-last fp16 [N, D, H, W, C] CUDA tensors; y_cl receives the RAW output (conv + bias) and ``stats``
    its per-(n, c) sums.  ``producer``: InNorm of x_cl when x_cl is itself a raw output (its InstanceNorm + LeakyReLU are
    applied while the kernel stages its input).  Replaces Convolution.conv at denoiser.py:56-59."""
    N, D, H, W, Cin = x_cl.shape
    assert x_cl.is_cuda and x_cl.dtype == torch.float16 and x_cl.is_contiguous() and y_cl.is_contiguous()
    assert tuple(y_cl.shape[:4]) == (N, D, H, W) and Cin % 8 == 0 and y_cl.shape[-1] % 8 == 0
    d = Conv3Desc(DUA_F16, N, D, H, W, Cin, Cin, 0, y_cl.shape[-1], y_cl.shape[-1], 0, 0, 0, 0, 0)
    rc = _L.dua_conv3d_k3_fwd(C.byref(d), x_cl.data_ptr(), w_packed.data_ptr(), bias_pad.data_ptr(),
                              C.byref(producer) if producer is not None else None, y_cl.data_ptr(), stats.data_ptr(),
                              None, 0, _stream())
    if rc:
        raise RuntimeError(f"dua_conv3d_k3_fwd: {rc}")
    return y_cl
