"""Caller side of the sampler on full volumes: sliding-window scheduling, blending, binarisation,
Dice -- and the multi-GPU form of it (one process per GPU, windows sharded, one all-gather).

Reference call site: Engine.infer (engine.py:167-182) =
    monai.inferers.sliding_window_inference(image, (96,96,96), sw_batch_size, model, overlap,
                                            pred_type="ddim_sample") -> sigmoid -> > 0.5
MONAI is not vendored in the reference (nor installed here), so the window schedule below restates
MONAI's documented behaviour for the arguments the reference passes (mode="constant",
padding_mode="constant", cval=0): pad up to the roi, scan interval int(roi*(1-overlap)) (>=1; == roi
when the image is exactly one roi), window starts clamped to image-roi, windows enumerated with the first
spatial axis slowest, constant importance map, sum / count.  PARITY UNPINNED for this function (no
MONAI to run against); tests pin it against an independent loop-based restatement in the oracle.

Windows are independent units (each gets its own encoder pass and its own x_T,
models/diffusion/diffusion.py:88-100), so the multi-GPU form shards them with no data-path
collective until the end: rank r runs windows r, r+W, r+2W, ...; one all-gather (RCCL over xGMI on a
GPU node) of the per-window outputs; every rank then blends identically.

The streamed form (streamed_sliding_window_inference, evaluate_volume; csrc/blend.hip) keeps no list of window outputs: each
predictor call's outputs are added into a device-resident fp32 sum volume at once, the window count is derived from the plan
(the window grid is a dense product, so the count is a product of three per-axis vectors), one pass divides, crops,
binarises and tallies Dice, and the multi-GPU form all-reduces the per-rank sum volumes instead of gathering windows.

``mode="gaussian"`` (with ``sigma_scale``) on every function here is MONAI's second blending mode, restated from
``compute_importance_map`` (MONAI >= 1.1; PARITY UNPINNED like the rest): a window's outputs are multiplied by a Gaussian
importance map before they are added and the sum is divided by the summed maps.  ``importance_vectors`` is the single source of
the weights; the default ``mode="constant"`` takes the code above unchanged.

``mirror_axes`` on the single-process and the streamed functions is mirror test-time augmentation (nnU-Net's default inference;
the reference trains with independent flips of the three spatial axes, utils.py:154-156, and predicts each window once): every
window batch is predicted under every flip of the given axes, the outputs are un-flipped and all of them are averaged.  The
contract is written once in include/dua_hip.h; ``mirror_flips`` is its flip set.  The default ``mirror_axes=None`` takes the
code above unchanged.
"""
from __future__ import annotations

import itertools
import math
import numbers
from typing import Callable, Sequence

import torch
import torch.nn.functional as F

from . import postprocess as pp
from .postprocess import POSTPROCESS_KEYS, SEGMENT_POSTPROCESS_KEYS  # noqa: F401  (the stage dicts' keys, kept under this name)


def _scan_interval(image_size, roi_size, overlap):
    out = []
    for im, roi in zip(image_size, roi_size):
        if roi == im:
            out.append(int(roi))
        else:
            iv = int(roi * (1 - overlap))
            out.append(iv if iv > 0 else 1)
    return tuple(out)


def dense_window_starts(image_size: Sequence[int], roi_size: Sequence[int], scan_interval: Sequence[int]):
    """Per-axis window starts, then their product with the first axis slowest."""
    per_axis = []
    for im, roi, iv in zip(image_size, roi_size, scan_interval):
        if iv == 0:
            n = 1
        else:
            num = int(math.ceil(float(im) / iv))
            first = next((d for d in range(num) if d * iv + roi >= im), None)
            n = first + 1 if first is not None else 1
        per_axis.append([min(d * iv, im - roi) for d in range(n)])
    return list(itertools.product(*per_axis))


def _plan(inputs, roi_size, overlap):
    spatial = tuple(inputs.shape[2:])
    roi = tuple(int(r) for r in roi_size)
    assert len(roi) == len(spatial) == 3
    if not 0 <= overlap < 1:
        raise ValueError("overlap must be >= 0 and < 1.")
    padded = tuple(max(s, r) for s, r in zip(spatial, roi))
    pad = []
    for k in range(len(spatial) - 1, -1, -1):           # F.pad wants the last axis first
        diff = max(roi[k] - spatial[k], 0)
        half = diff // 2
        pad.extend([half, diff - half])
    starts = dense_window_starts(padded, roi, _scan_interval(padded, roi, overlap))
    return spatial, roi, padded, pad, starts


def coverage_counts(padded, roi, starts):
    """Per-axis window coverage of a plan: three lists, ``n_axis[i]`` = the number of starts ``s`` of that axis with
    ``s <= i < s + roi``.  ``starts`` is the dense product ``_plan`` returns, so the number of windows over voxel (z, y, x) --
    the count map ``_blend`` accumulates -- is ``n_d[z] * n_h[y] * n_w[x]``."""
    per_axis = [sorted({s[k] for s in starts}) for k in range(3)]
    assert len(per_axis[0]) * len(per_axis[1]) * len(per_axis[2]) == len(starts), "window starts are not a dense product"
    out = []
    for k in range(3):
        n = [0] * int(padded[k])
        for s in per_axis[k]:
            for i in range(s, s + int(roi[k])):
                n[i] += 1
        out.append(n)
    return out


BLEND_MODES = ("constant", "gaussian")


def _sigma_scales(sigma_scale):
    scales = tuple(float(v) for v in sigma_scale) if isinstance(sigma_scale, (tuple, list)) else (float(sigma_scale),) * 3
    if len(scales) != 3 or not all(0.0 < v < math.inf for v in scales):
        raise ValueError(f"sigma_scale must be a positive number, or three of them, not {sigma_scale!r}")
    return scales


def importance_vectors(roi, mode="constant", sigma_scale=0.125):
    """The importance map of ``mode`` as (g0, g1, g2, floor): fp32 CPU vectors [r0], [r1], [r2] and a float, the map being
    ``w[z, y, x] = max((g0[z] * g1[y]) * g2[x], floor)`` with every product rounded to fp32 in this order (the outer-product
    order of MONAI's compute_importance_map).  "gaussian": ``g_k = exp(x**2 / (-2 * sigma_k**2))`` in fp32 with
    ``x = arange(-(r_k-1)/2, (r_k-1)/2 + 1)`` and ``sigma_k = r_k * sigma_scale_k``; ``floor = max(min(map), 1e-3)`` as an fp32
    value (MONAI's ``clamp_(min=...)``).  "constant": ones and floor 1.  Every path takes its weights from here."""
    if mode not in BLEND_MODES:
        raise ValueError(f"mode must be one of {BLEND_MODES}, not {mode!r}")
    scales = _sigma_scales(sigma_scale)
    roi = tuple(int(r) for r in roi)
    assert len(roi) == 3 and all(r >= 1 for r in roi)
    if mode == "constant":
        return (*(torch.ones(r, dtype=torch.float32) for r in roi), 1.0)
    vectors = []
    for r, scale in zip(roi, scales):
        sigma = r * scale
        x = torch.arange(start=-(r - 1) / 2.0, end=(r - 1) / 2.0 + 1, dtype=torch.float32)
        vectors.append(torch.exp(x ** 2 / (-2 * sigma ** 2)))
    g0, g1, g2 = vectors
    # a rounded product of positive numbers is monotonic in each factor, so the smallest element of the map is the product
    # of the three smallest elements taken in the map's own order
    lowest = float((g0.min() * g1.min()) * g2.min())
    floor = float(torch.tensor(max(lowest, 1e-3), dtype=torch.float32))
    return g0, g1, g2, floor


def importance_map(vectors, device=None, dtype=torch.float32):
    """[r0, r1, r2] map of ``importance_vectors``' result, built in fp32 on the CPU, then moved."""
    g0, g1, g2, floor = vectors
    m = ((g0[:, None, None] * g1[None, :, None]) * g2[None, None, :]).clamp_(min=floor)
    return m.to(device=device, dtype=dtype)


def axis_starts(starts):
    """The three ascending per-axis start lists whose product, first axis slowest, is the plan's ``starts``."""
    per_axis = [sorted({s[k] for s in starts}) for k in range(3)]
    assert list(itertools.product(*per_axis)) == list(starts), "window starts are not a dense product in D-major order"
    return per_axis


def window_table(starts, batch, device=None):
    """The plan as the int32 table dua_blend_accumulate reads: row ``idx`` = (b, d, h, w) of window ``idx`` = b * len(starts) + k,
    i.e. ``len(starts) * batch`` rows in window-index order.  Built once per plan (on ``device`` when given)."""
    rows = [(b, d, h, w) for b in range(int(batch)) for (d, h, w) in starts]
    t = torch.tensor(rows, dtype=torch.int32).view(-1, 4)
    return t if device is None else t.to(device)


def blend_traffic_bytes(windows_total, channels, roi, batch, padded, world, window_itemsize=4):
    """Derived (not measured) bytes every rank receives in the two multi-GPU forms: ``gathered`` = the flat tensor
    all_gather_into_tensor fills, world * ceil(windows / world) window outputs of ``window_itemsize`` bytes per element;
    ``reduced`` = the fp32 sum volume one all_reduce combines."""
    per_rank = -(-int(windows_total) // int(world))
    window = int(channels) * int(roi[0]) * int(roi[1]) * int(roi[2]) * int(window_itemsize)
    volume = int(batch) * int(channels) * int(padded[0]) * int(padded[1]) * int(padded[2]) * 4
    return {"gathered": int(world) * per_rank * window, "reduced": volume}


def mirror_flips(mirror_axes):
    """The flip set of mirror test-time augmentation: every subset of ``mirror_axes`` (distinct spatial axes from {0, 1, 2} =
    D, H, W of [B, C, D, H, W], in any order; None or () = no augmentation) as a 3-bit mask, bit a set = axis a reversed, in
    ascending order -- so the identity, mask 0, comes first: ``(2, 0)`` -> ``(0, 1, 4, 5)``, ``None`` -> ``(0,)``.
    ValueError on an axis outside {0, 1, 2}, a duplicate or a non-integer."""
    bits = 0
    for a in () if mirror_axes is None else tuple(mirror_axes):
        if isinstance(a, bool) or not isinstance(a, numbers.Integral) or a not in (0, 1, 2) or bits >> int(a) & 1:
            raise ValueError(f"mirror_axes: distinct spatial axes from (0, 1, 2), not {mirror_axes!r}")
        bits |= 1 << int(a)
    return tuple(f for f in range(8) if f & ~bits == 0)


def _flip_dims(flip):
    """The dims of ``torch.flip`` on a [b, C, D, H, W] tensor for a flip mask."""
    return [2 + a for a in range(3) if flip >> a & 1]


def _blend(outputs_by_index, batch, channels, padded, roi, starts, pad, spatial, device, dtype, weights=None, flips=1):
    """``weights``: None = the constant map (sum / count); else the importance map [*roi] on ``device``: every window is
    multiplied by it (one rounded product), added, and the sum is divided by the map summed once per window position.
    ``flips`` = F: every window index comes F times (its un-flipped outputs under the F flips of ``mirror_flips``); the count,
    or the map, is added for the first of them only and the divisor is F times it (a power of two: exact)."""
    out = torch.zeros((batch, channels, *padded), dtype=dtype, device=device)
    cnt = torch.zeros((1, 1, *padded), dtype=dtype, device=device)
    nwin = len(starts)
    counted = set()
    for idx, o in outputs_by_index:
        b, (d, h, w) = idx // nwin, starts[idx % nwin]
        first = idx not in counted
        counted.add(idx)
        if weights is not None:
            out[b:b + 1, :, d:d + roi[0], h:h + roi[1], w:w + roi[2]] += weights * o
            if b == 0 and first:
                cnt[:, :, d:d + roi[0], h:h + roi[1], w:w + roi[2]] += weights
            continue
        out[b:b + 1, :, d:d + roi[0], h:h + roi[1], w:w + roi[2]] += o
        if b == 0 and first:
            cnt[:, :, d:d + roi[0], h:h + roi[1], w:w + roi[2]] += 1
    out = out / cnt if flips == 1 else out / (cnt * flips)
    sl = [slice(None), slice(None)]
    for k in range(3):                                   # crop the padding away again
        lo = pad[2 * (2 - k)]
        sl.append(slice(lo, lo + spatial[k]))
    return out[tuple(sl)]


def _blend_weights(roi, mode, sigma_scale, device, dtype):
    """The ``weights`` argument of ``_blend`` for ``mode``; validates ``mode`` and ``sigma_scale`` either way."""
    vectors = importance_vectors(roi, mode, sigma_scale)
    return None if mode == "constant" else importance_map(vectors, device, dtype)


def _window(inputs, idx, nwin, starts, roi):
    b, (d, h, w) = idx // nwin, starts[idx % nwin]
    return inputs[b:b + 1, :, d:d + roi[0], h:h + roi[1], w:w + roi[2]]


def sliding_window_inference(inputs: torch.Tensor, roi_size, sw_batch_size: int, predictor: Callable, overlap: float = 0.25,
                             mirror_axes=None, mode: str = "constant", sigma_scale=0.125, **kwargs) -> torch.Tensor:
    """Single-process form (engine.py:173-177 semantics).  ``predictor(window_batch, **kwargs)`` -> [b,C,*roi].
    ``mode``: "constant" (the reference's) or "gaussian" with ``sigma_scale`` (``importance_vectors``).
    A model built with ``uncer_step=R`` is a predictor like any other here and in the sharded and streamed forms: the switch
    lives on the model, every window batch of b comes back as [b, C, *roi] (the Step-Uncertainty Fusion of its R runs).
    ``mirror_axes``: None, or the spatial axes (0 = D, 1 = H, 2 = W) of mirror test-time augmentation: each window batch is
    gathered once and predicted under every flip of ``mirror_flips(mirror_axes)`` in order, ``flip(predictor(flip(windows, f)),
    f)``, every un-flipped output is blended as a window output of its own and the divisor is F = 2^k times the unmirrored one.
    Step-Uncertainty Fusion composes without change (it lives in the predictor: F R DDIM loops per window)."""
    spatial, roi, padded, pad, starts = _plan(inputs, roi_size, overlap)
    importance_vectors(roi, mode, sigma_scale)              # refuse a bad mode or sigma_scale before any predictor call
    flips = mirror_flips(mirror_axes)
    x = F.pad(inputs, pad=pad, mode="constant", value=0.0)
    nwin, total = len(starts), len(starts) * inputs.shape[0]
    results = []
    for g in range(0, total, sw_batch_size):
        idxs = list(range(g, min(g + sw_batch_size, total)))
        windows = torch.cat([_window(x, i, nwin, starts, roi) for i in idxs])
        for f in flips:
            seg = predictor(windows, **kwargs) if f == 0 else \
                torch.flip(predictor(torch.flip(windows, _flip_dims(f)), **kwargs), _flip_dims(f))
            results += [(i, seg[k:k + 1]) for k, i in enumerate(idxs)]
    first = results[0][1]
    return _blend(results, inputs.shape[0], first.shape[1], padded, roi, starts, pad, spatial, first.device, first.dtype,
                  _blend_weights(roi, mode, sigma_scale, first.device, first.dtype), len(flips))


def balanced_batches(n: int, max_batch: int):
    """Sizes of the predictor calls for ``n`` windows of one rank: as few calls as ``max_batch`` allows, of (nearly) equal size.
    Cutting [0, n) into slices of ``max_batch`` leaves a tail call that can be a single window (BASELINE config 3 on 8 GPUs:
    6 windows per rank at sw_batch_size 4 -> 4 + 2, and the 2-window pass runs the coarse levels of the network at half the
    fill); 3 + 3 takes the same number of passes and no call is smaller than half of ``max_batch``."""
    if n <= 0:
        return []
    calls = -(-n // max(1, int(max_batch)))
    base, extra = divmod(n, calls)
    return [base + 1] * extra + [base] * (calls - extra)


def sharded_sliding_window_inference(inputs: torch.Tensor, roi_size, sw_batch_size: int, predictor: Callable,
                                     overlap: float = 0.25, group=None, gather_dtype: torch.dtype = None,
                                     timings: dict = None, mode: str = "constant", sigma_scale=0.125, **kwargs) -> torch.Tensor:
    """One process per GPU: windows dealt round-robin over the ranks of ``group``, one all-gather of the
    per-window outputs (fp32, or ``gather_dtype`` to halve the xGMI bytes), identical blend on every rank.
    ``inputs`` must be the same on all ranks.  ``timings`` (optional dict): accumulates the wall time of the
    collective under "all_gather_s" (device synchronised around it) and records "gathered_bytes".  ``mode``,
    ``sigma_scale``: as ``sliding_window_inference``."""
    import torch.distributed as dist
    world, rank = dist.get_world_size(group), dist.get_rank(group)
    spatial, roi, padded, pad, starts = _plan(inputs, roi_size, overlap)
    importance_vectors(roi, mode, sigma_scale)
    x = F.pad(inputs, pad=pad, mode="constant", value=0.0)
    nwin, total = len(starts), len(starts) * inputs.shape[0]
    mine = list(range(rank, total, world))
    per_rank = -(-total // world)
    local = None
    g = 0
    for nb in balanced_batches(len(mine), sw_batch_size):
        idxs = mine[g:g + nb]
        seg = predictor(torch.cat([_window(x, i, nwin, starts, roi) for i in idxs]), **kwargs)
        if local is None:
            gd = gather_dtype or seg.dtype
            local = torch.zeros((per_rank, *seg.shape[1:]), dtype=gd, device=seg.device)
        local[g:g + len(idxs)] = seg.to(local.dtype)
        g += nb
    if local is None:        # more ranks than windows: still take part in the collective
        probe = predictor(_window(x, 0, nwin, starts, roi), **kwargs)
        local = torch.zeros((per_rank, *probe.shape[1:]), dtype=gather_dtype or probe.dtype, device=probe.device)
    flat = torch.empty((world * per_rank, *local.shape[1:]), dtype=local.dtype, device=local.device)
    if timings is not None:
        import time
        if local.is_cuda:
            torch.cuda.synchronize(local.device)
        t0 = time.perf_counter()
    dist.all_gather_into_tensor(flat, local, group=group)
    if timings is not None:
        if local.is_cuda:
            torch.cuda.synchronize(local.device)
        timings["all_gather_s"] = timings.get("all_gather_s", 0.0) + time.perf_counter() - t0
        timings["gathered_bytes"] = flat.numel() * flat.element_size()
    gathered = flat.view(world, per_rank, *local.shape[1:])
    results = []
    for r in range(world):
        for k, i in enumerate(range(r, total, world)):
            results.append((i, gathered[r, k:k + 1].float()))
    results.sort(key=lambda t: t[0])
    return _blend(results, inputs.shape[0], local.shape[1], padded, roi, starts, pad, spatial, local.device, torch.float32,
                  _blend_weights(roi, mode, sigma_scale, local.device, torch.float32))


def _need_device(t, what):
    if not t.is_cuda:
        raise RuntimeError(f"{what} runs on an MI355X (device 'cuda'); there is no CPU path in this package")


def _streamed_sum(inputs, roi_size, sw_batch_size, predictor, overlap, group, gather_dtype, timings, kwargs, mode="constant",
                  sigma_scale=0.125, mirror_axes=None):
    """The sum volume fp32 [B, C, *padded] of this plan (all-reduced over ``group`` when given) and what the finish pass needs:
    (sum volume, divisor, crop offsets, spatial).  The divisor is the three coverage vectors on the device, or with
    ``mode="gaussian"`` the weight-sum volume fp32 [*padded], which every rank derives from the plan for itself.  With
    ``mirror_axes`` every call's window batch is predicted under the F flips of ``mirror_flips`` and each raw output goes to
    ``ops.blend_accumulate`` with its flip mask, which un-flips it while reading; the divisor returned is F times the unmirrored one."""
    from . import ops
    spatial, roi, padded, pad, starts = _plan(inputs, roi_size, overlap)
    flips = mirror_flips(mirror_axes)
    weights = None
    vectors = importance_vectors(roi, mode, sigma_scale)
    if mode != "constant":
        weights = (*(g.to(inputs.device) for g in vectors[:3]), vectors[3])
    world, rank = 1, 0
    if group is not None:
        import torch.distributed as dist
        world, rank = dist.get_world_size(group), dist.get_rank(group)
    dev = inputs.device
    x = F.pad(inputs, pad=pad, mode="constant", value=0.0) if any(pad) else inputs      # no copy of a volume that needs none
    batch = inputs.shape[0]
    nwin, total = len(starts), len(starts) * batch
    table = window_table(starts, batch, dev)
    err = ops.zeros((1,), torch.int32, dev)
    mine = list(range(rank, total, world))
    # one process: the calls of sliding_window_inference; ranks of a group: those of sharded_sliding_window_inference
    sizes = [min(sw_batch_size, total - g) for g in range(0, total, sw_batch_size)] if group is None else \
        balanced_batches(len(mine), sw_batch_size)
    acc = None
    g = 0
    for nb in sizes:
        idxs = mine[g:g + nb]
        windows = torch.cat([_window(x, i, nwin, starts, roi) for i in idxs])
        for f in flips:
            seg = predictor(windows if f == 0 else torch.flip(windows, _flip_dims(f)), **kwargs)
            if acc is None:
                acc = ops.zeros((batch, seg.shape[1], *padded), torch.float32, dev)
            if gather_dtype is not None:
                seg = seg.to(gather_dtype)
            ops.blend_accumulate(acc, seg.contiguous(), table, idxs[0], world, err, weights=weights, flip=f)
            del seg
        g += nb
        del windows
    if acc is None:          # more ranks than windows: still take part in the collective
        probe = predictor(_window(x, 0, nwin, starts, roi), **kwargs)
        acc = ops.zeros((batch, probe.shape[1], *padded), torch.float32, dev)
    if group is not None:
        import torch.distributed as dist
        if timings is not None:
            import time
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
        dist.all_reduce(acc, group=group)
        if timings is not None:
            torch.cuda.synchronize(dev)
            timings["all_reduce_s"] = timings.get("all_reduce_s", 0.0) + time.perf_counter() - t0
            timings["reduced_bytes"] = acc.numel() * acc.element_size()
    if int(err.item()):
        raise RuntimeError("streamed blend: a window position of the plan lies outside the padded volume")
    crop_lo = tuple(pad[2 * (2 - k)] for k in range(3))
    if weights is not None:
        per_axis = [torch.tensor(s, dtype=torch.int32).to(dev) for s in axis_starts(starts)]
        wsum = ops.blend_weight_sum(per_axis, roi, padded, weights)
        return acc, wsum if len(flips) == 1 else wsum.mul_(len(flips)), crop_lo, spatial
    counts = coverage_counts(padded, roi, starts)
    counts[0] = [n * len(flips) for n in counts[0]]            # F nd[z] nh[y] nw[x]: the finish pass needs no change
    coverage = [torch.tensor(n, dtype=torch.int32).to(dev) for n in counts]
    return acc, coverage, crop_lo, spatial


def streamed_sliding_window_inference(inputs: torch.Tensor, roi_size, sw_batch_size: int, predictor: Callable,
                                      overlap: float = 0.25, group=None, gather_dtype: torch.dtype = None,
                                      timings: dict = None, mirror_axes=None, mode: str = "constant", sigma_scale=0.125,
                                      **kwargs) -> torch.Tensor:
    """The volume ``sliding_window_inference`` returns -- same plan, padding, window order and predictor calls -- without the list
    of window outputs: every call's outputs are added into a device-resident fp32 sum volume at once (dua_blend_accumulate:
    the fp32 additions of ``_blend`` in the same order), and one pass divides by the window count derived from the plan and
    crops (dua_blend_finish).  ``group=None``: one process.  With a group, each rank adds its round-robin windows (dealt in
    ``balanced_batches`` calls, as ``sharded_sliding_window_inference`` does) into its own sum volume and ONE all_reduce of the
    fp32 volumes follows; ``timings`` accumulates its wall time under "all_reduce_s" and records "reduced_bytes";
    ``gather_dtype`` only narrows the window tensor handed to the accumulate call.  ``mode="gaussian"``: the weighted entry
    points (dua_blend_accumulate_weighted, dua_blend_weight_sum, dua_blend_finish_weighted), bit-equal to
    ``sliding_window_inference(mode="gaussian")`` on the same device; the all-reduce is the same.  ``mirror_axes``: as
    ``sliding_window_inference``, bit-equal to it on the same device in both modes; the raw output of each flipped call goes
    to dua_blend_accumulate_mirrored (or its weighted form), which un-flips it while reading -- no flipped copy of a window
    output -- and the divisor is scaled by F.  With a group each rank runs the F flips of its own windows into its own sum
    volume: the all-reduced bytes are unchanged.  Device tensors only."""
    from . import ops
    _need_device(inputs, "streamed_sliding_window_inference")
    acc, divisor, crop_lo, spatial = _streamed_sum(inputs, roi_size, sw_batch_size, predictor, overlap, group, gather_dtype,
                                                   timings, kwargs, mode, sigma_scale, mirror_axes)
    return ops.blend_finish(acc, divisor, crop_lo, spatial, want_q=True)[0]


def evaluate_volume(model, image: torch.Tensor, labels: torch.Tensor = None, roi_size=(96, 96, 96), sw_batch_size: int = 1,
                    overlap: float = 0.25, distributed: bool = False, group=None, postprocess: dict = None,
                    surface: dict = None, mirror_axes=None, fill_holes: dict = None, mode: str = "constant", sigma_scale=0.125):
    """Engine.infer (engine.py:167-182) and the Dice of the result (metric.py:37-49) in the streamed form: (mask uint8
    [B, C, D, H, W] = sigmoid(blend) > 0.5, dice fp64 [C] or None without ``labels``).  The normalised fp32 volume is never
    written: one pass over the sum volume divides, crops, binarises and counts.  ``labels``: one-hot [B, C, D, H, W] (non-zero =
    set) or a uint8 label map [B, D, H, W] (class c = channel c).  ``distributed``: shard the windows over the ranks of
    ``group`` (default: the world) and all-reduce the sum volumes.  ``mode``, ``sigma_scale``: as ``sliding_window_inference``.
    ``postprocess``: None, or a dict of ``postprocess.keep_largest_components`` keyword arguments (connectivity,
    num_components, min_size, channels, cap): the finish pass then writes the mask only, the component filter runs on it and
    tallies Dice in its own pass, and the result is (filtered mask, Dice of the filtered mask).
    A ``model`` built with ``uncer_step=R`` needs no argument here: each predictor call then runs R DDIM loops per window and
    returns their Step-Uncertainty Fusion (a plan of sw_batch_size R rows).
    ``surface``: None, or a dict with keys among ("tolerance", "voxel_spacing", "connectivity", "nan_for_nonexisting",
    "distances"); it needs ``labels``.  The result is then (mask, dice, report): ``metrics.surface_dice_table`` (Normalized
    Surface Dice at ``tolerance``) of the returned mask -- the filtered one with ``postprocess`` -- against the labels, or
    ``metrics.surface_report`` (the distance table too) with ``distances=True``.
    ``mirror_axes``: mirror test-time augmentation as in ``streamed_sliding_window_inference`` (F predictor calls per window
    batch, the same all-reduce).  ``postprocess``, ``surface`` and Step-Uncertainty Fusion compose with it without change:
    they run after the finish pass, or inside the predictor.
    ``fill_holes``: None, or a dict with keys among ("connectivity", "channels"): ``postprocess.fill_holes`` on the mask, AFTER
    ``postprocess`` when both are given (keep-largest first, then fill).  The mask, the Dice and the ``surface`` report are then
    those of the filled mask, the Dice from the fill pass's tallies.  None changes no launch of the paths above."""
    from . import ops
    mirror_flips(mirror_axes)                              # refuse bad axes before any predictor call
    if surface is not None:
        _surface_kwargs(surface, labels)
    if fill_holes is not None:
        pp.check_stage_kwargs("fill_holes", "mask", fill_holes)
    _need_device(image, "evaluate_volume")
    if postprocess is not None:
        pp.check_stage_kwargs("postprocess", "mask", postprocess)
    if distributed and group is None:
        import torch.distributed as dist
        group = dist.group.WORLD
    with torch.no_grad():
        acc, divisor, crop_lo, spatial = _streamed_sum(image, roi_size, sw_batch_size, model, overlap, group if distributed else None,
                                                       None, None, dict(pred_type="ddim_sample"), mode, sigma_scale, mirror_axes)
        mask, tallies = _run_stages(lambda ref: ops.blend_finish(acc, divisor, crop_lo, spatial, want_mask=True, labels=ref)[1:],
                                    _stages(postprocess, fill_holes, pp.filter_components, pp.fill_holes, "labels"), labels)
    dice = ops.dice_from_tallies(tallies) if tallies is not None else None
    if surface is None:
        return mask, dice
    from . import metrics
    kw = dict(surface)
    fn = metrics.surface_report if kw.pop("distances", False) else metrics.surface_dice_table
    return mask, dice, fn(mask, _one_hot_labels(labels, mask.shape[1]), kw.pop("tolerance"), **kw)


def segment_case(model, case, label: torch.Tensor = None, roi_size=(96, 96, 96), sw_batch_size: int = 1, overlap: float = 0.25,
                 distributed: bool = False, group=None, mirror_axes=None, mode: str = "constant", sigma_scale=0.125,
                 min_prob: float = 0.0, postprocess: dict = None, surface: dict = None, fill_holes: dict = None):
    """The deliverable of one case: (label map uint8 on the grid of the SCAN, Dice fp64 [C] against ``label`` or None).  ``case``:
    a ``prepare.PreparedCase`` -- the streamed blend runs on ``case.image[None, None]`` and one pass
    (dua_blend_finish_labelmap) turns the sum volume into the label map: per voxel of the scan the class probabilities
    sigmoid(blend) of the 8 surrounding prepared voxels, interpolated linearly, the lowest class with the largest one, 0 below
    ``min_prob`` and outside the foreground box.  No [C, *scan] tensor is written.  ``case`` may be a plain device tensor
    [1, 1, D, H, W] instead: it is its own grid (identity tables, every weight 0), and the result is the arg-max of
    sigmoid(blend) on it.  ``label``: the raw uint8 label map of the scan, [*scan] on the case's device; class c = channel c, a
    value >= C counts nowhere.  The other arguments as ``evaluate_volume``.  Argument errors are raised before any predictor
    call.

    ``postprocess``: None, or a dict of ``postprocess.filter_label_map`` keywords (SEGMENT_POSTPROCESS_KEYS): the label map is
    filtered as it is, on the scan's grid (one union-find for all classes, no one-hot tensor); the map returned is the filtered
    one and the Dice is that of the filtered map, from the filter pass's tallies.  ``surface``: None, or a dict with a
    ``tolerance`` and optionally ``connectivity``, ``nan_for_nonexisting``, ``classes`` (default 1 .. C - 1) and
    ``voxel_spacing`` (default ``case.source_spacing``, the scan's own spacing, or 1 for a plain tensor); it needs ``label``, and
    the result is then (map, dice, report) with report = ``metrics.label_map_surface_report`` of the returned map against
    ``label`` (one host read of the box table).  With neither, nothing new is launched.

    ``fill_holes``: None, or a dict with keys among ("connectivity", "classes"): ``postprocess.fill_holes_in_label_map`` on the
    label map, on the scan's grid, AFTER ``postprocess`` when both are given (keep-largest first, then fill).  The map, the Dice
    and the ``surface`` report are then those of the filled map, the Dice from the fill pass's tallies.  None changes no launch
    of the paths above."""
    from . import ops
    from .prepare import PreparedCase
    mirror_flips(mirror_axes)
    if postprocess is not None:
        pp.check_stage_kwargs("postprocess", "map", postprocess)
    if fill_holes is not None:
        pp.check_stage_kwargs("fill_holes", "map", fill_holes)
    if surface is not None:
        _segment_surface_kwargs(surface, label)
    min_prob = float(min_prob)
    if not 0.0 <= min_prob <= 1.0:                       # NaN fails both comparisons
        raise ValueError(f"segment_case: min_prob lies in [0, 1], got {min_prob}")
    if isinstance(case, PreparedCase):
        image, source_shape = case.image, tuple(case.source_shape)
        if not torch.is_tensor(image) or image.dim() != 3 or image.dtype != torch.float32:
            raise ValueError("segment_case: case.image is an fp32 tensor [D, H, W]")
        image = image[None, None]
    elif torch.is_tensor(case):
        if case.dim() != 5 or case.shape[0] != 1 or case.shape[1] != 1:
            raise ValueError(f"segment_case: a plain volume is [1, 1, D, H, W] (one case per call), got {tuple(case.shape)}")
        if case.dtype != torch.float32:
            raise ValueError(f"segment_case: a plain volume is float32, got {case.dtype}")
        image, source_shape = case, tuple(case.shape[2:])
    else:
        raise ValueError("segment_case: case is a PreparedCase or a device tensor [1, 1, D, H, W]")
    if label is not None:
        if not torch.is_tensor(label) or label.dtype != torch.uint8:
            raise ValueError("segment_case: label is a uint8 tensor, the raw label map of the scan")
        if tuple(label.shape) != source_shape:
            raise ValueError(f"segment_case: label has the shape of the scan {source_shape}, got {tuple(label.shape)}")
    _need_device(image, "segment_case")
    if label is not None:
        if label.device != image.device:
            raise ValueError(f"segment_case: label is on {label.device}, the case on {image.device}")
    if distributed and group is None:
        import torch.distributed as dist
        group = dist.group.WORLD
    if isinstance(case, PreparedCase):
        tables = case.linear_tables()
    else:
        D, H, W = source_shape
        steps = (H * W, W, 1)
        tables = (tuple(torch.arange(n, dtype=torch.int32, device=image.device) * s for n, s in zip(source_shape, steps)),
                  tuple(torch.zeros(n, dtype=torch.float32, device=image.device) for n in source_shape), (0, 1, 2))
    with torch.no_grad():
        acc, divisor, crop_lo, spatial = _streamed_sum(image, roi_size, sw_batch_size, model, overlap, group if distributed else None,
                                                       None, None, dict(pred_type="ddim_sample"), mode, sigma_scale, mirror_axes)
        out, tallies = _run_stages(
            lambda ref: ops.blend_finish_labelmap(acc, divisor, crop_lo, spatial, tables, source_shape, min_prob,
                                                  None if ref is None else ref.contiguous()),
            _stages(postprocess, fill_holes, pp.filter_label_map, pp.fill_holes_in_label_map, "reference", int(acc.shape[-4])), label)
    dice = ops.dice_from_tallies(tallies) if tallies is not None else None
    if surface is None:
        return out, dice
    from . import metrics
    kw = dict(surface)
    classes = kw.pop("classes", None)
    if classes is None:
        classes = range(1, int(acc.shape[-4]))
    if kw.get("voxel_spacing") is None:
        kw["voxel_spacing"] = case.source_spacing if isinstance(case, PreparedCase) else None
    return out, dice, metrics.label_map_surface_report(out, label, classes, kw.pop("tolerance"), **kw)


def _run_stages(first, stages, reference):
    """The chain behind ``postprocess=`` and ``fill_holes=``: ``first(ref)``, then every ``stage(result, ref)`` in order, each
    returning (result, tallies or None).  The LAST call that runs gets ``reference`` and so produces the tallies; every call
    before it gets None and tallies nothing.  Returns (the last result, its tallies).  Without stages this is ``first(reference)``
    and nothing else."""
    result, tallies = first(reference if not stages else None)
    for i, stage in enumerate(stages):
        result, tallies = stage(result, reference if i == len(stages) - 1 else None)
    return result, tallies


def _stages(postprocess, fill_holes, filter_fn, fill_fn, reference_key, *args):
    """The stages of ``_run_stages`` for the two dicts, each present when its dict is: ``filter_fn(result, *args, **postprocess)``,
    then ``fill_fn(result, *args, **fill_holes)`` (keep-largest first, then fill).  ``reference_key``: the keyword under which
    the two functions take the reference."""
    stages = []
    if postprocess is not None:
        stages.append(lambda result, ref: filter_fn(result, *args, **{reference_key: ref}, **postprocess))
    if fill_holes is not None:
        def fill(result, ref):
            out, _, *tallies = fill_fn(result, *args, **{reference_key: ref}, **fill_holes)
            return out, tallies[0] if tallies else None
        stages.append(fill)
    return stages


SEGMENT_SURFACE_KEYS = ("tolerance", "voxel_spacing", "connectivity", "nan_for_nonexisting", "classes")


def _segment_surface_kwargs(surface, label):
    """Refuse a ``surface`` argument of ``segment_case`` that is not a dict of SEGMENT_SURFACE_KEYS with a tolerance, or that
    comes without a label, before any predictor call."""
    if not isinstance(surface, dict) or any(k not in SEGMENT_SURFACE_KEYS for k in surface) or "tolerance" not in surface:
        raise ValueError(f"surface: None or a dict with a 'tolerance' and keys among {SEGMENT_SURFACE_KEYS}, got {surface!r}")
    if label is None:
        raise ValueError("surface: the surface metrics compare the label map with label; label is None")
    if surface.get("connectivity", 1) not in (1, 2, 3) or isinstance(surface.get("connectivity", 1), bool):
        raise ValueError(f"surface: connectivity must be 1, 2 or 3, got {surface.get('connectivity')!r}")
    from . import _native as nv
    from . import metrics, ops
    classes = surface.get("classes")
    if classes is not None:
        if isinstance(classes, (str, bytes)) or not hasattr(classes, "__iter__"):
            raise ValueError(f"surface: classes is None or a non-empty sequence of class ids, got {classes!r}")
        classes = list(classes)
        if not classes or any(isinstance(c, bool) or not isinstance(c, int) or not 0 <= c < nv.BLEND_MAX_CLASSES for c in classes):
            raise ValueError(f"surface: classes is None or a non-empty sequence of integers in 0..{nv.BLEND_MAX_CLASSES - 1}, got "
                             f"{classes!r}")
    # the tolerance against the classes when they are given; against its own length otherwise (the default classes are
    # 1 .. C - 1, known only once the predictor has run: values, T and the table's limits are still checked here)
    tolerance = surface["tolerance"]
    if hasattr(tolerance, "tolist"):
        tolerance = tolerance.tolist()
    try:
        if classes is not None:
            metrics._tolerance_rows(tolerance, len(classes))
        elif isinstance(tolerance, (int, float)) and not isinstance(tolerance, bool):
            metrics._tolerance_rows(tolerance, 1)
        else:
            metrics._tolerance_rows(tolerance, len(list(tolerance)))
        spacing = ops._spacing3(surface.get("voxel_spacing"))
    except TypeError as e:
        raise ValueError(f"surface: {e}") from None
    except ValueError as e:
        raise ValueError(e.args[0] if str(e).startswith(("tolerance", "voxel_spacing")) else
                         f"surface: tolerance and voxel_spacing hold numbers ({e})") from None
    if not all(0.0 < x < float("inf") for x in spacing):
        raise ValueError(f"surface: voxel_spacing must be finite and > 0, got {surface.get('voxel_spacing')!r}")


SURFACE_KEYS = ("tolerance", "voxel_spacing", "connectivity", "nan_for_nonexisting", "distances")


def _surface_kwargs(surface, labels):
    """Refuse a ``surface`` argument that is not a dict of these keys with a tolerance, or that comes without labels, before any
    predictor call."""
    if not isinstance(surface, dict) or any(k not in SURFACE_KEYS for k in surface) or "tolerance" not in surface:
        raise ValueError(f"surface: None or a dict with a 'tolerance' and keys among {SURFACE_KEYS}, got {surface!r}")
    if labels is None:
        raise ValueError("surface: the surface metrics compare the mask with labels; labels is None")


def _one_hot_labels(labels, channels):
    """``evaluate_volume``'s labels as a [B, C, D, H, W] mask: a one-hot tensor as it is, a uint8 label map [B, D, H, W]
    expanded (class c = channel c)."""
    if labels.dim() == 4:
        classes = torch.arange(channels, device=labels.device, dtype=labels.dtype).view(1, channels, 1, 1, 1)
        return labels[:, None] == classes
    return labels


def binarise(outputs: torch.Tensor) -> torch.Tensor:
    """engine.py:179-180."""
    return (torch.sigmoid(outputs) > 0.5).float()


def dice_per_class(outputs: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
    """metric.py:37-49 for every class at once, on the device, one host sync for the whole vector
    (the reference calls .item() three times per class): 2|A&B| / (|A|+|B|), 0 when both are empty."""
    a, b = outputs.bool(), labels.bool()
    dims = (0, 2, 3, 4)
    inter = (a & b).sum(dims).double()
    denom = a.sum(dims).double() + b.sum(dims).double()
    return torch.where(denom > 0, 2.0 * inter / denom.clamp(min=1), torch.zeros_like(denom))


def infer(model, image: torch.Tensor, roi_size=(96, 96, 96), sw_batch_size: int = 1, overlap: float = 0.25,
          distributed: bool = False, group=None, streaming: bool = False, postprocess: dict = None, mirror_axes=None,
          fill_holes: dict = None, mode: str = "constant", sigma_scale=0.125) -> torch.Tensor:
    """Engine.infer (engine.py:167-182): sliding-window DDIM sampling -> sigmoid -> > 0.5.  ``streaming``: the same through
    ``evaluate_volume`` (no list of window outputs, no fp32 normalised volume).  ``mode``, ``sigma_scale``: the blend's
    importance map, as ``sliding_window_inference``.  ``postprocess``: None, or a dict of
    ``postprocess.keep_largest_components`` keyword arguments applied to the binarised volume (fp32 is returned either way).
    Step-Uncertainty Fusion is the model's switch (``DiffUNet(..., uncer_step=R)``), not an argument of this function.
    ``mirror_axes``: mirror test-time augmentation, as ``sliding_window_inference``; ``postprocess`` and Step-Uncertainty
    Fusion compose with it without change.  The all-gather form (``distributed=True, streaming=False``) does not take it --
    its gathered bytes would grow F-fold -- and raises ValueError: use ``streaming=True``, whose all-reduce does not grow.
    ``fill_holes``: None, or a dict with keys among ("connectivity", "channels"): ``postprocess.fill_holes`` on the binarised
    volume, after ``postprocess`` when both are given."""
    if postprocess is not None:
        pp.check_stage_kwargs("postprocess", "mask", postprocess)
    if fill_holes is not None:
        pp.check_stage_kwargs("fill_holes", "mask", fill_holes)
    augmented = len(mirror_flips(mirror_axes)) > 1
    if streaming:
        return evaluate_volume(model, image, None, roi_size, sw_batch_size, overlap, distributed, group, postprocess,
                               mirror_axes=mirror_axes, mode=mode, sigma_scale=sigma_scale, fill_holes=fill_holes)[0].float()
    if distributed and augmented:
        raise ValueError("mirror_axes: the all-gather form would gather F times the window outputs; pass streaming=True "
                         "(one all-reduce of the same size) for mirror test-time augmentation across ranks")
    fn = sharded_sliding_window_inference if distributed else sliding_window_inference
    kw = dict(group=group) if distributed else dict(mirror_axes=mirror_axes)
    with torch.no_grad():
        out = fn(image, roi_size, sw_batch_size, model, overlap, mode=mode, sigma_scale=sigma_scale, pred_type="ddim_sample", **kw)
    return _run_stages(lambda ref: (binarise(out), None),
                       _stages(postprocess, fill_holes, pp.filter_components, pp.fill_holes, "labels"), None)[0].float()
