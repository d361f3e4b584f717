"""The contract of mirror test-time augmentation (include/dua_hip.h) restated in fp64 numpy, for the mirror tests, and the
rank program of their two-rank case.

The plan (windows, padding, window order) is the unmirrored one and is taken from ``inference._plan``; everything the feature
adds is written out here on its own: the flip set, flip -> predict -> un-flip, the weight on the un-flipped output, the
divisor F times the unmirrored one.  The predictor is called window by window (the stub of streamed_blend_stub gives the same
bits alone or inside a batch), its fp32 output is widened and every sum is fp64.

As a program (under torch.distributed.run, gloo, every rank on device 0): runs the sharded streamed blend with and without
``mirror_axes`` for each case of ``RANK_CASES`` and writes rank 0's volume, whether every rank ended with the same bits, and
the timings of both runs to ``<out>/case<k>.pt``."""
import itertools
import os
import sys

import numpy as np
import torch

# (volume shape, roi, overlap, sw_batch_size, mirror_axes, mode)
RANK_CASES = [
    ((1, 1, 11, 13, 18), (8, 8, 12), 0.5, 2, (0, 1, 2), "constant"),
    ((2, 1, 9, 16, 16), (8, 8, 8), 0.5, 4, (2,), "gaussian"),
]


def flip_masks(mirror_axes):
    """Every subset of the axes as a 3-bit mask, ascending."""
    axes = tuple(mirror_axes or ())
    return sorted(sum(1 << a for a in sub) for k in range(len(axes) + 1) for sub in itertools.combinations(axes, k))


def flip_np(a, mask):
    """``a`` [..., D, H, W] with the axes of ``mask`` reversed."""
    for axis in range(3):
        if mask >> axis & 1:
            a = np.flip(a, axis=a.ndim - 3 + axis)
    return a


def weight_map_np(vectors):
    """w = max((g0[z] * g1[y]) * g2[x], floor), each product rounded to fp32 in this order; returned as fp64."""
    g0, g1, g2 = (v.numpy().astype(np.float32) for v in vectors[:3])
    m = (g0[:, None, None] * g1[None, :, None]).astype(np.float32) * g2[None, None, :]
    return np.maximum(m.astype(np.float32), np.float32(vectors[3])).astype(np.float64)


def mirrored_blend_fp64(vol, roi, overlap, pred, mirror_axes, mode="constant", sigma_scale=0.125):
    """(q, mag, n) fp64 [B, C, *spatial]: q = sum over windows and flips of w unflip(o_f) / (F sum over windows of w),
    mag = the same with |w unflip(o_f)|, n = F times the number of windows over the voxel = the fp32 additions per voxel."""
    from diff_unet_amos_amd.inference import _plan, importance_vectors
    spatial, roi, padded, pad, starts = _plan(vol, roi, overlap)
    masks = flip_masks(mirror_axes)
    w = weight_map_np(importance_vectors(roi, mode, sigma_scale))
    x = torch.nn.functional.pad(vol, pad).numpy()
    B = vol.shape[0]
    total = mag = None
    wsum = np.zeros(padded)
    cover = np.zeros(padded)
    for b in range(B):
        for (d, h, ww) in starts:
            sl = (slice(d, d + roi[0]), slice(h, h + roi[1]), slice(ww, ww + roi[2]))
            window = x[(slice(b, b + 1), slice(None)) + sl]
            for f in masks:
                o = pred(torch.from_numpy(np.ascontiguousarray(flip_np(window, f))), pred_type="ddim_sample")
                o = flip_np(o.numpy().astype(np.float64), f)[0]
                if total is None:
                    total = np.zeros((B, o.shape[0], *padded))
                    mag = np.zeros_like(total)
                total[(b, slice(None)) + sl] += w * o
                mag[(b, slice(None)) + sl] += np.abs(w * o)
            if b == 0:
                wsum[sl] += w
                cover[sl] += 1
    F = len(masks)
    crop = (slice(None), slice(None)) + tuple(slice(pad[2 * (2 - k)], pad[2 * (2 - k)] + spatial[k]) for k in range(3))
    n = np.broadcast_to(F * cover, total.shape)
    return (torch.from_numpy((total / (F * wsum))[crop]), torch.from_numpy((mag / (F * wsum))[crop]),
            torch.from_numpy(np.ascontiguousarray(n[crop])))


def fp32_bound(q64, mag, n, mode):
    """|q_fp32 - q64| for a voxel whose n terms are added in fp32 in any order, u = 2^-24, (1 + 2^-10) for the second order
    (n <= 2^13).  Constant weights: the terms are exact, n - 1 rounded additions, the count is an exact integer and one correctly
    rounded division follows: (n - 1) u mag + ulp(q).  Gaussian: every term takes one rounded product and at most n - 1
    additions, the weight sum at most n - 1 more (its scaling by F is exact) and the division one: at most 2 n roundings on any
    term, n 2^-23 mag."""
    if mode == "constant":
        return (n - 1) * 2.0 ** -24 * (1 + 2.0 ** -10) * mag + 2.0 ** -23 * q64.abs() + 2.0 ** -149
    return n * 2.0 ** -23 * (1 + 2.0 ** -10) * mag + 2.0 ** -149


def _rank_main(out_dir):
    import torch.distributed as dist
    from diff_unet_amos_amd.inference import streamed_sliding_window_inference
    from streamed_blend_stub import make_predictor, seeded_volume
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    try:
        for k, (shape, roi, overlap, swb, axes, mode) in enumerate(RANK_CASES):
            pred = make_predictor(roi, dev)
            vol = seeded_volume(shape).to(dev)
            timings, plain = {}, {}
            q = streamed_sliding_window_inference(vol, roi, swb, pred, overlap, group=dist.group.WORLD, timings=timings,
                                                  mirror_axes=axes, mode=mode, pred_type="ddim_sample")
            streamed_sliding_window_inference(vol, roi, swb, pred, overlap, group=dist.group.WORLD, timings=plain, mode=mode,
                                              pred_type="ddim_sample")
            mine = q.cpu().view(torch.uint8).flatten()
            theirs = [torch.empty_like(mine) for _ in range(world)]
            dist.all_gather(theirs, mine)
            same = all(torch.equal(t, mine) for t in theirs)
            if rank == 0:
                torch.save({"q": q.cpu(), "same_on_every_rank": same, "timings": timings, "plain_timings": plain, "world": world},
                           os.path.join(out_dir, f"case{k}.pt"))
        dist.barrier()
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    _rank_main(sys.argv[1])
