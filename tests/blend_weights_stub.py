"""What the Gaussian-weighting tests share: the importance map written out from the contract, an fp64 weighted blend of the
stub predictor's windows, and the rank program of the two-rank case.

As a program (under torch.distributed.run, gloo, every rank on device 0): runs the sharded streamed blend and the sharded
evaluate_volume with ``mode="gaussian"`` for each case of ``streamed_blend_stub.RANK_CASES`` and writes rank 0's volume and
mask, and whether every rank ended with the same bits, to ``<out>/case<k>.pt``."""
import os
import sys

import torch


def weight_map(vectors):
    """(m, w) from ``importance_vectors``' result: m = (g0[z] * g1[y]) * g2[x], each product rounded to fp32 in this order,
    and w = max(m, floor).  fp32, on the CPU."""
    g0, g1, g2, floor = vectors
    m = (g0[:, None, None] * g1[None, :, None]) * g2[None, None, :]
    return m, torch.maximum(m, torch.tensor(floor, dtype=torch.float32))


def fp64_weighted_blend(vol, roi, overlap, pred, sigma_scale):
    """Plain fp64 blend of the stub's windows on the CPU (the stub gives the same bits there) with the fp32 map widened to
    fp64: (q = sum w o / sum w, sum |w o| / sum w, windows over each voxel, |sum w o| / sum w), cropped to the volume."""
    from diff_unet_amos_amd.inference import _plan, _window, coverage_counts, importance_vectors
    spatial, roi, padded, pad, starts = _plan(vol, roi, overlap)
    w = weight_map(importance_vectors(roi, "gaussian", sigma_scale))[1].double()
    x = torch.nn.functional.pad(vol, pad)
    B, nwin = vol.shape[0], len(starts)
    C = pred(_window(x, 0, nwin, starts, roi)).shape[1]
    total = torch.zeros(B, C, *padded, dtype=torch.float64)
    mag = torch.zeros_like(total)
    wsum = torch.zeros(padded, dtype=torch.float64)
    for i in range(nwin * B):
        b, (d, h, ww) = i // nwin, starts[i % nwin]
        o = pred(_window(x, i, nwin, starts, roi))[0].double()
        sl = (slice(d, d + roi[0]), slice(h, h + roi[1]), slice(ww, ww + roi[2]))
        total[(b, slice(None)) + sl] += w * o
        mag[(b, slice(None)) + sl] += (w * o).abs()
        if b == 0:
            wsum[sl] += w
    nd, nh, nw = (torch.tensor(n, dtype=torch.float64) for n in coverage_counts(padded, roi, starts))
    count = (nd[:, None, None] * nh[None, :, None] * nw[None, None, :]).expand_as(total)
    crop = (slice(None), slice(None)) + tuple(slice(pad[2 * (2 - k)], pad[2 * (2 - k)] + spatial[k]) for k in range(3))
    return (total / wsum)[crop], (mag / wsum)[crop], count[crop], (total.abs() / wsum)[crop]


def _rank_main(out_dir):
    import torch.distributed as dist
    from diff_unet_amos_amd.inference import evaluate_volume, streamed_sliding_window_inference
    from streamed_blend_stub import RANK_CASES, make_predictor, seeded_volume
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    try:
        for k, (shape, roi, overlap, swb) in enumerate(RANK_CASES):
            pred = make_predictor(roi, dev)
            vol = seeded_volume(shape).to(dev)
            timings = {}
            q = streamed_sliding_window_inference(vol, roi, swb, pred, overlap, group=dist.group.WORLD, timings=timings,
                                                  mode="gaussian", pred_type="ddim_sample")
            mask, dice = evaluate_volume(pred, vol, None, roi, swb, overlap, distributed=True, mode="gaussian")
            assert dice is None
            mine = torch.cat([q.cpu().view(torch.uint8).flatten(), mask.cpu().flatten()])
            theirs = [torch.empty_like(mine) for _ in range(world)]
            dist.all_gather(theirs, mine)
            same = all(torch.equal(t, mine) for t in theirs)
            if rank == 0:
                torch.save({"q": q.cpu(), "mask": mask.cpu(), "same_on_every_rank": same, "timings": timings, "world": world},
                           os.path.join(out_dir, f"case{k}.pt"))
        dist.barrier()
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    _rank_main(sys.argv[1])
