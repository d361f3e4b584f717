"""Deterministic stub predictor of the streamed-blend tests, and the rank program of their two-rank case.

The predictor is a function of the window contents plus a fixed pseudo-random field, built from operations that round once
and identically on every device and for every batch composition (multiply, add, flip, compare): the same window gives the same
bits on a CPU, on the GPU, alone or inside a batch, so a test can recompute any window's output wherever it likes.

As a program (under torch.distributed.run, gloo, every rank on device 0): runs the sharded streamed blend and the sharded
evaluate_volume for each case and writes rank 0's volume and mask, and whether every rank ended with the same bits, to
``<out>/case<k>.pt``."""
import os
import sys

import torch

CHANNELS = 4
MARKER = 7.0        # a data value no seeded volume contains: marks the voxels where windows of +3 and -3 meet


def make_predictor(roi, device, planted=False, channels=CHANNELS):
    """``predictor(x, pred_type=None)`` -> [b, channels, *roi] fp32.  Channel 0: 2 v + field; channel 1: flip(v) + 1 + field;
    channel 2: v v - 0.5 + field; the last channel: -10 + 0.1 field (never above 0: an empty class); further channels repeat
    channel 0's rule with their own field.  ``planted``: x has a second input channel whose value at the window's first voxel
    is the window's sign s = +-1, and a voxel whose data value is MARKER gets s * 3 in channel 0 instead."""
    g = torch.Generator().manual_seed(1234)
    field = (torch.randn(1, channels, *roi, generator=g) * 0.5).to(device)
    low = (field[:, -1:] * 0.1 - 10.0)

    def predictor(x, pred_type=None):
        v = x[:, :1]
        chans = []
        for c in range(channels - 1):
            if c == 1:
                o = v.flip(-1) + 1.0 + field[:, 1:2]
            elif c == 2:
                o = v * v - 0.5 + field[:, 2:3]
            else:
                o = v * 2.0 + field[:, c:c + 1]
            chans.append(o)
        if planted:
            s = x[:, 1:2, :1, :1, :1]
            chans[0] = torch.where(v == MARKER, (s * 3.0).expand_as(v), chans[0])
        chans.append(low.expand(x.shape[0], -1, -1, -1, -1))
        return torch.cat(chans, dim=1)

    return predictor


def seeded_volume(shape, seed=None):
    g = torch.Generator().manual_seed(sum(shape) if seed is None else seed)
    return torch.randn(*shape, generator=g)


# (volume shape, roi, overlap, sw_batch_size): a ragged plan with overlapping windows in every call, a batch of two padded
# volumes, and ONE window for two ranks (rank 1 has nothing to add and still takes part in the all-reduce)
RANK_CASES = [
    ((1, 1, 37, 50, 41), (16, 16, 16), 0.8, 3),
    ((2, 1, 9, 16, 16), (8, 8, 8), 0.5, 4),
    ((1, 1, 8, 8, 8), (8, 8, 8), 0.25, 2),
]


def _rank_main(out_dir):
    import torch.distributed as dist
    from diff_unet_amos_amd.inference import evaluate_volume, streamed_sliding_window_inference
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
                                                  pred_type="ddim_sample")
            mask, dice = evaluate_volume(pred, vol, None, roi, swb, overlap, distributed=True)
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
