#!/usr/bin/env python3
"""Step time of a 50-step DDIM sample (DiffUNet.forward, pred_type="ddim_sample": encoder once + 50 graph-replayed steps),
default widths, 16 classes, fp16, batch 1, at 96^3 and at an odd extent (replicate-padded decoder levels).
Each extent: one warm-up call, then the best of ``rounds`` timed calls; the two extents alternate twice.
usage: bench_odd_extent.py [D H W] [rounds]"""
import os
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from diff_unet_amos_amd.diff_unet import DiffUNet


def main():
    nums = [int(a) for a in sys.argv[1:]]
    odd = tuple(nums[:3]) if len(nums) >= 3 else (97, 96, 95)
    rounds = nums[3] if len(nums) >= 4 else 3
    torch.manual_seed(0)
    net = DiffUNet(in_channels=1, out_channels=16, sample_steps=50, compute_dtype=torch.float16).cuda().eval()
    for dims in [(96, 96, 96), odd] * 2:
        image = torch.rand(1, 1, *dims, device="cuda")
        with torch.no_grad():
            net(image, pred_type="ddim_sample")
            torch.cuda.synchronize()
            ts = []
            for _ in range(rounds):
                t0 = time.perf_counter()
                out = net(image, pred_type="ddim_sample")
                torch.cuda.synchronize()
                ts.append(time.perf_counter() - t0)
        best = min(ts)
        print(f"{dims}: 50-step ddim_sample best of {rounds} {best * 1e3:.1f} ms ({best / 50 * 1e3:.3f} ms/step, encoder included); "
              f"all {[round(t * 1e3, 1) for t in ts]} ms; finite={bool(torch.isfinite(out).all())}", flush=True)


if __name__ == "__main__":
    main()
