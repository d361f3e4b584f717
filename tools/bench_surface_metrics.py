"""Time metrics.surface_distance_table (csrc/surface.hip) on synthetic 16-class ellipsoid labels.

    python tools/bench_surface_metrics.py [--repeats 20] [--warmup 3] [--no-scipy] [--nsd]

For [1, 16, 256, 256, 192] and [1, 16, 96, 96, 96]: the median and spread of the whole call (device events around it, after
warm-up), and the bytes the three EDT passes move per call (computed from the shape, both directions: W pass 1 B read + 8 B
written, H pass 8 + 8, D pass 8 + 1 per voxel) over that whole-call time.  With scipy importable, the CPU baseline the
reference's path takes (medpy's algorithm restated with scipy.ndimage, one class at a time) for a few classes, scaled to 16.

--nsd adds, after each shape's lines and by the same method, the Normalized Surface Dice calls at tolerances (2, 3) mm for every
class: the distance table again as the yardstick, ops.surface_dice_table with the band-limited transform (bounded=True) and
with the unbounded one (bounded=False), and ops.surface_report (the distance table and the surface Dice from one transform).
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from diff_unet_amos_amd import metrics, ops  # noqa: E402

EDT_BYTES_PER_VOXEL = 2 * ((1 + 8) + (8 + 8) + (8 + 1))


def labels(shape, classes, jitter, seed):
    """classes ellipsoids of varied size and place, one per channel; jitter moves centres and radii (the 'prediction')."""
    g = torch.Generator().manual_seed(seed)
    D, H, W = shape
    grid = torch.meshgrid(*[torch.arange(n, dtype=torch.float32, device="cuda") for n in shape], indexing="ij")
    out = torch.empty((1, classes, *shape), dtype=torch.float32, device="cuda")
    for c in range(classes):
        r = torch.rand(6, generator=g)
        centre = [(0.3 + 0.4 * r[i].item()) * n for i, n in enumerate(shape)]
        radii = [(0.08 + 0.2 * r[3 + i].item()) * n for i, n in enumerate(shape)]
        if jitter:
            j = torch.rand(6, generator=g) - 0.5
            centre = [x + 0.03 * j[i].item() * n for i, (x, n) in enumerate(zip(centre, shape))]
            radii = [x * (1 + 0.1 * j[3 + i].item()) for i, x in enumerate(radii)]
        out[0, c] = (sum(((x - m) / s) ** 2 for x, m, s in zip(grid, centre, radii)) <= 1.0).float()
    return out


def time_call(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def time_gpu(test, ref, spacing, warmup, repeats):
    return time_call(lambda: metrics.surface_distance_table(test, ref, voxel_spacing=spacing), warmup, repeats)


NSD_TOLERANCES = (2.0, 3.0)


def nsd_lines(test, ref, spacing, warmup, repeats):
    """One line per call shape: the distance table (yardstick), surface Dice bounded / unbounded, the report."""
    rows = [list(NSD_TOLERANCES)] * test.shape[1]
    calls = (("surface_distance_table", lambda: metrics.surface_distance_table(test, ref, voxel_spacing=spacing)),
             ("surface_dice_table bounded=True", lambda: ops.surface_dice_table(test, ref, rows, spacing, bounded=True)),
             ("surface_dice_table bounded=False", lambda: ops.surface_dice_table(test, ref, rows, spacing, bounded=False)),
             ("surface_report", lambda: metrics.surface_report(test, ref, rows, voxel_spacing=spacing)))
    for name, fn in calls:
        ms = time_call(fn, warmup, repeats)
        print(f"  nsd: {name}: {statistics.median(ms):.2f} ms median over {len(ms)} calls (min {min(ms):.2f}, "
              f"max {max(ms):.2f})", flush=True)
    nsd = metrics.surface_dice_table(test, ref, rows, voxel_spacing=spacing)["nsd"]
    print(f"  nsd: class 0 at {NSD_TOLERANCES} mm = {[round(float(x), 4) for x in nsd[0, 0]]}", flush=True)


def scipy_baseline(test, ref, spacing, classes):
    from scipy import ndimage
    import numpy as np
    fp = ndimage.generate_binary_structure(3, 1)
    t0 = time.perf_counter()
    for c in range(classes):
        a, b = test[0, c].bool().cpu().numpy(), ref[0, c].bool().cpu().numpy()
        ba = a & ~ndimage.binary_erosion(a, structure=fp, border_value=0)
        bb = b & ~ndimage.binary_erosion(b, structure=fp, border_value=0)
        sab = ndimage.distance_transform_edt(~bb, sampling=spacing)[ba]
        sba = ndimage.distance_transform_edt(~ba, sampling=spacing)[bb]
        max(sab.max(), sba.max()), np.percentile(np.hstack((sab, sba)), 95), sab.mean(), sba.mean()
    return (time.perf_counter() - t0) / classes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-scipy", action="store_true")
    ap.add_argument("--scipy-classes", type=int, default=2)
    ap.add_argument("--nsd", action="store_true", help="also time the Normalized Surface Dice calls")
    args = ap.parse_args()
    spacing = (2.0, 1.5, 1.5)
    for shape in ((256, 256, 192), (96, 96, 96)):
        ref = labels(shape, 16, False, 1)
        test = labels(shape, 16, True, 1)
        ms = time_gpu(test, ref, spacing, args.warmup, args.repeats)
        med = statistics.median(ms)
        vox = 16 * shape[0] * shape[1] * shape[2]
        gbs = EDT_BYTES_PER_VOXEL * vox / (med * 1e-3) / 1e9
        t = metrics.surface_distance_table(test, ref, voxel_spacing=spacing)
        line = (f"[1,16,{shape[0]},{shape[1]},{shape[2]}]: {med:.2f} ms median over {len(ms)} calls "
                f"(min {min(ms):.2f}, max {max(ms):.2f}); EDT-pass bytes {EDT_BYTES_PER_VOXEL * vox / 1e9:.2f} GB per call "
                f"-> {gbs:.0f} GB/s over the whole call; hd95 of class 0 = {float(t['hd95'][0, 0]):.4f}")
        print(line, flush=True)
        if args.nsd:
            nsd_lines(test, ref, spacing, args.warmup, args.repeats)
        if not args.no_scipy:
            try:
                import scipy  # noqa: F401
            except ImportError:
                print("  scipy not importable: no CPU baseline")
                continue
            per = scipy_baseline(test, ref, spacing, args.scipy_classes)
            print(f"  scipy CPU baseline: {per * 1e3:.0f} ms per class ({args.scipy_classes} classes timed), "
                  f"{16 * per:.2f} s for 16 classes", flush=True)


if __name__ == "__main__":
    main()
