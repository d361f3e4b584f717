"""Time connected-component labelling, sizes and the keep-largest filter (csrc/components.hip) on the device.

    python tools/bench_components.py [--repeats 20] [--warmup 3] [--no-scipy] [--small]

Cases: a 16-class volume [1, 16, 256, 256, 192] (one ellipsoid per class plus 0.2 % single-voxel speckle), and two synthetic
extremes of one volume [256, 256, 192]: independent voxels at 30 % fill (hundreds of thousands of components, the numbering
and the size atomics at their worst) and one serpentine component (every second row full, rows joined alternately at either
end: the longest parent chains).  Per case, with device events around each stage after warm-up, median and spread of
``ops.cc_label``, ``ops.cc_sizes`` and ``ops.cc_filter``; the floor, one plain device pass over the same bytes (1 byte of mask
read, 4 bytes of label written per voxel: ``mask.to(torch.int32)``); and, with scipy importable, the host path it replaces:
copy the mask to the host, scipy.ndimage.label per volume, copy the labels back (a few volumes timed, scaled to all)."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from diff_unet_amos_amd import ops, postprocess  # noqa: E402

DEV = "cuda"


def ellipsoids(shape, classes, speckle, seed):
    g = torch.Generator().manual_seed(seed)
    grid = torch.meshgrid(*[torch.arange(n, dtype=torch.float32, device=DEV) for n in shape], indexing="ij")
    out = torch.empty((1, classes, *shape), dtype=torch.uint8, device=DEV)
    gd = torch.Generator(device=DEV).manual_seed(seed)
    for c in range(classes):
        r = torch.rand(6, generator=g)
        centre = [(0.3 + 0.4 * r[i].item()) * n for i, n in enumerate(shape)]
        radii = [(0.08 + 0.2 * r[3 + i].item()) * n for i, n in enumerate(shape)]
        body = sum(((x - m) / s) ** 2 for x, m, s in zip(grid, centre, radii)) <= 1.0
        out[0, c] = (body | (torch.rand(shape, device=DEV, generator=gd) < speckle)).to(torch.uint8)
    return out


def random_fill(shape, fill, seed):
    gd = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.rand((1, 1, *shape), device=DEV, generator=gd) < fill).to(torch.uint8)


def serpentine(shape):
    D, H, W = shape
    m = torch.zeros((1, 1, *shape), dtype=torch.uint8, device=DEV)
    m[0, 0, ::2, ::2, :] = 1
    m[0, 0, ::2, 1:H - 1:4, W - 1] = 1
    m[0, 0, ::2, 3:H - 1:4, 0] = 1
    m[0, 0, 1:D - 1:2, 0, 0] = 1
    return m


def timed(fn, warmup, repeats):
    for _ in range(warmup):
        out = fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return out, ms


def fmt(ms):
    return f"{statistics.median(ms):9.3f} ms (min {min(ms):.3f}, max {max(ms):.3f})"


def scipy_path(mask, volumes):
    from scipy import ndimage
    import numpy as np
    flat = mask.view(-1, *mask.shape[-3:])
    t0 = time.perf_counter()
    for v in range(volumes):
        host = flat[v].cpu().numpy()
        lab, _ = ndimage.label(host, ndimage.generate_binary_structure(3, 1))
        torch.from_numpy(lab.astype(np.int32)).to(DEV)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / volumes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-scipy", action="store_true")
    ap.add_argument("--scipy-volumes", type=int, default=2)
    ap.add_argument("--small", action="store_true", help="[64, 64, 48] volumes: a rehearsal of the tool, not a measurement")
    args = ap.parse_args()
    shape = (64, 64, 48) if args.small else (256, 256, 192)
    cap = postprocess.DEFAULT_CAP
    cases = (("16 classes, ellipsoid + 0.2 % speckle", lambda: ellipsoids(shape, 16, 0.002, 1)),
             ("random 30 % fill", lambda: random_fill(shape, 0.3, 2)),
             ("one serpentine component", lambda: serpentine(shape)))
    for name, make in cases:
        mask = make()
        V, vox = mask.numel() // (shape[0] * shape[1] * shape[2]), shape[0] * shape[1] * shape[2]
        (labels, counts), t_label = timed(lambda: ops.cc_label(mask, 1), args.warmup, args.repeats)
        sizes, t_sizes = timed(lambda: ops.cc_sizes(labels, cap), args.warmup, args.repeats)
        _, t_filter = timed(lambda: ops.cc_filter(labels, counts, sizes, 1, 0), args.warmup, args.repeats)
        _, t_floor = timed(lambda: mask.to(torch.int32), args.warmup, args.repeats)
        total = statistics.median(t_label) + statistics.median(t_sizes) + statistics.median(t_filter)
        print(f"{name}: [{V} x {shape[0]} x {shape[1]} x {shape[2]}], fill {float(mask.float().mean()):.3f}, components "
              f"{counts.tolist()[:4]}{' ...' if V > 4 else ''} (cap {cap})", flush=True)
        print(f"  label   {fmt(t_label)}\n  sizes   {fmt(t_sizes)}\n  filter  {fmt(t_filter)}\n  floor   {fmt(t_floor)}   "
              f"(1 + 4 bytes per voxel = {5 * V * vox / 1e9:.3f} GB -> {5 * V * vox / statistics.median(t_floor) / 1e6:.0f} GB/s)")
        print(f"  label + sizes + filter = {total:.3f} ms = {total / statistics.median(t_floor):.1f} x the floor", flush=True)
        if not args.no_scipy:
            try:
                import scipy  # noqa: F401
            except ImportError:
                print("  scipy not importable: no host baseline")
                continue
            n = min(args.scipy_volumes, V)
            per = scipy_path(mask, n)
            print(f"  host path (copy, scipy.ndimage.label, copy back): {per * 1e3:.0f} ms per volume ({n} timed), "
                  f"{V * per * 1e3:.0f} ms for {V}", flush=True)
        del labels, counts, sizes, mask


if __name__ == "__main__":
    main()
