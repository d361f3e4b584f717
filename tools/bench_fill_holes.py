#!/usr/bin/env python3
"""Filling the holes of a scan-sized label map on the device, against the nearest existing pass and against scipy on the host.

A synthetic case, seeded: 15 ellipsoid organs (classes 1..15) in a 160 x 512 x 512 scan; the prediction has every organ
displaced by a few voxels and, inside every organ, a handful of spherical pockets of background; one pocket of class 1 holds an
island of class 2 (the one place where the label-map rule differs from per-class binary_fill_holes).  Three things are timed:

  fill      postprocess.fill_holes_in_label_map(pred, 16, connectivity, reference=ref)   -- this change;
  filter    postprocess.filter_label_map(pred, 16, connectivity, 1, 0, reference=ref)    -- the nearest existing pass with the same
            union-find (on the foreground), interleaved with ``fill``, device events;
  scipy     pred.cpu(), then scipy.ndimage.binary_fill_holes(map == c, structure) for c = 1..15 and the map put together again
            -- what a user does today, the copy included, wall clock.

Before anything is timed the device result is compared, voxel for voxel, with the rule restated on the host with scipy
(ndimage.label of map == 0, then the dilation ring of every component that touches no face, inside its bounding box).

Prints one JSON line.

    python tools/bench_fill_holes.py            # full size
    python tools/bench_fill_holes.py --small    # a rehearsal: 40 x 96 x 96
    python tools/bench_fill_holes.py --enclosed --scipy-reps 0 [--connectivity 3]    # the contended case of the neighbour pass"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from diff_unet_amos_amd import _native as nv  # noqa: E402
from diff_unet_amos_amd import postprocess  # noqa: E402

CLASSES = 16
CAP = 65536
POCKETS = 6


def synthetic_case(shape, seed, device):
    """(prediction, reference) uint8 [D, H, W] on ``device``; the number of pocket voxels."""
    g = torch.Generator().manual_seed(seed)
    D, H, W = shape
    extent = torch.tensor([D, H, W], dtype=torch.float32)
    centre = (0.2 + 0.6 * torch.rand(CLASSES - 1, 3, generator=g)) * extent
    radius = (0.04 + 0.08 * torch.rand(CLASSES - 1, 3, generator=g)) * extent
    shift = torch.randint(-3, 4, (CLASSES - 1, 3), generator=g).float()
    d = torch.arange(D, device=device, dtype=torch.float32).view(D, 1, 1)
    h = torch.arange(H, device=device, dtype=torch.float32).view(1, H, 1)
    w = torch.arange(W, device=device, dtype=torch.float32).view(1, 1, W)

    def ellipsoid(c, r):
        return ((d - float(c[0])) / float(r[0])) ** 2 + ((h - float(c[1])) / float(r[1])) ** 2 + ((w - float(c[2])) / float(r[2])) ** 2 <= 1.0

    pred = torch.zeros(shape, dtype=torch.uint8, device=device)
    ref = torch.zeros(shape, dtype=torch.uint8, device=device)
    for k in range(CLASSES - 1):
        ref[ellipsoid(centre[k], radius[k])] = k + 1
        pred[ellipsoid(centre[k] + shift[k], radius[k])] = k + 1
    before = int((pred == 0).sum())
    for k in range(CLASSES - 1):                        # pockets well inside organ k + 1, each a small ellipsoid of background
        for _ in range(POCKETS):
            at = centre[k] + shift[k] + (torch.rand(3, generator=g) - 0.5) * radius[k]
            size = torch.clamp(radius[k] * (0.05 + 0.1 * float(torch.rand(1, generator=g))), min=1.0)
            pred[ellipsoid(at, size) & (pred == k + 1)] = 0
    at = centre[0] + shift[0]                           # the pocket with an island: class 1, at its centre
    pred[ellipsoid(at, torch.clamp(radius[0] * 0.2, min=2.0)) & (pred == 1)] = 0
    pred[int(at[0]), int(at[1]), int(at[2])] = 2
    return pred, ref, int((pred == 0).sum()) - before


def host_rule(m, C, k):
    """The label-map rule on the host with scipy: one labelling of the background, one dilation per enclosed component."""
    from scipy import ndimage
    st = ndimage.generate_binary_structure(3, k)
    lab, n = ndimage.label(m == 0, st)
    out = m.copy()
    open_labels = np.unique(np.concatenate([lab[0].ravel(), lab[-1].ravel(), lab[:, 0].ravel(), lab[:, -1].ravel(),
                                            lab[:, :, 0].ravel(), lab[:, :, -1].ravel()]))
    is_open = np.zeros(n + 1, dtype=bool)
    is_open[open_labels] = True
    for l, box in enumerate(ndimage.find_objects(lab), start=1):
        if is_open[l] or box is None:
            continue
        grown = tuple(slice(max(s.start - 1, 0), min(s.stop + 1, e)) for s, e in zip(box, m.shape))
        comp = lab[grown] == l
        ring = ndimage.binary_dilation(comp, st) & ~comp
        values = np.unique(m[grown][ring])
        if len(values) == 1 and 1 <= int(values[0]) < C:
            out[grown][comp] = values[0]
    return out


def host_per_class(pred, C, k):
    """What a user does today: the map to the host, binary_fill_holes per class, the map put together again."""
    from scipy import ndimage
    st = ndimage.generate_binary_structure(3, k)
    m = pred.cpu().numpy()
    out = m.copy()
    for c in range(1, C):
        filled = ndimage.binary_fill_holes(m == c, st)
        out[filled & (m == 0)] = c
    return out


def timed(functions, reps):
    """Interleaved: each of ``reps`` repetitions runs every function once, in order; device-event milliseconds per function."""
    times = [[] for _ in functions]
    for _ in range(reps):
        for i, f in enumerate(functions):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            f()
            stop.record()
            stop.synchronize()
            times[i].append(start.elapsed_time(stop))
    return [dict(median_ms=round(statistics.median(t), 3), min_ms=round(min(t), 3), max_ms=round(max(t), 3), reps=len(t)) for t in times]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--small", action="store_true", help="a rehearsal at 40 x 96 x 96")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scipy-reps", type=int, default=1)
    ap.add_argument("--connectivity", type=int, default=1)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--enclosed", action="store_true",
                    help="wrap the scan in a one-voxel shell of class 1 just inside its faces: the background around the organs is "
                         "then ONE enclosed component bordered by every class -- nothing more is filled, and all of its voxels "
                         "go through the neighbour pass (the contended case)")
    args = ap.parse_args()
    device = torch.device("cuda", 0)
    shape = (40, 96, 96) if args.small else (160, 512, 512)
    k = args.connectivity
    vox = shape[0] * shape[1] * shape[2]
    pred, ref, pocket_voxels = synthetic_case(shape, args.seed, device)
    if args.enclosed:
        inner = pred[1:-1, 1:-1, 1:-1]
        inner[0], inner[-1], inner[:, 0], inner[:, -1], inner[:, :, 0], inner[:, :, -1] = (1,) * 6

    def fill():
        return postprocess.fill_holes_in_label_map(pred, CLASSES, k, reference=ref)

    def keep():
        return postprocess.filter_label_map(pred, CLASSES, k, 1, 0, cap=CAP, reference=ref)

    out, filled, tallies = fill()
    keep()
    want = host_rule(pred.cpu().numpy(), CLASSES, k)
    differing = int((out.cpu().numpy() != want).sum())
    assert differing == 0, f"the device result differs from the rule restated with scipy in {differing} voxels"
    device_times = dict(zip(("fill", "filter"), timed([fill, keep], args.reps)))
    L = nv.lib()
    device_times["fill"]["bytes"] = int(L.dua_fill_holes_scratch_bytes(1, *shape, 1)) + vox
    device_times["filter"]["bytes"] = 4 * vox + int(L.dua_cc_map_scratch_bytes(1, *shape, CAP)) + vox
    host = []
    per_class = None
    for _ in range(args.scipy_reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        per_class = host_per_class(pred, CLASSES, k)
        host.append((time.perf_counter() - t0) * 1e3)
    scipy_times = dict(median_ms=round(statistics.median(host), 1), min_ms=round(min(host), 1), max_ms=round(max(host), 1),
                       reps=len(host)) if host else None
    print(json.dumps(dict(shape=shape, classes=CLASSES, connectivity=k, enclosed=args.enclosed, gpu=torch.cuda.get_device_name(0),
                          pocket_voxels=pocket_voxels, filled=int(filled.sum()), filled_per_class=filled.tolist(),
                          differs_from_rule=differing,
                          differs_from_per_class_scipy=None if per_class is None else int((per_class != want).sum()),
                          device=device_times, scipy_per_class_with_copy=scipy_times)))


if __name__ == "__main__":
    main()
