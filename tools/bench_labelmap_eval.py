#!/usr/bin/env python3
"""Filtering and scoring a scan-sized label map as it is, against the one-hot path on the same inputs, in one process.

A synthetic case, seeded: 15 ellipsoid organs (classes 1..15) in a 160 x 512 x 512 scan at spacing (2.5, 0.8, 0.8), the prediction
with every organ displaced by a few voxels and 20 000 single stray voxels of random classes ("speckle").  Two legs, each comparing
its two paths' outputs BEFORE anything is timed, then timing them interleaved with device events:

  (a) components: postprocess.filter_label_map on the map, against the one-hot expansion [1, 16, *scan] plus
      postprocess.keep_largest_components on it (the expansion is part of that path: a user holding a label map has to make it);
  (b) surface:    metrics.label_map_surface_report of the FILTERED map against the reference map, classes 1..15, against the
      expansion of both maps plus metrics.surface_report over the full extent.  asd / assd are compared under the derived bound
      2 (n - 1) 2^-53 (another summation order), everything else bit for bit.

Prints one JSON line with the times (median, min, max over --reps), and the derived workspace bytes of both paths.

    python tools/bench_labelmap_eval.py            # full size
    python tools/bench_labelmap_eval.py --small    # a rehearsal: 40 x 96 x 96, 2 000 stray voxels"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from diff_unet_amos_amd import _native as nv  # noqa: E402
from diff_unet_amos_amd import metrics, ops, postprocess  # noqa: E402

CLASSES = 16
SPACING = (2.5, 0.8, 0.8)
TOLERANCES = (1.0, 3.0)
CAP = 65536


def synthetic_case(shape, speckle, seed, device):
    """(prediction, reference) uint8 [D, H, W] on ``device``."""
    g = torch.Generator().manual_seed(seed)
    D, H, W = shape
    extent = torch.tensor([D, H, W], dtype=torch.float32)
    centre = (0.2 + 0.6 * torch.rand(CLASSES - 1, 3, generator=g)) * extent
    radius = (0.04 + 0.08 * torch.rand(CLASSES - 1, 3, generator=g)) * extent
    shift = torch.randint(-3, 4, (CLASSES - 1, 3), generator=g).float()
    d = torch.arange(D, device=device, dtype=torch.float32).view(D, 1, 1)
    h = torch.arange(H, device=device, dtype=torch.float32).view(1, H, 1)
    w = torch.arange(W, device=device, dtype=torch.float32).view(1, 1, W)
    pred = torch.zeros(shape, dtype=torch.uint8, device=device)
    ref = torch.zeros(shape, dtype=torch.uint8, device=device)
    for k in range(CLASSES - 1):
        for out, c in ((ref, centre[k]), (pred, centre[k] + shift[k])):
            inside = ((d - float(c[0])) / float(radius[k, 0])) ** 2 + ((h - float(c[1])) / float(radius[k, 1])) ** 2 + \
                     ((w - float(c[2])) / float(radius[k, 2])) ** 2 <= 1.0
            out[inside] = k + 1
    where = torch.randint(0, D * H * W, (speckle,), generator=g).to(device)
    value = torch.randint(1, CLASSES, (speckle,), generator=g).to(torch.uint8).to(device)
    pred.view(-1)[where] = value
    return pred, ref


def expand(m):
    return (m[None, None] == torch.arange(CLASSES, device=m.device, dtype=m.dtype).view(1, -1, 1, 1, 1)).to(torch.uint8)


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
    ap.add_argument("--seed", type=int, default=7)
    args = ap.parse_args()
    device = torch.device("cuda", 0)
    shape, speckle = ((40, 96, 96), 2000) if args.small else ((160, 512, 512), 20000)
    vox = shape[0] * shape[1] * shape[2]
    pred, ref = synthetic_case(shape, speckle, args.seed, device)
    classes = list(range(1, CLASSES))
    tol = [list(TOLERANCES)] * len(classes)
    L = nv.lib()

    # ---- (a) components ----
    def new_filter():
        return postprocess.filter_label_map(pred, CLASSES, 1, 1, 0, cap=CAP, reference=ref)

    def old_filter():
        return postprocess.filter_components(expand(pred), 1, 1, 0, channels=classes, cap=CAP, labels=ref[None])

    filtered, tallies = new_filter()
    kept, old_tallies = old_filter()
    count = postprocess.label_map_components(pred, CLASSES)[1]
    assert int(count) <= CAP, f"{int(count)} components overflow the size table"
    for c in classes:
        assert torch.equal(filtered == c, kept[0, c] != 0), f"components: class {c} differs"
    assert torch.equal(tallies[1:], old_tallies[1:]), "components: tallies differ"
    del kept
    components = dict(zip(("label_map", "one_hot"), timed([new_filter, old_filter], args.reps)))
    components["components"] = int(count)
    # labels int32 per volume + the call's workspace + the output (+ the expansion)
    components["label_map"]["bytes"] = 4 * vox + int(L.dua_cc_map_scratch_bytes(1, *shape, CAP)) + vox
    components["one_hot"]["bytes"] = CLASSES * (4 * vox + vox) + int(L.dua_cc_scratch_bytes(CLASSES, *shape, CAP)) + CLASSES * vox

    # ---- (b) surface ----
    def new_report():
        return metrics.label_map_surface_report(filtered, ref, classes, tol, SPACING)

    def old_report():
        return metrics.surface_report(expand(filtered)[:, 1:], expand(ref)[:, 1:], tol, SPACING)

    got, want = new_report(), old_report()
    for k in want:
        a, b = got[k].contiguous(), want[k].contiguous()
        if k in ("asd", "assd"):
            na, nb = want["surface_test"].double(), want["surface_reference"].double()
            n = 2 * (na - 1) + 2 if k == "asd" else 2 * (torch.maximum(na, nb) - 1) + 4          # terms summed, + the divisions / additions
            ok = ~torch.isnan(b)
            assert torch.equal(torch.isnan(a), torch.isnan(b)) and bool(((a[ok] - b[ok]).abs() <= n[ok] * 2.0 ** -53 * b[ok]).all()), k
        else:
            assert torch.equal(a.view(torch.int64) if a.dtype == torch.float64 else a,
                               b.view(torch.int64) if b.dtype == torch.float64 else b), f"surface: {k} differs"
    boxes = ops.surface_map_boxes(filtered[None], ref[None], CLASSES)[:, classes].cpu().tolist()
    surface = dict(zip(("label_map", "one_hot"), timed([new_report, old_report], args.reps)))
    surface["label_map"]["bytes"] = max(metrics.label_map_workspace_bytes(shape, boxes))
    surface["one_hot"]["bytes"] = int(L.dua_surface_scratch_bytes(len(classes), *shape)) + 2 * CLASSES * vox
    surface["box_voxels"] = sum((b[3] - b[0]) * (b[4] - b[1]) * (b[5] - b[2]) for b in boxes[0] if b[3])
    surface["hd95_mm"] = [round(float(x), 4) for x in got["hd95"][0]]
    surface["nsd_at_1mm"] = [round(float(x), 4) for x in got["nsd"][0, :, 0]]
    print(json.dumps(dict(shape=shape, speckle=speckle, classes=CLASSES, device=torch.cuda.get_device_name(0), components=components,
                          surface=surface)))


if __name__ == "__main__":
    main()
