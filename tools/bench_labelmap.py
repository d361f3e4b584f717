"""Time the label map on the grid of the scan (csrc/labelmap.hip) against the same result from torch operators.

    python tools/bench_labelmap.py [--repeats 3] [--warmup 2] [--rounds 3] [--small] [--out profiles/labelmap_bench.json]

One synthetic case: a 512 x 512 x 200 scan at 0.78 x 0.78 x 2.5 mm whose foreground box is [40, 472) x [60, 452) x [0, 200),
prepared to (1.5, 1.5, 2.0) mm "RAS" (225 x 204 x 250), 16 classes, a resident fp32 sum volume of N(0, 2) logits times
non-uniform window counts, and a random uint8 label map of the scan.  Two paths on the same device, in alternating rounds in
one process (``--rounds`` of ``--repeats`` calls each, device events around a whole round, after warm-up of both; the statistic
is the median round, the spread its min .. max):

    native : ops.blend_finish_labelmap -- one launch from the sum volume to the uint8 label map and its Dice tallies;
    torch  : what a user has today -- ops.blend_finish for q on the prepared grid, torch.sigmoid, one index_select pair and one
             lerp per axis (prepared axis 2, then 1, then 0: the contract's order) up to fp32 [C, X0, X1, X2] on the scan's grid,
             argmax over the classes, 0 outside the box, and the three tallies per class with torch comparisons.

Reported per path: the time per call and the peak memory the call adds to what is resident before it (the sum volume, the
tables, the reference map), from torch's allocator statistics.  The two label maps are compared (voxels that differ: torch
rounds a lerp as a + w * (b - a) in two operations, the kernel as one fmaf).  The figures the kernel's work derives from, per
source voxel inside the box: 8 C fp32 reads of the sum volume, 8 C exponentials, 16 C IEEE divisions, 7 C lerps; 1 label byte
written and 1 reference byte read per source voxel.  One JSON line at the end, also written to ``--out``.
"""
import argparse
import json
import os
import socket
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from diff_unet_amos_amd import ops, prepare  # noqa: E402

DEV = "cuda:0"
PIXDIM = (1.5, 1.5, 2.0)


def torch_labelmap(acc, divisor, spatial, tables, source_shape, reference, classes):
    """The contract in torch operators: (label map uint8 [*source], tallies int64 [C, 3])."""
    lo, weight, axis = tables
    q = ops.blend_finish(acc, divisor, (0, 0, 0), spatial, want_q=True)[0][0]
    p = torch.sigmoid(q)
    del q
    stride = (spatial[1] * spatial[2], spatial[2], 1)
    inside = None
    for j in (2, 1, 0):                                                  # the lerp order of the contract
        src_axis = axis.index(j)
        entry = lo[src_axis]
        lower = (entry.clamp(min=0) // stride[j]).long()
        upper = (lower + 1).clamp(max=spatial[j] - 1)
        shape = [1, 1, 1, 1]
        shape[1 + j] = -1
        a, b = p.index_select(1 + j, lower), p.index_select(1 + j, upper)
        p = a + weight[src_axis].view(shape) * (b - a)
        del a, b
        ok = (entry >= 0).view(shape[1:])
        inside = ok if inside is None else inside & ok
    order = [0] + [1 + axis[s] for s in range(3)]                        # prepared-axis order -> source-axis order
    label = p.permute(order).argmax(dim=0).to(torch.uint8)
    label = label * inside.permute([axis[s] for s in range(3)]).to(torch.uint8)
    del p
    c = torch.arange(classes, device=label.device, dtype=torch.uint8).view(-1, 1, 1, 1)
    tallies = torch.empty((classes, 3), dtype=torch.int64, device=label.device)
    for k in range(classes):                                             # per class: no [C, *source] boolean tensors on top
        a, b = label == c[k], reference == c[k]
        tallies[k, 0], tallies[k, 1], tallies[k, 2] = (a & b).sum(), a.sum(), b.sum()
    return label, tallies


def timed(fn, repeats):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(repeats):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / repeats                            # milliseconds per call


def peak_extra(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - before
    del out
    return int(extra)


def stats(rounds):
    return dict(median_ms=round(statistics.median(rounds), 3), min_ms=round(min(rounds), 3), max_ms=round(max(rounds), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--classes", type=int, default=16)
    ap.add_argument("--small", action="store_true", help="a 64 x 64 x 25 scan: a rehearsal of the tool, not a measurement")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_labelmap: no GPU: nothing is measured on a CPU")
    X = (64, 64, 25) if args.small else (512, 512, 200)
    box = ((5, 59), (7, 56), (0, 25)) if args.small else ((40, 472), (60, 452), (0, 200))
    spacing = (0.78, 0.78, 2.5)
    geom = prepare.prepared_geometry(X, box, np.diag(spacing + (1.0,)), PIXDIM)
    t = prepare.linear_restore_tables(geom)
    tables = (tuple(torch.from_numpy(v).to(DEV) for v in t["lo"]), tuple(torch.from_numpy(v).to(DEV) for v in t["weight"]), t["axis"])
    Cn, spatial = args.classes, geom.shape
    g = torch.Generator(device=DEV).manual_seed(0)
    divisor = [torch.randint(1, 5, (n,), generator=g, device=DEV, dtype=torch.int32) for n in spatial]
    den = (divisor[0].view(-1, 1, 1) * divisor[1].view(1, -1, 1) * divisor[2].view(1, 1, -1)).float()
    acc = torch.randn((1, Cn, *spatial), generator=g, device=DEV) * 2.0 * den
    del den
    reference = torch.randint(0, Cn, X, generator=g, device=DEV, dtype=torch.uint8)
    paths = {"native": lambda: ops.blend_finish_labelmap(acc, divisor, (0, 0, 0), spatial, tables, X, 0.0, reference),
             "torch": lambda: torch_labelmap(acc, divisor, spatial, tables, X, reference, Cn)}
    got, got_t = paths["native"]()
    want, want_t = paths["torch"]()
    differ = int((got != want).sum())
    tallies_native_exact = bool(torch.equal(got_t[:, 2], want_t[:, 2]))          # |reference == c| does not depend on the labels
    del want, want_t, got_t
    memory = {k: peak_extra(fn) for k, fn in paths.items()}
    for fn in paths.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    rounds = {k: [] for k in paths}
    for _ in range(args.rounds):
        for k, fn in paths.items():
            rounds[k].append(timed(fn, args.repeats))
    voxels = int(np.prod(X))
    inside = int(np.prod([hi - lo for lo, hi in box]))
    result = dict(host=socket.gethostname(), device=torch.cuda.get_device_name(0), source=list(X), box=[list(b) for b in box],
                  prepared=list(spatial), classes=Cn, spacing=list(spacing), pixdim=list(PIXDIM), repeats=args.repeats,
                  rounds=args.rounds, native=stats(rounds["native"]), torch_operators=stats(rounds["torch"]),
                  native_peak_extra_bytes=memory["native"], torch_peak_extra_bytes=memory["torch"],
                  class_by_source_fp32_bytes=4 * Cn * voxels, label_map_bytes=voxels, sum_volume_bytes=acc.numel() * 4,
                  voxels_inside_box=inside, exponentials=8 * Cn * inside, divisions=16 * Cn * inside, sum_reads_bytes=32 * Cn * inside,
                  labels_that_differ_from_torch=differ, reference_counts_equal=tallies_native_exact)
    result["torch_over_native"] = round(result["torch_operators"]["median_ms"] / result["native"]["median_ms"], 2)
    result["native_gexp_per_s"] = round(result["exponentials"] / result["native"]["median_ms"] / 1e6, 1)
    print(f"native {result['native']['median_ms']:9.3f} ms (+{memory['native'] / 2 ** 20:9.1f} MiB)   torch "
          f"{result['torch_operators']['median_ms']:9.3f} ms (+{memory['torch'] / 2 ** 20:9.1f} MiB)   torch / native "
          f"{result['torch_over_native']}   {result['native_gexp_per_s']} G exponentials / s   labels that differ {differ} of "
          f"{voxels}", flush=True)
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
