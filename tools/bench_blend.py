"""Time the whole-volume blend of sliding-window inference, streamed (csrc/blend.hip) against list-and-blend, predictor excluded.

    python tools/bench_blend.py [--volume 240 240 180] [--channels 16] [--roi 96] [--overlap 0.8] [--sw-batch 4]
                                [--repeats 5] [--warmup 2] [--mode constant|gaussian] [--sigma-scale 0.125] [--mirror 0,1,2]

A stub predictor hands out preallocated window outputs (a pool of --sw-batch random fp32 windows, reused by every call), so
only the blend is timed.  Per repeat, alternating the two forms, between device synchronisations:
  streamed : one dua_blend_accumulate per predictor call into the fp32 sum volume, then one dua_blend_finish that writes the
             uint8 mask and the Dice tallies against one-hot fp32 labels (inference.evaluate_volume without the predictor);
  listed   : inference._blend on the list of (index, window) pairs + binarise + dice_per_class on the same windows and labels.
The two masks are compared outside |q| <= 2^-20 and the Dice vectors printed.  Peak device memory (max_memory_allocated above
what is resident before the call: pool, labels, table) is reported for both; the listed form's figure does NOT contain the
list of window outputs a real predictor would leave (the pool is shared) -- that list is printed as derived bytes.  Bytes
moved by the streamed form are computed from the shapes.  The last lines are the derived (not measured) bytes a rank receives
in the gather and in the all-reduce form for 2, 4 and 8 ranks.

--mode gaussian: the streamed and the listed form blend with the Gaussian importance map (dua_blend_accumulate_weighted per
call, one dua_blend_weight_sum, dua_blend_finish_weighted; ``_blend`` with the map), and the constant-mode streamed form is
timed in the same alternation and printed next to them as "streamed_constant_seconds".

--mirror AXES (e.g. 0,1,2): instead of the above, the accumulate step of mirror test-time augmentation alone, over every call of
the plan into the same sum volume, alternating per repeat between device synchronisations:
  (a) the unmirrored accumulate (dua_blend_accumulate, or its weighted form with --mode gaussian);
  (b) the mirrored accumulate, once per flip mask of the axes (dua_blend_accumulate_mirrored: the un-flip is the read order);
  (c) torch.flip of the call's window outputs followed by the unmirrored accumulate -- the only way without the mirrored entry
      point -- once per mask.
One JSON line: median seconds of each, derived bytes (window read, volume read, volume written per window; (c) adds a read and
a write of the window) and rates, the ratios (b)/(a) and (b)/(c) per mask.  The three forms add different values, so only
times are compared; tests/test_mirror_gpu.py has the bit-equality of (b) and (c)."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from diff_unet_amos_amd import ops  # noqa: E402
from diff_unet_amos_amd.inference import (_blend, _plan, axis_starts, binarise, blend_traffic_bytes, coverage_counts,  # noqa: E402
                                          dice_per_class, importance_map, importance_vectors, window_table)


def clocks():
    """Whatever this box reports about the device clock, read-only."""
    try:
        return f"{torch.cuda.clock_rate()} MHz (torch.cuda.clock_rate)"
    except Exception:       # noqa: BLE001 -- no management library: say so
        return "not available"


def mirror_bench(args, dev, pool, table, calls, weights, Cn, roi, padded, nwin):
    from diff_unet_amos_amd.inference import _flip_dims, mirror_flips
    masks = mirror_flips(args.mirror)
    acc = ops.zeros((1, Cn, *padded), torch.float32, dev)

    def mirrored(f=0):
        for g0, nb in calls:
            ops.blend_accumulate(acc, pool[:nb], table, g0, weights=weights, flip=f)

    def flip_then_plain(f):
        for g0, nb in calls:
            ops.blend_accumulate(acc, torch.flip(pool[:nb], _flip_dims(f)) if f else pool[:nb], table, g0, weights=weights)

    def run(fn, *a):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(*a)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    forms = [("a", mirrored, ())] + [(f"b{f}", mirrored, (f,)) for f in masks] + [(f"c{f}", flip_then_plain, (f,)) for f in masks]
    for _ in range(args.warmup):
        for _, fn, a in forms:
            run(fn, *a)
    times = {name: [] for name, _, _ in forms}
    for _ in range(args.repeats):                                  # alternate the forms
        for name, fn, a in forms:
            times[name].append(run(fn, *a))
    med = {name: statistics.median(t) for name, t in times.items()}

    def spread(name):
        return {"median": med[name], "min": min(times[name]), "max": max(times[name])}

    window_bytes = Cn * roi[0] * roi[1] * roi[2] * 4
    moved = nwin * 3 * window_bytes                                # window read, volume read, volume written
    moved_c = nwin * 5 * window_bytes                              # + torch.flip: window read, flipped copy written
    print(json.dumps({
        "mirror_axes": list(args.mirror), "masks": list(masks), "mode": args.mode,
        "plan": {"padded": list(padded), "channels": Cn, "roi": list(roi), "windows": nwin, "sw_batch": args.sw_batch,
                 "calls": len(calls)},
        "clocks": clocks(), "device": torch.cuda.get_device_name(dev), "warmup": args.warmup, "repeats": args.repeats,
        "a_unmirrored_seconds": spread("a"),
        "b_mirrored_seconds": {str(f): spread(f"b{f}") for f in masks},
        "c_flip_then_unmirrored_seconds": {str(f): spread(f"c{f}") for f in masks},
        "microseconds_per_window": {"a": 1e6 * med["a"] / nwin, **{f"b{f}": 1e6 * med[f"b{f}"] / nwin for f in masks},
                                    **{f"c{f}": 1e6 * med[f"c{f}"] / nwin for f in masks}},
        "bytes_moved_derived": {"a_and_b": moved, "c_flipped_masks": moved_c},
        "bytes_per_second": {"a": moved / med["a"], **{f"b{f}": moved / med[f"b{f}"] for f in masks}},
        "b_over_a": {str(f): med[f"b{f}"] / med["a"] for f in masks},
        "b_over_c": {str(f): med[f"b{f}"] / med[f"c{f}"] for f in masks},
    }))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--volume", type=int, nargs=3, default=[240, 240, 180])
    ap.add_argument("--channels", type=int, default=16)
    ap.add_argument("--roi", type=int, default=96)
    ap.add_argument("--overlap", type=float, default=0.8)
    ap.add_argument("--sw-batch", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--mode", choices=["constant", "gaussian"], default="constant")
    ap.add_argument("--sigma-scale", type=float, default=0.125)
    ap.add_argument("--mirror", type=lambda t: tuple(int(v) for v in t.split(",")), default=None, metavar="AXES")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_blend.py measures on an MI355X; no GPU here")
    dev = torch.device("cuda", 0)
    Cn, roi = args.channels, (args.roi,) * 3
    probe = torch.empty(1, 1, *args.volume, device="meta")
    spatial, roi, padded, pad, starts = _plan(probe, roi, args.overlap)
    nwin = len(starts)
    g = torch.Generator(device=dev).manual_seed(0)
    pool = torch.randn(args.sw_batch, Cn, *roi, generator=g, device=dev)
    labels = (torch.rand(1, Cn, *spatial, generator=g, device=dev) > 0.6).float()
    table = window_table(starts, 1, dev)
    cov = [torch.tensor(n, dtype=torch.int32, device=dev) for n in coverage_counts(padded, roi, starts)]
    crop_lo = tuple(pad[2 * (2 - k)] for k in range(3))
    calls = [(g0, min(args.sw_batch, nwin - g0)) for g0 in range(0, nwin, args.sw_batch)]
    listed_windows = [(g0 + k, pool[k:k + 1]) for g0, nb in calls for k in range(nb)]

    gaussian = args.mode == "gaussian"
    vectors = importance_vectors(roi, args.mode, args.sigma_scale)
    weights = (*(v.to(dev) for v in vectors[:3]), vectors[3])
    wmap = importance_map(vectors, dev) if gaussian else None
    per_axis = [torch.tensor(s, dtype=torch.int32, device=dev) for s in axis_starts(starts)]

    if args.mirror is not None:
        return mirror_bench(args, dev, pool, table, calls, weights if gaussian else None, Cn, roi, padded, nwin)

    def streamed(weights=None):
        acc = ops.zeros((1, Cn, *padded), torch.float32, dev)
        for g0, nb in calls:
            ops.blend_accumulate(acc, pool[:nb], table, g0, weights=weights)
        divisor = cov if weights is None else ops.blend_weight_sum(per_axis, roi, padded, weights)
        _, mask, tallies = ops.blend_finish(acc, divisor, crop_lo, spatial, want_mask=True, labels=labels)
        return mask, ops.dice_from_tallies(tallies)

    def streamed_gaussian():
        return streamed(weights)

    def listed():
        q = _blend(listed_windows, 1, Cn, padded, roi, starts, pad, spatial, dev, torch.float32, wmap)
        mask = binarise(q)
        return mask, dice_per_class(mask, labels), q

    def run(fn):
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, torch.cuda.max_memory_allocated(dev) - base, out

    for _ in range(args.warmup):
        run(streamed); run(listed)
        if gaussian:
            run(streamed_gaussian)
    ts, tl, ps, pl, tc = [], [], [], [], []
    for _ in range(args.repeats):                                  # alternate the forms
        if gaussian:
            tc.append(run(streamed)[0])
        t, p, (mask_s, dice_s) = run(streamed_gaussian if gaussian else streamed)
        ts.append(t); ps.append(p)
        t, p, (mask_l, dice_l, q) = run(listed)
        tl.append(t); pl.append(p)
    outside = q.abs() > 2.0 ** -20
    agree = bool(torch.equal(mask_s.float()[outside], mask_l[outside]))
    window_bytes = Cn * roi[0] * roi[1] * roi[2] * 4
    volume_bytes = Cn * padded[0] * padded[1] * padded[2] * 4
    out_vox = Cn * spatial[0] * spatial[1] * spatial[2]
    moved = nwin * 3 * window_bytes + volume_bytes + volume_bytes + out_vox * (1 + 4)       # accumulate; zero fill; finish
    if gaussian:                                                   # wsum written once, read once by the finish pass
        moved += 2 * (volume_bytes // Cn)
    med_s, med_l = statistics.median(ts), statistics.median(tl)
    print(json.dumps({
        "plan": {"volume": list(spatial), "padded": list(padded), "channels": Cn, "roi": list(roi), "overlap": args.overlap,
                 "windows": nwin, "sw_batch": args.sw_batch, "calls": len(calls)},
        "mode": args.mode, "sigma_scale": args.sigma_scale,
        **({"streamed_constant_seconds": {"median": statistics.median(tc), "min": min(tc), "max": max(tc)}} if gaussian else {}),
        "clocks": clocks(), "device": torch.cuda.get_device_name(dev), "warmup": args.warmup, "repeats": args.repeats,
        "streamed_seconds": {"median": med_s, "min": min(ts), "max": max(ts)},
        "listed_seconds": {"median": med_l, "min": min(tl), "max": max(tl)},
        "streamed_peak_bytes": max(ps), "listed_peak_bytes": max(pl),
        "listed_window_list_bytes_derived": nwin * window_bytes,
        "streamed_bytes_moved_derived": moved, "streamed_bytes_per_second": moved / med_s,
        "masks_agree_outside_band": agree, "voxels_in_band": int((~outside).sum()),
        "dice_streamed": [round(float(v), 6) for v in dice_s.tolist()], "dice_listed": [round(float(v), 6) for v in dice_l.tolist()],
    }))
    for world in (2, 4, 8):
        b = blend_traffic_bytes(nwin, Cn, roi, 1, padded, world)
        print(json.dumps({"ranks": world, "gathered_bytes_per_rank_derived": b["gathered"], "reduced_bytes_per_rank_derived": b["reduced"]}))


if __name__ == "__main__":
    main()
