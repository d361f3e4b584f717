"""Time DeviceBatchProducer.next (csrc/augment.hip) against a torch-operator restatement of the same contract.

    python tools/bench_augment.py [--repeats 1000] [--warmup 20] [--rounds 7] [--with-step] [--out profiles/augment_bench.json]

For B in {1, 2, 10} at roi 96^3 and 16 classes over eight synthetic volumes of about 200 x 160 x 160 resident on the device:
``next`` into preallocated outputs, and the torch restatement a user would otherwise write (slice, flip, rot90, the two
intensity operations, a stacked == for the one-hot) from the same params on the same device in the same process.  The two are
timed in alternating rounds (``--rounds`` of ``--repeats`` calls each, device events around a whole round, after warm-up of
both); the statistic is the median round, the spread its min .. max.  The restatement gets its params from the host (the
producer's own rows, read back before the timed window), as a torch user's would be.  Achieved write bandwidth = the bytes
the outputs hold, 4 (1 + C) per voxel, over the median call time; ``apply`` alone is timed the same way.  ``--with-step``
adds one training step of NativeConvTrainer (graph mode, fp16, batch 2, 96^3, 16 classes: BASELINE config 4) on synthetic
inputs.  One JSON line at the end, also written to ``--out``.

    python tools/bench_augment.py --smoothing [--onehot-lib other/libdua_hip.so] [--rounds 21] [--repeats 200]

``--smoothing`` times, instead, the centroid-distance smoothed ``apply`` next to the one-hot ``apply`` at B = 2, roi 96^3 and
C = 13 and 15 channels (``class_ids = range(1, K)``, K = 14 and 16), same params, same outputs, alternating rounds in one
process.  The one-hot side is ``dua_aug_apply`` of ``--onehot-lib`` (default: the library ``DUA_HIP_LIB`` names, else the
package's own), loaded next to the package's library, so that the smoothed kernel of this tree is measured against the one-hot
kernel of another build.  Both write the same bytes, 4 (1 + C) per voxel.  It also times the once-per-volume centroid pass
(``dua_aug_class_centroids``) next to ``dua_aug_count_candidates`` on a 512 x 512 x 150 label map.

    python tools/bench_augment.py --affine [--rounds 21] [--repeats 200]

``--affine`` times, at the producer's own shape (B = 2, roi 96^3, 15 channels, ``class_ids = range(1, 16)``), the plain ``apply``
(``dua_aug_apply``), the resampling ``apply`` with a rotation of up to 30 degrees about every axis and a zoom from (0.7, 1.4) in
every row (``dua_aug_apply_affine``), and the same batch from torch operators (``affine_grid`` + ``grid_sample`` on the whole
volume, bilinear for the image and nearest for a float copy of the label map made beforehand, then flips, rot90, the intensity
operations and a stacked == for the one-hot), alternating rounds in one process.  All three write the same bytes, 4 (1 + C) per
voxel; each time is printed beside the bandwidth that makes of them.

    python tools/bench_augment.py --intensity [--rounds 21] [--repeats 200] [--with-step] [--out profiles/augment_bench.json]

``--intensity`` times the intensity stage (``IntensityAugmenter``, csrc/augment_intensity.hip) at roi 96^3 for B = 2 and B = 4:
``next`` of a producer without it, with every event forced on in every row, and with nnU-Net's default probabilities; the stage
alone (``apply`` on fixed all-on rows, out of place); and the same contract from torch operators on the same rows, device and
process (``randn`` for the noise, three ``conv3d`` over a symmetrically padded patch for the blur, reductions for the statistics,
``pow``), alternating rounds.  The torch form's output is compared with the kernels' on rows without noise (torch's generator
draws other normals).  ``--with-step`` relates the all-on cost to one config-4 training step.  With ``--out`` naming the file of
the plain run, the result is stored under its key ``intensity``.

    python tools/bench_augment.py --classes [--parent-lib other/libdua_hip.so] [--rounds 21] [--repeats 200]

``--classes`` times the draw alone (one workgroup, no voxel is moved) at B = 2 and B = 16 over the same 16-class volumes in one
process: today's draw (``dua_aug_draw``), the draw with ``class_ratios="present", uniform_prob=0.67`` and with sixteen equal
ratios and no uniform event (``dua_aug_draw_classes``), and, with ``--parent-lib``, ``dua_aug_draw`` of another build of the
library loaded next to this one (the parent commit's), on the same table.  Two figures per form: the time of a call through
``ops`` into preallocated rows, which is mostly the host's, and the time per draw of a captured graph of 100 draws in a row,
which is the device's.  It also times the once-per-volume ``dua_aug_count_class_candidates`` beside ``dua_aug_count_candidates``
on one of the volumes and on a 512 x 512 x 150 label map.
"""
import argparse
import ctypes
import json
import os
import socket
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from diff_unet_amos_amd import augment  # noqa: E402

DEV = "cuda:0"
ROI, CLASSES = (96, 96, 96), 16


def block_labels(shape, classes, g):
    coarse = torch.randint(0, classes * 3, tuple(-(-s // 8) for s in shape), generator=g)
    coarse = torch.where(coarse < classes, coarse, torch.zeros_like(coarse))
    label = coarse.repeat_interleave(8, 0).repeat_interleave(8, 1).repeat_interleave(8, 2)
    return label[:shape[0], :shape[1], :shape[2]].to(torch.uint8).contiguous()


def volumes(n, classes=CLASSES, num_classes=None):
    out = []
    for i in range(n):
        g = torch.Generator().manual_seed(100 + i)
        shape = (200 + 4 * (i % 3), 160 + 3 * (i % 4), 160 + 5 * (i % 2))
        label = block_labels(shape, classes, g)
        out.append(augment.DeviceVolume(torch.rand(shape, generator=g) - 0.3, label, device=DEV, num_classes=num_classes))
    return out


def torch_next(vols, rows, class_ids, out_images, out_labels):
    """The contract of dua_aug_apply in torch operators, one sample at a time, from host rows."""
    for b, (vid, sd, sh, sw, flip, k, scale, shift) in enumerate(rows):
        v = vols[vid]
        win = (slice(sd, sd + ROI[0]), slice(sh, sh + ROI[1]), slice(sw, sw + ROI[2]))
        p, q = v.image[win], v.label[win]
        dims = [a for a in (0, 1, 2) if flip >> a & 1]
        if dims:
            p, q = p.flip(dims), q.flip(dims)
        if k:
            p, q = torch.rot90(p, k, (0, 1)), torch.rot90(q, k, (0, 1))
        out_images[b, 0] = p * (1.0 + scale) + shift
        torch.eq(q[None], class_ids, out=out_labels[b])
    return out_images, out_labels


def timed_rounds(fns, repeats, rounds):
    """Alternating rounds of ``repeats`` calls of each function; per-call milliseconds of every round, per function."""
    ms = [[] for _ in fns]
    for _ in range(rounds):
        for i, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(repeats):
                fn()
            e1.record()
            e1.synchronize()
            ms[i].append(e0.elapsed_time(e1) / repeats)
    return ms


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}


def train_step_ms(warmup, steps):
    from diff_unet_amos_amd.diff_unet import DiffUNet
    from diff_unet_amos_amd.training import NativeConvTrainer
    torch.manual_seed(0)
    net = DiffUNet(in_channels=1, out_channels=CLASSES).to(DEV)
    tr = NativeConvTrainer(net, graph=True)
    g = torch.Generator().manual_seed(1)
    image = torch.rand(2, 1, *ROI, generator=g).to(DEV)
    labels = (torch.rand(2, CLASSES, *ROI, generator=g) > 0.8).float().to(DEV)
    for _ in range(warmup):
        tr.step(image, labels)
    torch.cuda.synchronize()
    per = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        tr.step(image, labels)
        e1.record()
        e1.synchronize()
        per.append(e0.elapsed_time(e1))
    return summary(per)


def smoothing_bench(args):
    from diff_unet_amos_amd import _native as nv
    from diff_unet_amos_amd import ops
    path = args.onehot_lib or os.environ.get("DUA_HIP_LIB") or nv.LIB_PATH
    other = ctypes.CDLL(path)
    other.dua_aug_apply.restype, other.dua_aug_apply.argtypes = nv._SIGS["dua_aug_apply"]
    B = 2
    result = {"metric": "augment_smoothed_apply_time", "unit": "ms", "box": socket.gethostname(),
              "device": torch.cuda.get_device_name(0), "roi": ROI, "B": B, "repeats": args.repeats, "rounds": args.rounds,
              "onehot_lib": os.path.relpath(path), "channels": {}}
    for K in (14, 16):
        vols = volumes(args.volumes, classes=K, num_classes=K)
        ids = torch.tensor([i % len(vols) for i in range(B)], dtype=torch.int32, device=DEV)
        kw = dict(roi=ROI, class_ids=range(1, K), flip_prob=0.5, rot90_prob=0.5, scale_prob=0.5, seed=2)
        hard, soft = augment.DeviceBatchProducer(vols, **kw), augment.DeviceBatchProducer(vols, smoothing=augment.LabelSmoothing(), **kw)
        params = hard.draw(ids)
        out_images = torch.empty((B, 1) + ROI, device=DEV)
        out_labels = torch.empty((B, K - 1) + ROI, device=DEV)

        def onehot_fn():
            nv.check(other.dua_aug_apply(nv.ptr(hard.table), len(vols), nv.ptr(params), B, *ROI, nv.ptr(hard.class_table), K - 1,
                                         nv.ptr(out_images), nv.ptr(out_labels), nv.ptr(hard._status), nv.stream_ptr()), "dua_aug_apply")

        def smoothed_fn():
            soft.apply(params, out_images, out_labels)

        onehot_fn()
        same = bool(torch.equal(out_labels, hard.apply(params)[1]))          # the other build writes this build's one-hot bits
        for _ in range(args.warmup):
            onehot_fn(); smoothed_fn()
        torch.cuda.synchronize()
        ms_hard, ms_soft = timed_rounds((onehot_fn, smoothed_fn), args.repeats, args.rounds)
        nbytes = 4 * K * B * ROI[0] * ROI[1] * ROI[2]
        entry = {"onehot_apply": summary(ms_hard), "smoothed_apply": summary(ms_soft), "bytes_written": nbytes,
                 "onehot_equal_between_builds": same,
                 "onehot_write_GBps": nbytes / (statistics.median(ms_hard) * 1e-3) / 1e9,
                 "smoothed_write_GBps": nbytes / (statistics.median(ms_soft) * 1e-3) / 1e9,
                 "smoothed_over_onehot": statistics.median(ms_soft) / statistics.median(ms_hard)}
        result["channels"][str(K - 1)] = entry
        print(f"C={K - 1}: one-hot apply {entry['onehot_apply']['median_ms']:.4f} ms = {entry['onehot_write_GBps']:.0f} GB/s, smoothed "
              f"apply {entry['smoothed_apply']['median_ms']:.4f} ms ({entry['smoothed_apply']['min_ms']:.4f} .. "
              f"{entry['smoothed_apply']['max_ms']:.4f}) = {entry['smoothed_write_GBps']:.0f} GB/s: ratio "
              f"{entry['smoothed_over_onehot']:.3f}; one-hot bits equal between builds: {same}", flush=True)
        assert hard.status == 0 and soft.status == 0
        del vols, hard, soft
    # once per case: the centroid pass next to the candidate count, on a label map of the size of a BTCV scan
    g = torch.Generator().manual_seed(7)
    shape = (150, 512, 512)
    label = block_labels(shape, 14, g).to(DEV)
    image = (torch.rand(shape, generator=g) - 0.3).to(DEV)
    fns = (lambda: ops.aug_class_centroids(label, 14), lambda: ops.aug_count_candidates(image, label, 0.0))
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    ms_cen, ms_cnt = timed_rounds(fns, 20, args.rounds)
    result["per_volume"] = {"shape": shape, "class_centroids": summary(ms_cen), "count_candidates": summary(ms_cnt)}
    print(f"{shape}: class centroids {statistics.median(ms_cen):.4f} ms, candidate count {statistics.median(ms_cnt):.4f} ms", flush=True)
    result["value"] = result["channels"]["15"]["smoothed_apply"]["median_ms"]
    return result


def affine_bench(args):
    import math
    import torch.nn.functional as F
    B, K = 2, 16
    vols = volumes(args.volumes, classes=K)
    ids = torch.tensor([i % len(vols) for i in range(B)], dtype=torch.int32, device=DEV)
    kw = dict(roi=ROI, class_ids=range(1, K), flip_prob=0.5, rot90_prob=0.5, scale_prob=0.5, seed=2)
    plain = augment.DeviceBatchProducer(vols, **kw)
    turned = augment.DeviceBatchProducer(vols, rotate_prob=1.0, rotate_range=(math.radians(30),) * 3, zoom_prob=1.0,
                                         zoom_range=(0.7, 1.4), **kw)
    params, affine = turned.draw(ids)
    out_images = torch.empty((B, 1) + ROI, device=DEV)
    out_labels = torch.empty((B, K - 1) + ROI, device=DEV)
    ref_images, ref_labels = torch.empty_like(out_images), torch.empty_like(out_labels)
    class_ids = torch.arange(1, K, dtype=torch.float32, device=DEV).view(-1, 1, 1, 1)
    # what a torch user prepares once: float label maps, and per sample the theta of affine_grid from the host rows
    label_f = [v.label.float()[None, None] for v in vols]
    ints, floats = augment.split_params(params.cpu())
    matrix = augment.split_affine(affine.cpu())[0].double()
    rows = []
    for (vid, sd, sh, sw, flip, k), (scale, shift), m in zip(ints.tolist(), floats.tolist(), matrix):
        size, start = vols[vid].shape, (sd, sh, sw)
        theta = torch.zeros(3, 4, dtype=torch.float64)
        for a in range(3):                                  # index order d, h, w; affine_grid wants x = w first
            for c in range(3):
                theta[2 - a, 2 - c] = m[a, c] * (ROI[c] - 1) / (size[a] - 1)
            theta[2 - a, 3] = 2.0 * (start[a] + (ROI[a] - 1) / 2) / (size[a] - 1) - 1.0
        rows.append((vid, flip, k, scale, shift, theta.float()[None].to(DEV)))

    def torch_fn():
        for b, (vid, flip, k, scale, shift, theta) in enumerate(rows):
            grid = F.affine_grid(theta, (1, 1) + ROI, align_corners=True)
            p = F.grid_sample(vols[vid].image[None, None], grid, mode="bilinear", padding_mode="zeros", align_corners=True)[0, 0]
            q = F.grid_sample(label_f[vid], grid, mode="nearest", padding_mode="zeros", align_corners=True)[0, 0]
            dims = [a for a in (0, 1, 2) if flip >> a & 1]
            if dims:
                p, q = p.flip(dims), q.flip(dims)
            if k:
                p, q = torch.rot90(p, k, (0, 1)), torch.rot90(q, k, (0, 1))
            ref_images[b, 0] = p * (1.0 + scale) + shift
            ref_labels[b] = q[None] == class_ids

    def apply_fn():
        plain.apply(params, out_images, out_labels)

    def affine_fn():
        turned.apply(params, out_images, out_labels, affine=affine)

    affine_fn(); torch_fn()
    image_gap = float((out_images - ref_images).abs().max())
    label_gap = float((out_labels != ref_labels).float().mean())
    for _ in range(args.warmup):
        apply_fn(); affine_fn(); torch_fn()
    torch.cuda.synchronize()
    ms_apply, ms_affine, ms_torch = timed_rounds((apply_fn, affine_fn, torch_fn), args.repeats, args.rounds)
    nbytes = 4 * K * B * ROI[0] * ROI[1] * ROI[2]
    result = {"metric": "augment_affine_apply_time", "unit": "ms", "box": socket.gethostname(), "device": torch.cuda.get_device_name(0),
              "roi": ROI, "B": B, "channels": K - 1, "repeats": args.repeats, "rounds": args.rounds, "bytes_written": nbytes,
              "apply": summary(ms_apply), "affine_apply": summary(ms_affine), "torch_grid_sample": summary(ms_torch),
              "max_image_gap_to_torch": image_gap, "label_fraction_differing_from_torch": label_gap}
    for name in ("apply", "affine_apply", "torch_grid_sample"):
        result[name]["write_GBps"] = nbytes / (result[name]["median_ms"] * 1e-3) / 1e9
        print(f"{name}: {result[name]['median_ms']:.4f} ms ({result[name]['min_ms']:.4f} .. {result[name]['max_ms']:.4f}) for "
              f"{nbytes} bytes written = {result[name]['write_GBps']:.0f} GB/s", flush=True)
    result["affine_over_apply"] = result["affine_apply"]["median_ms"] / result["apply"]["median_ms"]
    result["torch_over_affine"] = result["torch_grid_sample"]["median_ms"] / result["affine_apply"]["median_ms"]
    print(f"affine / apply = {result['affine_over_apply']:.3f}; torch / affine = {result['torch_over_affine']:.1f}; against torch: max "
          f"image gap {image_gap:.2e}, {100 * label_gap:.4f} % of the label values differ (nearest-voxel ties)", flush=True)
    assert plain.status == 0 and turned.status == 0
    result["value"] = result["affine_apply"]["median_ms"]
    return result


def classes_bench(args):
    from diff_unet_amos_amd import _native as nv
    from diff_unet_amos_amd import ops
    K, GRAPH_DRAWS = 16, 100
    vols = volumes(args.volumes, classes=K, num_classes=K)
    kw = dict(roi=ROI, class_ids=range(1, K), seed=2)
    plain = augment.DeviceBatchProducer(vols, **kw)
    present = augment.DeviceBatchProducer(vols, class_ratios="present", uniform_prob=0.67, **kw)
    equal = augment.DeviceBatchProducer(vols, class_ratios=[1.0] * K, **kw)
    parent = None
    if args.parent_lib:
        parent = ctypes.CDLL(args.parent_lib)
        parent.dua_aug_draw.restype, parent.dua_aug_draw.argtypes = nv._SIGS["dua_aug_draw"]
    result = {"metric": "augment_class_draw_time", "unit": "ms", "box": socket.gethostname(), "device": torch.cuda.get_device_name(0),
              "classes": K, "volumes": len(vols), "repeats": args.repeats, "rounds": args.rounds, "graph_draws": GRAPH_DRAWS,
              "parent_lib": os.path.relpath(args.parent_lib) if args.parent_lib else None, "batches": {}}
    for B in (2, 16):
        ids = torch.tensor([i % len(vols) for i in range(B)], dtype=torch.int32, device=DEV)
        params = torch.empty((B, 8), dtype=torch.int32, device=DEV)
        chosen = torch.empty(B, dtype=torch.int32, device=DEV)

        def plain_fn():
            ops.aug_draw(plain.table, ids, plain.cfg, plain.seed, plain._counter, params, plain._status)

        def class_fn(p):
            return lambda: ops.aug_draw_classes(p.table, ids, p.cfg, p.seed, p._counter, params, p._status, class_table=p.class_draw_table,
                                                num_classes=K, uniform_prob=p.uniform_prob, chosen=chosen, tally=p.class_tally)

        def parent_fn():
            nv.check(parent.dua_aug_draw(nv.ptr(plain.table), len(vols), nv.ptr(ids), B, ctypes.byref(plain.cfg), plain.seed,
                                         nv.ptr(plain._counter), 0, 0, nv.ptr(params), nv.ptr(plain._status), nv.stream_ptr()), "dua_aug_draw")

        fns = {"draw": plain_fn, "draw_classes_present_uniform_0.67": class_fn(present), "draw_classes_equal_ratios": class_fn(equal)}
        if parent is not None:
            fns["parent_draw"] = parent_fn
        if parent is not None:                                 # the two builds write the same rows for one counter
            plain._counter.zero_(); plain_fn(); mine = params.clone()
            plain._counter.zero_(); parent_fn()
            assert torch.equal(mine, params), "dua_aug_draw differs between the two builds"
        graphs = {}
        for name, fn in fns.items():
            for _ in range(args.warmup):
                fn()
            torch.cuda.synchronize()
            graph, stream = torch.cuda.CUDAGraph(), torch.cuda.Stream(device=DEV)
            stream.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(stream):
                with torch.cuda.graph(graph, stream=stream):
                    for _ in range(GRAPH_DRAWS):
                        fn()
            torch.cuda.current_stream().wait_stream(stream)
            graph.replay()
            graphs[name] = graph
        torch.cuda.synchronize()
        names = list(fns)
        ms_call = timed_rounds([fns[n] for n in names], args.repeats, args.rounds)
        ms_graph = timed_rounds([graphs[n].replay for n in names], max(args.repeats // GRAPH_DRAWS, 2), args.rounds)
        entry = {}
        for n, c, g in zip(names, ms_call, ms_graph):
            entry[n] = {"call": summary(c), "in_graph": summary([x / GRAPH_DRAWS for x in g])}
            print(f"B={B} {n}: call {entry[n]['call']['median_ms'] * 1e3:.2f} us ({entry[n]['call']['min_ms'] * 1e3:.2f} .. "
                  f"{entry[n]['call']['max_ms'] * 1e3:.2f}); per draw inside a graph of {GRAPH_DRAWS}: "
                  f"{entry[n]['in_graph']['median_ms'] * 1e3:.2f} us ({entry[n]['in_graph']['min_ms'] * 1e3:.2f} .. "
                  f"{entry[n]['in_graph']['max_ms'] * 1e3:.2f})", flush=True)
        result["batches"][str(B)] = entry
        assert plain.status == 0 and present.status == 0 and equal.status == 0
    # once per case: the class tables beside the pos / neg tables, on a producer volume and on a label map of the size of a scan
    g = torch.Generator().manual_seed(7)
    shape = (150, 512, 512)
    big_label = block_labels(shape, K, g).to(DEV)
    big_image = (torch.rand(shape, generator=g) - 0.3).to(DEV)
    result["per_volume"] = {}
    for name, image, label in (("producer_volume", vols[0].image, vols[0].label), ("scan", big_image, big_label)):
        fns = (lambda: ops.aug_count_class_candidates(image, label, K, 0.0), lambda: ops.aug_count_candidates(image, label, 0.0))
        for fn in fns:
            fn()
        torch.cuda.synchronize()
        ms_cls, ms_cnt = timed_rounds(fns, 20, args.rounds)
        result["per_volume"][name] = {"shape": tuple(image.shape), "count_class_candidates": summary(ms_cls),
                                      "count_candidates": summary(ms_cnt)}
        print(f"{tuple(image.shape)}: class tables {statistics.median(ms_cls):.4f} ms ({min(ms_cls):.4f} .. {max(ms_cls):.4f}), pos / neg "
              f"tables {statistics.median(ms_cnt):.4f} ms ({min(ms_cnt):.4f} .. {max(ms_cnt):.4f})", flush=True)
    result["value"] = result["batches"]["2"]["draw_classes_present_uniform_0.67"]["in_graph"]["median_ms"]
    return result


def torch_intensity(images, rows, out):
    """The contract of dua_aug_intensity_apply in whole-tensor torch operators, one sample at a time, from host rows
    (events, std, sigma, brightness, contrast, gamma)."""
    import torch.nn.functional as F
    for b, (mask, std, sigma, bright, contrast, gamma) in enumerate(rows):
        x = images[b:b + 1]
        if mask & 1:
            x = x + std * torch.randn_like(x)
        if mask & 2:
            R = int(4.0 * sigma + 0.5)
            i = torch.arange(-R, R + 1, dtype=torch.float64)
            k = torch.exp(-(i * i) / (2.0 * sigma * sigma))
            k = (k / k.sum()).float().to(x.device)
            for dim in (4, 3, 2):
                n, shape = x.shape[dim], [1, 1, 1, 1, 1]
                shape[dim] = 2 * R + 1
                x = torch.cat([x.narrow(dim, 0, R).flip(dim), x, x.narrow(dim, n - R, R).flip(dim)], dim=dim)
                x = F.conv3d(x, k.reshape(shape))
        if mask & 4:
            x = x * bright
        if mask & 8:
            m, lo, hi = x.mean(), x.min(), x.max()
            x = torch.minimum(torch.maximum((x - m) * contrast + m, lo), hi)
        if mask & 16:
            if mask & 32:
                x = -x
            m, s, lo, hi = x.mean(), x.std(unbiased=False), x.min(), x.max()
            y = torch.pow((x - lo) / ((hi - lo) + 1e-7), gamma) * (hi - lo) + lo
            x = (y - y.mean()) / (y.std(unbiased=False) + 1e-8) * s + m
            if mask & 32:
                x = -x
        out[b:b + 1] = x
    return out


def intensity_bench(args):
    forced = dict(noise_prob=1.0, blur_prob=1.0, brightness_prob=1.0, contrast_prob=1.0, gamma_prob=1.0)
    vols = volumes(args.volumes)
    result = {"metric": "augment_intensity_time", "unit": "ms", "box": socket.gethostname(), "device": torch.cuda.get_device_name(0),
              "roi": ROI, "classes": CLASSES, "repeats": args.repeats, "rounds": args.rounds, "batches": {}}
    for B in (2, 4):
        ids = torch.tensor([i % len(vols) for i in range(B)], dtype=torch.int32, device=DEV)
        kw = dict(roi=ROI, class_ids=range(CLASSES), seed=1)
        plain = augment.DeviceBatchProducer(vols, **kw)
        all_on = augment.DeviceBatchProducer(vols, intensity=augment.IntensityAugmenter(ROI, seed=3, device=DEV, **forced), **kw)
        default = augment.DeviceBatchProducer(vols, intensity=augment.IntensityAugmenter(ROI, seed=3, device=DEV), **kw)
        out_images = torch.empty((B, 1) + ROI, device=DEV)
        out_labels = torch.empty((B, CLASSES) + ROI, device=DEV)
        images = plain.next(ids)[0].clone()
        stage = augment.IntensityAugmenter(ROI, seed=3, device=DEV, **forced)
        rows = stage.draw(B)
        stage_out, torch_out = torch.empty_like(images), torch.empty_like(images)
        names = augment.split_intensity(rows)
        host = list(zip(names["events"].tolist(), *[names[k].tolist() for k in ("noise_std", "blur_sigma", "brightness", "contrast", "gamma")]))
        # the two forms on the same rows without the noise: what remains is rounding
        quiet = rows.clone()
        quiet_bits = quiet.view(torch.int32)
        quiet_bits[:, 0] &= ~1
        stage.apply(images, quiet, out=stage_out)
        torch_intensity(images, [(m & ~1, *r) for (m, *r) in host], torch_out)
        gap = float((stage_out - torch_out).abs().max())

        fns = (lambda: plain.next(ids, out_images, out_labels), lambda: all_on.next(ids, out_images, out_labels),
               lambda: default.next(ids, out_images, out_labels), lambda: stage.apply(images, rows, out=stage_out),
               lambda: torch_intensity(images, host, torch_out))
        for _ in range(args.warmup):
            for fn in fns:
                fn()
        torch.cuda.synchronize()
        ms = timed_rounds(fns, args.repeats, args.rounds)
        keys = ("next_plain", "next_all_on", "next_default_probabilities", "stage_all_on", "torch_operators_all_on")
        entry = {k: summary(m) for k, m in zip(keys, ms)}
        entry["all_on_cost_ms"] = entry["next_all_on"]["median_ms"] - entry["next_plain"]["median_ms"]
        entry["default_cost_ms"] = entry["next_default_probabilities"]["median_ms"] - entry["next_plain"]["median_ms"]
        entry["torch_over_stage"] = entry["torch_operators_all_on"]["median_ms"] / entry["stage_all_on"]["median_ms"]
        entry["max_gap_to_torch_without_noise"] = gap
        result["batches"][str(B)] = entry
        for k in keys:
            print(f"B={B} {k}: {entry[k]['median_ms']:.4f} ms ({entry[k]['min_ms']:.4f} .. {entry[k]['max_ms']:.4f})", flush=True)
        print(f"B={B}: all-on stage inside next costs {entry['all_on_cost_ms']:.4f} ms, with the default probabilities "
              f"{entry['default_cost_ms']:.4f} ms; torch operators / stage = {entry['torch_over_stage']:.1f}; max gap to torch without "
              f"noise {gap:.2e}", flush=True)
        assert plain.status == 0 and all_on.status == 0 and default.status == 0
    if args.with_step:
        result["train_step"] = train_step_ms(5, 20)
        result["all_on_B2_share_of_step"] = result["batches"]["2"]["all_on_cost_ms"] / result["train_step"]["median_ms"]
        print(f"training step (graph, fp16, batch 2): {result['train_step']['median_ms']:.2f} ms; the all-on stage at B=2 is "
              f"{100 * result['all_on_B2_share_of_step']:.2f} % of it", flush=True)
    result["value"] = result["batches"]["2"]["stage_all_on"]["median_ms"]
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--volumes", type=int, default=8)
    ap.add_argument("--with-step", action="store_true")
    ap.add_argument("--out", default="")
    ap.add_argument("--smoothing", action="store_true", help="smoothed apply next to the one-hot apply, and the centroid pass")
    ap.add_argument("--onehot-lib", default="", help="with --smoothing: the build whose dua_aug_apply is the one-hot side")
    ap.add_argument("--affine", action="store_true", help="resampling apply next to the plain apply and to torch's grid_sample")
    ap.add_argument("--classes", action="store_true", help="the draw with class ratios next to the draw without, and the class tables")
    ap.add_argument("--parent-lib", default="", help="with --classes: another build of the library whose dua_aug_draw is timed beside")
    ap.add_argument("--intensity", action="store_true", help="the intensity stage next to next() without it and to torch operators")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_augment.py measures on the GPU; none is visible")
    if args.intensity:
        result = intensity_bench(args)
        if args.out:
            merged = result
            if os.path.exists(args.out):
                with open(args.out) as f:
                    before = json.loads(f.read() or "{}")
                if before.get("metric") == "augment_next_time":
                    merged = dict(before, intensity=result)
            with open(args.out, "w") as f:
                f.write(json.dumps(merged) + "\n")
        print(json.dumps(result))
        return
    if args.smoothing or args.affine or args.classes:
        line = json.dumps(smoothing_bench(args) if args.smoothing else affine_bench(args) if args.affine else classes_bench(args))
        if args.out:
            with open(args.out, "w") as f:
                f.write(line + "\n")
        print(line)
        return
    vols = volumes(args.volumes)
    prod = augment.DeviceBatchProducer(vols, roi=ROI, class_ids=range(CLASSES), seed=1)
    class_ids = torch.arange(CLASSES, dtype=torch.uint8, device=DEV).view(-1, 1, 1, 1)
    result = {"metric": "augment_next_time", "unit": "ms", "box": socket.gethostname(), "device": torch.cuda.get_device_name(0),
              "roi": ROI, "classes": CLASSES, "repeats": args.repeats, "rounds": args.rounds, "batches": {}}
    for B in (1, 2, 10):
        ids = torch.tensor([i % len(vols) for i in range(B)], dtype=torch.int32, device=DEV)
        out_images = torch.empty((B, 1) + ROI, device=DEV)
        out_labels = torch.empty((B, CLASSES) + ROI, device=DEV)
        ref_images, ref_labels = torch.empty_like(out_images), torch.empty(out_labels.shape, dtype=torch.bool, device=DEV)
        ref_float = torch.empty_like(out_labels)
        # rows with every kind of transform in them (the default probabilities leave most samples untouched)
        busy = augment.DeviceBatchProducer(vols, roi=ROI, class_ids=range(CLASSES), flip_prob=0.5, rot90_prob=0.5, scale_prob=0.5,
                                           seed=2)
        params = busy.draw(ids)
        ints, floats = augment.split_params(params.cpu())
        rows = [tuple(i) + tuple(f) for i, f in zip(ints.tolist(), floats.tolist())]

        def torch_fn():
            torch_next(vols, rows, class_ids, ref_images, ref_labels)
            ref_float.copy_(ref_labels)                      # the trainer takes fp32 one-hot channels

        def next_fn():
            prod.next(ids, out_images, out_labels)

        def apply_fn():
            busy.apply(params, out_images, out_labels)

        # same tensors from both before anything is timed
        apply_fn(); torch_fn()
        same = bool(torch.equal(out_images, ref_images)) and bool(torch.equal(out_labels, ref_float))
        for _ in range(args.warmup):
            next_fn(); apply_fn(); torch_fn()
        torch.cuda.synchronize()
        ms_next, ms_apply, ms_torch = timed_rounds((next_fn, apply_fn, torch_fn), args.repeats, args.rounds)
        nbytes = 4 * (1 + CLASSES) * B * ROI[0] * ROI[1] * ROI[2]
        entry = {"next": summary(ms_next), "apply": summary(ms_apply), "torch_restatement": summary(ms_torch),
                 "outputs_equal_torch": same, "bytes_written": nbytes,
                 "next_write_GBps": nbytes / (statistics.median(ms_next) * 1e-3) / 1e9,
                 "apply_write_GBps": nbytes / (statistics.median(ms_apply) * 1e-3) / 1e9,
                 "torch_over_next": statistics.median(ms_torch) / statistics.median(ms_next)}
        result["batches"][str(B)] = entry
        print(f"B={B}: next {entry['next']['median_ms']:.4f} ms ({entry['next']['min_ms']:.4f} .. {entry['next']['max_ms']:.4f}), "
              f"apply alone {entry['apply']['median_ms']:.4f} ms = {entry['apply_write_GBps']:.0f} GB/s written, torch restatement "
              f"{entry['torch_restatement']['median_ms']:.4f} ms ({entry['torch_restatement']['min_ms']:.4f} .. "
              f"{entry['torch_restatement']['max_ms']:.4f}) = {entry['torch_over_next']:.1f}x; outputs equal: {same}", flush=True)
    assert prod.status == 0
    if args.with_step:
        result["train_step"] = train_step_ms(5, 20)
        result["next_B2_share_of_step"] = result["batches"]["2"]["next"]["median_ms"] / result["train_step"]["median_ms"]
        print(f"training step (graph, fp16, batch 2): {result['train_step']['median_ms']:.2f} ms; next at B=2 is "
              f"{100 * result['next_B2_share_of_step']:.2f} % of it", flush=True)
    result["value"] = result["batches"]["2"]["next"]["median_ms"]
    line = json.dumps(result)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
