"""Time case preparation (csrc/volume_prep.hip) against the same preparation in torch operators.

    python tools/bench_prepare.py [--repeats 20] [--warmup 3] [--rounds 5] [--small] [--out profiles/prepare_bench.json]

One synthetic abdominal CT case, 512 x 512 x 200 int16 at 0.78 x 0.78 x 2.5 mm (an elliptic body of tissue and bone inside
air, a blocky label map), prepared to (1.5, 1.5, 2.0) mm "RAS" from three storage orders:

    identity : stored [x][y][z], axes already R, A, S -- the prepared W axis is the source's fastest axis;
    flipped  : the same array with an "LPS" affine -- the first two strides are negative;
    permuted : stored [z][y][x] (200 x 512 x 512) -- the prepared W axis has the source's largest stride.

Per case, in alternating rounds in one process (``--rounds`` of ``--repeats`` calls each, device events around a whole round,
after warm-up of both; the statistic is the median round, the spread its min .. max):

    box      : dua_prep_foreground_box (one pass over the whole source);
    resample : dua_prep_resample with its tables already on the device (image and label in one launch);
    torch    : what a user has today -- clamp of the window, slicing to the box, flip / permute, and F.grid_sample
               (bilinear, align_corners) for the image and (nearest) for the label over a grid built from the per-axis
               coordinates, on the same device.  Its box comes from the host (the native one, read back before the window).

Bytes moved by the resample = the source box once (image elements and label bytes) plus the outputs once (4 + 1 bytes per
voxel); by the box pass = the whole source once.  GB/s = those bytes over the median time, printed next to the 6.29 TB/s a
float4 copy reaches on this chip (the HBM figure to compare a streaming kernel with).  The native image is also compared with
torch's (max |d|: the two agree to fp32 rounding; grid_sample computes its own coordinates in fp32).  One JSON line at the
end, also written to ``--out``.
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
import torch.nn.functional as F  # noqa: E402

from diff_unet_amos_amd import ops, prepare  # noqa: E402

DEV = "cuda:0"
HBM_COPY_GBPS = 6290.0
A_MIN, A_MAX = -175.0, 250.0
PIXDIM = (1.5, 1.5, 2.0)


def synthetic_case(shape, g):
    """[x][y][z] int16: air outside an elliptic cylinder that leaves a margin on the first two axes, tissue and bone inside."""
    X, Y, Z = shape
    x = (torch.arange(X, dtype=torch.float32) - X / 2) / (0.42 * X)
    y = (torch.arange(Y, dtype=torch.float32) - Y / 2) / (0.33 * Y)
    body = (x[:, None] ** 2 + y[None, :] ** 2) < 1.0
    hu = torch.randint(-160, 320, shape, generator=g, dtype=torch.int16)
    image = torch.where(body[:, :, None], hu, torch.full_like(hu, -1000))
    coarse = torch.randint(0, 48, tuple(-(-s // 8) for s in shape), generator=g)
    coarse = torch.where(coarse < 16, coarse, torch.zeros_like(coarse))
    label = coarse.repeat_interleave(8, 0).repeat_interleave(8, 1).repeat_interleave(8, 2)[:X, :Y, :Z]
    label = torch.where(body[:, :, None], label, torch.zeros_like(label)).to(torch.uint8)
    return image.contiguous(), label.contiguous()


def torch_prepare(src, lab, geom):
    """The contract in torch operators on the device; the coordinates are the contract's (host fp64, rounded to fp32)."""
    sl = tuple(slice(lo, hi) for lo, hi in geom.box)
    img = ((src[sl].float() - A_MIN) / (A_MAX - A_MIN)).clamp_(0.0, 1.0).permute(geom.perm)
    lb = lab[sl].permute(geom.perm)
    dims = [j for j, f in enumerate(geom.flip) if f]
    if dims:
        img, lb = img.flip(dims), lb.flip(dims)
    axes = []
    for j in range(3):
        n_in = geom.n_in[j]
        x = torch.from_numpy(np.minimum(np.arange(geom.shape[j]) * geom.pixdim[j] / geom.s_in[j], n_in - 1)).to(src.device)
        axes.append((2.0 * x / max(n_in - 1, 1) - 1.0).float())
    gd, gh, gw = torch.meshgrid(*axes, indexing="ij")
    grid = torch.stack((gw, gh, gd), dim=-1)[None]                       # grid_sample wants (x = W, y = H, z = D)
    out = F.grid_sample(img[None, None].contiguous(), grid, mode="bilinear", padding_mode="border", align_corners=True)[0, 0]
    out_l = F.grid_sample(lb[None, None].float().contiguous(), grid, mode="nearest", padding_mode="border", align_corners=True)
    return out, out_l[0, 0].to(torch.uint8)


def timed(fn, repeats):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(repeats):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3 / repeats                      # microseconds per call


def stats(rounds):
    return dict(median_us=round(statistics.median(rounds), 2), min_us=round(min(rounds), 2), max_us=round(max(rounds), 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--small", action="store_true", help="a 96 x 96 x 40 case: a rehearsal of the tool, not a measurement")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_prepare: no GPU: nothing is measured on a CPU")
    g = torch.Generator().manual_seed(0)
    shape = (96, 96, 40) if args.small else (512, 512, 200)
    image, label = synthetic_case(shape, g)
    spacing = (0.78, 0.78, 2.5)
    cases = {
        "identity": (image, label, np.diag(spacing + (1.0,))),
        "flipped": (image, label, np.diag((-spacing[0], -spacing[1], spacing[2], 1.0))),
        "permuted": (image.permute(2, 1, 0).contiguous(), label.permute(2, 1, 0).contiguous(),
                     np.array([[0, 0, spacing[0], 0], [0, spacing[1], 0, 0], [spacing[2], 0, 0, 0], [0, 0, 0, 1.0]])),
    }
    result = dict(host=socket.gethostname(), device=torch.cuda.get_device_name(0), source=list(shape), dtype="int16",
                  spacing=list(spacing), pixdim=list(PIXDIM), hbm_float4_copy_gbps=HBM_COPY_GBPS, repeats=args.repeats,
                  rounds=args.rounds, cases={})
    for name, (img, lab, affine) in cases.items():
        src, src_l = img.to(DEV), lab.to(DEV)
        words = ops.prep_foreground_box(src, A_MIN).tolist()
        box = tuple((words[j], words[3 + j] + 1) for j in range(3))
        geom = prepare.prepared_geometry(tuple(src.shape), box, affine, PIXDIM)
        tables = ops.prep_upload_tables(geom, src.device)
        native = {"box": lambda: ops.prep_foreground_box(src, A_MIN),
                  "resample": lambda: ops.prep_resample(src, src_l, geom, A_MIN, A_MAX - A_MIN, tables=tables),
                  "torch": lambda: torch_prepare(src, src_l, geom)}
        got, got_l = native["resample"]()
        want, want_l = native["torch"]()
        diff = float((got - want).abs().max())
        label_mismatch = int((got_l != want_l).sum())
        del want, want_l
        for fn in native.values():
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        rounds = {k: [] for k in native}
        for _ in range(args.rounds):
            for k, fn in native.items():
                rounds[k].append(timed(fn, args.repeats))
        box_vox = int(np.prod([hi - lo for lo, hi in box]))
        out_vox = int(np.prod(geom.shape))
        resample_bytes = box_vox * (src.element_size() + 1) + out_vox * 5
        box_bytes = src.numel() * src.element_size()
        row = dict(source=list(src.shape), box=[list(b) for b in box], prepared=list(geom.shape), perm=list(geom.perm),
                   flip=list(geom.flip), stride=list(geom.stride), box_pass=stats(rounds["box"]), resample=stats(rounds["resample"]),
                   torch_operators=stats(rounds["torch"]), box_pass_bytes=box_bytes, resample_bytes=resample_bytes,
                   max_abs_diff_vs_torch=diff, label_mismatches_vs_torch=label_mismatch)
        row["box_pass_gbps"] = round(box_bytes / row["box_pass"]["median_us"] / 1e3, 1)
        row["resample_gbps"] = round(resample_bytes / row["resample"]["median_us"] / 1e3, 1)
        row["resample_share_of_hbm_copy"] = round(row["resample_gbps"] / HBM_COPY_GBPS, 3)
        row["torch_over_native"] = round(row["torch_operators"]["median_us"] /
                                         (row["box_pass"]["median_us"] + row["resample"]["median_us"]), 2)
        result["cases"][name] = row
        print(f"{name:9s} box {row['box_pass']['median_us']:9.1f} us ({row['box_pass_gbps']:7.1f} GB/s)  resample "
              f"{row['resample']['median_us']:9.1f} us ({row['resample_gbps']:7.1f} GB/s of {HBM_COPY_GBPS:.0f})  torch "
              f"{row['torch_operators']['median_us']:10.1f} us  prepared {geom.shape}  max |d| {diff:.2e}  label mismatches "
              f"{label_mismatch}", flush=True)
        del src, src_l, got, got_l, tables
        torch.cuda.empty_cache()
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
