"""Signed distance maps of a label batch (ops.signed_distance_maps, csrc/sdf.hip) at the training shape: 2 x 16 volumes of 96^3,
argmax-partition labels (every voxel one-hot in the class of the nearest of C seeds: blobs, the distances a real label map has).
Times a warm loop with device events, several rounds; reports milliseconds (median and minimum over the rounds), the bytes the
three passes move (6 words per voxel: labels in, word out; word in, word out; word in, phi out) over that time, the same against
the minimum any implementation moves (labels in, phi out), and -- as context, not as a comparison of like with like -- the time
scipy.ndimage.distance_transform_edt takes for the same maps on the host (two transforms per volume), serial and on a pool of
processes, measured BEFORE the device is touched.  The maps of the first sample are checked against scipy's.  One JSON line.
Usage: python tools/bench_sdf.py [--batch 2] [--classes 16] [--size 96] [--repeats 20] [--rounds 5] [--procs 16] [--no-scipy]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def partition_labels(batch, classes, size, seed=0):
    """fp32 [batch, classes, size, size, size] one-hot: each voxel belongs to the nearest of ``classes`` random seeds."""
    rng = np.random.RandomState(seed)
    z, h, w = np.ogrid[:size, :size, :size]
    y = np.zeros((batch, classes, size, size, size), np.float32)
    for n in range(batch):
        seeds = rng.randint(size, size=(classes, 3))
        dist = np.stack([(z - s[0]) ** 2 + (h - s[1]) ** 2 + (w - s[2]) ** 2 for s in seeds])
        y[n] = np.arange(classes)[:, None, None, None] == dist.argmin(0)[None]
    return y


def scipy_phi(mask):
    """Kervadec's map of one volume in fp64 (0 for an empty or full mask), by two scipy transforms."""
    from scipy import ndimage
    if not mask.any() or mask.all():
        return np.zeros(mask.shape)
    return np.where(mask, 1.0 - ndimage.distance_transform_edt(mask), ndimage.distance_transform_edt(~mask))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--classes", type=int, default=16)
    ap.add_argument("--size", type=int, default=96)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--procs", type=int, default=16, help="processes of the scipy pool (host context)")
    ap.add_argument("--no-scipy", action="store_true")
    a = ap.parse_args()
    y = partition_labels(a.batch, a.classes, a.size)
    masks = [y[n, c] > 0.5 for n in range(a.batch) for c in range(a.classes)]
    host = None
    if not a.no_scipy:
        import multiprocessing as mp
        t0 = time.perf_counter()
        ref0 = [scipy_phi(m) for m in masks[:a.classes]]
        serial = (time.perf_counter() - t0) * len(masks) / a.classes
        with mp.get_context("fork").Pool(a.procs) as pool:          # before the device is touched: the children never see it
            pool.map(scipy_phi, masks[:a.procs])
            t0 = time.perf_counter()
            pool.map(scipy_phi, masks)
            pooled = time.perf_counter() - t0
        host = {"scipy_serial_ms": round(serial * 1e3, 1), "scipy_pool_ms": round(pooled * 1e3, 1), "pool_processes": a.procs}
    from diff_unet_amos_amd import ops
    dev = torch.device("cuda:0")
    labels = torch.from_numpy(y).to(dev)
    phi = torch.empty_like(labels)
    scratch = torch.empty(labels.numel(), dtype=torch.int32, device=dev)
    for _ in range(a.warmup):
        ops.signed_distance_maps(labels, out=phi, scratch=scratch)
    torch.cuda.synchronize()
    if host is not None:
        err = max(float(np.abs(phi[0, c].cpu().numpy().astype(np.float64) - ref0[c]).max()) for c in range(a.classes))
        assert err <= 2.0 ** -23 * a.size * 2, err
        host["max_abs_difference_to_scipy_sample0"] = err
    rounds = []
    for _ in range(a.rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.repeats):
            ops.signed_distance_maps(labels, out=phi, scratch=scratch)
        e1.record()
        torch.cuda.synchronize()
        rounds.append(e0.elapsed_time(e1) / a.repeats)
    med, best = sorted(rounds)[len(rounds) // 2], min(rounds)
    moved, least = 6 * labels.numel() * 4, 2 * labels.numel() * 4
    out = {"metric": "signed_distance_maps_time", "value": med, "unit": "ms", "min_ms": best, "rounds_ms": [round(x, 4) for x in rounds],
           "shape": list(labels.shape), "labels": "argmax partition into C blobs", "repeats": a.repeats, "rounds": a.rounds,
           "bytes_moved": moved, "moved_gbytes_per_s": round(moved / med / 1e6, 1), "bytes_minimum": least,
           "minimum_gbytes_per_s": round(least / med / 1e6, 1), "device": torch.cuda.get_device_name(0), "host": host}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
