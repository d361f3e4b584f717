"""Normalized Surface Dice (voxel-count form) restated in torch, independently of the kernels and of scipy: the erosion by padded
shifts, the squared distances by a brute-force minimum over all surface pairs from explicit squared differences in fp64, the
counts by d^2 <= tau^2, the empty rules.  The fixture tests/golden/surface_dice_golden.npz (tools/make_surface_dice_golden.py)
holds the same quantities computed with scipy."""
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "surface_dice_golden.npz")


def footprint(k):
    return [(dz, dy, dx) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)
            if 0 < (dz != 0) + (dy != 0) + (dx != 0) <= k]


def border(x, k):
    """x & ~erode(x): one binary erosion of a bool [D, H, W] tensor with generate_binary_structure(3, k), border_value 0."""
    D, H, W = x.shape
    p = torch.zeros((D + 2, H + 2, W + 2), dtype=torch.bool, device=x.device)
    p[1:-1, 1:-1, 1:-1] = x
    er = x.clone()
    for dz, dy, dx in footprint(k):
        er &= p[1 + dz:1 + dz + D, 1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
    return x & ~er


def directed_sq(ba, bb, spacing, chunk=2048):
    """For every voxel of ba (raster order), the fp64 squared distance to the nearest voxel of bb; +inf when bb is empty."""
    s = torch.tensor(spacing, dtype=torch.float64, device=ba.device)
    pa = ba.nonzero().double() * s
    pb = bb.nonzero().double() * s
    out = torch.full((pa.shape[0],), float("inf"), dtype=torch.float64, device=ba.device)
    if pb.shape[0] == 0:
        return out
    for i in range(0, pa.shape[0], chunk):
        q = pa[i:i + chunk]
        d2 = (q[:, None, 0] - pb[None, :, 0]) ** 2 + (q[:, None, 1] - pb[None, :, 1]) ** 2 + (q[:, None, 2] - pb[None, :, 2]) ** 2
        out[i:i + chunk] = d2.min(dim=1).values
    return out


def surface_dice_ref(a, b, tolerances, spacing=(1.0, 1.0, 1.0), k=1, nan_for_nonexisting=True):
    """One 3-D pair: dict(n_a, n_b ints; within_ab, within_ba lists of ints; nsd list of floats), one entry per tolerance."""
    a, b = a.bool(), b.bool()
    ba, bb = border(a, k), border(b, k)
    dab, dba = directed_sq(ba, bb, spacing), directed_sq(bb, ba, spacing)
    n_a, n_b = int(ba.sum()), int(bb.sum())
    wab, wba, nsd = [], [], []
    for tau in tolerances:
        t2 = float(tau) * float(tau)
        x, y = int((dab <= t2).sum()), int((dba <= t2).sum())
        wab.append(x); wba.append(y)
        if n_a + n_b == 0:
            nsd.append(float("nan") if nan_for_nonexisting else 0.0)
        else:
            nsd.append(float(np.float64(x + y) / np.float64(n_a + n_b)))
    return dict(n_a=n_a, n_b=n_b, within_ab=wab, within_ba=wba, nsd=nsd)


def golden():
    """(cases [(name, test bool tensor, reference bool tensor)], the loaded fixture)."""
    z = np.load(GOLDEN)
    out = []
    for i, name in enumerate(z["names"]):
        shape = tuple(int(v) for v in z["shapes"][i])
        n = int(np.prod(shape))
        o0, o1 = int(z["offsets"][i]), int(z["offsets"][i + 1])
        a = np.unpackbits(z["test"][o0:o1])[:n].reshape(shape).astype(bool)
        b = np.unpackbits(z["reference"][o0:o1])[:n].reshape(shape).astype(bool)
        out.append((str(name), torch.from_numpy(a), torch.from_numpy(b)))
    return out, z


def same_bits(x, y):
    """Two fp64 arrays (or floats) bit for bit, NaN positions equal."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    return x.shape == y.shape and np.array_equal(np.isnan(x), np.isnan(y)) and \
        np.array_equal(np.nan_to_num(x, nan=0.0).view(np.uint64), np.nan_to_num(y, nan=0.0).view(np.uint64))


def random_blobs(shape, gen, thresh, sigma=1.5):
    """Smooth random fields, normalised per volume and thresholded: blobs with ragged surfaces, on the CPU, deterministic."""
    x = torch.randn(shape, generator=gen, dtype=torch.float64)
    r = int(2 * sigma) + 1
    t = torch.arange(-r, r + 1, dtype=torch.float64)
    k = torch.exp(-t * t / (2 * sigma * sigma)); k /= k.sum()
    lead = x.shape[:-3]
    y = x.reshape(-1, 1, *x.shape[-3:])
    for ax in range(3):
        shp = [1, 1, 1, 1, 1]; shp[2 + ax] = k.numel()
        pad = [0, 0, 0, 0, 0, 0]; pad[2 * (2 - ax)] = pad[2 * (2 - ax) + 1] = r
        y = torch.nn.functional.conv3d(torch.nn.functional.pad(y, pad, mode="replicate"), k.reshape(shp))
    y = y / y.flatten(1).std(dim=1).reshape(-1, 1, 1, 1, 1)
    return y.reshape(*lead, *x.shape[-3:]) > thresh
