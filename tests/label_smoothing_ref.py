"""CPU restatement, in fp64, of the centroid-distance label smoothing contract of include/dua_hip.h ("training input:
centroid-distance label smoothing"), written from that text and sharing no code with the package.  Where a patch is taken
from a volume, the source index of every output voxel comes from tests/augment_ref.py: its ``apply`` is run on volumes whose
"image" is the index along one axis, so crop, flips and rotation are the ones the one-hot tests already pin down.

The bound the tests use is derived, not chosen.  With f(d) = alpha / (d ** order + epsilon), per element

    tol = |f'(d)| * delta_d  +  16 * 2^-24 * |out|  +  2^-20,      delta_d = delta_c + 4 * 2^-24 * d

delta_c: how far the centroid in use may be from the exact one.  The kernels divide exact integer sums in fp64 and round once
to fp32: at most half an ulp per axis of a coordinate below max(extent), so delta_c = sqrt(3) * 2^-24 * max(extent) bounds
the centroid's displacement.  Against the reference's golden the per-case discrepancy of the reference's own fp32 centroids,
stored in the fixture, is added.  4 * 2^-24 * d: three squares, two sums and a square root in fp32.  16 ulps of the result:
the reciprocal, pow, the product with alpha and the difference.  2^-20: where the one-hot 1 and f(d) nearly cancel, the
result is small and the error is a few ulps of 1."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import augment_ref  # noqa: E402

U = 2.0 ** -24


def class_sums(labels, K):
    """(counts int64 [K], sums int64 [K, 3]) of a class map, in exact integer arithmetic; ids >= K are an error."""
    lab = np.asarray(labels).astype(np.int64)
    assert lab.ndim == 3 and lab.min() >= 0 and lab.max() < K, "ids in [0, K)"
    counts = np.bincount(lab.reshape(-1), minlength=K).astype(np.int64)
    sums = np.zeros((K, 3), dtype=np.int64)
    grids = np.meshgrid(*[np.arange(s, dtype=np.int64) for s in lab.shape], indexing="ij")
    for k in range(K):
        mask = lab == k
        sums[k] = [int(grids[ax][mask].sum()) for ax in range(3)]
    return counts, sums


def centroids(labels, K):
    """float64 [K, 3]: exact sums divided in fp64, (0, 0, 0) for an absent class."""
    counts, sums = class_sums(labels, K)
    out = np.zeros((K, 3), dtype=np.float64)
    present = counts > 0
    out[present] = sums[present].astype(np.float64) / counts[present, None].astype(np.float64)
    return out


def smooth(onehot, dist, alpha, order, epsilon, max_value=None):
    """| onehot - alpha / (dist ** order + epsilon) |, clamped from above by max_value; float64."""
    out = np.abs(onehot - alpha / (dist ** order + epsilon))
    return out if max_value is None else np.minimum(out, max_value)


def field(labels, K, alpha=0.3, order=1.0, epsilon=1e-6, max_value=None, cent=None):
    """(out float64 [K, E0, E1, E2], dist float64 [K, E0, E1, E2]) of a whole class map."""
    lab = np.asarray(labels).astype(np.int64)
    cent = centroids(lab, K) if cent is None else np.asarray(cent, dtype=np.float64)
    idx = np.stack(np.meshgrid(*[np.arange(s, dtype=np.float64) for s in lab.shape], indexing="ij"), axis=-1)
    dist = np.sqrt(((idx[None] - cent[:, None, None, None, :]) ** 2).sum(-1))
    onehot = (lab[None] == np.arange(K).reshape(-1, 1, 1, 1)).astype(np.float64)
    return smooth(onehot, dist, alpha, order, epsilon, max_value), dist


def tolerance(dist, out, alpha, order, epsilon, delta_c):
    """The per-element bound of the module docstring (float64, same shape as ``dist``)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        slope = alpha * order * dist ** (order - 1.0) / (dist ** order + epsilon) ** 2
    return slope * (delta_c + 4 * U * dist) + 16 * U * np.abs(out) + 2.0 ** -20


def delta_c_device(extents):
    return np.sqrt(3.0) * U * max(extents)


class CoordVolume:
    """What augment_ref.apply needs of a volume, with the index along ``axis`` as the image."""

    def __init__(self, label, axis):
        shape = tuple(label.shape)
        view = [1, 1, 1]
        view[axis] = shape[axis]
        self.image = torch.arange(shape[axis], dtype=torch.float32).view(view).expand(shape).contiguous()
        self.label = label


def apply(volumes, ints, floats, roi, class_ids, K, alpha=0.3, order=1.0, epsilon=1e-6, max_value=None):
    """The expected smoothed batch of ``params`` rows: (images fp32 [B, 1, *roi] -- augment_ref's, bit for bit; labels float64
    [B, C, *roi]; dist float64 [B, C, *roi], for ``tolerance``).  ``volumes``: augment_ref.RefVolume."""
    ints = np.asarray(ints)
    images, onehot = augment_ref.apply(volumes, ints, floats, roi, class_ids)
    zeros = np.zeros((len(ints), 2), dtype=np.float32)
    coords = [augment_ref.apply([CoordVolume(v.label, ax) for v in volumes], ints, zeros, roi, class_ids)[0][:, 0].double().numpy()
              for ax in range(3)]                              # source index (d, h, w) of every output voxel, [B, *roi] each
    cents = [centroids(v.label.numpy(), K) for v in volumes]
    ids = list(class_ids)
    dist = np.empty((len(ints), len(ids)) + tuple(roi), dtype=np.float64)
    for b, row in enumerate(ints.tolist()):
        c = cents[row[0]][ids]                                 # [C, 3]
        dist[b] = np.sqrt(sum((coords[ax][b][None] - c[:, ax].reshape(-1, 1, 1, 1)) ** 2 for ax in range(3)))
    return images, smooth(onehot.double().numpy(), dist, alpha, order, epsilon, max_value), dist


def worst_ratio(got, want, tol):
    """max |got - want| / tol over EVERY element (none is left out), and where it is."""
    ratio = np.abs(np.asarray(got, dtype=np.float64) - want) / tol
    at = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    return float(ratio[at]), at
