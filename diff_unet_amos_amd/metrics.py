"""Surface-distance metrics of the reference's evaluation module (light_training/evaluation/metric.py:314-390), on the device.

The reference gets hausdorff_distance, hausdorff_distance_95, avg_surface_distance and avg_surface_distance_symmetric from
medpy.metric.binary on the CPU.  Here one call, ``surface_distance_table``, computes all four for every (sample, class) of a
batch in HIP (csrc/surface.hip, include/dua_hip.h "evaluation: surface distances"), with medpy's semantics:

- border(X) = X & ~erode(X), one binary erosion with generate_binary_structure(3, connectivity) and border_value 0;
- sds(A, B) = for every voxel of border(A), the Euclidean distance (offsets scaled by voxel_spacing) to border(B);
- hd = max of both directions, hd95 = np.percentile of both directions together at 95 (linear), asd = mean sds(test,
  reference) (directed), assd = the mean of the two directed means;
- the wrapper rule: test or reference empty or full -> NaN, or 0 with nan_for_nonexisting=False.

Metrics are taken per (n, c) on the 3-D volume [D, H, W].  (Handed a [1, D, H, W] array, medpy would treat the batch as a
fourth axis, and its border-value-0 erosion along that axis would make every foreground voxel a surface voxel; that behaviour
is not reproduced.)  There is no CPU path.
"""
from __future__ import annotations

import torch

from . import _native as nv
from . import ops

TABLE_KEYS = ("hd", "hd95", "asd", "assd", "tp", "fp", "fn", "tn")


def _device_mask(t, name):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: a torch tensor on the MI355X")
    if not t.is_cuda:
        raise RuntimeError(f"{name}: surface distances run on an MI355X (device 'cuda'); there is no CPU path in this package")
    if t.dtype not in (torch.float32, torch.uint8, torch.bool):
        t = t != 0
    return t


def surface_distance_table(test, reference, voxel_spacing=None, connectivity=1, nan_for_nonexisting=True):
    """hd, hd95, asd (test -> reference), assd and the confusion counts tp, fp, fn, tn of every (n, c) of two [N, C, D, H, W]
    device masks (fp32 as ``inference.binarise`` returns, uint8 or bool; non-zero is foreground; other dtypes are compared
    with 0 first).  voxel_spacing: None (1), a scalar or (d, h, w); connectivity 1, 2 or 3.  Returns a dict of fp64 [N, C]
    device tensors; nothing is synchronised with the host."""
    test, reference = _device_mask(test, "test"), _device_mask(reference, "reference")
    if test.dim() != 5 or tuple(test.shape) != tuple(reference.shape):
        raise ValueError(f"test and reference: two [N, C, D, H, W] masks of one shape, got {tuple(test.shape)} and "
                         f"{tuple(reference.shape)}")
    if connectivity not in (1, 2, 3):
        raise ValueError(f"connectivity must be 1, 2 or 3, got {connectivity!r}")
    N, Cc = test.shape[:2]
    _, table = ops.surface_distance_table(test, reference, voxel_spacing, connectivity, nan_for_nonexisting)
    col = {name: i for i, name in enumerate(nv.SURFACE_FIELDS)}
    return {k: table[:, col[k]].reshape(N, Cc) for k in TABLE_KEYS}


def _one(test, reference, key, nan_for_nonexisting, voxel_spacing, connectivity):
    test, reference = _device_mask(test, "test"), _device_mask(reference, "reference")
    if test.dim() != 3 or tuple(test.shape) != tuple(reference.shape):
        raise ValueError(f"test and reference: two 3-D masks of one shape, got {tuple(test.shape)} and {tuple(reference.shape)}")
    t = surface_distance_table(test[None, None], reference[None, None], voxel_spacing, connectivity, nan_for_nonexisting)
    return float(t[key][0, 0])


def hausdorff_distance(test=None, reference=None, confusion_matrix=None, nan_for_nonexisting=True, voxel_spacing=None,
                       connectivity=1, **kwargs):
    """metric.py:314-329 for one 3-D mask pair: a Python float."""
    return _one(test, reference, "hd", nan_for_nonexisting, voxel_spacing, connectivity)


def hausdorff_distance_95(test=None, reference=None, confusion_matrix=None, nan_for_nonexisting=True, voxel_spacing=None,
                          connectivity=1, **kwargs):
    """metric.py:332-350 for one 3-D mask pair: a Python float."""
    return _one(test, reference, "hd95", nan_for_nonexisting, voxel_spacing, connectivity)


def avg_surface_distance(test=None, reference=None, confusion_matrix=None, nan_for_nonexisting=True, voxel_spacing=None,
                         connectivity=1, **kwargs):
    """metric.py:353-368 for one 3-D mask pair (test -> reference): a Python float."""
    return _one(test, reference, "asd", nan_for_nonexisting, voxel_spacing, connectivity)


def avg_surface_distance_symmetric(test=None, reference=None, confusion_matrix=None, nan_for_nonexisting=True,
                                   voxel_spacing=None, connectivity=1, **kwargs):
    """metric.py:371-386 for one 3-D mask pair: a Python float."""
    return _one(test, reference, "assd", nan_for_nonexisting, voxel_spacing, connectivity)
