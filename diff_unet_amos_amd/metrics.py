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

``surface_dice_table`` adds Normalized Surface Dice (surface Dice at a tolerance), the second AMOS ranking metric, in the
voxel-count form (the one MONAI's SurfaceDiceMetric uses), with the same border and distances:

- within(A, B, tau) = the number of voxels of border(A) whose distance to border(B) is <= tau (compared squared, in fp64);
- nsd(tau) = (within(A, B) + within(B, A)) / (|border A| + |border B|);
- one border empty -> 0; both empty -> NaN, or 0 with nan_for_nonexisting=False.  The wrapper rule above does not apply (a full
  mask has a border: the faces of the volume).

The surfel-area-weighted form of the DeepMind ``surface-distance`` library is deliberately not provided; numbers of the two
forms must not be compared.  ``surface_report`` gives the distance table and the surface Dice from one distance transform.
"""
from __future__ import annotations

import torch

from . import _native as nv
from . import ops

TABLE_KEYS = ("hd", "hd95", "asd", "assd", "tp", "fp", "fn", "tn")
DICE_KEYS = ("nsd", "within_test", "within_reference", "surface_test", "surface_reference")


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


def _pair5(test, reference, connectivity):
    test, reference = _device_mask(test, "test"), _device_mask(reference, "reference")
    if test.dim() != 5 or tuple(test.shape) != tuple(reference.shape):
        raise ValueError(f"test and reference: two [N, C, D, H, W] masks of one shape, got {tuple(test.shape)} and "
                         f"{tuple(reference.shape)}")
    if connectivity not in (1, 2, 3):
        raise ValueError(f"connectivity must be 1, 2 or 3, got {connectivity!r}")
    return test, reference


def _tolerance_rows(tolerance, classes):
    """``tolerance`` as a [classes][T] list of floats: a scalar (every class, T = 1), a length-``classes`` sequence (one per
    class, T = 1) or a [classes, T] array."""
    if isinstance(tolerance, torch.Tensor):
        tolerance = tolerance.tolist()
    elif hasattr(tolerance, "tolist"):
        tolerance = tolerance.tolist()
    if isinstance(tolerance, (int, float)):
        rows = [[float(tolerance)]] * classes
    else:
        tolerance = list(tolerance)
        if len(tolerance) != classes:
            raise ValueError(f"tolerance: a scalar, {classes} values (one per class) or a [{classes}, T] table, got "
                             f"{tolerance!r}")
        rows = [[float(x) for x in r] if isinstance(r, (list, tuple)) else [float(r)] for r in tolerance]
    T = len(rows[0])
    limit = nv.SURFACE_MAX_TOLERANCE_ENTRIES
    if any(len(r) != T for r in rows) or not 1 <= T <= nv.SURFACE_MAX_TOLERANCES or classes * T > limit:
        raise ValueError(f"tolerance: 1 to {nv.SURFACE_MAX_TOLERANCES} values per class and at most {limit} in all, got "
                         f"{tolerance!r}")
    if not all(0.0 <= x < float("inf") for r in rows for x in r):
        raise ValueError(f"tolerance: finite values >= 0, got {tolerance!r}")
    return rows


def _dice_dict(counts, within, nsd, N, Cc):
    T = nsd.shape[1]
    return {"nsd": nsd.reshape(N, Cc, T), "within_test": within[:, :, 0].reshape(N, Cc, T),
            "within_reference": within[:, :, 1].reshape(N, Cc, T), "surface_test": counts[:, 3].reshape(N, Cc),
            "surface_reference": counts[:, 4].reshape(N, Cc)}


def surface_dice_table(test, reference, tolerance, voxel_spacing=None, connectivity=1, nan_for_nonexisting=True):
    """Normalized Surface Dice (voxel-count form; not the surfel-area form of the DeepMind surface-distance library) of every
    (n, c) of two [N, C, D, H, W] device masks (dtypes as ``surface_distance_table``).  ``tolerance``, in the unit of
    voxel_spacing: a scalar, a length-C sequence (one per class) or a [C, T] table (T tolerances per class, 1 <= T <= 8,
    C T <= 128), finite and >= 0.  Returns a dict of device tensors: ``nsd`` fp64 [N, C, T]; ``within_test`` /
    ``within_reference`` int64 [N, C, T] (surface voxels of test / reference within the tolerance of the other surface);
    ``surface_test`` / ``surface_reference`` int64 [N, C] (|border|).  nsd = (within_test + within_reference) / (surface_test +
    surface_reference); one surface empty -> 0; both empty -> NaN (0 with nan_for_nonexisting=False).  Nothing is synchronised
    with the host."""
    test, reference = _pair5(test, reference, connectivity)
    N, Cc = test.shape[:2]
    rows = _tolerance_rows(tolerance, Cc)
    counts, within, nsd = ops.surface_dice_table(test, reference, rows, voxel_spacing, connectivity, nan_for_nonexisting)
    return _dice_dict(counts, within, nsd, N, Cc)


def surface_report(test, reference, tolerance, voxel_spacing=None, connectivity=1, nan_for_nonexisting=True):
    """The keys of ``surface_distance_table`` and of ``surface_dice_table`` in one dict, from one border pass and one distance
    transform (dua_surface_report); every value is bit-identical to the separate calls'."""
    test, reference = _pair5(test, reference, connectivity)
    N, Cc = test.shape[:2]
    rows = _tolerance_rows(tolerance, Cc)
    counts, table, within, nsd = ops.surface_report(test, reference, rows, voxel_spacing, connectivity, nan_for_nonexisting)
    col = {name: i for i, name in enumerate(nv.SURFACE_FIELDS)}
    out = {k: table[:, col[k]].reshape(N, Cc) for k in TABLE_KEYS}
    out.update(_dice_dict(counts, within, nsd, N, Cc))
    return out


def normalized_surface_dice(test, reference, tolerance, voxel_spacing=None, connectivity=1, nan_for_nonexisting=True):
    """Normalized Surface Dice of one 3-D mask pair at one tolerance (voxel-count form, see ``surface_dice_table``): a Python
    float."""
    test, reference = _device_mask(test, "test"), _device_mask(reference, "reference")
    if test.dim() != 3 or tuple(test.shape) != tuple(reference.shape):
        raise ValueError(f"test and reference: two 3-D masks of one shape, got {tuple(test.shape)} and {tuple(reference.shape)}")
    t = surface_dice_table(test[None, None], reference[None, None], float(tolerance), voxel_spacing, connectivity,
                           nan_for_nonexisting)
    return float(t["nsd"][0, 0, 0])


# ---- two label maps, per class, inside the class's box (include/dua_hip.h "surface report of two label maps") --------------------

def label_map_workspace_bytes(shape, boxes):
    """Workspace bytes of ``label_map_surface_report`` per class: ``boxes`` are host rows [N][K][6] (d0, h0, w0, d1, h1, w1),
    half-open, d1 == 0 for a class in neither map; the result is a list of K ints, entry k the bytes class k needs -- the
    distance table's workspace on its largest box over the N map pairs, grown by one voxel per side and clamped to ``shape``.
    The (pair, class) rows of a call run one after the other and share one region, so a call needs ``max`` of the list.  Host
    arithmetic (dua_surface_map_scratch_bytes): no device is needed."""
    K = len(boxes[0])
    return [ops.surface_map_workspace_bytes(shape, [pair[k] for pair in boxes]) for k in range(K)]


def class_groups(needs, max_workspace_bytes=None):
    """The groups the classes 0 .. K - 1 are processed in under ``max_workspace_bytes`` (``needs``: bytes per class).  The classes
    of a group share one region sized to its largest class, so as soon as every class fits, ONE group does: the limit requires
    no more.  A class that alone exceeds the limit is refused (ValueError)."""
    if max_workspace_bytes is not None:
        if isinstance(max_workspace_bytes, bool) or not isinstance(max_workspace_bytes, int) or max_workspace_bytes < 1:
            raise ValueError(f"max_workspace_bytes must be None or an integer >= 1, got {max_workspace_bytes!r}")
        for k, need in enumerate(needs):
            if need > max_workspace_bytes:
                raise ValueError(f"max_workspace_bytes={max_workspace_bytes}: class index {k} alone needs {need} bytes")
    return [list(range(len(needs)))]


def _label_map_pair(test_map, reference_map):
    for t, name in ((test_map, "test_map"), (reference_map, "reference_map")):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name}: a torch tensor on the MI355X")
        if t.dtype != torch.uint8:
            raise ValueError(f"{name}: a uint8 label map of class ids, not {t.dtype}")
        if not t.is_cuda:
            raise RuntimeError(f"{name}: surface distances run on an MI355X (device 'cuda'); there is no CPU path in this package")
    if test_map.dim() not in (3, 4) or 0 in test_map.shape or tuple(test_map.shape) != tuple(reference_map.shape):
        raise ValueError(f"test_map and reference_map: two label maps [D, H, W] or [N, D, H, W] of one shape, got "
                         f"{tuple(test_map.shape)} and {tuple(reference_map.shape)}")
    if test_map.dim() == 3:
        return test_map[None], reference_map[None]
    return test_map, reference_map


def label_map_surface_report(test_map, reference_map, classes, tolerance, voxel_spacing=None, connectivity=1,
                             nan_for_nonexisting=True, boxes=None, max_workspace_bytes=None):
    """``surface_report`` of two uint8 device label maps ([D, H, W] or [N, D, H, W]) for the class ids in ``classes`` (K of them,
    each in 0..63), with the mask of class c read as (map == c) from the maps themselves -- no one-hot tensor -- and each class
    worked on inside its bounding box in both maps, grown by one voxel.  Returns the keys of ``surface_report``: fp64 / int64
    [N, K], and [N, K, T] for ``nsd`` / ``within_test`` / ``within_reference``.  Every integer count, hd, hd95, nsd and the
    within counts are bit-identical to ``surface_report`` on the expansion over the full extent; asd / assd sum the same fp64
    terms in another block order.  ``tolerance``: a scalar, K values or a [K, T] table, as ``surface_dice_table``.

    HOST SYNCHRONISATION: the box table int32 [N, K, 6] is computed on the device and read to the host once per call, to size
    the launches and the workspace; that is the only one.  ``boxes`` (what an earlier call's maps gave, an int32 tensor or
    nested rows [N][K][6], (d0, h0, w0, d1, h1, w1) half-open, d1 == 0 for a class in neither map) avoids it.
    ``max_workspace_bytes``: a limit on the workspace of the call (``max(label_map_workspace_bytes(...))``: the classes run
    one after the other in one region sized to the largest box, so one group of classes always suffices, see ``class_groups``);
    a class whose box alone needs more is refused with a ValueError before anything is launched."""
    a, b = _label_map_pair(test_map, reference_map)
    if connectivity not in (1, 2, 3):
        raise ValueError(f"connectivity must be 1, 2 or 3, got {connectivity!r}")
    ids = [int(c) for c in classes]
    if not ids or any(c < 0 or c >= nv.BLEND_MAX_CLASSES for c in ids):
        raise ValueError(f"classes: at least one class id in 0..{nv.BLEND_MAX_CLASSES - 1}, got {list(classes)!r}")
    N, K = a.shape[0], len(ids)
    rows = _tolerance_rows(tolerance, K)
    T = len(rows[0])
    if boxes is None:
        table = ops.surface_map_boxes(a, b, max(ids) + 1)[:, ids]
        boxes = table.cpu().tolist()                                  # the one host read of this function
    else:
        boxes = boxes.tolist() if hasattr(boxes, "tolist") else [[list(r) for r in pair] for pair in boxes]
        if len(boxes) != N or any(len(pair) != K or any(len(r) != 6 for r in pair) for pair in boxes):
            raise ValueError(f"boxes: [{N}][{K}][6] rows (d0, h0, w0, d1, h1, w1), one per (map pair, class)")
    class_groups(label_map_workspace_bytes(a.shape[1:], boxes), max_workspace_bytes)        # one group, or a refusal
    counts, table, within, nsd = ops.surface_map_report(a, b, ids, [r for pair in boxes for r in pair], rows, voxel_spacing,
                                                        connectivity, nan_for_nonexisting)
    table = table.view(N, K, -1)
    col = {name: i for i, name in enumerate(nv.SURFACE_FIELDS)}
    out = {k: table[:, :, col[k]] for k in TABLE_KEYS}
    out.update(_dice_dict(counts, within, nsd, N, K))
    return out
