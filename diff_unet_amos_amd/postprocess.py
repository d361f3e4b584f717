"""Connected-component post-processing of a segmentation mask, on the device: label the components of every (sample, class)
volume, count their voxels, keep the largest ones and drop those below a size -- the step between ``evaluate_volume``'s mask
and the surface metrics of ``metrics.py`` (one stray island far from an organ sets that organ's Hausdorff distance).

One labelling in HIP (csrc/components.hip, include/dua_hip.h "evaluation: connected components") serves every function here,
with these semantics, per 3-D volume [D, H, W] of a [..., D, H, W] mask (non-zero = foreground):

- labels = scipy.ndimage.label(volume, generate_binary_structure(3, connectivity))[0]: 6, 18 or 26 neighbours for connectivity
  1, 2, 3; background 0; components numbered 1, 2, ... by their first voxel in raster order (W fastest); count = their number;
- sizes[l - 1] = the voxels of label l, in a table of ``cap`` entries;
- keep-largest: the ``num_components`` components first in np.argsort(-sizes, kind="stable") -- the largest, a tie going to
  the component whose first voxel comes first; ``num_components=0`` puts no limit on the number;
- ``min_size``: a component with fewer voxels is dropped (exactly ``min_size`` voxels: kept);
- ``channels``: the class channels (axis -4) that are filtered; every other channel is copied through as (mask != 0);
- overflow: a volume with more than ``cap`` components has only its first ``cap`` (by number) tallied and considered; the
  components numbered above ``cap`` are dropped by the filter.  ``count`` tells: compare it with ``cap``.

Everything is integer work: results are exact, and equal between runs.  Nothing synchronises with the host, so every function
can be captured into a graph.  There is no CPU path.
"""
from __future__ import annotations

import math

import torch

from . import _native as nv
from . import ops

DEFAULT_CAP = 16384          # entries of the size table per volume when ``cap`` is not given (the overflow rule above)


def _device_mask(t, name):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: a torch tensor on the MI355X")
    if t.dim() < 3 or 0 in t.shape:
        raise ValueError(f"{name}: a non-empty [..., D, H, W] mask, got {tuple(t.shape)}")
    if t.is_complex():
        raise ValueError(f"{name}: a real or boolean mask, not {t.dtype}")
    if not t.is_cuda:
        raise RuntimeError(f"{name}: connected components run on an MI355X (device 'cuda'); there is no CPU path in this package")
    if t.dtype not in (torch.float32, torch.uint8, torch.bool):
        t = t != 0
    return t


def _connectivity(connectivity):
    if isinstance(connectivity, bool) or connectivity not in (1, 2, 3):
        raise ValueError(f"connectivity must be 1, 2 or 3, got {connectivity!r}")
    return int(connectivity)


def _count(value, name):
    if isinstance(value, bool) or not isinstance(value, int) or value < 0:
        raise ValueError(f"{name} must be an integer >= 0, got {value!r}")
    return value


def _cap(cap):
    cap = DEFAULT_CAP if cap is None else cap
    if isinstance(cap, bool) or not isinstance(cap, int) or not 1 <= cap <= nv.CC_MAX_CAP:
        raise ValueError(f"cap must be an integer in 1..{nv.CC_MAX_CAP}, got {cap!r}")
    return cap


def _channels(mask, channels):
    """The sorted channel list of ``channels`` (None: all), checked against the channel axis (-4) of ``mask``."""
    if channels is None:
        return None
    if not isinstance(mask, torch.Tensor):
        raise TypeError("mask: a torch tensor on the MI355X")
    if mask.dim() < 4:
        raise ValueError(f"channels needs a mask with a channel axis, [..., C, D, H, W]; got {tuple(mask.shape)}")
    Cn = mask.shape[-4]
    chosen = sorted({int(c) for c in channels})
    if any(c < 0 or c >= Cn for c in chosen):
        raise ValueError(f"channels must lie in 0..{Cn - 1}, got {list(channels)!r}")
    return chosen


def _selection_flags(chosen, shape, device):
    """uint8 device flags, one per volume of a [..., C, D, H, W] tensor of ``shape``: 1 where the volume's channel (or, for the
    one row of a label map, the class) is in ``chosen``; None for all.  Filled on the device, so a graph capture holds no copy
    from the host."""
    if chosen is None:
        return None
    flags = torch.zeros((math.prod(shape[:-4]), shape[-4]), dtype=torch.uint8, device=device)
    for c in chosen:
        flags[:, c] = 1
    return flags.view(-1)


def _reference_map(reference, label_map, m, runs):
    """``reference`` of a map-form tallying call as a tensor shaped like ``m`` (``label_map`` with a leading axis), or None."""
    if reference is None:
        return None
    if not isinstance(reference, torch.Tensor) or not reference.is_cuda:
        raise RuntimeError(f"reference: {runs} on an MI355X (device 'cuda'); there is no CPU path in this package")
    if reference.dtype != torch.uint8 or tuple(reference.shape) != tuple(label_map.shape):
        raise ValueError(f"reference: a uint8 label map {tuple(label_map.shape)}, got {reference.dtype} {tuple(reference.shape)}")
    return reference.view(m.shape)


def _reference_labels(mask, labels):
    """``labels`` of a tallying call on ``mask`` as (reference or None, classes, is a label map): one-hot like ``mask``
    [B, C, D, H, W] (fp32, uint8 or bool; other dtypes are compared with 0) or a uint8 label map [B, D, H, W]."""
    if labels is None:
        return None, 1, False
    if not isinstance(labels, torch.Tensor) or not labels.is_cuda:
        raise RuntimeError("labels: connected components run on an MI355X (device 'cuda'); there is no CPU path in this package")
    if mask.dim() != 5:
        raise ValueError(f"with labels, mask is [B, C, D, H, W]; got {tuple(mask.shape)}")
    Cn = mask.shape[1]
    if tuple(labels.shape) == tuple(mask.shape):
        ref, is_map = labels if labels.dtype in (torch.float32, torch.uint8, torch.bool) else labels != 0, False
    elif tuple(labels.shape) == (mask.shape[0], *mask.shape[2:]) and labels.dtype == torch.uint8:
        ref, is_map = labels, True
    else:
        raise ValueError(f"labels: one-hot {tuple(mask.shape)} or a uint8 label map {(mask.shape[0], *mask.shape[2:])}, got "
                         f"{labels.dtype} {tuple(labels.shape)}")
    if Cn > nv.BLEND_MAX_CLASSES:
        raise ValueError(f"at most {nv.BLEND_MAX_CLASSES} classes, got {Cn}")
    return ref, Cn, is_map


def label_components(mask, connectivity=1):
    """(labels int32 shaped like ``mask``, count int32 shaped like ``mask.shape[:-3]``) of a [..., D, H, W] device mask (fp32,
    uint8 or bool; other dtypes are compared with 0 first).  Per volume, labels equals
    scipy.ndimage.label(volume, generate_binary_structure(3, connectivity))[0] and count its number of components."""
    conn = _connectivity(connectivity)
    mask = _device_mask(mask, "mask")
    labels, counts = ops.cc_label(mask, conn)
    return labels.view(mask.shape), counts.view(mask.shape[:-3])


def component_sizes(labels, count, cap=None):
    """int32 [..., cap]: entry l - 1 is the number of voxels with label l of ``labels`` (int32 [..., D, H, W], as
    ``label_components`` returns it with ``count``).  A volume with count > cap has its labels above ``cap`` left out."""
    cap = _cap(cap)
    for t, name in ((labels, "labels"), (count, "count")):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name}: a torch tensor on the MI355X")
        if t.dtype != torch.int32:
            raise ValueError(f"{name}: int32 as label_components returns it, not {t.dtype}")
    if labels.dim() < 3 or 0 in labels.shape or tuple(count.shape) != tuple(labels.shape[:-3]):
        raise ValueError(f"labels [..., D, H, W] and count [...] of one label_components call, got {tuple(labels.shape)} and "
                         f"{tuple(count.shape)}")
    for t, name in ((labels, "labels"), (count, "count")):
        if not t.is_cuda:
            raise RuntimeError(f"{name}: connected components run on an MI355X (device 'cuda'); there is no CPU path in this package")
    sizes = ops.cc_sizes(labels.contiguous().view(-1, *labels.shape[-3:]), cap)
    return sizes.view(*labels.shape[:-3], cap)


def filter_components(mask, connectivity=1, num_components=1, min_size=0, channels=None, cap=None, labels=None):
    """``keep_largest_components`` and, when ``labels`` is given, the Dice tallies of its result in the same pass: (filtered
    uint8 mask, tallies int64 [C, 3] = (|A & B|, |A|, |B|) per class or None).  ``mask``: [B, C, D, H, W] when ``labels`` is
    given; ``labels``: one-hot like ``mask`` (fp32, uint8 or bool) or a uint8 label map [B, D, H, W] (class c = channel c), as
    ``evaluate_volume`` takes them.  ``ops.dice_from_tallies`` turns the tallies into Dice."""
    conn, k, min_size, cap = _connectivity(connectivity), _count(num_components, "num_components"), _count(min_size, "min_size"), \
        _cap(cap)
    chosen = _channels(mask, channels)
    mask = _device_mask(mask, "mask")
    flags = _selection_flags(chosen, mask.shape, mask.device)
    ref, Cn, is_map = _reference_labels(mask, labels)
    lab, counts = ops.cc_label(mask, conn, select=flags)
    sizes = ops.cc_sizes(lab, cap)
    out, tallies = ops.cc_filter(lab, counts, sizes, k, min_size, apply=flags, mask=mask if flags is not None else None,
                                 reference=ref, classes=Cn, label_map=is_map)
    return out.view(mask.shape), tallies


def keep_largest_components(mask, connectivity=1, num_components=1, min_size=0, channels=None, cap=None):
    """uint8 like ``mask`` ([..., D, H, W] or, with ``channels``, [..., C, D, H, W]): 1 where the voxel belongs to one of the
    ``num_components`` largest components of its volume (ties to the component whose first voxel comes first; 0 = no limit)
    that has at least ``min_size`` voxels.  ``channels``: the class channels that are filtered, the others are copied through
    (for AMOS, ``range(1, 16)`` leaves the background channel alone); None filters all."""
    return filter_components(mask, connectivity, num_components, min_size, channels, cap)[0]


def remove_small_components(mask, min_size, connectivity=1, channels=None, cap=None):
    """``keep_largest_components`` without a limit on the number: every component of at least ``min_size`` voxels stays."""
    return filter_components(mask, connectivity, 0, min_size, channels, cap)[0]


# ---- a label map as it is: one union-find for all classes (include/dua_hip.h "Components of a label map") ------------------------
#
# ``segment_case`` returns one uint8 label map on the grid of the scan.  The functions below label and filter it without the
# [C, *scan] one-hot tensor: a voxel with value c in 1 .. num_classes - 1 is foreground of class c, 0 and values >= num_classes
# are background to the labelling and pass through the filter, and two adjacent foreground voxels are connected only when they
# carry the same value.  Per class c the components are those of scipy.ndimage.label(label_map == c, structure), in scipy's
# order; all classes are numbered together by their first voxel.  The keep-largest rule applies per class.

def _device_label_map(t, name):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: a torch tensor on the MI355X")
    if t.dtype != torch.uint8:
        raise ValueError(f"{name}: a uint8 label map of class ids, not {t.dtype}")
    if t.dim() not in (3, 4) or 0 in t.shape:
        raise ValueError(f"{name}: a non-empty label map [D, H, W] or [N, D, H, W], got {tuple(t.shape)}")
    if not t.is_cuda:
        raise RuntimeError(f"{name}: connected components run on an MI355X (device 'cuda'); there is no CPU path in this package")
    return t if t.dim() == 4 else t[None]


def _num_classes(num_classes):
    if isinstance(num_classes, bool) or not isinstance(num_classes, int) or not 1 <= num_classes <= nv.BLEND_MAX_CLASSES:
        raise ValueError(f"num_classes must be an integer in 1..{nv.BLEND_MAX_CLASSES}, got {num_classes!r}")
    return num_classes


def _class_list(classes, num_classes):
    """The sorted list of ``classes`` (None: all), checked against 1 .. num_classes - 1."""
    if classes is None:
        return None
    chosen = sorted({int(c) for c in classes})
    if any(c < 1 or c >= num_classes for c in chosen):
        raise ValueError(f"classes must lie in 1..{num_classes - 1}, got {list(classes)!r}")
    return chosen


def label_map_components(label_map, num_classes, connectivity=1):
    """(labels int32 shaped like ``label_map``, count int32 [N] or a 0-d tensor) of a uint8 device label map [D, H, W] or
    [N, D, H, W]: the components of the classes 1 .. num_classes - 1, numbered 1, 2, ... together by their first voxel in raster
    order.  For every class c, the labels on (label_map == c) are those of scipy.ndimage.label(label_map == c, structure) in the
    same order; the class of a label is the map's value on it."""
    Cn, conn = _num_classes(num_classes), _connectivity(connectivity)
    m = _device_label_map(label_map, "label_map")
    labels, counts = ops.cc_label_map(m, Cn, conn)
    return labels.view(label_map.shape), counts.view(label_map.shape[:-3])


def filter_label_map(label_map, num_classes, connectivity=1, num_components=1, min_size=0, classes=None, cap=None, reference=None):
    """(filtered uint8 label map shaped like ``label_map``, tallies int64 [num_classes, 3] or None).  A component of class c stays
    when it is among the ``num_components`` largest components OF CLASS c (ties to the component whose first voxel comes first;
    0 = no limit) and has at least ``min_size`` voxels; the voxels of a dropped component become 0.  ``classes``: the classes that
    are filtered (None: 1 .. num_classes - 1), the others pass through, as do 0 and values >= num_classes.  ``cap``: the size
    table's entries per map, over all classes together (the overflow rule of the module).  ``reference``: a uint8 label map
    like ``label_map``; with it the same pass writes the Dice tallies (|A & B|, |A|, |B|) per class of the filtered map, which
    ``ops.dice_from_tallies`` turns into Dice."""
    Cn, conn = _num_classes(num_classes), _connectivity(connectivity)
    k, min_size, cap = _count(num_components, "num_components"), _count(min_size, "min_size"), _cap(cap)
    chosen = _class_list(classes, Cn)
    m = _device_label_map(label_map, "label_map")
    ref = _reference_map(reference, label_map, m, "connected components run")
    flags = _selection_flags(chosen, (Cn, *m.shape[1:]), m.device)
    lab, counts = ops.cc_label_map(m, Cn, conn)
    sizes = ops.cc_sizes(lab, cap)
    out, tallies = ops.cc_filter_map(m, Cn, lab, counts, sizes, k, min_size, apply=flags, reference=ref)
    return out.view(label_map.shape), tallies


def keep_largest_in_label_map(label_map, num_classes, connectivity=1, num_components=1, min_size=0, classes=None, cap=None):
    """``filter_label_map`` without a reference: the filtered uint8 label map alone."""
    return filter_label_map(label_map, num_classes, connectivity, num_components, min_size, classes, cap)[0]


# ---- filling of enclosed holes (include/dua_hip.h "evaluation: fill holes", csrc/fill_holes.hip) ---------------------------------
#
# The step that follows keep-largest in most organ pipelines: a pocket of background inside a solid organ costs Dice and adds
# a false inner surface to every surface metric.  The union-find of the components runs on the BACKGROUND voxels here;
# ``connectivity`` is scipy's generate_binary_structure(3, connectivity) and governs both how background voxels join and which
# voxels count as neighbours of a background component (1, the default, is ``binary_fill_holes``' default).

def fill_holes(mask, connectivity=1, channels=None, labels=None):
    """(filled mask of the input's dtype and shape, filled int64 ``mask.shape[:-3]`` -- the voxels filled per volume --) and,
    when ``labels`` is given, the Dice tallies int64 [C, 3] of the result as a third entry.  Per volume [D, H, W] a hole is a
    component of (mask == 0) with no voxel on a face of the volume; its voxels become 1, everything else is returned as it
    came, so (result != 0) equals scipy.ndimage.binary_fill_holes(volume, generate_binary_structure(3, connectivity)).
    ``channels``: the class channels (axis -4) that are filled, the others are copied through (None: all).  ``labels``: as
    ``filter_components`` takes them, with ``mask`` [B, C, D, H, W]."""
    conn = _connectivity(connectivity)
    chosen = _channels(mask, channels)
    dtype = mask.dtype if isinstance(mask, torch.Tensor) else None
    mask = _device_mask(mask, "mask")
    flags = _selection_flags(chosen, mask.shape, mask.device)
    ref, Cn, is_map = _reference_labels(mask, labels)
    out, filled, tallies = ops.fill_holes_mask(mask, conn, select=flags, reference=ref, classes=Cn, label_map=is_map)
    out = out.view(mask.shape)
    if mask.dtype == torch.bool:
        out = out.view(torch.bool)
    if out.dtype != dtype:
        out = out.to(dtype)                                     # a dtype that was compared with 0 on the way in
    filled = filled.view(mask.shape[:-3])
    return (out, filled) if labels is None else (out, filled, tallies)


def fill_holes_in_label_map(label_map, num_classes, connectivity=1, classes=None, reference=None):
    """(filled uint8 label map shaped like ``label_map``, filled int64 [num_classes] -- the voxels that became class c --) and,
    when ``reference`` (a uint8 label map like ``label_map``) is given, the Dice tallies int64 [num_classes, 3] of the result as a
    third entry.  A component of (label_map == 0) is filled with class c when it touches no face of the volume, every voxel
    adjacent to it carries the same value c, 1 <= c < num_classes and c is among ``classes`` (None: 1 .. num_classes - 1).  A
    component bordered by two values, by a value >= num_classes or by a class that is not selected stays 0; non-zero voxels never
    change.  All classes are decided on the input map in one pass, so the result does not depend on an order of the classes.
    For a map with one class it is ``binary_fill_holes(label_map == c)``; unlike ``binary_fill_holes`` run class by class it
    does not fill a pocket that holds an island of another class."""
    Cn, conn = _num_classes(num_classes), _connectivity(connectivity)
    chosen = _class_list(classes, Cn)
    m = _device_label_map(label_map, "label_map")
    ref = _reference_map(reference, label_map, m, "fill_holes runs")
    out, filled, tallies = ops.fill_holes_map(m, Cn, conn, classes=chosen, reference=ref)
    out = out.view(label_map.shape)
    return (out, filled) if reference is None else (out, filled, tallies)


# ---- the stage dicts of inference.py: ``postprocess=`` and ``fill_holes=`` of evaluate_volume / infer (the mask form) and of
# segment_case (the map form) -----------------------------------------------------------------------------------------------------

POSTPROCESS_KEYS = ("connectivity", "num_components", "min_size", "channels", "cap")            # filter_components
SEGMENT_POSTPROCESS_KEYS = ("connectivity", "num_components", "min_size", "classes", "cap")    # filter_label_map
FILL_HOLES_KEYS = ("connectivity", "channels")                                                  # fill_holes
FILL_HOLES_MAP_KEYS = ("connectivity", "classes")                                               # fill_holes_in_label_map

_STAGE_KEYS = {("postprocess", "mask"): POSTPROCESS_KEYS, ("postprocess", "map"): SEGMENT_POSTPROCESS_KEYS,
               ("fill_holes", "mask"): FILL_HOLES_KEYS, ("fill_holes", "map"): FILL_HOLES_MAP_KEYS}
_STAGE_VALUES = {"connectivity": _connectivity, "num_components": lambda v: _count(v, "num_components"),
                 "min_size": lambda v: _count(v, "min_size"), "cap": _cap}
# the key that holds a list of integers and their lower bound.  The channels of the mask-form ``postprocess=`` are not listed:
# filter_components takes whatever int() takes and checks the range against the mask's channel axis, which no one knows here.
_STAGE_SELECTION = {("postprocess", "map"): ("classes", 1), ("fill_holes", "mask"): ("channels", 0),
                    ("fill_holes", "map"): ("classes", 1)}


def check_stage_kwargs(stage, form, value):
    """Refuse the ``stage`` ("postprocess" or "fill_holes") argument of an inference function in the ``form`` "mask" or "map"
    unless it is a dict with keys among the stage's key tuple and values the stage's function takes, with that function's own
    message -- before any predictor call and any device work."""
    keys = _STAGE_KEYS[stage, form]
    if not isinstance(value, dict) or any(k not in keys for k in value):
        raise ValueError(f"{stage}: None or a dict with keys among {keys}, got {value!r}")
    for key, check in _STAGE_VALUES.items():
        if key in value:
            check(value[key])
    selection, low = _STAGE_SELECTION.get((stage, form), (None, 0))
    chosen = value.get(selection)
    if chosen is not None and (isinstance(chosen, (str, bytes)) or not hasattr(chosen, "__iter__") or
                               any(isinstance(c, bool) or not isinstance(c, int) or c < low for c in chosen)):
        raise ValueError(f"{stage}: {selection} is None or integers >= {low}, got {chosen!r}")
