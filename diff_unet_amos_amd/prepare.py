"""A raw CT case prepared on the device: window, foreground crop, reorientation and resampling.

The reference prepares a case on the host with MONAI (utils.py:125-136 for training, :168-177 for validation):
ScaleIntensityRanged(-175, 250 -> 0, 1, clip), CropForegroundd(source_key="image"), Orientationd("RAS") and
Spacingd((1.5, 1.5, 2.0), bilinear | nearest).  Here a scan as a NIfTI reader hands it over -- int16 Hounsfield units (or
fp32), an optional uint8 label map and the 4x4 affine -- becomes the fp32 image and uint8 label map of a ``DeviceVolume`` in
one box pass and one fused gather (csrc/volume_prep.hip)::

    case = prepare_case(image_hu, label, affine=affine)              # one host read: the foreground box
    volume = DeviceVolume(case.image, case.label, num_classes=16)    # or DeviceVolume.from_raw(image_hu, label, affine)
    mask_on_scan_grid = case.restore(prediction_mask)                # uint8 [C, *prepared] -> uint8 [C, *source]
    label_map, dice = inference.segment_case(model, case, raw_label) # uint8 [*source]: one class per voxel of the scan

What each step computes is fixed in include/dua_hip.h ("case preparation"), not by MONAI's source; tests/prepare_ref.py
restates it in fp64.  The geometry is host arithmetic on 16 numbers and a few KB of per-axis tables (numpy, fp64): the
functions of this module up to ``prepared_geometry`` need neither the library nor torch.
"""
from __future__ import annotations

import dataclasses

import numpy as np

AXIS_CODES = {"R": (0, 1), "L": (0, -1), "A": (1, 1), "P": (1, -1), "S": (2, 1), "I": (2, -1)}


def _affine(affine):
    a = np.asarray(affine, dtype=np.float64)
    if a.shape != (4, 4):
        raise ValueError(f"affine: a 4x4 matrix, got shape {a.shape}")
    if not np.isfinite(a).all():
        raise ValueError("affine: every entry is finite")
    return a


def orientation_from_affine(affine):
    """(world axis, sign) of source axes 0, 1, 2 -- int [3, 2] -- by nibabel's io_orientation rule: the 3x3 block divided by
    its column norms and replaced by the nearest orthogonal matrix (P Q^T of its SVD); for each source axis in turn the world
    axis with the largest absolute entry of its column, the sign of that entry, and that world axis's row zeroed before the
    next column.  Every world axis is claimed once.  An affine with a zero (or dependent) column raises ValueError."""
    a = _affine(affine)
    rzs = a[:3, :3]
    norms = np.sqrt((rzs * rzs).sum(axis=0))
    if (norms == 0).any():
        raise ValueError(f"affine: source axis {int(np.argmin(norms))} has a zero column")
    p, s, qt = np.linalg.svd(rzs / norms)
    if s.min() <= s.max() * 3 * np.finfo(np.float64).eps:
        raise ValueError("affine: the columns of its 3x3 block are linearly dependent")
    r = p @ qt
    out = np.zeros((3, 2), dtype=np.int64)
    for axis in range(3):
        col = r[:, axis]
        world = int(np.argmax(np.abs(col)))
        out[axis] = (world, -1 if col[world] < 0 else 1)
        r[world, :] = 0.0
    return out


def axcodes_to_orientation(axcodes):
    """(world axis, sign) of prepared axes 0, 1, 2 for three letters of R/L, A/P, S/I, one of each pair (48 codes)."""
    codes = tuple(str(c).upper() for c in axcodes)
    if len(codes) != 3 or any(c not in AXIS_CODES for c in codes) or {AXIS_CODES[c][0] for c in codes} != {0, 1, 2}:
        raise ValueError(f"axcodes: three letters, one of each of R/L, A/P and S/I, got {axcodes!r}")
    return np.array([AXIS_CODES[c] for c in codes], dtype=np.int64)


def spacing_tables(n_in, s_in, s_out):
    """The resampling of one axis from spacing ``s_in`` to ``s_out``: (n_out, lo int32 [n_out], weight fp32 [n_out], nearest int32
    [n_out], x fp64 [n_out]).  n_out = rint((n_in - 1) s_in / s_out) + 1 (half to even); output i reads x = min(i s_out / s_in,
    n_in - 1); lo = min(floor(x), n_in - 2), weight = x - lo (n_in == 1: 0 and 0); nearest = rint(x), half to even."""
    n_in, s_in, s_out = int(n_in), float(s_in), float(s_out)
    if n_in < 1 or not (np.isfinite(s_in) and s_in > 0 and np.isfinite(s_out) and s_out > 0):
        raise ValueError(f"spacing_tables: a positive extent and finite positive spacings, got {n_in}, {s_in}, {s_out}")
    n_out = int(np.round((n_in - 1) * s_in / s_out)) + 1
    x = np.minimum(np.arange(n_out, dtype=np.float64) * s_out / s_in, float(n_in - 1))
    lo = np.minimum(np.floor(x), max(n_in - 2, 0))
    weight = x - lo if n_in > 1 else np.zeros_like(x)
    return n_out, lo.astype(np.int32), weight.astype(np.float32), np.rint(x).astype(np.int32), x


def restore_table(n_in, s_in, s_out, n_out):
    """Prepared index int64 [n_in] each oriented index k of one axis reads on the way back: rint(k s_in / s_out), half to even,
    clamped to [0, n_out - 1]."""
    y = np.arange(int(n_in), dtype=np.float64) * float(s_in) / float(s_out)
    return np.clip(np.rint(y), 0, int(n_out) - 1).astype(np.int64)


def linear_restore_tables(geometry):
    """The linear way back of a ``PreparedGeometry``, per SOURCE axis: dict(lo, weight, step, axis), each a 3-tuple.  ``axis[p]`` is
    the prepared axis that shows source axis p, n its extent.  For the oriented index k of a source index inside the box,
    y = min(k s_in / s_out, n - 1), lower = floor(y) and ``weight`` = y - lower (fp32 [X_p], rounded once; at y = n - 1 the lower
    index is the last one and the weight 0, so equal spacings give zero weights throughout);
    ``lo`` (int32 [X_p]) is lower times the prepared element stride of that axis, -1 outside the box; a flipped axis reads the
    tables back to front.  ``step`` is that stride -- the distance to the upper neighbour -- or 0 when n == 1, where lower and
    weight are 0 as well.  ``spacing_tables`` in the other direction, the linear twin of ``PreparedGeometry.restore``
    (include/dua_hip.h, "label map on the grid of the scan")."""
    g = geometry
    out_stride = (g.shape[1] * g.shape[2], g.shape[2], 1)
    lo, weight, step, axis = [None] * 3, [None] * 3, [0] * 3, [0] * 3
    for j, (p, f) in enumerate(zip(g.perm, g.flip)):
        n = g.shape[j]
        y = np.minimum(np.arange(g.n_in[j], dtype=np.float64) * g.s_in[j] / g.pixdim[j], float(n - 1))
        lower = np.floor(y)
        w = (y - lower).astype(np.float32)
        below = lower.astype(np.int64) * out_stride[j]
        tab, wt = np.full(g.source_shape[p], -1, dtype=np.int64), np.zeros(g.source_shape[p], dtype=np.float32)
        b0, b1 = g.box[p]
        tab[b0:b1], wt[b0:b1] = (below[::-1], w[::-1]) if f else (below, w)
        lo[p], weight[p], step[p], axis[p] = tab.astype(np.int32), wt, out_stride[j] if n > 1 else 0, j
    return dict(lo=tuple(lo), weight=tuple(weight), step=tuple(step), axis=tuple(axis))


@dataclasses.dataclass(frozen=True)
class PreparedGeometry:
    """Everything the launches need, from host arithmetic alone.  ``perm[j]`` is the source axis behind prepared axis j and
    ``flip[j]`` says whether it runs backwards; ``n_in`` / ``s_in`` the cropped extent and spacing along the prepared axes;
    ``stride`` / ``base`` address oriented voxel (k0, k1, k2) in the C-contiguous source; ``lo`` / ``weight`` / ``nearest`` are
    the per-axis tables (axis 0 first); ``restore`` holds, per SOURCE axis, the prepared index times the prepared element
    stride of its oriented axis, -1 outside the box; ``affine`` maps prepared voxel indices to world coordinates."""
    source_shape: tuple
    box: tuple
    perm: tuple
    flip: tuple
    n_in: tuple
    s_in: tuple
    pixdim: tuple
    shape: tuple
    stride: tuple
    base: int
    lo: tuple
    weight: tuple
    nearest: tuple
    restore: tuple
    affine: np.ndarray


def prepared_geometry(shape, box, affine, pixdim=(1.5, 1.5, 2.0), axcodes="RAS"):
    """``shape``: the source extents (X0, X1, X2); ``box``: ((lo0, hi0), (lo1, hi1), (lo2, hi2)), half-open per source axis."""
    a = _affine(affine)
    shape = tuple(int(n) for n in shape)
    if len(shape) != 3 or min(shape) < 1:
        raise ValueError(f"shape: three positive extents, got {shape}")
    box = tuple((int(lo), int(hi)) for lo, hi in box)
    if len(box) != 3 or any(not 0 <= lo < hi <= n for (lo, hi), n in zip(box, shape)):
        raise ValueError(f"box: a non-empty half-open interval inside the volume per axis, got {box} for shape {shape}")
    pixdim = tuple(float(p) for p in pixdim)
    if len(pixdim) != 3 or not all(np.isfinite(p) and p > 0 for p in pixdim):
        raise ValueError(f"pixdim: three finite positive spacings, got {pixdim}")
    have, want = orientation_from_affine(a), axcodes_to_orientation(axcodes)
    norms = np.sqrt((a[:3, :3] ** 2).sum(axis=0))
    src_stride = (shape[1] * shape[2], shape[2], 1)
    perm, flip = [], []
    for world, sign in want:
        axis = int(np.nonzero(have[:, 0] == world)[0][0])
        perm.append(axis)
        flip.append(bool(have[axis, 1] != sign))
    n_in = tuple(box[p][1] - box[p][0] for p in perm)
    s_in = tuple(float(norms[p]) for p in perm)
    tables = [spacing_tables(n, si, so) for n, si, so in zip(n_in, s_in, pixdim)]
    out_shape = tuple(t[0] for t in tables)
    out_stride = (out_shape[1] * out_shape[2], out_shape[2], 1)
    stride = tuple(-src_stride[p] if f else src_stride[p] for p, f in zip(perm, flip))
    base = sum((box[p][1] - 1 if f else box[p][0]) * src_stride[p] for p, f in zip(perm, flip))
    restore = [None, None, None]
    # prepared index -> source index: x[perm[j]] = origin_j + sign_j (s_out_j / s_in_j) i_j
    m = np.zeros((4, 4), dtype=np.float64)
    m[3, 3] = 1.0
    for j, (p, f) in enumerate(zip(perm, flip)):
        back = restore_table(n_in[j], s_in[j], pixdim[j], out_shape[j]) * out_stride[j]
        tab = np.full(shape[p], -1, dtype=np.int64)
        tab[box[p][0]:box[p][1]] = back[::-1] if f else back
        restore[p] = tab.astype(np.int32)
        m[p, j] = (-1.0 if f else 1.0) * pixdim[j] / s_in[j]
        m[p, 3] = box[p][1] - 1 if f else box[p][0]
    return PreparedGeometry(shape, box, tuple(perm), tuple(flip), n_in, s_in, pixdim, out_shape, stride, int(base),
                            tuple(t[1] for t in tables), tuple(t[2] for t in tables), tuple(t[3] for t in tables),
                            tuple(restore), a @ m)


@dataclasses.dataclass
class PreparedCase:
    """``image`` fp32 and ``label`` uint8 (or None) on the prepared grid, both on the device; ``affine`` (numpy fp64 4x4) of
    that grid; ``source_shape`` and ``box`` (half-open per source axis) of the scan; ``orientation`` = (perm, flip) and the
    per-axis ``tables`` in ``geometry``."""
    image: object
    label: object
    affine: np.ndarray
    source_shape: tuple
    box: tuple
    orientation: tuple
    geometry: PreparedGeometry
    _restore_tables: object = None
    _linear_tables: object = None

    @property
    def tables(self):
        g = self.geometry
        return {"lo": g.lo, "weight": g.weight, "nearest": g.nearest}

    @property
    def source_spacing(self):
        """The voxel spacing of the scan per SOURCE axis (the unit of the affine, millimetres for AMOS), as the surface metrics
        take it for a label map on the scan's grid: ``geometry.s_in`` is per prepared axis, ``geometry.perm[j]`` the source
        axis behind prepared axis j.  Host arithmetic only."""
        g = self.geometry
        s = [0.0, 0.0, 0.0]
        for j, p in enumerate(g.perm):
            s[p] = float(g.s_in[j])
        return tuple(s)

    def linear_tables(self):
        """``linear_restore_tables`` of this case on its device, as ``ops.blend_finish_labelmap`` takes them: (three int32 lo
        vectors, three fp32 weight vectors, the prepared axis of each source axis); uploaded once."""
        import torch
        if self._linear_tables is None:
            t = linear_restore_tables(self.geometry)
            dev = self.image.device
            self._linear_tables = (tuple(torch.from_numpy(v).to(dev) for v in t["lo"]),
                                   tuple(torch.from_numpy(v).to(dev) for v in t["weight"]), t["axis"])
        return self._linear_tables

    def restore(self, mask):
        """A uint8 (or bool) mask on the prepared grid, [*prepared] or [C, *prepared], on the grid of the scan: uint8 [*source]
        or [C, *source].  A source voxel inside the foreground box reads the nearest prepared voxel; outside it is 0."""
        import torch
        from . import ops
        if not torch.is_tensor(mask):
            raise ValueError("PreparedCase.restore: mask is a tensor")
        if mask.dtype == torch.bool:
            mask = mask.view(torch.uint8)
        if mask.dtype != torch.uint8:
            raise ValueError(f"PreparedCase.restore: mask is uint8 or bool, got {mask.dtype}")
        shape = tuple(self.image.shape)
        if not (tuple(mask.shape) == shape or (mask.dim() == 4 and mask.shape[0] >= 1 and tuple(mask.shape[1:]) == shape)):
            raise ValueError(f"PreparedCase.restore: mask is [*{shape}] or [C, *{shape}], got {tuple(mask.shape)}")
        if mask.device != self.image.device:
            raise ValueError(f"PreparedCase.restore: mask is on {mask.device}, the case on {self.image.device}")
        if self._restore_tables is None:
            self._restore_tables = tuple(torch.from_numpy(t).to(self.image.device) for t in self.geometry.restore)
        m = mask.contiguous()
        out = ops.prep_restore(m if m.dim() == 4 else m[None], self.source_shape, self._restore_tables)
        return out if mask.dim() == 4 else out[0]


def _volume(x, name, dtypes):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(x)) if isinstance(x, np.ndarray) else x
    if not torch.is_tensor(t):
        raise ValueError(f"prepare_case: {name} is a numpy array or a tensor")
    if t.dim() == 4 and t.shape[0] == 1:
        t = t[0]
    if t.dim() != 3 or t.numel() == 0:
        raise ValueError(f"prepare_case: {name} is [X0, X1, X2], got {tuple(t.shape)}")
    if t.dtype not in dtypes:
        raise ValueError(f"prepare_case: {name} is {' or '.join(str(d) for d in dtypes)}, got {t.dtype}")
    return t


def prepare_case(image, label=None, affine=None, pixdim=(1.5, 1.5, 2.0), axcodes="RAS", a_min=-175.0, a_max=250.0,
                 device="cuda"):
    """Window, foreground crop, reorientation and resampling of one scan on ``device``; returns a ``PreparedCase``.

    ``image``: numpy array or tensor [X0, X1, X2], int16 or float32; ``label``: uint8 of the same shape, or None; ``affine``:
    4x4, voxel indices to world millimetres (required).  One host read per case: the foreground box, on which the output
    shape depends.  A scan with no voxel above ``a_min`` raises ValueError."""
    import torch
    from . import ops
    if affine is None:
        raise ValueError("prepare_case: affine is required (the 4x4 matrix of the scan)")
    a = _affine(affine)
    src = _volume(image, "image", (torch.int16, torch.float32))
    if src.numel() >= 2 ** 31:
        raise ValueError("prepare_case: image holds fewer than 2^31 voxels")
    lab = None
    if label is not None:
        lab = _volume(label, "label", (torch.uint8,))
        if lab.shape != src.shape:
            raise ValueError(f"prepare_case: label has the shape of image, got {tuple(lab.shape)} and {tuple(src.shape)}")
    a_min, a_max = float(a_min), float(a_max)
    if not (np.isfinite(a_min) and np.isfinite(a_max) and a_max > a_min):
        raise ValueError(f"prepare_case: a_min < a_max, both finite, got {a_min} and {a_max}")
    device = torch.device(device)
    if device.type != "cuda":
        raise ValueError(f"prepare_case: device is a GPU device, not {device}")
    orientation_from_affine(a), axcodes_to_orientation(axcodes)          # argument errors before any launch
    src = src.to(device).contiguous()
    lab = None if lab is None else lab.to(device).contiguous()
    words = ops.prep_foreground_box(src, a_min).tolist()                 # the one host read
    if words[6] == 0:
        raise ValueError(f"prepare_case: image has no voxel above a_min = {a_min}: no foreground to crop to")
    box = tuple((words[j], words[3 + j] + 1) for j in range(3))
    geom = prepared_geometry(tuple(src.shape), box, a, pixdim, axcodes)
    if int(np.prod(geom.shape, dtype=np.int64)) >= 2 ** 31:
        raise ValueError(f"prepare_case: the prepared volume {geom.shape} holds 2^31 voxels or more")
    out_image, out_label = ops.prep_resample(src, lab, geom, a_min, a_max - a_min)
    return PreparedCase(out_image, out_label, geom.affine, geom.source_shape, geom.box, (geom.perm, geom.flip), geom)
