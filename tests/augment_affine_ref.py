"""CPU restatement of the rotation-and-zoom contract of include/dua_hip.h ("training input: random rotation and zoom"), written
from that text and sharing no code with the package.  The Philox generator, the draw of the params rows, the plain apply and
the test volumes come from tests/augment_ref.py; this module adds

  * the draw of the affine rows: numpy integers for the random words, float32 for t and z, float64 for the matrix (``draw``);
  * the source coordinates s of every output voxel in numpy float32, one rounding per operation (``coordinates``);
  * the resampled batch in fp64, evaluated at those fp32 coordinates (``apply``), the labels at the nearest voxel;
  * an fp32 emulation of the same lerp tree and intensity transform (``apply(..., emulate=True)``);
  * ``image_bound(vmax, scale, shift)``, the bound on |device - fp64| per image voxel.

The bound is derived, not measured.  u = 2^-24 is the unit roundoff of fp32, vmax the largest magnitude among the voxels of the
volume and the pad value.  The coordinates, i and f are the same numbers on both sides (s is reproduced bit for bit, f = s - i
is exact), so only the values differ.  One level of the tree computes x = fmaf(f, fl(b - a), a) for inputs a, b that carry an
error of at most e and lie within v = vmax + e:

    fl(b - a) = (b - a)(1 + d1), |d1| <= u:     f |b - a| u <= 2 v u      (f < 1, |b - a| <= 2 v)
    the fma rounds once:                        |a + f fl(b - a)| u <= (v + 2 v u) u
    the inputs' errors enter as a convex combination (1 - f) e_a + f e_b:   <= e

so e' = e + 3 v u (1 + u) bounds the level's output against the exact tree, three times over (w, h, d) starting from e = 0:
about 9 vmax u.  The intensity transform then multiplies by F = fl(1 + scale), which is the same fp32 number on both sides, and
adds shift, two roundings:

    |device - fp64| <= F e3 + V F u + (V F (1 + u) + |shift|) u,      V = vmax + e3.

The fp64 restatement's own roundings (2^-53 relative, a dozen of them) are covered by the (1 + u) factors.  The emulation uses
float32(float64(f) * float64(b - a) + float64(a)) for fmaf: the product is exact in fp64, the sum is rounded to fp64 and then to
fp32, which differs from a true fma only in rare double roundings by one ulp; the emulation is held to the bound, not to the
device's bits."""
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import augment_ref  # noqa: E402
from augment_ref import philox4x32_10, symmetric, unit  # noqa: E402

U = 2.0 ** -24
AFFINE_WORDS, A_T, A_ZOOM, A_EVENTS, A_PAD = 16, 9, 12, 13, 14
F32, F64 = np.float32, np.float64

# the draw and statistics cases of tests/test_augment_affine_gpu.py; tests/test_augment_affine_ref.py checks the statistics of
# this seed with the restatement alone
STATS_SEED, STATS_CALLS, STATS_B = 2025, 2000, 10
STATS_AFFINE = dict(rotate_prob=0.5, rotate_range=(math.radians(30), math.radians(20), math.radians(10)), zoom_prob=0.5,
                    zoom_range=(0.7, 1.4), pad_value=-1.25)


def config(rotate_prob=0.0, rotate_range=(0.0, 0.0, 0.0), zoom_prob=0.0, zoom_range=(1.0, 1.0), pad_value=0.0):
    """The fp32 fields of dua_aug_affine_config as the host fills them: tan(angle / 2) and max - min in fp64, rounded once."""
    return dict(rotate_prob=F32(rotate_prob), tan_half=[F32(math.tan(float(r) / 2)) for r in rotate_range], zoom_prob=F32(zoom_prob),
                zoom_min=F32(zoom_range[0]), zoom_span=F32(float(zoom_range[1]) - float(zoom_range[0])), pad_value=F32(pad_value))


def matrix(t, z):
    """M (float32 [9], row-major) from the half-angle tangents t (float32 [3]) and the zoom z (float32): every operation one
    fp64 operation in the order the header writes them."""
    c, s = [], []
    for a in range(3):
        td = F64(t[a])
        q = td * td
        n = F64(1.0) + q
        c.append((F64(1.0) - q) / n)
        s.append((td + td) / n)
    (cd, ch, cw), (sd, sh, sw) = c, s
    zero = F64(0.0)
    R = [ch * cw, zero - (ch * sw), sh,
         (cd * sw) + (sd * (sh * cw)), (cd * cw) - (sd * (sh * sw)), zero - (sd * ch),
         (sd * sw) - (cd * (sh * cw)), (sd * cw) + (cd * (sh * sw)), cd * ch]
    g = F64(1.0) / F64(z)
    return np.array([F32(r * g) for r in R], dtype=F32)


def row(t=(0.0, 0.0, 0.0), z=1.0, events=0, pad_value=0.0, m=None):
    """One affine row (float32 [16]); ``m`` overrides the matrix (planted defects)."""
    t = np.array(t, dtype=F32)
    out = np.zeros(AFFINE_WORDS, dtype=F32)
    out[:9] = matrix(t, F32(z)) if m is None else np.asarray(m, dtype=F32).reshape(9)
    out[A_T:A_T + 3] = t
    out[A_ZOOM] = F32(z)
    out[A_EVENTS:A_EVENTS + 1].view(np.int32)[0] = events
    out[A_PAD] = F32(pad_value)
    return out


def affine_rows(B, counter, seed=0, rotate_prob=0.0, rotate_range=(0.0, 0.0, 0.0), zoom_prob=0.0, zoom_range=(1.0, 1.0),
                pad_value=0.0):
    """The affine rows float32 [B, 16] of call ``counter``: Philox blocks 3 and 4 of every sample."""
    cfg = config(rotate_prob, rotate_range, zoom_prob, zoom_range, pad_value)
    ctr = np.zeros((B, 2, 4), dtype=np.uint64)
    ctr[:, :, 0] = int(counter) & 0xFFFFFFFF
    ctr[:, :, 1] = (int(counter) >> 32) & 0xFFFFFFFF
    ctr[:, :, 2] = np.arange(B, dtype=np.uint64)[:, None]
    ctr[:, :, 3] = np.array([3, 4], dtype=np.uint64)[None, :]
    words = philox4x32_10(ctr, (int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF))
    rows = np.zeros((B, AFFINE_WORDS), dtype=F32)
    for b in range(B):
        w3, w4 = words[b]
        t, z, events = [F32(0), F32(0), F32(0)], F32(1), 0
        if unit(w3[0]) < cfg["rotate_prob"]:
            events |= 1
            t = [symmetric(cfg["tan_half"][a], w3[1 + a]) for a in range(3)]
        if unit(w4[0]) < cfg["zoom_prob"]:
            events |= 2
            z = F32(F32(cfg["zoom_span"] * unit(w4[1])) + cfg["zoom_min"])
        rows[b] = row(t, z, events, cfg["pad_value"])
    return rows


def draw(volumes, volume_ids, counter, seed=0, rotate_prob=0.0, rotate_range=(0.0, 0.0, 0.0), zoom_prob=0.0,
         zoom_range=(1.0, 1.0), pad_value=0.0, **base):
    """(ints int32 [B, 6], floats float32 [B, 2]) of augment_ref.draw, and the affine rows float32 [B, 16] of call ``counter``."""
    ints, floats = augment_ref.draw(volumes, volume_ids, counter, seed=seed, **base)
    return ints, floats, affine_rows(len(volume_ids), counter, seed, rotate_prob, rotate_range, zoom_prob, zoom_range, pad_value)


def window_index(roi, flip, k):
    """p (int64 [3, *roi]): for every output voxel the index inside the un-flipped, un-rotated window that the plain apply reads
    for it -- the index grids pushed through the flips and the rotation of augment_ref.apply."""
    p = np.stack(np.meshgrid(*[np.arange(r) for r in roi], indexing="ij"))
    for ax in (0, 1, 2):
        if flip >> ax & 1:
            p = np.flip(p, axis=1 + ax)
    return np.ascontiguousarray(np.rot90(p, k, axes=(1, 2)))


def coordinates(m, start, roi, p, dtype=F32):
    """s (dtype [3, *roi]): steps 1 and 2 of the header, one rounding per operation in float32 (exact enough in float64)."""
    m = np.asarray(m, dtype=dtype).reshape(3, 3)
    half = [dtype(r - 1) / dtype(2) for r in roi]
    r = [p[a].astype(dtype) - half[a] for a in range(3)]
    c = [dtype(start[a]) + half[a] for a in range(3)]
    return np.stack([((m[a, 0] * r[0] + m[a, 1] * r[1]) + m[a, 2] * r[2]) + c[a] for a in range(3)])


def _corner(image, idx, pad):
    inside = np.ones(idx[0].shape, dtype=bool)
    for a in range(3):
        inside &= (idx[a] >= 0) & (idx[a] < image.shape[a])
    clipped = [np.clip(idx[a], 0, image.shape[a] - 1) for a in range(3)]
    return np.where(inside, image[clipped[0], clipped[1], clipped[2]], pad), inside


def resample(image, label, s, pad, emulate=False, defect=None):
    """(value [*roi], label id int64 [*roi], j int64 [3, *roi]) at the coordinates s: steps 3, 4, 5 and 7.  fp64 arithmetic on
    the fp32 (or fp64) coordinates, or the fp32 emulation.  ``defect``: 'lerp_order' (every lerp taken from the far corner towards the near one: the
    weights f and 1 - f exchanged), 'axis_order' (d first, w last: the same trilinear value, other roundings), 'pad_per_voxel'
    (the pad decided from the nearest voxel for the whole cell) or 'round' (np.rint for the label)."""
    i = np.floor(s)
    f = (s - i).astype(F64)
    i = i.astype(np.int64)
    T = F32 if emulate else F64
    image = image.astype(T)
    pad = T(pad)

    def lerp(a, b, w):
        if defect == "lerp_order":
            a, b = b, a
        if emulate:
            return ((w * (b - a).astype(F64)) + a.astype(F64)).astype(F32)       # see the module docstring
        return a + w * (b - a)

    cor = {}
    for e in np.ndindex(2, 2, 2):
        cor[e], _ = _corner(image, [i[a] + e[a] for a in range(3)], pad)
    nearest = [(f[a] >= 0.5).astype(np.int64) for a in range(3)]
    if defect == "round":
        j = np.rint(s).astype(np.int64)
    else:
        j = np.stack([i[a] + nearest[a] for a in range(3)])
    lab, inside = _corner(label.astype(np.int64), j, 0)
    if defect == "axis_order":
        x = {(eh, ew): lerp(cor[(0, eh, ew)], cor[(1, eh, ew)], f[0]) for eh in (0, 1) for ew in (0, 1)}
        y = {ew: lerp(x[(0, ew)], x[(1, ew)], f[1]) for ew in (0, 1)}
        value = lerp(y[0], y[1], f[2])
    else:
        x = {(ed, eh): lerp(cor[(ed, eh, 0)], cor[(ed, eh, 1)], f[2]) for ed in (0, 1) for eh in (0, 1)}
        y = {ed: lerp(x[(ed, 0)], x[(ed, 1)], f[1]) for ed in (0, 1)}
        value = lerp(y[0], y[1], f[0])
    if defect == "pad_per_voxel":
        value = np.where(inside, value, pad)
    return value, lab, j


def apply(volumes, ints, floats, rows, roi, class_ids, emulate=False, defect=None, coord_dtype=F32):
    """(images [B, 1, *roi], labels float32 [B, C, *roi] one-hot, ids int64 [B, *roi], j int64 [B, 3, *roi]) of dua_aug_apply_affine
    for the params rows (ints, floats) and the affine rows; images float64, or float32 with ``emulate``.  ``volumes``:
    augment_ref.RefVolume.  ``defect``: one of resample's, 'transpose' (M transposed) or 'late_flip' (resampling applied after the flip)."""
    images, labels, ids_out, js = [], [], [], []
    ids = np.array(list(class_ids), dtype=np.int64).reshape(-1, 1, 1, 1)
    for (vid, sd, sh, sw, flip, k), (scale, shift), arow in zip(np.asarray(ints).tolist(), np.asarray(floats, dtype=F32), rows):
        vol = volumes[vid]
        m = np.asarray(arow[:9], dtype=F32).reshape(3, 3)
        if defect == "transpose":
            m = m.T
        p = window_index(roi, 0 if defect == "late_flip" else flip, k)
        s = coordinates(m, (sd, sh, sw), roi, p, dtype=coord_dtype)
        if defect == "late_flip":                             # the window flipped first and resampled afterwards
            for ax, st in enumerate((sd, sh, sw)):
                if flip >> ax & 1:
                    s[ax] = coord_dtype(2 * st + roi[ax] - 1) - s[ax]
        value, lab, j = resample(vol.image.numpy(), vol.label.numpy(), s, arow[A_PAD], emulate=emulate,
                                 defect=defect if defect in ("lerp_order", "axis_order", "pad_per_voxel", "round") else None)
        factor = F32(F32(1.0) + F32(scale))                   # the same fp32 number on both sides
        if emulate:
            out = ((value * factor).astype(F32) + F32(shift)).astype(F32)
        else:
            out = value * F64(factor) + F64(shift)
        images.append(out[None])
        labels.append((lab[None] == ids).astype(F32))
        ids_out.append(lab)
        js.append(j)
    return np.stack(images), np.stack(labels), np.stack(ids_out), np.stack(js)


def image_bound(vmax, scale, shift=0.0):
    """The bound of the module docstring on |device - fp64| of an image voxel (vmax: over the volume's voxels and the pad)."""
    vmax, shift = F64(abs(vmax)), F64(abs(shift))
    e = F64(0.0)
    for _ in range(3):
        e = e + 3.0 * (vmax + e) * U * (1.0 + U)
    F = abs(F64(F32(F32(1.0) + F32(scale))))
    V = vmax + e
    return float(F * e + V * F * U + (V * F * (1.0 + U) + shift) * U)


def row_bounds(volumes, ints, floats, rows):
    """image_bound per row, shaped [B, 1, 1, 1, 1]."""
    out = []
    for r, (scale, shift), arow in zip(np.asarray(ints).tolist(), np.asarray(floats, dtype=F32), rows):
        vmax = max(float(volumes[r[0]].image.abs().max()), abs(float(arow[A_PAD])))
        out.append(image_bound(vmax, scale, shift))
    return np.array(out, dtype=F64).reshape(-1, 1, 1, 1, 1)


def worst_ratio(got, want, bound):
    """max |got - want| / bound over every voxel, and where it is."""
    ratio = np.abs(np.asarray(got, dtype=F64) - want) / bound
    at = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    return float(ratio[at]), at


# ---- the apply cases, shared by the CPU tests (emulation, planted defects) and the GPU tests ----

ANGLES = (-30.0, -17.0, 0.0, 11.0, 30.0)


def _hand_rows(shapes, roi, flips_ks, seed, pad_value, zooms=(0.7, 1.4, 1.0)):
    """Hand-written rows: every (flip, k) of ``flips_ks``, angles from ANGLES on each axis (the +-30 degree ends included),
    the zooms in turn, starts at both clamped ends and in between, scale / shift zero and non-zero.  Two more rows zoom
    without turning, by 1 / 2 and by 2: their coordinates are multiples of a half and of a quarter, so that f is exactly 0.5
    at many voxels, above even and above odd indices (where rounding to even parts from the f >= 0.5 rule)."""
    rng = np.random.RandomState(seed)
    ints, floats, rows = [], [], []
    for n, (flip, k) in enumerate(flips_ks):
        vid = n % len(shapes)
        hi = [s - r for s, r in zip(shapes[vid], roi)]
        start = [0, 0, 0] if n % 4 == 0 else hi if n % 4 == 1 else [int(rng.randint(0, h + 1)) for h in hi]
        ints.append([vid, *start, flip, k])
        floats.append([0.0, 0.0] if n % 3 == 0 else [0.0731, 0.0] if n % 3 == 1 else [-0.0412, 0.0893])
        deg = [ANGLES[(n + a * 2) % len(ANGLES)] if n % 5 else (30.0, -30.0, 30.0)[a] for a in range(3)]
        t = [F32(math.tan(math.radians(d) / 2)) for d in deg]
        rows.append(row(t, zooms[n % len(zooms)], 3, pad_value))
    for n, (flip, z) in enumerate(((0, 0.5), (5, 2.0))):
        vid = n % len(shapes)
        ints.append([vid, *[(s - r) // 2 for s, r in zip(shapes[vid], roi)], flip, 0])
        floats.append([0.05, -0.02])
        rows.append(row((0.0, 0.0, 0.0), z, 2, pad_value))
    return np.array(ints, dtype=np.int32), np.array(floats, dtype=F32), np.stack(rows)


def apply_cases():
    """name -> dict(shapes, seeds, roi, class_ids, ints, floats, rows): the cases of the issue, at its shapes."""
    shapes = [(40, 36, 44), (33, 47, 38)]
    every = [(f, k) for f in range(8) for k in range(4)]
    cases = {}
    for name, shp, roi, fk, pad in (("cube16", shapes, (16, 16, 16), every, -3.5),
                                    ("narrow_4_byte_stores", shapes, (12, 12, 10), every[::3], 0.0),
                                    ("oblong_k0", shapes, (8, 12, 20), [(f, 0) for f in range(8)], 0.25),
                                    ("volume_of_roi_size", [(16, 16, 16)], (16, 16, 16), every[1::4], -3.5)):
        ints, floats, rows = _hand_rows(shp, roi, fk, len(cases), pad)
        cases[name] = dict(shapes=shp, seeds=[90 + len(cases) * 4 + i for i in range(len(shp))], roi=roi, class_ids=(0, 1, 3, 7, 15),
                           ints=ints, floats=floats, rows=rows)
    return cases


def case_volumes(case):
    """[(image, label)] of a case: augment_ref.synthetic_volume at the case's shapes and seeds, the label map moved on by one
    voxel along every axis: its 8^3 blocks then end above EVEN indices, where a tie f = 0.5 rounded to even stays inside the
    block and the f >= 0.5 rule leaves it."""
    out = []
    for s, seed in zip(case["shapes"], case["seeds"]):
        image, label = augment_ref.synthetic_volume(s, seed)
        out.append((image, torch.roll(label, (1, 1, 1), (0, 1, 2)).contiguous()))
    return out


def identity_rows(n, pad_value=0.0):
    return np.stack([row(pad_value=pad_value) for _ in range(n)])


def affine_event_counts(rows):
    events = rows[:, A_EVENTS].copy().view(np.int32)
    return {"rotation": int(np.sum(events & 1 != 0)), "zoom": int(np.sum(events & 2 != 0))}


def check_affine_statistics(rows, cfg):
    """Counts within n p +- 5 sqrt(n p (1 - p)); t within +-tan_half and 0 without the event; z within [zoom_min, zoom_max] (the
    fp32 ends the header gives: zoom_min and fadd(zoom_span, zoom_min)) and 1 without the event."""
    c = config(**cfg)
    n = len(rows)
    counts = affine_event_counts(rows)
    for name, p in (("rotation", float(c["rotate_prob"])), ("zoom", float(c["zoom_prob"]))):
        print(f"{name}: {counts[name]} of {n}, expected {n * p:.0f} +- {5 * math.sqrt(n * p * (1 - p)):.0f}")
        assert abs(counts[name] - n * p) <= 5 * math.sqrt(n * p * (1 - p)), (name, counts[name], n * p)
    events = rows[:, A_EVENTS].copy().view(np.int32)
    turned, zoomed = events & 1 != 0, events & 2 != 0
    for a in range(3):
        t = rows[:, A_T + a]
        assert np.all(np.abs(t) <= c["tan_half"][a]) and np.all(t[~turned] == 0), a
        print(f"t[{a}]: {t.min():.6f} .. {t.max():.6f} within +-{c['tan_half'][a]:.6f}")
    z = rows[:, A_ZOOM]
    top = F32(c["zoom_span"] + c["zoom_min"])
    assert abs(float(top) - cfg["zoom_range"][1]) <= 2.0 ** -23 * cfg["zoom_range"][1]      # the fp32 top is zoom_max, to an ulp
    assert np.all(z >= c["zoom_min"]) and np.all(z <= top) and np.all(z[~zoomed] == 1)
    print(f"z: {z.min():.6f} .. {z.max():.6f} within [{c['zoom_min']:.6f}, {top:.6f}]")
    return counts
