"""CPU restatement, in fp64, of the case-preparation contract of include/dua_hip.h ("case preparation"), written from that
text and sharing no code with the package: the window on every source voxel, the foreground box with numpy, the orientation
rule on the 3x3 block, the volume cropped, transposed and flipped with numpy operators, then one separable linear (image) or
nearest (label) pass per axis at coordinates evaluated in fp64.  tests/test_prepare_ref.py pins it down (against scipy, on
ties, on all 48 orientations); the GPU tests compare the kernels with it: labels and restored masks bit for bit, the image
within ``image_bound()``.

The bound (u = 2^-24, the unit round-off of fp32; every value below lies in [0, 1] up to the error already made):
  window : t = v - a_min, q = t / range, range = fp32(a_max - a_min): three roundings, relative error (1 + u)^3 - 1 on q;
           the clamp is 1-Lipschitz and everything it maps to 1 has |q| within 3.1 u of 1, so |f - f64| <= 3.1 u, counted as
           4 u (int16 sources convert exactly; a_min and a_max are fp32 numbers in the tests, so they carry no error).
  lerp   : fmaf(w~, fl(b - a), a) with w~ = w (1 + d), |d| <= u, the one rounding of the table weight.  With the inputs off by
           e: the convex combination a + w (b - a) is off by at most e; w (b - a) (d + d1 + d d1) adds at most
           |b - a| (2 u + u^2) <= 2 u (1 + 2 e); the rounding of the fmaf adds u (1 + e).  So e -> e + 3 u (1 + 2 e).
  tree   : three levels (W, then H, then D): 4 u + 3 * 3 u = 13 u, and the factor (1 + 2^-20) covers the second-order terms
           (e <= 13 u makes them below 13 u * 26 u).
"""
import itertools

import numpy as np

U32 = 2.0 ** -24
LETTERS = {"R": (0, 1), "L": (0, -1), "A": (1, 1), "P": (1, -1), "S": (2, 1), "I": (2, -1)}
ALL_AXCODES = ["".join(c) for p in itertools.permutations(("RL", "AP", "SI")) for c in itertools.product(*p)]


def image_bound():
    """|device image - fp64 restatement| is at most this, for any source and any geometry (module docstring)."""
    return (4 + 3 * 3) * U32 * (1 + 2.0 ** -20)


def window(v, a_min=-175.0, a_max=250.0):
    return np.clip((np.asarray(v, dtype=np.float64) - a_min) / (a_max - a_min), 0.0, 1.0)


def foreground_box(image, a_min=-175.0):
    """((lo, hi) per source axis, half-open) over the voxels above a_min; ValueError when there is none."""
    idx = np.nonzero(np.asarray(image) > a_min)
    if idx[0].size == 0:
        raise ValueError("no voxel above a_min")
    return tuple((int(i.min()), int(i.max()) + 1) for i in idx)


def io_orientation(affine):
    """[(world axis, sign)] for source axes 0, 1, 2."""
    block = np.array(affine, dtype=np.float64)[:3, :3]
    norm = np.linalg.norm(block, axis=0)
    if np.any(norm == 0):
        raise ValueError("zero column")
    u, _, vt = np.linalg.svd(block / norm)
    rot = u @ vt
    out = []
    for axis in range(3):
        world = int(np.abs(rot[:, axis]).argmax())
        out.append((world, 1 if rot[world, axis] >= 0 else -1))
        rot[world] = 0
    return out


def axis_plan(affine, axcodes="RAS"):
    """(perm, flip): prepared axis j shows source axis perm[j], reversed when flip[j]."""
    have = io_orientation(affine)
    perm, flip = [], []
    for letter in axcodes:
        world, sign = LETTERS[letter]
        src = [a for a, (w, _) in enumerate(have) if w == world]
        assert len(src) == 1, "every world axis is claimed by exactly one source axis"
        perm.append(src[0])
        flip.append(have[src[0]][1] != sign)
    return tuple(perm), tuple(flip)


def axis_coords(n_in, s_in, s_out):
    """(n_out, x fp64 [n_out]): the source coordinate every output index reads."""
    n_out = int(np.round((n_in - 1) * s_in / s_out)) + 1
    x = np.array([min(i * s_out / s_in, float(n_in - 1)) for i in range(n_out)], dtype=np.float64)
    return n_out, x


def _linear(vol, axis, x):
    n = vol.shape[axis]
    if n == 1:
        return np.take(vol, np.zeros(len(x), dtype=np.int64), axis=axis)
    lo = np.minimum(np.floor(x), n - 2).astype(np.int64)
    shape = [1, 1, 1]
    shape[axis] = len(x)
    w = (x - lo).reshape(shape)
    a, b = np.take(vol, lo, axis=axis), np.take(vol, lo + 1, axis=axis)
    return a + w * (b - a)


def _oriented(vol, box, perm, flip):
    v = vol[tuple(slice(lo, hi) for lo, hi in box)].transpose(perm)
    return v[tuple(slice(None, None, -1) if f else slice(None) for f in flip)]


def prepare(image, label, affine, pixdim=(1.5, 1.5, 2.0), axcodes="RAS", a_min=-175.0, a_max=250.0):
    """dict(image fp64, label uint8 or None, box, perm, flip, n_in, s_in, shape, coords, affine) of one case."""
    image = np.asarray(image)
    affine = np.array(affine, dtype=np.float64)
    box = foreground_box(image, a_min)
    perm, flip = axis_plan(affine, axcodes)
    norm = np.linalg.norm(affine[:3, :3], axis=0)
    vol = _oriented(window(image, a_min, a_max), box, perm, flip)
    lab = None if label is None else _oriented(np.asarray(label), box, perm, flip)
    n_in, s_in = vol.shape, tuple(float(norm[p]) for p in perm)
    coords = [axis_coords(n, si, so)[1] for n, si, so in zip(n_in, s_in, pixdim)]
    for axis in (2, 1, 0):                                   # fp64: the order matters at the 1e-16 level only
        vol = _linear(vol, axis, coords[axis])
    if lab is not None:
        lab = lab[np.ix_(*[np.rint(x).astype(np.int64) for x in coords])].astype(np.uint8)
    # prepared index i_j -> source index: origin + sign (s_out / s_in) i_j on source axis perm[j]
    to_source = np.zeros((4, 4))
    to_source[3, 3] = 1
    for j in range(3):
        lo, hi = box[perm[j]]
        to_source[perm[j], j] = (-1 if flip[j] else 1) * pixdim[j] / s_in[j]
        to_source[perm[j], 3] = hi - 1 if flip[j] else lo
    return dict(image=vol, label=lab, box=box, perm=perm, flip=flip, n_in=n_in, s_in=s_in, shape=vol.shape, coords=coords,
                pixdim=tuple(pixdim), source_shape=image.shape, affine=affine @ to_source)


def restore_indices(ref):
    """Per SOURCE axis: the prepared index (along the oriented axis that shows it) each source index reads, -1 outside the box."""
    out = [None] * 3
    for j in range(3):
        axis, (lo, hi) = ref["perm"][j], ref["box"][ref["perm"][j]]
        tab = np.full(ref["source_shape"][axis], -1, dtype=np.int64)
        for x in range(lo, hi):
            k = hi - 1 - x if ref["flip"][j] else x - lo
            tab[x] = min(max(int(np.rint(k * ref["s_in"][j] / ref["pixdim"][j])), 0), ref["shape"][j] - 1)
        out[axis] = tab
    return out


def restore(mask, ref):
    """uint8 [*source] (or [C, *source]) from a mask on the prepared grid [*prepared] (or [C, *prepared])."""
    mask = np.asarray(mask)
    if mask.ndim == 4:
        return np.stack([restore(m, ref) for m in mask])
    tabs = restore_indices(ref)
    inside = np.ix_(*[t >= 0 for t in tabs])
    inv = np.argsort(ref["perm"])                            # source axis a is prepared axis inv[a]
    picked = mask.transpose(tuple(inv))                      # axes in source order
    out = np.zeros(ref["source_shape"], dtype=np.uint8)
    out[inside] = picked[np.ix_(*[t[t >= 0] for t in tabs])]
    return out


def signed_permutation_affine(perm, signs, spacing=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0)):
    """The affine whose source axis a points along world axis perm[a] with sign signs[a] and spacing[a] millimetres a voxel."""
    a = np.zeros((4, 4))
    a[3, 3] = 1
    for axis in range(3):
        a[perm[axis], axis] = signs[axis] * spacing[axis]
    a[:3, 3] = origin
    return a


def all_signed_permutations():
    return [(p, s) for p in itertools.permutations(range(3)) for s in itertools.product((1, -1), repeat=3)]
