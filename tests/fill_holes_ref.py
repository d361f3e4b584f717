"""Reference for the fill-holes tests, in numpy alone (the scipy results live in tests/golden/fill_holes_golden.npz, written by
tools/make_fill_holes_golden.py).

THE CONTRACT (include/dua_hip.h "evaluation: fill holes"), restated.  All arithmetic is integer, every result is exact, no
tolerance appears anywhere.  ``connectivity`` k in {1, 2, 3} is scipy's generate_binary_structure(3, k); it governs both how
background voxels join and which voxels count as neighbours of a component.

Mask form, per volume m [D, H, W]: a hole is a k-connected component of {m == 0} with no voxel on any of the six faces; the
result is m with every hole voxel set to 1 = scipy.ndimage.binary_fill_holes(m, structure k).

Map form, for a uint8 map and C <= 64 classes: a hole is a k-connected component Hc of {map == 0} that touches no face, whose
outside k-neighbours all carry the same value c, with 1 <= c < C and c among ``classes`` (default all of 1 .. C - 1); it is
filled with c.  A component bordered by two values, by a value >= C or by an unselected class stays 0; non-zero voxels never
change; the rule is order-free.  For a map with one non-zero value c it is binary_fill_holes(map == c); unlike per-class
binary_fill_holes it does not fill a pocket that holds an island of another class.

Both forms count the filled voxels (per volume / per class) and, with a reference, the Dice tallies (|A & B|, |A|, |B|) per class
of the filled result.

``fill_mask`` / ``fill_map`` restate the contract directly (components by union-find, then the definition).  ``emulate_map``
walks the steps of csrc/fill_holes.hip instead -- roots, border flags from the faces, a 64-bit neighbour set per root with bit 0
for "value >= C or unselected", the fill decision "no flag and exactly one bit >= 1", tallies of the filled map -- and takes a
planted defect, so the CPU tests can show that every case list catches every defect."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fill_holes_golden.npz")

DEFECTS = ("border_face_missing", "ring_connectivity_1", "two_classes_lower", "value_ge_C_absent", "unselected_filled",
           "tallies_miss_filled")


def offsets(k):
    """The neighbour offsets of generate_binary_structure(3, k), without the centre."""
    return [(dz, dy, dx) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)
            if 1 <= (dz != 0) + (dy != 0) + (dx != 0) <= k]


_ROOTS = {}          # roots() of the volumes seen so far: the defect tests walk every case once per defect


def roots(member, k):
    """int64 array shaped like ``member``: the smallest linear index of the k-connected component of ``member`` a voxel belongs
    to, -1 outside ``member`` -- what the device's union-find holds after its flatten pass."""
    key = (member.shape, member.tobytes(), k)
    if key in _ROOTS:
        return _ROOTS[key].copy()
    D, H, W = member.shape
    parent = np.where(member.ravel(), np.arange(member.size), -1)

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    back = [o for o in offsets(k) if o < (0, 0, 0)]
    for p in np.flatnonzero(member.ravel()):
        d, h, w = np.unravel_index(p, member.shape)
        for dz, dy, dx in back:
            z, y, x = d + dz, h + dy, w + dx
            if 0 <= z < D and 0 <= y < H and 0 <= x < W and member[z, y, x]:
                a, b = find(p), find((z * H + y) * W + x)
                if a != b:
                    parent[max(a, b)] = min(a, b)
    out = np.array([find(p) if parent[p] >= 0 else -1 for p in range(member.size)], dtype=np.int64)
    _ROOTS[key] = out.reshape(member.shape)
    return _ROOTS[key].copy()


def face_mask(shape):
    f = np.zeros(shape, dtype=bool)
    f[0], f[-1], f[:, 0], f[:, -1], f[:, :, 0], f[:, :, -1] = (True,) * 6
    return f


def fill_mask(m, k):
    """(m != 0 with its holes filled, bool; the number of filled voxels)."""
    bg = np.asarray(m) == 0
    r = roots(bg, k)
    open_roots = np.unique(r[face_mask(bg.shape) & bg])
    holes = bg & ~np.isin(r, open_roots)
    return ~bg | holes, int(holes.sum())


def _ring_values(m, comp, k):
    """The values of the voxels k-adjacent to a voxel of ``comp`` and outside it."""
    D, H, W = m.shape
    vals = set()
    for d, h, w in np.argwhere(comp):
        for dz, dy, dx in offsets(k):
            z, y, x = d + dz, h + dy, w + dx
            if 0 <= z < D and 0 <= y < H and 0 <= x < W and not comp[z, y, x]:
                vals.add(int(m[z, y, x]))
    return vals


def fill_map(m, C, k, classes=None):
    """(the filled uint8 map, int64 [C] filled voxels per class), straight from the contract."""
    m = np.asarray(m, dtype=np.uint8)
    chosen = set(range(1, C)) if classes is None else {int(c) for c in classes}
    bg = m == 0
    r = roots(bg, k)
    faces = face_mask(m.shape)
    out, filled = m.copy(), np.zeros(C, dtype=np.int64)
    for root in np.unique(r[bg]):
        comp = r == root
        if (comp & faces).any():
            continue
        vals = _ring_values(m, comp, k)
        if len(vals) == 1:
            c = next(iter(vals))
            if 1 <= c < C and c in chosen:
                out[comp] = c
                filled[c] += int(comp.sum())
    return out, filled


def tallies_map(a, b, C):
    """int64 [C, 3] = (|A & B|, |A|, |B|) per class of two label maps; a value >= C counts nowhere."""
    return np.array([[((a == c) & (b == c)).sum(), (a == c).sum(), (b == c).sum()] for c in range(C)], dtype=np.int64)


def tallies_mask(a, b):
    """int64 [C, 3] of two [N, C, D, H, W] masks (non-zero = set), over batch and space."""
    a, b = np.asarray(a) != 0, np.asarray(b) != 0
    dims = (0, 2, 3, 4)
    return np.stack([(a & b).sum(dims), a.sum(dims), b.sum(dims)], axis=1).astype(np.int64)


def emulate_map(m, C, k, classes=None, reference=None, defect=None):
    """The passes of csrc/fill_holes.hip on one map, step by step: (out, filled [C], tallies [C, 3] or None).  ``defect``: None or
    one of DEFECTS, planted in the step it names."""
    assert defect is None or defect in DEFECTS, defect
    m = np.asarray(m, dtype=np.uint8)
    D, H, W = m.shape
    class_mask = 0
    for c in (range(1, C) if classes is None else classes):
        class_mask |= 1 << int(c)
    # init + merge + flatten: the root of every zero voxel
    r = roots(m == 0, k).ravel()
    flat = m.ravel()
    # border: one flag per root, from the voxels of the six faces
    border = np.zeros(m.size, dtype=bool)
    faces = face_mask(m.shape)
    if defect == "border_face_missing":
        faces[:, :, -1] = False
        faces[0], faces[-1], faces[:, 0], faces[:, -1], faces[:, :, 0] = (True,) * 5
    for p in np.flatnonzero(faces.ravel()):
        if r[p] >= 0:
            border[r[p]] = True
    # neighbours: a 64-bit set per root without a flag; bit 0 = a value >= C or an unselected class
    ring = offsets(1 if defect == "ring_connectivity_1" else k)
    sets = {}
    for p in np.flatnonzero(r >= 0):
        if border[r[p]]:
            continue
        d, h, w = np.unravel_index(p, m.shape)
        bits = 0
        for dz, dy, dx in ring:
            z, y, x = d + dz, h + dy, w + dx
            if not (0 <= z < D and 0 <= y < H and 0 <= x < W):
                continue
            val = int(m[z, y, x])
            if val == 0:
                continue
            if val >= C:
                bits |= 0 if defect == "value_ge_C_absent" else 1
            elif class_mask >> val & 1 or defect == "unselected_filled":
                bits |= 1 << val
            else:
                bits |= 1
        sets[int(r[p])] = sets.get(int(r[p]), 0) | bits
    # fill: no flag, and the set is exactly one bit >= 1
    out, filled = flat.copy(), np.zeros(C, dtype=np.int64)
    for p in np.flatnonzero(r >= 0):
        if border[r[p]]:
            continue
        s = sets.get(int(r[p]), 0)
        if defect == "two_classes_lower" and s > 1 and not s & 1:
            s &= -s                                             # the lowest class of several
        if s > 1 and s & (s - 1) == 0:
            c = s.bit_length() - 1
            out[p] = c
            filled[c] += 1
    out = out.reshape(m.shape)
    t = None
    if reference is not None:
        t = tallies_map(m if defect == "tallies_miss_filled" else out, np.asarray(reference), C)
    return out, filled, t


class Golden:
    """The fixture: ``maps`` is a list of dicts (name, map, C, k, classes or None, out, filled, ref, tallies); ``mask`` the
    [N, C, D, H, W] uint8 mask and ``mask_out[k]`` binary_fill_holes of every volume."""

    def __init__(self, path=GOLDEN):
        z = np.load(path)
        self.maps = []
        for name in z["map_names"].tolist():
            C, k = (int(x) for x in z[f"map/{name}/params"])
            classes = tuple(int(c) for c in z[f"map/{name}/classes"]) or None
            self.maps.append(dict(name=name, map=z[f"map/{name}/in"], C=C, k=k, classes=classes, out=z[f"map/{name}/out"],
                                  filled=z[f"map/{name}/filled"], ref=z[f"map/{name}/ref"], tallies=z[f"map/{name}/tallies"]))
        self.mask = z["mask/in"]
        self.mask_out = {k: z[f"mask/out_k{k}"] for k in (1, 2, 3)}

    def named(self, prefix):
        return [c for c in self.maps if c["name"].startswith(prefix)]
