#!/usr/bin/env python
"""Writes tests/golden/fill_holes_golden.npz: the inputs of the fill-holes tests and what scipy says about them.

    python tools/make_fill_holes_golden.py

Needs numpy and scipy; the tests read only the fixture.  Two kinds of cases:

  mask/<name>/...  a mask [N, C, D, H, W] (uint8), per connectivity k = 1, 2, 3 the result of
                   scipy.ndimage.binary_fill_holes(volume, generate_binary_structure(3, k)) on every (n, c) volume, and the
                   filled voxel counts [N, C];
  map/<name>/...   a uint8 label map [D, H, W], its class count C, connectivity k, the selected classes (empty = all), and
                   the label-map rule of include/dua_hip.h restated with ndimage.label + binary_dilation: a k-connected
                   component of (map == 0) that touches no face and whose k-dilation ring carries one value c, 1 <= c < C and
                   c selected, becomes c.  Beside it a reference map and the Dice tallies (|A & B|, |A|, |B|) per class of
                   the filled map against it.

Every volume has a few thousand voxels at the most; the file stays far below the size limit for committed files."""
import os

import numpy as np
from scipy import ndimage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "fill_holes_golden.npz")


def structure(k):
    return ndimage.generate_binary_structure(3, k)


def fill_map_scipy(m, C, k, classes):
    """The label-map rule, with scipy's labelling and dilation."""
    chosen = set(range(1, C)) if classes is None else set(classes)
    out = m.copy()
    lab, n = ndimage.label(m == 0, structure(k))
    face = np.zeros(m.shape, dtype=bool)
    face[0], face[-1], face[:, 0], face[:, -1], face[:, :, 0], face[:, :, -1] = (True,) * 6
    for l in range(1, n + 1):
        comp = lab == l
        if (comp & face).any():
            continue
        ring = ndimage.binary_dilation(comp, structure(k)) & ~comp
        values = np.unique(m[ring])
        if len(values) == 1 and 1 <= int(values[0]) < C and int(values[0]) in chosen:
            out[comp] = values[0]
    return out


def tallies(a, b, C):
    return np.array([[((a == c) & (b == c)).sum(), (a == c).sum(), (b == c).sum()] for c in range(C)], dtype=np.int64)


def reference_for(m, rng):
    """A plausible ground truth: the map with every zero inside the bounding box of the non-zero voxels given the most common
    class, then a few voxels flipped, so that filling changes |A & B| as well as |A|."""
    ref = m.copy()
    nz = np.argwhere(m != 0)
    if len(nz):
        lo, hi = nz.min(0), nz.max(0) + 1
        box = ref[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]]
        vals, counts = np.unique(m[m != 0], return_counts=True)
        box[box == 0] = vals[counts.argmax()]
    flip = rng.random(m.shape) < 0.05
    ref[flip] = rng.integers(0, 4, size=int(flip.sum())).astype(np.uint8)
    return ref


def general_map(shape, C, rng, boxes=6, big_values=2):
    m = np.zeros(shape, dtype=np.uint8)
    for _ in range(boxes):
        lo = [int(rng.integers(0, max(1, s - 3))) for s in shape]
        hi = [min(s, l + int(rng.integers(3, max(4, s // 2 + 2)))) for s, l in zip(shape, lo)]
        m[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = rng.integers(1, C)
    holes = rng.random(shape) < 0.12                    # single voxels and small clusters of background inside the boxes
    m[holes] = 0
    for _ in range(big_values):
        m[tuple(int(rng.integers(0, s)) for s in shape)] = 200
    return m


def map_cases():
    rng = np.random.default_rng(20240611)
    cases = []

    def add(name, m, C, classes=None, ks=(1,)):
        for k in ks:
            cases.append((f"{name} k{k}", np.ascontiguousarray(m, dtype=np.uint8), C, k, classes))

    add("general 9x10x11", general_map((9, 10, 11), 5, rng), 5, ks=(1, 2, 3))
    # a degenerate axis: every voxel is on a face
    m = np.ones((1, 7, 8), np.uint8); m[0, 2:5, 3:6] = 0
    add("degenerate 1x7x8", m, 4, ks=(1, 3))
    # rows longer than a workgroup: an enclosed tunnel over most of a 300-voxel row with side rooms, and one open to the w face
    m = np.full((3, 5, 300), 2, np.uint8)
    m[1, 2, 5:201] = 0; m[1, 1, 40:44] = 0; m[1, 3, 150:190] = 0; m[1, 2, 250:300] = 0; m[1, 1, 270] = 0
    add("rows 3x5x300", m, 3, ks=(1, 2))
    add("tile plus one 17x16x16", general_map((17, 16, 16), 16, rng, boxes=9, big_values=5), 16, ks=(1, 3))
    # pockets open to the outside through a diagonal only: A over a 3-diagonal, B over a 2-diagonal
    m = np.ones((7, 7, 7), np.uint8)
    for p in ((2, 2, 2), (1, 1, 1), (0, 0, 0), (4, 4, 4), (4, 5, 5), (4, 6, 6)):
        m[p] = 0
    add("diagonal pockets", m, 2, ks=(1, 2, 3))
    # a pocket whose only opening is on one face, each of the six in turn, beside a closed pocket
    for axis in range(3):
        for side in (0, 1):
            m = np.ones((7, 7, 9), np.uint8)
            m[5, 5, 7] = 0
            idx = [3, 3, 4]
            idx[axis] = slice(0, idx[axis] + 1) if side == 0 else slice(idx[axis], None)
            m[tuple(idx)] = 0
            add(f"open on face axis{axis} side{side}", m, 2, ks=(1,))
    # a hole bordered by two classes
    m = np.ones((5, 5, 6), np.uint8); m[:, :, 3:] = 2; m[2, 2, 2:4] = 0
    add("two classes", m, 3, ks=(1, 3))
    # nested shells: class 1 around class 2 around background
    m = np.zeros((7, 7, 7), np.uint8); m[1:6, 1:6, 1:6] = 1; m[2:5, 2:5, 2:5] = 2; m[3, 3, 3] = 0
    add("nested shells", m, 3, ks=(1, 3))
    # a pocket of class 1 that holds an island of class 2: per-class binary_fill_holes would fill it, this rule does not
    m = np.ones((7, 7, 7), np.uint8); m[2:5, 2:5, 2:5] = 0; m[3, 3, 3] = 2
    add("island in pocket", m, 3, ks=(1, 2))
    # a value >= C next to a hole blocks it; the hole beside it is filled
    m = np.ones((5, 6, 9), np.uint8); m[2, 2, 2] = 0; m[2, 2, 3] = 200; m[2, 3, 6] = 0
    add("value 200", m, 16, ks=(1,))
    # the same geometry where 200 touches the hole only over a 3-diagonal: blocked under k = 3 alone
    m = np.ones((5, 6, 9), np.uint8); m[2, 2, 2] = 0; m[3, 3, 3] = 200
    add("value 200 diagonal", m, 16, ks=(1, 3))
    # holes in classes 1 and 2, only class 2 selected
    m = np.ones((6, 6, 10), np.uint8); m[:, :, 5:] = 2; m[2, 2, 2] = 0; m[3, 3, 7] = 0
    add("classes=[2]", m, 3, classes=(2,), ks=(1,))
    add("classes=all", m, 3, ks=(1,))
    # the top bit of the set
    m = np.full((4, 5, 6), 63, np.uint8); m[1:3, 2, 2:4] = 0; m[0, 0, 0] = 64
    add("class 63", m, 64, ks=(1,))
    # single-class maps: the map form against the mask form
    m = (general_map((8, 9, 10), 2, rng, boxes=5, big_values=0) != 0).astype(np.uint8) * 3
    add("single class 3", m, 5, ks=(1, 2, 3))
    return cases


def mask_case():
    rng = np.random.default_rng(7)
    mask = np.zeros((2, 3, 9, 10, 11), np.uint8)
    mask[0, 0] = general_map((9, 10, 11), 2, rng, big_values=0) != 0
    mask[0, 1] = 1; mask[0, 1, 3:6, 4:7, 2:9] = 0; mask[0, 1, 4, 5, 0:2] = 1; mask[0, 1, 1, 1, 1] = 0
    mask[1, 0] = 1                                     # all one; (0, 2) stays all zero
    mask[1, 1] = general_map((9, 10, 11), 2, rng, boxes=8, big_values=0) != 0
    mask[1, 2] = 1; mask[1, 2, 2:7, 2:8, 2:9] = 0; mask[1, 2, 3:6, 3:7, 3:8] = 1; mask[1, 2, 4, 4:6, 4:7] = 0
    mask[1, 2, 0, 5, 5] = 0; mask[1, 2, 1, 5, 5] = 0                                      # a shaft from the d = 0 face to the shell
    return mask


def main():
    data = {}
    names = []
    rng = np.random.default_rng(99)
    for name, m, C, k, classes in map_cases():
        out = fill_map_scipy(m, C, k, classes)
        if m.max() < C and len(np.unique(m[m != 0])) == 1:      # one class: the rule is binary_fill_holes
            c = int(m.max())
            if classes is None or c in classes:
                assert np.array_equal(out == c, ndimage.binary_fill_holes(m == c, structure(k))), name
        ref = reference_for(m, rng)
        filled = np.array([((out == c) & (m == 0)).sum() if c else 0 for c in range(C)], dtype=np.int64)
        names.append(name)
        data[f"map/{name}/in"] = m
        data[f"map/{name}/params"] = np.array([C, k], dtype=np.int64)
        data[f"map/{name}/classes"] = np.array([] if classes is None else classes, dtype=np.int64)
        data[f"map/{name}/out"] = out
        data[f"map/{name}/filled"] = filled
        data[f"map/{name}/ref"] = ref
        data[f"map/{name}/tallies"] = tallies(out, ref, C)
        print(f"{name:40s} {m.shape}  filled {int(filled.sum())}")
    data["map_names"] = np.array(names)
    mask = mask_case()
    data["mask/in"] = mask
    for k in (1, 2, 3):
        out = np.zeros_like(mask)
        for n in range(mask.shape[0]):
            for c in range(mask.shape[1]):
                out[n, c] = ndimage.binary_fill_holes(mask[n, c], structure(k))
        data[f"mask/out_k{k}"] = out
        print(f"mask k{k}: filled per volume {(out != mask).sum((2, 3, 4)).tolist()}")
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, **data)
    print(f"{OUT}: {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
