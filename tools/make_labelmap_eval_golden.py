#!/usr/bin/env python3
"""Writes tests/golden/labelmap_eval_golden.npz: the label maps of tests/labelmap_eval_ref.py, the scipy.ndimage.label result
of every class of every map at the three connectivities (labels and counts of (map == c)), and the outputs of its filter cases
(scipy's per-class labels, numpy's stable argsort per class).  scipy is needed here only, on the CPU; the tests read the file.

    python tools/make_labelmap_eval_golden.py            # write the file
    python tools/make_labelmap_eval_golden.py --check    # recompute and compare with the committed file, array by array

A map is stored as the bit-packed masks of its values 0 .. C + 1 (np.packbits over the flattened one-hot array), labels are
uint16, filter outputs are bit-packed the same way."""
import argparse
import os
import sys

import numpy as np
from scipy import ndimage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import labelmap_eval_ref as LR  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "labelmap_eval_golden.npz")
VALUES = LR.C + 2


def pack(m):
    """The one-hot masks of the values 0 .. C + 1 of a map, bit-packed."""
    return np.packbits((np.asarray(m)[None] == np.arange(VALUES).reshape(-1, *([1] * m.ndim))).ravel())


def unpack(bits, shape):
    onehot = np.unpackbits(bits)[:VALUES * int(np.prod(shape))].reshape(VALUES, *shape)
    return onehot.argmax(axis=0).astype(np.uint8)


def scipy_label(volume, connectivity):
    lab, count = ndimage.label(volume, ndimage.generate_binary_structure(3, connectivity))
    assert count < 65536
    return lab.astype(np.uint16), count


def filter_volume(m, connectivity, k, min_size, classes):
    out = m.copy()
    for c in range(1, LR.C) if classes is None else classes:
        lab, count = scipy_label(m == c, connectivity)
        sz = np.bincount(lab.ravel(), minlength=count + 1)[1:]
        order = np.argsort(-sz, kind="stable")
        order = order[:k] if k > 0 else order
        kept = [l + 1 for l in order if sz[l] >= min_size]
        out[(m == c) & ~np.isin(lab, kept)] = 0
    return out


def build():
    g = {}
    for name, make in LR.MAPS.items():
        maps = make()
        g[f"{name}_shape"] = np.asarray(maps.shape, np.int32)
        g[f"{name}_map"] = pack(maps)
        assert np.array_equal(unpack(g[f"{name}_map"], maps.shape), maps)
        for conn in LR.CONNECTIVITIES:
            labs = np.zeros((maps.shape[0], LR.C, *maps.shape[1:]), np.uint16)
            counts = np.zeros((maps.shape[0], LR.C), np.int32)
            for n, m in enumerate(maps):
                for c in range(1, LR.C):
                    labs[n, c], counts[n, c] = scipy_label(m == c, conn)
            g[f"{name}_c{conn}_labels"], g[f"{name}_c{conn}_counts"] = labs, counts
    for name, (maker, conn, k, min_size, classes) in LR.FILTER_CASES.items():
        maps = LR.MAPS[maker]()
        g[f"filter_{name}"] = pack(np.stack([filter_volume(m, conn, k, min_size, classes) for m in maps]))
    return g


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--check", action="store_true", help="compare with the committed file instead of writing it")
    args = ap.parse_args()
    g = build()
    if args.check:
        have = np.load(OUT)
        assert sorted(have.files) == sorted(g), "the committed file holds other arrays"
        for k, v in g.items():
            assert have[k].dtype == v.dtype and np.array_equal(have[k], v), k
        print(f"{OUT}: {len(g)} arrays reproduced")
        return
    np.savez_compressed(OUT, **g)
    print(f"{OUT}: {len(g)} arrays, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
