#!/usr/bin/env python3
"""Writes tests/golden/components_golden.npz: the masks of tests/components_ref.py labelled by scipy.ndimage.label, their
component counts and sizes at the three connectivities, and the keep-largest / min-size outputs of its filter cases (scipy's
labels, numpy's stable argsort).  scipy is needed here only; the tests read the file.

    python tools/make_components_golden.py            # write the file
    python tools/make_components_golden.py --check    # recompute and compare with the committed file, array by array

Masks and filter outputs are bit-packed (np.packbits over the flattened array), labels are uint16."""
import argparse
import os
import sys

import numpy as np
from scipy import ndimage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import components_ref as CR  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "components_golden.npz")


def scipy_label(volume, connectivity):
    lab, count = ndimage.label(volume, ndimage.generate_binary_structure(3, connectivity))
    assert count < 65536
    return lab.astype(np.uint16), count


def label_batch(masks, connectivity):
    """(labels uint16 like masks, counts int32 [V], sizes int32 [V, max count])"""
    labs, counts = zip(*(scipy_label(m, connectivity) for m in masks))
    cap = max(max(counts), 1)
    sizes = np.stack([np.bincount(l.ravel(), minlength=cap + 1)[1:cap + 1] for l in labs]).astype(np.int32)
    return np.stack(labs), np.asarray(counts, np.int32), sizes


def filter_volume(volume, connectivity, k, min_size, cap):
    lab, count = scipy_label(volume, connectivity)
    n = count if cap is None else min(count, cap)
    sz = np.bincount(lab.ravel(), minlength=count + 1)[1:n + 1]
    order = np.argsort(-sz, kind="stable")
    order = order[:k] if k > 0 else order
    kept = [l + 1 for l in order if sz[l] >= min_size]
    return np.isin(lab, kept).astype(np.uint8)


def build():
    g = {}
    for si in range(len(CR.RANDOM_SHAPES)):
        for fi in range(len(CR.RANDOM_FILLS)):
            masks = CR.random_masks(si, fi)
            g[f"random_s{si}_f{fi}_mask"] = np.packbits(masks.ravel())
            for c in CR.CONNECTIVITIES:
                lab, counts, sizes = label_batch(masks, c)
                g[f"random_s{si}_f{fi}_c{c}_labels"], g[f"random_s{si}_f{fi}_c{c}_counts"] = lab, counts
                g[f"random_s{si}_f{fi}_c{c}_sizes"] = sizes
    for name, make in CR.SPECIAL_MASKS.items():
        mask = make()
        g[f"{name}_mask"] = np.packbits(mask.ravel())
        g[f"{name}_shape"] = np.asarray(mask.shape, np.int32)
        for c in CR.CONNECTIVITIES:
            lab, counts, sizes = label_batch(mask[None], c)
            g[f"{name}_c{c}_labels"], g[f"{name}_c{c}_counts"], g[f"{name}_c{c}_sizes"] = lab[0], counts, sizes[0]
    for name, (make, c, k, min_size, cap) in CR.FILTER_CASES.items():
        g[f"filter_{name}"] = np.packbits(filter_volume(make(), c, k, min_size, cap).ravel())
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
