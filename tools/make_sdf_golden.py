#!/usr/bin/env python
"""Writes tests/golden/sdf_golden.npz: for every (shape, kind) of tests/sdf_ref.py, in that order, the mask { y > 0.5 } as packed
bits ("masks", end to end) and the integer squared distances scipy's distance_transform_edt gives (of the mask inside it, of its
complement outside it; 0 for a volume without both sets) as int32 -- as they are, or as their differences along W where that
packs smaller ("delta": 1; np.cumsum(.., -1) restores them) -- end to end in one xz stream ("d2_xz").  The tests need numpy and
the standard library only (tests/sdf_ref.py: load_golden).

    python tools/make_sdf_golden.py
"""
import os
import sys
import lzma

import numpy as np
from scipy import ndimage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sdf_ref  # noqa: E402


def scipy_d2(pos):
    out = np.zeros(pos.shape, np.int32)
    for n in range(pos.shape[0]):
        for c in range(pos.shape[1]):
            m = pos[n, c]
            if m.any() and not m.all():
                e = np.where(m, ndimage.distance_transform_edt(m), ndimage.distance_transform_edt(~m))
                d2 = np.rint(e * e).astype(np.int64)
                assert np.abs(np.sqrt(d2.astype(np.float64)) - e).max() < 1e-9
                out[n, c] = d2
    return out


def main():
    masks, words, delta = [], [], []
    for shape in sdf_ref.SHAPES:
        for kind in sdf_ref.KINDS:
            pos = sdf_ref.make_labels(shape, kind) > np.float32(0.5)
            masks.append(np.packbits(pos.reshape(-1)))
            d2 = scipy_d2(pos)
            dd2 = np.diff(d2, axis=-1, prepend=np.int32(0))
            assert dd2.dtype == np.int32 and np.array_equal(np.cumsum(dd2, -1, dtype=np.int32), d2)
            smaller = len(lzma.compress(dd2.tobytes())) < len(lzma.compress(d2.tobytes()))
            delta.append(smaller)
            words.append((dd2 if smaller else d2).reshape(-1))
    stream = lzma.compress(np.concatenate(words).tobytes(), preset=9 | lzma.PRESET_EXTREME)
    path = os.path.join(ROOT, "tests", "golden", "sdf_golden.npz")
    np.savez_compressed(path, masks=np.concatenate(masks), delta=np.array(delta, np.uint8),
                        d2_xz=np.frombuffer(stream, np.uint8))
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
