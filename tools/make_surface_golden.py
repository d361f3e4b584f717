"""Generate tests/golden/surface_metrics_golden.npz: the surface-distance metrics of metric.py:314-390 (medpy.metric.binary
hd / hd95 / asd / assd behind the reference's wrappers) computed with scipy on the CPU, in fp64.

    PYTHONDONTWRITEBYTECODE=1 python tools/make_surface_golden.py

medpy is restated with scipy: border(X) = X & ~binary_erosion(X, generate_binary_structure(3, k), border_value=0),
sds(A, B) = distance_transform_edt(~border(B), sampling=s)[border(A)], then max / np.percentile(., 95) / mean; the wrapper
returns NaN when a mask is empty or full.  The tests only read the committed fixture (scipy is not needed to run them).

Contents: names (the cases), shapes int32 [cases, 3], test / reference: np.packbits of each case's flattened mask,
concatenated (offsets int64 [cases + 1] in bytes), spacings fp64 [2, 3], connectivities int32 [2], expected fp64
[cases, spacings, connectivities, 4] = (hd, hd95, asd, assd) with NaN under the wrapper rule.
"""
import os

import numpy as np
from scipy import ndimage

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "surface_metrics_golden.npz")
SPACINGS = np.array([[1.0, 1.0, 1.0], [2.0, 1.5, 1.5]])
CONNECTIVITIES = np.array([1, 3], dtype=np.int32)


def _ellipsoid(shape, centre, radii):
    g = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")
    return sum(((x - c) / r) ** 2 for x, c, r in zip(g, centre, radii)) <= 1.0


def cases():
    rng = np.random.default_rng(7)
    out = []
    s = (24, 20, 18)
    out.append(("blobs", _ellipsoid(s, (11, 9, 8), (7, 6, 5)), _ellipsoid(s, (13, 10, 9), (6, 7, 4.5))))
    a = np.zeros((16, 14, 12), bool); a[5, 2:12, 1:10] = True
    b = np.zeros((16, 14, 12), bool); b[9, 4:14, 3:12] = True
    out.append(("sheets", a, b))
    a = np.zeros((9, 11, 13), bool); a[2, 3, 4] = True
    b = np.zeros((9, 11, 13), bool); b[7, 8, 1] = True
    out.append(("single_voxels", a, b))
    a = np.zeros((12, 10, 14), bool); a[:5, :, 3:9] = True
    b = np.zeros((12, 10, 14), bool); b[4:, 2:8, 7:] = True
    out.append(("touching_faces", a, b))
    noise = ndimage.gaussian_filter(rng.standard_normal((20, 17, 15)), 1.6)
    out.append(("random_blobs", noise > 0.05, ndimage.gaussian_filter(rng.standard_normal((20, 17, 15)), 1.6) > 0.0))
    s = (10, 12, 9)
    out.append(("empty_test", np.zeros(s, bool), _ellipsoid(s, (5, 6, 4), (3, 4, 3))))
    out.append(("full_reference", _ellipsoid(s, (4, 5, 4), (3, 3, 3)), np.ones(s, bool)))
    a = np.zeros((7, 5, 9), bool); a[1:6, 2, 4] = True; a[3, 0:5, 4] = True
    b = np.zeros((7, 5, 9), bool); b[3, 2, 0:9] = True; b[0, 0, 0] = True
    out.append(("lines", a, b))
    return out


def border(x, k):
    return x & ~ndimage.binary_erosion(x, structure=ndimage.generate_binary_structure(3, int(k)), iterations=1, border_value=0)


def metrics(a, b, spacing, k):
    if not a.any() or a.all() or not b.any() or b.all():
        return [np.nan] * 4
    ba, bb = border(a, k), border(b, k)
    sab = ndimage.distance_transform_edt(~bb, sampling=spacing)[ba]
    sba = ndimage.distance_transform_edt(~ba, sampling=spacing)[bb]
    return [max(sab.max(), sba.max()), np.percentile(np.hstack((sab, sba)), 95), sab.mean(), (sab.mean() + sba.mean()) / 2]


def main():
    cs = cases()
    packed_a, packed_b, offs = [], [], [0]
    expected = np.zeros((len(cs), len(SPACINGS), len(CONNECTIVITIES), 4))
    for i, (_, a, b) in enumerate(cs):
        pa, pb = np.packbits(a.ravel()), np.packbits(b.ravel())
        packed_a.append(pa); packed_b.append(pb); offs.append(offs[-1] + len(pa))
        for j, sp in enumerate(SPACINGS):
            for m, k in enumerate(CONNECTIVITIES):
                expected[i, j, m] = metrics(a, b, sp, k)
    np.savez_compressed(OUT, names=np.array([c[0] for c in cs]), shapes=np.array([c[1].shape for c in cs], dtype=np.int32),
                        test=np.concatenate(packed_a), reference=np.concatenate(packed_b), offsets=np.array(offs, dtype=np.int64),
                        spacings=SPACINGS, connectivities=CONNECTIVITIES, expected=expected)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes, {len(cs)} cases)")


if __name__ == "__main__":
    main()
