"""Generate tests/golden/surface_dice_golden.npz: Normalized Surface Dice in the voxel-count form (the form of MONAI's
SurfaceDiceMetric; restated here with scipy, which is the arbiter) on the CPU, in fp64.

    PYTHONDONTWRITEBYTECODE=1 python tools/make_surface_dice_golden.py

border(X) = X & ~binary_erosion(X, generate_binary_structure(3, k), border_value=0); d_AB = distance_transform_edt(~border(B),
sampling=s)[border(A)] (+inf when border(B) is empty); within_AB(tau) = #{d_AB <= tau}; nsd = (within_AB + within_BA) /
(|border A| + |border B|); NaN when both borders are empty.  The wrapper rule of the distance table (a full mask -> NaN) does
not apply.  The tests only read the committed fixture (scipy is not needed to run them).

The cases are the masks of tests/golden/surface_metrics_golden.npz plus both_empty, identical and shifted_one_voxel.  The tool
enforces a gap condition and exits non-zero when it fails: for every attained finite distance d and every tolerance tau, either
d == tau exactly or |d - tau| > 1e-9 max(1, tau).  With it the counts do not depend on d <= tau versus d^2 <= tau^2, nor on
the order in which a squared distance is summed.

Contents: names, shapes int32 [cases, 3], test / reference (np.packbits of each flattened mask, concatenated; offsets int64
[cases + 1] in bytes), spacings fp64 [3, 3], connectivities int32 [2], tolerances fp64 [6], and for [cases, spacings,
connectivities]: n_a, n_b int64; within_ab, within_ba int64 [..., 6]; nsd fp64 [..., 6].
"""
import os
import sys

import numpy as np
from scipy import ndimage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "golden", "surface_metrics_golden.npz")
OUT = os.path.join(ROOT, "tests", "golden", "surface_dice_golden.npz")
SPACINGS = np.array([[1.0, 1.0, 1.0], [2.0, 1.5, 1.5], [0.8, 0.7, 1.3]])
CONNECTIVITIES = np.array([1, 3], dtype=np.int32)
TOLERANCES = np.array([0.0, 1.0, 1.5, 2.0, 3.0, 5.0])
GAP = 1e-9


def _ellipsoid(shape, centre, radii):
    g = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")
    return sum(((x - c) / r) ** 2 for x, c, r in zip(g, centre, radii)) <= 1.0


def cases():
    z = np.load(SRC)
    out = []
    for i, name in enumerate(z["names"]):
        shape = tuple(int(v) for v in z["shapes"][i])
        n = int(np.prod(shape))
        o0, o1 = int(z["offsets"][i]), int(z["offsets"][i + 1])
        out.append((str(name), np.unpackbits(z["test"][o0:o1])[:n].reshape(shape).astype(bool),
                    np.unpackbits(z["reference"][o0:o1])[:n].reshape(shape).astype(bool)))
    s = (9, 8, 10)
    out.append(("both_empty", np.zeros(s, bool), np.zeros(s, bool)))
    s = (14, 13, 16)
    e = _ellipsoid(s, (6.5, 6, 7), (4.5, 4, 5))
    out.append(("identical", e, e.copy()))
    moved = np.zeros_like(e)
    moved[:, :, 1:] = e[:, :, :-1]
    out.append(("shifted_one_voxel", e, moved))
    return out


def border(x, k):
    return x & ~ndimage.binary_erosion(x, structure=ndimage.generate_binary_structure(3, int(k)), iterations=1, border_value=0)


def directed(ba, bb, spacing):
    if not bb.any():
        return np.full(int(ba.sum()), np.inf)
    return ndimage.distance_transform_edt(~bb, sampling=spacing)[ba]


def check_gap(d, what):
    """Every finite distance is either exactly a tolerance or clearly away from it; returns the smallest non-zero relative gap."""
    d = np.unique(d[np.isfinite(d)])
    smallest = np.inf
    for tau in TOLERANCES:
        gap = np.abs(d - tau) / max(1.0, tau)
        bad = (gap != 0) & (gap <= GAP)
        if bad.any():
            print(f"gap condition fails: {what}, tau={tau}, distances {d[bad]}", file=sys.stderr)
            sys.exit(1)
        if (gap != 0).any():
            smallest = min(smallest, gap[gap != 0].min())
        # the squared comparison must agree with the unsquared one
        if not np.array_equal(d <= tau, d * d <= tau * tau):
            print(f"squared and unsquared comparisons differ: {what}, tau={tau}", file=sys.stderr)
            sys.exit(1)
    return smallest


def main():
    cs = cases()
    shape = (len(cs), len(SPACINGS), len(CONNECTIVITIES))
    n_a, n_b = np.zeros(shape, np.int64), np.zeros(shape, np.int64)
    wab, wba = np.zeros(shape + (len(TOLERANCES),), np.int64), np.zeros(shape + (len(TOLERANCES),), np.int64)
    nsd = np.zeros(shape + (len(TOLERANCES),), np.float64)
    packed_a, packed_b, offs = [], [], [0]
    smallest = np.inf
    for i, (name, a, b) in enumerate(cs):
        pa, pb = np.packbits(a.ravel()), np.packbits(b.ravel())
        packed_a.append(pa); packed_b.append(pb); offs.append(offs[-1] + len(pa))
        for j, sp in enumerate(SPACINGS):
            for m, k in enumerate(CONNECTIVITIES):
                ba, bb = border(a, k), border(b, k)
                dab, dba = directed(ba, bb, sp), directed(bb, ba, sp)
                smallest = min(smallest, check_gap(np.hstack((dab, dba)), (name, tuple(sp), int(k))))
                n_a[i, j, m], n_b[i, j, m] = ba.sum(), bb.sum()
                for t, tau in enumerate(TOLERANCES):
                    wab[i, j, m, t], wba[i, j, m, t] = (dab <= tau).sum(), (dba <= tau).sum()
                den = n_a[i, j, m] + n_b[i, j, m]
                nsd[i, j, m] = (wab[i, j, m] + wba[i, j, m]).astype(np.float64) / np.float64(den) if den else np.nan
    np.savez_compressed(OUT, names=np.array([c[0] for c in cs]), shapes=np.array([c[1].shape for c in cs], dtype=np.int32),
                        test=np.concatenate(packed_a), reference=np.concatenate(packed_b), offsets=np.array(offs, dtype=np.int64),
                        spacings=SPACINGS, connectivities=CONNECTIVITIES, tolerances=TOLERANCES, n_a=n_a, n_b=n_b,
                        within_ab=wab, within_ba=wba, nsd=nsd)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes, {len(cs)} cases); smallest non-zero relative gap {smallest:.3g}")


if __name__ == "__main__":
    main()
