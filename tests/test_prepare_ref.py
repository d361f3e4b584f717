"""The fp64 restatement of the case-preparation contract (tests/prepare_ref.py) and the host geometry of the package
(diff_unet_amos_amd/prepare.py), without a GPU: the restatement against scipy.ndimage.map_coordinates, the tie rule, the
rounding of n_out, all 48 orientations with and without an oblique perturbation, the restore geometry and the prepared
affine."""
import numpy as np
import pytest

import prepare_ref as R
from diff_unet_amos_amd import prepare as P

SHAPE = (13, 10, 7)
SPACING = (0.78, 2.9, 5.0)
PIXDIM = (1.5, 1.5, 2.0)


def _case(shape=SHAPE, seed=0, air=0.3):
    """An int16 scan with air (below a_min), soft tissue and bone (above a_max), and a label map of 4 classes."""
    rng = np.random.default_rng(seed)
    image = rng.integers(-400, 500, size=shape).astype(np.int16)
    image[rng.random(shape) < air] = -1000
    label = rng.integers(0, 4, size=shape).astype(np.uint8)
    return image, label


def _rotation(axis, degrees):
    axis = np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)
    k = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    t = np.deg2rad(degrees)
    return np.eye(3) + np.sin(t) * k + (1 - np.cos(t)) * (k @ k)


def test_restatement_against_scipy():
    from scipy import ndimage
    image, label = _case()
    image[0, 0, 0] = image[-1, -1, -1] = 100                 # the box is the whole volume
    ref = R.prepare(image, label, R.signed_permutation_affine((0, 1, 2), (1, 1, 1), SPACING), PIXDIM)
    assert ref["shape"] == (7, 18, 16) and ref["box"] == ((0, 13), (0, 10), (0, 7))
    for x in ref["coords"]:                                  # scipy's order-0 tie rule is not the contract's: this case has no tie
        assert not np.any(np.abs(x - np.floor(x) - 0.5) < 1e-9)
    grid = np.stack(np.meshgrid(*ref["coords"], indexing="ij"))
    want = ndimage.map_coordinates(R.window(image), grid, order=1, mode="nearest")
    err = float(np.abs(ref["image"] - want).max())
    print(f"restatement vs scipy order 1: max |d| = {err:.3e}")
    # one ulp of fp64 at 1 (2^-52 = 2.2e-16): two fp64 evaluations of the same 8-term sum in different orders cannot be asked
    # to agree more closely, and every order tried (separable in any axis order, the 8-corner sum) differs from scipy by
    # exactly this much somewhere
    assert err <= 2.0 ** -52
    want_label = ndimage.map_coordinates(label, grid, order=0, mode="nearest")
    assert ref["label"].size == 2016 and int((ref["label"] != want_label).sum()) == 0


def test_ties_round_half_to_even():
    n_out, x = R.axis_coords(9, 1.0, 2.5)
    assert n_out == 4 and x.tolist() == [0.0, 2.5, 5.0, 7.5]
    assert np.rint(x).astype(int).tolist() == [0, 2, 5, 8]
    n, lo, weight, nearest, xs = P.spacing_tables(9, 1.0, 2.5)
    assert n == 4 and xs.tolist() == x.tolist() and nearest.tolist() == [0, 2, 5, 8]
    assert lo.tolist() == [0, 2, 5, 7] and weight.tolist() == [0.0, 0.5, 0.0, 0.5]
    assert P.restore_table(4, 2.5, 1.0, 9).tolist() == [0, 2, 5, 8]           # 0, 2.5, 5, 7.5 on the way back
    assert P.restore_table(9, 1.0, 2.5, 4).tolist() == [0, 0, 1, 1, 2, 2, 2, 3, 3]   # 0.4 k; 2 / 2.5 = 0.8 -> 1


def test_n_out_rounds_half_to_even_and_the_coordinate_is_clamped():
    assert R.axis_coords(4, 1.0, 1.2)[0] == 3                # 3 / 1.2 = 2.5 -> 2
    assert R.axis_coords(8, 1.0, 2.0)[0] == 5                # 7 / 2 = 3.5 -> 4
    n_out, x = R.axis_coords(8, 1.0, 2.0)                    # (n_out - 1) r = 8 > n_in - 1 = 7: the last coordinate is clamped
    assert x.tolist() == [0.0, 2.0, 4.0, 6.0, 7.0]
    n, lo, weight, nearest, xs = P.spacing_tables(8, 1.0, 2.0)
    assert (n, xs.tolist()) == (5, x.tolist()) and lo.tolist() == [0, 2, 4, 6, 6] and weight.tolist() == [0, 0, 0, 0, 1]
    assert nearest.tolist() == [0, 2, 4, 6, 7]
    for n_in, s_in, s_out in ((4, 1.0, 1.2), (13, 0.78, 1.5), (10, 2.9, 1.5), (7, 5.0, 2.0), (2, 3.0, 7.0), (5, 1.0, 1.0)):
        n_ref, x_ref = R.axis_coords(n_in, s_in, s_out)
        n, lo, weight, nearest, xs = P.spacing_tables(n_in, s_in, s_out)
        assert n == n_ref and np.array_equal(xs, x_ref) and xs.max() <= n_in - 1
        assert np.array_equal(nearest, np.rint(x_ref)) and lo.min() >= 0 and lo.max() <= max(n_in - 2, 0)
        assert np.array_equal(weight, (x_ref - lo).astype(np.float32)) and weight.min() >= 0 and weight.max() <= 1
    for s_out in (0.3, 1.0, 4.0):                            # one voxel stays one voxel: lo 0, weight 0
        n, lo, weight, nearest, xs = P.spacing_tables(1, 1.0, s_out)
        assert (n, lo.tolist(), weight.tolist(), nearest.tolist()) == (1, [0], [0.0], [0])
        assert R.axis_coords(1, 1.0, s_out)[0] == 1


@pytest.mark.parametrize("perm,signs", R.all_signed_permutations())
def test_orientation_is_recovered(perm, signs):
    affine = R.signed_permutation_affine(perm, signs, SPACING, origin=(3.0, -2.0, 7.0))
    want = [[perm[a], signs[a]] for a in range(3)]
    assert P.orientation_from_affine(affine).tolist() == want
    assert [list(o) for o in R.io_orientation(affine)] == want
    rng = np.random.default_rng(perm[0] * 100 + perm[1] * 10 + (signs[0] + 1) * 4 + (signs[1] + 1) * 2 + (signs[2] + 1))
    for _ in range(4):                                       # oblique by up to 20 degrees: the same answer
        oblique = affine.copy()
        oblique[:3, :3] = _rotation(rng.normal(size=3), rng.uniform(-20, 20)) @ affine[:3, :3]
        got = P.orientation_from_affine(oblique)
        assert got.tolist() == want
        assert sorted(got[:, 0].tolist()) == [0, 1, 2]       # each world axis, so each source axis, claimed once
        assert [list(o) for o in R.io_orientation(oblique)] == want


def test_all_48_axis_codes_are_accepted_and_nothing_else():
    assert len(set(R.ALL_AXCODES)) == 48
    affine = R.signed_permutation_affine((1, 2, 0), (1, -1, -1), SPACING)
    for code in R.ALL_AXCODES:
        g = P.prepared_geometry(SHAPE, ((1, 12), (0, 9), (2, 7)), affine, PIXDIM, code)
        perm, flip = R.axis_plan(affine, code)
        assert (g.perm, g.flip) == (perm, flip)
    for bad in ("RAA", "RA", "RASI", "XYZ", "RLS"):
        with pytest.raises(ValueError, match="axcodes"):
            P.prepared_geometry(SHAPE, ((0, 13), (0, 10), (0, 7)), affine, PIXDIM, bad)
    zero = affine.copy()
    zero[:3, 1] = 0
    with pytest.raises(ValueError, match="zero column"):
        P.orientation_from_affine(zero)
    with pytest.raises(ValueError, match="finite"):
        P.orientation_from_affine(np.full((4, 4), np.nan))


@pytest.mark.parametrize("perm,signs", R.all_signed_permutations())
def test_geometry_agrees_with_the_restatement_and_restore_inverts_it(perm, signs):
    """The strides, base and tables of the package address exactly the voxels the restatement's transpose / flip / take pick,
    and source -> prepared -> restore is the identity on voxel indices inside the box when no axis is coarsened."""
    image, _ = _case(seed=1)
    image[:, :, 0] = -1000
    image[0] = -1000                                         # a box that is not the whole volume
    affine = R.signed_permutation_affine(perm, signs, SPACING, origin=(1.0, 2.0, 3.0))
    ids = np.arange(image.size, dtype=np.int64).reshape(image.shape)          # a "label" that names its own voxel
    for pixdim in ((0.78, 0.78, 0.78), PIXDIM):
        ref = R.prepare(image, None, affine, pixdim)
        g = P.prepared_geometry(image.shape, ref["box"], affine, pixdim)
        assert (g.perm, g.flip, g.n_in, g.shape, g.box) == (ref["perm"], ref["flip"], ref["n_in"], ref["shape"], ref["box"])
        assert np.allclose(g.affine, ref["affine"], rtol=0, atol=1e-12)
        # what the kernel reads for the label: base + sum nearest_j stride_j
        off = g.base + sum(np.asarray(g.nearest[j], dtype=np.int64).reshape([-1 if a == j else 1 for a in range(3)]) * g.stride[j]
                           for j in range(3))
        want = R._oriented(ids, ref["box"], ref["perm"], ref["flip"])[np.ix_(*[np.rint(x).astype(np.int64) for x in ref["coords"]])]
        assert np.array_equal(off, want)
        lo_off = g.base + sum(np.asarray(g.lo[j], dtype=np.int64).reshape([-1 if a == j else 1 for a in range(3)]) * g.stride[j]
                              for j in range(3))
        assert lo_off.min() >= 0 and lo_off.max() < image.size
        # restore: the package's premultiplied tables against the restatement's indices
        tabs = R.restore_indices(ref)
        out_stride = (g.shape[1] * g.shape[2], g.shape[2], 1)
        for axis in range(3):
            j = ref["perm"].index(axis)
            assert np.array_equal(g.restore[axis], np.where(tabs[axis] >= 0, tabs[axis] * out_stride[j], -1))
        if all(so <= si for so, si in zip(pixdim, ref["s_in"])):              # one-to-one forwards: restore(prepare(ids)) == ids
            prepared = want.reshape(-1)
            back = prepared[np.add.outer(np.add.outer(g.restore[0], g.restore[1]), g.restore[2])]
            inside = np.ix_(*[t >= 0 for t in tabs])
            assert np.array_equal(back[inside], ids[inside])


def test_restore_restatement_round_trip_and_zero_fill():
    image, label = _case(seed=2)
    image[:2] = -1000
    image[:, -1] = -1000
    affine = R.signed_permutation_affine((2, 0, 1), (-1, 1, -1), (2.0, 1.5, 4.0))
    ref = R.prepare(image, label, affine, (1.5, 1.5, 2.0))                    # every axis refined or kept
    back = R.restore(ref["label"], ref)
    inside = tuple(slice(lo, hi) for lo, hi in ref["box"])
    assert np.array_equal(back[inside], label[inside])
    outside = np.ones(image.shape, dtype=bool)
    outside[inside] = False
    assert not back[outside].any() and outside.any()
    stacked = R.restore(np.stack([ref["label"], ref["label"] + 1]), ref)
    assert stacked.shape == (2,) + image.shape and np.array_equal(stacked[0], back)


@pytest.mark.parametrize("perm,signs", [((0, 1, 2), (1, 1, 1)), ((1, 2, 0), (-1, 1, -1)), ((2, 1, 0), (1, -1, -1))])
def test_prepared_affine_puts_the_corners_where_the_source_voxels_are(perm, signs):
    image, _ = _case(seed=3)
    image[-1] = -1000
    image[:, 0] = -1000
    affine = R.signed_permutation_affine(perm, signs, SPACING, origin=(-11.0, 4.5, 30.0))
    affine[:3, :3] = _rotation((1.0, 2.0, -1.0), 12.0) @ affine[:3, :3]
    # target spacings chosen per SOURCE axis so that no far coordinate is clamped: 11 * 0.78 / 1.6 = 5.36 -> 5,
    # 8 * 2.9 / 1.5 = 15.47 -> 15, 6 * 5 / 2 = 15 (a clamped corner reads a voxel the affine cannot name)
    pixdim = tuple((1.6, 1.5, 2.0)[a] for a in R.axis_plan(affine)[0])
    ref = R.prepare(image, None, affine, pixdim)
    g = P.prepared_geometry(image.shape, ref["box"], affine, pixdim)
    norms = np.linalg.norm(g.affine[:3, :3], axis=0)
    assert np.allclose(norms, pixdim, rtol=1e-12)            # only the column norms change: the rotation is kept
    for corner in ((0, 0, 0), tuple(n - 1 for n in g.shape)):
        # the fractional source index this prepared voxel reads, from the restatement's coordinates (none is clamped here)
        src = np.zeros(4)
        src[3] = 1
        for j in range(3):
            x = ref["coords"][j][corner[j]]
            assert x == corner[j] * pixdim[j] / ref["s_in"][j]
            lo, hi = ref["box"][ref["perm"][j]]
            src[ref["perm"][j]] = hi - 1 - x if ref["flip"][j] else lo + x
        assert np.allclose(g.affine @ np.array(corner + (1,), dtype=np.float64), affine @ src, rtol=0, atol=1e-9)
        assert np.allclose(ref["affine"] @ np.array(corner + (1,), dtype=np.float64), affine @ src, rtol=0, atol=1e-9)


def test_the_bound_is_a_small_multiple_of_the_fp32_round_off():
    assert 13 * 2.0 ** -24 < R.image_bound() < 14 * 2.0 ** -24


def test_argument_errors_of_the_host_geometry():
    affine = R.signed_permutation_affine((0, 1, 2), (1, 1, 1), SPACING)
    with pytest.raises(ValueError, match="box"):
        P.prepared_geometry(SHAPE, ((0, 14), (0, 10), (0, 7)), affine)
    with pytest.raises(ValueError, match="pixdim"):
        P.prepared_geometry(SHAPE, ((0, 13), (0, 10), (0, 7)), affine, pixdim=(1.5, 0.0, 2.0))
    with pytest.raises(ValueError, match="affine"):
        P.prepared_geometry(SHAPE, ((0, 13), (0, 10), (0, 7)), np.eye(3))
    with pytest.raises(ValueError, match="spacing_tables"):
        P.spacing_tables(0, 1.0, 1.0)
