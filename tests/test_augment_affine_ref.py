"""tests/augment_affine_ref.py, the restatement the GPU tests of rotation and zoom compare the kernels with, pinned down on the
CPU first: against scipy.ndimage.affine_transform, against the plain apply for identity rows, the fp32 emulation against the
derived bound on every case the GPU test uses, planted defects that must each leave the bound or change a label on those
cases, and the event statistics of the seed the GPU test uses."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import augment_affine_ref as aref  # noqa: E402
import augment_ref as ref  # noqa: E402

F32, F64 = np.float32, np.float64


@pytest.fixture(scope="module")
def cases():
    """name -> (case, RefVolumes, fp64 batch, fp32 coordinates' labels): computed once, shared, left unchanged."""
    out = {}
    for name, case in aref.apply_cases().items():
        vols = [ref.RefVolume(image, label) for image, label in aref.case_volumes(case)]
        want = aref.apply(vols, case["ints"], case["floats"], case["rows"], case["roi"], case["class_ids"])
        out[name] = (case, vols, want)
    return out


def test_fp64_restatement_agrees_with_scipy():
    """With the coordinates in fp64 too, the lerp tree is scipy's order-1 spline and the nearest label its order 0.  scipy's
    mode="constant" answers cval wherever a coordinate lies outside [0, n - 1] and does not interpolate towards the pad, so it
    is the reference where every coordinate is inside the volume or the whole cell is outside; "grid-constant", which pads and
    then interpolates, is the contract's per-corner pad everywhere."""
    ndimage = pytest.importorskip("scipy.ndimage")
    shape, roi, pad = (23, 19, 27), (12, 10, 14), -3.5
    image, label = ref.synthetic_volume(shape, 7)
    vol = ref.RefVolume(image, label)
    checked = {"constant": 0, "grid-constant": 0, "labels": 0}
    for n, (deg, z, start) in enumerate((((30, -20, 10), 1.4, (5, 4, 6)), ((-30, 30, -30), 0.7, (0, 0, 0)),
                                         ((0, 0, 0), 1.0, (11, 9, 13)), ((12, 0, -7), 0.55, (3, 2, 1)))):
        t = [F32(math.tan(math.radians(d) / 2)) for d in deg]
        arow = aref.row(t, z, 3, pad)
        ints, floats = np.array([[0, *start, 0, 0]], dtype=np.int32), np.zeros((1, 2), dtype=F32)
        got, _, ids, _ = aref.apply([vol], ints, floats, [arow], roi, (0,), coord_dtype=F64)
        m = arow[:9].astype(F64).reshape(3, 3)
        half = (np.array(roi, dtype=F64) - 1) / 2
        offset = np.array(start, dtype=F64) + half - m @ half          # s = m (p - half) + start + half
        s = aref.coordinates(m, start, roi, aref.window_index(roi, 0, 0), dtype=F64)
        inside = np.all([(s[a] >= 0) & (s[a] <= shape[a] - 1) for a in range(3)], axis=0)
        far = np.any([(s[a] <= -1) | (s[a] >= shape[a]) for a in range(3)], axis=0)
        for mode, where in (("constant", inside | far), ("grid-constant", np.ones(roi, dtype=bool))):
            want = ndimage.affine_transform(image.double().numpy(), m, offset=offset, output_shape=roi, order=1, mode=mode, cval=pad)
            err = float(np.abs(got[0, 0] - want)[where].max())
            print(f"row {n} mode {mode}: {int(where.sum())} of {where.size} voxels, max |restatement - scipy| = {err:.3e}")
            assert err <= 1e-12
            checked[mode] += int(where.sum())
        f = s - np.floor(s)
        no_tie = np.all(np.abs(f - 0.5) > 1e-9, axis=0)
        lab = label.double().numpy()
        for mode, where in (("constant", (inside | far) & no_tie), ("grid-constant", no_tie)):
            want = ndimage.affine_transform(lab, m, offset=offset, output_shape=roi, order=0, mode=mode, cval=0.0)
            assert np.array_equal(ids[0][where], want[where].astype(np.int64)), (n, mode)
            checked["labels"] += int(where.sum())
    print(checked)
    assert checked["constant"] > 1000 and checked["labels"] > 1000
    assert int((~(inside | far)).sum()) > 0                           # the band where the two modes differ was met


def test_matrix_is_orthonormal_times_the_inverse_zoom_and_exact_without_an_event():
    rng = np.random.RandomState(0)
    worst = 0.0
    for n in range(400):
        t = [F32(math.tan(math.radians(a) / 2)) for a in rng.uniform(-90, 90, 3)]
        z = F32(rng.uniform(0.4, 2.5))
        m = aref.matrix(t, z).astype(F64).reshape(3, 3) * F64(z)
        worst = max(worst, float(np.abs(m @ m.T - np.eye(3)).max()), abs(float(np.linalg.det(m)) - 1.0))
    print(f"max |z^2 M M^T - I| and |det(z M) - 1| over 400 rows: {worst / aref.U:.2f} u")
    assert worst <= 4 * aref.U
    ident = aref.matrix([F32(0)] * 3, F32(1))
    assert np.array_equal(ident.view(np.int32), np.eye(3, dtype=F32).reshape(9).view(np.int32))       # +0 everywhere: the bits
    # a quarter turn about d: t = 1 exactly, the (h, w) plane turns and d stays
    quarter = aref.matrix([F32(1), F32(0), F32(0)], F32(1)).reshape(3, 3)
    assert np.array_equal(quarter, np.array([[1, 0, 0], [0, 0, -1], [0, 1, 0]], dtype=F32))
    assert np.array_equal(aref.matrix([F32(0)] * 3, F32(2)), (np.eye(3, dtype=F32) / 2).reshape(9))


def test_identity_rows_give_exactly_the_plain_apply(cases):
    for name, (case, vols, _) in cases.items():
        rows = aref.identity_rows(len(case["ints"]), pad_value=-3.5)
        want_images, want_labels = ref.apply(vols, case["ints"], case["floats"], case["roi"], case["class_ids"])
        got_images, got_labels, _, _ = aref.apply(vols, case["ints"], case["floats"], rows, case["roi"], case["class_ids"], emulate=True)
        assert got_images.dtype == F32
        assert np.array_equal(got_images.view(np.int32), want_images.numpy().view(np.int32)), name
        assert np.array_equal(got_labels, want_labels.numpy()), name


def test_fp32_emulation_stays_inside_the_bound_on_every_gpu_case(cases):
    for name, (case, vols, want) in cases.items():
        got = aref.apply(vols, case["ints"], case["floats"], case["rows"], case["roi"], case["class_ids"], emulate=True)
        bound = aref.row_bounds(vols, case["ints"], case["floats"], case["rows"])
        ratio, at = aref.worst_ratio(got[0], want[0], bound)
        padded = float(np.mean(np.any([(want[3][:, a] < 0) | (want[3][:, a] >= np.array([vols[r[0]].shape[a] for r in case["ints"]])
                                                                                  .reshape(-1, 1, 1, 1)) for a in range(3)], axis=0)))
        print(f"{name}: max |fp32 - fp64| / bound = {ratio:.3f} at {at}; bound {bound.min():.3e} .. {bound.max():.3e}; "
              f"{100 * padded:.1f} % of the voxels have their nearest index outside the volume")
        assert ratio <= 1.0, name
        assert np.array_equal(got[1], want[1]), name              # the labels do not depend on the arithmetic of the values
        assert want[1].sum() > 0 and 0 < padded < 0.9, name       # the case meets labels, and the pad without being all pad


@pytest.mark.parametrize("defect", ["lerp_order", "pad_per_voxel", "round", "transpose", "late_flip"])
def test_planted_defects_leave_the_bound_or_change_a_label(cases, defect):
    """Each defect is caught on EVERY case: the GPU test compares images within the bound and labels bit for bit on the same
    rows."""
    for name, (case, vols, want) in cases.items():
        got = aref.apply(vols, case["ints"], case["floats"], case["rows"], case["roi"], case["class_ids"], emulate=True, defect=defect)
        bound = aref.row_bounds(vols, case["ints"], case["floats"], case["rows"])
        ratio, _ = aref.worst_ratio(got[0], want[0], bound)
        labels_differ = int((got[2] != want[2]).sum())
        print(f"{defect} on {name}: max |defect - fp64| / bound = {ratio:.3g}, {labels_differ} labels differ")
        assert ratio > 1.0 or labels_differ > 0, (defect, name)


def test_the_order_of_the_axes_in_the_tree_moves_the_image_only_within_the_bound(cases):
    """Trilinear interpolation is the same polynomial in whichever order the axes are taken: d first and w last changes roundings
    only, so no derived bound can tell it from the contract's order (the planted 'lerp_order' is therefore the order of a
    lerp's two operands).  The header fixes w, h, d all the same, for the bits."""
    for name, (case, vols, want) in cases.items():
        got = aref.apply(vols, case["ints"], case["floats"], case["rows"], case["roi"], case["class_ids"], emulate=True, defect="axis_order")
        ratio, _ = aref.worst_ratio(got[0], want[0], aref.row_bounds(vols, case["ints"], case["floats"], case["rows"]))
        print(f"axis order d, h, w on {name}: max |fp32 - fp64| / bound = {ratio:.3f}")
        assert ratio <= 1.0 and np.array_equal(got[2], want[2])


def test_event_statistics_of_the_restatement_for_the_gpu_tests_seed():
    rows = np.concatenate([aref.affine_rows(aref.STATS_B, call, aref.STATS_SEED, **aref.STATS_AFFINE) for call in range(aref.STATS_CALLS)])
    assert len(rows) == 20000
    counts = aref.check_affine_statistics(rows, aref.STATS_AFFINE)
    both = int(np.sum(rows[:, aref.A_EVENTS].copy().view(np.int32) == 3))
    assert abs(both - 5000) <= 5 * math.sqrt(20000 * 0.25 * 0.75), both       # the two events are independent
    assert counts["rotation"] != counts["zoom"]
    # the matrix of every row is the one its t and z give, and the pad travels in the row
    for r in rows[:50]:
        assert np.array_equal(r[:9], aref.matrix(r[aref.A_T:aref.A_T + 3], r[aref.A_ZOOM]))
        assert r[aref.A_PAD] == F32(-1.25) and r[15] == 0


def test_image_bound_is_the_derived_number():
    u = aref.U
    assert aref.image_bound(1.0, 0.0) == pytest.approx(11 * u, rel=1e-5)      # 9 u from the tree, 2 u from the intensity transform
    assert aref.image_bound(3.5, 0.1, 0.1) > aref.image_bound(3.5, 0.0) > aref.image_bound(1.0, 0.0)
    assert aref.image_bound(3.5, 0.1, 0.1) < 16 * 3.5 * u
