"""Centroid-distance label smoothing without a GPU: the fp64 restatement (tests/label_smoothing_ref.py) against the reference's
own outputs (tests/golden/label_smoothing_golden.npz, tools/make_label_smoothing_golden.py) within the derived bound on every
element, and the argument checks of the Python layer and of the new C entry points."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import augment_ref as ref  # noqa: E402
import label_smoothing_ref as lsr  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "label_smoothing_golden.npz")


def _cases():
    gold = np.load(GOLDEN)
    return gold, gold["cases"].tolist()


def test_golden_holds_the_cases_the_feature_is_judged_on():
    gold, names = _cases()
    shapes = {n: gold[f"{n}_labels"].shape for n in names}
    assert all(len(set(s)) == 3 for s in shapes.values())                    # non-cubic: a swapped axis shows
    assert {int(gold[f"{n}_K"]) for n in names} == {3, 14}
    assert any(float(gold[f"{n}_order"]) != 1.0 for n in names)
    counts = {n: np.bincount(gold[f"{n}_labels"].reshape(-1), minlength=int(gold[f"{n}_K"])) for n in names}
    assert any((c == 0).any() for c in counts.values()) and any((c == 1).any() for c in counts.values())
    one = next(n for n in names if (counts[n] == 1).any())
    k = int(np.flatnonzero(counts[one] == 1)[0])
    at = tuple(int(i[0]) for i in np.nonzero(gold[f"{one}_labels"] == k))
    assert abs(float(gold[f"{one}_out"][(k,) + at]) - (0.3 / 1e-6 - 1.0)) < 0.5      # |1 - alpha / epsilon| at the class's voxel
    for n in names:
        out = gold[f"{n}_out"]
        assert out.dtype == np.float32 and out.shape == (int(gold[f"{n}_K"]),) + shapes[n] and gold[f"{n}_labels"].dtype == np.uint8
        assert 0.0 <= float(gold[f"{n}_centroid_gap"]) < 1e-5


def test_restatement_equals_the_reference_golden_within_the_derived_bound():
    gold, names = _cases()
    for name in names:
        labels, K = gold[f"{name}_labels"], int(gold[f"{name}_K"])
        kw = dict(alpha=float(gold[f"{name}_alpha"]), order=float(gold[f"{name}_order"]), epsilon=float(gold[f"{name}_epsilon"]))
        want, dist = lsr.field(labels, K, **kw)
        tol = lsr.tolerance(dist, want, kw["alpha"], kw["order"], kw["epsilon"],
                            float(gold[f"{name}_centroid_gap"]) + lsr.delta_c_device(labels.shape))
        assert np.isfinite(tol).all()                                        # no element is left out by an infinite bound
        ratio, at = lsr.worst_ratio(gold[f"{name}_out"], want, tol)
        print(f"{name}: extents {labels.shape}, K = {K}, {want.size} elements, max {want.max():.6g}: worst |reference - "
              f"restatement| / tol = {ratio:.3g} at {at}")
        assert ratio <= 1.0, (name, at, gold[f"{name}_out"][at], want[at], tol[at])


def test_absent_class_keeps_the_origin_and_a_patch_is_the_field_at_its_source_indices():
    """The two properties the device form rests on, with the restatement alone: an absent class has its centroid at (0, 0, 0);
    the smoothed patch of a params row equals the whole smoothed field cropped, flipped and rotated like any other key."""
    K = 5
    image, label = ref.synthetic_volume((24, 20, 28), 3, classes=K)
    label[label == 2] = 0
    assert not lsr.centroids(label.numpy(), K)[2].any()
    whole, _ = lsr.field(label.numpy(), K)
    vol = ref.RefVolume(image, label)
    ints = np.array([[0, 3, 1, 5, 5, 3], [0, 8, 4, 12, 2, 0], [0, 0, 0, 0, 0, 2]], dtype=np.int32)
    _, got, _ = lsr.apply([vol], ints, np.zeros((3, 2), dtype=np.float32), (16, 16, 16), range(1, K), K)
    for b, (_, sd, sh, sw, flip, k) in enumerate(ints.tolist()):
        p = torch.from_numpy(whole[1:, sd:sd + 16, sh:sh + 16, sw:sw + 16])
        for ax in (0, 1, 2):
            if flip >> ax & 1:
                p = p.flip(ax + 1)
        assert np.array_equal(torch.rot90(p, k, (1, 2)).numpy(), got[b]), b


def test_label_smoothing_arguments():
    from diff_unet_amos_amd import augment
    s = augment.LabelSmoothing()
    assert (s.alpha, s.order, s.epsilon, s.max_value) == (0.3, 1.0, 1e-6, None) and math.isinf(s.native().max_value)
    assert augment.LabelSmoothing(max_value=6.0).native().max_value == 6.0
    for bad in (dict(alpha=-0.1), dict(alpha=float("nan")), dict(alpha=float("inf")), dict(epsilon=0.0), dict(epsilon=-1e-6),
                dict(epsilon=1e-45), dict(order=0.0), dict(order=-1.0), dict(max_value=0.0), dict(max_value=float("nan"))):
        with pytest.raises(ValueError):
            augment.LabelSmoothing(**bad)
    image, label = ref.synthetic_volume((8, 8, 8), 1)
    for bad in (0, 257, -3):                                                 # refused before anything touches a device
        with pytest.raises(ValueError, match="num_classes"):
            augment.DeviceVolume(image, label, num_classes=bad)


def test_new_entry_points_refuse_bad_arguments_without_a_device():
    from diff_unet_amos_amd import _native as nv
    lib = nv.lib()
    one, odd = C.c_void_p(16), C.c_void_p(24)
    cen = lib.dua_aug_class_centroids
    assert cen(None, 8, 8, 8, 3, one, one, None) == nv.ERR_ARG
    assert cen(odd, 8, 8, 8, 3, one, one, None) == nv.ERR_ARG               # the label map is read 16 bytes at a time
    assert cen(one, 8, 8, 8, 0, one, one, None) == nv.ERR_ARG
    assert cen(one, 8, 8, 8, 257, one, one, None) == nv.ERR_ARG
    assert cen(one, 0, 8, 8, 3, one, one, None) == nv.ERR_ARG
    assert cen(one, 2048, 1024, 1024, 3, one, one, None) == nv.ERR_ARG      # 2^31 voxels
    assert cen(one, 8, 8, 8, 3, None, one, None) == nv.ERR_ARG
    assert cen(one, 8, 8, 8, 3, one, None, None) == nv.ERR_ARG
    app = lib.dua_aug_apply_smoothed
    ok = nv.AugSmoothing(0.3, 1.0, 1e-6, math.inf)

    def call(sm=ok, centroids=one, K=3, Cn=2, B=1, roi=(8, 8, 8), labels=one):
        return app(one, 1, centroids, K, C.byref(sm) if sm is not None else None, one, B, *roi, one, Cn, one, labels, None, None)

    for bad in (nv.AugSmoothing(-0.1, 1.0, 1e-6, math.inf), nv.AugSmoothing(math.nan, 1.0, 1e-6, math.inf),
                nv.AugSmoothing(0.3, 0.0, 1e-6, math.inf), nv.AugSmoothing(0.3, math.inf, 1e-6, math.inf),
                nv.AugSmoothing(0.3, 1.0, 0.0, math.inf), nv.AugSmoothing(0.3, 1.0, -1e-6, math.inf),
                nv.AugSmoothing(0.3, 1.0, 1e-45, math.inf), nv.AugSmoothing(0.3, 1.0, 1e-6, 0.0),
                nv.AugSmoothing(0.3, 1.0, 1e-6, math.nan)):
        assert call(sm=bad) == nv.ERR_ARG, (bad.alpha, bad.order, bad.epsilon, bad.max_value)
    assert call(sm=None) == nv.ERR_ARG
    assert call(centroids=None) == nv.ERR_ARG
    assert call(K=0) == nv.ERR_ARG and call(K=257) == nv.ERR_ARG
    assert call(Cn=0) == nv.ERR_ARG and call(Cn=nv.AUG_MAX_CLASSES + 1) == nv.ERR_ARG
    assert call(B=0) == nv.ERR_ARG and call(B=65536) == nv.ERR_ARG
    assert call(roi=(8, 0, 8)) == nv.ERR_ARG and call(roi=(2048, 1024, 1024)) == nv.ERR_ARG
    assert call(labels=None) == nv.ERR_ARG
