"""The label-map evaluation contract without a GPU: the numpy restatement (labelmap_eval_ref) against the scipy golden file and
against planted defects, the host-side box and workspace arithmetic of the surface report against the library's own, the scan
spacing of a prepared case, and the argument errors of ``segment_case``."""
import os

import numpy as np
import pytest
import torch

import labelmap_eval_ref as LR
from labelmap_ref import signed_permutation_affine

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "labelmap_eval_golden.npz")
VALUES = LR.C + 2


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def unpack(bits, shape):
    onehot = np.unpackbits(bits)[:VALUES * int(np.prod(shape))].reshape(VALUES, *shape)
    return onehot.argmax(axis=0).astype(np.uint8)


# ---- the restatement against scipy ----

@pytest.mark.parametrize("name", sorted(LR.MAPS))
def test_the_maps_are_those_of_the_golden_file(golden, name):
    maps = LR.MAPS[name]()
    assert maps.dtype == np.uint8 and maps.shape[0] == 2 and tuple(golden[f"{name}_shape"]) == maps.shape
    assert np.array_equal(unpack(golden[f"{name}_map"], maps.shape), maps)


@pytest.mark.parametrize("conn", LR.CONNECTIVITIES)
@pytest.mark.parametrize("name", sorted(LR.MAPS))
def test_labels_per_class_are_scipys(golden, name, conn):
    """The joint labelling restricted to a class, renumbered in increasing order, is scipy.ndimage.label(map == c): the same
    components in the same order; the joint count is the sum of the classes' counts."""
    maps = LR.MAPS[name]()
    for n, m in enumerate(maps):
        lab, count, cls = LR.label_map(m, LR.C, conn)
        assert count == int(golden[f"{name}_c{conn}_counts"][n].sum()) == int(lab.max()) and len(cls) == count
        assert not lab[(m == 0) | (m >= LR.C)].any() and (lab[(m >= 1) & (m < LR.C)] > 0).all()
        first = [int(np.flatnonzero(lab.ravel() == l)[0]) for l in range(1, count + 1)]
        assert first == sorted(first)                                                 # numbered by first voxel
        assert all(m.ravel()[p] == c for p, c in zip(first, cls))                     # the class of a label: the value at its root
        for c in range(1, LR.C):
            mine, k = LR.restrict(lab, m, c)
            assert k == int(golden[f"{name}_c{conn}_counts"][n, c])
            assert np.array_equal(mine, golden[f"{name}_c{conn}_labels"][n, c].astype(np.int32))


def test_the_checkerboard_and_the_serpentine_do_what_they_are_there_for(golden):
    m = LR.checkerboard_maps()[0]
    assert LR.label_map(m, LR.C, 1)[1] == m.size                                       # every voxel its own component
    assert LR.label_map(m, LR.C, 2)[1] == 2 and LR.label_map(m, LR.C, 3)[1] == 2        # one per class, never merged
    s = LR.serpentine_maps()[0]
    lab, count, cls = LR.label_map(s, LR.C, 1)
    assert sorted(cls.tolist()).count(2) == 1 and count == 1 + int(golden["serpentine_c1_counts"][0, 1])


@pytest.mark.parametrize("case", sorted(LR.FILTER_CASES))
def test_filter_cases_are_scipys(golden, case):
    maker, conn, k, min_size, classes = LR.FILTER_CASES[case]
    maps = LR.MAPS[maker]()
    want = unpack(golden[f"filter_{case}"], maps.shape)
    got = np.stack([LR.filter_map(m, LR.C, conn, k, min_size, classes) for m in maps])
    assert np.array_equal(got, want)
    assert np.array_equal(got[maps >= LR.C], maps[maps >= LR.C])                      # values >= C pass through


def test_cap_drops_the_labels_above_it():
    m = LR.touching_maps()[0]
    lab, count, cls = LR.label_map(m, LR.C, 1)
    assert count == 6
    out = LR.filter_map(m, LR.C, 1, 0, 0, None, cap=3)
    assert np.array_equal(out[lab > 3], np.zeros(int((lab > 3).sum()), np.uint8)) and np.array_equal(out[lab <= 3], m[lab <= 3])


def test_tallies_count_a_value_above_the_classes_nowhere():
    a, b = LR.touching_maps()
    t = LR.tallies(a, b, LR.C)
    assert int(t[:, 1].sum()) == int((a < LR.C).sum()) and int(t[:, 2].sum()) == int((b < LR.C).sum())
    assert t[4].tolist() == [0, 0, 16]


# ---- planted defects: every one is caught by a case above ----

def _caught_by_labels(golden, defect):
    for name in sorted(LR.MAPS):
        for n, m in enumerate(LR.MAPS[name]()):
            lab = LR.label_map(m, LR.C, 1, defect)[0]
            for c in range(1, LR.C):
                if not np.array_equal(LR.restrict(lab, m, c)[0], golden[f"{name}_c1_labels"][n, c].astype(np.int32)):
                    return True
    return False


def _caught_by_filter(golden, defect):
    for case, (maker, conn, k, min_size, classes) in LR.FILTER_CASES.items():
        maps = LR.MAPS[maker]()
        got = np.stack([LR.filter_map(m, LR.C, conn, k, min_size, classes, defect=defect) for m in maps])
        if not np.array_equal(got, unpack(golden[f"filter_{case}"], maps.shape)):
            return True
    return False


def _surface_pairs():
    return [LR.surface_maps(s) for s in LR.SURFACE_SHAPES] + [LR.full_class_maps(LR.SURFACE_SHAPES[0])]


def _caught_by_box_counts(defect):
    for t, r in _surface_pairs():
        for c in LR.SURFACE_CLASSES:
            got, want = LR.box_counts(t, r, c, 1, defect), LR.full_counts(t, r, c, 1)
            if any(not np.array_equal(got[k], want[k]) for k in want):
                return True
    return False


def _caught_by_workspace(defect):
    from diff_unet_amos_amd import metrics
    for t, r in _surface_pairs():
        boxes = [[LR.box_of(t, r, c) for c in LR.SURFACE_CLASSES]]
        have = metrics.label_map_workspace_bytes(t.shape, boxes)
        if have != [LR.workspace_bytes(t.shape, [b], defect) for b in boxes[0]]:
            return True
    return False


def test_the_contract_passes_every_check(golden):
    assert not _caught_by_labels(golden, None) and not _caught_by_filter(golden, None)
    assert not _caught_by_box_counts(None) and not _caught_by_workspace(None)


@pytest.mark.parametrize("defect", LR.DEFECTS)
def test_planted_defects_are_caught(golden, defect):
    caught = {"labels": _caught_by_labels(golden, defect), "filter": _caught_by_filter(golden, defect),
              "box counts": _caught_by_box_counts(defect), "workspace": _caught_by_workspace(defect)}
    expected = {"fused_classes": ("labels", "filter"), "topk_over_all_classes": ("filter",), "large_value_zeroed": ("filter",),
                "box_without_margin": ("workspace",), "tn_from_box": ("box counts",)}[defect]
    assert all(caught[k] for k in expected), caught


# ---- the box rule and the workspace arithmetic ----

def test_box_and_margin_by_hand():
    shape = (7, 9, 70)
    t, r = np.zeros(shape, np.uint8), np.zeros(shape, np.uint8)
    t[2:5, 4:8, 30:44] = 2
    r[3:6, 3:7, 32:47] = 2
    r[0:2, 0:9, 60:70] = 3
    assert LR.box_of(t, r, 2) == [2, 3, 30, 6, 8, 47] and LR.grown(LR.box_of(t, r, 2), shape) == ([1, 2, 29], [6, 7, 19])
    assert LR.box_of(t, r, 3) == [0, 0, 60, 2, 9, 70] and LR.grown(LR.box_of(t, r, 3), shape) == ([0, 0, 59], [3, 9, 11])  # clamped
    assert LR.box_of(t, r, 1)[3:] == [0, 0, 0] and LR.grown(LR.box_of(t, r, 1), shape) is None
    # inside the grown box the borders and every count are those of the full volume; tn counts the full volume
    for c in (1, 2, 3):
        got, want = LR.box_counts(t, r, c), LR.full_counts(t, r, c)
        assert all(np.array_equal(got[k], want[k]) for k in want), c
    assert LR.box_counts(t, r, 1)["tn"] == 7 * 9 * 70


def test_workspace_of_a_class_comes_from_its_box():
    """The library's host function agrees with the restated arithmetic, the box form needs a fraction of the expansion's bytes,
    a call needs the largest class only, and a class above the limit is refused."""
    from diff_unet_amos_amd import metrics, ops
    shape = (160, 512, 512)
    boxes = [[[40, 100, 100, 90, 200, 180], [2 ** 31 - 1] * 3 + [0] * 3, [0, 0, 0, 160, 512, 512], [159, 511, 500, 160, 512, 512]]]
    needs = metrics.label_map_workspace_bytes(shape, boxes)
    assert needs == [LR.workspace_bytes(shape, [b]) for b in boxes[0]] and needs[1] == 0
    assert needs[0] == LR.table_workspace_bytes(52, 102, 82) and needs[3] == LR.table_workspace_bytes(2, 2, 13)
    one_volume = ops.surface_map_workspace_bytes(shape, [boxes[0][2]])
    assert one_volume == needs[2] == LR.expansion_workspace_bytes(shape, 1)
    assert needs[0] * 50 < one_volume
    # two pairs: a class needs its larger box; a call needs the largest class, not the sum
    two = [boxes[0], [boxes[0][3], boxes[0][0], boxes[0][1], boxes[0][1]]]
    assert metrics.label_map_workspace_bytes(shape, two) == [needs[0], needs[0], needs[2], needs[3]]
    assert ops.surface_map_workspace_bytes(shape, boxes[0]) == max(needs) == needs[2]
    assert metrics.class_groups(needs) == metrics.class_groups(needs, needs[2]) == [[0, 1, 2, 3]]     # one region: one group
    with pytest.raises(ValueError, match="alone needs"):
        metrics.class_groups(needs, needs[2] - 1)
    with pytest.raises(ValueError, match="max_workspace_bytes"):
        metrics.class_groups(needs, 0)
    with pytest.raises(ValueError, match="box outside"):
        ops.surface_map_workspace_bytes(shape, [[0, 0, 0, 161, 512, 512]])
    with pytest.raises(ValueError, match="box outside"):
        ops.surface_map_workspace_bytes(shape, [[5, 0, 0, 5, 512, 512]])


def test_entry_points_refuse_bad_arguments_without_a_device():
    import ctypes as C
    from diff_unet_amos_amd import _native as nv
    L, one = nv.lib(), C.c_void_p(256)
    assert L.dua_cc_map_scratch_bytes(2, 6, 8, 130, 16) == L.dua_cc_scratch_bytes(2, 6, 8, 130, 16) + 256
    assert L.dua_cc_map_scratch_bytes(2, 6, 8, 130, 0) == nv.ERR_ARG
    assert L.dua_cc_label_map(2, 6, 8, 130, one, 6 * 8 * 130, 65, 1, one, one, one, 1 << 20, None) == nv.ERR_ARG       # C > 64
    assert L.dua_cc_label_map(2, 6, 8, 130, one, 6 * 8 * 130, 5, 4, one, one, one, 1 << 20, None) == nv.ERR_ARG        # connectivity
    assert L.dua_cc_label_map(2, 6, 8, 130, one, 6 * 8 * 130, 5, 1, one, one, one, 16, None) == nv.ERR_ARG             # workspace
    assert L.dua_cc_filter_map(2, 6, 8, 130, one, 6 * 8 * 130, 5, one, one, one, 16, 1, 0, None, one, one, None, one, 1 << 20,
                               None) == nv.ERR_ARG                                                                     # reference without tallies
    assert L.dua_surface_map_boxes(1, 6, 8, 130, one, 6 * 8 * 130, one, 6 * 8 * 130, 65, one, None) == nv.ERR_ARG
    box = (C.c_int * 6)(0, 0, 0, 7, 8, 130)                                                                            # d1 > D
    ids, tol = (C.c_int * 1)(1), (C.c_double * 1)(1.0)
    assert L.dua_surface_map_report(1, 6, 8, 130, one, 6 * 8 * 130, one, 6 * 8 * 130, 1, ids, box, 1, 1.0, 1.0, 1.0, 1, tol, 1,
                                    one, one, one, one, one, 1 << 30, None) == nv.ERR_ARG


# ---- the spacing of the scan ----

def test_source_spacing_of_a_permuted_flipped_anisotropic_scan():
    from diff_unet_amos_amd import prepare
    spacing = (0.8, 0.9, 3.1)
    affine = signed_permutation_affine((1, 2, 0), (1, -1, -1), spacing)
    shape = (24, 22, 18)
    geom = prepare.prepared_geometry(shape, ((2, 22), (1, 20), (1, 17)), affine)
    assert geom.perm == (2, 0, 1) and geom.flip == (True, False, True)
    case = prepare.PreparedCase(None, None, geom.affine, geom.source_shape, geom.box, (geom.perm, geom.flip), geom)
    assert case.source_spacing == pytest.approx(spacing, rel=1e-15) and isinstance(case.source_spacing, tuple)
    assert tuple(geom.s_in) == pytest.approx((3.1, 0.8, 0.9), rel=1e-15)               # per prepared axis: another order
    identity = prepare.prepared_geometry(shape, ((0, 24), (0, 22), (0, 18)), np.diag([2.0, 0.5, 0.7, 1.0]))
    case = prepare.PreparedCase(None, None, identity.affine, shape, identity.box, (identity.perm, identity.flip), identity)
    assert case.source_spacing == (2.0, 0.5, 0.7)


# ---- segment_case refuses malformed arguments before any predictor call ----

def _never(*a, **k):
    raise AssertionError("the predictor was called")


@pytest.mark.parametrize("kw,match", [
    (dict(postprocess=[1]), "postprocess"),
    (dict(postprocess={"channels": (1,)}), "postprocess"),
    (dict(postprocess={"connectivity": 4}), "connectivity"),
    (dict(postprocess={"num_components": -1}), "num_components"),
    (dict(postprocess={"min_size": 1.5}), "min_size"),
    (dict(postprocess={"cap": 0}), "cap"),
    (dict(postprocess={"classes": (0,)}), "classes"),
    (dict(surface={"tolerance": 1.0}), "label is None"),
    (dict(surface={}, label="given"), "tolerance"),
    (dict(surface={"tolerance": 1.0, "distances": True}, label="given"), "surface"),
    (dict(surface={"tolerance": 1.0, "connectivity": 0}, label="given"), "connectivity"),
    (dict(surface={"tolerance": 1.0, "classes": ()}, label="given"), "classes"),
    (dict(surface=3.0, label="given"), "surface"),
    (dict(surface={"tolerance": 1.0, "classes": (64,)}, label="given"), "classes"),
    (dict(surface={"tolerance": -1.0}, label="given"), "tolerance"),
    (dict(surface={"tolerance": float("nan")}, label="given"), "tolerance"),
    (dict(surface={"tolerance": [1.0, 2.0], "classes": (1, 2, 3)}, label="given"), "tolerance"),
    (dict(surface={"tolerance": [[1.0] * 9]}, label="given"), "tolerance"),
    (dict(surface={"tolerance": "wide"}, label="given"), "tolerance|surface"),
    (dict(surface={"tolerance": 1.0, "voxel_spacing": (1.0, 2.0)}, label="given"), "voxel_spacing"),
    (dict(surface={"tolerance": 1.0, "voxel_spacing": (1.0, 0.0, 1.0)}, label="given"), "voxel_spacing"),
])
def test_segment_case_argument_errors(kw, match):
    from diff_unet_amos_amd import inference
    volume = torch.zeros(1, 1, 8, 8, 8)
    kw = dict(kw)
    if kw.get("label") == "given":
        kw["label"] = torch.zeros(8, 8, 8, dtype=torch.uint8)
    with pytest.raises(ValueError, match=match):
        inference.segment_case(_never, volume, roi_size=(8, 8, 8), **kw)
