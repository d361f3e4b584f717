"""The label map on the grid of the scan, without a device: the host tables of prepare.linear_restore_tables against the
restatement of the header's text (tests/labelmap_ref.py), the fp32 emulation of the kernel against the fp64 reference under the
acceptance rule, every planted defect of the emulation caught, and the argument errors of the entry point and of
inference.segment_case (the library alone: every error is returned before a launch)."""
import ctypes as C

import numpy as np
import pytest
import torch

import labelmap_ref as R
from diff_unet_amos_amd import inference, prepare

CASES = ("case1", "case2", "case2_x8", "case3")


# ---- tables ----

@pytest.mark.parametrize("name", CASES)
def test_tables_against_the_restatement(name):
    case = R.make_case(name)
    g = case["geometry"]
    want = R.tables_ref(g.source_shape, g.box, g.perm, g.flip, g.n_in, g.s_in, g.pixdim, g.shape)
    stride = (g.shape[1] * g.shape[2], g.shape[2], 1)
    for p in range(3):
        lo, wt, step, axis = want[p]
        assert case["lo"][p].dtype == np.int32 and case["weight"][p].dtype == np.float32
        assert np.array_equal(case["lo"][p], lo) and case["step"][p] == step and case["axis"][p] == axis == g.perm.index(p)
        assert np.array_equal(case["weight"][p], wt.astype(np.float32))
        b0, b1 = g.box[p]
        assert (case["lo"][p][:b0] == -1).all() and (case["lo"][p][b1:] == -1).all() and (case["lo"][p][b0:b1] >= 0).all()
        assert (case["weight"][p][:b0] == 0).all() and (case["weight"][p][b1:] == 0).all()
        # lo + weight is the coordinate k s_in / s_out (clamped to the extent) within one fp32 rounding of the weight
        j = axis
        k = np.arange(b1 - b0, dtype=np.float64)
        if g.flip[j]:
            k = k[::-1]
        y = np.minimum(k * g.s_in[j] / g.pixdim[j], g.shape[j] - 1)
        got = case["lo"][p][b0:b1].astype(np.float64) / stride[j] + case["weight"][p][b0:b1].astype(np.float64)
        assert np.abs(got - y).max() <= R.U32
        assert (case["weight"][p] >= 0).all() and (case["weight"][p] <= 1).all()
        last = case["lo"][p][b0:b1] // stride[j] == g.shape[j] - 1                  # no upper neighbour there: weight 0
        assert (case["weight"][p][b0:b1][last] == 0).all() and (case["lo"][p][b0:b1] // stride[j] <= g.shape[j] - 1).all()


def test_flips_reverse_the_tables():
    X, box, world, signs, spacing = R.GEOMETRIES["case1"][:5]
    flipped = prepare.linear_restore_tables(prepare.prepared_geometry(X, box, R.signed_permutation_affine(world, signs, spacing)))
    plain = prepare.linear_restore_tables(prepare.prepared_geometry(X, box, R.signed_permutation_affine(world, (1, 1, 1), spacing)))
    assert flipped["axis"] == plain["axis"] == (1, 2, 0) and flipped["step"] == plain["step"]
    for p, sign in enumerate(signs):
        b0, b1 = box[p]
        for key in ("lo", "weight"):
            a, b = flipped[key][p][b0:b1], plain[key][p][b0:b1]
            assert np.array_equal(a, b[::-1] if sign < 0 else b)
            assert sign > 0 or not np.array_equal(a, b)


def test_extent_one_axis_and_equal_spacing():
    case = R.make_case("case3")
    assert case["spatial"][0] == 1 and case["step"][0] == 0
    assert case["lo"][0].tolist() == [0] and case["weight"][0].tolist() == [0.0]
    # s_in == s_out on every axis: the prepared grid is the cropped scan, every weight is 0 and lo walks the strides
    X, box = (6, 7, 5), ((1, 5), (0, 7), (2, 5))
    g = prepare.prepared_geometry(X, box, np.diag([1.5, 1.5, 2.0, 1.0]))
    t = prepare.linear_restore_tables(g)
    assert g.shape == (4, 7, 3) and t["axis"] == (0, 1, 2) and t["step"] == (21, 3, 1)
    for p in range(3):
        b0, b1 = box[p]
        assert (t["weight"][p] == 0).all()
        assert t["lo"][p][b0:b1].tolist() == [k * t["step"][p] for k in range(b1 - b0)]


def test_the_case_caches_its_device_tables_next_to_the_restore_tables():
    fields = [f.name for f in prepare.dataclasses.fields(prepare.PreparedCase)]
    assert fields[:8] == ["image", "label", "affine", "source_shape", "box", "orientation", "geometry", "_restore_tables"]
    assert fields[8:] == ["_linear_tables"]


# ---- the emulation against the fp64 reference; every defect caught ----

@pytest.fixture(scope="module")
def refs():
    out = {}
    for name in CASES:
        case = R.make_case(name)
        out[name] = (case, R.reference(case))
    weighted = R.make_case("case1", weighted=True)
    out["case1_weighted"] = (weighted, R.reference(weighted))
    return out


@pytest.mark.parametrize("name", CASES + ("case1_weighted",))
def test_emulation_agrees_with_the_reference(refs, name):
    case, ref = refs[name]
    label, _ = R.emulate(case)
    ex, _ = R.check(label, ref, what=name)
    assert ex == 0                                               # the seeds are fixed: no voxel of these cases needs the exemption
    assert (label[~ref["inside"]] == 0).all() and len(np.unique(label)) > 2
    for min_prob in (0.5, 0.9):
        R.check(R.emulate(case, min_prob)[0], R.reference(case, min_prob), min_prob, what=f"{name} min_prob {min_prob}")


def _caught(case, ref, defect, min_prob=0.0):
    label, _ = R.emulate(case, min_prob, defect)
    return int(((label != ref["label"]) & ~R.exempt(ref, min_prob)).sum())


@pytest.mark.parametrize("defect", ["lerp_axes_swapped", "wrong_neighbour", "flip_ignored", "crop_offset_dropped"])
def test_geometry_defects_are_caught_by_the_acceptance_rule(refs, defect):
    case, ref = refs["case1"]
    wrong = _caught(case, ref, defect)
    print(f"{defect}: {wrong} labels outside the exemption differ from the reference")
    assert wrong > 0
    with pytest.raises(AssertionError):
        R.check(R.emulate(case, defect=defect)[0], ref, what=defect)


def test_tie_defect_is_caught_on_a_planted_tie():
    """An exact tie is inside the exemption of the rule by construction, so it has its own check: the copy never wins."""
    case = R.plant_tie(R.make_case("case2"), 3, 9)
    ref = R.reference(case)
    clean, _ = R.emulate(case)
    assert (clean != 9).all() and (clean == 3).any() and np.array_equal(clean == 3, ref["label"] == 3)
    broken, _ = R.emulate(case, defect="tie_to_highest")
    assert (broken == 9).any() and (broken != 3).all()


def test_min_prob_defect_is_caught_on_a_planted_half():
    """A probability of exactly 0.5 equals min_prob = 0.5: kept by <, dropped by <=."""
    case = R.plant_half(R.make_case("case1"), 2)
    inside = R.reference(case)["inside"]
    clean, best = R.emulate(case, 0.5)
    assert (best[inside] == np.float32(0.5)).all() and (clean[inside] == 2).all() and (clean[~inside] == 0).all()
    broken, _ = R.emulate(case, 0.5, defect="min_prob_le")
    assert (broken == 0).all()
    above, _ = R.emulate(case, float(np.nextafter(np.float32(0.5), np.float32(1))))
    assert (above == 0).all()


def test_a_nan_never_wins():
    case = R.identity_case((3, 4, 5), 4, seed=3)
    case["sum"][0] = np.nan
    case["sum"][2, 1, 2, 3] = np.nan
    label, _ = R.emulate(case)
    assert (label != 0).all() and label[1, 2, 3] != 2
    case["sum"][:, 0, 0, 0] = np.nan
    assert R.emulate(case)[0][0, 0, 0] == 0 and R.reference(case)["label"][0, 0, 0] == 0


# ---- argument errors: the library alone ----

def _call(**kw):
    from diff_unet_amos_amd import _native as nv
    one = C.c_void_p(64)
    a = dict(sum=one, C=5, P=(16, 12, 8), nd=one, nh=one, nw=one, wsum=None, o=(2, 1, 1), n=(11, 9, 7), X=(17, 14, 12), lo=(one,) * 3,
             w=(one,) * 3, axis=(1, 2, 0), min_prob=0.0, out=one, ref=None, tallies=None)
    a.update(kw)
    return nv.lib().dua_blend_finish_labelmap(a["sum"], a["C"], *a["P"], a["nd"], a["nh"], a["nw"], a["wsum"], *a["o"], *a["n"],
                                              *a["X"], *a["lo"], *a["w"], *a["axis"], a["min_prob"], a["out"], a["ref"],
                                              a["tallies"], None)


def test_entry_point_argument_errors_before_any_launch():
    """Pointers that would fault if anything were launched or written: every call returns DUA_ERR_ARG."""
    from diff_unet_amos_amd import _native as nv
    one, odd, four = C.c_void_p(64), C.c_void_p(66), C.c_void_p(68)
    for name in ("sum", "out"):                                                    # a null pointer
        assert _call(**{name: None}) == nv.ERR_ARG, name
    for k in range(3):
        assert _call(lo=tuple(None if i == k else one for i in range(3))) == nv.ERR_ARG
        assert _call(w=tuple(None if i == k else one for i in range(3))) == nv.ERR_ARG
    assert _call(nd=None) == nv.ERR_ARG and _call(nh=None) == nv.ERR_ARG and _call(nw=None) == nv.ERR_ARG
    assert _call(wsum=one) == nv.ERR_ARG                                           # both divisor forms
    assert _call(nd=None, nh=None, nw=None) == nv.ERR_ARG                          # neither
    assert _call(ref=one) == nv.ERR_ARG and _call(tallies=one) == nv.ERR_ARG      # a reference without tallies, and the reverse
    for bad in (0, -1, nv.BLEND_MAX_CLASSES + 1, 256, 1 << 20):                    # C = 0, C > 255
        assert _call(C=bad) == nv.ERR_ARG, bad
    assert _call(X=(1 << 11, 1 << 10, 1 << 10)) == nv.ERR_ARG                      # 2^31 source voxels
    assert _call(P=(1 << 11, 1 << 10, 1 << 10), n=(1, 1, 1)) == nv.ERR_ARG         # 2^31 voxels in a plane of the sum volume
    assert _call(X=(0, 14, 12)) == nv.ERR_ARG and _call(n=(11, 0, 7)) == nv.ERR_ARG and _call(X=(17, 14, -3)) == nv.ERR_ARG
    assert _call(o=(6, 1, 1)) == nv.ERR_ARG and _call(o=(2, -1, 1)) == nv.ERR_ARG  # the crop leaves the volume
    for axis in ((0, 0, 1), (0, 1, 3), (-1, 1, 2), (2, 2, 2)):
        assert _call(axis=axis) == nv.ERR_ARG, axis
    for bad in (float("nan"), -0.25, 1.5, float("inf")):                           # min_prob NaN or outside [0, 1]
        assert _call(min_prob=bad) == nv.ERR_ARG, bad
    for name in ("sum", "nd", "nh", "nw"):                                         # a pointer off its natural alignment
        assert _call(**{name: odd}) == nv.ERR_ARG, name
    assert _call(nd=None, nh=None, nw=None, wsum=odd) == nv.ERR_ARG
    for k in range(3):
        assert _call(lo=tuple(odd if i == k else one for i in range(3))) == nv.ERR_ARG
        assert _call(w=tuple(odd if i == k else one for i in range(3))) == nv.ERR_ARG
    assert _call(ref=one, tallies=four) == nv.ERR_ARG                              # 64-bit counters on a 4-byte boundary


def test_segment_case_refuses_bad_arguments_before_any_predictor_call():
    calls = []

    def pred(x, **kw):
        calls.append(x.shape)
        raise AssertionError("the predictor must not run")

    vol = torch.zeros(1, 1, 8, 8, 8)
    for bad in (float("nan"), -0.1, 1.01):
        with pytest.raises(ValueError, match="min_prob"):
            inference.segment_case(pred, vol, min_prob=bad)
    for bad in (torch.zeros(2, 1, 8, 8, 8), torch.zeros(1, 2, 8, 8, 8), torch.zeros(8, 8, 8)):   # B != 1, two channels, no batch
        with pytest.raises(ValueError, match=r"\[1, 1, D, H, W\]"):
            inference.segment_case(pred, bad)
    with pytest.raises(ValueError, match="float32"):
        inference.segment_case(pred, vol.half())
    with pytest.raises(ValueError, match="PreparedCase or"):
        inference.segment_case(pred, np.zeros((1, 1, 8, 8, 8), dtype=np.float32))
    with pytest.raises(ValueError, match="mirror_axes"):
        inference.segment_case(pred, vol, mirror_axes=(3,))
    with pytest.raises(RuntimeError, match="runs on an MI355X"):                    # a host tensor: there is no CPU path
        inference.segment_case(pred, vol)
    g = prepare.prepared_geometry((6, 7, 5), ((1, 5), (0, 7), (2, 5)), np.diag([1.5, 1.5, 2.0, 1.0]))
    meta = torch.zeros(g.shape, device="meta")                   # no storage: nothing can be read, written or launched
    case = prepare.PreparedCase(meta, None, g.affine, g.source_shape, g.box, (g.perm, g.flip), g)
    with pytest.raises(ValueError, match="uint8"):
        inference.segment_case(pred, case, label=torch.zeros(6, 7, 5))
    with pytest.raises(ValueError, match="shape of the scan"):
        inference.segment_case(pred, case, label=torch.zeros(4, 7, 3, dtype=torch.uint8))
    assert calls == []
