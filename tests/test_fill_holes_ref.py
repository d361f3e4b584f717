"""tests/fill_holes_ref.py on the CPU: the numpy restatement of the fill-holes contract and the step-by-step emulation of
csrc/fill_holes.hip equal the scipy fixture on every case, exactly; every planted defect is caught by at least one case; the three
C entries check their arguments before touching a device; and ``fill_holes=`` is refused before any device work."""
import numpy as np
import pytest
import torch

import fill_holes_ref as FR


@pytest.fixture(scope="module")
def golden():
    return FR.Golden()


def test_the_fixture_holds_the_cases_of_the_contract(golden):
    names = [c["name"] for c in golden.maps]
    for prefix in ("general 9x10x11", "degenerate 1x7x8", "rows 3x5x300", "tile plus one 17x16x16", "diagonal pockets",
                   "two classes", "nested shells", "island in pocket", "value 200", "classes=[2]", "class 63", "single class 3"):
        assert any(n.startswith(prefix) for n in names), prefix
    assert len(golden.named("open on face")) == 6
    assert {c["k"] for c in golden.named("diagonal pockets")} == {1, 2, 3}
    assert tuple(golden.mask.shape) == (2, 3, 9, 10, 11) and not golden.mask[0, 2].any() and golden.mask[1, 0].all()
    # what the named cases are there to show
    assert all(int(c["filled"].sum()) == 0 and (c["map"] == 0).any() for c in golden.named("degenerate"))
    for c in golden.named("open on face"):
        assert int(c["filled"].sum()) == 1 and c["out"][5, 5, 7] == 1          # the closed pocket beside the open one
    assert [int(c["filled"].sum()) for c in golden.named("diagonal pockets")] == [4, 2, 0]
    assert all(int(c["filled"].sum()) == 0 for c in golden.named("two classes") + golden.named("island in pocket"))
    assert all(c["out"][3, 3, 3] == 2 for c in golden.named("nested shells"))
    assert [int(c["filled"].sum()) for c in golden.named("value 200 k")] == [1]
    assert [int(c["filled"].sum()) for c in golden.named("value 200 diagonal")] == [1, 0]
    assert golden.named("classes=[2]")[0]["filled"].tolist() == [0, 0, 1] and golden.named("classes=all")[0]["filled"].tolist() == [0, 1, 1]
    assert int(golden.named("class 63")[0]["filled"][63]) == 4
    assert max(c["map"].size for c in golden.maps) <= 4500


def test_the_restatement_equals_scipy_on_every_case(golden):
    for c in golden.maps:
        out, filled = FR.fill_map(c["map"], c["C"], c["k"], c["classes"])
        assert np.array_equal(out, c["out"]) and out.dtype == np.uint8, c["name"]
        assert np.array_equal(filled, c["filled"]), c["name"]
        assert np.array_equal(FR.tallies_map(out, c["ref"], c["C"]), c["tallies"]), c["name"]
    for k in (1, 2, 3):
        for n in range(golden.mask.shape[0]):
            for ch in range(golden.mask.shape[1]):
                out, filled = FR.fill_mask(golden.mask[n, ch], k)
                assert np.array_equal(out, golden.mask_out[k][n, ch] != 0), (k, n, ch)
                assert filled == int((golden.mask_out[k][n, ch] != golden.mask[n, ch]).sum())
    assert not (golden.mask_out[1][0, 2]).any()                  # an all-zero volume has no hole: its component touches the faces
    assert any((golden.mask_out[k] != golden.mask).any() for k in (1, 2, 3))


def test_the_emulation_of_the_kernel_steps_equals_scipy_on_every_case(golden):
    for c in golden.maps:
        out, filled, tallies = FR.emulate_map(c["map"], c["C"], c["k"], c["classes"], reference=c["ref"])
        assert np.array_equal(out, c["out"]) and np.array_equal(filled, c["filled"]) and np.array_equal(tallies, c["tallies"]), \
            c["name"]


def test_a_single_class_map_is_the_mask_form(golden):
    for c in golden.named("single class 3"):
        out, filled = FR.fill_map(c["map"], c["C"], c["k"])
        want, n = FR.fill_mask(c["map"] == 3, c["k"])
        assert np.array_equal(out == 3, want) and int(filled[3]) == n and int(filled.sum()) == n and n > 0


def _caught_by(golden, defect):
    hits = []
    for c in golden.maps:
        out, filled, tallies = FR.emulate_map(c["map"], c["C"], c["k"], c["classes"], reference=c["ref"], defect=defect)
        if not (np.array_equal(out, c["out"]) and np.array_equal(filled, c["filled"]) and np.array_equal(tallies, c["tallies"])):
            hits.append(c["name"])
    return hits


@pytest.mark.parametrize("defect", FR.DEFECTS)
def test_a_planted_defect_is_caught(golden, defect):
    assert _caught_by(golden, defect), defect


def test_the_defects_break_where_they_should(golden):
    assert "open on face axis2 side1 k1" in _caught_by(golden, "border_face_missing")
    assert "value 200 diagonal k3" in _caught_by(golden, "ring_connectivity_1")
    assert {"two classes k1", "two classes k3"} <= set(_caught_by(golden, "two_classes_lower"))
    assert "value 200 k1" in _caught_by(golden, "value_ge_C_absent")
    assert _caught_by(golden, "unselected_filled") == ["classes=[2] k1"]
    filling = [c["name"] for c in golden.maps if int(c["filled"].sum()) and not np.array_equal(
        FR.tallies_map(c["map"], c["ref"], c["C"]), c["tallies"])]
    assert filling and _caught_by(golden, "tallies_miss_filled") == filling


# ---- the C entries check their arguments before touching a device -------------------------------------------------------------------
def test_the_entries_reject_bad_arguments_without_a_device():
    import ctypes as C
    import os
    import subprocess
    from diff_unet_amos_amd import _native as nv
    if not os.path.exists(nv.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(os.path.dirname(nv.LIB_PATH), "csrc"), "-j4"], check=True)
    lib = nv.lib()
    one, ws = C.c_void_p(16), C.c_void_p(256)
    E = nv.ERR_ARG
    size = lib.dua_fill_holes_scratch_bytes
    vox, pvs = 9 * 10 * 11, 1024
    assert size(1, 9, 10, 11, 0) == 4096 + 256 + pvs                      # parents, one scan block, one flag byte per voxel
    assert size(1, 9, 10, 11, 1) == 4096 + 256 + pvs + 8 * pvs            # and the 64-bit sets
    assert size(2, 9, 10, 11, 1) == 2 * size(1, 9, 10, 11, 1) - 256       # the block counts of two maps share a 256-byte unit
    assert size(0, 9, 10, 11, 0) == E and size(1, 0, 10, 11, 0) == E and size(1, 2048, 2048, 512, 1) == E
    assert size(65536, 9, 10, 11, 0) == E
    big = 1 << 30
    mask = lib.dua_fill_holes_mask

    def m(V=1, D=9, H=10, W=11, src=one, dtype=nv.U8, stride=vox, k=1, select=None, out=one, filled=one, ref=None, rdtype=0, is_map=0,
          Cn=1, tallies=None, work=ws, nbytes=big):
        return mask(V, D, H, W, src, dtype, stride, k, select, out, filled, ref, rdtype, is_map, Cn, tallies, work, nbytes, None)

    for bad in (dict(src=None), dict(out=None), dict(filled=None), dict(work=None), dict(k=0), dict(k=4), dict(dtype=nv.F16),
                dict(stride=vox - 1), dict(V=0), dict(D=0), dict(nbytes=size(1, 9, 10, 11, 0) - 1), dict(work=C.c_void_p(128)),
                dict(filled=C.c_void_p(12)), dict(dtype=nv.F32, src=C.c_void_p(18)), dict(ref=one), dict(tallies=one),
                dict(ref=one, tallies=one, rdtype=nv.U8, Cn=65, V=65), dict(ref=one, tallies=one, rdtype=nv.U8, Cn=2),
                dict(ref=one, tallies=one, rdtype=nv.F16), dict(ref=one, tallies=one, rdtype=nv.F32, is_map=1),
                dict(ref=one, tallies=C.c_void_p(12), rdtype=nv.U8)):
        assert m(**bad) == E, bad
    fmap = lib.dua_fill_holes_map

    def f(V=1, D=9, H=10, W=11, src=one, stride=vox, Cn=16, k=1, class_mask=0xfffe, out=one, filled=one, ref=None, tallies=None, work=ws,
          nbytes=big):
        return fmap(V, D, H, W, src, stride, Cn, k, class_mask, out, filled, ref, tallies, work, nbytes, None)

    for bad in (dict(src=None), dict(out=None), dict(filled=None), dict(work=None), dict(k=0), dict(k=4), dict(Cn=65), dict(Cn=0),
                dict(stride=vox - 1), dict(V=0), dict(W=0), dict(nbytes=size(1, 9, 10, 11, 1) - 1), dict(nbytes=size(1, 9, 10, 11, 0)),
                dict(work=C.c_void_p(128)), dict(class_mask=1), dict(class_mask=1 << 16), dict(Cn=64, class_mask=(1 << 64) - 1),
                dict(ref=one), dict(tallies=one), dict(filled=C.c_void_p(12)), dict(ref=one, tallies=C.c_void_p(12))):
        assert f(**bad) == E, bad


# ---- fill_holes= is checked before any device work -------------------------------------------------------------------------------------
def _never(*args, **kwargs):
    raise AssertionError("the predictor was called")


@pytest.mark.parametrize("bad", [dict(connectivity=4), dict(connectivity=True), dict(size=3), dict(num_components=1), [1],
                                 dict(classes=(0,)), dict(classes="12"), dict(classes=(1.5,)), dict(classes=3), dict(channels=(1,))])
def test_segment_case_refuses_a_bad_fill_holes_before_any_device_work(bad):
    from diff_unet_amos_amd import inference
    vol = torch.zeros(1, 1, 8, 8, 8)                             # a CPU tensor: the device check would raise RuntimeError
    with pytest.raises(ValueError, match="fill_holes|connectivity"):
        inference.segment_case(_never, vol, None, (8, 8, 8), fill_holes=bad)


@pytest.mark.parametrize("bad", [dict(connectivity=0), dict(classes=(1,)), dict(cap=4), "all", dict(channels=(-1,)),
                                 dict(channels=(True,)), dict(channels=2)])
def test_evaluate_volume_and_infer_refuse_a_bad_fill_holes_before_any_device_work(bad):
    from diff_unet_amos_amd import inference
    vol = torch.zeros(1, 1, 8, 8, 8)
    with pytest.raises(ValueError, match="fill_holes|connectivity"):
        inference.evaluate_volume(_never, vol, None, (8, 8, 8), fill_holes=bad)
    for streaming in (False, True):
        with pytest.raises(ValueError, match="fill_holes|connectivity"):
            inference.infer(_never, vol, (8, 8, 8), streaming=streaming, fill_holes=bad)


def test_the_postprocess_keys_are_untouched_and_the_functions_need_a_device():
    from diff_unet_amos_amd import inference, postprocess
    assert inference.SEGMENT_POSTPROCESS_KEYS == ("connectivity", "num_components", "min_size", "classes", "cap")
    assert inference.POSTPROCESS_KEYS == ("connectivity", "num_components", "min_size", "channels", "cap")
    assert postprocess.FILL_HOLES_KEYS == ("connectivity", "channels") and postprocess.FILL_HOLES_MAP_KEYS == ("connectivity", "classes")
    with pytest.raises(ValueError, match="postprocess"):
        inference.segment_case(_never, torch.zeros(1, 1, 8, 8, 8), None, (8, 8, 8), postprocess=dict(fill_holes=True))
    with pytest.raises(RuntimeError, match="MI355X"):
        postprocess.fill_holes(torch.zeros(4, 4, 4))
    with pytest.raises(RuntimeError, match="MI355X"):
        postprocess.fill_holes_in_label_map(torch.zeros(4, 4, 4, dtype=torch.uint8), 3)
    with pytest.raises(ValueError, match="connectivity"):
        postprocess.fill_holes(torch.zeros(4, 4, 4), connectivity=0)
    with pytest.raises(ValueError, match="classes"):
        postprocess.fill_holes_in_label_map(torch.zeros(4, 4, 4, dtype=torch.uint8), 3, classes=(3,))
    with pytest.raises(ValueError, match="num_classes"):
        postprocess.fill_holes_in_label_map(torch.zeros(4, 4, 4, dtype=torch.uint8), 65)
