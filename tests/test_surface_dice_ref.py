"""Normalized Surface Dice without a GPU: the restatement (tests/surface_dice_ref.py) against the scipy fixture
(tests/golden/surface_dice_golden.npz), the empty rules, and what the entry points and the Python layers refuse before any device
work."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import surface_dice_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_EXTENT = 4096                                        # DUA_SURFACE_MAX_EXTENT


def test_restatement_equals_the_golden_exactly():
    cases, z = R.golden()
    assert [c[0] for c in cases][-3:] == ["both_empty", "identical", "shifted_one_voxel"] and len(cases) == 11
    tol = [float(t) for t in z["tolerances"]]
    assert tol == [0.0, 1.0, 1.5, 2.0, 3.0, 5.0]
    for i, (name, a, b) in enumerate(cases):
        for j, sp in enumerate(z["spacings"]):
            for m, k in enumerate(z["connectivities"]):
                r = R.surface_dice_ref(a, b, tol, tuple(float(x) for x in sp), int(k))
                what = (name, tuple(sp), int(k))
                assert r["n_a"] == int(z["n_a"][i, j, m]) and r["n_b"] == int(z["n_b"][i, j, m]), what
                assert r["within_ab"] == z["within_ab"][i, j, m].tolist(), what
                assert r["within_ba"] == z["within_ba"][i, j, m].tolist(), what
                assert R.same_bits(r["nsd"], z["nsd"][i, j, m]), what


def test_empty_rules():
    z = torch.zeros((6, 7, 5), dtype=torch.bool)
    blob = z.clone(); blob[2:4, 2:5, 1:3] = True
    full = torch.ones_like(z)
    r = R.surface_dice_ref(z, z, [0.0, 2.0])
    assert all(math.isnan(v) for v in r["nsd"]) and r["n_a"] == r["n_b"] == 0
    assert R.surface_dice_ref(z, z, [0.0, 2.0], nan_for_nonexisting=False)["nsd"] == [0.0, 0.0]
    for a, b in [(z, blob), (blob, z)]:                                   # one border empty: 0, with or without the flag
        for flag in (True, False):
            r = R.surface_dice_ref(a, b, [0.0, 100.0], nan_for_nonexisting=flag)
            assert r["nsd"] == [0.0, 0.0] and r["within_ab"] == r["within_ba"] == [0, 0]
    # a full mask has a border (the faces of the volume): the wrapper rule of the distance table does not apply
    r = R.surface_dice_ref(full, blob, [100.0])
    assert r["n_a"] == 6 * 7 * 5 - 4 * 5 * 3 and r["nsd"] == [1.0]


def test_identical_masks_give_one_at_tolerance_zero():
    cases, z = R.golden()
    i = [c[0] for c in cases].index("identical")
    assert z["tolerances"][0] == 0.0
    assert np.all(z["nsd"][i, :, :, :] == 1.0)
    name, a, b = cases[i]
    assert R.surface_dice_ref(a, b, [0.0])["nsd"] == [1.0]
    # the shifted ellipsoid is what separates d <= tau from d < tau: at unit spacing distances are exactly 1, 2, ...
    i = [c[0] for c in cases].index("shifted_one_voxel")
    assert 0.0 < z["nsd"][i, 0, 0, 0] < z["nsd"][i, 0, 0, 1] <= 1.0


@pytest.fixture(scope="module")
def lib():
    from diff_unet_amos_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "diff_unet_amos_amd", "csrc"), "-j4"], check=True)
    return _native.lib()


def _tol(values):
    return (C.c_double * len(values))(*values)


def test_entry_points_reject_bad_arguments_without_a_device(lib):
    from diff_unet_amos_amd import _native as nv
    one = C.c_void_p(256)
    E = nv.ERR_ARG
    F, U = nv.F32, nv.U8
    V, D, H, W = 4, 6, 7, 8
    vox = D * H * W
    need_dice = lib.dua_surface_dice_scratch_bytes(V, D, H, W)
    need_table = lib.dua_surface_scratch_bytes(V, D, H, W)
    assert 2 * V * vox * 8 < need_dice <= need_table
    assert lib.dua_surface_dice_scratch_bytes(V, 0, H, W) == E and lib.dua_surface_dice_scratch_bytes(0, D, H, W) == E
    assert lib.dua_surface_dice_scratch_bytes(V, D, H, MAX_EXTENT + 1) == E
    good = [1.0, 2.0, 0.0, 3.5]                                                            # [2][2]

    def dice(V=V, D=D, a=one, b=one, ta=F, tb=U, avs=vox, bvs=vox, k=1, sd=1.0, sh=1.0, sw=1.0, classes=2, T=2, tol=good,
             counts=one, within=one, nsd=one, ws=one, wsb=need_dice):
        t = None if tol is None else _tol(tol)
        return lib.dua_surface_dice_table(V, D, H, W, a, ta, avs, b, tb, bvs, k, sd, sh, sw, classes, T, t, 1, 1, counts, within,
                                          nsd, ws, wsb, None)

    def report(V=V, D=D, a=one, b=one, ta=F, tb=U, avs=vox, bvs=vox, k=1, sd=1.0, sh=1.0, sw=1.0, classes=2, T=2, tol=good,
               counts=one, out=one, within=one, nsd=one, ws=one, wsb=need_table):
        t = None if tol is None else _tol(tol)
        return lib.dua_surface_report(V, D, H, W, a, ta, avs, b, tb, bvs, k, sd, sh, sw, classes, T, t, 1, counts, out, within,
                                      nsd, ws, wsb, None)

    def bounded(D=D, seeds=one, svs=vox, mask=1, sd=1.0, sh=1.0, sw=1.0, md=2.0, out=one):
        return lib.dua_surface_edt_sq_bounded(V, D, H, W, seeds, svs, mask, sd, sh, sw, md, out, None)

    for fn in (dice, report):
        for kw in [dict(a=None), dict(b=None), dict(counts=None), dict(within=None), dict(nsd=None), dict(ws=None),
                   dict(tol=None)]:                                                        # null pointers
            assert fn(**kw) == E, (fn.__name__, kw)
        assert fn(T=0, tol=[1.0] * 4) == E                                                 # T outside 1..8
        assert fn(T=9, classes=1, tol=[1.0] * 9) == E
        assert fn(V=34, classes=17, T=8, tol=[1.0] * 136) == E                             # classes * T > 128
        assert fn(V=130, classes=130, T=1, tol=[1.0] * 130) == E
        assert fn(classes=3, T=1, tol=[1.0] * 3) == E                                      # V % classes != 0
        assert fn(classes=0) == E and fn(classes=-2) == E
        for bad in (-1.0, -1e-300, float("nan"), float("inf"), -float("inf")):             # a tolerance < 0 or non-finite
            assert fn(tol=[1.0, 2.0, bad, 3.5]) == E, (fn.__name__, bad)
        for s in (0.0, -1.0, float("nan"), float("inf")):                                  # spacing <= 0 or non-finite
            assert fn(sd=s) == E and fn(sh=s) == E and fn(sw=s) == E
        for k in (0, 4, -1):
            assert fn(k=k) == E
        assert fn(avs=vox - 1) == E and fn(bvs=vox - 1) == E                               # a stride below D H W
        assert fn(D=0) == E and fn(V=0, classes=1) == E and fn(D=-3) == E                  # extents
        assert fn(ta=1) == E and fn(tb=7) == E                                             # masks are fp32 or uint8
        assert fn(ws=C.c_void_p(264)) == E                                                 # workspace not 256-byte aligned
    assert report(out=None) == E
    assert dice(wsb=need_dice - 1) == E and report(wsb=need_table - 1) == E                # workspace smaller than the query

    for md in (-1.0, -1e-300, float("nan"), -float("inf")):                                # max_distance < 0 or NaN
        assert bounded(md=md) == E
    assert bounded(seeds=None) == E and bounded(out=None) == E
    assert bounded(svs=vox - 1) == E and bounded(mask=0) == E and bounded(mask=256) == E
    assert bounded(D=0) == E and bounded(D=MAX_EXTENT + 1) == E
    for s in (0.0, -1.0, float("nan"), float("inf")):
        assert bounded(sd=s) == E and bounded(sh=s) == E and bounded(sw=s) == E


def test_cpu_tensors_have_no_path():
    from diff_unet_amos_amd import metrics
    a = torch.zeros((1, 2, 4, 4, 4))
    for fn in (metrics.surface_dice_table, metrics.surface_report):
        with pytest.raises(RuntimeError, match="no CPU path"):
            fn(a, a, 1.0)
        with pytest.raises(RuntimeError, match="no CPU path"):
            fn(a, a, [[1.0, 2.0], [0.5, 3.0]], voxel_spacing=(2.0, 1.5, 1.5), connectivity=3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        metrics.normalized_surface_dice(a[0, 0], a[0, 0], 2.0, voxel_spacing=1.5)


def test_tolerance_forms():
    from diff_unet_amos_amd import metrics
    assert metrics._tolerance_rows(2.0, 3) == [[2.0]] * 3
    assert metrics._tolerance_rows([1.0, 2, 3.5], 3) == [[1.0], [2.0], [3.5]]
    assert metrics._tolerance_rows(np.array([[1.0, 2.0], [0.0, 3.0]]), 2) == [[1.0, 2.0], [0.0, 3.0]]
    assert metrics._tolerance_rows(torch.tensor([[1.0, 2.0], [0.0, 3.0]]), 2) == [[1.0, 2.0], [0.0, 3.0]]
    for bad, classes in [([1.0, 2.0], 3), ([[1.0, 2.0], [1.0]], 2), ([[1.0] * 9], 1), ([[]], 1), (-1.0, 2), (float("nan"), 1),
                         (float("inf"), 1), ([[1.0] * 8] * 17, 17)]:
        with pytest.raises(ValueError, match="tolerance"):
            metrics._tolerance_rows(bad, classes)


def test_evaluate_volume_refuses_a_bad_surface_argument_before_any_predictor_call():
    from diff_unet_amos_amd import inference

    def predictor(*a, **kw):
        raise AssertionError("the predictor was called")

    image = torch.zeros((1, 1, 8, 8, 8))
    labels = torch.zeros((1, 2, 8, 8, 8))
    for bad in [dict(tolerance=1.0, spacing=(1, 1, 1)), dict(tolerance=1.0, connectivty=1), "nsd", [1.0], dict(voxel_spacing=1.0)]:
        with pytest.raises(ValueError, match="surface"):
            inference.evaluate_volume(predictor, image, labels, roi_size=(8, 8, 8), surface=bad)
    with pytest.raises(ValueError, match="labels"):
        inference.evaluate_volume(predictor, image, None, roi_size=(8, 8, 8), surface=dict(tolerance=1.0))
