"""``inference.segment_case(postprocess=, surface=)`` on the GPU with the stub predictor of the streamed-blend tests: the filtered
map, its Dice and the surface report equal the same steps composed by hand from the plain call's map, and the plain call is the
parent's code path -- a 2-tuple with the map and Dice of ``ops.blend_finish_labelmap`` on the run's own sum volume."""
import numpy as np
import pytest
import torch

import labelmap_ref as R
from diff_unet_amos_amd import inference, metrics, ops, postprocess, prepare
from streamed_blend_stub import CHANNELS, make_predictor

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROI = (8, 8, 8)
KW = dict(mirror_axes=(0,), mode="gaussian")
SPACING = (0.8, 0.9, 3.1)                          # per source axis: anisotropic, permuted and flipped on the way to RAS


def _raw_scan(shape=(24, 22, 18), seed=2):
    rng = np.random.default_rng(seed)
    blocks = rng.choice(np.array([-100, 400], dtype=np.int16), size=tuple(-(-s // 6) for s in shape))
    image = np.kron(blocks, np.ones((6, 6, 6), dtype=np.int16))[:shape[0], :shape[1], :shape[2]]
    image = image + rng.integers(-20, 20, size=shape).astype(np.int16)
    image[:2] = image[-1:] = image[:, :1] = image[:, -2:] = image[:, :, :1] = image[:, :, -1:] = -1000      # air on every side
    label = np.kron(rng.integers(0, CHANNELS + 2, size=tuple(-(-s // 4) for s in shape)), np.ones((4, 4, 4), dtype=np.int64))
    label = label[:shape[0], :shape[1], :shape[2]].astype(np.uint8)                                           # values >= C too
    return image, label, R.signed_permutation_affine((1, 2, 0), (1, -1, -1), SPACING)


@pytest.fixture(scope="module")
def run():
    image, raw_label, affine = _raw_scan()
    case = prepare.prepare_case(image, None, affine=affine, device=DEV)
    pred = make_predictor(ROI, torch.device(DEV))
    label = torch.from_numpy(raw_label).to(DEV)
    plain = inference.segment_case(pred, case, label, ROI, 2, 0.25, **KW)
    return dict(case=case, pred=pred, label=label, plain=plain)


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int64) if a.dtype == torch.float64 else a,
                                                                     b.view(torch.int64) if b.dtype == torch.float64 else b)


def test_the_default_call_is_the_parents_path(run):
    case, pred, label, plain = run["case"], run["pred"], run["label"], run["plain"]
    assert isinstance(plain, tuple) and len(plain) == 2
    out, dice = plain
    with torch.no_grad():
        acc, divisor, crop_lo, spatial = inference._streamed_sum(case.image[None, None], ROI, 2, pred, 0.25, None, None, None,
                                                                 dict(pred_type="ddim_sample"), "gaussian", 0.125, (0,))
        want, tallies = ops.blend_finish_labelmap(acc, divisor, crop_lo, spatial, case.linear_tables(), tuple(case.source_shape), 0.0,
                                                  label)
    assert _same(out, want) and _same(dice, ops.dice_from_tallies(tallies))
    assert out.dtype == torch.uint8 and tuple(out.shape) == tuple(case.source_shape) and len(torch.unique(out)) >= 2
    none = inference.segment_case(pred, case, None, ROI, 2, 0.25, postprocess=None, surface=None, **KW)
    assert len(none) == 2 and none[1] is None and _same(none[0], out)


def test_postprocess_and_surface_equal_the_steps_composed_by_hand(run):
    case, pred, label, (out, _) = run["case"], run["pred"], run["label"], run["plain"]
    assert case.source_spacing == pytest.approx(SPACING, rel=1e-12)
    pp = dict(connectivity=2, num_components=1, min_size=2, classes=(1, 2))
    surf = dict(tolerance=[[1.0, 4.0]] * 2, classes=(0, 1), connectivity=1)
    got = inference.segment_case(pred, case, label, ROI, 2, 0.25, postprocess=pp, surface=surf, **KW)
    assert isinstance(got, tuple) and len(got) == 3
    want_map, tallies = postprocess.filter_label_map(out, CHANNELS, reference=label, **pp)
    assert _same(got[0], want_map) and _same(got[1], ops.dice_from_tallies(tallies))
    want_report = metrics.label_map_surface_report(want_map, label, (0, 1), [[1.0, 4.0]] * 2, case.source_spacing, 1)
    assert sorted(got[2]) == sorted(want_report) and all(_same(got[2][k], want_report[k]) for k in want_report)
    assert tuple(got[2]["nsd"].shape) == (1, 2, 2) and bool((got[2]["hd"] > 0).all())
    unit = metrics.label_map_surface_report(want_map, label, (0, 1), [[1.0, 4.0]] * 2, None, 1)
    assert not _same(unit["hd"], got[2]["hd"])                                            # the scan's spacing was used, not 1
    # each on its own; surface alone scores the unfiltered map, default classes 1 .. C - 1
    only_pp = inference.segment_case(pred, case, label, ROI, 2, 0.25, postprocess=pp, **KW)
    assert len(only_pp) == 2 and _same(only_pp[0], want_map) and _same(only_pp[1], got[1])
    only_surf = inference.segment_case(pred, case, label, ROI, 2, 0.25, surface=dict(tolerance=2.0), **KW)
    want = metrics.label_map_surface_report(out, label, range(1, CHANNELS), 2.0, case.source_spacing)
    assert len(only_surf) == 3 and _same(only_surf[0], out) and _same(only_surf[1], run["plain"][1])
    assert all(_same(only_surf[2][k], want[k]) for k in want) and tuple(only_surf[2]["hd"].shape) == (1, CHANNELS - 1)
    # a filter that surely drops: no component of class 1 has a million voxels, and its Dice becomes 0
    assert bool((out == 1).any())
    dropped = inference.segment_case(pred, case, label, ROI, 2, 0.25, postprocess=dict(min_size=10 ** 6, classes=(1,)), **KW)
    assert _same(dropped[0], torch.where(out == 1, torch.zeros_like(out), out)) and float(dropped[1][1]) == 0.0
    assert float(run["plain"][1][1]) > 0.0
    # postprocess without a label: the filtered map and no Dice
    no_label = inference.segment_case(pred, case, None, ROI, 2, 0.25, postprocess=pp, **KW)
    assert no_label[1] is None and _same(no_label[0], want_map)


# The native entry points each call makes after its last dua_blend_accumulate*, in order, as recorded before the stage chain of
# inference.py was written once (_run_stages): the chain must make exactly these calls.  With a label or without, the names are
# the same -- the reference is an argument of the last call, not a call of its own.
# (KW is the gaussian mode: its divisor, dua_blend_weight_sum, is made after the windows and before the finish pass.)
SEGMENT_CASE_CALLS = {
    "neither": ["dua_blend_weight_sum", "dua_blend_finish_labelmap"],
    "postprocess": ["dua_blend_weight_sum", "dua_blend_finish_labelmap", "dua_cc_label_map", "dua_cc_sizes", "dua_cc_filter_map"],
    "fill_holes": ["dua_blend_weight_sum", "dua_blend_finish_labelmap", "dua_fill_holes_map"],
    "both": ["dua_blend_weight_sum", "dua_blend_finish_labelmap", "dua_cc_label_map", "dua_cc_sizes", "dua_cc_filter_map",
             "dua_fill_holes_map"],
}
EVALUATE_VOLUME_CALLS = {
    "neither": ["dua_blend_weight_sum", "dua_blend_finish_weighted"],
    "postprocess": ["dua_blend_weight_sum", "dua_blend_finish_weighted", "dua_cc_label", "dua_cc_sizes", "dua_cc_filter"],
    "fill_holes": ["dua_blend_weight_sum", "dua_blend_finish_weighted", "dua_fill_holes_mask"],
    "both": ["dua_blend_weight_sum", "dua_blend_finish_weighted", "dua_cc_label", "dua_cc_sizes", "dua_cc_filter",
             "dua_fill_holes_mask"],
}


def _calls_after_the_last_accumulate(monkeypatch, fn):
    from diff_unet_amos_amd import _native as nv
    names, real = [], nv.check

    def check(rc, what):
        names.append(what)
        return real(rc, what)

    with monkeypatch.context() as m:
        m.setattr(nv, "check", check)
        fn()
    last = max(i for i, name in enumerate(names) if name.startswith("dua_blend_accumulate"))
    return names[last + 1:]


@pytest.mark.parametrize("stages", ["neither", "postprocess", "fill_holes", "both"])
def test_the_native_calls_after_the_blend_are_the_recorded_ones(run, monkeypatch, stages):
    case, pred, label = run["case"], run["pred"], run["label"]
    has_pp, has_fill = stages in ("postprocess", "both"), stages in ("fill_holes", "both")
    vol = case.image[None, None]
    onehot_map = (torch.arange(vol[0, 0].numel(), device=DEV) % CHANNELS).to(torch.uint8).view(1, *vol.shape[2:])
    for lab, ref in ((label, onehot_map), (None, None)):
        kw = dict(postprocess=dict(connectivity=2, num_components=1, min_size=2, classes=(1, 2)) if has_pp else None,
                  fill_holes=dict(connectivity=1, classes=(1, 2)) if has_fill else None)
        got = _calls_after_the_last_accumulate(monkeypatch, lambda: inference.segment_case(pred, case, lab, ROI, 2, 0.25, **kw, **KW))
        assert got == SEGMENT_CASE_CALLS[stages], ("segment_case", lab is not None)
        kw = dict(postprocess=dict(connectivity=2, num_components=1, min_size=2, channels=(1, 2)) if has_pp else None,
                  fill_holes=dict(connectivity=1, channels=(1, 2)) if has_fill else None)
        got = _calls_after_the_last_accumulate(monkeypatch, lambda: inference.evaluate_volume(pred, vol, ref, ROI, 2, 0.25, **kw, **KW))
        assert got == EVALUATE_VOLUME_CALLS[stages], ("evaluate_volume", ref is not None)


def test_a_plain_tensor_uses_unit_spacing(run):
    case, pred = run["case"], run["pred"]
    vol = case.image[None, None]
    plain, _ = inference.segment_case(pred, vol, None, ROI, 2, 0.25, **KW)
    ref = plain.flip(0).contiguous()
    got = inference.segment_case(pred, vol, ref, ROI, 2, 0.25, surface=dict(tolerance=1.0, classes=(1,)), **KW)
    want = metrics.label_map_surface_report(plain, ref, (1,), 1.0)
    assert _same(got[0], plain) and all(_same(got[2][k], want[k]) for k in want)
    given = inference.segment_case(pred, vol, ref, ROI, 2, 0.25, surface=dict(tolerance=1.0, classes=(1,), voxel_spacing=(2.0, 1.0, 1.0)),
                                   **KW)
    assert all(_same(given[2][k], v) for k, v in metrics.label_map_surface_report(plain, ref, (1,), 1.0, (2.0, 1.0, 1.0)).items())
