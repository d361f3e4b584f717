"""``postprocess.fill_holes`` / ``fill_holes_in_label_map`` and the ``fill_holes=`` argument of the inference entry points on the
GPU.  Everything is integer work: outputs, filled counts and tallies are compared for EXACT equality with the scipy fixture
(tests/golden/fill_holes_golden.npz) and the numpy restatement (tests/fill_holes_ref.py); no tolerance appears.

Map cases (name in the fixture -> what it exercises): general 9x10x11; degenerate 1x7x8 (every voxel on a face: nothing filled);
rows 3x5x300 (rows longer than a workgroup: roots cross workgroup boundaries); tile plus one 17x16x16; diagonal pockets (a hole
under k = 1, open under k = 3); open on face axis a side s (the border flag of each of the six faces); two classes (stays 0);
nested shells (the inner hole gets 2); island in pocket (not filled); value 200 (blocks the fill, C = 16); classes=[2] (only
class 2 is filled); class 63 (the top bit of the set); single class 3 (the map form is the mask form)."""
import numpy as np
import pytest
import torch

import fill_holes_ref as FR
from diff_unet_amos_amd import inference, ops, postprocess as pp
from streamed_blend_stub import CHANNELS, make_predictor
from test_segment_case_eval_gpu import KW, ROI, _raw_scan

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = FR.Golden()
MAP_NAMES = [c["name"] for c in GOLDEN.maps]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _np(t):
    return t.cpu().numpy()


@pytest.mark.parametrize("name", MAP_NAMES)
def test_the_map_form_equals_the_fixture(name):
    c = next(c for c in GOLDEN.maps if c["name"] == name)
    m, ref = _dev(c["map"]), _dev(c["ref"])
    out, filled, tallies = pp.fill_holes_in_label_map(m, c["C"], c["k"], classes=c["classes"], reference=ref)
    print(f"{name}: filled {int(filled.sum())} (fixture {int(c['filled'].sum())}), differing voxels "
          f"{int((_np(out) != c['out']).sum())}")
    assert out.dtype == torch.uint8 and out.shape == m.shape and filled.dtype == torch.int64 and tallies.dtype == torch.int64
    assert np.array_equal(_np(out), c["out"])
    assert np.array_equal(_np(filled), c["filled"]) and tuple(filled.shape) == (c["C"],)
    assert np.array_equal(_np(tallies), c["tallies"])
    assert torch.equal(m, _dev(c["map"]))                        # the input is left as it was
    plain = pp.fill_holes_in_label_map(m, c["C"], c["k"], classes=c["classes"])
    assert len(plain) == 2 and torch.equal(plain[0], out) and torch.equal(plain[1], filled)
    # the Dice of the tallies is the Dice of the returned map, recomputed in torch operators
    classes = torch.arange(c["C"], device=DEV).view(-1, 1, 1, 1)
    a, b = out[None] == classes, ref[None] == classes
    inter, denom = (a & b).sum((1, 2, 3)).double(), a.sum((1, 2, 3)).double() + b.sum((1, 2, 3)).double()
    want = torch.where(denom > 0, 2.0 * inter / denom.clamp(min=1), torch.zeros_like(denom))
    assert torch.equal(ops.dice_from_tallies(tallies), want)


def test_a_batch_of_maps_is_filled_map_by_map_and_counted_together():
    cases = GOLDEN.named("open on face")
    maps, refs = _dev(np.stack([c["map"] for c in cases])), _dev(np.stack([c["ref"] for c in cases]))
    out, filled, tallies = pp.fill_holes_in_label_map(maps, 2, 1, reference=refs)
    assert np.array_equal(_np(out), np.stack([c["out"] for c in cases]))
    assert np.array_equal(_np(filled), sum(c["filled"] for c in cases))
    assert np.array_equal(_np(tallies), sum(c["tallies"] for c in cases))


def test_a_single_class_map_is_the_mask_form():
    for c in GOLDEN.named("single class 3"):
        m = _dev(c["map"])
        out, filled = pp.fill_holes_in_label_map(m, c["C"], c["k"])
        mask, count = pp.fill_holes(m == 3, c["k"])
        assert mask.dtype == torch.bool and torch.equal(out == 3, mask) and int(filled[3]) == int(count) > 0
        assert np.array_equal(_np(mask), FR.fill_mask(c["map"] == 3, c["k"])[0])


@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32])
@pytest.mark.parametrize("k", [1, 2, 3])
def test_the_mask_form_equals_binary_fill_holes(k, dtype):
    mask_np, want = GOLDEN.mask, GOLDEN.mask_out[k]
    mask = _dev(mask_np).to(dtype)
    out, filled = pp.fill_holes(mask, k)
    print(f"k{k} {dtype}: filled {filled.tolist()}, differing voxels {int((_np(out != 0) != (want != 0)).sum())}")
    assert out.dtype == dtype and out.shape == mask.shape and filled.dtype == torch.int64
    assert np.array_equal(_np(out), want.astype(_np(out).dtype))
    assert np.array_equal(_np(filled), (want != mask_np).sum((2, 3, 4)))
    assert int(filled[0, 2]) == 0 and not bool(out[0, 2].any()) and bool(out[1, 0].all())        # all zero: no hole; all one
    # channels=[0, 2]: channel 1 is copied through and counts nothing
    some, some_filled = pp.fill_holes(mask, k, channels=[0, 2])
    expect = want.copy()
    expect[:, 1] = mask_np[:, 1]
    assert np.array_equal(_np(some), expect.astype(_np(some).dtype)) and int(some_filled[:, 1].sum()) == 0
    assert torch.equal(some_filled[:, [0, 2]], filled[:, [0, 2]]) and int(filled[:, 1].sum()) > 0
    # tallies against one-hot labels and against a label map, from the same pass
    onehot_np = np.roll(want, 1, axis=-1)
    labelmap_np = (np.arange(mask_np[0, 0].size).reshape(mask_np.shape[2:]) % 4).astype(np.uint8)[None].repeat(2, 0)
    _, _, t1 = pp.fill_holes(mask, k, labels=_dev(onehot_np).to(dtype))
    _, _, t2 = pp.fill_holes(mask, k, channels=[0, 2], labels=_dev(labelmap_np))
    assert np.array_equal(_np(t1), FR.tallies_mask(want, onehot_np))
    assert np.array_equal(_np(t2), FR.tallies_mask(expect, labelmap_np[:, None] == np.arange(3).reshape(1, 3, 1, 1, 1)))


def test_the_mask_form_copies_foreground_values_and_returns_the_input_dtype():
    want = GOLDEN.mask_out[1][1]
    soft = _dev(GOLDEN.mask[1]).float() * 0.7                    # [3, 9, 10, 11]: a mask without a batch axis, values 0 and 0.7
    out, filled = pp.fill_holes(soft)
    holes = _dev(want != GOLDEN.mask[1])
    assert torch.equal(out, torch.where(holes, torch.ones_like(soft), soft)) and tuple(filled.shape) == (3,)
    for dtype in (torch.bool, torch.int64, torch.float16):
        got, _ = pp.fill_holes(_dev(GOLDEN.mask[1]).to(dtype))
        assert got.dtype == dtype and np.array_equal(_np(got != 0), want != 0)


def test_one_graph_replay_of_the_map_form_gives_the_bits_of_the_eager_call():
    cases = GOLDEN.named("tile plus one 17x16x16")
    c, other = cases[0], cases[1]
    static, ref = _dev(other["map"]).flip(0).contiguous(), _dev(c["ref"])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                # warm-up outside the capture: library load, allocator
        pp.fill_holes_in_label_map(static, c["C"], c["k"], classes=(1, 2, 3, 5), reference=ref)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, filled, tallies = pp.fill_holes_in_label_map(static, c["C"], c["k"], classes=(1, 2, 3, 5), reference=ref)
    static.copy_(_dev(c["map"]))
    graph.replay()
    want = pp.fill_holes_in_label_map(_dev(c["map"]), c["C"], c["k"], classes=(1, 2, 3, 5), reference=ref)
    assert torch.equal(out, want[0]) and torch.equal(filled, want[1]) and torch.equal(tallies, want[2])
    ref_out, ref_filled = FR.fill_map(c["map"], c["C"], c["k"], (1, 2, 3, 5))
    assert np.array_equal(_np(out), ref_out) and np.array_equal(_np(filled), ref_filled) and int(ref_filled.sum()) > 0


# ---- segment_case / evaluate_volume / infer with fill_holes= ------------------------------------------------------------------------

def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int64) if a.dtype == torch.float64 else a,
                                                                     b.view(torch.int64) if b.dtype == torch.float64 else b)


@pytest.fixture(scope="module")
def run():
    from diff_unet_amos_amd import prepare
    image, _, affine = _raw_scan()
    case = prepare.prepare_case(image, None, affine=affine, device=DEV)
    vol = case.image[None, None].contiguous()                   # the plain-tensor case: its own grid
    pred = make_predictor(ROI, torch.device(DEV))
    plain, _ = inference.segment_case(pred, vol, None, ROI, 2, 0.25, **KW)
    label = plain.flip(0).contiguous()
    return dict(vol=vol, pred=pred, label=label, plain=inference.segment_case(pred, vol, label, ROI, 2, 0.25, **KW))


def test_segment_case_fills_after_the_map_is_made_and_none_is_the_parents_path(run):
    vol, pred, label, (out, dice) = run["vol"], run["pred"], run["label"], run["plain"]
    none = inference.segment_case(pred, vol, label, ROI, 2, 0.25, fill_holes=None, **KW)
    assert len(none) == 2 and _same(none[0], out) and _same(none[1], dice)
    fh = dict(connectivity=1)
    got = inference.segment_case(pred, vol, label, ROI, 2, 0.25, fill_holes=fh, **KW)
    want_map, filled, tallies = pp.fill_holes_in_label_map(out, CHANNELS, reference=label, **fh)
    print(f"segment_case: filled per class {filled.tolist()}")
    assert int(filled.sum()) > 0 and not _same(want_map, out)   # the stub's map has enclosed holes: the argument does something
    assert len(got) == 2 and _same(got[0], want_map) and _same(got[1], ops.dice_from_tallies(tallies))
    assert np.array_equal(_np(want_map), FR.fill_map(_np(out), CHANNELS, 1)[0])
    # the Dice returned is the Dice of the returned map, recomputed in torch operators
    classes = torch.arange(CHANNELS, device=DEV).view(-1, 1, 1, 1)
    a, b = got[0][None] == classes, label[None] == classes
    inter, denom = (a & b).sum((1, 2, 3)).double(), a.sum((1, 2, 3)).double() + b.sum((1, 2, 3)).double()
    assert torch.equal(got[1], torch.where(denom > 0, 2.0 * inter / denom.clamp(min=1), torch.zeros_like(denom)))
    # a selection of classes, no label: the filled map alone
    only = inference.segment_case(pred, vol, None, ROI, 2, 0.25, fill_holes=dict(connectivity=3, classes=(2,)), **KW)
    assert only[1] is None and _same(only[0], pp.fill_holes_in_label_map(out, CHANNELS, 3, classes=(2,))[0])


def test_segment_case_filters_first_then_fills_and_reports_the_final_map(run):
    from diff_unet_amos_amd import metrics
    vol, pred, label, (out, _) = run["vol"], run["pred"], run["label"], run["plain"]
    post, fh = dict(connectivity=2, num_components=1, min_size=2, classes=(1, 2)), dict(connectivity=2)
    surf = dict(tolerance=[[1.0, 4.0]] * 2, classes=(1, 2))
    got = inference.segment_case(pred, vol, label, ROI, 2, 0.25, postprocess=post, fill_holes=fh, surface=surf, **KW)
    kept = pp.filter_label_map(out, CHANNELS, **post)[0]
    want_map, _, tallies = pp.fill_holes_in_label_map(kept, CHANNELS, reference=label, **fh)
    assert len(got) == 3 and _same(got[0], want_map) and _same(got[1], ops.dice_from_tallies(tallies))
    report = metrics.label_map_surface_report(want_map, label, (1, 2), [[1.0, 4.0]] * 2, None)
    assert sorted(got[2]) == sorted(report) and all(_same(got[2][k], report[k]) for k in report)


def test_evaluate_volume_and_infer_fill_the_mask_after_the_filter(run):
    vol, pred = run["vol"], run["pred"]
    mask, _ = inference.evaluate_volume(pred, vol, None, ROI, 2, 0.25, **KW)
    labels = mask.flip(2).contiguous()
    post, fh = dict(num_components=1, channels=(0, 1, 2)), dict(connectivity=1, channels=(0, 2))
    got = inference.evaluate_volume(pred, vol, labels, ROI, 2, 0.25, postprocess=post, fill_holes=fh, **KW)
    kept = pp.keep_largest_components(mask, **post)
    want, filled, tallies = pp.fill_holes(kept, labels=labels, **fh)
    print(f"evaluate_volume: filled per volume {filled.tolist()}")
    assert int(filled[:, [0, 2]].sum()) > 0 and int(filled[:, [1, 3]].sum()) == 0
    assert len(got) == 2 and _same(got[0], want) and _same(got[1], ops.dice_from_tallies(tallies))
    assert _same(got[1], inference.dice_per_class(want, labels))
    only = inference.evaluate_volume(pred, vol, None, ROI, 2, 0.25, fill_holes=fh, **KW)
    assert only[1] is None and _same(only[0], pp.fill_holes(mask, **fh)[0])
    none = inference.evaluate_volume(pred, vol, labels, ROI, 2, 0.25, fill_holes=None, **KW)
    plain = inference.evaluate_volume(pred, vol, labels, ROI, 2, 0.25, **KW)
    assert _same(none[0], plain[0]) and _same(none[1], plain[1]) and _same(plain[0], mask)
    for streaming in (False, True):
        vol_out = inference.infer(pred, vol, ROI, 2, 0.25, streaming=streaming, postprocess=post, fill_holes=fh, **KW)
        assert vol_out.dtype == torch.float32 and torch.equal(vol_out, pp.fill_holes(kept, **fh)[0].float())
