"""The label map on the grid of the scan on the GPU (csrc/labelmap.hip, ops.blend_finish_labelmap, inference.segment_case)
against the fp64 restatement of the contract (tests/labelmap_ref.py) under its acceptance rule: a voxel is exempt only where the
reference's two largest probabilities (or the largest and min_prob) lie within 2 e of each other, at most 1 % of a case may be,
and every other voxel carries the reference's label exactly.  The inputs are a sum volume and a divisor built directly (logits
N(0, 2)), no network.  The shapes are the smallest at which the kernel can go wrong: a permuted and flipped geometry with the
box strictly inside the scan, crop offsets and non-uniform counts; rows that are and are not a multiple of the 4-voxel run; an
extent-1 axis; several workgroups; a channel offset past 2^31 elements.  Tallies are compared as integers with counts taken by
torch from the returned map."""
import ctypes as C

import numpy as np
import pytest
import torch

import labelmap_ref as R
from diff_unet_amos_amd import inference, ops, prepare
from streamed_blend_stub import CHANNELS, make_predictor

gpu = pytest.mark.gpu
DEV = "cuda:0"


def _device_inputs(case):
    acc = torch.from_numpy(case["sum"]).to(DEV)[None]
    if case["wsum"] is not None:
        divisor = torch.from_numpy(case["wsum"]).to(DEV)
    else:
        divisor = [torch.from_numpy(n).to(DEV) for n in case["counts"]]
    tables = (tuple(torch.from_numpy(np.ascontiguousarray(t)).to(DEV) for t in case["lo"]),
              tuple(torch.from_numpy(np.ascontiguousarray(t)).to(DEV) for t in case["weight"]), case["axis"])
    return acc, divisor, tables


def _run(case, min_prob=0.0, reference=None):
    acc, divisor, tables = _device_inputs(case)
    return ops.blend_finish_labelmap(acc, divisor, case["crop_lo"], case["spatial"], tables, case["source_shape"], min_prob, reference)


def _torch_tallies(label, reference, classes):
    c = torch.arange(classes, device=label.device).view(-1, 1, 1, 1)
    a, b = label[None] == c, reference[None] == c
    return torch.stack([(a & b).sum((1, 2, 3)), a.sum((1, 2, 3)), b.sum((1, 2, 3))], dim=1)


def _reference_map(case, seed):
    """A uint8 map on the source grid that agrees with nothing in particular and holds values >= C."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, case["C"] + 3, case["source_shape"], generator=g).to(torch.uint8).to(DEV)


@gpu
@pytest.mark.parametrize("name,weighted", [("case1", False), ("case1", True), ("case2", False), ("case2_x8", False), ("case3", False)])
def test_core_cases_against_the_fp64_reference(name, weighted):
    case = R.make_case(name, weighted=weighted)
    ref = R.reference(case)
    label, tallies = _run(case)
    assert tallies is None and label.dtype == torch.uint8 and tuple(label.shape) == case["source_shape"] and label.is_contiguous()
    ex, _ = R.check(label.cpu().numpy(), ref, what=f"{name}{' weighted' if weighted else ''}")
    assert ex == 0                                               # fixed seeds: no voxel of these cases needs the exemption
    assert (label.cpu().numpy()[~ref["inside"]] == 0).all()
    assert torch.equal(_run(case)[0], label)                     # two runs agree
    # with a reference map: the same labels, and the tallies are the counts torch takes from them
    refmap = _reference_map(case, 5)
    assert int(refmap.max()) >= case["C"]
    label2, tallies = _run(case, reference=refmap)
    assert torch.equal(label2, label)
    assert tallies.dtype == torch.int64 and torch.equal(tallies, _torch_tallies(label, refmap, case["C"]))
    assert int(tallies[:, 1].sum()) == label.numel() and int(tallies[:, 2].sum()) == int((refmap < case["C"]).sum()) < label.numel()


@gpu
@pytest.mark.parametrize("min_prob", [0.5, 0.9])
def test_min_prob_against_the_fp64_reference(min_prob):
    for name in ("case1", "case2"):
        case = R.make_case(name)
        ref = R.reference(case, min_prob)
        label, _ = _run(case, min_prob)
        R.check(label.cpu().numpy(), ref, min_prob, what=f"{name} min_prob {min_prob}")
        assert name != "case1" or (ref["label"] != R.reference(case)["label"]).any()      # the threshold removes labels there


@gpu
def test_min_prob_keeps_a_probability_equal_to_it():
    """Sums of 0 give a probability of exactly 0.5 at every corner and after every lerp: kept at min_prob = 0.5 (the rule is <),
    dropped one ulp above."""
    case = R.plant_half(R.make_case("case1"), 2)
    inside = torch.from_numpy(R.reference(case)["inside"]).to(DEV)
    label, _ = _run(case, 0.5)
    assert bool((label[inside] == 2).all()) and bool((label[~inside] == 0).all())
    above, _ = _run(case, float(np.nextafter(np.float32(0.5), np.float32(1))))
    assert int(above.max()) == 0


@gpu
def test_ties_go_to_the_lowest_channel_and_a_nan_never_wins():
    case = R.plant_tie(R.make_case("case2"), 3, 9)
    label, _ = _run(case)
    want = R.reference(case)["label"]
    assert bool((label != 9).all()) and np.array_equal(label.cpu().numpy() == 3, want == 3) and (want == 3).any()
    case = R.identity_case((3, 4, 5), 4, seed=3)
    case["sum"][0] = np.nan
    case["sum"][2, 1, 2, 3] = np.nan
    label, _ = _run(case)
    assert np.array_equal(label.cpu().numpy(), R.emulate(case)[0]) and bool((label != 0).all()) and int(label[1, 2, 3]) != 2
    case["sum"][:, 0, 0, 0] = np.nan
    assert int(_run(case)[0][0, 0, 0]) == 0


@gpu
@pytest.mark.parametrize("spatial,pad", [((20, 24, 36), (1, 2, 3)), ((5, 6, 7), (0, 0, 0))])
def test_identity_tables_against_argmax_of_blend_finish(spatial, pad):
    """Identity tables, every weight 0: the arg-max of sigmoid(q_out) of dua_blend_finish on the same sum volume.  17 280 voxels are
    17 workgroups."""
    case = R.identity_case(spatial, 6, seed=21, pad=pad)
    acc, divisor, tables = _device_inputs(case)
    q = ops.blend_finish(acc, divisor, pad, spatial, want_q=True)[0][0]
    ref = R.reference(case)
    prob = torch.sigmoid(q.double()).cpu().numpy()
    assert np.abs(prob - ref["prob"]).max() <= float(ref["bound"].max())        # the reference's logits are q_out
    label, _ = _run(case)
    got = label.cpu().numpy()
    R.check(got, ref, what=f"identity {spatial}")
    same = got == prob.argmax(axis=0)
    assert same[~R.exempt(ref)].all()


@gpu
def test_a_channel_offset_past_2_to_the_31_elements():
    """64 planes of 4096 x 8200 voxels: the last channel starts 2.1e9 elements into the sum volume.  Eight source voxels read the
    last row; the planted value sits in channel 63 alone."""
    Cn, H, W = 64, 4096, 8200
    acc = torch.zeros(1, Cn, 1, H, W, device=DEV)
    xs = [0, 1, 5, 100, 8190, 8198, 8199, 4000]
    for x in xs[:-1]:
        acc[0, Cn - 1, 0, H - 1, x] = 5.0
    acc[0, Cn - 1, 0, H - 2, 4000] = 5.0                          # not read: x = 4000 of the last row stays 0 in every channel
    ones = [torch.ones(n, dtype=torch.int32, device=DEV) for n in (1, H, W)]
    lo = (torch.tensor([0], dtype=torch.int32, device=DEV), torch.tensor([(H - 1) * W], dtype=torch.int32, device=DEV),
          torch.tensor(xs, dtype=torch.int32, device=DEV))
    weight = tuple(torch.zeros(n, device=DEV) for n in (1, 1, 8))
    label, _ = ops.blend_finish_labelmap(acc, ones, (0, 0, 0), (1, H, W), (lo, weight, (0, 1, 2)), (1, 1, 8))
    assert label.flatten().tolist() == [Cn - 1] * 7 + [0]


@gpu
def test_no_class_by_source_tensor_is_allocated():
    case = R.identity_case((48, 48, 48), 16, seed=4)
    acc, divisor, tables = _device_inputs(case)
    refmap = _reference_map(case, 6)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    label, tallies = ops.blend_finish_labelmap(acc, divisor, (0, 0, 0), case["spatial"], tables, case["source_shape"], 0.0, refmap)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - before
    print(f"peak extra memory {extra} bytes for {label.numel()} labels; one fp32 channel on the source grid is {4 * label.numel()}")
    assert extra <= label.numel() + 4096                         # the label map and the tallies: not even one fp32 channel
    assert torch.equal(tallies, _torch_tallies(label, refmap, 16))


# ---- segment_case, end to end ----

def _raw_scan(shape=(24, 22, 18), seed=2):
    rng = np.random.default_rng(seed)
    # 6^3 blocks of soft tissue and bone: the stub's channel 0 (2 v + field) wins in bone, channel 1 (flip(v) + 1 + field) elsewhere
    blocks = rng.choice(np.array([-100, 400], dtype=np.int16), size=tuple(-(-s // 6) for s in shape))
    image = np.kron(blocks, np.ones((6, 6, 6), dtype=np.int16))[:shape[0], :shape[1], :shape[2]]
    image = image + rng.integers(-20, 20, size=shape).astype(np.int16)
    image[:2] = image[-1:] = image[:, :1] = image[:, -2:] = image[:, :, :1] = image[:, :, -1:] = -1000      # air on every side
    label = rng.integers(0, CHANNELS + 2, size=shape).astype(np.uint8)                                          # values >= C too
    # source axes point along world (1, 2, 0) with signs (+, -, -): permuted and flipped on the way to RAS
    return image, label, R.signed_permutation_affine((1, 2, 0), (1, -1, -1), (0.8, 0.9, 1.1))


def _case_from_q(q, geometry):
    """The inputs of the restatement for a run whose normalised volume ``q`` (fp32 [C, *prepared]) is known: divisor 1."""
    t = prepare.linear_restore_tables(geometry)
    shape = tuple(q.shape[1:])
    return dict(name="from q_out", sum=q, counts=tuple(np.ones(n, dtype=np.int32) for n in shape), wsum=None, crop_lo=(0, 0, 0),
                spatial=shape, source_shape=geometry.source_shape, box=geometry.box, flip=geometry.flip, perm=geometry.perm,
                C=q.shape[0], lo=t["lo"], weight=t["weight"], step=t["step"], axis=t["axis"])


@gpu
def test_segment_case_end_to_end():
    """A synthetic raw scan through prepare_case, the stub predictor of the streamed-blend tests at roi 8^3 with mirroring along D
    and Gaussian weighting, then the label map on the scan's grid: against the fp64 reference fed from the run's own q_out."""
    image, raw_label, affine = _raw_scan()
    case = prepare.prepare_case(image, None, affine=affine, device=DEV)
    assert case.orientation == ((2, 0, 1), (True, False, True)) and all(lo > 0 and hi < n for (lo, hi), n in zip(case.box, image.shape))
    roi, kw = (8, 8, 8), dict(mirror_axes=(0,), mode="gaussian")
    pred = make_predictor(roi, torch.device(DEV))
    raw = torch.from_numpy(raw_label).to(DEV)
    label, dice = inference.segment_case(pred, case, raw, roi, 2, 0.25, **kw)
    assert label.dtype == torch.uint8 and tuple(label.shape) == image.shape and dice.dtype == torch.float64 and dice.shape == (CHANNELS,)
    q = inference.streamed_sliding_window_inference(case.image[None, None], roi, 2, pred, 0.25, pred_type="ddim_sample", **kw)[0]
    ref = R.reference(_case_from_q(q.cpu().numpy(), case.geometry))
    R.check(label.cpu().numpy(), ref, what="segment_case")
    inside_labels = np.unique(ref["label"][ref["inside"]]).tolist()
    assert inside_labels[:2] == [0, 1] and CHANNELS - 1 not in inside_labels                # both win somewhere; the stub's last class is empty
    tallies = _torch_tallies(label, raw, CHANNELS)
    assert torch.equal(dice, ops.dice_from_tallies(tallies)) and float(dice[CHANNELS - 1]) == 0.0 and float(dice[:2].min()) > 0.0
    assert case._linear_tables is not None and case.linear_tables() is case._linear_tables       # uploaded once
    again, none = inference.segment_case(pred, case, None, roi, 2, 0.25, **kw)
    assert none is None and torch.equal(again, label)
    # min_prob: what the reference gives with the same threshold
    thresholded, _ = inference.segment_case(pred, case, None, roi, 2, 0.25, min_prob=0.75, **kw)
    R.check(thresholded.cpu().numpy(), R.reference(_case_from_q(q.cpu().numpy(), case.geometry), 0.75), 0.75, what="segment_case 0.75")
    # a plain tensor is its own grid: the arg-max of sigmoid(q_out)
    vol = case.image[None, None]
    plain, none = inference.segment_case(pred, vol, None, roi, 2, 0.25, **kw)
    own = R.identity_case(tuple(vol.shape[2:]), CHANNELS, seed=0)
    own.update(sum=q.cpu().numpy(), counts=tuple(np.ones(n, dtype=np.int32) for n in vol.shape[2:]))
    R.check(plain.cpu().numpy(), R.reference(own), what="segment_case on a plain tensor")
    with pytest.raises(ValueError, match="is on"):
        inference.segment_case(pred, case, torch.from_numpy(raw_label), roi)


# ---- argument errors leave the outputs alone ----

@gpu
def test_argument_errors_leave_the_output_unchanged():
    from diff_unet_amos_amd import _native as nv
    case = R.make_case("case1")
    acc, divisor, (lo, weight, axis) = _device_inputs(case)
    X, P = case["source_shape"], tuple(acc.shape[2:])
    out = torch.full(X, 7, dtype=torch.uint8, device=DEV)
    refmap = _reference_map(case, 9)
    tallies = torch.full((case["C"], 3), -5, dtype=torch.int64, device=DEV)
    misaligned = torch.zeros(acc.numel() + 1, device=DEV)[1:]                   # fp32 data 4 bytes off is aligned; 2 bytes off:
    odd = C.c_void_p(misaligned.data_ptr() + 2)

    def call(sum_=nv.ptr(acc), Cn=case["C"], X_=X, min_prob=0.0, lo0=nv.ptr(lo[0])):
        return nv.lib().dua_blend_finish_labelmap(sum_, Cn, *P, *(nv.ptr(t) for t in divisor), None, *case["crop_lo"], *case["spatial"],
                                                  *X_, lo0, nv.ptr(lo[1]), nv.ptr(lo[2]), *(nv.ptr(t) for t in weight), *axis,
                                                  min_prob, nv.ptr(out), nv.ptr(refmap), nv.ptr(tallies), nv.stream_ptr())

    for kw in (dict(sum_=None), dict(lo0=None), dict(Cn=0), dict(Cn=256), dict(X_=(1 << 11, 1 << 10, 1 << 10)), dict(sum_=odd),
               dict(min_prob=float("nan"))):
        assert call(**kw) == nv.ERR_ARG, kw
    torch.cuda.synchronize()
    assert bool((out == 7).all()) and bool((tallies == -5).all())
    assert call() == 0                                                          # and the good call writes both
    assert torch.equal(out, _run(case)[0]) and torch.equal(tallies, _torch_tallies(out, refmap, case["C"]))
