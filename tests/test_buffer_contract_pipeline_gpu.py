"""Buffer contract of the input pipeline (intensity augmentation, the device batch producer, case preparation), the streamed
blend's finish pass and the whole plans (one denoiser evaluation, one training step); see
tests/test_buffer_contract_conv_gpu.py for the four checks and tests/buffer_contract.py for the three runs.

What check 2 (the same bytes in the three runs) covers, and the promise behind it:

  aug_intensity_apply            include/dua_hip.h:1455 (partials combined in a fixed order: the bits are the same from run to run)
  DeviceBatchProducer.next       include/dua_hip.h:1281, 1323 (params and labels reproducible bit for bit), and :1455
  prep_foreground_box            include/dua_hip.h:1642 (integer atomicMin / Max / Add: no dependence on the order of arrival)
  prep_resample, prep_restore    include/dua_hip.h:1611 (the deterministic front of the transform chain; one thread per output)
  blend_finish                   include/dua_hip.h:1516, 1530 (bit-equal, identical between runs; integer counters)
  one denoiser evaluation        include/dua_hip.h:30-32 (integer statistics) and tests/test_diffunet_gpu.py, which holds a
                                 graph replay to the eager bits
  one training step              the forward logits only: the backward adds with fp32 atomics (include/dua_hip.h:205, 294-296, and
                                 test_training_harness holds two walks to 1e-6, not to equality), so every gradient passes
                                 check 1 in every mode instead

UNSPECIFIED, the table of regions check 2 leaves out, is empty.
"""
import numpy as np
import pytest
import torch

import augment_intensity_ref as iref
import augment_ref as aref
import buffer_contract as BC
import prepare_ref as PR
import test_augment_intensity_gpu as TAI
import test_diffunet_gpu as TDU
import test_prepare_gpu as TPG
import test_training_harness as TTH
from streamed_blend_stub import CHANNELS, make_predictor, seeded_volume

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
UNSPECIFIED = {}


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


# ---- intensity augmentation and the producer -------------------------------------------------------------------------------------
def _intensity_case(shape, B, holders):
    from diff_unet_amos_amd import augment
    specs = [dict(iref.STAGE_CASES[("all", "all_above")[i % 2]], call=500 + i, sample=i) for i in range(B)]
    images = np.stack([iref.patch(shape, 30 + i) for i in range(B)])[:, None]
    rows = iref.make_rows(specs)
    aug = augment.IntensityAugmenter(shape, seed=TAI.SEED, device=DEV)
    aug.apply(TAI._dev(images), TAI._dev(rows))               # the augmenter now caches its scratch: guarded() drops it
    assert aug._scratch is not None
    holders.append(aug)
    x, r = TAI._dev(images), TAI._dev(rows)
    return (lambda: dict(out=aug.apply(x, r))), images, rows


def test_aug_intensity_apply():
    """B = 2 patches of 8^3 through every stage: the blur and statistics scratch (cached by the augmenter) and the output."""
    holders, others = [], []
    run, images, rows = _intensity_case((8, 8, 8), 2, holders)
    leftover, _, _ = _intensity_case((9, 17, 36), 3, others)
    outs, _ = BC.run_modes(run, leftover, holders=holders, leftover_holders=others)
    want, bound = iref.reference(images, rows, TAI.SEED)
    for mode in ("b", "a", "c"):
        got = outs[mode]["out"].cpu().numpy()
        for i in range(2):
            ratio = iref.worst_ratio(got[i], want[i], bound[i])
            assert np.all(np.isfinite(got[i])) and ratio <= 1.0, (mode, i, ratio)
    BC.same_bits(outs, unspecified=UNSPECIFIED)
    assert holders[0]._scratch is not None                    # put back


def _producer_case(roi, shapes, vid):
    from diff_unet_amos_amd import augment
    volumes = [aref.synthetic_volume(s, 60 + i) for i, s in enumerate(shapes)]
    dev_vols = [augment.DeviceVolume(image, label, device=DEV) for image, label in volumes]
    ref_vols = [aref.RefVolume(image, label) for image, label in volumes]
    class_ids = (0, 2, 5)
    ids = torch.tensor(vid, dtype=torch.int32, device=DEV)
    kw = dict(TAI.PRODUCER, roi=roi)

    def run():                                                # a fresh producer per run: its first call, counter 0
        intensity = augment.IntensityAugmenter(roi, seed=TAI.SEED, device=DEV, **TAI.INTENSITY)
        prod = augment.DeviceBatchProducer(dev_vols, class_ids=class_ids, seed=8, intensity=intensity, **kw)
        images, labels = prod.next(ids)
        return dict(images=images, labels=labels, rows=prod.intensity_rows, status=prod._status)
    return run, ref_vols, class_ids


def test_device_batch_producer_next():
    vid = [1, 0, 1]
    run, ref_vols, class_ids = _producer_case(TAI.PRODUCER["roi"], [(40, 36, 44), (33, 47, 38)], vid)
    leftover, _, _ = _producer_case(TAI.PRODUCER["roi"], [(21, 30, 26)], [0, 0, 0, 0, 0])
    outs, _ = BC.run_modes(run, leftover)
    _, labels0, rows0, (want0, bound0) = TAI._expect(ref_vols, vid, 0, TAI.PRODUCER["roi"], class_ids)
    o = outs["b"]
    assert np.array_equal(_bits(o["rows"].cpu().numpy()), _bits(rows0))
    assert np.array_equal(o["labels"].cpu().numpy(), labels0) and int(o["status"]) == 0
    assert iref.worst_ratio(o["images"].cpu().numpy(), want0, bound0) <= 1.0
    BC.same_bits(outs, unspecified=UNSPECIFIED)


# ---- case preparation ---------------------------------------------------------------------------------------------------------
def _prepare_case(image, label, affine, pixdim):
    from diff_unet_amos_amd import ops, prepare
    nothing = torch.from_numpy(np.full(image.shape, -175, dtype=image.dtype)).to(DEV)       # none above a_min

    def run():
        case = prepare.prepare_case(image, label, affine=affine, pixdim=pixdim, axcodes="RAS", device=DEV)
        return dict(image=case.image, label=case.label, restored=case.restore(case.label),
                    no_foreground=ops.prep_foreground_box(nothing, -175.0))
    return run


@pytest.mark.parametrize("dtype", sorted(TPG.DTYPES))
def test_case_preparation(dtype):
    """prep_foreground_box (with the scan that finds nothing), prep_resample and prep_restore at 13 x 10 x 7 through
    prepare.prepare_case and PreparedCase.restore."""
    image, label = TPG._restore_operands()
    image = image.astype(TPG.DTYPES[dtype])
    affine = PR.signed_permutation_affine((1, 2, 0), (1, -1, -1), TPG.SPACING)
    ref = PR.prepare(image, label, affine, TPG.PIXDIM, "RAS")
    big, big_label = TPG._case((20, 17, 9), seed=3, dtype=TPG.DTYPES[dtype])
    outs, _ = BC.run_modes(_prepare_case(image, label, affine, TPG.PIXDIM),
                           _prepare_case(big, big_label, np.diag([0.9, 1.1, 2.5, 1.0]), (1.5, 1.5, 1.5)))
    for mode in ("b", "a", "c"):
        o = outs[mode]
        assert tuple(o["image"].shape) == ref["shape"] and np.array_equal(o["label"].cpu().numpy(), ref["label"]), mode
        err = float(np.abs(o["image"].cpu().numpy().astype(np.float64) - ref["image"]).max())
        assert err <= PR.image_bound(), (mode, err)
        assert np.array_equal(o["restored"].cpu().numpy(), PR.restore(ref["label"], ref)), mode
        assert o["no_foreground"].tolist() == [2 ** 31 - 1] * 3 + [-1] * 3 + [0, 0], mode
    BC.same_bits(outs, unspecified=UNSPECIFIED)


# ---- the finish pass of the streamed blend ------------------------------------------------------------------------------------
def _blend_case(shape, roi, overlap, swb):
    from diff_unet_amos_amd.inference import evaluate_volume, streamed_sliding_window_inference
    dev = torch.device(DEV)
    pred = make_predictor(roi, dev)
    vol = seeded_volume(shape).to(dev)
    g = torch.Generator().manual_seed(5)
    label_map = torch.randint(0, CHANNELS - 1, (shape[0], *shape[2:]), generator=g).to(torch.uint8).to(dev)

    def run():
        q = streamed_sliding_window_inference(vol, roi, swb, pred, overlap, pred_type="ddim_sample")
        mask, dice = evaluate_volume(pred, vol, label_map, roi, swb, overlap)
        return dict(q=q, mask=mask, dice=dice)
    return run, pred, vol, label_map


@pytest.mark.parametrize("shape,roi,overlap,swb,other", [
    ((1, 1, 5, 8, 11), (8, 8, 8), 0.8, 3, ((2, 1, 9, 16, 16), (8, 8, 8), 0.5, 4)),            # padded, cropped by the finish pass
    ((1, 1, 32, 32, 48), (16, 16, 16), 0.5, 4, ((1, 1, 8, 8, 8), (8, 8, 8), 0.25, 2)),        # the 16-byte finish pass
], ids=["cropped", "16-byte"])
def test_blend_finish(shape, roi, overlap, swb, other):
    from diff_unet_amos_amd.inference import binarise, dice_per_class, sliding_window_inference
    run, pred, vol, label_map = _blend_case(shape, roi, overlap, swb)
    want = sliding_window_inference(vol, roi, swb, pred, overlap, pred_type="ddim_sample")       # the list-and-blend path
    outs, _ = BC.run_modes(run, _blend_case(*other)[0])
    o = outs["b"]
    assert torch.equal(o["q"], want)
    onehot = (label_map[:, None] == torch.arange(CHANNELS, device=vol.device).view(1, -1, 1, 1, 1)).float()
    assert torch.equal(o["dice"], dice_per_class(o["mask"].float(), onehot))
    assert not bool(((o["mask"].float() != binarise(want)) & (want.abs() > 2.0 ** -20)).any())
    BC.same_bits(outs, unspecified=UNSPECIFIED)


# ---- whole plans ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,mx,mean", [(torch.float32, 2e-3, 2e-4), (torch.float16, 1e-2, 1e-3)], ids=["f32", "f16"])
def test_one_denoiser_evaluation(dtype, mx, mean):
    """The TINY model at 2 x 32^3: the launch plan -- its activation buffers, statistics arena, packed weights and split-K scratch
    -- is built by the first forward call, inside the block."""
    g = torch.Generator().manual_seed(1)
    image = torch.rand(2, 1, 32, 32, 32, generator=g)
    x = torch.randn(2, 2, 32, 32, 32, generator=g)
    t = torch.tensor([999, 3])
    _, ref = TDU._pair(TDU.TINY, dtype)
    with torch.no_grad():
        want = ref(image=image, x=x, step=t, pred_type="denoise")
    dev = [v.cuda() for v in (image, x, t)]
    other = [v.cuda() for v in (torch.rand(1, 1, 32, 32, 48, generator=g), torch.randn(1, 2, 32, 32, 48, generator=g), t[:1])]
    nets = [TDU._pair(TDU.TINY, dtype)[0] for _ in range(4)]          # the same weights four times: a network keeps its plan

    def case(args):
        def run():
            net = nets.pop()
            with torch.no_grad():
                return dict(logits=net(image=args[0], x=args[1], step=args[2], pred_type="denoise"))
        return run

    outs, _ = BC.run_modes(case(dev), case(other), arena_bytes=256 << 20)
    d = (outs["b"]["logits"].cpu() - want).abs()
    assert d.max() < mx and d.mean() < mean, (float(d.max()), float(d.mean()))
    BC.same_bits(outs, unspecified=UNSPECIFIED)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_one_training_step(dtype):
    """Forward and backward of the HIP training path on the smallest model of test_training_harness (2 x 32^3): every activation,
    every packed weight, the cached weight-gradient and split-K workspaces and every gradient accumulator come from the arena."""
    from diff_unet_amos_amd.diff_unet import DiffUNet
    from diff_unet_amos_amd.training import native_conv_denoise
    from oracle.unet_ref import RefDiffUNet
    dev = torch.device(DEV)
    torch.manual_seed(0)
    ref = RefDiffUNet(**TTH.KW)
    net = DiffUNet(**TTH.KW)
    net.load_state_dict(ref.state_dict())
    net = net.to(dev)
    crit = TTH.Loss()
    scale = 4096.0 if dtype == torch.float16 else 1.0

    def case(n, seed):
        image, labels, noise, t = TTH._data(n, seed)
        x_t = ref.diffusion.q_sample(labels * 2 - 1, t, noise)
        args = [v.to(dev) for v in (image, x_t, t, labels)]

        def run():
            net.zero_grad(set_to_none=True)
            got = native_conv_denoise(net, args[0], args[1], args[2], dtype)
            (crit(got, args[3]) * scale).backward()
            return dict(logits=got.detach(), grads={k: p.grad for k, p in net.named_parameters()})
        return run, image, labels, x_t, t

    run, image, labels, x_t, t = case(2, 21)
    want = ref(image=image, x=x_t, step=t, pred_type="denoise")
    crit(want, labels).backward()
    outs, _ = BC.run_modes(run, case(1, 22)[0], arena_bytes=512 << 20)
    for mode in ("b", "a", "c"):
        for k, p in net.named_parameters():
            p.grad = outs[mode]["grads"][k]
        try:
            TTH._check_native_step(ref, net, outs[mode]["logits"], want, dtype, scale)
        except AssertionError as e:
            raise AssertionError(f"mode {mode}: {e}") from e
    net.zero_grad(set_to_none=True)
    BC.same_bits(outs, only={"logits"}, unspecified=UNSPECIFIED)
