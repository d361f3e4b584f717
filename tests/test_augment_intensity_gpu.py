"""The intensity-augmentation kernels (csrc/augment_intensity.hip) against the restatement of their contract
(tests/augment_intensity_ref.py): rows bit for bit, every voxel of every output within the derived bound, determinism, replay
from logged rows, event statistics, the noise's distribution, the producer integration under graph capture and the argument
checks of the C ABI."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import augment_intensity_ref as iref  # noqa: E402
import augment_ref as ref  # noqa: E402

gpu = pytest.mark.gpu
DEV = "cuda:0"
SEED = 77
STAGE_CASES, patch = iref.STAGE_CASES, iref.patch


def _aug():
    from diff_unet_amos_amd import augment
    return augment


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@gpu
@pytest.mark.parametrize("roi,B,calls", [((4, 4, 4), 1, 200), ((8, 9, 10), 3, 200), ((16, 16, 16), 16, 200), ((16, 16, 16), 37, 20)])
def test_drawn_rows_are_the_restatements_bit_for_bit(roi, B, calls):
    """The augmenter's own counter over ``calls`` launches, then explicit 64-bit counters; B = 37 takes three rounds of the
    draw's 16 waves."""
    kw = dict(noise_prob=0.5, blur_prob=0.5, brightness_prob=0.5, contrast_prob=0.5, gamma_prob=0.6, gamma_invert_prob=0.5,
              noise_std=(0.01, 0.09), gamma_range=(0.6, 1.7))
    aug = _aug().IntensityAugmenter(roi, seed=SEED, device=DEV, **kw)
    got = torch.stack([aug.draw(B) for _ in range(calls)]).cpu().numpy()
    assert aug.counter == calls
    for c in range(calls):
        assert np.array_equal(_bits(got[c]), _bits(iref.draw_rows(B, c, SEED, **kw))), c
    for c in ((1 << 32) + 5, (1 << 63) + 11):
        rows = aug.draw(B, counter=c).cpu().numpy()
        assert np.array_equal(_bits(rows), _bits(iref.draw_rows(B, c, SEED, **kw))), c
    assert aug.counter == calls                              # an explicit counter leaves the device word alone
    names = _aug().split_intensity(aug.draw(B, counter=7))
    want = iref.draw_rows(B, 7, SEED, **kw)
    assert names["call"] == [7] * B and names["sample"].tolist() == list(range(B))
    assert np.array_equal(names["events"].numpy(), _bits(want)[:, iref.C_EVENTS])
    assert np.array_equal(names["gamma"].numpy(), want[:, iref.C_GAMMA]) and np.array_equal(names["blur_sigma"].numpy(), want[:, iref.C_SIGMA])


# 16-byte and 4-byte rows; one tile, partial tiles in every direction, several tiles along w; one and several workgroups in the
# pointwise passes
STAGE_SHAPES = [(4, 4, 4), (8, 9, 10), (16, 16, 16), (9, 17, 36)]
FLAT = {"flat_gamma_below": dict(gamma=0.7), "flat_gamma_invert": dict(gamma=1.4, invert=True), "flat_contrast": dict(contrast=1.2),
        "flat_all_but_noise": dict(blur=0.9, brightness=0.8, contrast=1.2, gamma=0.75, invert=True)}


def _stage_batch(shape):
    names = list(STAGE_CASES) + list(FLAT)
    specs = [dict(STAGE_CASES.get(n) or FLAT.get(n) or {}, call=1000 + i, sample=i % 3) for i, n in enumerate(names)]
    images = np.stack([patch(shape, 20 + i, "flat" if n in FLAT else "ct") for i, n in enumerate(names)])[:, None]
    return names, images, iref.make_rows(specs)


@gpu
@pytest.mark.parametrize("shape", STAGE_SHAPES)
def test_every_stage_alone_and_all_together_within_the_derived_bound(shape):
    """Hand-built rows, one sample per case, one launch sequence for the batch: every voxel of every output within the bound; the
    row without an event gives back its input's bits; in place equals out of place; a second run equals the first."""
    names, images, rows = _stage_batch(shape)
    aug = _aug().IntensityAugmenter(shape, seed=SEED, device=DEV)
    x, r = _dev(images), _dev(rows)
    out = aug.apply(x, r)
    assert out is not x and torch.equal(x.cpu(), torch.from_numpy(images))          # the input is left alone
    got = out.cpu().numpy()
    want, bound = iref.reference(images, rows, SEED)
    for i, name in enumerate(names):
        ratio = iref.worst_ratio(got[i], want[i], bound[i])
        print(f"{shape} {name}: max |device - fp64| / bound = {ratio:.3f} (largest bound {bound[i].max():.3g})")
        assert np.all(np.isfinite(got[i])) and ratio <= 1.0, name
    assert np.array_equal(_bits(got[names.index("none")]), _bits(images[names.index("none")]))
    again = aug.apply(x, r).cpu().numpy()
    assert np.array_equal(_bits(again), _bits(got))
    y = x.clone()
    assert aug.apply(y, r, out=y) is y
    assert np.array_equal(_bits(y.cpu().numpy()), _bits(got))


@gpu
def test_a_patch_of_more_voxels_than_one_sweep_of_the_pointwise_grid():
    """64 x 64 x 68 voxels: 272 workgroups' worth of 16-byte groups against the 256 a sample gets, so the passes stride, and 256
    partials per statistic, so the reduction takes several per lane."""
    shape = (64, 64, 68)
    images = np.stack([patch(shape, 5), patch(shape, 6)])[:, None]
    rows = iref.make_rows([dict(STAGE_CASES["all_above"], invert=True), dict(STAGE_CASES["all"])], call=3)
    aug = _aug().IntensityAugmenter(shape, seed=SEED, device=DEV)
    got = aug.apply(_dev(images), _dev(rows)).cpu().numpy()
    want, bound = iref.reference(images, rows, SEED)
    for i in range(2):
        ratio = iref.worst_ratio(got[i], want[i], bound[i])
        print(f"sample {i}: max |device - fp64| / bound = {ratio:.3f}")
        assert ratio <= 1.0


@gpu
def test_logged_rows_and_the_seed_replay_a_batch_from_a_fresh_augmenter():
    shape = (12, 16, 20)
    images = _dev(np.stack([patch(shape, 40 + i) for i in range(5)])[:, None])
    aug = _aug().IntensityAugmenter(shape, seed=SEED, device=DEV, **{k: v for k, v in iref.ALL_ON.items() if k.endswith("prob")})
    for _ in range(3):
        aug.draw(5)                                          # the logged call is not the first
    first = aug(images)
    logged = aug.draw(5, counter=3).cpu()                    # what a log holds: the rows of call 3, on the host
    assert aug.counter == 4 and _aug().split_intensity(logged)["call"] == [3] * 5
    fresh = _aug().IntensityAugmenter(shape, seed=SEED, device=DEV)
    again = fresh.apply(images, logged.to(DEV))
    assert np.array_equal(_bits(again.cpu().numpy()), _bits(first.cpu().numpy()))
    other = _aug().IntensityAugmenter(shape, seed=SEED + 1, device=DEV).apply(images, logged.to(DEV))
    assert not torch.equal(other, first)                     # the seed keys the noise


@gpu
def test_event_statistics_and_ranges_over_twenty_thousand_rows():
    aug = _aug().IntensityAugmenter((8, 8, 8), seed=iref.STATS_SEED, device=DEV)
    rows = torch.cat([aug.draw(iref.STATS_B) for _ in range(iref.STATS_CALLS)]).cpu().numpy()
    assert aug.counter == iref.STATS_CALLS and len(rows) == 20000
    iref.check_statistics(rows, iref.DEFAULTS)
    for call in (0, 1, 777, iref.STATS_CALLS - 1):
        want = iref.draw_rows(iref.STATS_B, call, iref.STATS_SEED)
        assert np.array_equal(_bits(rows[call * iref.STATS_B:(call + 1) * iref.STATS_B]), _bits(want)), call


@gpu
def test_the_noise_is_standard_normal_and_keyed_by_call_and_sample():
    """std = 1 on a patch of zeros leaves the normals themselves: x = fl(0 + fl(1 z))."""
    shape, n = (32, 32, 32), 32 ** 3
    rows = iref.make_rows([dict(noise=1.0, call=3, sample=1), dict(noise=1.0, call=4, sample=1), dict(noise=1.0, call=3, sample=2),
                           dict(noise=1.0, call=3, sample=1)])
    aug = _aug().IntensityAugmenter(shape, seed=SEED, device=DEV)
    z = aug.apply(torch.zeros((4, 1) + shape, device=DEV), _dev(rows)).cpu().numpy().reshape(4, n).astype(np.float64)
    mean, var = z[0].mean(), z[0].var()
    print(f"mean {mean:.5f} (bound {5 / math.sqrt(n):.5f}), variance {var:.5f} (1 +- {5 * math.sqrt(2 / n):.5f})")
    assert abs(mean) <= 5 / math.sqrt(n) and abs(var - 1) <= 5 * math.sqrt(2 / n)
    want, ez = iref.normals(n, SEED, 3, 1)
    assert iref.worst_ratio(z[0], want, ez) <= 1.0
    assert np.array_equal(z[3], z[0])
    for other in (z[1], z[2]):                               # another call, another sample: other noise
        assert abs(np.corrcoef(z[0], other)[0, 1]) <= 5 / math.sqrt(n)


PRODUCER = dict(roi=(16, 16, 16), pos=2, neg=1, flip_prob=0.3, rot90_prob=0.4, max_k=3, scale_prob=0.5, scale_factors=0.1,
                shift_prob=0.5, shift_offsets=0.1)
INTENSITY = dict(noise_prob=0.6, blur_prob=0.6, brightness_prob=0.6, contrast_prob=0.6, gamma_prob=0.7, gamma_invert_prob=0.5)


def _expect(ref_vols, vid, counter, roi, class_ids):
    """(images, labels, intensity rows, (fp64 images, bound)) of producer call ``counter`` with PRODUCER and INTENSITY."""
    ints, floats = ref.draw(ref_vols, vid, counter, seed=8, **PRODUCER)
    images, labels = ref.apply(ref_vols, ints, floats, roi, class_ids)
    rows = iref.draw_rows(len(vid), counter, SEED, **INTENSITY)
    return images.numpy(), labels.numpy(), rows, iref.reference(images.numpy(), rows, SEED)


@gpu
def test_next_with_intensity_captured_in_a_graph_gives_the_restatements_batches_replay_by_replay():
    aug = _aug()
    roi = PRODUCER["roi"]
    volumes = [ref.synthetic_volume(s, 60 + i) for i, s in enumerate([(40, 36, 44), (33, 47, 38)])]
    dev_vols = [aug.DeviceVolume(image, label, device=DEV) for image, label in volumes]
    ref_vols = [ref.RefVolume(image, label) for image, label in volumes]
    class_ids, vid = (0, 2, 5), [1, 0, 1]
    ids = torch.tensor(vid, dtype=torch.int32, device=DEV)
    intensity = aug.IntensityAugmenter(roi, seed=SEED, device=DEV, **INTENSITY)
    prod = aug.DeviceBatchProducer(dev_vols, class_ids=class_ids, seed=8, intensity=intensity, **PRODUCER)
    plain = aug.DeviceBatchProducer(dev_vols, class_ids=class_ids, seed=8, **PRODUCER)
    assert plain.intensity is None and plain.intensity_rows is None

    def expect(counter):
        return _expect(ref_vols, vid, counter, roi, class_ids)

    first = prod.next(ids)                                   # an eager call first: the capture starts at counter 1
    today = plain.next(ids)
    images0, labels0, rows0, (want0, bound0) = expect(0)
    assert np.array_equal(_bits(today[0].cpu().numpy()), _bits(images0))          # intensity=None: today's bits
    assert np.array_equal(_bits(prod.intensity_rows.cpu().numpy()), _bits(rows0))
    assert np.array_equal(first[1].cpu().numpy(), labels0) and iref.worst_ratio(first[0].cpu().numpy(), want0, bound0) <= 1.0
    assert prod.counter == 1 and intensity.counter == 1
    out_images = torch.zeros((3, 1) + roi, device=DEV)
    out_labels = torch.zeros((3, len(class_ids)) + roi, device=DEV)
    graph = torch.cuda.CUDAGraph()
    stream = torch.cuda.Stream(device=DEV)
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):         # one stream: a graph without parallel branches
            prod.next(ids, out_images, out_labels)
    torch.cuda.current_stream().wait_stream(stream)
    assert prod.counter == 1 and intensity.counter == 1      # capturing ran nothing
    seen = []
    for counter in (1, 2):
        graph.replay()
        torch.cuda.synchronize()
        _, labels, rows, (want, bound) = expect(counter)
        ratio = iref.worst_ratio(out_images.cpu().numpy(), want, bound)
        print(f"replay at counter {counter}: events {_bits(rows)[:, 0].tolist()}, max |device - fp64| / bound = {ratio:.3f}")
        assert np.array_equal(_bits(prod.intensity_rows.cpu().numpy()), _bits(rows))
        assert np.array_equal(out_labels.cpu().numpy(), labels) and ratio <= 1.0
        seen.append(out_images.cpu().numpy().copy())
    assert not np.array_equal(seen[0], seen[1])
    assert prod.counter == 3 and intensity.counter == 3 and prod.status == 0


@gpu
def test_bad_producer_arguments_are_refused():
    aug = _aug()
    image, label = ref.synthetic_volume((20, 20, 20), 1)
    vols = [aug.DeviceVolume(image, label, device=DEV)]
    with pytest.raises(ValueError, match="intensity"):
        aug.DeviceBatchProducer(vols, roi=(16, 16, 16), intensity=aug.IntensityAugmenter((8, 8, 8), device=DEV))
    with pytest.raises(ValueError, match="intensity"):
        aug.DeviceBatchProducer(vols, roi=(16, 16, 16), intensity="noise")
    # the default device ("cuda", no index) is the producer's when that is the current one
    prod = aug.DeviceBatchProducer(vols, roi=(16, 16, 16), class_ids=range(4), intensity=aug.IntensityAugmenter((16, 16, 16), gamma_prob=1.0))
    images, _ = prod.next([0, 0])
    assert images.shape == (2, 1, 16, 16, 16) and prod.intensity_rows.shape == (2, 16) and bool(torch.isfinite(images).all())
    with pytest.raises(ValueError, match="images"):
        aug.IntensityAugmenter((8, 8, 8), device=DEV).apply(torch.zeros((1, 1, 8, 8, 9), device=DEV), torch.zeros((1, 16), device=DEV))


@gpu
def test_argument_errors_through_the_c_abi():
    from diff_unet_amos_amd import _native as nv
    lib = nv.lib()
    aug = _aug().IntensityAugmenter((8, 8, 8), device=DEV)
    rows = aug.draw(2)
    x = torch.zeros((2, 1, 8, 8, 8), device=DEV)
    need = lib.dua_aug_intensity_scratch_bytes(2, 8, 8, 8)
    assert need >= 2 * 512 * 4
    scratch = torch.empty(need, dtype=torch.uint8, device=DEV)
    p, s = nv.ptr, None
    assert lib.dua_aug_intensity_apply(p(x), p(rows), 2, 8, 8, 8, 0, p(x), p(scratch), need, s) == 0
    bad_apply = [
        (None, p(rows), 2, 8, 8, 8, 0, p(x), p(scratch), need, s), (p(x), None, 2, 8, 8, 8, 0, p(x), p(scratch), need, s),
        (p(x), p(rows), 2, 8, 8, 8, 0, None, p(scratch), need, s), (p(x), p(rows), 2, 8, 8, 8, 0, p(x), None, need, s),
        (p(x), p(rows), 2, 8, 8, 8, 0, p(x), p(scratch), need - 1, s), (p(x), p(rows), 0, 8, 8, 8, 0, p(x), p(scratch), need, s),
        (p(x), p(rows), 65536, 8, 8, 8, 0, p(x), p(scratch), 1 << 40, s), (p(x), p(rows), 2, 3, 8, 8, 0, p(x), p(scratch), need, s),
        (p(x), p(rows), 2, 8, 3, 8, 0, p(x), p(scratch), need, s), (p(x), p(rows), 2, 8, 8, 3, 0, p(x), p(scratch), need, s),
        (p(x), p(rows), 2, 2048, 2048, 512, 0, p(x), p(scratch), 1 << 40, s),
        (p(x), p(rows), 2, 8, 8, 8, 0, p(x), C.c_void_p(scratch.data_ptr() + 4), need, s),
    ]
    for args in bad_apply:
        assert lib.dua_aug_intensity_apply(*args) == nv.ERR_ARG, args
    for args in ((0, 8, 8, 8), (65536, 8, 8, 8), (1, 3, 8, 8), (1, 8, 8, 3), (1, 2048, 2048, 512)):
        assert lib.dua_aug_intensity_scratch_bytes(*args) == nv.ERR_ARG, args
    counter = torch.zeros(1, dtype=torch.int64, device=DEV)

    def cfg(**kw):
        c = nv.AugIntensityConfig.from_buffer_copy(bytes(aug.cfg))
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    assert lib.dua_aug_intensity_draw(C.byref(cfg()), 2, 0, p(counter), 0, 0, p(rows), s) == 0
    assert lib.dua_aug_intensity_draw(None, 2, 0, p(counter), 0, 0, p(rows), s) == nv.ERR_ARG
    assert lib.dua_aug_intensity_draw(C.byref(cfg()), 0, 0, p(counter), 0, 0, p(rows), s) == nv.ERR_ARG
    assert lib.dua_aug_intensity_draw(C.byref(cfg()), 2, 0, None, 0, 0, p(rows), s) == nv.ERR_ARG
    assert lib.dua_aug_intensity_draw(C.byref(cfg()), 2, 0, None, 1, 5, p(rows), s) == 0          # an explicit counter needs no word
    assert lib.dua_aug_intensity_draw(C.byref(cfg()), 2, 0, p(counter), 0, 0, None, s) == nv.ERR_ARG
    bad = [dict(noise_prob=1.5), dict(blur_prob=-0.5), dict(gamma_invert_prob=float("nan")), dict(noise_std_min=-0.1),
           dict(noise_std_span=-0.1), dict(blur_sigma_min=0.0), dict(blur_sigma_min=0.7, blur_sigma_span=0.5),      # a radius of 5
           dict(blur_sigma_span=float("inf")), dict(brightness_min=0.0), dict(contrast_min=-1.0), dict(contrast_span=float("nan")),
           dict(gamma_min=0.0), dict(gamma_span_above=float("inf")), dict(gamma_min=0.5, gamma_span_below=-0.6)]
    for kw in bad:
        assert lib.dua_aug_intensity_draw(C.byref(cfg(**kw)), 2, 0, p(counter), 0, 0, p(rows), s) == nv.ERR_ARG, kw
    torch.cuda.synchronize()
    assert int(counter.item()) == 1                          # only the one good call with the device word moved it
