"""The restatement of the intensity-augmentation contract (tests/augment_intensity_ref.py) pinned down on the CPU: its blur
against scipy, its fp32 emulation inside the derived bound, every planted defect outside it, the statistics of its draw, and the
argument checks of the Python class, which need no device."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import augment_intensity_ref as iref  # noqa: E402

SEED = 77


patch, STAGE_CASES = iref.patch, iref.STAGE_CASES
SHAPES = [(4, 4, 4), (8, 9, 10), (16, 16, 16)]


@pytest.mark.parametrize("sigma", [0.5, 0.62, 0.8, 1.0])
@pytest.mark.parametrize("shape", [(4, 4, 4), (5, 4, 7), (8, 9, 10), (16, 16, 16)])
def test_the_restated_blur_is_scipys_gaussian_filter(shape, sigma):
    ndimage = pytest.importorskip("scipy.ndimage")
    x = patch(shape, 3).astype(np.float64)
    want = ndimage.gaussian_filter(x, float(np.float32(sigma)), mode="reflect", truncate=4.0)
    got = iref.blur(x, sigma)
    assert iref.radius_and_taps(sigma)[0] == int(4.0 * float(np.float32(sigma)) + 0.5)
    assert np.max(np.abs(got - want)) <= 1e-14


def test_radius_and_taps():
    for sigma, R in ((0.5, 2), (0.624, 2), (0.625, 3), (0.874, 3), (0.875, 4), (1.0, 4)):
        r, taps = iref.radius_and_taps(sigma)
        assert r == R and len(taps) == 2 * R + 1 and abs(taps.sum() - 1) < 1e-15 and np.all(taps[::-1] == taps)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("name", list(STAGE_CASES))
def test_the_fp32_emulation_lies_within_the_derived_bound(name, shape):
    x = patch(shape, 11)
    row = iref.make_rows([STAGE_CASES[name]], call=5)[0]
    want, bound = iref.transform(x, row, SEED)
    got = iref.emulate(x, row, SEED)
    ratio = iref.worst_ratio(got, want, bound)
    print(f"{name} {shape}: max |emulation - fp64| / bound = {ratio:.3f}, largest bound {bound.max():.3g}")
    assert ratio <= 1.0
    if name == "none":
        assert np.array_equal(got.view(np.int32), x.view(np.int32)) and bound.max() == 0


@pytest.mark.parametrize("name", ["gamma_below", "gamma_above_invert", "contrast", "all"])
def test_a_constant_patch_stays_finite_and_comes_back(name):
    x = patch((8, 9, 10), 0, "flat")
    spec = dict(STAGE_CASES[name])
    spec.pop("noise", None)                                # noise would make it a patch like any other
    row = iref.make_rows([spec])[0]
    want, bound = iref.transform(x, row, SEED)
    got = iref.emulate(x, row, SEED)
    expect = np.float32(0.375) * np.float32(spec.get("brightness", 1.0))
    assert np.all(np.isfinite(got)) and np.all(np.isfinite(want)) and np.all(np.isfinite(bound))
    assert np.max(np.abs(want - float(expect))) <= 1e-6 and iref.worst_ratio(got, want, bound) <= 1.0


DEFECT_ROWS = {
    "reflect_index": dict(blur=0.9),
    "radius_off_by_one": dict(blur=0.9),
    "stats_before_brightness": dict(brightness=1.2, contrast=1.2),
    "sample_deviation": dict(gamma=1.3),
    "invert_once": dict(gamma=0.8, invert=True),
    "noise_block_shift": dict(noise=0.05),
}


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("defect", iref.DEFECTS)
def test_every_planted_defect_leaves_the_bound(defect, shape):
    x = patch(shape, 12)
    # alone at every shape; with every stage on at one shape, where the bound has grown through the statistics (gamma above 1: below
    # 1 the bound near t = 0 is |dt|^gamma and hides a tap of 1e-4; 720 voxels: the sample deviation differs by 1 / (2 n))
    specs = [DEFECT_ROWS[defect]] + ([dict(STAGE_CASES["all_above"], invert=True)] if shape == (8, 9, 10) else [])
    for spec in specs:
        row = iref.make_rows([spec], call=9)[0]
        want, bound = iref.transform(x, row, SEED)
        assert iref.worst_ratio(iref.emulate(x, row, SEED), want, bound) <= 1.0
        ratio = iref.worst_ratio(iref.emulate(x, row, SEED, defect=defect), want, bound)
        print(f"{defect} {shape} {sorted(spec)}: max |defect - fp64| / bound = {ratio:.3g}")
        assert ratio > 1.0


def test_noise_of_the_restatement_is_standard_normal_and_keyed_by_call_and_sample():
    n = 32 ** 3
    z, ez = iref.normals(n, SEED, 3, 1)
    assert abs(z.mean()) <= 5 / np.sqrt(n) and abs(z.var() - 1) <= 5 * np.sqrt(2 / n) and ez.max() < 1e-5
    for call, b in ((4, 1), (3, 2)):
        other, _ = iref.normals(n, SEED, call, b)
        assert abs(np.corrcoef(z, other)[0, 1]) <= 5 / np.sqrt(n)
    again, _ = iref.normals(n, SEED, 3, 1)
    assert np.array_equal(z, again)


def test_draw_statistics_and_ranges_of_the_restatement():
    rows = np.concatenate([iref.draw_rows(iref.STATS_B, c, iref.STATS_SEED) for c in range(iref.STATS_CALLS)])
    assert len(rows) == 20000
    iref.check_statistics(rows, iref.DEFAULTS)
    bits = rows.view(np.int32)
    assert np.array_equal(bits[:, iref.C_CALL_LO], np.repeat(np.arange(iref.STATS_CALLS), iref.STATS_B))
    assert np.array_equal(bits[:, iref.C_SAMPLE], np.tile(np.arange(iref.STATS_B), iref.STATS_CALLS))
    # the tags keep the draw's words apart from the producer's blocks (.., b, j) of the same seed and counter
    import augment_ref
    ctr = np.array([[7, 0, 2, j] for j in range(3)] + [[7, 0, 2, iref.DRAW_TAG + j] for j in range(3)], dtype=np.uint64)
    words = augment_ref.philox4x32_10(ctr, (5, 0))
    assert len({int(w) for w in words.reshape(-1)}) == 24


def test_draw_rows_with_forced_events_and_a_64_bit_counter():
    call = (3 << 32) | 17
    rows = iref.draw_rows(4, call, 9, **iref.ALL_ON)
    for b, row in enumerate(rows):
        mask, values, got_call, got_b = iref.split(row)
        assert mask & 31 == 31 and got_call == call and got_b == b
        assert 0.5 <= values[1] <= 1.0 and iref.radius_and_taps(values[1])[0] in (2, 3, 4)
    none = iref.draw_rows(4, call, 9, noise_prob=0, blur_prob=0, brightness_prob=0, contrast_prob=0, gamma_prob=0)
    assert np.all(none.view(np.int32)[:, 0] == 0) and np.all(none[:, 1:6] == np.float32([0, 0, 1, 1, 1]))


BAD_ARGUMENTS = [
    ("roi", dict(roi=(8, 8))), ("roi", dict(roi=(8, 3, 8))), ("roi", dict(roi="abc")),
    ("noise_prob", dict(noise_prob=1.5)), ("blur_prob", dict(blur_prob=-0.1)), ("brightness_prob", dict(brightness_prob=2)),
    ("contrast_prob", dict(contrast_prob=float("nan"))), ("gamma_prob", dict(gamma_prob=-1)),
    ("gamma_invert_prob", dict(gamma_invert_prob=1.01)),
    ("noise_std", dict(noise_std=(0.2, 0.1))), ("noise_std", dict(noise_std=(-0.1, 0.1))), ("noise_std", dict(noise_std=0.1)),
    ("blur_sigma", dict(blur_sigma=(0.5, 1.5))), ("blur_sigma", dict(blur_sigma=(0.0, 1.0))),
    ("blur_sigma", dict(blur_sigma=(0.5, float("inf")))),
    ("brightness_range", dict(brightness_range=(0.0, 1.0))), ("brightness_range", dict(brightness_range=(1.2, 0.8))),
    ("contrast_range", dict(contrast_range=(-1.0, 1.0))), ("contrast_range", dict(contrast_range=(0.5, float("nan")))),
    ("gamma_range", dict(gamma_range=(0.0, 1.5))), ("gamma_range", dict(gamma_range=(0.7, 1.5, 2.0))),
]


@pytest.mark.parametrize("name,kwargs", BAD_ARGUMENTS)
def test_bad_python_arguments_are_refused_by_name(name, kwargs):
    from diff_unet_amos_amd import augment
    with pytest.raises(ValueError, match=name):
        augment.IntensityAugmenter(**dict(dict(roi=(8, 8, 8)), **kwargs))


def test_good_python_arguments_fill_the_configuration_as_the_restatement_does():
    from diff_unet_amos_amd import augment
    kw = dict(noise_prob=0.3, noise_std=(0.01, 0.07), blur_sigma=(0.55, 0.95), brightness_range=(0.7, 1.3), contrast_range=(0.65, 1.5),
              gamma_range=(0.6, 1.9), gamma_invert_prob=0.4)
    aug = augment.IntensityAugmenter((8, 9, 10), seed=3, **kw)
    want = iref.config(**kw)
    for field, value in want.items():
        assert np.float32(getattr(aug.cfg, field)) == value, field
    assert aug.roi == (8, 9, 10) and aug.seed == 3
    for gamma_range in ((0.5, 0.9), (1.1, 1.6), (1.0, 1.0)):     # a range on one side of 1 is taken as the contract says
        got, ref = augment.IntensityAugmenter((4, 4, 4), gamma_range=gamma_range).cfg, iref.config(gamma_range=gamma_range)
        assert (np.float32(got.gamma_span_below), np.float32(got.gamma_span_above)) == (ref["gamma_span_below"], ref["gamma_span_above"])
