"""The CPU restatement of the augmented-batch contract (tests/augment_ref.py) against itself and torch, without a GPU: the
yardstick is pinned down here before tests/test_augment_gpu.py holds the kernels to it."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import augment_ref as ref  # noqa: E402



def test_philox_known_answers():
    """The known-answer vectors published with the generator (Random123 kat_vectors, philox4x32 10 rounds)."""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff, 0xffffffff), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
            (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        assert tuple(int(x) for x in ref.philox4x32_10(np.array(ctr, dtype=np.uint64), key)) == want


def test_philox_matches_a_plain_integer_form():
    """The vectorised form against Python integers, on the counter layout the sampler's known-answer test uses
    (tests/test_kernels_gpu.py: counter = (voxel, 0, step, quad), key = (seed, 0))."""
    def plain(c, k):
        c, k = list(c), list(k)
        for _ in range(10):
            p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
            c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ k[1], p0 & 0xFFFFFFFF]
            k = [(k[0] + 0x9E3779B9) & 0xFFFFFFFF, (k[1] + 0xBB67AE85) & 0xFFFFFFFF]
        return c
    ctr = np.array([[v, 0, 5, q] for v in (0, 1, 16383) for q in range(4)], dtype=np.uint64)
    got = ref.philox4x32_10(ctr, (1234, 0))
    for row, c in zip(got, ctr):
        assert [int(x) for x in row] == plain([int(x) for x in c], (1234, 0))


def test_unit_and_symmetric_are_fp32_exact():
    assert ref.unit(0xFFFFFFFF) == np.float32(1.0) - np.float32(2.0 ** -24) and ref.unit(0xFF) == 0
    assert ref.unit(0x80000000) == np.float32(0.5)
    assert ref.mulhi(0xFFFFFFFF, 3) == 2 and ref.mulhi(0, 3) == 0 and ref.mulhi(0x55555556, 3) == 1
    s = ref.symmetric(0.1, 0x80000000)
    assert s.dtype == np.float32 and s == np.float32(np.float32(np.float32(0.2) * np.float32(0.5)) + np.float32(-0.1))
    assert ref.symmetric(0.1, 0) == np.float32(-0.1)


@pytest.mark.parametrize("kind", ["both", "no_fg", "no_bg", "corner"])
def test_draw_stays_inside_the_volume_and_picks_a_member_of_its_set(kind):
    shape, roi = (37, 41, 45), (16, 16, 24)
    image, label = ref.synthetic_volume(shape, 3, kind)
    vol = ref.RefVolume(image, label)
    assert (len(vol.fg) > 0) == (kind != "no_fg") and (len(vol.bg) > 0) == (kind in ("both", "no_fg"))
    saw = set()
    for call in range(40):
        ints, floats, centres = ref.draw([vol], [0] * 10, call, seed=9, roi=roi, rot90_prob=0.5, return_centres=True)
        for row, (is_fg, centre) in zip(ints, centres):
            assert row[0] == 0
            for a in range(3):
                assert 0 <= row[1 + a] <= shape[a] - roi[a]
            assert 0 <= row[4] < 8 and 0 <= row[5] <= 3
            flat_l, flat_i = label.reshape(-1), image.reshape(-1)
            if is_fg:
                assert flat_l[centre] > 0
            else:
                assert flat_l[centre] == 0 and flat_i[centre] > 0
            saw.add(is_fg)
        assert np.all(np.abs(floats) <= np.float32(0.1))
    assert saw == {"both": {True, False}, "no_fg": {False}, "no_bg": {True}, "corner": {True}}[kind]
    if kind == "corner":                                    # the only candidate is the far corner: every start clamps to the end
        assert all(tuple(r[1:4]) == tuple(s - q for s, q in zip(shape, roi)) for r in ints)


def test_same_key_same_rows_and_other_keys_differ():
    vol = ref.RefVolume(*ref.synthetic_volume((40, 40, 40), 1))
    a = ref.draw([vol], [0] * 10, 7, seed=5, roi=(16, 16, 16))
    b = ref.draw([vol], [0] * 10, 7, seed=5, roi=(16, 16, 16))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert not np.array_equal(a[0], ref.draw([vol], [0] * 10, 8, seed=5, roi=(16, 16, 16))[0])
    assert not np.array_equal(a[0], ref.draw([vol], [0] * 10, 7, seed=6, roi=(16, 16, 16))[0])
    assert not np.array_equal(a[0], ref.draw([vol], [0] * 10, 7 + 2 ** 32, seed=5, roi=(16, 16, 16))[0])     # counter high word
    assert not np.array_equal(a[0], ref.draw([vol], [0] * 10, 7, seed=5 + 2 ** 32, roi=(16, 16, 16))[0])     # key high word


@pytest.mark.parametrize("class_ids", [tuple(range(16)), (1, 3, 7)])
def test_one_hot_channels_partition_the_listed_classes(class_ids):
    roi = (16, 16, 16)
    image, label = ref.synthetic_volume((33, 35, 37), 2)
    vol = ref.RefVolume(image, label)
    ints, floats = ref.draw([vol], [0] * 6, 0, seed=1, roi=roi, rot90_prob=0.5, flip_prob=0.5)
    images, labels = ref.apply([vol], ints, floats, roi, class_ids)
    assert images.shape == (6, 1) + roi and labels.shape == (6, len(class_ids)) + roi
    assert images.dtype == labels.dtype == torch.float32
    _, lab_int = ref.apply([vol], ints, floats, roi, tuple(range(256)))
    label_map = lab_int.argmax(1)                              # the transformed label map itself
    listed = torch.zeros(256, dtype=torch.bool)
    listed[list(class_ids)] = True
    assert torch.equal(labels.sum(1), listed[label_map].float())
    assert set(labels.unique().tolist()) <= {0.0, 1.0}


def test_apply_is_the_gather_the_header_describes():
    """The torch form (flip, flip, flip, rot90) against the inverse index map written out voxel by voxel: for output voxel
    (i, j, w), k = 1 reads x[j][n - 1 - i], k = 2 x[n - 1 - i][n - 1 - j], k = 3 x[n - 1 - j][i] of the flipped patch."""
    n, rw = 6, 8
    g = torch.Generator().manual_seed(0)
    image = torch.rand(11, 12, 13, generator=g)
    label = torch.randint(0, 4, (11, 12, 13), generator=g).to(torch.uint8)
    vol = ref.RefVolume(image, label)
    for flip in range(8):
        for k in range(4):
            start = (2, 3, 4)
            ints = np.array([[0, *start, flip, k]], dtype=np.int32)
            floats = np.array([[0.05, -0.02]], dtype=np.float32)
            images, labels = ref.apply([vol], ints, floats, (n, n, rw), (0, 1, 2, 3))
            want = torch.empty(n, n, rw)
            for i in range(n):
                for j in range(n):
                    a, c = [(i, j), (j, n - 1 - i), (n - 1 - i, n - 1 - j), (n - 1 - j, i)][k]
                    a = n - 1 - a if flip & 1 else a
                    c = n - 1 - c if flip & 2 else c
                    src = image[start[0] + a, start[1] + c, start[2]:start[2] + rw]
                    want[i, j] = src.flip(0) if flip & 4 else src
            factor = torch.tensor(1.0) + torch.tensor(0.05)
            assert torch.equal(images[0, 0], want * factor + torch.tensor(-0.02)), (flip, k)
            assert torch.equal(labels[0].argmax(0).to(torch.uint8),
                               ref.apply([ref.RefVolume(label.float(), label)], ints, np.zeros((1, 2), np.float32), (n, n, rw),
                                         (0,))[0][0, 0].to(torch.uint8)), (flip, k)


def test_the_fixed_statistics_seed_satisfies_the_derived_bounds():
    """The seed tests/test_augment_gpu.py uses for its statistics case, checked with the restatement alone."""
    cfg = dict(ref.DEFAULTS, roi=(16, 16, 16), seed=ref.STATS_SEED)
    vol = ref.RefVolume(*ref.stats_volume())
    ints, floats, fgs = [], [], []
    for call in range(ref.STATS_CALLS):
        i, f, c = ref.draw([vol], [0] * ref.STATS_B, call, return_centres=True, **cfg)
        ints.append(i); floats.append(f); fgs += [fg for fg, _ in c]
    ints, floats = np.concatenate(ints), np.concatenate(floats)
    assert len(ints) == 20000
    assert np.array_equal(np.array(fgs), ints[:, 1] <= 3) and np.all((ints[:, 1] <= 3) | (ints[:, 1] >= 20))
    # a scale or shift of exactly zero when the event happens would be miscounted: u = 1/2 exactly, 1 word in 2^24
    ref.check_event_counts(ref.event_counts(ints, floats, np.array(fgs)), len(ints), cfg)
