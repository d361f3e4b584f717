"""The restatement of the class-balanced crop centres (tests/augment_classes_ref.py) checked on its own, without a GPU: the
edge cases of cum, the K = 2 cross-check against the pos / neg candidate sets, and the frequencies of the drawn classes."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import augment_classes_ref as cref  # noqa: E402
import augment_ref as ref  # noqa: E402

EDGE_U = (0.0, 2.0 ** -24, 1.0 - 2.0 ** -24)


def test_a_class_with_ratio_zero_or_without_candidates_is_never_chosen():
    counts = [50, 7, 0, 300, 1, 0]
    ratios = [0.0, 2.0, 100.0, 1.0, 0.5, 3.0]                 # class 0 unweighted; classes 2 and 5 absent, 2 with the largest ratio
    row = cref.cum(ratios, counts)
    assert row.dtype == np.float32 and list(row[4:]) == [1.0, 1.0]             # the last present class, and every class after it
    assert row[0] == 0.0 and row[2] == row[1]                                  # e_k = 0: cum_k == cum_(k-1)
    assert row[1] == np.float32(2.0 / 3.5) and row[3] == np.float32(3.0 / 3.5)  # running sum and one division in fp64, rounded once
    seen = {cref.choose(row, np.float32(i) / np.float32(4096)) for i in range(4096)}
    seen |= {cref.choose(row, np.float32(u)) for u in EDGE_U}
    assert seen == {1, 3, 4}


def test_every_edge_u_chooses_a_present_class():
    rng = np.random.RandomState(5)
    for _ in range(200):
        K = int(rng.randint(1, 65))
        counts = [int(c) for c in rng.randint(0, 3, K) * rng.randint(1, 1000, K)]
        ratios = [float(r) for r in rng.randint(0, 3, K) * rng.rand(K) * 10.0 ** rng.randint(-6, 7)]
        present = [k for k in range(K) if counts[k] > 0 and ratios[k] > 0]
        if not present:
            with pytest.raises(ValueError, match="E == 0"):
                cref.cum(ratios, counts)
            continue
        row = cref.cum(ratios, counts)
        assert all(row[k] == 1.0 for k in range(present[-1], K)) and bool(np.all(np.diff(row) >= 0))
        for u in EDGE_U:
            assert cref.choose(row, np.float32(u)) in present
        assert cref.choose(row, np.float32(0.0)) == present[0] and cref.choose(row, np.float32(EDGE_U[2])) == present[-1]


def test_e_zero_is_reported():
    with pytest.raises(ValueError, match="E == 0"):
        cref.cum([0.0, 1.0, 1.0], [10, 0, 0])
    with pytest.raises(ValueError, match="E == 0"):
        cref.cum([0.0, 0.0], [10, 10])


def test_the_package_computes_the_same_cum():
    """DeviceBatchProducer's host function (Python floats) against the restatement (numpy float64), bit for bit."""
    from diff_unet_amos_amd import augment
    rng = np.random.RandomState(6)
    for _ in range(300):
        K = int(rng.randint(1, 65))
        counts = [int(c) for c in rng.randint(0, 2, K) * rng.randint(1, 10 ** 6, K)]
        ratios = [float(r) for r in rng.randint(0, 3, K) * rng.rand(K) * 10.0 ** rng.randint(-3, 4)]
        got = augment.class_cum(ratios, counts)
        if sum(cref.effective(ratios, counts)) == 0.0:
            assert got is None
            continue
        got = torch.tensor(got, dtype=torch.float64).to(torch.float32).numpy()
        assert np.array_equal(got.view(np.int32), cref.cum(ratios, counts).view(np.int32))


def test_with_two_classes_the_sets_are_the_pos_neg_sets():
    for seed, kind in ((1, "both"), (2, "no_fg"), (3, "no_bg")):
        image, label = ref.synthetic_volume((19, 23, 29), seed, kind=kind, classes=6)
        vol = ref.RefVolume(image, label, image_threshold=0.1)
        sets = cref.class_sets(image.numpy(), label.numpy(), 6, image_threshold=0.1)
        assert np.array_equal(sets[0], vol.bg)
        assert np.array_equal(np.sort(np.concatenate(sets[1:])), vol.fg)
        two = cref.class_sets(image.numpy(), (label > 0).to(torch.uint8).numpy(), 2, image_threshold=0.1)
        assert np.array_equal(two[0], vol.bg) and np.array_equal(two[1], vol.fg)
        table = cref.prefix_table(sets, image.numel())
        assert table.shape == (6, 14) and [int(t) for t in table[:, -1]] == [len(s) for s in sets]
        assert int(table[1:].sum(0)[-1]) == len(vol.fg)


def test_frequencies_and_ranks_over_twenty_thousand_restated_draws():
    vol = cref.frequency_volume()
    assert vol.counts[4] == 0 and vol.counts[1] == 1 and vol.counts[2] == 1 and min(vol.counts[0], vol.counts[3], vol.counts[5]) > 50
    chosen, ranks = [], []
    for call in range(cref.FREQ["calls"]):
        _, _, c, r = cref.draw_classes([vol], [0] * cref.FREQ["B"], call, seed=cref.FREQ["seed"], class_ratios=cref.FREQ["ratios"],
                                       uniform_prob=cref.FREQ["uniform_prob"], roi=cref.FREQ["roi"], return_ranks=True)
        chosen.append(c); ranks.extend(r)
    chosen = np.concatenate(chosen)
    assert len(chosen) == 20000
    cref.check_frequencies(chosen, vol)
    for k in (0, 3, 5, cref.UNIFORM):                          # given the class, the ranks are spread over [0, n_k)
        rk = [(r, n) for (r, n), c in zip(ranks, chosen) if c == k]
        assert all(0 <= r < n for r, n in rk)
        deciles = {r * 10 // n for r, n in rk}
        assert 0 in deciles and 9 in deciles, (k, sorted(deciles))


def test_without_ratios_and_without_the_uniform_event_the_rows_are_the_plain_draws():
    vols = [cref.RefClassVolume(*ref.synthetic_volume((24, 20, 28), 3, classes=5), 5)]
    base = dict(roi=(8, 8, 8), pos=2, neg=1, flip_prob=0.3, rot90_prob=0.4, scale_prob=0.5)
    for call in range(5):
        want = ref.draw(vols, [0] * 7, call, seed=9, **base)
        got = cref.draw_classes(vols, [0] * 7, call, seed=9, **base)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.int32), want[1].view(np.int32))
        everywhere = cref.draw_classes(vols, [0] * 7, call, seed=9, uniform_prob=1.0, **base)
        assert bool(np.all(everywhere[2] == cref.UNIFORM)) and np.array_equal(everywhere[0][:, 4:], want[0][:, 4:])
