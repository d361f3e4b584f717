"""The augmented-batch kernels (csrc/augment.hip, diff_unet_amos_amd/augment.py) against the CPU restatement of their contract
(tests/augment_ref.py): draw and apply bit for bit, event statistics within derived bounds, reproducibility, graph capture,
one training step fed by the producer, and the host-side argument checks."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import augment_ref as ref  # noqa: E402
from augment_ref import STATS_B, STATS_CALLS, STATS_SEED, check_event_counts, event_counts  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _aug():
    from diff_unet_amos_amd import augment
    return augment


def _pair(image, label, threshold=0.0):
    """The same case for the kernels and for the restatement."""
    return _aug().DeviceVolume(image, label, image_threshold=threshold, device=DEV), ref.RefVolume(image, label, threshold)


def _rows_all_flips_and_k(shapes, roi, ks, seed):
    """Hand-built rows: every flip combination x every k of ``ks``, volumes alternating, scale / shift zero and non-zero, starts
    at both clamped ends and in between."""
    rng = np.random.RandomState(seed)
    ints, floats = [], []
    for n, (flip, k) in enumerate((f, k) for f in range(8) for k in ks):
        vid = n % len(shapes)
        hi = [s - r for s, r in zip(shapes[vid], roi)]
        start = [0, 0, 0] if n % 4 == 0 else hi if n % 4 == 1 else [int(rng.randint(0, h + 1)) for h in hi]
        ints.append([vid, *start, flip, k])
        floats.append([0.0, 0.0] if n % 3 == 0 else [0.0731, 0.0] if n % 3 == 1 else [-0.0412, 0.0893])
    return np.array(ints, dtype=np.int32), np.array(floats, dtype=np.float32)


def _check_apply(dev_vols, ref_vols, ints, floats, roi, class_ids):
    aug = _aug()
    prod = aug.DeviceBatchProducer(dev_vols, roi=roi, class_ids=class_ids, rot90_prob=0.1 if roi[0] == roi[1] else 0.0)
    images, labels = prod.apply(aug.pack_params(ints, floats, device=DEV))
    want_images, want_labels = ref.apply(ref_vols, ints, floats, roi, class_ids)
    assert images.shape == want_images.shape and labels.shape == want_labels.shape
    assert images.is_contiguous() and labels.is_contiguous()
    bad_i = int((images.cpu() != want_images).sum()); bad_l = int((labels.cpu() != want_labels).sum())
    print(f"roi {roi}, {len(ints)} rows, {len(class_ids)} classes: {bad_i} image and {bad_l} label voxels differ")
    assert torch.equal(images.cpu(), want_images)
    assert torch.equal(labels.cpu(), want_labels)
    assert prod.status == 0


@pytest.mark.parametrize("class_ids", [tuple(range(16)), (1, 3, 7)])
def test_apply_is_bit_exact_for_every_flip_and_rotation(class_ids):
    shapes = [(70, 61, 53), (131, 97, 110)]
    pairs = [_pair(*ref.synthetic_volume(s, 10 + i)) for i, s in enumerate(shapes)]
    dev_vols, ref_vols = [p[0] for p in pairs], [p[1] for p in pairs]
    roi = (32, 32, 32)
    ints, floats = _rows_all_flips_and_k(shapes, roi, (0, 1, 2, 3), 0)
    _check_apply(dev_vols, ref_vols, ints, floats, roi, class_ids)
    roi = (32, 40, 48)                                         # not cubic: no rotation
    ints, floats = _rows_all_flips_and_k(shapes, roi, (0,), 1)
    _check_apply(dev_vols, ref_vols, ints, floats, roi, class_ids)
    roi = (8, 8, 7)                                            # roi_w not a multiple of 4: the 4-byte store form
    ints, floats = _rows_all_flips_and_k(shapes, roi, (0, 1, 2, 3), 2)
    _check_apply(dev_vols, ref_vols, ints, floats, roi, class_ids)


def test_apply_is_bit_exact_at_the_training_patch_size():
    shapes = [(131, 97, 110), (100, 96, 99)]
    pairs = [_pair(*ref.synthetic_volume(s, 20 + i)) for i, s in enumerate(shapes)]
    roi = (96, 96, 96)
    ints, floats = _rows_all_flips_and_k(shapes, roi, (0, 1, 2, 3), 3)
    for lo in range(0, len(ints), 4):                          # 4 rows (a quarter of a GB of labels) at a time
        _check_apply([p[0] for p in pairs], [p[1] for p in pairs], ints[lo:lo + 4], floats[lo:lo + 4], roi, tuple(range(16)))


def _draw_cases():
    shape = (70, 61, 53)
    cases = {kind: _pair(*ref.synthetic_volume(shape, 30 + i, kind)) for i, kind in enumerate(("both", "no_fg", "no_bg", "corner"))}
    cases["large"] = _pair(*ref.synthetic_volume((131, 97, 110), 40))       # 1 366 chunks: more than one step of the search
    return cases


def test_draw_is_bit_exact():
    aug = _aug()
    cases = _draw_cases()
    names = list(cases)
    dev_vols, ref_vols = [cases[n][0] for n in names], [cases[n][1] for n in names]
    assert dev_vols[names.index("no_fg")].fg_count == 0 and dev_vols[names.index("no_bg")].bg_count == 0
    assert (dev_vols[names.index("corner")].fg_count, dev_vols[names.index("corner")].bg_count) == (1, 0)
    for (dv, rv) in zip(dev_vols, ref_vols):
        assert (dv.fg_count, dv.bg_count) == (len(rv.fg), len(rv.bg))
    roi = (32, 32, 32)
    cfg = dict(roi=roi, pos=2, neg=1, flip_prob=0.3, rot90_prob=0.4, max_k=3, scale_prob=0.5, scale_factors=0.1, shift_prob=0.5,
               shift_offsets=0.1)
    rng = np.random.RandomState(5)
    keys = [(0, 0), (1, 0), (0, 1), (2 ** 32 + 3, 2 ** 32 + 7), (2 ** 63 + 11, 2 ** 40)]
    keys += [(int(rng.randint(0, 2 ** 31)) * 2 ** 20 + 17, int(rng.randint(0, 2 ** 31))) for _ in range(64 - len(keys))]
    bad = 0
    for n, (seed, counter) in enumerate(keys):
        prod = aug.DeviceBatchProducer(dev_vols, class_ids=range(16), seed=seed, **cfg)
        # one kind per call, then calls that mix all volumes
        ids = [n % len(names)] * 10 if n < 40 else [int(i) for i in rng.randint(0, len(names), 10)]
        got_i, got_f = aug.split_params(prod.draw(ids, counter=counter).cpu())
        want_i, want_f = ref.draw(ref_vols, ids, counter, seed=seed, **cfg)
        same = np.array_equal(got_i.numpy(), want_i) and np.array_equal(got_f.numpy().view(np.int32), want_f.view(np.int32))
        if not same:
            bad += 1
            print(f"seed {seed} counter {counter} ids {ids}:\n{got_i.numpy()}\n{want_i}\n{got_f.numpy()}\n{want_f}")
        assert prod.counter == 0                               # an overriding counter leaves the device word alone
    print(f"{len(keys)} (seed, counter) pairs x B = 10: {bad} calls differ")
    assert bad == 0
    corner = [r for r in got_i.numpy() if r[0] == names.index("corner")]
    assert all(tuple(r[1:4]) == (70 - 32, 61 - 32, 53 - 32) for r in corner)


def test_event_statistics_lie_within_the_derived_bounds():
    """N = 20 000 rows from 2 000 calls at B = 10 that advance the producer's own counter: every event count within
    N p +- 5 sqrt(N p (1 - p)) (left with probability < 1e-6 per count by a correct generator); the seed is fixed and
    tests/test_augment_ref.py checks it against the same bounds with the restatement alone."""
    aug = _aug()
    cfg = dict(ref.DEFAULTS, roi=(16, 16, 16), seed=STATS_SEED)
    image, label = ref.stats_volume()
    dv, rv = _pair(image, label)
    prod = aug.DeviceBatchProducer([dv], **cfg)
    ids = torch.zeros(STATS_B, dtype=torch.int32, device=DEV)
    rows = torch.cat([prod.draw(ids) for _ in range(STATS_CALLS)]).cpu()
    assert prod.counter == STATS_CALLS
    ints, floats = aug.split_params(rows)
    ints, floats = ints.numpy(), floats.numpy()
    assert len(ints) == 20000 and np.all((ints[:, 1] <= 3) | (ints[:, 1] >= 20))
    check_event_counts(event_counts(ints, floats, ints[:, 1] <= 3), len(ints), cfg)
    for call in (0, 1, 777, STATS_CALLS - 1):                  # and the rows are the restatement's, call by call
        want_i, want_f = ref.draw([rv], [0] * STATS_B, call, **cfg)
        assert np.array_equal(ints[call * STATS_B:(call + 1) * STATS_B], want_i)
        assert np.array_equal(floats[call * STATS_B:(call + 1) * STATS_B], want_f)


def _small_producer(seed, dev_vols):
    return _aug().DeviceBatchProducer(dev_vols, roi=(32, 32, 32), class_ids=range(16), flip_prob=0.5, rot90_prob=0.5,
                                      scale_prob=0.5, seed=seed)


def test_batches_are_reproducible_and_move_with_counter_and_seed():
    dev_vols = [_pair(*ref.synthetic_volume(s, 50 + i))[0] for i, s in enumerate([(70, 61, 53), (64, 80, 48)])]
    ids = [0, 1, 1, 0]
    a, b, c = _small_producer(3, dev_vols), _small_producer(3, dev_vols), _small_producer(4, dev_vols)
    a1, a2, b1, c1 = a.next(ids), a.next(ids), b.next(ids), c.next(ids)
    assert torch.equal(a1[0], b1[0]) and torch.equal(a1[1], b1[1])
    assert not torch.equal(a1[0], a2[0]) and not torch.equal(a1[0], c1[0])
    assert (a.counter, b.counter, c.counter) == (2, 1, 1)
    again = a.apply(a.draw(ids, counter=0))                    # replaying a logged call
    assert torch.equal(again[0], a1[0]) and torch.equal(again[1], a1[1]) and a.counter == 2


def test_next_captured_in_a_graph_moves_on_with_every_replay():
    dev_vols = [_pair(*ref.synthetic_volume(s, 60 + i))[0] for i, s in enumerate([(70, 61, 53), (64, 80, 48)])]
    ids = torch.tensor([1, 0, 1], dtype=torch.int32, device=DEV)
    eager = _small_producer(8, dev_vols)
    want = [tuple(t.clone() for t in eager.next(ids)) for _ in range(3)]
    prod = _small_producer(8, dev_vols)
    out_images = torch.zeros(3, 1, 32, 32, 32, device=DEV)
    out_labels = torch.zeros(3, 16, 32, 32, 32, device=DEV)
    graph = torch.cuda.CUDAGraph()
    stream = torch.cuda.Stream(device=DEV)
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):           # one stream: a graph without parallel branches
            prod.next(ids, out_images, out_labels)
    torch.cuda.current_stream().wait_stream(stream)
    assert prod.counter == 0                                   # capturing ran nothing
    for n in range(3):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out_images, want[n][0]) and torch.equal(out_labels, want[n][1]), n
    assert prod.counter == 3 and prod.status == 0


def test_one_training_step_fed_by_the_producer():
    """NativeConvTrainer.step on the tiny 32^3 net of tests/test_training_harness.py (its default mode: fp16 activations,
    eager): the loss from the producer's tensors equals, bit for bit, the loss of a second trainer with the same weights fed
    the restatement's tensors for the same params, noise and t."""
    from diff_unet_amos_amd.diff_unet import DiffUNet
    from diff_unet_amos_amd.training import NativeConvTrainer
    aug = _aug()
    kw = dict(in_channels=1, out_channels=2, features=(8, 8, 16, 32, 64, 8))
    pairs = [_pair(*ref.synthetic_volume(s, 70 + i, classes=3)) for i, s in enumerate([(70, 61, 53), (64, 80, 48)])]
    prod = aug.DeviceBatchProducer([p[0] for p in pairs], roi=(32, 32, 32), class_ids=(1, 2), flip_prob=0.5, rot90_prob=0.5, seed=12)
    ids = [0, 1]
    params = prod.draw(ids)
    images, labels = prod.apply(params)
    ints, floats = aug.split_params(params.cpu())
    want_images, want_labels = ref.apply([p[1] for p in pairs], ints.numpy(), floats.numpy(), (32, 32, 32), (1, 2))
    assert float(labels.sum()) > 0
    g = torch.Generator().manual_seed(3)
    noise = torch.randn(2, 2, 32, 32, 32, generator=g).to(DEV)
    t = torch.tensor([417, 80], device=DEV)
    losses = []
    for im, lb in ((images, labels), (want_images.to(DEV), want_labels.to(DEV))):
        torch.manual_seed(0)
        net = DiffUNet(**kw).to(DEV)
        losses.append(NativeConvTrainer(net, lr=1e-3).step(im, lb, noise=noise, t=t).cpu())
    print(f"loss fed by the producer {float(losses[0])!r}, fed by the restatement {float(losses[1])!r}")
    assert bool(torch.isfinite(losses[0]))
    assert torch.equal(losses[0], losses[1])


def test_bad_arguments_are_refused_on_the_host():
    aug = _aug()
    image, label = ref.synthetic_volume((40, 36, 44), 80)
    vol = aug.DeviceVolume(image, label, device=DEV)
    with pytest.raises(ValueError):                            # smaller than roi along one axis
        aug.DeviceBatchProducer([vol], roi=(32, 40, 32), rot90_prob=0.0)
    with pytest.raises(ValueError):                            # a rotation would change the patch shape
        aug.DeviceBatchProducer([vol], roi=(32, 16, 32), rot90_prob=0.1)
    aug.DeviceBatchProducer([vol], roi=(32, 16, 32), rot90_prob=0.0)
    with pytest.raises(ValueError):                            # no candidate of either kind
        aug.DeviceVolume(-image.abs() - 1.0, torch.zeros_like(label), device=DEV)
    with pytest.raises(ValueError):
        aug.DeviceBatchProducer([vol], roi=(16, 16, 16), class_ids=range(65))
    with pytest.raises(ValueError):
        aug.DeviceVolume(image.double(), label, device=DEV)
    with pytest.raises(ValueError):
        aug.DeviceVolume(image, label.to(torch.int16), device=DEV)
    with pytest.raises(ValueError):
        aug.DeviceVolume(image, label[:-1], device=DEV)
    prod = aug.DeviceBatchProducer([vol], roi=(16, 16, 16), class_ids=range(4))
    with pytest.raises(ValueError):
        prod.next([0, 1])                                      # one volume: id 1 does not exist
    params = prod.draw([0, 0], counter=0)
    with pytest.raises(AssertionError):
        prod.apply(params.cpu())
    with pytest.raises(AssertionError):
        prod.apply(params, out_images=torch.empty(2, 1, 16, 16, 16))                               # on the host
    with pytest.raises(AssertionError):
        prod.apply(params, out_labels=torch.empty(2, 4, 16, 16, 16, dtype=torch.float16, device=DEV))
    with pytest.raises(AssertionError):
        prod.apply(params, out_labels=torch.empty(2, 5, 16, 16, 16, device=DEV))                   # one channel too many
    with pytest.raises(AssertionError):
        prod.draw(torch.zeros(2, dtype=torch.int64, device=DEV))
    assert prod.counter == 0 and prod.status == 0


def test_rows_that_would_read_outside_a_volume_are_skipped_and_reported():
    """Hand-built params are outside input: a start beyond size - roi, a volume id outside the table or an odd k on a non-square
    window must neither read out of bounds nor pass silently."""
    aug = _aug()
    image, label = ref.synthetic_volume((40, 36, 44), 81)
    dv, rv = _pair(image, label)
    prod = aug.DeviceBatchProducer([dv], roi=(16, 16, 16), class_ids=range(4))
    ints = np.array([[0, 24, 20, 28, 0, 0], [0, 25, 0, 0, 0, 0], [1, 0, 0, 0, 0, 0], [0, 0, 0, -1, 0, 0], [0, 0, 0, 0, 8, 0],
                     [0, 0, 0, 0, 0, 4]], dtype=np.int32)
    floats = np.zeros((6, 2), dtype=np.float32)
    out_images = torch.full((6, 1, 16, 16, 16), -7.0, device=DEV)
    out_labels = torch.full((6, 4, 16, 16, 16), -7.0, device=DEV)
    prod.apply(aug.pack_params(ints, floats, device=DEV), out_images, out_labels)
    want_images, want_labels = ref.apply([rv], ints[:1], floats[:1], (16, 16, 16), range(4))
    assert torch.equal(out_images[:1].cpu(), want_images) and torch.equal(out_labels[:1].cpu(), want_labels)
    assert bool((out_images[1:] == -7.0).all()) and bool((out_labels[1:] == -7.0).all())
    assert prod.status == 1
