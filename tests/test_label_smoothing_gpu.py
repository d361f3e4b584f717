"""Centroid-distance label smoothing on the device (csrc/augment.hip: dua_aug_class_centroids, dua_aug_apply_smoothed;
augment.DeviceVolume(num_classes=...), augment.DeviceBatchProducer(smoothing=...)) against the fp64 restatement
tests/label_smoothing_ref.py and the reference's own outputs (tests/golden/label_smoothing_golden.npz).  Integer results are
compared exactly, the smoothed field within the derived bound of the restatement's docstring, on every element."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import augment_ref as ref  # noqa: E402
import label_smoothing_ref as lsr  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "label_smoothing_golden.npz")


def _aug():
    from diff_unet_amos_amd import augment
    return augment


def _case(shape, seed, K, absent=(), one_voxel=None):
    """A seeded volume with ids in [0, K); ``absent`` classes removed, ``one_voxel`` = (class, index): that class at one voxel."""
    image, label = ref.synthetic_volume(shape, seed, classes=K)
    for k in absent:
        label[label == k] = 0
    if one_voxel is not None:
        k, at = one_voxel
        label[label == k] = 0
        label[at] = k
    return image, label.contiguous()


def _pair(image, label, K):
    return _aug().DeviceVolume(image, label, device=DEV, num_classes=K), ref.RefVolume(image, label)


def _rows(shapes, roi, ks, seed):
    """Hand-built rows: every flip combination x every k of ``ks``, volumes alternating, crops at both clamped ends (they touch
    every face of the volume) and in between, scale / shift zero and non-zero."""
    rng = np.random.RandomState(seed)
    ints, floats = [], []
    for n, (flip, k) in enumerate((f, k) for f in range(8) for k in ks):
        vid = n % len(shapes)
        hi = [s - r for s, r in zip(shapes[vid], roi)]
        start = [0, 0, 0] if n % 4 == 0 else hi if n % 4 == 1 else [int(rng.randint(0, h + 1)) for h in hi]
        ints.append([vid, *start, flip, k])
        floats.append([0.0, 0.0] if n % 3 == 0 else [0.0731, 0.0] if n % 3 == 1 else [-0.0412, 0.0893])
    return np.array(ints, dtype=np.int32), np.array(floats, dtype=np.float32)


def _check_rows(dev_vols, ref_vols, ints, floats, roi, class_ids, K, what, **smoothing):
    """Device batch against the restatement, row by row: the bound's delta_c is that of the row's volume."""
    aug = _aug()
    prod = aug.DeviceBatchProducer(dev_vols, roi=roi, class_ids=class_ids, rot90_prob=0.1 if roi[0] == roi[1] else 0.0,
                                   smoothing=aug.LabelSmoothing(**smoothing))
    worst = 0.0
    for lo in range(0, len(ints), 8):
        images, labels = prod.apply(aug.pack_params(ints[lo:lo + 8], floats[lo:lo + 8], device=DEV))
        want_images, want, dist = lsr.apply(ref_vols, ints[lo:lo + 8], floats[lo:lo + 8], roi, class_ids, K, **smoothing)
        assert labels.is_contiguous() and tuple(labels.shape) == want.shape
        assert torch.equal(images.cpu(), want_images)                        # the image path is today's, bit for bit
        got = labels.cpu().numpy()
        for b, row in enumerate(ints[lo:lo + 8]):
            tol = lsr.tolerance(dist[b], want[b], smoothing.get("alpha", 0.3), smoothing.get("order", 1.0),
                                smoothing.get("epsilon", 1e-6), lsr.delta_c_device(ref_vols[row[0]].shape))
            assert np.isfinite(tol).all()
            ratio, at = lsr.worst_ratio(got[b], want[b], tol)
            worst = max(worst, ratio)
            assert ratio <= 1.0, (what, row.tolist(), at, got[b][at], want[b][at], tol[at])
    print(f"{what}: roi {roi}, {len(ints)} rows, {len(class_ids)} channels: worst |error| / tol = {worst:.3g}")
    assert prod.status == 0
    return worst


def test_centroids_counts_and_sums_are_exact():
    """Counts and index sums equal integer arithmetic on the host; centroids equal the fp64 quotient rounded once to fp32; an
    absent class gives zeros, a class of one voxel its index.  The large volume is more than one pass of the grid (2 048 blocks
    x 4 096 voxels) and not a multiple of 16 voxels; two runs agree bit for bit."""
    aug = _aug()
    cases = [((70, 61, 53), 16, (5, 15), (9, (41, 7, 50))), ((211, 199, 205), 14, (13,), (3, (0, 0, 0))), ((5, 3, 2), 3, (), None)]
    for n, (shape, K, absent, one) in enumerate(cases):
        image, label = _case(shape, 100 + n, K, absent, one)
        if shape == (5, 3, 2):
            image = image.abs() + 0.1
        dv = aug.DeviceVolume(image, label, device=DEV, num_classes=K)
        counts, sums = lsr.class_sums(label.numpy(), K)
        assert np.array_equal(dv.class_counts.cpu().numpy(), counts), (shape, dv.class_counts.tolist(), counts.tolist())
        assert np.array_equal(dv.class_sums.cpu().numpy(), sums), shape
        want = np.zeros((K, 3), dtype=np.float32)
        want[counts > 0] = (sums[counts > 0].astype(np.float64) / counts[counts > 0, None].astype(np.float64)).astype(np.float32)
        got = dv.centroids.cpu().numpy()
        assert got.dtype == np.float32 and np.array_equal(got.view(np.int32), want.view(np.int32)), (shape, got, want)
        for k in absent:
            assert counts[k] == 0 and not got[k].any()
        if one is not None:
            assert counts[one[0]] == 1 and tuple(got[one[0]]) == tuple(float(i) for i in one[1])
        again = aug.DeviceVolume(image, label, device=DEV, num_classes=K)
        assert torch.equal(again.centroids, dv.centroids) and torch.equal(again.class_sums, dv.class_sums)
        print(f"{shape}, K = {K}: counts {counts.tolist()}")


def test_constructor_checks():
    aug = _aug()
    image, label = _case((40, 36, 44), 110, 16)
    with pytest.raises(ValueError, match="num_classes"):                     # the map holds ids up to 15
        aug.DeviceVolume(image, label, device=DEV, num_classes=10)
    plain = aug.DeviceVolume(image, label, device=DEV)
    assert plain.centroids is None and plain.num_classes is None
    with pytest.raises(ValueError, match="centroids"):
        aug.DeviceBatchProducer([plain], roi=(16, 16, 16), smoothing=aug.LabelSmoothing())
    v16 = aug.DeviceVolume(image, label, device=DEV, num_classes=16)
    with pytest.raises(ValueError, match="centroids"):                       # one of two volumes without
        aug.DeviceBatchProducer([v16, plain], roi=(16, 16, 16), smoothing=aug.LabelSmoothing())
    with pytest.raises(ValueError, match="one num_classes"):
        aug.DeviceBatchProducer([v16, aug.DeviceVolume(image, label, device=DEV, num_classes=20)], roi=(16, 16, 16),
                                smoothing=aug.LabelSmoothing())
    with pytest.raises(ValueError, match="no centroid"):                     # class_ids defaults to range(16); 16 has no row
        aug.DeviceBatchProducer([v16], roi=(16, 16, 16), class_ids=range(1, 17), smoothing=aug.LabelSmoothing())
    with pytest.raises(ValueError):
        aug.DeviceBatchProducer([v16], roi=(16, 16, 16), smoothing=dict(alpha=0.3))
    aug.DeviceBatchProducer([v16], roi=(16, 16, 16), smoothing=aug.LabelSmoothing())
    aug.DeviceBatchProducer([v16], roi=(16, 16, 16))                         # centroids present, smoothing off: allowed


def test_smoothed_apply_matches_the_restatement_for_every_flip_and_rotation():
    """Two non-cubic volumes of different extents in one batch; volume 0 has an absent class (centroid at the origin, which
    the crops at start 0 contain) and a class of one voxel in the far corner region (the crops at the far end contain it:
    3e5 there); every flip x k = 0..3 on cubic and on roi[0] == roi[1] != roi[2] windows, flips alone on a window without
    equal extents, and the 4-byte store form (roi_w = 7)."""
    K = 16
    shapes = [(70, 61, 53), (131, 97, 110)]
    cases = [_case(shapes[0], 120, K, absent=(5,), one_voxel=(9, (66, 57, 50))), _case(shapes[1], 121, K)]
    pairs = [_pair(image, label, K) for image, label in cases]
    dev_vols, ref_vols = [p[0] for p in pairs], [p[1] for p in pairs]
    ids = tuple(range(1, K))                                                 # the reference's labels[:, 1:]
    for roi, ks, seed in (((32, 32, 32), (0, 1, 2, 3), 0), ((24, 24, 40), (0, 1, 2, 3), 1), ((32, 40, 48), (0,), 2),
                          ((8, 8, 7), (0, 1, 2, 3), 3)):
        ints, floats = _rows(shapes, roi, ks, seed)
        _check_rows(dev_vols, ref_vols, ints, floats, roi, ids, K, "defaults")
    ints, floats = _rows(shapes, (24, 24, 40), (0, 1, 2, 3), 4)
    _check_rows(dev_vols, ref_vols, ints, floats, (24, 24, 40), (0, 5, 9, 15), K, "order 2", alpha=0.5, order=2.0, epsilon=1e-3)
    _check_rows(dev_vols, ref_vols, ints[:8], floats[:8], (24, 24, 40), (0, 9), K, "order 1.5", alpha=0.2, order=1.5)
    _check_rows(dev_vols, ref_vols, ints[:8], floats[:8], (8, 8, 7), (0, 9), K, "order 1.5, narrow", alpha=0.2, order=1.5)


def test_whole_volume_patch_equals_the_reference_golden():
    """The patch is the whole volume, no flip, no rotation: the device output is the reference's smoothed label for the case,
    within the bound with the reference's own centroid discrepancy added; every case, every element."""
    aug = _aug()
    gold = np.load(GOLDEN)
    for name in gold["cases"].tolist():
        labels = torch.from_numpy(gold[f"{name}_labels"])
        K = int(gold[f"{name}_K"])
        kw = dict(alpha=float(gold[f"{name}_alpha"]), order=float(gold[f"{name}_order"]), epsilon=float(gold[f"{name}_epsilon"]))
        g = torch.Generator().manual_seed(7)
        image = torch.rand(labels.shape, generator=g) + 0.1
        dv = aug.DeviceVolume(image, labels, device=DEV, num_classes=K)
        roi = tuple(labels.shape)
        prod = aug.DeviceBatchProducer([dv], roi=roi, class_ids=range(K), rot90_prob=0.0, smoothing=aug.LabelSmoothing(**kw))
        images, got = prod.apply(aug.pack_params([[0, 0, 0, 0, 0, 0]], [[0.0, 0.0]], device=DEV))
        assert torch.equal(images[0, 0].cpu(), image) and prod.status == 0
        want = gold[f"{name}_out"].astype(np.float64)
        _, dist = lsr.field(labels.numpy(), K, **kw)
        tol = lsr.tolerance(dist, want, kw["alpha"], kw["order"], kw["epsilon"],
                            float(gold[f"{name}_centroid_gap"]) + lsr.delta_c_device(roi))
        assert np.isfinite(tol).all()
        ratio, at = lsr.worst_ratio(got[0].cpu().numpy(), want, tol)
        print(f"{name}: extents {roi}, K = {K}, max {want.max():.6g}: worst |device - reference| / tol = {ratio:.3g} at {at}")
        assert ratio <= 1.0, (name, at, float(got[0][at]), want[at], tol[at])


def _small_volumes(K=16):
    cases = [_case((70, 61, 53), 130, K, one_voxel=(9, (20, 30, 25))), _case((64, 80, 48), 131, K, absent=(3,))]
    return [_aug().DeviceVolume(image, label, device=DEV, num_classes=K) for image, label in cases]


def _producer(vols, seed, smoothing, class_ids=range(1, 16)):
    return _aug().DeviceBatchProducer(vols, roi=(32, 32, 32), class_ids=class_ids, flip_prob=0.5, rot90_prob=0.5, scale_prob=0.5,
                                      seed=seed, smoothing=smoothing)


def test_alpha_zero_and_no_smoothing_give_the_one_hot_bits(monkeypatch):
    """alpha = 0 writes bit for bit what the one-hot apply writes; smoothing=None is the one-hot producer itself: one draw and
    one one-hot apply per ``next``, never the smoothed entry point, and the bits of the restatement of the one-hot contract."""
    aug = _aug()
    from diff_unet_amos_amd import ops
    vols = _small_volumes()
    ids = [0, 1, 1, 0, 0, 1]
    plain, zero = _producer(vols, 5, None), _producer(vols, 5, aug.LabelSmoothing(alpha=0.0))
    params = plain.draw(ids, counter=3)
    assert torch.equal(params, zero.draw(ids, counter=3))
    a, b = plain.apply(params), zero.apply(params)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
    for order in (2.0, 0.5):
        c = _producer(vols, 5, aug.LabelSmoothing(alpha=0.0, order=order)).apply(params)
        assert torch.equal(a[1].view(torch.int32), c[1].view(torch.int32))
    calls = {"aug_draw": 0, "aug_apply": 0, "aug_apply_smoothed": 0}         # aug_apply without / with smoothing passed
    for name in ("aug_draw", "aug_apply"):
        def counted(*args, _f=getattr(ops, name), _n=name, **kw):
            calls[_n + "_smoothed" if kw.get("smoothing") is not None else _n] += 1
            return _f(*args, **kw)
        monkeypatch.setattr(ops, name, counted)
    images, labels = plain.next(ids)
    assert calls == {"aug_draw": 1, "aug_apply": 1, "aug_apply_smoothed": 0}
    ints, floats = aug.split_params(plain.draw(ids, counter=0).cpu())
    ref_vols = [ref.RefVolume(v.image.cpu(), v.label.cpu()) for v in vols]
    want = ref.apply(ref_vols, ints.numpy(), floats.numpy(), (32, 32, 32), range(1, 16))
    assert torch.equal(images.cpu(), want[0]) and torch.equal(labels.cpu(), want[1])
    smooth = _producer(vols, 5, aug.LabelSmoothing())
    smooth.next(ids)
    assert calls == {"aug_draw": 3, "aug_apply": 1, "aug_apply_smoothed": 1}


def test_max_value_clamps_and_only_clamps_and_runs_repeat_bit_for_bit():
    aug = _aug()
    vols = _small_volumes()
    free, capped = _producer(vols, 6, aug.LabelSmoothing()), _producer(vols, 6, aug.LabelSmoothing(max_value=2.0))
    ints = np.array([[0, 4, 14, 9, 3, 1], [1, 0, 0, 0, 0, 0], [0, 0, 10, 20, 6, 2]], dtype=np.int32)   # rows 0, 2 hold voxel (20, 30, 25)
    params = aug.pack_params(ints, np.zeros((3, 2), dtype=np.float32), device=DEV)
    a, b = free.apply(params), capped.apply(params)
    assert float(a[1].max()) > 1e5 and int((a[1] > 2.0).sum()) > 2          # the one-voxel class, and neighbours of centroids
    assert torch.equal(a[0], b[0]) and torch.equal(b[1], torch.clamp(a[1], max=2.0))
    again = free.apply(params)
    assert torch.equal(a[1].view(torch.int32), again[1].view(torch.int32)) and torch.equal(a[0], again[0])
    assert free.status == 0 and capped.status == 0


def test_smoothed_next_captured_in_a_graph_moves_on_with_every_replay():
    aug = _aug()
    vols = _small_volumes()
    ids = torch.tensor([1, 0, 1], dtype=torch.int32, device=DEV)
    eager = _producer(vols, 8, aug.LabelSmoothing())
    want = [tuple(t.clone() for t in eager.next(ids)) for _ in range(3)]
    assert not torch.equal(want[0][1], want[1][1]) and not torch.equal(want[1][1], want[2][1])
    prod = _producer(vols, 8, aug.LabelSmoothing())
    out_images = torch.zeros(3, 1, 32, 32, 32, device=DEV)
    out_labels = torch.zeros(3, 15, 32, 32, 32, device=DEV)
    graph = torch.cuda.CUDAGraph()
    stream = torch.cuda.Stream(device=DEV)
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):           # one stream: a graph without parallel branches
            prod.next(ids, out_images, out_labels)
    torch.cuda.current_stream().wait_stream(stream)
    assert prod.counter == 0
    for n in range(3):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out_images, want[n][0]) and torch.equal(out_labels.view(torch.int32), want[n][1].view(torch.int32)), n
    assert prod.counter == 3 and prod.status == 0
    logged = prod.apply(prod.draw(ids, counter=1))                           # a logged row reproduces the smoothed batch
    assert torch.equal(logged[1].view(torch.int32), want[1][1].view(torch.int32))


def test_rows_outside_a_volume_are_skipped_in_the_smoothed_form_too():
    aug = _aug()
    image, label = _case((40, 36, 44), 140, 4)
    dv = aug.DeviceVolume(image, label, device=DEV, num_classes=4)
    prod = aug.DeviceBatchProducer([dv], roi=(16, 16, 16), class_ids=range(4), smoothing=aug.LabelSmoothing())
    ints = np.array([[0, 24, 20, 28, 0, 0], [0, 25, 0, 0, 0, 0], [1, 0, 0, 0, 0, 0], [0, 0, 0, -1, 0, 0], [0, 0, 0, 0, 8, 0],
                     [0, 0, 0, 0, 0, 4]], dtype=np.int32)
    out_images = torch.full((6, 1, 16, 16, 16), -7.0, device=DEV)
    out_labels = torch.full((6, 4, 16, 16, 16), -7.0, device=DEV)
    prod.apply(aug.pack_params(ints, np.zeros((6, 2), dtype=np.float32), device=DEV), out_images, out_labels)
    assert bool((out_labels[0] >= 0).all()) and bool((out_images[1:] == -7.0).all()) and bool((out_labels[1:] == -7.0).all())
    assert prod.status == 1


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_one_trainer_step_on_a_smoothed_batch_matches_the_oracle(dtype):
    """The first soft-label run of the fused loss: one eager NativeConvTrainer.step on a smoothed batch against
    oracle/train_ref.py on the same tensors, with the tolerances tests/test_training_harness.py uses for hard labels (loss:
    1e-5 relative in fp32, test_native_trainer_other_loss_configuration; 2e-3 in fp16, test_full_size_gradients_fp16_path_vs_oracle;
    gradients: worst max-relative < 2e-3 in fp32, relative L2 < 5e-2 and cosine > 0.9 in fp16,
    test_native_conv_training_path_matches_oracle_autograd).  The volume keeps every voxel at least 0.05 from every centroid
    in use, so labels stay below 7 (asserted: otherwise the comparison says nothing about the loss kernels)."""
    from diff_unet_amos_amd.diff_unet import DiffUNet
    from diff_unet_amos_amd.training import NativeConvTrainer
    from oracle.train_ref import RefLoss, ref_training_step
    from oracle.unet_ref import RefDiffUNet
    aug = _aug()
    kw = dict(in_channels=1, out_channels=2, features=(8, 8, 16, 32, 64, 8))
    cases = [_case(s, 150 + i, 3) for i, s in enumerate([(70, 61, 53), (64, 80, 48)])]
    vols = [aug.DeviceVolume(image, label, device=DEV, num_classes=3) for image, label in cases]
    prod = aug.DeviceBatchProducer(vols, roi=(32, 32, 32), class_ids=(1, 2), flip_prob=0.5, rot90_prob=0.5, seed=12,
                                   smoothing=aug.LabelSmoothing())
    params = prod.draw([0, 1])
    images, labels = prod.apply(params)
    ints, floats = aug.split_params(params.cpu())
    ref_vols = [ref.RefVolume(image, label) for image, label in cases]
    _, want_labels, dist = lsr.apply(ref_vols, ints.numpy(), floats.numpy(), (32, 32, 32), (1, 2), 3)
    assert dist.min() >= 0.05 and float(labels.max()) < 7.0, (dist.min(), float(labels.max()))
    assert float((labels - torch.round(labels)).abs().max()) > 0.01          # soft labels indeed
    g = torch.Generator().manual_seed(3)
    noise = torch.randn(2, 2, 32, 32, 32, generator=g)
    t = torch.tensor([417, 80])
    torch.manual_seed(0)
    oracle = RefDiffUNet(**kw)
    net = DiffUNet(**kw)
    net.load_state_dict(oracle.state_dict())
    net = net.to(DEV)
    want = ref_training_step(oracle, images.cpu(), labels.cpu(), RefLoss(), noise, t)
    want.backward()
    got = float(NativeConvTrainer(net, lr=0.0, weight_decay=0.0, dtype=dtype).step(images, labels, noise=noise.to(DEV), t=t.to(DEV)))
    want = float(want)
    gp = dict(net.named_parameters())
    errs, coss, num, den = [], [], 0.0, 0.0
    for k, p in oracle.named_parameters():
        if k.endswith(".conv.bias"):                                         # bias before InstanceNorm: the true gradient is zero
            continue
        a, b = gp[k].grad.detach().cpu().double(), p.grad.double()
        errs.append(((a - b).abs().max().item() / (b.abs().max().item() + 1e-6), k))
        num += float(((a - b) ** 2).sum()); den += float((b ** 2).sum())
        if b.numel() >= 64:
            coss.append((float((a * b).sum() / (a.norm() * b.norm() + 1e-30)), k))
    errs.sort(reverse=True); coss.sort()
    rel_l2 = (num / den) ** 0.5
    print(f"[{dtype}] loss {got!r} vs oracle {want!r} (relative {abs(got - want) / abs(want):.2e}); labels up to "
          f"{float(labels.max()):.3f}; whole-gradient relative L2 error {rel_l2:.2e}; worst max-relative {errs[0][1]} {errs[0][0]:.2e}; "
          f"lowest cosine {coss[0][1]} {coss[0][0]:.4f}")
    assert np.isfinite(got)
    if dtype == torch.float32:
        assert abs(got - want) < 1e-5 * max(1.0, abs(want)), (got, want)
        assert errs[0][0] < 2e-3, errs[0]
    else:
        assert abs(got - want) < 2e-3 * abs(want), (got, want)
        assert rel_l2 < 5e-2 and coss[0][0] > 0.9, (rel_l2, coss[0])
