"""Random rotation and zoom in the device batch producer (dua_aug_draw_affine, dua_aug_apply_affine; csrc/augment.hip) against
the CPU restatement of their contract (tests/augment_affine_ref.py): the draw bit for bit, labels bit for bit, images within
the bound derived there, identity rows equal to the plain and the smoothed apply, smoothing composed within the bound of
tests/label_smoothing_ref.py, event statistics, graph capture, skipped rows and the argument checks."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import augment_affine_ref as aref  # noqa: E402
import augment_ref as ref  # noqa: E402
import label_smoothing_ref as lsref  # noqa: E402

gpu = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(40, 36, 44), (33, 47, 38)]
ROI = (16, 16, 16)
BASE = dict(roi=ROI, pos=2, neg=1, flip_prob=0.3, rot90_prob=0.4, max_k=3, scale_prob=0.5, scale_factors=0.1, shift_prob=0.5,
            shift_offsets=0.1)


def _aug():
    from diff_unet_amos_amd import augment
    return augment


def _pairs(volumes, num_classes=None):
    """The same cases for the kernels and for the restatement."""
    dev = [_aug().DeviceVolume(image, label, device=DEV, num_classes=num_classes) for image, label in volumes]
    return dev, [ref.RefVolume(image, label) for image, label in volumes]


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


@gpu
@pytest.mark.parametrize("rotate_prob,zoom_prob,calls", [(0.5, 0.5, 200), (0.0, 1.0, 20), (1.0, 0.0, 20)])
def test_draw_keeps_the_params_bits_and_gives_the_restatements_affine_rows(rotate_prob, zoom_prob, calls):
    aug = _aug()
    dev_vols, _ = _pairs([ref.synthetic_volume(s, 30 + i) for i, s in enumerate(SHAPES)])
    acfg = dict(aref.STATS_AFFINE, rotate_prob=rotate_prob, zoom_prob=zoom_prob)
    seed, B = 2 ** 40 + 77, 10
    plain = aug.DeviceBatchProducer(dev_vols, class_ids=range(4), seed=seed, **BASE)
    turned = aug.DeviceBatchProducer(dev_vols, class_ids=range(4), seed=seed, **BASE, **acfg)
    ids = torch.tensor([i % 2 for i in range(B)], dtype=torch.int32, device=DEV)
    want_params = torch.cat([plain.draw(ids) for _ in range(calls)])
    drawn = [turned.draw(ids) for _ in range(calls)]
    got_params, got_rows = torch.cat([d[0] for d in drawn]), torch.cat([d[1] for d in drawn]).cpu().numpy()
    assert plain.counter == turned.counter == calls and turned.status == 0
    assert torch.equal(got_params, want_params)                # dua_aug_draw's bits for the same seed and counter
    want_rows = np.concatenate([aref.affine_rows(B, call, seed, **acfg) for call in range(calls)])
    differ = int(np.sum(np.any(_bits(got_rows) != _bits(want_rows), axis=1)))
    print(f"{calls} calls x B = {B} at probabilities ({rotate_prob}, {zoom_prob}): {differ} affine rows differ from the restatement")
    assert differ == 0
    counts = aref.affine_event_counts(got_rows)
    if rotate_prob in (0.0, 1.0):
        assert counts == {"rotation": int(rotate_prob) * calls * B, "zoom": int(zoom_prob) * calls * B}
    # an overriding counter reproduces a logged call and leaves the device word alone
    params, rows = turned.draw(ids, counter=7)
    assert torch.equal(params, want_params[70:80]) and np.array_equal(_bits(rows.cpu().numpy()), _bits(want_rows[70:80]))
    assert turned.counter == calls
    m, t, z, events, pad = aug.split_affine(rows.cpu())
    assert m.shape == (B, 3, 3) and t.shape == (B, 3) and events.dtype == torch.int32
    assert np.array_equal(events.numpy(), _bits(want_rows[70:80])[:, aref.A_EVENTS]) and bool((pad == -1.25).all())


@pytest.fixture(scope="module")
def apply_cases():
    """name -> (case, RefVolumes, the fp64 batch of the restatement): computed once, shared by the tests, left unchanged."""
    out = {}
    for name, case in aref.apply_cases().items():
        volumes = aref.case_volumes(case)
        vols = [ref.RefVolume(image, label) for image, label in volumes]
        out[name] = (case, volumes, vols, aref.apply(vols, case["ints"], case["floats"], case["rows"], case["roi"], case["class_ids"]))
    return out


@gpu
@pytest.mark.parametrize("name", ["cube16", "narrow_4_byte_stores", "oblong_k0", "volume_of_roi_size"])
def test_apply_labels_bit_for_bit_and_images_within_the_derived_bound(apply_cases, name):
    aug = _aug()
    case, volumes, ref_vols, want = apply_cases[name]
    dev_vols, _ = _pairs(volumes)
    roi = case["roi"]
    prod = aug.DeviceBatchProducer(dev_vols, roi=roi, class_ids=case["class_ids"], rot90_prob=0.0)
    params = aug.pack_params(case["ints"], case["floats"], device=DEV)
    images, labels = prod.apply(params, affine=torch.from_numpy(case["rows"]).to(DEV))
    assert images.is_contiguous() and labels.is_contiguous() and prod.status == 0
    bound = aref.row_bounds(ref_vols, case["ints"], case["floats"], case["rows"])
    ratio, at = aref.worst_ratio(images.cpu().numpy(), want[0], bound)
    bad = int((labels.cpu().numpy() != want[1]).sum())
    print(f"{name}: roi {roi}, {len(case['ints'])} rows: max |device - fp64| / bound = {ratio:.3f} at {at} "
          f"(bound {bound.min():.3e} .. {bound.max():.3e}); {bad} label voxels differ")
    assert bad == 0
    assert ratio <= 1.0


@gpu
@pytest.mark.parametrize("name", ["cube16", "narrow_4_byte_stores"])
def test_identity_rows_give_the_bits_of_the_plain_and_of_the_smoothed_apply(apply_cases, name):
    aug = _aug()
    case, volumes, _, _ = apply_cases[name]
    dev_vols, _ = _pairs(volumes, num_classes=16)
    params = aug.pack_params(case["ints"], case["floats"], device=DEV)
    rows = torch.from_numpy(aref.identity_rows(len(case["ints"]), pad_value=-3.5)).to(DEV)
    for smoothing in (None, aug.LabelSmoothing(), aug.LabelSmoothing(order=1.5, max_value=50.0)):
        prod = aug.DeviceBatchProducer(dev_vols, roi=case["roi"], class_ids=case["class_ids"], smoothing=smoothing)
        plain, resampled = prod.apply(params), prod.apply(params, affine=rows)
        assert torch.equal(plain[0], resampled[0]), smoothing
        assert torch.equal(plain[1], resampled[1]), smoothing
        assert prod.status == 0


@gpu
@pytest.mark.parametrize("order", [1.0, 1.5])
def test_smoothing_composed_with_the_resampling_stays_within_its_bound(apply_cases, order):
    """The smoothed channels at the nearest index j, voxels whose j lies outside the volume included: j is exact, so the bound
    tests/label_smoothing_ref.py derives for the plain apply holds as it stands."""
    aug = _aug()
    K, alpha, eps = 16, 0.3, 1e-6
    for name in ("cube16", "narrow_4_byte_stores", "volume_of_roi_size"):
        case, volumes, ref_vols, want = apply_cases[name]
        dev_vols, _ = _pairs(volumes, num_classes=K)
        ids = list(case["class_ids"])
        prod = aug.DeviceBatchProducer(dev_vols, roi=case["roi"], class_ids=ids, smoothing=aug.LabelSmoothing(alpha, order, eps))
        params = aug.pack_params(case["ints"], case["floats"], device=DEV)
        images, labels = prod.apply(params, affine=torch.from_numpy(case["rows"]).to(DEV))
        onehot, j = want[1].astype(np.float64), want[3].astype(np.float64)
        cents = [lsref.centroids(v.label.numpy(), K) for v in ref_vols]
        dist = np.empty(onehot.shape, dtype=np.float64)
        for b, r in enumerate(case["ints"].tolist()):
            c = cents[r[0]][ids]
            dist[b] = np.sqrt(sum((j[b, ax][None] - c[:, ax].reshape(-1, 1, 1, 1)) ** 2 for ax in range(3)))
        expect = lsref.smooth(onehot, dist, alpha, order, eps)
        delta_c = np.array([lsref.delta_c_device(ref_vols[r[0]].shape) for r in case["ints"].tolist()]).reshape(-1, 1, 1, 1, 1)
        tol = lsref.tolerance(dist, expect, alpha, order, eps, delta_c)
        ratio, at = lsref.worst_ratio(labels.cpu().numpy(), expect, tol)
        outside = np.any([(j[:, a] < 0) | (j[:, a] >= np.array([ref_vols[r[0]].shape[a] for r in case["ints"]]).reshape(-1, 1, 1, 1))
                          for a in range(3)], axis=0)
        print(f"{name}, order {order}: max |device - fp64| / tolerance = {ratio:.3f} at {at}; {int(outside.sum())} voxels have j outside")
        assert ratio <= 1.0 and int(outside.sum()) > 0
        ibound = aref.row_bounds(ref_vols, case["ints"], case["floats"], case["rows"])
        assert aref.worst_ratio(images.cpu().numpy(), want[0], ibound)[0] <= 1.0
        assert prod.status == 0


@gpu
def test_event_statistics_and_ranges_over_twenty_thousand_rows():
    """2 000 calls x 10 samples that advance the producer's own counter: rotation and zoom counts within n p +- 5 sqrt(n p (1 -
    p)), every t within +-rotate_tan_half, every z within the zoom range; tests/test_augment_affine_ref.py checks the same seed
    with the restatement alone."""
    aug = _aug()
    dev_vols, _ = _pairs([ref.stats_volume()])
    prod = aug.DeviceBatchProducer(dev_vols, roi=ROI, class_ids=range(4), seed=aref.STATS_SEED, **aref.STATS_AFFINE)
    ids = torch.zeros(aref.STATS_B, dtype=torch.int32, device=DEV)
    rows = torch.cat([prod.draw(ids)[1] for _ in range(aref.STATS_CALLS)]).cpu().numpy()
    assert prod.counter == aref.STATS_CALLS and len(rows) == 20000
    aref.check_affine_statistics(rows, aref.STATS_AFFINE)
    for call in (0, 1, 777, aref.STATS_CALLS - 1):             # and the rows are the restatement's, call by call
        want = aref.affine_rows(aref.STATS_B, call, aref.STATS_SEED, **aref.STATS_AFFINE)
        assert np.array_equal(_bits(rows[call * aref.STATS_B:(call + 1) * aref.STATS_B]), _bits(want)), call


@gpu
def test_next_captured_in_a_graph_gives_the_restatements_batches_replay_by_replay():
    aug = _aug()
    volumes = [ref.synthetic_volume(s, 60 + i) for i, s in enumerate(SHAPES)]
    dev_vols, ref_vols = _pairs(volumes)
    acfg = dict(rotate_prob=0.7, rotate_range=(0.5, 0.3, 0.4), zoom_prob=0.7, zoom_range=(0.8, 1.25), pad_value=-0.5)
    cfg = dict(BASE, seed=8)
    class_ids, vid = (0, 2, 5), [1, 0, 1]
    prod = aug.DeviceBatchProducer(dev_vols, class_ids=class_ids, **cfg, **acfg)
    ids = torch.tensor(vid, dtype=torch.int32, device=DEV)
    first = prod.next(ids)                                     # an eager call first: the capture starts at counter c = 1
    assert first[0].shape == (3, 1) + ROI and prod.counter == 1
    out_images = torch.zeros((3, 1) + ROI, device=DEV)
    out_labels = torch.zeros((3, len(class_ids)) + ROI, device=DEV)
    graph = torch.cuda.CUDAGraph()
    stream = torch.cuda.Stream(device=DEV)
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):           # one stream: a graph without parallel branches
            prod.next(ids, out_images, out_labels)
    torch.cuda.current_stream().wait_stream(stream)
    assert prod.counter == 1                                   # capturing ran nothing
    for counter in (1, 2):
        graph.replay()
        torch.cuda.synchronize()
        ints, floats, rows = aref.draw(ref_vols, vid, counter, **cfg, **acfg)
        want = aref.apply(ref_vols, ints, floats, rows, ROI, class_ids)
        ratio, _ = aref.worst_ratio(out_images.cpu().numpy(), want[0], aref.row_bounds(ref_vols, ints, floats, rows))
        print(f"replay at counter {counter}: events {rows[:, aref.A_EVENTS].copy().view(np.int32).tolist()}, "
              f"max |device - fp64| / bound = {ratio:.3f}")
        assert np.array_equal(out_labels.cpu().numpy(), want[1]) and ratio <= 1.0
    assert prod.counter == 3 and prod.status == 0


@gpu
def test_rows_that_must_be_skipped_set_status_and_leave_their_outputs():
    """The rows dua_aug_apply skips are skipped here too; a matrix that reads far outside the volume is not one of them."""
    aug = _aug()
    volumes = [ref.synthetic_volume(SHAPES[0], 81)]
    dev_vols, ref_vols = _pairs(volumes)
    prod = aug.DeviceBatchProducer(dev_vols, roi=ROI, class_ids=range(4), rotate_prob=0.5, rotate_range=(0.3, 0.3, 0.3))
    ints = np.array([[0, 24, 20, 28, 0, 0], [0, 25, 0, 0, 0, 0], [1, 0, 0, 0, 0, 0], [0, 0, 0, -1, 0, 0], [0, 0, 0, 0, 8, 0],
                     [0, 0, 0, 0, 0, 4], [0, 3, 2, 1, 0, 0]], dtype=np.int32)
    floats = np.zeros((7, 2), dtype=np.float32)
    rows = np.stack([aref.row((0.2, -0.1, 0.05), 0.9, 3, 1.5)] * 6 + [aref.row((0.0, 0.0, 0.0), 0.01, 2, 1.5)])     # the last: far outside
    out_images = torch.full((7, 1) + ROI, -7.0, device=DEV)
    out_labels = torch.full((7, 4) + ROI, -7.0, device=DEV)
    params = aug.pack_params(ints, floats, device=DEV)
    with pytest.raises(ValueError):
        prod.apply(params, out_images, out_labels)             # a producer that rotates refuses a missing affine
    assert prod.status == 0
    prod.apply(params, out_images, out_labels, affine=torch.from_numpy(rows).to(DEV))
    keep = [0, 6]
    want = aref.apply(ref_vols, ints[keep], floats[keep], rows[keep], ROI, range(4))
    got_images, got_labels = out_images.cpu().numpy(), out_labels.cpu().numpy()
    assert aref.worst_ratio(got_images[keep], want[0], aref.row_bounds(ref_vols, ints[keep], floats[keep], rows[keep]))[0] <= 1.0
    assert np.array_equal(got_labels[keep], want[1])
    assert float(np.mean(got_images[6] == 1.5)) > 0.9          # nearly all pad, and written
    assert bool((out_images[1:6] == -7.0).all()) and bool((out_labels[1:6] == -7.0).all())
    assert prod.status == 1


@gpu
def test_bad_python_arguments_are_refused():
    aug = _aug()
    image, label = ref.synthetic_volume(SHAPES[0], 80)
    vol = aug.DeviceVolume(image, label, device=DEV)
    for bad in (dict(rotate_prob=1.5), dict(zoom_prob=-0.1), dict(rotate_prob=0.5, rotate_range=(0.1, 0.1)),
                dict(rotate_prob=0.5, rotate_range=(0.1, 0.1, 1.6)), dict(rotate_range=(-0.1, 0.0, 0.0)),
                dict(zoom_prob=0.5, zoom_range=(0.0, 1.0)), dict(zoom_prob=0.5, zoom_range=(1.2, 0.8)),
                dict(zoom_range=(1.0, float("inf"))), dict(zoom_range=(1.0,)), dict(pad_value=float("nan")), dict(pad_value="air")):
        with pytest.raises(ValueError):
            aug.DeviceBatchProducer([vol], roi=ROI, class_ids=range(4), **bad)
    # the defaults take today's path and return today's objects
    plain = aug.DeviceBatchProducer([vol], roi=ROI, class_ids=range(4), rotate_range=(0.3, 0.3, 0.3), zoom_range=(0.8, 1.2))
    params = plain.draw([0, 0], counter=0)
    assert torch.is_tensor(params) and params.shape == (2, 8)
    turned = aug.DeviceBatchProducer([vol], roi=ROI, class_ids=range(4), rotate_prob=0.5, rotate_range=(0.3, 0.3, 0.3))
    both = turned.draw([0, 0], counter=0)
    assert isinstance(both, tuple) and torch.equal(both[0], params) and both[1].shape == (2, 16)
    with pytest.raises(ValueError):
        turned.apply(both[0])
    with pytest.raises(AssertionError):
        turned.apply(both[0], affine=both[1].cpu())
    with pytest.raises(AssertionError):
        turned.apply(both[0], affine=both[1][:, :12].contiguous())
    images, labels = turned.apply(both[0], affine=both[1])
    again = turned.apply(*turned.draw([0, 0], counter=0)[:1], affine=both[1])         # a logged pair replays its batch
    assert torch.equal(images, again[0]) and torch.equal(labels, again[1]) and turned.status == 0


def test_split_affine_names_the_columns_on_the_host():
    aug = _aug()
    rows = np.stack([aref.row((0.1, -0.2, 0.05), 1.3, 3, -3.5), aref.row(), aref.row((0.0, 0.0, 0.0), 0.8, 2, 0.25)])
    m, t, z, events, pad = aug.split_affine(torch.from_numpy(rows))
    assert m.shape == (3, 3, 3) and np.array_equal(m.numpy().reshape(3, 9), rows[:, :9])
    assert np.array_equal(t.numpy(), rows[:, aref.A_T:aref.A_T + 3]) and z.tolist() == [np.float32(1.3), 1.0, np.float32(0.8)]
    assert events.dtype == torch.int32 and events.tolist() == [3, 0, 2] and pad.tolist() == [-3.5, 0.0, 0.25]
    assert len(aug.AFFINE_COLUMNS) == 5


def test_argument_errors_through_the_c_abi():
    """The entry points refuse bad arguments before they touch a device: the library is all this needs."""
    from diff_unet_amos_amd import _native as nv
    lib = nv.lib()
    one = C.c_void_p(16)
    cfg = nv.AugConfig((C.c_int * 3)(16, 16, 16), 3, 0.5, 0.1, 0.1, 0.1, 0.1, 0.5, 0.1, 0)

    def acfg(**kw):
        f = dict(rotate_prob=0.5, tan=(0.2, 0.2, 0.2), zoom_prob=0.5, zoom_min=0.7, zoom_span=0.7, pad_value=0.0)
        f.update(kw)
        return nv.AugAffineConfig(f["rotate_prob"], (C.c_float * 3)(*f["tan"]), f["zoom_prob"], f["zoom_min"], f["zoom_span"],
                                  f["pad_value"], 0)

    def draw(a, cfg=cfg, affine=one, counter=one, use=0):
        return lib.dua_aug_draw_affine(one, 1, one, 2, C.byref(cfg), C.byref(a) if a is not None else None, 0, counter, use, 0, one,
                                       affine, one, None)

    for bad in (dict(rotate_prob=1.5), dict(rotate_prob=float("nan")), dict(zoom_prob=-0.5), dict(tan=(0.2, 1.5, 0.2)),
                dict(tan=(-0.1, 0.2, 0.2)), dict(tan=(0.2, 0.2, float("nan"))), dict(zoom_min=0.0), dict(zoom_min=float("inf")),
                dict(zoom_span=-0.1), dict(zoom_span=float("nan")), dict(pad_value=float("inf")), dict(pad_value=float("nan"))):
        assert draw(acfg(**bad)) == nv.ERR_ARG, bad
    assert draw(None) == nv.ERR_ARG and draw(acfg(), affine=None) == nv.ERR_ARG and draw(acfg(), counter=None) == nv.ERR_ARG
    bad_cfg = nv.AugConfig((C.c_int * 3)(16, 8, 16), 3, 0.5, 0.1, 0.1, 0.1, 0.1, 0.5, 0.1, 0)        # rot90 on a non-square window
    assert draw(acfg(), cfg=bad_cfg) == nv.ERR_ARG

    sm = nv.AugSmoothing(0.3, 1.0, 1e-6, float("inf"))

    def apply(centroids=None, smoothing=None, K=0, affine=one, B=2, roi=(16, 16, 16), Cn=4, images=one, params=one):
        return lib.dua_aug_apply_affine(one, 1, centroids, K, C.byref(smoothing) if smoothing is not None else None, params, affine, B,
                                        *roi, one, Cn, images, one, one, None)

    assert apply(affine=None) == nv.ERR_ARG and apply(params=None) == nv.ERR_ARG and apply(images=None) == nv.ERR_ARG
    assert apply(B=0) == nv.ERR_ARG and apply(B=65536) == nv.ERR_ARG and apply(Cn=0) == nv.ERR_ARG and apply(Cn=65) == nv.ERR_ARG
    assert apply(roi=(16, 0, 16)) == nv.ERR_ARG and apply(roi=(2 ** 22 + 1, 1, 1)) == nv.ERR_ARG
    assert apply(roi=(2048, 2048, 2048)) == nv.ERR_ARG         # 2^33 voxels
    assert apply(centroids=one) == nv.ERR_ARG and apply(smoothing=sm) == nv.ERR_ARG         # both or neither
    assert apply(centroids=one, smoothing=sm, K=0) == nv.ERR_ARG and apply(centroids=one, smoothing=sm, K=257) == nv.ERR_ARG
    assert apply(centroids=one, smoothing=nv.AugSmoothing(-0.3, 1.0, 1e-6, 1.0), K=16) == nv.ERR_ARG
    assert apply(centroids=one, smoothing=nv.AugSmoothing(0.3, 1.0, 0.0, 1.0), K=16) == nv.ERR_ARG
