"""Class-balanced crop centres in the device batch producer (dua_aug_count_class_candidates, dua_aug_draw_classes;
csrc/augment.hip) against the CPU restatement of their contract (tests/augment_classes_ref.py): the class tables entry by entry,
the draw bit for bit (params, chosen classes, affine rows, tally), the untouched default path, replay, graph capture, one
training step, and the host and C argument checks."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import augment_affine_ref as aref  # noqa: E402
import augment_classes_ref as cref  # noqa: E402
import augment_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROI = (8, 8, 8)
SMALL, LONG = (19, 23, 29), (48, 40, 40)                      # 13 chunks, the last one partial; 75 chunks: a second search round
BASE = dict(roi=ROI, flip_prob=0.3, rot90_prob=0.4, max_k=3, scale_prob=0.5, scale_factors=0.1, shift_prob=0.5, shift_offsets=0.1)
AFFINE = dict(rotate_prob=0.5, rotate_range=(0.5, 0.3, 0.4), zoom_prob=0.5, zoom_range=(0.8, 1.25), pad_value=-0.5)
K6 = 6


def _aug():
    from diff_unet_amos_amd import augment
    return augment


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


@pytest.fixture(scope="module")
def cases():
    """The two volumes of the draw tests, on the device and restated: computed once, shared, left unchanged."""
    volumes = [cref.layered_volume(SMALL, K6, 21, absent=(4,)), cref.layered_volume(LONG, K6, 22, absent=(5,))]
    dev = [_aug().DeviceVolume(image, label, device=DEV, num_classes=K6) for image, label in volumes]
    return dev, [cref.RefClassVolume(image, label, K6) for image, label in volumes]


@pytest.mark.parametrize("K,absent", [(1, ()), (2, ()), (16, (7,)), (64, (40,))])
def test_class_tables_equal_the_restatement_entry_by_entry(K, absent):
    aug = _aug()
    thr = 0.1
    image, label = cref.layered_volume(SMALL, K, 40 + K, absent=absent)
    vol = aug.DeviceVolume(image, label, image_threshold=thr, device=DEV, num_classes=K)
    assert vol.class_prefix is None and vol.class_candidate_counts is None          # lazily
    table = vol.class_candidates()
    assert table is vol.class_candidates() and table.dtype == torch.int32 and tuple(table.shape) == (K, 14)
    sets = cref.class_sets(image.numpy(), label.numpy(), K, thr)
    want = cref.prefix_table(sets, image.numel())
    got = table.cpu().numpy().astype(np.int64)
    assert np.array_equal(got, want)
    counts = vol.class_candidate_counts
    assert counts.dtype == torch.int64 and counts.is_cuda and counts.tolist() == [len(s) for s in sets]
    n0 = int(((label == 0)).sum())
    print(f"K = {K}: candidates per class {counts.tolist()[:8]}..; the threshold keeps {len(sets[0])} of {n0} class-0 voxels")
    assert 0 < len(sets[0]) < n0                               # the threshold removes part of class 0
    for k in absent:
        assert len(sets[k]) == 0 and not got[k].any()
    if K > 2:
        assert list(sets[1]) == [0] and list(sets[2]) == [image.numel() - 1]       # one voxel each, the first and the last
    if K > 3:
        assert len(sets[3]) > 0 and got[3, -2] == 0            # lives in the last, partial chunk only
    pos_neg = vol.prefix.cpu().numpy().astype(np.int64)         # row 0 foreground, row 1 background
    assert np.array_equal(got[0], pos_neg[1])
    assert np.array_equal(got[1:].sum(0), pos_neg[0])
    with pytest.raises(ValueError, match="num_classes"):
        aug.DeviceVolume(image, label, device=DEV).class_candidates()


@pytest.mark.parametrize("ratios,uniform_prob,affine", [([1.0, 0.0, 3.0, 2.0, 5.0, 1.0], 0.0, False), ("present", 0.67, True),
                                                       ([0.0, 0.0, 0.0, 1.0, 2.5, 0.0], 1.0, False), ("present", 0.0, True),
                                                       ([2.0, 1.0, 1.0, 0.0, 0.0, 0.0], 0.67, False)])
def test_draw_gives_the_restatements_rows_classes_and_tally(cases, ratios, uniform_prob, affine):
    aug = _aug()
    dev_vols, ref_vols = cases
    acfg = AFFINE if affine else {}
    seed = 2 ** 41 + 5
    prod = aug.DeviceBatchProducer(dev_vols, class_ids=range(K6), seed=seed, class_ratios=ratios, uniform_prob=uniform_prob, **BASE,
                                   **acfg)
    assert prod.class_tally.dtype == torch.int64 and tuple(prod.class_tally.shape) == (K6 + 1,) and not prod.class_tally.any()
    call, hist = 0, np.zeros(K6 + 1, dtype=np.int64)
    for B, calls in ((1, 3), (16, 2), (17, 2), (2048, 2)):     # 2048: more samples than the workgroup has waves
        vid = [(b + b // 3) % 2 for b in range(B)]
        ids = torch.tensor(vid, dtype=torch.int32, device=DEV)
        for _ in range(calls):
            drawn = prod.draw(ids)
            params, rows = drawn if affine else (drawn, None)
            chosen = prod.chosen_classes.cpu().numpy()
            ints, floats, want_chosen = cref.draw_classes(ref_vols, vid, call, seed=seed, class_ratios=ratios,
                                                          uniform_prob=uniform_prob, **BASE)
            got_ints, got_floats = aug.split_params(params.cpu())
            assert chosen.dtype == np.int32 and np.array_equal(chosen, want_chosen), (B, call)
            assert np.array_equal(got_ints.numpy(), ints), (B, call)
            assert np.array_equal(_bits(got_floats.numpy()), _bits(floats)), (B, call)
            if affine:
                assert np.array_equal(_bits(rows.cpu().numpy()), _bits(aref.affine_rows(B, call, seed, **acfg))), (B, call)
            hist += np.bincount(np.where(chosen < 0, K6, chosen), minlength=K6 + 1)
            call += 1
    assert prod.counter == call and prod.status == 0
    assert prod.class_tally.cpu().tolist() == hist.tolist()    # the tally is the histogram of chosen
    print(f"ratios {ratios}, uniform_prob {uniform_prob}: tally {hist.tolist()}")
    if uniform_prob == 1.0:
        assert hist[K6] == hist.sum()
    if uniform_prob == 0.0:
        assert hist[K6] == 0
    logged = prod.draw(ids, counter=call - 1)                  # an overriding counter reproduces the last call
    assert torch.equal(logged[0] if affine else logged, params) and prod.counter == call
    prod.reset_class_tally()
    assert not prod.class_tally.any()


def test_drawn_frequencies_follow_the_ratios():
    """The 20 000 draws whose restated frequencies tests/test_augment_classes_ref.py bounds, drawn on the device."""
    aug = _aug()
    vol = cref.frequency_volume()
    dev = aug.DeviceVolume(vol.image, vol.label, device=DEV, num_classes=cref.FREQ["K"])
    prod = aug.DeviceBatchProducer([dev], roi=cref.FREQ["roi"], class_ids=range(cref.FREQ["K"]), seed=cref.FREQ["seed"],
                                   class_ratios=cref.FREQ["ratios"], uniform_prob=cref.FREQ["uniform_prob"])
    ids = torch.zeros(cref.FREQ["B"], dtype=torch.int32, device=DEV)
    chosen = []
    for _ in range(cref.FREQ["calls"]):
        prod.draw(ids)
        chosen.append(prod.chosen_classes.clone())
    chosen = torch.cat(chosen).cpu().numpy()
    cref.check_frequencies(chosen, vol)
    tally = prod.class_tally.cpu().numpy()
    assert int(tally.sum()) == len(chosen) == 20000 and prod.status == 0
    assert tally.tolist() == np.bincount(np.where(chosen < 0, cref.FREQ["K"], chosen), minlength=cref.FREQ["K"] + 1).tolist()


def test_the_default_producer_and_a_null_class_table_give_todays_bits(cases):
    from diff_unet_amos_amd import _native as nv
    from diff_unet_amos_amd import ops
    aug = _aug()
    _, ref_vols = cases
    fresh = [aug.DeviceVolume(v.image, v.label, device=DEV, num_classes=K6) for v in ref_vols]
    cfg = dict(BASE, pos=2, neg=1, seed=77)
    prod = aug.DeviceBatchProducer(fresh, class_ids=range(K6), **cfg)
    assert prod.class_tally is None and prod.chosen_classes is None and prod.class_draw_table is None
    assert all(v.class_prefix is None for v in fresh)          # class_candidates() was never called
    vid = [b % 2 for b in range(19)]
    ids = torch.tensor(vid, dtype=torch.int32, device=DEV)
    for call in (0, 1, 2 ** 33 + 4):
        params = prod.draw(ids, counter=call)
        assert torch.is_tensor(params)
        ints, floats = ref.draw(ref_vols, vid, call, **cfg)
        assert torch.equal(params.cpu(), aug.pack_params(ints, floats)), call
        # the new entry without a class table and without the uniform event: the bits of dua_aug_draw and of dua_aug_draw_affine
        again = torch.full_like(params, -9)
        ops.aug_draw_classes(prod.table, ids, prod.cfg, prod.seed, prod._counter, again, prod._status, counter_value=call)
        assert torch.equal(again, params), call
        turned = aug.DeviceBatchProducer(fresh, class_ids=range(K6), **cfg, **AFFINE)
        want_p, want_a = turned.draw(ids, counter=call)
        got_p, got_a = torch.full_like(want_p, -9), torch.full_like(want_a, -9.0)
        ops.aug_draw_classes(turned.table, ids, turned.cfg, turned.seed, turned._counter, got_p, turned._status, counter_value=call,
                             affine_cfg=turned.affine_cfg, affine=got_a)
        assert torch.equal(got_p, params) and torch.equal(want_p, params), call
        assert np.array_equal(_bits(got_a.cpu().numpy()), _bits(want_a.cpu().numpy())), call
    assert prod.counter == 0 and prod.status == 0
    # uniform_prob alone keeps the pos / neg rule for the rest and reports no classes
    anywhere = aug.DeviceBatchProducer(fresh, class_ids=range(K6), uniform_prob=0.5, **cfg)
    params = anywhere.draw(ids, counter=3)
    ints, floats, chosen = cref.draw_classes(ref_vols, vid, 3, uniform_prob=0.5, **cfg)
    assert torch.equal(params.cpu(), aug.pack_params(ints, floats)) and anywhere.chosen_classes is None
    assert 0 < int(np.sum(chosen == cref.UNIFORM)) < len(vid) and all(v.class_prefix is None for v in fresh)
    assert isinstance(nv.AugClassVolume(), C.Structure) and C.sizeof(nv.AugClassVolume) == 16


def test_a_logged_row_replays_its_patch_and_next_is_capturable(cases):
    aug = _aug()
    dev_vols, ref_vols = cases
    cfg = dict(BASE, seed=8)
    class_ids, vid = (0, 2, 5), [1, 0, 1, 1]
    B = len(vid)
    prod = aug.DeviceBatchProducer(dev_vols, class_ids=class_ids, class_ratios="present", uniform_prob=0.3, **cfg)
    ids = torch.tensor(vid, dtype=torch.int32, device=DEV)
    first = prod.next(ids)                                     # an eager call first: chosen_classes exists, the capture starts at c = 1
    ints, floats, chosen = cref.draw_classes(ref_vols, vid, 0, class_ratios="present", uniform_prob=0.3, **cfg)
    want = ref.apply(ref_vols, ints, floats, ROI, class_ids)
    assert torch.equal(first[0].cpu(), want[0]) and torch.equal(first[1].cpu(), want[1])
    replayed = prod.apply(aug.pack_params(ints, floats, device=DEV))         # a logged row is an ordinary row
    assert torch.equal(replayed[0], first[0]) and torch.equal(replayed[1], first[1])
    assert prod.chosen_classes.cpu().tolist() == chosen.tolist() and prod.counter == 1
    out_images = torch.zeros((B, 1) + ROI, device=DEV)
    out_labels = torch.zeros((B, len(class_ids)) + ROI, device=DEV)
    graph = torch.cuda.CUDAGraph()
    stream = torch.cuda.Stream(device=DEV)
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):           # one stream: a graph without parallel branches
            prod.next(ids, out_images, out_labels)
    torch.cuda.current_stream().wait_stream(stream)
    assert prod.counter == 1 and int(prod.class_tally.sum()) == B            # capturing ran nothing
    seen = set()
    for n, counter in enumerate((1, 2, 3)):
        graph.replay()
        torch.cuda.synchronize()
        ints, floats, chosen = cref.draw_classes(ref_vols, vid, counter, class_ratios="present", uniform_prob=0.3, **cfg)
        want = ref.apply(ref_vols, ints, floats, ROI, class_ids)
        assert prod.chosen_classes.cpu().tolist() == chosen.tolist(), counter
        assert torch.equal(out_images.cpu(), want[0]) and torch.equal(out_labels.cpu(), want[1]), counter
        assert int(prod.class_tally.sum()) == B * (n + 2)       # the tally grows by B per replay
        seen.add(tuple(ints[:, 1:4].reshape(-1).tolist()))
    assert len(seen) == 3 and prod.counter == 4 and prod.status == 0          # a new batch on every replay


def test_rows_that_cannot_be_drawn_get_volume_minus_one_and_set_status(cases):
    """A cum row the host would never build: it chooses a class without candidates, or no class at all; and an id outside the
    table.  Such a sample gets the volume -1 row, chosen -2, no count in the tally, and *status; its neighbours are drawn."""
    from diff_unet_amos_amd import _native as nv
    from diff_unet_amos_amd import ops
    aug = _aug()
    dev_vols, ref_vols = cases
    cfg = dict(BASE, seed=5)
    good = [1.0, 0.0, 3.0, 2.0, 5.0, 1.0]
    prod = aug.DeviceBatchProducer(dev_vols, class_ids=range(K6), class_ratios=good, **cfg)
    assert ref_vols[0].counts[4] == 0
    cum = prod.class_cum.clone()
    cum[0] = torch.tensor([0.0, 0.0, 0.0, 0.0, 1.0, 1.0])     # volume 0: always class 4, which it does not hold
    rows = (nv.AugClassVolume * 2)(*[nv.AugClassVolume(v.class_prefix.data_ptr(), cum.data_ptr() + 4 * K6 * i)
                                     for i, v in enumerate(dev_vols)])
    table = torch.frombuffer(bytearray(bytes(rows)), dtype=torch.uint8).reshape(2, -1).to(DEV)
    vid = [0, 1, 0, 1, 7]                                      # the last id is outside the table
    ids = torch.tensor(vid, dtype=torch.int32, device=DEV)
    for zero_row in (False, True):
        if zero_row:
            cum[0] = 0.0                                       # volume 0: no class can be chosen
        params = torch.full((5, 8), -9, dtype=torch.int32, device=DEV)
        chosen = torch.full((5,), -9, dtype=torch.int32, device=DEV)
        tally, status = torch.zeros(K6 + 1, dtype=torch.int64, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
        ops.aug_draw_classes(prod.table, ids, prod.cfg, prod.seed, prod._counter, params, status, counter_value=3, class_table=table,
                             num_classes=K6, uniform_prob=0.0, chosen=chosen, tally=tally)
        assert int(status.item()) == 1
        got = params.cpu()
        for b in (0, 2, 4):
            assert got[b].tolist() == [-1, 0, 0, 0, 0, 0, 0, 0] and int(chosen[b]) == cref.BAD, b
        assert int(tally.sum()) == 2 and set(chosen[[1, 3]].tolist()) <= {0, 2, 3, 4, 5}
        # samples 1 and 3 are the restatement's samples of the same index: the bad neighbours changed nothing
        full = cref.draw_classes(ref_vols, [1, 1, 1, 1, 1], 3, seed=5, class_ratios=good, **BASE)
        assert torch.equal(got[[1, 3]], aug.pack_params(full[0][[1, 3]], full[1][[1, 3]]))
        assert chosen[[1, 3]].tolist() == full[2][[1, 3]].tolist()


def test_one_training_step_fed_by_a_class_balanced_producer():
    """NativeConvTrainer.step on the tiny 32^3 net of tests/test_augment_gpu.py, fed by class_ratios="present"."""
    from diff_unet_amos_amd.diff_unet import DiffUNet
    from diff_unet_amos_amd.training import NativeConvTrainer
    aug = _aug()
    vols = [aug.DeviceVolume(*ref.synthetic_volume(s, 70 + i, classes=3), device=DEV, num_classes=3)
            for i, s in enumerate([(40, 36, 44), (33, 47, 38)])]
    prod = aug.DeviceBatchProducer(vols, roi=(32, 32, 32), class_ids=(1, 2), flip_prob=0.5, rot90_prob=0.5, seed=12, class_ratios="present")
    images, labels = prod.next([0, 1])
    assert set(prod.chosen_classes.cpu().tolist()) <= {1, 2} and float(labels.sum()) > 0
    torch.manual_seed(0)
    net = DiffUNet(in_channels=1, out_channels=2, features=(8, 8, 16, 32, 64, 8)).to(DEV)
    g = torch.Generator().manual_seed(3)
    noise = torch.randn(2, 2, 32, 32, 32, generator=g).to(DEV)
    loss = NativeConvTrainer(net, lr=1e-3).step(images, labels, noise=noise, t=torch.tensor([417, 80], device=DEV))
    print(f"loss of one step fed by class-balanced patches: {float(loss)!r}")
    assert bool(torch.isfinite(loss)) and prod.status == 0


def test_bad_python_arguments_are_refused_with_their_cause():
    aug = _aug()
    image, label = cref.layered_volume(SMALL, 4, 50)
    vol = aug.DeviceVolume(image, label, device=DEV, num_classes=4)
    kw = dict(roi=ROI, class_ids=range(4))
    for bad, cause in (([1.0, 1.0, 1.0], "one entry per class"), ([1.0] * 5, "one entry per class"), ([1.0, -1.0, 1.0, 1.0], "non-negative"),
                       ([1.0, float("nan"), 1.0, 1.0], "finite"), ([1.0, float("inf"), 1.0, 1.0], "finite"), ("all", "present"),
                       ([1.0, "x", 1.0, 1.0], "sequence of numbers")):
        with pytest.raises(ValueError, match=cause):
            aug.DeviceBatchProducer([vol], class_ratios=bad, **kw)
    for pn in (dict(pos=2), dict(neg=3), dict(pos=0.5, neg=0.5)):
        with pytest.raises(ValueError, match="pos"):
            aug.DeviceBatchProducer([vol], class_ratios="present", **pn, **kw)
    with pytest.raises(ValueError, match="num_classes"):
        aug.DeviceBatchProducer([vol, aug.DeviceVolume(image, label, device=DEV)], class_ratios="present", **kw)
    with pytest.raises(ValueError, match="one num_classes"):
        aug.DeviceBatchProducer([vol, aug.DeviceVolume(image, label, device=DEV, num_classes=5)], class_ratios="present", **kw)
    with pytest.raises(ValueError, match="at most 64"):
        aug.DeviceBatchProducer([aug.DeviceVolume(image, label, device=DEV, num_classes=65)], class_ratios="present", **kw)
    empty = aug.DeviceVolume(image, torch.zeros_like(label), device=DEV, num_classes=4)
    with pytest.raises(ValueError, match="volume 1 holds no voxel"):          # names the volume
        aug.DeviceBatchProducer([vol, empty], class_ratios="present", **kw)
    with pytest.raises(ValueError, match="volume 0 holds no voxel"):
        aug.DeviceBatchProducer([vol], class_ratios=[0.0, 0.0, 0.0, 0.0], **kw)
    aug.DeviceBatchProducer([vol, empty], class_ratios=[1.0, 1.0, 1.0, 1.0], **kw)       # class 0 occurs in both
    for p in (-0.1, 1.5, float("nan"), "often"):
        with pytest.raises(ValueError, match="uniform_prob"):
            aug.DeviceBatchProducer([vol], uniform_prob=p, **kw)
    with pytest.raises(ValueError, match="class_ratios"):
        aug.DeviceBatchProducer([vol], **kw).reset_class_tally()


def test_argument_errors_through_the_c_abi():
    """The entry points refuse bad arguments before they touch a device: the library is all this needs."""
    from diff_unet_amos_amd import _native as nv
    lib = nv.lib()
    one = C.c_void_p(16)
    cfg = nv.AugConfig((C.c_int * 3)(16, 16, 16), 3, 0.5, 0.1, 0.1, 0.1, 0.1, 0.5, 0.1, 0)
    acfg = nv.AugAffineConfig(0.5, (C.c_float * 3)(0.2, 0.2, 0.2), 0.5, 0.7, 0.7, 0.0, 0)

    def count(image=one, label=one, voxels=4096, thr=0.0, K=16, prefix=one):
        return lib.dua_aug_count_class_candidates(image, label, voxels, thr, K, prefix, None)

    assert count(image=None) == nv.ERR_ARG and count(label=None) == nv.ERR_ARG and count(prefix=None) == nv.ERR_ARG
    assert count(voxels=0) == nv.ERR_ARG and count(voxels=2 ** 31) == nv.ERR_ARG and count(thr=float("nan")) == nv.ERR_ARG
    assert count(K=0) == nv.ERR_ARG and count(K=65) == nv.ERR_ARG and count(K=-1) == nv.ERR_ARG

    def draw(a=None, affine=None, cfg=cfg, classes=one, K=16, p=0.5, chosen=one, tally=one, params=one, counter=one):
        return lib.dua_aug_draw_classes(one, 1, one, 2, C.byref(cfg), C.byref(a) if a is not None else None, 0, counter, 0, 0, params,
                                        affine, one, classes, K, p, chosen, tally, None)

    for p in (-0.1, 1.5, float("nan"), float("inf")):
        assert draw(p=p) == nv.ERR_ARG, p
    assert draw(K=0) == nv.ERR_ARG and draw(K=65) == nv.ERR_ARG
    assert draw(classes=None, tally=None) == nv.ERR_ARG and draw(classes=None, chosen=None) == nv.ERR_ARG      # nothing to report
    assert draw(a=acfg) == nv.ERR_ARG and draw(affine=one) == nv.ERR_ARG                                       # both or neither
    assert draw(params=None) == nv.ERR_ARG and draw(counter=None) == nv.ERR_ARG                                # what dua_aug_draw refuses
    bad_cfg = nv.AugConfig((C.c_int * 3)(16, 8, 16), 3, 0.5, 0.1, 0.1, 0.1, 0.1, 0.5, 0.1, 0)
    assert draw(cfg=bad_cfg) == nv.ERR_ARG
    bad_acfg = nv.AugAffineConfig(1.5, (C.c_float * 3)(0.2, 0.2, 0.2), 0.5, 0.7, 0.7, 0.0, 0)
    assert draw(a=bad_acfg, affine=one) == nv.ERR_ARG
