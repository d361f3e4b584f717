"""Normalized Surface Dice on the device (csrc/surface.hip, metrics.surface_dice_table / surface_report, the band-limited
distance transform, evaluate_volume(surface=...)) against the scipy fixture and the torch restatement of
tests/surface_dice_ref.py.  Equality is the bar: the quantities are integers and one IEEE division, and the bounded transform
makes the additions of the unbounded one in the same order.

The cases that are not in the fixture use spacings whose squares are exact in binary ((1, 1, 1), (2, 1.5, 1.5), (1.5, 1, 1)):
every squared distance is then exact in fp64 whatever the order of its three terms, so the restatement (which sums them in
another order than the kernels) must agree to the last count.  The fixture's third spacing (0.8, 0.7, 1.3) is covered by the gap
condition its generator enforces."""
import numpy as np
import pytest
import torch

import surface_dice_ref as R

pytestmark = pytest.mark.gpu


def _check_against_ref(t, a, b, rows, spacing, k, nan_for_nonexisting=True):
    """Every (n, c, t) of a metrics dict against the restatement; rows: the [C][T] tolerance table."""
    N, Cc = a.shape[:2]
    for n in range(N):
        for c in range(Cc):
            r = R.surface_dice_ref(a[n, c], b[n, c], rows[c], spacing, k, nan_for_nonexisting)
            what = (n, c)
            assert int(t["surface_test"][n, c]) == r["n_a"] and int(t["surface_reference"][n, c]) == r["n_b"], what
            assert t["within_test"][n, c].tolist() == r["within_ab"], what
            assert t["within_reference"][n, c].tolist() == r["within_ba"], what
            assert R.same_bits(t["nsd"][n, c].cpu().numpy(), r["nsd"]), what


def test_golden():
    from diff_unet_amos_amd import metrics, ops
    cases, z = R.golden()
    tol = [float(x) for x in z["tolerances"]]
    for i, (name, a, b) in enumerate(cases):
        ta, tb = a[None, None].float().cuda(), b[None, None].cuda()
        for j, sp in enumerate(z["spacings"]):
            for m, k in enumerate(z["connectivities"]):
                sp3, k = tuple(float(x) for x in sp), int(k)
                what = (name, sp3, k)
                t = metrics.surface_dice_table(ta, tb, [tol], voxel_spacing=sp3, connectivity=k)
                assert t["nsd"].shape == (1, 1, 6) and t["nsd"].dtype == torch.float64
                assert int(t["surface_test"][0, 0]) == int(z["n_a"][i, j, m]), what
                assert int(t["surface_reference"][0, 0]) == int(z["n_b"][i, j, m]), what
                assert t["within_test"][0, 0].tolist() == z["within_ab"][i, j, m].tolist(), what
                assert t["within_reference"][0, 0].tolist() == z["within_ba"][i, j, m].tolist(), what
                assert R.same_bits(t["nsd"][0, 0].cpu().numpy(), z["nsd"][i, j, m]), what
                _check_against_ref(t, a[None, None], b[None, None], [tol], sp3, k)
                for bounded in (True, False):
                    counts, within, nsd = ops.surface_dice_table(ta, tb, [tol], sp3, k, True, bounded=bounded)
                    assert counts[0, 3:].tolist() == [int(z["n_a"][i, j, m]), int(z["n_b"][i, j, m])], (what, bounded)
                    assert within[0, :, 0].tolist() == z["within_ab"][i, j, m].tolist(), (what, bounded)
                    assert within[0, :, 1].tolist() == z["within_ba"][i, j, m].tolist(), (what, bounded)
                    assert R.same_bits(nsd[0].cpu().numpy(), z["nsd"][i, j, m]), (what, bounded)
        # the per-pair function agrees with the table entry (one spacing and connectivity per case keeps this quick)
        t = metrics.surface_dice_table(ta, tb, [tol], voxel_spacing=(2.0, 1.5, 1.5), connectivity=3)
        for q in (0, 3):
            v = metrics.normalized_surface_dice(a.cuda(), b.to(torch.uint8).cuda(), tol[q], voxel_spacing=(2.0, 1.5, 1.5),
                                                connectivity=3)
            assert isinstance(v, float) and R.same_bits(v, float(t["nsd"][0, 0, q])), (name, q)
    # both empty with nan_for_nonexisting=False
    name, a, b = cases[[c[0] for c in cases].index("both_empty")]
    t = metrics.surface_dice_table(a[None, None].cuda(), b[None, None].cuda(), [tol], nan_for_nonexisting=False)
    assert t["nsd"][0, 0].tolist() == [0.0] * 6
    assert metrics.normalized_surface_dice(a.cuda(), b.cuda(), 1.0, nan_for_nonexisting=False) == 0.0


def test_per_class_rows_and_reproducible():
    from diff_unet_amos_amd import metrics
    g = torch.Generator().manual_seed(4)
    a = R.random_blobs((2, 3, 30, 27, 22), g, 0.05)
    b = R.random_blobs((2, 3, 30, 27, 22), g, 0.0)
    b[0, 2] = False                                                          # one class empty in one sample
    sp = (2.0, 1.5, 1.5)
    rows = [[1.5, 4.0], [0.0, 2.5], [3.0, 2.0]]                              # rows differ: a wrong v % classes fails
    t1 = metrics.surface_dice_table(a.cuda(), b.float().cuda(), rows, voxel_spacing=sp, connectivity=2)
    t2 = metrics.surface_dice_table(a.cuda(), b.float().cuda(), rows, voxel_spacing=sp, connectivity=2)
    assert t1["nsd"].shape == (2, 3, 2) and t1["within_test"].shape == (2, 3, 2) and t1["surface_test"].shape == (2, 3)
    for key in t1:
        x, y = t1[key].cpu().numpy(), t2[key].cpu().numpy()
        assert R.same_bits(x, y) if key == "nsd" else np.array_equal(x, y), key
    da, db = a.cuda(), b.cuda()                                              # the restatement's brute force, on the device
    _check_against_ref(t1, da, db, rows, sp, 2)
    assert float(t1["nsd"][0, 2, 0]) == 0.0 and int(t1["surface_reference"][0, 2]) == 0
    # rows that differ must give different counts somewhere, or the test would not see a wrong row
    swapped = metrics.surface_dice_table(a.cuda(), b.float().cuda(), rows[1:] + rows[:1], voxel_spacing=sp, connectivity=2)
    assert not torch.equal(swapped["within_test"], t1["within_test"])
    # a scalar and a per-class sequence are the T = 1 tables
    s = metrics.surface_dice_table(a.cuda(), b.cuda(), 2.0, voxel_spacing=sp)
    _check_against_ref(s, da, db, [[2.0]] * 3, sp, 1)
    s = metrics.surface_dice_table(a.cuda(), b.cuda(), [1.5, 0.0, 3.0], voxel_spacing=sp, nan_for_nonexisting=False)
    _check_against_ref(s, da, db, [[1.5], [0.0], [3.0]], sp, 1, False)


def _bounded_check(seeds, spacing, md):
    from diff_unet_amos_amd import ops
    full = ops.surface_edt_sq(seeds, spacing)
    got = ops.surface_edt_sq(seeds, spacing, max_distance=md)
    keep = full <= md * md
    inf = torch.full_like(full, float("inf"))
    want = torch.where(keep, full, inf)
    assert torch.equal(got.view(torch.int64), want.view(torch.int64)), (tuple(seeds.shape), spacing, md)
    return int(keep.sum())


@pytest.mark.parametrize("shape", [(35, 33, 40), (17, 64, 9), (1, 5, 7)])
def test_bounded_edt_is_the_unbounded_one_up_to_the_bound(shape):
    g = torch.Generator().manual_seed(sum(shape))
    a = R.random_blobs((2, 3, *shape), g, 0.0, sigma=1.2).reshape(6, *shape)
    a[1] = False                                                             # one volume without seeds
    surf = torch.stack([R.border(x, 1) for x in a]).to(torch.uint8).cuda()
    sparse = (torch.rand((6, *shape), generator=g) < 0.002).to(torch.uint8).cuda()    # far seeds: most of a volume is +inf
    for spacing in ((1.0, 1.0, 1.0), (2.0, 1.5, 1.5)):
        for md in (0.0, 1.5, 4.0):
            kept = _bounded_check(surf, spacing, md)
            assert kept >= int(surf.sum())                                   # the seeds themselves are at distance 0
            _bounded_check(sparse, spacing, md)


def test_bounded_edt_without_seeds_and_with_a_corner_seed():
    from diff_unet_amos_amd import ops
    shape = (21, 30, 26)
    none = torch.zeros((1, *shape), dtype=torch.uint8).cuda()
    corner = none.clone(); corner[0, 0, 0, 0] = 1
    far = none.clone(); far[0, -1, -1, -1] = 1
    for spacing in ((1.0, 1.0, 1.0), (2.0, 1.5, 1.5)):
        for md in (0.0, 1.5, 4.0):
            assert bool(torch.isinf(ops.surface_edt_sq(none, spacing, max_distance=md)).all())
            for seeds in (corner, far):
                kept = _bounded_check(seeds, spacing, md)
                assert kept >= 1 and (md == 0.0) == (kept == 1)
    # a bound beyond the volume's diagonal is the unbounded transform
    assert _bounded_check(corner, (1.0, 1.0, 1.0), 1000.0) == 21 * 30 * 26


def test_report_is_both_tables_bit_for_bit():
    from diff_unet_amos_amd import metrics
    g = torch.Generator().manual_seed(12)
    a = R.random_blobs((2, 3, 30, 27, 22), g, 0.05).cuda()
    b = R.random_blobs((2, 3, 30, 27, 22), g, 0.0)
    b[0, 2] = False                                                          # NaN rows in the distance table, 0 in the NSD
    b[1, 0] = True                                                           # a full mask: NaN in the distance table only
    b = b.float().cuda()
    sp, rows = (2.0, 1.5, 1.5), [[1.5, 4.0], [0.0, 2.5], [3.0, 2.0]]
    for flag in (True, False):
        rep = metrics.surface_report(a, b, rows, voxel_spacing=sp, connectivity=2, nan_for_nonexisting=flag)
        table = metrics.surface_distance_table(a, b, voxel_spacing=sp, connectivity=2, nan_for_nonexisting=flag)
        dice = metrics.surface_dice_table(a, b, rows, voxel_spacing=sp, connectivity=2, nan_for_nonexisting=flag)
        assert set(rep) == set(table) | set(dice) and set(dice) == set(metrics.DICE_KEYS)
        for key, want in list(table.items()) + list(dice.items()):
            x, y = rep[key].cpu().numpy(), want.cpu().numpy()
            assert x.dtype == y.dtype and (R.same_bits(x, y) if x.dtype == np.float64 else np.array_equal(x, y)), (key, flag)
    assert bool(rep["hd"].isnan().sum() == 0) and bool(table["hd"][1, 0] == 0.0)          # flag False: zeros, not NaN
    assert float(dice["nsd"][1, 0, 1]) > 0.0                                              # the full mask has a surface


def test_count_pass_over_many_blocks():
    from diff_unet_amos_amd import metrics
    g = torch.Generator().manual_seed(31)
    a = R.random_blobs((1, 4, 64, 64, 64), g, 0.4, sigma=2.5)
    b = R.random_blobs((1, 4, 64, 64, 64), g, 0.5, sigma=2.5)
    rows = [[0.0, 1.0, 2.0], [1.0, 3.0, 6.0], [1.5, 2.5, 40.0], [2.0, 4.0, 200.0]]
    sp = (2.0, 1.5, 1.5)
    t = metrics.surface_dice_table(a.cuda(), b.cuda(), rows, voxel_spacing=sp, connectivity=1)
    # 64^3 voxels = 16 blocks of the count pass per volume
    ref_a, ref_b = a.cuda(), b.cuda()                                        # the restatement's brute force, on the device
    _check_against_ref(t, ref_a, ref_b, rows, sp, 1)
    assert float(t["nsd"][0, 3, 2]) == 1.0                                   # a tolerance beyond the diagonal takes every voxel


def test_end_to_end_in_evaluate_volume():
    from diff_unet_amos_amd import inference, metrics
    from diff_unet_amos_amd.diff_unet import DiffUNet
    torch.manual_seed(3)
    net = DiffUNet(in_channels=1, out_channels=2, features=(8, 8, 16, 32, 64, 8), sample_steps=4,
                   compute_dtype=torch.float32).cuda().eval()
    g = torch.Generator().manual_seed(9)
    image = torch.rand(1, 1, 40, 40, 40, generator=g).cuda()
    onehot = R.random_blobs((1, 2, 40, 40, 40), g, 0.2, sigma=2.0)
    labels = onehot.float().cuda()
    model = lambda x, **kw: net(image=x, **kw)                               # noqa: E731
    kw = dict(roi_size=(32, 32, 32), sw_batch_size=1, overlap=0.25)
    surface = {"tolerance": [1.0, 2.0], "voxel_spacing": (1.5, 1.0, 1.0)}

    def same(x, y):
        for key in x:
            p, q = x[key].cpu().numpy(), y[key].cpu().numpy()
            assert R.same_bits(p, q) if p.dtype == np.float64 else np.array_equal(p, q), key
        assert set(x) == set(y)

    torch.manual_seed(5)
    plain = inference.evaluate_volume(model, image, labels, **kw)
    assert len(plain) == 2
    torch.manual_seed(5)
    out = inference.evaluate_volume(model, image, labels, surface=surface, **kw)
    assert len(out) == 3
    mask, dice, report = out
    assert torch.equal(mask, plain[0]) and torch.equal(dice, plain[1])
    assert report["nsd"].shape == (1, 2, 1) and set(report) == set(metrics.DICE_KEYS)
    same(report, metrics.surface_dice_table(mask, labels, [1.0, 2.0], voxel_spacing=(1.5, 1.0, 1.0)))
    _check_against_ref(report, mask.bool(), onehot.cuda(), [[1.0], [2.0]], (1.5, 1.0, 1.0), 1)

    # with the component filter: the report is of the filtered mask
    post = {"num_components": 1, "connectivity": 1}
    torch.manual_seed(5)
    fmask, fdice, freport = inference.evaluate_volume(model, image, labels, postprocess=post, surface=surface, **kw)
    torch.manual_seed(5)
    fplain = inference.evaluate_volume(model, image, labels, postprocess=post, **kw)
    assert len(fplain) == 2 and torch.equal(fmask, fplain[0]) and torch.equal(fdice, fplain[1])
    same(freport, metrics.surface_dice_table(fmask, labels, [1.0, 2.0], voxel_spacing=(1.5, 1.0, 1.0)))

    # a label map for labels, and the distance table with distances=True
    label_map = torch.zeros((1, 40, 40, 40), dtype=torch.uint8)
    label_map[onehot[:, 1] & ~onehot[:, 0]] = 1
    expanded = torch.stack([label_map == 0, label_map == 1], dim=1).cuda()
    torch.manual_seed(5)
    lmask, ldice, lreport = inference.evaluate_volume(model, image, label_map.cuda(), surface=dict(surface, distances=True), **kw)
    assert torch.equal(lmask, mask) and set(lreport) == set(metrics.DICE_KEYS) | set(metrics.TABLE_KEYS)
    same(lreport, metrics.surface_report(lmask, expanded, [1.0, 2.0], voxel_spacing=(1.5, 1.0, 1.0)))
