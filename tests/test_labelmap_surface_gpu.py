"""The surface report of two label maps on the GPU (csrc/surface.hip: dua_surface_map_boxes, dua_surface_map_report;
metrics.label_map_surface_report) against ``metrics.surface_report`` on the one-hot expansion over the full extent.

Bit-equal (compared as 64-bit patterns, so NaN equals NaN): every integer count, hd, hd95, nsd and the within counts -- all
seeds and queries of a class lie in its box, so each squared distance is the minimum of the same fp64 sums.  asd / assd sum
the same fp64 terms (the square roots of those distances) in another block order.  Their bound is derived, not measured: a sum
of n non-negative terms in any order is within (n - 1) 2^-53 of the exact sum, relatively, so two orders differ by at most
2 (n - 1) 2^-53 times the sum, with n the number of terms summed: |border test| for the directed asd.  The division by the
common integer count rounds once in each path (2 ulp more), and assd, the mean of the two directed means, is within the larger
of their two relative bounds plus the rounding of its own addition in each path (2 ulp more; the halving is exact).

Shapes: W = 70 and 66 cross a wave edge of a row; anisotropic spacing (5.0, 0.7, 0.7); organs touching faces of the volume, a
class absent from one map, one absent from both, a class filling the volume; N = 2."""
import numpy as np
import pytest
import torch

import labelmap_eval_ref as LR
from diff_unet_amos_amd import metrics, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOLERANCES = (1.0, 5.5)                      # T = 2: one below the D spacing, one above
EXACT = ("tp", "fp", "fn", "tn", "hd", "hd95", "nsd", "within_test", "within_reference", "surface_test", "surface_reference")
U = 2.0 ** -53


def _pair(shape):
    """Two map pairs of one shape, N = 2: the surface maps and their mirror image along W."""
    t, r = LR.surface_maps(shape)
    return (torch.from_numpy(np.stack([t, t[:, :, ::-1].copy()])).to(DEV), torch.from_numpy(np.stack([r, r[:, :, ::-1].copy()])).to(DEV))


def _expand(maps, classes):
    c = torch.tensor(classes, device=maps.device, dtype=maps.dtype).view(1, -1, 1, 1, 1)
    return (maps[:, None] == c).to(torch.uint8)


def _bits(t):
    return t.view(torch.int64) if t.dtype == torch.float64 else t


def _compare(got, want, what):
    assert sorted(got) == sorted(want)
    for k in EXACT:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, (what, k)
        assert torch.equal(_bits(got[k].contiguous()), _bits(want[k].contiguous())), (what, k, got[k], want[k])
    na, nb = want["surface_test"].double(), want["surface_reference"].double()
    # asd sums |border test| terms; assd is the mean of two directed means, each within its own relative bound, so within the
    # larger of the two; + 2 ulp for the two divisions compared (asd), + 2 more for the two additions compared (assd)
    terms = {"asd": 2.0 * (na - 1.0) + 2.0, "assd": 2.0 * (torch.maximum(na, nb) - 1.0) + 4.0}
    for k in ("asd", "assd"):
        g, w = got[k], want[k]
        assert torch.equal(torch.isnan(g), torch.isnan(w)), (what, k)
        ok = ~torch.isnan(w)
        err, bound = (g[ok] - w[ok]).abs(), terms[k][ok] * U * w[ok]
        print(f"{what} {k}: largest |box - full| = {float(err.max()) if err.numel() else 0.0:.3e}, "
              f"smallest bound = {float(bound.min()) if bound.numel() else 0.0:.3e}, values {w[ok].flatten().tolist()}")
        assert bool((err <= bound).all()), (what, k, err, bound)


@pytest.mark.parametrize("conn", (1, 3))
@pytest.mark.parametrize("shape", LR.SURFACE_SHAPES)
def test_report_equals_the_expansion(shape, conn):
    test, reference = _pair(shape)
    classes = list(LR.SURFACE_CLASSES)
    tol = [list(TOLERANCES)] * len(classes)
    got = metrics.label_map_surface_report(test, reference, classes, tol, LR.SURFACE_SPACING, conn)
    want = metrics.surface_report(_expand(test, classes), _expand(reference, classes), tol, LR.SURFACE_SPACING, conn)
    assert got["hd"].shape == (2, len(classes)) and got["nsd"].shape == (2, len(classes), len(TOLERANCES))
    _compare(got, want, f"{shape} c{conn}")
    # the situations the maps were built for
    k3, k4 = classes.index(3), classes.index(4)
    assert int(want["tp"][0, k3]) == 0 and int(want["fn"][0, k3]) > 0 and bool(torch.isnan(got["hd"][0, k3]))   # absent from the test
    assert float(got["nsd"][0, k3, 0]) == 0.0                                                                  # one border empty
    assert int(got["tn"][0, k4]) == test[0].numel() and bool(torch.isnan(got["nsd"][0, k4]).all())             # absent from both
    assert bool((got["hd"][:, classes.index(2)] > 0).all()) and bool((got["nsd"][:, classes.index(2), 1] >= got["nsd"][:, classes.index(2), 0]).all())
    # nan_for_nonexisting=False and a per-class scalar tolerance
    zero = metrics.label_map_surface_report(test, reference, classes, 2.0, LR.SURFACE_SPACING, conn, nan_for_nonexisting=False)
    _compare(zero, metrics.surface_report(_expand(test, classes), _expand(reference, classes), 2.0, LR.SURFACE_SPACING, conn, False),
             f"{shape} c{conn} zeros")
    assert float(zero["hd"][0, k4]) == 0.0 and float(zero["nsd"][0, k4, 0]) == 0.0


def test_a_class_that_fills_the_volume():
    t, r = LR.full_class_maps(LR.SURFACE_SHAPES[0])
    test, reference = torch.from_numpy(np.stack([t, r])).to(DEV), torch.from_numpy(np.stack([r, r])).to(DEV)
    got = metrics.label_map_surface_report(test, reference, [1, 0], [[0.5, 2.0]] * 2, LR.SURFACE_SPACING)
    want = metrics.surface_report(_expand(test, [1, 0]), _expand(reference, [1, 0]), [[0.5, 2.0]] * 2, LR.SURFACE_SPACING)
    _compare(got, want, "full class")
    assert bool(torch.isnan(got["hd"][0, 0])) and not bool(torch.isnan(got["nsd"][0, 0]).any())      # a full mask: NaN table, a border
    assert float(got["hd"][1, 0]) == 0.0 and float(got["nsd"][1, 0, 0]) == 1.0                       # identical maps


def test_boxes_are_the_bounding_boxes_and_passing_them_changes_nothing():
    test, reference = _pair(LR.SURFACE_SHAPES[1])
    table = ops.surface_map_boxes(test, reference, 6)
    assert table.dtype == torch.int32 and tuple(table.shape) == (2, 6, 6)
    want = [[LR.box_of(a, b, c) for c in range(6)] for a, b in zip(test.cpu().numpy(), reference.cpu().numpy())]
    assert table.cpu().tolist() == want
    classes = [5, 1, 4, 2]                                                                          # any order, any subset
    tol = [[1.0, 5.5]] * 4
    plain = metrics.label_map_surface_report(test, reference, classes, tol, LR.SURFACE_SPACING)
    rows = [[pair[c] for c in classes] for pair in want]
    for boxes in (rows, table[:, classes].cpu(), np.asarray(rows, np.int32)):
        given = metrics.label_map_surface_report(test, reference, classes, tol, LR.SURFACE_SPACING, boxes=boxes)
        for k in plain:
            assert torch.equal(_bits(given[k].contiguous()), _bits(plain[k].contiguous())), k
    # under a limit: the call needs the largest class's bytes and no more; one byte less is refused before any launch
    needs = metrics.label_map_workspace_bytes(test.shape[1:], rows)
    assert needs == [LR.workspace_bytes(test.shape[1:], [pair[k] for pair in rows]) for k in range(4)] and needs[2] == 0
    limited = metrics.label_map_surface_report(test, reference, classes, tol, LR.SURFACE_SPACING, max_workspace_bytes=max(needs))
    for k in plain:
        assert torch.equal(_bits(limited[k].contiguous()), _bits(plain[k].contiguous())), k
    with pytest.raises(ValueError, match="alone needs"):
        metrics.label_map_surface_report(test, reference, classes, tol, LR.SURFACE_SPACING, max_workspace_bytes=max(needs) - 1)
    # a 3-D pair is a batch of one; two runs give the same bits, asd included
    single = metrics.label_map_surface_report(test[1], reference[1], classes, tol, LR.SURFACE_SPACING)
    again = metrics.label_map_surface_report(test, reference, classes, tol, LR.SURFACE_SPACING)
    for k in plain:
        assert torch.equal(_bits(single[k].contiguous()), _bits(plain[k][1:].contiguous())), k
        assert torch.equal(_bits(again[k].contiguous()), _bits(plain[k].contiguous())), k


def test_argument_errors():
    test, reference = _pair(LR.SURFACE_SHAPES[0])
    with pytest.raises(ValueError, match="uint8 label map"):
        metrics.label_map_surface_report(test.int(), reference, [1], 1.0)
    with pytest.raises(ValueError, match="one shape"):
        metrics.label_map_surface_report(test, reference[0], [1], 1.0)
    with pytest.raises(ValueError, match="classes"):
        metrics.label_map_surface_report(test, reference, [], 1.0)
    with pytest.raises(ValueError, match="classes"):
        metrics.label_map_surface_report(test, reference, [64], 1.0)
    with pytest.raises(ValueError, match="connectivity"):
        metrics.label_map_surface_report(test, reference, [1], 1.0, connectivity=0)
    with pytest.raises(ValueError, match="tolerance"):
        metrics.label_map_surface_report(test, reference, [1, 2], [1.0])
    with pytest.raises(ValueError, match="boxes"):
        metrics.label_map_surface_report(test, reference, [1, 2], 1.0, boxes=[[[0, 0, 0, 1, 1, 1]]])
    with pytest.raises(ValueError, match="box outside"):
        metrics.label_map_surface_report(test, reference, [1], 1.0, boxes=[[[0, 0, 0, 99, 1, 1]], [[0, 0, 0, 1, 1, 1]]])
    with pytest.raises(RuntimeError, match="no CPU path"):
        metrics.label_map_surface_report(test.cpu(), reference.cpu(), [1], 1.0)
