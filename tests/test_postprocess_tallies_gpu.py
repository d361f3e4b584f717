"""The Dice tallies of the four tallying post-processing entry points -- ``filter_components``, ``fill_holes``,
``filter_label_map``, ``fill_holes_in_label_map`` -- on the GPU: the int64 [C, 3] table each returns equals (|A & B|, |A|, |B|)
recomputed with torch operators from the mask or map it returned with it.  Integers only: every comparison is exact.

The extents put the edges of the tally passes (1024 voxels per workgroup, 64 per wave) inside the volume: [3, 5, 67] is 1005
voxels, one block with a ragged last wave; [5, 15, 23] is 1725, a full block and a partial one.  C = 1 is class 0 alone (the
register path of the map form), 3 a handful of LDS words, 64 all of them.  Maps and map references hold the values C and C + 1,
which must count nowhere."""
import pytest
import torch

from diff_unet_amos_amd import postprocess

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BATCH = 2
EXTENTS = [(3, 5, 67), (5, 15, 23)]
CLASSES = [1, 3, 64]


def _maps(C, ext, seed):
    """uint8 [BATCH, *ext]: blocks of 3 x 3 x 4 voxels of one value in 0 .. C + 1, with single voxels punched to 0 (pockets inside
    a block are holes of one class; a value >= C is no class)."""
    g = torch.Generator().manual_seed(seed)
    coarse = torch.randint(0, C + 2, (BATCH, -(-ext[0] // 3), -(-ext[1] // 3), -(-ext[2] // 4)), generator=g)
    full = coarse.repeat_interleave(3, 1).repeat_interleave(3, 2).repeat_interleave(4, 3)[:, :ext[0], :ext[1], :ext[2]]
    full = torch.where(torch.rand(full.shape, generator=g) < 0.08, torch.zeros_like(full), full)
    full[:, 0, 0, :2], full[:, -1, -1, -2:] = C, C + 1                # whatever was drawn, both are there
    return full.to(torch.uint8).contiguous().to(DEV)


def _masks(C, ext, seed, density=0.7):
    """uint8 [BATCH, C, *ext] of independent voxels.  70 % foreground is one body with enclosed single-voxel holes, for the fill;
    35 %, just above the lattice's percolation threshold, is many components per volume, for the filter."""
    g = torch.Generator().manual_seed(seed)
    return (torch.rand((BATCH, C, *ext), generator=g) < density).to(torch.uint8).to(DEV)


def _class_axis(C):
    return torch.arange(C, device=DEV).view(1, C, 1, 1, 1)


def _tallies(a, b):
    """int64 [C, 3] = (|A & B|, |A|, |B|) per class of bool [B, C, D, H, W] tensors."""
    dims = (0, 2, 3, 4)
    return torch.stack([(a & b).sum(dims), a.sum(dims), b.sum(dims)], dim=1)


def _pass_one_through(C, low):
    """The selections of a case: everything, and -- where there is more than one to choose from -- all but the last."""
    return [None] if C - low < 2 else [None, tuple(range(low, C - 1))]


@pytest.mark.parametrize("ext", EXTENTS, ids=lambda e: "x".join(map(str, e)))
@pytest.mark.parametrize("C", CLASSES)
def test_the_mask_forms_tally_the_mask_they_return(C, ext):
    mask, sparse = _masks(C, ext, 11 * C + ext[2]), _masks(C, ext, 7 * C + ext[2], 0.35)
    onehot = _masks(C, ext, 13 * C + ext[0]) != 0
    ref_map = _maps(C, ext, 17 * C + ext[1])
    assert bool((ref_map >= C).any())
    references = [(onehot.float(), onehot), (onehot.to(torch.uint8), onehot), (onehot, onehot), (ref_map, ref_map[:, None] == _class_axis(C))]
    for channels in _pass_one_through(C, 0):
        for labels, b in references:
            out, tallies = postprocess.filter_components(sparse, num_components=1, min_size=2, channels=channels, labels=labels)
            assert out.dtype == torch.uint8 and out.shape == mask.shape and tallies.dtype == torch.int64
            assert torch.equal(tallies, _tallies(out != 0, b)), (C, ext, channels, labels.dtype, "filter_components")
            again = postprocess.filter_components(sparse, num_components=1, min_size=2, channels=channels, labels=labels)
            assert torch.equal(again[0], out) and torch.equal(again[1], tallies)
            assert 0 < int(out.sum()) < int(sparse.sum())                            # the filter kept something and dropped something
            for m in (mask, mask.float()):                                           # the uint8 and the fp32 fill kernel
                filled_mask, filled, tallies = postprocess.fill_holes(m, channels=channels, labels=labels)
                assert filled_mask.dtype == m.dtype and tallies.dtype == torch.int64
                assert torch.equal(tallies, _tallies(filled_mask != 0, b)), (C, ext, channels, labels.dtype, m.dtype, "fill_holes")
                assert torch.equal(filled, ((filled_mask != 0).sum((2, 3, 4)) - (mask != 0).sum((2, 3, 4))))
                assert int(filled.sum()) > 0                                         # something was filled
                again = postprocess.fill_holes(m, channels=channels, labels=labels)
                assert all(torch.equal(x, y) for x, y in zip(again, (filled_mask, filled, tallies)))
            if channels is not None:                                                 # the last channel passed through both
                assert torch.equal(out[:, -1], sparse[:, -1]) and torch.equal(filled_mask[:, -1], m[:, -1]) and int(filled[:, -1].sum()) == 0


@pytest.mark.parametrize("ext", EXTENTS, ids=lambda e: "x".join(map(str, e)))
@pytest.mark.parametrize("C", CLASSES)
def test_the_map_forms_tally_the_map_they_return(C, ext):
    label_map = _maps(C, ext, 19 * C + ext[2])
    reference = _maps(C, ext, 23 * C + ext[0])
    assert bool((label_map >= C).any()) and bool((reference >= C).any()) and bool((label_map == 0).any())
    b = reference[:, None] == _class_axis(C)
    before = (label_map[:, None] == _class_axis(C)).sum((0, 2, 3, 4))
    for classes in _pass_one_through(C, 1):
        out, tallies = postprocess.filter_label_map(label_map, C, connectivity=1, num_components=1, min_size=2, classes=classes,
                                                    reference=reference)
        assert out.dtype == torch.uint8 and out.shape == label_map.shape and tallies.dtype == torch.int64
        assert torch.equal(tallies, _tallies(out[:, None] == _class_axis(C), b)), (C, ext, classes, "filter_label_map")
        assert torch.equal(out[label_map >= C], label_map[label_map >= C])           # no class: passed through, counted nowhere
        again = postprocess.filter_label_map(label_map, C, connectivity=1, num_components=1, min_size=2, classes=classes,
                                             reference=reference)
        assert torch.equal(again[0], out) and torch.equal(again[1], tallies)
        filled_map, filled, ftallies = postprocess.fill_holes_in_label_map(label_map, C, classes=classes, reference=reference)
        after = (filled_map[:, None] == _class_axis(C)).sum((0, 2, 3, 4))
        assert torch.equal(ftallies, _tallies(filled_map[:, None] == _class_axis(C), b)), (C, ext, classes, "fill_holes_in_label_map")
        assert torch.equal(filled[1:], (after - before)[1:]) and int(filled[0]) == 0
        again = postprocess.fill_holes_in_label_map(label_map, C, classes=classes, reference=reference)
        assert all(torch.equal(x, y) for x, y in zip(again, (filled_map, filled, ftallies)))
        if C > 1:
            assert int((out != label_map).sum()) > 0 and int(filled.sum()) > 0       # both passes changed the map
        if classes is not None:                                                      # class C - 1 passed through both
            assert torch.equal(out == C - 1, label_map == C - 1) and int(filled[C - 1]) == 0
