"""Connected-component labelling and the keep-largest filter on the GPU (csrc/components.hip through ops.py, postprocess.py
and inference.evaluate_volume).  The work is integer-only, so every comparison is torch.equal: against the golden file that
tools/make_components_golden.py wrote from scipy.ndimage.label, or against the numpy restatement of tests/components_ref.py.
The shapes are the smallest that still reach each mechanism: W is no multiple of 64 and crosses one or two wave edges, volumes
span several 256-voxel blocks, and the numbering scan works on blocks of SCAN_BLOCK = 1024 voxels (CC_SCAN_BLOCK)."""
import os

import numpy as np
import pytest
import torch

import components_ref as CR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda", 0)
SCAN_BLOCK = 1024


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "components_golden.npz"))


def _pp():
    from diff_unet_amos_amd import postprocess
    return postprocess


def _unpack(bits, shape):
    return torch.from_numpy(np.unpackbits(bits)[:int(np.prod(shape))].reshape(shape).copy())


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a
    return t.to(DEV) if dtype is None else t.to(DEV, dtype)


def _label_strided(masks, connectivity, pad):
    """dua_cc_label on V volumes that lie ``vox + pad`` elements apart (the wrappers of ops.py always pass dense volumes):
    (labels int32 [V, D, H, W], counts int32 [V]).  The gaps are filled with 1, which must not be read as foreground."""
    from diff_unet_amos_amd import _native as nv
    V, D, H, W = masks.shape
    vox = D * H * W
    buf = torch.ones((V, vox + pad), dtype=masks.dtype, device=DEV)
    buf[:, :vox] = masks.reshape(V, vox)
    L = nv.lib()
    need = int(L.dua_cc_scratch_bytes(V, D, H, W, 1))
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    labels = torch.full((V, D, H, W), -7, dtype=torch.int32, device=DEV)
    counts = torch.full((V,), -7, dtype=torch.int32, device=DEV)
    code = nv.F32 if masks.dtype == torch.float32 else nv.U8
    nv.check(L.dua_cc_label(V, D, H, W, nv.ptr(buf), code, vox + pad, connectivity, None, nv.ptr(labels), nv.ptr(counts), nv.ptr(ws),
                            need, nv.stream_ptr()), "dua_cc_label")
    return labels, counts


@pytest.mark.parametrize("si", range(len(CR.RANDOM_SHAPES)))
@pytest.mark.parametrize("fi", range(len(CR.RANDOM_FILLS)))
def test_random_fill_labels_counts_and_sizes(golden, si, fi):
    """V = 3 volumes per call, a volume stride larger than D H W, all three connectivities."""
    pp = _pp()
    shape = (CR.RANDOM_VOLUMES, *CR.RANDOM_SHAPES[si])
    masks = _dev(_unpack(golden[f"random_s{si}_f{fi}_mask"], shape))
    for c in CR.CONNECTIVITIES:
        want = _dev(golden[f"random_s{si}_f{fi}_c{c}_labels"].astype(np.int32))
        want_counts = _dev(golden[f"random_s{si}_f{fi}_c{c}_counts"])
        want_sizes = _dev(golden[f"random_s{si}_f{fi}_c{c}_sizes"])
        labels, counts = _label_strided(masks, c, pad=37)
        assert torch.equal(counts, want_counts), (c, counts.tolist(), want_counts.tolist())
        assert torch.equal(labels, want), c
        dense, dense_counts = pp.label_components(masks, c)
        assert torch.equal(dense, want) and torch.equal(dense_counts, want_counts)
        cap = want_sizes.shape[1]
        assert torch.equal(pp.component_sizes(labels, counts, cap=cap), want_sizes)
        wide = pp.component_sizes(labels, counts, cap=cap + 5)                       # entries above the count stay 0
        assert torch.equal(wide[:, :cap], want_sizes) and int(wide[:, cap:].abs().sum()) == 0


@pytest.mark.parametrize("name", ["serpentine", "checkerboard", "isolated"])
def test_special_volumes(golden, name):
    """serpentine (8, 16, 72): one component of long thin paths, the longest parent chains the shape allows.  checkerboard
    (6, 6, 66): every foreground voxel its own component at connectivity 1 (1188 roots through the numbering scan), one
    component at 2 and 3.  isolated (6, 8, 130): single voxels whose roots fall into blocks 0, 2 and 4 of the scan."""
    pp = _pp()
    shape = tuple(int(v) for v in golden[f"{name}_shape"])
    mask = _dev(_unpack(golden[f"{name}_mask"], shape))
    nfg = int(mask.sum())
    for c in CR.CONNECTIVITIES:
        labels, count = pp.label_components(mask, c)
        assert count.shape == () and labels.shape == mask.shape
        assert int(count) == int(golden[f"{name}_c{c}_counts"][0])
        assert torch.equal(labels, _dev(golden[f"{name}_c{c}_labels"].astype(np.int32)))
        sizes = pp.component_sizes(labels, count, cap=max(int(count), 1))
        assert torch.equal(sizes, _dev(golden[f"{name}_c{c}_sizes"]))
        if name == "serpentine" or (name == "checkerboard" and c > 1):
            assert int(count) == 1 and int(sizes[0]) == nfg and torch.equal(labels, mask.int())
        if name == "isolated" or (name == "checkerboard" and c == 1):
            assert int(count) == nfg and torch.equal(labels[mask != 0], torch.arange(1, nfg + 1, dtype=torch.int32, device=DEV))
    if name == "isolated":
        blocks = torch.unique(torch.nonzero(mask.flatten()).flatten() // SCAN_BLOCK)
        assert blocks.numel() >= 3


def test_empty_full_and_corner_volumes():
    pp = _pp()
    shape = (4, 5, 70)
    both = torch.stack([torch.zeros(shape, dtype=torch.uint8), torch.ones(shape, dtype=torch.uint8)]).to(DEV)
    for c in CR.CONNECTIVITIES:
        labels, counts = pp.label_components(both, c)
        assert counts.tolist() == [0, 1] and torch.equal(labels, both.int())
        sizes = pp.component_sizes(labels, counts, cap=2)
        assert sizes.tolist() == [[0, 0], [4 * 5 * 70, 0]]
        assert torch.equal(pp.keep_largest_components(both, c), both)
        corners = _dev(CR.corners(shape))
        labels, counts = pp.label_components(corners, c)
        assert counts.tolist() == [1] * 8 and torch.equal(labels, corners.int())
        assert torch.equal(pp.keep_largest_components(corners, c, min_size=1), corners)
        assert int(pp.keep_largest_components(corners, c, min_size=2).sum()) == 0


@pytest.mark.parametrize("name", sorted(CR.FILTER_CASES))
def test_filter_cases(golden, name):
    """Equal sizes (the earlier component is kept), num_components 1 / 2 / 3, min_size equal to a size (kept) and one above
    (dropped), num_components = 0 with min_size only, and cap below the component count (the overflow rule)."""
    pp = _pp()
    make, c, k, min_size, cap = CR.FILTER_CASES[name]
    mask = _dev(make())
    want = _dev(_unpack(golden[f"filter_{name}"], tuple(mask.shape)))
    kw = {} if cap is None else {"cap": cap}
    got = pp.keep_largest_components(mask, c, k, min_size, **kw)
    assert got.dtype == torch.uint8 and torch.equal(got, want)
    if k == 0:
        assert torch.equal(pp.remove_small_components(mask, min_size, c, **kw), want)
    if cap is not None:                                       # the count still tells the whole number: the caller sees the overflow
        labels, count = pp.label_components(mask, c)
        assert int(count) > cap
        lab, n = CR.label(make(), c)
        assert torch.equal(pp.component_sizes(labels, count, cap=cap), _dev(CR.sizes(lab, cap)))


def test_mask_dtypes():
    pp = _pp()
    base = CR.random_masks(0, 1)                                                  # [3, 5, 7, 70]
    want_labels = torch.from_numpy(np.stack([CR.label(m, 2)[0] for m in base])).to(DEV)
    want_kept = _dev(CR.keep_largest_components(base, 2, 2))
    g = torch.Generator().manual_seed(5)
    values = torch.randn(base.shape, generator=g) * 3.0 + torch.where(torch.rand(base.shape, generator=g) < 0.5, 0.25, -7.0)
    values[values == 0] = 1.0
    fancy = torch.from_numpy(base).float() * values                               # foreground holds anything but 0, also negative
    for mask in (_dev(base), _dev(base).bool(), _dev(base).float(), _dev(fancy), _dev(base).long() * -3, _dev(fancy).double()):
        labels, _ = pp.label_components(mask, 2)
        assert torch.equal(labels, want_labels), mask.dtype
        assert torch.equal(pp.keep_largest_components(mask, 2, 2), want_kept), mask.dtype
    labels, _ = _label_strided(_dev(fancy), 2, pad=5)                             # fp32 through the strided entry
    assert torch.equal(labels, want_labels)


def test_channels_pass_through():
    pp = _pp()
    g = np.random.default_rng(11)
    m = (g.random((2, 4, 5, 6, 67)) < 0.3).astype(np.uint8)
    m[:, 0] *= g.integers(1, 9, size=m[:, 0].shape, dtype=np.uint8)              # the passed-through channel holds values 0 .. 8
    mask = _dev(m)
    got = pp.keep_largest_components(mask, 1, 2, channels=range(1, 4))
    assert torch.equal(got[:, 0], (mask[:, 0] != 0).to(torch.uint8))
    assert torch.equal(got, _dev(CR.keep_largest_components(m, 1, 2, channels=range(1, 4))))
    only = pp.keep_largest_components(mask, 3, 1, 2, channels=[2])
    assert torch.equal(only, _dev(CR.keep_largest_components(m, 3, 1, 2, channels=[2])))
    assert torch.equal(pp.keep_largest_components(mask, 1, 2), _dev(CR.keep_largest_components(m, 1, 2)))


def test_tallies_of_the_filter_pass():
    pp = _pp()
    from diff_unet_amos_amd import ops
    from diff_unet_amos_amd.inference import dice_per_class
    g = np.random.default_rng(3)
    B, Cn, shape = 2, 3, (5, 6, 67)
    mask = _dev((g.random((B, Cn, *shape)) < 0.4).astype(np.uint8))
    label_map = _dev(g.integers(0, Cn + 1, size=(B, *shape), dtype=np.uint8))       # value Cn: no class
    onehot = (label_map[:, None] == torch.arange(Cn, device=DEV, dtype=torch.uint8).view(1, Cn, 1, 1, 1))
    for channels in (None, [1, 2]):
        want_mask = pp.keep_largest_components(mask, 2, 3, channels=channels)
        a, b = want_mask.bool(), onehot
        want = torch.stack([(a & b).sum((0, 2, 3, 4)), a.sum((0, 2, 3, 4)), b.sum((0, 2, 3, 4))], dim=1)
        for ref in (onehot, onehot.to(torch.uint8), onehot.float() * 2.5, label_map):
            got_mask, tallies = pp.filter_components(mask, 2, 3, channels=channels, labels=ref)
            assert torch.equal(got_mask, want_mask)
            assert tallies.dtype == torch.int64 and torch.equal(tallies, want), (channels, ref.dtype, tallies.tolist(), want.tolist())
            assert torch.equal(ops.dice_from_tallies(tallies), dice_per_class(want_mask, onehot))


def _blob_case():
    """[1, 1, 12, 12, 12] image whose value c + 1 marks class c: a 3 x 3 x 3 blob and a single-voxel island per class; roi 8 with
    overlap 0.5 gives window starts (0, 4) per axis, the smallest plan with more than one window per axis.  The predictor's
    logit is +4 where the window holds c + 1 and -4 elsewhere, whatever the window, so the blend binarises to the marks."""
    Cn = 3
    image = torch.zeros(1, 1, 12, 12, 12)
    blobs = torch.zeros(1, Cn, 12, 12, 12)
    for c, (z, y, x) in enumerate(((1, 1, 1), (5, 6, 2), (8, 2, 7))):
        image[0, 0, z:z + 3, y:y + 3, x:x + 3] = c + 1
        blobs[0, c, z:z + 3, y:y + 3, x:x + 3] = 1
    for c, (z, y, x) in enumerate(((10, 10, 10), (0, 11, 5), (3, 9, 11))):
        image[0, 0, z, y, x] = c + 1

    def predictor(x, pred_type=None):
        return torch.cat([(x == c + 1).float() * 8.0 - 4.0 for c in range(Cn)], dim=1)

    return image.to(DEV), blobs.to(DEV), predictor


def test_evaluate_volume_with_postprocess():
    pp = _pp()
    from diff_unet_amos_amd.inference import dice_per_class, evaluate_volume, infer
    image, blobs, predictor = _blob_case()
    args = (predictor, image, blobs, (8, 8, 8), 2, 0.5)
    plain_mask, plain_dice = evaluate_volume(*args)
    assert int(plain_mask.sum()) == 3 * 28                                          # blob and island of every class
    none_mask, none_dice = evaluate_volume(*args, postprocess=None)
    assert torch.equal(none_mask, plain_mask) and torch.equal(none_dice, plain_dice)
    kw = dict(connectivity=1, num_components=1)
    mask, dice = evaluate_volume(*args, postprocess=kw)
    assert mask.dtype == torch.uint8 and torch.equal(mask, pp.keep_largest_components(plain_mask, **kw))
    assert torch.equal(mask, blobs.to(torch.uint8))
    assert torch.equal(dice, dice_per_class(mask, blobs)) and dice.tolist() == [1.0, 1.0, 1.0]
    assert all(d < 1.0 for d in plain_dice.tolist())
    # the label-map form: class c = channel c, 3 = no class
    marks = (blobs * torch.arange(1, 4, device=DEV).view(1, 3, 1, 1, 1)).sum(1)
    shifted = torch.where(marks == 0, torch.full_like(marks, 3.0), marks - 1).to(torch.uint8)
    _, dice_m = evaluate_volume(predictor, image, shifted, (8, 8, 8), 2, 0.5, postprocess=kw)
    assert torch.equal(dice_m, dice)
    only12 = evaluate_volume(*args, postprocess=dict(channels=[1, 2]))[0]
    assert torch.equal(only12[:, 0], plain_mask[:, 0]) and torch.equal(only12[:, 1:], blobs[:, 1:].to(torch.uint8))
    # infer: fp32, streamed or not
    for streaming in (True, False):
        out = infer(predictor, image, (8, 8, 8), 2, 0.5, streaming=streaming, postprocess=kw)
        assert out.dtype == torch.float32 and torch.equal(out, blobs)
        assert torch.equal(infer(predictor, image, (8, 8, 8), 2, 0.5, streaming=streaming), plain_mask.float())


def test_graph_capture_and_replay():
    """label_components and keep_largest_components read nothing back: captured once on a single stream, replayed on a second
    input, they give the eager result."""
    pp = _pp()
    first, second = _dev(CR.random_masks(0, 1)), _dev(CR.random_masks(0, 2))
    static = first.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                              # warm-up outside the capture: library load, allocator
        pp.label_components(static, 2)
        pp.keep_largest_components(static, 2, 2, channels=None)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        labels, counts = pp.label_components(static, 2)
        kept = pp.keep_largest_components(static, 2, 2, min_size=3)
    for mask in (first, second):
        static.copy_(mask)
        graph.replay()
        want_labels, want_counts = pp.label_components(mask, 2)
        assert torch.equal(labels, want_labels) and torch.equal(counts, want_counts)
        assert torch.equal(kept, pp.keep_largest_components(mask, 2, 2, min_size=3))
    assert torch.equal(labels, torch.from_numpy(np.stack([CR.label(m, 2)[0] for m in CR.random_masks(0, 2)])).to(DEV))
