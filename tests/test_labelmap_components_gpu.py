"""Components of a label map on the GPU (csrc/components.hip: dua_cc_label_map, dua_cc_filter_map; postprocess.label_map_components,
filter_label_map, keep_largest_in_label_map) against three witnesses, all with torch.equal: the existing one-hot path
(label_components / keep_largest_components on the expansion), the scipy golden file and the numpy restatement
(tests/labelmap_eval_ref.py).  The maps are the smallest that reach each mechanism: W = 67 and 130 cross one and two wave edges
of a row, 6 x 8 x 130 spans several 1024-voxel scan blocks, the checkerboard makes every run one voxel long, the serpentine is
one long component inside another class; N = 2 throughout."""
import os

import numpy as np
import pytest
import torch

import labelmap_eval_ref as LR
from diff_unet_amos_amd import ops
from diff_unet_amos_amd import postprocess as pp

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "labelmap_eval_golden.npz")
VALUES = LR.C + 2


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _unpack(bits, shape):
    onehot = np.unpackbits(bits)[:VALUES * int(np.prod(shape))].reshape(VALUES, *shape)
    return onehot.argmax(axis=0).astype(np.uint8)


def _expand(maps, classes=LR.C):
    """uint8 [N, C, D, H, W]: the one-hot tensor the label-map form avoids."""
    return (maps[:, None] == torch.arange(classes, device=maps.device, dtype=maps.dtype).view(1, -1, 1, 1, 1)).to(torch.uint8)


def _restrict(labels, maps, c):
    """The joint labels on (maps == c), renumbered 1, 2, ... in increasing order per map, and their number."""
    out, counts = torch.zeros_like(labels), []
    for n in range(maps.shape[0]):
        x = torch.where(maps[n] == c, labels[n], torch.zeros_like(labels[n]))
        values = torch.unique(x[x > 0])
        out[n][x > 0] = (torch.searchsorted(values, x[x > 0]) + 1).to(labels.dtype)
        counts.append(values.numel())
    return out, torch.tensor(counts, dtype=torch.int32, device=labels.device)


@pytest.mark.parametrize("conn", LR.CONNECTIVITIES)
@pytest.mark.parametrize("name", sorted(LR.MAPS))
def test_labels_against_the_expansion_the_golden_file_and_the_restatement(golden, name, conn):
    host = LR.MAPS[name]()
    maps = _dev(host)
    labels, count = pp.label_map_components(maps, LR.C, conn)
    assert labels.dtype == torch.int32 and labels.shape == maps.shape and count.dtype == torch.int32 and tuple(count.shape) == (2,)
    want_labels, want_count = pp.label_components(_expand(maps), conn)                  # [N, C, D, H, W], [N, C]
    assert torch.equal(count, want_count[:, 1:].sum(1).to(torch.int32))
    for c in range(1, LR.C):
        mine, k = _restrict(labels, maps, c)
        assert torch.equal(mine, want_labels[:, c]) and torch.equal(k, want_count[:, c])
        assert torch.equal(mine, _dev(golden[f"{name}_c{conn}_labels"][:, c].astype(np.int32)))
    ref = np.stack([LR.label_map(m, LR.C, conn)[0] for m in host])
    assert torch.equal(labels, _dev(ref))                                               # the joint numbering itself
    assert not labels[(maps == 0) | (maps >= LR.C)].any()
    one = pp.label_map_components(maps[1], LR.C, conn)                                   # a single map [D, H, W]
    assert torch.equal(one[0], labels[1]) and one[1].dim() == 0 and int(one[1]) == int(count[1])


def test_checkerboard_counts():
    maps = _dev(LR.checkerboard_maps())
    assert pp.label_map_components(maps, LR.C, 1)[1].tolist() == [maps[0].numel()] * 2
    assert pp.label_map_components(maps, LR.C, 2)[1].tolist() == [2, 2]
    assert pp.label_map_components(maps, LR.C, 3)[1].tolist() == [2, 2]


def test_sizes_are_those_of_the_expansion():
    maps = _dev(LR.random_maps(1))
    labels, count = pp.label_map_components(maps, LR.C, 1)
    cap = int(count.max())
    sizes = pp.component_sizes(labels, count, cap)
    want_labels, want_count = pp.label_components(_expand(maps), 1)
    want = pp.component_sizes(want_labels, want_count, cap)                              # [N, C, cap]
    for n in range(2):
        cls = torch.tensor(LR.label_map(maps[n].cpu().numpy(), LR.C, 1)[2].astype(np.int64), device=DEV)
        for c in range(1, LR.C):
            k = int(want_count[n, c])
            assert torch.equal(sizes[n, :int(count[n])][cls == c], want[n, c, :k])


@pytest.mark.parametrize("case", sorted(LR.FILTER_CASES))
def test_filter_against_the_expansion_the_golden_file_and_the_restatement(golden, case):
    maker, conn, k, min_size, classes = LR.FILTER_CASES[case]
    host = LR.MAPS[maker]()
    maps = _dev(host)
    out, tallies = pp.filter_label_map(maps, LR.C, conn, k, min_size, classes)
    assert tallies is None and out.dtype == torch.uint8 and out.shape == maps.shape
    assert torch.equal(out, _dev(_unpack(golden[f"filter_{case}"], host.shape)))
    assert torch.equal(out, _dev(np.stack([LR.filter_map(m, LR.C, conn, k, min_size, classes) for m in host])))
    kept = pp.keep_largest_components(_expand(maps), conn, k, min_size, channels=range(1, LR.C) if classes is None else classes)
    for c in range(1, LR.C):
        assert torch.equal((out == c).to(torch.uint8), kept[:, c])
    assert torch.equal(out[maps >= LR.C], maps[maps >= LR.C]) and torch.equal(out == 0, (maps == 0) | ((maps < LR.C) & (kept.sum(1) == 0)))
    assert torch.equal(pp.keep_largest_in_label_map(maps, LR.C, conn, k, min_size, classes), out)


def test_tallies_against_a_reference_map():
    maps = _dev(LR.touching_maps())
    test, reference = maps[:1], maps[1:]
    out, tallies = pp.filter_label_map(test, LR.C, 1, 1, 0, reference=reference)
    want = _dev(LR.tallies(out.cpu().numpy(), reference.cpu().numpy(), LR.C))
    assert tallies.dtype == torch.int64 and torch.equal(tallies, want)
    # the existing path on the expansion gives the same tallies for the classes it filters
    _, old = pp.filter_components(_expand(test), 1, 1, 0, channels=range(1, LR.C), labels=reference)
    assert torch.equal(tallies[1:], old[1:])
    assert torch.equal(ops.dice_from_tallies(tallies)[1:], ops.dice_from_tallies(old)[1:])
    # a batch of two maps sums over the batch, and a 3-D map is a batch of one
    both, t2 = pp.filter_label_map(maps, LR.C, 1, 1, 0, reference=maps.flip(0))
    assert torch.equal(t2, _dev(LR.tallies(both.cpu().numpy(), maps.flip(0).cpu().numpy(), LR.C)))
    single, t1 = pp.filter_label_map(test[0], LR.C, 1, 1, 0, reference=reference[0])
    assert torch.equal(single, out[0]) and torch.equal(t1, tallies)


def test_cap_overflow_drops_the_labels_above_it():
    host = LR.touching_maps()
    maps = _dev(host)
    labels, count = pp.label_map_components(maps, LR.C, 1)
    assert count.tolist() == [6, 4]
    out = pp.keep_largest_in_label_map(maps, LR.C, 1, 0, 0, cap=3)
    assert torch.equal(out, _dev(np.stack([LR.filter_map(m, LR.C, 1, 0, 0, None, cap=3) for m in host])))
    assert not out[labels > 3].any() and torch.equal(out[labels <= 3], maps[labels <= 3])
    sizes = pp.component_sizes(labels, count, 3)
    assert torch.equal(sizes, _dev(np.stack([LR.CR.sizes(LR.label_map(m, LR.C, 1)[0], 3) for m in host])))


def test_empty_and_single_class_maps():
    empty = torch.zeros((2, 5, 6, 67), dtype=torch.uint8, device=DEV)
    labels, count = pp.label_map_components(empty, LR.C, 3)
    assert not labels.any() and count.tolist() == [0, 0]
    out, tallies = pp.filter_label_map(empty, LR.C, reference=empty)
    assert not out.any() and tallies.tolist() == [[2 * 5 * 6 * 67] * 3] + [[0, 0, 0]] * (LR.C - 1)
    full = torch.full((2, 5, 6, 67), 3, dtype=torch.uint8, device=DEV)
    labels, count = pp.label_map_components(full, LR.C, 1)
    assert count.tolist() == [1, 1] and bool((labels == 1).all())
    assert torch.equal(pp.keep_largest_in_label_map(full, LR.C), full)
    assert not pp.keep_largest_in_label_map(full, LR.C, min_size=5 * 6 * 67 + 1).any()
    large = torch.full((2, 5, 6, 67), LR.C, dtype=torch.uint8, device=DEV)                # every value >= C: nothing to label
    assert pp.label_map_components(large, LR.C)[1].tolist() == [0, 0] and torch.equal(pp.keep_largest_in_label_map(large, LR.C), large)
    assert pp.label_map_components(full, 3)[1].tolist() == [0, 0]                          # 3 is >= num_classes = 3


def test_two_runs_give_identical_bits():
    maps = _dev(LR.random_maps(1))
    a = pp.label_map_components(maps, LR.C, 3)
    b = pp.label_map_components(maps, LR.C, 3)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    fa, ta = pp.filter_label_map(maps, LR.C, 2, 2, 3, reference=maps.flip(0))
    fb, tb = pp.filter_label_map(maps, LR.C, 2, 2, 3, reference=maps.flip(0))
    assert torch.equal(fa, fb) and torch.equal(ta, tb)


def test_graph_capture_and_replay():
    """Nothing is read back: captured once on a single stream, replayed on a second input, the functions give the eager result."""
    first, second = _dev(LR.random_maps(0)), _dev(LR.random_maps(0)).flip(0).contiguous()
    static, ref = first.clone(), first.flip(-1).contiguous()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                              # warm-up outside the capture: library load, allocator
        pp.label_map_components(static, LR.C, 2)
        pp.filter_label_map(static, LR.C, 2, 1, 2, classes=(1, 3), reference=ref)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        labels, counts = pp.label_map_components(static, LR.C, 2)
        kept, tallies = pp.filter_label_map(static, LR.C, 2, 1, 2, classes=(1, 3), reference=ref)
    for maps in (first, second):
        static.copy_(maps)
        graph.replay()
        want_labels, want_counts = pp.label_map_components(maps, LR.C, 2)
        assert torch.equal(labels, want_labels) and torch.equal(counts, want_counts)
        want_kept, want_tallies = pp.filter_label_map(maps, LR.C, 2, 1, 2, classes=(1, 3), reference=ref)
        assert torch.equal(kept, want_kept) and torch.equal(tallies, want_tallies)
    assert torch.equal(kept, _dev(np.stack([LR.filter_map(m, LR.C, 2, 1, 2, (1, 3)) for m in second.cpu().numpy()])))


def test_argument_errors():
    maps = _dev(LR.random_maps(0))
    with pytest.raises(ValueError, match="uint8 label map"):
        pp.label_map_components(maps.int(), LR.C)
    with pytest.raises(ValueError, match="num_classes"):
        pp.label_map_components(maps, 65)
    with pytest.raises(ValueError, match="connectivity"):
        pp.label_map_components(maps, LR.C, 4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        pp.label_map_components(maps.cpu(), LR.C)
    with pytest.raises(ValueError, match="classes must lie"):
        pp.filter_label_map(maps, LR.C, classes=(0,))
    with pytest.raises(ValueError, match="classes must lie"):
        pp.filter_label_map(maps, LR.C, classes=(LR.C,))
    with pytest.raises(ValueError, match="reference"):
        pp.filter_label_map(maps, LR.C, reference=maps[0])
    with pytest.raises(ValueError, match="cap"):
        pp.filter_label_map(maps, LR.C, cap=0)
