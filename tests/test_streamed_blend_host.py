"""Host side of the streamed sliding-window blend (no GPU): the window count derived from the plan, the device table's rows,
the derived byte figures of tools/bench_blend.py, and the refusal of CPU tensors."""
import pytest
import torch

from diff_unet_amos_amd.inference import (_blend, _plan, blend_traffic_bytes, coverage_counts, evaluate_volume, infer,
                                          streamed_sliding_window_inference, window_table)

PLANS = [
    ((20, 17, 13), (8, 8, 8), 0.25),
    ((37, 50, 41), (16, 16, 16), 0.8),
    ((37, 50, 41), (16, 16, 16), 0.25),
    ((37, 50, 41), (16, 16, 16), 0.0),           # overlap 0: interval == roi, the last window clamped back
    ((5, 8, 11), (8, 8, 8), 0.8),                # smaller than the roi along D: padded
    ((5, 6, 7), (8, 8, 8), 0.5),                 # smaller than the roi on every axis: one window over padding
    ((8, 8, 8), (8, 8, 8), 0.25),                # image == roi
    ((16, 8, 24), (8, 8, 8), 0.0),               # a multiple of the roi at overlap 0: every voxel under exactly one window
    ((9, 16, 16), (8, 8, 8), 0.5),
    ((30, 21, 19), (12, 10, 6), 0.8),            # anisotropic roi, interval 1 along W
    ((48, 48, 40), (32, 32, 32), 0.8),
]


def _count_map_of_blend(monkeypatch, padded, roi, starts):
    """Run _blend on all-ones windows and hand back the two volumes it accumulates (sum, count): _blend returns their ratio
    only, so the two torch.zeros buffers it fills in place are recorded while it runs."""
    made = []
    zeros = torch.zeros

    def recording_zeros(*a, **kw):
        made.append(zeros(*a, **kw))
        return made[-1]

    ones = [(k, zeros(1, 1, *roi) + 1) for k in range(len(starts))]
    monkeypatch.setattr(torch, "zeros", recording_zeros)
    try:
        ratio = _blend(ones, 1, 1, padded, roi, starts, [0] * 6, padded, "cpu", torch.float32)
    finally:
        monkeypatch.undo()
    assert len(made) == 2 and made[0].shape == (1, 1, *padded) and made[1].shape == (1, 1, *padded)
    return ratio, made[0][0, 0], made[1][0, 0]


@pytest.mark.parametrize("image,roi,overlap", PLANS)
def test_coverage_product_is_the_count_map_of_blend(image, roi, overlap, monkeypatch):
    """n_d (x) n_h (x) n_w equals, exactly, the count map _blend accumulates when it runs on all-ones windows (and the sum it
    accumulates from them, which is the same map)."""
    x = torch.zeros(1, 1, *image)
    spatial, roi, padded, pad, starts = _plan(x, roi, overlap)
    cov = coverage_counts(padded, roi, starts)
    assert [len(n) for n in cov] == list(padded) and all(isinstance(v, int) for n in cov for v in n)
    nd, nh, nw = (torch.tensor(n, dtype=torch.int64) for n in cov)
    want = nd[:, None, None] * nh[None, :, None] * nw[None, None, :]
    ratio, total, count = _count_map_of_blend(monkeypatch, padded, roi, starts)
    assert count.dtype == torch.float32 and float(count.min()) >= 1          # every voxel of the padded volume is under a window
    assert torch.equal(count.to(torch.int64), want) and torch.equal(count, want.float())
    assert torch.equal(total, count) and torch.equal(ratio, torch.ones_like(ratio))


@pytest.mark.parametrize("image,roi,overlap", PLANS)
@pytest.mark.parametrize("batch", [1, 2])
def test_window_table_rows(image, roi, overlap, batch):
    x = torch.zeros(batch, 1, *image)
    spatial, roi, padded, pad, starts = _plan(x, roi, overlap)
    table = window_table(starts, batch)
    assert table.dtype == torch.int32 and tuple(table.shape) == (len(starts) * batch, 4) and table.is_contiguous()
    nwin = len(starts)
    for idx, row in enumerate(table.tolist()):
        assert row == [idx // nwin, *starts[idx % nwin]]           # window-index order, as _window / _blend decode an index
        assert 0 <= row[0] < batch
        assert all(0 <= row[1 + k] <= padded[k] - roi[k] for k in range(3))


def test_count_map_of_the_reference_test_settings():
    """240 x 240 x 180 at roi 96^3, overlap 0.8 (cfg/btcv/test.yaml:5): interval 19, 9 x 9 x 6 = 486 windows."""
    x = torch.zeros(1, 1, 1, 1, 1).expand(1, 1, 240, 240, 180)
    spatial, roi, padded, pad, starts = _plan(x, (96, 96, 96), 0.8)
    assert len(starts) == 486 and sorted({s[2] for s in starts}) == [0, 19, 38, 57, 76, 84]
    nd, nh, nw = coverage_counts(padded, roi, starts)
    assert nd == nh and max(nd) == 6 and nd[0] == 1 and nd[19] == 2 and nd[239] == 1 and sum(nd) == 9 * 96 and sum(nw) == 6 * 96


def test_derived_bytes_of_the_486_window_plan():
    """The figures tools/bench_blend.py prints, against hand values: a 16 x 96^3 fp32 window is 56 623 104 B; 486 of them are
    27 518 828 544 B; ranks that do not divide 486 gather ceil(486 / W) W windows; the fp32 sum volume is 663 552 000 B."""
    args = (486, 16, (96, 96, 96), 1, (240, 240, 180))
    window = 16 * 96 ** 3 * 4
    assert window == 56623104
    assert blend_traffic_bytes(*args, world=2) == {"gathered": 486 * window, "reduced": 663552000}
    assert blend_traffic_bytes(*args, world=2)["gathered"] == 27518828544
    assert blend_traffic_bytes(*args, world=4) == {"gathered": 488 * window, "reduced": 663552000}
    assert blend_traffic_bytes(*args, world=8) == {"gathered": 488 * window, "reduced": 663552000}
    assert blend_traffic_bytes(*args, world=8)["gathered"] == 27632074752
    assert blend_traffic_bytes(*args, world=2, window_itemsize=2)["gathered"] == 486 * window // 2
    assert blend_traffic_bytes(10, 2, (4, 4, 4), 2, (6, 5, 4), world=3) == {"gathered": 3 * 4 * 2 * 64 * 4, "reduced": 2 * 2 * 120 * 4}


def test_streamed_functions_refuse_cpu_tensors():
    """One implementation, the HIP one: no torch twin on CPU tensors."""
    vol = torch.zeros(1, 1, 8, 8, 8)
    pred = lambda x, **kw: x                                       # noqa: E731
    with pytest.raises(RuntimeError, match="runs on an MI355X"):
        streamed_sliding_window_inference(vol, (8, 8, 8), 1, pred)
    with pytest.raises(RuntimeError, match="runs on an MI355X"):
        evaluate_volume(pred, vol, None, (8, 8, 8))
    with pytest.raises(RuntimeError, match="runs on an MI355X"):
        infer(pred, vol, (8, 8, 8), streaming=True)
    assert torch.equal(infer(pred, vol, (8, 8, 8)), torch.zeros(1, 1, 8, 8, 8))      # the default path is unchanged
