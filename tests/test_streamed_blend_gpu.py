"""The streamed sliding-window blend on the GPU (csrc/blend.hip): bit-equality with the list-and-blend path, mask and Dice of the
fused finish pass, the two-rank all-reduce form against an fp64 blend, peak memory, argument errors."""
import ctypes as C
import os
import socket
import subprocess
import sys

import pytest
import torch

from diff_unet_amos_amd.inference import (_plan, _window, binarise, coverage_counts, dice_per_class, evaluate_volume, infer,
                                          sliding_window_inference, streamed_sliding_window_inference, window_table)
from streamed_blend_stub import CHANNELS, MARKER, RANK_CASES, make_predictor, seeded_volume

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAND = 2.0 ** -20        # fp32 sigmoid(q) cannot exceed 0.5 below about 2^-23; the band allows for exp rounding
BAND_CAP = 1e-4          # at most this fraction of voxels may lie inside the band


@pytest.mark.parametrize("shape,roi,overlap,swb", [
    ((1, 1, 37, 50, 41), (16, 16, 16), 0.8, 1),      # ragged, 1040 windows, every W start at another alignment
    ((1, 1, 37, 50, 41), (16, 16, 16), 0.8, 4),      # overlapping windows inside one call
    ((2, 1, 37, 50, 41), (16, 16, 16), 0.25, 3),     # batch of two volumes, a call that spans both
    ((1, 1, 37, 50, 41), (16, 16, 16), 0.25, 4),
    ((1, 1, 5, 8, 11), (8, 8, 8), 0.8, 3),           # smaller than the roi along D: padded, cropped by the finish pass
    ((2, 1, 9, 16, 16), (8, 8, 8), 0.5, 4),
    ((1, 1, 32, 32, 48), (16, 16, 16), 0.5, 4),      # nothing cropped, planes a multiple of 4 voxels: the 16-byte finish pass
    ((1, 1, 8, 8, 8), (8, 8, 8), 0.25, 2),           # exactly one window
])
def test_streamed_equals_the_list_and_blend_path_bit_for_bit(shape, roi, overlap, swb):
    """The same fp32 additions in the same order and an exact integer count: torch.equal, not a tolerance.  Two runs agree
    bit for bit."""
    dev = torch.device("cuda", 0)
    pred = make_predictor(roi, dev)
    vol = seeded_volume(shape).to(dev)
    want = sliding_window_inference(vol, roi, swb, pred, overlap, pred_type="ddim_sample")
    got = streamed_sliding_window_inference(vol, roi, swb, pred, overlap, pred_type="ddim_sample")
    assert got.shape == want.shape == (shape[0], CHANNELS, *shape[2:]) and got.dtype == torch.float32
    diff = (got - want).abs()
    print(f"streamed vs list-and-blend {shape} roi {roi} overlap {overlap} swb {swb}: mismatching voxels "
          f"{int((got != want).sum())}, max |d| {float(diff.max()):.3e}")
    assert torch.equal(got, want)
    again = streamed_sliding_window_inference(vol, roi, swb, pred, overlap, pred_type="ddim_sample")
    assert torch.equal(again, got)


def test_fp16_windows_are_widened_then_added_in_fp32():
    """gather_dtype only narrows the window tensor handed to the accumulate call: the result is the fp32 blend of the rounded
    windows, as the gather form's ``.float()`` gives it."""
    dev = torch.device("cuda", 0)
    shape, roi, overlap, swb = (1, 1, 37, 50, 41), (16, 16, 16), 0.8, 4
    pred = make_predictor(roi, dev)
    rounded = lambda x, **kw: pred(x, **kw).half().float()         # noqa: E731
    vol = seeded_volume(shape).to(dev)
    want = sliding_window_inference(vol, roi, swb, rounded, overlap, pred_type="ddim_sample")
    got = streamed_sliding_window_inference(vol, roi, swb, pred, overlap, gather_dtype=torch.float16, pred_type="ddim_sample")
    assert torch.equal(got, want)


def _planted_case(dev):
    """32 x 32 x 48 at roi 32^3, overlap 0.5: two windows, W starts 0 and 16, both over w in [16, 32).  The second input channel
    carries +1 below w = 16 and -1 from there on, so the two windows have signs +1 and -1; five voxels of the overlap carry the
    MARKER value: channel 0 receives +3 and -3 there and blends to exactly 0."""
    shape, roi, overlap = (1, 2, 32, 32, 48), (32, 32, 32), 0.5
    vol = seeded_volume(shape, seed=77)
    vol[:, 1] = 1.0
    vol[:, 1, :, :, 16:] = -1.0
    planted = [(3, 4, 17), (10, 20, 16), (31, 0, 31), (16, 16, 24), (0, 31, 20)]
    for d, h, w in planted:
        vol[0, 0, d, h, w] = MARKER
    return vol.to(dev), roi, overlap, planted


@pytest.mark.parametrize("case", ["planted", "ragged", "padded_batch"])
def test_mask_and_dice_of_the_finish_pass(case):
    dev = torch.device("cuda", 0)
    planted = []
    if case == "planted":
        vol, roi, overlap, planted = _planted_case(dev)
        swb = 2
    elif case == "ragged":
        roi, overlap, swb = (16, 16, 16), 0.8, 4
        vol = seeded_volume((1, 1, 37, 50, 41)).to(dev)
    else:
        roi, overlap, swb = (8, 8, 8), 0.5, 4
        vol = seeded_volume((2, 1, 9, 16, 6)).to(dev)
    pred = make_predictor(roi, dev, planted=bool(planted))
    q = sliding_window_inference(vol, roi, swb, pred, overlap, pred_type="ddim_sample")          # the existing path alone
    want = binarise(q)
    in_band = q.abs() <= BAND
    frac = float(in_band.float().mean())
    print(f"{case}: {int(in_band.sum())} of {q.numel()} voxels inside |q| <= 2^-20 ({frac:.3e}); exact zeros {int((q == 0).sum())}")
    assert frac <= BAND_CAP                                        # a condition on the stub, checked on the existing path
    B, D, H, W = vol.shape[0], *vol.shape[2:]
    g = torch.Generator().manual_seed(5)
    onehot = (torch.rand(B, CHANNELS, D, H, W, generator=g) > 0.6).float()
    onehot[:, CHANNELS - 1] = 0                                    # an empty class on both sides: Dice 0
    onehot = onehot.to(dev)
    label_map = torch.randint(0, CHANNELS - 1, (B, D, H, W), generator=g).to(torch.uint8).to(dev)
    map_onehot = (label_map[:, None] == torch.arange(CHANNELS, device=dev).view(1, -1, 1, 1, 1)).float()

    mask, dice = evaluate_volume(pred, vol, onehot, roi, swb, overlap)
    assert mask.dtype == torch.uint8 and mask.shape == want.shape and dice.dtype == torch.float64 and dice.shape == (CHANNELS,)
    assert int(mask.max()) <= 1
    differ = (mask.float() != want) & ~in_band
    print(f"{case}: mask differs from binarise at {int(differ.sum())} voxels outside the band, "
          f"{int(((mask.float() != want) & in_band).sum())} inside")
    assert not bool(differ.any())
    for d, h, w in planted:                                        # q == 0 exactly: 0 in both
        assert float(q[0, 0, d, h, w]) == 0.0 and int(mask[0, 0, d, h, w]) == 0 and float(want[0, 0, d, h, w]) == 0.0
    assert bool(((q == 0) <= (mask == 0)).all())
    # tallies, and hence Dice, against dice_per_class on the kernel's OWN mask: exact
    assert torch.equal(dice, dice_per_class(mask.float(), onehot))
    assert float(dice[CHANNELS - 1]) == 0.0 and int(mask[:, CHANNELS - 1].sum()) == 0
    assert float(dice[:CHANNELS - 1].min()) > 0.0
    mask_u8, dice_u8 = evaluate_volume(pred, vol, onehot.bool(), roi, swb, overlap)              # one-hot as bool / uint8
    assert torch.equal(mask_u8, mask) and torch.equal(dice_u8, dice)
    mask_m, dice_m = evaluate_volume(pred, vol, label_map, roi, swb, overlap)                    # the label-map form
    assert torch.equal(mask_m, mask)
    assert torch.equal(dice_m, dice_per_class(mask.float(), map_onehot)) and float(dice_m[CHANNELS - 1]) == 0.0
    # the counts themselves
    from diff_unet_amos_amd import ops
    spatial, roi_, padded, pad, starts = _plan(vol, roi, overlap)
    acc = torch.zeros(B, CHANNELS, *padded, device=dev)
    table = window_table(starts, B, dev)
    x = torch.nn.functional.pad(vol, pad)
    for i in range(len(starts) * B):
        ops.blend_accumulate(acc, pred(_window(x, i, len(starts), starts, roi_)), table, i)
    cov = [torch.tensor(n, dtype=torch.int32, device=dev) for n in coverage_counts(padded, roi_, starts)]
    lo = tuple(pad[2 * (2 - k)] for k in range(3))
    q2, mask2, tallies = ops.blend_finish(acc, cov, lo, spatial, want_q=True, want_mask=True, labels=label_map)
    assert torch.equal(q2, q) and torch.equal(mask2, mask)
    a, b = mask.bool(), map_onehot.bool()
    want_t = torch.stack([(a & b).sum((0, 2, 3, 4)), a.sum((0, 2, 3, 4)), b.sum((0, 2, 3, 4))], dim=1)
    assert tallies.dtype == torch.int64 and torch.equal(tallies, want_t)
    # infer(streaming=True) is the mask as fp32
    assert torch.equal(infer(pred, vol, roi, swb, overlap, streaming=True), mask.float())


def _fp64_blend(vol, roi, overlap, pred):
    """fp64 blend of the same windows on the CPU (the stub gives the same bits there): (sum / count, sum of |o|, count)."""
    spatial, roi, padded, pad, starts = _plan(vol, roi, overlap)
    x = torch.nn.functional.pad(vol, pad)
    B, nwin = vol.shape[0], len(starts)
    total = torch.zeros(B, CHANNELS, *padded, dtype=torch.float64)
    mag = torch.zeros_like(total)
    cnt = torch.zeros(1, 1, *padded, dtype=torch.float64)
    for i in range(nwin * B):
        b, (d, h, w) = i // nwin, starts[i % nwin]
        o = pred(_window(x, i, nwin, starts, roi)).double()
        sl = (slice(b, b + 1), slice(None), slice(d, d + roi[0]), slice(h, h + roi[1]), slice(w, w + roi[2]))
        total[sl] += o
        mag[sl] += o.abs()
        if b == 0:
            cnt[(slice(None), slice(None)) + sl[2:]] += 1
    crop = (slice(None), slice(None)) + tuple(slice(pad[2 * (2 - k)], pad[2 * (2 - k)] + spatial[k]) for k in range(3))
    return (total / cnt)[crop], mag[crop], cnt.expand_as(total)[crop]


def test_two_ranks_all_reduce_against_an_fp64_blend(tmp_path):
    """Two ranks over gloo sharing device 0, started as bench.py starts its ranks, under a time limit of their own.  The
    all-reduced blend adds each voxel's cnt windows in another order than one process does: cnt - 1 fp32 additions, so
      |sum_fp32 - sum| <= (cnt - 1) 2^-24 sum|o_i| (1 + 2^-10)     (gamma_{cnt-1} <= (cnt - 1) u (1 + 2^-10) for cnt <= 2^13)
    and one correctly rounded division follows: |q - q64| <= that bound / cnt + ulp(q).  The reference is an fp64 blend of the
    same windows, not the code under test.  Masks agree with the single-process mask outside the 2^-20 band.  The third case
    has one window for two ranks."""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "tests", "streamed_blend_stub.py"), str(tmp_path)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=420)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    dev = torch.device("cuda", 0)
    for k, (shape, roi, overlap, swb) in enumerate(RANK_CASES):
        got = torch.load(os.path.join(tmp_path, f"case{k}.pt"))
        assert got["world"] == 2 and got["same_on_every_rank"]
        vol = seeded_volume(shape)
        q64, mag, cnt = _fp64_blend(vol, roi, overlap, make_predictor(roi, "cpu"))
        bound = (cnt - 1) * 2.0 ** -24 * mag * (1 + 2.0 ** -10) / cnt + 2.0 ** -23 * q64.abs() + 2.0 ** -149
        err = (got["q"].double() - q64).abs()
        print(f"two ranks, case {k} {shape}: max |q - q64| {float(err.max()):.3e}, max err / bound {float((err / bound).max()):.3f}, "
              f"max count {int(cnt.max())}, all_reduce {got['timings']['all_reduce_s']:.4f} s of {got['timings']['reduced_bytes']} B")
        assert bool((err <= bound).all())
        padded = _plan(vol, roi, overlap)[2]
        assert got["timings"]["reduced_bytes"] == shape[0] * CHANNELS * padded[0] * padded[1] * padded[2] * 4
        single, _ = evaluate_volume(make_predictor(roi, dev), vol.to(dev), None, roi, swb, overlap)
        outside = (q64.abs() > BAND)
        assert float((~outside).float().mean()) <= BAND_CAP
        assert torch.equal(got["mask"][outside], single.cpu()[outside])


def test_streamed_peak_memory_stays_near_the_sum_volume():
    """343 windows of 4 x 16^3 (64 KiB each, 21.4 MiB in all).  The streamed path allocates the padded input copy, the sum
    volume and, per call, the window batch and what the predictor makes of it: above the inputs its peak stays below the sum
    volume plus four predictor batches, and below half of nwin * window_bytes, which the list-and-blend path exceeds by
    construction (it holds every window)."""
    dev = torch.device("cuda", 0)
    shape, roi, overlap, swb = (1, 1, 40, 40, 40), (16, 16, 16), 0.75, 4
    pred = make_predictor(roi, dev)
    vol = seeded_volume(shape).to(dev)
    nwin = len(_plan(vol, roi, overlap)[4])
    assert nwin == 343
    window_bytes = CHANNELS * 16 ** 3 * 4
    sum_bytes = CHANNELS * 40 ** 3 * 4

    def peak(fn):
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        out = fn(vol, roi, swb, pred, overlap, pred_type="ddim_sample")
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated(dev) - base, out

    peak(streamed_sliding_window_inference)                        # first use: the library and its scratch are loaded
    streamed, got = peak(streamed_sliding_window_inference)
    del got
    listed, want = peak(sliding_window_inference)
    print(f"peak above the inputs: streamed {streamed} B, list-and-blend {listed} B; sum volume {sum_bytes} B, "
          f"predictor batch {swb * window_bytes} B, all windows {nwin * window_bytes} B")
    assert streamed < sum_bytes + 4 * swb * window_bytes
    assert streamed < nwin * window_bytes // 2 < listed


def test_argument_errors_and_an_out_of_range_row():
    from diff_unet_amos_amd import _native as nv
    from diff_unet_amos_amd import ops
    L = nv.lib()
    dev = torch.device("cuda", 0)
    B, Cn, P, R = 1, 2, 12, 8
    acc = torch.zeros(B, Cn, P, P, P, device=dev)
    win = torch.ones(1, Cn, R, R, R, device=dev)
    table = torch.tensor([[0, 0, 0, 0], [0, 4, 4, 4]], dtype=torch.int32, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    st = nv.stream_ptr()

    def accumulate(dtype=nv.F32, nb=1, C_=Cn, w=win, t=table, rows=2, off=0, stride=1, s=acc):
        return L.dua_blend_accumulate(dtype, nb, C_, R, R, R, nv.ptr(w), nv.ptr(t), rows, off, stride, nv.ptr(s), B, P, P, P,
                                      nv.ptr(err), st)

    assert accumulate() == 0
    assert accumulate(dtype=nv.U8) == nv.ERR_ARG and accumulate(dtype=7) == nv.ERR_ARG                 # bad dtype
    assert accumulate(C_=nv.BLEND_MAX_CLASSES + 1) == nv.ERR_ARG                                     # C over the limit
    assert accumulate(w=None) == nv.ERR_ARG and accumulate(t=None) == nv.ERR_ARG and accumulate(s=None) == nv.ERR_ARG
    assert accumulate(off=2) == nv.ERR_ARG and accumulate(nb=2, off=1) == nv.ERR_ARG and accumulate(stride=0) == nv.ERR_ARG
    assert L.dua_blend_accumulate(nv.F32, 1, Cn, 16, R, R, nv.ptr(win), nv.ptr(table), 2, 0, 1, nv.ptr(acc), B, P, P, P, None,
                                  st) == nv.ERR_ARG                                                  # roi above the volume
    torch.cuda.synchronize()
    assert int(err.item()) == 0 and float(acc.sum()) == Cn * R ** 3                                  # only the valid call ran

    cov = [torch.ones(P, dtype=torch.int32, device=dev) for _ in range(3)]
    mask = torch.empty(B, Cn, P, P, P, dtype=torch.uint8, device=dev)
    tallies = torch.empty(Cn, 3, dtype=torch.int64, device=dev)
    labels = torch.zeros(B, Cn, P, P, P, device=dev)

    def finish(s=acc, C_=Cn, n=cov[0], m=mask, lab=None, code=nv.F32, is_map=0, t=None, D=P, od=0):
        return L.dua_blend_finish(nv.ptr(s), B, C_, P, P, P, nv.ptr(n), nv.ptr(cov[1]), nv.ptr(cov[2]), od, 0, 0, D, P, P, None,
                                  nv.ptr(m), nv.ptr(lab), code, is_map, nv.ptr(t), st)

    assert finish() == 0 and finish(lab=labels, t=tallies) == 0
    assert finish(s=None) == nv.ERR_ARG and finish(n=None) == nv.ERR_ARG and finish(m=None) == nv.ERR_ARG     # null pointers
    assert finish(C_=nv.BLEND_MAX_CLASSES + 1) == nv.ERR_ARG
    assert finish(lab=labels, t=tallies, code=nv.F16) == nv.ERR_ARG and finish(lab=labels, t=tallies, is_map=1) == nv.ERR_ARG
    assert finish(lab=labels) == nv.ERR_ARG and finish(t=tallies) == nv.ERR_ARG                       # labels and tallies go together
    assert finish(od=1) == nv.ERR_ARG and finish(D=P + 1) == nv.ERR_ARG                                # crop outside the volume
    with pytest.raises(ValueError):
        ops.blend_accumulate(acc, win.double(), table, 0)

    # rows outside the volume, built on the host: clamped into it and flagged, no fault
    acc.zero_()
    bad = torch.tensor([[0, 0, 0, 0], [3, -5, 2, 100], [-1, 5, 1000, 4]], dtype=torch.int32).to(dev)
    ops.blend_accumulate(acc, win, bad, 0, err=err)
    torch.cuda.synchronize()
    assert int(err.item()) == 0
    ops.blend_accumulate(acc, torch.ones(2, Cn, R, R, R, device=dev), bad, 1, err=err)
    torch.cuda.synchronize()
    assert int(err.item()) == 1
    want = torch.zeros_like(acc)
    want[0, :, 0:8, 0:8, 0:8] += 1
    want[0, :, 0:8, 2:10, 4:12] += 1                               # (3, -5, 2, 100) -> (0, 0, 2, 4)
    want[0, :, 4:12, 4:12, 4:12] += 1                              # (-1, 5, 1000, 4) -> (0, 4, 4, 4)
    assert torch.equal(acc, want)
