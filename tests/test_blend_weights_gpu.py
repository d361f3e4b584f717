"""Gaussian window weighting of the streamed blend on the GPU (csrc/blend.hip, the weighted entry points): bit-equality with
the list-and-blend form written in torch operators on the same device, the weight-sum volume, mask and Dice of the weighted
finish pass, a clamped table row, argument errors, and the two-rank all-reduce form against an fp64 weighted blend."""
import functools
import itertools
import os
import socket
import subprocess
import sys

import pytest
import torch

from diff_unet_amos_amd.inference import (_plan, _window, axis_starts, dice_per_class, evaluate_volume, importance_vectors, infer,
                                          sliding_window_inference, streamed_sliding_window_inference, window_table)
from blend_weights_stub import fp64_weighted_blend, weight_map
from streamed_blend_stub import MARKER, RANK_CASES, make_predictor, seeded_volume

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAND = 2.0 ** -20        # as tests/test_streamed_blend_gpu.py: only the two-rank masks, whose sums differ, are compared outside it
BAND_CAP = 1e-4

# (volume, roi, overlap): every lane form of the accumulate kernel
PLANS = [
    ((20, 18, 23), (8, 6, 10), 0.5),         # odd row length 23: every shift of the wide form, by-element edges on both sides
    ((9, 33, 16), (8, 8, 16), 0.25),         # rows of 16 at a row length of 16: shift 0, the aligned 16-byte window loads
    ((12, 12, 13), (12, 12, 8), 0.8),        # W starts 0 .. 5 at a row length of 13: a partial last group
    ((5, 9, 7), (8, 6, 10), 0.8),            # smaller than the roi along D and W: padded, cropped by the finish pass
]
SIGMAS = [0.125, 0.5]                         # the floor 1e-3 clamps the map / the floor is the map's own minimum
FORMS = [(1, 1, 3), (2, 3, 1), (2, 3, 3)]     # (B, C, sw_batch_size)
CASES = [(*p, s, *f, None) for p, s, f in itertools.product(PLANS, SIGMAS, FORMS)] + \
        [(*p, s, 2, 3, 3, torch.float16) for p, s in itertools.product(PLANS, SIGMAS)]


def _device_weights(roi, sigma_scale, dev):
    vectors = importance_vectors(roi, "gaussian", sigma_scale)
    return (*(g.to(dev) for g in vectors[:3]), vectors[3]), weight_map(vectors)[1].to(dev)


@functools.lru_cache(maxsize=None)
def _torch_blend(shape, roi, overlap, sigma_scale, channels, halved, planted=False, seed=None):
    """The list-and-blend form in torch operators on the device, in window order: ``out[slice] += w * o``, ``cnt[slice] += w``,
    ``out / cnt``.  Returns (sum volume [B, C, *padded], cnt [*padded], cropped quotient); computed once per plan and shared --
    nobody writes into the result."""
    dev = torch.device("cuda", 0)
    vol = _volume(shape, planted, seed).to(dev)
    pred = make_predictor(roi, dev, planted=planted, channels=channels)
    spatial, roi, padded, pad, starts = _plan(vol, roi, overlap)
    w = _device_weights(roi, sigma_scale, dev)[1]
    x = torch.nn.functional.pad(vol, pad)
    B, nwin = vol.shape[0], len(starts)
    out = torch.zeros(B, channels, *padded, device=dev)
    cnt = torch.zeros(padded, device=dev)
    for i in range(nwin * B):
        b, (d, h, ww) = i // nwin, starts[i % nwin]
        o = pred(_window(x, i, nwin, starts, roi))[0]
        if halved:
            o = o.half().float()
        out[b, :, d:d + roi[0], h:h + roi[1], ww:ww + roi[2]] += w * o
        if b == 0:
            cnt[d:d + roi[0], h:h + roi[1], ww:ww + roi[2]] += w
    crop = (slice(None), slice(None)) + tuple(slice(pad[2 * (2 - k)], pad[2 * (2 - k)] + spatial[k]) for k in range(3))
    return out, cnt, (out / cnt)[crop]


def _volume(shape, planted=False, seed=None):
    vol = seeded_volume(shape, seed=seed)
    if planted:                                                    # the stub's planted input: see _planted_case
        vol[:, 1] = 1.0
        vol[:, 1, :, :, 16:] = -1.0
        for d, h, w in PLANTED:
            vol[0, 0, d, h, w] = MARKER
    return vol


@pytest.mark.parametrize("volume,roi,overlap,sigma_scale,B,C,swb,gather_dtype", CASES)
def test_streamed_gaussian_equals_the_torch_blend_bit_for_bit(volume, roi, overlap, sigma_scale, B, C, swb, gather_dtype):
    """One rounded product and one rounded addition per window and voxel in window order, the same weight sums, one IEEE
    division: torch.equal with the torch form on the same device, not a tolerance.  Two runs agree bit for bit."""
    dev = torch.device("cuda", 0)
    shape = (B, 1, *volume)
    want = _torch_blend(shape, roi, overlap, sigma_scale, C, gather_dtype is not None)[2]
    pred = make_predictor(roi, dev, channels=C)
    vol = seeded_volume(shape).to(dev)
    kw = dict(mode="gaussian", sigma_scale=sigma_scale, pred_type="ddim_sample")
    got = streamed_sliding_window_inference(vol, roi, swb, pred, overlap, gather_dtype=gather_dtype, **kw)
    assert got.shape == want.shape == (B, C, *volume) and got.dtype == torch.float32
    print(f"streamed gaussian {shape} roi {roi} overlap {overlap} sigma {sigma_scale} C {C} swb {swb} {gather_dtype}: mismatching "
          f"voxels {int((got != want).sum())}, max |d| {float((got - want).abs().max()):.3e}")
    assert torch.equal(got, want)
    assert torch.equal(streamed_sliding_window_inference(vol, roi, swb, pred, overlap, gather_dtype=gather_dtype, **kw), got)
    listed = pred if gather_dtype is None else (lambda x, **k: pred(x, **k).half().float())
    assert torch.equal(sliding_window_inference(vol, roi, swb, listed, overlap, **kw), want)     # the package's own list path
    constant = streamed_sliding_window_inference(vol, roi, swb, pred, overlap, gather_dtype=gather_dtype, pred_type="ddim_sample")
    assert torch.equal(streamed_sliding_window_inference(vol, roi, swb, pred, overlap, gather_dtype=gather_dtype, mode="constant",
                                                         pred_type="ddim_sample"), constant)
    assert not torch.equal(constant, got) or len(_plan(vol, roi, overlap)[4]) == 1


@pytest.mark.parametrize("volume,roi,overlap", PLANS + [((37, 50, 41), (16, 16, 16), 0.8)])
@pytest.mark.parametrize("sigma_scale", SIGMAS + [(0.125, 0.3, 0.2)])
def test_weight_sum_from_the_plan_equals_the_accumulated_map(volume, roi, overlap, sigma_scale):
    from diff_unet_amos_amd import ops
    dev = torch.device("cuda", 0)
    shape = (1, 1, *volume)
    want = _torch_blend(shape, roi, overlap, sigma_scale, 1, False)[1]
    spatial, roi, padded, pad, starts = _plan(torch.zeros(1, 1, 1, 1, 1).expand(1, 1, *volume), roi, overlap)
    per_axis = [torch.tensor(s, dtype=torch.int32, device=dev) for s in axis_starts(starts)]
    got = ops.blend_weight_sum(per_axis, roi, padded, _device_weights(roi, sigma_scale, dev)[0])
    assert got.dtype == torch.float32 and tuple(got.shape) == tuple(padded) and float(got.min()) > 0
    assert torch.equal(got, want)


@pytest.mark.parametrize("volume,roi,overlap", PLANS[:3])
@pytest.mark.parametrize("windows_dtype", [torch.float32, torch.float16])
def test_sum_volume_at_a_misaligned_base(volume, roi, overlap, windows_dtype):
    """A sum volume viewed 4 bytes past a 16-byte boundary takes the one-element-per-lane form: the same bits as the aligned
    volume and as the torch form; the weighted finish pass reads it by element too."""
    from diff_unet_amos_amd import ops
    dev = torch.device("cuda", 0)
    B, C, sigma_scale = 2, 3, 0.125
    shape = (B, 1, *volume)
    halved = windows_dtype == torch.float16
    want_sum, want_cnt, want_q = _torch_blend(shape, roi, overlap, sigma_scale, C, halved)
    vol = seeded_volume(shape).to(dev)
    pred = make_predictor(roi, dev, channels=C)
    spatial, roi, padded, pad, starts = _plan(vol, roi, overlap)
    weights = _device_weights(roi, sigma_scale, dev)[0]
    x = torch.nn.functional.pad(vol, pad)
    table = window_table(starts, B, dev)
    n = B * C * padded[0] * padded[1] * padded[2]
    backing = torch.zeros(n + 4, device=dev)
    assert backing.data_ptr() % 16 == 0
    shifted, aligned = backing[1:n + 1].view(B, C, *padded), torch.zeros(B, C, *padded, device=dev)
    assert shifted.data_ptr() % 16 == 4 and shifted.is_contiguous()
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    nwin = len(starts)
    for i in range(0, nwin * B, 3):
        idxs = list(range(i, min(i + 3, nwin * B)))
        seg = torch.cat([pred(_window(x, j, nwin, starts, roi)) for j in idxs]).to(windows_dtype)
        ops.blend_accumulate(shifted, seg, table, i, weights=weights, err=err)
        ops.blend_accumulate(aligned, seg, table, i, weights=weights, err=err)
    assert int(err.item()) == 0
    assert torch.equal(shifted, want_sum) and torch.equal(aligned, want_sum)
    assert float(backing[0]) == 0 and float(backing[n + 1:].abs().sum()) == 0                  # nothing beside the view
    per_axis = [torch.tensor(s, dtype=torch.int32, device=dev) for s in axis_starts(starts)]
    wsum = ops.blend_weight_sum(per_axis, roi, padded, weights)
    assert torch.equal(wsum, want_cnt)
    lo = tuple(pad[2 * (2 - k)] for k in range(3))
    assert torch.equal(ops.blend_finish(shifted, wsum, lo, spatial, want_q=True)[0], want_q)
    assert torch.equal(ops.blend_finish(aligned, wsum, lo, spatial, want_q=True)[0], want_q)


PLANTED = [(3, 4, 17), (10, 20, 16), (31, 0, 31), (16, 16, 24), (0, 31, 20)]


@pytest.mark.parametrize("case", ["planted", "padded_batch", "ragged"])
def test_mask_and_dice_of_the_weighted_finish_pass(case):
    """The mask against ``sum > 0`` of the bit-equal torch sum volume (wsum > 0, so q and the sum have one sign), everywhere;
    tallies against torch counts.  The planted case of the stub: 32 x 32 x 48 at roi 32^3, overlap 0.5, two windows with W
    starts 0 and 16 that give +3 and -3 at the MARKER voxels.  Where both windows' weights at such a voxel are the floor
    (the map is clamped near the window's faces) the sum is +3 f - 3 f = 0 exactly and the mask is 0."""
    from diff_unet_amos_amd import ops
    from streamed_blend_stub import CHANNELS
    dev = torch.device("cuda", 0)
    sigma_scale = 0.125
    if case == "planted":
        shape, roi, overlap, swb, seed = (1, 2, 32, 32, 48), (32, 32, 32), 0.5, 2, 77
    elif case == "padded_batch":
        shape, roi, overlap, swb, seed = (2, 1, 9, 16, 6), (8, 8, 8), 0.5, 4, None
    else:
        shape, roi, overlap, swb, seed = (1, 1, 20, 18, 23), (8, 6, 10), 0.5, 3, None
    planted = case == "planted"
    vol = _volume(shape, planted, seed).to(dev)
    pred = make_predictor(roi, dev, planted=planted)
    want_sum, want_cnt, want_q = _torch_blend(shape, roi, overlap, sigma_scale, CHANNELS, False, planted, seed)
    spatial, roi, padded, pad, starts = _plan(vol, roi, overlap)
    lo = tuple(pad[2 * (2 - k)] for k in range(3))
    crop = (slice(None), slice(None)) + tuple(slice(lo[k], lo[k] + spatial[k]) for k in range(3))
    want_mask = want_sum[crop] > 0
    B, D, H, W = shape[0], *shape[2:]
    g = torch.Generator().manual_seed(5)
    onehot = (torch.rand(B, CHANNELS, D, H, W, generator=g) > 0.6).float()
    onehot[:, CHANNELS - 1] = 0
    onehot = onehot.to(dev)
    label_map = torch.randint(0, CHANNELS - 1, (B, D, H, W), generator=g).to(torch.uint8).to(dev)
    map_onehot = label_map[:, None] == torch.arange(CHANNELS, device=dev).view(1, -1, 1, 1, 1)

    kw = dict(mode="gaussian", sigma_scale=sigma_scale)
    mask, dice = evaluate_volume(pred, vol, onehot, roi, swb, overlap, **kw)
    assert mask.dtype == torch.uint8 and mask.shape == want_mask.shape and int(mask.max()) <= 1
    tiny = (want_q > 0) & (want_q < 2.0 ** -22)
    print(f"{case}: mask differs from sum > 0 at {int((mask.bool() != want_mask).sum())} of {mask.numel()} voxels; "
          f"{int(tiny.sum())} voxels with 0 < q < 2^-22, exact zeros {int((want_q == 0).sum())}")
    assert torch.equal(mask.bool(), want_mask)
    assert torch.equal(dice, dice_per_class(mask.float(), onehot)) and float(dice[CHANNELS - 1]) == 0.0
    if planted:
        w = _device_weights(roi, sigma_scale, dev)[1]
        cancel = [(d, h, x) for d, h, x in PLANTED if float(w[d, h, x]) == float(w[d, h, x - 16])]
        assert (3, 4, 17) in cancel                                # both weights are the floor there
        for d, h, x in cancel:
            assert float(want_sum[0, 0, d, h, x]) == 0.0 and int(mask[0, 0, d, h, x]) == 0
    mask_m, dice_m = evaluate_volume(pred, vol, label_map, roi, swb, overlap, **kw)              # the label-map form
    assert torch.equal(mask_m, mask) and torch.equal(dice_m, dice_per_class(mask.float(), map_onehot.float()))
    assert torch.equal(infer(pred, vol, roi, swb, overlap, streaming=True, **kw), mask.float())
    # the entry points themselves: q, mask and the counts
    acc = torch.zeros(B, CHANNELS, *padded, device=dev)
    table = window_table(starts, B, dev)
    x = torch.nn.functional.pad(vol, pad)
    weights = _device_weights(roi, sigma_scale, dev)[0]
    for i in range(len(starts) * B):
        ops.blend_accumulate(acc, pred(_window(x, i, len(starts), starts, roi)), table, i, weights=weights)
    assert torch.equal(acc, want_sum)
    wsum = ops.blend_weight_sum([torch.tensor(s, dtype=torch.int32, device=dev) for s in axis_starts(starts)], roi, padded, weights)
    q2, mask2, tallies = ops.blend_finish(acc, wsum, lo, spatial, want_q=True, want_mask=True, labels=label_map)
    assert torch.equal(q2, want_q) and torch.equal(mask2, mask)
    a, b = want_mask, map_onehot
    want_t = torch.stack([(a & b).sum((0, 2, 3, 4)), a.sum((0, 2, 3, 4)), b.sum((0, 2, 3, 4))], dim=1)
    assert tallies.dtype == torch.int64 and torch.equal(tallies, want_t)


def test_two_ranks_all_reduce_against_an_fp64_weighted_blend(tmp_path):
    """Two ranks over gloo sharing device 0, under a time limit of their own.  A voxel under n windows: every term w o takes one
    rounded product and, over both ranks' partial sums and the all-reduce, at most n - 1 rounded additions:
      |sum_fp32 - sum| <= n 2^-24 sum|w_i o_i| (1 + 2^-10)                   (gamma_n <= n u (1 + 2^-10) for n <= 2^13)
    the weight sum is computed by every rank in full, n - 1 additions: wsum_fp32 = wsum (1 + t), |t| <= (n - 1) 2^-24 (1 + 2^-10),
    and one correctly rounded division follows:
      |q - q64| <= (n sum|w o| + (n - 1) |sum w o|) / wsum 2^-24 (1 + 2^-10) + ulp(q).
    The reference is an fp64 blend with the same fp32 map, not the code under test."""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "tests", "blend_weights_stub.py"), str(tmp_path)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=420)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    dev = torch.device("cuda", 0)
    for k, (shape, roi, overlap, swb) in enumerate(RANK_CASES):
        got = torch.load(os.path.join(tmp_path, f"case{k}.pt"))
        assert got["world"] == 2 and got["same_on_every_rank"]
        vol = seeded_volume(shape)
        q64, mag, n, tot = fp64_weighted_blend(vol, roi, overlap, make_predictor(roi, "cpu"), 0.125)
        bound = (n * mag + (n - 1) * tot) * 2.0 ** -24 * (1 + 2.0 ** -10) + 2.0 ** -23 * q64.abs() + 2.0 ** -149
        err = (got["q"].double() - q64).abs()
        print(f"two ranks gaussian, case {k} {shape}: max |q - q64| {float(err.max()):.3e}, max err / bound "
              f"{float((err / bound).max()):.3f}, windows over a voxel up to {int(n.max())}")
        assert bool((err <= bound).all())
        padded = _plan(vol, roi, overlap)[2]
        assert got["timings"]["reduced_bytes"] == shape[0] * got["q"].shape[1] * padded[0] * padded[1] * padded[2] * 4
        single, _ = evaluate_volume(make_predictor(roi, dev), vol.to(dev), None, roi, swb, overlap, mode="gaussian")
        outside = q64.abs() > BAND
        assert float((~outside).float().mean()) <= BAND_CAP
        assert torch.equal(got["mask"][outside], single.cpu()[outside])


def test_a_clamped_row_sets_err_and_stays_inside_the_volume():
    """Rows outside the volume, built on the host: clamped into it and flagged; the guard words around the volume stay zero."""
    from diff_unet_amos_amd import ops
    dev = torch.device("cuda", 0)
    B, Cn, P, R = 1, 2, 12, 8
    n, guard = B * Cn * P ** 3, 4096
    backing = torch.zeros(n + 2 * guard, device=dev)
    acc = backing[guard:guard + n].view(B, Cn, P, P, P)
    weights, w = _device_weights((R, R, R), 0.125, dev)
    win = torch.ones(1, Cn, R, R, R, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    bad = torch.tensor([[0, 0, 0, 0], [3, -5, 2, 100], [-1, 5, 1000, 4]], dtype=torch.int32).to(dev)
    ops.blend_accumulate(acc, win, bad, 0, weights=weights, err=err)
    torch.cuda.synchronize()
    assert int(err.item()) == 0
    ops.blend_accumulate(acc, torch.ones(2, Cn, R, R, R, device=dev), bad, 1, weights=weights, err=err)
    torch.cuda.synchronize()
    assert int(err.item()) == 1
    want = torch.zeros_like(acc)
    want[0, :, 0:8, 0:8, 0:8] += w
    want[0, :, 0:8, 2:10, 4:12] += w                               # (3, -5, 2, 100) -> (0, 0, 2, 4)
    want[0, :, 4:12, 4:12, 4:12] += w                              # (-1, 5, 1000, 4) -> (0, 4, 4, 4)
    assert torch.equal(acc, want)
    assert float(backing[:guard].abs().sum()) == 0 and float(backing[guard + n:].abs().sum()) == 0


def test_argument_errors_of_the_weighted_entry_points():
    from diff_unet_amos_amd import _native as nv
    from diff_unet_amos_amd import ops
    L = nv.lib()
    dev = torch.device("cuda", 0)
    B, Cn, P, R = 1, 2, 12, 8
    acc = torch.zeros(B, Cn, P, P, P, device=dev)
    win = torch.ones(1, Cn, R, R, R, device=dev)
    table = torch.tensor([[0, 0, 0, 0], [0, 4, 4, 4]], dtype=torch.int32, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    (g0, g1, g2, floor), w = _device_weights((R, R, R), 0.125, dev)
    st = nv.stream_ptr()

    def accumulate(dtype=nv.F32, nb=1, C_=Cn, w_=win, t=table, rows=2, off=0, stride=1, s=acc, a=g0, b=g1, c=g2, f=floor, r=R):
        return L.dua_blend_accumulate_weighted(dtype, nb, C_, r, R, R, nv.ptr(w_), nv.ptr(t), rows, off, stride, nv.ptr(a), nv.ptr(b),
                                               nv.ptr(c), f, nv.ptr(s), B, P, P, P, nv.ptr(err), st)

    assert accumulate() == 0
    assert accumulate(dtype=nv.U8) == nv.ERR_ARG and accumulate(dtype=7) == nv.ERR_ARG
    assert accumulate(C_=nv.BLEND_MAX_CLASSES + 1) == nv.ERR_ARG and accumulate(C_=0) == nv.ERR_ARG
    assert accumulate(w_=None) == nv.ERR_ARG and accumulate(t=None) == nv.ERR_ARG and accumulate(s=None) == nv.ERR_ARG
    assert accumulate(a=None) == nv.ERR_ARG and accumulate(b=None) == nv.ERR_ARG and accumulate(c=None) == nv.ERR_ARG
    assert accumulate(f=0.0) == nv.ERR_ARG and accumulate(f=-1.0) == nv.ERR_ARG and accumulate(f=float("nan")) == nv.ERR_ARG
    assert accumulate(off=2) == nv.ERR_ARG and accumulate(nb=2, off=1) == nv.ERR_ARG and accumulate(stride=0) == nv.ERR_ARG
    assert accumulate(r=0) == nv.ERR_ARG and accumulate(r=16) == nv.ERR_ARG                    # no extent, roi above the volume
    torch.cuda.synchronize()
    assert int(err.item()) == 0
    want = torch.zeros_like(acc)
    want[0, :, 0:8, 0:8, 0:8] += w
    assert torch.equal(acc, want)                                                              # only the valid call ran

    starts = torch.tensor([0, 4], dtype=torch.int32, device=dev)
    wsum = torch.zeros(P, P, P, device=dev)

    def weight_sum(sd=starts, n=2, a=g0, c=g2, out=wsum, f=floor, r=R, p=P):
        return L.dua_blend_weight_sum(nv.ptr(sd), n, nv.ptr(starts), 2, nv.ptr(starts), 2, r, R, R, nv.ptr(a), nv.ptr(g1), nv.ptr(c),
                                      f, nv.ptr(out), p, P, P, st)

    assert weight_sum() == 0
    assert weight_sum(sd=None) == nv.ERR_ARG and weight_sum(a=None) == nv.ERR_ARG and weight_sum(c=None) == nv.ERR_ARG
    assert weight_sum(out=None) == nv.ERR_ARG and weight_sum(n=0) == nv.ERR_ARG and weight_sum(f=0.0) == nv.ERR_ARG
    assert weight_sum(r=0) == nv.ERR_ARG and weight_sum(p=0) == nv.ERR_ARG and weight_sum(r=16) == nv.ERR_ARG
    torch.cuda.synchronize()
    assert float(wsum.min()) > 0

    mask = torch.empty(B, Cn, P, P, P, dtype=torch.uint8, device=dev)
    tallies = torch.empty(Cn, 3, dtype=torch.int64, device=dev)
    labels = torch.zeros(B, Cn, P, P, P, device=dev)

    def finish(s=acc, C_=Cn, ws=wsum, m=mask, lab=None, code=nv.F32, is_map=0, t=None, D=P, od=0):
        return L.dua_blend_finish_weighted(nv.ptr(s), B, C_, P, P, P, nv.ptr(ws), od, 0, 0, D, P, P, None, nv.ptr(m), nv.ptr(lab), code,
                                           is_map, nv.ptr(t), st)

    assert finish() == 0 and finish(lab=labels, t=tallies) == 0
    assert finish(s=None) == nv.ERR_ARG and finish(ws=None) == nv.ERR_ARG and finish(m=None) == nv.ERR_ARG
    assert finish(C_=nv.BLEND_MAX_CLASSES + 1) == nv.ERR_ARG and finish(C_=0) == nv.ERR_ARG
    assert finish(lab=labels, t=tallies, code=nv.F16) == nv.ERR_ARG and finish(lab=labels, t=tallies, is_map=1) == nv.ERR_ARG
    assert finish(lab=labels) == nv.ERR_ARG and finish(t=tallies) == nv.ERR_ARG
    assert finish(od=1) == nv.ERR_ARG and finish(D=P + 1) == nv.ERR_ARG and finish(D=0) == nv.ERR_ARG
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        ops.blend_accumulate(acc, win.double(), table, 0, weights=(g0, g1, g2, floor))
    with pytest.raises(ValueError):
        streamed_sliding_window_inference(acc, (R, R, R), 1, lambda x, **kw: x, mode="linear")
    with pytest.raises(ValueError):
        evaluate_volume(lambda x, **kw: x, acc, None, (R, R, R), mode="gaussian", sigma_scale=0.0)
