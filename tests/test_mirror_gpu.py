"""Mirror test-time augmentation on the GPU (csrc/blend.hip, the MIRROR forms of the accumulate kernel): the two entry points
bit for bit against ``sum[slice] += torch.flip(window)`` at every shift, edge and mask, the streamed path against the
list-and-blend path, evaluate_volume, the two-rank all-reduce form against the fp64 restatement, argument errors."""
import os
import socket
import subprocess
import sys

import pytest
import torch

from diff_unet_amos_amd.inference import (_plan, binarise, dice_per_class, evaluate_volume, importance_map, importance_vectors,
                                          infer, sliding_window_inference, streamed_sliding_window_inference)
from mirror_ref import RANK_CASES, fp32_bound, mirrored_blend_fp64
from streamed_blend_stub import CHANNELS, make_predictor, seeded_volume

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAND = 2.0 ** -20        # as tests/test_streamed_blend_gpu.py: fp32 sigmoid(q) cannot exceed 0.5 below about 2^-23
AXES = [(2,), (0, 1), (0, 1, 2)]
# the CPU test's ragged plan, and a padded batch of two (tests/test_mirror_host.py)
PLANS = [
    ((1, 1, 11, 13, 18), (8, 8, 12), 0.5, 2),
    ((2, 1, 7, 9, 16), (8, 8, 8), 0.5, 4),
]


def _dims(flip):
    return [1 + a for a in range(3) if flip >> a & 1]              # of a [C, rd, rh, rw] window


def _copy_at(src, narrow):
    """A copy of ``src`` whose first element lies on a 16-byte boundary, or (``narrow``) 4 bytes past one."""
    holder = torch.empty(src.numel() + 4, dtype=src.dtype, device=src.device)
    assert holder.data_ptr() % 16 == 0
    out = (holder[1:1 + src.numel()] if narrow else holder[:src.numel()]).view(src.shape).copy_(src)
    assert out.data_ptr() % 16 == (4 if narrow else 0) and out.is_contiguous()
    return out


@pytest.mark.parametrize("narrow", [False, True], ids=["wide", "narrow"])
@pytest.mark.parametrize("weighted", [False, True], ids=["constant", "gaussian"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
def test_op_equals_slice_add_of_the_flipped_window_bit_for_bit(dtype, weighted, narrow):
    """Four windows of one call at w offsets 0 .. 3 and d, h offsets (0 | 1), all overlapping, into a volume of odd Wp that
    starts from random values: every ``shift`` occurs, rows differ in it, the two partial groups of a row and (rw = 1, 3) rows
    without a whole group occur, and the order of the four additions matters.  ``narrow``: the volume is viewed 4 bytes past a
    16-byte boundary (the one-element-per-lane form).  Reference: the same slice-adds of ``torch.flip`` in torch operators on
    the same device; torch.equal.  Mask 0 is also compared with the unmirrored entry point."""
    from diff_unet_amos_amd import ops
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(11)
    checked = 0
    for rw in (1, 3, 4, 6, 9):
        for rd in (2, 3):
            for rh in (2, 3):
                for Cn in (1, 3):
                    B, Dp, Hp = 2, rd + 1, rh + 1
                    Wp = rw + 3 + (rw % 2)                         # odd, and room for the w offsets 0 .. 3
                    assert Wp % 2 == 1
                    shape = (B, Cn, Dp, Hp, Wp)
                    start = torch.randn(shape, generator=g).to(dev)
                    rows = [(1, k & 1, k >> 1, k) for k in range(4)]
                    table = torch.tensor([(0, 0, 0, 0)] + rows, dtype=torch.int32).to(dev)       # the call starts at row 1
                    win = torch.randn(4, Cn, rd, rh, rw, generator=g).to(dev).to(dtype)
                    weights = wmap = None
                    if weighted:
                        vectors = importance_vectors((rd, rh, rw), "gaussian", 0.125)
                        weights = (*(v.to(dev) for v in vectors[:3]), vectors[3])
                        wmap = importance_map(vectors, dev)
                    for flip in range(8):
                        want = start.clone()
                        for k, (b, d, h, w) in enumerate(rows):
                            o = torch.flip(win[k].float(), _dims(flip))
                            want[b, :, d:d + rd, h:h + rh, w:w + rw] += o if wmap is None else wmap * o
                        got = _copy_at(start, narrow)
                        if weighted:
                            ops.blend_accumulate(got, win, table, 1, weights=weights, flip=flip)
                        else:
                            ops.blend_accumulate(got, win, table, 1, flip=flip)
                        assert torch.equal(got, want), (rw, rd, rh, Cn, flip, int((got != want).sum()))
                        checked += 1
                        if flip == 0:
                            plain = _copy_at(start, narrow)
                            if weighted:
                                ops.blend_accumulate(plain, win, table, 1, weights=weights)
                            else:
                                ops.blend_accumulate(plain, win, table, 1)
                            assert torch.equal(got, plain)
    assert checked == 5 * 2 * 2 * 2 * 8


@pytest.mark.parametrize("mode", ["constant", "gaussian"])
@pytest.mark.parametrize("axes", AXES)
@pytest.mark.parametrize("shape,roi,overlap,swb", PLANS)
def test_streamed_equals_the_list_and_blend_path_bit_for_bit(shape, roi, overlap, swb, axes, mode):
    """The same fp32 additions in the same order and a divisor scaled by the same power of two: torch.equal."""
    dev = torch.device("cuda", 0)
    pred = make_predictor(roi, dev)
    vol = seeded_volume(shape).to(dev)
    want = sliding_window_inference(vol, roi, swb, pred, overlap, mirror_axes=axes, mode=mode, pred_type="ddim_sample")
    got = streamed_sliding_window_inference(vol, roi, swb, pred, overlap, mirror_axes=axes, mode=mode, pred_type="ddim_sample")
    assert got.shape == want.shape == (shape[0], CHANNELS, *shape[2:]) and got.dtype == torch.float32
    print(f"streamed vs list-and-blend {shape} axes {axes} {mode}: mismatching voxels {int((got != want).sum())}, "
          f"max |d| {float((got - want).abs().max()):.3e}")
    assert torch.equal(got, want)
    plain = streamed_sliding_window_inference(vol, roi, swb, pred, overlap, mode=mode, pred_type="ddim_sample")
    assert float((got - plain).abs().max()) > 1e-2                 # the stub is not flip-equivariant: the average moved
    for none in ((), None):                                        # and no axes is the unmirrored call
        assert torch.equal(streamed_sliding_window_inference(vol, roi, swb, pred, overlap, mirror_axes=none, mode=mode,
                                                             pred_type="ddim_sample"), plain)


@pytest.mark.parametrize("mode", ["constant", "gaussian"])
def test_fp16_windows_are_widened_then_added_in_fp32(mode):
    dev = torch.device("cuda", 0)
    shape, roi, overlap, swb = PLANS[0]
    pred = make_predictor(roi, dev)
    rounded = lambda x, **kw: pred(x, **kw).half().float()         # noqa: E731
    vol = seeded_volume(shape).to(dev)
    want = sliding_window_inference(vol, roi, swb, rounded, overlap, mirror_axes=(0, 1, 2), mode=mode, pred_type="ddim_sample")
    got = streamed_sliding_window_inference(vol, roi, swb, pred, overlap, gather_dtype=torch.float16, mirror_axes=(0, 1, 2),
                                            mode=mode, pred_type="ddim_sample")
    assert torch.equal(got, want)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


@pytest.mark.parametrize("shape,roi,overlap,swb", PLANS)
def test_evaluate_volume(shape, roi, overlap, swb):
    """Mask and Dice of the mirrored streamed evaluation against the list path; once with ``postprocess`` and once with
    ``surface``: both run after the finish pass and compose unchanged."""
    from diff_unet_amos_amd import metrics
    from diff_unet_amos_amd import postprocess as pp
    dev = torch.device("cuda", 0)
    axes, mode = (0, 2), "gaussian" if shape[0] == 2 else "constant"
    pred = make_predictor(roi, dev)
    vol = seeded_volume(shape).to(dev)
    q = sliding_window_inference(vol, roi, swb, pred, overlap, mirror_axes=axes, mode=mode, pred_type="ddim_sample")
    want = binarise(q)
    in_band = q.abs() <= BAND
    g = torch.Generator().manual_seed(5)
    onehot = (torch.rand(shape[0], CHANNELS, *shape[2:], generator=g) > 0.6).float()
    onehot[:, CHANNELS - 1] = 0
    onehot = onehot.to(dev)
    kw = dict(roi_size=roi, sw_batch_size=swb, overlap=overlap, mirror_axes=axes, mode=mode)
    mask, dice = evaluate_volume(pred, vol, onehot, **kw)
    print(f"{shape}: {int(in_band.sum())} voxels inside |q| <= 2^-20, mask differs from binarise at "
          f"{int((mask.float() != want).sum())}")
    assert mask.dtype == torch.uint8 and not bool(((mask.float() != want) & ~in_band).any())
    assert torch.equal(dice, dice_per_class(mask.float(), onehot))
    if not bool(in_band.any()):
        assert torch.equal(mask.float(), want) and torch.equal(dice, dice_per_class(want, onehot))
    plain_mask, _ = evaluate_volume(pred, vol, onehot, roi, swb, overlap, mode=mode)
    assert not torch.equal(mask, plain_mask)                       # the augmentation moved voxels across 0.5
    assert torch.equal(infer(pred, vol, roi, swb, overlap, streaming=True, mirror_axes=axes, mode=mode), mask.float())
    if not bool(in_band.any()):
        assert torch.equal(infer(pred, vol, roi, swb, overlap, mirror_axes=axes, mode=mode), mask.float())
    post = dict(connectivity=1, num_components=1)
    fmask, fdice = evaluate_volume(pred, vol, onehot, postprocess=post, **kw)
    assert torch.equal(fmask, pp.keep_largest_components(mask, **post)) and torch.equal(fdice, dice_per_class(fmask, onehot))
    assert not torch.equal(fmask, mask)
    smask, sdice, report = evaluate_volume(pred, vol, onehot, surface={"tolerance": 1.0}, **kw)
    assert torch.equal(smask, mask) and torch.equal(sdice, dice)
    ref = metrics.surface_dice_table(mask, onehot, 1.0)
    assert set(report) == set(ref) and all(_same_bits(report[k], ref[k]) for k in ref)


def test_two_ranks_all_reduce_against_the_fp64_restatement(tmp_path):
    """Two ranks over gloo sharing device 0, under a time limit of their own.  Each rank runs the F flips of its own windows;
    the all-reduce adds each voxel's n = F coverage terms in another order than one process does, which the bound of
    ``mirror_ref.fp32_bound`` (any order) covers.  The all-reduced bytes are those of the unmirrored run."""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "tests", "mirror_ref.py"), str(tmp_path)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=420)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    for k, (shape, roi, overlap, swb, axes, mode) in enumerate(RANK_CASES):
        got = torch.load(os.path.join(tmp_path, f"case{k}.pt"))
        assert got["world"] == 2 and got["same_on_every_rank"]
        vol = seeded_volume(shape)
        q64, mag, n = mirrored_blend_fp64(vol, roi, overlap, make_predictor(roi, "cpu"), axes, mode)
        bound = fp32_bound(q64, mag, n, mode)
        err = (got["q"].double() - q64).abs()
        print(f"two ranks, case {k} {shape} axes {axes} {mode}: max |q - q64| {float(err.max()):.3e}, max err / bound "
              f"{float((err / bound).max()):.3f}, additions per voxel up to {int(n.max())}")
        assert bool((err <= bound).all())
        padded = _plan(vol, roi, overlap)[2]
        assert got["timings"]["reduced_bytes"] == got["plain_timings"]["reduced_bytes"] == \
            shape[0] * CHANNELS * padded[0] * padded[1] * padded[2] * 4


def test_argument_errors_and_an_out_of_range_row():
    from diff_unet_amos_amd import _native as nv
    from diff_unet_amos_amd import ops
    L = nv.lib()
    dev = torch.device("cuda", 0)
    B, Cn, P, R = 1, 2, 12, 8
    acc = torch.zeros(B, Cn, P, P, P, device=dev)
    g = torch.Generator().manual_seed(3)
    win = torch.randn(2, Cn, R, R, R, generator=g).to(dev)
    table = torch.tensor([[0, 0, 0, 0], [0, 4, 4, 4]], dtype=torch.int32, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    vectors = importance_vectors((R, R, R), "gaussian", 0.125)
    weights = (*(v.to(dev) for v in vectors[:3]), vectors[3])
    st = nv.stream_ptr()

    def mirrored(flip, dtype=nv.F32, C_=Cn, w=win, off=0):
        return L.dua_blend_accumulate_mirrored(dtype, 1, C_, R, R, R, nv.ptr(w), nv.ptr(table), 2, off, 1, flip, nv.ptr(acc), B, P,
                                               P, P, nv.ptr(err), st)

    def weighted(flip, floor=weights[3], g2=weights[2]):
        return L.dua_blend_accumulate_weighted_mirrored(nv.F32, 1, Cn, R, R, R, nv.ptr(win), nv.ptr(table), 2, 0, 1, flip,
                                                        nv.ptr(weights[0]), nv.ptr(weights[1]), nv.ptr(g2), floor, nv.ptr(acc), B,
                                                        P, P, P, nv.ptr(err), st)

    for bad in (8, -1, 1 << 20):
        assert mirrored(bad) == nv.ERR_ARG and weighted(bad) == nv.ERR_ARG
    assert mirrored(5, dtype=nv.U8) == nv.ERR_ARG and mirrored(5, C_=nv.BLEND_MAX_CLASSES + 1) == nv.ERR_ARG
    assert mirrored(5, w=None) == nv.ERR_ARG and mirrored(5, off=2) == nv.ERR_ARG
    assert weighted(5, floor=0.0) == nv.ERR_ARG and weighted(5, g2=None) == nv.ERR_ARG
    torch.cuda.synchronize()
    assert int(err.item()) == 0 and float(acc.abs().sum()) == 0.0          # no refused call touched the volume
    for bad in (8, -1):
        with pytest.raises(ValueError):
            ops.blend_accumulate(acc, win, table, 0, flip=bad)
        with pytest.raises(ValueError):
            ops.blend_accumulate(acc, win, table, 0, weights=weights, flip=bad)
    with pytest.raises(ValueError):
        ops.blend_accumulate(acc, win.double(), table, 0, flip=1)

    # rows outside the volume, built on the host: clamped into it and flagged, no fault -- as the unmirrored form
    bad_rows = torch.tensor([[0, 0, 0, 0], [3, -5, 2, 100], [-1, 5, 1000, 4]], dtype=torch.int32).to(dev)
    ops.blend_accumulate(acc, win[:1], bad_rows, 0, flip=6, err=err)
    torch.cuda.synchronize()
    assert int(err.item()) == 0
    ops.blend_accumulate(acc, win, bad_rows, 1, flip=6, err=err)
    torch.cuda.synchronize()
    assert int(err.item()) == 1
    want = torch.zeros_like(acc)
    want[0, :, 0:8, 0:8, 0:8] += torch.flip(win[0], [2, 3])
    want[0, :, 0:8, 2:10, 4:12] += torch.flip(win[0], [2, 3])      # (3, -5, 2, 100) -> (0, 0, 2, 4)
    want[0, :, 4:12, 4:12, 4:12] += torch.flip(win[1], [2, 3])     # (-1, 5, 1000, 4) -> (0, 4, 4, 4)
    assert torch.equal(acc, want)
