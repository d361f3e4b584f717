"""Sliding-window scheduler / blend and its sharded (multi-process, gloo on CPU) form."""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from diff_unet_amos_amd.inference import (_plan, balanced_batches, binarise, dice_per_class, sharded_sliding_window_inference,
                                          sliding_window_inference)
from oracle.sliding_window_ref import sliding_window_ref
from oracle.unet_ref import dice_coeff


def _predictor(x, pred_type=None):
    """Deterministic, position-independent function of the window contents with 3 output channels."""
    assert pred_type == "ddim_sample"
    return torch.cat([x * 2.0, x.flip(-1) + 1.0, torch.tanh(x) * x.mean(dim=(2, 3, 4), keepdim=True)], dim=1)


def _predictor_np(x):
    return _predictor(torch.from_numpy(x), pred_type="ddim_sample").numpy()


def test_window_count_of_config3():
    """256x256x192, roi 96^3, overlap 0.25 -> interval 72 -> 4 x 4 x 3 = 48 windows."""
    _, _, _, _, starts = _plan(torch.zeros(1, 1, 256, 256, 192), (96, 96, 96), 0.25)
    assert len(starts) == 48
    assert sorted({s[0] for s in starts}) == [0, 72, 144, 160] and sorted({s[2] for s in starts}) == [0, 72, 96]
    assert starts[0] == (0, 0, 0) and starts[1] == (0, 0, 72)         # last axis fastest
    with pytest.raises(ValueError):
        _plan(torch.zeros(1, 1, 8, 8, 8), (4, 4, 4), 1.0)


def test_per_rank_batches_are_balanced():
    """BASELINE config 3 on 8 GPUs: 6 windows per rank at sw_batch_size 4 run as 3 + 3, not 4 + 2; never more calls than
    slicing by sw_batch_size would make, never a call above sw_batch_size or below half of it (when there are two or more)."""
    assert balanced_batches(6, 4) == [3, 3]
    assert balanced_batches(48, 4) == [4] * 12 and balanced_batches(0, 4) == [] and balanced_batches(3, 4) == [3]
    for n in range(1, 60):
        for b in range(1, 9):
            sizes = balanced_batches(n, b)
            assert sum(sizes) == n and len(sizes) == -(-n // b) and max(sizes) <= b
            assert max(sizes) - min(sizes) <= 1 and (len(sizes) == 1 or 2 * min(sizes) >= b)


DEVICES = ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)]      # the scheduler also runs with device tensors under -m gpu


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("shape,roi,overlap,swb", [
    ((1, 1, 20, 17, 13), (8, 8, 8), 0.25, 4),
    ((2, 1, 9, 16, 16), (8, 8, 8), 0.5, 3),       # batch of 2 volumes
    ((1, 1, 5, 8, 11), (8, 8, 8), 0.8, 1),        # smaller than the roi along D: symmetric zero padding, then crop
    ((1, 1, 8, 8, 8), (8, 8, 8), 0.25, 2),        # exactly one window
])
def test_matches_loop_restatement(shape, roi, overlap, swb, device):
    g = torch.Generator().manual_seed(sum(shape))
    vol = torch.randn(*shape, generator=g)
    got = sliding_window_inference(vol.to(device), roi, swb, _predictor, overlap, pred_type="ddim_sample")
    want = sliding_window_ref(vol.numpy(), roi, overlap, _predictor_np)
    assert got.shape == (shape[0], 3, *shape[2:]) and got.device.type == device
    assert np.allclose(got.cpu().numpy(), want, rtol=1e-5, atol=1e-5)


def _worker(rank, world, port, shape, roi, overlap, swb, gather_dtype, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        g = torch.Generator().manual_seed(sum(shape))
        vol = torch.randn(*shape, generator=g)
        out = sharded_sliding_window_inference(vol, roi, swb, _predictor, overlap, gather_dtype=gather_dtype,
                                               pred_type="ddim_sample")
        q.put((rank, out.numpy()))
        dist.barrier()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,shape,overlap", [(2, (1, 1, 20, 17, 13), 0.25), (3, (2, 1, 9, 16, 16), 0.5), (2, (1, 1, 8, 8, 8), 0.25)])
def test_sharded_equals_single_process(world, shape, overlap):
    """world_size 2 and 3 over gloo: every rank ends with the single-process result (odd window counts,
    a rank with no window at all)."""
    roi, swb = (8, 8, 8), 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29500 + (os.getpid() + world + int(overlap * 100)) % 2000
    procs = [ctx.Process(target=_worker, args=(r, world, port, shape, roi, overlap, swb, None, q)) for r in range(world)]
    for p in procs:
        p.start()
    outs = dict(q.get(timeout=90) for _ in range(world))
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    g = torch.Generator().manual_seed(sum(shape))
    vol = torch.randn(*shape, generator=g)
    want = sliding_window_inference(vol, roi, swb, _predictor, overlap, pred_type="ddim_sample").numpy()
    for r in range(world):
        assert np.allclose(outs[r], want, rtol=1e-6, atol=1e-6), r


@pytest.mark.parametrize("device", DEVICES)
def test_binarise_and_dice_match_reference_formulas(device):
    g = torch.Generator().manual_seed(0)
    logits = (torch.randn(2, 4, 6, 6, 6, generator=g) * 3).to(device)
    labels = (torch.rand(2, 4, 6, 6, 6, generator=g) > 0.6).float().to(device)
    labels[:, 3] = 0
    logits[:, 3] = -10                                   # class 3 empty on both sides -> dice 0 (metric.py:45-49)
    pred = binarise(logits)
    assert torch.equal(pred, (torch.sigmoid(logits) > 0.5).float())
    got = dice_per_class(pred, labels)
    for c in range(4):
        assert abs(float(got[c]) - dice_coeff(pred[:, c].cpu(), labels[:, c].cpu())) < 1e-12
    assert float(got[3]) == 0.0


def _bench_line(args, timeout):
    """Run bench.py as the driver does for N > 1 (its own torch.distributed.run launch, rendezvous on 127.0.0.1) with two
    ranks sharing this box's one GPU over gloo; return the JSON line rank 0 printed."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, DUA_BENCH_BACKEND="gloo")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--no-roofline", "--no-cpu-baseline"] + args,
                       env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_bench_config3_runs_end_to_end_on_two_ranks(tmp_path):
    """The driver's first N > 1 run must not be the code's first: `bench.py --config 3 --gpus 2` (windows sharded over the
    ranks, one all-gather, blend on every rank) on a 144 x 144 x 96 volume = 4 windows, two per rank in ONE balanced call.
    Its two outputs (2 x 127 MB) are dumped as seeded samples within the 64 MB budget."""
    out = tmp_path / "dump"
    line = _bench_line(["--config", "3", "--steps", "1", "--warmup", "0", "--volume", "144", "144", "96", "--dump-outputs", str(out)], 600)
    assert line["n_gpus"] == 2 and line["config"]["windows"] == 4 and line["scaling"] == "strong"
    assert line["all_gather_seconds"] > 0 and line["gathered_bytes"] == 2 * 2 * 16 * 96 ** 3 * 4
    assert line["value"] > 0 and 0.0 <= line["foreground_fraction"] <= 1.0
    assert sorted(os.listdir(out)) == ["logits.npy", "segmentation.npy"]
    logits, seg = np.load(out / "logits.npy"), np.load(out / "segmentation.npy")
    assert logits.dtype == seg.dtype == np.float32 and logits.ndim == seg.ndim == 1
    assert 0 < logits.nbytes + seg.nbytes <= 64 << 20 and np.isfinite(logits).all() and set(np.unique(seg)) <= {0.0, 1.0}


@pytest.mark.gpu
def test_bench_config4_runs_end_to_end_on_two_ranks(tmp_path):
    """`bench.py --config 4 --gpus 2 --batch 1`: the DDP reducer's bucketed all-reduce under backward, two ranks."""
    out = tmp_path / "dump"
    line = _bench_line(["--config", "4", "--steps", "2", "--warmup", "1", "--batch", "1", "--dump-outputs", str(out)], 900)
    assert np.load(out / "loss.npy").item() == line["loss"]
    assert np.isfinite(np.load(out / "parameters.npy")).all()
    assert line["n_gpus"] == 2 and line["config"]["batch_per_gpu"] == 1
    assert np.isfinite(line["loss"]) and line["value"] > 0 and line["flat_allreduce_seconds"] > 0
    assert line["gradient_bytes"] == 38405520 * 4


@pytest.mark.gpu
def test_bench_config2_runs_end_to_end_on_two_ranks(tmp_path):
    """`bench.py --gpus 2` (the headline config: replicas only, no data-path collective): both ranks replay the --steps steps
    and run the 1000-step loop between barriers, rank 0 prints the contract line with the aggregate of the two replicas and
    alone writes the --dump-outputs files."""
    out = tmp_path / "dump"
    line = _bench_line(["--steps", "5", "--warmup", "2", "--dump-outputs", str(out)], 900)
    assert line["n_gpus"] == 2 and line["scaling"] == "weak" and line["finite"] is True
    assert line["steps"] == 5 and line["warmup"] == 2 and line["ms_per_step"] > 0
    assert line["full_loop"]["steps"] == 1000 and line["full_loop"]["seconds"] > 0 and line["full_loop"]["finite"] is True
    assert abs(line["value"] - 2 * 96 ** 3 / (line["ms_per_step"] * 1e-3)) < 1e-3 * line["value"]
    assert "roofline" not in line
    assert sorted(os.listdir(out)) == ["sample.npy"]
    sample = np.load(out / "sample.npy")
    assert sample.dtype == np.float32 and sample.shape == (1, 16, 96, 96, 96) and np.isfinite(sample).all()
