"""Config 4 (training step, batch 2, 96^3, 16 classes) on the HIP training path (training.NativeConvTrainer): eager or
as one replayed HIP graph.  One JSON line.
Usage: python tools/bench_train.py [--steps K] [--graph] [--losses mse,bce,multi_neighbor,dice | mse,dice_ce,generalized_dice | ...] [--loss-combine sum]
       [--max-grad-norm 12] [--ema-rate 0.9999] [--boundary-weight 0.01 [--rounds 5]]
--boundary-weight A: the step with the boundary term (NativeConvTrainer(boundary_weight=A): signed distance maps of the labels,
one more reduce pass, the term in the gradient pass) against the same step without it: two trainers on copies of one network in
ONE process, on argmax-partition labels (tools/bench_sdf.py), timed in alternating blocks of --steps steps, --rounds times."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from diff_unet_amos_amd.diff_unet import DiffUNet          # noqa: E402
from diff_unet_amos_amd.training import NativeConvTrainer         # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--batch", type=int, default=2)
ap.add_argument("--classes", type=int, default=16)
ap.add_argument("--size", type=int, default=96)
ap.add_argument("--dtype", default="float16")
ap.add_argument("--graph", action="store_true", help="replay the whole training step as one HIP graph")
ap.add_argument("--losses", default="mse,bce,dice", help="loss names (losses/loss.py): any of mse, bce, dice, multi_neighbor, ce, dice_ce, generalized_dice; "
                "cfg/amos/train.yaml: mse,bce,multi_neighbor,dice")
ap.add_argument("--loss-combine", default="sum", choices=("sum", "mean", "log"))
ap.add_argument("--max-grad-norm", type=float, default=None, help="clip the global gradient norm (inf: measure it only)")
ap.add_argument("--ema-rate", type=float, default=None, help="keep an EMA of the weights at this rate")
ap.add_argument("--boundary-weight", type=float, default=None, help="A/B the step with the boundary term at this weight against the step without it")
ap.add_argument("--rounds", type=int, default=5, help="alternating blocks per arm of the --boundary-weight comparison")
ap.add_argument("--no-gc", action="store_true", help="disable the Python cyclic GC during the timed loop (diagnosis)")
ap.add_argument("--ab-wgrad", default="", help="comma list of weight-gradient launch forms (dua_conv3_desc.policy, ops.WGRAD_POLICY): time the loop once per value, same process")
a = ap.parse_args()
dev = torch.device("cuda:0")
torch.manual_seed(0)
net = DiffUNet(in_channels=1, out_channels=a.classes).to(dev)
tr = NativeConvTrainer(net, dtype=getattr(torch, a.dtype), graph=a.graph, losses=a.losses, loss_combine=a.loss_combine,
                       max_grad_norm=a.max_grad_norm, ema_rate=a.ema_rate)
image = torch.rand(a.batch, 1, a.size, a.size, a.size, device=dev)
labels = (torch.rand(a.batch, a.classes, a.size, a.size, a.size, device=dev) > 0.8).float()
for _ in range(a.warmup):
    tr.step(image, labels)
torch.cuda.synchronize()
if a.no_gc:
    import gc
    gc.collect()
    gc.disable()
per = []
for _ in range(a.steps):
    t0 = time.perf_counter()
    loss = tr.step(image, labels)
    torch.cuda.synchronize()
    per.append(time.perf_counter() - t0)
dt = sum(per) / len(per)
ab = {}
if a.ab_wgrad:
    from diff_unet_amos_amd import ops
    for v in [int(x) for x in a.ab_wgrad.split(",")]:
        ops.WGRAD_POLICY = v
        tr.step(image, labels)
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.steps):
            t0 = time.perf_counter()
            tr.step(image, labels)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        ab.setdefault(str(v), []).append(round(sorted(ts)[len(ts) // 2] * 1e3, 2))
    ops.WGRAD_POLICY = 0
bnd = None
if a.boundary_weight is not None:
    import copy
    from bench_sdf import partition_labels
    labels_b = torch.from_numpy(partition_labels(a.batch, a.classes, a.size)).to(dev)
    torch.manual_seed(0)
    base = DiffUNet(in_channels=1, out_channels=a.classes).to(dev)
    kw = dict(dtype=getattr(torch, a.dtype), graph=a.graph, losses=a.losses, loss_combine=a.loss_combine,
              max_grad_norm=a.max_grad_norm, ema_rate=a.ema_rate)
    arms = {"without": NativeConvTrainer(copy.deepcopy(base), **kw),
            "with": NativeConvTrainer(copy.deepcopy(base), boundary_weight=a.boundary_weight, **kw)}
    for t in arms.values():
        for _ in range(a.warmup):
            t.step(image, labels_b)
    torch.cuda.synchronize()
    blocks = {k: [] for k in arms}
    for _ in range(a.rounds):
        for k, t in arms.items():
            t0 = time.perf_counter()
            for _ in range(a.steps):
                t.step(image, labels_b)
            torch.cuda.synchronize()
            blocks[k].append((time.perf_counter() - t0) / a.steps * 1e3)
    med = {k: sorted(v)[len(v) // 2] for k, v in blocks.items()}
    bnd = {"weight": a.boundary_weight, "labels": "argmax partition", "rounds": a.rounds, "steps_per_block": a.steps,
           "median_ms": {k: round(v, 3) for k, v in med.items()}, "min_ms": {k: round(min(v), 3) for k, v in blocks.items()},
           "block_ms": {k: [round(x, 3) for x in v] for k, v in blocks.items()},
           "added_ms_median": round(med["with"] - med["without"], 3), "boundary_term": float(arms["with"].boundary_term())}
print(json.dumps({"metric": "train_step_time", **({"boundary": bnd} if bnd is not None else {}), "value": dt * 1e3, "unit": "ms", "median_ms": sorted(per)[len(per) // 2] * 1e3, "per_step_ms": [round(x * 1e3, 2) for x in per], "ab_wgrad_median_ms": ab, "native": True,
                  "path": "HIP conv fwd/dgrad/wgrad + fused InstanceNorm/LeakyReLU/add fwd/bwd under autograd; fused loss, pooling, 1x1-head and transposed-conv (in-place concat) kernels; AdamW = torch; " + a.dtype,
                  "graph": a.graph, "batch": a.batch,
                  "size": a.size, "classes": a.classes, "max_grad_norm": a.max_grad_norm, "ema_rate": a.ema_rate,
                  "grad_norm": tr.grad_norm() if a.max_grad_norm is not None else None, "losses": a.losses, "loss_combine": a.loss_combine, "loss": float(loss),
                  "max_mem_GiB": torch.cuda.max_memory_allocated() / 2**30}))
