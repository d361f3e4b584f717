"""Time Step-Uncertainty Fusion (SUF) of R DDIM runs of one window, three ways, and the fusion launch on its own.

    python tools/bench_suf.py [--patch 96] [--classes 16] [--steps 10] [--runs 4] [--repeats 7] [--warmup 2] [--kernel-iters 50]

One DiffUNet (default widths, fp16) and one window; per repeat, alternating the forms, a host clock around the call ending in
a device synchronise:
  fused   : DiffUNet(uncer_step=R) through forward(image, pred_type="ddim_sample"): R encoder passes, then T replays of one
            captured graph holding the batch-R step (its tail writing the logits) and dua_suf_accumulate.
  by_hand : what one writes without the fused loop: one encoder pass, R loops at batch 1 stepping the launch plan eagerly with
            every step's logits copied out (2 R T tensors kept, as the original code does), then
            gaussian_diffusion.step_uncertainty_fusion on them.
  plain   : the un-fused call (uncer_step=None) on the window repeated R times: the same R encoder passes and batch-R steps
            without logits and without the fusion -- the floor the fused form sits on.
Then dua_suf_accumulate alone on the loop's own buffers, --kernel-iters launches between two device events, and its achieved
bytes per second against the derived (R + 2) C voxels 4 bytes per launch.  The fused result is compared with the by-hand one
(different x_T, so only shape and range are compared) -- correctness is the test suite's business."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from diff_unet_amos_amd import _native as nv  # noqa: E402
from diff_unet_amos_amd import ops  # noqa: E402
from diff_unet_amos_amd.diff_unet import DiffUNet  # noqa: E402
from diff_unet_amos_amd.gaussian_diffusion import step_uncertainty_fusion, suf_step_coef  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--patch", type=int, default=96)
    ap.add_argument("--classes", type=int, default=16)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--runs", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--kernel-iters", type=int, default=50)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_suf.py measures on an MI355X; no GPU here")
    dev = torch.device("cuda", 0)
    R, T, Cn, dims = args.runs, args.steps, args.classes, (args.patch,) * 3
    torch.manual_seed(0)
    net = DiffUNet(in_channels=1, out_channels=Cn, sample_steps=T, compute_dtype=torch.float16).to(dev).eval()
    image = torch.rand(1, 1, *dims, device=dev)
    d = net.sample_diffusion

    def fused():
        net.uncer_step = R
        return net(image, pred_type="ddim_sample")

    def plain():
        net.uncer_step = None
        return net(image.repeat_interleave(R, dim=0), pred_type="ddim_sample")

    def by_hand():
        net.embed_model(image)
        plan = net._rt.plan(1, dims, dev)
        coef_table, row_of_step = plan._step_tables(d, "ddim", 0.0)
        logits = torch.empty(1, Cn, *dims, device=dev)
        outs, xs = [], []
        for _ in range(R):
            plan._reset(torch.randn(1, Cn, *dims, device=dev))
            plan.new_seed()
            outs.append([]); xs.append([])
            for _ in range(T):
                plan._one_step_logits(nv.MODE_DDIM, row_of_step, coef_table, None, logits)
                outs[-1].append(logits.clone())
                xs[-1].append(logits.clamp(-1, 1))
        return step_uncertainty_fusion(outs, xs)

    def run(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.no_grad():
            out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    forms = {"fused": fused, "by_hand": by_hand, "plain": plain}
    for _ in range(args.warmup):
        for fn in forms.values():
            run(fn)
    times = {k: [] for k in forms}
    outs = {}
    for _ in range(args.repeats):                                  # alternate the forms
        for k, fn in forms.items():
            t, outs[k] = run(fn)
            times[k].append(t)

    # the fusion launch alone, on buffers the size of the loop's
    vox = dims[0] * dims[1] * dims[2]
    logits = torch.randn(R, Cn, *dims, device=dev) * 3
    acc = torch.zeros(1, Cn, *dims, device=dev)
    coef = suf_step_coef(T, dev)
    word = torch.tensor([T // 2], dtype=torch.int32, device=dev)
    for _ in range(5):
        ops.suf_accumulate(logits, acc, coef, step_word=word)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(args.kernel_iters):
        ops.suf_accumulate(logits, acc, coef, step_word=word)
    e1.record()
    torch.cuda.synchronize()
    launch_s = e0.elapsed_time(e1) * 1e-3 / args.kernel_iters
    launch_bytes = (R + 2) * Cn * vox * 4

    summary = lambda v: {"median": statistics.median(v), "min": min(v), "max": max(v)}      # noqa: E731
    print(json.dumps({
        "plan": {"patch": list(dims), "classes": Cn, "steps": T, "runs": R, "dtype": "float16"},
        "device": torch.cuda.get_device_name(dev), "warmup": args.warmup, "repeats": args.repeats,
        "fused_seconds": summary(times["fused"]), "by_hand_seconds": summary(times["by_hand"]),
        "plain_batch_R_seconds": summary(times["plain"]),
        "fused_minus_plain_seconds_per_step": (statistics.median(times["fused"]) - statistics.median(times["plain"])) / T,
        "accumulate_launch": {"iters": args.kernel_iters, "seconds": launch_s, "bytes_derived": launch_bytes,
                              "bytes_per_second": launch_bytes / launch_s,
                              "tail_logits_bytes_per_step_derived": R * Cn * vox * 4},
        "fused_shape": list(outs["fused"].shape), "fused_abs_max": float(outs["fused"].abs().max()),
        "by_hand_abs_max": float(outs["by_hand"].abs().max()),
    }))


if __name__ == "__main__":
    main()
