"""The optimizer phase of a training step alone, on the full config-4 parameter set (DiffUNet, 16 classes), three forms
interleaved in one process:
  (a) grads_nonfinite + adamw_step + adamw_advance                      the step without the options        32 B / parameter
  (b) grad_norm + adamw_step with clip and EMA + adamw_advance          the options in the library's launches   40 B / parameter
  (c) _amp_foreach_non_finite_check_and_unscale_, clip_grad_norm_(foreach=True), fused torch.optim.AdamW, _foreach_mul_ /
      _foreach_add_                                                     the same in torch operators        ~68 B / parameter
Bytes per parameter, from what each pass reads and writes: (a) check 4 + AdamW 28 (p, m, v read and written, g read);
(b) norm 4 + AdamW 28 + EMA 8; (c) unscale 8 + norm 4 + clip 8 + AdamW 28 + mul_ 8 + add_ 12.
Every form runs ``--rounds`` times in turn (a, b, c, a, b, c, ...), each timed by device events around ``--reps`` back-to-back
phases; the medians, the spread and the ratios go out as one JSON line.
Usage: python tools/bench_optim.py [--rounds 20] [--reps 10] [--classes 16]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from diff_unet_amos_amd import ops          # noqa: E402
from diff_unet_amos_amd.diff_unet import DiffUNet          # noqa: E402
from diff_unet_amos_amd.training import NativeAdamW          # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=20)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--classes", type=int, default=16)
ap.add_argument("--max-grad-norm", type=float, default=12.0)
ap.add_argument("--ema-rate", type=float, default=0.9999)
a = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_optim.py times device launches: it needs a GPU")
dev = torch.device("cuda:0")
torch.manual_seed(0)
BYTES = {"a": 32, "b": 40, "c": 68}


def parameter_set():
    net = DiffUNet(in_channels=1, out_channels=a.classes).to(dev)
    ps = [p for p in net.parameters() if p.requires_grad]
    for p in ps:
        p.grad = torch.randn_like(p) * 1024.0            # a loss-scaled gradient
    return ps


scale = torch.full((), 1024.0, device=dev)
flag, growth, seen = torch.zeros((), device=dev), torch.zeros((), dtype=torch.int32, device=dev), torch.zeros((), device=dev)

# (a) and (b): the library's optimizer, each on its own copy of the parameters
pa, pb, pc = parameter_set(), parameter_set(), parameter_set()
numel = sum(p.numel() for p in pa)
opt_a, opt_b = NativeAdamW(pa, lr=2e-4, weight_decay=1e-4), NativeAdamW(pb, lr=2e-4, weight_decay=1e-4)
opt_a.materialize_state(); opt_b.materialize_state()
ema_b = [p.detach().clone() for p in pb]
norm, coef = torch.zeros((), device=dev), torch.ones((), device=dev)
partials = torch.zeros(ops.grad_norm_partials(pb), dtype=torch.float64, device=dev)


def form_a():
    ops.grads_nonfinite([p.grad for p in pa], flag)
    opt_a.step(grad_scale=scale, found_inf=flag, advance=False)
    ops.adamw_advance(opt_a._count, flag, scale, growth, 2.0, 0.5, 1 << 30, seen=seen)


def form_b():
    grads = [p.grad for p in pb]
    ops.grad_norm(grads, a.max_grad_norm, grad_scale=scale, found_inf=flag, norm=norm, coef=coef, partials=partials)
    opt_b.step(grad_scale=scale, found_inf=flag, advance=False, clip_coef=coef, ema=ema_b, ema_rate=a.ema_rate)
    ops.adamw_advance(opt_b._count, flag, scale, growth, 2.0, 0.5, 1 << 30, seen=seen)


# (c): torch operators.  The gradients are unscaled in place, so every phase multiplies them back afterwards -- outside no timing,
# inside the event pair: the restore is one _foreach_mul_ (8 B / parameter) that form (c) does not need in a real step, measured
# separately and subtracted.
opt_c = torch.optim.AdamW(pc, lr=2e-4, weight_decay=1e-4, fused=True)
ema_c = [p.detach().clone() for p in pc]
found_c, inv_c = torch.zeros(1, device=dev), torch.full((1,), 1.0 / 1024.0, device=dev)


def form_c():
    grads = [p.grad for p in pc]
    torch._amp_foreach_non_finite_check_and_unscale_(grads, found_c, inv_c)
    torch.nn.utils.clip_grad_norm_(pc, a.max_grad_norm, foreach=True)
    opt_c.step()
    with torch.no_grad():
        torch._foreach_mul_(ema_c, a.ema_rate)
        torch._foreach_add_(ema_c, [p.detach() for p in pc], alpha=1 - a.ema_rate)


def restore_c():
    with torch.no_grad():
        torch._foreach_mul_([p.grad for p in pc], 1024.0)


def timed(fn, reps, after=None):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
        if after is not None:
            after()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / reps          # ms per phase


forms = {"a": (form_a, None), "b": (form_b, None), "c": (form_c, restore_c), "restore": (restore_c, None)}
for fn, after in forms.values():                # warm-up: code objects, optimizer state
    timed(fn, 3, after)
times = {k: [] for k in forms}
for _ in range(a.rounds):
    for k, (fn, after) in forms.items():
        times[k].append(timed(fn, a.reps, after))


def med(xs):
    return sorted(xs)[len(xs) // 2]


m = {k: med(v) for k, v in times.items()}
m["c"] -= m["restore"]
out = {"metric": "optimizer_phase_time", "unit": "ms", "parameters": numel, "tensors": len(pa), "rounds": a.rounds, "reps": a.reps,
       "max_grad_norm": a.max_grad_norm, "ema_rate": a.ema_rate, "grad_norm": float(norm), "clip_coef": float(coef)}
for k in "abc":
    lo, hi = min(times[k]), max(times[k])
    off = m["restore"] if k == "c" else 0.0
    out[k] = {"median_ms": round(m[k], 4), "min_ms": round(lo - off, 4), "max_ms": round(hi - off, 4), "bytes_per_parameter": BYTES[k],
              "GB_per_s": round(BYTES[k] * numel / (m[k] * 1e-3) / 1e9, 1)}
out["b_over_a"] = round(m["b"] / m["a"], 3)
out["c_over_b"] = round(m["c"] / m["b"], 3)
out["restore_ms"] = round(m["restore"], 4)
print(json.dumps(out))
