"""Accuracy of the loss kernels' sigmoid, s = 1 / (1 + __expf(-p)), against float64, measured through the kernel itself.

An fp32 ops.seg_loss_grad call with N = C = 1, V a power of two, the BCE weight only, labels 0 and g = V stores s: 1 / M and g / M
are exact powers of two.  Swept: every finite fp16 value, and a dense fp32 sweep of [-104, 104] (a uniform lattice plus
uniform random points).  Reported: the worst relative error, the worst residual after the argument rounding that arithmetic
explains (1.25 * 2^-24 |p| (1 - s), tests/loss_fp64ref.py), the whole relative error at that point, and what happens below the
smallest normal.  EPS_SIG of tests/loss_fp64ref.py is twice the relative error at the point of the worst residual, rounded up.

    python tools/probe_loss_sigmoid.py [out.json]
"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from diff_unet_amos_amd import ops  # noqa: E402

DEV = "cuda:0"
LOG_V = 20
P_COEF = 1.25 * 2.0 ** -24


def stored_sigmoid(p):
    """p: fp32 [2^LOG_V] on the device -> the s the gradient kernel computed for it."""
    V = p.numel()
    logits = p.view(1, 1, 1, V, 1).contiguous()
    labels = torch.zeros(1, 1, 1, 1, V, device=DEV)
    sums = torch.ones(6, dtype=torch.float64, device=DEV)
    out = ops.seg_loss_grad(logits, labels, sums, torch.tensor(float(V), device=DEV), ("bce",))
    return out.view(-1)


def measure(p):
    V = 1 << LOG_V
    stats = dict(points=int(p.numel()), worst_rel=0.0, worst_rel_at=0.0, worst_residual=0.0, worst_residual_at=0.0,
                 rel_at_worst_residual=0.0, worst_rel_small_p=0.0, tail_abs_over_flt_min=0.0, denormal_outputs=0)
    for lo in range(0, p.numel(), V):
        chunk = p[lo:lo + V]
        n = chunk.numel()
        if n < V:
            chunk = torch.cat([chunk, torch.zeros(V - n, device=DEV)])
        got = stored_sigmoid(chunk)[:n].double()
        x = chunk[:n].double()
        ref = torch.sigmoid(x)
        err = (got - ref).abs()
        body = ref >= 2.0 ** -100                      # below it g / M * s underflows inside the probe itself
        if bool(body.any()):
            rel = torch.where(body, err / ref, torch.zeros_like(err))
            res = rel - P_COEF * x.abs() * (1 - ref)
            k, j = int(rel.argmax()), int(res.argmax())
            if float(rel[k]) > stats["worst_rel"]:
                stats["worst_rel"], stats["worst_rel_at"] = float(rel[k]), float(x[k])
            if float(res[j]) > stats["worst_residual"]:
                stats["worst_residual"], stats["worst_residual_at"] = float(res[j]), float(x[j])
                stats["rel_at_worst_residual"] = float(rel[j])
            small = rel[x.abs() <= 1]
            if small.numel():
                stats["worst_rel_small_p"] = max(stats["worst_rel_small_p"], float(small.max()))
        if bool((~body).any()):
            stats["tail_abs_over_flt_min"] = max(stats["tail_abs_over_flt_min"], float(err[~body].max()) / 2.0 ** -126)
        stats["denormal_outputs"] += int(((got > 0) & (got < 2.0 ** -126)).sum())
    return stats


def main():
    g = torch.Generator(device=DEV).manual_seed(0)
    bits = torch.arange(0, 1 << 16, dtype=torch.int32).to(torch.int16)
    f16 = bits.view(torch.float16)
    f16 = f16[torch.isfinite(f16)].float().to(DEV)
    lattice = torch.linspace(-104.0, 104.0, (1 << 24) + 1, dtype=torch.float64).float().to(DEV)
    rand = (torch.rand(1 << 24, device=DEV, generator=g, dtype=torch.float64) * 208 - 104).float()
    near = (torch.rand(1 << 22, device=DEV, generator=g, dtype=torch.float64) * 36 - 18).float()
    out = dict(fp16_all_finite=measure(f16), fp32_lattice=measure(lattice), fp32_random=measure(rand), fp32_random_18=measure(near))
    worst = max((v for v in out.values() if isinstance(v, dict)), key=lambda v: v["worst_residual"])
    out["worst_residual"], out["rel_at_worst_residual"] = worst["worst_residual"], worst["rel_at_worst_residual"]
    out["eps_sig"] = 2 * out["rel_at_worst_residual"]
    print(json.dumps(out, indent=1))
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
