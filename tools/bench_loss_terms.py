"""Time forward + backward of the fused loss with ce / dice_ce / generalized_dice (csrc/seg_loss_terms.hip) at the config-4 shape.

    python tools/bench_loss_terms.py [--losses mse,bce,dice_ce,generalized_dice] [--combine sum] [--repeats 20] [--warmup 5]
                                     [--rounds 5] [--small] [--out profiles/loss_terms_bench.json]

Operands: fp16 channels-last logits [2, 96, 96, 96, 16] (N(0, 1) values) and fp32 NCDHW labels (one-hot, 30 % of the voxels all
zero), the shape of the config-4 training step.  Paths, all on the same device in one process, in alternating rounds
(``--rounds`` of ``--repeats`` forward + backward pairs each, device events around a whole round, after warm-up of every path; the
statistic is the median round, the spread its min .. max):

    terms        : _SegLoss with ``--losses`` -- the reduce, its fixed-order partial sum, the tail and the gradient pass of
                   csrc/seg_loss_terms.hip;
    terms_ce     : the same with "ce" alone (the cheapest new name: no Dice constants);
    three_term   : _SegLoss with mse,bce,dice -- the existing kernels of csrc/seg_loss.hip: what the extra terms cost over a pass
                   that is already memory bound;
    torch        : the ``--losses`` loss written in torch operators on the device (fp32 from the fp16 logits), forward and
                   autograd backward to the fp16 logits -- what a user without these kernels would run.

And the launches alone, by direct calls of the C entries on preallocated buffers (no autograd, no allocation), the same
rounds: ``reduce`` (the pass and its partial sum), ``gradient`` for ``--losses``, and the three-term ``old_reduce`` /
``old_gradient`` -- with the bytes each must move (logits + labels read; for the gradient also the logits-sized write).

Also reported: the bytes a forward + backward pair must move (logits read twice, labels read twice, the gradient written once)
and the rate they make of each native time; the loss values of ``terms`` and ``torch`` (they must agree).  One JSON line at the
end, also written to ``--out``.
"""
import argparse
import json
import os
import socket
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from diff_unet_amos_amd import _native as nv  # noqa: E402
from diff_unet_amos_amd import ops  # noqa: E402
from diff_unet_amos_amd.training import _SegLoss, parse_losses  # noqa: E402

DEV = "cuda:0"
EPS = 1e-5


def torch_loss(logits, labels, names, combine):
    """losses/loss.py:64-86 over ``names`` in torch operators; logits channels-last [N, D, H, W, Cs], labels [N, C, D, H, W]."""
    C = labels.shape[1]
    p = logits[..., :C].permute(0, 4, 1, 2, 3).float()
    s = torch.sigmoid(p)
    ax = (2, 3, 4)

    def dice():
        return (1.0 - (2.0 * (s * labels).sum(ax) + EPS) / (s.sum(ax) + labels.sum(ax) + EPS)).mean()

    def ce():
        return torch.nn.functional.cross_entropy(p, labels)

    def gdice():
        I, S, Y = (s * labels).sum(ax), s.sum(ax), labels.sum(ax)
        w = torch.reciprocal(Y * Y)
        inf = torch.isinf(w)
        w = torch.where(inf, torch.zeros_like(w), w)
        w = w + inf * w.max(1, keepdim=True).values
        return (1.0 - (2.0 * (w * I).sum(1) + EPS) / ((w * (S + Y)).sum(1) + EPS)).mean()

    term = dict(mse=lambda: ((s - labels) ** 2).mean(),
                bce=lambda: torch.nn.functional.binary_cross_entropy_with_logits(p, labels),
                dice=dice, ce=ce, dice_ce=lambda: dice() + ce(), generalized_dice=gdice)
    terms = [term[n]() for n in names]
    total = torch.stack(terms).sum()
    if len(terms) > 1 and combine == "mean":
        return total / len(terms)
    if len(terms) > 1 and combine == "log":
        return torch.log(1 + total)
    return total


def native_pair(logits, labels, names, combine):
    x = logits.detach().requires_grad_(True)
    L = _SegLoss.apply(x, labels, names, combine)
    L.backward()
    return L.detach(), x.grad


def torch_pair(logits, labels, names, combine):
    x = logits.detach().requires_grad_(True)
    L = torch_loss(x, labels, names, combine)
    L.backward()
    return L.detach(), x.grad


class DirectTerms:
    """The launches alone: dua_seg_loss_terms_* and the three-term entries on buffers allocated once."""

    def __init__(self, logits, labels):
        self.N, self.C = labels.shape[:2]
        self.V = labels[0, 0].numel()
        self.logits, self.labels = logits, labels
        self.sums = torch.empty(self.N * self.C * 4 + 3, dtype=torch.float64, device=DEV)
        self.consts = torch.empty(self.N * self.C * 2, dtype=torch.float32, device=DEV)
        self.nbytes = int(nv.lib().dua_seg_loss_terms_scratch_bytes(self.N, self.C, self.V))
        self.scratch = torch.empty(self.nbytes // 8, dtype=torch.float64, device=DEV)
        self.out = torch.empty(2, dtype=torch.float32, device=DEV)
        self.grad = torch.empty_like(logits)
        self.old_sums = torch.zeros(self.N * self.C * 4 + 2, dtype=torch.float64, device=DEV)

    def reduce(self):
        L, N, C, V = nv.lib(), self.N, self.C, self.V
        nv.check(L.dua_seg_loss_terms_reduce(nv.dt_code(self.logits.dtype), N, C, V, nv.ptr(self.logits), self.logits.shape[-1],
                                             nv.ptr(self.labels), nv.ptr(self.sums), nv.ptr(self.scratch), self.nbytes,
                                             nv.stream_ptr()), "reduce")

    def finish(self, use):
        nv.check(nv.lib().dua_seg_loss_terms_finish(self.N, self.C, self.V, *use, 0, None, 0, nv.ptr(self.sums), nv.ptr(self.out[0:]),
                                                    nv.ptr(self.out[1:]), nv.ptr(self.consts), nv.stream_ptr()), "finish")

    def gradient(self, use):
        nv.check(nv.lib().dua_seg_loss_terms_grad(nv.dt_code(self.logits.dtype), self.N, self.C, self.V, nv.ptr(self.logits),
                                                  self.logits.shape[-1], nv.ptr(self.labels), nv.ptr(self.consts), nv.ptr(self.out[1:]),
                                                  *use, nv.ptr(self.grad), self.grad.shape[-1], nv.stream_ptr()), "grad")

    def old_reduce(self):
        """dua_seg_loss_reduce accumulating into sums that are never cleared: the values are not used."""
        nv.check(nv.lib().dua_seg_loss_reduce(nv.dt_code(self.logits.dtype), self.N, self.C, self.V, nv.ptr(self.logits),
                                              self.logits.shape[-1], nv.ptr(self.labels), nv.ptr(self.old_sums), nv.stream_ptr()),
                 "old reduce")

    def old_gradient(self):
        nv.check(nv.lib().dua_seg_loss_grad(nv.dt_code(self.logits.dtype), self.N, self.C, self.V, nv.ptr(self.logits),
                                            self.logits.shape[-1], nv.ptr(self.labels), nv.ptr(self.old_sums), None, 1.0, 1.0, 1.0,
                                            nv.ptr(self.grad), self.grad.shape[-1], nv.stream_ptr()), "old grad")


def timed(fn, repeats):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(repeats):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / repeats * 1e3                     # microseconds per forward + backward pair


def stats(rounds):
    return dict(median_us=round(statistics.median(rounds), 1), min_us=round(min(rounds), 1), max_us=round(max(rounds), 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--losses", default="mse,bce,dice_ce,generalized_dice")
    ap.add_argument("--combine", default="sum")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--small", action="store_true", help="2 x 16 x 24^3: a rehearsal of the tool, not a measurement")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    names, combine = parse_losses(args.losses, args.combine)
    assert "multi_neighbor" not in names and any(n in ops.EXT_LOSS_NAMES for n in names), "--losses: at least one new name, no multi_neighbor"
    if not torch.cuda.is_available():
        sys.exit("bench_loss_terms: no GPU: nothing is measured on a CPU")
    N, C, S = 2, 16, (24 if args.small else 96)
    g = torch.Generator(device=DEV).manual_seed(0)
    logits = torch.randn((N, S, S, S, C), generator=g, device=DEV).half()
    cls = torch.randint(0, C, (N, S, S, S), generator=g, device=DEV)
    labels = torch.nn.functional.one_hot(cls, C).permute(0, 4, 1, 2, 3).float()
    labels = (labels * (torch.rand((N, 1, S, S, S), generator=g, device=DEV) >= 0.3)).contiguous()
    del cls
    direct = DirectTerms(logits, labels)
    use = tuple(int(n in names) for n in ops.TERM_LOSS_NAMES)
    direct.reduce(); direct.finish(use)
    launches = {"reduce": direct.reduce, "gradient": lambda: direct.gradient(use), "old_reduce": direct.old_reduce,
                "old_gradient": direct.old_gradient}
    paths = {"terms": lambda: native_pair(logits, labels, names, combine),
             "terms_ce": lambda: native_pair(logits, labels, ("ce",), "sum"),
             "three_term": lambda: native_pair(logits, labels, ops.LOSS_NAMES, "sum"),
             "torch": lambda: torch_pair(logits, labels, names, combine)}
    L_native, g_native = paths["terms"]()
    L_torch, g_torch = paths["torch"]()
    L_three, _ = paths["three_term"]()
    values = dict(terms=float(L_native), torch=float(L_torch), three_term=float(L_three))
    grad_diff = float((g_native.float() - g_torch.float()).abs().max())
    del g_native, g_torch
    both = {**paths, **launches}
    for fn in both.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    rounds = {k: [] for k in both}
    for _ in range(args.rounds):
        for k, fn in both.items():
            rounds[k].append(timed(fn, args.repeats))
    V = S ** 3
    pair_bytes = 2 * (N * V * C * 2 + N * C * V * 4) + N * V * C * 2
    result = dict(host=socket.gethostname(), device=torch.cuda.get_device_name(0), shape=[N, S, S, S, C], dtype="float16",
                  losses=list(names), combine=combine, repeats=args.repeats, rounds=args.rounds, warmup=args.warmup,
                  pair_bytes=pair_bytes, loss_values=values, largest_gradient_difference_to_torch=grad_diff)
    for k in paths:
        result[k] = stats(rounds[k])
        if k != "torch":
            result[k]["gbytes_per_s"] = round(pair_bytes / result[k]["median_us"] / 1e3, 1)
    read_bytes = N * V * C * 2 + N * C * V * 4
    result["launches"] = {}
    for k in launches:
        nbytes = read_bytes + (N * V * C * 2 if "gradient" in k else 0)
        result["launches"][k] = dict(stats(rounds[k]), bytes=nbytes, gbytes_per_s=round(nbytes / statistics.median(rounds[k]) / 1e3, 1))
    result["terms_over_three_term"] = round(result["terms"]["median_us"] / result["three_term"]["median_us"], 3)
    result["torch_over_terms"] = round(result["torch"]["median_us"] / result["terms"]["median_us"], 2)
    print("   ".join(f"{k} {result[k]['median_us']:9.1f} us" for k in paths), flush=True)
    print("   ".join(f"{k} {v['median_us']:9.1f} us ({v['gbytes_per_s']} GB/s)" for k, v in result["launches"].items()), flush=True)
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
