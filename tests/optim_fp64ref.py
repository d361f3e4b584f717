"""fp64 references and per-element bounds of the gradient-norm / clip / EMA kernels (csrc/train_glue.hip: grads_sumsq,
grad_norm_finish, adamw_step_ex), in the style of tests/glue_fp64ref.py, whose AdamW reference and conventions they build on
(u = 2^-24, DEN = 2^-149, SECOND_ORDER, ``f32`` for the scalars of the C ABI).  A plain helper module (``import optim_fp64ref``).

* Partials.  partials[b] = sum over chunk b (<= 4096 elements) of (double)g (double)g.  Every product is exact in fp64 (24 x 24
  bits), so the reference is ``math.fsum`` of the exact squares, rounded once.  The device adds the n terms of a chunk as a tree
  (16 per lane, six butterfly levels, three adds over the waves); adding a zero is exact, so at most n - 1 additions round, all
  terms are >= 0, and with fsum's own rounding the device is within n 2^-53 of the reference, relatively:
      e_part = n 2^-53 part
* S = the partials in a fixed order: thread t adds ceil(count / 256) of them, the butterfly six more, the waves three.
      e_S = (4096 + ceil(count / 256) + 9 + 1) 2^-53 S                     (non-negative terms: relative errors do not add up)
* norm = fl32(sqrt(S) / scale): the fp64 square root and division round at 2^-53 each, then ONE fp32 rounding.
      e_norm = norm (e_S / (2 S) + 2^-52) + u norm + DEN                  (S = 0: norm = 0 exactly, the bound is DEN)
* coef = min(1, fl(max_norm / fl(norm + 1e-6f))):  d = norm + 1e-6f,  e_d = e_norm + u d;  q = max_norm / d,
      e_q = q e_d / d + u q + DEN;   e_coef = e_q, and where q - e_q >= 1 (or max_norm = inf) the clamp holds on the device
  as well: coef = 1 exactly (bound DEN).  A non-finite S: found_inf = 1, coef = 0 exactly.
* Step.  g' = fl(fl(g inv) c).  fl(g inv) is exact in the reference (glue_fp64ref); the reference multiplies it by ITS coefficient
  in fp64, so the device's g' differs by the rounding of the product and by the coefficient's own error:
      e_g = u |g'| + |fl(g inv)| e_coef + DEN
  It enters adam_one through m and v, and from there as glue_fp64ref's adamw_bound propagates e_m and e_v:
      e_m = 3 u |(1 - b1)(g' - m)| + u |m'| + DEN + (1 - b1) e_g
      e_v = 3 u (1 - b2) g'^2 + u b2 v + u v' + 2 DEN + (1 - b2)(2 |g'| e_g + e_g^2)
* EMA.  e' = fl(e + fl(w fl(p' - e))), w = fl32(1 - rate) formed in double by the caller (an operand, like the betas):
      e_e = 3 u |w (p' - e)| + u |e'| + w e_p + DEN
  (the difference, the product and its operand's rounding; the sum; the error of p' times w).

``emu_*`` restate each kernel's order of operations (fp64 for the norm, torch fp32 for the step) with the planted defects
tests/test_optim_fp64ref.py rejects on the inputs tests/test_optim_gpu.py uses (``make_case``, ``make_norm_grads``).
"""
from __future__ import annotations

import math

import numpy as np
import torch

import glue_fp64ref as GR
from glue_fp64ref import DEN, SECOND_ORDER, U32, f32

F32, F64 = torch.float32, torch.float64
U64 = 2.0 ** -53
CHUNK = GR.AD_CHUNK
EPS_CLIP = f32(1e-6)          # the 1e-6f of clip_grad_norm_ as the kernel holds it


def _cdiv(a, b):
    return -(-a // b)


def chunks_of(tensors):
    """The (tensor index, first element, length) of every workgroup's chunk, in launch order."""
    return [(i, o, min(CHUNK, t.numel() - o)) for i, t in enumerate(tensors) for o in range(0, t.numel(), CHUNK)]


# ---- norm and coefficient ---------------------------------------------------------------------------------------------------------
def partials_ref(tensors):
    """(ref, bound), float64 [chunks]: the exactly rounded sum of the exact squares of every chunk."""
    ref, bnd = [], []
    for i, o, n in chunks_of(tensors):
        x = tensors[i].detach().reshape(-1)[o:o + n].double().cpu().numpy()
        with np.errstate(over="ignore", invalid="ignore"):
            sq = x * x
        s = math.fsum(sq.tolist()) if np.isfinite(sq).all() else float(sq.sum())
        ref.append(s)
        bnd.append(n * U64 * s + 1e-320 if math.isfinite(s) else float("inf"))
    return torch.tensor(ref, dtype=F64), torch.tensor(bnd, dtype=F64)


def norm_ref(partials, scale, max_norm):
    """dict of host floats from the reference's partials: S, norm, coef, found (0 / 1) and the bounds e_norm, e_coef;
    ``scale``: the fp32 loss scale or None."""
    count = partials.numel()
    S = math.fsum(partials.tolist()) if bool(torch.isfinite(partials).all()) else float(partials.sum())
    sc = 1.0 if scale is None else f32(scale)
    if not math.isfinite(S):
        return dict(S=S, norm=math.sqrt(S) / sc if S == S else S, coef=0.0, found=1.0, e_norm=0.0, e_coef=0.0)
    norm = math.sqrt(S) / sc
    e_S = (CHUNK + _cdiv(count, 256) + 10) * U64 * S
    e_norm = (norm * (e_S / (2 * S) + 2 * U64) if S > 0 else 0.0) + U32 * norm + DEN
    out = dict(S=S, norm=norm, found=0.0, e_norm=e_norm * SECOND_ORDER)
    d = norm + EPS_CLIP
    if math.isinf(max_norm):
        return dict(out, coef=1.0, e_coef=DEN)
    q = f32(max_norm) / d
    e_q = (q * (e_norm + U32 * d) / d + U32 * q) * SECOND_ORDER + DEN
    return dict(out, coef=min(1.0, q), e_coef=DEN if q - e_q >= 1.0 else e_q)


def max_norms(partials, scale):
    """Clip thresholds around a case's own norm, from the reference: half of it (coef < 1), twice it -- 1.05 times where twice
    leaves fp32 -- and inf (coef == 1).  A zero norm: 1 and inf."""
    n = norm_ref(partials, scale, math.inf)["norm"]
    if n == 0:
        return [1.0, math.inf]
    return [0.5 * n, 2.0 * n if 2.0 * n < 3e38 else 1.05 * n, math.inf]


def _tree64(x):
    """x [..., 64] float64: six xor-shuffle levels -> [...]."""
    for o in (32, 16, 8, 4, 2, 1):
        x = x + x[..., torch.arange(64) ^ o]
    return x[..., 0]


def _waves64(acc):
    """acc [256] float64, one value per thread: the butterfly of each wave, then ((w0 + w1) + w2) + w3."""
    w = _tree64(acc.view(4, 64))
    return float(((w[0] + w[1]) + w[2]) + w[3])


def emu_partials(tensors):
    """grads_sumsq_kernel in float64 on the CPU: lane t owns the elements i of a chunk with (i >> 2) & 255 == t, in ascending i."""
    out = []
    for i, o, n in chunks_of(tensors):
        x = torch.zeros(CHUNK, dtype=F64)
        x[:n] = tensors[i].detach().reshape(-1)[o:o + n].double().cpu()
        x = x.view(4, 256, 4)                      # [piece j][lane t][q]
        acc = torch.zeros(256, dtype=F64)
        for j in range(4):
            for q in range(4):
                acc = acc + x[j, :, q] * x[j, :, q]
        out.append(_waves64(acc))
    return torch.tensor(out, dtype=F64)


def emu_norm_finish(partials, scale, max_norm, defect=None):
    """grad_norm_finish_kernel: (norm, coef, found) as fp32-valued host floats.  ``defect``: scaled_norm (the norm of the
    still-scaled gradients), no_clamp (the coefficient not limited to 1)."""
    count = partials.numel()
    pad = torch.zeros(_cdiv(count, 256) * 256, dtype=F64)
    pad[:count] = partials
    acc = torch.zeros(256, dtype=F64)
    for row in pad.view(-1, 256):
        acc = acc + row
    S = _waves64(acc)
    sc = 1.0 if (scale is None or defect == "scaled_norm") else f32(scale)
    with np.errstate(over="ignore", invalid="ignore"):
        nf = np.float32(np.sqrt(np.float64(S)) / sc)
        if not math.isfinite(S):
            return float(nf), 0.0, 1.0
        q = np.float32(max_norm) / (nf + np.float32(1e-6))
        coef = q if defect == "no_clamp" else min(np.float32(1.0), q)
    return float(nf), float(coef), 0.0


# ---- the step ---------------------------------------------------------------------------------------------------------------------
def ema_w(rate):
    """(float)(1.0 - rate): the fp32 weight the caller hands the kernel."""
    return f32(1.0 - float(rate))


def _step(p, g, m, v, e, k, lr, beta1, beta2, eps, wd, inv_scale, coef, w, fp32_abi=True):
    gu = g.double() * inv_scale
    if fp32_abi:
        gu = gu.float().double()
    gc = gu * coef
    r = GR._adamw(p, gc, m, v, k, lr, beta1, beta2, eps, wd, 1.0, fp32_abi=False)
    if fp32_abi:            # the bias-correction constants as the kernel holds them; g' stays the unrounded fp64 product
        c1, c2 = GR.bias_constants(k, beta1, beta2)
        r["c1"], r["c2"] = c1, c2
        r["q"] = r["r"] / c2
        r["den"] = r["q"] + eps
        r["num"] = (lr / c1) * r["m"]
        r["f"] = r["num"] / r["den"]
        r["p"] = r["p1"] - r["f"]
    r["gu1"] = gu
    if e is not None:
        r["ed"] = w * (r["p"] - e.double())
        r["e"] = e.double() + r["ed"]
    return r


def step_ref(p, g, m, v, e, k, lr, beta1, beta2, eps, wd, inv_scale, coef=1.0, w=None, fp32_abi=True):
    """One adamw_step_ex in float64: (p, m, v, g', e) -- e None without an EMA.  ``coef``: the reference's clip coefficient;
    ``w`` = ema_w(rate).  ``fp32_abi`` as glue_fp64ref.adamw_ref: False is the plain float64 statement of unscale, clip_grad_norm_'s
    multiply, torch.optim.AdamW and update_ema."""
    r = _step(p, g, m, v, e, k, lr, beta1, beta2, eps, wd, inv_scale, coef, w, fp32_abi)
    return r["p"], r["m"], r["v"], r["gu"], r.get("e")


def step_bound(p, g, m, v, e, k, lr, beta1, beta2, eps, wd, inv_scale, coef=1.0, e_coef=0.0, w=None):
    """(bound p, m, v, g', e) of step_ref's results (module docstring)."""
    r = _step(p, g, m, v, e, k, lr, beta1, beta2, eps, wd, inv_scale, coef, w)
    e_g = U32 * r["gu"].abs() + r["gu1"].abs() * e_coef + DEN
    e_p1 = 2 * U32 * r["decay"].abs() + U32 * r["p1"].abs() + DEN
    e_m = 3 * U32 * r["md"].abs() + U32 * r["m"].abs() + DEN + (1.0 - beta1) * e_g
    e_v = (3 * U32 * r["gg"] + U32 * r["bv"].abs() + U32 * r["v"].abs() + 2 * DEN
           + (1.0 - beta2) * (2 * r["gu"].abs() * e_g + e_g * e_g))
    root = r["r"]
    safe = root.clamp_min(1e-300)
    e_r = torch.where(e_v <= 1e-3 * r["v"], e_v / (2 * safe), torch.minimum(e_v / safe, e_v.sqrt())) + U32 * root
    e_q = e_r / r["c2"] + U32 * r["q"] + DEN
    e_den = e_q + U32 * r["den"]
    e_num = 2 * U32 * r["num"].abs() + abs(lr / r["c1"]) * e_m + DEN
    e_f = e_num / r["den"] + r["f"].abs() * e_den / r["den"] + U32 * r["f"].abs() + DEN
    e_p = e_p1 + e_f + U32 * r["p"].abs()
    e_e = None
    if e is not None:
        e_e = (3 * U32 * r["ed"].abs() + U32 * r["e"].abs() + w * e_p + DEN) * SECOND_ORDER
    return e_p * SECOND_ORDER, e_m * SECOND_ORDER, e_v * SECOND_ORDER, e_g * SECOND_ORDER, e_e


def emu_step(p, g, m, v, e, k, lr, beta1, beta2, eps, wd, scale=None, coef=None, rate=None, found=0.0, defect=None):
    """adamw_ex_kernel on one tensor in torch fp32: (p, m, v, g', e).  ``coef``: the fp32 coefficient or None; ``rate``: the EMA
    rate or None.  ``defect``: clip_update (the coefficient scales the update, not the gradient), ema_pre (the EMA of the
    parameter before the update), rate_swapped (rate and 1 - rate exchanged), w_fp32 (1.f - rate formed in fp32), ema_on_skip (a
    skipped step still averages)."""
    _f = GR._f
    t = lambda x: torch.tensor(x, dtype=F32)      # noqa: E731
    p0, e0 = _f(p), (None if e is None else _f(e))
    w = None
    if rate is not None:
        w = np.float32(1.0 - float(rate))
        if defect == "w_fp32":
            w = np.float32(1.0) - np.float32(rate)
        if defect == "rate_swapped":
            w = np.float32(rate)
    if found != 0.0:
        en = e0
        if defect == "ema_on_skip" and e0 is not None:
            en = _f(e0 + _f(t(w) * _f(p0 - e0)))
        return p0, _f(m), _f(v), _f(g), en
    one = np.float32(1.0)
    inv = one if scale is None else one / np.float32(scale)
    gu = _f(_f(g) * t(inv))
    c = None if coef is None else np.float32(coef)
    if c is not None and defect != "clip_update":
        gu = _f(gu * t(c))
    pn, mn, vn, _ = GR.emu_adamw(p, gu, m, v, k, lr, beta1, beta2, eps, wd)
    if c is not None and defect == "clip_update":
        lr32, wd32 = np.float32(lr), np.float32(wd)
        p1 = _f(p0 - _f(t(lr32 * wd32) * p0))
        pn = _f(p1 - _f(t(c) * _f(p1 - pn)))
    en = None
    if e0 is not None:
        src = p0 if defect == "ema_pre" else pn
        en = _f(e0 + _f(t(w) * _f(src - e0)))
    return pn, mn, vn, gu, en


# ---- the inputs the CPU and the GPU file share -------------------------------------------------------------------------------------
SIZES = [1, 3, 4095, 4096, 4097, 2 * 4096 + 513] + [9 + 2 * i for i in range(59)]          # 65 tensors: two by-value lists
GAP = 8                                                                                     # sentinel words between tensors
SENT = 777.25


def layout():
    """(starts, total): every tensor starts on a multiple of four floats of one flat buffer, GAP sentinel words around each."""
    starts, off = [], GAP
    for n in SIZES:
        starts.append(off)
        off += _cdiv(n, 4) * 4 + GAP
    return starts, off


def make_case(seed=12):
    """dict: starts, total, mask (tensor words) and the pristine flat fp32 buffers p, g, m, v, e (CPU), SENT outside the tensors.
    p, g, m, v as glue_fp64ref.make_adam_inputs; e independent of p (|p - e| of the order of |e|: the hardest case for the EMA
    bound to tell a wrong weight), with every 5th element equal to p and every 9th zero."""
    starts, total = layout()
    mask = torch.zeros(total, dtype=torch.bool)
    for s, n in zip(starts, SIZES):
        mask[s:s + n] = True
    p, g, m, v = GR.make_adam_inputs(total, seed)
    e = torch.randn(total, generator=torch.Generator().manual_seed(seed + 1))
    i = torch.arange(total)
    e = torch.where(i % 5 == 2, p, e)
    e = torch.where(i % 9 == 4, torch.zeros_like(e), e)
    flat = [torch.where(mask, x, torch.full_like(x, SENT)) for x in (p, g, m, v, e)]
    return dict(starts=starts, total=total, mask=mask, flat=flat)


def views(flat, starts):
    return [flat[s:s + n] for s, n in zip(starts, SIZES)]


NORM_KINDS = ("random", "extreme", "extreme_scaled", "zero")


def make_norm_grads(kind, seed=3):
    """(flat fp32 gradient buffer, loss scale or None) on the layout above.  random: glue_fp64ref's gradients (1e-20 .. 1e4).
    extreme: one +3e38 and one -1e38 (the fp32 norm stays finite without a scale), subnormals, +-0, FLT_MIN, and tensor 7 all zero.
    extreme_scaled: +-3e38 in many places under a scale of 2^20.  zero: every gradient zero (norm 0, coef 1, nothing NaN)."""
    starts, total = layout()
    mask = torch.zeros(total, dtype=torch.bool)
    for s, n in zip(starts, SIZES):
        mask[s:s + n] = True
    g = GR.make_adam_inputs(total, seed)[1]
    scale = None
    if kind == "zero":
        g = torch.zeros(total)
    elif kind != "random":
        i = torch.arange(total)
        small = torch.tensor([1e-45, -1e-45, 1e-40, -0.0, 2.0 ** -126, 0.0, -3e-39, 1.5])
        g = torch.where(i % 3 == 1, small[i % small.numel()], g)
        g[starts[7]:starts[7] + SIZES[7]] = 0.0
        if kind == "extreme":
            g[starts[2] + 4094] = 3e38
            g[starts[5] + 8192 + 512] = -1e38
        else:
            g = torch.where(i % 17 == 5, torch.where(i % 2 == 0, 3e38, -3e38).float(), g)
            scale = 2.0 ** 20
    return torch.where(mask, g, torch.full_like(g, SENT)), scale
