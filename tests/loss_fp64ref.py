"""fp64 references of the fused segmentation loss (csrc/seg_loss.hip, the seg_loss_finish[_mn] tail of csrc/train_glue.hip) and
per-sum / per-element error bounds, in the style of tests/fp64ref.py.  A plain helper module (``import loss_fp64ref``).

The references are evaluated in float64 on the exact operands a kernel read: the fp16 / fp32 logits as stored (channels-last
[N, D, H, W, Cs], first C channels), the fp32 labels as stored ([N, C, D, H, W]), and -- for the tail and the gradient -- the
fp64 ``sums`` (and multi_neighbor partials) the device produced.  All tensors stay on the device of the logits, so the full-size
cases evaluate on the GPU's fp64 units.  Per-element quantities are [N, C, V].

Bounds (derived from the kernels' arithmetic; u = 2^-24):

* sigmoid.  s = 1 / (1 + __expf(-p)) compiles (-O3 -ffp-contract=off, gfx950) to v_mul_f32 by -log2(e) rounded to fp32,
  v_exp_f32, an add, and an IEEE division (v_div_scale / v_div_fmas / v_div_fixup: correctly rounded, denormals kept).  The
  rounded product and the rounded constant move the exponent's argument by at most |p| (2^-24 + 1.3e-8) <= 1.25 u |p| relative
  in e^-p, which reaches s scaled by (1 - s).  The hardware exponential, the add and the division are covered by EPS_SIG (the
  one measured constant, below).  v_exp_f32 does not produce denormals and overflows to +inf above 2^128, where s becomes 0
  while the true s is below the smallest normal: + 2^-126.
      e_s = s (1.25 u |p| (1 - s) + EPS_SIG) + 2^-126
* softplus.  log1pf(__expf(-|p|)): the exponential's relative error d reaches log1p(e) as e / (1 + e) d <= log1p(e) d; log1pf
  itself is within 2 ulp (the OpenCL accuracy its library implements): 4 u.
* reduce.  A thread adds ceil(V / (G 256)) terms per channel, G = min(512, ceil(V / 256)) workgroups per sample (C times that
  many for the squared-error and BCE accumulators, which run over all channels), then six shuffle levels; fp64 after that.
  A chain of n additions is off by at most n u sum |terms| (first order).  The terms carry their own errors: s y rounds once
  and inherits e_s, (s - y)^2 inherits 2 |d| (e_s + u |d|), a BCE term three roundings of its parts and the softplus error.
  With binary labels the products s y and the sum of y are exact in fp32 (integers below 2^24); the bound does not use that:
  it is the soft-label bound, valid for both.
* tail.  L and dcomb are fp64 expressions of the sums, rounded once to fp32.
* gradient.  Per element, from the fp32 operations of seg_loss_grad_kernel (grad_bound counts them), then the rounding of the
  stored value u_out |ref| + floor_out (2^-11, 2^-25 for fp16: subnormals are kept, so a store that flushes them fails).
  Nothing is normalised by the tensor's maximum.

``check`` is fp64ref.check (max(|err| / bound) and the worst element) behind a layout shim.
"""
from __future__ import annotations

import itertools
import math

import numpy as np
import torch

import fp64ref
from fp64ref import FLOOR16, FLOOR32, U16, U32, CheckResult, unit   # noqa: F401  (re-exported for the tests)

EPS_DICE = 1e-5
P_COEF = 1.25 * U32
FLT_MIN = 2.0 ** -126
EPS_SIG = 2.0 * 1.24e-7
"""Relative error allowed for v_exp_f32 + the add + the division of the kernels' sigmoid: twice the worst error measured against
float64 on an MI355X with tools/probe_loss_sigmoid.py (1.237e-7 at p = -0.043, where the argument's rounding explains only
1.6e-9 of it; DESIGN.md section 10e, "Loss kernels: fp64 check": the sweep, the measured values, this constant).  The only
number in this module that comes from a measurement."""
LOG1P_ULPS = 4 * U32
SECOND_ORDER = 1.001          # first-order bounds times this: products of two relative errors of <= 1e-4 each
LOG2E_32 = float(np.float32(1.4426950408889634))
LOSS_NAMES = ("mse", "bce", "dice")


def check(got, ref, bnd):
    """fp64ref.check on tensors of any layout (the [N, C, V] views of channels-last buffers are not contiguous)."""
    return fp64ref.check(got.double().contiguous(), ref.double().contiguous(), bnd.double().contiguous())


def _cdiv(a, b):
    return -(-a // b)


def reduce_geometry(V):
    """(workgroups per sample, additions per thread and channel) of dua_seg_loss_reduce."""
    G = min(512, _cdiv(V, 256))
    return G, _cdiv(V, G * 256)


def grad_geometry(V):
    G = min(4096, _cdiv(V, 256))
    return G, _cdiv(V, G * 256)


def operands(logits, labels):
    """The kernels' operands as float64 [N, C, V] on the logits' device: p (a view), y."""
    N, C = labels.shape[:2]
    V = labels[0, 0].numel()
    p = logits.reshape(N, V, logits.shape[-1])[..., :C].double().permute(0, 2, 1)
    return p, labels.to(logits.device).reshape(N, C, V).double()


def sigmoid_err(p, s):
    return s * (P_COEF * p.abs() * (1 - s) + EPS_SIG) + FLT_MIN


# ---- reduce --------------------------------------------------------------------------------------------------------------------
def reduce_ref(logits, labels):
    """I = sum s y, S = sum s, Y = sum y per (n, c); sum (s - y)^2 and sum BCE over everything; with each the sum of |terms| and
    the sum of the terms' own errors (module docstring) that reduce_bound needs."""
    p, y = operands(logits, labels)
    N, C, V = p.shape
    s = torch.sigmoid(p)
    es = sigmoid_err(p, s)
    r = dict(N=N, C=C, V=V)
    sy = s * y
    r["I"], r["I_abs"], r["I_err"] = sy.sum(2), sy.abs().sum(2), (y.abs() * es + U32 * sy.abs()).sum(2)
    r["S"], r["S_abs"], r["S_err"] = s.sum(2), s.sum(2), es.sum(2)
    r["Y"], r["Y_abs"], r["Y_err"] = y.sum(2), y.abs().sum(2), torch.zeros_like(r["S"])
    del sy
    d = s - y
    r["mse"], r["mse_abs"], r["mse_err"] = (d * d).sum(), (d * d).sum(), (2 * d.abs() * (es + U32 * d.abs())).sum()
    del d
    sp = torch.log1p(torch.exp(-p.abs()))
    hinge, py = p.clamp_min(0), p * y
    b = hinge - py + sp
    parts = hinge + py.abs() + sp
    r["bce"], r["bce_abs"] = b.sum(), b.abs().sum()
    r["bce_err"] = (3 * U32 * parts + sp * (P_COEF * p.abs() + EPS_SIG + LOG1P_ULPS)).sum()
    return r


def ref_sums(r):
    """The reference's sums in the layout of the device buffer: [N * C * 4 + 2] (I, S, Y, 0 per (n, c), then mse, bce)."""
    per = torch.stack([r["I"], r["S"], r["Y"], torch.zeros_like(r["I"])], -1).reshape(-1)
    return torch.cat([per, torch.stack([r["mse"], r["bce"]])])


def reduce_bound(r):
    """Per-sum limit for the fp64 ``sums`` buffer of ops.seg_loss_reduce, in its layout (the unused fourth word: ~0)."""
    _, n = reduce_geometry(r["V"])
    per_c, all_c = U32 * (n + 6), U32 * (n * r["C"] + 6)
    f64 = 2.0 ** -45           # the fp64 atomics and the four-wave sum: far below every fp32 term
    bI = (r["I_err"] + (per_c + f64) * r["I_abs"]) * SECOND_ORDER + FLOOR32
    bS = (r["S_err"] + (per_c + f64) * r["S_abs"]) * SECOND_ORDER + FLOOR32
    bY = (r["Y_err"] + (per_c + f64) * r["Y_abs"]) * SECOND_ORDER + FLOOR32
    per = torch.stack([bI, bS, bY, torch.full_like(bI, 1e-300)], -1).reshape(-1)
    bm = (r["mse_err"] + (all_c + f64) * r["mse_abs"]) * SECOND_ORDER + FLOOR32
    bb = (r["bce_err"] + (all_c + f64) * r["bce_abs"]) * SECOND_ORDER + FLOOR32
    return torch.cat([per, torch.stack([bm, bb])])


# ---- tail ------------------------------------------------------------------------------------------------------------------------
def finish_ref(sums, N, C, V, names, combine, mn=None):
    """(L, dcomb) in float64 from the sums the tail read (the device's ``sums`` and multi_neighbor partials [N, K + 1] copied
    back, or a reference's): losses/loss.py:64-86."""
    sums = sums.double().cpu()
    q = sums[:N * C * 4].view(N * C, 4)
    terms = []
    if "mse" in names:
        terms.append(sums[N * C * 4] / (N * C * V))
    if "bce" in names:
        terms.append(sums[N * C * 4 + 1] / (N * C * V))
    if "dice" in names:
        terms.append((1.0 - (2.0 * q[:, 0] + EPS_DICE) / (q[:, 1] + q[:, 2] + EPS_DICE)).sum() / (N * C))
    if mn is not None:
        mn = mn.double().cpu()
        terms.append(mn[:, :-1].sum() / mn[:, -1].sum())
    total = torch.stack(terms).sum()
    if len(terms) > 1 and combine == "mean":
        return total / len(terms), torch.tensor(1.0 / len(terms), dtype=torch.float64)
    if len(terms) > 1 and combine == "log":
        return torch.log(1 + total), 1 / (1 + total)
    return total, torch.tensor(1.0, dtype=torch.float64)


def finish_bound(ref):
    """One fp32 rounding of an fp64 result (2^-40 relative for the fp64 evaluation's own order and its log)."""
    return (U32 + 2.0 ** -40) * ref.abs() + FLOOR32


def loss_bound(r, bnd, names, combine, mn_value=0.0, mn_tol=0.0):
    """How far L from the device's sums may be from L from the reference's sums: reduce_bound ``bnd`` propagated through the
    terms (dice: |d f| <= 2 dI / De + (2 I + e) (dS + dY) / De^2 per (n, c)), ``mn_tol`` for the multi_neighbor term, the
    combine's derivative, the tail's rounding."""
    N, C, V = r["N"], r["C"], r["V"]
    b = bnd.double().cpu()
    q = b[:N * C * 4].view(N * C, 4)
    tot, count = 0.0, 0
    if "mse" in names:
        tot, count = tot + float(b[-2]) / (N * C * V), count + 1
    if "bce" in names:
        tot, count = tot + float(b[-1]) / (N * C * V), count + 1
    if "dice" in names:
        I, De = r["I"].reshape(-1).cpu(), (r["S"] + r["Y"]).reshape(-1).cpu() + EPS_DICE
        tot += float((2 * q[:, 0] / De + (2 * I + EPS_DICE) * (q[:, 1] + q[:, 2]) / (De * De)).sum()) / (N * C)
        count += 1
    if "multi_neighbor" in names:
        tot, count = tot + mn_tol, count + 1
    L, dc = finish_ref(ref_sums(r), N, C, V, names, combine,
                       torch.tensor([[mn_value, 1.0]], dtype=torch.float64) if "multi_neighbor" in names else None)
    scale = 1.0 if count == 1 or combine == "sum" else float(dc)
    if count > 1 and combine == "log":
        scale = 1.0 / (1.0 + max(0.0, float(torch.expm1(L)) - tot))
    return L, tot * scale * SECOND_ORDER + float(finish_bound(L))


# ---- gradient ----------------------------------------------------------------------------------------------------------------------
def grad_ref(logits, labels, sums, g, weights):
    """Per-element gradient g * [(w_mse 2 (s - y) s (1 - s) + w_bce (s - y)) / M + w_dice (k0 y + k1) s (1 - s)] in float64 from
    the device sums the kernel read; ``g``: the fp32 scale as stored; ``weights`` = (w_mse, w_bce, w_dice).  Returns a dict: ref
    [N, C, V] and the pieces grad_bound needs."""
    p, y = operands(logits, labels)
    N, C, V = p.shape
    w_mse, w_bce, w_dice = (float(w) for w in weights)
    M = float(N * C * V)
    q = sums.double().to(p.device)[:N * C * 4].view(N, C, 4)
    De, Ie = q[..., 1] + q[..., 2] + EPS_DICE, 2.0 * q[..., 0] + EPS_DICE
    k0 = (-2.0 / De * (w_dice / (N * C)))[..., None]
    k1 = (Ie / (De * De) * (w_dice / (N * C)))[..., None]
    s, om = torch.sigmoid(p), torch.sigmoid(-p)
    d, ds = s - y, s * om
    A, B = (2.0 * w_mse / M) * d * ds, (w_bce / M) * d
    t_abs = (k0 * y).abs() + k1.abs()
    Cd = (k0 * y + k1) * ds
    g = float(g)
    return dict(ref=g * (A + B + Cd), g=g, p=p, s=s, d=d, ds=ds, A=A, B=B, Cd=Cd, t=k0 * y + k1, t_abs=t_abs,
                a_mse=2.0 * w_mse / M, a_bce=w_bce / M)


def grad_bound(r, dtype_out):
    """Per-element bound on seg_loss_grad_kernel's output.  With u = 2^-24 and e_s the sigmoid's error:
      a_mse, a_bce   1 / fl(fl(N C) V): the product and the reciprocal round            2 u relative
      k0, k1         the fp64 value cast to fp32, invNC = fl(w / fl(N C)), their product  3 u relative
      d  = fl(s - y)                                                                     e_s + u |d|
      ds = fl(s fl(1 - s))                                                               e_s + 2 u ds
      A  = fl(fl(a_mse d) ds)        |A| 4 u + a_mse (ds e_d + |d| e_ds)
      B  = fl(a_bce d)               |B| 3 u + a_bce e_d
      t  = fl(fl(k0 y) + k1)         5 u (|k0 y| + |k1|)       (cancellation: the bound holds the operands' sizes, not |t|)
      C  = fl(t ds)                  ds e_t + |t| e_ds + u |C|
      fl(fl(A + B) + C), fl(g ...)   2 u (|A| + |B| + |C|) + u |sum|
    plus 2^-149 per fp32 operation that may underflow (8 of them), then the stored value's rounding."""
    u_out, floor = unit(dtype_out)
    es = sigmoid_err(r["p"], r["s"])
    e_d = es + U32 * r["d"].abs()
    e_ds = es + 2 * U32 * r["ds"]
    A, B, Cd = r["A"].abs(), r["B"].abs(), r["Cd"].abs()
    eA = 4 * U32 * A + abs(r["a_mse"]) * (r["ds"] * e_d + r["d"].abs() * e_ds)
    eB = 3 * U32 * B + abs(r["a_bce"]) * e_d
    eC = r["ds"] * 5 * U32 * r["t_abs"] + r["t"].abs() * e_ds + U32 * Cd
    inner = eA + eB + eC + 3 * U32 * (A + B + Cd) + 8 * 2.0 ** -149
    return abs(r["g"]) * inner * SECOND_ORDER + u_out * r["ref"].abs() + floor


def grad_rows(out, C):
    """The kernel's output [N, D, H, W, Cs] as [N, C, V] (its first C channels) and the padding channels."""
    N, Cs = out.shape[0], out.shape[-1]
    o = out.reshape(N, -1, Cs)
    return o[..., :C].permute(0, 2, 1), o[..., C:]


PAD_BOUND = 2.0 ** -150


def check_padding(pad):
    """The gradient's padding channels (Cs > C) against zero.  The kernel never writes them, so nothing may round there: the
    bound is below the smallest value fp32 (let alone fp16) can hold, and any stored non-zero value has ratio > 1."""
    if pad.numel() == 0:
        return CheckResult(0.0, (), 0.0, 0.0, PAD_BOUND)
    return check(pad, torch.zeros_like(pad, dtype=torch.float64), torch.full_like(pad, PAD_BOUND, dtype=torch.float64))


# ---- multi_neighbor on the CPU, per sample ------------------------------------------------------------------------------------------
def mn_partials_restated(logits_ncdhw, labels, K):
    """The partials the tail reads, from the CPU restatement of tests/test_multi_neighbor.py: fp64 [N, 2] = (sum of squared
    angle differences, entry count) per sample."""
    from test_multi_neighbor import _class_centroids, _pair_angles
    rows = []
    for i in range(logits_ncdhw.shape[0]):
        lc, valid = _class_centroids(labels[i].float(), K)
        pc, _ = _class_centroids(torch.sigmoid(logits_ncdhw[i].float()), K)
        if int(valid.sum()) < 2:
            rows.append([0.0, 1.0])
            continue
        dl = (_pair_angles(pc[valid]) - _pair_angles(lc[valid])) ** 2
        rows.append([float(dl.double().sum()), float(dl.numel())])
    return torch.tensor(rows, dtype=torch.float64)


# ---- the kernels' own arithmetic in torch fp32 (CPU) ------------------------------------------------------------------------------
def _f32(x):
    return x.to(torch.float32)


def emu_sigmoid(p32, defect=None):
    """fl(1 / fl(1 + E)), E = 2^fl(p * -log2e) rounded once to fp32 (an exact hardware exponential)."""
    t = _f32(p32 * np.float32(-LOG2E_32))
    E = _f32(torch.exp2(t.double()))
    s = _f32(1.0 / _f32(1.0 + E))
    if defect == "sigmoid_ulp":
        s = _f32(s * np.float32(1 + 2.0 ** -10))
    return s


def _wave_tree(x):
    """x [..., 64 k] fp32: six xor-shuffle levels inside each wave of 64 -> [..., k] (lane 0's value)."""
    x = x.reshape(*x.shape[:-1], -1, 64)
    for o in (32, 16, 8, 4, 2, 1):
        x = _f32(x + x[..., torch.arange(64) ^ o])
    return x[..., 0]


def emu_reduce(logits, labels, defect=None):
    """dua_seg_loss_reduce in torch fp32: workgroup b's thread t walks voxels b 256 + t + i G 256; per-thread chains per channel
    (I, S, Y) and over all channels in the kernel's order (squared error with fmaf, BCE), the wave tree, fp64 after it.
    Returns the fp64 sums buffer.  ``defect``: drop_tail, group_labels, sigmoid_ulp."""
    N, C = labels.shape[:2]
    V = labels[0, 0].numel()
    G, n = reduce_geometry(V)
    T = G * 256
    pad = n * T - V
    p = _f32(logits.reshape(N, V, -1)[..., :C]).permute(0, 2, 1)
    y = labels.reshape(N, C, V).float()
    live = torch.nn.functional.pad(torch.ones(V, dtype=torch.bool), (0, pad)).view(n, T)
    pp = torch.nn.functional.pad(p, (0, pad)).reshape(N, C, n, T)
    yy = torch.nn.functional.pad(y, (0, pad)).reshape(N, C, n, T)
    vec8 = logits.dtype == torch.float16 and C % 8 == 0 and logits.shape[-1] % 8 == 0
    steps = n - 1 if defect == "drop_tail" and n > 1 else n
    sums = torch.zeros(N * C * 4 + 2, dtype=torch.float64)
    mse = torch.zeros(N, T, dtype=torch.float32)
    bce = torch.zeros(N, T, dtype=torch.float32)
    zero = torch.zeros(N, T, dtype=torch.float32)
    groups = [list(range(c0, c0 + 8)) for c0 in range(0, C, 8)] if vec8 else [[c] for c in range(C)]
    for grp in groups:
        acc = {c: [zero.clone(), zero.clone(), zero.clone()] for c in grp}
        for i in range(steps):
            for c in grp:
                cy = c - grp[0] if defect == "group_labels" else c
                pv, yv, on = pp[:, c, i], yy[:, cy, i], live[i][None]
                s = emu_sigmoid(pv, defect)
                I, S, Y = acc[c]
                acc[c] = [torch.where(on, _f32(I + _f32(s * yv)), I), torch.where(on, _f32(S + s), S),
                          torch.where(on, _f32(Y + yv), Y)]
                dd = _f32(s - yv)
                mse = torch.where(on, _f32(dd.double() * dd.double() + mse.double()), mse)
                sp = _f32(torch.log1p(_f32(torch.exp2(_f32(pv.abs() * np.float32(-LOG2E_32)).double())).double()))
                term = _f32(_f32(pv.clamp_min(0) - _f32(pv * yv)) + sp)
                bce = torch.where(on, _f32(bce + term), bce)
        for c in grp:
            for j in range(3):
                sums.view(-1)[:N * C * 4].view(N, C, 4)[:, c, j] = _wave_tree(acc[c][j]).double().sum(-1)
    sums[-2] = _wave_tree(mse).double().sum()
    sums[-1] = _wave_tree(bce).double().sum()
    return sums


def emu_finish(sums, N, C, V, names, combine, mn=None, defect=None):
    """seg_loss_finish_kernel: fp64, one rounding to fp32.  ``defect``: m_without_c, no_eps, log_without_mn."""
    sums = sums.double()
    M = float(N * V) if defect == "m_without_c" else float(N * C * V)
    e = 0.0 if defect == "no_eps" else EPS_DICE
    q = sums[:N * C * 4].view(N * C, 4)
    total, count, mn_term = 0.0, 0, 0.0
    if "mse" in names:
        total, count = total + sums[N * C * 4] / M, count + 1
    if "bce" in names:
        total, count = total + sums[N * C * 4 + 1] / M, count + 1
    if "dice" in names:
        total, count = total + (1.0 - (2.0 * q[:, 0] + e) / (q[:, 1] + q[:, 2] + e)).sum() / (N * C), count + 1
    if mn is not None:
        mn_term = mn[:, :-1].double().sum() / mn[:, -1].double().sum()
        total, count = total + mn_term, count + 1
    total = torch.as_tensor(total, dtype=torch.float64)
    L, dc = total, torch.tensor(1.0, dtype=torch.float64)
    if count > 1 and combine == "mean":
        L, dc = total / count, torch.tensor(1.0 / count, dtype=torch.float64)
    elif count > 1 and combine == "log":
        L = torch.log(1 + total)
        dc = 1 / (1 + (total - mn_term if defect == "log_without_mn" else total))
    return L.float(), dc.float()


def emu_grad(logits, labels, sums, g, weights, out_stride=None, defect=None):
    """seg_loss_grad_kernel in torch fp32, operation by operation; stored in the logits' dtype into a zeroed [.., out_stride]
    buffer.  ``defect``: k1_sign, y_squared, sigmoid_ulp, padding, flush_subnormals."""
    N, C = labels.shape[:2]
    V = labels[0, 0].numel()
    Cs = logits.shape[-1] if out_stride is None else out_stride
    f = np.float32
    w_mse, w_bce, w_dice = (f(w) for w in weights)
    invM = f(1.0) / (f(f(N) * f(C)) * f(V))
    invNC = w_dice / f(f(N) * f(C))
    a_mse, a_bce = f(f(2.0) * w_mse) * invM, w_bce * invM
    q = sums.double()[:N * C * 4].view(N, C, 4)
    De, Ie = q[..., 1] + q[..., 2] + EPS_DICE, 2.0 * q[..., 0] + EPS_DICE
    k0 = _f32(_f32(-2.0 / De) * invNC)[..., None]
    k1 = _f32(_f32(Ie / (De * De)) * invNC)[..., None]
    if defect == "k1_sign":
        k1 = -k1
    p = _f32(logits.reshape(N, V, -1)[..., :C]).permute(0, 2, 1)
    y = labels.reshape(N, C, V).float()
    s = emu_sigmoid(p, defect)
    ds, d = _f32(s * _f32(1.0 - s)), _f32(s - y)
    ky = _f32(k0 * (_f32(y * y) if defect == "y_squared" else y))
    v = _f32(_f32(_f32(_f32(a_mse * d) * ds) + _f32(a_bce * d)) + _f32(_f32(ky + k1) * ds))
    v = _f32(f(g) * v).to(logits.dtype)
    if defect == "flush_subnormals" and logits.dtype == torch.float16:
        v = torch.where(v.float().abs() < 2.0 ** -14, torch.zeros_like(v), v)
    out = torch.zeros(N, V, Cs, dtype=logits.dtype)
    out[..., :C] = v.permute(0, 2, 1)
    if defect == "padding" and Cs > C:
        out[..., C:] = 2.0 ** -20          # a store that runs past the C channels of a row
    return out.reshape(*logits.shape[:-1], Cs)


# ---- cases ---------------------------------------------------------------------------------------------------------------------------
def subsets():
    """Every non-empty subset of mse / bce / dice, in the kernels' order."""
    return [tuple(n for n, k in zip(LOSS_NAMES, m) if k) for m in itertools.product((0, 1), repeat=3) if any(m)]


def make_labels(kind, N, C, dims, gen):
    """binary: one-hot classes with 30 % unlabelled voxels; multi_hot: independent channels; soft: fractional values in [0, 1.3]
    (the shape of centroid-distance smoothed labels: most near 0 or 1, none exactly representable sums)."""
    if kind == "binary":
        cls = torch.randint(0, C, (N, *dims), generator=gen)
        lab = torch.nn.functional.one_hot(cls, C).permute(0, 4, 1, 2, 3).float()
        return (lab * (torch.rand(N, 1, *dims, generator=gen) >= 0.3)).contiguous()
    if kind == "multi_hot":
        return (torch.rand(N, C, *dims, generator=gen) > 0.8).float()
    hard = (torch.rand(N, C, *dims, generator=gen) > 0.8).float()
    return (hard - 0.3 * torch.rand(N, C, *dims, generator=gen) ** 4).abs().contiguous()


def make_logits(kind, N, C, dims, gen, dtype, labels=None):
    """NCDHW fp32 values representable in ``dtype``.  randn3; zero; saturated: a tenth of the voxels at +-20, +-40, +-88, +-100
    (+-65504 in fp16), signs independent of the labels so that both agreeing and disagreeing saturation occurs; corners: channel
    0 predicts nothing under an empty label (S + Y -> eps), channel C - 1 predicts its labels perfectly (2 I ~ S + Y)."""
    x = torch.randn(N, C, *dims, generator=gen) * 3
    if kind == "zero":
        x = torch.zeros_like(x)
    elif kind == "saturated":
        mags = torch.tensor([20.0, 40.0, 88.0, 100.0 if dtype == torch.float32 else 65504.0])
        pick = torch.randint(0, 4, x.shape, generator=gen)
        sign = torch.randint(0, 2, x.shape, generator=gen) * 2.0 - 1.0
        x = torch.where(torch.rand(x.shape, generator=gen) < 0.1, mags[pick] * sign, x)
    elif kind == "corners":
        labels[:, 0] = 0
        x[:, 0] = -30.0 - torch.rand(N, *dims, generator=gen)
        x[:, C - 1] = torch.where(labels[:, C - 1] > 0.5, 25.0, -25.0)
    return x.to(dtype).float()


def channels_last(x, dtype, Cs, offset_elems=0, device="cpu"):
    """NCDHW -> the kernels' [N, D, H, W, Cs] buffer on ``device`` (padding channels hold a poison value a correct kernel never
    reads into its sums); ``offset_elems``: the tensor is a contiguous view that many elements into a larger buffer."""
    N, C = x.shape[:2]
    shape = (N, *x.shape[2:], Cs)
    buf = torch.full((math.prod(shape) + offset_elems,), 7.0, dtype=dtype)
    buf[offset_elems:].view(shape)[..., :C] = x.permute(0, 2, 3, 4, 1).to(dtype)
    return buf.to(device)[offset_elems:].view(shape)
