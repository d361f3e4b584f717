"""fp64 references, error bounds and an fp32 emulation of the fused loss with ce / dice_ce / generalized_dice
(csrc/seg_loss_terms.hip; the contract is in include/dua_hip.h at dua_seg_loss_terms_*), in the style of tests/loss_fp64ref.py,
whose sigmoid, softplus and per-channel reasoning this module reuses.  A plain helper module (``import loss_terms_fp64ref``).

The references are evaluated in float64 on the stored operands: the fp16 / fp32 logits (channels-last [N, D, H, W, Cs], first C
channels), the fp32 labels ([N, C, D, H, W]) and -- for the tail, the constants and the gradient -- the fp64 ``sums`` the device
produced.  Per-element quantities are [N, C, V], per-voxel ones [N, V].

Bounds (u = 2^-24; EPS_SIG, LOG1P_ULPS, SECOND_ORDER, P_COEF from loss_fp64ref):

* exponential.  __expf(x) is v_mul_f32 by log2(e) rounded to fp32 and v_exp_f32.  Where x = fl(p - m) the subtraction rounds
  too, so the argument is off by at most (u + P_COEF) |p - m| and e^x by that much relatively; v_exp_f32 itself is within
  1 ulp = 2 u (the ISA's accuracy), below EPS_SIG -- which was measured for v_exp_f32 plus an add plus a division and is reused
  here unchanged rather than splitting it.  v_exp_f32 gives 0 where the result is below the smallest normal: + 2^-126.
      e_exp(a) = e^-a ((u + P_COEF) a + EPS_SIG) + 2^-126,   a = m - p >= 0
* log-sum-exp, reduce pass.  The row is walked in ceil(C / 8) groups with a running maximum; a term enters as e^(p - m_g) and is
  multiplied by e^(m_old - m_new) each time the maximum moves.  The arguments of that chain telescope to a = m - p exactly, so
  the argument rounding is the one above; the chain has at most NG exponentials and NG - 1 products per term, and l is a chain
  of C + NG fp32 operations:
      e_l = sum_c [ e^-a_c ((u + P_COEF) a_c + NG (EPS_SIG + u)) + 2^-126 ] + (C + NG) u l
  logf is within 2 ulp (HIP math API accuracy table; LOGF_ULPS of tests/suf_fp64ref.py), l >= 1:
      e_lse = e_l / l + 4 u log l + u |lse|
* cross-entropy bracket of a voxel, t = fl(fl(Y_v lse) - dot):  Y_v is a chain of C additions (C u sum |y|), dot a chain of C
  rounded products ((C + 1) u sum |p y|):
      e_t = |Y_v| e_lse + |lse| C u sum|y| + u |Y_v lse| + (C + 1) u sum|p y| + u |t|
  The bound holds the operands' sizes: at p = +-200 the two halves of t are ~200 each and the kernel does subtract them.
* reduce.  Per thread n = ceil(V / (G 256)) additions per channel (G = min(512, ceil(V / 256)) workgroups per sample), n C for the
  squared-error and BCE accumulators, n for the cross-entropy one, then six shuffle levels; fp64 after that, in a fixed order.
  The squared error is fl(d d) added (no fmaf here): one more rounding per term than loss_fp64ref's.
* tail.  L, dcomb and the per-(n, c) constants k0, k1 are fp64 expressions of the sums, rounded once to fp32.
* gradient.  grad_bound counts the fp32 operations of seg_loss_terms_grad_kernel; the softmax there is two passes over the row
  held in registers (m is the exact maximum, NG = 1 in e_l).

No constant of this module comes from a measurement of its own: EPS_SIG is loss_fp64ref's.
"""
from __future__ import annotations

import itertools

import numpy as np
import torch

import loss_fp64ref as LR
from loss_fp64ref import (EPS_DICE, EPS_SIG, FLOOR32, FLT_MIN, LOG1P_ULPS, LOG2E_32, P_COEF, SECOND_ORDER, U32,  # noqa: F401
                          channels_last, check, check_padding, finish_bound, grad_rows, operands, reduce_geometry, unit)

LOGF_ULPS = 2                                   # HIP math API, maximum ULP error of logf (tests/suf_fp64ref.py)
LOGF_REL = 2 * LOGF_ULPS * U32
OLD_NAMES = ("mse", "bce", "dice")
EXT_NAMES = ("ce", "dice_ce", "generalized_dice")
TERM_NAMES = OLD_NAMES + EXT_NAMES              # the order of the use_* flags
F64 = torch.float64


def _cdiv(a, b):
    return -(-a // b)


def groups_of(C):
    """Channel groups the kernels are instantiated for."""
    return 1 if C <= 8 else 2 if C <= 16 else 3 if C <= 24 else 4 if C <= 32 else 8


def exp_err(a, ng=1):
    """Absolute error of the kernels' e^-a for a = m - p >= 0, through a chain of ng exponentials (module docstring)."""
    return torch.exp(-a) * ((U32 + P_COEF) * a + ng * (EPS_SIG + U32)) + FLT_MIN


# ---- restatements (what the CPU tests hold against torch) ----------------------------------------------------------------------------
def ce_restated(p, y):
    """[N, C, V] float64 -> the contract's ce: 1 / (N V) sum [Y_v lse_v - sum_c y_c p_c]."""
    N, C, V = p.shape
    m = p.max(1).values
    lse = m + torch.log(torch.exp(p - m[:, None]).sum(1))
    return (y.sum(1) * lse - (y * p).sum(1)).sum() / (N * V)


def ce_grad_restated(p, y):
    N, C, V = p.shape
    return (y.sum(1, keepdim=True) * torch.softmax(p, 1) - y) / (N * V)


def dice_restated(p, y):
    s = torch.sigmoid(p)
    return (1.0 - (2.0 * (s * y).sum(2) + EPS_DICE) / (s.sum(2) + y.sum(2) + EPS_DICE)).mean()


def gdice_weights(Y):
    """[N, C] label sums -> the contract's weights: 1 / Y^2, inf -> 0 -> the largest finite weight of the same sample."""
    w = 1.0 / (Y * Y)
    inf = torch.isinf(w)
    w = torch.where(inf, torch.zeros_like(w), w)
    return w + inf * w.max(1, keepdim=True).values


def gdice_parts(I, S, Y, w=None):
    """(f [N], A [N], B [N], w [N, C]) from the per-(n, c) sums (``w``: other weights than the contract's, for the emulation)."""
    w = gdice_weights(Y) if w is None else w
    A = 2.0 * (w * I).sum(1) + EPS_DICE
    B = (w * (S + Y)).sum(1) + EPS_DICE
    return 1.0 - A / B, A, B, w


def gdice_restated(p, y):
    s = torch.sigmoid(p)
    return gdice_parts((s * y).sum(2), s.sum(2), y.sum(2))[0].mean()


def monai_generalized_dice(input, target):
    """MONAI GeneralizedDiceLoss(sigmoid=True).forward with its defaults, line by line (include_background=True, w_type
    "square", smooth_nr = smooth_dr = 1e-5, batch=False, reduction "mean"); input / target [N, C, *spatial]."""
    input = torch.sigmoid(input)
    reduce_axis = torch.arange(2, len(input.shape)).tolist()
    intersection = torch.sum(target * input, reduce_axis)
    ground_o = torch.sum(target, reduce_axis)
    pred_o = torch.sum(input, reduce_axis)
    denominator = ground_o + pred_o
    w = torch.reciprocal(ground_o * ground_o)
    infs = torch.isinf(w)
    w[infs] = 0.0
    max_values = torch.max(w, dim=1)[0].unsqueeze(dim=1)
    w = w + infs * max_values
    numer = 2.0 * (intersection * w).sum(1, keepdim=True) + 1e-5
    denom = (denominator * w).sum(1, keepdim=True) + 1e-5
    f = 1.0 - (numer / denom)
    return torch.mean(f)


def loss_restated(p, y, names, combine):
    """The whole loss in float64 torch operators from [N, C, V] operands (no multi_neighbor): every name one term."""
    s = torch.sigmoid(p)
    term = dict(mse=lambda: ((s - y) ** 2).mean(),
                bce=lambda: torch.nn.functional.binary_cross_entropy_with_logits(p, y),
                dice=lambda: dice_restated(p, y), ce=lambda: ce_restated(p, y),
                dice_ce=lambda: dice_restated(p, y) + ce_restated(p, y), generalized_dice=lambda: gdice_restated(p, y))
    terms = [term[n]() for n in names]
    total = torch.stack(terms).sum()
    if len(terms) > 1 and combine == "mean":
        return total / len(terms)
    if len(terms) > 1 and combine == "log":
        return torch.log(1 + total)
    return total


# ---- reduce ----------------------------------------------------------------------------------------------------------------------------
def reduce_ref(logits, labels):
    """loss_fp64ref.reduce_ref plus the cross-entropy sum: value, sum of |terms|, sum of the terms' own errors; the squared
    error's extra rounding (fl(d d), then the addition)."""
    r = LR.reduce_ref(logits, labels)
    p, y = operands(logits, labels)
    N, C, V = p.shape
    r["mse_err"] = r["mse_err"] + U32 * r["mse_abs"]
    m = p.max(1).values
    a = m[:, None] - p
    l = torch.exp(-a).sum(1)
    ng = groups_of(C)
    e_l = exp_err(a, ng).sum(1) + (C + ng) * U32 * l
    lse = m + torch.log(l)
    e_lse = e_l / l + LOGF_REL * torch.log(l) + U32 * lse.abs()
    Yv, ya, pya = y.sum(1), y.abs().sum(1), (p * y).abs().sum(1)
    t = Yv * lse - (p * y).sum(1)
    e_t = Yv.abs() * e_lse + lse.abs() * C * U32 * ya + U32 * (Yv * lse).abs() + (C + 1) * U32 * pya + U32 * t.abs()
    r["ce"], r["ce_abs"], r["ce_err"] = t.sum(), t.abs().sum(), e_t.sum()
    return r


def ref_sums(r):
    """[N C 4 + 3]: (I, S, Y, 0) per (n, c), then mse, bce, ce."""
    return torch.cat([LR.ref_sums(r), r["ce"].reshape(1)])


def reduce_bound(r):
    """Per-sum limit for the fp64 sums of dua_seg_loss_terms_reduce, in its layout."""
    _, n = reduce_geometry(r["V"])
    f64 = 2.0 ** -45
    b = LR.reduce_bound(r)
    bc = (r["ce_err"] + (U32 * (n + 6) + f64) * r["ce_abs"]) * SECOND_ORDER + FLOOR32
    return torch.cat([b, bc.reshape(1)])


# ---- tail ------------------------------------------------------------------------------------------------------------------------------
def _split(sums, N, C):
    sums = sums.double()
    return sums[:N * C * 4].view(N, C, 4), sums[N * C * 4:N * C * 4 + 3]


def finish_ref(sums, N, C, V, names, combine, mn=None):
    """(L, dcomb, k0 [N, C], k1 [N, C]) in float64 from the sums the tail read.  dice_ce is one term holding dice + ce; the
    constants are the Dice part once per selecting name plus the generalized-Dice part."""
    q, w3 = _split(sums.cpu(), N, C)
    I, S, Y = q[..., 0], q[..., 1], q[..., 2]
    De, Ie = S + Y + EPS_DICE, 2.0 * I + EPS_DICE
    dice = (1.0 - Ie / De).sum() / (N * C)
    ce = w3[2] / (N * V)
    k0, k1 = torch.zeros(N, C, dtype=F64), torch.zeros(N, C, dtype=F64)
    terms = []
    for name in names:
        if name == "mse":
            terms.append(w3[0] / (N * C * V))
        elif name == "bce":
            terms.append(w3[1] / (N * C * V))
        elif name in ("dice", "dice_ce"):
            terms.append(dice + ce if name == "dice_ce" else dice)
            k0 = k0 - 2.0 / (De * N * C)
            k1 = k1 + Ie / (De * De * N * C)
        elif name == "ce":
            terms.append(ce)
        elif name == "generalized_dice":
            f, A, B, w = gdice_parts(I, S, Y)
            terms.append(f.mean())
            k0 = k0 - 2.0 * w / (B[:, None] * N)
            k1 = k1 + A[:, None] * w / (B[:, None] ** 2 * N)
        elif name == "multi_neighbor":
            m = mn.double().cpu()
            terms.append(m[:, :-1].sum() / m[:, -1].sum())
        else:
            raise KeyError(name)
    total, count = torch.stack(terms).sum(), len(terms)
    L, dc = total, torch.tensor(1.0, dtype=F64)
    if count > 1 and combine == "mean":
        L, dc = total / count, torch.tensor(1.0 / count, dtype=F64)
    elif count > 1 and combine == "log":
        L, dc = torch.log(1 + total), 1 / (1 + total)
    return L, dc, k0, k1


def consts_bound(k):
    """One fp32 rounding of an fp64 result (subnormals kept)."""
    return (U32 + 2.0 ** -40) * k.abs() + 2.0 ** -149


def loss_bound(r, bnd, names, combine):
    """How far L from the device's sums may be from L from the reference's sums (no multi_neighbor): reduce_bound ``bnd``
    propagated through the terms.  dice: loss_fp64ref.loss_bound's rule.  generalized_dice: w = 1 / Y^2 moves by 2 w dY / Y
    (an absent class's replaced weight by the largest such move of its sample), A by 2 sum (w dI + I dw), B by
    sum (w (dS + dY) + (S + Y) dw), f by dA / B + A dB / B^2.  Returns (L from the reference sums, the limit)."""
    N, C, V = r["N"], r["C"], r["V"]
    b = bnd.double().cpu()
    bq, b3 = _split(b, N, C)
    I, S, Y = r["I"].cpu(), r["S"].cpu(), r["Y"].cpu()
    tot = 0.0
    for name in names:
        if name == "mse":
            tot += float(b3[0]) / (N * C * V)
        if name == "bce":
            tot += float(b3[1]) / (N * C * V)
        if name in ("dice", "dice_ce"):
            De = S + Y + EPS_DICE
            tot += float((2 * bq[..., 0] / De + (2 * I + EPS_DICE) * (bq[..., 1] + bq[..., 2]) / (De * De)).sum()) / (N * C)
        if name in ("ce", "dice_ce"):
            tot += float(b3[2]) / (N * V)
        if name == "generalized_dice":
            _, A, B, w = gdice_parts(I, S, Y)
            present = Y != 0
            dw = torch.where(present, 2 * w * bq[..., 2] / Y.abs().clamp_min(1e-300), torch.zeros_like(w))
            dw = torch.where(present, dw, dw.max(1, keepdim=True).values.expand_as(dw))
            dA = 2 * (w * bq[..., 0] + I.abs() * dw).sum(1)
            dB = (w * (bq[..., 1] + bq[..., 2]) + (S + Y).abs() * dw).sum(1)
            tot += float((dA / B + A * dB / (B * B)).sum()) / N
    L, dc, _, _ = finish_ref(ref_sums(r), N, C, V, names, combine)
    count = len(names)
    scale = 1.0 if count == 1 or combine == "sum" else float(dc)
    if count > 1 and combine == "log":
        scale = 1.0 / (1.0 + max(0.0, float(torch.expm1(L)) - tot))
    return L, tot * scale * SECOND_ORDER + float(finish_bound(L))


# ---- gradient ----------------------------------------------------------------------------------------------------------------------------
def grad_ref(logits, labels, sums, g, names):
    """Per-element gradient g [mse' + bce' + (k0 y + k1) s (1 - s) + ce'] in float64, the constants from the device sums the tail
    read; ``g``: the fp32 scale as stored.  Returns ref [N, C, V] and the pieces grad_bound needs."""
    p, y = operands(logits, labels)
    N, C, V = p.shape
    M = float(N * C * V)
    _, _, k0, k1 = finish_ref(sums, N, C, V, [n for n in names if n != "multi_neighbor"] or ["mse"], "sum")
    use_k = any(n in names for n in ("dice", "dice_ce", "generalized_dice"))
    k0 = (k0 if use_k else torch.zeros_like(k0)).to(p.device)[..., None]
    k1 = (k1 if use_k else torch.zeros_like(k1)).to(p.device)[..., None]
    a_mse = 2.0 / M if "mse" in names else 0.0
    a_bce = 1.0 / M if "bce" in names else 0.0
    a_ce = (("ce" in names) + ("dice_ce" in names)) / float(N * V)
    s, om = torch.sigmoid(p), torch.sigmoid(-p)
    d, ds = s - y, s * om
    A, B = a_mse * d * ds, a_bce * d
    t = k0 * y + k1
    K = t * ds
    m = p.max(1, keepdim=True).values
    a = m - p
    E = torch.exp(-a)
    l = E.sum(1, keepdim=True)
    Yv = y.sum(1, keepdim=True)
    rl = Yv / l
    CE = a_ce * (rl * E - y)
    g = float(g)
    return dict(ref=g * (A + B + K + CE), g=g, p=p, y=y, s=s, d=d, ds=ds, A=A, B=B, K=K, CE=CE, t=t,
                t_abs=(k0 * y).abs() + k1.abs(), a_mse=a_mse, a_bce=a_bce, a_ce=a_ce, a=a, E=E, l=l, Yv=Yv, rl=rl, C=C)


def grad_bound(r, dtype_out):
    """Per-element bound on seg_loss_terms_grad_kernel's output.  e_s: loss_fp64ref.sigmoid_err; a_mse, a_bce, a_ce, k0, k1 are
    fp64 values rounded once (u relative each).
      d  = fl(s - y)                        e_d  = e_s + u |d|
      ds = fl(s fl(1 - s))                  e_ds = e_s + 2 u ds
      A  = fl(fl(a_mse d) ds)               3 u |A| + a_mse (ds e_d + |d| e_ds)
      B  = fl(a_bce d)                      2 u |B| + a_bce e_d
      t  = fl(fl(k0 y) + k1)                3 u (|k0 y| + |k1|)    (the operands' sizes: t may cancel)
      K  = fl(t ds)                         ds e_t + |t| e_ds + u |K|
      Y_v chain of C additions              e_Y = C u sum |y|
      l  chain of C exponentials            e_l = sum_c e_exp(a_c) + C u l
      rl = fl(Y_v / l)                      e_rl = e_Y / l + |Y_v| e_l / l^2 + u |rl|
      q  = fl(rl E_c)                       e_q = E_c e_rl + |rl| e_exp(a_c) + u |q|
      CE = fl(a_ce fl(q - y))               a_ce (e_q + u |q - y|) + 2 u |CE|
      the sum of the four parts, fl(g ..)   4 u (|A| + |B| + |K| + |CE|)
    plus 2^-149 per fp32 operation that may underflow (12 of them), then the stored value's rounding."""
    u_out, floor = unit(dtype_out)
    C = r["C"]
    es = LR.sigmoid_err(r["p"], r["s"])
    e_d = es + U32 * r["d"].abs()
    e_ds = es + 2 * U32 * r["ds"]
    A, B, K, CE = r["A"].abs(), r["B"].abs(), r["K"].abs(), r["CE"].abs()
    eA = 3 * U32 * A + r["a_mse"] * (r["ds"] * e_d + r["d"].abs() * e_ds)
    eB = 2 * U32 * B + r["a_bce"] * e_d
    eK = r["ds"] * 3 * U32 * r["t_abs"] + r["t"].abs() * e_ds + U32 * K
    e_E = exp_err(r["a"])
    e_l = e_E.sum(1, keepdim=True) + C * U32 * r["l"]
    e_Y = C * U32 * r["y"].abs().sum(1, keepdim=True)
    e_rl = e_Y / r["l"] + r["Yv"].abs() * e_l / (r["l"] * r["l"]) + U32 * r["rl"].abs()
    q = r["rl"] * r["E"]
    e_q = r["E"] * e_rl + r["rl"].abs() * e_E + U32 * q.abs()
    eCE = r["a_ce"] * (e_q + U32 * (q - r["y"]).abs()) + 2 * U32 * CE
    inner = eA + eB + eK + eCE + 4 * U32 * (A + B + K + CE) + 12 * 2.0 ** -149
    return abs(r["g"]) * inner * SECOND_ORDER + u_out * r["ref"].abs() + floor


# ---- the kernels' own arithmetic in torch fp32 (CPU), with planted defects -------------------------------------------------------------------
def _f32(x):
    return x.to(torch.float32)


def emu_exp(x32):
    """__expf: fl(x log2e) through an exact 2^t rounded once; results below the smallest normal are 0 (v_exp_f32)."""
    t = _f32(x32 * np.float32(LOG2E_32))
    E = _f32(torch.exp2(t.double()))
    return torch.where(E < FLT_MIN, torch.zeros_like(E), E)


def emu_reduce(logits, labels, defect=None):
    """dua_seg_loss_terms_reduce in torch fp32: workgroup b's thread t owns voxels b 256 + t + i G 256 and walks each row in
    groups of eight channels (running maximum, rescaled l); per-thread chains, the wave tree, fp64 from the four waves on, the
    workgroups in order.  Returns the fp64 sums [N C 4 + 3].  ``defect``: lse_without_max."""
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
    zero = torch.zeros(N, T, dtype=torch.float32)
    acc = [[zero.clone(), zero.clone(), zero.clone()] for _ in range(C)]
    mse, bce, ce = zero.clone(), zero.clone(), zero.clone()
    for i in range(n):
        on = live[i][None]
        m = torch.full((N, T), float("-inf"), dtype=torch.float32)
        l, Yv, dot = zero.clone(), zero.clone(), zero.clone()
        for c0 in range(0, C, 8):
            grp = range(c0, min(C, c0 + 8))
            if defect == "lse_without_max":
                gm = torch.zeros_like(m)
            else:
                gm = m
                for c in grp:
                    gm = torch.maximum(gm, pp[:, c, i])
                l = _f32(l * emu_exp(_f32(m - gm)))
            m = gm
            for c in grp:
                pv, yv = pp[:, c, i], yy[:, c, i]
                s = LR.emu_sigmoid(pv)
                I, S, Y = acc[c]
                acc[c] = [torch.where(on, _f32(I + _f32(s * yv)), I), torch.where(on, _f32(S + s), S),
                          torch.where(on, _f32(Y + yv), Y)]
                dd = _f32(s - yv)
                mse = torch.where(on, _f32(mse + _f32(dd * dd)), mse)
                sp = _f32(torch.log1p(_f32(torch.exp2(_f32(pv.abs() * np.float32(-LOG2E_32)).double())).double()))
                bce = torch.where(on, _f32(bce + _f32(_f32(pv.clamp_min(0) - _f32(pv * yv)) + sp)), bce)
                l = _f32(l + emu_exp(_f32(pv - m)))
                Yv = _f32(Yv + yv)
                dot = _f32(dot + _f32(pv * yv))
        lse = _f32(m + _f32(torch.log(l.double())))
        ce = torch.where(on, _f32(ce + _f32(_f32(Yv * lse) - dot)), ce)
    sums = torch.zeros(N * C * 4 + 3, dtype=F64)
    q = sums[:N * C * 4].view(N, C, 4)
    for c in range(C):
        for j in range(3):
            q[:, c, j] = LR._wave_tree(acc[c][j]).double().sum(-1)
    for j, x in enumerate((mse, bce, ce)):
        sums[N * C * 4 + j] = LR._wave_tree(x).double().sum()
    return sums


def emu_finish(sums, N, C, V, names, combine, mn=None, defect=None):
    """seg_loss_terms_finish_kernel as the kernel computes it (use flags, multiplicities, one wave per sample), in fp64 with one
    rounding to fp32: (L, dcomb, consts fp32 [N, C, 2]).  Written apart from finish_ref, so that the planted defects live here
    and not in the reference.  ``defect``: ce_divisor_ncv, inf_weights_zero, batch_max_weight, dice_ce_two_terms,
    gdice_consts_fp32 (weights, A, B and the constants in fp32 operations from the sums rounded to fp32)."""
    use = {n: int(n in names) for n in TERM_NAMES}
    nd, nce = use["dice"] + use["dice_ce"], use["ce"] + use["dice_ce"]
    q, w3 = _split(sums.cpu(), N, C)
    I, S, Y = q[..., 0], q[..., 1], q[..., 2]
    NC, e = float(N * C), EPS_DICE
    k0, k1 = torch.zeros(N, C, dtype=F64), torch.zeros(N, C, dtype=F64)
    total, count = torch.zeros((), dtype=F64), 0
    if use["mse"]:
        total, count = total + w3[0] / (NC * V), count + 1
    if use["bce"]:
        total, count = total + w3[1] / (NC * V), count + 1
    if nd:
        De, Ie = S + Y + e, 2.0 * I + e
        total, count = total + nd * ((1.0 - Ie / De).sum() / NC), count + use["dice"]
        k0, k1 = -2.0 * nd / (De * NC), nd * Ie / (De * De * NC)
    if nce:
        total = total + nce * (w3[2] / (NC * V if defect == "ce_divisor_ncv" else float(N) * V))
        count += use["ce"]
    count += use["dice_ce"] * (2 if defect == "dice_ce_two_terms" else 1)
    if use["generalized_dice"]:
        w = 1.0 / (Y * Y)
        inf = torch.isinf(w)
        w = torch.where(inf, torch.zeros_like(w), w)
        if defect == "batch_max_weight":
            w = w + inf * w.max()
        elif defect != "inf_weights_zero":
            w = w + inf * w.max(1, keepdim=True).values
        f, A, B, _ = gdice_parts(I, S, Y, w)
        total, count = total + f.sum() / N, count + 1
        g0, g1 = -2.0 * w / (B[:, None] * N), A[:, None] * w / (B[:, None] ** 2 * N)
        if defect == "gdice_consts_fp32":
            fl = np.float32
            I32, S32, Y32 = _f32(I), _f32(S), _f32(Y)
            w32 = _f32(1.0 / _f32(Y32 * Y32))
            inf32 = torch.isinf(w32)
            w32 = torch.where(inf32, torch.zeros_like(w32), w32)
            w32 = _f32(w32 + inf32 * w32.max(1, keepdim=True).values)
            A32 = _f32(fl(2.0) * _f32(w32 * I32).sum(1, dtype=torch.float32) + fl(e))[:, None]
            B32 = _f32(_f32(w32 * _f32(S32 + Y32)).sum(1, dtype=torch.float32) + fl(e))[:, None]
            g0 = _f32(_f32(fl(-2.0) * w32) / _f32(B32 * fl(N))).double()
            g1 = _f32(_f32(A32 * w32) / _f32(_f32(B32 * B32) * fl(N))).double()
            k0, k1 = _f32(k0).double(), _f32(k1).double()
        k0, k1 = k0 + g0, k1 + g1
    if mn is not None:
        m = mn.double().cpu()
        total, count = total + m[:, :-1].sum() / m[:, -1].sum(), count + 1
    L, dc = total, torch.tensor(1.0, dtype=F64)
    if count > 1 and combine == "mean":
        L, dc = total / count, torch.tensor(1.0 / count, dtype=F64)
    elif count > 1 and combine == "log":
        L, dc = torch.log(1 + total), 1 / (1 + total)
    return L.float(), dc.float(), torch.stack([k0, k1], -1).float()


def emu_grad(logits, labels, consts, g, names, out_stride=None, defect=None):
    """seg_loss_terms_grad_kernel in torch fp32, operation by operation; stored in the logits' dtype into a zeroed
    [.., out_stride] buffer.  ``defect``: grad_softmax_minus_y, ce_divisor_ncv."""
    N, C = labels.shape[:2]
    V = labels[0, 0].numel()
    Cs = logits.shape[-1] if out_stride is None else out_stride
    f = np.float32
    M = float(N) * C * V
    nce = ("ce" in names) + ("dice_ce" in names)
    a_mse, a_bce = f(2.0 / M), f(1.0 / M)
    a_ce = f(nce / (M if defect == "ce_divisor_ncv" else float(N) * V))
    p = _f32(logits.reshape(N, V, -1)[..., :C]).permute(0, 2, 1)
    y = labels.reshape(N, C, V).float()
    s = LR.emu_sigmoid(p)
    ds, d = _f32(s * _f32(1.0 - s)), _f32(s - y)
    acc = torch.zeros_like(p)
    if "mse" in names:
        acc = _f32(acc + _f32(_f32(a_mse * d) * ds))
    if "bce" in names:
        acc = _f32(acc + _f32(a_bce * d))
    if any(n in names for n in ("dice", "dice_ce", "generalized_dice")):
        k0, k1 = consts[..., 0].float()[..., None], consts[..., 1].float()[..., None]
        acc = _f32(acc + _f32(_f32(_f32(k0 * y) + k1) * ds))
    if nce:
        m = p.max(1, keepdim=True).values
        E = emu_exp(_f32(p - m))
        l, Yv = torch.zeros(N, 1, V), torch.zeros(N, 1, V)
        for c in range(C):
            l, Yv = _f32(l + E[:, c:c + 1]), _f32(Yv + y[:, c:c + 1])
        rl = torch.ones_like(l) / l if defect == "grad_softmax_minus_y" else _f32(Yv / l)
        acc = _f32(acc + _f32(a_ce * _f32(_f32(_f32(rl) * E) - y)))
    v = _f32(f(g) * acc).to(logits.dtype)
    out = torch.zeros(N, V, Cs, dtype=logits.dtype)
    out[..., :C] = v.permute(0, 2, 1)
    return out.reshape(*logits.shape[:-1], Cs)


# ---- cases ---------------------------------------------------------------------------------------------------------------------------------
LABEL_KINDS = ("onehot_background", "class_absent", "empty_sample", "soft")
LOGIT_KINDS = ("randn", "saturated")


def subsets():
    """Every non-empty subset of ce / dice_ce / generalized_dice."""
    return [tuple(n for n, k in zip(EXT_NAMES, m) if k) for m in itertools.product((0, 1), repeat=3) if any(m)]


def make_labels(kind, N, C, dims, gen):
    """onehot_background: one-hot classes, 30 % of the voxels all zero (background under include_background: false);
    class_absent: the same with class 1 missing from sample 0 only; empty_sample: the last sample has no class at all;
    soft: fractional values whose per-voxel sums lie between 0 and 1.3 (the shape of smoothed labels)."""
    if kind == "soft":
        cls = torch.randint(0, C, (N, *dims), generator=gen)
        hot = torch.nn.functional.one_hot(cls, C).permute(0, 4, 1, 2, 3).float()
        spread = torch.rand(N, C, *dims, generator=gen) ** 4
        lab = 0.9 * hot + 0.1 * spread / spread.sum(1, keepdim=True)
        lab = lab * (1.3 * torch.rand(N, 1, *dims, generator=gen))
        assert float(lab.sum(1).max()) <= 1.3001 and float(lab.sum(1).min()) >= 0.0
        return lab.contiguous()
    cls = torch.randint(0, C, (N, *dims), generator=gen)
    if kind == "class_absent":
        cls[0][cls[0] == 1] = 0
    lab = torch.nn.functional.one_hot(cls, C).permute(0, 4, 1, 2, 3).float()
    lab = lab * (torch.rand(N, 1, *dims, generator=gen) >= 0.3)
    if kind == "empty_sample":
        lab[N - 1] = 0
    return lab.contiguous()


def make_logits(kind, N, C, dims, gen, dtype):
    """NCDHW fp32 values representable in ``dtype``.  randn: unit normal.  saturated: a fifth of the entries at +-60 (fp16) or
    +-200 (fp32), signs independent of the labels."""
    x = torch.randn(N, C, *dims, generator=gen)
    if kind == "saturated":
        mag = 60.0 if dtype == torch.float16 else 200.0
        sign = torch.randint(0, 2, x.shape, generator=gen) * 2.0 - 1.0
        x = torch.where(torch.rand(x.shape, generator=gen) < 0.2, mag * sign, x)
    return x.to(dtype).float()
