"""fp64 references, error bounds and an fp32 emulation of the boundary term of the fused loss (csrc/seg_loss_terms.hip:
seg_loss_boundary_reduce_kernel, seg_loss_boundary_finish_kernel; the BND forms of seg_loss_grad_kernel in csrc/seg_loss.hip and
of seg_loss_terms_grad_kernel; the contract is in include/dua_hip.h at dua_seg_loss_boundary_*), in the manner of
tests/loss_terms_fp64ref.py.  The named part runs in the kernel family its names take without the term (``three_term(names)``:
tests/loss_fp64ref.py's references and bounds, else tests/loss_terms_fp64ref.py's), and this module reuses them.  A plain helper
module (``import boundary_fp64ref``).

The references are evaluated in float64 on the stored operands: the fp16 / fp32 logits (channels-last, first C channels), the
device's fp32 phi ([N, C, D, H, W], exact by tests/test_sdf_gpu.py), the fp32 alpha and scales as stored, and -- for L and the
gradient's named part -- the fp64 sums the device produced.

Bounds (u = 2^-24; e_s = loss_fp64ref.sigmoid_err with its EPS_SIG; M = N C V):

* reduce.  A thread adds fl(s phi) for its n = ceil(V / (G 256)) voxels x C channels in one fp32 chain (the dead channels of a
  last group add exact zeros), then six shuffle levels; fp64 from the four waves on, the workgroups in a fixed order:
      |sum - ref| <= sum (|phi| e_s + u |s phi|) + (u (n C + 6) + 2^-45) sum |s phi|
* B = sum / M in fp64, rounded once to fp32:  finish_bound(B) on top of the sum's bound / M.
* L = fl32(L_named + alpha B): L_named is the fp32 value the tail stored (one rounding of the fp64 expression of the device
  sums: finish_bound(L_named)), the sum is formed in fp64 from the fp64 B and rounded once (finish_bound(L)); B's error enters
  times alpha.
* gradient, per element, o = fl(gs acc) as the family's grad_bound bounds it for an fp32 result, and
      ds = fl(s fl(1 - s))                           e_ds = e_s + 2 u ds
      b  = fl(gb fl(fl(phi ds) a)),  a = fl32(1 / M)   e_b = |gb| a |phi| e_ds + 4 u |b|
      fl(o + b)                                      u (|o| + |b|)
  plus 2^-149 per product that may underflow (3), then the ONE rounding to the logits' dtype.

No constant of this module comes from a measurement of its own.
"""
from __future__ import annotations

import numpy as np
import torch

import loss_fp64ref as LR
import loss_terms_fp64ref as LT
from loss_fp64ref import FLOOR32, SECOND_ORDER, U32, check, finish_bound, operands, reduce_geometry, unit  # noqa: F401

F64 = torch.float64


def phi_rows(phi, device=None):
    N, C = phi.shape[:2]
    f = phi.reshape(N, C, -1).double()
    return f if device is None else f.to(device)


# ---- reduce and tail -------------------------------------------------------------------------------------------------------------------
def reduce_ref(logits, labels, phi):
    """sum s phi over everything in float64, the sum of |terms| and of the terms' own errors."""
    p, _ = operands(logits, labels)
    f = phi_rows(phi, p.device)
    N, C, V = p.shape
    s = torch.sigmoid(p)
    sf = s * f
    return dict(N=N, C=C, V=V, sum=sf.sum(), abs=sf.abs().sum(), err=(f.abs() * LR.sigmoid_err(p, s) + U32 * sf.abs()).sum())


def sum_bound(r):
    _, n = reduce_geometry(r["V"])
    return (r["err"] + (U32 * (n * r["C"] + 6) + 2.0 ** -45) * r["abs"]) * SECOND_ORDER + FLOOR32


def term_ref(r):
    """(B, its bound) for the fp32 B the device stores."""
    M = float(r["N"] * r["C"] * r["V"])
    B = r["sum"] / M
    return B, sum_bound(r) / M + finish_bound(B)


def loss_ref(L_named, alpha, r):
    """(L, its bound): ``L_named`` the float64 value of the tail's expression on the device sums (loss_terms_fp64ref.finish_ref),
    ``alpha`` the fp32 weight as stored."""
    M = float(r["N"] * r["C"] * r["V"])
    a = abs(float(alpha))
    L = L_named + float(alpha) * r["sum"] / M
    return L, finish_bound(L_named) + a * sum_bound(r) / M * SECOND_ORDER + finish_bound(L)


# ---- the named part, in the family its names take ---------------------------------------------------------------------------------------------
def three_term(names):
    """True: csrc/seg_loss.hip (a name set within mse / bce / dice / multi_neighbor); False: csrc/seg_loss_terms.hip."""
    return not any(n in LT.EXT_NAMES for n in names)


def _weights(names):
    return [1.0 if n in names else 0.0 for n in LR.LOSS_NAMES]


def named_finish_ref(sums, N, C, V, names, combine, mn=None):
    """(L_named, dcomb) in float64 from the sums the tail read."""
    if three_term(names):
        return LR.finish_ref(sums, N, C, V, names, combine, mn)
    return LT.finish_ref(sums, N, C, V, names, combine, mn)[:2]


# ---- gradient ----------------------------------------------------------------------------------------------------------------------------
def grad_ref(logits, labels, sums, gs, names, phi, gb):
    """gs [named terms] + gb phi s (1 - s) / M in float64; ``gs``, ``gb``: the fp32 scales as stored.  Returns the named part's
    dict of the family's grad_ref with ref = the whole gradient, named = its named part, b = its boundary part."""
    if three_term(names):
        r = LR.grad_ref(logits, labels, sums, gs, _weights(names))
    else:
        r = LT.grad_ref(logits, labels, sums, gs, names)       # multi_neighbor has no gradient: its name selects no part
    N, C, V = r["p"].shape
    r["three"], r["named"] = three_term(names), r["ref"]
    r["f"] = phi_rows(phi, r["p"].device)
    r["gb"], r["a_bnd"] = float(gb), float(np.float32(1.0 / (float(N) * C * V)))
    r["b"] = r["gb"] * r["f"] * r["ds"] * r["a_bnd"]
    r["ref"] = r["named"] + r["b"]
    return r


def grad_bound(r, dtype_out):
    u_out, floor = unit(dtype_out)
    whole = r["ref"]
    r["ref"] = r["named"]
    e_o = (LR if r["three"] else LT).grad_bound(r, torch.float32)              # fl(gs acc), an fp32 value
    r["ref"] = whole
    e_ds = LR.sigmoid_err(r["p"], r["s"]) + 2 * U32 * r["ds"]
    b = r["b"].abs()
    e_b = abs(r["gb"]) * r["a_bnd"] * r["f"].abs() * e_ds + 4 * U32 * b + 3 * 2.0 ** -149
    o = r["named"].abs() + e_o
    return (e_o + e_b + U32 * (o + b + e_b)) * SECOND_ORDER + u_out * whole.abs() + floor


# ---- the kernels' own arithmetic in torch fp32 (CPU), with planted defects -------------------------------------------------------------------
DEFECTS = ("divisor_nv", "phi_s", "scaled_by_dcomb", "alpha_twice", "padding_written")


def _f32(x):
    return x.to(torch.float32)


def emu_reduce(logits, phi):
    """seg_loss_boundary_reduce_kernel in torch fp32: workgroup b's thread t owns voxels b 256 + t + i G 256 and adds fl(s phi)
    channel by channel in one chain; the wave tree, fp64 from the four waves on, the workgroups in order.  Returns the fp64 sum."""
    N, C = phi.shape[:2]
    V = phi[0, 0].numel()
    G, n = reduce_geometry(V)
    T = G * 256
    pad = n * T - V
    p = _f32(logits.reshape(N, V, -1)[..., :C]).permute(0, 2, 1)
    pp = torch.nn.functional.pad(p, (0, pad)).reshape(N, C, n, T)
    ff = torch.nn.functional.pad(phi.reshape(N, C, V).float(), (0, pad)).reshape(N, C, n, T)
    live = torch.nn.functional.pad(torch.ones(V, dtype=torch.bool), (0, pad)).view(n, T)
    acc = torch.zeros(N, T, dtype=torch.float32)
    for i in range(n):
        for c in range(C):
            acc = torch.where(live[i][None], _f32(acc + _f32(LR.emu_sigmoid(pp[:, c, i]) * ff[:, c, i])), acc)
    return LR._wave_tree(acc).double().sum()


def emu_finish(bsum, N, C, V, L_named, alpha, defect=None):
    """seg_loss_boundary_finish_kernel: (B fp32, L fp32) from the fp64 sum, the fp32 L_named and the fp32 alpha."""
    M = float(N) * V if defect == "divisor_nv" else float(N) * C * V
    B = bsum.double() / M
    a = float(alpha) ** 2 if defect == "alpha_twice" else float(alpha)
    return B.float(), (L_named.double() + a * B).float() if a != 0.0 else L_named.float()


def emu_named(logits, labels, names, combine):
    """The named part's reduce and tail in the family's emulation: (sums, L_named fp32, dcomb fp32, consts or None)."""
    N, C = labels.shape[:2]
    V = labels[0, 0].numel()
    if three_term(names):
        sums = LR.emu_reduce(logits, labels)
        return (sums,) + LR.emu_finish(sums, N, C, V, names, combine) + (None,)
    sums = LT.emu_reduce(logits, labels)
    return (sums,) + LT.emu_finish(sums, N, C, V, names, combine)


def emu_grad(logits, labels, sums, consts, gs, names, phi, gb, out_stride=None, defect=None, dcomb=1.0, alpha=1.0):
    """The BND form of the family's gradient kernel in torch fp32: its emu_grad's fl(gs acc) as an fp32 value, the boundary part
    added, ONE rounding to the logits' dtype into a zeroed [.., out_stride] buffer.  ``dcomb``, ``alpha``: what the defects
    scaled_by_dcomb and alpha_twice multiply the boundary part by once more."""
    N, C = labels.shape[:2]
    V = labels[0, 0].numel()
    Cs = logits.shape[-1] if out_stride is None else out_stride
    f = np.float32
    grad_names = [n for n in names if n != "multi_neighbor"]
    lg32 = logits.float()
    if three_term(names):
        o = LR.emu_grad(lg32, labels, sums, gs, _weights(names)).reshape(N, V, -1)[..., :C].permute(0, 2, 1)
    elif grad_names:
        o = LT.emu_grad(lg32, labels, consts, gs, grad_names).reshape(N, V, -1)[..., :C].permute(0, 2, 1)
    else:
        o = torch.zeros(N, C, V)
    p = _f32(lg32.reshape(N, V, -1)[..., :C]).permute(0, 2, 1)
    s = LR.emu_sigmoid(p)
    ds = s if defect == "phi_s" else _f32(s * _f32(1.0 - s))
    a_bnd = f(1.0 / (float(N) * V if defect == "divisor_nv" else float(N) * C * V))
    gbv = f(gb)
    if defect == "scaled_by_dcomb":
        gbv = f(gbv * f(dcomb))
    if defect == "alpha_twice":
        gbv = f(gbv * f(alpha))
    b = _f32(gbv * _f32(_f32(phi.reshape(N, C, V).float() * ds) * a_bnd))
    v = _f32(o + b).to(logits.dtype)
    out = torch.zeros(N, V, Cs, dtype=logits.dtype)
    out[..., :C] = v.permute(0, 2, 1)
    if defect == "padding_written" and Cs > C:
        out[..., C:] = v.permute(0, 2, 1)[..., :1]
    return out.reshape(*logits.shape[:-1], Cs)


# ---- cases ---------------------------------------------------------------------------------------------------------------------------------
SHAPES = ((2, 3, 5, 7, 9), (2, 4, 33, 35, 40))
NAME_SETS = (("dice",), ("mse", "bce", "dice"), ("dice_ce", "multi_neighbor"))
COMBINES = ("sum", "mean", "log")
ALPHA = 0.37          # not 1, so that applying it twice shows


def make_case(shape, dtype, Cs, seed=3):
    """(logits channels-last [N, D, H, W, Cs] on the CPU, labels fp32 one-hot with 30 % unlabelled voxels)."""
    N, C, D, H, W = shape
    g = torch.Generator().manual_seed(seed + C)
    labels = LT.make_labels("onehot_background", N, C, (D, H, W), g)
    x = LT.make_logits("randn", N, C, (D, H, W), g, dtype)
    return LT.channels_last(x, dtype, Cs, 0, "cpu"), labels
