"""fp64 reference of the Step-Uncertainty Fusion step (csrc/suf.hip, dua_suf_accumulate; the torch form is
gaussian_diffusion.step_uncertainty_fusion) with a per-element error bound, in the style of tests/loss_fp64ref.py and
tests/sampler_fp64ref.py.  A plain helper module (``import suf_fp64ref``).

The contract (include/dua_hip.h).  Window (group) g has R runs in adjacent batch rows n = g R + r; step k of T counts in loop
order; l_r is run r's raw model output.  Per (g, class, voxel):

    m   = (l_0 + l_1 + ... + l_{R-1}) / R
    p   = max(sigmoid(m), 0.001)
    u   = -p log(p)
    a_k = sigmoid((k + 1) / T)
    w   = exp(a_k (1 - u))
    acc += w (x0_0 + ... + x0_{R-1}),   x0_r = clamp(l_r, -1, 1)

``step_ref`` evaluates this in float64 on the exact fp32 operands (logits and acc as stored); 0.001 and a_k are the real numbers
there, and the roundings of the kernel's fp32 copies of them are terms of the bound.

The bound, operation by operation (U = 2^-24, the unit roundoff; an error of n ulp is at most 2 n U relative; the build is
-ffp-contract=off, so nothing fuses):

* the sum of the logits: R - 1 additions, each off by at most U times its partial sum:   e_S = (R - 1) U sum|l_r|
* the IEEE division by (float) R (exact for R <= 2^24):                                   e_m = e_S / R + U |m| + 2^-150
* the sigmoid, 1 / (1 + __expf(-m)), the form of seg_loss.hip: the argument's error reaches s scaled by s' = s (1 - s), and the
  evaluation itself is loss_fp64ref.sigmoid_err (its e_s, with EPS_SIG; it covers the exponential's overflow, where the kernel
  gets s = 0 and the true s is below 2^-126):                                             e_s = s (1 - s) e_m + sigmoid_err(m, s)
* max(., 0.001f) is 1-Lipschitz; where the clamp can be active the kernel's constant is off by U 0.001:
                                                                                          e_p = e_s [+ U 0.001]
* logf: LOGF_ULPS from the HIP math API's accuracy table; the negation is exact, the product rounds once.  u = h(p) with
  h'(p) = -(log p + 1), h''(p) = -1 / p (p >= 0.001, so the second-order term is kept explicitly: the first vanishes at 1 / e):
                                            e_u = |log p + 1| e_p + e_p^2 / (2 p) + (2 LOGF_ULPS + 1) U |u|
* 1 - u rounds once:                                                                      e_v = e_u + U (1 - u)
* a_k is an fp32 table entry (U a_k) and the product rounds once:                         e_t = a_k e_v + 2 U a_k (1 - u)
* expf: EXPF_ULPS from the same table; d exp(t) = exp(t) dt:                              e_w = w (e_t + 2 EXPF_ULPS U)
* the sum of the clamped logits (the clamp is exact): R - 1 additions:                    e_X = (R - 1) U sum|x0_r|
* the product w X rounds once:                                                            e_P = |X| e_w + w e_X + U |w X|
* the final add rounds once, and a result below the smallest normal is off by half a subnormal:
                                            bound = SECOND_ORDER (e_P + U |ref|) + 2^-150

SECOND_ORDER (1.001) covers products of two relative errors, each below 1e-4 here.  Nothing is fitted to what a kernel returns,
nothing is normalised by a tensor's maximum and there is no percentage clause: ``check`` looks at every element.

A loop of T steps (``loop_ref``) is the sum of its steps' bounds: an error already in acc passes through the add unchanged.

HIP math API reference, "Single precision mathematical functions", maximum ULP error: expf 1, logf 2.
"""
from __future__ import annotations

import math

import numpy as np
import torch

import fp64ref
import loss_fp64ref
from fp64ref import FLOOR32, U32
from loss_fp64ref import SECOND_ORDER, emu_sigmoid, sigmoid_err

P_MIN = 0.001
LOGF_ULPS = 2
EXPF_ULPS = 1

check = loss_fp64ref.check


def step_coef(k, T):
    """a_k as a real number (float64)."""
    return 1.0 / (1.0 + math.exp(-(k + 1) / T))


def operands(logits, acc, G):
    """float64 views: l [G, R, P] (runs of a group adjacent), acc [G, P]."""
    assert logits.shape[0] % G == 0
    return logits.double().reshape(G, logits.shape[0] // G, -1), acc.double().reshape(G, -1)


def step_ref(logits, acc, G, k, T):
    """One fusion step in float64 on the fp32 operands: dict(ref, bound, below (p clamp active), outside (|l| > 1)), ref and
    bound shaped like ``acc``."""
    l, a0 = operands(logits, acc, G)
    R = l.shape[1]
    m = l.sum(1) / R
    s = torch.sigmoid(m)
    p = s.clamp(min=P_MIN)
    logp = torch.log(p)
    u = -p * logp
    a = step_coef(k, T)
    w = torch.exp(a * (1 - u))
    x0 = l.clamp(-1, 1)
    X = x0.sum(1)
    ref = a0 + w * X
    # the bound (module docstring)
    e_m = (R - 1) * U32 * l.abs().sum(1) / R + U32 * m.abs() + FLOOR32
    e_s = s * (1 - s) * e_m + sigmoid_err(m, s)
    e_p = e_s + (s <= P_MIN + e_s).double() * (U32 * P_MIN)
    e_u = (logp + 1).abs() * e_p + e_p * e_p / (2 * p) + (2 * LOGF_ULPS + 1) * U32 * u.abs()
    e_v = e_u + U32 * (1 - u)
    e_t = a * e_v + 2 * U32 * a * (1 - u)
    e_w = w * (e_t + 2 * EXPF_ULPS * U32)
    e_X = (R - 1) * U32 * x0.abs().sum(1)
    e_P = X.abs() * e_w + w * e_X + U32 * (w * X).abs()
    bound = SECOND_ORDER * (e_P + U32 * ref.abs()) + FLOOR32
    return {"ref": ref.reshape(acc.shape), "bound": bound.reshape(acc.shape), "below": s < P_MIN, "outside": l.abs() > 1}


def loop_ref(step_logits, G):
    """A whole loop from acc = 0: ``step_logits[k]`` the fp32 logits [G R, C, ...] of step k.  (ref, bound) float64 [G, C, ...]."""
    T = len(step_logits)
    shape = (G, *step_logits[0].shape[1:])
    acc = torch.zeros(shape, dtype=torch.float64, device=step_logits[0].device)
    bound = torch.zeros_like(acc)
    for k, lg in enumerate(step_logits):
        r = step_ref(lg, acc, G, k, T)
        acc, bound = r["ref"], bound + r["bound"]
    return acc, bound


# ---- the kernel's own arithmetic in torch fp32 (CPU), library calls rounded once ------------------------------------------------
def _f32(x):
    return x.to(torch.float32)


DEFECTS = ("mean_of_sigmoids", "no_p_clamp", "k_over_T", "x0_unclamped", "sum_for_mean", "runs_strided")


def emu_step(logits, acc, G, k, T, defect=None):
    """fp32 emulation of dua_suf_accumulate (sums in run order, IEEE division, loss_fp64ref.emu_sigmoid, logf / expf as
    correctly rounded functions); ``defect``: one of DEFECTS."""
    assert defect is None or defect in DEFECTS
    N = logits.shape[0]
    R = N // G
    flat = logits.reshape(N, -1)
    l = flat.reshape(R, G, -1).transpose(0, 1) if defect == "runs_strided" else flat.reshape(G, R, -1)
    clamp = (lambda t: t) if defect == "x0_unclamped" else (lambda t: t.clamp(-1, 1))
    sl, sx = l[:, 0].clone(), clamp(l[:, 0]).clone()
    ss = emu_sigmoid(l[:, 0])
    for r in range(1, R):
        sl = _f32(sl + l[:, r])
        sx = _f32(sx + clamp(l[:, r]))
        ss = _f32(ss + emu_sigmoid(l[:, r]))
    rc = np.float32(R)
    m = sl if defect == "sum_for_mean" else _f32(sl / rc)
    p = _f32(ss / rc) if defect == "mean_of_sigmoids" else emu_sigmoid(m)
    if defect != "no_p_clamp":
        p = p.clamp(min=float(np.float32(P_MIN)))
    else:
        p = p.clamp(min=2.0 ** -126)               # keep the logarithm finite: the defect is the missing 0.001, not a NaN
    u = _f32(-p * _f32(torch.log(p.double())))
    a = np.float32(step_coef(k - 1 if defect == "k_over_T" else k, T))
    t = _f32(a * _f32(1 - u))
    w = _f32(torch.exp(t.double()))
    return _f32(acc.reshape(G, -1) + _f32(w * sx)).reshape(acc.shape)


# ---- shared cases ----------------------------------------------------------------------------------------------------------------
ODD, POW2 = (5, 7, 9), (8, 8, 8)                    # 315 voxels: class planes off 16-byte alignment, scalar path; 512: vector path
STEPS = ((0, 10), (9, 10), (2, 3))
PLANTED = (0.0, 1.0, -1.0, 0.5, -6.9, -7.0, 100.0, -100.0)      # -6.9 / -7 straddle the 0.001 clamp; +-100: the exponential's overflow
SCALES = (0.3, 1.5, 6.0, 12.0)


def _cases():
    out = []
    Cs, Gs = (1, 3, 16), (1, 2)
    i = 0
    for dims in (ODD, POW2):
        for R in (1, 2, 3, 4, 5):
            out.append({"G": Gs[i % 2], "R": R, "C": Cs[i % 3], "dims": dims, "step": STEPS[i % 3]})
            i += 1
    # the combinations the walk above misses: every C on both paths with two groups, the widest at the odd extent
    out += [{"G": 2, "R": 3, "C": 16, "dims": ODD, "step": STEPS[1]}, {"G": 2, "R": 2, "C": 1, "dims": POW2, "step": STEPS[2]},
            {"G": 1, "R": 5, "C": 3, "dims": ODD, "step": STEPS[0]}, {"G": 2, "R": 4, "C": 3, "dims": POW2, "step": STEPS[1]}]
    for n, c in enumerate(out):
        c["seed"] = 100 + n
        c["id"] = f"G{c['G']}-R{c['R']}-C{c['C']}-{'x'.join(map(str, c['dims']))}-k{c['step'][0]}of{c['step'][1]}"
    return out


CASES = _cases()


def make_logits(case, salt=0):
    """fp32 [G R, C, *dims] (CPU): normals scaled per (group, class, voxel) -- the same scale in every run -- by one of SCALES,
    then PLANTED written into every run at spread positions of each group."""
    G, R, C, dims = case["G"], case["R"], case["C"], case["dims"]
    P = C * dims[0] * dims[1] * dims[2]
    gen = torch.Generator().manual_seed(case["seed"] * 1000 + salt)
    scale = torch.tensor(SCALES)[torch.randint(0, len(SCALES), (G, 1, P), generator=gen)]
    l = torch.randn(G, R, P, generator=gen) * scale
    for i, v in enumerate(PLANTED):
        l[:, :, (i * P) // len(PLANTED) + i % 3] = v
    return l.reshape(G * R, C, *dims).float().contiguous()


def make_acc(case):
    """fp32 [G, C, *dims] (CPU): O(5) values, exactly zero in about a third of the elements."""
    gen = torch.Generator().manual_seed(case["seed"] * 1000 + 999)
    shape = (case["G"], case["C"], *case["dims"])
    acc = 5 * torch.randn(shape, generator=gen)
    acc[torch.rand(shape, generator=gen) < 0.3] = 0.0
    return acc.float().contiguous()
