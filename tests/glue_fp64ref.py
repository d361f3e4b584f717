"""fp64 references of the training-glue kernels (csrc/train_glue.hip: q_sample_affine, temb_train_fwd / temb_train_bwd,
grads_nonfinite, adamw_step, adamw_advance, stats_channel_sums) and per-element error bounds, in the style of tests/fp64ref.py and
tests/loss_fp64ref.py.  A plain helper module (``import glue_fp64ref``).

Every reference is float64, evaluated on the exact operands a launch read: the fp32 tensors as stored and the fp32 scalars as the
C ABI receives them.  The ABI takes ``float beta1, beta2, eps, lr, weight_decay, a, b``: the references take the fp32-rounded
values (``f32``).  torch.optim.AdamW holds Python doubles (0.9, 0.999, 1e-8); the 3e-8 relative between 0.9 and float(0.9f) is a
property of the interface, not an error of the kernel, and no bound covers it.  All tensors stay on the device of the operands.

Bounds (u = 2^-24; the library is built -O3 -ffp-contract=off without fast-math, so fp32 +, -, *, / and sqrtf round once each
(IEEE division and square root: no -fno-hip-fp32-correctly-rounded-divide-sqrt), only the explicit fmaf calls fuse, denormals are
kept; an operation whose result may underflow loses at most DEN = 2^-149 absolutely).  First-order sums of roundings are multiplied
by SECOND_ORDER.  Nothing is normalised by a tensor's maximum, nothing is taken from a kernel's output.

* q_sample_affine.  out = fl(fl(c0 x0) + fl(c1 e)), x0 = fl(fl(a s) + b), t clamped to [0, T - 1] -- the kernel's clamp is the
  contract (torch indexing would raise or wrap): the reference clamps.  The roundings of x0 reach the result times |c0|:
      |c0| u (|a s| + |x0|)  +  u (|c0 x0| + |c1 e|)  +  u |ref|          (x0; the two products; the sum, which is the store)
* Library functions.  sinf, cosf and expf are calls into the device library (only the loss kernels use __expf; EPS_SIG of
  loss_fp64ref does not apply).  Their error is the accuracy the library documents, the OpenCL figures the project already uses
  for log1pf: sin and cos 4 ulp, exp 3 ulp; one ulp is at most 2 u of the value.
      sigmoid  s = fl(1 / fl(1 + E)), E = expf(-x):  e_s = s ((1 - s) 6 u + 2 u) + 2^-126
               (d s / s = -(1 - s) d E / E; the add; the division; 2^-126 where E overflows and s is stored as 0 or a denormal)
      swish    fl(x s):                               |x| e_s + u |x s| + DEN
      dswish   fl(s fl(1 + fl(x fl(1 - s)))):         w = 1 + x (1 - s),  e_w = |x| e_s + 2 u |x| (1 - s) + u |w|,
                                                      e_s |w| + s e_w + u |s w| + DEN
* Matrix-vector rows of temb_train_fwd.  A lane adds ceil(K / 64) fmaf terms (one rounding each), six shuffle levels add the 64
  lanes, one add for the bias: (ceil(K / 64) + 7) u (sum |w x| + |b|).
      stage 0   arg = fl(t freq) is an operand (one IEEE product, formed in fp32 on the host the same way).  e = [sin | cos](arg)
                is stored by the launch and checked at 4 ulp; z1 = W0 e + b0 is checked against the reference's own e, so the
                4 ulp of e enter z1's bound as 8 u sum |w e|; h1 = swish(z1) is checked on the z1 the launch stored.
      stage 1   z2 = W1 h1 + b1 on the stored h1, s = swish(z2) on the stored z2.
      stage 2   add_b = Wp_b s + bp_b on the stored s, block-major: block b's [N][cout_b] at N * (cout_0 + .. + cout_{b-1}).
* temb_train_bwd.  A chunk of 64 rows: each row half is a chain of 32 fmaf terms, one add joins the halves (33 roundings on the
  longest path), the next launch adds the nch chunk partials in a fixed order starting from 0 (nch roundings):
      d s   = sum_r Wp[r][k] dadd[r]              (33 + nch1) u sum |w d|,         nch1 = ceil(P / 64)
      dz2   = fl(d s dswish(z2))                  e_ds |dswish| + |d s| e_dswish + u |dz2| + DEN      (z2 as stored)
      d h   = sum_r W1[r][k] dz2[r]               (33 + nch2) u sum |w dz2|,       nch2 = hidden / 64   (dz2 as the device stored it)
      dz1   = fl(d h dswish(z1))                  as dz2; it is not stored, its error e_dz1 enters dw0 and db0 per sample
      dw[o][k] = sum_n d[n][o] act[n][k]          N fmaf terms: N u sum |d act| (+ sum_n e_dz1[n] |e[n][k]| for dw0)
      db[o]    = sum_n d[n][o]                    N adds: N u sum |d| (+ sum_n e_dz1[n] for db0)
  with (d, act) = (dadd_b, s), (dz2, h1), (dz1, e), every activation as stored by the forward launches.
* adamw_step, per element, as adam_one is written; g' = fl(g inv) is exact in the reference (24 x 24 bits fit a double, rounded
  once), as are inv = fl(1 / scale) and the two bias-correction constants c1 = fl(1 - beta1^k), c2 = fl(sqrt(1 - beta2^k)),
  evaluated in fp64 and rounded once as the kernel does.  The fp32 scalars lr wd, 1 - beta1, 1 - beta2, lr / c1 round once each.
      p1 = fl(p - fl(fl(lr wd) p))                e_p1 = 2 u |lr wd p| + u |p1| + DEN
      m' = fl(m + fl(fl(1 - b1) fl(g' - m)))      e_m  = 3 u |(1 - b1)(g' - m)| + u |m'| + DEN
      v' = fl(fl(b2 v) + fl(fl(fl(1 - b2) g') g')) e_v = 3 u (1 - b2) g'^2 + u b2 v + u v' + 2 DEN      (g'^2 may underflow)
      r  = sqrtf(v')                              e_r  = e_v / (2 r) where e_v <= 1e-3 v', else min(e_v / r, sqrt(e_v)); + u r
                                                  (|sqrt a - sqrt b| = |a - b| / (sqrt a + sqrt b) <= sqrt |a - b|: v' = 0 is bounded)
      q  = fl(r / c2), den = fl(q + eps)          e_q = e_r / c2 + u q + DEN,  e_den = e_q + u den
      num = fl(fl(lr / c1) m')                    e_num = 2 u |num| + |lr / c1| e_m + DEN
      f  = fl(num / den)                          e_f = e_num / den + |f| e_den / den + u |f| + DEN
      p' = fl(p1 - f)                             e_p = e_p1 + e_f + u |p'|
  The DEN terms are the absolute floor: with g = 0, v = 0 the update is p1 exactly (den = eps), and an underflowing g'^2 costs
  at most 2 DEN in v'.
* adamw_advance: integers and one fp32 product; exact equality.
* stats_channel_sums: fp64 sum over the samples of the decoded words, rounded once: u |ref| (+ 2^-45 sum |S| for the order of
  the fp64 additions).

``emu_*`` restate each kernel's own order of operations in torch fp32 on the CPU (a correctly rounded library function stands in
for sinf / cosf / expf), each with the planted defects tests/test_glue_fp64ref.py rejects.
"""
from __future__ import annotations

import math

import numpy as np
import torch

import fp64ref
from fp64ref import FLOOR32, U32, CheckResult   # noqa: F401  (re-exported for the tests)

F32, F64 = torch.float32, torch.float64
SECOND_ORDER = 1.001          # first-order bounds times this: products of two relative errors of <= 1e-4 each
FLT_MIN = 2.0 ** -126
FLT_MAX = float(np.finfo(np.float32).max)
DEN = 2.0 ** -149             # the smallest fp32 subnormal
ULP = 2 * U32                 # one ulp of a value, relative to it, at most
SINCOS_ULPS, EXP_ULPS = 4, 3  # documented accuracy of the device library's sinf / cosf and expf
STAT_FRAC = float(2 ** 44)
AD_CHUNK = 4096               # elements per workgroup of grads_nonfinite / adamw_step
TF_ROWS, TB_ROWS = 16, 64     # rows per workgroup of temb_train_fwd / per chunk of temb_train_bwd


def f32(x):
    """A Python number as the C ABI's ``float`` parameter holds it."""
    return float(np.float32(x))


def check(got, ref, bnd):
    """fp64ref.check on tensors of any layout."""
    return fp64ref.check(got.double().contiguous(), ref.double().contiguous(), bnd.double().contiguous())


def _cdiv(a, b):
    return -(-a // b)


# ---- q_sample_affine -----------------------------------------------------------------------------------------------------------
def q_sample_affine_ref(src, a, b, eps, sched, t):
    """(ref, bound), float64 [N, per]: c0 (a s + b) + c1 e with (c0, c1) = sched[clamp(t, 0, T - 1)] as stored (fp32)."""
    N = src.shape[0]
    s, e = src.reshape(N, -1).double(), eps.reshape(N, -1).double()
    a, b = f32(a), f32(b)
    c = sched.double()[t.to(sched.device).clamp(0, sched.shape[0] - 1)]
    c0, c1 = c[:, 0:1], c[:, 1:2]
    as_ = a * s
    x0 = as_ + b
    ref = c0 * x0 + c1 * e
    bnd = c0.abs() * U32 * (as_.abs() + x0.abs()) + U32 * ((c0 * x0).abs() + (c1 * e).abs() + ref.abs())
    return ref, bnd * SECOND_ORDER + (2 * c0.abs() + 2) * DEN


# ---- the library functions -------------------------------------------------------------------------------------------------------
def _sigmoid(x):
    """(s, 1 - s, e_s) of the kernels' tg_sigmoid at float64 x."""
    s, om = torch.sigmoid(x), torch.sigmoid(-x)
    return s, om, s * (om * EXP_ULPS * ULP + 2 * U32) + FLT_MIN


def swish_ref(x):
    x = x.double()
    s, _, es = _sigmoid(x)
    ref = x * s
    return ref, (x.abs() * es + U32 * ref.abs()) * SECOND_ORDER + DEN


def dswish_ref(x, without_x_term=False):
    x = x.double()
    s, om, es = _sigmoid(x)
    w = 1 + x * om
    if without_x_term:
        w = torch.ones_like(w)
    ew = x.abs() * es + 2 * U32 * x.abs() * om + U32 * w.abs()
    ref = s * w
    return ref, (es * w.abs() + s * ew + U32 * ref.abs()) * SECOND_ORDER + DEN


# ---- timestep embedding -----------------------------------------------------------------------------------------------------------
def temb_freqs(half):
    """exp(arange(half) * -(ln 10000 / (half - 1))) in fp32, as models/diffusion/utils.py:15-17 computes it."""
    return torch.exp(torch.arange(half, dtype=F32) * -(math.log(10000) / (half - 1)))


def split_saved(saved, half, hid):
    """The [N][2 half + 4 hid] buffer of temb_train_fwd as views: e, z1, h1, z2, s."""
    ed = 2 * half
    return dict(e=saved[:, :ed], z1=saved[:, ed:ed + hid], h1=saved[:, ed + hid:ed + 2 * hid],
                z2=saved[:, ed + 2 * hid:ed + 3 * hid], s=saved[:, ed + 3 * hid:ed + 4 * hid])


def _rows(W, x, bias, extra_u=0.0):
    """x [N, K] @ W[R, K]^T + bias: (ref, bound) of one temb_train_fwd stage; ``extra_u``: relative error of x itself."""
    W, x, bias = W.double(), x.double(), bias.double()
    K = W.shape[1]
    ref = x @ W.t() + bias
    mag = x.abs() @ W.abs().t()
    chain = _cdiv(K, 64) + 7
    return ref, (chain * U32 * (mag + bias.abs()) + extra_u * mag) * SECOND_ORDER + chain * DEN


def block_major(rows):
    """[N, cout_b] per block -> the flat block-major buffer."""
    return torch.cat([r.reshape(-1) for r in rows])


def block_rows(flat, N, couts):
    """The flat block-major buffer -> [N, cout_b] views."""
    out, off = [], 0
    for c in couts:
        out.append(flat[N * off:N * off + N * c].view(N, c))
        off += c
    return out


def temb_fwd_ref(t, freqs, w0, b0, w1, b1, ws, bs, saved=None):
    """dict name -> (ref, bound) for e, z1, h1, z2, s (each [N, .]) and add (flat, block-major).  ``saved``: the device's buffer,
    so that every stage is evaluated on what its launch read; None chains the reference's own values (the plain float64
    statement of the embedder, bounds meaningless)."""
    half, hid = freqs.numel(), w1.shape[0]
    arg = (t.to(F32)[:, None] * freqs.to(F32)[None, :]).double()          # one fp32 product per element: the operand
    e = torch.cat([torch.sin(arg), torch.cos(arg)], 1)
    out = {"e": (e, SINCOS_ULPS * ULP * e.abs() + DEN)}
    dev = split_saved(saved, half, hid) if saved is not None else None
    out["z1"] = _rows(w0, e, b0, extra_u=SINCOS_ULPS * ULP)
    out["h1"] = swish_ref(dev["z1"] if dev else out["z1"][0])
    out["z2"] = _rows(w1, dev["h1"] if dev else out["h1"][0], b1)
    out["s"] = swish_ref(dev["z2"] if dev else out["z2"][0])
    per = [_rows(w, dev["s"] if dev else out["s"][0], b) for w, b in zip(ws, bs)]
    out["add"] = (block_major([p[0] for p in per]), block_major([p[1] for p in per]))
    return out


def _chunk_sum(W, d, nch):
    """d [N, R] through W [R, K] in chunks of 64 rows: (ref [N, K], e [N, K]) with the (33 + nch) u chain."""
    W, d = W.double(), d.double()
    ref, mag = d @ W, d.abs() @ W.abs()
    return ref, (33 + nch) * U32 * mag + (33 + nch) * DEN


def _outer(d, act, ed=None):
    """sum_n d[n][o] act[n][k] and sum_n d[n][o]: ((dw, bound), (db, bound)); ``ed``: the error of d itself."""
    d, act = d.double(), act.double()
    N = d.shape[0]
    dw, mw = d.t() @ act, d.abs().t() @ act.abs()
    db, mb = d.sum(0), d.abs().sum(0)
    bw, bb = N * U32 * mw, N * U32 * mb
    if ed is not None:
        bw, bb = bw + ed.t() @ act.abs(), bb + ed.sum(0)
    return (dw, bw * SECOND_ORDER + (N + 1) * DEN), (db, bb * SECOND_ORDER + (N + 1) * DEN)


def temb_bwd_ref(dadd, w1, ws, saved, half, dz2=None, dswish_without_x=False):
    """dict name -> (ref, bound): dz2 [N, hid] from dadd, the block weights and the stored z2; dw0, db0, dw1, db1 and the lists
    dw, db from ``dz2`` (the device's; None: the reference's own) and the stored z1, h1, s, e."""
    hid, N = w1.shape[0], saved.shape[0]
    couts = [w.shape[0] for w in ws]
    P = sum(couts)
    sv = split_saved(saved, half, hid)
    drows = block_rows(dadd, N, couts)
    ds, e_ds = _chunk_sum(torch.cat(list(ws), 0), torch.cat(drows, 1), _cdiv(P, TB_ROWS))
    k2, e_k2 = dswish_ref(sv["z2"], dswish_without_x)
    g = ds * k2
    out = {"dz2": (g, (e_ds * k2.abs() + ds.abs() * e_k2 + U32 * g.abs()) * SECOND_ORDER + DEN)}
    dz2 = g if dz2 is None else dz2.double()
    dh, e_dh = _chunk_sum(w1, dz2, hid // TB_ROWS)
    k1, e_k1 = dswish_ref(sv["z1"], dswish_without_x)
    dz1 = dh * k1
    e_dz1 = (e_dh * k1.abs() + dh.abs() * e_k1 + U32 * dz1.abs()) * SECOND_ORDER + DEN
    out["dw0"], out["db0"] = _outer(dz1, sv["e"], e_dz1)
    out["dw1"], out["db1"] = _outer(dz2, sv["h1"])
    per = [_outer(d, sv["s"]) for d in drows]
    out["dw"], out["db"] = [p[0] for p in per], [p[1] for p in per]
    return out


# ---- AdamW ------------------------------------------------------------------------------------------------------------------------
def bias_constants(k, beta1, beta2, fp32_abi=True):
    """(1 - beta1^k, sqrt(1 - beta2^k)) in float64, rounded once to fp32 as the kernel holds them."""
    c1, c2 = 1.0 - math.pow(beta1, k), math.sqrt(1.0 - math.pow(beta2, k))
    return (f32(c1), f32(c2)) if fp32_abi else (c1, c2)


def _adamw(p, g, m, v, k, lr, beta1, beta2, eps, wd, inv_scale, fp32_abi=True):
    p, g, m, v = p.double(), g.double(), m.double(), v.double()
    c1, c2 = bias_constants(k, beta1, beta2, fp32_abi)
    gu = g * inv_scale
    if fp32_abi:
        gu = gu.float().double()
    r = dict(gu=gu, c1=c1, c2=c2)
    r["decay"] = lr * wd * p
    r["p1"] = p - r["decay"]
    r["md"] = (1.0 - beta1) * (gu - m)
    r["m"] = m + r["md"]
    r["gg"], r["bv"] = (1.0 - beta2) * gu * gu, beta2 * v
    r["v"] = r["bv"] + r["gg"]
    r["r"] = r["v"].sqrt()
    r["q"] = r["r"] / c2
    r["den"] = r["q"] + eps
    r["num"] = (lr / c1) * r["m"]
    r["f"] = r["num"] / r["den"]
    r["p"] = r["p1"] - r["f"]
    return r


def adamw_ref(p, g, m, v, k, lr, beta1, beta2, eps, wd, inv_scale, fp32_abi=True):
    """One AdamW step in float64, operation for operation as adam_one is written: (p, m, v, g_unscaled).  ``fp32_abi`` (the
    kernel's interface): the scalars are taken as given (pass f32 values), g_unscaled and the two bias-correction constants are
    rounded once to fp32.  False: plain float64 throughout, torch.optim.AdamW's own statement."""
    r = _adamw(p, g, m, v, k, lr, beta1, beta2, eps, wd, inv_scale, fp32_abi)
    return r["p"], r["m"], r["v"], r["gu"]


def adamw_bound(p, g, m, v, k, lr, beta1, beta2, eps, wd, inv_scale):
    """(bound p, bound m, bound v) of adamw_ref's results (module docstring)."""
    r = _adamw(p, g, m, v, k, lr, beta1, beta2, eps, wd, inv_scale)
    e_p1 = 2 * U32 * r["decay"].abs() + U32 * r["p1"].abs() + DEN
    e_m = 3 * U32 * r["md"].abs() + U32 * r["m"].abs() + DEN
    e_v = 3 * U32 * r["gg"] + U32 * r["bv"].abs() + U32 * r["v"].abs() + 2 * DEN
    root = r["r"]
    safe = root.clamp_min(1e-300)
    e_r = torch.where(e_v <= 1e-3 * r["v"], e_v / (2 * safe), torch.minimum(e_v / safe, e_v.sqrt())) + U32 * root
    e_q = e_r / r["c2"] + U32 * r["q"] + DEN
    e_den = e_q + U32 * r["den"]
    e_num = 2 * U32 * r["num"].abs() + abs(lr / r["c1"]) * e_m + DEN
    e_f = e_num / r["den"] + r["f"].abs() * e_den / r["den"] + U32 * r["f"].abs() + DEN
    e_p = e_p1 + e_f + U32 * r["p"].abs()
    return e_p * SECOND_ORDER, e_m * SECOND_ORDER, e_v * SECOND_ORDER


def advance_ref(step, found, scale, growth, factor, backoff, interval):
    """adamw_advance on host numbers: (step, found, scale, growth, seen) after the call.  ``scale`` / ``growth`` may be None.
    Integers and one fp32 product (torch._amp_update_scale_'s rule; a product that is not finite leaves the scale)."""
    bad = found != 0
    if bad:
        if scale is not None:
            scale = float(np.float32(scale) * np.float32(backoff))
        if growth is not None:
            growth = 0
    else:
        step += 1
        if growth is not None:
            if growth + 1 == interval:
                if scale is not None:
                    with np.errstate(over="ignore"):
                        ns = float(np.float32(scale) * np.float32(factor))
                    if math.isfinite(ns):
                        scale = ns
                growth = 0
            else:
                growth += 1
    return step, 0.0, scale, growth, 1.0 if bad else 0.0


# ---- stats_channel_sums -------------------------------------------------------------------------------------------------------------
def stats_channel_sums_ref(stats, C):
    """(ref, bound) [C]: the fp64 sum over the samples of the decoded "sum x" words of an int64 [N, 8, 4, c_pad] buffer."""
    w = stats.sum(1)
    S = (w[:, 0].double() + w[:, 1].double() / STAT_FRAC)[:, :C]
    ref = S.sum(0)
    return ref, U32 * ref.abs() + 2.0 ** -45 * S.abs().sum(0) + FLOOR32


# ---- the kernels' own arithmetic in torch fp32 (CPU) ------------------------------------------------------------------------------
def _f(x):
    return x.to(F32)


def _fma(a, b, c):
    """fmaf on fp32 tensors: the product is exact in float64, the sum rounds there far below fp32's last place."""
    return _f(a.double() * b.double() + c.double())


def _wave_tree(x):
    """x [..., 64] fp32: six xor-shuffle levels -> [...] (lane 0's value)."""
    for o in (32, 16, 8, 4, 2, 1):
        x = _f(x + x[..., torch.arange(64) ^ o])
    return x[..., 0]


def emu_q_sample_affine(src, a, b, eps, sched, t, defect=None):
    """q_sample_affine_kernel into a NaN-filled [N, per] buffer.  ``defect``: one_coef (sample 0's coefficients for all),
    last_piece (the last 16-byte piece of every sample left unwritten)."""
    N = src.shape[0]
    s, e = _f(src.reshape(N, -1)), _f(eps.reshape(N, -1))
    tc = t.clamp(0, sched.shape[0] - 1)
    if defect == "one_coef":
        tc = tc[:1].expand(N)
    c0, c1 = _f(sched)[tc, 0:1], _f(sched)[tc, 1:2]
    x0 = _f(_f(torch.tensor(a, dtype=F32) * s) + torch.tensor(b, dtype=F32))
    out = torch.full_like(s, float("nan"))
    out[:] = _f(_f(c0 * x0) + _f(c1 * e))
    if defect == "last_piece":
        out[:, -4:] = float("nan")
    return out


def emu_sigmoid(x):
    return _f(1.0 / _f(1.0 + _f(torch.exp(-x.double()))))


def emu_swish(x):
    return _f(x * emu_sigmoid(x))


def emu_dswish(x, defect=None):
    s = emu_sigmoid(x)
    if defect == "dswish_no_x":
        return s
    return _f(s * _f(1.0 + _f(x * _f(1.0 - s))))


def _emu_rows(W, x, bias):
    """One temb_train_fwd stage: lane l of a wave chains fmaf over k = l, l + 64, ..; the wave tree; the bias."""
    R, K = W.shape
    n = _cdiv(K, 64)
    Wp = torch.nn.functional.pad(_f(W), (0, n * 64 - K)).view(R, n, 64)
    xp = torch.nn.functional.pad(_f(x), (0, n * 64 - K)).view(-1, n, 64)
    acc = torch.zeros(xp.shape[0], R, 64, dtype=F32)
    for i in range(n):
        acc = _fma(Wp[None, :, i], xp[:, None, i], acc)
    return _f(_wave_tree(acc) + _f(bias))


def emu_temb_fwd(t, freqs, w0, b0, w1, b1, ws, bs, defect=None):
    """The three launches of dua_temb_train_fwd: (add flat block-major, NaN where nothing was written; saved [N, 2 half + 4 hid]).
    ``defect``: sincos_swapped, add_offset (block b at off + n cout instead of N off + n cout)."""
    N = t.numel()
    arg = _f(t.to(F32)[:, None] * _f(freqs)[None, :])
    sn, cs = _f(torch.sin(arg.double())), _f(torch.cos(arg.double()))
    e = torch.cat([cs, sn] if defect == "sincos_swapped" else [sn, cs], 1)
    z1 = _emu_rows(w0, e, b0)
    h1 = emu_swish(z1)
    z2 = _emu_rows(w1, h1, b1)
    s = emu_swish(z2)
    P = sum(w.shape[0] for w in ws)
    add = torch.full((N * P,), float("nan"), dtype=F32)
    off = 0
    for w, b in zip(ws, bs):
        c = w.shape[0]
        rows = _emu_rows(w, s, b)
        base = off if defect == "add_offset" else N * off
        add[base:base + N * c] = rows.reshape(-1)
        off += c
    return add, torch.cat([e, z1, h1, z2, s], 1)


def _emu_chunks(W, d):
    """Chunk partials of d [N, R] through W [R, K]: [N, nch, K]; each chunk = (even rows, 32 fmaf) + (odd rows, 32 fmaf)."""
    R, K = W.shape
    nch = _cdiv(R, TB_ROWS)
    Wp = torch.nn.functional.pad(_f(W), (0, 0, 0, nch * TB_ROWS - R)).view(nch, TB_ROWS, K)
    dp = torch.nn.functional.pad(_f(d), (0, nch * TB_ROWS - R)).view(-1, nch, TB_ROWS)
    halves = []
    for rg in (0, 1):
        acc = torch.zeros(dp.shape[0], nch, K, dtype=F32)
        for j in range(TB_ROWS // 2):
            acc = _fma(Wp[None, :, rg + 2 * j], dp[:, :, rg + 2 * j, None], acc)
        halves.append(acc)
    return _f(halves[0] + halves[1])


def _emu_chain(parts):
    acc = torch.zeros_like(parts[:, 0])
    for c in range(parts.shape[1]):
        acc = _f(acc + parts[:, c])
    return acc


def _emu_outer(d, act):
    N = d.shape[0]
    dw = torch.zeros(d.shape[1], act.shape[1], dtype=F32)
    db = torch.zeros(d.shape[1], dtype=F32)
    for n in range(N):
        dw = _fma(_f(d[n])[:, None], _f(act[n])[None, :], dw)
        db = _f(db + _f(d[n]))
    return dw, db


def emu_temb_bwd(dadd, w1, ws, saved, half, defect=None):
    """The three launches of dua_temb_train_bwd: dict dz2, dw0, db0, dw1, db1, dw (list), db (list).  ``defect``: dswish_no_x,
    drop_last_chunk (the last partial chunk of the temb_proj rows left out of d s)."""
    hid, N = w1.shape[0], saved.shape[0]
    couts = [w.shape[0] for w in ws]
    sv = split_saved(_f(saved), half, hid)
    drows = block_rows(_f(dadd), N, couts)
    part1 = _emu_chunks(torch.cat(list(ws), 0), torch.cat(drows, 1))
    if defect == "drop_last_chunk":
        part1 = part1[:, :-1]
    dz2 = _f(_emu_chain(part1) * emu_dswish(sv["z2"], defect))
    dz1 = _f(_emu_chain(_emu_chunks(w1, dz2)) * emu_dswish(sv["z1"], defect))
    out = {"dz2": dz2}
    out["dw0"], out["db0"] = _emu_outer(dz1, sv["e"])
    out["dw1"], out["db1"] = _emu_outer(dz2, sv["h1"])
    per = [_emu_outer(d, sv["s"]) for d in drows]
    out["dw"], out["db"] = [p[0] for p in per], [p[1] for p in per]
    return out


def emu_adamw(p, g, m, v, k, lr, beta1, beta2, eps, wd, scale=None, defect=None):
    """adamw_kernel on one tensor in torch fp32: (p, m, v, g').  ``defect``: k_is_step, wd_after, no_inv_scale, sqrt_v_over_bc2."""
    one = np.float32(1.0)
    lr, beta1, beta2, eps, wd = (np.float32(x) for x in (lr, beta1, beta2, eps, wd))
    kk = k - 1 if defect == "k_is_step" else k
    c1 = np.float32(1.0 - math.pow(float(beta1), kk))
    c2 = np.float32(math.sqrt(1.0 - math.pow(float(beta2), kk)))
    if defect == "sqrt_v_over_bc2":
        c2 = np.float32(1.0 - math.pow(float(beta2), kk))
    inv = one if scale is None or defect == "no_inv_scale" else one / np.float32(scale)
    lr_wd, w1, w2, step_size = lr * wd, one - beta1, one - beta2, lr / c1
    t = lambda x: torch.tensor(x, dtype=F32)      # noqa: E731
    p, g, m, v = _f(p), _f(g), _f(m), _f(v)
    gu = _f(g * t(inv))
    if defect != "wd_after":
        p = _f(p - _f(t(lr_wd) * p))
    m = _f(m + _f(t(w1) * _f(gu - m)))
    v = _f(_f(t(beta2) * v) + _f(_f(t(w2) * gu) * gu))
    den = _f(_f(v.sqrt() / t(c2)) + t(eps))
    p = _f(p - _f(_f(t(step_size) * m) / den))
    if defect == "wd_after":
        p = _f(p - _f(t(lr_wd) * p))
    return p, m, v, gu


def emu_advance(step, found, scale, growth, factor, backoff, interval, defect=None):
    """adamw_advance_kernel.  ``defect``: no_backoff (a bad step resets ``growth`` and leaves the scale)."""
    if defect == "no_backoff" and found != 0:
        return step, 0.0, scale, (0 if growth is not None else None), 1.0
    return advance_ref(step, found, scale, growth, factor, backoff, interval)


# ---- cases and checks shared by the CPU and the GPU file ----------------------------------------------------------------------------
SHIPPED_WIDTHS = [64, 64, 128, 256, 512, 256, 128, 64, 72]          # the nine temb_proj of DiffUNet: P = 1544


def make_temb_params(hid, half, couts, seed, device="cpu"):
    """(w0, b0, w1, b1, [w_b], [b_b]) scaled as tests/test_train_glue_gpu.py scales them; every tensor its own allocation."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)      # noqa: E731
    head = [r(hid, 2 * half) * 0.09, r(hid) * 0.1, r(hid, hid) * 0.045, r(hid) * 0.1]
    ws, bs = [r(c, hid) * 0.045 for c in couts], [r(c) * 0.1 for c in couts]
    to = lambda x: x.to(device).contiguous()         # noqa: E731
    return (*[to(x) for x in head], [to(w) for w in ws], [to(b) for b in bs])


def make_timesteps(N, shift=0):
    """0, 1 and 999 first (rotated by ``shift``, so that N = 1 sees each of them over the cases), then a spread."""
    base = [0, 1, 999]
    return torch.tensor([base[(i + shift) % 3] if i < 3 else (37 * i + 11 * shift) % 1000 for i in range(N)], dtype=torch.int64)


def temb_fwd_checks(add, saved, ref, half, hid):
    """CheckResult per quantity of temb_fwd_ref against the launches' ``add`` and ``saved``."""
    got = dict(split_saved(saved, half, hid), add=add)
    return {k: check(got[k], *ref[k]) for k in ("e", "z1", "h1", "z2", "s", "add")}


def temb_bwd_checks(got, ref):
    """CheckResult per gradient of temb_bwd_ref against a dict like emu_temb_bwd's (lists flattened to dw[i], db[i])."""
    res = {k: check(got[k], *ref[k]) for k in ("dz2", "dw0", "db0", "dw1", "db1")}
    for name in ("dw", "db"):
        for i, (g, r) in enumerate(zip(got[name], ref[name])):
            res[f"{name}[{i}]"] = check(g, *r)
    return res


def make_adam_inputs(n, seed):
    """(p, g, m, v) fp32 [n] on the CPU: v >= 0; every 7th element has g = 0 and v = 0 exactly (every 14th also m = 0), every
    11th |g| near 1e-20 (its square underflows), every 13th |g| near 1e4."""
    gen = torch.Generator().manual_seed(seed)
    p, g, m = (torch.randn(n, generator=gen) for _ in range(3))
    m = m * 0.1
    v = (torch.randn(n, generator=gen) * 0.1) ** 2
    i = torch.arange(n)
    mag = 1 + torch.rand(n, generator=gen)
    g = torch.where(i % 11 == 4, g.sign() * 1e-20 * mag, g)
    g = torch.where(i % 13 == 6, g.sign() * 1e4 * mag, g)
    zero = i % 7 == 3
    g, v = torch.where(zero, torch.zeros_like(g), g), torch.where(zero, torch.zeros_like(v), v)
    m = torch.where(i % 14 == 3, torch.zeros_like(m), m)
    return p, g, m, v
