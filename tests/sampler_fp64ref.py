"""fp64 references of the sampler tail (csrc/sampler.hip: final_conv_sampler in every form, q_sample, sampler_step), derived
per-element bounds, the numpy restatement of its noise generator and an fp32 emulation of the kernel's own arithmetic.

A plain helper module of the suite (``import sampler_fp64ref as T``), the sampler's counterpart of ``fp64ref`` (``R``) and
``swin_fp64ref`` (``S``), whose pieces it reuses: ``R.tail_transform``, ``R.contract``, ``R.bound``, ``R.check``,
``S.residual_norm_act_ref`` / ``_bound``.  Every reference is evaluated on the EXACT operands the kernel read: the stored raw /
res / ra tensors widened, the fp32 scale / shift of the kernels' own preamble (``ops.instnorm_finalize`` on the GPU, held there
to ``R.finalize`` of the statistics words), the fp32 weights, the fp32 coefficient rows, the fp32 state before the launch and
the fp32 eps field.  No constant below is fitted to what a kernel returns; the one number that cannot be derived is the
``5e-3`` of the Box-Muller known answer (``PHILOX_TOL``: the kernel takes the hardware's fast logarithm, sine and cosine), which
stays as tests/test_kernels_gpu.py has it and only identifies the counter: a wrong counter or key is off by O(1).

The head (u = 2^-24).  logit_c = b_c + sum_k a_k w_ck over the K channels.
    a_k    plain     LeakyReLU(fmaf(raw, sc, sh)) in fp32, emulated from float64 with one rounding (``R.tail_transform``): a rare
                     double rounding moves an input by one fp32 ulp, the ``emulated_in`` term of ``R.bound`` (C_RSS u sqrt(sum (a w)^2))
           identity  raw itself (norm = None, slope 1: fmaf(raw, 1, 0) and the slope product are exact)
           residual  LeakyReLU(fmaf(raw, sc, sh) + fmaf(res, rsc, rsh)) + ra (1 - sigmoid(ra)) for the real channels k < kvalid, in
                     float64 (``S.residual_norm_act_ref``); the kernel's fp32 value is within e_k = ``S.residual_norm_act_bound``
                     (6 roundings of the partial sums, the reverse-attention term's exponential and division, the other slope
                     within the pre-activation's rounding of 0): the logit moves by at most sum_k e_k |w_ck| (``act_err``).
                     Padding channels (kvalid <= k < K) have scale = shift = 0 and zero fragments: they contribute exactly 0
                     whatever the weights there are, and the reference leaves them out.
    sum    VALU form: acc = b_c, then one fmaf per channel: K + 1 roundings, u (K + 1) sum |terms| (``R.bound``, n_chain = K + 1).
           MFMA form: weights and activations are carried as fp16 pairs, x = hi + lo + d with |hi - x| <= 2^-11 |x| and
           |d| <= 2^-11 |lo| <= 2^-22 |x|; the products hi hi + lo hi + hi lo are exact in the fp32 accumulation, what is left of
           a w is lo lo + d terms: at most 3 * 2^-22 |a w| (``split``).  The accumulation is 3 K / 32 MFMA steps + 5 levels inside
           an instruction + the bias: far fewer than the K + 1 the bound allows, and that surplus is what pays for the one thing the
           split term leaves out: a lo half below 2^-14 (every |x| < 8) is an fp16 subnormal and rounds to a multiple of 2^-24, an
           absolute 2^-25 instead of 2^-11 |lo|.  tests/test_sampler_fp64ref.py runs an emulation with real fp16 subnormal
           rounding through the bound for every case, and shows that dropping either lo product does not pass.

The update (``sampler_update``; -ffp-contract=off: products and sums round separately).  dL = the head's bound above.
    x0^    = clamp(L, -1, 1); the clamp is exact and 1-Lipschitz:                       |d x0^| <= dL
    DDPM   x = fl(fl(fl(k0 x0^) + fl(k1 xt)) + fl(k2 eps)): three products, two sums, each sum bounded by the sum of |terms|:
                                                           |d x| <= |k0| dL + 4 u (|k0 x0^| + |k1 xt| + |k2 eps|) + floor
    DDIM   e = fl(fl(fl(k0 xt) - x0^) / k1):               de = (dL + 2 u (|k0 xt| + |x0^|)) / |k1| + u_div |e|
           x = fl(fl(fl(x0^ k2) + fl(k3 e)) + fl(k4 eps)): |d x| <= |k2| dL + |k3| de + 4 u (|k2 x0^| + |k3 e| + |k4 eps|) + floor
           u_div: csrc/Makefile compiles with -O3 -ffp-contract=off and neither -ffast-math nor
           -fno-hip-fp32-correctly-rounded-divide-sqrt, so fp32 ``/`` is the IEEE sequence (v_div_scale / v_rcp + fma refinement /
           v_div_fmas / v_div_fixup in the ISA of sampler.hip, denormal mode 3): correctly rounded, u_div = 2^-24 (``U_DIV_SAMPLER``),
           not the 2.5 ulp ``S.U_DIV`` allows an approximate division.
    xsum   s = fl(s_old + x0^):                            |d s| <= dL + u |s_old + x0^| + floor
    xstart                                                 dL
    xin    the stored state converted to the input type: bit-equal to its round-to-nearest, nothing to bound.
q_sample: fl(fl(c0 x0) + fl(c1 eps)): 3 u (|c0 x0| + |c1 eps|) + floor (``q_sample_ref``).

Noise: Philox4x32-10 (Salmon et al., SC'11; ``philox4x32_10`` below, pinned to the Random123 known-answer vectors by the host
test) with counter (lo32(gv), hi32(gv), step, class quad), gv = n vox + v, and key (lo32(seed), hi32(seed)); the four words
become two Box-Muller pairs, classes 4 q .. 4 q + 3 (``philox_normals``).

``emulate_tail`` restates the kernel's arithmetic in torch fp32 (fp16 hi / lo split, the three products per 32-channel step with
lo x lo dropped, one fp32 rounding per MFMA, the fmaf chain of the VALU form, the update) with switches for the planted defects
of tests/test_sampler_fp64ref.py; ``CASES`` / ``build_case`` are the inputs both test files share.
"""
from __future__ import annotations

import numpy as np
import torch

import fp64ref as R
import swin_fp64ref as S
from fp64ref import FLOOR32, U32

F16, F32, F64 = torch.float16, torch.float32, torch.float64
U_DIV_SAMPLER = U32                 # fp32 '/' is correctly rounded under the Makefile's flags (module docstring)
PHILOX_TOL = 5e-3                   # |kernel Box-Muller - float64 Box-Muller|: fast log / sin / cos (tests/test_kernels_gpu.py)
DDPM, DDIM = "ddpm", "ddim"


# ---- the head ---------------------------------------------------------------------------------------------------------------
def tail_logits_ref(raw, sc, sh, wf, bf, slope=R.SLOPE, identity=False, residual=None):
    """raw float64 [P, K] (exact stored values), sc / sh fp32 [P, K] (per-row constants of the kernel's preamble), wf [C, K],
    bf [C] -> (ref, sum |terms|, sum terms^2, act_err), each [P, C] (act_err: 0.0 unless ``residual``).
    ``identity``: the activation is raw.  ``residual`` = dict(res, rsc, rsh, ra or None, kvalid): raw / res / ra hold the real
    channels [P, kvalid]; wf's columns behind kvalid are ignored (they meet exact zeros)."""
    wfd, bfd = wf.detach().cpu().double(), bf.detach().cpu().double()
    act_err = 0.0
    if residual is not None:
        kv = residual["kvalid"]
        ra = residual.get("ra")
        a, parts = S.residual_norm_act_ref(raw[:, :kv], sc[:, :kv].double(), sh[:, :kv].double(), residual["res"][:, :kv],
                                           residual["rsc"][:, :kv].double(), residual["rsh"][:, :kv].double(), slope=slope,
                                           ra=None if ra is None else ra[:, :kv])
        wfd = wfd[:, :kv]
        act_err = S.residual_norm_act_bound(a, parts, F32) @ wfd.abs().t()
    elif identity:
        a = raw
    else:
        a = R.tail_transform(raw, sc, sh, slope)
    ref, ab, sq = R.contract(a, wfd.t())
    return ref + bfd, ab + bfd.abs(), sq, act_err


def tail_logits_bound(ref, ab, sq, K, split, emulated=True, act_err=0.0):
    """``split``: the MFMA form's fp16 hi / lo pairs (3 * 2^-22 of every product); ``emulated``: the activation is an fp32
    emulation of a fused transform (plain form), not an exact operand (identity) or a bounded one (residual: ``act_err``)."""
    extra = (3 * 2.0 ** -22 * ab if split else 0.0) + act_err
    return R.bound(ref, ab, sq, K + 1, F32, emulated_in=F32 if emulated else None, extra=extra)


# ---- the update -------------------------------------------------------------------------------------------------------------
def _mode(mode):
    return {1: DDPM, 2: DDIM}.get(mode, mode)


def update_ref(mode, coef_row_fp32, L, xt, eps, dL=0.0):
    """coef rows fp32 broadcastable to L (last axis 8: [..., 8]), L / xt / eps float64 of one shape [...]: returns
    (x0^, x_{t-1}, bound of x0^, bound of x_{t-1}) in float64 (module docstring).  ``dL``: bound on the kernel's logits."""
    k = coef_row_fp32.double()
    x0 = L.clamp(-1.0, 1.0)
    b0 = dL + torch.zeros_like(x0)
    if _mode(mode) == DDPM:
        t0, t1, t2 = k[..., 0] * x0, k[..., 1] * xt, k[..., 2] * eps
        x = t0 + t1 + t2
        bx = k[..., 0].abs() * dL + 4 * U32 * (t0.abs() + t1.abs() + t2.abs()) + FLOOR32
        return x0, x, b0, bx
    assert _mode(mode) == DDIM
    p = k[..., 0] * xt
    e = (p - x0) / k[..., 1]
    de = (dL + 2 * U32 * (p.abs() + x0.abs())) / k[..., 1].abs() + U_DIV_SAMPLER * e.abs()
    t0, t1, t2 = x0 * k[..., 2], k[..., 3] * e, k[..., 4] * eps
    x = t0 + t1 + t2
    bx = k[..., 2].abs() * dL + k[..., 3].abs() * de + 4 * U32 * (t0.abs() + t1.abs() + t2.abs()) + FLOOR32
    return x0, x, b0, bx


def xsum_ref(s_old, x0, dL=0.0):
    """running sum of x0^: (s_old + x0^, bound)"""
    s = s_old + x0
    return s, dL + U32 * s.abs() + FLOOR32


def q_sample_ref(c0, c1, x0, eps):
    t0, t1 = c0.double() * x0, c1.double() * eps
    return t0 + t1, 3 * U32 * (t0.abs() + t1.abs()) + FLOOR32


# ---- the noise --------------------------------------------------------------------------------------------------------------
_M32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key0, key1):
    """ctr uint64 [..., 4] (32-bit words), key words -> uint64 [..., 4]: ten rounds of Philox4x32 (Random123 philox.h)."""
    ctr = np.asarray(ctr, dtype=np.uint64)
    k0, k1 = np.uint64(key0) & _M32, np.uint64(key1) & _M32
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * ctr[..., 0]
        p1 = np.uint64(0xCD9E8D57) * ctr[..., 2]
        n0 = ((p1 >> np.uint64(32)) ^ ctr[..., 1] ^ k0) & _M32
        n2 = ((p0 >> np.uint64(32)) ^ ctr[..., 3] ^ k1) & _M32
        ctr = np.stack([n0, p1 & _M32, n2, p0 & _M32], -1)
        k0 = (k0 + np.uint64(0x9E3779B9)) & _M32
        k1 = (k1 + np.uint64(0xBB67AE85)) & _M32
    return ctr


def philox_normals(seed64, step, N, vox, quads):
    """float64 [N, vox, 4 * quads]: the standard normals final_conv_sampler draws for sample n, voxel v, classes 4 q + j:
    counter (lo32(gv), hi32(gv), step, q), gv = n vox + v, key (lo32(seed), hi32(seed)); u = (word + 0.5) 2^-32 in fp32 as the
    kernel forms it, Box-Muller in float64."""
    seed64 = int(seed64) & (2 ** 64 - 1)
    gv = (np.arange(N, dtype=np.uint64)[:, None] * np.uint64(vox) + np.arange(vox, dtype=np.uint64)[None, :]).reshape(-1)
    ctr = np.zeros((N * vox, quads, 4), dtype=np.uint64)
    ctr[..., 0] = (gv & _M32)[:, None]
    ctr[..., 1] = (gv >> np.uint64(32))[:, None]
    ctr[..., 2] = np.uint64(int(step) & 0xFFFFFFFF)
    ctr[..., 3] = np.arange(quads, dtype=np.uint64)[None, :]
    w = philox4x32_10(ctr, seed64 & 0xFFFFFFFF, seed64 >> 32)
    u = ((w.astype(np.float32) + np.float32(0.5)) * np.float32(2.3283064365386963e-10)).astype(np.float64)
    out = np.empty((N * vox, quads, 4))
    for j in (0, 2):
        rad = np.sqrt(-2.0 * np.log(u[..., j]))
        out[..., j] = rad * np.cos(2 * np.pi * u[..., j + 1])
        out[..., j + 1] = rad * np.sin(2 * np.pi * u[..., j + 1])
    return out.reshape(N, vox, 4 * quads)


# ---- the grid of the persistent forms ---------------------------------------------------------------------------------------
def tile_walk(vox, N, wgs_per_cu, cus):
    """As tail_entry sizes the MFMA forms (csrc/sampler.hip tail_grid): g = min(tiles, wgs_per_cu * CUs // N) workgroups per
    sample, workgroup b walks tiles b, b + g, ... -> dict(tiles, g, walks = (most, fewest) tiles per workgroup, last = voxels of
    the last tile)."""
    tiles = -(-vox // 256)
    g = max(min(tiles, wgs_per_cu * cus // N), 1)
    return dict(tiles=tiles, g=g, walks=(-(-tiles // g), tiles // g), last=vox - (tiles - 1) * 256)


# ---- shared inputs ----------------------------------------------------------------------------------------------------------
# form: "plain" (<KS,false,false>), "extra" (<KS,false,true>), "res" (<KS,true>), "valu", "identity" (MFMA, norm = None)
# T16: (steps of the schedule, t) per sample for N = 16: t in {0, 1, 500, 998, 999} of the 1000-step schedule, all ten rows of
# the 10-step one, + one more interior row; T3 for N = 3.  Both start with a t = 0 row.
T16 = [(1000, 0), (1000, 1), (1000, 500), (1000, 998), (1000, 999)] + [(10, t) for t in range(10)] + [(1000, 250)]
T3 = [(1000, 0), (10, 7), (1000, 500)]
CASES = {
    "a": dict(form="plain", dtype=F16, K=64, C=16, N=16, dims=(23, 29, 41), xin_pad=8, wgs=3, walks=(3, 2), tiles=107, g=48, last=211),
    "b": dict(form="extra", dtype=F16, K=64, C=16, N=16, dims=(23, 29, 41), xin_pad=8, wgs=3, walks=(3, 2), tiles=107, g=48, last=211),
    "c1": dict(form="extra", dtype=F16, K=32, C=13, N=16, dims=(19, 24, 31), xin_pad=8, wgs=3, walks=(2, 1), tiles=56, g=48, last=56),
    "c4": dict(form="extra", dtype=F16, K=128, C=9, N=16, dims=(19, 24, 31), xin_pad=8, wgs=3, walks=(2, 1), tiles=56, g=48, last=56),
    "d1": dict(form="res", dtype=F16, K=32, kvalid=24, C=16, N=16, dims=(19, 24, 31), xin_pad=8, wgs=2, walks=(2, 1), tiles=56, g=32, last=56, slope=0.01),
    "d2": dict(form="res", dtype=F16, K=64, kvalid=48, C=16, N=16, dims=(19, 24, 31), xin_pad=8, wgs=2, walks=(2, 1), tiles=56, g=32, last=56, slope=0.01),
    "e32-3-8": dict(form="valu", dtype=F32, K=8, C=3, N=3, dims=(5, 7, 37), xin_pad=8),
    "e32-16-24": dict(form="valu", dtype=F32, K=24, C=16, N=3, dims=(5, 7, 37), xin_pad=8),
    "e32-20-64": dict(form="valu", dtype=F32, K=64, C=20, N=3, dims=(5, 7, 37), xin_pad=8),
    "e32-29-136": dict(form="valu", dtype=F32, K=136, C=29, N=3, dims=(5, 7, 37), xin_pad=8),
    "e16-16-24": dict(form="valu", dtype=F16, K=24, C=16, N=3, dims=(5, 7, 37), xin_pad=8),
    "e16-20-64": dict(form="valu", dtype=F16, K=64, C=20, N=3, dims=(5, 7, 37), xin_pad=8),
    "f": dict(form="identity", dtype=F16, K=64, C=16, N=3, dims=(5, 7, 37), xin_pad=8),
}
SEED64, STEP = 0x1234ABCD0BADF00D, 7          # Philox key with a non-zero high word, step word


def state_stride(C):
    return -(-C // 8) * 8


def coef_rows(ts, mode, eta=0.3, masked=True):
    """fp32 [N, 8] rows of (steps, t) pairs through the package's own tables; ``masked=False``: without the 1[t != 0] factor (the
    planted defect of the host test)."""
    from diff_unet_amos_amd.gaussian_diffusion import make_spaced
    rows = []
    for steps, t in ts:
        d = _sched(steps, make_spaced)
        tt = torch.tensor([t])
        if masked or t != 0:
            rows.append(d.ddpm_coef(tt)[0] if mode == DDPM else d.ddim_coef(tt, eta)[0])
        else:                                      # what the row would hold without the mask
            r = torch.zeros(8)
            if mode == DDPM:
                r[:3] = d.ddpm_coef(tt)[0, :3]
                r[2] = torch.exp(0.5 * d._look(d._model_log_variance, tt))[0]
            else:
                r[:5] = d.ddim_coef(tt, eta)[0, :5]
                r[4] = 0.25                         # sigma(t = 0) is 0 in the tables themselves: any non-zero weight
            rows.append(r)
    return torch.stack(rows).float().contiguous()


_SCHED = {}


def _sched(steps, make_spaced):
    if steps not in _SCHED:
        _SCHED[steps] = make_spaced(1000, [steps])
    return _SCHED[steps]


def _lrelu(t, slope):
    return torch.where(t > 0, t, t * slope)


def build_case(name, vox=None):
    """Seeded CPU inputs of case ``name`` ([N, vox, .] rows; ``vox``: a reduced voxel count for the host test): raw (+ res, ra_src)
    in the case's type with per-channel means and scales away from (0, 1), gamma / beta away from (1, 0), wf scaled so that the
    logits have standard deviation about 1 (from the normalised model of the inputs, not from any kernel), bf, the state, an
    injected noise field, a starting xsum."""
    c = dict(CASES[name])
    c["name"] = name
    N, K, C, dt = c["N"], c["K"], c["C"], c["dtype"]
    V = vox or c["dims"][0] * c["dims"][1] * c["dims"][2]
    c["vox"] = V
    kv = c.get("kvalid", K)
    slope = c.setdefault("slope", R.SLOPE if c["form"] != "identity" else 1.0)
    g = torch.Generator().manual_seed(1000 + sorted(CASES).index(name))
    mu, sg = torch.randn(kv, generator=g), 0.5 + torch.rand(kv, generator=g)
    c["raw"] = (torch.randn(N, V, kv, generator=g) * sg + mu).to(dt)
    c["gamma"] = 1.0 + 0.3 * torch.randn(kv, generator=g)
    c["beta"] = 0.3 * torch.randn(kv, generator=g)
    z = torch.randn(4096, kv, generator=g, dtype=F64)
    if c["form"] == "identity":
        c["raw"] = (torch.randn(N, V, K, generator=g) * 0.8).to(dt)
        model = z * 0.8
    elif c["form"] == "res":
        c["res"] = (torch.randn(N, V, kv, generator=g) * 2 + 0.5).to(dt)
        c["rgamma"] = 1.0 + 0.3 * torch.randn(kv, generator=g)
        c["rbeta"] = 0.3 * torch.randn(kv, generator=g)
        c["ra_off"] = 8
        c["ra_src"] = torch.randn(N, V, kv + 16, generator=g).to(dt)
        z2, z3 = torch.randn(4096, kv, generator=g, dtype=F64), torch.randn(4096, kv, generator=g, dtype=F64)
        model = _lrelu(z * c["gamma"].double() + c["beta"].double() + z2 * c["rgamma"].double() + c["rbeta"].double(), slope)
        model = model + z3 * (1 - torch.sigmoid(z3))
    else:
        model = _lrelu(z * c["gamma"].double() + c["beta"].double(), slope)
    w = torch.randn(C, K, generator=g)                     # the padding columns of the residual form stay non-zero
    c["bf"] = 0.1 * torch.randn(C, generator=g)
    std = (model @ w[:, :kv].double().t()).std(0).mean()
    c["wf"] = (w / float(std)).contiguous()
    cx = c["cx"] = state_stride(C)
    c["xt"] = torch.randn(N, V, cx, generator=g)
    c["noise"] = torch.randn(N, V, C, generator=g)
    c["xsum0"] = torch.randn(N, V, cx, generator=g)
    c["ts"] = T16 if N == 16 else T3
    return c


def host_constants(raw, gamma, beta):
    """fp32 scale, shift [N, C] from float64 sums of the stored values (the host test's stand-in for ops.instnorm_finalize)."""
    v = raw.double()
    sums = torch.stack([v.sum(1), (v * v).sum(1)], -1)
    sc, sh, _, _ = R.finalize(sums, gamma, beta, raw.shape[1])
    return sc.float(), sh.float()


def _rows(per_sample, V):
    """[N, C] per-sample constants -> [N * V, C] per-row"""
    return per_sample.repeat_interleave(V, 0)


def case_reference(c, consts, mode, eps, logits_only=False, head=None):
    """The whole fp64 reference of one launch of case ``c``.  consts = (sc, sh) or (sc, sh, rsc, rsh) fp32 [N, .]; eps float64
    [N, V, >= C] (the field the kernel used); mode DDPM / DDIM.  Returns dict of float64 [N, V, C] tensors: L, bL, and unless
    ``logits_only``: x0, xn, b0, bn, xsum, bs.  ``head``: the dict of an earlier call on the same operands (L and bL are reused:
    computed once, shared, left unchanged)."""
    N, V, K, C = c["N"], c["vox"], c["K"], c["C"]
    kv = c.get("kvalid", K)
    flat = lambda t: t.double().reshape(N * V, -1)
    form = c["form"]
    if head is not None:
        return _with_update(c, dict(L=head["L"], bL=head["bL"]), mode, eps)
    residual = None
    if form == "res":
        off = c["ra_off"]
        ra = flat(c["ra_src"])[:, off:off + kv] if c.get("use_ra", True) else None
        residual = dict(res=flat(c["res"]), rsc=_rows(consts[2], V), rsh=_rows(consts[3], V), ra=ra, kvalid=kv)
    sc = sh = None
    if form != "identity":
        sc, sh = _rows(consts[0], V), _rows(consts[1], V)
    L, ab, sq, aerr = tail_logits_ref(flat(c["raw"]), sc, sh, c["wf"], c["bf"], c["slope"], identity=form == "identity",
                                      residual=residual)
    mfma = form != "valu"
    bL = tail_logits_bound(L, ab, sq, K, split=mfma, emulated=form in ("plain", "extra", "valu"), act_err=aerr)
    out = dict(L=L.view(N, V, C), bL=bL.view(N, V, C))
    return out if logits_only else _with_update(c, out, mode, eps)


def _with_update(c, out, mode, eps):
    C = c["C"]
    k = coef_rows(c["ts"], mode)[:, None, None, :]
    xt = c["xt"][..., :C].double()
    x0, xn, b0, bn = update_ref(mode, k, out["L"], xt, eps[..., :C].double(), out["bL"])
    s, bs = xsum_ref(c["xsum0"][..., :C].double(), x0, out["bL"])
    out.update(x0=x0, xn=xn, b0=b0, bn=bn, xsum=s, bs=bs)
    return out


def input_conditions(L):
    """(share of logits inside (-1, 1), share below -1, share above 1) of an fp64 reference"""
    n = L.numel()
    return (float(((L > -1) & (L < 1)).sum()) / n, float((L <= -1).sum()) / n, float((L >= 1).sum()) / n)


# ---- the kernel's own arithmetic, in torch fp32 -----------------------------------------------------------------------------
MUTATIONS = ("drop_aw_yl", "drop_awl_y", "act_fp16_only", "skip_clamp", "swap_k2_k3", "neighbour_row", "eps_next_quad",
             "eps_next_tile", "xsum_unclamped", "ignore_t0_mask")
SPLIT_MUTATIONS = MUTATIONS[:3]                      # meaningful for the MFMA forms only


def _fma32(a, b, c):
    """fmaf on fp32 tensors: the float64 product of two fp32 values is exact, one rounding of the sum to float64 below fp32's"""
    return (a.double() * b.double() + c.double()).float()


def emulate_tail(c, consts, mode, eps, mutate=None):
    """fp32 [N, V, C] outputs (L, x0, xn, xsum) of final_conv_sampler on case ``c`` as the kernel computes them (module docstring);
    eps fp32 [N, V, >= C].  ``mutate``: one of MUTATIONS."""
    assert mutate is None or mutate in MUTATIONS
    N, V, K, C = c["N"], c["vox"], c["K"], c["C"]
    kv = c.get("kvalid", K)
    form, slope = c["form"], np.float32(c["slope"])
    one = torch.ones((), dtype=F32)
    flat = lambda t: t.float().reshape(N * V, -1)
    raw = flat(c["raw"])
    if form == "identity":
        t = raw
    else:
        t = _fma32(raw[:, :kv], _rows(consts[0], V), _rows(consts[1], V))
        if form == "res":
            t = t + _fma32(flat(c["res"])[:, :kv], _rows(consts[2], V), _rows(consts[3], V))
        t = torch.where(t > 0, t, t * slope)
        if form == "res" and c.get("use_ra", True):
            s = flat(c["ra_src"])[:, c["ra_off"]:c["ra_off"] + kv]
            t = t + s * (one - one / (one + torch.exp(-s)))
    wf, bf = c["wf"].float(), c["bf"].float()
    if form == "valu":
        acc = bf[None].expand(N * V, C).contiguous()
        for k in range(K):
            acc = _fma32(t[:, k:k + 1], wf[None, :, k], acc)
    else:
        if kv < K:                                       # padding channels: exact zeros
            t = torch.cat([t, torch.zeros(N * V, K - kv)], 1)
        y = t.half()
        yl = (t - y.float()).half()
        aw = wf.half()
        awl = (wf - aw.float()).half()
        if mutate == "act_fp16_only":
            yl = torch.zeros_like(yl)
        acc = bf[None].expand(N * V, C).contiguous()
        for ks in range(K // 32):
            sl = slice(32 * ks, 32 * ks + 32)
            mm = lambda a, w: a[:, sl].double() @ w[:, sl].double().t()      # 32 exact products, summed far below fp32's rounding
            if mutate != "drop_awl_y":
                acc = (acc.double() + mm(y, awl)).float()
            if mutate != "drop_aw_yl":
                acc = (acc.double() + mm(yl, aw)).float()
            acc = (acc.double() + mm(y, aw)).float()
    L = acc.view(N, V, C)
    k = coef_rows(c["ts"], mode, masked=mutate != "ignore_t0_mask")[:, None, :]          # [N, 1, 8]
    nz = 2 if mode == DDPM else 4
    if mutate == "swap_k2_k3":
        k = k.clone()
        k[..., [2, 3]] = k[..., [3, 2]]
    kn = k[..., nz:nz + 1]
    if mutate == "neighbour_row":
        kn = torch.roll(kn, -1, 0)
    e = eps.float()
    if mutate == "eps_next_quad":
        e = torch.roll(e, -4, 2)
    if mutate == "eps_next_tile":
        e = torch.roll(e, -256, 1)
    e = e[..., :C]
    xt = c["xt"][..., :C].float()
    xs = L if mutate == "skip_clamp" else L.clamp(-1, 1)
    if mode == DDPM:
        xn = (k[..., 0:1] * xs + k[..., 1:2] * xt) + kn * e
    else:
        ee = (k[..., 0:1] * xt - xs) / k[..., 1:2]
        xn = (xs * k[..., 2:3] + k[..., 3:4] * ee) + kn * e
    xsum = c["xsum0"][..., :C].float() + (L if mutate == "xsum_unclamped" else xs)
    return dict(L=L, x0=xs, xn=xn, xsum=xsum)


def worst_ratio(got, ref):
    """max err / bound over the outputs of ``emulate_tail`` / a launch against ``case_reference`` -> (ratio, which output)"""
    best = (0.0, "")
    for key, rk, bk in (("L", "L", "bL"), ("x0", "x0", "b0"), ("xn", "xn", "bn"), ("xsum", "xsum", "bs")):
        if key in got and rk in ref:
            r = R.check(got[key], ref[rk], ref[bk])
            if not r.ratio <= best[0]:
                best = (r.ratio, f"{key} {r}")
    return best
