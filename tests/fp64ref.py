"""fp64 references of the denoiser's forward kernels at sampled output voxels, and per-element error bounds.

A plain helper module of the suite (imported as ``from fp64ref import ...``).  The references are evaluated on the EXACT
operands a kernel read: activations gathered from its input buffer, weights rounded to fp16 the way the packer rounds them (or
decoded from the packed buffer), a fused input transform emulated in the kernel's own arithmetic.  The only legitimate
differences left are then the kernel's fp32 accumulation and the rounding of what it stores, which ``bound`` turns into a
per-element limit derived from the arithmetic (not calibrated on measurements):

    |got - ref| <= 2^-24 * n_chain * sum_k |a_k w_k|          fp32 accumulation
                 + u_out * |ref| + floor_out                     rounding of the stored value
                 + c_rss * u_in * sqrt(sum_k (a_k w_k)^2)       1-ulp differences of emulated inputs (fused transforms only)
                 + extra                                        terms a caller derives for its own operand (bias table, tail split)

* Accumulation: a sum formed as a chain of n fp32 additions (each operand exact: fp16 x fp16 products fit fp32) is off by at
  most (n - 1) 2^-24 sum |terms| (recursive summation, first order).  An MFMA adds k products into its accumulator per step
  (k = 16 / 32 for fp16): n_chain = ceil(K / k) + log2(k) for the adds inside the instruction, + 1 for the bias, + the number
  of split-K partials that a finish kernel adds up.  The fp32 kernels chain one fmaf per product: n_chain = K + 1.
* Output: round-to-nearest into fp16 moves a value by at most 2^-11 of itself (2^-24 for fp32) above the normal range, and by
  half the smallest subnormal (2^-25 / 2^-150) below it.
* Emulated inputs: the emulation rounds the transform once from float64 where the kernel rounds fp32 intermediates (a fused
  multiply-add contracted or not): once in a while an input lands one fp16 ulp (2 * 2^-11
  relative) away.  If every input did so with random signs the sum would move by 2^-10 sqrt(sum (a w)^2); c_rss = 2 at
  u_in = 2^-11 covers that, far more than the rare flips need.  fp32 plans: the same form with u_in = 2^-24.

* fp16 operands below the normal range (``nominal=``, MFMA kernels only).  The accumulation rule above rests on a premise about the
  matrix instruction that tests/test_mfma_model_gpu.py now holds on the instruction itself, against exact integer arithmetic
  (tests/mfma_model.py has the model and the sweeps).  Measured on an MI355X, v_mfma_f32_32x32x16_f16 and v_mfma_f32_16x16x32_f16
  alike: the instruction is a chain of K / 8 steps, acc <- fp32(acc + 8 products); inside a step the nine terms are aligned by
  EXPONENT FIELD to the largest one, and a bit arrives exactly down to 24 places below that nominal exponent, not 25 -- for a small
  product normal x normal, normal x subnormal and subnormal x subnormal, next to a large product, a large accumulator, or a large
  product with a one-ulp subnormal factor (24 in each of these 3 x 4 x 2 classes; 23 where the running sum is rounded to fp32
  between two steps, which is the chain's own rounding).  MFMA_W = 23 is one less than the smallest alignment width found.
  A subnormal has the exponent field of 2^-14 whatever its value: nm(x) = 2^max(floor(log2 |x|), -14) (0 for 0).  A step whose
  largest nominal exponent e_g belongs to a product with a subnormal factor drops less than 2^(e_g - W) from each of the OTHER
  eight terms (the product that sets e_g has no bit below 2^(e_g - 20)), and 2^e_g = nm(a) nm(b) of that product.  Summed over the
  steps of an element's chain, whichever kernel runs them:
      MFMA_LOSSY * 2^-MFMA_W * sum over the products k with a subnormal factor of nm(a_k) nm(b_k)          (``nominal_sum``)
  A step whose largest term is a product of normal operands or the accumulator aligns as it does without subnormals, which is what
  the accumulation term is held to on every case; with no subnormal operand in a contraction the sum is empty and the bound is
  bit for bit the one above.  Nothing in it comes from a kernel's output.

``check(got, ref, bound)`` reports max(|err| / bound) and the worst element.
"""
from __future__ import annotations

import itertools
import math

import numpy as np
import torch

U16, U32 = 2.0 ** -11, 2.0 ** -24            # unit roundoff (half an ulp, relative)
FLOOR16, FLOOR32 = 2.0 ** -25, 2.0 ** -150   # half the smallest subnormal
C_RSS = 2.0
SLOPE = 0.1


def unit(dtype):
    return (U16, FLOOR16) if dtype == torch.float16 else (U32, FLOOR32)


def chain_length(K, dtype, split_parts=0):
    """Longest fp32 accumulation chain of a K-term contraction (module docstring)."""
    if dtype == torch.float16:
        return -(-K // 16) + 4 + 1 + split_parts
    return K + 1 + split_parts


MFMA_W = 23
"""Alignment width of the fp16 matrix instructions, in places below the largest nominal exponent of a step, less one guard bit.
Measured 24 on an MI355X (gfx950) with dua_mfma_single against exact integer sums, for v_mfma_f32_32x32x16_f16 and
v_mfma_f32_16x16x32_f16, small product nn / ns / ss, large term a product, the accumulator, a product with a subnormal factor, at
every k index (tests/test_mfma_model_gpu.py prints the table and fails if a width below MFMA_W + 1 turns up)."""
MFMA_LOSSY = 8
"""Terms of one step (8 products + the accumulator) that can lose bits to the alignment: all but the one that sets it."""


def nm16(x, ulp_off=False):
    """(nominal magnitude 2^max(floor(log2 |x|), -14) with 0 for 0, is-subnormal mask) of exact fp16 values held in any float type.
    ``ulp_off``: the kernel's operand may lie one fp16 ulp from x (an emulated input): the magnitude of the next binade, and 2^-14
    itself counts as subnormal."""
    a = x.double().abs()
    e = torch.frexp(a)[1] - 1
    nm = torch.where(a > 0, torch.exp2(e.clamp_min(-14).double()), torch.zeros_like(a))
    if ulp_off:
        return 2 * nm, (a > 0) & (a <= 2.0 ** -14)
    return nm, (a > 0) & (a < 2.0 ** -14)


def nominal_sum(A, Wm, ulp_off=False):
    """A [P, K], Wm [K, O] (exact fp16 values) -> sum over the k where a_k or w_k is subnormal of nm(a_k) nm(w_k), [P, O]: gathered
    like ``contract``'s sum of |terms|, exactly zero where no operand of the contraction is subnormal.  ``ulp_off``: for A (nm16)."""
    (na, sa), (nw, sw) = nm16(A, ulp_off), nm16(Wm)
    return (na * sa) @ nw + (na * ~sa) @ (nw * sw)


SUBNORMAL_REGIMES = ("straddle", "subnormal", "ulps")
_LOG_UNIFORM = {"straddle": (-24.0, -10.0), "subnormal": (-24.0, -14.0), "decayed": (-20.0, -8.0)}


def subnormal_regime(shape, regime, seed, device="cpu"):
    """An fp16 operand in one of the regimes a step at a low loss scale produces, and the share of its elements that are subnormal
    by construction.  Gradients: "straddle" magnitudes log-uniform in [2^-24, 2^-10] (10 of 14 octaves below 2^-14), "subnormal"
    log-uniform in [2^-24, 2^-14) (all), "ulps" uniform in {0, +-1, +-2, +-3} x 2^-24 (6 of 7; the rest zero).  Weights: "decayed"
    log-uniform in [2^-20, 2^-8] (6 of 12 octaves).  Random signs."""
    g = torch.Generator().manual_seed(seed)
    if regime == "ulps":
        return (torch.randint(-3, 4, shape, generator=g).double() * 2.0 ** -24).half().to(device), 6 / 7
    lo, hi = _LOG_UNIFORM[regime]
    mag = torch.exp2(lo + (hi - lo) * torch.rand(shape, generator=g, dtype=torch.float64))
    if regime == "subnormal":
        mag = mag.clamp_max(2.0 ** -14 - 2.0 ** -24)                     # the largest subnormal: nothing rounds up to 2^-14
    sign = torch.randint(0, 2, shape, generator=g).double() * 2 - 1
    return _f16_rne(mag * sign).half().to(device), (-14.0 - lo) / (hi - lo)


def subnormal_share(t):
    """share of the elements of an fp16 tensor that are subnormal (non-zero, below 2^-14)"""
    return float(((t != 0) & (t.abs().double() < 2.0 ** -14)).double().mean())


def subnormal_term(nominal):
    """The bound's term for fp16 operands below the normal range (module docstring); ``nominal``: nominal_sum of the contraction."""
    return MFMA_LOSSY * 2.0 ** -MFMA_W * nominal


def bound(ref, abs_sum, sq_sum, n_chain, dtype_out, emulated_in=None, extra=0.0, nominal=None):
    """Per-element bound (float64, the shape of ``ref``); ``emulated_in``: dtype of emulated inputs or None; ``nominal``: the
    contraction's nominal_sum (fp16 MFMA kernels whose operands may be subnormal) or None."""
    u_out, floor = unit(dtype_out)
    b = U32 * n_chain * abs_sum * (1 + u_out) + u_out * ref.abs() + floor
    if emulated_in is not None:
        b = b + C_RSS * unit(emulated_in)[0] * sq_sum.sqrt()
    b = b + extra
    return b if nominal is None else b + subnormal_term(nominal) * (1 + u_out)


class CheckResult:
    def __init__(self, ratio, where, got, ref, bnd):
        self.ratio, self.where, self.got, self.ref, self.bound = ratio, where, got, ref, bnd

    def __repr__(self):
        return (f"max |err|/bound = {self.ratio:.3g} at {self.where}: got {self.got:.6g}, ref {self.ref:.6g}, "
                f"bound {self.bound:.3g}")


def check(got, ref, bnd, coords=None):
    """max(|got - ref| / bound) and the worst element (index tuple, or ``coords[row]`` + column for 2-D results).  A non-finite
    value counts as infinitely far off."""
    got, ref, bnd = got.double(), ref.double(), bnd.double()
    err = (got - ref).abs()
    r = err / bnd
    r = torch.where(torch.isfinite(r), r, torch.full_like(r, math.inf))
    k = int(torch.argmax(r))
    idx = tuple(int(i) for i in np.unravel_index(k, tuple(r.shape)))
    where = idx if coords is None else (tuple(int(v) for v in coords[idx[0]]), *idx[1:])
    return CheckResult(float(r.view(-1)[k]), where, float(got.view(-1)[k]), float(ref.view(-1)[k]), float(bnd.view(-1)[k]))


# ---- which voxels ------------------------------------------------------------------------------------------------------------
def _boundary_coords(S):
    """Coordinates of one axis on 8-voxel tile edges (0, 7 mod 8) and 4-plane slab edges (3, 4 mod 8), plus the last plane."""
    return sorted({c for c in range(S) if c % 8 in (0, 3, 4, 7)} | {S - 1})


def sample_voxels(N, dims, n_random=2000, seed=0):
    """int64 [P, 4] (n, d, h, w), unique and sorted: the 8 corners, points on every face and edge, a lattice through tile and
    slab boundaries (every combination near both ends of every axis, a seeded subset of the interior), ~n_random seeded random
    voxels; every sample index gets the structured points, the random ones are spread over the samples."""
    g = np.random.default_rng(seed)
    D, H, W = dims
    axes = [_boundary_coords(S) for S in dims]
    ends = [[c for c in a if c < 9 or c >= S - 9] for a, S in zip(axes, dims)]
    pts = set()
    for n in range(N):
        for corner in itertools.product(*[(0, S - 1) for S in dims]):
            pts.add((n, *corner))
        # edges: two coordinates at an end, the third along the axis; faces: one at an end, two along it
        for ax in range(3):
            others = [a for a in range(3) if a != ax]
            for e0, e1 in itertools.product((0, 1), repeat=2):
                for c in g.choice(axes[ax], size=min(6, len(axes[ax])), replace=False):
                    p = [0, 0, 0]
                    p[ax] = int(c)
                    p[others[0]] = 0 if e0 == 0 else dims[others[0]] - 1
                    p[others[1]] = 0 if e1 == 0 else dims[others[1]] - 1
                    pts.add((n, *p))
            for end in (0, dims[ax] - 1):
                for _ in range(12):
                    p = [0, 0, 0]
                    p[ax] = end
                    for o in others:
                        p[o] = int(g.choice(axes[o]))
                    pts.add((n, *p))
        for p in itertools.product(*ends):
            pts.add((n, *p))
        for _ in range(600):
            pts.add((n, *(int(g.choice(a)) for a in axes)))
    for _ in range(n_random):
        pts.add((int(g.integers(N)), int(g.integers(D)), int(g.integers(H)), int(g.integers(W))))
    return torch.tensor(sorted(pts), dtype=torch.int64)


TAPS = torch.tensor(list(itertools.product((-1, 0, 1), repeat=3)), dtype=torch.int64)     # tap t = (kd * 3 + kh) * 3 + kw


def gather_taps(x, pts, c_off, cin):
    """x: channels-last [N, D, H, W, Cs] (any device, channels-last rows); pts [P, 4] -> float64 CPU [P, 27, cin] of the 3x3x3
    neighbourhoods with zero padding, plus the in-volume mask [P, 27].  Gathered on x's device, only the samples move."""
    N, D, H, W, _ = x.shape
    p = pts.to(x.device)
    c = p[:, None, 1:] + TAPS.to(x.device)[None]
    ok = ((c >= 0) & (c < torch.tensor([D, H, W], device=x.device))).all(-1)
    cc = torch.where(ok[..., None], c, torch.zeros_like(c))
    v = x[p[:, None, 0].expand_as(ok), cc[..., 0], cc[..., 1], cc[..., 2], c_off:c_off + cin]
    v = torch.where(ok[..., None], v, torch.zeros_like(v))
    return v.cpu().double(), ok.cpu()


def gather_points(x, pts, c_off, cin):
    """channels-last x at pts -> float64 CPU [P, cin]"""
    p = pts.to(x.device)
    return x[p[:, 0], p[:, 1], p[:, 2], p[:, 3], c_off:c_off + cin].cpu().double()


# ---- the fused input transform, in the kernel's arithmetic ------------------------------------------------------------------
def finalize(sums, gamma, beta, count, eps=1e-5):
    """InstanceNorm scale = gamma / sqrt(var + eps), shift = beta - mean * scale in float64 from the decoded statistics words
    (float64 [N, c_pad, 2]), [N, C] each, and the per-element bounds on how far the consumers' fp32 preamble may land from
    them: 1 / sqrt(var + eps) rounded to fp32, the gamma product (scale: 2 roundings, with double-precision error far below);
    the mean rounded to fp32, its product with the fp32 scale, the subtraction from beta (shift: the product's and the scale's
    roundings carry |mean * scale|, the subtraction |shift|).  The transforms are then emulated on the kernel's own fp32
    constants (ops.instnorm_finalize), which these bounds hold to fp64."""
    C = gamma.numel()
    S, Q = sums[:, :C, 0].double(), sums[:, :C, 1].double()
    mean = S / count
    var = (Q / count - mean * mean).clamp_min(0)
    sc = gamma.double()[None] / torch.sqrt(var + float(np.float32(eps)))
    sh = beta.double()[None] - mean * sc
    b_sc = 3 * U32 * sc.abs() + 1e-300
    b_sh = U32 * (6 * (mean * sc).abs() + sh.abs()) + 1e-300
    return sc, sh, b_sc, b_sh


def _f16_rne(v):
    """float64 -> fp16 with one round-to-nearest-even (numpy converts directly; torch goes through fp32)."""
    return torch.from_numpy(v.numpy().astype(np.float16).astype(np.float64))


def transform(raw, sc, sh, add, dtype, slope=SLOPE):
    """LeakyReLU(raw * sc + sh) + add for raw float64 [..., C] (exact values of the stored operands) with per-channel fp32 sc,
    sh, add broadcast to it.  fp16: max(fp16(raw * sc + (sh + add)), fp16(raw * (slope sc) + fma(slope, sh, add))) -- the
    kernels' two mixed-precision fma and a max (csrc/common.hpp xform_frag_mix); fp32: fmaf, the slope, the add, in fp32.
    Returns float64 values of the kernel's operand type."""
    sc, sh, add = sc.double(), sh.double(), add.double()
    if dtype == torch.float16:
        b = (sh + add).float().double()
        sn = (np.float32(slope) * sc.float()).double()
        an = (np.float32(slope) * sh + add).float().double()
        return torch.maximum(_f16_rne(raw * sc + b), _f16_rne(raw * sn + an))
    y = (raw * sc + sh).float()
    y = torch.where(y > 0, y, y * np.float32(slope))
    return (y + add.float()).double()


def tail_transform(raw, sc, sh, slope=SLOPE):
    """The 1x1x1 head's input: LeakyReLU(fmaf(raw, sc, sh)) in fp32, not rounded further (csrc/sampler.hip)."""
    y = (raw * sc.double() + sh.double()).float()
    return torch.where(y > 0, y, y * np.float32(slope)).double()


# ---- references ----------------------------------------------------------------------------------------------------------
def contract(A, Wm):
    """A [P, K], Wm [K, O] (float64) -> (sum a w, sum |a w|, sum (a w)^2), each [P, O]."""
    return A @ Wm, A.abs() @ Wm.abs(), (A * A) @ (Wm * Wm)


def conv3_weights(w, dtype):
    """nn.Conv3d weight [Cout, Cin, 3, 3, 3] -> float64 [27 * Cin, Cout] in gather_taps order, rounded as the packer rounds."""
    wq = w.detach().float().cpu()
    if dtype == torch.float16:
        wq = wq.half()
    Cout, Cin = w.shape[:2]
    return wq.double().reshape(Cout, Cin, 27).permute(2, 1, 0).reshape(27 * Cin, Cout)


def conv3_ref(A, Wm, bias):
    """A [P, 27, Cin] (the activation the kernel multiplies: zero outside the volume) -> (ref, abs_sum, sq_sum) [P, Cout];
    the bias counts as one more term of the chain."""
    ref, ab, sq = contract(A.reshape(A.shape[0], -1), Wm)
    b = bias.detach().double().cpu()[None]
    return ref + b, ab + b.abs(), sq


def conv3_dense_ref(x, cin, Wm, bias=None, nominal=False):
    """conv3_ref at EVERY voxel, on x's device: x channels-last [N, D, H, W, >= cin] (its first cin channels, zero padding), Wm
    from conv3_weights -> (ref, sum |terms|, sum terms^2[, nominal_sum]) as float64 [N, D, H, W, Cout], 27 shifted GEMMs."""
    N, D, H, W, _ = x.shape
    xp = torch.zeros((N, D + 2, H + 2, W + 2, cin), dtype=torch.float64, device=x.device)
    xp[:, 1:-1, 1:-1, 1:-1] = x[..., :cin].double()
    Wd = Wm.to(x.device)
    outs = [torch.zeros((N * D * H * W, Wd.shape[1]), dtype=torch.float64, device=x.device) for _ in range(4 if nominal else 3)]
    if nominal:
        nw, sw = nm16(Wd)
    for t, (kd, kh, kw) in enumerate(itertools.product(range(3), repeat=3)):
        a, w = xp[:, kd:kd + D, kh:kh + H, kw:kw + W].reshape(-1, cin), Wd[t * cin:(t + 1) * cin]
        outs[0] += a @ w
        outs[1] += a.abs() @ w.abs()
        outs[2] += (a * a) @ (w * w)
        if nominal:
            na, sa = nm16(a)
            nt, st = nw[t * cin:(t + 1) * cin], sw[t * cin:(t + 1) * cin]
            outs[3] += (na * sa) @ nt + (na * ~sa) @ (nt * st)
    if bias is not None:
        b = bias.detach().double().to(x.device)[None]
        outs[0] += b
        outs[1] += b.abs()
    return tuple(o.reshape(N, D, H, W, -1) for o in outs)


def deconv_ref(A, w, bias, dtype, child):
    """ConvTranspose3d(k2, s2) at sampled output voxels: A [P, Cin] = the activation at each voxel's parent, ``child`` [P] =
    (d & 1) * 4 + (h & 1) * 2 + (w & 1); w [Cin, Cout, 2, 2, 2]."""
    wq = w.detach().float().cpu()
    if dtype == torch.float16:
        wq = wq.half()
    Wc = wq.double().reshape(w.shape[0], w.shape[1], 8)[:, :, child].permute(2, 0, 1)       # [P, Cin, Cout]
    ref = torch.einsum("pc,pco->po", A, Wc)
    ab = torch.einsum("pc,pco->po", A.abs(), Wc.abs())
    sq = torch.einsum("pc,pco->po", A * A, Wc * Wc)
    b = bias.detach().double().cpu()[None]
    return ref + b, ab + b.abs(), sq


def deconv_res_ref(lo, skip, w3, wd, child, up_first=True):
    """dua_deconv_k2s2_res_fwd at sampled fine-grid voxels: conv1x1x1(cat((ConvTranspose3d_k2s2(lo), skip))) without the
    upsampled tensor.  lo [P, Cu] = the coarse activation at each voxel's parent, skip [P, Cs] = the skip half at the voxel
    (float64, exact fp16 values), ``child`` [P] = (d & 1) * 4 + (h & 1) * 2 + (w & 1); w3 [Cout, Cmid + Cs] (``up_first``: the
    upsampled half's columns first), wd [Cu, Cmid, 2, 2, 2].  The composed weights W3_up . Wd[child] are formed in fp32 and
    rounded once to fp16 as ops.pack_deconv_res_weights forms them (a one-ulp flip of a weight whose fp32 composition sums in
    another order is what the caller's ``emulated_in`` term of ``bound`` covers), the skip weights are rounded to fp16.
    Returns (ref, sum |terms|, sum terms^2), each [P, Cout]; the chain is ``chain_length(Cu + Cs, fp16)``."""
    w3, wd = w3.detach().float().cpu(), wd.detach().float().cpu()
    Cu, Cmid = wd.shape[:2]
    Cs = w3.shape[1] - Cmid
    w3_up, w3_sk = (w3[:, :Cmid], w3[:, Cmid:]) if up_first else (w3[:, Cs:], w3[:, :Cs])
    comp = torch.einsum("umk,om->uok", wd.reshape(Cu, Cmid, 8), w3_up).half().double()          # [Cu, Cout, 8]
    wsk = w3_sk.half().double().t()                                                              # [Cs, Cout]
    Wc = comp[:, :, child].permute(2, 0, 1)                                                      # [P, Cu, Cout]
    ref = torch.einsum("pc,pco->po", lo, Wc) + skip @ wsk
    ab = torch.einsum("pc,pco->po", lo.abs(), Wc.abs()) + skip.abs() @ wsk.abs()
    sq = torch.einsum("pc,pco->po", lo ** 2, Wc ** 2) + skip ** 2 @ wsk ** 2
    return ref, ab, sq


def replicate_source(pts, coarse_dims):
    """Output voxels of a transposed convolution whose buffer is one plane longer on an odd axis: the replicate-padded plane
    2 * S copies plane 2 * S - 1 (UpCat.forward's pad).  Returns the voxel the value is computed at."""
    lim = torch.tensor([2 * s - 1 for s in coarse_dims], dtype=torch.int64)
    q = pts.clone()
    q[:, 1:] = torch.minimum(q[:, 1:], lim)
    return q


def border_class(pts, dims):
    """(cd * 3 + ch) * 3 + cw per voxel: 0 on the low face of an axis, 2 on the high face, 1 inside (the fold's bias table)."""
    cls = torch.zeros(pts.shape[0], dtype=torch.int64)
    for a, S in enumerate(dims):
        c = pts[:, 1 + a]
        k = torch.where(c == 0, 0, torch.where(c == S - 1, 2, 1))
        cls = cls * 3 + k
    return cls


def fold_bias_table(wc_up, bc, bd):
    """[27, Cout] float64 bias per border class of the folded up-convolution and the matching sum of |terms|: bc + the
    transposed convolution's bias through every conv tap that stays inside the volume (csrc/upconv.hip)."""
    wc_up = wc_up.detach().double().cpu()
    Cout = wc_up.shape[0]
    bcd = torch.zeros(Cout, dtype=torch.float64) if bc is None else bc.detach().double().cpu()
    bdd = torch.zeros(wc_up.shape[1], dtype=torch.float64) if bd is None else bd.detach().double().cpu()
    rows, arows = [], []
    for cd, ch, cw in itertools.product(range(3), repeat=3):
        v, a = bcd.clone(), bcd.abs()
        for kd, kh, kw in itertools.product(range(3), repeat=3):
            if any((c == 0 and k == 0) or (c == 2 and k == 2) for c, k in ((cd, kd), (ch, kh), (cw, kw))):
                continue
            v = v + wc_up[:, :, kd, kh, kw] @ bdd
            a = a + wc_up[:, :, kd, kh, kw].abs() @ bdd.abs()
        rows.append(v)
        arows.append(a)
    return torch.stack(rows), torch.stack(arows)


def _taps_1d(phi, delta):
    """(conv tap k, deconv child a) pairs of one axis whose input voxel o + k - 1 (o = 2 m + phi) is child a of parent
    m + delta - 1 + phi"""
    return {(0, 0): [(0, 1)], (0, 1): [(1, 0), (2, 1)], (1, 0): [(0, 0), (1, 1)], (1, 1): [(2, 0)]}[(phi, delta)]


def compose_fold(wc_up, wd):
    """W'[(phi, delta)] = sum over taps Wc_up[tap] Wd[child]^T, float64 [Cout, Cu], and the matching sum of |products|."""
    wc_up, wd = wc_up.detach().double().cpu(), wd.detach().double().cpu()
    out = {}
    for phi in itertools.product(range(2), repeat=3):
        for delta in itertools.product(range(2), repeat=3):
            acc = abs_acc = 0
            for (kd, ad), (kh, ah), (kw, aw) in itertools.product(*(_taps_1d(p, d) for p, d in zip(phi, delta))):
                acc = acc + wc_up[:, :, kd, kh, kw] @ wd[:, :, ad, ah, aw].t()
                abs_acc = abs_acc + wc_up[:, :, kd, kh, kw].abs() @ wd[:, :, ad, ah, aw].abs().t()
            out[phi + delta] = (acc, abs_acc)
    return out


def decode_fold_weights(wu, Cout, Cu):
    """The packed composed weights (dua_pack_upconv_weights, streaming order
    [cout tile][pd][ph][g][dd][dh][hcl][pw][dw][q][hh][r][e]) -> {(pd, ph, pw, dd, dh, dw): float64 [Cout, Cu]}."""
    nct, G = -(-Cout // 64), Cu // 64
    t = wu.view(torch.float16).view(nct, 2, 2, G, 2, 2, 4, 2, 2, 2, 2, 32, 8).cpu().double()
    out = {}
    for pd, ph, pw, dd, dh, dw in itertools.product(range(2), repeat=6):
        m = t[:, pd, ph, :, dd, dh, :, pw, dw]                       # [ct][g][hcl][q][hh][r][e]
        m = m.permute(0, 3, 5, 1, 2, 4, 6).reshape(nct * 64, Cu)      # [ct q r] x [g hcl hh e]
        out[(pd, ph, pw, dd, dh, dw)] = m[:Cout]
    return out


def fold_parents(pts, dims):
    """Per output voxel o = 2 m + phi and each delta in {0,1}^3: its coarse parent m + delta - 1 + phi (int64 [P, 8, 3]), the
    in-volume mask [P, 8] and the parity phi [P, 3]."""
    phi = pts[:, 1:] & 1
    m = pts[:, 1:] >> 1
    deltas = torch.tensor(list(itertools.product((0, 1), repeat=3)), dtype=torch.int64)
    par = m[:, None] + deltas[None] - 1 + phi[:, None]
    lim = torch.tensor([S // 2 for S in dims], dtype=torch.int64)
    ok = ((par >= 0) & (par < lim)).all(-1)
    return par, ok, phi, deltas


def fold_ref(A_skip, Wm_skip, U, ok, phi, deltas, Wp, bias_rows, bias_abs):
    """The folded up-convolution: skip half as a 3x3x3 convolution (A_skip [P, 27, Cskip], Wm_skip [27 Cskip, Cout]) + the
    composed weights over the 8 parents (U [P, 8, Cu] activations of the parents, zero outside; Wp from decode_fold_weights)
    + the border-class bias (bias_rows / bias_abs [P, Cout])."""
    ref, ab, sq = contract(A_skip.reshape(A_skip.shape[0], -1), Wm_skip)
    keys = [tuple(p) for p in phi.tolist()]
    for j, dl in enumerate(deltas.tolist()):
        Wj = torch.stack([Wp[k + tuple(dl)] for k in keys])                # [P, Cout, Cu]
        Uj = torch.where(ok[:, j, None], U[:, j], torch.zeros_like(U[:, j]))
        ref = ref + torch.einsum("pc,poc->po", Uj, Wj)
        ab = ab + torch.einsum("pc,poc->po", Uj.abs(), Wj.abs())
        sq = sq + torch.einsum("pc,poc->po", Uj * Uj, Wj * Wj)
    return ref + bias_rows, ab + bias_abs, sq


def materialize_ref(raw, sc, sh, add, emb):
    """LeakyReLU(raw sc + sh) + add (+ emb) in float64 from the fp32 constants, and the sum of |terms| of its four fp32
    operations (fmaf, slope, add, emb add)."""
    t = raw * sc.double() + sh.double()
    y = torch.where(t > 0, t, t * float(np.float32(SLOPE))) + add.double()
    mag = (raw * sc.double()).abs() + sh.double().abs() + add.double().abs()
    if emb is not None:
        y = y + emb
        mag = mag + emb.abs()
    return y, mag


def materialize_bound(ref, mag, dtype):
    """fmaf, the slope product, two adds: at most 4 fp32 roundings of values bounded by ``mag``, plus 1 ulp of the fp32
    scale / shift (the preamble's order of operations), then the rounding of the stored value."""
    u_out, floor = unit(dtype)
    return U32 * 6 * mag + u_out * ref.abs() + floor


def stats_bound(y_abs_sum, y_sq_sum, dtype, n_contrib):
    """Bound on |statistics words - fp64 sums of the stored output| per (n, c): the kernels sum their fp32 accumulators (at
    most 2^-11 / 2^-24 from the stored values) in fp32 chains of at most 1024 values per contribution before converting to
    fixed-point words (2^-44 each)."""
    u_out, _ = unit(dtype)
    bs = (u_out + U32 * 1024) * y_abs_sum + n_contrib * 2.0 ** -43
    bq = (2 * u_out + u_out * u_out + U32 * 1024) * y_sq_sum + n_contrib * 2.0 ** -43
    return bs, bq


# ---- backward kernels ---------------------------------------------------------------------------------------------------------
# The same bound form as the forward kernels: 2^-24 * (longest fp32 chain) * sum |terms| + the rounding of the stored value, with
# the chain read off each launcher.  A partial sum that a reduce kernel adds is one term of its chain; the chains nest, so an
# element's total chain is the length inside the main kernel plus the length of every reduction it then passes through.
def _cdiv(a, b):
    return -(-a // b)


def wgrad_fo_partitions(N, D, H, W, Cin, Cout, policy=0):
    """Mirror of wgrad_fo_partitions (csrc/conv3d_wgrad_fo.hip): (P, combos, total tiles) of the fetch-once form (4x8x8 tiles,
    64 co x 32 ci combos).  Pinned against dua_conv3d_k3_wgrad_workspace by the GPU tests."""
    combos = _cdiv(Cout, 64) * _cdiv(Cin, 32)
    total = N * _cdiv(D, 4) * _cdiv(H, 8) * _cdiv(W, 8)
    mult = ((policy & 31) >> 1) or 1
    P = min(_cdiv(256 * mult, combos), total)
    if P >= 8:
        P &= ~7
    return max(P, 1), combos, total


def wgrad_fo_route(combos, perm):
    """The reduce kernel the fetch-once launcher picks: "taps" (wgrad_fo_reduce_taps_kernel) for >= 32 slabs and the identity
    channel map, else "plain" (wgrad_fo_reduce_kernel)."""
    return "taps" if combos >= 32 and perm is None else "plain"


def wgrad_fo_chain(P, total, route):
    """Longest chain of one dW element through the fetch-once form.  A partition walks tiles part, part + P, ...: at most
    ceil(total / P) tiles of 256 voxels, 16 MFMA 32x32x16 steps each, + log2(16) = 4 adds inside the instruction.  The plain
    reduce sums P partials in four interleaved chains of ceil(P / 4) and adds the four in a tree of depth 2; the tap-gathering
    reduce sums them in one chain of P.  + 1: the += into dW."""
    main = _cdiv(total, P) * 16 + 4
    red = (_cdiv(P, 4) + 2) if route == "plain" else P
    return main + red + 1


def wgrad_3kd_partitions(N, D, H, W, Cin, Cout, policy):
    """Mirror of wgrad_partitions (csrc/conv3d_wgrad.hip): (P, combos, total tiles) of the three-kd form (2x8x8 tiles, one kd
    plane of 64 co x 64 ci per workgroup)."""
    combos = _cdiv(Cout, 64) * _cdiv(Cin, 64) * 3
    total = N * _cdiv(D, 2) * _cdiv(H, 8) * _cdiv(W, 8)
    mv = (policy & 31) >> 1
    mult = mv or (1 if total < 32 else 3)
    P = min(_cdiv(256 * mult, combos), total)
    if P >= 8:
        P = (P + 7) & ~7
    return max(P, 1), combos, total


def wgrad_3kd_workspace(P, combos):
    return P * combos * 9 * 4096 * 4 if P > 1 else 0


def wgrad_3kd_chain(P, total, dtype, partials):
    """Longest chain of one dW element through the three-kd form: ceil(total / P) tiles of 128 voxels; fp16: 8 MFMA 32x32x16
    steps per tile + 4 adds inside the instruction; fp32: 64 MFMA 32x32x2 steps + 1 add inside + 1 for the product's rounding.
    With partial sums: wgrad_reduce_kernel's four chains of ceil(P / 4), a depth-2 tree and the += (+ 3).  Without: the P
    workgroups' fp32 atomics into dW, in any order -- a chain of P adds."""
    main = _cdiv(total, P) * (8 + 4 if dtype == torch.float16 else 64 + 2)
    return main + (_cdiv(P, 4) + 3 if partials else P)


def _tall_gemm(a, b):
    """a^T b for a [V, m], b [V, n] with V in the hundreds of thousands: the long axis in up to 256 pieces (one batched GEMM, the pieces
    added in fp64), since a library GEMM with an m x n output of a few tiles walks all of V on a few compute units."""
    V = a.shape[0]
    S = min(256, V // 4096)
    if S < 2:
        return a.t() @ b
    V0 = V // S * S
    out = torch.bmm(a[:V0].view(S, V0 // S, -1).transpose(1, 2), b[:V0].view(S, V0 // S, -1)).sum(0)
    return out + a[V0:].t() @ b[V0:] if V0 < V else out


def wgrad_ref(x, c_off, cin, dy, co_off, cout, cin_src=None, perm=None, nominal=False):
    """fp64 weight gradient of the 3x3x3 convolution as 27 shifted GEMMs on x's device (no fp64 convolution), in the
    reference layout [cout, cin_src, 3, 3, 3], and sum |x| |dy| per element.  x, dy: channels-last buffers (the kernel's exact
    operands); ``perm`` (packed channel -> source channel, < 0: none) or the first ``cin_src`` packed channels.  ``nominal``: also
    the nominal_sum of every element (fp16 operands), gathered the same way."""
    N, D, H, W, _ = x.shape
    xp = torch.zeros((N, D + 2, H + 2, W + 2, cin), dtype=torch.float64, device=x.device)
    xp[:, 1:-1, 1:-1, 1:-1] = x[..., c_off:c_off + cin].double()
    g = dy[..., co_off:co_off + cout].double().reshape(-1, cout)
    ga = g.abs()
    outs = [torch.empty((27, cout, cin), dtype=torch.float64, device=x.device) for _ in range(3 if nominal else 2)]
    if nominal:
        ng, sg = nm16(g)
        g_sub, g_norm = ng * sg, ng * ~sg
    for t, (kd, kh, kw) in enumerate(itertools.product(range(3), repeat=3)):
        xs = xp[:, kd:kd + D, kh:kh + H, kw:kw + W].reshape(-1, cin)
        outs[0][t] = _tall_gemm(g, xs)
        outs[1][t] = _tall_gemm(ga, xs.abs())
        if nominal:
            nx, sx = nm16(xs)
            outs[2][t] = _tall_gemm(g_sub, nx) + _tall_gemm(g_norm, nx * sx)
    outs = [o.permute(1, 2, 0) for o in outs]                    # [cout, cin packed, 27]
    if perm is None:
        cs = cin if cin_src is None else cin_src
        outs = [o[:, :cs] for o in outs]
    else:
        p = perm[:cin].long().cpu()
        cs = cin_src
        keep = [(cp, int(ci)) for cp, ci in enumerate(p.tolist()) if 0 <= ci < cs]
        folded = [torch.zeros((cout, cs, 27), dtype=torch.float64, device=x.device) for _ in outs]
        for cp, ci in keep:
            for f, o in zip(folded, outs):
                f[:, ci] += o[:, cp]
        outs = folded
    return tuple(o.reshape(cout, cs, 3, 3, 3).contiguous() for o in outs)


def wgrad_bound(ref, abs_sum, dw0, n_chain, nominal=None):
    """Bound on dW = dw0 + (the kernel's sum) against dw0 + ref: the starting value is one more term of the chain (the += adds
    it), the fp32 result is stored as it is (its last rounding is that += , counted in n_chain).  ``nominal``: wgrad_ref's
    nominal_sum, the term for subnormal fp16 operands (module docstring)."""
    d0 = dw0.double()
    b = U32 * n_chain * (abs_sum + d0.abs()) * (1 + U32) + FLOOR32
    return b if nominal is None else b + subnormal_term(nominal) * (1 + U32)


# InstanceNorm + LeakyReLU backward (csrc/instnorm_bwd.hip): z = zh * gamma + beta, zh = (y - mean) * rstd; dZ = dA or slope dA
def in_bwd_reduce_chain(C, vox, dtype):
    """Per-thread fp32 chain of in_bwd_reduce_kernel: gpc = C / EPG channel groups, tpg = 256 / gpc threads per group, blocks =
    clamp(ceil(vox / (8 tpg)), 1, 1024) per sample; a thread walks the voxels tpg * blocks apart.  The block and replica
    reductions after it are in fp64 (2^-53 per add, below 2^-24 by far: counted as 2 fp32 steps)."""
    epg = 8 if dtype == torch.float16 else 4
    tpg = 256 // (C // epg)
    blocks = min(max(_cdiv(vox, tpg * 8), 1), 1024)
    return _cdiv(vox, tpg * blocks) + 2


DGRAD_REDUCE_CHAIN = 2 * 8 + 3 + 2
"""Per-lane fp32 chain of conv3d_k3_dgrad_reduce's sums (csrc/conv3d_wide.hip backward-sums epilogue): MB / 2 <= 2 plane pairs x 8
voxels per lane and tile (the halo holds at most 10 planes: TD = 2 MB <= 8), a 3-level shuffle tree; fp64 after that (+2)."""


def in_bwd_ref(dA, raw, sums_dec, gamma, beta, count, eps=1e-5, slope=SLOPE):
    """fp64 InstanceNorm + LeakyReLU backward on x's device.  dA, raw: [N, V, C] exact operand values (any float type);
    ``sums_dec``: stats_decode of the forward statistics words (the kernels' own), float64 [N, c_pad, 2].  Returns a dict:
    S0, S1, S2 [N, C]; their abs sums A0, A1, A2; dY [N, V, C]; and per-element pieces the bounds need: zhat, z, dz, rstd,
    mean, e_zh (bound on the kernel's fp32 zh), near (|z| within the margin where fp32 may take the other slope)."""
    N, V, C = raw.shape
    dev = raw.device
    sd = sums_dec.to(dev)
    mean = sd[:, :C, 0] / count
    var = (sd[:, :C, 1] / count - mean * mean).clamp_min(0)
    rstd = 1.0 / torch.sqrt(var + float(np.float32(eps)))
    g = gamma.double().to(dev)[None, None]
    b = beta.double().to(dev)[None, None]
    y, d = raw.double(), dA.double()
    zhat = (y - mean[:, None]) * rstd[:, None]
    z = zhat * g + b
    sl = float(np.float32(slope))
    dz = torch.where(z > 0, d, d * sl)
    # the kernel's zh = fl(fl(y - fl32(mean)) * fl32(rstd)): mean off by U32 |mean|, rstd by U32, two roundings
    e_zh = U32 * (3 * zhat.abs() + rstd[:, None] * mean[:, None].abs()) * (1 + 4 * U32)
    margin = g.abs() * e_zh + 2 * U32 * ((zhat * g).abs() + b.abs())
    near = z.abs() <= margin
    S0, S1, S2 = d.sum(1), dz.sum(1), (dz * zhat).sum(1)
    A0, A1, A2 = d.abs().sum(1), dz.abs().sum(1), (dz * zhat).abs().sum(1)
    gr = g * rstd[:, None]
    dY = gr * (dz - S1[:, None] / V - zhat * S2[:, None] / V)
    return dict(S0=S0, S1=S1, S2=S2, A0=A0, A1=A1, A2=A2, dY=dY, zhat=zhat, z=z, dz=dz, d=d, rstd=rstd, mean=mean, e_zh=e_zh,
                near=near, gr=gr, V=V, slope=sl)


def in_bwd_sums_bound(r, n_chain):
    """Bounds [N, C] on the kernel's S0, S1, S2 against fp64: the fp32 chains (dZ's slope product rounds once more, the fmaf
    chain of S2 once more for zh), zh's own error e_zh in S2, and (1 - slope) |dA| (|dA zhat| for S2) for every element near the
    kink, where fp32 may take the other slope."""
    kink = (1 - r["slope"]) * r["d"].abs() * r["near"]
    e2 = (r["dz"].abs() * r["e_zh"]).sum(1)
    b0 = U32 * n_chain * r["A0"] + FLOOR32
    b1 = U32 * (n_chain + 1) * r["A1"] + kink.sum(1) + FLOOR32
    b2 = U32 * (n_chain + 2) * r["A2"] + e2 + (kink * r["zhat"].abs()).sum(1) + FLOOR32
    return b0, b1, b2


def in_bwd_dy_bound(r, b1, b2, dtype):
    """Bound [N, V, C] on the apply kernel's dY = gamma rstd (dZ - S1 / V - zh S2 / V) in fp32, stored in ``dtype``: the sums off
    by b1, b2 (then rounded to fp32 after the division), zh off by e_zh, dZ rounded once, two subtractions and the product
    of up to M = |dZ| + |S1| / V + |zh S2| / V rounded 4 times; rstd rounded to fp32 and the two products (3 U32 |dY|); the
    stored value's rounding; near the kink (1 - slope) |dA| gamma rstd."""
    u_out, floor = unit(dtype)
    V = r["V"]
    S1, S2 = r["S1"][:, None], r["S2"][:, None]
    M = r["dz"].abs() + S1.abs() / V + (r["zhat"] * S2).abs() / V
    et = 4 * U32 * M + (b1[:, None] + r["zhat"].abs() * b2[:, None]) / V + r["e_zh"] * (S2.abs() + b2[:, None]) / V
    gr = r["gr"].abs()
    kink = (1 - r["slope"]) * r["d"].abs() * r["near"]
    return (gr * (et + kink) * (1 + 4 * U32) + 3 * U32 * r["dY"].abs()) * (1 + u_out) + u_out * r["dY"].abs() + floor


def head_bwd_chains(vox, dtype, mfma):
    """(du chain, dW / db chain) of dua_head_bwd.  du: fp16 MFMA path one 32x32x16 over K <= 16 classes (chain_length(16)); fp32
    an fmaf chain of K <= 16 (+1).  dW, db: the MFMA path's waves add 32 voxels per 16x16x32 step over ceil(tiles / blocks)
    128-voxel tiles (+ log2(32) inside), the plain kernel's threads 16 voxels of every 64-voxel tile of theirs with fmaf; a
    4-way tree over the waves (+2); head_reduce_kernel's 16 slices of ceil(blocks / 16) partials in four chains (+2) and the
    16 slices' atomics into the zeroed outputs (+16)."""
    t64 = _cdiv(vox, 64)
    blocks = min(max(t64, 1), 1024)
    if mfma:
        t128 = _cdiv(vox, 128)
        g2 = min(t128, blocks)
        main, du = _cdiv(t128, g2) + 5, chain_length(16, torch.float16)
    else:
        g2 = blocks
        main, du = _cdiv(t64, g2) * 16, 17
    return du, main + 2 + _cdiv(_cdiv(g2, 16), 4) + 2 + 16


def deconv_bwd_chains(N, D, H, W, Cin, Cout, dtype):
    """(dx chain, dW chain, P) of dua_deconv_k2s2_bwd.  dx: a contraction over 8 taps x Cout (chain_length).  dW: P =
    min(ceil(768 / (8 combos)), tiles) partitions (deconv_wgrad_partitions, 64 ci x 64 co combos, 128 / 64-voxel tiles for fp16
    / fp32); four waves take a quarter of every tile each: 2 MFMA 32x32x16 steps (+4 inside) or 8 MFMA 32x32x2 (+1 inside, +1
    product rounding) per tile; a two-round tree over the waves (+2); deconv_wgrad_reduce_kernel's two chains of ceil(P / 2)
    and their sum (+1); the += into the zeroed dW (+1)."""
    combos = _cdiv(Cin, 64) * _cdiv(Cout, 64)
    tv = 128 if dtype == torch.float16 else 64
    total = N * _cdiv(D * H * W, tv)
    P = max(min(_cdiv(768, 8 * combos), total), 1)
    main = _cdiv(total, P) * (2 + 4 if dtype == torch.float16 else 8 + 2)
    return chain_length(8 * Cout, dtype), main + 2 + _cdiv(P, 2) + 1 + 1, P


def deconv_fold_dy(dy, D, H, W):
    """The transposed convolution's output gradient as its backward reads it, float64 [N, 2D, 2H, 2W, C]: a replicate-padded plane
    (dy one plane longer on an odd axis) adds into the plane it copies, axis by axis (corners reach the corner)."""
    t = dy.double()
    for ax, S in ((1, D), (2, H), (3, W)):
        if t.shape[ax] == 2 * S + 1:
            body = t.narrow(ax, 0, 2 * S).clone()
            body.narrow(ax, 2 * S - 1, 1).add_(t.narrow(ax, 2 * S, 1))
            t = body
    return t


def deconv_bwd_ref(x, dyf, w, dtype):
    """x float64 [N, D, H, W, Cin], dyf = deconv_fold_dy [N, 2D, 2H, 2W, Cout], w [Cin, Cout, 2, 2, 2] (rounded to ``dtype`` as
    the data-gradient packer rounds it) -> (dx, |dx| terms, squared terms) [N, D, H, W, Cin] and (dw, |dw| terms) like w."""
    N, D, H, W, Cin = x.shape
    Cout = dyf.shape[-1]
    A = dyf.reshape(N, D, 2, H, 2, W, 2, Cout).permute(0, 1, 3, 5, 2, 4, 6, 7).reshape(-1, 8 * Cout)
    wq = (w.half() if dtype == torch.float16 else w.float()).double()
    Wm = wq.permute(2, 3, 4, 1, 0).reshape(8 * Cout, Cin)
    dx, ax, sq = A @ Wm, A.abs() @ Wm.abs(), (A * A) @ (Wm * Wm)
    X = x.double().reshape(-1, Cin)
    dw = (X.t() @ A).reshape(Cin, 2, 2, 2, Cout).permute(0, 4, 1, 2, 3)
    aw = (X.abs().t() @ A.abs()).reshape(Cin, 2, 2, 2, Cout).permute(0, 4, 1, 2, 3)
    shp = (N, D, H, W, Cin)
    return dx.reshape(shp), ax.reshape(shp), sq.reshape(shp), dw.contiguous(), aw.contiguous()


def deconv_bwd_nominal(x, dyf, w, padded):
    """nominal_sum of deconv_bwd_ref's two contractions on the same fp16 operands: (for dx [N, D, H, W, Cin], for dw like w).
    ``padded``: the kernel's folded dy is its own fp16 rounding of a sum, up to one ulp from the fp64 fold rounded once (the
    difference the RSS term covers): its nominal magnitudes are taken with nm16's ``ulp_off``."""
    N, D, H, W, Cin = x.shape
    Cout = dyf.shape[-1]
    A = _f16_rne(dyf.cpu()).to(dyf.device).reshape(N, D, 2, H, 2, W, 2, Cout).permute(0, 1, 3, 5, 2, 4, 6, 7).reshape(-1, 8 * Cout)
    Wm = w.half().double().permute(2, 3, 4, 1, 0).reshape(8 * Cout, Cin)
    ndx = nominal_sum(A, Wm, ulp_off=padded).reshape(N, D, H, W, Cin)
    ndw = nominal_sum(A.t(), x.double().reshape(-1, Cin), ulp_off=padded).reshape(2, 2, 2, Cout, Cin).permute(4, 3, 0, 1, 2)
    return ndx, ndw.contiguous()


# ---- forward transposed convolution, materialize and the training head, standalone ---------------------------------------------
# Chains read off csrc/deconv.hip and csrc/head.hip.  fp16: a 32-channel chunk is two MFMA 32x32x16 steps (16 products each, + log2(16)
# adds inside the instruction).  fp32: a 16-channel chunk is eight MFMA 32x32x2 steps; whether a step rounds once or once per product
# is not specified, so every product counts as one fmaf of the chain (the module docstring's rule for fp32 kernels).
def deconv_fwd_chain(form, cin, dtype):
    """Longest fp32 chain of one output element of dua_deconv_k2s2_fwd in the given form.
    "one_tap" (deconv_k2s2_kernel): the chunks one after the other into one accumulator, then + bias.
    "ksplit" (deconv_k2s2_ksplit_kernel): wave w sums chunks w, w + 4, ... (ceil(nchunks / 4) of them); the four partial tiles are
    added to zero in the order 0..3 (4 additions, the first of them exact), then + bias.
    "alltaps" (deconv_k2s2_alltaps_kernel, both tile sizes): the accumulator STARTS at the bias (a term of the sum, no rounding of
    its own), then the chunks one after the other."""
    ck, per_chunk, inside = (32, 2, 4) if dtype == torch.float16 else (16, 16, 0)
    nch = _cdiv(cin, ck)
    if form == "one_tap":
        return per_chunk * nch + inside + 1
    if form == "ksplit":
        return per_chunk * _cdiv(nch, 4) + inside + 4 + 1
    if form == "alltaps":
        return per_chunk * nch + inside
    raise ValueError(form)


def deconv_ref_by_child(A, w, bias, dtype, child):
    """``deconv_ref`` evaluated child by child: the same three sums, without gathering a [P, Cin, Cout] weight tensor per voxel
    (P = every voxel of an output with 512 input channels would be gigabytes)."""
    P, cout = A.shape[0], w.shape[1]
    ref = torch.zeros((P, cout), dtype=torch.float64)
    ab, sq = torch.zeros_like(ref), torch.zeros_like(ref)
    for k in range(8):
        rows = (child == k).nonzero().view(-1)
        if rows.numel():
            r, a, s = deconv_ref(A[rows], w, bias, dtype, torch.full((1,), k, dtype=torch.int64).expand(rows.numel()))
            ref[rows], ab[rows], sq[rows] = r, a, s
    return ref, ab, sq


def all_voxels(N, dims):
    """int64 [N D H W, 4] (n, d, h, w): every voxel, in sample_voxels' sorted order."""
    D, H, W = dims
    g = torch.meshgrid(torch.arange(N), torch.arange(D), torch.arange(H), torch.arange(W), indexing="ij")
    return torch.stack([t.reshape(-1) for t in g], 1)


def deconv_sources(pts, coarse_dims):
    """Output voxels of a (possibly replicate-padded) transposed convolution -> (parent voxel [P, 4] in the coarse grid, child
    [P] = (d & 1) * 4 + (h & 1) * 2 + (w & 1)) of the voxel each value is computed at (replicate_source)."""
    q = replicate_source(pts, coarse_dims)
    parent = q.clone()
    parent[:, 1:] >>= 1
    return parent, (q[:, 1] & 1) * 4 + (q[:, 2] & 1) * 2 + (q[:, 3] & 1)


def channel_sums(x):
    """float64 [N, C, 2] = (sum x, sum x^2) over the voxels of channels-last x [N, ..., C]: the statistics a producer leaves."""
    v = x.double().reshape(x.shape[0], -1, x.shape[-1])
    return torch.stack([v.sum(1), (v * v).sum(1)], -1)


def pool_ref(ref, bnd):
    """Floor MaxPool3d(2) of a channels-last fp64 reference [N, D, H, W, C] and, per window, the largest of its eight bounds: the
    maximum of the rounded outputs is the rounding of the maximum, so it lies within that of the fp64 maximum."""
    p = lambda t: torch.nn.functional.max_pool3d(t.permute(0, 4, 1, 2, 3), 2).permute(0, 2, 3, 4, 1)      # noqa: E731
    return p(ref), p(bnd)


def head_fwd_route(C, dtype):
    """dua_head_fwd: "mfma" (head_fwd_mfma_kernel: fp16, C = 32 or 64, the weights rounded to fp16 MFMA operands) or "plain"
    (head_fwd_kernel: fp32 weights in registers, one fmaf per channel)."""
    return "mfma" if dtype == torch.float16 and C in (32, 64) else "plain"


def head_fwd_chain(C, dtype):
    """mfma: the accumulator starts at the bias, C / 32 MFMA 16x16x32 steps (+ log2(32) adds inside); plain: bias, then C fmaf."""
    return C // 32 + 5 if head_fwd_route(C, dtype) == "mfma" else C + 1


def head_fwd_ref(u, w, b, dtype):
    """logits = u W^T + b on the operands as the kernel rounds them: u [P, C] float64 (stored values), w fp32 [K, C] (through
    fp16 on the mfma route), b fp32 [K].  Returns (ref, sum |terms|, sum terms^2), [P, K]."""
    wq = w.detach().float().cpu()
    if head_fwd_route(w.shape[1], dtype) == "mfma":
        wq = wq.half()
    ref, ab, sq = contract(u, wq.double().t())
    bb = b.detach().double().cpu()[None]
    return ref + bb, ab + bb.abs(), sq
