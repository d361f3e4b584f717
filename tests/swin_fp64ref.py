"""fp64 references of the Swin kernels (BASELINE config 5) on sampled token rows, and per-element error bounds.

A plain helper module of the suite (``import swin_fp64ref as S``), the Swin counterpart of ``fp64ref`` (``R``), whose constants
(``U16``, ``U32``, ``FLOOR16``, ``C_RSS``) and contraction bound (``R.bound``, ``R.chain_length``) it reuses.  Every reference
is evaluated on the EXACT operands the kernel read: fp16 buffers widened, fp32 inputs rounded to fp16 where the kernel rounds
them (``f16``), the fp32 token stream as the kernel STORED it where a kernel writes the stream and normalises it in the same
launch (the stored value is the LayerNorm's input bit for bit, so the stream is checked against ``x + update`` and the norm
against the stored stream; nothing has to be propagated through the norm's Jacobian).  The semantics are restated from the
reference project and pinned to ``oracle/swin_ref.py`` by tests/test_swin_fp64ref.py.

No constant below is fitted to a measurement of a kernel.  The numeric constants are: those of ``fp64ref``; instruction
accuracies as documented (``v_rcp_f32``, ``v_exp_f32``, ``v_rsq_f32`` / ``rsqrtf``: 1 ulp = 2 U32; a division that is not
correctly rounded: 2.5 ulp = 5 U32, ``U_DIV``); the Abramowitz-Stegun 7.1.26 approximation error 1.5e-7, re-established on the
CPU against ``torch.erf`` by the test file.  gamma_n = n U32 / (1 - n U32) is the usual bound on (1 + U32)^n - 1.

Contractions (token_linear, token_gemm, swin_mlp): ``R.bound`` with the chain of the kernel taken: MFMA 32x32x16 adds 16
products per step, ``R.chain_length(K, fp16)`` = ceil(K / 16) + 4 + 1 (bias); the split-K form adds its ``ksplit`` partials to
the bias in a finish launch (``split_parts=ksplit``).  Steps padded with zeros add exact zeros.  RESIDUAL adds the result to the
fp32 stream: one more term (|x|) and one more step.

GELU (``gelu_erf`` of csrc/common.hpp, operation by operation; z = |x| / sqrt 2, t = 1 / (1 + p z), E = P(t) t exp(-z^2)):
    z      = fl(|x| c)                 constant and product                         rel 2 U32
    w      = fma(p, z, 1)              p rounded, one rounding; p z < w             rel 3 U32 + U32
    t      = rcp(w)                    1 ulp                                        rel e_t = 6 U32
    P(t)   Horner, 4 fma, 5 rounded coefficients: |fl P - P| <= gamma_9 Pabs(t) (Higham, Horner), and t's own error moves P by
           at most e_t t |P'|abs <= 4 e_t Pabs(t), Pabs = the polynomial of |a_i| (the coefficients alternate in sign: near
           x = 0, P(1) = 1 but Pabs(1) = 4.48, which is why the rounding terms, not the approximation, dominate)
    E      = fl(fl(P t) exp)           exp = v_exp_f32(fl(-z^2 log2 e)): z^2 carries rel 5 U32 (an absolute 5 U32 z^2 in the
                                       exponent), the log2 e product 2 U32 z^2, the instruction 2 U32, two products 2 U32, t e_t
           |E~ - E| <= (gamma_9 + 4 e_t) Pabs(t) t exp(-z^2) + E U32 (10 + 7 z^2)                                   =: err_E
    erf~   = fl(1 - E~)                |erf~ - erf| <= 1.5e-7 + err_E + U32 (1 - E)
    out    = fl(0.5 x fl(1 + s erf~))  |out - gelu(x)| <= 0.5 |x| (1.5e-7 + err_E + U32 (1 - E) + 2 U32) + U32 |gelu(x)|
    a pre-activation that is itself off by e_x moves the result by at most 1.13 e_x (|gelu'| <= 1.13), then the stored value's
    rounding.  The error is ABSOLUTE in 0.5 |x|: in the far negative tail, where gelu(x) -> 0, it exceeds the value.

LayerNorm (``group_layernorm`` of csrc/swin_tokens.hip and its copies; v = the exact fp32 inputs, C of them):
    s~     a chain of n fp32 adds (per-lane chain + the group butterfly)            |s~ - s| <= gamma_n sum |v|
    mean~  = s~ / C                                                                 e_m = (gamma_n sum|v| + U_DIV (|s| + ..)) / C
    d~_i   = fl(v_i - mean~)           |d~_i - (v_i - mean)| <= U32 |v_i - mean| + e_m (1 + U32)                    =: err_d
    q~     = sum d~_i^2 (fmaf chain + butterfly): sum (v_i - mean~)^2 = Q + C (mean~ - mean)^2 exactly, each d~_i^2 within
             (1 + U32)^2, the chain gamma_n; / C, + eps, all terms positive, so (var + eps) carries the relative error
             e_v = gamma_n + 2 U32 + U_DIV + U32 + e_m^2 / (var + eps)  (products of these are below 1e-12 and added as e_v^2)
    rstd~  = rsqrtf(.) 1 ulp           e_r = 0.5 e_v / (1 - e_v)^1.5 + 2 U32
    out    = fl(fl(fl(d~ rstd~) gamma) + beta)
             |t~ - t| <= (|v_i - mean| + err_d) rstd (1 + e_r) |gamma| (1 + U32)^2 - |v_i - mean| rstd |gamma|       =: err_t
             |out - ref| <= err_t + U32 (|t| + err_t + |beta|), then the rounding of the stored value
    The bound is relative to |v - mean| rstd |gamma| except for the e_m rstd |gamma| term: a row with |mean| >> std pays
    gamma_n |mean| rstd there, and only there -- the kernels centre before squaring, a sum-of-squares form would pay |mean|^2.

Attention (csrc/window_attention.hip: 32-key blocks, running maximum m_b, probabilities rounded to fp16, P V and the
denominator accumulated by the same MFMAs, one division at the end).  q, k, v are fp16 (the fp32 instantiation rounds them on
load, ``load8``; 0.25 q is exact unless it falls below 2^-14: FLOOR16 |k| per product).  With exact z = 0.25 q.k + bias + mask:
    z~     one MFMA over 16 exact products on top of the bias in the accumulator, then the mask add:
           |z~ - z| <= U32 (chain_length(16) + 1) (0.25 sum |q k| + |bias| + |mask|) + FLOOR16 sum |k|              =: e_z
    p~_k   = fp16(exp2(fma(z~, L, fl(-m_b L)))), L = fl(log2 e).  In nats the argument is
           [(z~ - m_b)(1 + dL) - m_b d1 (1 + dL)](1 + d2): off by e_a = e_z + U32 (2 |z - m_b| + |m_b|) (1 + 3 U32); v_exp_f32
           1 ulp; fp16 rounding U16 above the subnormal range, an absolute min(FLOOR16, p~) below it (a value under 2^-25
           becomes 0: the error is the value).  Each later block that raises the maximum multiplies the running sums by
           alpha~ = exp2(fl(fl(m_old - m_new) L)), off by 3 U32 (m_new - m_old) + 2 U32 relative -- the same factor on
           numerator and denominator, i.e. one more relative error of the weights of all EARLIER keys (R_b, summed over the later
           blocks).  The m_b telescope whatever their computed values are, and a common factor cancels in the quotient.  So, in
           units where the row maximum has weight 1,
           w_k = p_k (1 + e_k) + h_k, 1 + e_k <= exp(e_a) (1 + 2 U32) (1 + U16) exp(R_b), |h_k| <= min(FLOOR16, p_k (1 + e_k))
    exact arithmetic on perturbed weights: sum_k w_k v_kd / sum_k w_k - ref_d = sum_k dw_k (v_kd - ref_d) / sum_k w_k because
    sum_k p_k (v_kd - ref_d) = 0, with |dw_k| <= e_k p_k + h_k =: dp_k and sum_k w_k >= S - sum_k dp_k =: D_low > 0:
           B1 = sum_k dp_k |v_kd - ref_d| / D_low          -- exact, not first order: the remainder sits in D_low
    accumulation: numerator and denominator each pass n_c = 3 nb + 4 roundings (per block one rescale product and two MFMA steps,
    + 4 inside the instruction): |N~ - N_w| <= g A_w, D~ = D_w (1 + e), |e| <= g = gamma_{n_c}, A_w = sum w_k |v_kd| <= A_up =
    sum (p_k + dp_k) |v_kd|; the quotient 1 / D~ (U_DIV) and the product (U32):
           B2 = (2 g / (1 - g) + 8 U32) A_up / D_low       (8 > U_DIV + 1 + their products with 1 + 2 g / (1 - g))
    |out - ref| <= (B1 + B2)(1 + u_out) + u_out |ref| + floor_out.
    The fp32 instantiation stores fp32 but keeps fp16 probabilities: its bound is dominated by U16 sum p_k |v_kd - ref_d| / S,
    three orders above an fp32 rounding, and says so.

Statistics words: ``R.stats_bound`` against fp64 sums of the STORED output.

patch_embed (Conv3d k = s = 2 as a [tokens x 8 Cp] GEMM, + bias + t_proj row, the fp32 stream, LayerNorm without affine + emb):
the kernels store the stream x from the very registers they normalise, so, with x requested, the argument of SCATTER holds
again: x is held to the contraction bound, the norm to the LayerNorm bound on the stored x.  fp16 form (patch_embed_mfma_kernel):
weights rounded to fp16 on staging, MFMA chain ``R.chain_length(K, fp16)`` (its + 1 is the add of c = fl(bias + tadd)) + 1 for
that sum's own rounding; LayerNorm over 4 lanes of 12 values.  fp32 form (patch_embed_kernel): acc = fl(bias + tadd), then one
fmaf per product: K + 1 roundings; a serial LayerNorm over the 48 registers (``ln_chain(48, 1)``).

linear_f32: fp32 MFMA 32x32x2 = a k-ordered fmaf chain (one rounding per product), + bias: ``R.chain_length(K, fp32)`` = K + 1.
Its GELU is 0.5 v (1 + erff(v c)): erff at the 4 ulp the HIP math API documents (8 U32 |erf|), the argument's two roundings
move erf by at most 2 U32 z erf'(z), the add 1 + erf and the two products one rounding each (``gelu_erff_bound``).

residual_norm_act (tail of UnetResBlock): evaluated on the kernel's own fp32 scale / shift (``ops.instnorm_finalize``, which the
GPU test holds to ``R.finalize`` of the statistics words within its b_sc / b_sh), y = fma(raw, sc, sh), rr = fma(res, rsc, rsh)
or res, y + rr, the slope product, + post, + s (1 - 1 / (1 + exp(-s))): at most 6 roundings of partial sums bounded by the sum
of |terms| (gamma_6 mag), plus the reverse-attention term's own error: exp(-s) = v_exp_f32(fl(-s log2 e)) relative
(2 + 2 |s|) U32, which moves sigma by sigma (1 - sigma) of that; 1 + e and the division U32 + U_DIV of sigma; 1 - sigma one
rounding; the product one rounding.
"""
from __future__ import annotations

import math

import numpy as np
import torch

import fp64ref as R
from fp64ref import FLOOR16, U16, U32

U_DIV = 5 * U32                     # a division that is not correctly rounded: 2.5 ulp
U_ULP = 2 * U32                     # 1 ulp instructions: v_rcp_f32, v_exp_f32, rsqrtf
AS_ERR = 1.5e-7                     # Abramowitz-Stegun 7.1.26, |erf_AS - erf|
AS_P = 0.3275911
AS_A = (0.254829592, -0.284496736, 1.421413741, -1.453152027, 1.061405429)
GELU_LIP = 1.13
F16, F32 = torch.float16, torch.float32


def gamma_n(n):
    return n * U32 / (1 - n * U32)


def f16(v):
    """float64 / fp32 -> fp16 (one round-to-nearest-even) -> float64: an operand the kernel rounds on load."""
    return R._f16_rne(v.double())


# ---- which rows ---------------------------------------------------------------------------------------------------------------
def structured_rows(M, tiles=(32, 64, 128), boundaries=(), window=None):
    """The rows a tiled kernel goes wrong at first: both sides of every 32-, 64- and 128-row tile edge (for M beyond 4096: of
    the first and last 4 tiles of each size), the whole last partial tile's first and last row, both sides of every sample
    boundary, first / last token of the first / last window."""
    rows = {0, M - 1}
    for t in tiles:
        nt = -(-M // t)
        ks = range(1, nt) if nt <= 32 else list(range(1, 5)) + list(range(nt - 4, nt))
        for k in ks:
            rows.update((k * t - 1, k * t))
        rows.add((nt - 1) * t)
    for b in boundaries:
        rows.update((b - 1, b))
    if window:
        rows.update((window - 1, M - window))
    return {r for r in rows if 0 <= r < M}


def sample_rows(M, n_random=256, seed=0, **kw):
    """int64 sorted unique rows: ``structured_rows`` plus seeded random rows."""
    g = np.random.default_rng(seed)
    rows = structured_rows(M, **kw)
    rows.update(int(r) for r in g.integers(0, M, size=min(n_random, M)))
    return torch.tensor(sorted(rows), dtype=torch.int64)


# ---- window geometry ----------------------------------------------------------------------------------------------------------
def window_token_map(B, dims, ws, ss, roll_sign=-1, crop=True):
    """int64 [B * windows * tokens]: the voxel (linear index into [B, D, H, W]) a window token holds, -1 for padding:
    pad to a window multiple -> roll(-shift) -> window_partition (transformer.py:378-417).  ``roll_sign`` / ``crop`` exist for
    the planted defects of the CPU test."""
    D, H, W = dims
    pad = [(ws[i] - dims[i] % ws[i]) % ws[i] for i in range(3)]
    Dp, Hp, Wp = D + pad[0], H + pad[1], W + pad[2]
    idx = torch.full((B, Dp, Hp, Wp), -1, dtype=torch.int64)
    idx[:, :D, :H, :W] = torch.arange(B * D * H * W).view(B, D, H, W)
    if not crop:                                   # defect: the padded border is taken for real voxels (clamped)
        idx = torch.where(idx < 0, torch.zeros_like(idx), idx)
    if any(ss):
        idx = torch.roll(idx, shifts=tuple(roll_sign * s for s in ss), dims=(1, 2, 3))
    wd, wh, ww = ws
    t = idx.view(B, Dp // wd, wd, Hp // wh, wh, Wp // ww, ww).permute(0, 1, 3, 5, 2, 4, 6)
    return t.reshape(-1)


def region_ids(dims, ws, ss):
    """uint8 [windows, tokens]: the region label compute_mask (attention.py:135-157) gives every token of the padded map."""
    pad = [(ws[i] - dims[i] % ws[i]) % ws[i] for i in range(3)]
    dp = [dims[i] + pad[i] for i in range(3)]
    img = torch.zeros(dp, dtype=torch.int64)
    cnt = 0
    for sd in (slice(-ws[0]), slice(-ws[0], -ss[0]), slice(-ss[0], None)):
        for sh in (slice(-ws[1]), slice(-ws[1], -ss[1]), slice(-ss[1], None)):
            for sw in (slice(-ws[2]), slice(-ws[2], -ss[2]), slice(-ss[2], None)):
                img[sd, sh, sw] = cnt
                cnt += 1
    t = img.view(dp[0] // ws[0], ws[0], dp[1] // ws[1], ws[1], dp[2] // ws[2], ws[2]).permute(0, 2, 4, 1, 3, 5)
    return t.reshape(-1, ws[0] * ws[1] * ws[2]).to(torch.uint8)


def table_bias(table_t, heads_sel, n, grid=(7, 7, 7), own_grid=None, transpose=False):
    """Dense bias [P, n, n] (query, key) of the heads ``heads_sel`` from the transposed table [heads, (2gd-1)(2gh-1)(2gw-1)]:
    token -> coordinate through the TABLE's grid, also for clipped windows (the reference slices the 7^3 index to [:n, :n],
    attention.py:104).  ``own_grid`` (defect): coordinates through the clipped window's own grid.  ``transpose`` (defect):
    [k][q] read as [q][k]."""
    gd, gh, gw = grid
    cd, ch, cw = own_grid or grid
    t = torch.arange(n)
    co = torch.stack([t // (ch * cw), (t // cw) % ch, t % cw], 1)
    rel = co[:, None] - co[None]                                               # [q, k, 3]
    idx = ((rel[..., 0] + gd - 1) * (2 * gh - 1) + rel[..., 1] + gh - 1) * (2 * gw - 1) + rel[..., 2] + gw - 1
    b = table_t.double()[heads_sel][:, idx]                                   # [P, q, k]
    return b.transpose(1, 2) if transpose else b


def region_mask(reg, wins, nw):
    """[P, n, n] 0 / -100 from region ids [nw, n] for windows ``wins`` (mask row = window % nw)."""
    r = reg.long()[wins % nw]
    return torch.where(r[:, :, None] != r[:, None, :], -100.0, 0.0).double()


# ---- attention ----------------------------------------------------------------------------------------------------------------
def attention_ref(q, k, v, bias, mask=None, scale=0.25):
    """q, k, v float64 [P, n, 16] (fp16 values), bias [P, n, n] (query, key), mask [P, n, n] or None -> dict with the reference
    ``out`` [P, n, 16] and what ``attention_bound`` needs."""
    qk = scale * torch.einsum("pqd,pkd->pqk", q, k)
    A = scale * torch.einsum("pqd,pkd->pqk", q.abs(), k.abs()) + bias.abs()
    z = qk + bias
    if mask is not None:
        z = z + mask
        A = A + mask.abs()
    M = z.max(-1, keepdim=True).values
    p = torch.exp(z - M)
    S = p.sum(-1, keepdim=True)
    out = torch.einsum("pqk,pkd->pqd", p, v) / S
    return dict(out=out, z=z, A=A, p=p, S=S, M=M, v=v, ksum=k.abs().sum(-1))


def attention_bound(r, dtype_out):
    """Per-element bound [P, n, 16] (module docstring)."""
    z, A, p, S, v, out = r["z"], r["A"], r["p"], r["S"], r["v"], r["out"]
    P, n, _ = z.shape
    nb = -(-n // 32)
    u_out, floor = R.unit(dtype_out)
    e_z = U32 * (R.chain_length(16, F16) + 1) * A + FLOOR16 * r["ksum"][:, None, :]
    zp = torch.nn.functional.pad(z, (0, nb * 32 - n), value=-math.inf).view(P, n, nb, 32)
    m_b = torch.cummax(zp.max(-1).values, -1).values                           # running maximum after block b  [P, n, nb]
    rise = torch.zeros_like(m_b)
    rise[..., 1:] = m_b[..., 1:] - m_b[..., :-1]
    step = 3 * U32 * rise + U_ULP
    step[..., 0] = 0.0                                                         # the first block rescales zeros
    R_b = step.flip(-1).cumsum(-1).flip(-1) - step                             # later blocks only
    m_k = m_b.repeat_interleave(32, -1)[..., :n]
    R_k = R_b.repeat_interleave(32, -1)[..., :n]
    e_a = e_z + U32 * (2 * (z - m_k).abs() + m_k.abs()) * (1 + 3 * U32)
    e_k = torch.exp(e_a + R_k) * (1 + U_ULP) * (1 + U16) - 1
    dp = e_k * p + torch.minimum(torch.full_like(p, FLOOR16), p * (1 + e_k))
    D_low = S - dp.sum(-1, keepdim=True)
    assert bool((D_low > 0.5).all())
    B1 = torch.empty_like(out)
    for i in range(P):                                                         # [n, n, 16] per pair
        B1[i] = torch.einsum("qk,qkd->qd", dp[i], (v[i][None] - out[i][:, None]).abs())
    A_up = torch.einsum("pqk,pkd->pqd", p + dp, v.abs())
    g = gamma_n(3 * nb + 4)
    B2 = (2 * g / (1 - g) + 8 * U32) * A_up
    return (B1 + B2) / D_low * (1 + u_out) + u_out * out.abs() + floor


# ---- GELU ---------------------------------------------------------------------------------------------------------------------
def gelu64(x):
    return 0.5 * x * (1 + torch.erf(x * 0.7071067811865476))


def as_erf64(z):
    """The Abramowitz-Stegun 7.1.26 form in float64 (z >= 0) -> (erf_AS, t, P(t), Pabs(t), E)."""
    t = 1 / (1 + AS_P * z)
    P = torch.zeros_like(z)
    Pa = torch.zeros_like(z)
    for a in reversed(AS_A):
        P = P * t + a
        Pa = Pa * t + abs(a)
    E = P * t * torch.exp(-z * z)
    return 1 - E, t, P, Pa, E


def gelu_bound(x, e_x, dtype_out):
    """Bound on |stored gelu_erf(x~) - gelu(x)| for a float64 pre-activation x whose fp32 value is within e_x."""
    u_out, floor = R.unit(dtype_out)
    z = x.abs() * 0.7071067811865476
    _, t, _, Pa, E = as_erf64(z)
    e_t = 6 * U32
    err_E = (gamma_n(9) + 4 * e_t) * Pa * t * torch.exp(-z * z) + E * U32 * (10 + 7 * z * z)
    g = gelu64(x)
    b = 0.5 * x.abs() * (AS_ERR + err_E + U32 * (1 - E) + 2 * U32) + U32 * g.abs() + GELU_LIP * e_x
    return b * (1 + u_out) + u_out * g.abs() + floor


def gelu_erf_emulated(x32):
    """``gelu_erf`` of csrc/common.hpp in torch fp32 on the CPU, operation by operation (IEEE reciprocal and exp instead of the
    1-ulp instructions)."""
    one = torch.ones((), dtype=F32)
    z = x32.abs() * np.float32(0.70710678118654752)
    t = one / torch.addcmul(one, z, torch.tensor(np.float32(0.3275911)))
    p = t * np.float32(1.061405429) + np.float32(-1.453152027)
    for a in (1.421413741, -0.284496736, 0.254829592):
        p = p * t + np.float32(a)
    e = one - p * t * torch.exp(-z * z)
    return np.float32(0.5) * x32 * (one + torch.copysign(e, x32))


# ---- contractions and their epilogues ------------------------------------------------------------------------------------------
def linear_ref(A, W, bias=None):
    """A [P, K], W [N, K] (float64, exact fp16 values), bias [N] or None -> (value, sum |a w| (+ |bias|), sum (a w)^2)."""
    ref, ab, sq = R.contract(A, W.t())
    if bias is not None:
        b = bias.double()[None]
        ref, ab = ref + b, ab + b.abs()
    return ref, ab, sq


def linear_bound(ref, ab, sq, K, dtype_out, ksplit=0, emulated_in=None, extra=0.0):
    return R.bound(ref, ab, sq, R.chain_length(K, F16, ksplit), dtype_out, emulated_in, extra)


def linear_gelu_bound(ref, ab, K, dtype_out, ksplit=0):
    """GELU epilogue: the pre-activation (never stored) is off by gamma_n sum |terms|."""
    return gelu_bound(ref, gamma_n(R.chain_length(K, F16, ksplit)) * ab, dtype_out)


def residual_ref(x_old, ref, ab):
    """x += result on the fp32 stream: one more term, one more step (use chain + 1, fp32 output)."""
    return x_old + ref, ab + x_old.abs()


def residual_bound(ref_x, ab_x, sq, K, ksplit=0, emulated_in=None, extra=0.0):
    return R.bound(ref_x, ab_x, sq, R.chain_length(K, F16, ksplit) + 1, F32, emulated_in, extra)


def stats_ref(stored, samples):
    """fp64 sums of the STORED output [samples * V, N] -> (sum, sum of squares, sum |y|) each [samples, N]."""
    y = stored.double().view(samples, -1, stored.shape[-1])
    return y.sum(1), (y * y).sum(1), y.abs().sum(1)


def mlp_ref(ln2, w1, b1, w2, b2, x_old, hidden_fp16=True):
    """x + linear2(fp16(GELU(linear1(ln2)))) on rows ln2 [P, C]; the hidden activation is an emulated input of the second
    product.  Returns (ref, bound)."""
    C = ln2.shape[1]
    pre, _, _ = linear_ref(ln2, w1, b1)
    h = gelu64(pre)
    if hidden_fp16:
        h = f16(h)
    ref, ab, sq = linear_ref(h, w2, b2)
    ref, ab = residual_ref(x_old, ref, ab)
    # a hidden unit below the fp16 normal range moves by one subnormal step (2^-24), not by a relative ulp
    tiny = (h.abs() < 2.0 ** -13).double()
    extra = 2.0 ** -24 * (tiny @ w2.abs().t())
    return ref, residual_bound(ref, ab, sq, 4 * C, emulated_in=F16, extra=extra)


# ---- LayerNorm and the kernels built on it -----------------------------------------------------------------------------------
def ln_chain(cpl, group):
    """fp32 adds of the row sum: a per-lane chain of ``cpl`` values, a butterfly over ``group`` lanes."""
    return cpl + int(math.log2(group))


def layernorm_ref(v, gamma=None, beta=None, eps=1e-5, divisor=None, eps_inside=True):
    """v float64 [P, C] -> (out, parts): biased variance, eps inside the root.  ``divisor`` / ``eps_inside`` exist for the
    planted defects."""
    C = v.shape[1]
    eps = float(np.float32(eps))
    mean = v.mean(1, keepdim=True)
    var = ((v - mean) ** 2).sum(1, keepdim=True) / (divisor or C)
    rstd = 1 / torch.sqrt(var + eps) if eps_inside else 1 / (torch.sqrt(var) + eps)
    g = torch.ones(C, dtype=torch.float64) if gamma is None else gamma.double()
    b = torch.zeros(C, dtype=torch.float64) if beta is None else beta.double()
    if b.dim() == 1:
        b = b[None]
    t = (v - mean) * rstd * g[None]
    return t + b, dict(v=v, mean=mean, var=var, rstd=rstd, g=g[None].abs(), b=b.abs(), t=t.abs(), eps=eps)


def layernorm_bound(out, parts, n_chain, dtype_out):
    v, mean, var, rstd, g, b, t = (parts[k] for k in ("v", "mean", "var", "rstd", "g", "b", "t"))
    C = v.shape[1]
    u_out, floor = R.unit(dtype_out)
    gn = gamma_n(n_chain)
    sa = v.abs().sum(1, keepdim=True)
    e_m = (gn * sa + U_DIV * (v.sum(1, keepdim=True).abs() + gn * sa)) / C
    dev = (v - mean).abs()
    err_d = U32 * dev + e_m * (1 + U32)
    e_v = gn + 2 * U32 + U_DIV + U32 + e_m * e_m / (var + parts["eps"])
    e_v = e_v + e_v * e_v
    e_r = 0.5 * e_v / (1 - e_v) ** 1.5 + U_ULP
    err_t = (dev + err_d) * rstd * (1 + e_r) * g * (1 + U32) ** 2 - dev * rstd * g
    pre = err_t + U32 * (t + err_t + b)
    return pre * (1 + u_out) + u_out * out.abs() + floor


def stream_add_bound(ref):
    """x + y in one fp32 add."""
    return U32 * ref.abs() + R.FLOOR32


def patch_merge_corners(legacy):
    """(di, dj, dk) of the 8 gathered blocks: patch.py:82-89 (legacy: x5 == x2, x6 == x3) or itertools.product order."""
    if legacy:
        return [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (0, 1, 0), (0, 0, 1), (1, 1, 1)]
    return [(i, j, k) for i in range(2) for j in range(2) for k in range(2)]


def patch_merge_gather(x, toks, legacy=True):
    """x [B, D, H, W, C] (any device) -> [P, 8C] float64 CPU rows of the gathered, zero-padded 2x2x2 neighbourhoods of output
    tokens ``toks`` (linear in [B, ceil D/2, ceil H/2, ceil W/2])."""
    B, D, H, W, C = x.shape
    D2, H2, W2 = (D + 1) // 2, (H + 1) // 2, (W + 1) // 2
    t = toks.to(x.device)
    w2, h2, d2, b = t % W2, (t // W2) % H2, (t // (W2 * H2)) % D2, t // (W2 * H2 * D2)
    parts = []
    for di, dj, dk in patch_merge_corners(legacy):
        d, h, w = 2 * d2 + di, 2 * h2 + dj, 2 * w2 + dk
        ok = (d < D) & (h < H) & (w < W)
        val = x[b, d.clamp(max=D - 1), h.clamp(max=H - 1), w.clamp(max=W - 1)]
        parts.append(torch.where(ok[:, None], val, torch.zeros_like(val)))
    return torch.cat(parts, 1).double().cpu()


def patch_merge_chain(C, ntok):
    """(chain, form) of dua_patch_merge_norm (csrc/swin_ops.hip:154): a whole workgroup per token ("wide") when ntok < 2048 and
    8 C % 256 == 0, else one wave per token; per-lane chain of 8 C / lanes values, a 64-lane butterfly, + 2 adds over the waves."""
    wide = ntok < 2048 and (8 * C) % 256 == 0
    return (8 * C // 256 + 6 + 2, "wide") if wide else (-(-8 * C // 64) + 6, "wave")


def attention_form(windows, heads):
    """dua_window_attention_fwd's ``dim3 grid(windows, heads, (long)windows * heads >= 1024 ? 1 : (nb + 3) / 4)``
    (csrc/window_attention.hip): one workgroup per (window, head) from 1024 pairs on, else query blocks split over z."""
    return "one-workgroup" if windows * heads >= 1024 else "split"


# ---- patch_embed ---------------------------------------------------------------------------------------------------------------
def patch_embed_weights(w, cin_packed, dtype):
    """Conv3d(k2, s2) weight [E, Cin, 2, 2, 2] -> float64 [8 * cin_packed, E] in (tap = kd kh kw, channel) order, zero beyond
    Cin, rounded to fp16 for the MFMA form (ops.pack_patch_embed_weights + the kernel's staging)."""
    E, Cin = w.shape[:2]
    wp = torch.zeros(8, cin_packed, E, dtype=torch.float64)
    wp[:, :Cin] = w.detach().double().permute(2, 3, 4, 1, 0).reshape(8, Cin, E)
    wp = wp.reshape(8 * cin_packed, E)
    return f16(wp) if dtype == F16 else wp.float().double()


def patch_embed_rows(xin, toks, cin_packed):
    """xin [B, D, H, W, Cs] (any device) -> float64 CPU [P, 8 * cin_packed]: the 2x2x2 voxels of output tokens ``toks``."""
    B, D, H, W, _ = xin.shape
    D2, H2, W2 = D // 2, H // 2, W // 2
    t = toks.to(xin.device)
    w2, h2, d2, b = t % W2, (t // W2) % H2, (t // (W2 * H2)) % D2, t // (W2 * H2 * D2)
    parts = [xin[b, 2 * d2 + (tap >> 2), 2 * h2 + ((tap >> 1) & 1), 2 * w2 + (tap & 1), :cin_packed] for tap in range(8)]
    return torch.cat(parts, 1).double().cpu()


def patch_embed_ref(A, Wm, bias, tadd_rows):
    """A [P, K], Wm [K, E], bias [E], tadd_rows [P, E] or None -> (stream value, sum |terms|, sum of squares)."""
    ref, ab, sq = R.contract(A, Wm)
    add = bias.double()[None] + (0 if tadd_rows is None else tadd_rows.double())
    ab = ab + bias.double().abs()[None] + (0 if tadd_rows is None else tadd_rows.double().abs())
    return ref + add, ab, sq


def patch_embed_chain(K, dtype):
    """(contraction chain, LayerNorm chain, form)"""
    if dtype == F16:
        return R.chain_length(K, F16) + 1, ln_chain(12, 4), "mfma"
    return R.chain_length(K, F32), ln_chain(48, 1), "fmaf"


# ---- linear_f32 ----------------------------------------------------------------------------------------------------------------
ERFF_ULP = 4                       # HIP math API: erff, maximum ulp error


def gelu_erff_bound(x, e_x):
    """0.5 v (1 + erff(v c)) in fp32, stored as fp32 (module docstring)."""
    z = x.abs() * 0.7071067811865476
    erf = torch.erf(z)
    d_arg = 2 * U32 * z * (2 / math.sqrt(math.pi)) * torch.exp(-z * z)
    g = gelu64(x)
    return 0.5 * x.abs() * (2 * ERFF_ULP * U32 * erf + d_arg + U32 * (1 + erf)) * (1 + 4 * U32) + 2 * U32 * g.abs() + GELU_LIP * e_x + R.FLOOR32


def linear_f32_bound(ref, ab, sq, K, gelu=False):
    n = R.chain_length(K, F32)
    if gelu:
        return gelu_erff_bound(ref, gamma_n(n) * ab)
    return R.bound(ref, ab, sq, n, F32)


# ---- residual_norm_act ---------------------------------------------------------------------------------------------------------
def residual_norm_act_ref(raw, sc, sh, res, rsc=None, rsh=None, slope=0.01, post=None, ra=None, slope32=True):
    """LeakyReLU(raw sc + sh + (res rsc + rsh | res)) [+ post] [+ ra (1 - sigmoid(ra))] in float64 on rows [P, C] with
    per-row constants [P, C] (blocks.py:308-316, denoiser.py:370-408) -> (ref, bound ingredients).  The kernel's slope is
    the fp32 value of ``slope`` (``slope32``; the oracle tie passes False)."""
    sl = float(np.float32(slope)) if slope32 else slope
    y = raw * sc + sh
    mag = (raw * sc).abs() + sh.abs()
    if rsc is not None:
        y = y + res * rsc + rsh
        mag = mag + (res * rsc).abs() + rsh.abs()
    else:
        y = y + res
        mag = mag + res.abs()
    pre = y
    y = torch.where(y > 0, y, y * sl)
    err_ra = torch.zeros_like(y)
    if post is not None:
        y, mag = y + post, mag + post.abs()
    if ra is not None:
        sg = torch.sigmoid(ra)
        t = ra * (1 - sg)
        d_sg = sg * (1 - sg) * (2 + 2 * ra.abs()) * U32 + sg * (U32 + U_DIV)
        err_ra = (ra.abs() * (d_sg + U32 * (1 - sg)) + U32 * t.abs()) * (1 + 4 * U32)
        y, mag = y + t, mag + t.abs()
    return y, dict(mag=mag, err_ra=err_ra, pre=pre, slope=sl)


def residual_norm_act_bound(ref, parts, dtype_out):
    """gamma_6 mag + the reverse-attention term's error; where the pre-activation is within its own rounding of 0 the other
    slope may be taken: (1 - slope) times that margin."""
    u_out, floor = R.unit(dtype_out)
    e_pre = gamma_n(3) * parts["mag"]
    kink = (1 - parts["slope"]) * torch.where(parts["pre"].abs() <= e_pre, e_pre, torch.zeros_like(e_pre))
    b = gamma_n(6) * parts["mag"] + parts["err_ra"] + kink
    return b * (1 + u_out) + u_out * ref.abs() + floor
