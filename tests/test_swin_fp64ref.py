"""The Swin fp64 references and bounds of tests/swin_fp64ref.py, on the CPU: each reference equals the oracle's module in float64;
a torch emulation of the kernels' own arithmetic (fp32 accumulation over fp16 operands, block-wise running maximum with fp16
probabilities, fp32 LayerNorm, fp16 / fp32 stores) passes every bound; every planted defect is rejected on at least one sampled
element (each test asserts ratio > 1, so it fails if its mutation is removed)."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fp64ref as R
import swin_fp64ref as S
from oracle.swin_ref import (RefMlp, RefPatchMerging, RefSwinTransformer, RefUnetResBlock, RefWindowAttention, compute_mask,
                             patch_merging_gather, window_partition, window_reverse)

F16, F32, F64 = torch.float16, torch.float32, torch.float64
L2E = np.float32(1.4426950408889634)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _close(a, b, tol=1e-12):
    return float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max()))


# ---- the references against the oracle ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("heads,ws,dims,shift", [(3, (7, 7, 7), (14, 14, 14), (3, 3, 3)), (24, (6, 6, 6), (6, 6, 6), None),
                                                 (3, (3, 4, 5), (6, 8, 5), (1, 2, 0)), (12, (3, 3, 3), (3, 3, 3), None)])
def test_attention_ref_equals_the_oracle(heads, ws, dims, shift):
    torch.manual_seed(heads)
    att = RefWindowAttention(heads * 16, heads, (7, 7, 7) if max(ws) <= 7 and ws[0] == ws[1] == ws[2] else ws).double()
    with torch.no_grad():
        att.relative_position_bias_table.normal_(0, 0.5)
    B, n = 2, ws[0] * ws[1] * ws[2]
    xw = window_partition(torch.randn(B, *dims, heads * 16, generator=_gen(1), dtype=F64), ws)
    mask = compute_mask(dims, ws, shift).double() if shift is not None else None
    with torch.no_grad():
        qkv = att.qkv(xw)
        want = att.attention_core(qkv, mask)
    Wn = qkv.shape[0]
    wins = torch.arange(Wn).repeat_interleave(heads)
    hs = torch.arange(heads).repeat(Wn)
    t = qkv.view(Wn, n, 3, heads, 16)
    q, k, v = (t[wins, :, i, hs] for i in range(3))
    table_t = att.relative_position_bias_table.detach().t().contiguous()
    if att.window_size == (7, 7, 7):
        bias = S.table_bias(table_t, hs, n, (7, 7, 7))
    else:
        bias = att.bias(n).detach()[hs]
    m = None
    if shift is not None:
        reg = S.region_ids(dims, ws, shift)
        m = S.region_mask(reg, wins, mask.shape[0])
        assert torch.equal(m, mask[wins % mask.shape[0]])
    r = S.attention_ref(q, k, v, bias, m)
    got = r["out"].view(Wn, heads, n, 16).permute(0, 2, 1, 3).reshape(Wn, n, heads * 16)
    assert _close(got, want)


def test_layernorm_family_refs_equal_the_oracle():
    g = _gen(2)
    B, dims, C, ws, ss = 2, (9, 8, 10), 48, (7, 7, 7), (3, 3, 3)
    x = torch.randn(B, *dims, C, generator=g, dtype=F64)
    g1, b1 = torch.randn(C, generator=g, dtype=F64), torch.randn(C, generator=g, dtype=F64)
    pad = [(ws[i] - dims[i] % ws[i]) % ws[i] for i in range(3)]
    n1 = F.pad(F.layer_norm(x, [C], g1, b1), (0, 0, 0, pad[2], 0, pad[1], 0, pad[0]))
    want = window_partition(torch.roll(n1, shifts=tuple(-s for s in ss), dims=(1, 2, 3)), ws).reshape(-1, C)
    tm = S.window_token_map(B, dims, ws, ss)
    out, _ = S.layernorm_ref(x.view(-1, C)[tm.clamp(min=0)], g1, b1)
    out = torch.where((tm >= 0)[:, None], out, torch.zeros_like(out))
    assert _close(out, want)
    # the way back: window_reverse -> roll(+shift) -> crop == scatter through the same map
    yw = torch.randn(want.shape, generator=g, dtype=F64)
    dp = [dims[i] + pad[i] for i in range(3)]
    back = torch.roll(window_reverse(yw.view(-1, 343, C), ws, [B, *dp]), shifts=ss, dims=(1, 2, 3))[:, :dims[0], :dims[1], :dims[2]]
    mine = torch.zeros(B * dims[0] * dims[1] * dims[2], C, dtype=F64)
    mine[tm[tm >= 0]] = yw[tm >= 0]
    assert _close(mine, back.reshape(-1, C))
    # proj_out (stage_out: no affine) and PatchMerging (legacy and not, odd extents)
    xs = torch.randn(2, 48, 3, 4, 5, generator=g, dtype=F64)
    want2 = RefSwinTransformer.proj_out(xs, True).permute(0, 2, 3, 4, 1).reshape(-1, 48)
    assert _close(S.layernorm_ref(xs.permute(0, 2, 3, 4, 1).reshape(-1, 48))[0], want2)
    for legacy in (True, False):
        xm = torch.randn(2, 5, 6, 7, 16, generator=g, dtype=F64)
        pm = RefPatchMerging(16, legacy=legacy).double()
        with torch.no_grad():
            pm.norm.weight.normal_(1, 0.3); pm.norm.bias.normal_(0, 0.3)
            want3 = pm.norm(patch_merging_gather(xm, legacy)).reshape(-1, 128)
        rows = S.patch_merge_gather(xm, torch.arange(want3.shape[0]), legacy)
        assert _close(S.layernorm_ref(rows, pm.norm.weight.detach(), pm.norm.bias.detach())[0], want3)


def test_mlp_ref_equals_the_oracles_mlp_block():
    g = _gen(3)
    C = 48
    torch.manual_seed(3)
    mlp = RefMlp(C, 4 * C).double()
    ln2, x0 = torch.randn(50, C, generator=g, dtype=F64), torch.randn(50, C, generator=g, dtype=F64)
    with torch.no_grad():
        want = x0 + mlp(ln2)
    got, _ = S.mlp_ref(ln2, mlp.linear1.weight.detach(), mlp.linear1.bias.detach(), mlp.linear2.weight.detach(),
                       mlp.linear2.bias.detach(), x0, hidden_fp16=False)
    assert _close(got, want)


def test_patch_embed_ref_equals_the_oracle_and_accepts_the_emulation():
    g = _gen(4)
    B, D, H, W, cin, cp, E = 2, 6, 4, 8, 17, 24, 48
    torch.manual_seed(4)
    conv = torch.nn.Conv3d(cin, E, 2, 2).double()
    x = torch.randn(B, cin, D, H, W, generator=g, dtype=F64)
    tadd = torch.randn(B, E, generator=g, dtype=F64)
    with torch.no_grad():
        x0 = conv(x) + tadd[:, :, None, None, None]
        want_x = x0.permute(0, 2, 3, 4, 1).reshape(-1, E)
        want_ln = RefSwinTransformer.proj_out(x0, True).permute(0, 2, 3, 4, 1).reshape(-1, E)
    xin = torch.zeros(B, D, H, W, 32, dtype=F64)
    xin[..., :cin] = x.permute(0, 2, 3, 4, 1)
    toks = torch.arange(want_x.shape[0])
    per = (D // 2) * (H // 2) * (W // 2)
    A = S.patch_embed_rows(xin, toks, cp)
    Wm = torch.zeros(8, cp, E, dtype=F64)
    Wm[:, :cin] = conv.weight.detach().permute(2, 3, 4, 1, 0).reshape(8, cin, E)
    ref, _, _ = S.patch_embed_ref(A, Wm.reshape(8 * cp, E), conv.bias.detach(), tadd[toks // per])
    assert _close(ref, want_x) and _close(S.layernorm_ref(ref)[0], want_ln)
    # both forms' arithmetic: fp16 operands with fp32 accumulation; fp32 operands
    for dtype in (F16, F32):
        xq = xin.to(dtype)
        Wq = S.patch_embed_weights(conv.weight, cp, dtype)
        Aq = S.patch_embed_rows(xq, toks, cp)
        ref, ab, sq = S.patch_embed_ref(Aq, Wq, conv.bias.detach().float(), tadd.float()[toks // per])
        n, n_ln, _ = S.patch_embed_chain(8 * cp, dtype)
        emu = Aq.float() @ Wq.float() + (conv.bias.detach().float()[None] + tadd.float()[toks // per])
        cx = R.check(emu, ref, R.bound(ref, ab, sq, n, F32))
        emb = torch.randn(ref.shape, generator=g).to(dtype)
        lref, parts = S.layernorm_ref(emu.double(), None, emb.double())
        cl = R.check((_emulate_ln(emu, torch.ones(E), emb.float())).to(dtype), lref, S.layernorm_bound(lref, parts, n_ln, dtype))
        print(f"patch_embed {dtype}: stream {cx}\n  norm {cl}")
        assert cx.ratio <= 1.0 and cl.ratio <= 1.0
        bad = emu.clone()
        prod = Aq.float()[3] * Wq.float()[:, 0]
        bad[3, 0] -= prod[prod.abs().argmax()]
        assert R.check(bad, ref, R.bound(ref, ab, sq, n, F32)).ratio > 1.0


def _sums(t):
    """[N, C, 2] (sum, sum of squares) of a channels-first tensor, as stats_decode returns them."""
    f = t.double().flatten(2)
    return torch.stack([f.sum(2), (f * f).sum(2)], 2)


@pytest.mark.parametrize("second_norm", [True, False])
def test_residual_norm_act_ref_equals_the_oracle_and_rejects_defects(second_norm):
    """The tail of RefUnetResBlock.forward: lrelu(norm2(conv2 out) + (norm3(conv3 out) | input))."""
    g = _gen(6)
    N, C, dims = 2, 16, (4, 6, 5)
    blk = RefUnetResBlock(8 if second_norm else C, C, affine=True).double()
    with torch.no_grad():
        for m in (blk.norm2,) + ((blk.norm3,) if second_norm else ()):
            m.weight.normal_(1.0, 0.3); m.bias.normal_(0.0, 0.3)
    a = torch.randn(N, C, *dims, generator=g).half()
    r = torch.randn(N, C, *dims, generator=g).half()
    V = dims[0] * dims[1] * dims[2]
    with torch.no_grad():
        want = blk.lrelu(blk.norm2(a.double()) + (blk.norm3(r.double()) if second_norm else r.double()))
    rows = lambda t: t.double().permute(0, 2, 3, 4, 1).reshape(-1, C)
    per = lambda c: c.repeat_interleave(V, 0)
    sc, sh, _, _ = R.finalize(_sums(a), blk.norm2.weight.detach(), blk.norm2.bias.detach(), V)
    rsc = rsh = None
    if second_norm:
        rsc, rsh, _, _ = R.finalize(_sums(r), blk.norm3.weight.detach(), blk.norm3.bias.detach(), V)
        rsc, rsh = per(rsc), per(rsh)
    ref, parts = S.residual_norm_act_ref(rows(a), per(sc), per(sh), rows(r), rsc, rsh, 0.01, slope32=False)
    assert _close(ref, rows(want), 1e-11)                     # eps is the kernels' fp32 1e-5 in R.finalize: 2.5e-13 of var + eps
    # the kernel's arithmetic on fp32 constants, with the denoiser's two adds
    post, ra = torch.randn(ref.shape, generator=g).half(), (3 * torch.randn(ref.shape, generator=g)).half()
    c32 = [None if t is None else t.float() for t in (per(sc), per(sh), rsc, rsh)]
    ref, parts = S.residual_norm_act_ref(rows(a), c32[0].double(), c32[1].double(), rows(r), None if rsc is None else c32[2].double(),
                                         None if rsc is None else c32[3].double(), 0.01, post.double(), ra.double())
    bnd = S.residual_norm_act_bound(ref, parts, F16)

    def emulate(norm_res=second_norm, slope=0.01):
        y = rows(a).float() * c32[0] + c32[1]
        y = y + (rows(r).float() * c32[2] + c32[3] if norm_res else rows(r).float())
        y = torch.where(y > 0, y, y * np.float32(slope)) + post.float()
        s_ = ra.float()
        return (y + s_ * (1 - 1 / (1 + torch.exp(-s_)))).half()

    ok = R.check(emulate(), ref, bnd)
    print(f"residual_norm_act second norm {second_norm}: emulation {ok}")
    assert ok.ratio <= 1.0
    assert R.check(emulate(slope=0.1), ref, bnd).ratio > 1.0                        # the other block family's slope
    if second_norm:
        assert R.check(emulate(norm_res=False), ref, bnd).ratio > 1.0               # norm3 skipped


def test_linear_f32_bound_accepts_an_fp32_chain_and_rejects_a_dropped_product():
    g = _gen(8)
    M, K, N = 216, 768, 96
    A, W, b = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) / K ** 0.5, torch.randn(N, generator=g)
    ref, ab, sq = S.linear_ref(A.double(), W.double(), b)
    pre = A @ W.t() + b[None]
    assert R.check(pre, ref, S.linear_f32_bound(ref, ab, sq, K)).ratio <= 1.0
    gel = F.gelu(pre)
    assert R.check(gel, S.gelu64(ref), S.linear_f32_bound(ref, ab, sq, K, gelu=True)).ratio <= 1.0
    bad = _drop_largest_product(pre, A, W, [5])
    assert R.check(bad, ref, S.linear_f32_bound(ref, ab, sq, K)).ratio > 1.0
    assert R.check(F.gelu(bad), S.gelu64(ref), S.linear_f32_bound(ref, ab, sq, K, gelu=True)).ratio > 1.0
    # the K + 1 worst-case chain is wide at K = 768 (769 U32 sum |a w|); the GELU form is told apart at the plan's K = 48
    A, W = 2 * torch.randn(M, 48, generator=g), torch.randn(N, 48, generator=g) / 48 ** 0.5
    ref, ab, sq = S.linear_ref(A.double(), W.double(), b)
    pre = A @ W.t() + b[None]
    assert R.check(F.gelu(pre), S.gelu64(ref), S.linear_f32_bound(ref, ab, sq, 48, gelu=True)).ratio <= 1.0
    assert R.check(_tanh_gelu(pre), S.gelu64(ref), S.linear_f32_bound(ref, ab, sq, 48, gelu=True)).ratio > 1.0


def test_gelu_polynomial_error_is_what_the_bound_assumes():
    """Abramowitz-Stegun 7.1.26 in float64 against torch.erf on 4e6 points of [-12, 12]: within the documented 1.5e-7; the same
    formula in fp32 exceeds it several times over (the rounding terms the bound derives), and stays inside the bound."""
    x = torch.linspace(-12, 12, 4_000_001, dtype=F64)
    z = x.abs() * 0.7071067811865476
    erf_as = S.as_erf64(z)[0]
    err = (erf_as - torch.erf(z)).abs().max()
    print(f"A-S 7.1.26 in float64: max |erf_AS - erf| = {float(err):.3e}")
    assert float(err) <= S.AS_ERR
    got = S.gelu_erf_emulated(x.float()).double()
    xr = x.float().double()
    e32 = (got - S.gelu64(xr)).abs()
    rel = (e32 / (0.5 * xr.abs()).clamp_min(1e-30))[xr.abs() > 1e-3].max()
    print(f"the same in fp32: max |err| / (0.5 |x|) = {float(rel):.3e}")
    assert float(rel) > S.AS_ERR                      # the approximation term alone would not cover fp32
    c = R.check(got, S.gelu64(xr), S.gelu_bound(xr, torch.zeros_like(xr), F32))
    print("fp32 emulation against the bound:", c)
    assert c.ratio <= 1.0
    tail = xr < -6                                     # the error is absolute: beyond the value itself in the far tail
    assert bool((S.gelu_bound(xr, torch.zeros_like(xr), F32)[tail] > S.gelu64(xr)[tail].abs()).all())


# ---- contractions: emulation accepted, defects rejected -----------------------------------------------------------------------
def _linear_case(M, K, N, seed):
    g = _gen(seed)
    A = torch.randn(M, K, generator=g).half()
    W = (torch.randn(N, K, generator=g) / K ** 0.5).half()
    b = torch.randn(N, generator=g)
    return A, W, b


def _emulate_linear(A, W, b, ksplit=1, drop=None, twice=None):
    K = A.shape[1]
    kper = -(-(-(-K // 64)) // ksplit) * 64
    acc = b.clone()[None].repeat(A.shape[0], 1) if ksplit > 1 else None
    parts = []
    for s in range(-(-K // kper)):
        sl = slice(s * kper, min(K, (s + 1) * kper))
        parts.append(A[:, sl].float() @ W[:, sl].float().t())
    if ksplit == 1:
        return parts[0] + b[None]
    for s, p_ in enumerate(parts):
        if s == drop:
            continue
        acc = acc + p_
        if s == twice:
            acc = acc + p_
    return acc


def _drop_largest_product(pre, A, W, rows):
    """pre [M, N] fp32 minus the largest product of each of ``rows``' column 0 .. (as test_fp64ref.py does)."""
    out = pre.clone()
    for r_ in rows:
        prod = A[r_].float() * W[0].float()
        out[r_, 0] -= prod[prod.abs().argmax()]
    return out


@pytest.mark.parametrize("M,K,N,ksplit", [(300, 384, 96, 1), (343, 3072, 768, 8), (27, 3072, 768, 16), (200, 72, 96, 1)])
def test_linear_bounds_accept_the_emulation_and_reject_defects(M, K, N, ksplit):
    A, W, b = _linear_case(M, K, N, K + M)
    rows = S.sample_rows(M, 64, seed=1)
    ref, ab, sq = S.linear_ref(A[rows].double(), W.double(), b)
    ks = ksplit if ksplit > 1 else 0
    bnd = S.linear_bound(ref, ab, sq, K, F16, ks)
    pre = _emulate_linear(A, W, b, ksplit)
    ok = R.check(pre.half()[rows], ref, bnd)
    print(f"{M}x{K}->{N} split {ksplit}: emulation {ok}")
    assert ok.ratio <= 1.0
    # GELU and residual epilogues on the same pre-activation
    okg = R.check(S.gelu_erf_emulated(pre).half()[rows], S.gelu64(ref), S.linear_gelu_bound(ref, ab, K, F16, ks))
    x0 = torch.randn(M, N, generator=_gen(5))
    rx, abx = S.residual_ref(x0[rows].double(), ref, ab)
    okr = R.check((x0 + pre)[rows], rx, S.residual_bound(rx, abx, sq, K, ks))
    assert okg.ratio <= 1.0 and okr.ratio <= 1.0, (okg, okr)
    # one dropped product (the largest of its row), in the fp16 output and in the fp32 stream
    bad = _drop_largest_product(pre, A, W, rows.tolist())
    assert R.check(bad.half()[rows], ref, bnd).ratio > 1.0
    assert R.check((x0 + bad)[rows], rx, S.residual_bound(rx, abx, sq, K, ks)).ratio > 1.0
    # the bias of the neighbouring output channel
    nb_ = (pre - b[None] + torch.roll(b, 1)[None])
    assert R.check(nb_.half()[rows], ref, bnd).ratio > 1.0
    if ksplit > 1:
        assert R.check(_emulate_linear(A, W, b, ksplit, drop=ksplit // 2).half()[rows], ref, bnd).ratio > 1.0
        assert R.check(_emulate_linear(A, W, b, ksplit, twice=1).half()[rows], ref, bnd).ratio > 1.0


def _tanh_gelu(x):
    return 0.5 * x * (1 + torch.tanh(0.7978845608028654 * (x + 0.044715 * x ** 3)))


def test_gelu_bound_rejects_the_tanh_form():
    A, W, b = _linear_case(400, 96, 384, 9)
    A = (A.float() * 2.5).half()                              # pre-activations out to +-8: both tails
    ref, ab, _ = S.linear_ref(A.double(), W.double(), b)
    pre = _emulate_linear(A, W, b)
    bnd = S.linear_gelu_bound(ref, ab, 96, F16)
    assert R.check(S.gelu_erf_emulated(pre).half(), S.gelu64(ref), bnd).ratio <= 1.0
    assert float(ref.min()) < -6 and float(ref.max()) > 6
    assert R.check(_tanh_gelu(pre).half(), S.gelu64(ref), bnd).ratio > 1.0


def test_mlp_bound_accepts_fp16_and_fp32_hidden_and_rejects_a_dropped_product():
    g = _gen(11)
    C, M = 96, 333
    ln2 = (torch.randn(M, C, generator=g) * 1.5).half()
    w1, w2 = (torch.randn(4 * C, C, generator=g) / C ** 0.5).half(), (torch.randn(C, 4 * C, generator=g) / (4 * C) ** 0.5).half()
    b1, b2, x0 = torch.randn(4 * C, generator=g), torch.randn(C, generator=g), torch.randn(M, C, generator=g)
    ref, bnd = S.mlp_ref(ln2.double(), w1.double(), b1, w2.double(), b2, x0.double())
    h32 = S.gelu_erf_emulated(ln2.float() @ w1.float().t() + b1[None])
    out16 = x0 + (h32.half().float() @ w2.float().t() + b2[None])
    out32 = x0 + (h32 @ w2.float().t() + b2[None])            # hidden kept in fp32: closer to the reference, must still pass
    a, b_ = R.check(out16, ref, bnd), R.check(out32, ref, bnd)
    print("mlp fp16 hidden:", a, "\nmlp fp32 hidden:", b_)
    assert a.ratio <= 1.0 and b_.ratio <= 1.0
    bad = out16.clone()
    prod = h32.half().float()[7] * w2.float()[0]
    bad[7, 0] -= prod[prod.abs().argmax()]
    assert R.check(bad, ref, bnd).ratio > 1.0


# ---- LayerNorm: emulation accepted, defects rejected ----------------------------------------------------------------------------
def _ln_rows(C, seed):
    """Rows of ordinary, low-variance (std 0.01) and high-mean (100 +- 0.3) tokens."""
    g = _gen(seed)
    v = torch.randn(96, C, generator=g)
    v[32:64] *= 0.01
    v[64:] = 100 + 0.3 * v[64:]
    return v


def _emulate_ln(v32, gamma, beta, eps=1e-5, div=None, eps_inside=True):
    C = v32.shape[1]
    mean = v32.sum(1, keepdim=True) / C
    d = v32 - mean
    var = (d * d).sum(1, keepdim=True) / np.float32(div or C)
    rstd = 1 / torch.sqrt(var + np.float32(eps)) if eps_inside else 1 / (torch.sqrt(var) + np.float32(eps))
    return d * rstd * gamma[None] + beta[None]


@pytest.mark.parametrize("C,dtype", [(48, F16), (384, F16), (768, F32), (3072, F16)])
def test_layernorm_bound_accepts_the_emulation_and_rejects_defects(C, dtype):
    v = _ln_rows(C, C)
    g = _gen(C + 1)
    gamma, beta = 1 + 0.3 * torch.randn(C, generator=g), 0.3 * torch.randn(C, generator=g)
    ref, parts = S.layernorm_ref(v.double(), gamma, beta)
    n = S.ln_chain(12, max(C // 12, 4)) if C <= 768 else S.patch_merge_chain(C // 8, 27)[0]
    bnd = S.layernorm_bound(ref, parts, n, dtype)
    ok = R.check(_emulate_ln(v, gamma, beta).to(dtype), ref, bnd)
    print(f"LayerNorm C {C} {dtype}: emulation {ok}")
    assert ok.ratio <= 1.0
    assert R.check(_emulate_ln(v, gamma, beta, div=C - 1).to(dtype), ref, bnd).ratio > 1.0
    assert R.check(_emulate_ln(v, gamma, beta, eps_inside=False).to(dtype), ref, bnd).ratio > 1.0
    # the high-mean rows: the bound stays relative to |v - mean| rstd up to the e_m rstd term (no |mean|^2 term)
    # (derived: gamma_n (1 + U_DIV) |mean| rstd |gamma| for the mean, the same again at most for everything relative to
    # |v - mean| rstd |gamma| <= a few units, plus the output rounding -- nothing of the order |mean|^2 rstd^2 U32 = 7e-3)
    rs, gmax = float(parts["rstd"][64:].max()), float(gamma.abs().max())
    lim = 2 * S.gamma_n(n) * (1 + S.U_DIV) * 100.3 * rs * gmax + 2 * R.unit(dtype)[0] * float(ref[64:].abs().max() + 1)
    assert float(bnd[64:].max()) < lim, (float(bnd[64:].max()), lim)


def test_mean_taken_before_the_pending_update_is_rejected():
    g = _gen(21)
    C = 96
    x, y = torch.randn(64, C, generator=g), (0.1 * torch.randn(64, C, generator=g)).half()
    gamma, beta = 1 + 0.3 * torch.randn(C, generator=g), 0.3 * torch.randn(C, generator=g)
    v = x + y.float()
    ref, parts = S.layernorm_ref(v.double(), gamma, beta)
    bnd = S.layernorm_bound(ref, parts, S.ln_chain(12, 8), F16)
    assert R.check(_emulate_ln(v, gamma, beta).half(), ref, bnd).ratio <= 1.0
    mean_old = x.sum(1, keepdim=True) / C
    d = v - mean_old
    bad = d * (1 / torch.sqrt((d * d).sum(1, keepdim=True) / C + np.float32(1e-5))) * gamma[None] + beta[None]
    assert R.check(bad.half(), ref, bnd).ratio > 1.0


def test_geometry_defects_are_rejected():
    """Roll with the wrong sign, crop omitted at a padded border (49 -> 48), patch-merge duplicates in non-legacy order."""
    g = _gen(23)
    B, dims, C, ws, ss = 1, (8, 9, 10), 48, (7, 7, 7), (3, 3, 3)
    x = torch.randn(B * 8 * 9 * 10, C, generator=g)
    gamma, beta = 1 + 0.3 * torch.randn(C, generator=g), 0.3 * torch.randn(C, generator=g)
    tm = S.window_token_map(B, dims, ws, ss)
    rows = S.sample_rows(tm.numel(), 400, seed=2, window=343)

    def gathered(tmap):
        o = _emulate_ln(x[tmap.clamp(min=0)], gamma, beta).half()
        return torch.where((tmap >= 0)[:, None], o, torch.zeros_like(o))[rows]

    ref, parts = S.layernorm_ref(x.double()[tm.clamp(min=0)][rows], gamma, beta)
    real = (tm >= 0)[rows][:, None]
    ref = torch.where(real, ref, torch.zeros_like(ref))
    bnd = torch.where(real, S.layernorm_bound(ref, parts, S.ln_chain(12, 4), F16), torch.full_like(ref, R.FLOOR16))
    assert R.check(gathered(tm), ref, bnd).ratio <= 1.0
    assert R.check(gathered(S.window_token_map(B, dims, ws, ss, roll_sign=1)), ref, bnd).ratio > 1.0
    assert R.check(gathered(S.window_token_map(B, dims, ws, ss, crop=False)), ref, bnd).ratio > 1.0
    xm = torch.randn(1, 6, 6, 6, 48, generator=g)
    toks = torch.arange(27)
    gm, bt = 1 + 0.3 * torch.randn(384, generator=g), 0.3 * torch.randn(384, generator=g)
    ref, parts = S.layernorm_ref(S.patch_merge_gather(xm, toks, True), gm, bt)
    n, form = S.patch_merge_chain(48, 27)
    assert form == "wave" and S.patch_merge_chain(96, 27)[1] == "wide"
    bnd = S.layernorm_bound(ref, parts, n, F16)
    assert R.check(_emulate_ln(S.patch_merge_gather(xm, toks, True).float(), gm, bt).half(), ref, bnd).ratio <= 1.0
    assert R.check(_emulate_ln(S.patch_merge_gather(xm, toks, False).float(), gm, bt).half(), ref, bnd).ratio > 1.0


# ---- attention: emulation accepted, defects rejected ------------------------------------------------------------------------
def _emulate_attention(q, k, v, bias, mask, out_dtype, pad_leak=False):
    """The kernel's order in torch fp32: 32-key blocks, running maximum, fp16 probabilities, one division; q, k, v fp16 [P, n, 16],
    bias / mask fp32 [P, n, n] (query, key)."""
    P, n, _ = q.shape
    nb = -(-n // 32)
    qs = (q.float() * 0.25).half().float()
    z = bias + qs @ k.float().transpose(1, 2)
    if mask is not None:
        z = z + mask
    npad = nb * 32 - n
    z = F.pad(z, (0, npad), value=0.0 if pad_leak else -3.0e38)
    vp = F.pad(v.float(), (0, 0, 0, npad))
    mx = torch.full((P, n, 1), -3.0e38)
    O, Dn = torch.zeros(P, n, 16), torch.zeros(P, n, 1)
    for b in range(nb):
        zb = z[:, :, 32 * b:32 * b + 32]
        mnew = torch.maximum(mx, zb.max(-1, keepdim=True).values)
        alpha = torch.exp2((mx - mnew) * L2E)
        mx = mnew
        p = torch.exp2(zb * L2E + (-mnew * L2E)).half().float()
        O = O * alpha + p @ vp[:, 32 * b:32 * b + 32]
        Dn = Dn * alpha + p.sum(-1, keepdim=True)
    return (O * (1 / Dn)).to(out_dtype)


def _attn_case(n, heads, seed):
    g = _gen(seed)
    return tuple(torch.randn(2 * heads, n, 16, generator=g).half() for _ in range(3))


@pytest.mark.parametrize("n,scale,dtype", [(343, 1.0, F16), (343, 3.0, F32), (216, 2.0, F16), (60, 1.0, F16), (27, 3.0, F16), (6, 1.0, F32)])
def test_attention_bound_accepts_the_emulation(n, scale, dtype):
    q, k, v = _attn_case(n, 3, n)
    bias = 0.5 * torch.randn(6, n, n, generator=_gen(n + 1))
    q = (q.float() * scale).half()
    r = S.attention_ref(q.double(), k.double(), v.double(), bias.double())
    c = R.check(_emulate_attention(q, k, v, bias, None, dtype), r["out"], S.attention_bound(r, dtype))
    print(f"attention n {n} scale {scale} {dtype}: emulation {c}")
    assert c.ratio <= 1.0


def test_attention_bound_covers_a_maximum_that_rises_in_every_block():
    n = 343
    q, k, v = _attn_case(n, 1, 77)
    bias = torch.linspace(-30, 30, n)[None, None, :].repeat(2, n, 1).contiguous()      # keys ordered by increasing score
    r = S.attention_ref(q.double(), k.double(), v.double(), bias.double())
    c = R.check(_emulate_attention(q, k, v, bias, None, F16), r["out"], S.attention_bound(r, F16))
    print("rising maximum:", c)
    assert c.ratio <= 1.0


def _shifted_case():
    """Two images of 8 shifted 7^3 windows, table bias, region mask: the production operands in miniature (one head)."""
    dims, ws, ss = (14, 14, 14), (7, 7, 7), (3, 3, 3)
    reg = S.region_ids(dims, ws, ss)
    wins = torch.arange(16)
    g = _gen(31)
    q, k, v = (torch.randn(16, 343, 16, generator=g).half() for _ in range(3))
    table_t = 0.5 * torch.randn(1, 2197, generator=g)
    hs = torch.zeros(16, dtype=torch.int64)
    return reg, wins, q, k, v, table_t, hs


def test_attention_bound_rejects_planted_defects():
    reg, wins, q, k, v, table_t, hs = _shifted_case()
    bias = S.table_bias(table_t, hs, 343)
    mask = S.region_mask(reg, wins, 8)
    r = S.attention_ref(q.double(), k.double(), v.double(), bias, mask)
    bnd = S.attention_bound(r, F16)

    def ratio(bias_=bias, mask_=mask, **kw):
        return R.check(_emulate_attention(q, k, v, bias_.float(), mask_.float(), F16, **kw), r["out"], bnd).ratio

    assert ratio() <= 1.0
    assert ratio(pad_leak=True) > 1.0                                        # a padding key enters the softmax with score 0
    assert ratio(bias_=S.table_bias(table_t, hs, 343, transpose=True)) > 1.0  # bias read as [q][k] instead of [k][q]
    wrong = S.region_mask(reg, torch.where(wins >= 8, wins + 1, wins), 8)    # second image: another window's mask row
    assert ratio(mask_=wrong) > 1.0
    nocmp = mask.clone()
    nocmp[:, :, 32:64] = 0.0                                                  # region compare dropped for one key block
    assert ratio(mask_=nocmp) > 1.0


def test_attention_bound_rejects_a_clipped_window_indexed_through_its_own_grid():
    g = _gen(41)
    n = 216
    q, k, v = (torch.randn(4, n, 16, generator=g).half() for _ in range(3))
    table_t = 0.5 * torch.randn(4, 2197, generator=g)
    hs = torch.arange(4)
    bias = S.table_bias(table_t, hs, n, (7, 7, 7))
    r = S.attention_ref(q.double(), k.double(), v.double(), bias)
    bnd = S.attention_bound(r, F16)
    assert R.check(_emulate_attention(q, k, v, bias.float(), None, F16), r["out"], bnd).ratio <= 1.0
    own = S.table_bias(table_t, hs, n, (7, 7, 7), own_grid=(6, 6, 6))
    assert R.check(_emulate_attention(q, k, v, own.float(), None, F16), r["out"], bnd).ratio > 1.0


# ---- the sampler ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,bounds,window", [(1000, (), None), (3000, (1500,), None), (110592, (), 343), (27, (), 27), (2 * 2744, (2744,), 343)])
def test_structured_rows_are_sampled(M, bounds, window):
    rows = set(S.sample_rows(M, 128, seed=3, boundaries=bounds, window=window).tolist())
    assert {0, M - 1} <= rows and all(0 <= r < M for r in rows)
    for t in (32, 64, 128):
        nt = -(-M // t)
        edges = [k for k in range(1, nt) if nt <= 32 or k < 5 or k >= nt - 4]
        assert all(k * t - 1 in rows and k * t in rows for k in edges), t
        assert (nt - 1) * t in rows                                           # the last (partial) tile's first row
    for b in bounds:
        assert b - 1 in rows and b in rows
    if window:
        assert {window - 1, M - window} <= rows
    assert len(rows) > len(S.structured_rows(M, boundaries=bounds, window=window)) or M <= 128
