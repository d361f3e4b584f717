"""The Swin kernels (BASELINE config 5) against the fp64 references and derived bounds of tests/swin_fp64ref.py, on the GPU,
through diff_unet_amos_amd.ops: every sampled element must satisfy |got - ref| <= bound (no exclusions).  Shapes are the ones
swin_engine's plan issues for feature size 48 on a 96^3 patch (token grids 48 / 24 / 12 / 6 / 3, C = 48 / 96 / 192 / 384 / 768,
heads 3 / 6 / 12 / 24) plus the edges the kernels handle specially; every table names the dispatch form a case takes and the test
asserts it (from dua_token_gemm_workspace, or from the dispatch predicate restated in swin_fp64ref with its source line), so a
policy change fails the test instead of moving coverage.
"""
import os

import pytest
import torch

import fp64ref as R
import swin_fp64ref as S

pytestmark = pytest.mark.gpu
F16, F32 = torch.float16, torch.float32
DEV = "cuda"
torch.set_num_threads(min(16, len(os.sched_getaffinity(0))))


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _report(entry, case, form, shape, nsamp, c):
    print(f"{entry:24s} {case:34s} {form:14s} {str(shape):26s} samples {nsamp:8d}  err/bound {c.ratio:6.3f} at {c.where}")
    assert c.ratio <= 1.0, (entry, case, c)


# ---- window_attention ------------------------------------------------------------------------------------------------------
# name, B, dims, window (clipped), shift or None, heads, dtype, operands, form (dua_window_attention_fwd's grid: windows * heads >= 1024 ? 1 : ...)
ATTN = [
    ("stage 0 as shipped", 1, (48, 48, 48), (7, 7, 7), (3, 3, 3), 3, F16, "table+region", "one-workgroup"),
    ("stage 0 batch 2", 2, (48, 48, 48), (7, 7, 7), (3, 3, 3), 3, F16, "table+region", "one-workgroup"),
    ("stage 0 fp32 input", 1, (48, 48, 48), (7, 7, 7), (3, 3, 3), 3, F32, "table+region", "one-workgroup"),
    ("stage 1", 1, (24, 24, 24), (7, 7, 7), (3, 3, 3), 6, F16, "table+region", "split"),
    ("stage 1 fp32 dense", 1, (24, 24, 24), (7, 7, 7), (3, 3, 3), 6, F32, "dense+dense", "split"),
    ("64x96x32 stage 2", 1, (8, 12, 4), (7, 7, 4), (3, 3, 0), 12, F16, "table+region", "split"),
    ("6^3 clipped, 24 heads", 2, (6, 6, 6), (6, 6, 6), None, 24, F16, "table", "split"),
    ("3^3 single partial block", 2, (3, 3, 3), (3, 3, 3), None, 24, F16, "table", "split"),
    ("n = 60 (3, 4, 5)", 2, (6, 8, 5), (3, 4, 5), (1, 2, 0), 3, F16, "dense+dense", "split"),
    ("n = 6", 2, (2, 4, 3), (1, 2, 3), None, 6, F32, "dense", "split"),
    ("maximum rises every block", 2, (7, 7, 7), (7, 7, 7), None, 3, F16, "rising", "split"),
    ("own region in last block", 2, (7, 7, 7), (7, 7, 7), None, 3, F16, "last-block-region", "split"),
]


@pytest.mark.parametrize("case", ATTN, ids=[c[0] for c in ATTN])
def test_window_attention(case):
    from diff_unet_amos_amd import ops
    name, B, dims, ws, ss, heads, dtype, operands, form = case
    n = ws[0] * ws[1] * ws[2]
    nw = 1
    for i in range(3):
        nw *= -(-dims[i] // ws[i])
    Wn, C = B * nw, heads * 16
    assert S.attention_form(Wn, heads) == form
    g = _gen(len(name) + n)
    qkv = torch.randn(Wn, n, 3 * C, generator=g)
    table_t = 0.5 * torch.randn(heads, 2197, generator=g)
    reg = dense_b = dense_m = None
    if ss is not None:
        reg = S.region_ids(dims, ws, ss)
    if operands == "last-block-region":                       # queries 320.. see only the keys of the last, partial block
        reg = torch.zeros(1, n, dtype=torch.uint8)
        reg[0, 320:] = 1
    if operands.startswith("dense"):
        dense_b = 0.5 * torch.randn(heads, n, n, generator=g)                                  # [head][q][k]
    if operands == "rising":                                  # keys ordered by increasing score, |score| up to ~30
        dense_b = torch.linspace(-30, 30, n)[None, None, :].repeat(heads, n, 1).contiguous()
    if operands == "dense+dense":
        dense_m = S.region_mask(reg, torch.arange(nw), nw).float()                             # [window][q][k]
    qd = qkv.to(dtype).to(DEV).contiguous()
    kw = {}
    if dense_b is None:
        kw.update(bias_table=table_t.to(DEV), table_grid=(7, 7, 7))
    if dense_m is not None:
        kw.update(mask_t=dense_m.transpose(1, 2).contiguous().to(DEV), windows_per_image=nw)
    elif reg is not None:
        kw.update(region_ids=reg.to(DEV), windows_per_image=reg.shape[0])
    out = ops.window_attention(qd, heads, None if dense_b is None else dense_b.transpose(1, 2).contiguous().to(DEV), **kw)
    torch.cuda.synchronize()
    assert out.dtype == dtype
    # (window, head) pairs: first / last window of every image, the last windows along each axis (assembled from wrapped
    # pieces: mixed regions), seeded random ones; first, last and a random head
    gw = torch.Generator().manual_seed(5)
    wsel = {0, nw - 1, Wn - 1, Wn - nw, max(nw - 2, 0)} | {int(w) for w in torch.randint(0, Wn, (5,), generator=gw)}
    hsel = sorted({0, heads - 1, int(torch.randint(0, heads, (1,), generator=gw))})
    wins = torch.tensor(sorted(wsel)).repeat_interleave(len(hsel))
    hs = torch.tensor(hsel).repeat(len(wsel))
    t = qd[wins.to(DEV)].cpu().view(len(wins), n, 3, heads, 16)
    q, k, v = (S.f16(t[torch.arange(len(wins)), :, i, hs]) for i in range(3))                 # fp32 input: rounded on load
    bias = S.table_bias(table_t, hs, n) if dense_b is None else dense_b.double()[hs]
    mask = None
    if dense_m is not None:
        mask = dense_m.double()[wins % nw]
    elif reg is not None:
        mask = S.region_mask(reg, wins, reg.shape[0])
    r = S.attention_ref(q, k, v, bias, mask)
    got = out[wins.to(DEV)].cpu().view(len(wins), n, heads, 16)[torch.arange(len(wins)), :, hs]
    c = R.check(got, r["out"], S.attention_bound(r, dtype), coords=torch.stack([wins, hs], 1))
    _report("window_attention", name, form, (Wn, n, heads, str(dtype)[6:]), got.numel(), c)


# ---- token_linear ---------------------------------------------------------------------------------------------------------
def _lin_ops(M, K, N, seed, lda_extra=0, scale=1.0):
    g = _gen(seed)
    A = (scale * torch.randn(M, K + lda_extra, generator=g)).half()
    W = (torch.randn(N, K, generator=g) / K ** 0.5).half()
    b = torch.randn(N, generator=g)
    return A, W, b


# M, K, N, mode, strided A, out_off   (the fine-stage layers of the plan: qkv 48 -> 144, 96 -> 288; proj; linear1 / linear2)
TOKLIN = [(110592, 48, 144, "plain", 0, 0), (13824, 96, 288, "plain", 0, 8), (1000, 48, 144, "plain", 16, 8), (513, 384, 96, "plain", 0, 0),
          (129, 24, 48, "plain", 0, 8), (13824, 96, 384, "gelu", 0, 0), (300, 48, 192, "gelu", 16, 8), (900, 192, 48, "residual", 0, 0),
          (13829, 384, 96, "residual", 0, 0)]


@pytest.mark.parametrize("M,K,N,mode,extra,out_off", TOKLIN)
def test_token_linear(M, K, N, mode, extra, out_off):
    from diff_unet_amos_amd import ops
    A, W, b = _lin_ops(M, K, N, M + K + N, extra, 2.5 if mode == "gelu" else 1.0)
    rows = S.sample_rows(M, 512, seed=1)
    Ad = A.to(DEV)[:, :K]
    ref, ab, sq = S.linear_ref(A[rows, :K].double(), W.double(), b)
    if mode == "residual":
        x0 = torch.randn(M, N, generator=_gen(7))
        x = x0.to(DEV)
        ops.token_linear(Ad, W.to(DEV), b.to(DEV), "residual", x=x)
        torch.cuda.synchronize()
        rx, abx = S.residual_ref(x0[rows].double(), ref, ab)
        c = R.check(x[rows.to(DEV)].cpu(), rx, S.residual_bound(rx, abx, sq, K), coords=rows[:, None])
    else:
        out = torch.full((M, N + out_off), 7.0, dtype=F16, device=DEV)
        ops.token_linear(Ad, W.to(DEV), b.to(DEV), mode, out=out, out_off=out_off)
        torch.cuda.synchronize()
        assert out_off == 0 or bool((out[:, :out_off] == 7).all())                     # the untouched columns, exactly
        got = out[rows.to(DEV), out_off:].cpu()
        if mode == "gelu":
            c = R.check(got, S.gelu64(ref), S.linear_gelu_bound(ref, ab, K, F16), coords=rows[:, None])
        else:
            c = R.check(got, ref, S.linear_bound(ref, ab, sq, K, F16), coords=rows[:, None])
    _report("token_linear", f"{mode} {M}x{K}->{N}", "128-row tiles", (M, K, N), len(rows) * N, c)


def test_token_linear_stats_with_a_sample_boundary_inside_a_tile():
    from diff_unet_amos_amd import ops
    B, V, K, N = 2, 1500, 96, 48                               # 1500 = 11 tiles + 92 rows: the boundary falls inside a 128-row tile
    A, W, _ = _lin_ops(B * V, K, N, 3, 16)
    Ad, Wd = A.to(DEV)[:, :K], W.to(DEV)
    out, st = torch.empty(B * V, N, dtype=F16, device=DEV), ops.stats_buffer(B, N, DEV)
    ops.token_linear(Ad, Wd, None, "stats", out=out, stats=st, samples=B)
    torch.cuda.synchronize()
    rows = S.sample_rows(B * V, 512, seed=2, boundaries=(V,))
    ref, ab, sq = S.linear_ref(A[rows, :K].double(), W.double())
    c = R.check(out[rows.to(DEV)].cpu(), ref, S.linear_bound(ref, ab, sq, K, F16), coords=rows[:, None])
    _report("token_linear", "stats output", "128-row tiles", (B * V, K, N), len(rows) * N, c)
    # R.stats_bound allows u_out sum |y| for sums of unrounded accumulators; this kernel sums the STORED values, so the bound is
    # about three orders loose here: it sees rows attributed to the wrong sample, not one dropped row or a tile counted twice at
    # small |y|.  A bound for this kernel's own chain (tiles per workgroup, 5 shuffle levels, fp64 after) is a follow-up.
    s, q, sa = S.stats_ref(out.cpu(), B)
    bs, bq = R.stats_bound(sa, q, F16, -(-V // 128))
    sd = ops.stats_decode(st).cpu()
    _report("token_linear", "stats words: sum", "128-row tiles", (B, N), B * N, R.check(sd[:, :N, 0].contiguous(), s, bs))
    _report("token_linear", "stats words: sum of squares", "128-row tiles", (B, N), B * N, R.check(sd[:, :N, 1].contiguous(), q, bq))
    out_b, st_b = torch.empty_like(out), ops.stats_buffer(B, N, DEV)
    ops.token_linear(Ad, Wd, None, "stats", out=out_b, stats=st_b, samples=B, background=1)
    assert torch.equal(out_b, out)                            # one workgroup per CU: the same output bit for bit
    sdb = ops.stats_decode(st_b).cpu()
    assert R.check(sdb[:, :N, 0].contiguous(), s, bs).ratio <= 1.0 and R.check(sdb[:, :N, 1].contiguous(), q, bq).ratio <= 1.0


# dims, C, window, shift, K.  C = 192 runs with K = 96: with K = N = 192 the resident weights and the fp32 tile exceed the LDS limit
# (include/dua_hip.h), which test_token_linear_scatter_rejects_what_does_not_fit_lds pins
@pytest.mark.parametrize("dims,C,ws,ss,K", [((9, 8, 10), 48, (7, 7, 7), (3, 3, 3), 48), ((8, 14, 7), 96, (7, 7, 7), (3, 3, 0), 96),
                                          ((12, 12, 12), 192, (7, 7, 7), (3, 3, 3), 96)])
def test_token_linear_scatter(dims, C, ws, ss, K):
    """proj + window_reverse + roll back + crop + shortcut + norm2 on a shifted, padded, cropped geometry."""
    from diff_unet_amos_amd import ops
    B = 2
    geom = ops.window_geom(B, dims, C, ws, ss)
    tm = S.window_token_map(B, dims, ws, ss)
    Mw = tm.numel()
    A, W, b = _lin_ops(Mw, K, C, C + 1)
    g = _gen(C)
    gm, bt = 1 + 0.3 * torch.randn(C, generator=g), 0.3 * torch.randn(C, generator=g)
    x0 = torch.randn(B * dims[0] * dims[1] * dims[2], C, generator=g)
    x, ln = x0.to(DEV).view(B, *dims, C).contiguous(), torch.zeros(B, *dims, C, dtype=F16, device=DEV)
    ops.token_linear(A.to(DEV), W.to(DEV), b.to(DEV), "scatter", x=x, geom=geom, gamma=gm.to(DEV), beta=bt.to(DEV), ln_out=ln)
    torch.cuda.synchronize()
    rows = S.sample_rows(Mw, 512, seed=3, boundaries=(Mw // 2,), window=343)
    rows = rows[tm[rows] >= 0]                                 # padding tokens write nothing; every voxel is written once:
    vox = tm[rows]
    ref, ab, sq = S.linear_ref(A[rows].double(), W.double(), b)
    rx, abx = S.residual_ref(x0[vox].double(), ref, ab)
    xs = x.view(-1, C)[vox.to(DEV)].cpu()
    _report("token_linear", f"scatter stream C {C}", "128-row tiles", (Mw, K, C), xs.numel(),
            R.check(xs, rx, S.residual_bound(rx, abx, sq, K), coords=rows[:, None]))
    lref, parts = S.layernorm_ref(xs.double(), gm, bt)         # the stored stream IS the norm's input
    _report("token_linear", f"scatter norm2 C {C}", "128-row tiles", (Mw, K, C), xs.numel(),
            R.check(ln.view(-1, C)[vox.to(DEV)].cpu(), lref, S.layernorm_bound(lref, parts, S.ln_chain(12, C // 12), F16), coords=rows[:, None]))
    written = torch.zeros(x0.shape[0], dtype=torch.bool)
    written[tm[tm >= 0]] = True
    assert bool(written.all())


def test_token_linear_scatter_rejects_what_does_not_fit_lds():
    """K = N = 192: 6 * 32 * 400 + 16 bytes of weights + 128 * 784 of fp32 tile = 177 168 > 160 KiB.  The launcher must refuse with
    DUA_ERR_ARG and touch nothing (include/dua_hip.h documents the limit; the plan uses PLAIN + window_scatter_add_norm there)."""
    from diff_unet_amos_amd import ops
    B, dims, C, ws, ss = 1, (7, 7, 7), 192, (7, 7, 7), (0, 0, 0)
    geom = ops.window_geom(B, dims, C, ws, ss)
    A, W, b = _lin_ops(343, C, C, 5)
    x = torch.full((B, *dims, C), 3.0, device=DEV)
    ln = torch.full((B, *dims, C), 7.0, dtype=F16, device=DEV)
    ones = torch.ones(C, device=DEV)
    with pytest.raises(RuntimeError, match="dua_token_linear failed: invalid argument"):
        ops.token_linear(A.to(DEV), W.to(DEV), b.to(DEV), "scatter", x=x, geom=geom, gamma=ones, beta=ones, ln_out=ln)
    torch.cuda.synchronize()
    assert bool((x == 3).all()) and bool((ln == 7).all())


# ---- swin_mlp ----------------------------------------------------------------------------------------------------------------
# C = 96 runs at 13 824 tokens in the plan (the 24^3 stage); 110 592 is the 48^3 stage's count, run at both widths
@pytest.mark.parametrize("C,M,scale", [(48, 110592, 1.0), (96, 13824, 1.0), (96, 110592, 1.0), (48, 1000, 2.5), (96, 777, 2.5)])
def test_swin_mlp(C, M, scale):
    from diff_unet_amos_amd import ops
    g = _gen(C + M)
    ln2 = (scale * torch.randn(M, C, generator=g)).half()
    w1, w2 = (torch.randn(4 * C, C, generator=g) / C ** 0.5).half(), (torch.randn(C, 4 * C, generator=g) / (4 * C) ** 0.5).half()
    b1, b2, x0 = torch.randn(4 * C, generator=g), torch.randn(C, generator=g), torch.randn(M, C, generator=g)
    x = x0.to(DEV)
    ops.swin_mlp(ln2.to(DEV), w1.to(DEV), b1.to(DEV), w2.to(DEV), b2.to(DEV), x)
    torch.cuda.synchronize()
    rows = S.sample_rows(M, 512, seed=4)
    ref, bnd = S.mlp_ref(ln2[rows].double(), w1.double(), b1, w2.double(), b2, x0[rows].double())
    if scale > 1:
        pre = S.linear_ref(ln2[rows].double(), w1.double(), b1)[0]
        assert float(pre.min()) < -6 and float(pre.max()) > 6                           # both GELU tails are reached
    _report("swin_mlp", f"C {C} M {M} scale {scale}", "128-row tiles", (M, C), len(rows) * C, R.check(x[rows.to(DEV)].cpu(), ref, bnd, coords=rows[:, None]))


# ---- token_gemm ------------------------------------------------------------------------------------------------------------
def gemm_ksplit(M, K, N):
    """dua_token_gemm_workspace / dua_token_gemm restated (csrc/swin_gemm_wide.hip:200-230): the K slices that hold work, 0 = no split."""
    tiles, ksteps = -(-M // 64) * -(-N // 64), -(-K // 64)
    if tiles >= 128 or ksteps < 8:
        return 0, 0
    z = min(256 // tiles, ksteps // 2, 16)
    if z < 2:
        return 0, 0
    kper = -(-ksteps // z) * 64
    return z, -(-K // kper)


# M, K, N, mode, K slices (pinned: 0 = the single-launch form)
TOKGEMM = [(343, 3072, 768, "plain", 3), (27, 3072, 768, "gelu", 16), (27, 3072, 768, "residual", 16), (2744, 192, 576, "plain", 0),
           (1728, 768, 192, "gelu", 3), (21952, 96, 288, "plain", 0), (1000, 96, 96, "gelu", 0), (216, 1536, 384, "residual", 8),
           (13824, 384, 96, "residual", 0), (216, 384, 1536, "gelu", 0), (100, 72, 96, "plain", 0), (300, 200, 96, "gelu", 0),
           (64, 520, 64, "plain", 3), (70, 1096, 96, "residual", 9)]


@pytest.mark.parametrize("M,K,N,mode,ksplit", TOKGEMM)
def test_token_gemm(M, K, N, mode, ksplit):
    from diff_unet_amos_amd import ops, _native as nv
    z, ks = gemm_ksplit(M, K, N)
    assert ks == ksplit, (z, ks)
    assert int(nv.lib().dua_token_gemm_workspace(M, K, N)) == z * M * N * 4             # the library takes the same form
    A, W, b = _lin_ops(M, K, N, M + K, 16, 2.5 if mode == "gelu" else 1.0)
    rows = S.sample_rows(M, 384, seed=5)
    Ad = A.to(DEV)[:, :K]
    ref, ab, sq = S.linear_ref(A[rows, :K].double(), W.double(), b)
    if mode == "residual":
        x0 = torch.randn(M, N, generator=_gen(9))
        x = ops.token_gemm(Ad, W.to(DEV), b.to(DEV), "residual", x=x0.to(DEV))
        torch.cuda.synchronize()
        rx, abx = S.residual_ref(x0[rows].double(), ref, ab)
        c = R.check(x[rows.to(DEV)].cpu(), rx, S.residual_bound(rx, abx, sq, K, ks), coords=rows[:, None])
    else:
        out = torch.full((M, N + 8), 7.0, dtype=F16, device=DEV)
        ops.token_gemm(Ad, W.to(DEV), b.to(DEV), mode, out=out, out_off=8)
        torch.cuda.synchronize()
        assert bool((out[:, :8] == 7).all())
        got = out[rows.to(DEV), 8:].cpu()
        if mode == "gelu":
            c = R.check(got, S.gelu64(ref), S.linear_gelu_bound(ref, ab, K, F16, ks), coords=rows[:, None])
        else:
            c = R.check(got, ref, S.linear_bound(ref, ab, sq, K, F16, ks), coords=rows[:, None])
    _report("token_gemm", f"{mode} {M}x{K}->{N}", f"{ks} K slices" if ks else "single launch", (M, K, N), len(rows) * N, c)


# ---- the LayerNorm kernels -------------------------------------------------------------------------------------------------
def _stream(shape, seed, high_mean):
    x = torch.randn(*shape, generator=_gen(seed))
    return 100 + 0.3 * x if high_mean else x                  # |mean| >> std: the kernels centre before squaring


# B, dims, C, window, shift, dtype, rows with mean 100 / std 0.3
GATHER = [(1, (48, 48, 48), 48, (7, 7, 7), (3, 3, 3), F16, False), (2, (9, 8, 10), 48, (7, 7, 7), (3, 3, 3), F32, False),
          (2, (8, 14, 7), 96, (7, 7, 7), (3, 3, 0), F16, True), (2, (12, 12, 12), 192, (7, 7, 7), (0, 0, 0), F16, False),
          (2, (6, 6, 6), 384, (6, 6, 6), (0, 0, 0), F16, False), (2, (3, 3, 3), 768, (3, 3, 3), (0, 0, 0), F16, False)]


@pytest.mark.parametrize("B,dims,C,ws,ss,dtype,high", GATHER)
def test_window_gather_norm_and_scatter_add_norm(B, dims, C, ws, ss, dtype, high):
    from diff_unet_amos_amd import ops
    g = _gen(C + dims[0])
    nvox = B * dims[0] * dims[1] * dims[2]
    x0 = _stream((nvox, C), C, high)
    y = (0.3 * torch.randn(nvox, C, generator=g)).to(dtype)
    g1, b1, g2, b2 = (0.3 * torch.randn(C, generator=g) + (1.0 if i % 2 == 0 else 0.0) for i in range(4))
    geom = ops.window_geom(B, dims, C, ws, ss)
    tm = S.window_token_map(B, dims, ws, ss)
    n = ws[0] * ws[1] * ws[2]
    x = x0.to(DEV).view(B, *dims, C).contiguous()
    win = torch.full((tm.numel(), C), 7.0, dtype=dtype, device=DEV)
    ops.window_gather_norm(x, geom, g1.to(DEV), b1.to(DEV), win.view(-1, n, C), y=y.to(DEV).view(B, *dims, C))
    torch.cuda.synchronize()
    chain = S.ln_chain(12, C // 12)
    rows = S.sample_rows(tm.numel(), 512, seed=6, boundaries=(tm.numel() // B,), window=n)
    vox = tm[rows].clamp(min=0)
    xs = x.view(-1, C)[vox.to(DEV)].cpu()
    sref = x0[vox].double() + y[vox].double()
    _report("window_gather_norm", f"stream C {C} {dims}", f"{C // 12} lanes/token", (tm.numel(), C), xs.numel(), R.check(xs, sref, S.stream_add_bound(sref)))
    ref, parts = S.layernorm_ref(xs.double(), g1, b1)
    real = (tm[rows] >= 0)[:, None]
    ref = torch.where(real, ref, torch.zeros_like(ref))                                    # F.pad after norm1: exact zeros
    bnd = torch.where(real, S.layernorm_bound(ref, parts, chain, dtype), torch.full_like(ref, 1e-300))
    _report("window_gather_norm", f"norm1 C {C} {dims}{' mean 100' if high else ''}", f"{C // 12} lanes/token", (tm.numel(), C), xs.numel(),
            R.check(win[rows.to(DEV)].cpu(), ref, bnd, coords=rows[:, None]))
    # the way back
    yw = torch.randn(tm.numel(), C, generator=g).to(dtype)
    x1 = x.clone().view(-1, C).cpu()
    ln = torch.empty(nvox, C, dtype=dtype, device=DEV)
    ops.window_scatter_add_norm(x, geom, yw.to(DEV).view(-1, n, C), g2.to(DEV), b2.to(DEV), ln.view(B, *dims, C))
    torch.cuda.synchronize()
    src = torch.empty(nvox, dtype=torch.int64)
    src[tm[tm >= 0]] = torch.arange(tm.numel())[tm >= 0]
    vrows = S.sample_rows(nvox, 512, seed=7, boundaries=(nvox // B,))
    xs2 = x.view(-1, C)[vrows.to(DEV)].cpu()
    sref = x1[vrows].double() + yw[src[vrows]].double()
    _report("window_scatter_add_norm", f"stream C {C} {dims}", f"{C // 12} lanes/token", (nvox, C), xs2.numel(), R.check(xs2, sref, S.stream_add_bound(sref)))
    ref, parts = S.layernorm_ref(xs2.double(), g2, b2)
    _report("window_scatter_add_norm", f"norm2 C {C} {dims}{' mean 100' if high else ''}", f"{C // 12} lanes/token", (nvox, C), xs2.numel(),
            R.check(ln[vrows.to(DEV)].cpu(), ref, S.layernorm_bound(ref, parts, chain, dtype), coords=vrows[:, None]))


@pytest.mark.parametrize("C,dtype,high", [(48, F16, False), (96, F16, True), (192, F32, False), (384, F16, False), (768, F16, False)])
def test_stage_out(C, dtype, high):
    from diff_unet_amos_amd import ops
    B, per = 2, 1001
    g = _gen(C)
    y = _stream((B * per, C), C + 2, high).to(dtype)
    ta = torch.randn(B, C + 8, generator=g)
    emb = torch.randn(B * per, C, generator=g).to(dtype)
    out = torch.full((B * per, C + 8), 7.0, dtype=dtype, device=DEV)
    xs = torch.empty(B * per, C, dtype=F32, device=DEV)
    ops.stage_out(y.to(DEV), B, C, out, 8, tadd=ta.to(DEV)[:, 8:], emb=emb.to(DEV), x=xs)
    torch.cuda.synchronize()
    assert bool((out[:, :8] == 7).all())
    rows = S.sample_rows(B * per, 512, seed=8, boundaries=(per,))
    xr = xs[rows.to(DEV)].cpu()
    sref = y[rows].double() + ta[rows // per, 8:].double()
    _report("stage_out", f"stream C {C}", f"{C // 12} lanes/token", (B * per, C), xr.numel(), R.check(xr, sref, S.stream_add_bound(sref)))
    ref, parts = S.layernorm_ref(xr.double(), None, emb[rows].double())
    _report("stage_out", f"norm + emb C {C}{' mean 100' if high else ''}", f"{C // 12} lanes/token", (B * per, C), xr.numel(),
            R.check(out[rows.to(DEV), 8:].cpu(), ref, S.layernorm_bound(ref, parts, S.ln_chain(12, C // 12), dtype), coords=rows[:, None]))


# shape, legacy, dtype, mean 100, form (csrc/swin_ops.hip:154: ntok < 2048 && 8 C % 256 == 0 -> a workgroup per token)
MERGE = [((1, 48, 48, 48, 48), True, F16, False, "wave"), ((1, 24, 24, 24, 96), True, F16, False, "wide"), ((1, 12, 12, 12, 192), True, F16, True, "wide"),
         ((1, 6, 6, 6, 384), True, F16, False, "wide"), ((2, 5, 7, 6, 96), True, F32, False, "wide"), ((1, 4, 4, 4, 16), False, F16, False, "wave"),
         ((2, 9, 6, 11, 48), False, F16, False, "wave")]


@pytest.mark.parametrize("shape,legacy,dtype,high,form", MERGE)
def test_patch_merge_norm(shape, legacy, dtype, high, form):
    from diff_unet_amos_amd import ops
    B, D, H, W, C = shape
    ntok = B * ((D + 1) // 2) * ((H + 1) // 2) * ((W + 1) // 2)
    chain, took = S.patch_merge_chain(C, ntok)
    assert took == form
    g = _gen(sum(shape))
    x = _stream(shape, C, high)
    y = (0.1 * torch.randn(*shape, generator=g)).to(dtype)
    gm, bt = 1 + 0.2 * torch.randn(8 * C, generator=g), 0.2 * torch.randn(8 * C, generator=g)
    got = ops.patch_merge_norm(x.to(DEV), gm.to(DEV), bt.to(DEV), legacy=legacy, y=y.to(DEV), dtype=dtype)
    torch.cuda.synchronize()
    toks = S.sample_rows(ntok, 384, seed=9)
    v = S.patch_merge_gather(x + y.float(), toks, legacy)       # the pending y is added first, in one fp32 add, as the kernel does
    ref, parts = S.layernorm_ref(v, gm, bt)
    c = R.check(got.view(-1, 8 * C)[toks.to(DEV)].cpu(), ref, S.layernorm_bound(ref, parts, chain, dtype), coords=toks[:, None])
    _report("patch_merge_norm", f"{shape} legacy {legacy}{' mean 100' if high else ''}", form, (ntok, 8 * C), ref.numel(), c)


@pytest.mark.parametrize("dtype", [F16, F32])
def test_gelu(dtype):
    from diff_unet_amos_amd import ops
    h = torch.cat([torch.linspace(-12, 12, 1 << 16), 3 * torch.randn(1 << 16, generator=_gen(1))]).to(dtype)
    got = ops.gelu_(h.clone().to(DEV)).cpu()
    x = h.double()
    _report("gelu_", str(dtype)[6:], "elementwise", tuple(h.shape), h.numel(), R.check(got, S.gelu64(x), S.gelu_bound(x, torch.zeros_like(x), dtype)))


# ---- patch_embed ------------------------------------------------------------------------------------------------------------
# dtype -> form (dua_patch_embed: fp16 takes patch_embed_mfma_kernel, fp32 the fmaf kernel)
@pytest.mark.parametrize("dtype,form,shape,high", [(F16, "mfma", (2, 8, 6, 10, 17, 24), False), (F32, "fmaf", (2, 8, 6, 10, 17, 24), False),
                                                   (F16, "mfma", (1, 96, 96, 96, 17, 24), False), (F16, "mfma", (2, 10, 6, 6, 32, 32), True),
                                                   (F32, "fmaf", (1, 10, 6, 6, 8, 8), True)])
def test_patch_embed(dtype, form, shape, high):
    from diff_unet_amos_amd import ops
    B, D, H, W, cin, cp = shape
    E, K = 48, 8 * cp
    n, n_ln, took = S.patch_embed_chain(K, dtype)
    assert took == form
    g = _gen(sum(shape))
    torch.manual_seed(sum(shape))
    conv = torch.nn.Conv3d(cin, E, 2, 2)
    ntok = B * (D // 2) * (H // 2) * (W // 2)
    per = ntok // B
    xin = torch.zeros(B, D, H, W, 32, dtype=dtype)
    xin[..., :cin] = torch.randn(B, D, H, W, cin, generator=g).to(dtype)
    bias = conv.bias.detach() + (100.0 if high else 0.0)           # |mean| >> std over the 48 channels
    tadd = torch.randn(B, E + 8, generator=g)
    emb = torch.randn(ntok, E, generator=g).to(dtype)
    wp = ops.pack_patch_embed_weights(conv.weight.detach().to(DEV), cp)
    out = torch.full((ntok, 2 * E), 7.0, dtype=dtype, device=DEV)
    stream = torch.empty(ntok, E, dtype=F32, device=DEV)
    xd = xin.to(DEV)
    ops.patch_embed(xd, cp, wp, bias.to(DEV).contiguous(), out.view(B, D // 2, H // 2, W // 2, 2 * E), E, tadd=tadd.to(DEV)[:, 8:],
                    emb=emb.to(DEV), x=stream)
    torch.cuda.synchronize()
    assert bool((out[:, :E] == 7).all())
    toks = S.sample_rows(ntok, 512, seed=11, boundaries=(per,) if B > 1 else ())
    A = S.patch_embed_rows(xd, toks, cp)
    Wm = S.patch_embed_weights(conv.weight, cp, dtype)
    assert dtype == F16 or torch.equal(Wm.float(), wp.cpu().view(K, E))                       # the packed order is the reference's
    ref, ab, sq = S.patch_embed_ref(A, Wm, bias, tadd[toks // per, 8:])
    xs = stream[toks.to(DEV)].cpu()
    _report("patch_embed", f"stream {shape}", form, (ntok, K, E), xs.numel(), R.check(xs, ref, R.bound(ref, ab, sq, n, F32), coords=toks[:, None]))
    lref, parts = S.layernorm_ref(xs.double(), None, emb[toks].double())
    _report("patch_embed", f"norm + emb {shape}{' mean 100' if high else ''}", form, (ntok, K, E), xs.numel(),
            R.check(out[toks.to(DEV), E:].cpu(), lref, S.layernorm_bound(lref, parts, n_ln, dtype), coords=toks[:, None]))


# ---- linear_f32 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,K,N,gelu,strided", [(1000, 48, 144, False, False), (343 * 3, 48, 192, True, False), (216, 768, 3072, False, False),
                                                (77, 20, 50, False, False), (513, 96, 48, False, True), (64, 4, 1, True, True)])
def test_linear_f32(M, K, N, gelu, strided):
    """The shapes of tests/test_swin.py::test_linear_f32_kernel_matches_torch against fp64 with the K + 1 chain."""
    from diff_unet_amos_amd import ops
    g = _gen(M + K + N)
    wide = torch.randn(M, K + 12 if strided else K, generator=g)
    w, b = torch.randn(N, K, generator=g) / K ** 0.5, torch.randn(N, generator=g)
    got = ops.linear_f32(wide.to(DEV)[:, :K], w.to(DEV), b.to(DEV), gelu=gelu)
    torch.cuda.synchronize()
    rows = S.sample_rows(M, 256, seed=12, tiles=(32, 64))
    ref, ab, sq = S.linear_ref(wide[rows, :K].double(), w.double(), b)
    want = S.gelu64(ref) if gelu else ref
    c = R.check(got[rows.to(DEV)].cpu(), want, S.linear_f32_bound(ref, ab, sq, K, gelu), coords=rows[:, None])
    _report("linear_f32", f"{M}x{K}->{N}{' gelu' if gelu else ''}{' strided' if strided else ''}", "fp32 MFMA", (M, K, N), len(rows) * N, c)


# ---- residual_norm_act ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F16, F32])
@pytest.mark.parametrize("second_norm,post,ra", [(False, False, False), (True, False, False), (True, True, False), (False, False, True),
                                                 (True, True, True)])
def test_residual_norm_act(dtype, second_norm, post, ra):
    from diff_unet_amos_amd import ops
    N, dims, C = 2, (9, 10, 11), 48
    V = dims[0] * dims[1] * dims[2]
    g = _gen(17 + 2 * second_norm + post)
    raw = (torch.randn(N, *dims, C, generator=g) * 1.5 + 0.3).to(dtype).to(DEV)
    res = (torch.randn(N, *dims, C, generator=g) * 2 + 0.5).to(dtype).to(DEV)
    wide = (2 * torch.randn(N, *dims, 2 * C, generator=g)).to(dtype).to(DEV)       # post_add / ra_src: channel slices of a wider buffer
    gam = [(1 + 0.3 * torch.randn(C, generator=g)).to(DEV) for _ in range(2)]
    bet = [(0.3 * torch.randn(C, generator=g)).to(DEV) for _ in range(2)]

    def consts(t, k):
        st = ops.instnorm_stats(t, C, ops.stats_buffer(N, C, DEV))
        nrm = ops.Norm(st, gam[k], bet[k], V, slope=0.01)
        sc64, sh64, b_sc, b_sh = R.finalize(ops.stats_decode(st).cpu(), gam[k].cpu(), bet[k].cpu(), V, 1e-5)
        sc, sh = (c.cpu() for c in ops.instnorm_finalize(nrm, N, C))
        assert R.check(sc, sc64, b_sc).ratio <= 1 and R.check(sh, sh64, b_sh).ratio <= 1      # the preamble's constants, to fp64
        return nrm, sc.double(), sh.double()

    na, sc, sh = consts(raw, 0)
    nb, rsc, rsh = consts(res, 1) if second_norm else (None, None, None)
    kw = {}
    if post:
        kw.update(post_add=wide, post_off=0)
    if ra:
        kw.update(ra_src=wide, ra_off=C)
    out = torch.full((N, *dims, C + 8), 7.0, dtype=dtype, device=DEV)
    ops.residual_norm_act(raw, na, res, nb, slope=0.01, out=out, out_off=8, **kw)
    torch.cuda.synchronize()
    assert bool((out[..., :8] == 7).all())
    back = torch.full_like(out, 7.0)
    ops.residual_norm_act(raw, na, res, nb, slope=0.01, out=back, out_off=8, background=True, **kw)
    assert torch.equal(out, back)                             # one workgroup per CU: the same values
    rows = S.sample_rows(N * V, 768, seed=13, boundaries=(V,))
    rd = rows.to(DEV)
    pick = lambda t, lo, hi: t.view(N * V, -1)[rd, lo:hi].cpu().double()
    smp = rows // V
    ref, parts = S.residual_norm_act_ref(pick(raw, 0, C), sc[smp], sh[smp], pick(res, 0, C), rsc[smp] if second_norm else None,
                                         rsh[smp] if second_norm else None, 0.01, pick(wide, 0, C) if post else None,
                                         pick(wide, C, 2 * C) if ra else None)
    c = R.check(pick(out, 8, C + 8), ref, S.residual_norm_act_bound(ref, parts, dtype), coords=rows[:, None])
    _report("residual_norm_act", f"{str(dtype)[6:]} norm3 {second_norm} post {post} ra {ra}", "grid-stride", (N * V, C), ref.numel(), c)
