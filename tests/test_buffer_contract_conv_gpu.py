"""Buffer contract of the convolution families: packed weights and their consumers, the split-K workspace, the backward
workspaces and the K-split token GEMM.

Every case runs through its ``ops`` entry point three times (tests/buffer_contract.py): every buffer the entry point allocates
for itself -- packed weights, workspaces, the cached grow-only scratch, op-allocated outputs -- zero-filled, 0xFF-filled
(NaN / -1 / 255), and left over from a case of other extents, each between fences.  Per case:

1. the 0xFF-filled run passes the family's fp64 reference check (here: in every mode, see below);
2. what the header promises to be the same bits on every run is byte-equal across the three modes;
3. no fence byte was touched;
4. the arena served allocations and none went past it.

SAME_BITS names the results check 2 covers, each with the line of include/dua_hip.h that makes the promise.  The convolution
outputs themselves carry no such promise in the header (dw is "ACCUMULATED into with fp32 atomics", dua_hip.h:205), so they are
held to check 1 in EVERY mode instead.  Packed-weight buffers are not compared directly: the bytes of their padding lanes are
not part of any description; they are compared through the convolution that multiplies them (NaN x 0 is NaN).
"""
import pytest
import torch

import buffer_contract as BC
import fp64ref as R
import test_backward_fp64 as TB
import test_kernels_gpu as TK
import test_swin_fp64 as TS
import test_upconv as TU

pytestmark = pytest.mark.gpu

F16, F32 = torch.float16, torch.float32
DTYPES = [F16, F32]
IDS = ["f16", "f32"]

# result name -> the promise
SAME_BITS = {
    "stats": "include/dua_hip.h:30-32 (integer atomics: two launches on the same inputs agree bit for bit)",
    "scale": "include/dua_hip.h:30-32 (every scale / shift derived from the sums)",
    "shift": "include/dua_hip.h:30-32",
}
# check 2 masks nothing here: no row.
UNSPECIFIED = {}


def _ops():
    from diff_unet_amos_amd import ops
    return ops


def _every_mode(outs, check):
    for mode in ("b", "a", "c"):
        try:
            check(outs[mode])
        except AssertionError as e:
            raise AssertionError(f"mode {mode}: {e}") from e


def _bits(outs):
    BC.same_bits(outs, only=set(SAME_BITS), unspecified=UNSPECIFIED)


# ---- conv3d_k3 with weights packed inside the block ------------------------------------------------------------------------------
def _conv3_run(dtype, shape):
    """pack_conv3_weights -> conv3d_k3 -> from_channels_last, and instnorm_finalize on the statistics: the packed buffer, the
    padded bias, the statistics rows and every output come from the allocator."""
    ops = _ops()
    N, Cin, Cout, D, H, W = shape
    g, x, w, b = TK._conv3_operands(shape)
    xcl = TK._cl(x, dtype)
    wd, bd = w.cuda(), b.cuda()
    gamma, beta = (torch.rand(Cout, generator=g) + 0.5).cuda(), torch.randn(Cout, generator=g).cuda()

    def run():
        wp, bp = ops.pack_conv3_weights(wd, bd, dtype)
        y = torch.empty((N, D, H, W, Cout), dtype=dtype, device="cuda")
        stats = ops.stats_buffer(N, Cout, "cuda")
        ops.conv3d_k3(xcl, Cin, 0, wp, bp, Cout, y, 0, stats)
        scale, shift = ops.instnorm_finalize(ops.Norm(stats, gamma, beta, D * H * W), N, Cout)
        return dict(y=ops.from_channels_last(y, Cout), stats=stats, scale=scale, shift=shift)

    def check(out):
        TK._fp64_bound_check(out["y"].cpu(), x.to(dtype).float(), w, b, dtype, seed=sum(shape))
    return run, check


CONV_SHAPES = [(2, 40, 72, 6, 10, 12), (1, 8, 16, 2, 2, 2)]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape,other", [(CONV_SHAPES[0], CONV_SHAPES[1]), (CONV_SHAPES[1], CONV_SHAPES[0])], ids=["ragged", "2x2x2"])
def test_conv3_packed_weights_and_outputs(dtype, shape, other):
    run, check = _conv3_run(dtype, shape)
    outs, served = BC.run_modes(run, _conv3_run(dtype, other)[0])
    _every_mode(outs, check)
    _bits(outs)
    assert served["b"] >= 7, served          # packed weights, bias, y, statistics, scale, shift, the NCDHW copy


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_conv3_permuted_padded_input_channels(dtype):
    """The first denoiser layer's case: 6 source channels mapped into 8 packed ones, two of them padding of the packed buffer."""
    ops = _ops()
    image, xt, w, b, buf, perm = TK._permuted_operands(dtype)
    wd, bd = w.cuda(), b.cuda()
    x = torch.cat([image, xt], 1)

    def run():
        wp, bp = ops.pack_conv3_weights(wd, bd, dtype, cin_packed=8, perm=perm + [-1] * (8 - len(perm)))
        y = torch.empty((1, 8, 8, 8, 16), dtype=dtype, device="cuda")
        stats = ops.stats_buffer(1, 16, "cuda")
        ops.conv3d_k3(buf, 8, 0, wp, bp, 16, y, 0, stats)
        return dict(y=ops.from_channels_last(y, 16), stats=stats)

    outs, _ = BC.run_modes(run, _conv3_run(dtype, CONV_SHAPES[1])[0])
    _every_mode(outs, lambda o: TK._fp64_bound_check(o["y"].cpu(), x.to(dtype).float(), w, b, dtype, seed=3))
    _bits(outs)


def _tap_run(classes, shape, cout):
    ops = _ops()
    N, D, H, W = shape
    cin_p = classes + 8
    x, w, b, perm, xp = TK._tap_operands(classes, shape, cout)
    wd, bd = w.cuda(), b.cuda()

    def run():
        wp, bp = ops.pack_conv3_weights(wd, bd, F16, cin_packed=cin_p, perm=perm, tap_channel=classes)
        y = torch.empty((N, D, H, W, cout), dtype=F16, device="cuda")
        stats = ops.stats_buffer(N, cout, "cuda")
        ops.conv3d_k3(xp, cin_p, 0, wp, bp, cout, y, 0, stats, tap_channel=classes)
        return dict(y=ops.from_channels_last(y, cout), stats=stats)

    def check(out):
        TK._fp64_bound_check(out["y"].cpu(), x.half().double(), w, b, F16, seed=classes + D)
    return run, check


def test_conv3_single_channel_tap_form():
    run, check = _tap_run(16, (2, 10, 9, 13), 64)
    outs, _ = BC.run_modes(run, _tap_run(16, (1, 9, 17, 8), 96)[0])
    _every_mode(outs, check)
    _bits(outs)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_conv3_dgrad_packed_weights(dtype):
    """pack_conv3_weights_dgrad through the data gradient of the ragged shape: dy [.., Cout] -> dx [.., Cin]."""
    ops = _ops()

    def case(shape):
        N, Cin, Cout, D, H, W = shape
        g, dy, w, _ = TK._conv3_operands((N, Cout, Cin, D, H, W))       # the operands of the convolution Cout -> Cin ...
        w = torch.randn(Cout, Cin, 3, 3, 3, generator=g) / (27 * Cout) ** 0.5      # ... with the FORWARD layer's weights
        dycl, wdev = TK._cl(dy, dtype), w.cuda()

        def run():
            wp, bp = ops.pack_conv3_weights_dgrad(wdev, dtype, cout_packed=Cout)
            dx = torch.empty((N, D, H, W, Cin), dtype=dtype, device="cuda")
            stats = ops.stats_buffer(N, Cin, "cuda")
            ops.conv3d_k3(dycl, Cout, 0, wp, bp, Cin, dx, 0, stats)
            return dict(y=ops.from_channels_last(dx, Cin), stats=stats)

        def check(out):
            wt = w.flip(2, 3, 4).transpose(0, 1).contiguous()
            TK._fp64_bound_check(out["y"].cpu(), dy.to(dtype).float(), wt, torch.zeros(Cin), dtype, seed=sum(shape))
        return run, check

    run, check = case(CONV_SHAPES[0])
    outs, _ = BC.run_modes(run, case(CONV_SHAPES[1])[0])
    _every_mode(outs, check)
    _bits(outs)


def test_batched_weight_packing_consumed_by_a_convolution():
    """ConvPacks.run() for (Cout, Cin) = (64, 64) and (136, 72) -- one flat buffer, 256-byte slots, the second tensor with a
    ragged last chunk and a ragged output tile -- each consumed by a convolution on a small ragged volume."""
    ops = _ops()
    N, D, H, W = 1, 3, 5, 6

    def case(pairs, seed):
        g = torch.Generator().manual_seed(seed)
        ws = [torch.randn(co, ci, 3, 3, 3, generator=g) / (27 * ci) ** 0.5 for co, ci in pairs]
        xs = [torch.randn(N, ci, D, H, W, generator=g) for _, ci in pairs]
        wdev, xcl = [w.cuda() for w in ws], [TK._cl(x, F16) for x in xs]

        def run():
            packs = ops.ConvPacks(F16)
            for w in wdev:
                packs.add(w, "fwd", w.shape[1])
            packs.run()
            out = {}
            for i, (w, x) in enumerate(zip(wdev, xcl)):
                co, ci = w.shape[:2]
                wp = packs.get(w, "fwd", ci)
                assert wp is not None
                y = torch.empty((N, D, H, W, co), dtype=F16, device="cuda")
                stats = ops.stats_buffer(N, co, "cuda")
                ops.conv3d_k3(x, ci, 0, wp, ops.zero_bias(co, "cuda"), co, y, 0, stats)
                out[f"y{i}"] = ops.from_channels_last(y, co)
                out[f"stats{i}"] = stats
            return out

        def check(out):
            for i, (w, x) in enumerate(zip(ws, xs)):
                TK._fp64_bound_check(out[f"y{i}"].cpu(), x.half().float(), w, torch.zeros(w.shape[0]), F16, seed=seed + i)
        return run, check

    run, check = case([(64, 64), (136, 72)], 5)
    outs, _ = BC.run_modes(run, case([(72, 40)], 6)[0])
    _every_mode(outs, check)
    BC.same_bits(outs, only={"stats0", "stats1"})


# ---- transposed convolution and the folded forms -----------------------------------------------------------------------------------
def _deconv_run(dtype, shape):
    ops = _ops()
    N, Cin, Cout, D, H, W = shape
    _, raw, w, b = TK._deconv_operands(shape)
    xcl, wd, bd = TK._cl(raw, dtype), w.cuda(), b.cuda()

    def run():
        wp, bp = ops.pack_deconv_weights(wd, bd, dtype)
        y = torch.empty((N, 2 * D, 2 * H, 2 * W, Cout), dtype=dtype, device="cuda")
        ops.deconv_k2s2(xcl, Cin, 0, wp, bp, Cout, y, 0)
        return dict(y=y)

    def check(out):
        dims = (D, H, W)
        pts = R.all_voxels(N, tuple(2 * s for s in dims))
        parent, child = R.deconv_sources(pts, dims)
        A = R.gather_points(xcl.cpu(), parent, 0, Cin)
        ref, ab, sq = R.deconv_ref_by_child(A, w, b, dtype, child)
        kind = {0: "one_tap", 1: "ksplit", 2: "alltaps"}[ops.deconv_kernel_kind(dtype, N, D, H, W, Cin, Cout)]
        bnd = R.bound(ref, ab, sq, R.deconv_fwd_chain(kind, Cin, dtype), dtype)
        res = R.check(R.gather_points(out["y"].cpu(), pts, 0, Cout), ref, bnd, pts)
        assert res.ratio <= 1, res
    return run, check


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_deconv_packed_weights_and_output(dtype):
    run, check = _deconv_run(dtype, (2, 40, 72, 2, 4, 6))
    outs, _ = BC.run_modes(run, _deconv_run(dtype, (1, 64, 32, 3, 3, 3))[0])
    _every_mode(outs, check)


def _deconv_res_run(shape):
    """The folded residual branch (dua_deconv_k2s2_res_fwd) of test_upconv.test_deconv_res_matches_deconv_cat_pointwise."""
    ops = _ops()
    dt = F16
    N, Cs, Cu, Cmid, Cout, D, H, W = shape            # D, H, W: COARSE extents
    skip, lo, w3, wd, cat, lbuf = TU._deconv_res_operands(shape)
    w3d, wdd = w3.cuda(), wd.cuda()

    def run():
        wp, wsp = ops.pack_deconv_res_weights(w3d, wdd, Cs, up_first=True)
        y = torch.empty((N, 2 * D, 2 * H, 2 * W, Cout), dtype=dt, device="cuda")
        stats = ops.stats_buffer(N, Cout, "cuda")
        ops.deconv_res(lbuf, Cu, 0, wp, cat, Cs, Cmid, wsp, Cout, y, 0, stats)
        return dict(y=ops.from_channels_last(y, Cout, 0), stats=stats)

    def check(out):
        TU._deconv_res_fp64_check(out["y"].cpu(), skip, lo, w3, wd, shape)
    return run, check


def test_folded_residual_branch():
    run, check = _deconv_res_run((1, 8, 32, 16, 24, 4, 6, 2))
    outs, _ = BC.run_modes(run, _deconv_res_run((2, 96, 64, 96, 96, 6, 10, 14))[0])
    _every_mode(outs, check)
    _bits(outs)


def _upconv_run(shape):
    """The folded up-convolution (dua_upconv_k3_fwd) with pack_upconv_weights inside the block: two packed buffers and the
    27-row bias table, whose columns behind Cout are padding when Cout is no multiple of 64."""
    ops = _ops()
    dt = F16
    N, Cs, Cu, Cmid, Cout, D, H, W, soff, sstride, uoff, ustride, ooff, ostride = shape
    xs, raw_u, wc, bc, wd, bd, norm, xbuf, ubuf = TU._upconv_operands(shape)
    dev = [t.cuda() for t in (wc, bc, wd, bd)]

    def run():
        w_skip, wu, btab = ops.pack_upconv_weights(*dev, Cs)
        y = torch.zeros((N, D, H, W, ostride), dtype=dt, device="cuda")
        stats = ops.stats_buffer(N, Cout, "cuda")
        ops.upconv_k3(xbuf, Cs, soff, ubuf, Cu, uoff, norm, w_skip, wu, btab, Cout, y, ooff, stats)
        return dict(y=ops.from_channels_last(y, Cout, ooff), stats=stats, wu=wu)

    def check(out):
        TU._fp64_fold_check(out["y"].cpu(), xs.to(dt).double(), TK._kernel_act(raw_u, norm, dt), wc, bc, wd, bd, out["wu"], False, True,
                            seed=sum(shape))
    return run, check


def test_folded_upconvolution():
    run, check = _upconv_run((2, 32, 128, 64, 72, 16, 24, 40, 32, 64, 64, 192, 16, 96))
    outs, _ = BC.run_modes(run, _upconv_run((1, 16, 64, 32, 64, 8, 8, 8, 0, 16, 0, 64, 0, 64))[0])
    _every_mode(outs, check)
    _bits(outs)


# ---- split-K workspace -----------------------------------------------------------------------------------------------------------
def _splitk_run(dtype, shape):
    """test_kernels_gpu.test_conv3_split_k with the workspace from ops.splitk_ws: the cached grow-only buffer, allocated inside
    the block (in leftover mode: holding the partial tiles of the larger layer)."""
    ops = _ops()
    N, Cin, Cout, D, H, W = shape
    g, raw, w, b = TK._conv3_operands(shape)
    norm, _ = TK._producer(raw, dtype, g, add=torch.randn(N, Cin, generator=g))
    assert ops.conv3_workspace_bytes(dtype, N, D, H, W, Cin, Cout) > 0, "these shapes are expected to take the split-K path"
    xcl, wd, bd = TK._cl(raw, dtype), w.cuda(), b.cuda()
    act = TK._kernel_act(raw, norm, dtype)

    def run():
        wp, bp = ops.pack_conv3_weights(wd, bd, dtype)
        ws = ops.splitk_ws(dtype, N, D, H, W, Cin, Cout, torch.device("cuda", torch.cuda.current_device()))
        assert ws is not None
        y = torch.empty((N, D, H, W, Cout), dtype=dtype, device="cuda")
        stats = ops.stats_buffer(N, Cout, "cuda")
        ops.conv3d_k3(xcl, Cin, 0, wp, bp, Cout, y, 0, stats, norm=norm, workspace=ws)
        return dict(y=ops.from_channels_last(y, Cout), stats=stats)

    def check(out):
        TK._fp64_bound_check(out["y"].cpu(), act, w, b, dtype, emulated=True, split_parts=3 * -(-Cin // ops.chunk_elems(dtype)),
                             seed=sum(shape))
    return run, check


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_split_k_workspace(dtype):
    run, check = _splitk_run(dtype, (2, 72, 136, 6, 6, 6))
    outs, _ = BC.run_modes(run, _splitk_run(dtype, (1, 128, 256, 12, 12, 12))[0])
    _every_mode(outs, check)
    _bits(outs)


# ---- backward workspaces ---------------------------------------------------------------------------------------------------------
def _wgrad_run(geo, dtype, policy):
    """conv3d_k3_wgrad without a caller workspace: the cached scratch of ops._wgrad_ws, allocated inside the block."""
    ops = _ops()
    N, D, H, W, cx, co_x, cin, cy, co_y, cout, cin_src, _ = TB.GEOS[geo]
    x, dy, perm, dw0, ref, ab = TB._operands(geo, dtype)
    form = TB._form(geo, dtype, policy, "full", perm)

    def run():
        dw = dw0.clone()
        ops.WGRAD_POLICY = policy
        try:
            ops.conv3d_k3_wgrad(x, cin, co_x, dy, cout, co_y, dw, perm=perm)
        finally:
            ops.WGRAD_POLICY = 0
        (ws,) = ops._WGRAD_WS.values()
        return dict(dw=dw, ws_bytes=ws.numel())

    def check(out):
        assert out["ws_bytes"] == form["ws"] > 0, "the launch is meant to take its partial sums through the cached workspace"
        res = R.check(out["dw"].double(), dw0.double() + ref, R.wgrad_bound(ref, ab, dw0, form["chain"]))
        assert res.ratio <= 1.0, res
    return run, check, form


@pytest.mark.parametrize("geo,policy,route,other", [("l6", 0, "fo-taps", ("l12", 0)), ("l12", TB.THREE_KD, "3kd-part", ("l6", 0))],
                         ids=["fo", "3kd-partials"])
def test_wgrad_workspace(geo, policy, route, other):
    """The smallest geometries of test_backward_fp64.GEOS that reach the fetch-once route and the three-kd route with partial
    sums (6^3 and 12^3, batch 2; 54 and 108 MiB of partials); the leftover run is the other geometry in the fetch-once route,
    whose partials fill the same cached buffer."""
    run, check, form = _wgrad_run(geo, F16, policy)
    assert form["name"] == route, form
    leftover = _wgrad_run(other[0], F16, other[1])[0]
    TB._CACHE.clear()                                 # the closures keep the operands
    outs, _ = BC.run_modes(run, leftover, arena_bytes=256 << 20)
    _every_mode(outs, check)


def _deconv_bwd_run(level):
    ops = _ops()
    dims, fine, cin, cout, cskip = level
    x, dcat, w = TB._deconv_bwd_operands(dims, fine, cin, cout, cskip)

    def run():
        dx, dw = ops.deconv_k2s2_bwd(x, cin, 8, dcat, cout, cskip, w)
        return dict(dx=dx, dw=dw)

    def check(out):
        TB._check_deconv_bwd(dims, fine, cin, cout, cskip, x, dcat, w, out["dx"], out["dw"])
    return run, check


def test_deconv_backward_workspace():
    levels = sorted(TB.DECONV_LEVELS, key=lambda c: c[0][0] * c[0][1] * c[0][2] * c[2] * c[3])
    run, check = _deconv_bwd_run(levels[0])
    outs, _ = BC.run_modes(run, _deconv_bwd_run(levels[1])[0], arena_bytes=128 << 20)
    _every_mode(outs, check)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_head_backward_workspace(dtype):
    ops = _ops()

    def case(shape):
        u, w, b, dl = TK._head_operands(dtype, shape)

        def run():
            du, dW, db = ops.head_bwd(dl, u, w)
            return dict(du=du, dW=dW, db=db)
        return run, lambda out: TB._check_head_bwd(u, dl, w, out["du"], out["dW"], out["db"], mfma=dtype == F16 and shape[4] == 64)

    run, check = case((1, 3, 5, 7, 8, 2))
    outs, _ = BC.run_modes(run, case((2, 4, 4, 5, 64, 11))[0])
    _every_mode(outs, check)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_instnorm_backward(dtype):
    ops = _ops()

    def case(shape):
        N, D, H, W, C = shape
        raw, gamma, beta, add, dA, stats, norm = TK._instnorm_bwd_operands(dtype, shape)

        def run():
            dY = torch.empty_like(raw)
            sums = ops.instnorm_bwd_sums(raw, norm)
            from diff_unet_amos_amd import _native as nv
            import ctypes
            d = nv.NormBwdDesc(nv.dt_code(dtype), N, D * H * W, C, C, 0, C, 0, C, 0)
            nv.check(nv.lib().dua_instnorm_bwd_reduce(ctypes.byref(d), nv.ptr(dA), nv.ptr(raw), norm.ref(N, C), nv.ptr(sums),
                                                      nv.stream_ptr()), "dua_instnorm_bwd_reduce")
            dgamma, dbeta, dadd = ops.instnorm_bwd(dA, 0, raw, C, norm, dY, sums=sums)
            return dict(dY=dY, sums=sums, dgamma=dgamma, dbeta=dbeta, dadd=dadd)

        def check(out):
            TB._check_in_bwd(f"{shape} {dtype}", dA, raw, gamma, beta, stats, out["sums"], out["dY"],
                             (out["dgamma"], out["dbeta"], out["dadd"]), R.in_bwd_reduce_chain(C, D * H * W, dtype), True)
        return run, check

    run, check = case((1, 6, 10, 4, 24))
    outs, _ = BC.run_modes(run, case((2, 4, 4, 4, 136))[0])
    _every_mode(outs, check)


# ---- Swin: the K-split token GEMM ----------------------------------------------------------------------------------------------
def _token_gemm_run(M, K, N, mode, ksplit):
    from diff_unet_amos_amd import ops
    import swin_fp64ref as S
    assert TS.gemm_ksplit(M, K, N)[1] == ksplit > 1
    A, W, b = TS._lin_ops(M, K, N, M + K, 16, 2.5 if mode == "gelu" else 1.0)
    rows = S.sample_rows(M, 384, seed=5)
    Ad, Wd, bd = A.to(TS.DEV)[:, :K], W.to(TS.DEV), b.to(TS.DEV)
    ref, ab, sq = S.linear_ref(A[rows, :K].double(), W.double(), b)
    x0 = torch.randn(M, N, generator=TS._gen(9))

    def run():
        if mode == "residual":
            return dict(out=ops.token_gemm(Ad, Wd, bd, "residual", x=x0.to(TS.DEV)))
        out = torch.empty((M, N), dtype=F16, device=TS.DEV)
        return dict(out=ops.token_gemm(Ad, Wd, bd, mode, out=out))

    def check(out):
        got = out["out"][rows.to(TS.DEV)].cpu()
        if mode == "residual":
            rx, abx = S.residual_ref(x0[rows].double(), ref, ab)
            c = R.check(got, rx, S.residual_bound(rx, abx, sq, K, ksplit), coords=rows[:, None])
        elif mode == "gelu":
            c = R.check(got, S.gelu64(ref), S.linear_gelu_bound(ref, ab, K, F16, ksplit), coords=rows[:, None])
        else:
            c = R.check(got, ref, S.linear_bound(ref, ab, sq, K, F16, ksplit), coords=rows[:, None])
        assert c.ratio <= 1, c
    return run, check


def test_token_gemm_k_split_workspace():
    cases = sorted((c for c in TS.TOKGEMM if c[4] > 1), key=lambda c: c[0] * c[1] * c[2])
    run, check = _token_gemm_run(*cases[0])
    outs, _ = BC.run_modes(run, _token_gemm_run(*cases[1])[0])
    _every_mode(outs, check)
