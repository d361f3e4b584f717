"""DiffUNet at any patch extent >= 32: nn.MaxPool3d(2) floors odd extents, and UpCat replicate-pads the upsampled half by one
plane on every axis where it is one short of the skip (models/basic_unet/denoiser.py:176-186; oracle/unet_ref.py RefUpCat).
Kernels (floor pooling in dua_materialize and its backward, dua_deconv_k2s2_pad_fwd / _bwd) against torch, then the network,
the samplers, training and the sliding window against the oracle with the tolerances of the even-extent tests."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

TINY = dict(in_channels=1, out_channels=2, features=(8, 8, 16, 32, 64, 8))
ODD = (35, 33, 40)          # levels (35,33,40) (17,16,20) (8,8,10) (4,4,5) (2,2,2): pads at levels 0 (d, h), 1 (d) and 3 (w)


# ---- 1. level geometry (CPU) ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [(63, 48, 40), (33, 35, 97), (97, 96, 95), (64, 64, 64)])
def test_level_geometry_matches_the_oracle(dims):
    from diff_unet_amos_amd.engine import level_geometry
    from oracle.unet_ref import RefUpCat
    S, pad = level_geometry(*dims)
    x = torch.zeros(1, 1, *dims)
    want = [tuple(x.shape[2:])]
    for _ in range(4):
        x = F.max_pool3d(x, 2)
        want.append(tuple(x.shape[2:]))
    assert S == want
    for l in range(4):
        # the oracle's UpCat pads exactly the axes where 2 x the coarse extent falls short of the skip
        seen = {}
        up = RefUpCat(8, 8, 8)
        up.convs = torch.nn.Identity()
        up.convs.forward = lambda t, temb: t                                                   # noqa: E731
        up.upsample.register_forward_hook(lambda m, i, o: seen.__setitem__("up", tuple(o.shape[2:])))
        with torch.no_grad():
            out = up(torch.zeros(1, 8, *S[l + 1]), torch.zeros(1, 8, *S[l]), None)
        assert tuple(out.shape[2:]) == S[l]
        assert pad[l] == tuple(a - b for a, b in zip(S[l], seen["up"]))
    if dims == (64, 64, 64):
        assert pad == [(0, 0, 0)] * 4


def test_extents_below_32_are_refused():
    from diff_unet_amos_amd.engine import level_geometry
    for dims in ((31, 64, 64), (64, 30, 64), (64, 64, 17)):
        with pytest.raises(AssertionError):
            level_geometry(*dims)


# ---- 2. materialise with floor pooling --------------------------------------------------------------------------------------
def _norm_inputs(raw, C, seed):
    from diff_unet_amos_amd import ops
    g = torch.Generator().manual_seed(seed)
    N = raw.shape[0]
    r = raw[..., :C].double().cpu()
    sums = torch.stack([r.sum((1, 2, 3)), (r * r).sum((1, 2, 3))], -1)
    stats = ops.stats_encode(sums.cuda())
    gamma = (torch.rand(C, generator=g) + 0.5).cuda()
    beta = torch.randn(C, generator=g).cuda()
    return ops.Norm(stats, gamma, beta, raw.shape[1] * raw.shape[2] * raw.shape[3]), gamma, beta, N


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,blocked", [(torch.float32, False), (torch.float16, False), (torch.float16, True)],
                         ids=["fp32", "fp16", "fp16-blocked"])      # the 16-channel-block layout is fp16 only
@pytest.mark.parametrize("dims", [(9, 6, 8), (7, 11, 13), (6, 8, 5), (33, 35, 40)])
def test_materialize_floor_pooling(dtype, dims, blocked):
    from diff_unet_amos_amd import ops
    C, N = 32, 2
    g = torch.Generator().manual_seed(sum(dims))
    raw = torch.randn(N, *dims, 40, generator=g).to(dtype).cuda()
    emb = torch.randn(N, *dims, C, generator=g).to(dtype).cuda()
    norm, gamma, beta, _ = _norm_inputs(raw, C, 3)
    out = torch.full((N, *dims, 48), 7.0, dtype=dtype, device="cuda")
    pooled = torch.full((N, dims[0] // 2, dims[1] // 2, dims[2] // 2, C), 7.0, dtype=dtype, device="cuda")
    ops.materialize(raw, C, norm, out, 16, emb=emb, pooled=pooled)
    # the activation itself against torch
    r = raw[..., :C].float()
    mean, var = r.mean((1, 2, 3), keepdim=True), r.var((1, 2, 3), unbiased=False, keepdim=True)
    y = (r - mean) / torch.sqrt(var + 1e-5) * gamma + beta
    want = F.leaky_relu(y, 0.1) + emb.float()
    tol = 1e-4 if dtype == torch.float32 else 2e-2
    assert (out[..., 16:16 + C].float() - want).abs().max().item() < tol
    assert bool((out[..., :16] == 7).all()) and bool((out[..., 16 + C:] == 7).all())
    # pooling is bit-equal to F.max_pool3d (floor) of what was materialised
    act = out[..., 16:16 + C].permute(0, 4, 1, 2, 3).float()
    assert torch.equal(pooled.float(), F.max_pool3d(act, 2).permute(0, 2, 3, 4, 1))
    if blocked:
        ob = ops.to_blocked(torch.full((N, *dims, 48), 7.0, dtype=dtype, device="cuda"))
        pb = torch.empty_like(pooled)
        ops.materialize(raw, C, norm, ob, 16, emb=emb, pooled=pb, out_blocked=True)
        assert torch.equal(ops.from_blocked(ob), out) and torch.equal(pb, pooled)
    else:
        plain = torch.empty((N, *dims, C), dtype=dtype, device="cuda")     # no pooling: the same activation
        ops.materialize(raw, C, norm, plain, 0, emb=emb)
        assert torch.equal(plain, out[..., 16:16 + C])


# ---- 3. padded transposed convolution ---------------------------------------------------------------------------------------
MASKS = [(a, b, c) for a in (0, 1) for b in (0, 1) for c in (0, 1)]
# (coarse extent, Cin) per kernel form: all-taps needs >= 32768 coarse voxels and <= 4 Cin chunks; k-split needs >= 8 chunks
FORMS = {"alltaps": ((32, 33, 32), 32), "ksplit": ((5, 4, 6), 256), "onetap": ((5, 4, 6), 64)}
KIND = {"alltaps": 2, "ksplit": 1, "onetap": 0}


def _deconv_case(dtype, form, mask, seed):
    from diff_unet_amos_amd import ops
    (D, H, W), cin = FORMS[form]
    if form == "ksplit" and dtype == torch.float32:
        cin = 128                                     # 4-channel fp32 groups: 8 chunks of 16
    cout, N = 24, 2
    cin_off, cs_in = 8, cin + 16
    cout_off, cs_out = 16, 56
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, D, H, W, cs_in, generator=g).to(dtype)
    w = torch.randn(cin, cout, 2, 2, 2, generator=g) / np.sqrt(cin)
    b = torch.randn(cout, generator=g)
    out = tuple(2 * e + m for e, m in zip((D, H, W), mask))
    assert ops.deconv_kernel_kind(dtype, N, D, H, W, cin, cout) == KIND[form]
    return x, w, b, out, (N, cin, cin_off, cs_in, cout, cout_off, cs_out)


def _ref_deconv(x_cl, cin_off, cin, w, b, out):
    xs = x_cl[..., cin_off:cin_off + cin].double().permute(0, 4, 1, 2, 3)
    y = F.conv_transpose3d(xs, w.double(), b.double(), stride=2)
    pad = [0, out[2] - y.shape[4], 0, out[1] - y.shape[3], 0, out[0] - y.shape[2]]
    return F.pad(y, pad, "replicate")


# the all-taps form runs on a large tile grid: three masks cover its per-pair edge logic; the other forms take all eight
FWD_CASES = [(f, m) for f in FORMS for m in MASKS if f != "alltaps" or m in ((0, 0, 1), (1, 1, 0), (1, 1, 1))]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("form,mask", FWD_CASES, ids=[f"{f}-{''.join(map(str, m))}" for f, m in FWD_CASES])
def test_padded_deconv_forward(dtype, form, mask):
    from diff_unet_amos_amd import ops
    x, w, b, out, (N, cin, cin_off, cs_in, cout, cout_off, cs_out) = _deconv_case(dtype, form, mask, 11 + sum(mask))
    wp, bp = ops.pack_deconv_weights(w.cuda(), b.cuda(), dtype)
    y = torch.full((N, *out, cs_out), 3.0, dtype=dtype, device="cuda")
    ops.deconv_k2s2(x.cuda(), cin, cin_off, wp, bp, cout, y, cout_off)
    want = _ref_deconv(x, cin_off, cin, w, b, out).permute(0, 2, 3, 4, 1)
    got = y[..., cout_off:cout_off + cout].double().cpu()
    err = (got - want).abs().max().item() / want.abs().max().item()
    assert err < (1e-5 if dtype == torch.float32 else 3e-3), err
    assert bool((y[..., :cout_off] == 3).all()) and bool((y[..., cout_off + cout:] == 3).all())
    if form == "alltaps" and dtype == torch.float16:       # the 16-channel-block output of the same launch
        yb = ops.to_blocked(torch.full((N, *out, 64), 3.0, dtype=dtype, device="cuda"))
        ops.deconv_k2s2(x.cuda(), cin, cin_off, wp, bp, cout, yb, 16, out_blocked=True)
        assert torch.equal(ops.from_blocked(yb)[..., 16:16 + cout], y[..., cout_off:cout_off + cout])


@pytest.mark.gpu
def test_padded_deconv_is_its_own_op_kind_in_the_step_list():
    """A recorded padded deconvolution carries y's extents; an even one records the plain op exactly as before."""
    from diff_unet_amos_amd import _native as nv
    from diff_unet_amos_amd import ops
    assert nv.OP_DECONV_PAD == 5 and "dua_deconv_k2s2_pad_fwd" in nv.exported_symbols()
    x = torch.zeros(1, 4, 5, 6, 8, device="cuda")
    wp = torch.zeros(8 * 1 * 1 * 4 * 64 * 16, dtype=torch.uint8, device="cuda")
    bp = torch.zeros(64, device="cuda")
    ys = (torch.zeros(1, 9, 10, 13, 16, device="cuda"), torch.zeros(1, 8, 10, 12, 16, device="cuda"))
    rec = []
    with ops.recording(rec):          # recorded, not launched
        ops.deconv_k2s2(x, 8, 0, wp, bp, 8, ys[0], 8)
        ops.deconv_k2s2(x, 8, 0, wp, bp, 8, ys[1], 8)
    assert [r.kind for r in rec] == [nv.OP_DECONV_PAD, nv.OP_DECONV]
    assert (rec[0].mat.D, rec[0].mat.H, rec[0].mat.W) == (9, 10, 13) and (rec[1].mat.D, rec[1].mat.H, rec[1].mat.W) == (0, 0, 0)


# ---- 4. backward: max pooling and the padded transposed convolution ---------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("dims", [(9, 6, 8), (7, 11, 13), (33, 35, 40)])
def test_maxpool_backward_odd_extents(dtype, dims):
    from diff_unet_amos_amd import ops
    C, N = 24, 2
    g = torch.Generator().manual_seed(sum(dims))
    act = torch.randn(N, *dims, 40, generator=g).to(dtype)
    dA = torch.randn(N, *dims, 32, generator=g).to(dtype)
    dP = torch.randn(N, dims[0] // 2, dims[1] // 2, dims[2] // 2, C, generator=g).to(dtype)
    got = ops.maxpool2_bwd_add(act.cuda(), 8, C, dA.cuda(), 8, dP.cuda()).double().cpu()
    a = act[..., 8:8 + C].double().permute(0, 4, 1, 2, 3).requires_grad_(True)
    F.max_pool3d(a, 2).backward(dP.double().permute(0, 4, 1, 2, 3))
    want = a.grad.permute(0, 2, 3, 4, 1) + dA[..., 8:8 + C].double()
    tol = 1e-6 if dtype == torch.float32 else 4e-3
    assert (got - want).abs().max().item() < tol * max(1.0, want.abs().max().item())
    odd = [i for i, e in enumerate(dims) if e & 1]
    for i in odd:                                   # the trailing plane: dA only
        sl = [slice(None)] * 5
        sl[1 + i] = dims[i] - 1
        assert torch.equal(got[tuple(sl)], dA[..., 8:8 + C].double()[tuple(sl)])


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("mask", MASKS, ids=["".join(map(str, m)) for m in MASKS])
@pytest.mark.parametrize("coarse", [(5, 4, 6), (16, 17, 9)])
def test_padded_deconv_backward(dtype, mask, coarse):
    from diff_unet_amos_amd import ops
    from diff_unet_amos_amd.training import _channel_sums
    N, cin, cout = 2, 64, 24
    cin_off, cout_off, cs_out = 8, 16, 56
    D, H, W = coarse
    out = tuple(2 * e + m for e, m in zip(coarse, mask))
    g = torch.Generator().manual_seed(5 + sum(mask))
    x = torch.randn(N, D, H, W, cin + 16, generator=g).to(dtype)
    w = torch.randn(cin, cout, 2, 2, 2, generator=g) / np.sqrt(cin)
    b = torch.randn(cout, generator=g)
    dy = torch.randn(N, *out, cs_out, generator=g).to(dtype)
    dx, dw = ops.deconv_k2s2_bwd(x.cuda(), cin, cin_off, dy.cuda(), cout, cout_off, w.cuda())
    db = _channel_sums(dy.cuda(), cout, cout_off)
    xs = x[..., cin_off:cin_off + cin].double().permute(0, 4, 1, 2, 3).requires_grad_(True)
    wd, bd = w.double().requires_grad_(True), b.double().requires_grad_(True)
    y = _ref_deconv(xs.permute(0, 2, 3, 4, 1), 0, cin, wd, bd, out)
    y.backward(dy[..., cout_off:cout_off + cout].double().permute(0, 4, 1, 2, 3))

    def rel(a, ref):
        return ((a.double().cpu() - ref) ** 2).sum().sqrt().item() / (ref ** 2).sum().sqrt().item()
    tol = 1e-5 if dtype == torch.float32 else 5e-3
    assert rel(dx, xs.grad.permute(0, 2, 3, 4, 1)) < tol
    assert rel(dw, wd.grad) < tol
    assert rel(db, bd.grad) < tol


# ---- 5.-7. the network, the samplers and training against the oracle ----------------------------------------------------------
def _pair(kw, dtype, seed=0, sample_steps=10):
    from diff_unet_amos_amd.diff_unet import DiffUNet
    from oracle.unet_ref import RefDiffUNet
    torch.manual_seed(seed)
    ref = RefDiffUNet(sample_steps=sample_steps, **kw).eval()
    with torch.no_grad():
        for n, p in ref.named_parameters():
            if ".adn.N." in n:
                p.copy_(torch.randn_like(p) * 0.3 + (1.0 if n.endswith("weight") else 0.0))
    net = DiffUNet(sample_steps=sample_steps, compute_dtype=dtype, **kw)
    net.load_state_dict(ref.state_dict())
    return net.cuda().eval(), ref


_ORACLE = {}


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,mx,mean", [(torch.float32, 2e-3, 2e-4), (torch.float16, 1e-2, 1e-3)], ids=["fp32", "fp16"])
@pytest.mark.parametrize("dims,kw", [((63, 48, 40), TINY), ((97, 96, 95), dict(in_channels=1, out_channels=2))],
                         ids=["63x48x40-tiny", "97x96x95-default"])
def test_denoise_matches_oracle_at_odd_extents(dtype, mx, mean, dims, kw):
    net, ref = _pair(kw, dtype)
    g = torch.Generator().manual_seed(1)
    image = torch.rand(2, 1, *dims, generator=g)
    x = torch.randn(2, 2, *dims, generator=g)
    t = torch.tensor([999, 3])
    key = (dims, tuple(kw.get("features", ())))
    if key not in _ORACLE:                     # one CPU oracle pass per geometry, shared by both dtypes
        with torch.no_grad():
            _ORACLE[key] = ref(image=image, x=x, step=t, pred_type="denoise")
    want = _ORACLE[key]
    with torch.no_grad():
        got = net(image=image.cuda(), x=x.cuda(), step=t.cuda(), pred_type="denoise").cpu()
    d = (got - want).abs()
    print(f"\n[{dtype} {dims}] |dlogit| max {d.max():.3e} mean {d.mean():.3e}")
    assert d.max() < mx and d.mean() < mean


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_ddim_sample_matches_oracle_at_an_odd_extent(dtype):
    from oracle.unet_ref import binarise, dice_coeff
    net, ref = _pair(dict(in_channels=1, out_channels=2), dtype)
    g = torch.Generator().manual_seed(2)
    image = torch.rand(1, 1, *ODD, generator=g)
    xT = torch.randn(1, 2, *ODD, generator=g)
    with torch.no_grad():
        want = ref.ddim_sample(image, x_T=[xT], step_noise=[[torch.zeros_like(xT)] * 10])
        emb = net.embed_model(image.cuda())
        out = net.sample_diffusion.ddim_sample_loop(net.model, (1, 2, *ODD), noise=xT.cuda(),
                                                    model_kwargs={"image": image.cuda(), "embeddings": emb})
    got = sum(s for s in out["all_samples"]).cpu()
    dice = [dice_coeff(binarise(got)[:, c], binarise(want)[:, c]) for c in range(2)]
    print(f"\n[{dtype}] sum-x0 |d| max {(got - want).abs().max():.3e}; Dice per class {dice}")
    assert min(dice) > 1 - 1e-3, dice


@pytest.mark.gpu
def test_graph_replay_equals_eager_at_an_odd_extent():
    from diff_unet_amos_amd import _native as nv
    net, _ = _pair(TINY, torch.float16)
    image = torch.rand(1, 1, *ODD).cuda()
    with torch.no_grad():
        a = net(image, pred_type="ddim_sample")
    assert a.shape == (1, 2, *ODD) and torch.isfinite(a).all()
    plan = net._rt.plan(1, ODD, image.device)
    assert nv.OP_DECONV_PAD in [op.kind for op in plan._step_ops]
    d = net.sample_diffusion
    xT = torch.randn(1, 2, *ODD, device="cuda")
    with torch.no_grad():
        net.embed_model(image)
        g1 = plan.sample_loop(d, "ddim", noise=xT, use_graph=True, seed=7)["sum_pred_xstart"].clone()
        eg = plan.sample_loop(d, "ddim", noise=xT, use_graph=False, seed=7)["sum_pred_xstart"].clone()
    assert torch.equal(g1, eg)


@pytest.mark.gpu
def test_ddpm_finishing_steps_run_at_an_odd_extent():
    """fp16 DDPM loop: the last steps run on the companion exact-fp32 plan, whose geometry must be the same."""
    net, _ = _pair(TINY, torch.float16)
    net.ddpm_finish_fp32_steps = 2
    image = torch.rand(1, 1, *ODD).cuda()
    plan = net._rt.plan(1, ODD, image.device)
    xT = torch.randn(1, 2, *ODD, device="cuda")
    with torch.no_grad():
        net.embed_model(image)
        out = plan.sample_loop(net.sample_diffusion, "ddpm", noise=xT, use_graph=True, seed=3)["sample"]
    assert out.shape == (1, 2, *ODD) and torch.isfinite(out).all()
    assert plan._hi.S == plan.S and plan._hi.pad == plan.pad


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_training_step_matches_oracle_at_an_odd_extent(dtype):
    from diff_unet_amos_amd.diff_unet import DiffUNet
    from oracle.train_ref import RefLoss as Loss
    from oracle.unet_ref import RefDiffUNet
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    ref = RefDiffUNet(**TINY)
    net = DiffUNet(compute_dtype=dtype, **TINY)
    net.load_state_dict(ref.state_dict())
    net = net.to(dev).train()
    g = torch.Generator().manual_seed(11)
    image = torch.rand(2, 1, *ODD, generator=g)
    labels = (torch.rand(2, 2, *ODD, generator=g) > 0.7).float()
    crit = Loss()
    np.random.seed(5)
    x_t, t, _ = net(x=labels.to(dev) * 2 - 1, pred_type="q_sample")
    preds = net(x=x_t, step=t, image=image.to(dev), pred_type="denoise")
    scale = 1024.0 if dtype == torch.float16 else 1.0
    (crit(preds, labels.to(dev)) * scale).backward()
    # the oracle in float64: the reference value of every gradient, free of the oracle's own fp32 rounding (at 32^3 a
    # LeakyReLU input within fp32 rounding of the kink moves the oracle's fp32 gradients by up to 2e-2, tests/test_training_harness.py)
    ref = ref.double()
    ref.model.temb.dense[0].register_forward_pre_hook(lambda m, a: (a[0].double(),))     # its sinusoid table is built in fp32
    want = ref(image=image.double(), x=x_t.cpu().double(), step=t.cpu(), pred_type="denoise")
    crit(want, labels.double()).backward()
    gp = dict(net.named_parameters())
    num = den = 0.0
    checked = []
    for k, p in ref.named_parameters():
        if k.endswith(".conv.bias"):         # a Conv3d bias in front of InstanceNorm: true gradient zero (the deconv biases are not)
            continue
        gk = gp[k].grad.detach().cpu().double() / scale
        num += float(((gk - p.grad.double()) ** 2).sum()); den += float((p.grad.double() ** 2).sum())
        if "upsample.deconv" in k:           # every UpCat's transposed convolution (weight AND bias), padded levels included
            checked.append(k)
            r = float(((gk - p.grad.double()) ** 2).sum().sqrt() / (p.grad.double() ** 2).sum().sqrt())
            cos = float(F.cosine_similarity(gk.flatten(), p.grad.double().flatten(), dim=0))
            print(f"[{dtype}] {k}: relative L2 {r:.2e}, cosine {cos:.6f}, norm ratio {float(gk.norm() / p.grad.double().norm()):.4f}")
            if dtype == torch.float32:
                assert r < 1e-3, (k, r)
            else:
                # fp16 activations: the bias gradient of the 4x4x5 level is a column sum with heavy cancellation (measured relative
                # L2 0.2, cosine 0.98 there; 3e-3 / 0.99999 at level 0, fp32 1e-6 everywhere).  Direction and SIZE: a scale error
                # in the fold of the padded planes moves the norm ratio.
                ratio = float(gk.norm() / p.grad.double().norm())
                assert cos > 0.95 and abs(ratio - 1) < 0.1 and r < 0.35, (k, r, cos, ratio)
    assert sorted(checked) == sorted(f"model.upcat_{i}.upsample.deconv.{w}" for i in (1, 2, 3, 4) for w in ("weight", "bias"))
    rel = (num / den) ** 0.5
    print(f"[{dtype}] odd-extent training step: whole-gradient relative L2 error vs oracle {rel:.2e}")
    assert rel < (1e-4 if dtype == torch.float32 else 5e-2), rel


@pytest.mark.gpu
@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_native_trainer_learns_at_an_odd_extent(graph):
    from diff_unet_amos_amd.diff_unet import DiffUNet
    from diff_unet_amos_amd.training import NativeConvTrainer
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    net = DiffUNet(**TINY).to(dev)
    tr = NativeConvTrainer(net, lr=2e-3, graph=graph)
    g = torch.Generator().manual_seed(11)
    image = torch.rand(2, 1, *ODD, generator=g).to(dev)
    labels = (torch.rand(2, 2, *ODD, generator=g) > 0.7).float().to(dev)
    noise = torch.randn(2, 2, *ODD, generator=g).to(dev)
    t = torch.randint(0, 1000, (2,), generator=g).to(dev)
    losses = [float(tr.step(image, labels, noise=noise, t=t)) for _ in range(10)]
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses


# ---- 8. sliding window with an ROI that is not a multiple of 16 ----------------------------------------------------------------
@pytest.mark.gpu
def test_infer_with_a_ragged_roi_matches_the_oracle_sliding_window():
    from diff_unet_amos_amd import inference
    from oracle.sliding_window_ref import sliding_window_ref
    from oracle.unet_ref import binarise, dice_coeff
    roi = (40, 56, 72)
    net, ref = _pair(TINY, torch.float32)
    g = torch.Generator().manual_seed(31)
    vol = torch.rand(1, 1, 48, 60, 80, generator=g)

    def seed_of(w):
        return int(w.double().abs().sum().item() * 1e3) % (2 ** 31)

    def ref_fn(win):
        w = torch.from_numpy(win).float()
        torch.manual_seed(seed_of(w.cuda()))
        xT = torch.randn(1, 2, *roi, device="cuda").cpu()
        with torch.no_grad():
            return ref.ddim_sample(w, x_T=[xT], step_noise=[[torch.zeros(1, 2, *roi)] * 10]).numpy()

    def predictor(x, **kw):
        torch.manual_seed(seed_of(x))
        return net(image=x, **kw)

    want = torch.from_numpy(sliding_window_ref(vol.numpy(), roi, 0.25, ref_fn)).float()
    with torch.no_grad():
        got = inference.sliding_window_inference(vol.cuda(), roi, 1, predictor, 0.25, pred_type="ddim_sample").cpu()
        seg = inference.infer(predictor, vol.cuda(), roi_size=roi, sw_batch_size=1, overlap=0.25).cpu()
    assert got.shape == (1, 2, 48, 60, 80)
    dice = [dice_coeff(binarise(got)[:, c], binarise(want)[:, c]) for c in range(2)]
    assert (got - want).abs().mean() < 1e-3 and min(dice) > 1 - 1e-3, dice
    assert torch.equal(seg, binarise(got))


# ---- 9. even extents are untouched ------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_even_plan_records_no_new_op_kind():
    from diff_unet_amos_amd import _native as nv
    from diff_unet_amos_amd import ops
    net, _ = _pair(TINY, torch.float16)
    plan = net._rt.plan(1, (64, 64, 64), torch.device("cuda", 0))
    plan.refresh_weights()
    assert plan.pad == [(0, 0, 0)] * 4
    rec = []
    with ops.recording(rec):
        plan.denoiser_body(zero_stats=False)
    kinds = {r.kind for r in rec}
    assert nv.OP_DECONV_PAD not in kinds and kinds <= {nv.OP_CONV3, nv.OP_MATERIALIZE, nv.OP_DECONV, nv.OP_UPCONV}
