"""Step-Uncertainty Fusion on the MI355X: dua_suf_accumulate on every shared case against the fp64 reference under the derived
bound (tests/suf_fp64ref.py), its determinism and what it must leave alone, the identity clamp(logits) == the tail's xstart
that lets the kernel read R tensors per step instead of 2 R, and the fused loop end to end through both launch plans and
through DiffUNet.forward."""
import pytest
import torch

import suf_fp64ref as sf

pytestmark = pytest.mark.gpu

IDS = [c["id"] for c in sf.CASES]
I32 = torch.int32
TINY = dict(in_channels=1, out_channels=2, features=(8, 8, 16, 32, 64, 8))


def _word(v):
    return torch.tensor([v], dtype=I32, device="cuda")


@pytest.fixture(scope="module")
def refs():
    """Per case: operands on the device and the float64 step, computed once and left unchanged."""
    out = {}
    for c in sf.CASES:
        k, T = c["step"]
        logits, acc = sf.make_logits(c), sf.make_acc(c)
        out[c["id"]] = (logits.cuda(), acc.cuda(), sf.step_ref(logits, acc, c["G"], k, T))
    return out


@pytest.mark.parametrize("case", sf.CASES, ids=IDS)
def test_kernel_meets_the_bound_on_every_case(case, refs):
    from diff_unet_amos_amd import ops
    from diff_unet_amos_amd.gaussian_diffusion import suf_step_coef
    logits, acc, r = refs[case["id"]]
    k, T = case["step"]
    coef = suf_step_coef(T, "cuda")
    kept = logits.clone()
    err = _word(0)
    by_word = ops.suf_accumulate(logits, acc.clone(), coef, step_word=_word(k), err_word=err)
    by_arg = ops.suf_accumulate(logits, acc.clone(), coef, step=k)
    again = ops.suf_accumulate(logits, acc.clone(), coef, step_word=_word(k), step=T + 5)       # the word wins over the argument
    for name, got in (("step from the device word", by_word), ("step from the argument", by_arg)):
        res = sf.check(got.cpu(), r["ref"], r["bound"])
        print(f"{case['id']} ({name}): {res}")
        assert res.ratio <= 1.0, (name, res)
    assert torch.equal(by_word, by_arg) and torch.equal(by_word, again)                         # no atomics: the same bits
    assert torch.equal(logits, kept) and int(err.item()) == 0


def test_unaligned_accumulator_takes_the_scalar_path(refs):
    """voxels % 4 == 0 but acc 4 bytes off 16-byte alignment: the same bits as the vector path."""
    from diff_unet_amos_amd import ops
    from diff_unet_amos_amd.gaussian_diffusion import suf_step_coef
    case = next(c for c in sf.CASES if c["dims"] == sf.POW2 and c["G"] == 2 and c["C"] == 3)
    logits, acc, _ = refs[case["id"]]
    k, T = case["step"]
    coef = suf_step_coef(T, "cuda")
    want = ops.suf_accumulate(logits, acc.clone(), coef, step=k)
    buf = torch.zeros(acc.numel() + 1, device="cuda")
    off = buf[1:].view(acc.shape)
    off.copy_(acc)
    assert off.data_ptr() % 16 == 4 and off.is_contiguous()
    assert torch.equal(ops.suf_accumulate(logits, off, coef, step=k), want) and float(buf[0]) == 0.0


def test_step_word_outside_the_table_is_clamped_and_reported(refs):
    from diff_unet_amos_amd import ops
    from diff_unet_amos_amd.gaussian_diffusion import suf_step_coef
    case = sf.CASES[0]
    logits, acc, _ = refs[case["id"]]
    T = case["step"][1]
    coef = suf_step_coef(T, "cuda")
    for word, clamped in ((T, T - 1), (T + 1000, T - 1), (-1, 0)):
        err = _word(0)
        got = ops.suf_accumulate(logits, acc.clone(), coef, step_word=_word(word), err_word=err)
        assert int(err.item()) == 1 and torch.equal(got, ops.suf_accumulate(logits, acc.clone(), coef, step=clamped))
        ops.suf_accumulate(logits, acc.clone(), coef, step_word=_word(word))                   # no error word: still clamped
    with pytest.raises(RuntimeError, match="invalid argument"):
        ops.suf_accumulate(logits, acc.clone(), coef, step=T)


def _diffunet(uncer_step=None, steps=3, dtype=torch.float16):
    from diff_unet_amos_amd.diff_unet import DiffUNet
    torch.manual_seed(0)
    net = DiffUNet(sample_steps=steps, compute_dtype=dtype, uncer_step=uncer_step, **TINY)
    with torch.no_grad():
        for n, p in net.named_parameters():
            if ".adn.N." in n:
                p.copy_(torch.randn_like(p) * 0.3 + (1.0 if n.endswith("weight") else 0.0))
    return net.cuda().eval()


def test_clamped_logits_are_the_tails_xstart_bit_for_bit():
    """One DiffUNet step writing both outputs: x0^ = clamp(logits, -1, 1) exactly, which is why dua_suf_accumulate reads the
    logits alone."""
    from diff_unet_amos_amd import _native as nv
    net = _diffunet()
    g = torch.Generator().manual_seed(3)
    image = torch.rand(2, 1, 32, 32, 32, generator=g).cuda()
    x_T = torch.randn(2, 2, 32, 32, 32, generator=g).cuda()
    with torch.no_grad():
        net.embed_model(image)
        plan = net._rt.plan(2, (32, 32, 32), image.device)
        plan._reset(x_T)
        plan.new_seed(1)
        coef_table, row_of_step = plan._step_tables(net.sample_diffusion, "ddim", 0.0)
        logits, xstart = torch.zeros_like(x_T), torch.zeros_like(x_T)
        for _ in range(2):
            plan.native_step(nv.MODE_DDIM, row_of_step=row_of_step, coef_table=coef_table, logits=logits, xstart=xstart)
            assert torch.equal(logits.clamp(-1, 1), xstart)
            assert float(logits.abs().max()) > 1.0 and float(logits.abs().min()) < 1.0         # both sides of the clamp


def _end_to_end(net, dims, G=2, R=2):
    """The fused loop of ``net``'s launch plan: eager against the fp64 fusion of its own recorded logits, graph == eager ==
    graph again, and the sampler state untouched by the fusion."""
    T = net.sample_diffusion.num_timesteps
    d = net.sample_diffusion
    g = torch.Generator().manual_seed(8)
    image = torch.rand(G, 1, *dims, generator=g).cuda().repeat_interleave(R, dim=0)
    x_T = torch.randn(G * R, 2, *dims, generator=g).cuda()
    with torch.no_grad():
        net.embed_model(image)
        plan = net._rt.plan(G * R, dims, image.device)
        recorded = []
        eager = plan.sample_loop(d, "ddim", noise=x_T, use_graph=False, seed=5, fuse_runs=R, step_logits=recorded)
        assert len(recorded) == T and tuple(eager["fused_pred_xstart"].shape) == (G, 2, *dims)
        assert eager["sum_pred_xstart"] is None
        ref, bound = sf.loop_ref(recorded, G)
        res = sf.check(eager["fused_pred_xstart"], ref, bound)
        print(f"{type(plan).__name__} {dims} G {G} R {R} T {T}: {res}")
        assert res.ratio <= 1.0, res
        n_graphs = len(plan.graphs)
        g1 = plan.sample_loop(d, "ddim", noise=x_T, seed=5, fuse_runs=R)
        g2 = plan.sample_loop(d, "ddim", noise=x_T, seed=5, fuse_runs=R)
        assert len(plan.graphs) == n_graphs + 1
        for other in (g1, g2):
            assert torch.equal(other["fused_pred_xstart"], eager["fused_pred_xstart"])
            assert torch.equal(other["sample"], eager["sample"])
        plain = plan.sample_loop(d, "ddim", noise=x_T, seed=5)
        assert torch.equal(plain["sample"], eager["sample"])                  # the fusion does not disturb the sampler state
        # the runs of a window differ (own x_T each), and the result is not the plain sum of their predictions
        assert float((recorded[0][0] - recorded[0][1]).abs().max()) > 1e-3
        both = plain["sum_pred_xstart"].reshape(G, R, *plain["sum_pred_xstart"].shape[1:]).sum(1)
        assert float((eager["fused_pred_xstart"] - both).abs().max()) > 1e-2
    return plan, x_T, eager


def test_fused_loop_end_to_end_diffunet():
    _end_to_end(_diffunet(), (32, 32, 32))


def test_fused_loop_end_to_end_swin():
    from diff_unet_amos_amd.diff_swin_unetr import DiffSwinUNETR
    from diff_unet_amos_amd.gaussian_diffusion import make_spaced
    torch.manual_seed(6)
    net = DiffSwinUNETR(in_channels=1, out_channels=2, feature_size=48, compute_dtype=torch.float16).eval()
    with torch.no_grad():
        for k, p in net.named_parameters():
            if "relative_position_bias_table" in k:
                p.normal_(0, 0.3)
    net.sample_diffusion = make_spaced(1000, [3])
    _end_to_end(net.cuda(), (64, 64, 64))


def test_forward_with_uncer_step_equals_the_driver():
    """DiffUNet(..., uncer_step=2) through forward(image, pred_type="ddim_sample"): shape, finite, and under the same torch
    seed the bits of the driver-level loop from the same x_T; one window at a time (a plan of R rows, whose small levels may
    take other launch forms than the plan of 2 R rows) runs too."""
    R, dims = 2, (32, 32, 32)
    net = _diffunet(uncer_step=R)
    image = torch.rand(2, 1, *dims, generator=torch.Generator().manual_seed(9)).cuda()
    with torch.no_grad():
        torch.manual_seed(21)
        out = net(image, pred_type="ddim_sample")
        assert tuple(out.shape) == (2, 2, *dims) and bool(torch.isfinite(out).all())
        torch.manual_seed(21)
        x_T = torch.randn(2 * R, 2, *dims, device="cuda")
        net.embed_model(image.repeat_interleave(R, dim=0))
        plan = net._rt.plan(2 * R, dims, image.device)
        want = plan.sample_loop(net.sample_diffusion, "ddim", noise=x_T, fuse_runs=R)["fused_pred_xstart"]
        assert torch.equal(out, want)
        net.batched_sampling = False
        one = net(image, pred_type="ddim_sample")
        assert tuple(one.shape) == (2, 2, *dims) and bool(torch.isfinite(one).all())
        net.batched_sampling = True
        # the streamed whole-volume evaluation with the switch set: two windows in one predictor call, a plan of 2 R rows
        from diff_unet_amos_amd.inference import evaluate_volume
        volume = torch.rand(1, 1, 32, 32, 48, generator=torch.Generator().manual_seed(10)).cuda()
        mask, dice = evaluate_volume(net, volume, roi_size=dims, sw_batch_size=2)
        assert tuple(mask.shape) == (1, 2, 32, 32, 48) and mask.dtype == torch.uint8 and dice is None
        net.uncer_step = None                                                  # the switch off: the plain sum again
        plain = net(image, pred_type="ddim_sample")
        assert tuple(plain.shape) == (2, 2, *dims) and float(plain.abs().max()) <= 3.0 + 1e-5
