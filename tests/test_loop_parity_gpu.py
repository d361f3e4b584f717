"""The acceptance bar -- Dice within 1e-3 of the reference on identical inputs, over a sampling LOOP, in fp16 -- held where the
shipped fp16 launch sequences really run: 64^3, N = 1, 16 classes is the smallest shape at which the first-layer kernel
(16 + 1 input channels), the wide-tile convolution (16 x 8 x 8 = 1024 base workgroups for d0b and u0b), the level-0 folded
up-convolution (512 tiles >= 200) and, for Swin, fold_up[0] / res_up[0] are all chosen.  The loops of test_diffunet_gpu.py and
test_swin.py run at 32^3 or on 8-channel layers, where none of them is.  Every case first asserts which kernels its plan chose.

Inputs and oracle: tests/loop_parity_cases.py (a: 10-step DDIM, b: the last 20 steps of the 1000-step DDPM process through
sample_loop(first_step=980), c: DiffSwinUNETR 10-step DDIM).  tools/loop_parity_floor.py measured, for the seeds in use, what
rounding the model's x input through fp16 ALONE does to the oracle's own Dice: at most a quarter of the bound.

Also here: sample_loop(first_step=s) from a snapshot repeats the full run's bits."""
import os

import pytest
import torch

import loop_parity_cases as L

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


# max / mean |d| against the oracle at 3x what the MI355X measured (the results are bit-reproducible; the margin is for later
# legitimate re-orderings).  a, c: (sum of the x0 predictions, final state); b: x_0.
# Measured, with worst-class 1 - Dice (bound 1e-3; fp16-input floor of the inputs 9.4e-5 / 1.8e-4 / 8.8e-5):
#   a  sum 1.488e-2 / 1.708e-3, state 4.209e-3 / 5.086e-4, 1 - Dice 4.72e-4
#   b  x_0 8.390e-3 / 4.118e-4, 1 - Dice 8.17e-4; drift after 981 / 990 / 998 / 1000 steps: max 3.87e-4 / 1.64e-3 / 3.99e-3 / 8.39e-3
#   c  sum 2.824e-2 / 3.385e-3, state 8.553e-3 / 9.063e-4, 1 - Dice 7.20e-4
BOUNDS = {"a": ((3 * 1.488e-2, 3 * 1.708e-3), (3 * 4.209e-3, 3 * 5.086e-4)),
          "b": (3 * 8.390e-3, 3 * 4.118e-4),
          "c": ((3 * 2.824e-2, 3 * 3.385e-3), (3 * 8.553e-3, 3 * 9.063e-4))}


def _threads():
    torch.set_num_threads(max(1, min(16, len(os.sched_getaffinity(0)))))


def _dice(got, want):
    from oracle.unet_ref import binarise, dice_coeff
    a, b = binarise(got), binarise(want)
    return [dice_coeff(a[:, c], b[:, c]) for c in range(a.shape[1])]


def _assert_balanced(want):
    """On the ORACLE's result alone: no class mask so small or so full that a handful of voxels decides its Dice."""
    from oracle.unet_ref import binarise
    sh = L.shares(binarise(want))
    assert L.SHARE_MIN < min(sh) and max(sh) < L.SHARE_MAX, sh


def _diff(what, got, want, bound):
    d = (got.cpu() - want).abs()
    mx, mean = float(d.max()), float(d.mean())
    print(f"{what}: |d| max {mx:.3e} mean {mean:.3e}")
    assert mx < bound[0] and mean < bound[1], (what, mx, mean)


@pytest.fixture(scope="module")
def unet():
    """Cases a and b: the fp16 DiffUNet at default widths on the device, its oracle, and the 64^3 plan -- with the shipped
    kernels asserted, by the calls Plan._level0_layout makes."""
    from diff_unet_amos_amd import ops
    _threads()
    net, ref = L.unet_nets(torch.float16)
    net = net.cuda()
    plan = net._rt.plan(1, L.DIMS, DEV)
    assert [plan._fold_level(l) for l in range(4)] == [True, False, False, False]
    assert plan._level0_layout() == (True, True, True)
    (a0, b0), (u0a, u0b) = plan.den[0], plan.dec[0]
    kind = lambda *a: ops.conv3_kernel_kind(torch.float16, 1, *L.DIMS, *a)          # noqa: E731
    assert plan.cin0 >= L.CLASSES + 1 and a0.tap == 16
    assert kind(plan.cin0, plan.cin0, a0.cout, False, a0.tap) == ops.KIND_FIRST
    assert kind(a0.cout, plan.f[0], b0.cout, True) == ops.KIND_WIDE                 # d0b
    assert kind(u0a.cout, plan.dec_out[0], u0b.cout, True) == ops.KIND_WIDE         # u0b
    assert plan.finish_fp32_steps == 2
    return net, ref, plan


def _ddim_case(name, net, ref, plan, inp, bound_sum, bound_state):
    want = L.oracle_ddim(ref, inp)
    _assert_balanced(want["sum"])
    xT = inp["xT"].cuda()
    with torch.no_grad():
        net.embed_model(inp["image"].cuda())
        eager = {k: v.clone() for k, v in plan.sample_loop(net.sample_diffusion, "ddim", noise=xT, use_graph=False).items()}
        graph = plan.sample_loop(net.sample_diffusion, "ddim", noise=xT, use_graph=True)
    for k in ("sample", "sum_pred_xstart"):
        assert torch.equal(eager[k], graph[k]), k
    dice = _dice(graph["sum_pred_xstart"].cpu(), want["sum"])
    print(f"\n[{name}] 1 - Dice(build, oracle) of the binarised sum: max {1 - min(dice):.2e}; per class {[f'{1 - d:.1e}' for d in dice]}")
    _diff(f"[{name}] sum of x0 predictions", graph["sum_pred_xstart"], want["sum"], bound_sum)
    _diff(f"[{name}] final state", graph["sample"], want["sample"], bound_state)
    assert min(dice) > 1 - 1e-3, dice


def test_diffunet_ddim_loop_on_the_shipped_kernels_holds_the_dice_bound(unet):
    """a: RefDiffUNet.ddim_sample(image, x_T=[xT], step_noise=zeros) against plan.sample_loop(net.sample_diffusion, "ddim"),
    eager and replayed from the captured graph (same bits)."""
    net, ref, plan = unet
    inp = L.inputs_a()
    with torch.no_grad():           # the oracle of loop_parity_cases IS ddim_sample's: the same calls in the same order
        assert torch.equal(ref.ddim_sample(inp["image"], x_T=[inp["xT"]], step_noise=[[torch.zeros_like(inp["xT"])] * 10]),
                           L.oracle_ddim(ref, inp)["sum"])
    _ddim_case("a: DiffUNet DDIM x10", net, ref, plan, inp, BOUNDS["a"][0], BOUNDS["a"][1])


def test_diffunet_ddpm_tail_on_the_shipped_kernels_holds_the_dice_bound(unet):
    """b: the last 20 steps of the 1000-step process from x_19 = q_sample(ball labels), every step's noise injected: 18 steps of
    the fp16 plan and the two finishing steps of its fp32 companion, as shipped, against RefDiffusion.p_sample."""
    net, ref, plan = unet
    inp = L.inputs_b(ref)
    T, marks = 1000, (981, 990, 998, 1000)
    want = L.oracle_ddpm_tail(ref, inp, marks)
    _assert_balanced(want["sample"])
    snaps = {m: None for m in marks}
    with torch.no_grad():
        net.embed_model(inp["image"].cuda())
        out = plan.sample_loop(net.diffusion, "ddpm", noise=inp["x_start"].cuda(), step_noise=inp["draws"],
                               first_step=T - L.K_TAIL, snapshots=snaps)
    line = []
    for m in marks:
        d = (snaps[m].cpu() - want[m]).abs()
        line.append(f"{m}: {d.max():.2e}/{d.mean():.2e}")
    print("\n[b: DiffUNet DDPM 980..999] drift (max/mean |dx| after k steps): " + ", ".join(line))
    assert torch.equal(snaps[T], out["sample"]) and torch.isfinite(out["sample"]).all()
    dice = _dice(out["sample"].cpu(), want["sample"])
    print(f"[b] 1 - Dice(build, oracle) of the binarised x_0: max {1 - min(dice):.2e}; per class {[f'{1 - d:.1e}' for d in dice]}")
    _diff("[b] x_0", out["sample"], want["sample"], BOUNDS["b"])
    assert min(dice) > 1 - 1e-3, dice


def test_diff_swin_unetr_ddim_loop_in_fp16_holds_the_dice_bound():
    """c: the fp16 Swin plan (fold_up, res_up, the wide token GEMM, the two-stream step order) over 10 DDIM steps."""
    _threads()
    net, ref = L.swin_nets(torch.float16)
    net = net.cuda()
    plan = net._rt.plan(1, L.DIMS, DEV)
    assert plan.fold_up[:2] == [True, False] and plan.res_up[0]
    _ddim_case("c: DiffSwinUNETR DDIM x10", net, ref, plan, L.inputs_c(), BOUNDS["c"][0], BOUNDS["c"][1])


# ---- sample_loop(first_step=s) -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_loop_resumed_from_a_snapshot_repeats_the_full_run(dtype):
    """The 10-step DDPM loop of the tiny network at 32^3 with in-kernel noise (seed 7), and the same loop started at step 4 from
    the full run's state after 4 steps: the noise is keyed by (call seed, step) and the statistics are integer sums, so the
    final sample has the same bits -- replayed from the graph (the counter word is put back to 4 behind the capture's warm-up
    step) and eagerly.  fp16: steps 4 .. 7 on the fp16 plan, 8 and 9 on its fp32 companion."""
    net, _ = L.unet_pair(dict(in_channels=1, out_channels=2, features=(8, 8, 16, 32, 64, 8)), dtype)
    net = net.cuda()
    g = torch.Generator().manual_seed(9)
    image, xT = torch.rand(1, 1, 32, 32, 32, generator=g).cuda(), torch.randn(1, 2, 32, 32, 32, generator=g).cuda()
    d10 = net.sample_diffusion
    with torch.no_grad():
        net.embed_model(image)
        plan = net._rt.plan(1, (32, 32, 32), DEV)
        snaps = {4: None}
        full = plan.sample_loop(d10, "ddpm", noise=xT, seed=7, snapshots=snaps)["sample"].clone()
        assert not plan.graphs
        graph = plan.sample_loop(d10, "ddpm", noise=snaps[4], first_step=4, seed=7, use_graph=True)["sample"].clone()
        assert len(plan.graphs) == 1 and int(plan.counter.item()) == 10
        again = plan.sample_loop(d10, "ddpm", noise=snaps[4], first_step=4, seed=7, use_graph=True)["sample"].clone()
        eager = plan.sample_loop(d10, "ddpm", noise=snaps[4], first_step=4, seed=7, use_graph=False)["sample"].clone()
        other = plan.sample_loop(d10, "ddpm", noise=snaps[4], first_step=5, seed=7, use_graph=True)["sample"]
    for got in (graph, again, eager):
        assert torch.equal(full, got), float((full - got).abs().max())
    assert not torch.equal(full, other)                         # one step fewer, other noise: the argument is not ignored
    for bad in (-1, 10):
        with pytest.raises(ValueError, match="first_step"):
            plan.sample_loop(d10, "ddpm", noise=xT, first_step=bad)
    with pytest.raises(NotImplementedError, match="fuse_runs"):
        plan.sample_loop(d10, "ddim", noise=xT, first_step=1, fuse_runs=1)
