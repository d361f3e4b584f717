"""Cache-policy bits on the denoiser step's loads and stores (csrc/common.hpp, DUA_CACHE_PARTS) move where a line is kept and
never a value.  What can go wrong is visibility, not arithmetic: a hand-off store that has not reached memory when the next
launch reads it, a streaming load served a line of the previous patch, a replayed graph that overlaps what eager launches with a
synchronise in between cannot.  So every check here is bit equality, on the buffers a step hands to the next one (x_state, xin).

1. three steps launched kernel by kernel with a device synchronise after every launch == the same three steps replayed from a
   captured graph (default-width fp16 plan at 64^3: the smallest extent at which the first-layer, wide, folded, plain, split-K,
   transposed-convolution, materialise and tail kernels all run -- asserted from the launcher's own answers);
2. encoder + two steps of image A, then of image B, then of A again from the same seed and state: both A runs equal, B differs;
3. one step of the odd-extent batch-2 plan of tests/test_launch_sequence_fp64.py twice in this process (reproducible), and
   against the same step in a child process on the library DUA_HIP_LIB names -- a build with -DDUA_CACHE_PARTS=0
   (tools/build_diag.sh cp0 -DDUA_CACHE_PARTS=0); skipped, saying so, when DUA_HIP_LIB is not set."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

FEATURES = (64, 64, 128, 256, 512, 64)
CLASSES = 16
DEV = "cuda:0"
SEED = 20240607
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WRAPPED = ("conv3d_k3", "upconv_k3", "deconv_k2s2", "materialize", "final_conv_sampler", "step_begin")


def _net():
    """Default widths, InstanceNorm affine away from (1, 0) so that the fused transforms are not identities."""
    from diff_unet_amos_amd.diff_unet import DiffUNet
    torch.manual_seed(0)
    net = DiffUNet(in_channels=1, out_channels=CLASSES, features=FEATURES, compute_dtype=torch.float16)
    with torch.no_grad():
        for n, p in net.named_parameters():
            if ".adn.N." in n:
                p.copy_(torch.randn_like(p) * 0.3 + (1.0 if n.endswith("weight") else 0.0))
    return net.cuda().eval()


def _inputs(N, dims, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(N, 1, *dims, generator=g), torch.randn(N, CLASSES, *dims, generator=g)


def _stage(plan, image, x, encoder=True):
    """The state every run starts from: the condition of ``image`` resident, x_T in x_state and xin, step counter and key reset."""
    with torch.no_grad():
        if encoder:
            plan.run_encoder(image.to(DEV))
        plan._reset(x.to(DEV))
    plan.x_sum.zero_()
    plan.counter.zero_()
    plan.err_word.zero_()
    plan.seed_word.fill_(SEED)


def _handoffs(plan):
    torch.cuda.synchronize()
    assert int(plan.err_word) == 0
    return {"x_state": plan.x_state.clone(), "xin": plan.xin.clone()}


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and bool((a.view(torch.uint8) == b.view(torch.uint8)).all())


def _assert_same(a, b, what):
    diff = [k for k in a if not _same_bits(a[k], b[k])]
    assert not diff, f"{what}: {diff} differ"


@pytest.fixture(scope="module")
def plan64():
    """(net, plan, (coef_table, row_of_step)) of the default-width fp16 plan at 64^3, shared by the first two tests."""
    net = _net()
    plan = net._rt.plan(1, (64, 64, 64), torch.device(DEV))
    plan.refresh_weights()
    yield net, plan, plan._step_tables(net.sample_diffusion, "ddpm", 0.0)
    torch.cuda.empty_cache()


def _synchronised_steps(plan, tables, nsteps, monkeypatch):
    """``nsteps`` DDPM steps as step_begin + Plan.denoiser_body + Plan.tail with a device synchronise after every launch; returns
    the set of kernels the launches took, as the launcher itself answers."""
    from diff_unet_amos_amd import _native as nv
    from diff_unet_amos_amd import ops
    coef_table, row_of_step = tables
    took = set()
    orig = {k: getattr(ops, k) for k in WRAPPED}

    def conv3d_k3(x, cin, cin_off, w_packed, bias_pad, cout, y, cout_off, out_stats, norm=None, workspace=None, tap_channel=None,
                  background=False, in_blocked=False, out_blocked=False):
        N, D, H, W, cs = x.shape
        d = nv.Conv3Desc(nv.dt_code(x.dtype), N, D, H, W, cin, cs, cin_off, cout, y.shape[-1], cout_off,
                         0 if tap_channel is None else tap_channel + 1, 0,
                         (nv.IN_BLOCKED if in_blocked else 0) | (nv.OUT_BLOCKED if out_blocked else 0), ops.CONV_POLICY)
        f = ops.conv3_form(d, norm is not None, 0 if workspace is None else workspace.numel() * workspace.element_size())
        kind = int(nv.lib().dua_conv3d_k3_kernel_kind(ctypes.byref(d), 1 if norm is not None else 0, 1 if f.ksplit > 1 else 0))
        took.add({0: "v2", 1: "first", 2: "wide"}[kind] + (" split-K" if f.ksplit > 1 else ""))
        orig["conv3d_k3"](x, cin, cin_off, w_packed, bias_pad, cout, y, cout_off, out_stats, norm=norm, workspace=workspace,
                          tap_channel=tap_channel, background=background, in_blocked=in_blocked, out_blocked=out_blocked)
        torch.cuda.synchronize()

    def named(key, label):
        def call(*a, **kw):
            took.add(label)
            orig[key](*a, **kw)
            torch.cuda.synchronize()
        return call

    monkeypatch.setattr(ops, "conv3d_k3", conv3d_k3)
    for key, label in (("upconv_k3", "fold"), ("deconv_k2s2", "deconv"), ("materialize", "materialize"),
                       ("final_conv_sampler", "tail"), ("step_begin", "step_begin")):
        monkeypatch.setattr(ops, key, named(key, label))
    with torch.no_grad():
        for _ in range(nsteps):
            ops.step_begin(plan.N, plan.temb_table, plan.cur_add, row_of_step=row_of_step, counter=plan.counter, coef_table=coef_table,
                           cur_coef=plan.cur_coef, step_word=plan.step_word, err_word=plan.err_word, clear=plan.den_stats)
            plan.denoiser_body(zero_stats=False)
            plan.tail(nv.MODE_DDPM)
    monkeypatch.undo()
    return took


def test_replay_sees_what_eager_sees(plan64, monkeypatch):
    from diff_unet_amos_amd import _native as nv
    net, plan, tables = plan64
    image, x = _inputs(1, (64, 64, 64), 11)
    _stage(plan, image, x)
    took = _synchronised_steps(plan, tables, 3, monkeypatch)
    want = _handoffs(plan)
    print(f"kernels of a 64^3 step: {sorted(took)}; level 0 folds: {plan._fold_level(0)}")
    need = {"first", "wide", "v2", "v2 split-K", "fold", "deconv", "materialize", "tail", "step_begin"}
    assert need <= took and plan._fold_level(0), f"the 64^3 plan does not reach {sorted(need - took)}: the case tests less than it claims"
    assert int(plan.counter) == 3

    def step():
        plan.native_step(nv.MODE_DDPM, row_of_step=tables[1], coef_table=tables[0])

    _stage(plan, image, x, encoder=False)
    with torch.no_grad():
        step()                                   # records the op list and warms the launch path up, outside the capture
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            step()
    _stage(plan, image, x, encoder=False)
    for _ in range(3):
        g.replay()
    got = _handoffs(plan)
    assert int(plan.counter) == 3
    _assert_same(want, got, "three replayed steps against three steps synchronised after every launch")
    assert bool(torch.isfinite(got["x_state"]).all()) and float(got["x_state"].std()) > 0


def test_a_new_patch_is_not_served_stale_bytes(plan64):
    from diff_unet_amos_amd import _native as nv
    net, plan, tables = plan64
    image_a, x = _inputs(1, (64, 64, 64), 12)
    image_b = torch.rand(1, 1, 64, 64, 64, generator=torch.Generator().manual_seed(13))

    def run(image):
        _stage(plan, image, x)
        with torch.no_grad():
            for _ in range(2):
                plan.native_step(nv.MODE_DDPM, row_of_step=tables[1], coef_table=tables[0])
        out = _handoffs(plan)
        out["emb[0]"] = plan.emb[0].clone()
        out["cat[0]"] = plan.cat[0].clone()
        return out

    a1, b, a2 = run(image_a), run(image_b), run(image_a)
    _assert_same(a1, a2, "image A before and after image B, same seed and state")
    same = [k for k in a1 if _same_bits(a1[k], b[k])]
    assert not same, f"another image left {same} unchanged"
    assert bool(torch.isfinite(a1["x_state"]).all())


ODD = dict(N=2, dims=(63, 48, 40), seed=14)


def _odd_step(net=None):
    """One DDPM step of the odd-extent batch-2 plan from its staged state: (net, hand-off buffers)."""
    from diff_unet_amos_amd import _native as nv
    net = net or _net()
    plan = net._rt.plan(ODD["N"], ODD["dims"], torch.device(DEV))
    plan.refresh_weights()
    tables = plan._step_tables(net.sample_diffusion, "ddpm", 0.0)
    _stage(plan, *_inputs(ODD["N"], ODD["dims"], ODD["seed"]))
    with torch.no_grad():
        plan.native_step(nv.MODE_DDPM, row_of_step=tables[1], coef_table=tables[0])
    return net, _handoffs(plan)


def test_odd_extents_and_batch_rows_against_the_build_without_policy_bits(tmp_path):
    from diff_unet_amos_amd import _native as nv
    net, first = _odd_step()
    _, second = _odd_step(net)
    _assert_same(first, second, "two runs of the (63, 48, 40) batch-2 step in this build")
    assert bool(torch.isfinite(first["x_state"]).all()) and not _same_bits(first["x_state"][0], first["x_state"][1])
    other = os.environ.get("DUA_HIP_LIB")
    if not other:
        pytest.skip("DUA_HIP_LIB is not set: no build with -DDUA_CACHE_PARTS=0 to compare against "
                    "(tools/build_diag.sh cp0 -DDUA_CACHE_PARTS=0, then DUA_HIP_LIB=tools/diag/cp0/libdua_hip.so)")
    other = os.path.abspath(other)
    assert os.path.isfile(other), other
    # the child runs on the library this process does NOT run on
    env = {k: v for k, v in os.environ.items() if k != "DUA_DEBUG"}
    if os.path.abspath(nv.LIB_PATH) != other:
        env["DUA_DEBUG"] = "1"
    env["DUA_HIP_LIB"] = other
    out = tmp_path / "other.pt"
    subprocess.run([sys.executable, os.path.abspath(__file__), str(out)], cwd=ROOT, env=env, check=True, timeout=300)
    theirs = torch.load(out, map_location=DEV)
    assert os.path.abspath(theirs.pop("lib")) != os.path.abspath(nv.LIB_PATH), "both runs used the same library"
    _assert_same(first, theirs, "the (63, 48, 40) batch-2 step in this build and in the build DUA_HIP_LIB names")


if __name__ == "__main__":          # the child of the last test: the same step on whatever library the environment selects
    sys.path.insert(0, ROOT)
    from diff_unet_amos_amd import _native

    _, bufs = _odd_step()
    torch.save({**{k: v.cpu() for k, v in bufs.items()}, "lib": _native.LIB_PATH}, sys.argv[1])
