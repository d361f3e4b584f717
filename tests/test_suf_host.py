"""Step-Uncertainty Fusion above the kernel, without a GPU: SamplerDriver.sample_loop(fuse_runs=R) on a stub plan of its own (the
hooks replaced by recorders, as tests/test_sampler_driver.py does for the plain loop), Diffusion.ddim_sample(uncer_step=R) on a
tiny CPU model through the generic path against the fp64 reference, and dua_suf_accumulate's argument errors."""
import ctypes as C

import pytest
import torch
import torch.nn as nn

import suf_fp64ref as sf
from diff_unet_amos_amd import _native as nv
from diff_unet_amos_amd.diffusion import Diffusion
from diff_unet_amos_amd.gaussian_diffusion import make_spaced, suf_step_coef
from diff_unet_amos_amd.sampler_driver import SamplerDriver

T = 5


class _Graph:
    def __init__(self, log):
        self.log = log

    def replay(self):
        self.log.append(("replay",))


class StubPlan(SamplerDriver):
    """N = 4 rows of 2 classes at 2^3 on the CPU; every hook a recorder."""

    def __init__(self, N=4, finish=0):
        self.N, self.C, self.dims, self.dev = N, 2, (2, 2, 2), torch.device("cpu")
        self.cx = 8
        self.xin = torch.zeros(N, 2, 2, 2, 8)
        self.temb_table = torch.zeros(1000, 4)
        self.finish, self.log = finish, []
        self._alloc_sampler_state(self.N, self.dims, self.cx, self.dev)

    def refresh_weights(self):
        self.log.append(("refresh_weights",))

    def _reset(self, x_T):
        self.log.append(("reset", x_T))

    def _result(self, want_sum):
        return {"want_sum": want_sum}

    def _one_step(self, mode, row_of_step, coef_table, eps, want_sum):
        self.log.append(("step", mode, row_of_step, coef_table, eps, want_sum))

    def _one_step_logits(self, mode, row_of_step, coef_table, eps, logits):
        self.log.append(("step_logits", mode, row_of_step, coef_table, eps, logits))
        logits += 1.0

    def _accumulate_runs(self, logits, acc, step_coef):
        self.log.append(("accumulate", logits, acc, step_coef))
        acc += logits.reshape(acc.shape[0], -1, *acc.shape[1:]).sum(1)

    def _evaluate(self, rows, out):
        self.log.append(("evaluate", rows))

    def _capture(self, step_fn):
        self.log.append(("capture", step_fn))
        return _Graph(self.log)

    def _finish_count(self, kind, T):
        return self.finish

    def _finish(self, first_step, T, run):
        self.log.append(("finish", first_step, T))

    def names(self):
        return [e[0] for e in self.log if e[0] != "refresh_weights"]


@pytest.fixture(scope="module")
def diffusion():
    return make_spaced(1000, [T])


@pytest.fixture
def x_T():
    return torch.zeros(4, 2, 2, 2, 2)


def test_fuse_runs_drives_the_new_hook_once_per_step(diffusion, x_T):
    p = StubPlan()
    draws = [torch.full((4, 2, 2, 2, 2), float(k)) for k in range(T)]
    recorded = []
    out = p.sample_loop(diffusion, "ddim", noise=x_T, step_noise=draws, seed=1, fuse_runs=2, step_logits=recorded)
    assert p.names() == ["reset"] + ["step_logits", "accumulate"] * T and not p.graphs
    coef_table, row_of_step = p.tables[(diffusion, "ddim", 0.0)]
    step_coef = p.tables[(diffusion, "suf")]
    assert torch.equal(step_coef, suf_step_coef(T)) and step_coef.dtype == torch.float32
    steps = [e for e in p.log if e[0] == "step_logits"]
    for k, (_, mode, rows, coef, eps, logits) in enumerate(steps):
        assert mode == nv.MODE_DDIM and rows is row_of_step and coef is coef_table and torch.equal(eps, draws[k])
        assert logits is p.suf_logits and tuple(logits.shape) == (4, 2, 2, 2, 2) and logits.dtype == torch.float32
    for _, logits, acc, coef in (e for e in p.log if e[0] == "accumulate"):
        assert logits is p.suf_logits and acc is p.suf_acc[2] and coef is step_coef
    assert tuple(p.suf_acc[2].shape) == (2, 2, 2, 2, 2) and p.suf_acc[2].dtype == torch.float32
    # the result: no plain sum, the fused volume a copy of the accumulator (the stub adds k + 1 per run at step k)
    assert out["want_sum"] is False and set(out) == {"want_sum", "fused_pred_xstart"}
    assert torch.equal(out["fused_pred_xstart"], torch.full((2, 2, 2, 2, 2), 2.0 * sum(range(1, T + 1))))
    assert out["fused_pred_xstart"] is not p.suf_acc[2]
    assert [float(t.flatten()[0]) for t in recorded] == [float(k + 1) for k in range(T)] and all(t is not p.suf_logits for t in recorded)
    # a second loop starts from a zeroed accumulator
    del p.log[:]
    p.suf_logits.zero_()
    again = p.sample_loop(diffusion, "ddim", noise=x_T, use_graph=False, seed=1, fuse_runs=2)
    assert torch.equal(again["fused_pred_xstart"], out["fused_pred_xstart"])
    assert [e[4] for e in p.log if e[0] == "step_logits"] == [None] * T          # in-kernel noise without step_noise


def test_fuse_runs_captures_once_under_its_own_key(diffusion, x_T):
    p = StubPlan()
    p.sample_loop(diffusion, "ddim", noise=x_T, seed=1, fuse_runs=2)
    assert p.names() == ["reset", "capture", "reset"] + ["replay"] * T
    key = (diffusion, "ddim", 0.0, False, "fuse_runs", 2)
    assert list(p.graphs) == [key]
    step_fn = next(e[1] for e in p.log if e[0] == "capture")
    del p.log[:]
    step_fn()                                                                   # what was captured: the step, then the accumulate
    assert p.names() == ["step_logits", "accumulate"] and p.log[0][4] is None
    del p.log[:]
    p.sample_loop(diffusion, "ddim", noise=x_T, seed=2, fuse_runs=2)            # same key: nothing captured
    assert p.names() == ["reset"] + ["replay"] * T and len(p.graphs) == 1
    p.sample_loop(diffusion, "ddim", noise=x_T, seed=2)                         # the plain loop keeps its own graph
    p.sample_loop(diffusion, "ddim", noise=x_T, seed=2, fuse_runs=4)            # another R: another graph and accumulator
    assert set(p.graphs) == {key, (diffusion, "ddim", 0.0, True), (diffusion, "ddim", 0.0, False, "fuse_runs", 4)}
    assert tuple(p.suf_acc[4].shape) == (1, 2, 2, 2, 2)


def test_fuse_runs_rejects_before_any_hook(diffusion, x_T):
    p = StubPlan()
    with pytest.raises(NotImplementedError, match="DDIM"):
        p.sample_loop(diffusion, "ddpm", noise=x_T, seed=1, fuse_runs=2)
    for bad in (3, 0, -2, nv.SUF_MAX_RUNS + 4):
        with pytest.raises(ValueError, match="fuse_runs"):
            p.sample_loop(diffusion, "ddim", noise=x_T, seed=1, fuse_runs=bad)
    assert p.log == [] and not p.graphs and not p.tables and not hasattr(p, "suf_logits")
    p = StubPlan(finish=2)                                                      # finishing steps on a companion plan: not fused
    with pytest.raises(NotImplementedError):
        p.sample_loop(diffusion, "ddim", noise=x_T, seed=1, fuse_runs=2)
    assert p.log == []


def test_without_fuse_runs_the_calls_are_todays(diffusion, x_T):
    p = StubPlan()
    out = p.sample_loop(diffusion, "ddim", noise=x_T, use_graph=False, seed=1)
    assert out == {"want_sum": True}
    assert p.names() == ["reset"] + ["step"] * T
    coef_table, row_of_step = p.tables[(diffusion, "ddim", 0.0)]
    assert all(e[1:] == (nv.MODE_DDIM, row_of_step, coef_table, None, True) for e in p.log if e[0] == "step")
    assert list(p.tables) == [(diffusion, "ddim", 0.0)] and not hasattr(p, "suf_logits")
    del p.log[:]
    p.sample_loop(diffusion, "ddim", noise=x_T, seed=1)
    assert p.names() == ["reset", "capture", "reset"] + ["replay"] * T and list(p.graphs) == [(diffusion, "ddim", 0.0, True)]


# ---- Diffusion.ddim_sample(uncer_step=R) through the generic path -------------------------------------------------------------
class _Encoder(nn.Module):
    def forward(self, image):
        return [image * (i + 1) for i in range(5)]


class _Denoiser(nn.Module):
    """Any callable that is not the HIP denoiser (no ``fused_engine``): logits from x_t, t, the image and an embedding."""

    def forward(self, x, t, image=None, embeddings=None):
        return 3.0 * x * (1.0 + 0.2 * t.view(-1, 1, 1, 1, 1).float()) + 8.0 * (image - 0.5) + 0.25 * embeddings[1]


class _TorchDDIM:
    """A sampling process in torch operators with ddim_sample_loop's interface (the package's own runs its update on the GPU)."""

    def __init__(self, steps):
        self.num_timesteps = steps

    def ddim_sample_loop(self, model, shape, noise=None, model_kwargs=None):
        x = noise if noise is not None else torch.randn(*shape)
        outs, xs = [], []
        for i in reversed(range(self.num_timesteps)):
            out = model(x, torch.tensor([i] * shape[0]), **model_kwargs)
            x0 = out.clamp(-1, 1)
            x = 0.6 * x0 + 0.4 * x
            outs.append(out)
            xs.append(x0)
        return {"sample": x, "all_samples": xs, "all_model_outputs": outs}


def _tiny(steps=3, classes=3):
    net = Diffusion(out_channels=classes, sample_steps=steps)
    net.embed_model, net.model = _Encoder(), _Denoiser()
    net.sample_diffusion = _TorchDDIM(steps)
    return net


@pytest.mark.parametrize("R", [1, 2, 3])
def test_ddim_sample_with_uncer_step_equals_the_fp64_fusion(R):
    steps, classes, B, dims = 3, 3, 2, (3, 4, 5)
    net = _tiny(steps, classes)
    image = torch.rand(B, 1, *dims, generator=torch.Generator().manual_seed(5))
    torch.manual_seed(11)
    got = net.ddim_sample(image, uncer_step=R)
    assert tuple(got.shape) == (B, classes, *dims) and got.dtype == torch.float32
    # the same loops by hand: one randn of B R rows, row g R + r starts run r of window g
    torch.manual_seed(11)
    x_T = torch.randn(B * R, classes, *dims)
    kw = {"image": image, "embeddings": net.embed_model(image)}
    runs = [net.sample_diffusion.ddim_sample_loop(net.model, (B, classes, *dims), noise=x_T[r::R].contiguous(), model_kwargs=kw)
            for r in range(R)]
    step_logits = [torch.stack([runs[r]["all_model_outputs"][k] for r in range(R)], 1).reshape(B * R, classes, *dims)
                   for k in range(steps)]
    ref, bound = sf.loop_ref(step_logits, B)
    res = sf.check(got, ref, bound)
    print(f"R = {R}: {res}")
    assert res.ratio <= 1.0
    # through forward (the attribute), and one window at a time: the same bits
    net.uncer_step = R
    torch.manual_seed(11)
    assert torch.equal(net(image, pred_type="ddim_sample"), got)
    net.batched_sampling = False
    torch.manual_seed(11)
    assert torch.equal(net(image, pred_type="ddim_sample"), got)
    # R = 1 still weights the steps: not the plain sum
    if R == 1:
        plain = sum(runs[0]["all_samples"])
        assert float((got - plain).abs().max()) > 0.1


def test_ddim_sample_without_uncer_step_is_todays():
    net = _tiny()
    assert net.uncer_step is None
    image = torch.rand(2, 1, 3, 4, 5, generator=torch.Generator().manual_seed(5))
    kw = {"image": image, "embeddings": net.embed_model(image)}
    torch.manual_seed(3)
    want = sum(net.sample_diffusion.ddim_sample_loop(net.model, (2, 3, 3, 4, 5), model_kwargs=kw)["all_samples"])
    for call in (lambda: net.ddim_sample(image), lambda: net.ddim_sample(image, uncer_step=None),
                 lambda: net(image, pred_type="ddim_sample")):
        torch.manual_seed(3)
        assert torch.equal(call(), want)
    with pytest.raises(ValueError, match="uncer_step"):
        net.ddim_sample(image, uncer_step=0)


def test_infer_and_the_sliding_window_take_a_model_with_the_switch_set():
    """The model carries the switch: infer / sliding_window_inference need no argument.  One window: the binarised fusion;
    several windows in batches of two: the volume's shape."""
    from diff_unet_amos_amd.inference import binarise, infer, sliding_window_inference
    net = _tiny()
    net.uncer_step = 2
    image = torch.rand(1, 1, 4, 4, 4, generator=torch.Generator().manual_seed(5))
    torch.manual_seed(7)
    want = binarise(net.ddim_sample(image, uncer_step=2))
    torch.manual_seed(7)
    assert torch.equal(infer(net, image, roi_size=(4, 4, 4)), want)
    volume = torch.rand(1, 1, 4, 6, 9, generator=torch.Generator().manual_seed(6))
    out = sliding_window_inference(volume, (4, 4, 4), 2, net, overlap=0.25, pred_type="ddim_sample")
    assert tuple(out.shape) == (1, 3, 4, 6, 9) and bool(torch.isfinite(out).all())
    assert set(infer(net, volume, roi_size=(4, 4, 4), sw_batch_size=2).unique().tolist()) <= {0.0, 1.0}


def test_models_take_uncer_step_as_a_constructor_keyword():
    from diff_unet_amos_amd.diff_swin_unetr import DiffSwinUNETR
    from diff_unet_amos_amd.diff_unet import DiffUNet
    kw = dict(in_channels=1, out_channels=2, features=(8, 8, 16, 32, 64, 8))
    assert DiffUNet(**kw).uncer_step is None and DiffUNet(uncer_step=4, **kw).uncer_step == 4
    assert DiffSwinUNETR(in_channels=1, out_channels=2, feature_size=48).uncer_step is None
    assert DiffSwinUNETR(in_channels=1, out_channels=2, feature_size=48, uncer_step=2).uncer_step == 2


# ---- the entry point's argument errors (the library alone, no device) ---------------------------------------------------------
def test_suf_accumulate_rejects_bad_arguments_before_touching_the_device():
    lib = nv.lib()
    one = C.c_void_p(16)
    good = dict(G=2, R=4, C=3, vox=315, logits=one, coef=one, nsteps=10, step_word=one, step=0, err=None, acc=one)

    def call(**over):
        a = {**good, **over}
        return lib.dua_suf_accumulate(a["G"], a["R"], a["C"], a["vox"], a["logits"], a["coef"], a["nsteps"], a["step_word"],
                                      a["step"], a["err"], a["acc"], None)

    for over in (dict(G=0), dict(G=65536), dict(R=0), dict(R=nv.SUF_MAX_RUNS + 1), dict(C=0), dict(vox=0), dict(vox=-4),
                 dict(nsteps=0), dict(logits=None), dict(coef=None), dict(acc=None),
                 dict(step_word=None, step=-1), dict(step_word=None, step=10), dict(C=2 ** 20, vox=2 ** 40)):
        assert call(**over) == nv.ERR_ARG, over
    src = open(nv.LIB_PATH[:-len("libdua_hip.so")] + "../include/dua_hip.h").read()
    assert f"#define DUA_SUF_MAX_RUNS {nv.SUF_MAX_RUNS}\n" in src
