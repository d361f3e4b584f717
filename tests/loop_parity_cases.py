"""Inputs and oracle runs of tests/test_loop_parity_gpu.py: the three sampling loops at the smallest shape at which every shipped
fp16 kernel is chosen (64^3 patch, N = 1, 16 classes).  CPU only -- no device, no plan -- so that tools/loop_parity_floor.py can
run the same inputs through the oracle alone and say how much of the Dice bound the inputs themselves use up.

  a  DiffUNet, default widths, 10-step DDIM (eta 0), sum of the clamped x0 predictions
  b  DiffUNet, default widths, the last K = 20 steps of the 1000-step DDPM process, every step's noise injected
  c  DiffSwinUNETR, feature size 48, 10-step DDIM (eta 0), sum of the clamped x0 predictions

``round_from``: the oracle with ONLY the model's x input rounded through fp16 on the steps whose model timestep is >= round_from
(the steps the product runs on fp16 operands; its posterior arithmetic and its state stay fp32).  None = the oracle itself."""
import math

import torch

DIMS = (64, 64, 64)
CLASSES = 16
K_TAIL = 20                      # case b: steps 980 .. 999 of the 1000-step process (model timesteps 19 .. 0)
SEED_WEIGHTS_UNET = 0
SEED_INPUTS_A = 41
SEED_INPUTS_B = 41
SEED_WEIGHTS_SWIN = 3
SEED_INPUTS_C = 4
SHARE_MIN, SHARE_MAX = 0.02, 0.98


def unet_pair(kw, dtype, seed=0, sample_steps=10, affine_noise=True):
    """(DiffUNet on the host, RefDiffUNet) with one state dict -- test_diffunet_gpu._pair before its .cuda()."""
    from diff_unet_amos_amd.diff_unet import DiffUNet
    from oracle.unet_ref import RefDiffUNet
    torch.manual_seed(seed)
    ref = RefDiffUNet(sample_steps=sample_steps, **kw).eval()
    if affine_noise:
        with torch.no_grad():
            for n, p in ref.named_parameters():
                if ".adn.N." in n:
                    p.copy_(torch.randn_like(p) * 0.3 + (1.0 if n.endswith("weight") else 0.0))
    net = DiffUNet(sample_steps=sample_steps, compute_dtype=dtype, **kw)
    net.load_state_dict(ref.state_dict())
    return net.eval(), ref


def swin_pair(classes, dtype, seed=0, sample_steps=10):
    """(DiffSwinUNETR on the host, its oracle) with one state dict -- test_swin._swin_pair before its .cuda(), both sides on the
    ``sample_steps``-step respacing of the 1000-step process."""
    from diff_unet_amos_amd.diff_swin_unetr import DiffSwinUNETR
    from diff_unet_amos_amd.gaussian_diffusion import make_spaced
    from oracle.diffusion_ref import RefDiffusion
    from oracle.swin_ref import make_ref_diff_swin_unetr
    torch.manual_seed(seed)
    net = DiffSwinUNETR(in_channels=1, out_channels=classes, feature_size=48, compute_dtype=dtype).eval()
    with torch.no_grad():
        for k, p in net.named_parameters():
            if "relative_position_bias_table" in k:
                p.normal_(0, 0.3)                   # visible position bias (the default init is N(0, 0.02))
    ref = make_ref_diff_swin_unetr(1, classes, 48).eval()
    ref.load_state_dict(net.state_dict())
    net.sample_diffusion = make_spaced(1000, [sample_steps])
    ref.sample_diffusion = RefDiffusion(1000, [sample_steps])
    return net, ref


def unet_nets(dtype=torch.float16):
    """The pair of cases a and b."""
    return unet_pair(dict(in_channels=1, out_channels=CLASSES), dtype, seed=SEED_WEIGHTS_UNET)


def swin_nets(dtype=torch.float16):
    """The pair of case c."""
    return swin_pair(CLASSES, dtype, seed=SEED_WEIGHTS_SWIN)


def ddim_inputs(seed):
    g = torch.Generator().manual_seed(seed)
    return {"image": torch.rand(1, 1, *DIMS, generator=g), "xT": torch.randn(1, CLASSES, *DIMS, generator=g)}


def inputs_a():
    return ddim_inputs(SEED_INPUTS_A)


def inputs_c():
    return ddim_inputs(SEED_INPUTS_C)


def label_balls():
    """A +-1 label volume [1, CLASSES, 64, 64, 64]: one ball per class, centres on a tilted circle around the patch centre."""
    z, y, x = torch.meshgrid(*[torch.arange(n, dtype=torch.float32) for n in DIMS], indexing="ij")
    out = torch.empty(1, CLASSES, *DIMS)
    for c in range(CLASSES):
        a = 2 * math.pi * c / CLASSES
        cz, cy, cx = 32 + 13 * math.cos(a), 32 + 13 * math.sin(a), 32 + 9 * math.cos(2 * a + 1)
        r = 11 + 2 * (c % 4)
        out[0, c] = ((z - cz) ** 2 + (y - cy) ** 2 + (x - cx) ** 2 < r * r).float() * 2 - 1
    return out


def inputs_b(ref):
    """x_19 = q_sample(x0, 19) of the ball volume under ``ref``'s 1000-step process, and the K_TAIL per-step draws."""
    g = torch.Generator().manual_seed(SEED_INPUTS_B)
    image = torch.rand(1, 1, *DIMS, generator=g)
    x0 = label_balls()
    x_start = ref.diffusion.q_sample(x0, torch.tensor([K_TAIL - 1]), torch.randn(1, CLASSES, *DIMS, generator=g))
    return {"image": image, "x0": x0, "x_start": x_start,
            "draws": [torch.randn(1, CLASSES, *DIMS, generator=g) for _ in range(K_TAIL)]}


class RoundedInput(torch.nn.Module):
    """``model`` with its x input rounded through fp16 wherever the model timestep is >= round_from."""

    def __init__(self, model, round_from):
        super().__init__()
        self.model, self.round_from = model, round_from

    def forward(self, x, t, **kw):
        if int(t.min()) >= self.round_from:
            x = x.half().float()
        return self.model(x, t, **kw)


def _model(ref, round_from):
    return ref.model if round_from is None else RoundedInput(ref.model, round_from)


def oracle_ddim(ref, inp, round_from=None):
    """{"sum": sum of the clamped x0 predictions, "sample": x_0} of ref.sample_diffusion's DDIM loop at eta 0.  With
    round_from=None the sum is RefDiffUNet.ddim_sample(image, x_T=[xT], step_noise=zeros), the same calls in the same order."""
    T = ref.sample_diffusion.num_timesteps
    with torch.no_grad():
        emb = ref.embed_model(inp["image"])
        out = ref.sample_diffusion.ddim_sample_loop(_model(ref, round_from), inp["xT"], [torch.zeros_like(inp["xT"])] * T,
                                                    model_kwargs={"image": inp["image"], "embeddings": emb})
    acc = torch.zeros_like(inp["xT"])
    for s in out["all_samples"]:
        acc += s
    return {"sum": acc, "sample": out["sample"]}


def oracle_ddpm_tail(ref, inp, marks=(), round_from=None):
    """RefDiffusion.p_sample for t = K_TAIL - 1 .. 0 of the 1000-step process from inp["x_start"]: {"sample": x_0, absolute step
    count k in ``marks``: the state after k steps}."""
    T = ref.diffusion.num_timesteps
    model, res = _model(ref, round_from), {}
    with torch.no_grad():
        emb = ref.embed_model(inp["image"])
        img = inp["x_start"]
        for j, t in enumerate(reversed(range(K_TAIL))):
            img = ref.diffusion.p_sample(model, img, torch.tensor([t]), inp["draws"][j],
                                         model_kwargs={"image": inp["image"], "embeddings": emb})["sample"]
            if T - t in marks:
                res[T - t] = img.clone()
    res["sample"] = img
    return res


def shares(mask):
    """Per-class share of set voxels of a binarised [1, C, ...] volume."""
    return [float(mask[0, c].mean()) for c in range(mask.shape[1])]


def floor(a, b):
    """1 - min over classes of Dice(binarise(a), binarise(b))."""
    from oracle.unet_ref import binarise, dice_coeff
    a, b = binarise(a), binarise(b)
    return 1 - min(dice_coeff(a[:, c], b[:, c]) for c in range(a.shape[1]))
