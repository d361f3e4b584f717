"""``Diffusion``: the drop-in boundary of the hot path.

Same constructor, attributes and ``forward(image, x, step, pred_type)`` dispatch as the reference's
models/diffusion/diffusion.py:11-102; the three branches run on HIP kernels.  ``pred_type="denoise"`` under autograd
(what Trainer.training_step calls, train.py:258-268) runs the same kernels forward and their backward kernels through
``training.native_conv_denoise``; without grad it runs the inference launch plan (engine.py).
"""
from __future__ import annotations

from typing import Sequence

import torch
import torch.nn as nn

from .basic_unet import _wants_grad
from .gaussian_diffusion import UniformSampler, make_spaced, step_uncertainty_fusion


class Diffusion(nn.Module):
    def __init__(self, spatial_dims: int = 3, in_channels: int = 3, out_channels: int = 1, image_size: int = 96,
                 spatial_size: int = 96, features: Sequence[int] = (32, 64, 128, 256, 512), dropout: float = 0.2,
                 timesteps: int = 1000, mode: str = "train", sample_steps: int = 10, uncer_step: int = None):
        super().__init__()
        # None: ddim_sample returns the plain sum of the steps' predictions (the reference); R >= 1: R DDIM runs per window
        # fused by Step-Uncertainty Fusion (ddim_sample's docstring)
        self.uncer_step = uncer_step
        self.num_classes = out_channels
        self.mode = mode
        self.timesteps = timesteps
        self.embed_model: nn.Module = None
        self.model: nn.Module = None
        # diffusion.py:31-45: a full process for training and a respaced one for inference.
        # ``sample_steps`` (10 in the reference) is the only added knob: BASELINE configs use 10/50/1000.
        self.diffusion = make_spaced(timesteps, [timesteps])
        self.sample_diffusion = make_spaced(timesteps, [sample_steps])
        self.sampler = UniformSampler(timesteps)

    def forward(self, image: torch.Tensor = None, x: torch.Tensor = None, step: torch.Tensor = None,
                pred_type: str = None):
        if image is not None and x is not None:
            assert image.device == x.device
        if pred_type == "q_sample":
            return self.q_sample(x)
        if pred_type == "denoise":
            return self.denoise(image, x, step)
        if pred_type == "ddim_sample":
            return self.ddim_sample(image, uncer_step=getattr(self, "uncer_step", None))
        raise NotImplementedError(f"No such prediction type : {pred_type}")

    def q_sample(self, x: torch.Tensor):
        """diffusion.py:65-69: eps ~ N(0,1) (torch RNG), t ~ U{0..T-1} (numpy global RNG)."""
        noise = torch.randn_like(x)
        t, _ = self.sampler.sample(x.shape[0], x.device)
        return self.diffusion.q_sample(x, t, noise), t, noise

    def denoise(self, image: torch.Tensor, x: torch.Tensor, step: torch.Tensor) -> torch.Tensor:
        """diffusion.py:71-84."""
        assert image.size(0) == x.size(0) == step.size(0)
        if _wants_grad(x, image, *self.parameters()):
            from .training import native_conv_denoise     # HIP forward + backward kernels under autograd
            return native_conv_denoise(self, image, x, step, self.compute_dtype)
        embeddings = self.embed_model(image)
        return self.model(x=x, t=step, embeddings=embeddings, image=image)

    def ddim_sample(self, image: torch.Tensor, uncer_step: int = None) -> torch.Tensor:
        """diffusion.py:86-102: per window, encoder once, DDIM loop, sum of the clamped x0 predictions.

        The reference walks the batch one sample at a time; every sample is independent (own encoder pass, own
        x_T), so the HIP path runs the whole batch through one launch plan -- the small U-Net levels, which
        cannot fill 256 CUs with one 96^3 patch, get B times the workgroups.  ``batched_sampling = False``
        restores the per-sample loop.

        ``uncer_step`` = R >= 1 (``forward`` passes the attribute of that name; None, the default, is the path above,
        untouched): Diff-UNet's published rule, R DDIM runs per window fused by Step-Uncertainty Fusion
        (gaussian_diffusion.step_uncertainty_fusion has the formula).  R = 1 is not the plain sum: the steps are still
        weighted.  See ``_ddim_sample_suf``."""
        if uncer_step is not None:
            return self._ddim_sample_suf(image, int(uncer_step))
        shape1 = (1, self.num_classes, *image.shape[2:])
        with torch.no_grad():
            if getattr(self, "batched_sampling", True) and len(image) > 1:
                embeddings = self.embed_model(image)
                out = self.sample_diffusion.ddim_sample_loop(
                    self.model, (len(image), *shape1[1:]), model_kwargs={"image": image, "embeddings": embeddings})
                acc = torch.zeros((len(image), *shape1[1:]), device=image.device)
                for s in out["all_samples"]:
                    acc += s.to(image.device)
                return acc
            res = []
            for i in range(len(image)):
                batch = image[i, ...].unsqueeze(0)
                embeddings = self.embed_model(batch)
                out = self.sample_diffusion.ddim_sample_loop(self.model, shape1,
                                                             model_kwargs={"image": batch, "embeddings": embeddings})
                acc = torch.zeros(shape1, device=image.device)
                for s in out["all_samples"]:
                    acc += s.to(image.device)
                res.append(acc)
        return torch.cat(res, dim=0)

    def _ddim_sample_suf(self, image: torch.Tensor, R: int) -> torch.Tensor:
        """R DDIM runs per window and their Step-Uncertainty Fusion; returns the fused volume [B, C, D, H, W].

        One ``randn`` of B R rows gives every run its own x_T: row g R + r starts run r of window g.  With the HIP denoiser the
        image batch is repeated with ``repeat_interleave(R)`` and the B R rows run through ONE launch plan, each step followed by
        the fusion launch (SamplerDriver.sample_loop(fuse_runs=R)); that is R encoder passes per window where one would do, once
        per loop -- one evaluation in 1 + T -- rather than a second way of handing embeddings to a plan.  Any other model runs R
        generic loops from one encoder pass and ``step_uncertainty_fusion`` on their recorded outputs.
        ``batched_sampling = False`` keeps meaning one window at a time, which is then a batch of R."""
        if R < 1:
            raise ValueError(f"uncer_step must be None or >= 1, got {R}")
        B, C, dims = len(image), self.num_classes, tuple(image.shape[2:])
        res = []
        with torch.no_grad():
            noise = torch.randn(B * R, C, *dims, device=image.device)
            whole = getattr(self, "batched_sampling", True) and B > 1
            for lo, hi in ([(0, B)] if whole else [(i, i + 1) for i in range(B)]):
                img, x_T = image[lo:hi], noise[lo * R:hi * R]
                if getattr(self.model, "fused_engine", None) is not None:
                    rep = img.repeat_interleave(R, dim=0)
                    kw = {"image": rep, "embeddings": self.embed_model(rep)}
                    shape = ((hi - lo) * R, C, *dims)
                    fused = self.sample_diffusion._fused(self.model, shape, True, None, None, kw)
                    if fused is None:
                        raise RuntimeError("the HIP denoiser has no launch plan: it must be owned by a DiffUNet / DiffSwinUNETR")
                    out = fused.sample_loop(self.sample_diffusion, "ddim", shape, noise=x_T, model_kwargs=kw, fuse_runs=R)
                    res.append(out["fused_pred_xstart"])
                    continue
                kw = {"image": img, "embeddings": self.embed_model(img)}
                outputs, samples = [], []
                for r in range(R):
                    out = self.sample_diffusion.ddim_sample_loop(self.model, (hi - lo, C, *dims), noise=x_T[r::R].contiguous(),
                                                                 model_kwargs=kw)
                    outputs.append(out["all_model_outputs"])
                    samples.append(out["all_samples"])
                res.append(step_uncertainty_fusion(outputs, samples).to(image.device))
        return res[0] if len(res) == 1 else torch.cat(res, dim=0)
