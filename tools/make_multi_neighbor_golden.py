"""Generate tests/golden/multi_neighbor_golden.npz from the REFERENCE ITSELF (needs a checkout of aarchiiive/diff-unet-amos;
the tests only read the committed fixture).

    PYTHONDONTWRITEBYTECODE=1 python tools/make_multi_neighbor_golden.py <reference checkout>

losses/loss.py is loaded by file path and only its MultiNeighborLoss (:234-301) is run, on the CPU.  Its import-time
dependencies that this term never touches are placeholders: the names it imports from monai.losses are empty classes, and
the package-relative ``.utils`` is an empty module with a ``dist_map_transform`` attribute.  Nothing is copied: the fixture
is data only -- inputs and the reference's outputs for them.

Per case <c>: <c>_logits fp16 [N, C, D, H, W] (the reference's layout), <c>_classes int8 [N, D, H, W] (the class of each
voxel, -1 = none: labels = one-hot over C, an all-zero label column where -1), <c>_K = num_classes, <c>_value = the
reference's loss (fp32).
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

REF = sys.argv[1] if len(sys.argv) > 1 else None          # the reference checkout
OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")

MONAI_NAMES = ("FocalLoss", "DiceLoss", "DiceFocalLoss", "DiceCELoss", "GeneralizedDiceLoss", "GeneralizedDiceFocalLoss",
               "GeneralizedWassersteinDiceLoss")


def _ref_loss_module():
    sys.dont_write_bytecode = True
    monai = types.ModuleType("monai")
    monai_losses = types.ModuleType("monai.losses")
    for name in MONAI_NAMES:
        setattr(monai_losses, name, type(name, (), {}))
    monai.losses = monai_losses
    pkg = types.ModuleType("ref_losses")
    pkg.__path__ = []
    utils = types.ModuleType("ref_losses.utils")
    utils.dist_map_transform = None
    sys.modules.update({"monai": monai, "monai.losses": monai_losses, "ref_losses": pkg, "ref_losses.utils": utils})
    spec = importlib.util.spec_from_file_location("ref_losses.loss", os.path.join(REF, "losses", "loss.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def labels_from_classes(classes, C):
    """int8 [N, D, H, W] class map (-1 = none) -> fp32 one-hot [N, C, D, H, W]."""
    cl = torch.as_tensor(classes).long()
    onehot = torch.nn.functional.one_hot(cl.clamp(min=0), C).permute(0, 4, 1, 2, 3).float()
    return onehot * (cl >= 0).unsqueeze(1).float()


def _case(g, N, C, D, H, W, scale, none_frac=0.0):
    logits = (torch.randn(N, C, D, H, W, generator=g) * scale).half()
    classes = torch.randint(0, C, (N, D, H, W), generator=g)
    classes[torch.rand(N, D, H, W, generator=g) < none_frac] = -1
    return logits, classes.to(torch.int8)


def main():
    if not REF:
        raise SystemExit(__doc__)
    mn = _ref_loss_module()
    g = torch.Generator().manual_seed(20261015)
    cases = {}
    # non-cubic extent (a swap of d, h, w shows), C = 16, N = 2; sample 1 has no labelled voxel: fewer than 2 valid classes
    logits, classes = _case(g, 2, 16, 12, 16, 20, 3.0, 0.3)
    classes[1] = -1
    cases["noncubic"] = (logits, classes, 16)
    # depth 6 < K = 16 (classes 6..15 can never occur), and saturated logits: >= 20 at several depths of a column, so that
    # the fp32 sigmoid ties at 1.0 and the first of them wins
    logits, classes = _case(g, 2, 16, 6, 10, 14, 4.0, 0.5)
    sat = torch.rand(2, 16, 1, 10, 14, generator=g) < 0.4
    for d, v in ((1, 20.0), (3, 24.0), (4, 31.0)):
        logits[:, :, d:d + 1] = torch.where(sat, torch.tensor(v, dtype=torch.float16), logits[:, :, d:d + 1])
    cases["saturated"] = (logits, classes, 16)
    # K = 5 < C = 8: the channels beyond K still vote, their depth indices >= K are not classes
    logits, classes = _case(g, 3, 8, 10, 9, 7, 4.0, 0.2)
    cases["k_lt_c"] = (logits, classes, 5)

    out = {"provenance": np.array("losses/loss.py MultiNeighborLoss of the reference checkout, CPU fp32")}
    for name, (logits, classes, K) in cases.items():
        labels = labels_from_classes(classes, logits.shape[1])
        value = mn.MultiNeighborLoss(num_classes=K)(logits.float(), labels)
        assert value.grad_fn is None
        out[f"{name}_logits"] = logits.numpy()
        out[f"{name}_classes"] = classes.numpy()
        out[f"{name}_K"] = np.array(K, dtype=np.int32)
        out[f"{name}_value"] = np.array(float(value), dtype=np.float32)
        print(f"{name}: logits {tuple(logits.shape)}, K = {K}: loss = {float(value):.8g}")
    os.makedirs(OUT, exist_ok=True)
    np.savez_compressed(os.path.join(OUT, "multi_neighbor_golden.npz"), **out)


if __name__ == "__main__":
    main()
