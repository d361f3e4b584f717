"""Generate tests/golden/label_smoothing_golden.npz from the REFERENCE ITSELF (needs a checkout of aarchiiive/diff-unet-amos;
the tests only read the committed fixture).

    PYTHONDONTWRITEBYTECODE=1 python tools/make_label_smoothing_golden.py <reference checkout>

dataset/cache_dataset.py is loaded by file path and only ``LabelSmoothingCacheDataset.label_smoothing`` (:105-153, with
``rational`` :151-153) is run, on the CPU, on an instance made without its constructor (which would build a MONAI
CacheDataset) and given the four attributes the method reads.  The MONAI names the file imports are placeholders: empty
classes in empty modules.  Nothing is copied: the fixture is data only -- inputs and the reference's outputs for them.

Per case <c>: <c>_labels uint8 [E0, E1, E2] (class ids), <c>_K = num_classes, <c>_alpha, <c>_order, <c>_epsilon (float64 of
the Python floats passed), <c>_out fp32 [K, E0, E1, E2] (the reference's smoothed label), <c>_centroid_gap float64: the
largest difference between the centroids as the reference computes them (``indices[mask].mean(0)`` in fp32, restated here)
and the exact ones (integer sums divided in fp64) -- the tests add it to their bound.
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

REF = sys.argv[1] if len(sys.argv) > 1 else None          # the reference checkout
OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")


def _ref_dataset_class():
    sys.dont_write_bytecode = True
    names = {"monai": (), "monai.data": ("CacheDataset",), "monai.data.utils": ("pickle_hashing",),
             "monai.transforms": ("LoadImaged", "RandomizableTrait", "Transform", "convert_to_contiguous", "Compose")}
    mods = {}
    for mod_name, attrs in names.items():
        mod = types.ModuleType(mod_name)
        mod.__path__ = []
        for a in attrs:
            setattr(mod, a, type(a, (), {}))
        mods[mod_name] = mod
    mods["monai"].data, mods["monai"].transforms = mods["monai.data"], mods["monai.transforms"]
    mods["monai.data"].utils = mods["monai.data.utils"]
    sys.modules.update(mods)
    spec = importlib.util.spec_from_file_location("ref_cache_dataset", os.path.join(REF, "dataset", "cache_dataset.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.LabelSmoothingCacheDataset


def _blobs(g, shape, K, block, background=0.5):
    """A piecewise-constant class map: ids drawn per block of ``block`` voxels, about ``background`` of them 0."""
    coarse = torch.randint(0, K, tuple(-(-s // b) for s, b in zip(shape, block)), generator=g)
    keep = torch.rand(coarse.shape, generator=g) >= background
    coarse = coarse * keep
    for ax, b in enumerate(block):
        coarse = coarse.repeat_interleave(b, ax)
    return coarse[:shape[0], :shape[1], :shape[2]].to(torch.uint8).contiguous()


def centroid_gap(labels, K):
    """max |fp32 centroid as the reference computes it - exact centroid| over classes and axes."""
    idx = torch.stack(torch.meshgrid(*[torch.arange(s) for s in labels.shape], indexing="ij"), dim=-1)
    gap = 0.0
    for k in range(K):
        mask = labels == k
        if bool(mask.any()):
            ref32 = idx.float()[mask].mean(dim=0).double()
            exact = idx[mask].sum(dim=0).double() / float(mask.sum())
            gap = max(gap, float((ref32 - exact).abs().max()))
    return gap


def main():
    if not REF:
        raise SystemExit(__doc__)
    cls = _ref_dataset_class()
    g = torch.Generator().manual_seed(20261016)
    cases = {}
    # non-cubic extents (a swapped axis shows), K = 3, the reference's defaults
    cases["noncubic_k3"] = (_blobs(g, (12, 17, 23), 3, (4, 5, 6)), 3, 0.3, 1.0, 1e-6)
    # K = 14 with classes 5 and 13 absent: their centroid stays (0, 0, 0)
    lab = _blobs(g, (16, 20, 12), 14, (4, 4, 3), background=0.3)
    lab[lab == 5] = 4
    lab[lab == 13] = 0
    cases["absent_k14"] = (lab, 14, 0.3, 1.0, 1e-6)
    # a class of one voxel: distance 0 at that voxel, |1 - alpha / epsilon| = 3e5
    lab = _blobs(g, (10, 14, 18), 14, (5, 7, 6), background=0.4)
    lab[lab == 7] = 6
    lab[3, 9, 11] = 7
    cases["one_voxel_k14"] = (lab, 14, 0.3, 1.0, 1e-6)
    # order != 1, other alpha and epsilon
    cases["order2_k3"] = (_blobs(g, (9, 11, 13), 3, (3, 4, 5)), 3, 0.5, 2.0, 1e-3)
    cases["order_half_k3"] = (_blobs(g, (11, 9, 14), 3, (4, 3, 5)), 3, 0.2, 0.5, 1e-6)

    out = {"provenance": np.array("dataset/cache_dataset.py LabelSmoothingCacheDataset.label_smoothing of the reference "
                                  "checkout, CPU fp32"),
           "cases": np.array(sorted(cases))}
    for name, (labels, K, alpha, order, epsilon) in cases.items():
        ds = object.__new__(cls)
        ds.num_classes, ds.smoothing_alpha, ds.smoothing_order, ds.epsilon = K, alpha, order, epsilon
        with torch.no_grad():
            smoothed = cls.label_smoothing(ds, labels[None])
        assert smoothed.shape == (K,) + tuple(labels.shape) and smoothed.dtype == torch.float32, (smoothed.shape, smoothed.dtype)
        out[f"{name}_labels"] = labels.numpy()
        out[f"{name}_K"] = np.array(K, dtype=np.int32)
        out[f"{name}_alpha"], out[f"{name}_order"], out[f"{name}_epsilon"] = np.float64(alpha), np.float64(order), np.float64(epsilon)
        out[f"{name}_out"] = smoothed.numpy()
        out[f"{name}_centroid_gap"] = np.float64(centroid_gap(labels, K))
        counts = torch.bincount(labels.reshape(-1).long(), minlength=K).tolist()
        print(f"{name}: extents {tuple(labels.shape)}, K = {K}, counts {counts}: max {float(smoothed.max()):.6g}, "
              f"centroid gap {out[f'{name}_centroid_gap']:.3g}")
    os.makedirs(OUT, exist_ok=True)
    np.savez_compressed(os.path.join(OUT, "label_smoothing_golden.npz"), **out)


if __name__ == "__main__":
    main()
