"""Host side of mirror test-time augmentation (no GPU): the flip set, the predictor calls the list path makes, its values against
the fp64 restatement of the contract (tests/mirror_ref.py), the default path, the refusals and the binding's registry."""
import importlib.util
import os
import re

import pytest
import torch

from diff_unet_amos_amd import inference
from diff_unet_amos_amd.inference import _plan, infer, sliding_window_inference
from mirror_ref import flip_masks, fp32_bound, mirrored_blend_fp64
from streamed_blend_stub import CHANNELS, make_predictor, seeded_volume

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("dua_blend_accumulate_mirrored", "dua_blend_accumulate_weighted_mirrored")
# (volume shape, roi, overlap, sw_batch_size): a ragged plan (2 x 3 x 2 windows, clamped last starts), and a batch of two
# volumes (padded along D, 6 windows each: the second call spans both)
CASES = [
    ((1, 1, 11, 13, 18), (8, 8, 12), 0.5, 2),
    ((2, 1, 7, 9, 16), (8, 8, 8), 0.5, 4),
]
AXES = [(2,), (0, 1), (2, 0, 1)]


def test_mirror_flips():
    flips = inference.mirror_flips
    assert flips((2, 0)) == (0, 1, 4, 5) and flips([0, 2]) == (0, 1, 4, 5)
    assert flips(()) == (0,) and flips(None) == (0,)
    assert flips((1,)) == (0, 2) and flips((2, 1, 0)) == tuple(range(8))
    for axes in [(), (0,), (1, 2), (2, 0, 1)]:
        assert list(flips(axes)) == flip_masks(axes)
    for bad in [(3,), (-1,), (0, 0), (1, 2, 1), (1.0,), ("0",), (None,), (True,)]:
        with pytest.raises(ValueError):
            flips(bad)


def _counting(pred):
    calls = []

    def counted(x, **kw):
        calls.append(x.clone())
        return pred(x, **kw)

    return counted, calls


@pytest.mark.parametrize("mode", ["constant", "gaussian"])
def test_no_axes_is_the_call_without_the_argument(mode):
    shape, roi, overlap, swb = CASES[0]
    vol = seeded_volume(shape)
    pred, calls = _counting(make_predictor(roi, "cpu"))
    want = sliding_window_inference(vol, roi, swb, pred, overlap, mode=mode, pred_type="ddim_sample")
    n = len(calls)
    for axes in ((), None):
        del calls[:]
        got = sliding_window_inference(vol, roi, swb, pred, overlap, mirror_axes=axes, mode=mode, pred_type="ddim_sample")
        assert torch.equal(got, want) and len(calls) == n
    assert torch.equal(infer(pred, vol, roi, swb, overlap, mirror_axes=(), mode=mode), infer(pred, vol, roi, swb, overlap, mode=mode))


@pytest.mark.parametrize("axes", AXES)
def test_the_predictor_sees_every_flip_of_every_window_batch_in_mask_order(axes):
    shape, roi, overlap, swb = *CASES[0][:3], 5                    # 12 windows: calls of 5, 5 and 2
    vol = seeded_volume(shape)
    pred, plain = _counting(make_predictor(roi, "cpu"))
    sliding_window_inference(vol, roi, swb, pred, overlap, pred_type="ddim_sample")
    pred, calls = _counting(make_predictor(roi, "cpu"))
    sliding_window_inference(vol, roi, swb, pred, overlap, mirror_axes=axes, pred_type="ddim_sample")
    masks = flip_masks(axes)
    assert len(plain) > 1 and plain[-1].shape[0] < swb and len(calls) == len(masks) * len(plain)
    for g, windows in enumerate(plain):                            # the window batches are the unmirrored plan's
        for j, f in enumerate(masks):
            dims = [2 + a for a in range(3) if f >> a & 1]
            assert torch.equal(calls[g * len(masks) + j], torch.flip(windows, dims) if dims else windows), (g, f)


@pytest.mark.parametrize("mode", ["constant", "gaussian"])
@pytest.mark.parametrize("axes", AXES)
@pytest.mark.parametrize("shape,roi,overlap,swb", CASES)
def test_list_path_against_the_fp64_restatement(shape, roi, overlap, swb, axes, mode):
    """The bound is ``mirror_ref.fp32_bound``: from the n = F coverage fp32 additions a voxel receives and the magnitudes of
    its terms.  The stub's channel 1 reverses W and every channel adds a fixed field, so a missing or wrong un-flip, a weight
    on the flipped output or a divisor that is not F times the unmirrored one lands far outside it."""
    pred = make_predictor(roi, "cpu")
    vol = seeded_volume(shape)
    got = sliding_window_inference(vol, roi, swb, pred, overlap, mirror_axes=axes, mode=mode, pred_type="ddim_sample")
    q64, mag, n = mirrored_blend_fp64(vol, roi, overlap, pred, axes, mode)
    assert got.dtype == torch.float32 and got.shape == q64.shape == (shape[0], CHANNELS, *shape[2:])
    bound = fp32_bound(q64, mag, n, mode)
    err = (got.double() - q64).abs()
    print(f"{shape} roi {roi} axes {axes} {mode}: max |q - q64| {float(err.max()):.3e}, max err / bound "
          f"{float((err / bound).max()):.3f}, additions per voxel up to {int(n.max())}")
    assert int(n.max()) > len(flip_masks(axes)) and bool((err <= bound).all())
    plain = sliding_window_inference(vol, roi, swb, pred, overlap, mode=mode, pred_type="ddim_sample")
    assert float((got - plain).abs().max()) > 1e-2                 # the stub is not flip-equivariant: the average moved


@pytest.mark.parametrize("mode", ["constant", "gaussian"])
def test_an_equivariant_predictor_gives_the_unmirrored_blend(mode):
    """A pointwise function of the window commutes with every flip, so all F un-flipped outputs are the unmirrored output
    and the average is the unmirrored blend: the mirrored fp32 result lies within the same derived bound (n = F coverage
    additions) of the UNMIRRORED fp64 blend."""
    shape, roi, overlap, swb = CASES[0]
    axes = (0, 1, 2)

    def pointwise(x, pred_type=None):
        return torch.cat([x * 2.0 + 1.0, x * x - 0.5, -x], dim=1)

    vol = seeded_volume(shape)
    got = sliding_window_inference(vol, roi, swb, pointwise, overlap, mirror_axes=axes, mode=mode, pred_type="ddim_sample")
    q64, mag, n = mirrored_blend_fp64(vol, roi, overlap, pointwise, (), mode)
    bound = fp32_bound(q64, mag, 8 * n, mode)
    err = (got.double() - q64).abs()
    print(f"equivariant, {mode}: max |q - q64 unmirrored| {float(err.max()):.3e}, max err / bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())


def test_bad_axes_and_the_all_gather_form_are_refused_before_any_predictor_call():
    vol = torch.zeros(1, 1, 8, 8, 8)
    pred, calls = _counting(lambda x, **kw: x)
    with pytest.raises(ValueError, match="streaming=True"):
        infer(pred, vol, (8, 8, 8), distributed=True, streaming=False, mirror_axes=(0,))
    for bad in [(3,), (0, 0), (1.5,)]:
        with pytest.raises(ValueError, match="mirror_axes"):
            sliding_window_inference(vol, (8, 8, 8), 1, pred, mirror_axes=bad)
        with pytest.raises(ValueError, match="mirror_axes"):
            infer(pred, vol, (8, 8, 8), mirror_axes=bad)
        with pytest.raises(ValueError, match="mirror_axes"):
            inference.evaluate_volume(pred, vol, None, (8, 8, 8), mirror_axes=bad)
        with pytest.raises(ValueError, match="mirror_axes"):
            infer(pred, vol, (8, 8, 8), streaming=True, mirror_axes=bad)
    assert calls == []
    with pytest.raises(RuntimeError, match="runs on an MI355X"):   # good axes: the streamed form still has no CPU twin
        inference.streamed_sliding_window_inference(vol, (8, 8, 8), 1, pred, mirror_axes=(0,))
    assert calls == []


def _header_parameters(name):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dua_hip.h")).read(), flags=re.S)
    params = re.search(r"\bint " + name + r"\s*\(([^)]*)\)\s*;", src).group(1)
    return [" ".join(p.split()) for p in params.split(",")]


def test_the_new_symbols_are_registered_and_the_bindings_agree_with_the_header():
    import ctypes as C
    from diff_unet_amos_amd import _native as nv
    assert nv.ABI_VERSION == 8                                     # no struct, buffer layout or existing signature changed
    nv.lib()
    os.environ["DUA_HIP_SO"] = nv.LIB_PATH
    spec = importlib.util.spec_from_file_location("_dua_stub_mirror", os.path.join(ROOT, "include", "_dua.py"))
    stub = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(stub)
    for name in NEW_SYMBOLS:
        assert name in nv.exported_symbols()
        res, args = nv._SIGS[name]
        fn = getattr(stub._L, name)
        assert res is C.c_int and fn.restype is C.c_int and list(fn.argtypes) == list(args)
        params = _header_parameters(name)
        assert len(params) == len(args)
        for p, t in zip(params, args):                             # int -> c_int, float -> c_float, any pointer -> c_void_p
            want = C.c_void_p if "*" in p else C.c_float if p.startswith("float ") else C.c_int
            assert t is want, (name, p, t)
        assert params[11] == "int flip"
    # the mirrored forms take the unmirrored arguments plus the flip word, in the same order
    for name in NEW_SYMBOLS:
        plain = _header_parameters(name.replace("_mirrored", ""))
        assert [p for p in _header_parameters(name) if p != "int flip"] == plain
