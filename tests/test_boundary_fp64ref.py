"""The boundary term's references, bounds and emulation on the CPU (tests/boundary_fp64ref.py): the emulation of the kernels'
fp32 arithmetic stays within the derived bounds of the fp64 references on the shapes the GPU test uses, every planted defect
exceeds them there, and the new C entries refuse bad arguments without a device."""
import ctypes as C

import numpy as np
import pytest
import torch

import boundary_fp64ref as BR
import loss_terms_fp64ref as LT
import sdf_ref

F16, F32 = torch.float16, torch.float32
SCALE = 2.0 ** 12
COMBINE = "mean"                                                    # a combine whose dcomb is not 1
# (shape, dtype, padding channels, names): both kernel families (csrc/seg_loss.hip, csrc/seg_loss_terms.hip) on both shapes
CONFIGS = [(BR.SHAPES[0], F16, 0, ("mse", "bce", "dice")), (BR.SHAPES[0], F32, 5, ("mse", "bce", "dice")),
           (BR.SHAPES[1], F16, 5, ("mse", "bce", "dice")), (BR.SHAPES[0], F32, 5, ("dice_ce", "generalized_dice")),
           (BR.SHAPES[1], F16, 5, ("dice_ce", "generalized_dice"))]


@pytest.fixture(scope="module", params=CONFIGS,
                ids=[f"{'x'.join(map(str, s))}-{str(d)[6:]}-pad{p}-{'+'.join(n)}" for s, d, p, n in CONFIGS])
def case(request):
    """One emulated forward / backward: operands, the emulated 'device' values and the fp64 references with their bounds."""
    shape, dtype, pad, NAMES = request.param
    N, Cc = shape[:2]
    V = shape[2] * shape[3] * shape[4]
    logits, labels = BR.make_case(shape, dtype, Cc + pad)
    phi = torch.from_numpy(sdf_ref.contract(labels.numpy())[0])
    sums, L_named, dcomb, consts = BR.emu_named(logits, labels, NAMES, COMBINE)
    alpha = torch.tensor(BR.ALPHA, dtype=F32)
    gs, gb = float(np.float32(SCALE) * dcomb.numpy()), float(np.float32(SCALE) * alpha.numpy())
    r = BR.reduce_ref(logits, labels, phi)
    wB, bB = BR.term_ref(r)
    wLn = BR.named_finish_ref(sums, N, Cc, V, NAMES, COMBINE)[0]
    wL, bL = BR.loss_ref(wLn, alpha, r)
    gr = BR.grad_ref(logits, labels, sums, gs, NAMES, phi, gb)
    return dict(shape=shape, names=NAMES, N=N, C=Cc, V=V, logits=logits, labels=labels, phi=phi, sums=sums, L_named=L_named, dcomb=dcomb,
                consts=consts, alpha=alpha, gs=gs, gb=gb, wB=wB, bB=bB, wL=wL, bL=bL, gr=gr, gbound=BR.grad_bound(gr, dtype))


def _emulate(c, defect=None):
    bsum = BR.emu_reduce(c["logits"], c["phi"])
    B, L = BR.emu_finish(bsum, c["N"], c["C"], c["V"], c["L_named"], c["alpha"], defect)
    grad = BR.emu_grad(c["logits"], c["labels"], c["sums"], c["consts"], c["gs"], c["names"], c["phi"], c["gb"], defect=defect,
                       dcomb=float(c["dcomb"]), alpha=float(c["alpha"]))
    got, pad = LT.grad_rows(grad, c["C"])
    return dict(B=abs(float(B) - float(c["wB"])) / float(c["bB"]), L=abs(float(L) - float(c["wL"])) / float(c["bL"]),
                grad=BR.check(got, c["gr"]["ref"], c["gbound"]).ratio, pad=LT.check_padding(pad).ratio)


def test_the_emulation_is_within_the_bounds(case):
    res = _emulate(case)
    print(case["shape"], {k: f"{v:.3g}" for k, v in res.items()}, "B", float(case["wB"]), "L", float(case["wL"]))
    assert all(v <= 1.0 for v in res.values()), res
    assert res["grad"] > 0.01                       # the gradient's bound is within two orders of the emulation's actual error


@pytest.mark.parametrize("defect", BR.DEFECTS)
def test_every_planted_defect_exceeds_a_bound(case, defect):
    res = _emulate(case, defect)
    if defect == "padding_written" and case["logits"].shape[-1] == case["C"]:
        assert res == _emulate(case)                # no padding channels in this configuration: nothing to write into
        return
    print(case["shape"], defect, {k: f"{v:.3g}" for k, v in res.items()})
    assert max(res.values()) > 1.0, (defect, res)
    if defect in ("divisor_nv", "alpha_twice"):
        assert res["L"] > 1.0 and res["grad"] > 1.0, (defect, res)      # value and gradient both show these


def test_the_boundary_part_matters_in_the_cases():
    """B of the test cases is three orders above its bound: a kernel that dropped the term could not stay within it."""
    logits, labels = BR.make_case(BR.SHAPES[0], F16, 3)
    phi = torch.from_numpy(sdf_ref.contract(labels.numpy())[0])
    r = BR.reduce_ref(logits, labels, phi)
    B, bB = BR.term_ref(r)
    assert abs(float(B)) > 1e3 * float(bB)


def test_the_c_entries_refuse_bad_arguments_without_a_device():
    from diff_unet_amos_amd import _native as nv
    lib = nv.lib()
    one = C.c_void_p(16)
    big = 1 << 40
    assert lib.dua_seg_loss_boundary_scratch_bytes(2, 4, 46200) == 2 * 181 * 8
    assert lib.dua_seg_loss_boundary_scratch_bytes(2, 65, 100) == nv.ERR_ARG
    red = lambda **k: lib.dua_seg_loss_boundary_reduce(  # noqa: E731
        k.get("dtype", nv.F16), 2, k.get("C", 4), 315, k.get("logits", one), k.get("stride", 4), k.get("phi", one),
        k.get("alpha", one), k.get("loss", one), k.get("bterm", one), k.get("scratch", one), k.get("nbytes", big), None)
    for bad in (dict(logits=None), dict(phi=None), dict(alpha=None), dict(loss=None), dict(bterm=None), dict(scratch=None),
                dict(C=65, stride=65), dict(stride=3), dict(nbytes=2 * 2 * 8 - 1), dict(dtype=7)):
        assert red(**bad) == nv.ERR_ARG, bad
    grad = lambda **k: lib.dua_seg_loss_terms_boundary_grad(  # noqa: E731
        nv.F16, 2, k.get("C", 4), 315, k.get("logits", one), k.get("stride", 4), k.get("labels", one), k.get("consts", one), None,
        *k.get("use", (0, 0, 1, 0, 0, 0)), k.get("phi", one), k.get("bscale", one), k.get("out", one), k.get("ostride", 4), None)
    for bad in (dict(logits=None), dict(labels=None), dict(phi=None), dict(bscale=None), dict(out=None), dict(consts=None),
                dict(C=65, stride=65, ostride=65), dict(stride=3), dict(ostride=3), dict(use=(0, 0, 2, 0, 0, 0))):
        assert grad(**bad) == nv.ERR_ARG, bad
    grad3 = lambda **k: lib.dua_seg_loss_boundary_grad(  # noqa: E731
        k.get("dtype", nv.F16), 2, k.get("C", 4), 315, k.get("logits", one), k.get("stride", 4), k.get("labels", one),
        k.get("sums", one), None, 1.0, 1.0, 1.0, k.get("phi", one), k.get("bscale", one), k.get("out", one), k.get("ostride", 4),
        None)
    for bad in (dict(logits=None), dict(labels=None), dict(sums=None), dict(phi=None), dict(bscale=None), dict(out=None),
                dict(C=65, stride=65, ostride=65), dict(stride=3), dict(ostride=3), dict(dtype=7)):
        assert grad3(**bad) == nv.ERR_ARG, bad
