"""The fused segmentation loss on the GPU (csrc/seg_loss.hip, the seg_loss_finish[_mn] tail, the multi_neighbor term through
it) against the fp64 references and derived bounds of tests/loss_fp64ref.py: the ``sums`` buffer, L, dcomb and EVERY gradient
element of every case, through _SegLoss (ops.seg_loss_reduce forward, ops.seg_loss_grad backward).  Each assertion is
``ratio <= 1`` of fp64ref.check with the CheckResult in the message; the figures are printed before they are asserted (run with
-s to see them)."""
import time

import numpy as np
import pytest
import torch

import loss_fp64ref as LR
from oracle.train_ref import RefLoss

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F16, F32, F64 = torch.float16, torch.float32, torch.float64
ALL4 = LR.LOSS_NAMES + ("multi_neighbor",)
SCALE = 2.0 ** 12                      # NativeConvTrainer's init_scale: what the backward of a training step is seeded with
T0 = time.time()


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _inputs(dtype, N, C, Cs, dims, label_kind, logit_kind, seed=3, offset_elems=0):
    g = _gen(seed)
    labels = LR.make_labels(label_kind, N, C, dims, g)
    x = LR.make_logits(logit_kind, N, C, dims, g, dtype, labels)
    return LR.channels_last(x, dtype, Cs, offset_elems, DEV), labels.to(DEV).contiguous()


def _seg_loss(logits, labels, names, combine, scale):
    """One forward and backward through _SegLoss: (L, sums, dcomb, the fp32 g the gradient kernel read, dlogits)."""
    from diff_unet_amos_amd.training import _SegLoss
    x = logits.detach().requires_grad_(True)
    L = _SegLoss.apply(x, labels, tuple(names), combine)
    _, _, sums, dcomb = L.grad_fn.saved_tensors
    (L * scale).backward()
    g = float(torch.tensor(scale, dtype=F32, device=DEV) * dcomb)
    return L.detach(), sums, dcomb, g, x.grad


def _check_case(logits, labels, names=LR.LOSS_NAMES, combine="sum", scale=SCALE, what="", r=None, mn=None):
    """sums against reduce_ref (when the names have sums), L / dcomb against finish_ref of the device sums, every gradient
    element against grad_ref of the device sums; padding channels of the gradient are zero.  Returns the pieces."""
    from diff_unet_amos_amd import ops
    N, C = labels.shape[:2]
    V = labels[0, 0].numel()
    L, sums, dcomb, g, grad = _seg_loss(logits, labels, names, combine, scale)
    res = {}
    if r is None:
        r = LR.reduce_ref(logits, labels)
    res["sums"] = LR.check(sums, LR.ref_sums(r), LR.reduce_bound(r))
    if "multi_neighbor" in names and mn is None:
        mn = ops.multi_neighbor_partials(logits, labels).cpu()          # integer sums, written not accumulated: deterministic
    wL, wdc = LR.finish_ref(sums, N, C, V, names, combine, mn if "multi_neighbor" in names else None)
    res["L"] = LR.check(L.cpu().reshape(1), wL.reshape(1), LR.finish_bound(wL).reshape(1))
    res["dcomb"] = LR.check(dcomb.cpu().reshape(1), wdc.reshape(1), LR.finish_bound(wdc).reshape(1))
    gr = LR.grad_ref(logits, labels, sums, g, [float(n in names) for n in LR.LOSS_NAMES])
    got, pad = LR.grad_rows(grad, C)
    res["grad"] = LR.check(got, gr["ref"], LR.grad_bound(gr, logits.dtype))
    res["pad"] = LR.check_padding(pad)
    print(f"[{time.time() - T0:6.1f}s] {what} {tuple(logits.shape)} {str(logits.dtype)[6:]} {'+'.join(names)}/{combine}: "
          + "; ".join(f"{k}: {v}" for k, v in res.items()))
    for k, v in res.items():
        assert v.ratio <= 1.0, (what, k, v)
    return dict(L=L, sums=sums, dcomb=dcomb, g=g, grad=got, ref=gr["ref"], r=r, wL=wL)


def _lost_shares(got, ref):
    """(share of sum |grad| the store loses, share of elements stored as exact zero whose reference is not)."""
    got, ref = got.double(), ref
    return float((got - ref).abs().sum() / ref.abs().sum()), float(((got == 0) & (ref != 0)).double().mean())


# ---- geometry ----------------------------------------------------------------------------------------------------------------------
GEOMETRY = [
    ("one past the first loop", F16, 1, 8, 8, (1, 3, 43691), "soft", "saturated"),
    ("the last volume without a loop", F32, 1, 3, 6, (32, 64, 64), "binary", "randn3"),
    ("V = 131073, fp32", F32, 2, 16, 16, (1, 3, 43691), "multi_hot", "randn3"),
    ("V = 131072, fp16", F16, 2, 16, 24, (32, 64, 64), "soft", "corners"),
    ("V = 255", F16, 1, 13, 16, (3, 5, 17), "soft", "saturated"),
    ("V = 255, fp32", F32, 2, 8, 8, (3, 5, 17), "binary", "randn3"),
    ("V = 1", F32, 3, 1, 1, (1, 1, 1), "binary", "zero"),
    ("V = 1, fp16", F16, 2, 16, 16, (1, 1, 1), "multi_hot", "randn3"),
    ("odd extents", F16, 3, 16, 24, (70, 45, 51), "multi_hot", "corners"),
    ("odd extents, fp32", F32, 3, 5, 5, (70, 45, 51), "soft", "saturated"),
    ("the gradient kernel's loop", F16, 1, 8, 8, (128, 128, 96), "soft", "randn3"),
    ("production shape, fp32", F32, 1, 16, 16, (96, 96, 96), "multi_hot", "randn3"),
]


@pytest.mark.parametrize("case", GEOMETRY, ids=[c[0] for c in GEOMETRY])
def test_geometry(case):
    what, *spec = case
    logits, labels = _inputs(*spec)
    _check_case(logits, labels, what=what)


@pytest.mark.parametrize("C", [1, 3, 8, 13, 16, 24, 64])
@pytest.mark.parametrize("dtype", [F16, F32], ids=["f16", "f32"])
def test_row_layouts(C, dtype):
    """Cs in {C, C + 3, the next multiple of 8, C + 8}: the vec8 path (fp16, C % 8 == 0, Cs % 8 == 0) and every way out of it."""
    dims = (10, 12, 14) if C == 64 else (20, 24, 28)
    for Cs in sorted({C, C + 3, -(-(C + 1) // 8) * 8, C + 8}):
        logits, labels = _inputs(dtype, 2, C, Cs, dims, "soft" if C % 2 else "binary", "randn3", seed=C)
        _check_case(logits, labels, what=f"C {C} Cs {Cs}")


def test_channel_groups_at_a_looping_volume():
    """C = 24 and 64 (c0 = 8 .. 56) with more than one stride per thread."""
    for C, dims in ((24, (40, 60, 64)), (64, (33, 64, 64))):
        logits, labels = _inputs(F16, 1, C, C, dims, "multi_hot", "randn3", seed=C)
        _check_case(logits, labels, what=f"groups C {C}")


def test_misaligned_contiguous_rows():
    """fp16, C % 8 == 0, rows contiguous, but the base 8 bytes into its buffer: the 16-byte loads are not allowed."""
    logits, labels = _inputs(F16, 2, 8, 8, (20, 24, 28), "binary", "randn3", offset_elems=4)
    assert logits.data_ptr() % 16 == 8 and logits.is_contiguous()
    _check_case(logits, labels, what="base + 8 bytes")


# ---- label and logit kinds -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F16, F32], ids=["f16", "f32"])
@pytest.mark.parametrize("logit_kind", ["randn3", "saturated", "zero", "corners"])
@pytest.mark.parametrize("label_kind", ["binary", "multi_hot", "soft"])
def test_label_and_logit_kinds(label_kind, logit_kind, dtype):
    logits, labels = _inputs(dtype, 2, 8, 8, (20, 24, 28), label_kind, logit_kind, seed=17)
    _check_case(logits, labels, what=f"{label_kind} labels, {logit_kind} logits")


@pytest.mark.parametrize("dtype", [F16, F32], ids=["f16", "f32"])
def test_smoothed_labels_from_the_batch_producer(dtype):
    """A real smoothed batch (the reference's defaults: values are unbounded near a centroid); kernel and reference read the
    same fp32 tensor."""
    from diff_unet_amos_amd import augment
    g = _gen(41)
    image = torch.rand(48, 52, 56, generator=g)
    label = torch.randint(0, 5, (12, 13, 14), generator=g).to(torch.uint8)
    label = label.repeat_interleave(4, 0).repeat_interleave(4, 1).repeat_interleave(4, 2).contiguous()
    vol = augment.DeviceVolume(image, label, device=DEV, num_classes=5)
    prod = augment.DeviceBatchProducer([vol], roi=(40, 40, 36), class_ids=range(5), seed=2, smoothing=augment.LabelSmoothing())
    _, labels = prod.next([0, 0])
    assert prod.status == 0 and labels.dtype == F32 and tuple(labels.shape) == (2, 5, 40, 40, 36)
    frac = float(((labels != 0) & (labels != 1)).float().mean())
    assert frac > 0.5, f"the batch is not smoothed: {frac:.2f} of the values are fractional"
    x = LR.make_logits("randn3", 2, 5, (40, 40, 36), g, dtype)
    _check_case(LR.channels_last(x, dtype, 8, 0, DEV), labels.contiguous(), what=f"smoothed batch (max label {float(labels.max()):.3g})")


# ---- every subset of names with every combine ------------------------------------------------------------------------------------------
def _mn_case(seed, N=2, C=4, dims=(2200, 8, 8)):
    """V = 140800 in few, deep columns (N C H W = 512 of depth 2200), logits randn rounded to fp16: a seed can be found whose
    columns are all further than 1e-5 from a depth tie."""
    from test_multi_neighbor import labels_from_classes
    g = _gen(seed)
    x = torch.randn(N, C, *dims, generator=g).half().float()
    classes = torch.randint(0, C, (N, *dims), generator=g)
    classes[torch.rand(N, *dims, generator=g) < 0.3] = -1
    return x, labels_from_classes(classes, C)


MN_SEED = 10     # chosen on the CPU: of seeds 0..10, seeds 1, 7 and 10 pass; 10 has the widest vote gap (7.0e-5)


def test_every_subset_of_names_with_every_combine():
    from diff_unet_amos_amd import ops
    from test_multi_neighbor import _min_vote_gap, multi_neighbor_restated
    x, labels = _mn_case(MN_SEED)
    gap = _min_vote_gap(x)
    assert gap > 1e-5, f"ill-posed comparison: a prediction column is {gap:.1e} from a depth tie"
    C = x.shape[1]
    logits, labels_d = LR.channels_last(x, F16, 8, 0, DEV), labels.to(DEV).contiguous()
    assert LR.reduce_geometry(labels[0, 0].numel())[1] == 2
    mn = ops.multi_neighbor_partials(logits, labels_d).cpu()
    term, want = float(mn[:, :C].sum() / mn[:, C].sum()), float(multi_neighbor_restated(x, labels, C))
    print(f"multi_neighbor: kernel {term:.9g}, restated {want:.9g}, vote gap {gap:.2e}")
    assert want > 0 and abs(term - want) <= 1e-5 * abs(want), (term, want)
    r = LR.reduce_ref(logits, labels_d)
    for names in LR.subsets():
        for combine in ("sum", "mean", "log"):
            _check_case(logits, labels_d, names, combine, what="subset", r=r)
            _check_case(logits, labels_d, names + ("multi_neighbor",), combine, what="subset + mn", r=r, mn=mn)
    # multi_neighbor alone: no sums, no gradient; the tail returns the term as it is
    L, _, dcomb = ops.seg_loss_reduce(logits, labels_d, ("multi_neighbor",), "log")
    wL, _ = LR.finish_ref(torch.zeros(2 * C * 4 + 2, dtype=F64), 2, C, labels[0, 0].numel(), ("multi_neighbor",), "log", mn)
    assert float(dcomb) == 1.0 and abs(float(L) - float(wL)) <= float(LR.finish_bound(wL)), (float(L), float(wL))


# ---- full size ---------------------------------------------------------------------------------------------------------------------------
def _full_size_inputs(seed, clamp=None):
    g = _gen(seed)
    labels = LR.make_labels("binary", 2, 16, (96, 96, 96), g)
    x = torch.randn(2, 16, 96, 96, 96, generator=g) * 3
    if clamp is not None:
        x = x.clamp(-clamp, clamp)
    return x.half().float(), labels


def test_full_size_four_names_against_an_independent_reference():
    """2 x 16 x 96^3 fp16 logits generated directly (no network): L of the four names against the fp64 three terms of the
    REFERENCE's sums (not the device's) plus the CPU restatement of multi_neighbor.  The non-circular counterpart of
    test_full_size_step_with_the_amos_set.  The bound: reduce_bound propagated through the tail (loss_fp64ref.loss_bound), and
    for the multi_neighbor term the 1e-5 relative that tests/test_multi_neighbor.py holds the kernel to.  Logits are clamped to
    |p| <= 8: fp16 neighbours there differ by 1.3e-6 in the sigmoid, 20 fp32 ulps, so a depth vote is an exact tie (first index
    wins on both sides) or clear."""
    from test_multi_neighbor import multi_neighbor_restated
    x, labels = _full_size_inputs(5, clamp=8.0)
    mn_cpu = float(multi_neighbor_restated(x, labels, 16))
    logits, labels_d = LR.channels_last(x, F16, 16, 0, DEV), labels.to(DEV).contiguous()
    for combine in ("sum", "log"):
        out = _check_case(logits, labels_d, ALL4, combine, what="full size, four names")
        wL, bL = LR.loss_bound(out["r"], LR.reduce_bound(out["r"]), ALL4, combine, mn_cpu, 1e-5 * abs(mn_cpu))
        L = float(out["L"])
        print(f"full size {combine}: L {L:.9g}, independent fp64 {float(wL):.9g}, |err| / bound {abs(L - float(wL)) / bL:.3g}, "
              f"multi_neighbor (CPU) {mn_cpu:.6g}")
        assert abs(L - float(wL)) <= bL, (combine, L, float(wL), bL)


def _report_shares(what, out, logits):
    lost, zeroed = _lost_shares(out["grad"], out["ref"])
    sub = float((out["ref"].abs() < 2.0 ** -14).double().mean())
    print(f"fp16 gradient at {tuple(logits.shape)}, g = 2^12 * dcomb, {what}: share of sum |grad| lost by the store "
          f"{lost:.3e}; elements stored as zero with a non-zero reference {zeroed:.3e}; elements in the subnormal range {sub:.3f}")
    return lost, zeroed


def test_fp16_gradient_at_production_scale_random_logits():
    """2 x 16 x 96^3, g = 2^12 dcomb: 1 / M = 3.5e-8, so most elements are fp16 subnormals.  Asserted: the per-element bound
    (it holds the subnormal floor 2^-25, so a store that flushes subnormals fails).  Reported, not asserted: how much of the
    gradient the fp16 store loses ("Loss kernels: fp64 check")."""
    x, labels = _full_size_inputs(9)
    logits, labels_d = LR.channels_last(x, F16, 16, 0, DEV), labels.to(DEV).contiguous()
    assert LR.reduce_geometry(96 ** 3)[1] == 7
    out = _check_case(logits, labels_d, what="production shape, randn * 3")
    _report_shares("randn * 3 logits", out, logits)
    assert float((out["grad"] != 0).double().mean()) > 0.5         # and the subnormals are there


def test_fp16_gradient_at_production_scale_network_logits():
    """The same on the head output of an initialised DiffUNet on a random image (what the first training steps see)."""
    from diff_unet_amos_amd.diff_unet import DiffUNet
    from diff_unet_amos_amd.training import NativeConvTrainer
    torch.manual_seed(0)
    net = DiffUNet(in_channels=1, out_channels=16).to(DEV)
    tr = NativeConvTrainer(net, lr=0.0, dtype=F16)
    seen = []
    tr.module.register_forward_hook(lambda mod, inp, out: seen.append(out.detach().clone()))
    g = torch.Generator(device=DEV).manual_seed(3)
    image = torch.rand(2, 1, 96, 96, 96, device=DEV, generator=g)
    labels = LR.make_labels("binary", 2, 16, (96, 96, 96), _gen(4)).to(DEV).contiguous()
    assert np.isfinite(float(tr.step(image, labels))) and len(seen) == 1
    logits = seen[0].contiguous()
    assert logits.dtype == F16 and tuple(logits.shape) == (2, 96, 96, 96, 16)
    del tr, net
    out = _check_case(logits, labels, what="production shape, network logits")
    print(f"network logits: mean {float(logits.float().mean()):.3f}, std {float(logits.float().std()):.3f}")
    _report_shares("DiffUNet head output at initialisation", out, logits)


# ---- non-finite input -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F16, F32], ids=["f16", "f32"])
@pytest.mark.parametrize("bad,label", [(float("nan"), 0.0), (float("nan"), 1.0), (float("inf"), 1.0), (float("inf"), 0.0),
                                       (float("-inf"), 0.0), (float("-inf"), 1.0)])
def test_non_finite_logit_agrees_in_kind_with_the_reference(bad, label, dtype):
    """One non-finite logit: L is finite or not exactly as RefLoss gives it in fp32 (a non-finite L is what makes the trainer's
    overflow check skip the step).  NaN must give a non-finite L."""
    from diff_unet_amos_amd import ops
    g = _gen(8)
    labels = LR.make_labels("binary", 1, 8, (6, 7, 8), g)
    x = LR.make_logits("randn3", 1, 8, (6, 7, 8), g, dtype)
    x[0, 3, 2, 4, 5], labels[0, 3, 2, 4, 5] = bad, label
    want = RefLoss("mse,bce,dice", "sum")(x, labels)
    L, _, _ = ops.seg_loss_reduce(LR.channels_last(x, dtype, 8, 0, DEV), labels.to(DEV).contiguous())
    print(f"logit {bad} under label {label}: L {float(L)}, RefLoss fp32 {float(want)}")
    assert bool(torch.isfinite(L)) == bool(torch.isfinite(want)), (float(L), float(want))
    if bad != bad:
        assert not bool(torch.isfinite(L))


# ---- determinism --------------------------------------------------------------------------------------------------------------------------------
def test_two_runs_agree():
    """The reduce kernel adds fp64 partials with atomics in any order: sums agree to 1e-13 relative, L is bit-equal in fp32; and
    ops.seg_loss_grad on the same sums is what _SegLoss's backward returned."""
    from diff_unet_amos_amd import ops
    logits, labels = _inputs(F16, 2, 16, 16, (64, 64, 48), "soft", "randn3", seed=21)
    L1, s1, d1 = ops.seg_loss_reduce(logits, labels)
    L2, s2, d2 = ops.seg_loss_reduce(logits, labels)
    spread = float(((s1 - s2).abs() / s1.abs().clamp_min(1e-300)).max())
    print(f"two runs of sums: largest relative difference {spread:.3e}")
    assert spread <= 1e-13 and torch.equal(L1, L2) and torch.equal(d1, d2)
    L, sums, dcomb, g, grad = _seg_loss(logits, labels, LR.LOSS_NAMES, "sum", SCALE)
    again = ops.seg_loss_grad(logits, labels, sums, torch.tensor(SCALE, device=DEV) * dcomb)
    assert torch.equal(again, grad)
