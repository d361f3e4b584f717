"""tests/loss_terms_fp64ref.py on the CPU: the restatements of ce / dice_ce / generalized_dice against torch, the fp32 emulation of
csrc/seg_loss_terms.hip inside the derived bounds on every case, every planted defect outside them on at least one, the names
the trainer accepts, and the new C entries' argument checks (no device needed)."""
import pytest
import torch

import loss_terms_fp64ref as LT

F16, F32, F64 = torch.float16, torch.float32, torch.float64
DIMS = (6, 5, 7)
SHAPES = [("C16 f16", F16, 2, 16, 16), ("C5 f16", F16, 2, 5, 8), ("C5 f32", F32, 2, 5, 8)]
CASES = [(s, lab, log) for s in SHAPES for lab in LT.LABEL_KINDS for log in LT.LOGIT_KINDS]
IDS = [f"{s[0]}-{lab}-{log}" for s, lab, log in CASES]
ALL6 = LT.TERM_NAMES
SCALE = 2.0 ** 12


def _case(shape, label_kind, logit_kind, seed=5):
    _, dtype, N, C, Cs = shape
    g = torch.Generator().manual_seed(seed)
    labels = LT.make_labels(label_kind, N, C, DIMS, g)
    x = LT.make_logits(logit_kind, N, C, DIMS, g, dtype)
    return LT.channels_last(x, dtype, Cs), labels


def _operands(shape, label_kind, logit_kind):
    logits, labels = _case(shape, label_kind, logit_kind)
    return LT.operands(logits, labels)


# ---- the restatements against torch -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_ce_is_cross_entropy_with_probability_targets(case):
    p, y = _operands(*case)
    p = p.contiguous().requires_grad_(True)
    want = torch.nn.functional.cross_entropy(p, y)
    got = LT.ce_restated(p, y)
    assert abs(float((got - want).detach())) <= 1e-12 * max(1.0, abs(float(want.detach()))), (got, want)
    (dwant,) = torch.autograd.grad(want, p)
    dgot = LT.ce_grad_restated(p.detach(), y)
    assert float((dgot - dwant).abs().max()) <= 1e-14


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_generalized_dice_is_the_monai_forward(case):
    logits, labels = _case(*case)
    p, y = LT.operands(logits, labels)
    N, C, V = p.shape
    p = p.contiguous().requires_grad_(True)
    want = LT.monai_generalized_dice(p.view(N, C, *DIMS), y.view(N, C, *DIMS))
    got = LT.gdice_restated(p, y)
    assert abs(float((got - want).detach())) <= 1e-12, (got, want)
    (dwant,) = torch.autograd.grad(want, p)
    sums = LT.ref_sums(LT.reduce_ref(logits, labels))
    L, _, k0, k1 = LT.finish_ref(sums, N, C, V, ("generalized_dice",), "sum")
    assert abs(float(L - want.detach())) <= 1e-12
    s = torch.sigmoid(p.detach())
    dgot = s * (1 - s) * (k0[..., None] * y + k1[..., None])
    assert float((dgot - dwant).abs().max()) <= 1e-12 * max(1.0, float(dwant.abs().max()))


def test_the_weights_of_absent_classes():
    Y = torch.tensor([[4.0, 0.0, 2.0], [0.0, 0.0, 0.0], [0.5, 1.0, 0.0]], dtype=F64)
    w = LT.gdice_weights(Y)
    assert w.tolist() == [[1 / 16, 1 / 4, 1 / 4], [0.0, 0.0, 0.0], [4.0, 1.0, 4.0]]


@pytest.mark.parametrize("case", CASES[::5], ids=IDS[::5])
def test_dice_ce_is_dice_plus_ce_and_one_term(case):
    logits, labels = _case(*case)
    p, y = LT.operands(logits, labels)
    N, C, V = p.shape
    sums = LT.ref_sums(LT.reduce_ref(logits, labels))
    dice, ce = LT.dice_restated(p, y), LT.ce_restated(p, y)
    alone = LT.finish_ref(sums, N, C, V, ("dice_ce",), "mean")
    assert abs(float(alone[0] - (dice + ce))) <= 1e-12 and float(alone[1]) == 1.0          # alone: returned as it is
    mse = ((torch.sigmoid(p) - y) ** 2).mean()
    two = LT.finish_ref(sums, N, C, V, ("mse", "dice_ce"), "mean")
    assert abs(float(two[0] - (mse + dice + ce) / 2)) <= 1e-12 and float(two[1]) == 0.5     # with mse: two terms, not three
    both = LT.finish_ref(sums, N, C, V, ("dice", "dice_ce"), "sum")
    assert abs(float(both[0] - (2 * dice + ce))) <= 1e-12                                   # the Dice part twice
    assert torch.equal(both[2], 2 * LT.finish_ref(sums, N, C, V, ("dice",), "sum")[2])


@pytest.mark.parametrize("combine", ["sum", "mean", "log"])
def test_the_whole_gradient_is_autograd_of_the_restated_loss(combine):
    """grad_ref (what the GPU test holds the kernel to) against autograd through loss_restated, for every subset of the new names
    with and without the old ones: the per-(n, c) constants, the multiplicities and the combine's derivative."""
    logits, labels = _case(SHAPES[1], "soft", "randn")
    p, y = LT.operands(logits, labels)
    N, C, V = p.shape
    sums = LT.ref_sums(LT.reduce_ref(logits, labels))
    for names in LT.subsets() + [ALL6, ("dice", "dice_ce"), ("bce", "ce", "generalized_dice")]:
        q = p.contiguous().requires_grad_(True)
        L = LT.loss_restated(q, y, names, combine)
        (want,) = torch.autograd.grad(L, q)
        wL, dc, _, _ = LT.finish_ref(sums, N, C, V, names, combine)
        assert abs(float(wL - L.detach())) <= 1e-12, (names, wL, L)
        got = LT.grad_ref(logits, labels, sums, float(dc), names)["ref"]
        assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max())), names


# ---- the emulation: inside the bound as it is, outside it with each planted defect ------------------------------------------------------------
def _emulate(case, names, combine, defect=None):
    """The three kernels' emulation against the references: ratios for sums, L, dcomb, consts, grad (|err| / bound, > 1 fails)."""
    logits, labels = _case(*case)
    N, C = labels.shape[:2]
    V = labels[0, 0].numel()
    r = LT.reduce_ref(logits, labels)
    sums = LT.emu_reduce(logits, labels, defect)
    res = dict(sums=LT.check(sums, LT.ref_sums(r), LT.reduce_bound(r)))
    if not bool(torch.isfinite(sums).all()):
        return res
    L, dc, consts = LT.emu_finish(sums, N, C, V, names, combine, None, defect)
    wL, wdc, k0, k1 = LT.finish_ref(sums, N, C, V, names, combine)
    res["L"] = LT.check(L.reshape(1), wL.reshape(1), LT.finish_bound(wL).reshape(1))
    res["dcomb"] = LT.check(dc.reshape(1), wdc.reshape(1), LT.finish_bound(wdc).reshape(1))
    if any(n in names for n in ("dice", "dice_ce", "generalized_dice")):
        k = torch.stack([k0, k1], -1)
        res["consts"] = LT.check(consts, k, LT.consts_bound(k))
    g = float(torch.tensor(SCALE, dtype=F32) * dc)
    grad = LT.emu_grad(logits, labels, consts, g, names, defect=defect)
    gr = LT.grad_ref(logits, labels, sums, g, names)
    got, pad = LT.grad_rows(grad, C)
    res["grad"] = LT.check(got, gr["ref"], LT.grad_bound(gr, logits.dtype))
    res["pad"] = LT.check_padding(pad)
    return res


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_emulation_stays_inside_the_bound(case):
    for names, combine in ((ALL6, "sum"), (LT.EXT_NAMES, "mean"), (("ce",), "sum"), (("generalized_dice", "dice_ce"), "log")):
        res = _emulate(case, names, combine)
        for k, v in res.items():
            assert v.ratio <= 1.0, (names, combine, k, v)


@pytest.mark.parametrize("shape", [("C24 f16", F16, 2, 24, 24), ("C29 f32", F32, 1, 29, 32), ("C37 f16", F16, 1, 37, 40)],
                         ids=["three groups", "four groups, the last partial", "eight groups, five live, the last partial"])
def test_the_emulation_stays_inside_the_bound_with_more_channel_groups(shape):
    """C = 24, 29, 37: the instantiations for 3, 4 and 8 channel groups; the running maximum moves across up to five groups."""
    for label_kind, logit_kind in (("soft", "randn"), ("class_absent", "saturated")):
        res = _emulate((shape, label_kind, logit_kind), ALL6, "sum")
        for k, v in res.items():
            assert v.ratio <= 1.0, (label_kind, logit_kind, k, v)


DEFECTS = {
    "lse_without_max": (("ce",), "sum"),
    "grad_softmax_minus_y": (("ce",), "sum"),
    "ce_divisor_ncv": (("ce",), "sum"),
    "inf_weights_zero": (("generalized_dice",), "sum"),
    "batch_max_weight": (("generalized_dice",), "sum"),
    "dice_ce_two_terms": (("mse", "dice_ce"), "mean"),
    "gdice_consts_fp32": (("generalized_dice",), "sum"),
}


@pytest.mark.parametrize("defect", sorted(DEFECTS))
def test_a_planted_defect_breaks_the_bound(defect):
    names, combine = DEFECTS[defect]
    broken = []
    for case, cid in zip(CASES, IDS):
        res = _emulate(case, names, combine, defect)
        bad = {k: v.ratio for k, v in res.items() if not v.ratio <= 1.0}
        if bad:
            broken.append((cid, bad))
    print(f"{defect}: breaks {len(broken)} of {len(CASES)} cases; first: {broken[:1]}")
    assert broken, defect


def test_the_defects_break_where_they_should():
    """The cases the issue's label kinds exist for: an absent class shows the weights left at 0, a sample without classes the
    batch-wide maximum, voxels whose labels do not sum to 1 the softmax - y gradient, +-200 the log-sum-exp without its maximum."""
    for defect, label, logit, key in (("inf_weights_zero", "class_absent", "randn", "L"),
                                      ("batch_max_weight", "empty_sample", "randn", "consts"),
                                      ("grad_softmax_minus_y", "onehot_background", "randn", "grad"),
                                      ("grad_softmax_minus_y", "soft", "randn", "grad"),
                                      ("lse_without_max", "soft", "saturated", "sums")):
        names, combine = DEFECTS[defect]
        res = _emulate((SHAPES[2], label, logit), names, combine, defect)
        assert not res[key].ratio <= 1.0, (defect, label, res[key])


# ---- the names the trainer accepts ------------------------------------------------------------------------------------------------------------
def test_parse_losses_accepts_the_new_names_and_refuses_the_rest():
    from diff_unet_amos_amd import ops
    from diff_unet_amos_amd.training import parse_losses
    assert ops.EXT_LOSS_NAMES == ("ce", "dice_ce", "generalized_dice")
    assert ops.ALL_LOSS_NAMES == ops.SEG_LOSS_NAMES + ops.EXT_LOSS_NAMES
    assert ops.LOSS_NAMES == ("mse", "bce", "dice") and ops.SEG_LOSS_NAMES == ("mse", "bce", "dice", "multi_neighbor")
    assert parse_losses("ce", "sum") == (("ce",), "sum")
    assert parse_losses("generalized_dice,mse,dice_ce,multi_neighbor,ce", "log")[0] == ("generalized_dice", "mse", "dice_ce",
                                                                                      "multi_neighbor", "ce")
    for name in ("focal", "dice_focal", "generalized_dice_focal", "boundary", "hausdorff_er", "generalized_wasserstein_dice"):
        with pytest.raises(NotImplementedError, match=rf"Loss \({name}\) is not listed yet"):
            parse_losses(f"ce,{name}")


# ---- the C entries check their arguments before touching a device ------------------------------------------------------------------------------
def test_the_new_entries_reject_bad_arguments_without_a_device():
    import ctypes as C
    import os
    import subprocess
    from diff_unet_amos_amd import _native as nv
    if not os.path.exists(nv.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(os.path.dirname(nv.LIB_PATH), "csrc"), "-j4"], check=True)
    lib = nv.lib()
    one = C.c_void_p(16)
    E = nv.ERR_ARG
    assert lib.dua_seg_loss_terms_scratch_bytes(2, 16, 96 ** 3) == 2 * 512 * 51 * 8
    assert lib.dua_seg_loss_terms_scratch_bytes(2, 5, 210) == 2 * 1 * 18 * 8
    assert lib.dua_seg_loss_terms_scratch_bytes(2, 65, 210) == E and lib.dua_seg_loss_terms_scratch_bytes(0, 5, 210) == E
    big = 1 << 30
    # reduce: C > 64, null pointers, stride < C, a dtype that is neither, scratch too small
    assert lib.dua_seg_loss_terms_reduce(nv.F16, 2, 65, 210, one, 72, one, one, one, big, None) == E
    assert lib.dua_seg_loss_terms_reduce(nv.F16, 2, 16, 210, None, 16, one, one, one, big, None) == E
    assert lib.dua_seg_loss_terms_reduce(nv.F16, 2, 16, 210, one, 16, None, one, one, big, None) == E
    assert lib.dua_seg_loss_terms_reduce(nv.F16, 2, 16, 210, one, 16, one, None, one, big, None) == E
    assert lib.dua_seg_loss_terms_reduce(nv.F16, 2, 16, 210, one, 16, one, one, None, big, None) == E
    assert lib.dua_seg_loss_terms_reduce(nv.F16, 2, 16, 210, one, 8, one, one, one, big, None) == E
    assert lib.dua_seg_loss_terms_reduce(7, 2, 16, 210, one, 16, one, one, one, big, None) == E
    assert lib.dua_seg_loss_terms_reduce(nv.F16, 2, 16, 210, one, 16, one, one, one, 2 * 51 * 8 - 1, None) == E
    # finish: no term selected, a bad combine, C > 64, null outputs, Dice-shaped names without a constants buffer, a flag of 2
    fin = lib.dua_seg_loss_terms_finish
    assert fin(2, 16, 210, 0, 0, 0, 0, 0, 0, 0, None, 0, one, one, one, one, None) == E
    assert fin(2, 16, 210, 0, 0, 0, 1, 0, 0, 0, None, 3, one, one, one, one, None) == E
    assert fin(2, 16, 210, 0, 0, 0, 1, 0, 0, 0, None, -1, one, one, one, one, None) == E
    assert fin(2, 65, 210, 0, 0, 0, 1, 0, 0, 0, None, 0, one, one, one, one, None) == E
    assert fin(2, 16, 210, 0, 0, 0, 1, 0, 0, 0, None, 0, None, one, one, one, None) == E
    assert fin(2, 16, 210, 0, 0, 0, 1, 0, 0, 0, None, 0, one, None, one, one, None) == E
    assert fin(2, 16, 210, 0, 0, 0, 1, 0, 0, 0, None, 0, one, one, None, one, None) == E
    assert fin(2, 16, 210, 0, 0, 0, 0, 1, 0, 0, None, 0, one, one, one, None, None) == E
    assert fin(2, 16, 210, 0, 0, 0, 0, 0, 1, 0, None, 0, one, one, one, None, None) == E
    assert fin(2, 16, 210, 0, 0, 0, 2, 0, 0, 0, None, 0, one, one, one, one, None) == E
    assert fin(2, 16, 210, 0, 0, 0, 1, 0, 0, 65, one, 0, one, one, one, one, None) == E
    # grad: the same, and a gradient stride below C
    grad = lib.dua_seg_loss_terms_grad
    assert grad(nv.F16, 2, 16, 210, one, 16, one, one, None, 0, 0, 0, 0, 0, 0, one, 16, None) == E
    assert grad(nv.F16, 2, 65, 210, one, 72, one, one, None, 0, 0, 0, 1, 0, 0, one, 72, None) == E
    assert grad(nv.F16, 2, 16, 210, None, 16, one, one, None, 0, 0, 0, 1, 0, 0, one, 16, None) == E
    assert grad(nv.F16, 2, 16, 210, one, 16, None, one, None, 0, 0, 0, 1, 0, 0, one, 16, None) == E
    assert grad(nv.F16, 2, 16, 210, one, 16, one, one, None, 0, 0, 0, 1, 0, 0, None, 16, None) == E
    assert grad(nv.F16, 2, 16, 210, one, 16, one, None, None, 0, 0, 0, 0, 0, 1, one, 16, None) == E
    assert grad(nv.F16, 2, 16, 210, one, 8, one, one, None, 0, 0, 0, 1, 0, 0, one, 16, None) == E
    assert grad(nv.F16, 2, 16, 210, one, 16, one, one, None, 0, 0, 0, 1, 0, 0, one, 8, None) == E
    assert grad(3, 2, 16, 210, one, 16, one, one, None, 0, 0, 0, 1, 0, 0, one, 16, None) == E
