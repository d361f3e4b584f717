"""ce / dice_ce / generalized_dice in the fused loss on the GPU (csrc/seg_loss_terms.hip through ops.seg_loss_reduce /
ops.seg_loss_grad and _SegLoss) against the fp64 references and derived bounds of tests/loss_terms_fp64ref.py: every sum, L, dcomb,
every per-(n, c) constant and EVERY gradient element of every case; padding channels stay zero.  Each assertion is ``ratio <= 1``
of fp64ref.check with the CheckResult in the message; the figures are printed before they are asserted (run with -s)."""
import time

import pytest
import torch

import loss_terms_fp64ref as LT

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F16, F32, F64 = torch.float16, torch.float32, torch.float64
ALL6 = LT.TERM_NAMES
SCALE = 2.0 ** 12                      # NativeConvTrainer's init_scale
SMALL = (6, 5, 7)
SHAPES = [("C16 f16 vector path", F16, 2, 16, 16, SMALL),
          ("C5 f16 scalar path", F16, 2, 5, 8, SMALL),
          ("C5 f32 scalar path", F32, 2, 5, 8, SMALL),
          ("C16 f16 64x64x48", F16, 1, 16, 16, (64, 64, 48))]
T0 = time.time()


def _inputs(shape, label_kind, logit_kind, seed=5):
    _, dtype, N, C, Cs, dims = shape
    g = torch.Generator().manual_seed(seed)
    labels = LT.make_labels(label_kind, N, C, dims, g)          # one sample: "empty_sample" leaves no class anywhere
    x = LT.make_logits(logit_kind, N, C, dims, g, dtype)
    return LT.channels_last(x, dtype, Cs, 0, DEV), labels.to(DEV).contiguous()


def _seg_loss(logits, labels, names, combine, scale):
    from diff_unet_amos_amd.training import _SegLoss
    x = logits.detach().requires_grad_(True)
    L = _SegLoss.apply(x, labels, tuple(names), combine)
    _, _, sums, dcomb = L.grad_fn.saved_tensors
    (L * scale).backward()
    g = float(torch.tensor(scale, dtype=F32, device=DEV) * dcomb)
    return L.detach(), sums, dcomb, g, x.grad


def _check_case(logits, labels, names=ALL6, combine="sum", scale=SCALE, what="", r=None, mn=None):
    """sums against reduce_ref, L / dcomb / constants against finish_ref of the device sums, every gradient element against
    grad_ref of the device sums, padding channels zero."""
    return _check_results(logits, labels, _seg_loss(logits, labels, names, combine, scale), names, combine, what, r, mn)


def _check_results(logits, labels, results, names=ALL6, combine="sum", what="", r=None, mn=None):
    """``_check_case`` on the results of a ``_seg_loss`` call made elsewhere."""
    from diff_unet_amos_amd import ops
    N, C = labels.shape[:2]
    V = labels[0, 0].numel()
    L, buf, dcomb, g, grad = results
    assert buf.numel() == N * C * 5 + 3                    # the seg_loss_terms path: sums, then the constants
    sums, consts = buf[:N * C * 4 + 3], ops._terms_consts(buf, N, C).view(N, C, 2)
    if r is None:
        r = LT.reduce_ref(logits, labels)
    res = dict(sums=LT.check(sums, LT.ref_sums(r), LT.reduce_bound(r)))
    if "multi_neighbor" in names and mn is None:
        mn = ops.multi_neighbor_partials(logits, labels).cpu()
    wL, wdc, k0, k1 = LT.finish_ref(sums, N, C, V, names, combine, mn)
    res["L"] = LT.check(L.cpu().reshape(1), wL.reshape(1), LT.finish_bound(wL).reshape(1))
    res["dcomb"] = LT.check(dcomb.cpu().reshape(1), wdc.reshape(1), LT.finish_bound(wdc).reshape(1))
    if any(n in names for n in ("dice", "dice_ce", "generalized_dice")):
        k = torch.stack([k0, k1], -1)
        res["consts"] = LT.check(consts.cpu(), k, LT.consts_bound(k))
    gr = LT.grad_ref(logits, labels, sums, g, names)
    got, pad = LT.grad_rows(grad, C)
    res["grad"] = LT.check(got, gr["ref"], LT.grad_bound(gr, logits.dtype))
    res["pad"] = LT.check_padding(pad)
    print(f"[{time.time() - T0:6.1f}s] {what} {tuple(logits.shape)} {str(logits.dtype)[6:]} {'+'.join(names)}/{combine}: "
          + "; ".join(f"{k}: {v}" for k, v in res.items()))
    for k, v in res.items():
        assert v.ratio <= 1.0, (what, k, v)
    return dict(L=L, sums=sums, dcomb=dcomb, grad=grad, r=r)


# ---- shapes x labels x logits ----------------------------------------------------------------------------------------------------------
CASES = [(s, lab, log) for s in SHAPES for lab in LT.LABEL_KINDS for log in LT.LOGIT_KINDS]


@pytest.mark.parametrize("case", CASES, ids=[f"{s[0]}-{lab}-{log}" for s, lab, log in CASES])
def test_all_six_terms(case):
    shape, label_kind, logit_kind = case
    logits, labels = _inputs(*case)
    if shape[5] != SMALL:
        assert LT.reduce_geometry(labels[0, 0].numel()) == (512, 2)        # the grid stride and the partial sum loop
    _check_case(logits, labels, what=f"{label_kind} labels, {logit_kind} logits")


MORE_GROUPS = [("C24 f16: three groups, vector path", F16, 2, 24, 24, SMALL),
               ("C29 f32: four groups, the last partial", F32, 1, 29, 32, SMALL),
               ("C32 f16: four groups, vector path", F16, 1, 32, 32, SMALL),
               ("C37 f16: eight groups, five live, the last partial", F16, 1, 37, 40, SMALL),
               ("C64 f16: eight groups, vector path", F16, 2, 64, 64, SMALL)]


@pytest.mark.parametrize("shape", MORE_GROUPS, ids=[s[0] for s in MORE_GROUPS])
def test_the_instantiations_for_more_channel_groups(shape):
    """C above 16: the reduce and gradient kernels instantiated for 3, 4 and 8 channel groups (C = 37 leaves three of the eight
    groups empty and the fifth partly filled)."""
    for label_kind, logit_kind in (("soft", "randn"), ("class_absent", "saturated")):
        logits, labels = _inputs(shape, label_kind, logit_kind)
        _check_case(logits, labels, what=f"{shape[0]}; {label_kind} labels, {logit_kind} logits")


def test_the_tail_with_multi_neighbor_alone_takes_no_sums():
    """dua_seg_loss_terms_finish with no use_* flag and the multi_neighbor partials: the header allows sums = NULL (and consts = NULL)
    for this call; it returns the term as it is."""
    from diff_unet_amos_amd import _native as nv
    from diff_unet_amos_amd import ops
    logits, labels = _inputs(SHAPES[0], "onehot_background", "randn")
    N, C = labels.shape[:2]
    mn = ops.multi_neighbor_partials(logits, labels)
    out = torch.full((2,), float("nan"), dtype=F32, device=DEV)
    nv.check(nv.lib().dua_seg_loss_terms_finish(N, C, labels[0, 0].numel(), 0, 0, 0, 0, 0, 0, C, nv.ptr(mn), 2, None, nv.ptr(out[0:]),
                                                nv.ptr(out[1:]), None, nv.stream_ptr()), "finish")
    m = mn.cpu()
    want = m[:, :-1].sum() / m[:, -1].sum()
    assert float(out[1]) == 1.0 and abs(float(out[0]) - float(want)) <= float(LT.finish_bound(want)), (out, want)


def test_every_subset_of_the_new_names_with_every_combine():
    logits, labels = _inputs(SHAPES[1], "soft", "randn")
    r = LT.reduce_ref(logits, labels)
    for names in LT.subsets():
        for combine in ("sum", "mean", "log"):
            _check_case(logits, labels, names, combine, what="subset", r=r)
    _check_case(logits, labels, ("dice", "dice_ce"), "mean", what="the Dice part twice", r=r)


def test_a_mix_with_mse_bce_and_multi_neighbor():
    logits, labels = _inputs(SHAPES[0], "onehot_background", "randn")
    for combine in ("sum", "mean", "log"):
        _check_case(logits, labels, ("mse", "bce", "multi_neighbor", "dice_ce", "generalized_dice"), combine, what="mix")
    _check_case(logits, labels, ("multi_neighbor", "ce"), "log", what="multi_neighbor + ce")


def test_an_unselected_term_cannot_reach_the_output():
    """The gradient kernel selects by branch, not by a weight of 0: NaN planted in the constants buffer of a ce-only call (whose
    tail never writes it, and whose gradient must not read it) does not reach the output -- 0 * NaN would."""
    from diff_unet_amos_amd import ops
    logits, labels = _inputs(SHAPES[1], "empty_sample", "randn")
    N, C = labels.shape[:2]
    L, buf, dcomb = ops.seg_loss_reduce(logits, labels, ("ce",), "sum")
    ops._terms_consts(buf, N, C).fill_(float("nan"))
    grad = ops.seg_loss_grad(logits, labels, buf, dcomb, ("ce",))
    assert bool(torch.isfinite(grad).all())
    gr = LT.grad_ref(logits, labels, buf[:N * C * 4 + 3], 1.0, ("ce",))
    got, pad = LT.grad_rows(grad, C)
    res = LT.check(got, gr["ref"], LT.grad_bound(gr, logits.dtype))
    assert res.ratio <= 1.0 and LT.check_padding(pad).ratio <= 1.0, res


# ---- determinism, and the old names on the old kernels -------------------------------------------------------------------------------------
def test_two_reduce_calls_give_identical_bits():
    from diff_unet_amos_amd import ops
    logits, labels = _inputs(SHAPES[3], "soft", "randn")
    L1, s1, d1 = ops.seg_loss_reduce(logits, labels, ALL6, "log")
    L2, s2, d2 = ops.seg_loss_reduce(logits, labels, ALL6, "log")
    assert s1.data_ptr() != s2.data_ptr()
    assert torch.equal(s1.view(torch.int64), s2.view(torch.int64)) and torch.equal(L1, L2) and torch.equal(d1, d2)
    g1 = ops.seg_loss_grad(logits, labels, s1, d1, ALL6)
    g2 = ops.seg_loss_grad(logits, labels, s2, d2, ALL6)
    assert torch.equal(g1, g2)


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[2]], ids=["f16", "f32"])
def test_the_old_names_take_the_old_entries(shape):
    """A name set within mse / bce / dice / multi_neighbor: ops.seg_loss_reduce / ops.seg_loss_grad give the bits of a direct
    call of dua_seg_loss_reduce / _finish[_mn] / _grad (one workgroup per sample here, so its fp64 atomics have one order)."""
    from diff_unet_amos_amd import _native as nv
    from diff_unet_amos_amd import ops
    logits, labels = _inputs(shape, "soft", "randn")
    N, C = labels.shape[:2]
    V = labels[0, 0].numel()
    for names, combine in ((("mse", "bce", "dice"), "sum"), (("dice", "mse"), "log"), (("bce", "multi_neighbor"), "mean")):
        L, sums, dcomb = ops.seg_loss_reduce(logits, labels, names, combine)
        grad = ops.seg_loss_grad(logits, labels, sums, dcomb * SCALE, names)
        assert sums.numel() == N * C * 4 + 2
        want = torch.zeros(N * C * 4 + 2, dtype=F64, device=DEV)
        nv.check(nv.lib().dua_seg_loss_reduce(nv.dt_code(logits.dtype), N, C, V, nv.ptr(logits), logits.shape[-1], nv.ptr(labels),
                                              nv.ptr(want), nv.stream_ptr()), "reduce")
        out = torch.empty(2, dtype=F32, device=DEV)
        use = [int(n in names) for n in ("mse", "bce", "dice")]
        ci = ("sum", "mean", "log").index(combine)
        if "multi_neighbor" in names:
            mn = ops.multi_neighbor_partials(logits, labels)
            nv.check(nv.lib().dua_seg_loss_finish_mn(N, C, V, *use, C, nv.ptr(mn), ci, nv.ptr(want), nv.ptr(out[0:]),
                                                     nv.ptr(out[1:]), nv.stream_ptr()), "finish_mn")
        else:
            nv.check(nv.lib().dua_seg_loss_finish(N, C, V, *use, ci, nv.ptr(want), nv.ptr(out[0:]), nv.ptr(out[1:]),
                                                  nv.stream_ptr()), "finish")
        gw = torch.zeros_like(logits)
        gs = (out[1] * SCALE).reshape(1).contiguous()
        nv.check(nv.lib().dua_seg_loss_grad(nv.dt_code(logits.dtype), N, C, V, nv.ptr(logits), logits.shape[-1], nv.ptr(labels),
                                            nv.ptr(want), nv.ptr(gs), *[float(u) for u in use], nv.ptr(gw), gw.shape[-1],
                                            nv.stream_ptr()), "grad")
        assert torch.equal(sums.view(torch.int64), want.view(torch.int64)), names
        assert torch.equal(L, out[0]) and torch.equal(dcomb, out[1]) and torch.equal(grad, gw), names


# ---- through the trainer ----------------------------------------------------------------------------------------------------------------------
def test_a_trainer_step_eager_and_captured():
    """NativeConvTrainer(losses="mse,dice_ce,generalized_dice") at the 32^3 minimum patch: the captured step's loss has the bits
    of the eager step's, the eager loss is within loss_bound of the fp64 restatement on the step's own logits (reduce_bound
    propagated through the terms: an independent reference, not the device's sums), and every gradient is finite."""
    from diff_unet_amos_amd.diff_unet import DiffUNet
    from diff_unet_amos_amd.training import NativeConvTrainer
    names = ("mse", "dice_ce", "generalized_dice")
    g = torch.Generator().manual_seed(11)
    image = torch.rand(2, 1, 32, 32, 32, generator=g).to(DEV)
    labels = LT.make_labels("onehot_background", 2, 4, (32, 32, 32), g).to(DEV)
    noise = torch.randn(2, 4, 32, 32, 32, generator=g).to(DEV)
    t = torch.tensor([700, 20], device=DEV)
    losses = []
    for graph in (False, True):
        torch.manual_seed(0)
        net = DiffUNet(in_channels=1, out_channels=4, features=(8, 8, 16, 32, 64, 8)).to(DEV)
        tr = NativeConvTrainer(net, lr=1e-3, dtype=F16, graph=graph, losses=",".join(names), loss_combine="sum")
        assert tr.loss_names == names
        seen = []
        if not graph:
            tr.module.register_forward_hook(lambda mod, inp, out: seen.append(out.detach().clone()))
        L = tr.step(image, labels, noise=noise, t=t).clone()
        torch.cuda.synchronize()
        assert bool(torch.isfinite(L)) and not tr.last_step_overflowed()
        grads = [p.grad for p in tr.params if p.grad is not None]
        assert grads and all(bool(torch.isfinite(x).all()) for x in grads)
        if not graph:
            logits = seen[0].contiguous()
            assert tuple(logits.shape[:4]) == (2, 32, 32, 32) and logits.shape[-1] >= 4 and logits.dtype == F16
            r = LT.reduce_ref(logits, labels)
            wL, bL = LT.loss_bound(r, LT.reduce_bound(r), names, "sum")
            print(f"trainer step: L {float(L):.9g}, fp64 restatement {float(wL):.9g}, |err| / bound "
                  f"{abs(float(L) - float(wL)) / bL:.3g}")
            p, y = LT.operands(logits, labels)
            assert abs(float(LT.loss_restated(p, y, names, "sum")) - float(wL)) <= 1e-9
            assert abs(float(L) - float(wL)) <= bL, (float(L), float(wL), bL)
        losses.append(L)
        del tr, net
    print(f"eager {float(losses[0]):.9g}, captured {float(losses[1]):.9g}")
    assert torch.equal(losses[0], losses[1]), (float(losses[0]), float(losses[1]))
