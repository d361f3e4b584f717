"""The boundary term of the fused loss on the GPU (ops.signed_distance_maps, ops.seg_loss_boundary_reduce / _grad through
_SegLoss, and NativeConvTrainer(boundary_weight=...)) against the fp64 references and derived bounds of
tests/boundary_fp64ref.py: B, L and EVERY gradient element; alpha = 0 gives the bits of the path without the term; padding
channels stay zero.  The figures are printed before they are asserted (run with -s)."""
import pytest
import torch

import boundary_fp64ref as BR
import loss_terms_fp64ref as LT
import sdf_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F16, F32 = torch.float16, torch.float32
SCALE = 2.0 ** 12
CONFIGS = [(shape, dtype, pad) for shape in BR.SHAPES for dtype in (F16, F32) for pad in (0, 5)]
_CASES = {}


def _case(shape, dtype, pad):
    """Operands on the device, the maps and the fp64 reduce of the boundary sum: computed once per configuration."""
    key = (shape, dtype, pad)
    if key not in _CASES:
        from diff_unet_amos_amd import ops
        logits, labels = BR.make_case(shape, dtype, shape[1] + pad)
        logits, labels = logits.to(DEV), labels.to(DEV).contiguous()
        phi = ops.signed_distance_maps(labels)
        assert torch.equal(phi.cpu(), torch.from_numpy(sdf_ref.contract(labels.cpu().numpy())[0]))
        _CASES[key] = dict(logits=logits, labels=labels, phi=phi, r=BR.reduce_ref(logits, labels, phi))
    return _CASES[key]


def _seg_loss(logits, labels, names, combine, boundary):
    from diff_unet_amos_amd.training import _SegLoss
    x = logits.detach().requires_grad_(True)
    L = _SegLoss.apply(x, labels, tuple(names), combine, boundary)
    saved = L.grad_fn.saved_tensors
    (L * SCALE).backward()
    return L.detach(), saved[2], saved[3], x.grad


def _check_results(config, c, names, combine, alpha, bterm, L, buf, dcomb, grad, mn):
    """B, L, dcomb and every gradient element of one _seg_loss call with the boundary term against the fp64 references."""
    shape, dtype, pad = config
    logits, labels, phi, r = c["logits"], c["labels"], c["phi"], c["r"]
    N, C = shape[:2]
    V = labels[0, 0].numel()
    wB, bB = BR.term_ref(r)
    three = BR.three_term(names)                           # the kernel family: the one these names take without the term
    assert buf.numel() == (N * C * 4 + 2 if three else N * C * 5 + 3)
    sums = buf if three else buf[:N * C * 4 + 3]
    wLn, wdc = BR.named_finish_ref(sums, N, C, V, names, combine, mn)
    wL, bL = BR.loss_ref(wLn, alpha, r)
    gs, gb = float(torch.tensor(SCALE, dtype=F32, device=DEV) * dcomb), float(torch.tensor(SCALE, dtype=F32, device=DEV) * alpha)
    gr = BR.grad_ref(logits, labels, buf, gs, names, phi, gb)
    got, padding = LT.grad_rows(grad, C)
    res = dict(B=abs(float(bterm) - float(wB)) / float(bB), L=abs(float(L) - float(wL)) / float(bL),
               dcomb=LT.check(dcomb.cpu().reshape(1), wdc.reshape(1), LT.finish_bound(wdc).reshape(1)).ratio,
               grad=BR.check(got, gr["ref"], BR.grad_bound(gr, dtype)).ratio, pad=LT.check_padding(padding).ratio)
    print(f"{shape} {str(dtype)[6:]} pad {pad} {'+'.join(names)}/{combine}: B {float(bterm):.9g} (fp64 {float(wB):.9g}), "
          f"L {float(L):.9g} (fp64 {float(wL):.9g}); |err| / bound: " + ", ".join(f"{k} {v:.3g}" for k, v in res.items()))
    for k, v in res.items():
        assert v <= 1.0, (names, combine, k, v)


@pytest.mark.parametrize("config", CONFIGS, ids=[f"{'x'.join(map(str, s))}-{str(d)[6:]}-pad{p}" for s, d, p in CONFIGS])
def test_value_and_gradient_within_the_bounds(config):
    from diff_unet_amos_amd import ops
    shape, dtype, pad = config
    c = _case(*config)
    logits, labels, phi, r = c["logits"], c["labels"], c["phi"], c["r"]
    N, C = shape[:2]
    V = labels[0, 0].numel()
    alpha = torch.tensor(BR.ALPHA, dtype=F32, device=DEV)
    zero = torch.zeros((), dtype=F32, device=DEV)
    for names in BR.NAME_SETS:
        mn = ops.multi_neighbor_partials(logits, labels).cpu() if "multi_neighbor" in names else None
        for combine in BR.COMBINES:
            bterm = torch.full((), float("nan"), dtype=F32, device=DEV)
            L, buf, dcomb, grad = _seg_loss(logits, labels, names, combine, (phi, alpha, bterm))
            _check_results(config, c, names, combine, alpha, bterm, L, buf, dcomb, grad, mn)
            # alpha = 0: the value and every gradient element of the path without the term
            L0, _, _, grad0 = _seg_loss(logits, labels, names, combine, (phi, zero))
            Ln, _, _, gradn = _seg_loss(logits, labels, names, combine, None)
            assert torch.equal(L0, Ln) and torch.equal(grad0, gradn), (names, combine)


def test_two_calls_give_identical_bits():
    c = _case(BR.SHAPES[1], F16, 0)
    alpha = torch.tensor(BR.ALPHA, dtype=F32, device=DEV)
    a = _seg_loss(c["logits"], c["labels"], ("dice",), "sum", (c["phi"], alpha))
    b = _seg_loss(c["logits"], c["labels"], ("dice",), "sum", (c["phi"], alpha))
    assert torch.equal(a[0], b[0]) and torch.equal(a[3], b[3])


def test_alpha_zero_leaves_the_loss_alone_whatever_b_is():
    """A map that holds an inf makes B non-finite; with alpha = 0 the tail must not form 0 * B: L and the gradient stay those of
    the path without the term."""
    c = _case(BR.SHAPES[0], F32, 0)
    phi = c["phi"].clone()
    phi.view(-1)[3] = float("inf")
    zero = torch.zeros((), dtype=F32, device=DEV)
    bterm = torch.zeros((), dtype=F32, device=DEV)
    for names in BR.NAME_SETS:
        L0, _, _, grad0 = _seg_loss(c["logits"], c["labels"], names, "sum", (phi, zero, bterm))
        Ln, _, _, gradn = _seg_loss(c["logits"], c["labels"], names, "sum", None)
        assert not bool(torch.isfinite(bterm)) and bool(torch.isfinite(L0))
        assert torch.equal(L0, Ln) and torch.equal(grad0, gradn), names


# ---- through the trainer ----------------------------------------------------------------------------------------------------------------------
def _trainer_inputs():
    g = torch.Generator().manual_seed(11)
    image = torch.rand(2, 1, 32, 32, 32, generator=g).to(DEV)
    labels = LT.make_labels("onehot_background", 2, 4, (32, 32, 32), g).to(DEV)
    noise = torch.randn(2, 4, 32, 32, 32, generator=g).to(DEV)
    return image, labels, noise, torch.tensor([700, 20], device=DEV)


def _trainer(graph, **kw):
    from diff_unet_amos_amd.diff_unet import DiffUNet
    from diff_unet_amos_amd.training import NativeConvTrainer
    torch.manual_seed(0)
    net = DiffUNet(in_channels=1, out_channels=4, features=(8, 8, 16, 32, 64, 8)).to(DEV)
    return NativeConvTrainer(net, lr=0.0, weight_decay=0.0, dtype=F16, graph=graph, losses="mse,bce,dice", **kw)


def test_a_trainer_step_eager_and_captured_and_a_weight_schedule():
    """lr = 0 keeps the weights, so every step sees the same logits: the captured step's loss and B have the bits of the eager
    step's; set_boundary_weight between replays moves the loss by (a2 - a1) B without a recapture, to within the rounding of the
    two fp32 losses and of the stored B; the maps the step used are the contract's."""
    image, labels, noise, t = _trainer_inputs()
    a1, a2 = 0.25, 1.5
    seen = {}
    for graph in (False, True):
        tr = _trainer(graph, boundary_weight=a1)
        L1 = tr.step(image, labels, noise=noise, t=t).clone()
        B1 = tr.boundary_term().clone()
        torch.cuda.synchronize()
        assert bool(torch.isfinite(L1)) and not tr.last_step_overflowed()
        assert all(bool(torch.isfinite(p.grad).all()) for p in tr.params if p.grad is not None)
        assert torch.equal(tr._bnd["phi"].cpu(), torch.from_numpy(sdf_ref.contract(labels.cpu().numpy())[0]))
        captured = tr._graph
        tr.set_boundary_weight(a2)
        L2 = tr.step(image, labels, noise=noise, t=t).clone()
        B2 = tr.boundary_term().clone()
        assert tr._graph is captured                                 # no recapture
        assert torch.equal(B1, B2)                                   # lr = 0: the same logits, the same B
        # L_i = fl32(L_named + a_i B) with the same fp32 L_named: two roundings of L, B's own rounding times the weights' gap
        u = 2.0 ** -24
        tol = u * (abs(float(L1)) + abs(float(L2))) + (a2 - a1) * u * abs(float(B1)) * 1.001 + 2.0 ** -149
        err = abs((float(L2) - float(L1)) - (a2 - a1) * float(B1))
        print(f"graph={graph}: L({a1}) {float(L1):.9g}, L({a2}) {float(L2):.9g}, B {float(B1):.9g}; |dL - da B| {err:.3g}, bound {tol:.3g}")
        assert abs(float(B1)) > 1e-3 and err <= tol, (err, tol)
        seen[graph] = (L1, B1, L2)
        with pytest.raises(ValueError):
            tr.set_boundary_weight(-1.0)
        del tr
    for e, g in zip(seen[False], seen[True]):
        assert torch.equal(e, g), (float(e), float(g))


def test_no_boundary_weight_changes_nothing_and_bad_weights_are_refused():
    image, labels, noise, t = _trainer_inputs()
    a = _trainer(False)
    b = _trainer(False, boundary_weight=None)
    assert b._bnd is None
    La, Lb = a.step(image, labels, noise=noise, t=t), b.step(image, labels, noise=noise, t=t)
    assert torch.equal(La, Lb)
    with pytest.raises(RuntimeError):
        b.boundary_term()
    for bad in (-0.5, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            _trainer(False, boundary_weight=bad)
