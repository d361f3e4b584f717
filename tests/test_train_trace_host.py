"""tests/train_trace.py without a device.  The wiring table against the oracle network's structure (oracle.unet_ref.RefDiffUNet, the
network test_training_harness.py differentiates on the host) at the default widths and at (8, 8, 16, 32, 64, 8): layer set, parameter
names and shapes, the channel counts of every concat, the nine timestep-embedding blocks in the order they run.  Then the verifier
on a trace synthesised from the table itself: it accepts the clean trace and names each planted defect -- as
test_batched_forms_defects.py does for the batched plans, this shows that the wiring check of test_train_step_fp64.py can fail."""
import pytest
import torch

import train_trace as TT
from oracle.unet_ref import RefDiffUNet

WIDTHS = [TT.DEFAULT_FEATURES, (8, 8, 16, 32, 64, 8)]
ALL_UP = ("upcat_4", "upcat_3", "upcat_2", "upcat_1")


def _every_block(t):
    return [b.name for b in t.blocks]


@pytest.mark.parametrize("features", WIDTHS, ids=["default", "small"])
def test_table_matches_the_oracle_network(features):
    classes = 16 if features[0] == 64 else 2
    ref = RefDiffUNet(in_channels=1, out_channels=classes, features=features).eval()
    table = TT.Table(features, 1, classes, fold=ALL_UP[2:], reduce=("conv_0", "upcat_1"))
    params = dict(ref.named_parameters())
    # parameter names: the table names every parameter of the network, ties every one of them to a gradient, and knows no other
    assert set(table.layer_params()) == set(params) == set(table.grads)
    # shapes: every gradient's launch output has the parameter's shape (a bias in front of an InstanceNorm has no launch)
    zeros = {n for n, w in table.grads.items() if w == "zeros"}
    assert zeros == {n for n in params if n.endswith(".conv.bias") and "final_conv" not in n and "deconv" not in n} and len(zeros) == 28
    for name, want in table.grads.items():
        if want != "zeros":
            shape = table.launches[want[0]].outs[want[1]]
            assert int(torch.tensor(shape).prod()) == params[name].numel(), (name, shape)
            if len(shape) == params[name].dim():
                assert tuple(shape) == tuple(params[name].shape), (name, shape)
    # layer set: 14 TwoConv blocks, 28 convolutions with the oracle's channel counts; the first layers' buffers are padded to 8
    assert len(table.blocks) == 14
    mods = dict(ref.named_modules())
    for b in table.blocks:
        two = mods[b.prefix]
        assert tuple(two.conv_0.conv.weight.shape[:2]) == (b.cout, b.cin) and tuple(two.conv_1.conv.weight.shape[:2]) == (b.cout, b.cout)
        assert b.cs == -(-b.cin // 8) * 8 and (b.temb is None) == (not hasattr(two, "temb_proj"))
    # every concat: [skip channels, upsampled channels] = [the encoder-side block's output, the transposed convolution's output]
    for b in table.up:
        cin_d, up, cat = table.deconv[b.name]
        dec = mods[f"model.{b.name}.upsample.deconv"]
        assert tuple(dec.weight.shape[:2]) == (cin_d, up) and cat + up == mods[b.prefix].conv_0.conv.weight.shape[1] == b.cs
        assert table.down[b.level].cout == cat
        x = {p.d_off: p for p in table.launches[f"{b.name}.conv_0/wgrad"].ins["x"]}
        assert (x[0].src, x[0].count) == (f"{table.down[b.level].name}.conv_1/mat", cat)
        assert (x[cat].src, x[cat].count) == (f"{b.name}/deconv", up)
    # the nine temb blocks in the order the oracle's forward runs them
    order = []
    for b in table.den:
        mods[f"{b.prefix}.temb_proj"].register_forward_hook(lambda m, i, o, name=b.name: order.append((name, o.shape[1])))
    g = torch.Generator().manual_seed(0)
    with torch.no_grad():
        ref(image=torch.rand(1, 1, 32, 32, 32, generator=g), x=torch.randn(1, classes, 32, 32, 32, generator=g), step=torch.tensor([5]),
            pred_type="denoise")
    assert order == [(b.name, b.cout) for b in table.den] and len(order) == 9
    assert [b.temb for b in table.den] == list(range(9)) and table.temb_rows(2, 2) == (2 * (features[0] + features[1]), 2 * sum(features[:3]))
    add = table.launches["temb/bwd"].ins["dadd"]
    assert [(p.src, p.d_off, p.count) for p in add] == [(f"{b.name}.conv_0/norm_bwd", table.temb_offs[i], b.cout) for i, b in enumerate(table.den)]


def _clean(reduce=("conv_0", "down_1", "upcat_1"), fold=("upcat_1",), N=2):
    table = TT.Table(fold=fold, reduce=reduce)
    trace, grads = TT.synthesize(table, N=N, seed=7)
    return table, {r.label: r for r in trace}, trace, grads


@pytest.mark.parametrize("reduce,fold", [((), ()), (("conv_0", "down_1", "upcat_1"), ("upcat_1",)),
                                         ([b for b in _every_block(TT.Table())], ALL_UP)], ids=["plain", "some", "all"])
def test_the_clean_trace_is_accepted(reduce, fold):
    table, by, trace, grads = _clean(reduce, fold)
    assert TT.verify(table, trace, grads) == []
    n = len(table.launches)
    print(f"{n} launches, {sum(len(e.ins) for e in table.launches.values())} operands, {len(table.aliases)} aliases, {len(table.grads)} gradients")
    # 28 layers x (conv, mat, norm_bwd, wgrad) + 26 data gradients + 8 max-pool backwards + 4 x (pack, deconv, deconv_bwd, 2 bias) + ...
    assert n == 28 * 4 + 26 + 8 + 4 * 5 + 2 + 2 + 1 + 2 + 2 + 2 + len(fold)


def _found(findings, *needles):
    return all(any(n in f for f in findings) for n in needles)


def test_swapped_dadd_row_slots_are_reported():
    table, by, trace, grads = _clean()
    d = by["temb/bwd"].ins["dadd"].t
    (a0, a1), (b0, b1) = table.temb_rows(0, 2), table.temb_rows(1, 2)
    assert a1 - a0 == b1 - b0                                       # equal widths: no shape can tell the two blocks apart
    keep = d[a0:a1].clone()
    d[a0:a1] = d[b0:b1]
    d[b0:b1] = keep
    f = TT.verify(table, trace, grads)
    assert len(f) == 2 and _found(f, "temb/bwd: operand dadd [0, 64)", "is not conv_0.conv_0/norm_bwd:dadd", "is not down_1.conv_0/norm_bwd:dadd"), f


def test_the_other_convolutions_sums_are_reported():
    table, by, trace, grads = _clean()
    by["conv_0.conv_0/norm_bwd"].ins["sums"] = by["conv_0.conv_1/norm_bwd"].outs["sums"]
    f = TT.verify(table, trace, grads)
    assert f == ["conv_0.conv_0/norm_bwd: operand sums is not conv_0.conv_1/dgrad:sums"], f
    # and a block that must run its own reduce pass, handed sums all the same
    by["down_2.conv_0/norm_bwd"].ins["sums"] = by["down_2.conv_1/norm_bwd"].outs["sums"]
    assert "down_2.conv_0/norm_bwd: operand sums is not in the table" in TT.verify(table, trace, grads)


@pytest.mark.parametrize("shift", [None, 8], ids=["exchanged", "shifted-by-8"])
def test_exchanged_or_shifted_concat_halves_are_reported(shift):
    table, by, trace, grads = _clean()
    cin_d, up, cat = table.deconv["upcat_1"]
    dx = by["upcat_1.conv_0/dgrad"].outs["dx"]
    dy, dA = by["upcat_1/deconv_bwd"].ins["dy"], by["conv_0.conv_1/pool_bwd"].ins["dA"]
    if shift is None:
        dy.t, dy.ptr = dx.t[..., :up].clone(), dx.ptr
        dA.t, dA.ptr = dx.t[..., cat:].clone(), dx.ptr + cat * 4
        want = ("upcat_1/deconv_bwd: operand dy [0, 64) <- [64, 128) is not upcat_1.conv_0/dgrad:dx", "upcat_1/deconv_bwd: dy is not in place",
                "conv_0.conv_1/pool_bwd: operand dA [0, 64) <- [0, 64) is not upcat_1.conv_0/dgrad:dx", "conv_0.conv_1/pool_bwd: dA is not in place")
    else:
        dy.t, dy.ptr = dx.t[..., cat - shift:cat - shift + up].clone(), dx.ptr + (cat - shift) * 4
        want = ("upcat_1/deconv_bwd: operand dy [0, 64) <- [64, 128) is not upcat_1.conv_0/dgrad:dx", "upcat_1/deconv_bwd: dy is not in place")
    f = TT.verify(table, trace, grads)
    assert len(f) == len(want) and _found(f, *want), f


def test_a_copy_of_the_concat_half_is_reported_as_not_in_place():
    table, by, trace, grads = _clean()
    by["down_2.conv_1/pool_bwd"].ins["dA"].ptr += 1 << 30                     # the right values at another address
    f = TT.verify(table, trace, grads)
    assert len(f) == 1 and f[0].startswith("down_2.conv_1/pool_bwd: dA is not in place"), f
    table, by, trace, grads = _clean()
    by["upcat_3/deconv"].outs["y"].ptr += 1 << 30                             # the transposed convolution into a buffer of its own
    f = TT.verify(table, trace, grads)
    assert len(f) == 1 and f[0].startswith("upcat_3/deconv: y is not in place"), f
    table, by, trace, grads = _clean()
    by["upcat_2.conv_0/conv"].ins["x"].ptr += 1 << 30                         # the skip copied into the concat
    f = TT.verify(table, trace, grads)
    assert len(f) == 1 and f[0].startswith("upcat_2.conv_0/conv: x is not in place"), f


def test_d_emb_without_the_pooled_path_is_reported():
    table, by, trace, grads = _clean()
    cat = table.deconv["upcat_3"][2]
    by["enc.down_2.conv_1/pool_bwd"].ins["dA"].t = by["upcat_3.conv_0/dgrad"].outs["dx"].t[..., :cat].clone()       # dA as down_2 received it
    f = TT.verify(table, trace, grads)
    assert f == ["enc.down_2.conv_1/pool_bwd: operand dA is not down_2.conv_1/pool_bwd:out"], f


def test_exchanged_sample_rows_of_the_temb_add_are_reported():
    table, by, trace, grads = _clean(N=2)
    add = by["down_3.conv_0/mat"].ins["add"]
    assert add.t.shape == (2, 256)
    add.t = add.t.flip(0).clone()
    f = TT.verify(table, trace, grads)
    assert len(f) == 1 and f[0].startswith("down_3.conv_0/mat: operand add [0, 256) <- [256, 512) is not temb/fwd:add"), f


def test_a_gradient_from_the_neighbouring_layer_is_reported():
    table, by, trace, grads = _clean()
    a, b = by["conv_0.conv_0/norm_bwd"].outs["dgamma"].t, by["conv_0.conv_1/norm_bwd"].outs["dgamma"].t
    assert a.shape == b.shape
    grads["model.conv_0.conv_1.adn.N.weight"] = a.clone()
    f = TT.verify(table, trace, grads)
    assert f == ["model.conv_0.conv_1.adn.N.weight: gradient is not conv_0.conv_1/norm_bwd:dgamma"], f


def test_a_scaled_or_absent_gradient_is_reported():
    table, by, trace, grads = _clean()
    grads["model.upcat_2.convs.temb_proj.weight"] = grads["model.upcat_2.convs.temb_proj.weight"] * 2
    grads["model.down_1.convs.conv_0.conv.bias"] = torch.full((3,), 1e-30)
    grads["embed_model.down.3.convs.conv_1.conv.weight"] = None
    f = TT.verify(table, trace, grads)
    assert sorted(f) == ["embed_model.down.3.convs.conv_1.conv.weight: no gradient",
                         "model.down_1.convs.conv_0.conv.bias: gradient is not exact zeros",
                         "model.upcat_2.convs.temb_proj.weight: gradient is not temb/bwd:pdw7"], f


def test_a_missing_launch_is_reported():
    table, by, trace, grads = _clean()
    trace = [r for r in trace if r.label != "down_2.conv_0/wgrad"]
    f = TT.verify(table, trace, grads)
    assert f == ["down_2.conv_0/wgrad: missing launch"], f
    # a launch the table does not know, a launch of the wrong kind (the fold where the shape does not allow it), one launched twice
    trace.append(TT.Rec("down_2.conv_0/pack_dgrad", "pack"))
    by["upcat_2.conv_0/conv"].kind = "fold"
    trace.append(by["head/bwd"])
    f = TT.verify(table, trace, grads)
    assert _found(f, "down_2.conv_0/pack_dgrad: launch not in the table", "upcat_2.conv_0/conv: kind fold, the table says conv",
                  "head/bwd: launched twice"), f
