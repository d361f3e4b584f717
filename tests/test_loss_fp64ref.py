"""The loss references and bounds of tests/loss_fp64ref.py, on the CPU: each reference equals the oracle's RefLoss in float64 (value
and autograd gradient, every subset of names under every combine; with multi_neighbor: the restated term plus the three); a
torch fp32 emulation of the kernels' own arithmetic order passes every bound; every planted defect is rejected (each test asserts
ratio > 1, so it fails if its mutation is removed)."""
import functools

import pytest
import torch

import loss_fp64ref as LR
from oracle.train_ref import RefLoss

F16, F32, F64 = torch.float16, torch.float32, torch.float64
COMBINES = ("sum", "mean", "log")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _rel(got, want):
    return float((got - want).abs().max()) / float(want.abs().max())


# ---- the references against the oracle ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["binary", "soft"])
@pytest.mark.parametrize("combine", COMBINES)
@pytest.mark.parametrize("names", LR.subsets(), ids=lambda n: "+".join(n))
def test_refs_equal_the_oracle(names, combine, kind):
    g = _gen(11)
    N, C, dims = 2, 3, (5, 6, 7)
    labels = LR.make_labels(kind, N, C, dims, g).double()
    x = (torch.randn(N, C, *dims, generator=g, dtype=F64) * 3).requires_grad_(True)
    want = RefLoss(",".join(names), combine)(x, labels)
    want.backward()
    want = want.detach()
    logits = x.detach().permute(0, 2, 3, 4, 1).contiguous()
    r = LR.reduce_ref(logits, labels)
    sums = LR.ref_sums(r)
    V = dims[0] * dims[1] * dims[2]
    L, dc = LR.finish_ref(sums, N, C, V, names, combine)
    assert abs(float(L) - float(want)) <= 1e-12 * abs(float(want)), (float(L), float(want))
    gr = LR.grad_ref(logits, labels, sums, float(dc), [float(n in names) for n in LR.LOSS_NAMES])
    assert _rel(gr["ref"], x.grad.reshape(N, C, V)) <= 1e-12


@pytest.mark.parametrize("combine", COMBINES)
def test_refs_with_multi_neighbor_equal_the_restatement_plus_the_three_terms(combine):
    """The restated term is an fp32 mean of fp32 squares; the partials' fp64 quotient differs from it by that mean's rounding,
    at most (entries) 2^-24 of the term."""
    from test_multi_neighbor import _random_case, multi_neighbor_restated
    x, labels = _random_case(5, 2, 6, 9, 10, 7)
    N, C, V = 2, 6, 9 * 10 * 7
    mn = LR.mn_partials_restated(x, labels, C)
    term = float(multi_neighbor_restated(x, labels, C))
    assert term > 0.01
    three = [float(RefLoss(n, "sum")(x.double(), labels.double())) for n in LR.LOSS_NAMES]
    total = sum(three) + term
    want = {"sum": total, "mean": total / 4, "log": float(torch.log1p(torch.tensor(total, dtype=F64)))}[combine]
    want_dc = {"sum": 1.0, "mean": 0.25, "log": 1 / (1 + total)}[combine]
    logits = x.double().permute(0, 2, 3, 4, 1).contiguous()
    sums = LR.ref_sums(LR.reduce_ref(logits, labels))
    L, dc = LR.finish_ref(sums, N, C, V, LR.LOSS_NAMES + ("multi_neighbor",), combine, mn)
    slack = 1e-12 * abs(want) + float(mn[:, 1].sum()) * LR.U32 * term
    assert abs(float(L) - want) <= slack and abs(float(dc) - want_dc) <= slack, (float(L), want, float(dc), want_dc)


def test_multi_neighbor_ref_equals_the_golden_cases():
    from test_multi_neighbor import _golden_cases
    for name, x, labels, K, want in _golden_cases():
        N, C = x.shape[:2]
        mn = LR.mn_partials_restated(x, labels, K)
        L, dc = LR.finish_ref(torch.zeros(N * C * 4 + 2, dtype=F64), N, C, x[0, 0].numel(), ("multi_neighbor",), "sum", mn)
        assert abs(float(L) - want) <= 1e-5 * abs(want) and float(dc) == 1.0, (name, float(L), want)


# ---- the emulation inside the bounds ------------------------------------------------------------------------------------------------
ALL4 = LR.LOSS_NAMES + ("multi_neighbor",)
MN = torch.tensor([[0.8, 0.3, 12.0], [0.1, 0.6, 12.0]], dtype=F64)        # made-up partials: the term is 0.075


@functools.lru_cache(maxsize=None)
def _case(dtype, N, C, Cs, dims, label_kind, logit_kind, seed=3):
    g = _gen(seed)
    labels = LR.make_labels(label_kind, N, C, dims, g)
    x = LR.make_logits(logit_kind, N, C, dims, g, dtype, labels)
    return LR.channels_last(x, dtype, Cs), labels


def _check_all(logits, labels, g_scale, names=LR.LOSS_NAMES, combine="sum", mn=None, reduce_defect=None, finish_defect=None,
               grad_defect=None, out_stride=None):
    """Emulated reduce, tail and gradient against the references; returns the CheckResults by name."""
    N, C = labels.shape[:2]
    V = labels[0, 0].numel()
    r = LR.reduce_ref(logits, labels)
    sums = LR.emu_reduce(logits, labels, reduce_defect)
    res = {"sums": LR.check(sums, LR.ref_sums(r), LR.reduce_bound(r))}
    clean = sums if reduce_defect is None else LR.emu_reduce(logits, labels)
    L, dc = LR.emu_finish(clean, N, C, V, names, combine, mn, finish_defect)
    wL, wdc = LR.finish_ref(clean, N, C, V, names, combine, mn)
    res["L"] = LR.check(L.reshape(1), wL.reshape(1), LR.finish_bound(wL).reshape(1))
    res["dcomb"] = LR.check(dc.reshape(1), wdc.reshape(1), LR.finish_bound(wdc).reshape(1))
    g = float(torch.tensor(g_scale, dtype=F32) * LR.emu_finish(clean, N, C, V, names, combine, mn)[1])
    w = [float(n in names) for n in LR.LOSS_NAMES]
    out = LR.emu_grad(logits, labels, clean, g, w, out_stride, grad_defect)
    gr = LR.grad_ref(logits, labels, clean, g, w)
    got, pad = LR.grad_rows(out, C)
    res["grad"] = LR.check(got, gr["ref"], LR.grad_bound(gr, logits.dtype))
    res["pad"] = LR.check_padding(pad)
    return res


EMU_CASES = [
    (F16, 1, 8, 8, (1, 3, 43691), "soft", "randn3"),            # V = 131073: the modelled chain is 2, with a ragged tail
    (F32, 1, 3, 6, (2, 256, 257), "binary", "saturated"),       # V = 131584, fp32, Cs > C
    (F16, 2, 16, 24, (6, 5, 7), "multi_hot", "corners"),
    (F16, 1, 13, 16, (3, 5, 17), "soft", "saturated"),          # V = 255
    (F32, 3, 1, 1, (1, 1, 1), "binary", "zero"),                # V = 1
    (F16, 1, 64, 64, (4, 4, 5), "binary", "randn3"),
    (F32, 2, 24, 27, (7, 4, 5), "soft", "corners"),
]


@pytest.mark.parametrize("case", EMU_CASES, ids=lambda c: f"{str(c[0])[-2:]}-N{c[1]}-C{c[2]}-Cs{c[3]}-{'x'.join(map(str, c[4]))}-{c[5]}-{c[6]}")
def test_emulation_is_inside_every_bound(case):
    logits, labels = _case(*case)
    assert case is not EMU_CASES[0] or LR.reduce_geometry(labels[0, 0].numel())[1] == 2
    for names, combine, mn in ((LR.LOSS_NAMES, "sum", None), (ALL4, "log", MN), (("bce", "dice"), "mean", None)):
        if case[1] != 2 and mn is not None:
            continue
        res = _check_all(logits, labels, 2.0 ** 12, names, combine, mn)
        for k in ("sums", "L", "dcomb", "grad", "pad"):
            assert res[k].ratio <= 1.0, (k, names, combine, res[k])


# ---- every planted defect is rejected -----------------------------------------------------------------------------------------------
BIG = (F16, 1, 16, 16, (1, 3, 43691), "soft", "corners")        # two channel groups, a ragged second stride, soft labels
SMALL = (F16, 2, 16, 24, (8, 9, 10), "soft", "corners")
SMALL_BINARY = (F16, 2, 16, 24, (8, 9, 10), "binary", "randn3")


def _rejected(case, key, g_scale=2.0 ** 12, **kw):
    logits, labels = _case(*case)
    base = _check_all(logits, labels, g_scale, **{k: v for k, v in kw.items() if not k.endswith("_defect")})
    bad = _check_all(logits, labels, g_scale, **kw)
    assert base[key].ratio <= 1.0, ("the unmutated emulation", base[key])
    return bad[key]


def test_rejects_a_dropped_last_stride():
    assert _rejected(BIG, "sums", reduce_defect="drop_tail").ratio > 1.0


def test_rejects_a_channel_group_reading_group_0s_labels():
    assert _rejected(BIG, "sums", reduce_defect="group_labels").ratio > 1.0


def test_rejects_a_sigmoid_one_fp16_ulp_off():
    assert _rejected(BIG, "sums", reduce_defect="sigmoid_ulp").ratio > 1.0
    assert _rejected(SMALL, "grad", grad_defect="sigmoid_ulp").ratio > 1.0


def test_rejects_m_without_the_factor_c():
    assert _rejected(SMALL, "L", finish_defect="m_without_c").ratio > 1.0


def test_rejects_a_missing_dice_epsilon():
    assert _rejected(SMALL, "L", finish_defect="no_eps").ratio > 1.0


def test_rejects_log_dcomb_without_the_multi_neighbor_term():
    assert _rejected(SMALL, "dcomb", names=ALL4, combine="log", mn=MN, finish_defect="log_without_mn").ratio > 1.0


def test_rejects_k1_with_the_wrong_sign():
    assert _rejected(SMALL, "grad", grad_defect="k1_sign").ratio > 1.0


def test_rejects_y_squared_on_soft_labels_only():
    assert _rejected(SMALL, "grad", grad_defect="y_squared").ratio > 1.0
    assert _rejected(SMALL_BINARY, "grad", grad_defect="y_squared").ratio <= 1.0     # invisible with binary labels


def test_rejects_nonzero_padding_channels():
    assert _rejected(SMALL, "pad", grad_defect="padding").ratio > 1.0


def test_rejects_an_fp16_store_that_flushes_subnormals():
    """g = 1 at M = 2 * 16 * 720: every element is below fp16's smallest normal, as at full size under the loss scale."""
    assert _rejected(SMALL, "grad", g_scale=1.0, grad_defect="flush_subnormals").ratio > 1.0
