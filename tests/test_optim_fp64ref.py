"""tests/optim_fp64ref.py on the CPU: the references equal torch's own operators in float64 (clip_grad_norm_, torch.optim.AdamW,
update_ema of the reference), the fp32 emulation of every kernel stays inside every bound on the inputs the GPU test uses, and
each planted defect is rejected by them -- except the EMA updated on a skipped step, which no bound is asked about: a skipped step
is checked for bit equality (here on the emulation, in tests/test_optim_gpu.py on the device), and the defect breaks that."""
import math

import pytest
import torch

import glue_fp64ref as GR
import optim_fp64ref as OR

F64 = torch.float64
LR, EPS, WD, BETAS = 3e-3, 1e-8, 1e-2, (0.9, 0.999)


@pytest.fixture(scope="module")
def case():
    return OR.make_case()


def _norm_case(kind):
    flat, scale = OR.make_norm_grads(kind)
    tensors = OR.views(flat, OR.layout()[0])
    return tensors, scale, OR.partials_ref(tensors)


def _max_norms(kind):
    tensors, scale, (pref, _) = _norm_case(kind)
    return OR.max_norms(pref, scale)


# ---- the references against torch in float64 ------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", [0.99, 0.9999])
@pytest.mark.parametrize("clip", [0.5, 2.0])
def test_references_equal_torch_operators_in_float64(rate, clip):
    """Unscale, clip_grad_norm_, torch.optim.AdamW and update_ema (mul_(rate).add_(p, alpha=1 - rate)) on float64 tensors."""
    gen = torch.Generator().manual_seed(5)
    shapes = [(5,), (4097,), (33, 7)]
    ps = [torch.randn(*s, generator=gen, dtype=F64) for s in shapes]
    gs = [torch.randn(*s, generator=gen, dtype=F64) * 1024 for s in shapes]
    es = [p + 0.01 * torch.randn(*p.shape, generator=gen, dtype=F64) for p in ps]
    inv = 1.0 / 1024.0
    params = [torch.nn.Parameter(p.clone()) for p in ps]
    opt = torch.optim.AdamW(params, lr=LR, betas=BETAS, eps=EPS, weight_decay=WD)
    ms = [torch.zeros_like(p) for p in ps]
    vs = [torch.zeros_like(p) for p in ps]
    ema = [e.clone() for e in es]
    cur = [p.clone() for p in ps]
    for k in (1, 2, 3):
        unscaled = [g * inv * (1 + 0.1 * k) for g in gs]
        total = math.sqrt(sum(float((g ** 2).sum()) for g in unscaled))
        max_norm = clip * total
        for q, g in zip(params, unscaled):
            q.grad = g.clone()
        got_total = torch.nn.utils.clip_grad_norm_(params, max_norm)
        opt.step()
        with torch.no_grad():
            for e, q in zip(ema, params):
                e.mul_(rate).add_(q.detach(), alpha=1 - rate)
        nr = OR.norm_ref(OR.partials_ref(unscaled)[0], None, max_norm)
        assert abs(nr["norm"] - float(got_total)) <= 1e-12 * float(got_total)
        coef = min(1.0, max_norm / (nr["norm"] + 1e-6))              # float64 statement (norm_ref holds max_norm and 1e-6 as fp32)
        assert (coef < 1.0) == (clip < 1.0)
        for i in range(len(ps)):
            rp, rm, rv, rg, re = OR.step_ref(cur[i], gs[i] * (1 + 0.1 * k), ms[i], vs[i], es[i], k, LR, *BETAS, EPS, WD, inv, coef,
                                             1.0 - rate, fp32_abi=False)
            assert torch.allclose(rg, params[i].grad, rtol=1e-12, atol=0)
            assert torch.allclose(rp, params[i].detach(), rtol=1e-12, atol=1e-15)
            st = opt.state[params[i]]
            assert torch.allclose(rm, st["exp_avg"], rtol=1e-12, atol=1e-18) and torch.allclose(rv, st["exp_avg_sq"], rtol=1e-12, atol=0)
            assert torch.allclose(re, ema[i], rtol=1e-12, atol=1e-15)
            cur[i], ms[i], vs[i], es[i] = rp, rm, rv, re


def test_ema_weight_is_formed_in_double():
    assert OR.ema_w(0.9999) == GR.f32(1.0 - 0.9999)
    import numpy as np
    bad = float(np.float32(1.0) - np.float32(0.9999))
    assert abs(bad - OR.ema_w(0.9999)) / OR.ema_w(0.9999) > 1e-4          # what 1.f - rate loses: 1.66e-4 of w


# ---- norm and coefficient --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", OR.NORM_KINDS)
def test_norm_emulation_is_inside_every_bound(kind):
    tensors, scale, (pref, pbnd) = _norm_case(kind)
    part = OR.emu_partials(tensors)
    assert GR.check(part, pref, pbnd).ratio <= 1.0
    seen = set()
    for max_norm in _max_norms(kind):
        r = OR.norm_ref(pref, scale, max_norm)
        norm, coef, found = OR.emu_norm_finish(part, scale, max_norm)
        assert found == 0.0 and abs(norm - r["norm"]) <= r["e_norm"] and abs(coef - r["coef"]) <= r["e_coef"], (kind, max_norm, r)
        assert math.isfinite(norm) and math.isfinite(coef)
        seen.add(r["coef"] < 1.0)
    assert seen == ({True, False} if kind != "zero" else {False})
    if kind == "zero":
        assert r["norm"] == 0.0 and r["coef"] == 1.0


def test_partials_do_not_depend_on_where_a_chunk_starts():
    """The emulation (and the kernel) assign elements to lanes by index: a shifted copy of the same values gives the same bits."""
    flat, _ = OR.make_norm_grads("random")
    tensors = OR.views(flat, OR.layout()[0])
    shifted = [torch.cat([torch.zeros(1), t])[1:] for t in tensors]
    assert torch.equal(OR.emu_partials(tensors), OR.emu_partials(shifted))


@pytest.mark.parametrize("kind", ["random", "extreme_scaled"])
def test_rejects_the_norm_of_the_scaled_gradients(kind):
    tensors, scale, (pref, _) = _norm_case(kind)
    scale = 1024.0 if scale is None else scale
    r = OR.norm_ref(pref, scale, 1.0)
    norm, coef, _ = OR.emu_norm_finish(OR.emu_partials(tensors), scale, 1.0, defect="scaled_norm")
    assert abs(norm - r["norm"]) > r["e_norm"]
    good = OR.emu_norm_finish(OR.emu_partials(tensors), scale, 1.0)
    assert abs(good[0] - r["norm"]) <= r["e_norm"] and abs(good[1] - r["coef"]) <= r["e_coef"]


@pytest.mark.parametrize("kind", ["random", "extreme", "extreme_scaled"])
def test_rejects_an_unclamped_coefficient(kind):
    tensors, scale, (pref, _) = _norm_case(kind)
    part = OR.emu_partials(tensors)
    loose = [m for m in _max_norms(kind) if math.isfinite(m) and OR.norm_ref(pref, scale, m)["coef"] == 1.0]
    assert loose
    for max_norm in loose:
        r = OR.norm_ref(pref, scale, max_norm)
        _, coef, _ = OR.emu_norm_finish(part, scale, max_norm, defect="no_clamp")
        assert abs(coef - r["coef"]) > r["e_coef"]


def test_a_non_finite_gradient_raises_the_flag():
    flat, _ = OR.make_norm_grads("random")
    starts = OR.layout()[0]
    for bad in (math.inf, -math.inf, math.nan):
        f = flat.clone()
        f[starts[5] + 4096] = bad
        tensors = OR.views(f, starts)
        r = OR.norm_ref(OR.partials_ref(tensors)[0], None, 1.0)
        norm, coef, found = OR.emu_norm_finish(OR.emu_partials(tensors), None, 1.0)
        assert r["found"] == 1.0 and found == 1.0 and coef == 0.0 and r["coef"] == 0.0 and not math.isfinite(norm)


# ---- the step --------------------------------------------------------------------------------------------------------------------
STEP_CASES = [(k, rate, coef, scale) for k in (1, 10, 100001) for rate in (0.99, 0.9999) for coef in (0.37, 1.0)
              for scale in (None, 1024.0)]


def _check_step(case, k, rate, coef, scale, defect=None, found=0.0, e_coef=None):
    p, g, m, v, e = case["flat"]
    inv = 1.0 if scale is None else GR.f32(1.0 / scale)
    a = (k, GR.f32(LR), GR.f32(BETAS[0]), GR.f32(BETAS[1]), GR.f32(EPS), GR.f32(WD))
    c32 = GR.f32(coef)
    # the coefficient reaches the kernel from the finish kernel: the reference's own value, the device's within e_coef of it
    e_coef = 2 * GR.U32 * c32 if e_coef is None else e_coef
    got = OR.emu_step(p, g, m, v, e, *a, scale=scale, coef=c32, rate=rate, found=found, defect=defect)
    ref = OR.step_ref(p, g, m, v, e, *a, inv, coef, OR.ema_w(rate))
    bnd = OR.step_bound(p, g, m, v, e, *a, inv, coef, e_coef, OR.ema_w(rate))
    mask = case["mask"]
    return {n: GR.check(got[i][mask], ref[i][mask], bnd[i][mask]).ratio for i, n in enumerate("pmvge")}


@pytest.mark.parametrize("k,rate,coef,scale", STEP_CASES)
def test_step_emulation_is_inside_every_bound(case, k, rate, coef, scale):
    res = _check_step(case, k, rate, coef, scale)
    assert max(res.values()) <= 1.0, res


@pytest.mark.parametrize("k,rate,scale", [(k, r, s) for k in (1, 10, 100001) for r in (0.99, 0.9999) for s in (None, 1024.0)])
def test_rejects_the_coefficient_applied_to_the_update(case, k, rate, scale):
    res = _check_step(case, k, rate, 0.37, scale, defect="clip_update")
    assert res["m"] > 1.0 and res["v"] > 1.0 and res["g"] > 1.0, res


@pytest.mark.parametrize("defect", ["ema_pre", "rate_swapped", "w_fp32"])
@pytest.mark.parametrize("k,rate,coef,scale", STEP_CASES)
def test_rejects_ema_defects(case, k, rate, coef, scale, defect):
    res = _check_step(case, k, rate, coef, scale, defect=defect)
    assert res["e"] > 1.0, res
    assert max(res[n] for n in "pmvg") <= 1.0, res          # the defect is the EMA's alone


def test_rejects_an_ema_update_on_a_skipped_step(case):
    p, g, m, v, e = case["flat"]
    a = (10, LR, *BETAS, EPS, WD)
    good = OR.emu_step(p, g, m, v, e, *a, scale=1024.0, coef=0.5, rate=0.99, found=1.0)
    for x, y in zip(good, (p, m, v, g, e)):
        assert torch.equal(x, y)                            # a skipped step leaves p, m, v, g and e to the bit
    bad = OR.emu_step(p, g, m, v, e, *a, scale=1024.0, coef=0.5, rate=0.99, found=1.0, defect="ema_on_skip")
    assert not torch.equal(bad[4], e)
