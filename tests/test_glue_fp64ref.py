"""The training-glue references and bounds of tests/glue_fp64ref.py, on the CPU: each reference equals an independent float64
statement to 1e-12 relative (torch.optim.AdamW on float64 parameters, torch._amp_update_scale_, the oracle's q_sample on
2 y - 1, float64 autograd through the restated embedder); a torch fp32 emulation of each kernel's own operation order passes
every bound; every planted defect is rejected (each test asserts ratio > 1, or inequality for the exact quantities, so it fails
if its mutation is removed)."""
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import glue_fp64ref as GR
from oracle.diffusion_ref import RefDiffusion

F32, F64 = torch.float32, torch.float64
HYPER = dict(lr=3e-3, beta1=0.9, beta2=0.999, eps=1e-8, wd=1e-2)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _rel(got, want):
    return float((got - want).abs().max()) / max(float(want.abs().max()), 1e-300)


def _sched(T=1000):
    d = RefDiffusion(T)
    return d, torch.from_numpy(np.stack([d.sqrt_alphas_cumprod, d.sqrt_one_minus_alphas_cumprod], 1)).float().contiguous()


# ---- the references against independent float64 statements --------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 7])
@pytest.mark.parametrize("wd", [0.0, 1e-2])
def test_adamw_ref_equals_torch_adamw_in_float64(k, wd):
    """One step of torch.optim.AdamW on float64 tensors from the same state, the same double betas passed to both."""
    p, g, m, v = (x.double() for x in GR.make_adam_inputs(500, 3))
    if k == 1:
        m, v = torch.zeros_like(m), torch.zeros_like(v)
    q = torch.nn.Parameter(p.clone())
    opt = torch.optim.AdamW([q], lr=3e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd, foreach=False)
    if k > 1:
        opt.state[q] = dict(step=torch.tensor(float(k - 1)), exp_avg=m.clone(), exp_avg_sq=v.clone())
    q.grad = g / 1024.0
    opt.step()
    gp, gm, gv, gu = GR.adamw_ref(p, g, m, v, k, 3e-3, 0.9, 0.999, 1e-8, wd, 1.0 / 1024.0, fp32_abi=False)
    assert torch.equal(gu, g / 1024.0)
    assert _rel(gp, q.detach()) <= 1e-12
    assert _rel(gm, opt.state[q]["exp_avg"]) <= 1e-12 and _rel(gv, opt.state[q]["exp_avg_sq"]) <= 1e-12


SEQUENCE = [0, 0, 1, 0, 0, 0, 1, 1, 0, 0, 0, 0]        # found_inf per step: growths at interval 2, single and double overflows


def test_advance_ref_equals_amp_update_scale():
    scale, growth = torch.full((1,), 8.0), torch.zeros(1, dtype=torch.int32)
    st = (0, 0.0, 8.0, 0)
    grew = shrank = False
    for bad in SEQUENCE:
        before = st[2]
        torch._amp_update_scale_(scale, growth, torch.full((1,), float(bad)), 2.0, 0.5, 2)
        step, found, s, gr, seen = GR.advance_ref(st[0], float(bad), st[2], st[3], 2.0, 0.5, 2)
        assert (s, gr) == (float(scale), int(growth)) and found == 0.0 and seen == float(bad)
        assert step == st[0] + (0 if bad else 1)
        grew, shrank = grew or s > before, shrank or s < before
        st = (step, found, s, gr)
    assert grew and shrank


def test_advance_ref_keeps_a_scale_that_would_overflow_and_takes_null_forms():
    big = GR.f32(2.0 ** 127)
    assert GR.advance_ref(3, 0.0, big, 1, 2.0, 0.5, 2) == (4, 0.0, big, 0, 0.0)
    assert GR.advance_ref(3, 1.0, None, None, 2.0, 0.5, 2) == (3, 0.0, None, None, 1.0)
    assert GR.advance_ref(3, 0.0, None, 1, 2.0, 0.5, 2) == (4, 0.0, None, 0, 0.0)
    assert GR.advance_ref(3, 0.0, 4.0, None, 2.0, 0.5, 2) == (4, 0.0, 4.0, None, 0.0)


def test_q_sample_affine_ref_equals_the_oracle():
    d, sched = _sched()
    g = _gen(5)
    y = (torch.rand(3, 2, 4, 5, 6, generator=g) > 0.6).double()
    noise = torch.randn(y.shape, generator=g, dtype=F64)
    t = torch.tensor([0, 999, 417])
    want = d.q_sample(2 * y - 1, t, noise)
    ref, _ = GR.q_sample_affine_ref(y, 2.0, -1.0, noise, sched, t)
    assert _rel(ref, want.reshape(3, -1)) <= 1e-12
    # the clamp is the kernel's contract
    lo, _ = GR.q_sample_affine_ref(y, 2.0, -1.0, noise, sched, torch.tensor([-5, 1007, 0]))
    assert torch.equal(lo, GR.q_sample_affine_ref(y, 2.0, -1.0, noise, sched, torch.tensor([0, 999, 0]))[0])


def _temb_double(t, freqs, params):
    """tests/test_train_glue_gpu.py's _temb_reference in double: models/diffusion/utils.py:5-54 + denoiser.py:51-52,65; the
    fp32 product t * freq is the embedder's operand."""
    w0, b0, w1, b1 = params[:4]
    arg = (t.float()[:, None] * freqs[None, :]).double()
    e = torch.cat([torch.sin(arg), torch.cos(arg)], dim=1)
    h = F.linear(e, w0, b0)
    h = h * torch.sigmoid(h)
    temb = F.linear(h, w1, b1)
    s = temb * torch.sigmoid(temb)
    return [F.linear(s, params[4 + 2 * i], params[5 + 2 * i]) for i in range((len(params) - 4) // 2)]


def test_temb_refs_equal_float64_autograd():
    """add and all 4 + 2 B parameter gradients."""
    half, hid, couts, N = 5, 256, [3, 70, 1, 64], 3
    w0, b0, w1, b1, ws, bs = GR.make_temb_params(hid, half, couts, 2)
    params = [w0, b0, w1, b1] + [x for pair in zip(ws, bs) for x in pair]
    params = [p.double().requires_grad_() for p in params]
    t, freqs = GR.make_timesteps(N), GR.temb_freqs(half)
    want = _temb_double(t, freqs, params)
    gens = [torch.randn(N, c, generator=_gen(9 + i), dtype=F64) for i, c in enumerate(couts)]
    gw = torch.autograd.grad(want, params, gens)
    dp = [p.detach() for p in params]
    fwd = GR.temb_fwd_ref(t, freqs, dp[0], dp[1], dp[2], dp[3], dp[4::2], dp[5::2])
    assert _rel(fwd["add"][0], GR.block_major(want).detach()) <= 1e-12
    saved = torch.cat([fwd[k][0] for k in ("e", "z1", "h1", "z2", "s")], 1)
    bwd = GR.temb_bwd_ref(GR.block_major(gens), dp[2], dp[4::2], saved, half)
    got = [bwd["dw0"][0], bwd["db0"][0], bwd["dw1"][0], bwd["db1"][0]]
    for i in range(len(couts)):
        got += [bwd["dw"][i][0], bwd["db"][i][0]]
    for i, (a, b) in enumerate(zip(got, gw)):
        assert _rel(a, b) <= 1e-12, i


def test_stats_channel_sums_ref_decodes_and_sums_the_words():
    st = torch.zeros(2, 8, 4, 64, dtype=torch.int64)
    st[0, 0, 0, 5], st[0, 3, 1, 5], st[1, 7, 0, 5], st[1, 2, 1, 5] = 7, 2 ** 43, -2, 2 ** 42      # 7.5 and -1.75
    st[1, 1, 2, 5] = 99                                                                            # a sum of squares: not read
    ref, bnd = GR.stats_channel_sums_ref(st, 8)
    assert float(ref[5]) == 5.75 and float(ref.abs().sum()) == 5.75 and float(bnd[5]) < 1e-6


# ---- the emulations inside the bounds ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per", [4, 1028, 1029, 4100, 37])
def test_q_sample_emulation_is_inside_the_bound(per):
    _, sched = _sched()
    g = _gen(per)
    src, eps = (torch.rand(3, per, generator=g) > 0.7).float(), torch.randn(3, per, generator=g)
    for t in ([0, 999, 417], [-5, 1007, 0]):
        t = torch.tensor(t)
        ref, bnd = GR.q_sample_affine_ref(src, 2.0, -1.0, eps, sched, t)
        res = GR.check(GR.emu_q_sample_affine(src, 2.0, -1.0, eps, sched, t), ref, bnd)
        assert res.ratio <= 1.0, res


def test_q_sample_emulation_with_general_operands_is_inside_the_bound():
    _, sched = _sched()
    g = _gen(1)
    src, eps = torch.randn(2, 4096, generator=g) * 3, torch.randn(2, 4096, generator=g)
    t = torch.tensor([500, 17])
    ref, bnd = GR.q_sample_affine_ref(src, 0.37, 1.9, eps, sched, t)
    res = GR.check(GR.emu_q_sample_affine(src, GR.f32(0.37), GR.f32(1.9), eps, sched, t), ref, bnd)
    assert res.ratio <= 1.0, res


TEMB_CASES = [(256, 64, (3, 70, 1, 64, 7), 3), (512, 3, (7, 58, 64), 1), (256, 100, (1,) * 16, 5), (256, 64, (64, 130), 64)]


@functools.lru_cache(maxsize=None)
def _temb_emulated(hid, half, couts, N, fwd_defect=None, bwd_defect=None):
    w0, b0, w1, b1, ws, bs = GR.make_temb_params(hid, half, list(couts), 4)
    t, freqs = GR.make_timesteps(N), GR.temb_freqs(half)
    add, saved = GR.emu_temb_fwd(t, freqs, w0, b0, w1, b1, ws, bs, fwd_defect)
    fwd = GR.temb_fwd_checks(add, saved, GR.temb_fwd_ref(t, freqs, w0, b0, w1, b1, ws, bs, saved), half, hid)
    clean = saved if fwd_defect is None else GR.emu_temb_fwd(t, freqs, w0, b0, w1, b1, ws, bs)[1]
    dadd = GR.block_major([torch.randn(N, c, generator=_gen(20 + i)) for i, c in enumerate(couts)])
    got = GR.emu_temb_bwd(dadd, w1, ws, clean, half, bwd_defect)
    bwd = GR.temb_bwd_checks(got, GR.temb_bwd_ref(dadd, w1, ws, clean, half, dz2=got["dz2"]))
    return fwd, bwd


@pytest.mark.parametrize("case", TEMB_CASES, ids=lambda c: f"hid{c[0]}-half{c[1]}-P{sum(c[2])}-N{c[3]}")
def test_temb_emulation_is_inside_every_bound(case):
    fwd, bwd = _temb_emulated(*case)
    for k, v in {**fwd, **bwd}.items():
        assert v.ratio <= 1.0, (k, v)


ADAM_SWEEP = [(k, b, wd, sc) for k in (1, 2, 10, 1000, 100001) for b in ((0.9, 0.999), (0.5, 0.9)) for wd in (0.0, 1e-2)
              for sc in (None, 1024.0)]


def _adam_check(n, k, betas, wd, scale, lr=3e-3, eps=1e-8, defect=None, seed=6):
    p, g, m, v = GR.make_adam_inputs(n, seed)
    got = GR.emu_adamw(p, g, m, v, k, lr, betas[0], betas[1], eps, wd, scale, defect)
    a = (k, GR.f32(lr), GR.f32(betas[0]), GR.f32(betas[1]), GR.f32(eps), GR.f32(wd), 1.0 if scale is None else GR.f32(1.0 / scale))
    ref, bnd = GR.adamw_ref(p, g, m, v, *a), GR.adamw_bound(p, g, m, v, *a)
    res = {name: GR.check(got[i], ref[i], bnd[i]) for i, name in enumerate(("p", "m", "v"))}
    res["g"] = bool(torch.equal(got[3].double(), ref[3]))
    return res


def test_adamw_emulation_is_inside_every_bound():
    for k, betas, wd, scale in ADAM_SWEEP:
        res = _adam_check(4099, k, betas, wd, scale)
        assert res["g"], (k, betas, wd, scale)
        for name in ("p", "m", "v"):
            assert res[name].ratio <= 1.0, (k, betas, wd, scale, name, res[name])


# ---- every planted defect is rejected -------------------------------------------------------------------------------------------------------
def test_rejects_adamw_with_k_equal_to_step():
    assert _adam_check(500, 3, (0.9, 0.999), 1e-2, 1024.0)["p"].ratio <= 1.0
    assert _adam_check(500, 3, (0.9, 0.999), 1e-2, 1024.0, defect="k_is_step")["p"].ratio > 1.0


def test_rejects_adamw_with_weight_decay_after_the_step():
    """lr = wd = 0.1: the two orders differ by lr wd times the update, 1e-3 of it."""
    assert _adam_check(500, 3, (0.9, 0.999), 0.1, None, lr=0.1)["p"].ratio <= 1.0
    assert _adam_check(500, 3, (0.9, 0.999), 0.1, None, lr=0.1, defect="wd_after")["p"].ratio > 1.0


def test_rejects_adamw_without_the_inverse_scale():
    bad = _adam_check(500, 3, (0.9, 0.999), 1e-2, 1024.0, defect="no_inv_scale")
    assert not bad["g"] and bad["p"].ratio > 1.0 and bad["m"].ratio > 1.0 and bad["v"].ratio > 1.0


def test_rejects_adamw_with_sqrt_v_over_bc2():
    assert _adam_check(500, 3, (0.9, 0.999), 1e-2, None, defect="sqrt_v_over_bc2")["p"].ratio > 1.0


SMALL = (256, 64, (3, 70, 1, 64, 7), 3)          # N > 1, unequal widths, P = 145: a partial last chunk


def test_rejects_dswish_without_its_x_term():
    _, clean = _temb_emulated(*SMALL)
    _, bad = _temb_emulated(*SMALL, bwd_defect="dswish_no_x")
    assert clean["dz2"].ratio <= 1.0 and bad["dz2"].ratio > 1.0 and bad["dw0"].ratio > 1.0


def test_rejects_swapped_sin_and_cos_halves():
    clean, _ = _temb_emulated(*SMALL)
    bad, _ = _temb_emulated(*SMALL, fwd_defect="sincos_swapped")
    assert clean["e"].ratio <= 1.0 and bad["e"].ratio > 1.0 and bad["z1"].ratio > 1.0


def test_rejects_add_at_the_sample_major_offset():
    clean, _ = _temb_emulated(*SMALL)
    bad, _ = _temb_emulated(*SMALL, fwd_defect="add_offset")
    assert clean["add"].ratio <= 1.0 and bad["add"].ratio > 1.0


def test_rejects_a_dropped_last_partial_chunk():
    _, clean = _temb_emulated(*SMALL)
    _, bad = _temb_emulated(*SMALL, bwd_defect="drop_last_chunk")
    assert clean["dz2"].ratio <= 1.0 and bad["dz2"].ratio > 1.0


def _qs_rejected(defect):
    _, sched = _sched()
    g = _gen(2)
    src, eps = (torch.rand(3, 1028, generator=g) > 0.7).float(), torch.randn(3, 1028, generator=g)
    t = torch.tensor([0, 999, 417])
    ref, bnd = GR.q_sample_affine_ref(src, 2.0, -1.0, eps, sched, t)
    assert GR.check(GR.emu_q_sample_affine(src, 2.0, -1.0, eps, sched, t), ref, bnd).ratio <= 1.0
    return GR.check(GR.emu_q_sample_affine(src, 2.0, -1.0, eps, sched, t, defect), ref, bnd)


def test_rejects_q_sample_with_one_samples_coefficients_for_all():
    assert _qs_rejected("one_coef").ratio > 1.0


def test_rejects_q_sample_with_the_last_piece_unwritten():
    bad = _qs_rejected("last_piece")
    assert bad.ratio > 1.0 and bad.where[1] >= 1024


def test_rejects_an_advance_that_resets_growth_without_halving_the_scale():
    st, bad = (0, 8.0, 0), (0, 8.0, 0)
    for found in SEQUENCE:
        step, _, scale, growth, _ = GR.advance_ref(st[0], float(found), st[1], st[2], 2.0, 0.5, 2)
        st = (step, scale, growth)
        step, _, scale, growth, _ = GR.emu_advance(bad[0], float(found), bad[1], bad[2], 2.0, 0.5, 2, defect="no_backoff")
        bad = (step, scale, growth)
    assert st[0] == bad[0] and st[2] == bad[2] and st[1] != bad[1]
    assert math.isclose(bad[1] / st[1], 8.0)          # three halvings were skipped
