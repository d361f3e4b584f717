"""The sampler tail (csrc/sampler.hip) against the fp64 references and derived bounds of tests/sampler_fp64ref.py, on the GPU,
through diff_unet_amos_amd.ops: EVERY element of every output a launch writes must satisfy |got - ref| <= bound (nothing is
sampled), the next denoiser input must be the bit-exact fp16 / fp32 image of the stored state with its other channels untouched,
and the in-kernel noise of the shipped plain step must be bit-equal to the field of the VALU form, which is held to the numpy
Philox restatement.  Each case names the instantiation it reaches and asserts the tile walk it is meant to produce from the
device's CU count, the way tail_entry sizes its grid: on a device with another CU count the walk assertion fails instead of the
case quietly not looping.  Every test prints one table row per checked output: entry, form, shape, max err / bound, worst element.

Measured on one MI355X (256 CUs), the largest err / bound per case: see DESIGN.md section 10f.
"""
import os

import numpy as np
import pytest
import torch

import fp64ref as R
import sampler_fp64ref as T

pytestmark = pytest.mark.gpu
DEV = "cuda"
F16, F32 = torch.float16, torch.float32
torch.set_num_threads(max(1, min(16, len(os.sched_getaffinity(0)))))


def _ops():
    from diff_unet_amos_amd import ops
    return ops


def _mode(mode):
    from diff_unet_amos_amd import _native as nv
    return {T.DDPM: nv.MODE_DDPM, T.DDIM: nv.MODE_DDIM, "logits": nv.MODE_LOGITS}[mode]


def _row(entry, form, shape, what, res):
    print(f"{entry:22s} {form:34s} {shape:24s} {what:7s} err/bound {res.ratio:8.4f}  worst at {res.where}: got {res.got:.7g}, "
          f"ref {res.ref:.7g}, bound {res.bound:.3g}")
    assert res.ratio <= 1.0, (entry, form, what, res)


def _walk(c):
    """The grid tail_entry derives on THIS device, and the walk the case is stated for."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    w = T.tile_walk(c["vox"], c["N"], c["wgs"], cus)
    want = dict(tiles=c["tiles"], g=c["g"], walks=c["walks"], last=c["last"])
    assert w == want, (f"case {c['name']}: on {cus} CUs the grid is {w}, the case is written for {want} (256 CUs): "
                       "its workgroups would not walk the tiles this test exists for")
    assert w["walks"][0] >= 2
    return f"{w['tiles']} tiles / g {w['g']}: walks {w['walks'][0]} or {w['walks'][1]}"


# ---- a case on the device ---------------------------------------------------------------------------------------------------
_DEVCASE, _HEAD, _FIELD = {}, {}, {}


def _constants(ops, x, Cc, gamma, beta, vox, slope, what):
    """Statistics with ops.instnorm_stats, the consumers' fp32 scale / shift with ops.instnorm_finalize, held to the float64
    values of the statistics words within the preamble's rounding (as tests/test_launch_sequence_fp64.py does)."""
    N = x.shape[0]
    stats = ops.stats_buffer(N, Cc, DEV)
    ops.instnorm_stats(x, Cc, stats)
    norm = ops.Norm(stats, gamma.to(DEV), beta.to(DEV), vox, slope=slope, eps=1e-5)
    sc, sh = (t.cpu() for t in ops.instnorm_finalize(norm, N, Cc))
    sc64, sh64, b_sc, b_sh = R.finalize(ops.stats_decode(stats).cpu(), gamma, beta, vox, 1e-5)
    for name, got, ref, b in (("scale", sc, sc64, b_sc), ("shift", sh, sh64, b_sh)):
        r = R.check(got, ref, b)
        assert r.ratio <= 1, f"{what}: InstanceNorm {name} of the preamble: {r}"
    return norm, sc, sh


def _device_case(name):
    if name in _DEVCASE:
        return _DEVCASE[name]
    ops = _ops()
    c = T.build_case(name)
    N, V, K, C, cx = c["N"], c["vox"], c["K"], c["C"], c["cx"]
    kv = c.get("kvalid", K)
    sp = (N, *c["dims"])
    d = dict(raw=c["raw"].view(*sp, -1).to(DEV).contiguous(), wf=c["wf"].to(DEV), bf=c["bf"].to(DEV), norm=None, consts=())
    if c["form"] != "identity":
        d["norm"], sc, sh = _constants(ops, d["raw"], kv, c["gamma"], c["beta"], V, c["slope"], f"{name} raw")
        d["consts"] = (sc, sh)
    if c["form"] == "res":
        d["res"] = c["res"].view(*sp, -1).to(DEV).contiguous()
        d["rnorm"], rsc, rsh = _constants(ops, d["res"], kv, c["rgamma"], c["rbeta"], V, c["slope"], f"{name} res")
        d["consts"] = d["consts"] + (rsc, rsh)
        d["ra_src"] = c["ra_src"].view(*sp, -1).to(DEV).contiguous()
    d["seed"] = torch.tensor([T.SEED64], dtype=torch.int64, device=DEV)
    d["step"] = torch.tensor([T.STEP], dtype=torch.int32, device=DEV)
    _DEVCASE[name] = (c, d)
    return c, d


def _field(N, dims, cx):
    """The eps field E [N, vox, cx] (fp32, CPU) the in-kernel generator draws at (SEED64, STEP): a launch of the VALU form with
    zero weights and the DDPM row (0, 0, 1): x_new = 0 * x0^ + 0 * x_t + 1 * eps = eps exactly."""
    key = (N, dims, cx)
    if key not in _FIELD:
        ops = _ops()
        C = cx if cx == 16 else cx - 3
        raw = torch.zeros(N, *dims, 8, dtype=F16, device=DEV)
        z = ops.Norm(ops.stats_buffer(N, 8, DEV), torch.ones(8, device=DEV), torch.zeros(8, device=DEV), dims[0] * dims[1] * dims[2])
        state = torch.zeros(N, *dims, cx, device=DEV)
        coef = torch.zeros(N, 8, device=DEV)
        coef[:, 2] = 1.0
        ops.final_conv_sampler(raw, 8, z, torch.zeros(C, 8, device=DEV), torch.zeros(C, device=DEV), C, _mode(T.DDPM), coef=coef,
                               x_state=state, step_word=torch.tensor([T.STEP], dtype=torch.int32, device=DEV),
                               seed_dev=torch.tensor([T.SEED64], dtype=torch.int64, device=DEV))
        torch.cuda.synchronize()
        _FIELD[key] = state.view(N, -1, cx).cpu()
    return _FIELD[key]


def _launch(c, d, mode, inject, want, coef=None, use_ra=True):
    """One launch of the case; returns the outputs it wrote as CPU [N, V, C] tensors (+ 'xin' [N, V, stride], 'state_full')."""
    ops = _ops()
    N, V, K, C, cx = c["N"], c["vox"], c["K"], c["C"], c["cx"]
    sp = (N, *c["dims"])
    dt = c["dtype"]
    kw = dict(seed_dev=d["seed"], step_word=d["step"])
    out = {}
    if mode != "logits":
        out["state"] = c["xt"].view(*sp, cx).to(DEV).contiguous()
        out["xin"] = torch.full((*sp, cx + c["xin_pad"]), 4.0, dtype=dt, device=DEV)
        kw.update(coef=(T.coef_rows(c["ts"], mode) if coef is None else coef).to(DEV), x_state=out["state"], xin=out["xin"])
        if inject:
            kw["noise"] = c["noise"].permute(0, 2, 1).contiguous().view(N, C, *c["dims"]).to(DEV)
        if "xsum" in want:
            out["xsum"] = c["xsum0"].view(*sp, cx).to(DEV).contiguous()
            kw["xstart_sum"] = out["xsum"]
        if "xstart" in want:
            out["xstart"] = torch.zeros(N, C, *c["dims"], device=DEV)
            kw["xstart"] = out["xstart"]
    if "logits" in want or mode == "logits":
        out["logits"] = torch.zeros(N, C, *c["dims"], device=DEV)
        kw["logits"] = out["logits"]
    if c["form"] == "res":
        kv = c["kvalid"]
        kw["residual"] = (d["res"], d["rnorm"], d["ra_src"] if use_ra else None, c["ra_off"] if use_ra else 0, kv)
    ops.final_conv_sampler(d["raw"], K, d["norm"], d["wf"], d["bf"], C, _mode(mode), **kw)
    torch.cuda.synchronize()
    got = {}
    ncv = lambda t: t.view(N, C, V).permute(0, 2, 1).contiguous().cpu()
    if "logits" in out:
        got["L"] = ncv(out["logits"])
    if mode != "logits":
        # the next input: the round-to-nearest image of the stored state in channels [0, C), everything behind untouched
        xin, st = out["xin"], out["state"]
        assert torch.equal(xin[..., :C], st[..., :C].to(dt)), f"{c['name']} {mode}: xin is not the stored state rounded to {dt}"
        assert bool((xin[..., C:] == 4.0).all()), f"{c['name']} {mode}: channels >= C of xin were written"
        got["xn"] = st.view(N, V, cx)[..., :C].cpu()
        got["state_full"] = st.view(N, V, cx).cpu()
        if "xsum" in out:
            got["xsum"] = out["xsum"].view(N, V, cx)[..., :C].cpu()
        if "xstart" in out:
            got["x0"] = ncv(out["xstart"])
    return got


def _head(c, d, use_ra=True):
    key = (c["name"], use_ra)
    if key not in _HEAD:
        c["use_ra"] = use_ra
        _HEAD[key] = T.case_reference(c, d["consts"], None, None, logits_only=True)
        inside, below, above = T.input_conditions(_HEAD[key]["L"])
        assert inside >= 0.40 and below >= 0.05 and above >= 0.05, (c["name"], inside, below, above)
    return _HEAD[key]


def _check(c, d, entry, form, mode, got, eps, use_ra=True):
    c["use_ra"] = use_ra
    head = _head(c, d, use_ra)
    ref = head if mode == "logits" else T.case_reference(c, d["consts"], mode, eps.double(), head=head)
    shape = f"{c['N']}x{'x'.join(map(str, c['dims']))} {c.get('kvalid', c['K'])}->{c['C']}"
    n = 0
    for key, rk, bk in (("L", "L", "bL"), ("x0", "x0", "b0"), ("xn", "xn", "bn"), ("xsum", "xsum", "bs")):
        if key in got:
            _row(entry, form, shape, f"{mode[:4]}/{key}", R.check(got[key], ref[rk], ref[bk]))
            n += 1
    assert n > 0


# ---- a. the shipped plain step ----------------------------------------------------------------------------------------------
def test_plain_form_draws_the_field_of_the_valu_form_bit_for_bit():
    """final_conv_sampler_mfma_kernel<2, false, false> with the row (0, 0, 1) stores its eps: over 16 samples and 107 tiles walked
    3 or 2 per workgroup it must equal the VALU form's field E bit for bit (the counter inside the software-pipelined loop), and
    E must be the Philox restatement at (n vox + v, step 7, quads 0..3) under a key with a non-zero high word."""
    c, d = _device_case("a")
    walk = _walk(c)
    E = _field(c["N"], c["dims"], c["cx"])
    coef = torch.zeros(c["N"], 8)
    coef[:, 2] = 1.0
    got = _launch(c, d, T.DDPM, False, (), coef=coef)
    diff = got["state_full"] != E
    if bool(diff.any()):
        idx = diff.nonzero()
        first = tuple(int(v) for v in idx[0])
        raise AssertionError(f"plain form and VALU form differ in {len(idx)} of {E.numel()} elements, first at (n, v, class) {first} "
                             f"(tile {first[1] // 256}): {float(got['state_full'][first])} vs {float(E[first])}; largest "
                             f"|difference| {float((got['state_full'] - E).abs().max())}")
    want = T.philox_normals(T.SEED64, T.STEP, c["N"], c["vox"], 4)
    err = np.abs(E.double().numpy() - want)
    k = np.unravel_index(int(err.argmax()), err.shape)
    print(f"{'final_conv_sampler':22s} {'<2,false,false> == VALU == Philox':34s} {walk}: bit-equal over {E.numel()} values; "
          f"|E - restatement| max {err.max():.3g} at {tuple(int(v) for v in k)}")
    assert err.max() < T.PHILOX_TOL, (float(err.max()), k)


@pytest.mark.parametrize("mode", [T.DDPM, T.DDIM])
def test_plain_pipelined_step(mode):
    """<2, false, false>: fp16, K 64, C 16, N 16 each on its own coefficient row (t = 0 included), 23 x 29 x 41 voxels, xin stride
    24, in-kernel noise with seed_dev and step word 7, no extra outputs: the shipped DDPM step (and the same instantiation in
    DDIM mode).  eps operand of the reference: the field E of the bit-for-bit test above."""
    c, d = _device_case("a")
    walk = _walk(c)
    E = _field(c["N"], c["dims"], c["cx"])
    got = _launch(c, d, mode, False, ())
    _check(c, d, "final_conv_sampler", f"a <2,false,false> {walk}", mode, got, E)


# ---- b. EXTRA <2> -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,mode", [("i", T.DDIM), ("ii", T.DDPM), ("ii", T.DDIM)])
def test_extra_form_k64(variant, mode):
    """<2, false, true> at case (a)'s shape: (i) xstart_sum + in-kernel noise, what the DDIM loop ships; (ii) injected noise +
    logits + xstart + xstart_sum."""
    c, d = _device_case("b")
    walk = _walk(c)
    if variant == "i":
        got = _launch(c, d, mode, False, ("xsum",))
        eps = _field(c["N"], c["dims"], c["cx"])
    else:
        got = _launch(c, d, mode, True, ("xsum", "logits", "xstart"))
        eps = c["noise"]
    _check(c, d, "final_conv_sampler", f"b({variant}) <2,false,true> {walk}", mode, got, eps)


# ---- c. <1> and <4> ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["c1", "c4"])
@pytest.mark.parametrize("mode", [T.DDPM, T.DDIM])
def test_k32_and_k128_forms(name, mode):
    """<1> (K 32, C 13: a partial class quad) and <4> (K 128, C 9) at N 16, 19 x 24 x 31.  Both grids are sized with 3 workgroups
    per CU (tail_entry passes 3 whatever K is): g = 48 per sample, 56 tiles, walks 2 or 1.  <4> is compiled with
    __launch_bounds__(256, 2): where only two of its workgroups fit a CU, the 768 of the grid take a second round; the values do
    not depend on that.  DDPM with in-kernel noise + xstart_sum, DDIM with injected noise and every output."""
    c, d = _device_case(name)
    walk = _walk(c)
    if mode == T.DDPM:
        got = _launch(c, d, mode, False, ("xsum", "logits"))
        eps = _field(c["N"], c["dims"], c["cx"])
    else:
        got = _launch(c, d, mode, True, ("xsum", "logits", "xstart"))
        eps = c["noise"]
    _check(c, d, "final_conv_sampler", f"{name} <{c['K'] // 32},false,true> {walk}", mode, got, eps)


# ---- d. residual forms -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["d1", "d2"])
@pytest.mark.parametrize("use_ra", [True, False], ids=["ra", "no-ra"])
def test_residual_forms(name, use_ra):
    """<1, true> (24 real channels in K 32) and <2, true> (48 in K 64), N 16, 19 x 24 x 31, res with mean 0.5 and scale 2, both
    norms' gamma / beta away from (1, 0), ra_src read at channel offset 8, non-zero weights in the padding columns (they must
    meet exact zeros): logits mode, and DDPM with in-kernel noise + xstart_sum.  g = 2 * CUs // 16 = 32: walks 2 or 1, two voxel
    blocks in flight (MBS = 2)."""
    c, d = _device_case(name)
    walk = _walk(c)
    form = f"{name} <{c['K'] // 32},true> {'ra' if use_ra else 'no ra'} {walk}"
    got = _launch(c, d, "logits", False, (), use_ra=use_ra)
    _check(c, d, "final_conv_sampler_res", form, "logits", got, None, use_ra)
    got = _launch(c, d, T.DDPM, False, ("xsum",), use_ra=use_ra)
    _check(c, d, "final_conv_sampler_res", form, T.DDPM, got, _field(c["N"], c["dims"], c["cx"]), use_ra)


# ---- e. VALU forms ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in T.CASES if n.startswith("e")])
@pytest.mark.parametrize("mode", [T.DDPM, T.DDIM])
def test_valu_forms(name, mode):
    """final_conv_sampler_kernel<T, CX>: N 3, 5 x 7 x 37 = 1295 voxels (a partial last block), fp32 (C, K) = (3, 8), (16, 24),
    (20, 64), (29, 136) -> CX 8, 16, 24, 32 and fp16 (16, 24), (20, 64); injected noise, every output."""
    c, d = _device_case(name)
    got = _launch(c, d, mode, True, ("xsum", "logits", "xstart"))
    _check(c, d, "final_conv_sampler", f"{name} VALU<{'f16' if c['dtype'] == F16 else 'f32'},{c['cx']}>", mode, got, c["noise"])


def test_valu_form_noise_at_cx32_is_the_philox_restatement():
    """In-kernel noise of the VALU form at CX = 32: class quads 0 to 7 of three samples against philox_normals, then a DDPM step
    on that field."""
    name = "e32-29-136"
    c, d = _device_case(name)
    E = _field(c["N"], c["dims"], 32)
    want = T.philox_normals(T.SEED64, T.STEP, c["N"], c["vox"], 8)
    err = np.abs(E.double().numpy() - want)
    k = np.unravel_index(int(err.argmax()), err.shape)
    print(f"{'final_conv_sampler':22s} {'VALU<f16,32> noise, quads 0..7':34s} |E - restatement| max {err.max():.3g} at "
          f"{tuple(int(v) for v in k)}")
    assert err.max() < T.PHILOX_TOL, (float(err.max()), k)
    got = _launch(c, d, T.DDPM, False, ("xsum", "xstart"))
    _check(c, d, "final_conv_sampler", f"{name} VALU<f32,32> in-kernel noise", T.DDPM, got, E)


# ---- f. identity form --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["logits", T.DDPM, T.DDIM])
def test_identity_form(mode):
    """norm = None (an already materialised activation, slope 1), K 64, fp16: the MFMA form on exact operands."""
    c, d = _device_case("f")
    got = _launch(c, d, mode, True, ("xsum", "logits", "xstart"))
    _check(c, d, "final_conv_sampler", "f <2,false,true> identity", mode, got, c["noise"])


# ---- g. the grid-stride loops of the elementwise kernels ----------------------------------------------------------------------
def test_grid_stride_loops_of_q_sample_and_sampler_step():
    """q_sample_kernel and sampler_step_kernel cap their grid at 16384 blocks of 256: N = 3 samples of (2 * 16384 * 256 + 79) // 3
    elements make every thread loop twice and 79 threads a third time, with sample boundaries inside blocks.  Every element
    against update_ref / q_sample_ref with dL = 0 (the operands are exact), both modes, xstart_out and xstart_sum."""
    ops = _ops()
    N, per = 3, (2 * 16384 * 256 + 77 + 2) // 3
    total = N * per
    assert total > 2 * 16384 * 256 and total - 2 * 16384 * 256 < 256 and per % 256 != 0
    g = torch.Generator().manual_seed(77)
    L = 1.2 * torch.randn(N, per, generator=g)
    xt, eps, s0 = (torch.randn(N, per, generator=g) for _ in range(3))
    Ld, xd, ed = L.to(DEV), xt.to(DEV), eps.to(DEV)
    shape = f"{N}x{per}"
    from diff_unet_amos_amd.gaussian_diffusion import make_spaced
    qc = make_spaced(1000, [1000]).q_coef(torch.tensor([0, 500, 999])).float()
    got = ops.q_sample(Ld, ed, qc.to(DEV)).cpu()
    ref, bnd = T.q_sample_ref(qc[:, None, 0], qc[:, None, 1], L.double(), eps.double())
    _row("q_sample", "grid-stride, 16384 blocks", shape, "xt", R.check(got, ref, bnd))
    for mode in (T.DDPM, T.DDIM):
        coef = T.coef_rows(T.T3, mode)
        xs, ssum = torch.empty_like(Ld), s0.to(DEV)
        xn = ops.sampler_step(_mode(mode), Ld, xd, ed, coef.to(DEV), xstart_out=xs, xstart_sum=ssum)
        torch.cuda.synchronize()
        x0, x, b0, bx = T.update_ref(mode, coef[:, None, :], L.double(), xt.double(), eps.double(), 0.0)
        s, bs = T.xsum_ref(s0.double(), x0, 0.0)
        _row("sampler_step", "grid-stride, 16384 blocks", shape, f"{mode}/xn", R.check(xn.cpu(), x, bx))
        assert torch.equal(xs.cpu().double(), x0), f"{mode}: xstart_out is not the clamp of its input"
        _row("sampler_step", "grid-stride, 16384 blocks", shape, f"{mode}/xsum", R.check(ssum.cpu(), s, bs))
