"""The training-glue kernels on the GPU (csrc/train_glue.hip: q_sample_affine, temb_train_fwd / temb_train_bwd, grads_nonfinite,
adamw_step, adamw_advance, stats_channel_sums) against the fp64 references and derived bounds of tests/glue_fp64ref.py.  Every
case checks EVERY element: ``fp64ref.check(...).ratio <= 1`` with the worst element in the message; the exact quantities (the
overflow flag, the loss-scale rule, the unscaled gradient, guard words, skipped steps) are compared for equality.  Every output
is pre-filled with NaN and surrounded by guard words, so a word that is not written, or one written past an end, fails.  The
figures are printed before they are asserted (run with -s to see them; the module prints the largest ratio per kernel at its
end).  The last test needs only the shared library: every entry point returns ERR_ARG for bad arguments before any launch."""
import collections
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest
import torch

import glue_fp64ref as GR

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
F32, F64 = torch.float32, torch.float64
NAN = float("nan")
SENT = 777.25                      # guard words: finite, positive (a v that takes it stays valid), unlike any result
GUARD = 64                         # floats of guard on either side of a buffer (256 bytes: alignment is kept)
WORST = collections.defaultdict(float)


def _ops():
    from diff_unet_amos_amd import ops
    return ops


def _bits(x):
    return x.contiguous().view(torch.int32)


def _same_bits(a, b):
    return bool(torch.equal(_bits(a), _bits(b)))


def _note(kernel, what, res):
    """Print and record CheckResults (a dict or one), then assert them."""
    res = res if isinstance(res, dict) else {"": res}
    top = max(res.items(), key=lambda kv: kv[1].ratio)
    WORST[kernel] = max(WORST[kernel], top[1].ratio)
    print(f"{kernel} {what}: worst {top[0]} {top[1]}")
    for k, v in res.items():
        assert v.ratio <= 1.0, (kernel, what, k, v)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if WORST:
        print("\nlargest |err| / bound per kernel: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(WORST.items())))


def _guarded(n, fill=NAN, lead=0):
    """(whole buffer, the n-element payload view ``lead`` floats past the first guard): guards hold SENT, the payload ``fill``."""
    buf = torch.full((GUARD + lead + n + GUARD,), SENT, dtype=F32, device=DEV)
    view = buf[GUARD + lead:GUARD + lead + n]
    view.fill_(fill)
    return buf, view


def _guards_intact(buf, lead, n):
    return bool((buf[:GUARD + lead] == SENT).all()) and bool((buf[GUARD + lead + n:] == SENT).all())


# ---- q_sample_affine -------------------------------------------------------------------------------------------------------------------
T_STEPS = 1000


@pytest.fixture(scope="module")
def sched():
    betas = torch.linspace(1e-4, 2e-2, T_STEPS, dtype=F64)
    acp = torch.cumprod(1 - betas, 0)
    return torch.stack([acp.sqrt(), (1 - acp).sqrt()], 1).float().to(DEV).contiguous()


def _q_sample_case(sched, N, per, ts, leads=(0, 0, 0), what=""):
    """src, eps and out are views ``leads`` floats into guarded buffers; one launch per timestep vector in ``ts``."""
    g = torch.Generator(device=DEV).manual_seed(per % 9973)
    n = N * per
    sbuf, src = _guarded(n, 0.0, leads[0])
    ebuf, eps = _guarded(n, 0.0, leads[1])
    src.copy_((torch.rand(n, device=DEV, generator=g) > 0.7).float())
    eps.copy_(torch.randn(n, device=DEV, generator=g))
    for t in ts:
        obuf, out = _guarded(n, NAN, leads[2])
        t = torch.tensor(t, dtype=torch.int64, device=DEV)
        got = _ops().q_sample_affine(src.view(N, per), 2.0, -1.0, eps.view(N, per), sched, t, out=out.view(N, per))
        assert got.data_ptr() == out.data_ptr()
        ref, bnd = GR.q_sample_affine_ref(src.view(N, per), 2.0, -1.0, eps.view(N, per), sched, t)
        _note("q_sample_affine", f"{what} N {N} per {per} t {t.tolist()}", GR.check(got, ref, bnd))
        del ref, bnd
        assert _guards_intact(obuf, leads[2], n) and _guards_intact(sbuf, leads[0], n) and _guards_intact(ebuf, leads[1], n)


T_PLAIN, T_CLAMPED = (0, T_STEPS - 1, 417), (-5, T_STEPS + 7, 0)


@gpu
@pytest.mark.parametrize("n4", [1, 255, 256, 257, 1023, 1024, 1025, 2 * 1024 + 513, 4 * 1024 + 1])
def test_q_sample_affine_vector_path(sched, n4):
    """n4 sixteen-byte pieces per sample: the clamped-load tail either side of a multiple of 256 and of one workgroup's 1024.
    The second launch's timesteps lie outside [0, T - 1]: the kernel's clamp is the contract.  The vector path's own grid cap
    (65535 workgroups of 1024 pieces) needs more than 1 GiB per stream and is left out on purpose."""
    _q_sample_case(sched, 3, 4 * n4, (T_PLAIN, T_CLAMPED), what="vector")


@gpu
@pytest.mark.parametrize("per,leads", [(4 * 257 + 1, (0, 0, 0)), (4 * 257 + 2, (0, 0, 0)), (4 * 257 + 3, (0, 0, 0)),
                                       (4 * 257, (1, 0, 0)), (4 * 257, (0, 1, 0)), (4 * 257, (0, 0, 1))],
                         ids=["per%4=1", "per%4=2", "per%4=3", "src+4B", "eps+4B", "out+4B"])
def test_q_sample_affine_scalar_path(sched, per, leads):
    _q_sample_case(sched, 3, per, (T_PLAIN, T_CLAMPED), leads, what="scalar")


@gpu
def test_q_sample_affine_scalar_grid_stride_loop(sched):
    """per = 65535 * 256 + 259: three elements more than the capped grid covers in one pass (67 MB per stream; the reference is
    evaluated on the device)."""
    _q_sample_case(sched, 1, 65535 * 256 + 259, ((417,),), what="grid-stride")


# ---- timestep embedding ---------------------------------------------------------------------------------------------------------------------
P4096 = [512, 1000, 3, 2048, 533]
LAYOUTS = [("shipped", 64, GR.SHIPPED_WIDTHS), ("half3", 3, GR.SHIPPED_WIDTHS), ("half512", 512, GR.SHIPPED_WIDTHS),
           ("ragged145", 64, [1, 3, 64, 5, 70, 2]), ("P129", 64, [7, 58, 64]), ("sixteen-ones", 64, [1] * 16), ("P4096", 64, P4096)]


def _temb_forward(hid, half, couts, N, shift):
    from diff_unet_amos_amd import _native as nv
    ops = _ops()
    w0, b0, w1, b1, ws, bs = GR.make_temb_params(hid, half, couts, 100 + shift, DEV)
    t, freqs = GR.make_timesteps(N, shift).to(DEV), GR.temb_freqs(half).to(DEV)
    P, width = sum(couts), 2 * half + 4 * hid
    abuf, add = _guarded(N * P)
    sbuf, saved = _guarded(N * width)
    rc = nv.lib().dua_temb_train_fwd(N, nv.ptr(t), nv.ptr(freqs), half, hid, nv.ptr(w0), nv.ptr(b0), nv.ptr(w1), nv.ptr(b1),
                                     C.byref(ops._temb_blocks(ws, bs=bs)), nv.ptr(add), nv.ptr(saved), nv.stream_ptr())
    assert rc == 0
    saved = saved.view(N, width)
    assert _guards_intact(abuf, 0, N * P) and _guards_intact(sbuf, 0, N * width)
    return dict(t=t, freqs=freqs, w0=w0, b0=b0, w1=w1, b1=b1, ws=ws, bs=bs, add=add, saved=saved)


def _temb_backward(c, hid, half, couts, N, dadd):
    """One dua_temb_train_bwd into a NaN-filled flat buffer laid out as ops.temb_train_bwd lays it out, between guards."""
    from diff_unet_amos_amd import _native as nv
    ops = _ops()
    P, ed = sum(couts), 2 * half
    nscratch = N * hid * (1 + -(-P // 64) + hid // 64)
    pad = -P % 4
    total = hid * ed + hid + hid * hid + hid + P * hid + P + pad + nscratch
    buf, flat = _guarded(total)
    pos = [0]

    def take(*shape):
        n = int(np.prod(shape))
        v = flat[pos[0]:pos[0] + n].view(*shape)
        pos[0] += n
        return v

    out = dict(dw0=take(hid, ed), db0=take(hid), dw1=take(hid, hid), db1=take(hid))
    out["dw"] = [take(co, hid) for co in couts]
    out["db"] = [take(co) for co in couts]
    gap = flat[pos[0]:pos[0] + pad]
    pos[0] += pad
    scratch = take(nscratch)
    assert pos[0] == total and scratch.data_ptr() % 16 == 0
    rc = nv.lib().dua_temb_train_bwd(N, half, hid, nv.ptr(c["w1"]), C.byref(ops._temb_blocks(c["ws"], dws=out["dw"], dbs=out["db"])),
                                     nv.ptr(dadd), nv.ptr(c["saved"]), nv.ptr(scratch), nv.ptr(out["dw0"]), nv.ptr(out["db0"]),
                                     nv.ptr(out["dw1"]), nv.ptr(out["db1"]), nv.stream_ptr())
    assert rc == 0
    assert _guards_intact(buf, 0, total) and bool(torch.isnan(gap).all())
    assert bool(torch.isfinite(scratch).all()), "a scratch word was not written"
    out["dz2"] = scratch[:N * hid].view(N, hid)
    return out, flat


@gpu
@pytest.mark.parametrize("layout", LAYOUTS, ids=[l[0] for l in LAYOUTS])
@pytest.mark.parametrize("N", [1, 3, 64])
@pytest.mark.parametrize("hid", [256, 512])
def test_temb_train_forward_and_backward(hid, N, layout):
    """Through the C entry points, stage by stage on what each launch read: e, z1, h1, z2, s, add; dz2 and all 4 + 2 B parameter
    gradients from one random cotangent per block.  Every word must come out finite and within bound, the guards unchanged,
    and a second backward bit-equal to the first."""
    name, half, couts = layout
    shift = LAYOUTS.index(layout) + (hid // 256) + N
    c = _temb_forward(hid, half, couts, N, shift)
    ref = GR.temb_fwd_ref(c["t"], c["freqs"], c["w0"], c["b0"], c["w1"], c["b1"], c["ws"], c["bs"], c["saved"])
    _note("temb_train_fwd", f"{name} hid {hid} N {N}", GR.temb_fwd_checks(c["add"], c["saved"], ref, half, hid))
    g = torch.Generator(device=DEV).manual_seed(shift)
    dadd = GR.block_major([torch.randn(N, co, device=DEV, generator=g) for co in couts]).contiguous()
    got, flat = _temb_backward(c, hid, half, couts, N, dadd)
    ref = GR.temb_bwd_ref(dadd, c["w1"], c["ws"], c["saved"], half, dz2=got["dz2"])
    _note("temb_train_bwd", f"{name} hid {hid} N {N}", GR.temb_bwd_checks(got, ref))
    _, again = _temb_backward(c, hid, half, couts, N, dadd)
    assert _same_bits(flat, again), "two backward runs differ"


@gpu
def test_temb_wrappers_hand_over_the_same_launches():
    """ops.temb_train_fwd / ops.temb_train_bwd (torch.empty outputs) at a P that is no multiple of 4: bit-equal to the C path."""
    ops = _ops()
    hid, half, couts, N = 256, 64, [7, 58, 64], 3
    c = _temb_forward(hid, half, couts, N, 5)
    add, saved = ops.temb_train_fwd(c["t"], half, c["w0"], c["b0"], c["w1"], c["b1"], c["ws"], c["bs"])
    assert _same_bits(add, c["add"]) and _same_bits(saved, c["saved"])
    dadd = torch.randn(N * sum(couts), device=DEV)
    got, _ = _temb_backward(c, hid, half, couts, N, dadd)
    dw0, db0, dw1, db1, dws, dbs = ops.temb_train_bwd(dadd, saved, half, c["w1"], c["ws"])
    for a, b in zip([dw0, db0, dw1, db1, *dws, *dbs], [got["dw0"], got["db0"], got["dw1"], got["db1"], *got["dw"], *got["db"]]):
        assert _same_bits(a, b)


# ---- grads_nonfinite ---------------------------------------------------------------------------------------------------------------------------
PLANTS = [(4100, 0), (4100, 4099), (4100, 4095), (4100, 4096), (4100, 4097), (5, 4), (6, 5), (7, 6), (8193, 8192), (4098, 4097),
          (4099, 4098), (70001, 70000)]


@gpu
@pytest.mark.parametrize("lead", [0, 1], ids=["aligned", "offset4B"])
@pytest.mark.parametrize("slot", [(0, 64), (63, 64), (64, 65)], ids=["first-of-64", "last-of-64", "first-of-second-list"])
def test_grads_nonfinite_finds_one_planted_value(slot, lead):
    """One non-finite value per launch: at both ends, at a 4096-element chunk boundary, in every scalar tail length, in the last
    chunk of a long tensor; the carrier 16-byte aligned or 4 bytes off; first or last of a list, or first of the second list."""
    ops = _ops()
    index, count = slot
    g = torch.Generator(device=DEV).manual_seed(7)
    fillers = [torch.randn(17, device=DEV, generator=g) for _ in range(count - 1)]
    found = torch.zeros((), device=DEV)
    for n in sorted({p[0] for p in PLANTS}):
        buf = torch.randn(n + 8, device=DEV, generator=g)
        carrier = buf[lead:lead + n]
        assert carrier.data_ptr() % 16 == 4 * lead
        grads = fillers[:index] + [carrier] + fillers[index:]
        assert len(grads) == count and grads[index] is carrier
        ops.grads_nonfinite(grads, found)
        assert float(found) == 0.0, f"n {n}: a finite list was flagged"
        for pos in [p[1] for p in PLANTS if p[0] == n]:
            for bad in (float("inf"), float("-inf"), NAN):
                keep = carrier[pos].clone()
                carrier[pos] = bad
                found.zero_()
                ops.grads_nonfinite(grads, found)
                assert float(found) == 1.0, f"n {n}, element {pos}, {bad}: not found"
                carrier[pos] = keep
        found.zero_()


@gpu
@pytest.mark.parametrize("lead", [0, 1], ids=["aligned", "offset4B"])
def test_grads_nonfinite_leaves_extreme_finite_values_alone(lead):
    ops = _ops()
    specials = torch.tensor([GR.FLT_MAX, -GR.FLT_MAX, 1e-45, -1e-45, 1e-40, -0.0, 2.0 ** -126, 0.0], device=DEV)
    found = torch.zeros((), device=DEV)
    grads = []
    for i in range(65):
        n = 70001 if i == 64 else (4100 if i == 0 else 5 + i % 4)
        buf = torch.zeros(n + 8, device=DEV)
        t = buf[lead:lead + n]
        t.copy_(specials[torch.arange(n, device=DEV) % specials.numel()])
        grads.append(t)
    ops.grads_nonfinite(grads, found)
    assert float(found) == 0.0


# ---- adamw_step ------------------------------------------------------------------------------------------------------------------------------------
AD_SIZES = [1, 3, 5, 64, 130, 4095, 4096, 4097, 8193, 70001] + [9 + 2 * i for i in range(55)]
AD_GAP = 8


@pytest.fixture(scope="module")
def adam_case():
    """Four flat buffers holding 65 tensors between 8-word sentinel gaps (every tensor starts on a multiple of four floats), the
    pristine copies, and the mask of tensor words."""
    starts, off = [], AD_GAP
    for n in AD_SIZES:
        starts.append(off)
        off += -(-n // 4) * 4 + AD_GAP
    total = off
    mask = torch.zeros(total, dtype=torch.bool)
    for s, n in zip(starts, AD_SIZES):
        mask[s:s + n] = True
    pristine = [torch.where(mask, x, torch.full_like(x, SENT)).to(DEV) for x in GR.make_adam_inputs(total, 12)]
    work = [torch.zeros(total + 4, device=DEV) for _ in range(4)]
    return dict(starts=starts, total=total, mask=mask.to(DEV), pristine=pristine, work=work)


def _adam_views(case, leads):
    bases = [w[l:l + case["total"]] for w, l in zip(case["work"], leads)]
    for b, src in zip(bases, case["pristine"]):
        b.copy_(src)
    return bases, [[b[s:s + n] for s, n in zip(case["starts"], AD_SIZES)] for b in bases]


AD_LEADS = {"aligned": (0, 0, 0, 0), "g-offset": (0, 1, 0, 0), "v-offset": (0, 0, 0, 1)}
LR_HOST, LR_DEVICE, EPS = 3e-3, 7e-4, 1e-8


@gpu
@pytest.mark.parametrize("leads", list(AD_LEADS), ids=list(AD_LEADS))
@pytest.mark.parametrize("k", [1, 2, 10, 1000, 100001])
def test_adamw_step_every_element(adam_case, k, leads):
    """One step from step = k - 1 over 65 tensors (two by-value lists): p, m, v of every element against adamw_ref within
    adamw_bound; g' exactly fl(g inv) when stored, untouched when not; every sentinel word untouched.  Swept: betas, weight
    decay, the loss scale (None: the null pointer), lr_dev (the device value must win over the host's), store_grad."""
    ops = _ops()
    mask, pristine = adam_case["mask"], adam_case["pristine"]
    step = torch.full((), k - 1, dtype=torch.int32, device=DEV)
    found = torch.zeros((), device=DEV)
    lr_dev = torch.full((), LR_DEVICE, device=DEV)
    tiny = torch.full_like(pristine[0], 1e-300, dtype=F64)
    for betas, wd, scale, use_dev in itertools.product(((0.9, 0.999), (0.5, 0.9)), (0.0, 1e-2), (None, 1024.0), (False, True)):
        lr = float(lr_dev) if use_dev else GR.f32(LR_HOST)
        inv = 1.0 if scale is None else GR.f32(1.0 / scale)
        a = (k, lr, GR.f32(betas[0]), GR.f32(betas[1]), GR.f32(EPS), GR.f32(wd), inv)
        ref, bnd = GR.adamw_ref(*pristine, *a), GR.adamw_bound(*pristine, *a)
        ref = [torch.where(mask, r, x.double()) for r, x in zip(ref[:3], (pristine[0], pristine[2], pristine[3]))] + [ref[3]]
        bnd = [torch.where(mask, b, tiny) for b in bnd]
        gs = None if scale is None else torch.full((), scale, device=DEV)
        for store in (False, True):
            bases, views = _adam_views(adam_case, AD_LEADS[leads])
            ops.adamw_step(*views, step, LR_HOST, betas, EPS, wd, lr_dev=lr_dev if use_dev else None, grad_scale=gs,
                           found_inf=found, store_grad=store)
            what = f"k {k} {leads} betas {betas} wd {wd} scale {scale} lr_dev {use_dev} store {store}"
            _note("adamw_step", what, {"p": GR.check(bases[0], ref[0], bnd[0]), "m": GR.check(bases[2], ref[1], bnd[1]),
                                       "v": GR.check(bases[3], ref[2], bnd[2])})
            want_g = torch.where(mask, ref[3].float(), pristine[1]) if store else pristine[1]
            assert _same_bits(bases[1], want_g), what + ": g"
    assert int(step) == k - 1 and float(found) == 0.0


@gpu
@pytest.mark.parametrize("leads", list(AD_LEADS), ids=list(AD_LEADS))
def test_adamw_step_is_skipped_when_an_overflow_was_found(adam_case, leads):
    ops = _ops()
    step = torch.full((), 4, dtype=torch.int32, device=DEV)
    found = torch.ones((), device=DEV)
    bases, views = _adam_views(adam_case, AD_LEADS[leads])
    ops.adamw_step(*views, step, LR_HOST, (0.9, 0.999), EPS, 1e-2, grad_scale=torch.full((), 1024.0, device=DEV), found_inf=found,
                   store_grad=True)
    for b, src in zip(bases, adam_case["pristine"]):
        assert _same_bits(b, src)
    assert float(found) == 1.0 and int(step) == 4


# ---- adamw_advance -----------------------------------------------------------------------------------------------------------------------------------
@gpu
def test_adamw_advance_equals_the_rule_step_by_step():
    """From 2^126 at interval 2: a growth to 2^127, a growth that would pass FLT_MAX (the scale stays, growth resets), an
    overflow, a double overflow, growths again."""
    ops = _ops()
    sequence = [0, 0, 0, 0, 1, 0, 1, 1, 0, 0, 0, 0, 0]
    step = torch.zeros((), dtype=torch.int32, device=DEV)
    scale = torch.full((), 2.0 ** 126, device=DEV)
    growth = torch.zeros((), dtype=torch.int32, device=DEV)
    found, seen = torch.zeros((), device=DEV), torch.full((), 5.0, device=DEV)
    st = (0, 0.0, 2.0 ** 126, 0)
    scales = []
    for i, bad in enumerate(sequence):
        found.fill_(float(bad))
        ops.adamw_advance(step, found, scale, growth, 2.0, 0.5, 2, seen=seen)
        want = GR.advance_ref(st[0], float(bad), st[2], st[3], 2.0, 0.5, 2)
        got = (int(step), float(found), float(scale), int(growth), float(seen))
        assert got == want, (i, got, want)
        st = want[:4]
        scales.append(want[2])
    assert scales[1] == 2.0 ** 127 and scales[3] == 2.0 ** 127 and scales[4] == 2.0 ** 126 and scales[7] == 2.0 ** 124
    assert int(step) == sequence.count(0)


@gpu
def test_adamw_advance_null_forms():
    ops = _ops()
    mk = lambda v, dt=F32: torch.full((), v, dtype=dt, device=DEV)      # noqa: E731
    for bad in (0.0, 1.0):
        # no scale: growth still counts; no growth: the scale still backs off; no seen; no found_inf: always a good step
        step, found, growth, seen = mk(3, torch.int32), mk(bad), mk(1, torch.int32), mk(5.0)
        ops.adamw_advance(step, found, None, growth, 2.0, 0.5, 2, seen=seen)
        assert (int(step), float(found), None, int(growth), float(seen)) == GR.advance_ref(3, bad, None, 1, 2.0, 0.5, 2)
        step, found, scale, seen = mk(3, torch.int32), mk(bad), mk(8.0), mk(5.0)
        ops.adamw_advance(step, found, scale, None, 2.0, 0.5, 2, seen=seen)
        assert (int(step), float(found), float(scale), None, float(seen)) == GR.advance_ref(3, bad, 8.0, None, 2.0, 0.5, 2)
        step, found, scale, growth = mk(3, torch.int32), mk(bad), mk(8.0), mk(1, torch.int32)
        ops.adamw_advance(step, found, scale, growth, 2.0, 0.5, 2, seen=None)
        assert (int(step), float(found), float(scale), int(growth)) == GR.advance_ref(3, bad, 8.0, 1, 2.0, 0.5, 2)[:4]
    step, scale, growth, seen = mk(3, torch.int32), mk(8.0), mk(1, torch.int32), mk(5.0)
    ops.adamw_advance(step, None, scale, growth, 2.0, 0.5, 2, seen=seen)
    assert (int(step), float(scale), int(growth), float(seen)) == (4, 16.0, 0, 0.0)


# ---- stats_channel_sums ------------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("N,C,Cx", [(1, 300, 304), (3, 300, 304), (1, 24, 24)])
def test_stats_channel_sums(N, C, Cx):
    """C = 300 in rows of c_pad = 320: the channel index leaves the first 256-thread block.  ops.instnorm_stats takes channel
    counts that are multiples of 8, so the statistics are accumulated over Cx = 304 channels and the first 300 are summed."""
    ops = _ops()
    g = torch.Generator(device=DEV).manual_seed(C + N)
    x = (torch.randn(N, 5, 6, 7, Cx, device=DEV, generator=g) * 3).half()
    st = ops.stats_buffer(N, Cx, x.device)
    assert st.shape[3] == (320 if C == 300 else 64)
    ops.instnorm_stats(x, Cx, st)
    got = ops.stats_channel_sums(st, C)
    ref, bnd = GR.stats_channel_sums_ref(st, C)
    assert got.shape == (C,) and float(ref.abs().min()) > 0
    _note("stats_channel_sums", f"N {N} C {C}", GR.check(got, ref, bnd))


# ---- argument errors: no device needed ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from diff_unet_amos_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "diff_unet_amos_amd", "csrc"), "-j4"], check=True)
    return _native.lib()


def test_glue_entry_points_reject_bad_arguments_without_a_device(lib):
    """Every call below carries exactly one bad argument and must return ERR_ARG before anything is launched."""
    from diff_unet_amos_amd import _native as nv
    E = nv.ERR_ARG
    one, odd = C.c_void_p(256), C.c_void_p(260)            # a 16-byte aligned and a 4-byte aligned non-null address

    def blocks(nblocks=2, cout=(8, 8), w=one, b=one, dw=one, db=one):
        blk = nv.TembBlocks()
        blk.nblocks = nblocks
        for i in range(min(max(nblocks, 0), nv.TEMB_MAX_BLOCKS)):
            blk.cout[i] = cout[i % len(cout)]
            blk.w[i], blk.b[i], blk.dw[i], blk.db[i] = w.value, b.value, dw.value, db.value
        return blk

    null = C.c_void_p(None)
    bad_blocks = [dict(nblocks=0), dict(nblocks=17), dict(cout=(8, 0)), dict(cout=(8, -1)), dict(w=null), dict(w=odd),
                  dict(cout=(4000, 97))]

    def fwd(N=2, t=one, freqs=one, half=4, hid=256, w0=one, b0=one, w1=one, b1=one, blk="ok", add=one, saved=one):
        blk = C.byref(blocks()) if blk == "ok" else blk
        return lib.dua_temb_train_fwd(N, t, freqs, half, hid, w0, b0, w1, b1, blk, add, saved, None)

    def bwd(N=2, half=4, hid=256, w1=one, blk="ok", dadd=one, saved=one, scratch=one, dw0=one, db0=one, dw1=one, db1=one):
        blk = C.byref(blocks()) if blk == "ok" else blk
        return lib.dua_temb_train_bwd(N, half, hid, w1, blk, dadd, saved, scratch, dw0, db0, dw1, db1, None)

    shapes = [dict(N=0), dict(N=-1), dict(N=65), dict(half=0), dict(half=513), dict(hid=0), dict(hid=128), dict(hid=384),
              dict(hid=768), dict(hid=1024)]
    for kw in shapes:
        assert fwd(**kw) == E and bwd(**kw) == E, kw
    for name in ("t", "freqs", "w0", "b0", "w1", "b1", "add", "saved"):
        assert fwd(**{name: None}) == E, name
    for name in ("w1", "dadd", "saved", "scratch", "dw0", "db0", "dw1", "db1"):
        assert bwd(**{name: None}) == E, name
    assert bwd(w1=odd) == E and bwd(scratch=odd) == E
    assert fwd(blk=None) == E and bwd(blk=None) == E
    for kw in bad_blocks:
        assert fwd(blk=C.byref(blocks(**kw))) == E and bwd(blk=C.byref(blocks(**kw))) == E, kw
    assert fwd(blk=C.byref(blocks(b=null))) == E
    assert bwd(blk=C.byref(blocks(dw=null))) == E and bwd(blk=C.byref(blocks(db=null))) == E

    def qs(N=2, per=8, src=one, eps=one, sched=one, T=10, t=one, out=one):
        return lib.dua_q_sample_affine(N, per, src, 2.0, -1.0, eps, sched, T, t, out, None)

    for kw in [dict(N=0), dict(N=65536), dict(per=0), dict(per=-4), dict(T=0), dict(T=-1), dict(src=None), dict(eps=None),
               dict(sched=None), dict(t=None), dict(out=None)]:
        assert qs(**kw) == E, kw

    def sums(N=1, Cc=8, c_pad=64, stats=one, out=one):
        return lib.dua_stats_channel_sums(N, Cc, c_pad, stats, out, None)

    for kw in [dict(N=0), dict(Cc=0), dict(c_pad=7), dict(stats=None), dict(out=None)]:
        assert sums(**kw) == E, kw

    def adam_list(count=2, numel=(5, 5), p=one, g=one, m=one, v=one):
        l = nv.AdamWList()
        l.count = count
        for i in range(min(max(count, 0), nv.ADAMW_MAX_TENSORS)):
            l.numel[i] = numel[i % len(numel)]
            l.p[i], l.g[i], l.m[i], l.v[i] = p.value, g.value, m.value, v.value
        return l

    bad_lists = [dict(count=0), dict(count=-1), dict(count=65), dict(numel=(5, 0)), dict(numel=(5, -3)), dict(g=null)]

    def nonfinite(l="ok", found=one):
        return lib.dua_grads_nonfinite(C.byref(adam_list()) if l == "ok" else l, found, None)

    def adam(l="ok", beta1=0.9, beta2=0.999, eps=1e-8, step=one):
        return lib.dua_adamw_step(C.byref(adam_list()) if l == "ok" else l, 1e-3, None, beta1, beta2, eps, 1e-2, None, None, step, 0,
                                  None)

    assert nonfinite(found=None) == E and nonfinite(l=None) == E and adam(l=None) == E and adam(step=None) == E
    for kw in bad_lists:
        assert nonfinite(l=C.byref(adam_list(**kw))) == E and adam(l=C.byref(adam_list(**kw))) == E, kw
    for name in ("p", "m", "v"):
        assert adam(l=C.byref(adam_list(**{name: null}))) == E, name
    for bad in (1.0, 1.5, -0.1, NAN):
        assert adam(beta1=bad) == E and adam(beta2=bad) == E, bad
    for bad in (-1e-8, NAN):
        assert adam(eps=bad) == E, bad

    def advance(step=one, interval=2):
        return lib.dua_adamw_advance(step, None, None, None, 2.0, 0.5, interval, None, None)

    assert advance(step=None) == E and advance(interval=0) == E and advance(interval=-1) == E
