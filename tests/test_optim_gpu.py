"""The gradient-norm / clip / EMA kernels on the GPU (csrc/train_glue.hip: grads_sumsq, grad_norm_finish, adamw_step_ex) against
the fp64 references and derived bounds of tests/optim_fp64ref.py.  65 tensors (two by-value lists) of sizes 1, 3, 4095, 4096,
4097, 2 * 4096 + 513 and odd small ones live in flat buffers between sentinel words; every case checks EVERY word of those buffers
(a tensor word within its bound, a sentinel word unchanged), with the views 16-byte aligned or 4 bytes off.  The exact quantities
(the overflow flag, skipped steps, the unchanged path, alignment independence, repeatability) are compared for equality.  Figures
are printed before they are asserted (-s shows them).  The last test needs only the shared library."""
import ctypes as C
import itertools
import math
import os
import subprocess

import pytest
import torch

import glue_fp64ref as GR
import optim_fp64ref as OR

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
F32, F64 = torch.float32, torch.float64
NAN = float("nan")
LR, EPS, WD, BETAS = 3e-3, 1e-8, 1e-2, (0.9, 0.999)
LEADS = {"aligned": (0, 0, 0, 0, 0), "offset4B": (1, 1, 1, 1, 1), "e-offset": (0, 0, 0, 0, 1)}


def _ops():
    from diff_unet_amos_amd import ops
    return ops


def _bits(x):
    return x.contiguous().view(torch.int32)


def _same_bits(a, b):
    return bool(torch.equal(_bits(a), _bits(b)))


@pytest.fixture(scope="module")
def case():
    """optim_fp64ref.make_case on the device: pristine flat buffers p, g, m, v, e, work buffers one word longer (the 4-byte
    lead), the mask of tensor words, and the reference's partials of g (computed once)."""
    c = OR.make_case()
    pref, pbnd = OR.partials_ref(OR.views(c["flat"][1], c["starts"]))
    return dict(starts=c["starts"], total=c["total"], mask=c["mask"].to(DEV), pristine=[x.to(DEV) for x in c["flat"]],
                work=[torch.zeros(c["total"] + 4, device=DEV) for _ in range(5)], pref=pref, pbnd=pbnd)


def _views(case, leads, flats=None):
    """Fresh copies of the pristine buffers (or ``flats``) in the work buffers at the given leads: (bases, lists of views)."""
    flats = case["pristine"] if flats is None else flats
    bases = [w[l:l + case["total"]] for w, l in zip(case["work"], leads)]
    for b, src, l in zip(bases, flats, leads):
        b.copy_(src)
        assert b.data_ptr() % 16 == 4 * l
    return bases, [OR.views(b, case["starts"]) for b in bases]


def _guarded_partials(count):
    buf = torch.full((count + 4,), OR.SENT, dtype=F64, device=DEV)
    buf[2:2 + count] = NAN
    return buf, buf[2:2 + count]


def _norm_launch(grads, max_norm, scale, found=None):
    """ops.grad_norm into NaN-filled scalars and guarded partials: (partials, norm, coef) as host / CPU values."""
    ops = _ops()
    count = ops.grad_norm_partials(grads)
    buf, part = _guarded_partials(count)
    norm, coef = torch.full((), NAN, device=DEV), torch.full((), NAN, device=DEV)
    gs = None if scale is None else torch.full((), scale, device=DEV)
    n2, c2 = ops.grad_norm(grads, max_norm, grad_scale=gs, found_inf=found, norm=norm, coef=coef, partials=part)
    assert n2 is norm and c2 is coef
    assert bool((buf[:2] == OR.SENT).all()) and bool((buf[2 + count:] == OR.SENT).all()), "partials: a guard word was written"
    return part.cpu().clone(), norm.cpu().clone(), coef.cpu().clone()


# ---- partials, norm, coefficient ------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("kind", OR.NORM_KINDS)
def test_partials_norm_and_coefficient(case, kind):
    """Every partial, the norm and the coefficient within their bounds, for clip thresholds on both sides of the norm and inf;
    identical bits from the aligned and the 4-byte-offset views and from a second run; the flag unwritten; nothing NaN."""
    flat, scale = OR.make_norm_grads(kind)
    pref, pbnd = OR.partials_ref(OR.views(flat, case["starts"]))
    flat = flat.to(DEV)
    below, at_one = 0, 0
    for max_norm in OR.max_norms(pref, scale):
        r = OR.norm_ref(pref, scale, max_norm)
        runs = []
        for lead in (0, 1, 0):
            base = case["work"][1][lead:lead + case["total"]]
            base.copy_(flat)
            found = torch.zeros((), device=DEV)
            part, norm, coef = _norm_launch(OR.views(base, case["starts"]), max_norm, scale, found)
            assert float(found) == 0.0 and _same_bits(base, flat)
            runs.append((part, norm, coef))
        part, norm, coef = runs[0]
        res = GR.check(part, pref, pbnd)
        print(f"{kind} max_norm {max_norm:.6g}: partials {res}; norm {float(norm):.9g} ref {r['norm']:.9g} bound {r['e_norm']:.3g}; "
              f"coef {float(coef):.9g} ref {r['coef']:.9g} bound {r['e_coef']:.3g}")
        assert res.ratio <= 1.0, res
        assert abs(float(norm) - r["norm"]) <= r["e_norm"] and abs(float(coef) - r["coef"]) <= r["e_coef"]
        assert math.isfinite(float(norm)) and math.isfinite(float(coef)) and bool(torch.isfinite(part).all())
        for other, what in ((runs[1], "4-byte offset"), (runs[2], "second run")):
            assert all(_same_bits(a, b) for a, b in zip(runs[0], other)), what
        below += r["coef"] < 1.0
        at_one += r["coef"] == 1.0 and float(coef) == 1.0
    if kind == "zero":
        assert r["norm"] == 0.0 and float(norm) == 0.0 and float(coef) == 1.0
    else:
        assert below >= 1 and at_one >= 2          # clipped, not clipped, and inf


# ---- the overflow flag --------------------------------------------------------------------------------------------------------------
PLANTS = [(4100, 0), (4100, 4099), (4100, 4095), (4100, 4096), (4100, 4097), (5, 4), (6, 5), (7, 6), (8193, 8192), (4098, 4097),
          (4099, 4098), (70001, 70000)]          # the slots of test_grads_nonfinite_finds_one_planted_value


@gpu
@pytest.mark.parametrize("lead", [0, 1], ids=["aligned", "offset4B"])
@pytest.mark.parametrize("slot", [(0, 64), (63, 64), (64, 65)], ids=["first-of-64", "last-of-64", "first-of-second-list"])
def test_overflow_flag_is_set_exactly_when_grads_nonfinite_sets_it(slot, lead):
    ops = _ops()
    index, count = slot
    g = torch.Generator(device=DEV).manual_seed(7)
    fillers = [torch.randn(17, device=DEV, generator=g) for _ in range(count - 1)]
    norm, coef = torch.zeros((), device=DEV), torch.zeros((), device=DEV)

    def flags(grads):
        a, b = torch.zeros((), device=DEV), torch.zeros((), device=DEV)
        ops.grads_nonfinite(grads, a)
        ops.grad_norm(grads, 1.0, found_inf=b, norm=norm, coef=coef)
        return float(a), float(b)

    for n in sorted({p[0] for p in PLANTS}):
        buf = torch.randn(n + 8, device=DEV, generator=g)
        carrier = buf[lead:lead + n]
        grads = fillers[:index] + [carrier] + fillers[index:]
        assert flags(grads) == (0.0, 0.0), n
        assert math.isfinite(float(norm)) and 0.0 < float(coef) <= 1.0
        for pos in [p[1] for p in PLANTS if p[0] == n]:
            for bad in (float("inf"), float("-inf"), NAN):
                keep = carrier[pos].clone()
                carrier[pos] = bad
                assert flags(grads) == (1.0, 1.0), (n, pos, bad)
                assert float(coef) == 0.0 and not math.isfinite(float(norm))
                carrier[pos] = keep


@gpu
@pytest.mark.parametrize("lead", [0, 1], ids=["aligned", "offset4B"])
def test_overflow_flag_stays_unwritten_on_extreme_finite_values(lead):
    ops = _ops()
    specials = torch.tensor([GR.FLT_MAX, -GR.FLT_MAX, 1e-45, -1e-45, 1e-40, -0.0, 2.0 ** -126, 0.0], device=DEV)
    grads = []
    for i in range(65):
        n = 70001 if i == 64 else (4100 if i == 0 else 5 + i % 4)
        buf = torch.zeros(n + 8, device=DEV)
        t = buf[lead:lead + n]
        t.copy_(specials[torch.arange(n, device=DEV) % specials.numel()])
        grads.append(t)
    a, b = torch.zeros((), device=DEV), torch.full((), 0.25, device=DEV)
    ops.grads_nonfinite(grads, a)
    norm, coef = ops.grad_norm(grads, 1.0, grad_scale=torch.full((), 2.0 ** 40, device=DEV), found_inf=b)
    assert float(a) == 0.0 and float(b) == 0.25          # 0.25: not even rewritten with a zero
    assert math.isfinite(float(norm)) and 0.0 < float(coef) < 1.0


# ---- the step -----------------------------------------------------------------------------------------------------------------------
def _lists(views):
    ops = _ops()
    return ops._adamw_lists(views[0], views[1], views[2], views[3])


@gpu
@pytest.mark.parametrize("leads", ["aligned", "offset4B"])
def test_step_ex_without_clip_and_ema_is_adamw_step(case, leads):
    """dua_adamw_step_ex(clip_coef = NULL, ema = NULL) against dua_adamw_step: the same bits in p, m, v, and in g when stored.
    The entry point forwards to dua_adamw_step in that case, so this shows the delegation (and that nothing else is launched),
    not that adamw_kernel kept its bits when its body became a template: that rests on the instruction-by-instruction comparison
    of the two builds' ISA and on tests/test_glue_fp64.py, which bounds every element of dua_adamw_step as before."""
    from diff_unet_amos_amd import _native as nv
    ops, L = _ops(), nv.lib()
    step = torch.full((), 9, dtype=torch.int32, device=DEV)
    gs = torch.full((), 1024.0, device=DEV)
    for store in (False, True):
        bases, views = _views(case, LEADS[leads])
        ops.adamw_step(*views[:4], step, LR, BETAS, EPS, WD, grad_scale=gs, store_grad=store)
        want = [b.clone() for b in bases[:4]]
        bases, views = _views(case, LEADS[leads])
        for l in _lists(views):
            nv.check(L.dua_adamw_step_ex(C.byref(l), LR, None, BETAS[0], BETAS[1], EPS, WD, nv.ptr(gs), None, nv.ptr(step), int(store),
                                         None, None, 0.0, nv.stream_ptr()), "dua_adamw_step_ex")
        for name, b, w in zip("pgmv", bases, want):
            assert _same_bits(b, w), (name, store)
        assert _same_bits(bases[1], case["pristine"][1]) != store          # g: rewritten exactly when stored


@gpu
@pytest.mark.parametrize("leads", list(LEADS))
@pytest.mark.parametrize("k", [1, 10, 100001])
def test_step_every_element(case, k, leads):
    """One step from step = k - 1 with the coefficient the finish kernel produced: p, m, v, e, and g' when stored, of every
    element within step_bound of step_ref; g untouched when not stored; every sentinel word untouched.  Swept: the EMA rate, a
    clip threshold below and above the norm, the loss scale (None: the null pointer), store_grad."""
    ops = _ops()
    mask, pristine, pref = case["mask"], case["pristine"], case["pref"]
    step = torch.full((), k - 1, dtype=torch.int32, device=DEV)
    found = torch.zeros((), device=DEV)
    tiny = torch.full_like(pristine[0], 1e-300, dtype=F64)
    coefs = set()
    worst = 0.0
    for rate, clip, scale, store in itertools.product((0.99, 0.9999), (0, 1), (None, 1024.0), (False, True)):
        max_norm = OR.max_norms(pref, scale)[clip]
        nr = OR.norm_ref(pref, scale, max_norm)
        inv = 1.0 if scale is None else GR.f32(1.0 / scale)
        w = OR.ema_w(rate)
        a = (k, GR.f32(LR), GR.f32(BETAS[0]), GR.f32(BETAS[1]), GR.f32(EPS), GR.f32(WD), inv)
        ref = OR.step_ref(*pristine, *a, nr["coef"], w)
        bnd = OR.step_bound(*pristine, *a, nr["coef"], nr["e_coef"], w)
        order = (0, 3, 1, 2, 4)                                   # (p, m, v, g', e) -> the buffers' order p, g, m, v, e
        ref = [torch.where(mask, ref[i], x.double()) for i, x in zip(order, pristine)]
        bnd = [torch.where(mask, bnd[i], tiny) for i in order]
        gs = None if scale is None else torch.full((), scale, device=DEV)
        bases, views = _views(case, LEADS[leads])
        norm, coef = ops.grad_norm(views[1], max_norm, grad_scale=gs, found_inf=found)
        assert abs(float(coef) - nr["coef"]) <= nr["e_coef"] and abs(float(norm) - nr["norm"]) <= nr["e_norm"]
        coefs.add(float(coef) < 1.0)
        ops.adamw_step(*views[:4], step, LR, BETAS, EPS, WD, grad_scale=gs, found_inf=found, store_grad=store, clip_coef=coef,
                       ema=views[4], ema_rate=rate)
        res = {n: GR.check(bases[i], ref[i], bnd[i]) for i, n in enumerate("pgmve") if n != "g" or store}
        top = max(res.items(), key=lambda kv: kv[1].ratio)
        worst = max(worst, top[1].ratio)
        what = f"k {k} {leads} rate {rate} coef {float(coef):.6g} scale {scale} store {store}"
        print(f"adamw_step_ex {what}: worst {top[0]} {top[1]}")
        for n, v in res.items():
            assert v.ratio <= 1.0, (what, n, v)
        if not store:
            assert _same_bits(bases[1], pristine[1]), what + ": g"
    assert coefs == {True, False}
    assert int(step) == k - 1 and float(found) == 0.0
    print(f"largest |err| / bound: {worst:.3f}")


@gpu
@pytest.mark.parametrize("leads", list(LEADS))
@pytest.mark.parametrize("option", ["clip", "ema"])
def test_step_every_element_with_one_option(case, option, leads):
    """The two single-option forms of the kernel, every element as above at k = 10: ``clip`` (clip_coef, no EMA: the e buffer is
    not handed over and stays as it was) and ``ema`` (no clip_coef: g' = fl(g inv) exactly, the reference's coefficient is 1
    without an error)."""
    ops = _ops()
    mask, pristine, pref = case["mask"], case["pristine"], case["pref"]
    k = 10
    step = torch.full((), k - 1, dtype=torch.int32, device=DEV)
    tiny = torch.full_like(pristine[0], 1e-300, dtype=F64)
    for rate, scale, store in itertools.product((0.99, 0.9999), (None, 1024.0), (False, True)):
        inv = 1.0 if scale is None else GR.f32(1.0 / scale)
        gs = None if scale is None else torch.full((), scale, device=DEV)
        bases, views = _views(case, LEADS[leads])
        coef, nr = None, dict(coef=1.0, e_coef=0.0)
        if option == "clip":
            max_norm = OR.max_norms(pref, scale)[0]
            nr = OR.norm_ref(pref, scale, max_norm)
            _, coef = ops.grad_norm(views[1], max_norm, grad_scale=gs)
            assert abs(float(coef) - nr["coef"]) <= nr["e_coef"] and float(coef) < 1.0
        w = OR.ema_w(rate)
        a = (k, GR.f32(LR), GR.f32(BETAS[0]), GR.f32(BETAS[1]), GR.f32(EPS), GR.f32(WD), inv)
        ref = OR.step_ref(*pristine, *a, nr["coef"], w)
        bnd = OR.step_bound(*pristine, *a, nr["coef"], nr["e_coef"], w)
        order = (0, 3, 1, 2, 4)
        ref = [torch.where(mask, ref[i], x.double()) for i, x in zip(order, pristine)]
        bnd = [torch.where(mask, bnd[i], tiny) for i in order]
        ops.adamw_step(*views[:4], step, LR, BETAS, EPS, WD, grad_scale=gs, store_grad=store, clip_coef=coef,
                       ema=views[4] if option == "ema" else None, ema_rate=rate if option == "ema" else None)
        names = [n for n in "pgmve" if (n != "g" or store) and (n != "e" or option == "ema")]
        res = {n: GR.check(bases["pgmve".index(n)], ref["pgmve".index(n)], bnd["pgmve".index(n)]) for n in names}
        what = f"{option} only, {leads} rate {rate} scale {scale} store {store}"
        top = max(res.items(), key=lambda kv: kv[1].ratio)
        print(f"adamw_step_ex {what}: worst {top[0]} {top[1]}")
        for n, v in res.items():
            assert v.ratio <= 1.0, (what, n, v)
        if option == "clip":
            assert _same_bits(bases[4], pristine[4]), what + ": e"
        if not store:
            assert _same_bits(bases[1], pristine[1]), what + ": g"
        elif option == "ema":
            assert _same_bits(bases[1], ref[1].float()), what + ": g' = fl(g inv)"


@gpu
@pytest.mark.parametrize("leads", list(LEADS))
@pytest.mark.parametrize("option", ["both", "clip", "ema"])
def test_step_is_skipped_when_an_overflow_was_found(case, leads, option):
    ops = _ops()
    step = torch.full((), 4, dtype=torch.int32, device=DEV)
    found = torch.ones((), device=DEV)
    bases, views = _views(case, LEADS[leads])
    ops.adamw_step(*views[:4], step, LR, BETAS, EPS, WD, grad_scale=torch.full((), 1024.0, device=DEV), found_inf=found,
                   store_grad=True, clip_coef=torch.full((), 0.5, device=DEV) if option != "ema" else None,
                   ema=views[4] if option != "clip" else None, ema_rate=0.99 if option != "clip" else None)
    for b, src in zip(bases, case["pristine"]):
        assert _same_bits(b, src)
    assert float(found) == 1.0 and int(step) == 4


# ---- argument errors: no device needed ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from diff_unet_amos_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "diff_unet_amos_amd", "csrc"), "-j4"], check=True)
    return _native.lib()


def test_optimizer_entry_points_reject_bad_arguments_without_a_device(lib):
    """Every call below carries exactly one bad argument and must return ERR_ARG before anything is launched."""
    from diff_unet_amos_amd import _native as nv
    E = nv.ERR_ARG
    one, null = C.c_void_p(256), C.c_void_p(None)

    def adam_list(count=2, numel=(5, 5), p=one, g=one, m=one, v=one):
        l = nv.AdamWList()
        l.count = count
        for i in range(min(max(count, 0), nv.ADAMW_MAX_TENSORS)):
            l.numel[i] = numel[i % len(numel)]
            l.p[i], l.g[i], l.m[i], l.v[i] = p.value, g.value, m.value, v.value
        return l

    def ema_list(count=2, hole=None):
        e = nv.AdamWEma()
        for i in range(count):
            e.e[i] = None if i == hole else one.value
        return e

    bad_lists = [dict(count=0), dict(count=-1), dict(count=65), dict(numel=(5, 0)), dict(numel=(5, -3)), dict(g=null)]
    assert lib.dua_adamw_blocks(C.byref(adam_list())) == 2
    assert lib.dua_adamw_blocks(C.byref(adam_list(numel=(4096, 4097)))) == 3
    assert lib.dua_adamw_blocks(None) < 0

    def sumsq(l="ok", partials=one):
        return lib.dua_grads_sumsq(C.byref(adam_list()) if l == "ok" else l, partials, None)

    assert sumsq(l=None) == E and sumsq(partials=None) == E
    for kw in bad_lists:
        assert sumsq(l=C.byref(adam_list(**kw))) == E and lib.dua_adamw_blocks(C.byref(adam_list(**kw))) < 0, kw

    def finish(partials=one, count=3, max_norm=1.0, norm=one, coef=one):
        return lib.dua_grad_norm_finish(partials, count, None, max_norm, norm, coef, None, None)

    for kw in [dict(partials=None), dict(norm=None), dict(coef=None), dict(count=0), dict(count=-1), dict(max_norm=0.0),
               dict(max_norm=-1.0), dict(max_norm=NAN)]:
        assert finish(**kw) == E, kw

    def step_ex(l="ok", beta1=0.9, beta2=0.999, eps=1e-8, step=one, clip=one, ema="ok", w=0.01):
        ema = C.byref(ema_list()) if ema == "ok" else ema
        return lib.dua_adamw_step_ex(C.byref(adam_list()) if l == "ok" else l, 1e-3, None, beta1, beta2, eps, 1e-2, None, None, step,
                                     0, clip, ema, w, None)

    assert step_ex(l=None) == E and step_ex(step=None) == E and step_ex(l=None, clip=None, ema=None) == E
    for kw in bad_lists:
        assert step_ex(l=C.byref(adam_list(**kw))) == E, kw
    for name in ("p", "m", "v"):
        assert step_ex(l=C.byref(adam_list(**{name: null}))) == E, name
    for bad in (1.0, 1.5, -0.1, NAN):
        assert step_ex(beta1=bad) == E and step_ex(beta2=bad) == E, bad
    for bad in (-1e-8, NAN):
        assert step_ex(eps=bad) == E, bad
    for hole in (0, 1):
        assert step_ex(ema=C.byref(ema_list(hole=hole))) == E and step_ex(ema=C.byref(ema_list(hole=hole)), clip=None) == E, hole
    for bad in (0.0, -0.01, 1.0000001, 2.0, NAN):
        assert step_ex(w=bad) == E and step_ex(w=bad, clip=None) == E, bad
