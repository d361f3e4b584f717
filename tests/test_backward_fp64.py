"""Every backward kernel of the training step and each of its launch forms, at the geometry training runs it at, against an fp64
reference on the exact operands it read (tests/fp64ref.py), element by element within a bound derived from the launcher's own
arithmetic: the 3x3x3 weight gradient (fetch-once form with its two reduce routes and partition multipliers, the three-kd forms
with and without partial sums, fp32), the data gradient as training._dgrad launches it and the norm-backward-sums launch, the
InstanceNorm + LeakyReLU backward pair, the head backward and the max-pool backward.  Each case also pins the form it exercises
(partition count, reduce route, workspace size, kernel kind), so a launcher change that moves it fails here instead of quietly
testing another kernel."""
import ctypes

import pytest
import torch

import fp64ref as R

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
F16, F32 = torch.float16, torch.float32


def _ops():
    from diff_unet_amos_amd import ops
    return ops


def _nv():
    from diff_unet_amos_amd import _native as nv
    return nv


def _randn(shape, seed, dtype, scale=1.0, shift=0.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randn(shape, generator=g, device=DEV) * scale + shift).to(dtype)


# ---- weight gradient ------------------------------------------------------------------------------------------------------------
# geometry: (N, D, H, W, x channels, cin_off, cin, dy channels, cout_off, cout, cin_src, perm?)
GEOS = {
    "first24": (2, 96, 96, 96, 24, 0, 24, 64, 0, 64, 17, False),      # the denoiser's first conv: 17 channels packed into 24
    "first24perm": (2, 96, 96, 96, 24, 0, 24, 64, 0, 64, 17, True),   # ... with a channel map
    "c64": (2, 96, 96, 96, 64, 0, 64, 64, 0, 64, 64, False),
    "cat128": (2, 96, 96, 96, 128, 0, 128, 64, 0, 64, 128, False),    # UpCat's conv over the 128-wide concat
    "l12": (2, 12, 12, 12, 512, 0, 512, 256, 0, 256, 512, False),     # 64 slabs: the tap-gathering reduce
    "l6": (2, 6, 6, 6, 512, 0, 512, 512, 0, 512, 512, False),         # 128 slabs
    "odd": (2, 63, 48, 40, 64, 0, 64, 64, 0, 64, 64, False),          # the odd-extent plan's level 0
    "slices": (2, 48, 48, 48, 88, 8, 72, 160, 16, 136, 72, False),    # channel offsets, strides, ragged slab and co tile
}
THREE_KD = 256

# (geometry, dtype, policy, workspace: "full" / "short", the regime the case must be in)
CASES = [
    ("first24", F16, 0, "full", "fo-plain"),
    ("first24", F16, 16, "full", "fo-plain ragged"),          # P = 2048 over 6912 tiles: multiple of 8, ragged last round
    ("first24perm", F16, 0, "full", "fo-plain"),
    ("c64", F16, 0, "full", "fo-plain"),
    ("c64", F16, 4, "full", "fo-plain"),
    ("c64", F16, 8, "full", "fo-plain ragged"),               # P = 512 over 6912 tiles
    ("cat128", F16, 0, "full", "fo-plain"),
    ("l12", F16, 0, "full", "fo-taps small"),                 # P = 4 < 8
    ("l12", F16, 4, "full", "fo-taps"),
    ("l6", F16, 0, "full", "fo-taps small"),                  # P = 2
    ("l6", F16, 8, "full", "fo-taps clamped"),                # 1024 / 128 = 8 partitions asked, 4 tiles
    ("odd", F16, 0, "full", "fo-plain ragged"),               # P = 128 over 960 tiles, 480 per sample
    ("slices", F16, 0, "full", "fo-plain"),
    ("slices", F16, THREE_KD, "full", "3kd-part"),
] + [("c64", F16, THREE_KD | v, ws, f"3kd-{'part' if ws == 'full' else 'atomic'}")
     for v in (0, 128, 64, 32, 1) for ws in ("full", "short")] + [
    ("l12", F16, THREE_KD, "full", "3kd-part"),
    ("c64", F32, 0, "full", "3kd-part"),
    ("c64", F32, 0, "short", "3kd-atomic"),
    ("odd", F32, 0, "full", "3kd-part"),
]

_CACHE = {}


def _operands(geo, dtype):
    """Inputs, starting dW and the fp64 reference of one geometry (the cases of a geometry are consecutive: one entry kept)."""
    key = (geo, dtype)
    if key not in _CACHE:
        _CACHE.clear()
        torch.cuda.empty_cache()
        N, D, H, W, cx, co_x, cin, cy, co_y, cout, cin_src, use_perm = GEOS[geo]
        seed = sum(map(ord, geo))
        x = _randn((N, D, H, W, cx), seed, dtype)
        dy = _randn((N, D, H, W, cy), seed + 1, dtype)
        perm = None
        if use_perm:       # packed j < 16: source j + 1; packed 16: source 0 (the image); the rest padding
            perm = torch.full((-(-cin // 64) * 64,), -1, dtype=torch.int32, device=DEV)
            perm[:16] = torch.arange(1, 17, dtype=torch.int32)
            perm[16] = 0
        dw0 = _randn((cout, cin_src, 3, 3, 3), seed + 2, F32)
        ref, ab = R.wgrad_ref(x, co_x, cin, dy, co_y, cout, cin_src=cin_src, perm=perm)
        _CACHE[key] = (x, dy, perm, dw0, ref, ab)
    return _CACHE[key]


def _wgrad_ws(geo, dtype, policy):
    nv = _nv()
    N, D, H, W, cx, co_x, cin, cy, co_y, cout, _, _ = GEOS[geo]
    d = nv.Conv3Desc(nv.dt_code(dtype), N, D, H, W, cin, cx, co_x, cout, cy, co_y, 0, 0, 0, policy)
    return int(nv.lib().dua_conv3d_k3_wgrad_workspace(ctypes.byref(d)))


def _form(geo, dtype, policy, ws_mode, perm):
    """(form name, P, chain, workspace bytes the launcher asks for) from the mirrors of the launchers."""
    N, D, H, W, _, _, cin, _, _, cout, _, _ = GEOS[geo]
    if dtype == F16 and not policy & THREE_KD:
        P, combos, total = R.wgrad_fo_partitions(N, D, H, W, cin, cout, policy)
        route = R.wgrad_fo_route(combos, perm)
        return dict(name=f"fo-{route}", P=P, total=total, chain=R.wgrad_fo_chain(P, total, route),
                    ws=P * combos * 27 * 2048 * 4)
    P, combos, total = R.wgrad_3kd_partitions(N, D, H, W, cin, cout, policy)
    need = R.wgrad_3kd_workspace(P, combos)
    partials = ws_mode == "full" and P > 1
    return dict(name=f"3kd-{'part' if partials else 'atomic'}", P=P, total=total,
                chain=R.wgrad_3kd_chain(P, total, dtype, partials), ws=need)


@pytest.mark.parametrize("geo,dtype,policy,ws_mode,regime", CASES,
                         ids=[f"{c[0]}-{'f16' if c[1] == F16 else 'f32'}-p{c[2]}-{c[3]}-{c[4].replace(' ', '-')}" for c in CASES])
def test_conv3_wgrad_within_fp64_bound(geo, dtype, policy, ws_mode, regime):
    ops = _ops()
    N, D, H, W, cx, co_x, cin, cy, co_y, cout, cin_src, _ = GEOS[geo]
    x, dy, perm, dw0, ref, ab = _operands(geo, dtype)
    form = _form(geo, dtype, policy, ws_mode, perm)
    # the form: the route, the workspace the C++ sizes (pins the Python mirror of the partition count), the regime
    assert regime.split()[0] == form["name"], (regime, form)
    assert _wgrad_ws(geo, dtype, policy) == form["ws"], "partition mirror drifted from the launcher"
    P, total = form["P"], form["total"]
    if "ragged" in regime:
        assert P % 8 == 0 and total % P != 0
    if "small" in regime:
        assert P < 8 and P % 8 != 0 and P < total
    if "clamped" in regime:
        combos = R.wgrad_fo_partitions(N, D, H, W, cin, cout, policy)[1]
        assert P == total and -(-256 * (((policy & 31) >> 1) or 1) // combos) > total
    elif form["name"].startswith("fo"):
        assert N > 1 and P <= total // N          # every partition's walk runs from the first sample into the last
    if ws_mode == "full":
        ws = torch.empty(max(form["ws"], 16), dtype=torch.uint8, device=DEV)
    else:                  # too small: launch_wgrad drops the partials and the workgroups add into dW themselves
        assert form["ws"] > 16
        ws = torch.empty(16, dtype=torch.uint8, device=DEV)
    dw = dw0.clone()
    ops.WGRAD_POLICY = policy
    try:
        ops.conv3d_k3_wgrad(x, cin, co_x, dy, cout, co_y, dw, perm=perm, workspace=ws)
    finally:
        ops.WGRAD_POLICY = 0
    torch.cuda.synchronize()
    bnd = R.wgrad_bound(ref, ab, dw0, form["chain"])
    res = R.check(dw.double(), dw0.double() + ref, bnd)
    print(f"wgrad {geo} {dtype} policy {policy} {form['name']} P={P} tiles={total}: {res}")
    assert res.ratio <= 1.0, res


def test_wgrad_cases_cover_every_regime():
    """The case list above reaches every partition regime of the fetch-once launcher (a multiple of 8 with a ragged last round,
    fewer than 8 and no multiple of 8, clamped to the tile count) and every reduce route."""
    regimes = {r.split()[1] for (_, _, _, _, r) in CASES if len(r.split()) > 1}
    assert {"ragged", "small", "clamped"} <= regimes
    routes = {r.split()[0] for (_, _, _, _, r) in CASES}
    assert routes == {"fo-plain", "fo-taps", "3kd-part", "3kd-atomic"}


# ---- data gradient --------------------------------------------------------------------------------------------------------------
# (N, S, forward cin, forward cout) of the 96^3 plan's levels; the data gradient maps dy [.., cout] -> dx [.., cin]
# launch -> (dua_conv3d_k3_kernel_kind, split-K), as the launcher decides today (0 = v2, 2 = the wide-tile form)
DGRAD_KIND = {(96, 64, 64): (2, False), (48, 64, 64): (0, False), (24, 128, 128): (0, False), (12, 256, 256): (0, False),
              (6, 512, 512): (0, True), (96, 64, 128): (2, False)}
DGRAD_LEVELS = [(2, 96, 64, 64), (2, 48, 64, 64), (2, 24, 128, 128), (2, 12, 256, 256), (2, 6, 512, 512), (2, 96, 128, 64)]


@pytest.mark.parametrize("N,S,cin_f,cout_f", DGRAD_LEVELS, ids=[f"{s}^3-{a}to{b}" for (_, s, a, b) in DGRAD_LEVELS])
def test_conv3_dgrad_launch_within_fp64_bound(N, S, cin_f, cout_f):
    """training._dgrad: pack_conv3_weights_dgrad, then conv3d_k3 on dy with ops.splitk_ws; reference = the forward reference on
    w.flip(2, 3, 4).transpose(0, 1) rounded to fp16, the split-K partials the finish kernel adds counted in the chain."""
    ops, nv = _ops(), _nv()
    dt = F16
    dy = _randn((N, S, S, S, cout_f), S + cin_f, dt)
    w = _randn((cout_f, cin_f, 3, 3, 3), S + cout_f, F32, scale=(27 * cout_f) ** -0.5)
    wp, bp = ops.pack_conv3_weights_dgrad(w, dt, cout_packed=cout_f)
    ws = ops.splitk_ws(dt, N, S, S, S, cout_f, cin_f, DEV)
    d = nv.Conv3Desc(nv.dt_code(dt), N, S, S, S, cout_f, cout_f, 0, cin_f, cin_f, 0, 0, 0, 0, ops.CONV_POLICY)
    ws_bytes = 0 if ws is None else ws.numel() * ws.element_size()
    split = ops.conv3_form(d, False, ws_bytes).ksplit > 1                          # the launcher's own answer for this call
    kind = int(nv.lib().dua_conv3d_k3_kernel_kind(ctypes.byref(d), 0, 1 if split else 0))
    assert (kind, split) == DGRAD_KIND[(S, cout_f, cin_f)], (kind, split)
    dx = torch.empty((N, S, S, S, cin_f), dtype=dt, device=DEV)
    ops.conv3d_k3(dy, cout_f, 0, wp, bp, cin_f, dx, 0, ops.stats_buffer(N, cin_f, DEV), workspace=ws)
    torch.cuda.synchronize()
    pts = R.sample_voxels(N, (S, S, S), n_random=3000, seed=S)
    A, _ = R.gather_taps(dy, pts, 0, cout_f)
    wd = w.flip(2, 3, 4).transpose(0, 1).contiguous()
    ref, ab, sq = R.conv3_ref(A, R.conv3_weights(wd, dt), torch.zeros(cin_f))
    parts = 3 * -(-cout_f // ops.chunk_elems(dt)) if split else 0
    bnd = R.bound(ref, ab, sq, R.chain_length(27 * cout_f, dt, parts), dt)
    res = R.check(R.gather_points(dx, pts, 0, cin_f), ref, bnd, pts)
    print(f"dgrad {S}^3 {cout_f}->{cin_f} kind {kind} split {split}: {res}")
    assert res.ratio <= 1.0, res


# ---- InstanceNorm + LeakyReLU backward ------------------------------------------------------------------------------------------
def _norm_case(N, S, C, seed, shift=0.3):
    ops = _ops()
    raw = _randn((N, S, S, S, C), seed, F16, scale=1.5, shift=shift)
    g = torch.Generator(device=DEV).manual_seed(seed + 1)
    gamma = torch.rand(C, generator=g, device=DEV) + 0.5
    beta = torch.randn(C, generator=g, device=DEV) * 0.2
    add = torch.randn(N, C, generator=g, device=DEV)
    rd = raw.double()
    stats = ops.stats_encode(torch.stack([rd.sum((1, 2, 3)), (rd * rd).sum((1, 2, 3))], -1))
    norm = ops.Norm(stats, gamma, beta, S ** 3, add=add, add_stride=C)
    return raw, gamma, beta, stats, norm


def _check_in_bwd(tag, dA_vals, raw, gamma, beta, stats, sums, dY, grads, chain, want_add):
    """sums (the kernel's fp64 replica rows) against S0..S2, dY against the reference within in_bwd_dy_bound, the parameter
    gradients against theirs."""
    ops = _ops()
    N, C = raw.shape[0], raw.shape[-1]
    V = raw.shape[1] * raw.shape[2] * raw.shape[3]
    r = R.in_bwd_ref(dA_vals.reshape(N, V, C), raw.reshape(N, V, C), ops.stats_decode(stats), gamma, beta, V)
    b0, b1, b2 = R.in_bwd_sums_bound(r, chain)
    got = sums.sum(1)[:, :C, :3]
    out = []
    for j, (ref, b) in enumerate(((r["S0"], b0), (r["S1"], b1), (r["S2"], b2))):
        res = R.check(got[..., j], ref, b)
        out.append(res)
        assert res.ratio <= 1.0, (tag, f"S{j}", res)
    near = r["near"]
    assert near.double().mean().item() < 1e-4, near.double().mean().item()
    bd = R.in_bwd_dy_bound(r, b1, b2, raw.dtype)
    res = R.check(dY.reshape(N, V, C), r["dY"], bd)
    assert res.ratio <= 1.0, (tag, "dY", res)
    out.append(res)
    dgamma, dbeta, dadd = grads
    # the apply launch rounds the kernel's fp64 sums to fp32 (dadd: per sample) and adds the samples with fp32 atomics
    rb = R.check(dbeta, r["S1"].sum(0), (b1 + R.U32 * r["S1"].abs()).sum(0) * (1 + N * R.U32)
                 + N * R.U32 * r["S1"].abs().sum(0) + R.FLOOR32)
    rg = R.check(dgamma, r["S2"].sum(0), (b2 + R.U32 * r["S2"].abs()).sum(0) * (1 + N * R.U32)
                 + N * R.U32 * r["S2"].abs().sum(0) + R.FLOOR32)
    assert rb.ratio <= 1.0 and rg.ratio <= 1.0, (tag, rb, rg)
    if want_add:
        ra = R.check(dadd, r["S0"], b0 + R.U32 * r["S0"].abs() + R.FLOOR32)
        assert ra.ratio <= 1.0, (tag, "dadd", ra)
        out.append(ra)
    print(f"instnorm bwd {tag}: S0 {out[0].ratio:.3g} S1 {out[1].ratio:.3g} S2 {out[2].ratio:.3g} dY {out[3].ratio:.3g} "
          f"dbeta {rb.ratio:.3g} dgamma {rg.ratio:.3g} near-kink {near.double().mean().item():.2e}")


@pytest.mark.parametrize("layout", ["dense", "concat-half"])
@pytest.mark.parametrize("want_add", [True, False])
@pytest.mark.parametrize("shift", [0.3, 40.0], ids=["mean-small", "mean-far"])
def test_instnorm_backward_within_fp64_bound(layout, want_add, shift):
    """96^3, batch 2, 64 channels; dA contiguous or read in place from one half of a 128-wide concat gradient (offset 64,
    stride 128, as _slice_of hands it over); sums from the reduce launch."""
    ops, nv = _ops(), _nv()
    N, S, C = 2, 96, 64
    raw, gamma, beta, stats, norm = _norm_case(N, S, C, 11 + int(shift), shift)
    if layout == "dense":
        dbuf, off = _randn((N, S, S, S, C), 21, F16), 0
    else:
        dbuf, off = _randn((N, S, S, S, 2 * C), 22, F16), C
    dA_vals = dbuf[..., off:off + C]
    V = S ** 3
    d = nv.NormBwdDesc(nv.dt_code(F16), N, V, C, dbuf.shape[-1], off, C, 0, C, 0)
    sums = ops.instnorm_bwd_sums(raw, norm)
    nv.check(nv.lib().dua_instnorm_bwd_reduce(ctypes.byref(d), nv.ptr(dbuf), nv.ptr(raw), norm.ref(N, C), nv.ptr(sums),
                                              nv.stream_ptr()), "dua_instnorm_bwd_reduce")
    dY = torch.empty_like(raw)
    grads = ops.instnorm_bwd(dbuf, off, raw, C, norm, dY, want_add=want_add, sums=sums)
    torch.cuda.synchronize()
    assert (grads[2] is None) == (not want_add)
    _check_in_bwd(f"{layout} add={want_add} shift={shift}", dA_vals, raw, gamma, beta, stats, sums, dY, grads,
                  R.in_bwd_reduce_chain(C, V, F16), want_add)


@pytest.mark.parametrize("cin", [64, 128])
def test_dgrad_reduce_within_fp64_bound(cin):
    """conv3d_k3_dgrad_reduce at 96^3, batch 2: dx against fp64 (the forward reference on the flipped, transposed fp16 weights),
    its norm-backward sums against fp64 sums of its own dx, and the apply pass on them."""
    ops = _ops()
    N, S, C = 2, 96, 64
    dt = F16
    dy = _randn((N, S, S, S, cin), 31 + cin, dt, scale=0.5)
    w = _randn((cin, C, 3, 3, 3), 32 + cin, F32, scale=(27 * cin) ** -0.5)
    raw, gamma, beta, stats, norm = _norm_case(N, S, C, 33 + cin)
    assert ops.conv3d_k3_dgrad_reduce_supported(dt, N, S, S, S, cin, C)
    wp, bp = ops.pack_conv3_weights_dgrad(w, dt, cout_packed=cin)
    dx = torch.empty((N, S, S, S, C), dtype=dt, device=DEV)
    sums = ops.instnorm_bwd_sums(raw, norm)
    ops.conv3d_k3_dgrad_reduce(dy, cin, wp, bp, C, dx, raw, norm, sums)
    torch.cuda.synchronize()
    pts = R.sample_voxels(N, (S, S, S), n_random=3000, seed=cin)
    A, _ = R.gather_taps(dy, pts, 0, cin)
    ref, ab, sq = R.conv3_ref(A, R.conv3_weights(w.flip(2, 3, 4).transpose(0, 1).contiguous(), dt), torch.zeros(C))
    res = R.check(R.gather_points(dx, pts, 0, C), ref, R.bound(ref, ab, sq, R.chain_length(27 * cin, dt), dt), pts)
    print(f"dgrad_reduce {cin}->{C} dx: {res}")
    assert res.ratio <= 1.0, res
    dY = torch.empty_like(raw)
    grads = ops.instnorm_bwd(dx, 0, raw, C, norm, dY, want_add=True, sums=sums)
    torch.cuda.synchronize()
    _check_in_bwd(f"dgrad_reduce {cin}", dx, raw, gamma, beta, stats, sums, dY, grads, R.DGRAD_REDUCE_CHAIN, True)


# ---- head and max-pool backward ---------------------------------------------------------------------------------------------------
def _check_head_bwd(u, dl, w, du, dW, db, mfma, nominal=False):
    """du, dW, db of ops.head_bwd against fp64 on the operands it read; ``mfma``: the launch took the MFMA path (fp16 weights);
    ``nominal``: with the bound's term for subnormal fp16 operands (the three contractions are MFMA ones; db multiplies by ones)."""
    dtype = u.dtype
    C, K = u.shape[-1], dl.shape[-1]
    V = u.numel() // C
    c_du, c_w = R.head_bwd_chains(V, dtype, mfma=mfma)
    ud, dld = u.double().reshape(V, C), dl.double().reshape(V, K)
    wq = (w.half() if mfma else w).double()                  # the MFMA path multiplies fp16 weights
    ref_du = dld @ wq
    b_du = R.bound(ref_du, dld.abs() @ wq.abs(), None, c_du, dtype, nominal=R.nominal_sum(dld, wq) if nominal else None)
    ref_w, ab_w = dld.t() @ ud, dld.abs().t() @ ud.abs()
    b_w = R.U32 * c_w * ab_w * (1 + R.U32) + R.FLOOR32
    ref_b, ab_b = dld.sum(0), dld.abs().sum(0)
    b_b = R.U32 * c_w * ab_b * (1 + R.U32) + R.FLOOR32
    if nominal:
        assert mfma
        t_w = R.subnormal_term(R.nominal_sum(dld.t(), ud)) * (1 + R.U32)
        t_b = R.subnormal_term(R.nominal_sum(dld.t(), torch.ones_like(ud[:, :1]))[:, 0]) * (1 + R.U32)
        print(f"head bwd: the subnormal term is {_share(R.subnormal_term(R.nominal_sum(dld, wq)), b_du)} of du's bound, "
              f"{_share(t_w, b_w + t_w)} of dW's, {_share(t_b, b_b + t_b)} of db's")
        b_w, b_b = b_w + t_w, b_b + t_b
    r1 = R.check(du.reshape(V, C), ref_du, b_du)
    r2 = R.check(dW, ref_w, b_w)
    r3 = R.check(db, ref_b, b_b)
    print(f"head bwd {dtype}: du {r1}; dW {r2}; db {r3}")
    assert max(r1.ratio, r2.ratio, r3.ratio) <= 1.0, (r1, r2, r3)


@pytest.mark.parametrize("dtype", [F16, F32])
def test_head_backward_within_fp64_bound(dtype):
    """96^3, batch 2, C = 64, K = 16: fp16 takes the MFMA path and head_reduce_kernel, fp32 the plain kernel and the same reduce."""
    ops = _ops()
    N, S, C, K = 2, 96, 64, 16
    u = _randn((N, S, S, S, C), 41, dtype)
    dl = _randn((N, S, S, S, K), 42, dtype)
    w = _randn((K, C), 43, F32, scale=0.2)
    du, dW, db = ops.head_bwd(dl, u, w)
    torch.cuda.synchronize()
    _check_head_bwd(u, dl, w, du, dW, db, mfma=dtype == F16)


@pytest.mark.parametrize("dtype", [F16, F32])
def test_maxpool_backward_within_fp64_bound(dtype):
    """96^3, batch 2, many ties: out = dA + dP routed to the first maximum of each 2x2x2 block, one rounding of that sum."""
    ops = _ops()
    N, S, C = 2, 96, 64
    g = torch.Generator(device=DEV).manual_seed(51)
    act = (torch.randint(-3, 4, (N, S, S, S, C + 8), generator=g, device=DEV).float() * 0.5).to(dtype)
    dA = _randn((N, S, S, S, C + 16), 52, dtype)
    dP = _randn((N, S // 2, S // 2, S // 2, C), 53, dtype)
    out = ops.maxpool2_bwd_add(act, 8, C, dA, 16, dP)
    torch.cuda.synchronize()
    h = S // 2
    a = act[..., 8:8 + C].reshape(N, h, 2, h, 2, h, 2, C).permute(0, 1, 3, 5, 2, 4, 6, 7).reshape(N, h, h, h, 8, C)
    first = a.double().argmax(4)                              # torch's rule: the first maximum in (d, h, w) raster order
    routed = torch.zeros((N, h, h, h, 8, C), dtype=torch.float64, device=DEV)
    routed.scatter_(4, first.unsqueeze(4), dP.double().unsqueeze(4))
    routed = routed.reshape(N, h, h, h, 2, 2, 2, C).permute(0, 1, 4, 2, 5, 3, 6, 7).reshape(N, S, S, S, C)
    ref = routed + dA[..., 16:16 + C].double()
    u_out, floor = R.unit(dtype)
    ties = (a == a.max(4, keepdim=True).values).sum(4) > 1
    assert ties.double().mean().item() > 0.1
    res = R.check(out, ref, u_out * ref.abs() + floor)
    print(f"maxpool bwd {dtype}: {res}")
    assert res.ratio <= 1.0, res


# ---- transposed convolution backward ----------------------------------------------------------------------------------------------
# (coarse dims, fine dims, Cin, Cout, concat skip channels): every level transition of the 96^3 plan and of the 63x48x40 plan
DECONV_LEVELS = [((6, 6, 6), (12, 12, 12), 512, 256, 256), ((12, 12, 12), (24, 24, 24), 256, 128, 128),
                 ((24, 24, 24), (48, 48, 48), 128, 64, 64), ((48, 48, 48), (96, 96, 96), 64, 64, 64),
                 ((3, 3, 2), (7, 6, 5), 512, 256, 256), ((7, 6, 5), (15, 12, 10), 256, 128, 128),
                 ((15, 12, 10), (31, 24, 20), 128, 64, 64), ((31, 24, 20), (63, 48, 40), 64, 64, 64)]


@pytest.mark.parametrize("dims,fine,cin,cout,cskip", DECONV_LEVELS,
                         ids=[f"{'x'.join(map(str, c[0]))}-{c[2]}to{c[3]}" for c in DECONV_LEVELS])
def test_deconv_backward_within_fp64_bound(dims, fine, cin, cout, cskip):
    """deconv_k2s2_bwd, batch 2, fp16: dy read in place from the upsampled half of the concat gradient; the padded form where the
    fine level is one plane longer than 2x the coarse one (its folded dy operand is summed and rounded once: an emulated input,
    covered by the RSS term as the forward's fused transforms are)."""
    ops = _ops()
    x, dcat, w = _deconv_bwd_operands(dims, fine, cin, cout, cskip)
    dx, dw = ops.deconv_k2s2_bwd(x, cin, 8, dcat, cout, cskip, w)
    torch.cuda.synchronize()
    _check_deconv_bwd(dims, fine, cin, cout, cskip, x, dcat, w, dx, dw)


def _deconv_bwd_operands(dims, fine, cin, cout, cskip, N=2, dt=F16):
    """(x with 8 channels in front, the concat gradient whose upsampled half is dy, w) of one DECONV_LEVELS entry."""
    D, H, W = dims
    seed = sum(dims) + cin
    x = _randn((N, D, H, W, cin + 8), seed, dt)
    dcat = _randn((N, *fine, cskip + cout), seed + 1, dt)
    w = _randn((cin, cout, 2, 2, 2), seed + 2, F32, scale=cin ** -0.5)
    return x, dcat, w


def _check_deconv_bwd(dims, fine, cin, cout, cskip, x, dcat, w, dx, dw, N=2, dt=F16, nominal=False):
    """``nominal``: with the bound's term for subnormal fp16 operands on both contractions"""
    nv = _nv()
    D, H, W = dims
    padded = tuple(fine) != (2 * D, 2 * H, 2 * W)
    c_dx, c_dw, P = R.deconv_bwd_chains(N, D, H, W, cin, cout, dt)
    d = nv.Conv3Desc(nv.dt_code(dt), N, D, H, W, cin, cin + 8, 8, cout, cskip + cout, cskip)
    combos = -(-cin // 64) * -(-cout // 64)
    assert int(nv.lib().dua_deconv_k2s2_bwd_workspace(ctypes.byref(d))) == P * combos * 8 * 4096 * 4   # pins the mirror of P
    dyf = R.deconv_fold_dy(dcat[..., cskip:], D, H, W)
    xs = x[..., 8:8 + cin]
    ref, ab, sq, rw, aw = R.deconv_bwd_ref(xs, dyf, w, dt)
    ndx, ndw = R.deconv_bwd_nominal(xs, dyf, w, padded) if nominal else (None, None)
    b1 = R.bound(ref, ab, sq, c_dx, dt, emulated_in=dt if padded else None, nominal=ndx)
    r1 = R.check(dx, ref, b1)
    b2 = R.U32 * c_dw * aw * (1 + R.U32) + R.FLOOR32
    if padded:
        A2 = (dyf * dyf).reshape(N, D, 2, H, 2, W, 2, cout).permute(0, 1, 3, 5, 2, 4, 6, 7).reshape(-1, 8 * cout)
        ssq = ((xs.double().reshape(-1, cin) ** 2).t() @ A2).reshape(cin, 2, 2, 2, cout).permute(0, 4, 1, 2, 3).contiguous()
        b2 = b2 + R.C_RSS * R.U16 * ssq.sqrt()
    if nominal:
        b2 = b2 + R.subnormal_term(ndw) * (1 + R.U32)
        print(f"deconv bwd: the subnormal term is {_share(R.subnormal_term(ndx), b1)} of dx's bound, {_share(R.subnormal_term(ndw), b2)} of dw's")
    r2 = R.check(dw, rw, b2)
    print(f"deconv bwd {dims}->{fine} {cin}->{cout} P={P}{' padded' if padded else ''}: dx {r1}; dw {r2}")
    assert r1.ratio <= 1.0 and r2.ratio <= 1.0, (r1, r2)


# ---- fp16 operands below the normal range -------------------------------------------------------------------------------------------
# What a step at the trainer's initial loss scale feeds the backward kernels: gradient operands that straddle 2^-14, lie below it
# throughout, or are a few subnormal ulps (fp64ref.subnormal_regime), the other operand O(1) as above.  The bounds are the ones
# above plus fp64ref's term for subnormal operands, derived from the matrix-instruction model that tests/test_mfma_model_gpu.py holds
# on the instruction; every element is compared, and the floor of half a subnormal ulp in the bound of an fp16 output makes a
# flushed OUTPUT fail as well.
def _share(term, bnd):
    return f"{float((term / bnd).mean()):.2f}"


def _gradient(shape, regime, seed):
    """the gradient operand of a regime on the device; its subnormal share is asserted before anything is launched"""
    t, want = R.subnormal_regime(shape, regime, seed, DEV)
    got = R.subnormal_share(t)
    assert abs(got - want) < 0.02, (regime, got, want)
    return t


GEOS.update({"sub4": (1, 4, 4, 4, 512, 0, 512, 512, 0, 512, 512, False),       # the deepest level of a 64^3 step: the taps route
             "sub2": (1, 2, 2, 2, 512, 0, 512, 512, 0, 512, 512, False),
             "subragged": (2, 6, 5, 7, 40, 0, 40, 72, 0, 72, 40, False)})      # the plain route, every tile ragged
SUB_WGRAD = [("sub4", 0, "full", "fo-taps"), ("sub2", 0, "full", "fo-taps"), ("subragged", 0, "full", "fo-plain"),
             ("l12", THREE_KD, "full", "3kd-part"), ("l12", THREE_KD, "short", "3kd-atomic")]
_SUB_CACHE = {}


def _sub_wgrad_operands(geo, regime):
    key = (geo, regime)
    if key not in _SUB_CACHE:
        _SUB_CACHE.clear()
        N, D, H, W, cx, co_x, cin, cy, co_y, cout, cin_src, _ = GEOS[geo]
        seed = sum(map(ord, geo + regime))
        x = _randn((N, D, H, W, cx), seed, F16)
        dy = _gradient((N, D, H, W, cy), regime, seed + 1)
        dw0 = _randn((cout, cin_src, 3, 3, 3), seed + 2, F32, scale=2.0 ** -20)
        _SUB_CACHE[key] = (x, dy, dw0) + R.wgrad_ref(x, co_x, cin, dy, co_y, cout, cin_src=cin_src, nominal=True)
    return _SUB_CACHE[key]


@pytest.mark.parametrize("regime", R.SUBNORMAL_REGIMES)
@pytest.mark.parametrize("geo,policy,ws_mode,route", SUB_WGRAD, ids=[f"{c[0]}-{c[3]}" for c in SUB_WGRAD])
def test_conv3_wgrad_subnormal_dy_within_fp64_bound(geo, policy, ws_mode, route, regime):
    ops = _ops()
    N, D, H, W, cx, co_x, cin, cy, co_y, cout, cin_src, _ = GEOS[geo]
    x, dy, dw0, ref, ab, nom = _sub_wgrad_operands(geo, regime)
    form = _form(geo, F16, policy, ws_mode, None)
    assert form["name"] == route, form
    assert _wgrad_ws(geo, F16, policy) == form["ws"], "partition mirror drifted from the launcher"
    ws = torch.empty(max(form["ws"], 16) if ws_mode == "full" else 16, dtype=torch.uint8, device=DEV)
    assert ws_mode == "full" or form["ws"] > 16
    dw = dw0.clone()
    ops.WGRAD_POLICY = policy
    try:
        ops.conv3d_k3_wgrad(x, cin, co_x, dy, cout, co_y, dw, workspace=ws)
    finally:
        ops.WGRAD_POLICY = 0
    torch.cuda.synchronize()
    bnd = R.wgrad_bound(ref, ab, dw0, form["chain"], nominal=nom)
    res = R.check(dw.double(), dw0.double() + ref, bnd)
    old = R.check(dw.double(), dw0.double() + ref, R.wgrad_bound(ref, ab, dw0, form["chain"]))
    print(f"wgrad {geo} {regime} {form['name']} P={form['P']} tiles={form['total']}: {res}; the subnormal term is "
          f"{_share(R.subnormal_term(nom), bnd)} of the bound (without it: ratio {old.ratio:.3g})")
    assert res.ratio <= 1.0, res


def _dense_conv_check(tag, x, cin, w_ref, bias, y, cout, chain):
    """every element of a 3x3x3 convolution launch (forward, or the data gradient on flipped, transposed weights) against fp64"""
    ref, ab, sq, nom = R.conv3_dense_ref(x, cin, R.conv3_weights(w_ref, F16), bias, nominal=True)
    bnd = R.bound(ref, ab, sq, chain, F16, nominal=nom)
    res = R.check(y[..., :cout], ref, bnd)
    sub_out = R.subnormal_share(y[..., :cout])
    print(f"{tag}: {res}; the subnormal term is {_share(R.subnormal_term(nom), bnd)} of the bound; {sub_out:.2f} of the stored outputs "
          f"are subnormal")
    assert res.ratio <= 1.0, res


SUB_DGRAD = [(2, 6, 512, 512), (1, 12, 256, 256)]


@pytest.mark.parametrize("regime", R.SUBNORMAL_REGIMES)
@pytest.mark.parametrize("N,S,cin_f,cout_f", SUB_DGRAD, ids=[f"{n}x{s}^3-{a}to{b}" for (n, s, a, b) in SUB_DGRAD])
def test_conv3_dgrad_subnormal_dy_within_fp64_bound(N, S, cin_f, cout_f, regime):
    """training._dgrad as in test_conv3_dgrad_launch_within_fp64_bound, dy in the regime, every element of dx"""
    ops, nv = _ops(), _nv()
    dy = _gradient((N, S, S, S, cout_f), regime, S + cin_f)
    w = _randn((cout_f, cin_f, 3, 3, 3), S + cout_f, F32, scale=(27 * cout_f) ** -0.5)
    wp, bp = ops.pack_conv3_weights_dgrad(w, F16, cout_packed=cout_f)
    ws = ops.splitk_ws(F16, N, S, S, S, cout_f, cin_f, DEV)
    d = nv.Conv3Desc(nv.dt_code(F16), N, S, S, S, cout_f, cout_f, 0, cin_f, cin_f, 0, 0, 0, 0, ops.CONV_POLICY)
    split = ops.conv3_form(d, False, 0 if ws is None else ws.numel() * ws.element_size()).ksplit > 1
    dx = torch.empty((N, S, S, S, cin_f), dtype=F16, device=DEV)
    ops.conv3d_k3(dy, cout_f, 0, wp, bp, cin_f, dx, 0, ops.stats_buffer(N, cin_f, DEV), workspace=ws)
    torch.cuda.synchronize()
    parts = 3 * -(-cout_f // ops.chunk_elems(F16)) if split else 0
    _dense_conv_check(f"dgrad {N}x{S}^3 {cout_f}->{cin_f} {regime} split {split}", dy, cout_f,
                      w.flip(2, 3, 4).transpose(0, 1).contiguous(), None, dx, cin_f, R.chain_length(27 * cout_f, F16, parts))


@pytest.mark.parametrize("regime", R.SUBNORMAL_REGIMES)
def test_dgrad_reduce_subnormal_dy_within_fp64_bound(regime):
    """conv3d_k3_dgrad_reduce at the smallest shape it supports (262 144 voxels: 1 x 64^3, 64 -> 64), every element of dx"""
    ops = _ops()
    N, S, C = 1, 64, 64
    assert ops.conv3d_k3_dgrad_reduce_supported(F16, N, S, S, S, C, C)
    assert not any(ops.conv3d_k3_dgrad_reduce_supported(F16, 1, a, b, c, C, C) for a, b, c in ((64, 64, 56), (56, 64, 64), (64, 56, 64)))
    dy = _gradient((N, S, S, S, C), regime, 61)
    w = _randn((C, C, 3, 3, 3), 62, F32, scale=(27 * C) ** -0.5)
    raw, gamma, beta, stats, norm = _norm_case(N, S, C, 63)
    wp, bp = ops.pack_conv3_weights_dgrad(w, F16, cout_packed=C)
    dx = torch.empty((N, S, S, S, C), dtype=F16, device=DEV)
    ops.conv3d_k3_dgrad_reduce(dy, C, wp, bp, C, dx, raw, norm, ops.instnorm_bwd_sums(raw, norm))
    torch.cuda.synchronize()
    _dense_conv_check(f"dgrad_reduce 64^3 {regime}", dy, C, w.flip(2, 3, 4).transpose(0, 1).contiguous(), None, dx, C,
                      R.chain_length(27 * C, F16))


SUB_DECONV = [((2, 2, 2), (4, 4, 4), 512, 256, 256), ((5, 4, 6), (11, 8, 13), 128, 64, 64)]      # the second: padded on two axes


@pytest.mark.parametrize("regime", R.SUBNORMAL_REGIMES)
@pytest.mark.parametrize("dims,fine,cin,cout,cskip", SUB_DECONV, ids=["2x2x2-512to256", "5x4x6-padded-128to64"])
def test_deconv_backward_subnormal_dy_within_fp64_bound(dims, fine, cin, cout, cskip, regime):
    ops = _ops()
    x, _, w = _deconv_bwd_operands(dims, fine, cin, cout, cskip)
    dcat = _gradient((2, *fine, cskip + cout), regime, sum(fine) + cin)
    dx, dw = ops.deconv_k2s2_bwd(x, cin, 8, dcat, cout, cskip, w)
    torch.cuda.synchronize()
    _check_deconv_bwd(dims, fine, cin, cout, cskip, x, dcat, w, dx, dw, nominal=True)


def test_head_backward_on_loss_gradients_at_the_initial_scale():
    """(1, 5, 7, 9) voxels, 64 channels, 16 classes: dlogits = seg_loss_grad at 2^12 x dcomb on logits spread over +-16 whose labels
    mostly agree with them -- where the sigmoid saturates the gradient underflows into the subnormals, as it does in training."""
    ops = _ops()
    N, dims, C, K = 1, (5, 7, 9), 64, 16
    g = torch.Generator(device=DEV).manual_seed(71)
    logits = ((torch.rand((N, *dims, K), generator=g, device=DEV) * 32 - 16)).to(F16)
    flip = torch.rand((N, *dims, K), generator=g, device=DEV) < 0.05
    labels = ((logits > 0) ^ flip).float().permute(0, 4, 1, 2, 3).contiguous()
    _, sums, dcomb = ops.seg_loss_reduce(logits, labels)
    dl = ops.seg_loss_grad(logits, labels, sums, dcomb * 2.0 ** 12)
    share = R.subnormal_share(dl)
    print(f"head bwd: {share:.2f} of the loss gradient is subnormal, {float((dl == 0).float().mean()):.2f} zero")
    assert share > 0.25, share
    u = _randn((N, *dims, C), 72, F16)
    w = _randn((K, C), 73, F32, scale=0.2)
    du, dW, db = ops.head_bwd(dl, u, w)
    torch.cuda.synchronize()
    _check_head_bwd(u, dl, w, du, dW, db, mfma=True, nominal=True)


def _decayed(shape, seed):
    w, want = R.subnormal_regime(shape, "decayed", seed, DEV)
    assert abs(R.subnormal_share(w) - want) < 0.02
    return w


def test_conv3_forward_with_weights_across_the_normal_boundary():
    """conv3d_k3 fp16, 1 x 8^3, 64 -> 64, weights log-uniform in [2^-20, 2^-8] (what a decayed layer can hold): the packer and the
    kernel must keep the subnormal half of them"""
    ops = _ops()
    N, S, C = 1, 8, 64
    x = _randn((N, S, S, S, C), 81, F16)
    w = _decayed((C, C, 3, 3, 3), 82).float()
    b = _randn((C,), 83, F32, scale=2.0 ** -12)
    wp, bp = ops.pack_conv3_weights(w, b, F16)
    y = torch.empty((N, S, S, S, C), dtype=F16, device=DEV)
    ops.conv3d_k3(x, C, 0, wp, bp, C, y, 0, ops.stats_buffer(N, C, DEV))
    torch.cuda.synchronize()
    _dense_conv_check("conv3d_k3 forward, decayed weights", x, C, w, b, y, C, R.chain_length(27 * C, F16))


def test_token_gemm_with_weights_across_the_normal_boundary():
    """token_gemm at the smallest K-split case of test_swin_fp64.TOKGEMM (64 x 520 -> 64, 3 K slices), every row"""
    ops, nv = _ops(), _nv()
    M, K, Nn, ks = 64, 520, 64, 3
    assert int(nv.lib().dua_token_gemm_workspace(M, K, Nn)) > 0          # the K-split form
    A = _randn((M, K), 91, F16)
    Wt = _decayed((Nn, K), 92)
    b = _randn((Nn,), 93, F32, scale=2.0 ** -12)
    out = torch.empty((M, Nn), dtype=F16, device=DEV)
    ops.token_gemm(A, Wt, b, "plain", out=out)
    torch.cuda.synchronize()
    Ad, Wd = A.double(), Wt.double()
    ref, ab, sq = R.contract(Ad, Wd.t())
    ref, ab = ref + b.double()[None], ab + b.double().abs()[None]
    nom = R.nominal_sum(Ad, Wd.t())
    bnd = R.bound(ref, ab, sq, R.chain_length(K, F16, ks), F16, nominal=nom)
    res = R.check(out, ref, bnd)
    print(f"token_gemm {M}x{K}->{Nn}, decayed weights: {res}; the subnormal term is {_share(R.subnormal_term(nom), bnd)} of the bound")
    assert res.ratio <= 1.0, res
