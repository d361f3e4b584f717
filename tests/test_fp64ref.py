"""The fp64 bound check (tests/fp64ref.py) has teeth: a torch CPU fp32 evaluation on fp16-rounded operands, stored as fp16, passes
it; the same result with one wrong product, one tap read with wrap-around instead of zero padding, or the bias of the wrong border
class of the folded up-convolution does not -- at a border voxel and at an interior tile-boundary voxel, for a 64-channel and a
128-channel (concat) contraction."""
import pytest
import torch
import torch.nn.functional as F

import fp64ref as R

DIMS = (16, 16, 24)
BORDER = (0, 0, 7, 8)          # low depth face, on tile edges along h and w
INTERIOR = (0, 7, 8, 4)        # inside, on an 8-voxel tile edge (d = 7 | 8), a slab edge in w


def _conv_case(cin):
    """A 64- or 128-input-channel convolution: fp16-rounded operands, the kernel's stand-in (torch CPU fp32, stored fp16), and
    the checker's reference at the sampled voxels."""
    g = torch.Generator().manual_seed(cin)
    x = torch.randn(1, cin, *DIMS, generator=g).half().float()
    w = torch.randn(64, cin, 3, 3, 3, generator=g) / (27 * cin) ** 0.5
    b = torch.randn(64, generator=g)
    got = F.conv3d(x, w.half().float(), b, padding=1).half()              # [1, 64, D, H, W]
    pts = R.sample_voxels(1, DIMS, n_random=300, seed=cin)
    A, _ = R.gather_taps(x.permute(0, 2, 3, 4, 1).contiguous(), pts, 0, cin)
    Wm = R.conv3_weights(w, torch.float16)
    ref, ab, sq = R.conv3_ref(A, Wm, b)
    bnd = R.bound(ref, ab, sq, R.chain_length(27 * cin, torch.float16), torch.float16)
    return dict(x=x, w=w.half().double(), got=got, pts=pts, A=A, Wm=Wm, ref=ref, bnd=bnd)


def _fold_case():
    """UpCat's first convolution over cat([skip 64, deconv(u) 64]) in the folded form (composed weights rounded once to fp16,
    27-class bias table in fp32), evaluated in fp32 as the kernel's stand-in."""
    g = torch.Generator().manual_seed(7)
    Cs, Cu, Cm, Co = 64, 64, 64, 64
    xs = torch.randn(1, Cs, *DIMS, generator=g).half().float()
    u = torch.randn(1, Cu, *(s // 2 for s in DIMS), generator=g).half().float()
    wc = torch.randn(Co, Cs + Cm, 3, 3, 3, generator=g) / (27 * (Cs + Cm)) ** 0.5
    bc = torch.randn(Co, generator=g)
    wd = torch.randn(Cu, Cm, 2, 2, 2, generator=g) / Cu ** 0.5
    bd = torch.randn(Cm, generator=g)
    Wp = {k: v[0].half().double() for k, v in R.compose_fold(wc[:, Cs:], wd).items()}
    rows, arows = R.fold_bias_table(wc[:, Cs:], bc, bd)
    pts = R.sample_voxels(1, DIMS, n_random=300, seed=5)
    par, ok, phi, deltas = R.fold_parents(pts, DIMS)
    ucl = u.permute(0, 2, 3, 4, 1).contiguous()
    U = ucl[pts[:, None, 0].expand_as(ok), par[..., 0].clamp(0, DIMS[0] // 2 - 1), par[..., 1].clamp(0, DIMS[1] // 2 - 1),
            par[..., 2].clamp(0, DIMS[2] // 2 - 1)].double()
    A, _ = R.gather_taps(xs.permute(0, 2, 3, 4, 1).contiguous(), pts, 0, Cs)
    Wm = R.conv3_weights(wc[:, :Cs], torch.float16)
    cls = R.border_class(pts, DIMS)
    ref, ab, sq = R.fold_ref(A, Wm, U, ok, phi, deltas, Wp, rows[cls], arows[cls])
    btab32 = rows.float().double()           # the packer's fp32 table
    got, _, _ = R.fold_ref(A.float(), Wm.float(), U.float(), ok, phi, deltas, {k: v.float() for k, v in Wp.items()},
                           btab32[cls].float(), arows[cls].float())
    got = got.half().double()
    bnd = R.bound(ref, ab, sq, R.chain_length(27 * Cs + 8 * Cu, torch.float16), torch.float16, extra=R.U32 * 1800 * arows[cls])
    return dict(pts=pts, A=A, Wm=Wm, U=U, ok=ok, phi=phi, deltas=deltas, Wp=Wp, rows=btab32, cls=cls, ref=ref, bnd=bnd, got=got,
                xs=xs)


def _row(pts, p):
    hit = (pts == torch.tensor(p)).all(1).nonzero()
    assert hit.numel() == 1, f"{p} is not among the sampled voxels"
    return int(hit[0, 0])


def _got_conv(c):
    pts = c["pts"]
    return c["got"][pts[:, 0], :, pts[:, 1], pts[:, 2], pts[:, 3]].double()       # [P, 64]


def test_structured_voxels_are_sampled():
    D, H, W = 63, 48, 40
    pts = R.sample_voxels(2, (D, H, W), n_random=100)
    assert len({tuple(p) for p in pts.tolist()}) == pts.shape[0]
    for n in range(2):
        for corner in [(0, 0, 0), (D - 1, H - 1, W - 1), (0, H - 1, 0), (D - 1, 0, W - 1)]:
            _row(pts, (n, *corner))
        for p in [(0, 7, 8), (0, 8, 39), (62, 47, 0), (7, 4, 3), (55, 40, 32), (56, 39, 39)]:
            _row(pts, (n, *p))
    for a, S in enumerate((D, H, W)):
        seen = set(pts[:, 1 + a].tolist())
        assert {0, 3, 4, 7, 8, S - 1} <= seen


@pytest.mark.parametrize("cin", [64, 128])
def test_unmutated_result_passes(cin):
    c = _conv_case(cin)
    r = R.check(_got_conv(c), c["ref"], c["bnd"], c["pts"])
    assert r.ratio <= 1, r
    assert r.ratio > 0.05, f"the bound is loose where it should be tight: {r}"


def test_unmutated_fold_passes():
    c = _fold_case()
    r = R.check(c["got"], c["ref"], c["bnd"], c["pts"])
    assert r.ratio <= 1, r


@pytest.mark.parametrize("cin", [64, 128])
@pytest.mark.parametrize("where", [BORDER, INTERIOR], ids=["border", "interior"])
def test_one_dropped_product_is_rejected(cin, where):
    c = _conv_case(cin)
    i, o = _row(c["pts"], where), 5
    prods = (c["A"][i].reshape(-1) * c["Wm"][:, o]).abs()
    nz = prods[prods > 0]
    k = int((prods - nz.median()).abs().argmin())
    got = _got_conv(c)
    got[i, o] = float(torch.as_tensor(got[i, o] - c["A"][i].reshape(-1)[k] * c["Wm"][k, o]).half())
    r = R.check(got, c["ref"], c["bnd"], c["pts"])
    assert r.ratio > 1 and r.where[0] == where, r


@pytest.mark.parametrize("cin", [64, 128])
@pytest.mark.parametrize("where", [BORDER, INTERIOR], ids=["border", "interior"])
def test_one_wrapped_tap_is_rejected(cin, where):
    """Border voxel: the tap at depth -1 read from the last plane instead of zero padding.  Interior voxel: the tap across the
    tile edge (depth 8) read from the first plane of the voxel's own tile (depth 0), a halo that was never loaded."""
    c = _conv_case(cin)
    i, o = _row(c["pts"], where), 3
    n, d, h, w = where
    t = 4 if d == 0 else 22                     # tap (kd, kh, kw) = (0, 1, 1): depth -1; (2, 1, 1): depth + 1
    src_d = DIMS[0] - 1 if d == 0 else (d + 1) - 8
    want_d = d - 1 if d == 0 else d + 1
    x = c["x"][n].double()
    right = x[:, want_d, h, w] if 0 <= want_d < DIMS[0] else torch.zeros_like(x[:, 0, h, w])
    wrong = x[:, src_d, h, w]
    wt = c["w"][o, :, t // 9, (t // 3) % 3, t % 3]
    got = _got_conv(c)
    got[i, o] = float(torch.as_tensor(got[i, o] + ((wrong - right) * wt).sum()).half())
    r = R.check(got, c["ref"], c["bnd"], c["pts"])
    assert r.ratio > 1 and r.where[0] == where, r


@pytest.mark.parametrize("where", [BORDER, INTERIOR], ids=["border", "interior"])
@pytest.mark.parametrize("mutation", ["product", "wrap", "bias_class"])
def test_fold_mutations_are_rejected(where, mutation):
    c = _fold_case()
    i, o = _row(c["pts"], where), 9
    got = c["got"].clone()
    if mutation == "product":
        prods = (c["A"][i].reshape(-1) * c["Wm"][:, o]).abs()
        k = int((prods - prods[prods > 0].median()).abs().argmin())
        delta = -c["A"][i].reshape(-1)[k] * c["Wm"][k, o]
    elif mutation == "wrap":
        n, d, h, w = where
        t = 4 if d == 0 else 22
        src_d = DIMS[0] - 1 if d == 0 else d + 1 - 8
        x = c["xs"][n].double()
        right = torch.zeros_like(x[:, 0, h, w]) if d == 0 else x[:, d + 1, h, w]
        wrong = x[:, src_d, h, w]
        delta = ((wrong - right) * c["Wm"].reshape(27, -1, 64)[t, :, o]).sum()
    else:
        cls = int(c["cls"][i])
        other = 13 if cls != 13 else 12          # interior <-> the low w face
        delta = c["rows"][other, o] - c["rows"][cls, o]
    got[i, o] = float(torch.as_tensor(got[i, o] + delta).half())
    r = R.check(got, c["ref"], c["bnd"], c["pts"])
    assert r.ratio > 1 and r.where[0] == where, (mutation, r)


def test_fp16_transform_emulation_rounds_once():
    """The fused input transform: two mixed fmas rounded once into fp16, the larger kept; against the same arithmetic spelled
    out per element with numpy's direct float64 -> fp16 conversion."""
    import numpy as np
    g = torch.Generator().manual_seed(3)
    raw = torch.randn(4000, 16, generator=g).half().double()
    sc = (torch.rand(16, generator=g) + 0.5).float()
    sh = torch.randn(16, generator=g).float()
    add = torch.randn(16, generator=g).float()
    got = R.transform(raw, sc, sh, add, torch.float16)
    for k in range(0, 4000, 97):
        for c in range(16):
            x = float(raw[k, c])
            p = np.float16(x * float(sc[c]) + float(np.float32(sh[c]) + np.float32(add[c])))
            sn = np.float32(np.float32(0.1) * np.float32(sc[c]))
            an = np.float32(float(np.float32(0.1)) * float(sh[c]) + float(add[c]))
            q = np.float16(x * float(sn) + float(an))
            assert float(got[k, c]) == float(max(p, q))
    # against the exact function: within one fp16 ulp everywhere
    exact = torch.nn.functional.leaky_relu(raw * sc.double() + sh.double(), 0.1) + add.double()
    assert bool(((got - exact).abs() <= 2 ** -10 * exact.abs() + 2 ** -24).all())


# ---- backward bounds ------------------------------------------------------------------------------------------------------------
WG_DIMS = (8, 8, 24)          # 4x8x8 tiles: 2 x 1 x 3 per sample


def _wgrad_case(cin=24, cin_src=17, cout=16, P=4):
    """The fetch-once weight gradient, simulated in fp32 on fp16-rounded operands as the kernel sums it: per-tile partials,
    each partition the tiles part, part + P, ... (walking from sample 0 into sample 1), the partitions reduced, added into dw0."""
    g = torch.Generator().manual_seed(cin + P)
    N = 2
    x = torch.randn(N, *WG_DIMS, cin, generator=g).half()
    dy = torch.randn(N, *WG_DIMS, cout, generator=g).half()
    dw0 = torch.randn(cout, cin_src, 3, 3, 3, generator=g)
    ref, ab = R.wgrad_ref(x, 0, cin, dy, 0, cout, cin_src=cin_src)
    full, _ = R.wgrad_ref(x, 0, cin, dy, 0, cout)                 # every packed channel (the filter's input)
    D, H, W = WG_DIMS
    tiles = [(n, d, h, w) for n in range(N) for d in range(0, D, 4) for h in range(0, H, 8) for w in range(0, W, 8)]

    def tile_dw(t):
        n, d, h, w = t
        m = torch.zeros(N, *WG_DIMS, 1, dtype=torch.float64)
        m[n, d:d + 4, h:h + 8, w:w + 8] = 1
        r, _ = R.wgrad_ref(x, 0, cin, (dy.double() * m).float(), 0, cout)
        return r.float()
    parts = []
    for p in range(P):
        s = torch.zeros(cout, cin, 3, 3, 3)
        for t in tiles[p::P]:
            s = s + tile_dw(t)
        parts.append(s)
    total = len(tiles)
    return dict(x=x, dy=dy, dw0=dw0, ref=ref, ab=ab, full=full, parts=parts, cin_src=cin_src, P=P, total=total,
                bnd=R.wgrad_bound(ref, ab, dw0, R.wgrad_fo_chain(P, total, "plain")))


def _wgrad_got(c, parts=None, cin_src=None):
    s = sum(c["parts"] if parts is None else parts)
    cs = c["cin_src"] if cin_src is None else cin_src
    out = c["dw0"].clone()
    k = min(cs, c["cin_src"])
    out[:, :k] += s[:, :k]
    if cs > c["cin_src"]:              # the filter lets one channel too many through: it lands in the next row of dw
        flat = out.view(-1, 27)
        for co in range(s.shape[0]):
            i = co * c["cin_src"] + c["cin_src"]
            if i < flat.shape[0]:
                flat[i] += s[co, c["cin_src"]].reshape(27)
    return out.double()


@pytest.fixture(scope="module")
def wg():
    return _wgrad_case()


def test_wgrad_bound_accepts_the_kernels_summation(wg):
    res = R.check(_wgrad_got(wg), wg["dw0"].double() + wg["ref"], wg["bnd"])
    assert res.ratio <= 1.0, res


def test_wgrad_bound_rejects_a_dropped_partition(wg):
    res = R.check(_wgrad_got(wg, parts=wg["parts"][:1] + wg["parts"][2:]), wg["dw0"].double() + wg["ref"], wg["bnd"])
    assert res.ratio > 1.0, res


def test_wgrad_bound_rejects_a_partition_counted_twice(wg):
    res = R.check(_wgrad_got(wg, parts=wg["parts"] + wg["parts"][2:3]), wg["dw0"].double() + wg["ref"], wg["bnd"])
    assert res.ratio > 1.0, res


@pytest.mark.parametrize("cin_src", [16, 18])
def test_wgrad_bound_rejects_the_source_channel_filter_off_by_one(wg, cin_src):
    res = R.check(_wgrad_got(wg, cin_src=cin_src), wg["dw0"].double() + wg["ref"], wg["bnd"])
    assert res.ratio > 1.0, res


def test_wgrad_bound_rejects_a_tap_shifted_at_the_border(wg):
    """Tap kw = 2 reads voxel w + 1: at the last plane the kernel must read zero; here it reads the row's first voxel (wrap)."""
    x, dy = wg["x"], wg["dy"]
    W = WG_DIMS[2]
    wrong = x.double()[:, :, :, 0:1]                             # what the wrapped tap reads at w = W - 1
    extra = torch.zeros(dy.shape[-1], x.shape[-1], 3, 3, 3, dtype=torch.float64)
    xp = torch.zeros(2, WG_DIMS[0] + 2, WG_DIMS[1] + 2, 1, x.shape[-1], dtype=torch.float64)
    xp[:, 1:-1, 1:-1] = wrong
    g = dy.double()[:, :, :, W - 1]
    for kd in range(3):
        for kh in range(3):
            xs = xp[:, kd:kd + WG_DIMS[0], kh:kh + WG_DIMS[1], 0]
            extra[:, :, kd, kh, 2] = g.reshape(-1, g.shape[-1]).t() @ xs.reshape(-1, x.shape[-1])
    got = _wgrad_got(wg) + extra[:, :wg["cin_src"]]
    res = R.check(got, wg["dw0"].double() + wg["ref"], wg["bnd"])
    assert res.ratio > 1.0, res


def _in_bwd_case():
    """InstanceNorm + LeakyReLU backward simulated in the kernels' fp32 arithmetic (fp32 mean / rstd from the statistics, zh,
    z, the slope, per-element then summed), and its fp64 reference."""
    g = torch.Generator().manual_seed(3)
    N, V, C = 2, 4096, 16
    raw = (torch.randn(N, V, C, generator=g) * 1.5 + 0.3).half()
    dA = torch.randn(N, V, C, generator=g).half()
    gamma = torch.rand(C, generator=g) + 0.5
    beta = torch.randn(C, generator=g) * 0.2
    rd = raw.double()
    sums = torch.stack([rd.sum(1), (rd * rd).sum(1)], -1)
    r = R.in_bwd_ref(dA, raw, sums, gamma, beta, V)
    mu, rs = r["mean"].float()[:, None], r["rstd"].float()[:, None]
    zh = (raw.float() - mu) * rs
    z = zh * gamma + beta
    d = dA.float()
    slope = torch.tensor(R.SLOPE, dtype=torch.float32)
    return dict(r=r, zh=zh, z=z, d=d, slope=slope, gamma=gamma, rs=rs, V=V)


def _in_bwd_sim(c, flip=None):
    dz = torch.where(c["z"] > 0, c["d"], c["d"] * c["slope"])
    if flip is not None:                              # one element takes the other slope
        n, v, ch = flip
        dz[n, v, ch] = c["d"][n, v, ch] * c["slope"] if c["z"][n, v, ch] > 0 else c["d"][n, v, ch]
    S1, S2 = dz.double().sum(1).float(), (dz * c["zh"]).double().sum(1).float()
    V = c["V"]
    dY = (c["gamma"] * c["rs"] * (dz - (S1 / V)[:, None] - c["zh"] * (S2 / V)[:, None])).half()
    return S1.double(), S2.double(), dY.double()


def test_instnorm_backward_bound_accepts_the_kernels_arithmetic():
    c = _in_bwd_case()
    r = c["r"]
    b0, b1, b2 = R.in_bwd_sums_bound(r, R.in_bwd_reduce_chain(16, c["V"], torch.float16))
    S1, S2, dY = _in_bwd_sim(c)
    assert R.check(S1, r["S1"], b1).ratio <= 1.0 and R.check(S2, r["S2"], b2).ratio <= 1.0
    res = R.check(dY, r["dY"], R.in_bwd_dy_bound(r, b1, b2, torch.float16))
    assert res.ratio <= 1.0, res


def test_instnorm_backward_bound_rejects_a_wrong_slope_outside_the_kink_margin():
    c = _in_bwd_case()
    r = c["r"]
    b0, b1, b2 = R.in_bwd_sums_bound(r, R.in_bwd_reduce_chain(16, c["V"], torch.float16))
    # the element with the largest |dA| among those whose z lies outside the margin but within 0.05 of the kink
    cand = (~r["near"]) & (r["z"].abs() < 0.05)
    score = torch.where(cand, r["d"].abs(), torch.zeros_like(r["d"]))
    k = int(torch.argmax(score))
    flip = tuple(int(i) for i in torch.unravel_index(torch.tensor(k), score.shape))
    S1, S2, dY = _in_bwd_sim(c, flip)
    res = R.check(dY, r["dY"], R.in_bwd_dy_bound(r, b1, b2, torch.float16))
    assert res.ratio > 1.0, res
    assert tuple(res.where) == flip


# ---- the residual branch over cat((ConvTranspose3d(lo), skip)) without the upsampled tensor (R.deconv_res_ref) ---------------------
def _deconv_res_case():
    """48 coarse channels -> 48 middle, 48 skip channels, 48 outputs on an 8 x 12 x 8 fine grid; the kernel's stand-in composes
    the weights per child with matrix products in fp32 (another summation order than the reference's einsum), rounds them once
    to fp16, contracts in fp32 and stores fp16."""
    g = torch.Generator().manual_seed(11)
    Cu, Cmid, Cs, Co, dims = 48, 48, 48, 48, (8, 12, 8)
    lo = torch.randn(1, *(s // 2 for s in dims), Cu, generator=g).half()
    skip = torch.randn(1, *dims, Cs, generator=g).half()
    w3 = torch.randn(Co, Cmid + Cs, generator=g) / (Cmid + Cs) ** 0.5
    wd = torch.randn(Cu, Cmid, 2, 2, 2, generator=g) / Cu ** 0.5
    pts = R.sample_voxels(1, dims, n_random=200, seed=3)
    child = (pts[:, 1] & 1) * 4 + (pts[:, 2] & 1) * 2 + (pts[:, 3] & 1)
    par = pts.clone()
    par[:, 1:] >>= 1
    lo_q, sk_q = R.gather_points(lo, par, 0, Cu), R.gather_points(skip, pts, 0, Cs)
    comp = torch.stack([(w3[:, :Cmid] @ wd.reshape(Cu, Cmid, 8)[:, :, k].t()).half().float() for k in range(8)])     # [8, Co, Cu]
    wsk = w3[:, Cmid:].half().float()

    def stand_in(ch, with_skip=True):
        y = torch.einsum("pc,poc->po", lo_q.float(), comp[ch])
        if with_skip:
            y = y + sk_q.float() @ wsk.t()
        return y.half()

    ref, ab, sq = R.deconv_res_ref(lo_q, sk_q, w3, wd, child)
    bnd = R.bound(ref, ab, sq, R.chain_length(Cu + Cs, torch.float16), torch.float16, emulated_in=torch.float16)
    return dict(pts=pts, child=child, stand_in=stand_in, ref=ref, bnd=bnd)


def test_deconv_res_emulation_passes():
    c = _deconv_res_case()
    r = R.check(c["stand_in"](c["child"]), c["ref"], c["bnd"], c["pts"])
    assert r.ratio <= 1, r
    assert r.ratio > 0.05, f"the bound is loose where it should be tight: {r}"


@pytest.mark.parametrize("where", [BORDER, INTERIOR], ids=["border", "interior"])
def test_deconv_res_wrong_child_is_rejected(where):
    """One voxel takes the composed weights of the child with the other parity along w."""
    c = _deconv_res_case()
    where = (where[0], where[1], where[2], where[3] % 8)          # the case's grid is 8 wide
    i = _row(c["pts"], where)
    ch = c["child"].clone()
    ch[i] ^= 1
    got = c["stand_in"](c["child"])
    got[i] = c["stand_in"](ch)[i]
    r = R.check(got, c["ref"], c["bnd"], c["pts"])
    assert r.ratio > 1 and r.where[0] == where, r


def test_deconv_res_missing_skip_term_is_rejected():
    c = _deconv_res_case()
    i = _row(c["pts"], (0, 7, 8, 4))
    got = c["stand_in"](c["child"])
    got[i] = c["stand_in"](c["child"], with_skip=False)[i]
    r = R.check(got, c["ref"], c["bnd"], c["pts"])
    assert r.ratio > 1 and r.where[0] == (0, 7, 8, 4), r
