"""The bounds of test_deconv_fp64.py, test_materialize_fp64.py and test_head_fwd_fp64.py have teeth.  Each kernel's summation is
emulated on the CPU -- fp16 / fp32 operands, the accumulator rounded to fp32 after every MFMA step (fp16: 16 exact products per step;
fp32: one fmaf per product), chunks in the kernel's order, the k-split's four partial tiles added to zero in the order 0..3, the
bias where the form adds it, one rounding into the stored type -- and passes its bound; the same result with one planted defect does
not, at the voxel the defect was planted in.  Bounds are the derived ones (fp64ref.bound with the form's chain, materialize_bound):
nothing here is calibrated."""
import pytest
import torch

import fp64ref as R

F16, F32 = torch.float16, torch.float32
BORDER, INTERIOR = (0, 0, 0, 0), (0, 3, 4, 5)


# ---- the transposed convolution -----------------------------------------------------------------------------------------------------
def _weights_at(w, dtype, child):
    wq = w.half() if dtype == F16 else w.float()
    return wq.double().reshape(w.shape[0], w.shape[1], 8)[:, :, child].permute(2, 0, 1)        # [P, Cin, Cout]


def emulate_deconv(A, Wsel, bias, dtype, form, acc_dtype=F32, partials=(0, 1, 2, 3)):
    """A [P, Cin] float64 (values of the kernel's operand type), Wsel [P, Cin, Cout], bias [P, Cout] fp32 -> the stored output
    [P, Cout] as float64.  ``acc_dtype``: the type the accumulator is rounded to after every step; ``partials``: which of the
    k-split's four partial tiles are added, in which order."""
    rnd = lambda t: t.to(acc_dtype).double()                # noqa: E731
    cin = A.shape[1]
    ck, step = (32, 16) if dtype == F16 else (16, 1)
    nch = -(-cin // ck)

    def run(chunks, acc):
        for ch in chunks:
            for k0 in range(ch * ck, min((ch + 1) * ck, cin), step):
                k1 = min(k0 + step, cin)
                acc = rnd(acc + (A[:, k0:k1, None] * Wsel[:, k0:k1]).sum(1))
        return acc
    zero = torch.zeros((A.shape[0], Wsel.shape[2]), dtype=torch.float64)
    b = bias.double()
    if form == "one_tap":
        out = rnd(run(range(nch), zero) + b)
    elif form == "alltaps":
        out = run(range(nch), b.clone())
    else:
        tiles = [run(range(w, nch, 4), zero) for w in range(4)]
        o = zero
        for w in partials:
            o = rnd(o + tiles[w])
        out = rnd(o + b)
    return out.to(dtype).double()


def _deconv_case(form, dtype):
    """A replicate-padded launch (every output extent odd) with a ragged last chunk and a second, 8-wide output-channel tile."""
    cin = {(F16, "ksplit"): 272, (F32, "ksplit"): 136}.get((dtype, form), 40)
    cout, coarse = 72, ((2, 3, 3) if form == "ksplit" else (3, 4, 5))
    g = torch.Generator().manual_seed(cin + len(form))
    x = (torch.randn(1, *coarse, cin, generator=g) * 1.5 + 0.25).to(dtype)
    w = torch.randn(cin, cout, 2, 2, 2, generator=g) / cin ** 0.5
    b = torch.randn(cout, generator=g)
    out_dims = tuple(2 * s + 1 for s in coarse)
    pts = R.all_voxels(1, out_dims)
    parent, child = R.deconv_sources(pts, coarse)
    A = R.gather_points(x, parent, 0, cin)
    ref, ab, sq = R.deconv_ref_by_child(A, w, b, dtype, child)
    chain = R.deconv_fwd_chain(form, cin, dtype)
    return dict(form=form, dtype=dtype, cin=cin, cout=cout, coarse=coarse, out_dims=out_dims, pts=pts, child=child, A=A, w=w, b=b,
                ref=ref, fused=R.bound(ref, ab, sq, chain, dtype, emulated_in=dtype), plain=R.bound(ref, ab, sq, chain, dtype),
                got=emulate_deconv(A, _weights_at(w, dtype, child), b[None].expand(len(pts), -1), dtype, form))


_CASES = {}


def _case(form, dtype):
    if (form, dtype) not in _CASES:
        _CASES[(form, dtype)] = _deconv_case(form, dtype)
    return _CASES[(form, dtype)]


def _row(pts, p):
    hit = (pts == torch.tensor(p)).all(1).nonzero()
    assert hit.numel() == 1, p
    return int(hit[0, 0])


def _with_row(c, i, A=None, child=None, bias=None, **kw):
    """The emulated output with row i recomputed from changed operands."""
    A = c["A"][i:i + 1] if A is None else A
    child = c["child"][i:i + 1] if child is None else child
    bias = c["b"][None] if bias is None else bias
    got = c["got"].clone()
    got[i] = emulate_deconv(A, _weights_at(c["w"], c["dtype"], child), bias, c["dtype"], c["form"], **kw)[0]
    return got


FORMS = ["one_tap", "ksplit", "alltaps"]


def test_grouped_reference_equals_the_per_voxel_one():
    c = _case("one_tap", F16)
    ref, ab, sq = R.deconv_ref(c["A"], c["w"], c["b"], F16, c["child"])
    r2, a2, s2 = R.deconv_ref_by_child(c["A"], c["w"], c["b"], F16, c["child"])
    for p, q in ((ref, r2), (ab, a2), (sq, s2)):
        assert float((p - q).abs().max()) <= 1e-13 * float(ab.max())


def test_chains_follow_the_launchers():
    assert R.deconv_fwd_chain("one_tap", 40, F16) == 2 * 2 + 4 + 1 and R.deconv_fwd_chain("one_tap", 40, F32) == 16 * 3 + 1
    assert R.deconv_fwd_chain("ksplit", 272, F16) == 2 * 3 + 4 + 4 + 1 and R.deconv_fwd_chain("ksplit", 136, F32) == 16 * 3 + 4 + 1
    assert R.deconv_fwd_chain("alltaps", 128, F16) == 2 * 4 + 4 and R.deconv_fwd_chain("alltaps", 64, F32) == 64
    assert R.head_fwd_chain(64, F16) == 7 and R.head_fwd_chain(8, F16) == 9 and R.head_fwd_chain(64, F32) == 65


@pytest.mark.parametrize("dtype", [F16, F32])
@pytest.mark.parametrize("form", FORMS)
def test_deconv_emulation_passes(form, dtype):
    c = _case(form, dtype)
    r = R.check(c["got"], c["ref"], c["plain"], c["pts"])
    print(f"deconv {form} {dtype} {c['cin']}->{c['cout']} {c['coarse']}: {r}")
    assert r.ratio <= 1, r


@pytest.mark.parametrize("dtype", [F16, F32])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("where", [BORDER, INTERIOR], ids=["border", "interior"])
@pytest.mark.parametrize("defect", ["dropped_channel", "child_parity", "bias_second_tile"])
def test_deconv_defects_are_rejected(defect, where, form, dtype):
    """Against the looser bound of the two (the one fused launches are held to)."""
    c = _case(form, dtype)
    where = tuple(min(v, s - 1) for v, s in zip(where, (1, *c["out_dims"])))
    i = _row(c["pts"], where)
    if defect == "dropped_channel":                          # the last channel of the ragged last chunk
        A = c["A"][i:i + 1].clone()
        A[0, -1] = 0
        got = _with_row(c, i, A=A)
    elif defect == "child_parity":
        got = _with_row(c, i, child=c["child"][i:i + 1] ^ 1)
    else:
        b = c["b"][None].clone()
        b[0, 64:] = 0
        got = _with_row(c, i, bias=b)
    r = R.check(got, c["ref"], c["fused"], c["pts"])
    assert r.ratio > 1 and r.where[0] == where, (defect, r)


@pytest.mark.parametrize("dtype", [F16, F32])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("where", ["edge", "face"])
def test_pad_plane_copied_from_the_wrong_plane_is_rejected(where, form, dtype):
    """The replicate-pad plane 2 S holds plane 2 S - 1; a copy of plane 2 S - 2 is the other child of the same parent."""
    c = _case(form, dtype)
    Do, Ho, Wo = c["out_dims"]
    p = (0, Do - 1, 0, Wo - 1) if where == "edge" else (0, Do - 1, 2, 3)
    i = _row(c["pts"], p)
    assert int(c["child"][i]) & 4
    got = _with_row(c, i, child=c["child"][i:i + 1] & ~4)
    r = R.check(got, c["ref"], c["fused"], c["pts"])
    assert r.ratio > 1 and r.where[0] == p, r


@pytest.mark.parametrize("dtype", [F16, F32])
@pytest.mark.parametrize("where", [BORDER, INTERIOR], ids=["border", "interior"])
@pytest.mark.parametrize("partials", [(0, 1, 3), (0, 1, 2, 2, 3)], ids=["dropped", "twice"])
def test_ksplit_partial_defects_are_rejected(partials, where, dtype):
    c = _case("ksplit", dtype)
    where = tuple(min(v, s - 1) for v, s in zip(where, (1, *c["out_dims"])))
    i = _row(c["pts"], where)
    r = R.check(_with_row(c, i, partials=partials), c["ref"], c["fused"], c["pts"])
    assert r.ratio > 1 and r.where[0] == where, r


@pytest.mark.parametrize("dtype", [F16, F32])
@pytest.mark.parametrize("form", FORMS)
def test_accumulation_in_fp16_is_rejected(form, dtype):
    """Shown against the bound of unfused launches: the fused bound's input term is itself of the size of fp16 roundings."""
    c = _case(form, dtype)
    got = emulate_deconv(c["A"], _weights_at(c["w"], dtype, c["child"]), c["b"][None].expand(len(c["pts"]), -1), dtype, form,
                         acc_dtype=F16)
    for where in (BORDER, INTERIOR):
        where = tuple(min(v, s - 1) for v, s in zip(where, (1, *c["out_dims"])))
        i = _row(c["pts"], where)
        g = c["got"].clone()
        g[i] = got[i]
        r = R.check(g, c["ref"], c["plain"], c["pts"])
        assert r.ratio > 1 and r.where[0] == where, r


# ---- materialize ------------------------------------------------------------------------------------------------------------------
def emulate_materialize(raw, sc, sh, ad, emb, dtype, slope=R.SLOPE, use_add=True):
    """fmaf, the slope product, + add, + emb in fp32, one rounding into ``dtype`` (materialize_kernel)."""
    import numpy as np
    y = (raw.double() * sc.double() + sh.double()).float()
    y = torch.where(y > 0, y, y * np.float32(slope))
    if use_add:
        y = y + ad.float()
    if emb is not None:
        y = y + emb.float()
    return y.to(dtype)


def _mat_case(dtype):
    g = torch.Generator().manual_seed(11)
    N, dims, C, es = 2, (5, 6, 7), 24, 40
    raw = (torch.randn(N, *dims, C, generator=g) * torch.tensor([1.5, 2.5]).view(2, 1, 1, 1, 1) + 0.25).to(dtype)
    embw = torch.randn(N, *dims, es, generator=g).to(dtype)
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.5
    ad = torch.randn(N, C, generator=g)
    sc64, sh64, _, _ = R.finalize(R.channel_sums(raw), gamma, beta, raw[0, ..., 0].numel())
    sc, sh = sc64.float(), sh64.float()
    v = lambda t: t[:, None, None, None, :]          # noqa: E731
    ref, mag = R.materialize_ref(raw.double(), v(sc), v(sh), v(ad), embw[..., :C].double())
    return dict(raw=raw, embw=embw, sc=v(sc), sh=v(sh), ad=v(ad), C=C, ref=ref, bnd=R.materialize_bound(ref, mag, dtype), dtype=dtype)


def _mat_got(c, **kw):
    emb = kw.pop("emb", c["embw"][..., :c["C"]])
    return emulate_materialize(c["raw"], c["sc"], c["sh"], c["ad"], emb, c["dtype"], **kw)


@pytest.mark.parametrize("dtype", [F16, F32])
def test_materialize_emulation_passes(dtype):
    c = _mat_case(dtype)
    got = _mat_got(c)
    r = R.check(got, c["ref"], c["bnd"])
    print(f"materialize {dtype}: {r}")
    assert r.ratio <= 1, r
    pr, pb = R.pool_ref(c["ref"], c["bnd"])
    pooled = torch.nn.functional.max_pool3d(got.float().permute(0, 4, 1, 2, 3), 2).permute(0, 2, 3, 4, 1)
    assert R.check(pooled, pr, pb).ratio <= 1


@pytest.mark.parametrize("dtype", [F16, F32])
@pytest.mark.parametrize("defect", ["slope", "no_add", "emb_stride"])
def test_materialize_defects_are_rejected(defect, dtype):
    c = _mat_case(dtype)
    if defect == "slope":
        got = _mat_got(c, slope=0.01)
    elif defect == "no_add":
        got = _mat_got(c, use_add=False)
    else:                                                    # emb rows read C apart instead of its own stride apart
        e = c["embw"]
        got = _mat_got(c, emb=e.reshape(-1)[:e.numel() // e.shape[-1] * c["C"]].view(*e.shape[:4], c["C"]))
    r = R.check(got, c["ref"], c["bnd"])
    assert r.ratio > 1, (defect, r)


@pytest.mark.parametrize("dtype", [F16, F32])
def test_pooling_window_shifted_on_an_odd_axis_is_rejected(dtype):
    """Extent 5 pools planes (0, 1), (2, 3); windows (1, 2), (3, 4) are neither bit-equal to the floor pooling of the stored output
    nor within the windows' bounds of the fp64 maximum."""
    c = _mat_case(dtype)
    got = _mat_got(c).float()
    pool = lambda t: torch.nn.functional.max_pool3d(t.permute(0, 4, 1, 2, 3), 2).permute(0, 2, 3, 4, 1)      # noqa: E731
    shifted = pool(got[:, 1:])
    assert shifted.shape == pool(got).shape and not torch.equal(shifted, pool(got))
    pr, pb = R.pool_ref(c["ref"], c["bnd"])
    assert R.check(shifted, pr, pb).ratio > 1


# ---- the training head's forward pass ------------------------------------------------------------------------------------------------
def emulate_head(u, w, b, dtype):
    """mfma route: fp16 weights, the accumulator starts at the bias, 32 exact products per step; plain: fp32 weights, bias, then
    one fmaf per channel."""
    route = R.head_fwd_route(w.shape[1], dtype)
    wq = (w.half() if route == "mfma" else w.float()).double()
    acc = b.double()[None].expand(u.shape[0], -1)
    step = 32 if route == "mfma" else 1
    for k0 in range(0, w.shape[1], step):
        acc = (acc + u[:, k0:k0 + step].double() @ wq[:, k0:k0 + step].t()).float().double()
    return acc.to(dtype).double()


@pytest.mark.parametrize("dtype", [F16, F32])
@pytest.mark.parametrize("C,K", [(64, 16), (32, 13), (8, 2)])
def test_head_forward_emulation_and_defects(dtype, C, K):
    g = torch.Generator().manual_seed(C + K)
    u = torch.randn(300, C, generator=g).to(dtype)
    w, b = torch.randn(K, C, generator=g) * 0.2, torch.randn(K, generator=g)
    ref, ab, sq = R.head_fwd_ref(u.double(), w, b, dtype)
    bnd = R.bound(ref, ab, sq, R.head_fwd_chain(C, dtype), dtype)
    got = emulate_head(u, w, b, dtype)
    r = R.check(got, ref, bnd)
    print(f"head fwd {dtype} C={C} K={K} {R.head_fwd_route(C, dtype)}: {r}")
    assert r.ratio <= 1, r
    # one product dropped (the median-sized one of its row), the bias of the last class dropped
    wq = (w.half() if R.head_fwd_route(C, dtype) == "mfma" else w).double()
    i, k = 123, K // 2
    prods = u[i].double() * wq[k]
    c = int((prods.abs() - prods.abs().median()).abs().argmin())
    bad = got.clone()
    bad[i, k] = float((got[i, k] - prods[c]).to(dtype))
    r1 = R.check(bad, ref, bnd)
    assert r1.ratio > 1 and r1.where == (i, k), r1
    bad = got.clone()
    bad[i, K - 1] = float((got[i, K - 1] - b[K - 1].double()).to(dtype))
    r2 = R.check(bad, ref, bnd)
    assert r2.ratio > 1 and r2.where == (i, K - 1), r2
