"""One fp16 training step in place -- training.native_logits_cl + _SegLoss and a plain ``.backward()``, default widths, 16 classes --
traced launch by launch (tests/train_trace.py) and held to two things:

(a) wiring: every operand of every launch equals, bit for bit, the output of the launch the network definition names (channel offsets,
    temb row blocks, which layer's statistics and sums, which half of a concat gradient), the required in-place reads and writes hold
    by address, and every parameter's ``.grad`` is the output of the launch the table ties it to;
(b) numerics: every recorded launch against the fp64 reference of its operation on the operands it read, within the bound the
    per-kernel tests derive (tests/fp64ref.py, glue_fp64ref.py, loss_fp64ref.py), chain lengths from the launcher mirrors, the mirrors
    pinned against the launchers' own workspace and form queries;
(c) the near-kink share of the InstanceNorm backward reference stays below 1e-4 wherever a channel row has >= 10^4 elements (it enters
    the bound: a large share would make the bound vacuous);
(d) one printed line per launch (label, kind, shape, points, |err| / bound) and the worst ratio per kind.

Pack launches (ConvPacks.run, the per-layer, transposed-convolution and fold packers) have no reference of their own here: their
outputs are wired to their consumers in (a), and each consumer's reference is evaluated on the fp32 PARAMETERS rounded as the packer
must round them, so a wrong packing fails at the convolution that read it (the fold's composed weights are decoded and checked).

Two cases, the smallest shapes that reach every route.  ``even-64``: N = 1, 64^3 with ops.TRAIN_FOLD_MIN_TILES lowered -- the folded
forward and conv3d_k3_dgrad_reduce; the sets of blocks that took them must equal what ops.upconv_supported /
ops.conv3d_k3_dgrad_reduce_supported answer and be non-empty.  ``odd-b2``: N = 2, (33, 35, 40), timesteps 37 and 811, samples of
different scale -- floor pooling, replicate-padded transposed convolutions and their backward, the odd max-pool backward, two sample
rows in every temb block, per-sample statistics.

Two loss scales.  ``test_training_step_wiring_and_every_launch_in_fp64`` seeds the backward with 2^22: the output gradients of every
level are in fp16's normal range, and the bounds are the ones the per-kernel tests derive, without the term below.
``test_training_step_at_the_trainers_initial_loss_scale`` seeds it with NativeConvTrainer's own default ``init_scale`` (2^12, read
from the signature), the regime every fp16 run starts in: the output gradients of the two deepest levels (4^3, 2^3 voxels) are then
fp16 SUBNORMALS throughout (mean |dy| 3e-7 and 5e-8), and the share of subnormal dy is printed with every weight-gradient, data-
gradient, transposed-convolution-backward and head-backward row.  fp64ref's accumulation rule alone does not hold there: the fetch-once
weight gradient of those layers lands up to 1.07 (even-64, enc.down_4.conv_1) and 2.89 (odd-b2, down_4.conv_1) times the old bound,
because the matrix instruction aligns its products by exponent FIELD and a subnormal operand sits up to 10 bits below its field.
tests/test_mfma_model_gpu.py measures that on the instruction (24 places below the largest nominal exponent of a step of 8 products
arrive, the 25th does not) and fp64ref's ``nominal=`` term turns it into a derived part of the bound (fp64ref's module docstring);
the backward MFMA launches (dgrad, dgrad_reduce, wgrad, deconv_bwd, head_bwd) are held to the bound with that term, every other
launch to the same bound as at 2^22, and nothing overflows (a non-finite value has ratio inf).

Measured worst |err| / bound per kind (even-64; odd-b2), records: conv .992 .992, fold .755, mat .998 .999, deconv .993 .993, head_fwd
.987 .990, loss_reduce .352 .570, loss_grad .997 .995, head_bwd .998 .998, pool_bwd .999 .999, norm_bwd .998 .998, dgrad .914 .924,
dgrad_reduce .910, wgrad .204 .138, deconv_bwd .966 .901, bias_stats .053 .090, bias_sums .993 .969, temb_fwd .404 .430, temb_bwd .998
.961, to_cl .999 .999; near-kink share at most 1.2e-7 (enc.conv_0.conv_1) and 5.1e-7 (upcat_1.conv_0), zero in every other layer.
At the trainer's scale, the backward kinds: head_bwd .991 .974, pool_bwd .940 .982, norm_bwd .999 .996, dgrad .880 .894, dgrad_reduce
.867, wgrad .159 .128, deconv_bwd .935 .783, loss_grad .935 .980, temb_bwd .999 .969; subnormal dy per layer 0.3 .. 0.95 (even-64)."""
import ctypes
import time
import zlib

import pytest
import torch

import fp64ref as R
import glue_fp64ref as GR
import loss_fp64ref as LR
import train_trace as TT

pytestmark = pytest.mark.gpu

F16, F32 = torch.float16, torch.float32
CLASSES = 16
SCALE = 2.0 ** 22
CASES = {"even-64": dict(N=1, dims=(64, 64, 64), t=(417,), fold_min_tiles=1, seed=11),
         "odd-b2": dict(N=2, dims=(33, 35, 40), t=(37, 811), fold_min_tiles=None, seed=12)}
NEAR_CAP, NEAR_MIN_ROW = 1e-4, 10 ** 4
DECONV_FORM = {0: "one_tap", 1: "ksplit", 2: "alltaps"}


def _net(seed):
    from diff_unet_amos_amd.diff_unet import DiffUNet
    torch.manual_seed(seed)
    net = DiffUNet(in_channels=1, out_channels=CLASSES)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for n, p in net.named_parameters():
            if ".adn.N.weight" in n:
                p.copy_(torch.rand(p.shape, generator=g) + 0.5)                       # gamma around 1 +- 0.5
            elif ".adn.N.bias" in n:
                p.copy_(torch.randn(p.shape, generator=g) * 0.2)                      # beta around +- 0.2
            elif n.endswith(".bias"):                                                 # conv, deconv, head, temb biases
                p.copy_(torch.randn(p.shape, generator=g) * 0.1)
    return net.cuda()


def _inputs(case):
    c = CASES[case]
    N, dims = c["N"], c["dims"]
    g = torch.Generator().manual_seed(c["seed"])
    image = torch.rand(N, 1, *dims, generator=g)
    labels = (torch.rand(N, CLASSES, *dims, generator=g) > 0.8).float()
    x_t = torch.randn(N, CLASSES, *dims, generator=g)
    for n in range(1, N):                                  # samples of different scale
        image[n] *= 1 - 0.4 * n
        x_t[n] = x_t[n] * (1 + 0.5 * n) + 0.25 * n
    return image.cuda(), x_t.cuda(), torch.tensor(c["t"], dtype=torch.int64).cuda(), labels.cuda()


def _level_dims(dims, level):
    return tuple(s >> level for s in dims)


def _expected_routes(table, N, dims, fold_on):
    """(blocks whose first convolution may fold, blocks whose conv_1 data gradient may take the reduce along): the launchers' own
    queries over the shapes the network definition gives, nothing read from training.py's decisions."""
    from diff_unet_amos_amd import ops
    fold, reduce = set(), set()
    for b in table.up:
        D, H, W = _level_dims(dims, b.level)
        cin_d, up, cat = table.deconv[b.name]
        if fold_on and D % 8 == 0 and H % 8 == 0 and W % 8 == 0 and ops.upconv_supported(F16, N, D, H, W, cat, cat + up, cin_d, cin_d, b.cout, b.cout):
            fold.add(b.name)
    for b in table.blocks:
        D, H, W = _level_dims(dims, b.level)
        if ops.conv3d_k3_dgrad_reduce_supported(F16, N, D, H, W, b.cout, b.cout):
            reduce.add(b.name)
    return fold, reduce


# ---- per-launch references ------------------------------------------------------------------------------------------------------------------
class _Ctx:
    def __init__(self, case, table, net, nominal=False):
        from diff_unet_amos_amd import _native as nv
        from diff_unet_amos_amd import ops
        self.case, self.table, self.ops, self.nv = case, table, ops, nv
        self.nominal = nominal             # bounds of the backward MFMA launches with fp64ref's term for subnormal fp16 operands
        self.params = {n: p.detach() for n, p in net.named_parameters()}
        self.prefix = {f"{b.name}.{c}": f"{b.prefix}.{c}" for b in table.blocks for c in ("conv_0", "conv_1")}
        self.rows, self.near, self._pts, self.spent = [], [], {}, {}

    def p(self, layer, what):
        return self.params[f"{self.prefix[layer]}.{what}"]

    def pts(self, N, dims):
        """Every voxel of a small volume, the structured sample of fp64ref.sample_voxels (both faces of every axis of every sample,
        tile and slab edges) above 1024 voxels per sample; one set per (N, dims), shared by the launches of a level."""
        key = (N, tuple(dims))
        if key not in self._pts:
            if dims[0] * dims[1] * dims[2] <= 1024:
                self._pts[key] = R.all_voxels(N, dims)
            else:
                self._pts[key] = R.sample_voxels(N, dims, n_random=300, seed=zlib.crc32(f"{self.case}/{key}".encode()))
        return self._pts[key]

    def row(self, r, what, shape, n, res):
        self.rows.append(dict(label=r.label + (f" {what}" if what else ""), kind=r.kind, shape=shape, n=n, ratio=res.ratio, res=res))


def _dev_contract(A, Wm, bias):
    """fp64ref.conv3_ref's three sums with the GEMMs on the device (the operands gathered by fp64ref.gather_taps)"""
    ref, ab, sq = R.contract(A.reshape(A.shape[0], -1).cuda(), Wm.cuda())
    b = bias.detach().double().cuda()[None]
    return (ref + b).cpu(), (ab + b.abs()).cpu(), sq.cpu()


def _stats_ratio(c, y, stats):
    N, cout = y.shape[0], y.shape[-1]
    v = y.reshape(N, -1, cout).double()
    S, Q, A = v.sum(1).cpu(), (v * v).sum(1).cpu(), v.abs().sum(1).cpu()
    words = c.ops.stats_decode(stats).cpu()[:, :cout]
    bs, bq = R.stats_bound(A, Q, F16, v.shape[1])
    return R.check(torch.stack([words[..., 0], words[..., 1]]), torch.stack([S, Q]), torch.stack([bs, bq]))


def _sub(t):
    """share of subnormal elements of an fp16 gradient operand, for the printed rows"""
    return f"dy-subnormal={R.subnormal_share(t):.2f}"


def _conv_like(c, r, x, y, w, bias, cin, cout, cs_in, cs_out, stats=None, gradient=False):
    """A 3x3x3 convolution launch (forward, or the data gradient = the forward kernel on flipped, transposed weights): sampled
    outputs against gather_taps + conv3_ref within R.bound, split-K partials from the launcher's own form.  ``gradient``: x is a
    gradient operand (its subnormal share is printed; with c.nominal the bound has the term for subnormal operands)."""
    ops, nv = c.ops, c.nv
    N, D, H, W = r.meta["dims"][:4]
    d = nv.Conv3Desc(nv.dt_code(F16), N, D, H, W, cin, cs_in, r.meta.get("cin_off", 0), cout, cs_out, r.meta.get("cout_off", 0), 0, 0, 0,
                     ops.CONV_POLICY)
    split = r.kind != "dgrad_reduce" and ops.conv3_form(d, False, r.meta["ws_bytes"]).ksplit > 1
    pts = c.pts(N, (D, H, W))
    A, _ = R.gather_taps(x, pts, 0, cin)
    Wm = R.conv3_weights(w, F16)
    ref, ab, sq = _dev_contract(A, Wm, bias)
    parts = 3 * -(-cin // ops.chunk_elems(F16)) if split else 0
    nom = R.nominal_sum(A.reshape(A.shape[0], -1).cuda(), Wm.cuda()).cpu() if gradient and c.nominal else None
    bnd = R.bound(ref, ab, sq, R.chain_length(27 * cin, F16, parts), F16, nominal=nom)
    res = R.check(R.gather_points(y, pts, 0, cout), ref, bnd, pts)
    what = " ".join((["split"] if split else []) + ([_sub(x[..., :cin])] if gradient else []))
    c.row(r, what, f"{N}x{D}x{H}x{W} {cin}->{cout}", len(pts), res)
    if stats is not None:
        c.row(r, "stats", f"{N}x{cout}", N * cout * 2, _stats_ratio(c, y, stats))


def chk_conv(c, r):
    layer = r.label.split("/")[0]
    w, cin = c.p(layer, "conv.weight"), r.meta["cin"]
    wp = torch.zeros((w.shape[0], cin, 3, 3, 3), device=w.device)
    wp[:, :w.shape[1]] = w                                 # a first layer's 1 / 17 channels in a buffer padded to 8 / 24: zero weights
    _conv_like(c, r, r.ins["x"].t, r.outs["raw"].t, wp, c.p(layer, "conv.bias"), cin, r.meta["cout"], r.meta["cs_in"], r.meta["cs_out"],
               stats=r.outs["stats"].t)


def chk_dgrad(c, r):
    layer = r.label.split("/")[0]
    w = c.p(layer, "conv.weight")
    wd = w.flip(2, 3, 4).transpose(0, 1).contiguous()
    cin, cout = r.meta["cin"], r.meta["cout"]
    assert tuple(wd.shape[:2]) == (cout, cin), (wd.shape, cin, cout)
    r.meta.setdefault("ws_bytes", 0)
    _conv_like(c, r, r.ins["dy"].t, r.outs["dx"].t, wd, torch.zeros(cout), cin, cout, r.meta.get("cs_in", cin), r.meta.get("cs_out", cout),
               gradient=True)


def chk_fold(c, r):
    layer = r.label.split("/")[0]
    up = layer.split(".")[0]
    N, D, H, W = r.meta["dims"][:4]
    cskip, cu, cout = r.meta["cskip"], r.meta["cu"], r.meta["cout"]
    xs, un = r.ins["xs"].t, r.ins["u"].t
    pts = c.pts(N, (D, H, W))
    A, _ = R.gather_taps(xs, pts, 0, cskip)
    par, ok, phi, deltas = R.fold_parents(pts, (D, H, W))
    lim = torch.tensor([D // 2 - 1, H // 2 - 1, W // 2 - 1])
    pc = torch.minimum(par.clamp_min(0), lim).to(un.device)
    nn_ = pts[:, None, 0].expand_as(ok).to(un.device)
    U = un[nn_, pc[..., 0], pc[..., 1], pc[..., 2], :cu].cpu().double()
    wc, bc = c.p(layer, "conv.weight").float().cpu(), c.p(layer, "conv.bias")
    wd, bd = c.params[f"model.{up}.upsample.deconv.weight"].float().cpu(), c.params[f"model.{up}.upsample.deconv.bias"]
    Wp = R.decode_fold_weights(r.ins["wu"].t, cout, cu)
    for k, (m, mabs) in R.compose_fold(wc[:, cskip:], wd[:cu]).items():       # the packer's composed weights: fp64 composition, one fp16 rounding
        res = R.check(Wp[k], m, R.U16 * m.abs() + R.FLOOR16 + R.U32 * (8 * m.shape[1] + 1) * mabs)
        assert res.ratio <= 1, f"{r.label}: composed weights {k}: {res}"
    rows, arows = R.fold_bias_table(wc[:, cskip:], bc, bd)
    cls = R.border_class(pts, (D, H, W))
    ref, ab, sq = R.fold_ref(A, R.conv3_weights(wc[:, :cskip], F16), U, ok, phi, deltas, Wp, rows[cls], arows[cls])
    cmid = wc.shape[1] - cskip
    bnd = R.bound(ref, ab, sq, R.chain_length(27 * cskip + 8 * cu, F16), F16, extra=R.U32 * (27 * cmid + 1) * arows[cls])
    y = r.outs["raw"].t
    c.row(r, "", f"{N}x{D}x{H}x{W} {cskip}+{cu}->{cout}", len(pts), R.check(R.gather_points(y, pts, 0, cout), ref, bnd, pts))
    c.row(r, "stats", f"{N}x{cout}", N * cout * 2, _stats_ratio(c, y, r.outs["stats"].t))


def _consts(c, r, N, C):
    """fp32 scale / shift as the consumers' preamble forms them, held to fp64 from the statistics words; the add rows"""
    ops = c.ops
    stats, gamma, beta = r.ins["stats"].t, r.ins["gamma"].t, r.ins["beta"].t
    norm = ops.Norm(stats, gamma, beta, r.meta["count"])
    sc64, sh64, b_sc, b_sh = R.finalize(ops.stats_decode(stats).cpu(), gamma.cpu(), beta.cpu(), r.meta["count"], r.meta["eps"])
    sc, sh = (t.cpu() for t in ops.instnorm_finalize(norm, N, C))
    for what, got, ref, b in (("scale", sc, sc64, b_sc), ("shift", sh, sh64, b_sh)):
        res = R.check(got, ref, b)
        assert res.ratio <= 1, f"{r.label}: InstanceNorm {what} of the preamble: {res}"
    ad = r.ins["add"].t.reshape(N, C).cpu() if "add" in r.ins else torch.zeros(N, C)
    return sc, sh, ad


def chk_mat(c, r):
    raw, out = r.ins["raw"].t, r.outs["act"].t
    N, D, H, W, C = raw.shape
    sc, sh, ad = _consts(c, r, N, C)
    emb = r.ins["emb"].t if "emb" in r.ins else None

    def ref_at(p):
        n = p[:, 0]
        e = R.gather_points(emb, p, 0, C) if emb is not None else None
        return R.materialize_ref(R.gather_points(raw, p, 0, C), sc[n], sh[n], ad[n], e)

    pts = c.pts(N, (D, H, W))
    ref, mag = ref_at(pts)
    c.row(r, "", f"{N}x{D}x{H}x{W} {C}", len(pts), R.check(R.gather_points(out, pts, 0, C), ref, R.materialize_bound(ref, mag, F16), pts))
    if "pooled" in r.outs:               # floor pooling: max of the rounded outputs = rounding of the max, the window's largest bound
        pp = c.pts(N, (D // 2, H // 2, W // 2))
        best = bnd = None
        for k in range(8):
            q = pp.clone()
            q[:, 1:] = 2 * q[:, 1:] + torch.tensor([k >> 2, (k >> 1) & 1, k & 1])
            v, m = ref_at(q)
            b = R.materialize_bound(v, m, F16)
            best = v if best is None else torch.maximum(best, v)
            bnd = b if bnd is None else torch.maximum(bnd, b)
        c.row(r, "pool", f"{N}x{D // 2}x{H // 2}x{W // 2} {C}", len(pp), R.check(R.gather_points(r.outs["pooled"].t, pp, 0, C), best, bnd, pp))


def chk_deconv(c, r):
    nv = c.nv
    up = r.label.split("/")[0]
    m = r.meta
    N, D, H, W = m["dims"][:4]
    cin, cout, out_dims = m["cin"], m["cout"], m["out_dims"]
    d = nv.Conv3Desc(nv.dt_code(F16), N, D, H, W, cin, m["cs_in"], m["cin_off"], cout, m["cs_out"], m["cout_off"], 0, 0, 0, c.ops.CONV_POLICY)
    f = nv.DeconvForm()
    nv.check(nv.lib().dua_deconv_k2s2_form(ctypes.byref(d), 0, *out_dims, ctypes.byref(f)), "dua_deconv_k2s2_form")
    form = DECONV_FORM[f.kernel]
    w, b = c.params[f"model.{up}.upsample.deconv.weight"], c.params[f"model.{up}.upsample.deconv.bias"]
    pts = c.pts(N, out_dims)
    parent, child = R.deconv_sources(pts, (D, H, W))
    A = R.gather_points(r.ins["x"].t, parent, 0, cin)
    ref, ab, sq = R.deconv_ref_by_child(A, w, b, F16, child)
    bnd = R.bound(ref, ab, sq, R.deconv_fwd_chain(form, cin, F16), F16)
    res = R.check(R.gather_points(r.outs["y"].t, pts, 0, cout), ref, bnd, pts)
    c.row(r, form, f"{N}x{D}x{H}x{W} {cin}->{cout} -> {'x'.join(map(str, out_dims))}", len(pts), res)


def chk_head_fwd(c, r):
    u, out = r.ins["u"].t, r.outs["out"].t
    N, D, H, W, C = u.shape
    K = out.shape[-1]
    pts = c.pts(N, (D, H, W))
    ref, ab, sq = R.head_fwd_ref(R.gather_points(u, pts, 0, C), r.ins["weight"].t.reshape(K, C), r.ins["bias"].t, F16)
    bnd = R.bound(ref, ab, sq, R.head_fwd_chain(C, F16), F16)
    c.row(r, R.head_fwd_route(C, F16), f"{N}x{D}x{H}x{W} {C}->{K}", len(pts), R.check(R.gather_points(out, pts, 0, K), ref, bnd, pts))


def chk_loss_reduce(c, r):
    logits, labels = r.ins["logits"].t, r.ins["labels"].t
    N, C = labels.shape[:2]
    V = labels[0, 0].numel()
    ref = LR.reduce_ref(logits, labels)
    sums = r.outs["sums"].t
    c.row(r, "sums", f"{N}x{C}x{V}", sums.numel(), LR.check(sums, LR.ref_sums(ref), LR.reduce_bound(ref)))
    wL, wdc = LR.finish_ref(sums, N, C, V, r.meta["names"], r.meta["combine"], None)
    c.row(r, "L", "", 1, LR.check(r.outs["L"].t.cpu().reshape(1), wL.reshape(1), LR.finish_bound(wL).reshape(1)))
    c.row(r, "dcomb", "", 1, LR.check(r.outs["dcomb"].t.cpu().reshape(1), wdc.reshape(1), LR.finish_bound(wdc).reshape(1)))


def chk_loss_grad(c, r):
    logits, labels = r.ins["logits"].t, r.ins["labels"].t
    C = labels.shape[1]
    gr = LR.grad_ref(logits, labels, r.ins["sums"].t, r.meta["g"], [float(n in r.meta["names"]) for n in LR.LOSS_NAMES])
    got, pad = LR.grad_rows(r.outs["out"].t, C)
    c.row(r, "", f"{tuple(got.shape)} g={r.meta['g']:g}", got.numel(), LR.check(got, gr["ref"], LR.grad_bound(gr, F16)))
    c.row(r, "padding", "", pad.numel(), LR.check_padding(pad))


def chk_head_bwd(c, r):
    dl, u, w = r.ins["dlogits"].t, r.ins["u"].t, r.ins["weight"].t
    K, C = w.shape
    V = u.numel() // C
    c_du, c_w = R.head_bwd_chains(V, F16, mfma=True)
    ud, dld = u.double().reshape(V, C), dl.double().reshape(V, K)
    wq = w.half().double()                                 # the MFMA path multiplies fp16 weights
    ref_du = dld @ wq
    t_du = t_w = t_b = None
    if c.nominal:                                          # three MFMA contractions over dlogits (db multiplies by ones)
        t_du = R.nominal_sum(dld, wq)
        t_w = R.subnormal_term(R.nominal_sum(dld.t(), ud)) * (1 + R.U32)
        t_b = R.subnormal_term(R.nominal_sum(dld.t(), torch.ones_like(ud[:, :1]))[:, 0]) * (1 + R.U32)
    c.row(r, f"du {_sub(dl)}", f"{V}x{K}->{C}", V * C,
          R.check(r.outs["du"].t.reshape(V, C), ref_du, R.bound(ref_du, dld.abs() @ wq.abs(), None, c_du, F16, nominal=t_du)))
    ref_w, ab_w = dld.t() @ ud, dld.abs().t() @ ud.abs()
    c.row(r, "dW", f"{K}x{C}", K * C, R.check(r.outs["dW"].t, ref_w, R.U32 * c_w * ab_w * (1 + R.U32) + R.FLOOR32 + (0.0 if t_w is None else t_w)))
    c.row(r, "db", f"{K}", K, R.check(r.outs["db"].t, dld.sum(0), R.U32 * c_w * dld.abs().sum(0) * (1 + R.U32) + R.FLOOR32 + (0.0 if t_b is None else t_b)))


def chk_pool_bwd(c, r):
    """out = dA + dP routed to the first maximum of each 2x2x2 window (floor pooling: a trailing odd plane gets dA only), one rounding"""
    act, dA, dP = r.ins["act"].t, r.ins["dA"].t, r.ins["dP"].t
    N, D, H, W, C = act.shape
    hd, hh, hw = D // 2, H // 2, W // 2
    a = act[:, :2 * hd, :2 * hh, :2 * hw].reshape(N, hd, 2, hh, 2, hw, 2, C).permute(0, 1, 3, 5, 2, 4, 6, 7).reshape(N, hd, hh, hw, 8, C)
    first = a.double().argmax(4)                           # torch's rule: the first maximum in (d, h, w) raster order
    routed = torch.zeros((N, hd, hh, hw, 8, C), dtype=torch.float64, device=act.device)
    routed.scatter_(4, first.unsqueeze(4), dP.double().unsqueeze(4))
    routed = routed.reshape(N, hd, hh, hw, 2, 2, 2, C).permute(0, 1, 4, 2, 5, 3, 6, 7).reshape(N, 2 * hd, 2 * hh, 2 * hw, C)
    ref = dA.double().clone()
    ref[:, :2 * hd, :2 * hh, :2 * hw] += routed
    u_out, floor = R.unit(F16)
    c.row(r, "odd" if (D % 2 or H % 2 or W % 2) else "", f"{N}x{D}x{H}x{W} {C}", ref.numel(), R.check(r.outs["out"].t, ref, u_out * ref.abs() + floor))


def chk_norm_bwd(c, r):
    """tests/test_backward_fp64.py::_check_in_bwd on the recorded operands: the reduce sums (this launch's own pass, or the ones the
    data-gradient launch took along), dY, dgamma, dbeta and the dadd rows"""
    ops = c.ops
    dA, raw = r.ins["dA"].t, r.ins["raw"].t
    N, D, H, W, C = raw.shape
    V = D * H * W
    given = "sums" in r.ins
    sums = r.ins["sums"].t if given else r.outs["sums"].t
    chain = R.DGRAD_REDUCE_CHAIN if given else R.in_bwd_reduce_chain(C, V, F16)
    ref = R.in_bwd_ref(dA.reshape(N, V, C), raw.reshape(N, V, C), ops.stats_decode(r.ins["stats"].t), r.ins["gamma"].t, r.ins["beta"].t, V,
                       eps=r.meta["eps"])
    b0, b1, b2 = R.in_bwd_sums_bound(ref, chain)
    got = sums.sum(1)[:, :C, :3]
    shape = f"{N}x{V}x{C}"
    tag = "dgrad-sums " if given else ""
    for j, (s, b) in enumerate(((ref["S0"], b0), (ref["S1"], b1), (ref["S2"], b2))):
        c.row(r, f"{tag}S{j}", shape, N * C, R.check(got[..., j], s, b))
    near = ref["near"].double().mean().item()
    c.near.append((r.label, V, near))
    c.row(r, "dY", shape, N * V * C, R.check(r.outs["dY"].t.reshape(N, V, C), ref["dY"], R.in_bwd_dy_bound(ref, b1, b2, F16)))
    # the apply launch rounds the kernel's fp64 sums to fp32 (dadd: per sample) and adds the samples with fp32 atomics
    for name, s, b in (("dbeta", ref["S1"], b1), ("dgamma", ref["S2"], b2)):
        bnd = (b + R.U32 * s.abs()).sum(0) * (1 + N * R.U32) + N * R.U32 * s.abs().sum(0) + R.FLOOR32
        c.row(r, name, f"{C}", C, R.check(r.outs[name].t, s.sum(0), bnd))
    if "dadd" in r.outs:
        c.row(r, "dadd", f"{N}x{C}", N * C, R.check(r.outs["dadd"].t.reshape(N, C), ref["S0"], b0 + R.U32 * ref["S0"].abs() + R.FLOOR32))


def chk_wgrad(c, r):
    nv = c.nv
    m = r.meta
    N, D, H, W = m["dims"][:4]
    cin, cout = m["cin"], m["cout"]
    dw, dw0 = r.outs["dw"].t, m["dw0"]
    assert not m["perm"] and not bool(dw0.any())
    cin_src = dw.shape[1]
    ref, ab, *nom = R.wgrad_ref(r.ins["x"].t, 0, cin, r.ins["dy"].t, 0, cout, cin_src=cin_src, nominal=c.nominal)
    P, combos, total = R.wgrad_fo_partitions(N, D, H, W, cin, cout, 0)
    route = R.wgrad_fo_route(combos, None)
    d = nv.Conv3Desc(nv.dt_code(F16), N, D, H, W, cin, m["cs_in"], 0, cout, m["cs_out"], 0, 0, 0, 0, c.ops.WGRAD_POLICY)
    ws = int(nv.lib().dua_conv3d_k3_wgrad_workspace(ctypes.byref(d)))
    assert ws == P * combos * 27 * 2048 * 4, f"{r.label}: partition mirror drifted from the launcher: {ws} vs P={P} combos={combos}"
    bnd = R.wgrad_bound(ref, ab, dw0, R.wgrad_fo_chain(P, total, route), nominal=nom[0] if nom else None)
    res = R.check(dw.double(), dw0.double() + ref, bnd)
    dy = r.ins["dy"].t
    sub = float(((dy != 0) & (dy.abs() < 2.0 ** -14)).float().mean())
    term = f" sub-term={float((R.subnormal_term(nom[0]) / bnd).mean()):.2f}" if nom else ""       # its mean share of the bound
    c.row(r, f"fo-{route} P={P} dy-subnormal={sub:.2f}{term}", f"{N}x{D}x{H}x{W} {cin}({cin_src})->{cout}", dw.numel(), res)


def chk_deconv_bwd(c, r):
    nv = c.nv
    m = r.meta
    N, D, H, W = m["dims"][:4]
    cin, cout = m["cin"], m["cout"]
    xs, dy, w = r.ins["x"].t, r.ins["dy"].t, r.ins["w"].t
    padded = tuple(dy.shape[1:4]) != (2 * D, 2 * H, 2 * W)
    c_dx, c_dw, P = R.deconv_bwd_chains(N, D, H, W, cin, cout, F16)
    d = nv.Conv3Desc(nv.dt_code(F16), N, D, H, W, cin, m["cs_in"], m["cin_off"], cout, m["cs_out"], m["cout_off"])
    combos = -(-cin // 64) * -(-cout // 64)
    ws = int(nv.lib().dua_deconv_k2s2_bwd_workspace(ctypes.byref(d)))
    assert ws == P * combos * 8 * 4096 * 4, f"{r.label}: partition mirror drifted from the launcher: {ws} vs P={P} combos={combos}"
    dyf = R.deconv_fold_dy(dy, D, H, W)
    ref, ab, sq, rw, aw = R.deconv_bwd_ref(xs, dyf, w, F16)
    shape = f"{N}x{D}x{H}x{W} {cin}<-{cout}{' padded' if padded else ''}"
    ndx, ndw = R.deconv_bwd_nominal(xs, dyf, w, padded) if c.nominal else (None, None)
    c.row(r, f"dx {_sub(dy)}", shape, ref.numel(),
          R.check(r.outs["dx"].t, ref, R.bound(ref, ab, sq, c_dx, F16, emulated_in=F16 if padded else None, nominal=ndx)))
    b2 = R.U32 * c_dw * aw * (1 + R.U32) + R.FLOOR32
    if c.nominal:
        b2 = b2 + R.subnormal_term(ndw) * (1 + R.U32)
    if padded:        # the folded dy operand is summed and rounded once: an emulated input, covered by the RSS term
        A2 = (dyf * dyf).reshape(N, D, 2, H, 2, W, 2, cout).permute(0, 1, 3, 5, 2, 4, 6, 7).reshape(-1, 8 * cout)
        ssq = ((xs.double().reshape(-1, cin) ** 2).t() @ A2).reshape(cin, 2, 2, 2, cout).permute(0, 4, 1, 2, 3).contiguous()
        b2 = b2 + R.C_RSS * R.U16 * ssq.sqrt()
    c.row(r, f"dw P={P}", shape, rw.numel(), R.check(r.outs["dw"].t, rw, b2))


def chk_bias_stats(c, r):
    """dua_instnorm_stats (fp16): a thread adds its voxels in fp32 (the reduce pass's geometry: in_bwd_reduce_chain), blocks and
    replicas in fp64; one fixed-point conversion (2^-44) per block and channel, at most 1024 blocks."""
    x, st = r.ins["x"].t, r.outs["stats"].t
    N, C = x.shape[0], x.shape[-1]
    v = x.reshape(N, -1, C).double()
    chain = R.in_bwd_reduce_chain(C, v.shape[1], F16)
    words = c.ops.stats_decode(st)[:, :C]
    ref = torch.stack([v.sum(1), (v * v).sum(1)])
    bnd = torch.stack([R.U32 * chain * v.abs().sum(1), R.U32 * (chain + 1) * (v * v).sum(1)]) + 1024 * 2.0 ** -43
    c.row(r, "", f"{N}x{v.shape[1]}x{C}", 2 * N * C, R.check(torch.stack([words[..., 0], words[..., 1]]), ref, bnd))


def chk_bias_sums(c, r):
    C = r.meta["c"]
    ref, bnd = GR.stats_channel_sums_ref(r.ins["stats"].t, C)
    c.row(r, "", f"{C}", C, GR.check(r.outs["out"].t, ref, bnd))


def _temb_lists(r, what, n=9):
    return [r.ins[f"{what}{i}"].t for i in range(n)]


def chk_temb_fwd(c, r):
    half = r.meta["half"]
    i = r.ins
    hid = i["w1"].t.shape[0]
    freqs = c.ops.temb_freqs(half, i["t"].t.device)
    assert torch.equal(freqs.cpu(), GR.temb_freqs(half))
    ref = GR.temb_fwd_ref(i["t"].t, freqs, i["w0"].t, i["b0"].t, i["w1"].t, i["b1"].t, _temb_lists(r, "pw"), _temb_lists(r, "pb"), r.outs["saved"].t)
    for k, res in GR.temb_fwd_checks(r.outs["add"].t, r.outs["saved"].t, ref, half, hid).items():
        c.row(r, k, f"N={i['t'].t.numel()}", ref[k][0].numel(), res)


def chk_temb_bwd(c, r):
    half = r.meta["half"]
    got = dict(dz2=r.meta["dz2"], dw0=r.outs["dw0"].t, db0=r.outs["db0"].t, dw1=r.outs["dw1"].t, db1=r.outs["db1"].t,
               dw=[r.outs[f"pdw{i}"].t for i in range(9)], db=[r.outs[f"pdb{i}"].t for i in range(9)])
    ref = GR.temb_bwd_ref(r.ins["dadd"].t, r.ins["w1"].t, _temb_lists(r, "pw"), r.ins["saved"].t, half, dz2=got["dz2"])
    for k, res in GR.temb_bwd_checks(got, ref).items():
        c.row(r, k, f"N={r.ins['saved'].t.shape[0]}", 0, res)


def chk_to_cl(c, r):
    """NCDHW fp32 -> channels-last fp16, zero fill: one rounding"""
    parts = [r.ins[k].t for k in sorted(r.ins)]
    out = r.outs["out"].t
    src = torch.cat(parts, 1).permute(0, 2, 3, 4, 1).double()
    ref = torch.zeros(out.shape, dtype=torch.float64, device=out.device)
    ref[..., :src.shape[-1]] = src
    c.row(r, "", f"{tuple(out.shape)}", out.numel(), R.check(out, ref, R.U16 * ref.abs() + R.FLOOR16))


CHECKS = dict(conv=chk_conv, fold=chk_fold, mat=chk_mat, deconv=chk_deconv, head_fwd=chk_head_fwd, loss_reduce=chk_loss_reduce,
              loss_grad=chk_loss_grad, head_bwd=chk_head_bwd, pool_bwd=chk_pool_bwd, norm_bwd=chk_norm_bwd, dgrad=chk_dgrad,
              dgrad_reduce=chk_dgrad, wgrad=chk_wgrad, deconv_bwd=chk_deconv_bwd, bias_stats=chk_bias_stats, bias_sums=chk_bias_sums,
              temb_fwd=chk_temb_fwd, temb_bwd=chk_temb_bwd, to_cl=chk_to_cl)
WIRED_ONLY = {"pack_batch", "pack", "pack_deconv", "pack_fold", "external"}


@pytest.mark.parametrize("case", list(CASES))
def test_training_step_wiring_and_every_launch_in_fp64(case, monkeypatch):
    _step_in_fp64(case, monkeypatch, SCALE, nominal=False)


@pytest.mark.parametrize("case", list(CASES))
def test_training_step_at_the_trainers_initial_loss_scale(case, monkeypatch):
    """The same step, wiring and per-launch checks with the backward seeded at NativeConvTrainer's own default ``init_scale``: the
    gradient operands of the deep levels are fp16 subnormals, and the backward MFMA launches are held to their bounds with
    fp64ref's term for such operands."""
    import inspect

    from diff_unet_amos_amd.training import NativeConvTrainer
    scale = inspect.signature(NativeConvTrainer.__init__).parameters["init_scale"].default
    assert isinstance(scale, float) and 1.0 < scale < SCALE
    _step_in_fp64(case, monkeypatch, scale, nominal=True)


def _step_in_fp64(case, monkeypatch, scale, nominal):
    from diff_unet_amos_amd import _native as nv
    from diff_unet_amos_amd import ops
    from diff_unet_amos_amd.training import _SegLoss, native_logits_cl
    spec = CASES[case]
    N, dims = spec["N"], spec["dims"]
    t0 = time.time()
    nv.prepare(torch.device("cuda", 0))
    if spec["fold_min_tiles"] is not None:
        monkeypatch.setattr(ops, "TRAIN_FOLD_MIN_TILES", spec["fold_min_tiles"])
    net = _net(spec["seed"])
    fold, reduce = _expected_routes(TT.Table(), N, dims, spec["fold_min_tiles"] is not None)
    table = TT.Table(fold=fold, reduce=reduce)
    image, x_t, t, labels = _inputs(case)
    with TT.Tracer(net, table) as tr:
        tr.begin(image=image, x_t=x_t, t=t, labels=labels)
        logits = native_logits_cl(net, image, x_t, t, F16)
        loss = _SegLoss.apply(logits, labels)
        (loss * scale).backward()
    torch.cuda.synchronize()
    trace = tr.trace
    grads = {n: p.grad for n, p in net.named_parameters()}
    t_step = time.time() - t0

    # ---- the routes: what ran folded / with the reduce along equals the launchers' answers -----------------------------------------
    by = {r.label: r for r in trace}
    folded = {r.label.split(".")[0] for r in trace if r.kind == "fold"}
    reduced = {r.label.split(".conv_1/")[0] for r in trace if r.kind == "dgrad_reduce"}
    print(f"\n[{case}] backward seeded with {scale:g}; {len(trace) - 2} launches recorded in {t_step:.1f} s; folded {sorted(folded)} (queries: {sorted(fold)}); "
          f"reduce along {sorted(reduced)} (queries: {sorted(reduce)})")
    assert folded == fold and reduced == reduce, (folded, fold, reduced, reduce)
    if case == "even-64":
        assert fold and reduce, "the case is meant to reach the folded forward and conv3d_k3_dgrad_reduce"
    # ---- (a) wiring --------------------------------------------------------------------------------------------------------------
    findings = TT.verify(table, trace, grads)
    for f in findings:
        print("  wiring:", f)
    tied = sum(1 for n, w in table.grads.items() if grads.get(n) is not None)
    print(f"  wiring: {len(table.launches)} tabled launches, {sum(len(e.ins) for e in table.launches.values())} operands, "
          f"{len(table.aliases)} in-place requirements, {tied} of {len(grads)} parameters tied to a launch")
    assert not findings, findings
    assert tied == len(grads) == len(table.grads)
    # ---- (b) every launch against fp64 ------------------------------------------------------------------------------------------------
    c = _Ctx(case, table, net, nominal)
    errors = []
    for r in trace:
        if r.kind in WIRED_ONLY:
            continue
        t1 = time.time()
        try:
            CHECKS[r.kind](c, r)
        except Exception as exc:          # keep going: one run shows every launch
            errors.append(f"{r.label} ({r.kind}): {type(exc).__name__}: {exc}")
        c.spent[r.kind] = c.spent.get(r.kind, 0.0) + time.time() - t1
        r.ins, r.outs = {}, {}            # the clones of this launch are done with
    torch.cuda.synchronize()
    # ---- (d) the table ------------------------------------------------------------------------------------------------------------------
    print(f"  {'launch':<60} {'kind':<13} {'shape':<40} {'points':>9} {'err/bound':>10}  worst at")
    worst = {}
    for row in c.rows:
        print(f"  {row['label']:<60} {row['kind']:<13} {row['shape']:<40} {row['n']:>9} {row['ratio']:>10.4f}  {row['res'].where}")
        worst[row["kind"]] = max(worst.get(row["kind"], 0.0), row["ratio"])
    print(f"  [{case}] worst |err| / bound per kind: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())))
    # ---- (c) near-kink share ---------------------------------------------------------------------------------------------------------------
    print(f"  [{case}] near-kink share of the norm-backward reference per layer (elements per channel row): "
          + ", ".join(f"{l.split('/')[0]} {s:.1e} ({v})" for l, v, s in c.near))
    print(f"  [{case}] {time.time() - t0:.1f} s in all; references by kind: " + ", ".join(f"{k} {v:.1f}" for k, v in sorted(c.spent.items()) if v >= 0.05))
    assert not errors, errors
    assert set(worst) == set(CHECKS) - ({"fold"} if not fold else set()) - ({"dgrad_reduce"} if not reduce else set()), sorted(worst)
    checked = {row["label"].split(" ")[0] for row in c.rows}
    assert checked == {l for l, e in table.launches.items() if e.kind not in WIRED_ONLY}, "a launch went without a reference"
    bad = [(l, s) for l, v, s in c.near if v >= NEAR_MIN_ROW and not s < NEAR_CAP]
    assert not bad, f"near-kink share over {NEAR_CAP}: pick another seed: {bad}"
    over = [(row["label"], row["res"]) for row in c.rows if not row["ratio"] <= 1.0]
    assert not over, f"{case}: launches over their fp64 bound: {over}"
