"""Every launch of the shipped denoiser evaluation, at its real shape, layout and channel offsets, against an fp64 reference on the
operands it read (tests/fp64ref.py): Plan.denoiser_body() launched kernel by kernel -- the one place the launch sequence is
written down -- and the head in logits mode, with ops.conv3d_k3 / upconv_k3 / deconv_k2s2 / materialize / final_conv_sampler
wrapped so that each call is launched, synchronised, sampled on the device and checked per element against its bound, and the
InstanceNorm statistics words a convolution leaves against fp64 sums of what it stored.

Three plans at default widths (64, 64, 128, 256, 512, 64), 16 classes: the benchmarked fp16 96^3 patch; fp16 at batch 2 with
an odd extent (replicate-padded transposed convolutions, floor pooling, per-sample statistics rows); the exact-fp32 companion
plan the last DDPM steps run on, at 64^3.  Which kernel every launch takes is pinned below, as the policy is written today: a
policy change that moves a launch makes this test fail instead of quietly testing another kernel."""
import ctypes
import os
import zlib

import pytest
import torch

import fp64ref as R
import sampler_fp64ref as T

pytestmark = pytest.mark.gpu

FEATURES = (64, 64, 128, 256, 512, 64)
CLASSES = 16

# launch -> (kernel kind, split-K).  Convolutions: kinds of dua_conv3d_k3_kernel_kind ("v2", "first" = resident-weight first layer,
# "wide" = the wide-tile form); "fold" = dua_upconv_k3_fwd; "deconv<k>" = dua_deconv_k2s2_kernel_kind k; "mat" = materialise.
_ENC_FP16_96 = [("d0a", "first", False), ("d0b", "wide", False), ("m0", "mat", False),
                ("d1a", "v2", False), ("d1b", "v2", False), ("m1", "mat", False),
                ("d2a", "v2", False), ("d2b", "v2", False), ("m2", "mat", False),
                ("d3a", "v2", True), ("d3b", "v2", True), ("m3", "mat", False),
                ("d4a", "v2", True), ("d4b", "v2", True), ("m4", "mat", False)]
EXPECTED = {
    "fp16-96": dict(
        N=1, dims=(96, 96, 96), dtype=torch.float16, fold=[True, True, False, False], layout=(True, True, True),
        seq=_ENC_FP16_96 + [
            ("up3", "deconv1", False), ("u3a", "v2", True), ("u3b", "v2", True),
            ("up2", "deconv1", False), ("u2a", "v2", False), ("u2b", "v2", False),
            ("u1a", "fold", False), ("u1b", "v2", False),
            ("u0a", "fold", False), ("u0b", "wide", False), ("head", "tail", False)]),
    "fp16-b2-odd": dict(
        N=2, dims=(63, 48, 40), dtype=torch.float16, fold=[False, False, False, False], layout=(False, False, False),
        seq=[("d0a", "first", False), ("d0b", "v2", False), ("m0", "mat", False),
             ("d1a", "v2", False), ("d1b", "v2", False), ("m1", "mat", False),
             ("d2a", "v2", True), ("d2b", "v2", True), ("m2", "mat", False),
             ("d3a", "v2", True), ("d3b", "v2", True), ("m3", "mat", False),
             ("d4a", "v2", True), ("d4b", "v2", True), ("m4", "mat", False),
             ("up3", "deconv1", False), ("u3a", "v2", True), ("u3b", "v2", True),
             ("up2", "deconv1", False), ("u2a", "v2", True), ("u2b", "v2", True),
             ("up1", "deconv0", False), ("u1a", "v2", False), ("u1b", "v2", False),
             ("up0", "deconv0", False), ("u0a", "v2", False), ("u0b", "v2", False), ("head", "tail", False)]),
    "fp32-64": dict(
        N=1, dims=(64, 64, 64), dtype=torch.float32, fold=[False, False, False, False], layout=(False, False, False),
        seq=[("d0a", "v2", False), ("d0b", "v2", False), ("m0", "mat", False),
             ("d1a", "v2", False), ("d1b", "v2", False), ("m1", "mat", False),
             ("d2a", "v2", True), ("d2b", "v2", True), ("m2", "mat", False),
             ("d3a", "v2", True), ("d3b", "v2", True), ("m3", "mat", False),
             ("d4a", "v2", True), ("d4b", "v2", True), ("m4", "mat", False),
             ("up3", "deconv0", False), ("u3a", "v2", True), ("u3b", "v2", True),
             ("up2", "deconv1", False), ("u2a", "v2", True), ("u2b", "v2", True),
             ("up1", "deconv1", False), ("u1a", "v2", False), ("u1b", "v2", False),
             ("up0", "deconv2", False), ("u0a", "v2", False), ("u0b", "v2", False), ("head", "tail", False)]),
}
KIND_NAMES = {0: "v2", 1: "first", 2: "wide"}


def _net():
    from diff_unet_amos_amd.diff_unet import DiffUNet
    torch.manual_seed(0)
    net = DiffUNet(in_channels=1, out_channels=CLASSES, features=FEATURES, compute_dtype=torch.float16)
    with torch.no_grad():
        for n, p in net.named_parameters():
            if ".adn.N." in n:                     # InstanceNorm affine away from (1, 0): the transforms are not identities
                p.copy_(torch.randn_like(p) * 0.3 + (1.0 if n.endswith("weight") else 0.0))
    return net.cuda().eval()


class _Checker:
    """The wrappers of one plan's launches and the rows of the table they fill."""

    def __init__(self, plan, case):
        from diff_unet_amos_amd import ops
        self.ops, self.plan, self.case, self.rows = ops, plan, case, []
        self.dt = plan.dtype
        self.orig = dict(conv3d_k3=ops.conv3d_k3, upconv_k3=ops.upconv_k3, deconv_k2s2=ops.deconv_k2s2,
                         materialize=ops.materialize, final_conv_sampler=ops.final_conv_sampler)
        self.names = {}
        for l in range(5):
            a, b = plan.den[l]
            self.names[plan.rawA[l].data_ptr()] = (f"d{l}a", a)
            self.names[plan.rawB[l].data_ptr()] = (f"d{l}b", b)
        for l in range(4):
            a, b = plan.dec[l]
            self.names[plan.uA[l].data_ptr()] = (f"u{l}a", a)
            self.names[plan.uB[l].data_ptr()] = (f"u{l}b", b)
            self.names[plan.cat[l].data_ptr()] = (f"m{l}", l)
        self.names[plan.x4.data_ptr()] = ("m4", 4)

    # ---- shared pieces ---------------------------------------------------------------------------------------------------
    def _pts(self, name, N, dims):
        return R.sample_voxels(N, dims, n_random=2000, seed=zlib.crc32(f"{self.case}/{name}".encode()))

    def _consts(self, norm, N):
        """fp32 scale, shift, add [N, C] of a producer descriptor as the consumers' preamble forms them (ops.instnorm_finalize:
        the same preamble), held to the fp64 values from the statistics words within the preamble's rounding."""
        stats, gamma, beta, add = norm.keep
        C = gamma.numel()
        sc64, sh64, b_sc, b_sh = R.finalize(self.ops.stats_decode(stats).cpu(), gamma.cpu(), beta.cpu(), norm.c.count, norm.c.eps)
        sc, sh = (t.cpu() for t in self.ops.instnorm_finalize(norm, N, C))
        for what, got, ref, b in (("scale", sc, sc64, b_sc), ("shift", sh, sh64, b_sh)):
            r = R.check(got, ref, b)
            assert r.ratio <= 1, f"{self.case}: InstanceNorm {what} of the preamble: {r}"
        if add is None:
            ad = torch.zeros(N, C)
        else:
            stride = norm.c.add_stride or C
            ad = torch.stack([add[n * stride:n * stride + C].cpu() for n in range(N)])
        return sc, sh, ad

    def _act(self, raw, n_idx, norm, N, ok=None):
        """The activation the kernel multiplies: raw values (float64 [P, ..., C]) through the emulated transform, zero outside."""
        if norm is None:
            return raw
        sc, sh, ad = self._consts(norm, N)
        shape = (-1,) + (1,) * (raw.dim() - 2) + (raw.shape[-1],)
        a = R.transform(raw, sc[n_idx].view(shape), sh[n_idx].view(shape), ad[n_idx].view(shape), self.dt)
        return a if ok is None else torch.where(ok[..., None], a, torch.zeros_like(a))

    def _stats_ratio(self, y, c_off, cout, stats):
        """statistics words against fp64 sums of the stored output (per sample and channel)"""
        N = y.shape[0]
        yv = y[..., c_off:c_off + cout].reshape(N, -1, cout)
        S, Q, A = [], [], []
        for n in range(N):
            v = yv[n].double()
            S.append(v.sum(0)); Q.append((v * v).sum(0)); A.append(v.abs().sum(0))
        S, Q, A = (torch.stack(t).cpu() for t in (S, Q, A))
        words = self.ops.stats_decode(stats).cpu()[:, :cout]
        bs, bq = R.stats_bound(A, Q, self.dt, yv.shape[1])
        rs = ((words[..., 0] - S).abs() / bs).max()
        rq = ((words[..., 1] - Q).abs() / bq).max()
        return float(torch.maximum(rs, rq))

    def _row(self, name, kind, split, shape, npts, res, stats_ratio=None):
        self.rows.append(dict(name=name, kind=kind, split=split, shape=shape, n=npts, ratio=res.ratio, where=res.where,
                              res=res, stats=stats_ratio))

    def _blocked(self, t, flag):
        return self.ops.from_blocked(t) if flag else t

    # ---- wrappers ----------------------------------------------------------------------------------------------------------
    def conv3d_k3(self, x, cin, cin_off, w_packed, bias_pad, cout, y, cout_off, out_stats, norm=None, workspace=None,
                  tap_channel=None, background=False, in_blocked=False, out_blocked=False):
        from diff_unet_amos_amd import _native as nv
        ops = self.ops
        name, layer = self.names[y.data_ptr()]
        N, D, H, W, cs = x.shape
        d = nv.Conv3Desc(nv.dt_code(x.dtype), N, D, H, W, cin, cs, cin_off, cout, y.shape[-1], cout_off,
                         0 if tap_channel is None else tap_channel + 1, 0,
                         (nv.IN_BLOCKED if in_blocked else 0) | (nv.OUT_BLOCKED if out_blocked else 0), ops.CONV_POLICY)
        ws_bytes = 0 if workspace is None else workspace.numel() * workspace.element_size()
        split = ops.conv3_form(d, norm is not None, ws_bytes).ksplit > 1           # the launcher's own answer for this call
        kind = KIND_NAMES[int(nv.lib().dua_conv3d_k3_kernel_kind(ctypes.byref(d), 1 if norm is not None else 0, 1 if split else 0))]
        xs = x.clone()
        self.orig["conv3d_k3"](x, cin, cin_off, w_packed, bias_pad, cout, y, cout_off, out_stats, norm=norm, workspace=workspace,
                               tap_channel=tap_channel, background=background, in_blocked=in_blocked, out_blocked=out_blocked)
        torch.cuda.synchronize()
        xc, yc = self._blocked(xs, in_blocked), self._blocked(y, out_blocked)
        pts = self._pts(name, N, (D, H, W))
        A, ok = R.gather_taps(xc, pts, cin_off, cin)
        A = self._act(A, pts[:, 0], norm, N, ok)
        w = layer.w.detach().float().cpu()
        if layer.perm is not None:                 # packed input channel j holds source channel perm[j] (or zero padding)
            wp = torch.zeros(w.shape[0], cin, 3, 3, 3)
            for j, s in enumerate(layer.perm[:cin]):
                if s >= 0:
                    wp[:, j] = w[:, s]
            w = wp
        ref, ab, sq = R.conv3_ref(A, R.conv3_weights(w, self.dt), layer.b)
        parts = 3 * -(-cin // ops.chunk_elems(self.dt)) if split else 0
        bnd = R.bound(ref, ab, sq, R.chain_length(27 * cin, self.dt, parts), self.dt,
                      emulated_in=self.dt if norm is not None else None)
        res = R.check(R.gather_points(yc, pts, cout_off, cout), ref, bnd, pts)
        self._row(name, kind, split, f"{N}x{D}x{H}x{W} {cin}->{cout}", len(pts), res, self._stats_ratio(yc, cout_off, cout, out_stats))

    def upconv_k3(self, xs, cskip, cskip_off, u, cu, cu_off, norm, w_skip, wu, btab, cout, y, cout_off, out_stats, in_blocked=False,
                  out_blocked=False):
        name, layer = self.names[y.data_ptr()]
        l = int(name[1])
        dec = self.plan.deconv[l]
        N, D, H, W, _ = xs.shape
        xsn, un = xs.clone(), u.clone()
        self.orig["upconv_k3"](xs, cskip, cskip_off, u, cu, cu_off, norm, w_skip, wu, btab, cout, y, cout_off, out_stats,
                               in_blocked=in_blocked, out_blocked=out_blocked)
        torch.cuda.synchronize()
        xc, yc = self._blocked(xsn, in_blocked), self._blocked(y, out_blocked)
        pts = self._pts(name, N, (D, H, W))
        A, _ = R.gather_taps(xc, pts, cskip_off, cskip)
        par, ok, phi, deltas = R.fold_parents(pts, (D, H, W))
        lim = torch.tensor([D // 2 - 1, H // 2 - 1, W // 2 - 1])
        pc = torch.minimum(par.clamp_min(0), lim).to(un.device)
        nn_ = pts[:, None, 0].expand_as(ok).to(un.device)
        U = un[nn_, pc[..., 0], pc[..., 1], pc[..., 2], cu_off:cu_off + cu].cpu().double()
        U = self._act(U, pts[:, 0], norm, N, ok)
        wc = layer.w.detach().float().cpu()
        Wp = R.decode_fold_weights(wu, cout, cu)
        # the packer's composed weights: the fp64 composition rounded once to fp16
        comp = R.compose_fold(wc[:, cskip:], dec.weight.detach().float().cpu()[:cu])
        for k, (m, mabs) in comp.items():
            wb = R.U16 * m.abs() + R.FLOOR16 + R.U32 * (8 * m.shape[1] + 1) * mabs
            r = R.check(Wp[k], m, wb)
            assert r.ratio <= 1, f"{self.case} {name}: composed weights {k}: {r}"
        rows, arows = R.fold_bias_table(wc[:, cskip:], layer.b, dec.bias)
        cls = R.border_class(pts, (D, H, W))
        ref, ab, sq = R.fold_ref(A, R.conv3_weights(wc[:, :cskip], self.dt), U, ok, phi, deltas, Wp, rows[cls], arows[cls])
        cmid = wc.shape[1] - cskip
        bnd = R.bound(ref, ab, sq, R.chain_length(27 * cskip + 8 * cu, self.dt), self.dt,
                      emulated_in=self.dt if norm is not None else None, extra=R.U32 * (27 * cmid + 1) * arows[cls])
        res = R.check(R.gather_points(yc, pts, cout_off, cout), ref, bnd, pts)
        self._row(name, "fold", False, f"{N}x{D}x{H}x{W} {cskip}+{cu}->{cout}", len(pts), res,
                  self._stats_ratio(yc, cout_off, cout, out_stats))

    def deconv_k2s2(self, x, cin, cin_off, w_packed, bias_pad, cout, y, cout_off, norm=None, out_blocked=False):
        ops = self.ops
        l = int(self.names[y.data_ptr()][0][1])
        name, dec = f"up{l}", self.plan.deconv[l]
        N, D, H, W, _ = x.shape
        kind = f"deconv{ops.deconv_kernel_kind(x.dtype, N, D, H, W, cin, cout)}"
        xs = x.clone()
        self.orig["deconv_k2s2"](x, cin, cin_off, w_packed, bias_pad, cout, y, cout_off, norm=norm, out_blocked=out_blocked)
        torch.cuda.synchronize()
        yc = self._blocked(y, out_blocked)
        dims = tuple(y.shape[1:4])
        pts = self._pts(name, N, dims)
        q = R.replicate_source(pts, (D, H, W))
        parent = q.clone()
        parent[:, 1:] >>= 1
        child = ((q[:, 1] & 1) * 4 + (q[:, 2] & 1) * 2 + (q[:, 3] & 1))
        A = self._act(R.gather_points(xs, parent, cin_off, cin), pts[:, 0], norm, N)
        ref, ab, sq = R.deconv_ref(A, dec.weight, dec.bias, self.dt, child)
        bnd = R.bound(ref, ab, sq, R.chain_length(cin, self.dt), self.dt, emulated_in=self.dt if norm is not None else None)
        res = R.check(R.gather_points(yc, pts, cout_off, cout), ref, bnd, pts)
        self._row(name, kind, False, f"{N}x{D}x{H}x{W} {cin}->{cout} -> {'x'.join(map(str, dims))}", len(pts), res)

    def materialize(self, raw, Cc, norm, out, out_off, emb=None, pooled=None, out_blocked=False):
        name, _ = self.names[out.data_ptr()]
        N, D, H, W, _ = raw.shape
        rs = raw.clone()
        self.orig["materialize"](raw, Cc, norm, out, out_off, emb=emb, pooled=pooled, out_blocked=out_blocked)
        torch.cuda.synchronize()
        oc = self._blocked(out, out_blocked)
        sc, sh, ad = self._consts(norm, N)
        pts = self._pts(name, N, (D, H, W))

        def ref_at(p):
            n = p[:, 0]
            e = R.gather_points(emb, p, 0, Cc) if emb is not None else None
            return R.materialize_ref(R.gather_points(rs, p, 0, Cc), sc[n], sh[n], ad[n], e)

        ref, mag = ref_at(pts)
        res = R.check(R.gather_points(oc, pts, out_off, Cc), ref, R.materialize_bound(ref, mag, self.dt), pts)
        npts = len(pts)
        if pooled is not None:                    # max of the rounded outputs = rounding of the max: the window's largest bound
            pp = self._pts(name + "/pool", N, (D // 2, H // 2, W // 2))
            best = bnd = None
            for k in range(8):
                c = pp.clone()
                c[:, 1:] = 2 * c[:, 1:] + torch.tensor([k >> 2, (k >> 1) & 1, k & 1])
                r, m = ref_at(c)
                b = R.materialize_bound(r, m, self.dt)
                best = r if best is None else torch.maximum(best, r)
                bnd = b if bnd is None else torch.maximum(bnd, b)
            rp = R.check(R.gather_points(pooled, pp, 0, Cc), best, bnd, pp)
            npts += len(pp)
            if rp.ratio > res.ratio:
                res = rp
        self._row(name, "mat", False, f"{N}x{D}x{H}x{W} {Cc}{' +pool' if pooled is not None else ''}", npts, res)

    def final_conv_sampler(self, raw, K, norm, wf, bf, num_classes, mode, logits=None, **kw):
        from diff_unet_amos_amd import _native as nv
        assert mode == nv.MODE_LOGITS and logits is not None
        rs = raw.clone()
        self.orig["final_conv_sampler"](raw, K, norm, wf, bf, num_classes, mode, logits=logits, **kw)
        torch.cuda.synchronize()
        N, D, H, W, _ = raw.shape
        sc, sh, _ = self._consts(norm, N)
        pts = self._pts("head", N, (D, H, W))
        n = pts[:, 0]
        # fp16 plans: each fp32 operand is carried as an fp16 pair (hi + lo, csrc/sampler.hip), the lo x lo product dropped:
        # 3 * 2^-22 of every product (tests/sampler_fp64ref.py)
        ref, ab, sq, _ = T.tail_logits_ref(R.gather_points(rs, pts, 0, K), sc[n], sh[n], wf, bf)
        bnd = T.tail_logits_bound(ref, ab, sq, K, split=self.dt == torch.float16)
        p = pts.to(logits.device)
        got = logits[p[:, 0], :, p[:, 1], p[:, 2], p[:, 3]].cpu()
        self._row("head", "tail", False, f"{N}x{D}x{H}x{W} {K}->{num_classes}", len(pts), R.check(got, ref, bnd, pts))


def _run_case(case, monkeypatch):
    from diff_unet_amos_amd import _native as nv
    from diff_unet_amos_amd import ops
    from diff_unet_amos_amd.engine import Plan
    exp = EXPECTED[case]
    torch.set_num_threads(max(1, min(16, len(os.sched_getaffinity(0)))))
    net = _net()
    N, dims, dt = exp["N"], exp["dims"], exp["dtype"]
    dev = torch.device("cuda", 0)
    # fp16 plans come from the runtime; the fp32 plan is the companion an fp16 plan builds for the last DDPM steps (Plan._hi_plan)
    plan = net._rt.plan(N, dims, dev) if dt == torch.float16 else Plan(net, N, *dims, torch.float32, dev)
    plan.refresh_weights()
    assert [plan._fold_level(l) for l in range(4)] == exp["fold"], f"{case}: fold levels moved"
    assert plan._level0_layout() == exp["layout"], f"{case}: level-0 layouts moved"
    g = torch.Generator().manual_seed(len(case))
    image = torch.rand(N, 1, *dims, generator=g)
    x = torch.randn(N, CLASSES, *dims, generator=g)
    t = torch.tensor([500, 37][:N])
    with torch.no_grad():
        plan.run_encoder(image.cuda())
        ops.to_channels_last(x.cuda().contiguous(), plan.xin, 0, CLASSES)
        plan.cur_add.copy_(plan.temb_table[t.to(dev).long()])
        chk = _Checker(plan, case)
        for k in chk.orig:
            monkeypatch.setattr(ops, k, getattr(chk, k))
        plan.denoiser_body()
        logits = torch.zeros((N, CLASSES, *dims), dtype=torch.float32, device=dev)
        plan.tail(nv.MODE_LOGITS, logits=logits)
        monkeypatch.undo()
    print(f"\n[{case}] {len(chk.rows)} launches; max |err| / bound per launch, statistics words likewise")
    print(f"  {'launch':<6} {'kind':<8} {'split':<5} {'shape':<34} {'samples':>7} {'err/bound':>10} {'stats':>8}  worst at")
    for r in chk.rows:
        st = "" if r["stats"] is None else f"{r['stats']:.3f}"
        print(f"  {r['name']:<6} {r['kind']:<8} {str(r['split']):<5} {r['shape']:<34} {r['n']:>7} {r['ratio']:>10.4f} {st:>8}  {r['where']}")
    seq = [(r["name"], r["kind"], r["split"]) for r in chk.rows]
    assert seq == exp["seq"], f"{case}: the launch sequence or its dispatch moved:\n got {seq}\nwant {exp['seq']}"
    bad = [(r["name"], r["res"]) for r in chk.rows if not r["ratio"] <= 1]
    assert not bad, f"{case}: launches over their fp64 bound: {bad}"
    bad = [(r["name"], r["stats"]) for r in chk.rows if r["stats"] is not None and not r["stats"] <= 1]
    assert not bad, f"{case}: statistics words off the sums of the stored outputs: {bad}"


@pytest.mark.parametrize("case", list(EXPECTED))
def test_every_launch_within_its_fp64_bound(case, monkeypatch):
    _run_case(case, monkeypatch)
