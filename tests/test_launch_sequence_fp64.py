"""Every launch of the shipped denoiser evaluation, at its real shape, layout and channel offsets, against an fp64 reference on the
operands it read (tests/fp64ref.py): Plan.denoiser_body() launched kernel by kernel -- the one place the launch sequence is
written down -- and the head in logits mode, with ops.conv3d_k3 / upconv_k3 / deconv_k2s2 / materialize / final_conv_sampler
wrapped so that each call is launched, synchronised, sampled on the device and checked per element against its bound, and the
InstanceNorm statistics words a convolution leaves against fp64 sums of what it stored.

Six plans at default widths (64, 64, 128, 256, 512, 64), 16 classes: the benchmarked fp16 96^3 patch; fp16 at batch 2 with
an odd extent (replicate-padded transposed convolutions, floor pooling, per-sample statistics rows); the exact-fp32 companion
plan the last DDPM steps run on, at 64^3; and the 96^3 patch at batch 2, 3 and 4 (sliding-window batches, balanced batches of
three, step-uncertainty runs in adjacent rows), whose launch forms are functions of the workgroup count N x 96^3 gives: other
kernels, tile depths and splits than at N = 1.  The samples of these three differ in scale and timestep, so that a row of
statistics, scale / shift or embedding add taken from a neighbouring sample is far outside every bound.  Which kernel every
launch takes is pinned below, as the policy is written today -- the coarse kind and, in FORMS, the kernel of the form query with
its tile depth and split: a policy change that moves a launch makes this test fail instead of quietly testing another kernel.

test_rows_of_a_batch_do_not_see_each_other runs the batch-4 plan twice, the second time with another image, state and timestep
in row 2 only: every other row of every buffer the plan exposes and of the logits keeps its bits."""
import ctypes
import math
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
# The batched cases must be able to tell the samples of a batch apart (case_inputs).  Two measures, both in units of what a check
# allows: an elementwise consumer (materialise, the head, the transposed convolution's input) rounds at 2^-11 of a value, so the
# scale and add rows of neighbouring samples are held 8 x 2^-11 apart in the typical channel (median relative distance, APART);
# a convolution sums thousands of terms, so for every fused convolution the reference is evaluated once more with the next sample's
# rows and must lie more than twice the bound away (column "rows n+1" of the table, as tests/test_batched_forms_defects.py).
APART = 2.0 ** -8
TIMESTEPS = (500, 37, 811, 203)            # one per sample of a batch; the first two are what the batch-1 and batch-2 cases always used


def _batched_96(N, level1, level2, level3, split4):
    """EXPECTED entry and FORMS row of the fp16 96^3 plan at batch N > 1: (kind, kernel, tile depth) of the convolutions at 48^3,
    24^3 and 12^3 and the split of the two at 6^3; the rest does not move with N."""
    k1, k2, k3 = level1[0], level2[0], level3[0]
    seq = [("d0a", "first", False), ("d0b", "wide", False), ("m0", "mat", False),
           ("d1a", k1, False), ("d1b", k1, False), ("m1", "mat", False),
           ("d2a", k2, False), ("d2b", k2, False), ("m2", "mat", False),
           ("d3a", k3, False), ("d3b", k3, False), ("m3", "mat", False),
           ("d4a", "v2", True), ("d4b", "v2", True), ("m4", "mat", False),
           ("up3", "deconv1", False), ("u3a", k3, False), ("u3b", k3, False),
           ("up2", "deconv1", False), ("u2a", k2, False), ("u2b", k2, False),
           ("u1a", "fold", False), ("u1b", k1, False),
           ("u0a", "fold", False), ("u0b", "wide", False), ("head", "tail", False)]
    forms = {"d0a": ("FIRST", 4, 1), "d0b": ("WIDE", 8, 1), "u0b": ("WIDE", 8, 1), "d4a": ("V2_4_KD", 4, split4), "d4b": ("V2_4_KD", 4, split4)}
    for names, (_, kernel, depth) in ((("d1a", "d1b", "u1b"), level1), (("d2a", "d2b", "u2a", "u2b"), level2),
                                      (("d3a", "d3b", "u3a", "u3b"), level3)):
        forms.update({n: (kernel, depth, 1) for n in names})
    return dict(N=N, dims=(96, 96, 96), dtype=torch.float16, fold=[True, True, False, False], layout=(True, True, True), seq=seq,
                distinct=True), forms


# launch -> (kernel of dua_conv3d_k3_form without its DUA_CONV3_ prefix, tile depth, ksplit): the coarse kind above cannot tell a
# two-deep tile from a four-deep one, a kd-plane kernel from a plain one, or one split from another
FORMS = {
    "fp16-96": {"d0a": ("FIRST", 4, 1), "d0b": ("WIDE", 8, 1), "d1a": ("V2_4", 4, 1), "d1b": ("V2_4", 4, 1),
                "d2a": ("V2_2_KD", 2, 1), "d2b": ("V2_2_KD", 2, 1), "d3a": ("V2_4_KD", 4, 4), "d3b": ("V2_4_KD", 4, 5),
                "d4a": ("V2_4_KD", 4, 12), "d4b": ("V2_4_KD", 4, 16), "u3a": ("V2_4_KD", 4, 5), "u3b": ("V2_4_KD", 4, 5),
                "u2a": ("V2_2_KD", 2, 1), "u2b": ("V2_2_KD", 2, 1), "u1b": ("V2_4", 4, 1), "u0b": ("WIDE", 8, 1)},
    "fp16-b2-odd": {"d0a": ("FIRST", 4, 1), "d0b": ("V2_4", 4, 1), "d1a": ("V2_2", 2, 1), "d1b": ("V2_2", 2, 1),
                    "d2a": ("V2_4_KD", 4, 3), "d2b": ("V2_4_KD", 4, 4), "d3a": ("V2_4_KD", 4, 12), "d3b": ("V2_4_KD", 4, 12),
                    "d4a": ("V2_4_KD", 4, 12), "d4b": ("V2_4_KD", 4, 16), "u3a": ("V2_4_KD", 4, 16), "u3b": ("V2_4_KD", 4, 12),
                    "u2a": ("V2_4_KD", 4, 4), "u2b": ("V2_4_KD", 4, 4), "u1a": ("V2_2", 2, 1), "u1b": ("V2_2", 2, 1),
                    "u0a": ("V2_4", 4, 1), "u0b": ("V2_4", 4, 1)},
    "fp32-64": {"d0a": ("V2_4", 4, 1), "d0b": ("V2_4", 4, 1), "d1a": ("V2_2_KD", 2, 1), "d1b": ("V2_2_KD", 2, 1),
                "d2a": ("V2_4_KD", 4, 6), "d2b": ("V2_4_KD", 4, 8), "d3a": ("V2_4_KD", 4, 24), "d3b": ("V2_4_KD", 4, 24),
                "d4a": ("V2_4_KD", 4, 24), "d4b": ("V2_4_KD", 4, 32), "u3a": ("V2_4_KD", 4, 32), "u3b": ("V2_4_KD", 4, 24),
                "u2a": ("V2_4_KD", 4, 8), "u2b": ("V2_4_KD", 4, 8), "u1a": ("V2_2_KD", 2, 1), "u1b": ("V2_2_KD", 2, 1),
                "u0a": ("V2_4", 4, 1), "u0b": ("V2_4", 4, 1)},
}
# The batched 96^3 plans.  The level-2 fold stays off at every batch: its coarse tensor has 256 channels and dua_upconv_k3_supported
# takes at most 128, so u2a is a plain convolution also at N = 4, where 27 * 4 * 2 = 216 tiles pass Plan.UPCONV_MIN_TILES.
for _n, _args in ((2, (("v2", "V2_4", 4), ("v2", "V2_4", 4), ("v2", "V2_2_KD", 2), 8)),
                  (3, (("wide", "WIDE", 8), ("v2", "V2_4", 4), ("v2", "V2_2", 2), 5)),
                  (4, (("wide", "WIDE", 8), ("v2", "V2_4", 4), ("v2", "V2_2", 2), 4))):
    EXPECTED[f"fp16-96-b{_n}"], FORMS[f"fp16-96-b{_n}"] = _batched_96(_n, *_args)


def form_names(nv):
    """dua_conv3_form.kernel -> its name without the prefix"""
    return {getattr(nv, n): n[len("CONV3_"):] for n in dir(nv) if n.startswith("CONV3_")}


def case_inputs(case):
    """(image [N, 1, D, H, W], x [N, classes, D, H, W], timesteps [N]) of a case, on the host.  The cases marked ``distinct`` make
    the samples of a batch differ in what InstanceNorm does not remove.  A factor on a sample is not enough: the network is
    positively homogeneous up to its biases, the first normalisation divides the factor out, and the scale rows of two samples
    of white noise then agree to 1e-3 (measured: 7.6e-4 at the first materialise with factors 1 and 1.5).  So sample n's state
    and image are noise in blocks of (n + 1)^3 equal voxels -- another spatial correlation, so other variances behind every
    convolution -- scaled by 1 + 0.5 n (state) and 1 - 0.2 n (image) and moved by 0.25 n; with the distinct timesteps every scale,
    shift and add row of a sample is far from its neighbours' (_Checker._consts asserts it at every launch)."""
    exp = EXPECTED[case]
    N, dims = exp["N"], exp["dims"]
    g = torch.Generator().manual_seed(len(case))
    image = torch.rand(N, 1, *dims, generator=g)
    x = torch.randn(N, CLASSES, *dims, generator=g)
    if exp.get("distinct"):
        for n in range(N):
            k = n + 1
            assert all(s % k == 0 for s in dims)
            for t in (x, image):
                coarse = t[n, :, :dims[0] // k, :dims[1] // k, :dims[2] // k]
                t[n] = coarse.repeat_interleave(k, 1).repeat_interleave(k, 2).repeat_interleave(k, 3)
            x[n] = x[n] * (1 + 0.5 * n) + 0.25 * n
            image[n] *= 1 - 0.2 * n
    return image, x, torch.tensor(TIMESTEPS[:N])


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
        self.ops, self.plan, self.case, self.rows, self.apart = ops, plan, case, [], []
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
        pts = R.sample_voxels(N, dims, n_random=2000, seed=zlib.crc32(f"{self.case}/{name}".encode()))
        # the structured points of the sampler are per sample: both faces of every axis of EVERY sample are among them
        for n in range(N):
            p = pts[pts[:, 0] == n]
            for ax, S in enumerate(dims):
                assert bool((p[:, 1 + ax] == 0).any()) and bool((p[:, 1 + ax] == S - 1).any()), (self.case, name, n, ax)
        return pts

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
        if EXPECTED[self.case].get("distinct"):
            # how far apart the rows of neighbouring samples are, in the typical channel (_run_case holds it to APART)
            rel = lambda v: float(((v - v.roll(1, 0)).abs() / v.abs().clamp_min(1e-30)).median())      # noqa: E731
            self.apart.append((C, rel(sc), rel(ad) if add is not None else math.inf))      # asserted once the table is printed
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

    def _row(self, name, kind, split, shape, npts, res, stats_ratio=None, form=None, tell=None):
        self.rows.append(dict(name=name, kind=kind, split=split, shape=shape, n=npts, ratio=res.ratio, where=res.where,
                              res=res, stats=stats_ratio, form=form, tell=tell))

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
        f = ops.conv3_form(d, norm is not None, ws_bytes)                          # the launcher's own answer for this call
        split = f.ksplit > 1
        form = (form_names(nv)[f.kernel], f.tile_depth, f.ksplit)
        assert form == FORMS[self.case][name], f"{self.case} {name}: the launch form moved: {form}, pinned {FORMS[self.case][name]}"
        kind = KIND_NAMES[int(nv.lib().dua_conv3d_k3_kernel_kind(ctypes.byref(d), 1 if norm is not None else 0, 1 if split else 0))]
        xs = x.clone()
        self.orig["conv3d_k3"](x, cin, cin_off, w_packed, bias_pad, cout, y, cout_off, out_stats, norm=norm, workspace=workspace,
                               tap_channel=tap_channel, background=background, in_blocked=in_blocked, out_blocked=out_blocked)
        torch.cuda.synchronize()
        xc, yc = self._blocked(xs, in_blocked), self._blocked(y, out_blocked)
        pts = self._pts(name, N, (D, H, W))
        A_raw, ok = R.gather_taps(xc, pts, cin_off, cin)
        A = self._act(A_raw, pts[:, 0], norm, N, ok)
        w = layer.w.detach().float().cpu()
        if layer.perm is not None:                 # packed input channel j holds source channel perm[j] (or zero padding)
            wp = torch.zeros(w.shape[0], cin, 3, 3, 3)
            for j, s in enumerate(layer.perm[:cin]):
                if s >= 0:
                    wp[:, j] = w[:, s]
            w = wp
        Wm = R.conv3_weights(w, self.dt)
        ref, ab, sq = R.conv3_ref(A, Wm, layer.b)
        parts = 3 * -(-cin // ops.chunk_elems(self.dt)) if split else 0
        bnd = R.bound(ref, ab, sq, R.chain_length(27 * cin, self.dt, parts), self.dt,
                      emulated_in=self.dt if norm is not None else None)
        res = R.check(R.gather_points(yc, pts, cout_off, cout), ref, bnd, pts)
        tell = None
        if norm is not None and EXPECTED[self.case].get("distinct"):
            # would this check notice the scale / shift / add rows of the next sample?  The same reference with those rows, in
            # units of the bound (the largest element): a kernel that read them would land about there
            mixed = R.conv3_ref(self._act(A_raw, (pts[:, 0] + 1) % N, norm, N, ok), Wm, layer.b)[0]
            tell = float(((mixed - ref).abs() / bnd).max())
        self._row(name, kind, split, f"{N}x{D}x{H}x{W} {cin}->{cout}", len(pts), res, self._stats_ratio(yc, cout_off, cout, out_stats),
                  form=form, tell=tell)

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
    image, x, t = case_inputs(case)
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
    print(f"  {'launch':<6} {'kind':<8} {'split':<5} {'form (kernel, depth, ksplit)':<28} {'shape':<34} {'samples':>7} {'err/bound':>10} {'stats':>8} {'rows n+1':>9}  worst at")
    for r in chk.rows:
        st = "" if r["stats"] is None else f"{r['stats']:.3f}"
        fm = "" if r["form"] is None else "{} d{} k{}".format(*r["form"])
        tl = "" if r["tell"] is None else f"{r['tell']:.0f}"
        print(f"  {r['name']:<6} {r['kind']:<8} {str(r['split']):<5} {fm:<28} {r['shape']:<34} {r['n']:>7} {r['ratio']:>10.4f} {st:>8} {tl:>9}  {r['where']}")
    if exp.get("distinct"):
        near = min(chk.apart, key=lambda a: min(a[1:]))
        print(f"  median relative distance between the rows of neighbouring samples, smallest of {len(chk.apart)} descriptors read: "
              f"scale {near[1]:.3f}, add {near[2]:.3f} ({near[0]} channels)")
        assert min(near[1:]) > APART, f"{case}: scale / add rows of neighbouring samples nearly equal: {sorted(set(chk.apart))}"
        blind = [(r["name"], r["tell"]) for r in chk.rows if r["tell"] is not None and not r["tell"] > 2]
        assert not blind and sum(r["tell"] is not None for r in chk.rows) == 9, f"{case}: a neighbour's rows would pass: {blind}"
    seq = [(r["name"], r["kind"], r["split"]) for r in chk.rows]
    assert seq == exp["seq"], f"{case}: the launch sequence or its dispatch moved:\n got {seq}\nwant {exp['seq']}"
    assert {r["name"]: r["form"] for r in chk.rows if r["form"] is not None} == FORMS[case], f"{case}: not every pinned form was launched"
    bad = [(r["name"], r["res"]) for r in chk.rows if not r["ratio"] <= 1]
    assert not bad, f"{case}: launches over their fp64 bound: {bad}"
    bad = [(r["name"], r["stats"]) for r in chk.rows if r["stats"] is not None and not r["stats"] <= 1]
    assert not bad, f"{case}: statistics words off the sums of the stored outputs: {bad}"


@pytest.mark.parametrize("case", list(EXPECTED))
def test_every_launch_within_its_fp64_bound(case, monkeypatch):
    _run_case(case, monkeypatch)


def _evaluate(plan, image, x, t):
    """One evaluation as _run_case stages it, unwrapped: (logits, copies of every buffer the plan exposes and of the statistics
    words of every convolution of the denoiser)."""
    from diff_unet_amos_amd import _native as nv
    from diff_unet_amos_amd import ops
    dev = plan.dev
    with torch.no_grad():
        plan.run_encoder(image.to(dev))
        ops.to_channels_last(x.to(dev).contiguous(), plan.xin, 0, CLASSES)
        plan.cur_add.copy_(plan.temb_table[t.to(dev).long()])
        plan.denoiser_body()
        logits = torch.zeros((plan.N, CLASSES, *plan.dims), dtype=torch.float32, device=dev)
        plan.tail(nv.MODE_LOGITS, logits=logits)
    torch.cuda.synchronize()
    snap = {"x4": plan.x4.clone(), "logits": logits}
    for key in ("rawA", "rawB", "uA", "uB", "cat"):
        for l, buf in enumerate(getattr(plan, key)):
            snap[f"{key}[{l}]"] = buf.clone()
    for pair in plan.den + plan.dec:
        for c in pair:
            snap[f"stats {c.name}"] = c.stats.clone()
    return snap


def test_rows_of_a_batch_do_not_see_each_other():
    """The fp16-96-b4 plan evaluated twice, the second time with another image, state and timestep in row 2 and nothing else
    changed: rows 0, 1 and 3 of the logits, of rawA, rawB, uA, uB, cat (every level), x4 and of every convolution's statistics
    words keep their bits, row 2 of each changes.  Every voxel, where the per-launch check samples.  Bit equality is the contract:
    a sample's workgroups read its own rows only, the statistics are integer atomics per sample and split-K partials are summed
    in a fixed order; a halo read across a sample boundary, a row of statistics / scale / add of a neighbour, or a mis-decoded
    blockIdx of the batched grids would carry row 2's change into another row.  (A buffer in 16-channel blocks keeps the sample
    outermost, so indexing the sample holds there too.)"""
    case, changed = "fp16-96-b4", 2
    exp = EXPECTED[case]
    N, dims = exp["N"], exp["dims"]
    net = _net()
    plan = net._rt.plan(N, dims, torch.device("cuda", 0))
    plan.refresh_weights()
    assert [plan._fold_level(l) for l in range(4)] == exp["fold"] and plan._level0_layout() == exp["layout"]
    image, x, t = case_inputs(case)
    before = _evaluate(plan, image, x, t)
    g = torch.Generator().manual_seed(20)
    image[changed] = torch.rand(1, *dims, generator=g) * 0.45
    x[changed] = torch.randn(CLASSES, *dims, generator=g) * 0.7
    t[changed] = 999
    after = _evaluate(plan, image, x, t)
    assert before.keys() == after.keys() and len(before) == 2 + 5 + 5 + 4 + 4 + 4 + 18
    leaked = [(k, n) for k in before for n in range(N) if n != changed and not torch.equal(before[k][n], after[k][n])]
    assert not leaked, f"rows other than {changed} changed with it: {leaked}"
    same = [k for k in before if torch.equal(before[k][changed], after[k][changed])]
    assert not same, f"row {changed} did not change in {same}"
