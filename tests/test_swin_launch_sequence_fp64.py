"""Every launch of the Swin plans (BASELINE config 5), in place: SwinPlan.run_encoder and step_begin + denoiser_body + tail (logits
mode) run eagerly with every ``ops`` entry point swin_engine.py calls wrapped, so that each launch is snapshotted, launched,
synchronised and held per element to the fp64 reference and derived bound the kernel tests already use (tests/swin_fp64ref.py
``S``, tests/fp64ref.py ``R``, tests/sampler_fp64ref.py ``T``) -- on the operands it actually read: the plan's reused scratch, its
channel offsets into the concat buffers, its statistics slices, its t_proj columns, its side-stream scratch set with
``background=`` as shipped (``two_streams`` stays at its default).  The statistics words a launch leaves are held to fp64 sums of
what it stored, the fp32 scale / shift its consumers derive from them (ops.instnorm_finalize) to ``R.finalize``.  The whole-tensor
moves (to_channels_last in run_encoder / stage_condition / denoise, from_channels_last in SwinEmbeddings) are checked for bit equality.

A check on "the operands it read" cannot see a launch that reads the wrong buffer, so the recorded rows (op, form, source buffer
and channel range, destination and offset, every further operand by name) must equal, in order, the sequence tests/swin_plan_cases.py
writes down by hand from the networks' structure; the reference of a launch takes its weights from the module that table names,
not from what the plan packed.  The forms come from the launchers' own answers (ops.conv3_form / dua_conv3d_k3_kernel_kind,
dua_deconv_k2s2_kernel_kind, dua_token_gemm_workspace) and from the dispatch rules restated in swin_fp64ref, so a dispatch change
fails here instead of moving coverage.

Cases (feature size 48; relative-position tables and LayerNorm affines away from their initial values; different timesteps per
sample):
  fp16-16c-64   64^3, 16 classes, upconv_min_tiles = 64: fold_up = [True, True], res_up = [True, True] (decoder2's coarse tensor
                has 96 <= 128 channels, so its residual branch folds too and only decoder5..3 launch a transposed convolution),
                the tap first convolution ("first/tap") of d1, the wide form for conv2 of e1 and u1 (d1's conv2 runs on the
                side stream with background=True, where the launcher stays with v2 -- pinned as such), the fused MFMA tail with
                the deferred _tail_src.
  fp16-3c-b2    batch 2, 64 x 32 x 32, 3 classes: per-sample statistics rows and t rows, token grids 32x16x16 .. 4x2x2 (padded
                7^3 windows, a (7, 4, 4) window with shift (3, 0, 0), an unshifted clipped (4, 2, 2) window), level 0 folds (256
                tiles), level 1 runs deconv_k2s2 + the plain conv1, a materialised decoder1 with ra, the VALU tail, no tap form.
                (conv3 of level 1 has 48 <= 64 outputs at feature size 48 and therefore always takes the fused token_linear
                "stats"; token_gemm + instnorm_stats is what levels 2..4 run, in every fp16 case, and is pinned there.)
  fp32-2c       32 x 32 x 64, 2 classes: the exact-fp32 parity plan, every GEMM on linear_f32, the MLP output y handed to the next
                window_gather_norm / patch_merge_norm, no fold.

The check can fail: for one launch of each kind in fp16-16c-64 the reference is re-evaluated on the stored samples with one
planted change on the reference side (a t_proj column moved to the next block's, post_add dropped, ra_off = 0, the skip half read
at channel offset 0, the statistics slice of the previous block, the bias of a fused epilogue omitted) and must be rejected."""
import ctypes
import os
import time
import zlib

import pytest
import torch

import fp64ref as R
import sampler_fp64ref as T
import swin_fp64ref as S
import swin_plan_cases as P

pytestmark = pytest.mark.gpu
F16, F32 = torch.float16, torch.float32
SLOPE, EPS = 0.01, 1e-5
NROWS, NVOX = 256, 1000                       # seeded random token rows / voxels per launch, on top of the structured ones
KIND_NAMES = {0: "v2", 1: "first", 2: "wide"}
# launches of fp16-16c-64's denoiser whose reference is re-evaluated with a planted change
PLANTED = {"t_column": "d4.conv2", "post_add": "d4.tail", "ra_off": "u4.tail", "skip_off": "u2.conv1", "stats_slice": "d3.conv2",
           "bias": "den.s0.b0.proj"}
torch.set_num_threads(max(1, min(16, len(os.sched_getaffinity(0)))))


def _net(case):
    from diff_unet_amos_amd.diff_swin_unetr import DiffSwinUNETR
    c = P.CASES[case]
    torch.manual_seed(0)
    net = DiffSwinUNETR(in_channels=1, out_channels=c["classes"], feature_size=P.F,
                        compute_dtype=F16 if c["dtype"] == "fp16" else F32).eval()
    with torch.no_grad():
        for k, p in net.named_parameters():
            if "relative_position_bias_table" in k:
                p.normal_(0, 0.3)                   # visible position bias (the default init is N(0, 0.02))
            elif ".norm" in k:                      # LayerNorm affine away from (1, 0)
                p.copy_(torch.randn_like(p) * 0.2 + (1.0 if k.endswith("weight") else 0.0))
    net.upconv_min_tiles = c["upconv_min_tiles"]
    return net.cuda()


def gemm_ksplit(M, K, N):
    """dua_token_gemm_workspace / dua_token_gemm restated (csrc/swin_gemm_wide.hip:200-230, as tests/test_swin_fp64.py has it):
    (z, the K slices that hold work); 0 = no split."""
    tiles, ksteps = -(-M // 64) * -(-N // 64), -(-K // 64)
    if tiles >= 128 or ksteps < 8:
        return 0, 0
    z = min(256 // tiles, ksteps // 2, 16)
    if z < 2:
        return 0, 0
    kper = -(-ksteps // z) * 64
    return z, -(-K // kper)


def _worst(*results):
    return max(results, key=lambda r: r.ratio)


class _Checker:
    """The wrappers of one plan's launches and the rows they record."""

    WRAPPED = ("patch_embed", "window_gather_norm", "token_linear", "token_gemm", "linear_f32", "window_attention",
               "window_scatter_add_norm", "swin_mlp", "patch_merge_norm", "stage_out", "conv3d_k3", "upconv_k3", "deconv_k2s2",
               "deconv_res", "instnorm_stats", "residual_norm_act", "final_conv_sampler", "to_channels_last", "from_channels_last")

    def __init__(self, net, plan, case, expect, keep=()):
        from diff_unet_amos_amd import ops
        self.ops, self.net, self.plan, self.case, self.expect = ops, net, plan, case, expect
        self.dt, self.N, self.dev = plan.dtype, plan.N, plan.dev
        self.orig = {k: getattr(ops, k) for k in self.WRAPPED}
        self.rows, self.moves, self.keep, self.saved, self.decoded = [], 0, set(keep), {}, {}
        self.geom = None
        self.tmp = {}
        n = self.names = {}
        for attr in ("img_in", "xin", "raw1", "raw2", "res3", "raw1b", "raw2b", "res3b", "win", "att", "ln2", "merged", "qkv_buf",
                     "hid_buf", "red_buf", "po_buf"):
            if hasattr(plan, attr):
                n[getattr(plan, attr).data_ptr()] = attr
        for attr in ("hs", "cat", "dec", "e_hs", "e_enc", "stream"):
            for i, t in enumerate(getattr(plan, attr)):
                if t is not None:
                    n[t.data_ptr()] = f"{attr}[{i}]"
        for r in plan.e_res + plan.d_res + plan.u_res:
            for k in range(3):
                n[r.st[k].data_ptr()] = f"{r.name}.st{k}"
        # linear_f32 outputs of the fp32 plan, named by the layer whose weight they were made with (the plan's packs)
        self.wrole = {}
        for vit in (plan.e_vit, plan.d_vit):
            for st in vit["stages"]:
                self.wrole[st["wred"].data_ptr()] = "tmp.red"
                for b in st["blocks"]:
                    for key, role in (("wqkv", "tmp.qkv"), ("wproj", "tmp.po"), ("w1", "tmp.h"), ("w2", "tmp.y")):
                        self.wrole[b[key].data_ptr()] = role

    # ---- names -------------------------------------------------------------------------------------------------------------
    def _name(self, t):
        p = t.data_ptr()
        return self.names.get(p) or self.tmp.get(p) or f"?{p:x}"

    def _t(self, t):
        """t_proj column offset of a view into cur_add"""
        return None if t is None else (t.data_ptr() - self.plan.cur_add.data_ptr()) // 4

    def _next(self, op):
        i = len(self.rows)
        assert i < len(self.expect), f"{self.case}: launch {i} ({op}) is beyond the {len(self.expect)} launches of the table"
        e = self.expect[i]
        assert e["op"] == op, f"{self.case}: launch {i} is {op}, the table has {e['op']} ({e['name']}) there"
        return e

    def _seed(self, name):
        return zlib.crc32(f"{self.case}/{name}".encode()) & 0x7fffffff

    def _rec(self, e, form, src, dst, shape, n, result, sratio=None, **extra):
        self.rows.append(dict(name=e["name"], op=e["op"], form=form, src=src, dst=dst, shape=shape, n=n, ratio=result.ratio, res=result,
                              stats=sratio, extra={k: v for k, v in extra.items() if v is not None}))

    def _save(self, e, evaluate):
        if e["name"] in self.keep:
            self.saved[e["name"]] = evaluate

    # ---- modules -------------------------------------------------------------------------------------------------------------
    def _vit(self, net):
        return (self.net.embed_model if net == "enc" else self.net.model).swinViT

    def _layer(self, name):
        """"<net>.s<i>.b<k>.<what>" -> (block module, stage); "<net>.s<i>.<what>" -> (None, stage)"""
        p = name.split(".")
        stage = self._vit(p[0]).stages()[int(p[1][1])]
        return (stage.blocks[int(p[2][1])] if p[2][0] == "b" and p[2][1:].isdigit() else None), stage

    def _res_module(self, blk):
        enc, den = self.net.embed_model, self.net.model
        if blk[0] == "e":
            return getattr(enc, f"encoder{blk[1:]}").layer
        if blk[0] == "d":
            return getattr(den, f"encoder{blk[1:]}").layer
        return getattr(den, f"decoder{blk[1:]}").conv_block

    def _perm(self, blk):
        """packed input channel p of xin = channel perm[p] of cat([image, x]); None elsewhere"""
        return list(range(1, self.plan.C + 1)) + [0] if blk in ("d1", "den") else None

    def _packed_cols(self, w, cin_packed, blk):
        """weight [Cout, Cin, ...] -> [Cout, cin_packed, ...] in the packed channel order of the block's input, zero beyond"""
        perm = self._perm(blk)
        w = w.detach().float().cpu()
        if perm is not None:
            w = w[:, perm]
        out = torch.zeros(w.shape[0], cin_packed, *w.shape[2:])
        out[:, :w.shape[1]] = w
        return out

    def _linear(self, name):
        """(weight fp32 [N, K], bias fp32 or None) of the nn.Linear a row names"""
        blk, stage = self._layer(name)
        what = name.split(".")[-1]
        lin = dict(qkv=lambda: blk.attn.qkv, proj=lambda: blk.attn.proj, fc1=lambda: blk.mlp.linear1, fc2=lambda: blk.mlp.linear2,
                   red=lambda: stage.downsample.reduction)[what]()
        return lin.weight.detach().float().cpu(), None if lin.bias is None else lin.bias.detach().float().cpu()

    def _w16(self, w):
        return (w.half() if self.dt == F16 else w).double()

    # ---- InstanceNorm consumers ---------------------------------------------------------------------------------------------
    def _consts(self, norm, C):
        """fp32 scale, shift, add [N, C] of a producer descriptor as the consumers' preamble forms them (ops.instnorm_finalize),
        held to the fp64 values from the statistics words within the preamble's rounding."""
        stats, gamma, beta, add = norm.keep
        dec = self.ops.stats_decode(stats).cpu()
        self.decoded[self._name(stats)] = (dec, norm.c.count)
        sc64, sh64, b_sc, b_sh = R.finalize(dec, gamma.cpu()[:C], beta.cpu()[:C], norm.c.count, norm.c.eps)
        sc, sh = (t.cpu() for t in self.ops.instnorm_finalize(norm, self.N, C))
        for what, got, ref, b in (("scale", sc, sc64, b_sc), ("shift", sh, sh64, b_sh)):
            r = R.check(got, ref, b)
            assert r.ratio <= 1, f"{self.case}: InstanceNorm {what} of the preamble ({self._name(stats)}): {r}"
        return sc, sh, self._add(add, norm.c.add_stride, C)

    def _add(self, add, stride, C, shift=0):
        if add is None:
            return torch.zeros(self.N, C)
        stride = stride or C
        return torch.stack([add[n * stride + shift:n * stride + shift + C].cpu() for n in range(self.N)])

    def _stats_ratio(self, y, c_off, cout, stats, n_contrib=None):
        """statistics words against fp64 sums of the stored output (per sample and channel)"""
        N = y.shape[0]
        v = y.reshape(N, -1, y.shape[-1])[..., c_off:c_off + cout].double()
        Ssum, Q, A = v.sum(1).cpu(), (v * v).sum(1).cpu(), v.abs().sum(1).cpu()
        words = self.ops.stats_decode(stats).cpu()[:, :cout]
        bs, bq = R.stats_bound(A, Q, self.dt, n_contrib or v.shape[1])
        return float(torch.maximum(((words[..., 0] - Ssum).abs() / bs).max(), ((words[..., 1] - Q).abs() / bq).max()))

    # ---- whole-tensor moves: bit equality -----------------------------------------------------------------------------------
    def to_channels_last(self, src, dst, c_off=0, c_fill=None):
        out = self.orig["to_channels_last"](src, dst, c_off, c_fill)
        torch.cuda.synchronize()
        Cc = src.shape[1]
        assert torch.equal(dst[..., c_off:c_off + Cc], src.permute(0, 2, 3, 4, 1).to(dst.dtype)), \
            f"{self.case}: to_channels_last into {self._name(dst)} at {c_off} is not the rounded source"
        if c_fill is not None and c_fill > Cc:
            assert not bool(dst[..., c_off + Cc:c_off + c_fill].any()), f"{self.case}: to_channels_last fill of {self._name(dst)}"
        self.moves += 1
        return out

    def from_channels_last(self, src, C_, c_off=0, out=None):
        out = self.orig["from_channels_last"](src, C_, c_off, out)
        torch.cuda.synchronize()
        assert torch.equal(out, src[..., c_off:c_off + C_].permute(0, 4, 1, 2, 3).float()), \
            f"{self.case}: from_channels_last of {self._name(src)} is not the stored tensor"
        self.moves += 1
        return out

    # ---- the Swin ops ------------------------------------------------------------------------------------------------------
    def patch_embed(self, xin, cin_packed, w_packed, bias, out, out_off=0, tadd=None, emb=None, x=None, eps=1e-5):
        e = self._next("patch_embed")
        self.orig["patch_embed"](xin, cin_packed, w_packed, bias, out, out_off, tadd=tadd, emb=emb, x=x, eps=eps)
        torch.cuda.synchronize()
        net = e["name"].split(".")[0]
        conv = self._vit(net).patch_embed.proj
        B, D, H, W, _ = xin.shape
        E, K = conv.weight.shape[0], 8 * cin_packed
        ntok = B * (D // 2) * (H // 2) * (W // 2)
        per = ntok // B
        n, n_ln, form = S.patch_embed_chain(K, self.dt)
        toks = S.sample_rows(ntok, NROWS, seed=self._seed(e["name"]), boundaries=(per,) if B > 1 else ())
        td = toks.to(self.dev)
        A = S.patch_embed_rows(xin, toks, cin_packed)
        Wm = S.patch_embed_weights(self._packed_cols(conv.weight, cin_packed, net)[:, :cin_packed], cin_packed, self.dt)
        trow = None if tadd is None else tadd.cpu()[toks // per]
        ref, ab, sq = S.patch_embed_ref(A, Wm, conv.bias.detach().float().cpu(), trow)
        xs = x.view(-1, E)[td].cpu()
        r1 = R.check(xs, ref, R.bound(ref, ab, sq, n, F32), coords=toks[:, None])
        embr = None if emb is None else emb.view(-1, E)[td].cpu().double()
        lref, parts = S.layernorm_ref(xs.double(), None, embr)
        got = out.view(ntok, -1)[td, out_off:out_off + E].cpu()
        r2 = R.check(got, lref, S.layernorm_bound(lref, parts, n_ln, self.dt), coords=toks[:, None])
        self._rec(e, form, (self._name(xin), 0, cin_packed), (self._name(out), out_off), f"{ntok}x{K}->{E}", len(toks), _worst(r1, r2),
                  t=self._t(tadd), emb=None if emb is None else self._name(emb), x=self._name(x))

    def _geom(self, g):
        self.geom = dict(B=g.B, dims=(g.D, g.H, g.W), C=g.C, ws=(g.wd, g.wh, g.ww), ss=(g.sd, g.sh, g.sw))
        return self.geom, f"w{g.wd}.{g.wh}.{g.ww} s{g.sd}.{g.sh}.{g.sw}"

    def window_gather_norm(self, x, geom, gamma, beta, out, y=None, eps=1e-5):
        e = self._next("window_gather_norm")
        x0 = x.clone() if y is not None else None                 # x += y in place
        self.orig["window_gather_norm"](x, geom, gamma, beta, out, y=y, eps=eps)
        torch.cuda.synchronize()
        g, form = self._geom(geom)
        C, B = g["C"], g["B"]
        blk, _ = self._layer(e["name"])
        tm = S.window_token_map(B, g["dims"], g["ws"], g["ss"])
        n = g["ws"][0] * g["ws"][1] * g["ws"][2]
        rows = S.sample_rows(tm.numel(), NROWS, seed=self._seed(e["name"]), boundaries=(tm.numel() // B,) if B > 1 else (), window=n)
        vox = tm[rows].clamp(min=0)
        vd = vox.to(self.dev)
        xs = x.view(-1, C)[vd].cpu()
        res = []
        if y is not None:
            sref = x0.view(-1, C)[vd].cpu().double() + y.reshape(-1, C)[vd].cpu().double()
            res.append(R.check(xs, sref, S.stream_add_bound(sref), coords=rows[:, None]))
        ref, parts = S.layernorm_ref(xs.double(), blk.norm1.weight.detach().float().cpu(), blk.norm1.bias.detach().float().cpu())
        real = (tm[rows] >= 0)[:, None]
        ref = torch.where(real, ref, torch.zeros_like(ref))                                    # F.pad after norm1: exact zeros
        bnd = torch.where(real, S.layernorm_bound(ref, parts, S.ln_chain(12, C // 12), self.dt), torch.full_like(ref, 1e-300))
        res.append(R.check(out.view(-1, C)[rows.to(self.dev)].cpu(), ref, bnd, coords=rows[:, None]))
        self._rec(e, form, (self._name(x), 0, C), (self._name(out), 0), f"{tm.numel()}x{C}", len(rows), _worst(*res),
                  y=None if y is None else self._name(y))

    def _lin_rows(self, e, M, **kw):
        return S.sample_rows(M, NROWS, seed=self._seed(e["name"]), **kw)

    def _conv3_weight(self, e, K):
        blk = e["name"].split(".")[0]
        m = self._res_module(blk)
        return self._packed_cols(m.conv3.conv.weight.reshape(m.conv3.conv.weight.shape[0], -1), K, blk)

    def token_linear(self, A, W, bias=None, mode="plain", out=None, out_off=0, x=None, stats=None, samples=1, geom=None, gamma=None,
                     beta=None, ln_out=None, eps=1e-5, background=False):
        e = self._next("token_linear")
        x0 = x.clone() if mode in ("scatter", "residual") else None
        ret = self.orig["token_linear"](A, W, bias, mode, out=out, out_off=out_off, x=x, stats=stats, samples=samples, geom=geom,
                                        gamma=gamma, beta=beta, ln_out=ln_out, eps=eps, background=background)
        torch.cuda.synchronize()
        M, K = A.shape
        N = W.shape[0]
        form = mode + ("/bg" if background else "")
        if mode == "stats":
            w, b = self._conv3_weight(e, K), None
        else:
            w, b = self._linear(e["name"])
        w = w.half().double()
        if mode == "plain":
            rows = self._lin_rows(e, M)
            rd = rows.to(self.dev)
            ref, ab, sq = S.linear_ref(A[rd].cpu().double(), w, b)
            got = out.view(M, -1)[rd, out_off:out_off + N].cpu()
            res = R.check(got, ref, S.linear_bound(ref, ab, sq, K, F16), coords=rows[:, None])
            self._rec(e, form, (self._name(A), 0, K), (self._name(out), out_off), f"{M}x{K}->{N}", len(rows), res)
        elif mode == "stats":
            V = M // samples
            rows = self._lin_rows(e, M, boundaries=(V,) if samples > 1 else ())
            rd = rows.to(self.dev)
            ref, ab, sq = S.linear_ref(A[rd].cpu().double(), w)
            res = R.check(out.view(M, -1)[rd, out_off:out_off + N].cpu(), ref, S.linear_bound(ref, ab, sq, K, F16), coords=rows[:, None])
            # the form tests/test_swin_fp64.py uses for this kernel: sums of the STORED values, one contribution per 128-row tile
            st = self._stats_ratio(out.view(samples, V, -1), out_off, N, stats, n_contrib=-(-V // 128))
            self._rec(e, form, (self._name(A), 0, K), (self._name(out), out_off), f"{M}x{K}->{N}", len(rows), res, st, stats=self._name(stats))
        elif mode == "scatter":
            g, gform = self._geom(geom)
            blk, _ = self._layer(e["name"])
            tm = S.window_token_map(g["B"], g["dims"], g["ws"], g["ss"])
            n = g["ws"][0] * g["ws"][1] * g["ws"][2]
            assert tm.numel() == M
            rows = self._lin_rows(e, M, boundaries=(M // g["B"],) if g["B"] > 1 else (), window=n)
            rows = rows[tm[rows] >= 0]                             # padding tokens write nothing; every voxel is written once
            vd = tm[rows].to(self.dev)
            Ar, x0r = A[rows.to(self.dev)].cpu().double(), x0.view(-1, N)[vd].cpu().double()
            xs, lns = x.view(-1, N)[vd].cpu(), ln_out.view(-1, N)[vd].cpu()
            g2, b2 = blk.norm2.weight.detach().float().cpu(), blk.norm2.bias.detach().float().cpu()

            def evaluate(no_bias=False):
                ref, ab, sq = S.linear_ref(Ar, w, None if no_bias else b)
                rx, abx = S.residual_ref(x0r, ref, ab)
                r1 = R.check(xs, rx, S.residual_bound(rx, abx, sq, K), coords=rows[:, None])
                lref, parts = S.layernorm_ref(xs.double(), g2, b2)          # the stored stream IS the norm's input
                return _worst(r1, R.check(lns, lref, S.layernorm_bound(lref, parts, S.ln_chain(12, N // 12), F16), coords=rows[:, None]))

            self._save(e, evaluate)
            self._rec(e, "scatter " + gform, (self._name(A), 0, K), (self._name(ln_out), 0), f"{M}x{K}->{N}", len(rows), evaluate(),
                      x=self._name(x))
        else:
            raise AssertionError(f"{self.case}: token_linear mode {mode} is not in the table")
        return ret

    def token_gemm(self, A, W, bias=None, mode="plain", out=None, out_off=0, x=None, workspace=None):
        from diff_unet_amos_amd import _native as nv
        e = self._next("token_gemm")
        x0 = x.clone() if mode == "residual" else None
        ret = self.orig["token_gemm"](A, W, bias, mode, out=out, out_off=out_off, x=x, workspace=workspace)
        torch.cuda.synchronize()
        M, K = A.shape
        N = W.shape[0]
        z, ks = gemm_ksplit(M, K, N)
        need = int(nv.lib().dua_token_gemm_workspace(M, K, N))
        assert need == z * M * N * 4, f"{self.case} {e['name']}: dua_token_gemm_workspace {need} is not {z} slices of {M}x{N}"
        form = f"{mode}/z{need // (M * N * 4)}"
        if e["name"].endswith(".conv3"):
            w, b = self._conv3_weight(e, K), None
        else:
            w, b = self._linear(e["name"])
        assert (b is None) == (bias is None)
        w = w.half().double()
        rows = S.sample_rows(M, NROWS, seed=self._seed(e["name"]))
        rd = rows.to(self.dev)
        ref, ab, sq = S.linear_ref(A[rd].cpu().double(), w, b)
        if mode == "residual":
            rx, abx = S.residual_ref(x0.view(M, N)[rd].cpu().double(), ref, ab)
            res = R.check(x.view(M, N)[rd].cpu(), rx, S.residual_bound(rx, abx, sq, K, ks), coords=rows[:, None])
            dst = (self._name(x), 0)
        else:
            got = out.view(M, -1)[rd, out_off:out_off + N].cpu()
            if mode == "gelu":
                res = R.check(got, S.gelu64(ref), S.linear_gelu_bound(ref, ab, K, F16, ks), coords=rows[:, None])
            else:
                res = R.check(got, ref, S.linear_bound(ref, ab, sq, K, F16, ks), coords=rows[:, None])
            dst = (self._name(out), out_off)
        self._rec(e, form, (self._name(A), 0, K), dst, f"{M}x{K}->{N}", len(rows), res)
        return ret

    def linear_f32(self, x, w, bias=None, gelu=False, out=None):
        e = self._next("linear_f32")
        ret = self.orig["linear_f32"](x, w, bias, gelu=gelu, out=out)
        torch.cuda.synchronize()
        K, N = x.shape[-1], w.shape[0]
        M = x.numel() // K
        if out is None:                                           # a fresh tensor: named by the layer it was made with
            role = self.wrole.get(w.data_ptr(), "tmp.?")
            self.tmp = {p: r for p, r in self.tmp.items() if r != role}
            self.tmp[ret.data_ptr()] = role
        if e["name"].endswith(".conv3"):
            wm, b = self._conv3_weight(e, K), None
        else:
            wm, b = self._linear(e["name"])
        assert (b is None) == (bias is None)
        rows = S.sample_rows(M, NROWS, seed=self._seed(e["name"]), tiles=(32, 64))
        rd = rows.to(self.dev)
        ref, ab, sq = S.linear_ref(x.reshape(-1, K)[rd].cpu().double(), wm.double(), b)
        want = S.gelu64(ref) if gelu else ref
        res = R.check(ret.view(M, N)[rd].cpu(), want, S.linear_f32_bound(ref, ab, sq, K, gelu), coords=rows[:, None])
        self._rec(e, "gelu" if gelu else "plain", (self._name(x), 0, K), (self._name(ret), 0), f"{M}x{K}->{N}", len(rows), res)
        return ret

    def window_attention(self, qkv, heads, bias_t, mask_t=None, windows_per_image=1, region_ids=None, out=None, bias_table=None,
                         table_grid=(7, 7, 7)):
        e = self._next("window_attention")
        ret = self.orig["window_attention"](qkv, heads, bias_t, mask_t=mask_t, windows_per_image=windows_per_image,
                                            region_ids=region_ids, out=out, bias_table=bias_table, table_grid=table_grid)
        torch.cuda.synchronize()
        assert bias_t is None and mask_t is None and tuple(table_grid) == P.WINDOW
        blk, _ = self._layer(e["name"])
        g = self.geom                                             # the geometry of the gather that filled these windows
        Wn, n, _ = qkv.shape
        nw = windows_per_image
        shifted = any(g["ss"])
        assert (region_ids is not None) == shifted and Wn == g["B"] * nw and n == g["ws"][0] * g["ws"][1] * g["ws"][2]
        reg = None
        if shifted:
            reg = S.region_ids(g["dims"], g["ws"], g["ss"])
            assert torch.equal(reg, region_ids.cpu()), f"{self.case} {e['name']}: region ids are not compute_mask's"
        form = S.attention_form(Wn, heads) + ("+region" if shifted else "")
        # (window, head) pairs: first / last window of every image, the last windows along each axis (mixed regions), seeded random
        # ones; first, last and a random head
        gw = torch.Generator().manual_seed(self._seed(e["name"]))
        wsel = {0, nw - 1, Wn - 1, Wn - nw, max(nw - 2, 0)} | {int(w) for w in torch.randint(0, Wn, (4,), generator=gw)}
        hsel = sorted({0, heads - 1, int(torch.randint(0, heads, (1,), generator=gw))})
        wins = torch.tensor(sorted(wsel)).repeat_interleave(len(hsel))
        hs = torch.tensor(hsel).repeat(len(wsel))
        t = qkv[wins.to(self.dev)].cpu().view(len(wins), n, 3, heads, 16)
        q, k, v = (S.f16(t[torch.arange(len(wins)), :, i, hs]) for i in range(3))               # fp32 input: rounded on load
        table_t = blk.attn.relative_position_bias_table.detach().float().cpu().t().contiguous()
        r = S.attention_ref(q, k, v, S.table_bias(table_t, hs, n), None if reg is None else S.region_mask(reg, wins, nw))
        got = ret[wins.to(self.dev)].cpu().view(len(wins), n, heads, 16)[torch.arange(len(wins)), :, hs]
        res = R.check(got, r["out"], S.attention_bound(r, qkv.dtype), coords=torch.stack([wins, hs], 1))
        self._rec(e, form, (self._name(qkv), 0, qkv.shape[-1]), (self._name(ret), 0), f"{Wn}x{n}x{heads}", got.numel() // 16, res)
        return ret

    def window_scatter_add_norm(self, x, geom, yw, gamma, beta, out, eps=1e-5):
        e = self._next("window_scatter_add_norm")
        x0 = x.clone()
        self.orig["window_scatter_add_norm"](x, geom, yw, gamma, beta, out, eps=eps)
        torch.cuda.synchronize()
        g, form = self._geom(geom)
        C, B = g["C"], g["B"]
        blk, _ = self._layer(e["name"])
        tm = S.window_token_map(B, g["dims"], g["ws"], g["ss"])
        nvox = x.numel() // C
        src = torch.empty(nvox, dtype=torch.int64)
        src[tm[tm >= 0]] = torch.arange(tm.numel())[tm >= 0]
        vrows = S.sample_rows(nvox, NROWS, seed=self._seed(e["name"]), boundaries=(nvox // B,) if B > 1 else ())
        vd = vrows.to(self.dev)
        xs = x.view(-1, C)[vd].cpu()
        sref = x0.view(-1, C)[vd].cpu().double() + yw.reshape(-1, C)[src[vrows].to(self.dev)].cpu().double()
        r1 = R.check(xs, sref, S.stream_add_bound(sref), coords=vrows[:, None])
        ref, parts = S.layernorm_ref(xs.double(), blk.norm2.weight.detach().float().cpu(), blk.norm2.bias.detach().float().cpu())
        r2 = R.check(out.view(-1, C)[vd].cpu(), ref, S.layernorm_bound(ref, parts, S.ln_chain(12, C // 12), self.dt), coords=vrows[:, None])
        self._rec(e, form, (self._name(yw), 0, C), (self._name(out), 0), f"{nvox}x{C}", len(vrows), _worst(r1, r2), x=self._name(x))

    def swin_mlp(self, ln2, w1, b1, w2, b2, x):
        e = self._next("swin_mlp")
        x0 = x.clone()
        ret = self.orig["swin_mlp"](ln2, w1, b1, w2, b2, x)
        torch.cuda.synchronize()
        blk, _ = self._layer(e["name"])
        M, C = ln2.shape
        rows = S.sample_rows(M, NROWS, seed=self._seed(e["name"]))
        rd = rows.to(self.dev)
        f = lambda p: p.detach().float().cpu()  # noqa: E731
        ref, bnd = S.mlp_ref(ln2[rd].cpu().double(), f(blk.mlp.linear1.weight).half().double(), f(blk.mlp.linear1.bias),
                             f(blk.mlp.linear2.weight).half().double(), f(blk.mlp.linear2.bias), x0.view(M, C)[rd].cpu().double())
        res = R.check(x.view(M, C)[rd].cpu(), ref, bnd, coords=rows[:, None])
        self._rec(e, "fused", (self._name(ln2), 0, C), (self._name(x), 0), f"{M}x{C}", len(rows), res)
        return ret

    def patch_merge_norm(self, x, gamma, beta, legacy=True, eps=1e-5, y=None, dtype=None, out=None):
        e = self._next("patch_merge_norm")
        ret = self.orig["patch_merge_norm"](x, gamma, beta, legacy=legacy, eps=eps, y=y, dtype=dtype, out=out)
        torch.cuda.synchronize()
        _, stage = self._layer(e["name"])
        B, D, H, W, C = x.shape
        ntok = B * ((D + 1) // 2) * ((H + 1) // 2) * ((W + 1) // 2)
        chain, form = S.patch_merge_chain(C, ntok)
        assert legacy
        toks = S.sample_rows(ntok, NROWS, seed=self._seed(e["name"]), boundaries=(ntok // B,) if B > 1 else ())
        xy = x if y is None else x + y.view_as(x).float()         # the pending y is added first, in one fp32 add, as the kernel does
        v = S.patch_merge_gather(xy, toks, legacy)
        nm = stage.downsample.norm
        ref, parts = S.layernorm_ref(v, nm.weight.detach().float().cpu(), nm.bias.detach().float().cpu())
        res = R.check(ret.view(-1, 8 * C)[toks.to(self.dev)].cpu(), ref, S.layernorm_bound(ref, parts, chain, self.dt), coords=toks[:, None])
        self._rec(e, form, (self._name(x), 0, C), (self._name(ret), 0), f"{ntok}x{8 * C}", len(toks), res, y=None if y is None else self._name(y))
        return ret

    def stage_out(self, y, B, Cc, out, out_off=0, tadd=None, emb=None, x=None, eps=1e-5):
        e = self._next("stage_out")
        self.orig["stage_out"](y, B, Cc, out, out_off, tadd=tadd, emb=emb, x=x, eps=eps)
        torch.cuda.synchronize()
        M = y.numel() // Cc
        per = M // B
        rows = S.sample_rows(M, NROWS, seed=self._seed(e["name"]), boundaries=(per,) if B > 1 else ())
        rd = rows.to(self.dev)
        sref = y.view(M, Cc)[rd].cpu().double()
        if tadd is not None:
            sref = sref + tadd.cpu()[rows // per].double()
        res = []
        if x is not None:
            xr = x.view(M, Cc)[rd].cpu()
            res.append(R.check(xr, sref, S.stream_add_bound(sref), coords=rows[:, None]))
        else:
            xr = sref.float()                                     # not stored (the last stage): the one fp32 add, emulated
        embr = None if emb is None else emb.view(M, Cc)[rd].cpu().double()
        ref, parts = S.layernorm_ref(xr.double(), None, embr)
        got = out.view(M, -1)[rd, out_off:out_off + Cc].cpu()
        res.append(R.check(got, ref, S.layernorm_bound(ref, parts, S.ln_chain(12, Cc // 12), self.dt), coords=rows[:, None]))
        self._rec(e, "", (self._name(y), 0, Cc), (self._name(out), out_off), f"{M}x{Cc}", len(rows), _worst(*res), t=self._t(tadd),
                  emb=None if emb is None else self._name(emb), x=None if x is None else self._name(x))
        return out

    # ---- convolutions --------------------------------------------------------------------------------------------------------
    def _pts(self, name, dims):
        return R.sample_voxels(self.N, dims, n_random=NVOX, seed=self._seed(name))

    def conv3d_k3(self, x, cin, cin_off, w_packed, bias_pad, cout, y, cout_off, out_stats, norm=None, workspace=None, tap_channel=None,
                  background=False, in_blocked=False, out_blocked=False):
        from diff_unet_amos_amd import _native as nv
        ops = self.ops
        e = self._next("conv3d_k3")
        assert not in_blocked and not out_blocked
        N, D, H, W, cs = x.shape
        d = nv.Conv3Desc(nv.dt_code(x.dtype), N, D, H, W, cin, cs, cin_off, cout, y.shape[-1], cout_off,
                         0 if tap_channel is None else tap_channel + 1, 1 if background else 0, 0, ops.CONV_POLICY)
        ws_bytes = 0 if workspace is None else workspace.numel() * workspace.element_size()
        split = ops.conv3_form(d, norm is not None, ws_bytes).ksplit > 1           # the launcher's own answer for this call
        kind = KIND_NAMES[int(nv.lib().dua_conv3d_k3_kernel_kind(ctypes.byref(d), 1 if norm is not None else 0, 1 if split else 0))]
        form = kind + ("/split" if split else "") + ("/tap" if tap_channel is not None else "") + ("/bg" if background else "")
        self.orig["conv3d_k3"](x, cin, cin_off, w_packed, bias_pad, cout, y, cout_off, out_stats, norm=norm, workspace=workspace,
                               tap_channel=tap_channel, background=background)
        torch.cuda.synchronize()
        blk, which = e["name"].split(".")
        m = self._res_module(blk)
        conv = m.conv1.conv if which == "conv1" else m.conv2.conv
        w = self._packed_cols(conv.weight, cin, blk) if which == "conv1" else conv.weight.detach().float().cpu()
        Wm = R.conv3_weights(w, self.dt)
        pts = self._pts(e["name"], (D, H, W))
        A, ok = R.gather_taps(x, pts, cin_off, cin)
        got = R.gather_points(y, pts, cout_off, cout)
        parts = 3 * -(-cin // ops.chunk_elems(self.dt)) if split else 0
        chain = R.chain_length(27 * cin, self.dt, parts)
        zero = torch.zeros(cout)
        extra = {}
        if norm is None:
            def evaluate():
                ref, ab, sq = R.conv3_ref(A, Wm, zero)
                return R.check(got, ref, R.bound(ref, ab, sq, chain, self.dt), pts)
        else:
            sc, sh, ad = self._consts(norm, cin)
            stats, _, _, add = norm.keep
            extra = dict(norm=self._name(stats), t=self._t(add))
            count, stride, n_idx = norm.c.count, norm.c.add_stride, pts[:, 0]

            def evaluate(t_shift=0, stats_from=None):
                s, h, a = sc, sh, ad
                if t_shift:                                       # the t_proj columns of another block
                    a = self._add(add, stride, cin, t_shift)
                if stats_from is not None:                        # another block's statistics words, this block's count
                    s, h, _, _ = R.finalize(stats_from, torch.ones(cin), torch.zeros(cin), count, EPS)
                    s, h = s.float(), h.float()
                act = R.transform(A, s[n_idx].view(-1, 1, cin), h[n_idx].view(-1, 1, cin), a[n_idx].view(-1, 1, cin), self.dt, slope=SLOPE)
                act = torch.where(ok[..., None], act, torch.zeros_like(act))
                ref, ab, sq = R.conv3_ref(act, Wm, zero)
                return R.check(got, ref, R.bound(ref, ab, sq, chain, self.dt, emulated_in=self.dt), pts)
        self._save(e, evaluate)
        self._rec(e, form, (self._name(x), cin_off, cin), (self._name(y), cout_off), f"{N}x{D}x{H}x{W} {cin}->{cout}", len(pts), evaluate(),
                  self._stats_ratio(y, cout_off, cout, out_stats), stats=self._name(out_stats), **extra)

    def upconv_k3(self, xs, cskip, cskip_off, u, cu, cu_off, norm, w_skip, wu, btab, cout, y, cout_off, out_stats, in_blocked=False,
                  out_blocked=False):
        e = self._next("upconv_k3")
        assert norm is None and not in_blocked and not out_blocked and cu_off == 0
        self.orig["upconv_k3"](xs, cskip, cskip_off, u, cu, cu_off, norm, w_skip, wu, btab, cout, y, cout_off, out_stats)
        torch.cuda.synchronize()
        blk = e["name"].split(".")[0]
        m = self._res_module(blk)
        dec = getattr(self.net.model, f"decoder{blk[1:]}").transp_conv.conv
        N, D, H, W, _ = xs.shape
        pts = self._pts(e["name"], (D, H, W))
        par, ok, phi, deltas = R.fold_parents(pts, (D, H, W))
        lim = torch.tensor([D // 2 - 1, H // 2 - 1, W // 2 - 1])
        pc = torch.minimum(par.clamp_min(0), lim).to(self.dev)
        nn_ = pts[:, None, 0].expand_as(ok).to(self.dev)
        U = u[nn_, pc[..., 0], pc[..., 1], pc[..., 2], :cu].cpu().double()
        wc = m.conv1.conv.weight.detach().float().cpu()                  # torch.cat((up, skip)): the upsampled half first
        cmid = wc.shape[1] - cskip
        wd = dec.weight.detach().float().cpu()                           # [Cu real, Cmid, 2, 2, 2]; the buffer's padding meets zero rows
        Wp = R.decode_fold_weights(wu, cout, cu)
        comp = R.compose_fold(wc[:, :cmid], wd)
        for k, (mm, mabs) in comp.items():                               # the packer's composed weights: fp64 composition rounded once
            full, fabs = torch.zeros(cout, cu, dtype=torch.float64), torch.zeros(cout, cu, dtype=torch.float64)
            full[:, :mm.shape[1]], fabs[:, :mm.shape[1]] = mm, mabs
            r = R.check(Wp[k], full, R.U16 * full.abs() + R.FLOOR16 + R.U32 * (8 * mm.shape[1] + 1) * fabs)
            assert r.ratio <= 1, f"{self.case} {e['name']}: composed weights {k}: {r}"
        rows, arows = R.fold_bias_table(wc[:, :cmid], None, None)
        cls = R.border_class(pts, (D, H, W))
        Wsk = R.conv3_weights(wc[:, cmid:], self.dt)
        got = R.gather_points(y, pts, cout_off, cout)
        bound_n = R.chain_length(27 * cskip + 8 * cu, self.dt)

        A_skip, _ = R.gather_taps(xs, pts, cskip_off, cskip)
        A_at_0 = R.gather_taps(xs, pts, 0, cskip)[0] if e["name"] in self.keep else None

        def evaluate(skip_at_0=False):
            A = A_at_0 if skip_at_0 else A_skip
            ref, ab, sq = R.fold_ref(A, Wsk, U, ok, phi, deltas, Wp, rows[cls], arows[cls])
            return R.check(got, ref, R.bound(ref, ab, sq, bound_n, self.dt, extra=R.U32 * (27 * cmid + 1) * arows[cls]), pts)

        self._save(e, evaluate)
        self._rec(e, "fold", (self._name(xs), cskip_off, cskip), (self._name(y), cout_off), f"{N}x{D}x{H}x{W} {cskip}+{cu}->{cout}",
                  len(pts), evaluate(), self._stats_ratio(y, cout_off, cout, out_stats), up=self._name(u), stats=self._name(out_stats))

    def deconv_k2s2(self, x, cin, cin_off, w_packed, bias_pad, cout, y, cout_off, norm=None, out_blocked=False):
        e = self._next("deconv_k2s2")
        assert norm is None and not out_blocked
        N, D, H, W, _ = x.shape
        form = f"deconv{self.ops.deconv_kernel_kind(x.dtype, N, D, H, W, cin, cout)}"
        self.orig["deconv_k2s2"](x, cin, cin_off, w_packed, bias_pad, cout, y, cout_off)
        torch.cuda.synchronize()
        dec = getattr(self.net.model, f"decoder{e['name'][2:]}").transp_conv.conv
        dims = tuple(y.shape[1:4])
        assert dims == (2 * D, 2 * H, 2 * W)
        pts = self._pts(e["name"], dims)
        parent = pts.clone()
        parent[:, 1:] >>= 1
        child = (pts[:, 1] & 1) * 4 + (pts[:, 2] & 1) * 2 + (pts[:, 3] & 1)
        ref, ab, sq = R.deconv_ref(R.gather_points(x, parent, cin_off, cin), dec.weight, torch.zeros(cout), self.dt, child)
        res = R.check(R.gather_points(y, pts, cout_off, cout), ref, R.bound(ref, ab, sq, R.chain_length(cin, self.dt), self.dt), pts)
        self._rec(e, form, (self._name(x), cin_off, cin), (self._name(y), cout_off), f"{N}x{D}x{H}x{W} {cin}->{cout}", len(pts), res)

    def deconv_res(self, lo, cin, cin_off, w_packed, xs, cs, cs_off, ws_packed, cout, y, cout_off, stats):
        e = self._next("deconv_res")
        self.orig["deconv_res"](lo, cin, cin_off, w_packed, xs, cs, cs_off, ws_packed, cout, y, cout_off, stats)
        torch.cuda.synchronize()
        blk = e["name"].split(".")[0]
        m = self._res_module(blk)
        dec = getattr(self.net.model, f"decoder{blk[1:]}").transp_conv.conv
        N, D, H, W, _ = lo.shape
        dims = (2 * D, 2 * H, 2 * W)
        pts = self._pts(e["name"], dims)
        parent = pts.clone()
        parent[:, 1:] >>= 1
        child = (pts[:, 1] & 1) * 4 + (pts[:, 2] & 1) * 2 + (pts[:, 3] & 1)
        w3 = m.conv3.conv.weight.detach().float().cpu().reshape(cout, -1)
        ref, ab, sq = R.deconv_res_ref(R.gather_points(lo, parent, cin_off, cin), R.gather_points(xs, pts, cs_off, cs), w3, dec.weight,
                                       child, up_first=True)
        bnd = R.bound(ref, ab, sq, R.chain_length(cin + cs, self.dt), self.dt, emulated_in=self.dt)
        res = R.check(R.gather_points(y, pts, cout_off, cout), ref, bnd, pts)
        self._rec(e, "res", (self._name(lo), cin_off, cin), (self._name(y), cout_off), f"{N}x{D}x{H}x{W} {cin}+{cs}->{cout}", len(pts), res,
                  self._stats_ratio(y, cout_off, cout, stats), skip=(self._name(xs), cs_off, cs), stats=self._name(stats))

    def instnorm_stats(self, x, Cc, stats, c_off=0):
        e = self._next("instnorm_stats")
        ret = self.orig["instnorm_stats"](x, Cc, stats, c_off)
        torch.cuda.synchronize()
        st = self._stats_ratio(x, c_off, Cc, stats)
        res = R.CheckResult(st, (), 0.0, 0.0, 0.0)
        N, D, H, W, _ = x.shape
        self._rec(e, "", (self._name(x), c_off, Cc), (self._name(stats), 0), f"{N}x{D}x{H}x{W} {Cc}", N * D * H * W, res, st)
        return ret

    def residual_norm_act(self, raw, norm, res, res_norm=None, slope=0.01, out=None, out_off=0, post_add=None, post_off=0,
                          ra_src=None, ra_off=0, res_off=0, background=False):
        e = self._next("residual_norm_act")
        assert out is not None and slope == SLOPE and post_off == 0 and res_off == 0
        ret = self.orig["residual_norm_act"](raw, norm, res, res_norm, slope=slope, out=out, out_off=out_off, post_add=post_add,
                                             post_off=post_off, ra_src=ra_src, ra_off=ra_off, res_off=res_off, background=background)
        torch.cuda.synchronize()
        N, D, H, W, C = raw.shape
        V = D * H * W
        sc, sh, _ = self._consts(norm, C)
        rsc = rsh = None
        if res_norm is not None:
            rsc, rsh, _ = self._consts(res_norm, C)
        rows = S.sample_rows(N * V, 2 * NROWS, seed=self._seed(e["name"]), boundaries=(V,) if N > 1 else ())
        rd, smp = rows.to(self.dev), rows // V
        pick = lambda t, lo, hi: t.view(N * V, -1)[rd, lo:hi].cpu().double()  # noqa: E731
        rawr, resr, got = pick(raw, 0, C), pick(res, 0, C), pick(out, out_off, out_off + C)
        postr = None if post_add is None else pick(post_add, 0, C)
        rar = None if ra_src is None else pick(ra_src, ra_off, ra_off + C)
        ra0 = None if ra_src is None else pick(ra_src, 0, C)
        d = lambda t: None if t is None else t[smp].double()  # noqa: E731

        def evaluate(drop_post=False, ra_at_0=False):
            ref, parts = S.residual_norm_act_ref(rawr, d(sc), d(sh), resr, d(rsc), d(rsh), SLOPE, None if drop_post else postr,
                                                 ra0 if ra_at_0 else rar)
            return R.check(got, ref, S.residual_norm_act_bound(ref, parts, self.dt), coords=rows[:, None])

        self._save(e, evaluate)
        self._rec(e, "bg" if background else "", (self._name(raw), 0, C), (self._name(out), out_off), f"{N}x{D}x{H}x{W} {C}", len(rows),
                  evaluate(), norm=self._name(norm.keep[0]), res=self._name(res),
                  res_norm=None if res_norm is None else self._name(res_norm.keep[0]),
                  post_add=None if post_add is None else self._name(post_add), ra=None if ra_src is None else (self._name(ra_src), ra_off))
        return ret

    def final_conv_sampler(self, raw, K, norm, wf, bf, num_classes, mode, logits=None, residual=None, **kw):
        from diff_unet_amos_amd import _native as nv
        e = self._next("final_conv_sampler")
        assert mode == nv.MODE_LOGITS and logits is not None
        self.orig["final_conv_sampler"](raw, K, norm, wf, bf, num_classes, mode, logits=logits, residual=residual, **kw)
        torch.cuda.synchronize()
        N, D, H, W, _ = raw.shape
        head = self.net.model.out.conv.conv
        wfm = torch.zeros(num_classes, K)
        wfm[:, :P.F] = head.weight.detach().float().cpu().reshape(num_classes, -1)
        bfm = head.bias.detach().float().cpu()
        mfma = self.dt == F16 and self.ops.state_stride(num_classes) == 16 and K in (32, 64, 128)       # csrc/sampler.hip:570
        pts = self._pts(e["name"], (D, H, W))
        n = pts[:, 0]
        p = pts.to(self.dev)
        got = logits[p[:, 0], :, p[:, 1], p[:, 2], p[:, 3]].cpu()
        extra = {}
        if residual is not None:
            res, res_norm, ra_src, ra_off, ch = residual
            sc, sh, _ = self._consts(norm, ch)
            rsc, rsh, _ = self._consts(res_norm, ch)
            rd = dict(res=R.gather_points(res, pts, 0, ch), rsc=rsc[n], rsh=rsh[n], ra=R.gather_points(ra_src, pts, ra_off, ch), kvalid=ch)
            ref, ab, sq, aerr = T.tail_logits_ref(R.gather_points(raw, pts, 0, ch), sc[n], sh[n], wfm, bfm, slope=SLOPE, residual=rd)
            form, src = ("mfma" if mfma else "valu") + " residual", (self._name(raw), 0, ch)
            extra = dict(norm=self._name(norm.keep[0]), res=self._name(res), res_norm=self._name(res_norm.keep[0]),
                         ra=(self._name(ra_src), ra_off))
        else:
            assert norm is None
            ref, ab, sq, aerr = T.tail_logits_ref(R.gather_points(raw, pts, 0, K), None, None, wfm, bfm, identity=True)
            form, src = ("mfma" if mfma else "valu") + " identity", (self._name(raw), 0, K)
        bnd = T.tail_logits_bound(ref, ab, sq, K, split=mfma, emulated=False, act_err=aerr)
        self._rec(e, form, src, ("logits", 0), f"{N}x{D}x{H}x{W} {K}->{num_classes}", len(pts), R.check(got, ref, bnd, pts), **extra)


# ---- plans, runs -------------------------------------------------------------------------------------------------------------
def _build(case):
    """(net, plan, image, x, t, NCDHW embeddings): the plan with its weights packed and the condition of one random image resident."""
    c = P.CASES[case]
    net = _net(case)
    dev = torch.device("cuda", 0)
    plan = net._rt.plan(c["N"], c["dims"], dev)
    g = torch.Generator().manual_seed(len(case))
    image = torch.rand(c["N"], 1, *c["dims"], generator=g).cuda()
    x = torch.randn(c["N"], c["classes"], *c["dims"], generator=g).cuda()
    t = torch.tensor([500, 37][:c["N"]])
    with torch.no_grad():
        emb = plan.run_encoder(image)
        staged = [[e.clone() for e in emb[0]]] + [emb[k].clone() for k in range(1, 5)]
    assert plan.fold_up == c["fold"] and plan.res_up == c["res_up"], f"{case}: fold levels moved: {plan.fold_up} {plan.res_up}"
    assert plan.fused_tail == c["fused_tail"] and (plan.d_res[0].tap is not None) == c["tap"], f"{case}: tail / tap form moved"
    assert plan.two_streams
    return dict(net=net, plan=plan, image=image, x=x, t=t, staged=staged, runs={})


def _run(b, case, network):
    """One checked pass of ``network``; the checker is kept for the tests that share it."""
    if network in b["runs"]:
        return b["runs"][network]
    from diff_unet_amos_amd import ops
    plan = b["plan"]
    chk = _Checker(b["net"], plan, case, P.sequence(case, network), keep=PLANTED.values() if case == "fp16-16c-64" else ())
    t0 = time.perf_counter()
    with pytest.MonkeyPatch.context() as mp, torch.no_grad():
        for k in chk.WRAPPED:
            mp.setattr(ops, k, getattr(chk, k))
        if network == "encoder":
            emb = plan.run_encoder(b["image"])
            for k in range(5):
                emb[k]                                            # SwinEmbeddings: from_channels_last of all nine maps
        else:
            plan.stage_condition(b["image"], b["staged"])         # caller-supplied NCDHW embeddings: to_channels_last of all of them
            chk.logits = plan.denoise(b["x"], b["t"])
    chk.seconds = time.perf_counter() - t0
    b["runs"][network] = chk
    return chk


@pytest.fixture(scope="module")
def plans():
    """case -> the built plan with its staged condition, built on first use and released when this file is done."""
    cache = {}

    def get(case):
        if case not in cache:
            cache[case] = _build(case)
        return cache[case]

    yield get
    cache.clear()
    torch.cuda.empty_cache()


def _fmt(v):
    return "" if v is None else f"{v:.3f}"


@pytest.mark.parametrize("network", ["encoder", "denoiser"])
@pytest.mark.parametrize("case", list(P.CASES))
def test_every_launch_within_its_fp64_bound_and_in_its_place(case, network, plans):
    chk = _run(plans(case), case, network)
    print(f"\n[{case} {network}] {len(chk.rows)} launches, {chk.moves} whole-tensor moves bit-equal, {chk.seconds:.1f} s; "
          f"max |err| / bound per launch, statistics words likewise")
    print(f"  {'launch':<18} {'op':<24} {'form':<22} {'shape':<30} {'samples':>7} {'err/bound':>10} {'stats':>8}  worst at")
    for r in chk.rows:
        print(f"  {r['name']:<18} {r['op']:<24} {r['form']:<22} {r['shape']:<30} {r['n']:>7} {r['ratio']:>10.4f} {_fmt(r['stats']):>8}  "
              f"{r['res'].where}")
    worst = {}
    for r in chk.rows:
        worst[r["op"]] = max(worst.get(r["op"], 0.0), r["ratio"])
    print("  largest err/bound per op: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())))
    want = P.sequence(case, network)
    got_keys, want_keys = [P.key(r) for r in chk.rows], [P.key(r) for r in want]
    diff = [(i, g, w) for i, (g, w) in enumerate(zip(got_keys, want_keys)) if g != w]
    assert not diff and len(got_keys) == len(want_keys), \
        f"{case} {network}: the launch sequence, its dataflow or its dispatch moved ({len(got_keys)} launches, table {len(want_keys)}):\n" + \
        "\n".join(f" launch {i}:\n   got  {g}\n   want {w}" for i, g, w in diff[:8])
    assert chk.moves == (2 + 9 if network == "encoder" else 1 + 9 + 1), f"{case} {network}: {chk.moves} whole-tensor moves"
    bad = [(r["name"], r["res"]) for r in chk.rows if not r["ratio"] <= 1]
    assert not bad, f"{case} {network}: launches over their fp64 bound: {bad}"
    bad = [(r["name"], r["stats"]) for r in chk.rows if r["stats"] is not None and not r["stats"] <= 1]
    assert not bad, f"{case} {network}: statistics words off the sums of the stored outputs: {bad}"
    if network == "denoiser":
        assert bool(torch.isfinite(chk.logits).all())


@pytest.mark.parametrize("defect", list(PLANTED))
def test_a_planted_reference_side_defect_is_rejected(defect, plans):
    """Nothing is re-run on the device: the stored samples of one launch, the reference with one change."""
    case = "fp16-16c-64"
    chk = _run(plans(case), case, "denoiser")
    name = PLANTED[defect]
    evaluate = chk.saved[name]
    toff, _ = P.t_offsets(P.CASES[case]["classes"])
    clean = evaluate()
    if defect == "t_column":                                      # d4's conv2 reads encoder10's columns
        bad = evaluate(t_shift=toff["d10"] - toff["d4"])
    elif defect == "post_add":                                    # enc3 = encoder4(...) without + embeddings[4]
        bad = evaluate(drop_post=True)
    elif defect == "ra_off":                                      # r3 taken from the upsampled half of cat[3]
        bad = evaluate(ra_at_0=True)
    elif defect == "skip_off":                                    # the skip half read where the upsampled half would be
        bad = evaluate(skip_at_0=True)
    elif defect == "stats_slice":                                 # d3's norm1 from the sums the block launched before it (d4) left
        dec, _ = chk.decoded["d4.st0"]
        bad = evaluate(stats_from=dec[:, :2 * P.F])
    else:                                                         # proj's bias left out of the scatter epilogue
        bad = evaluate(no_bias=True)
    print(f"planted {defect:<12} at {name:<16} err/bound {clean.ratio:.3f} -> {bad.ratio:.3g}")
    assert clean.ratio <= 1, (defect, clean)
    assert bad.ratio > 1, (defect, bad)
