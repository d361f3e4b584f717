"""The launch sequence of the two Swin-UNETR networks (BASELINE config 5), written down by hand from the networks' structure for
the cases of tests/test_swin_launch_sequence_fp64.py.  CPU only (like tests/conv_form_cases.py): no device, no plan, no import of
the package -- the table is what diff_unet_amos_amd/swin_engine.py has to issue, not a restatement of what it does issue.

Structure (feature size 48, depths (2, 2, 2, 2), window 7^3, heads 3 / 6 / 12 / 24), with the reference's lines:
  * SwinUNETREncoder.forward (models/swin_unetr/encoder.py:212-219): swinViT(image) -> five hidden states, then encoder1(image),
    encoder2..4(hidden_states_out[0..2]).
  * SwinUNETRDenoiser.forward (models/swin_unetr/denoiser.py:353-403): hidden_states_out[i] + embeddings[0][i] (367-368),
    enc_k = encoder_{k+1}(...) + embeddings[k + 1] with r_k = reverse_attention(enc_k) (370-383), dec4 = encoder10(hs[4]) (387),
    decoder5(dec4, hs[3]) (388), decoder4..1 each followed by + r_k (389-397), out (398).
  * SwinTransformer.forward (transformer.py:270-316): patch_embed, + t_proj[0], four stages each followed by + t_proj[i + 1] and
    the normalised output; a stage is two blocks (transformer.py:378-434: norm1, pad, roll, partition, attention, reverse, roll
    back, crop, shortcut, norm2, MLP, shortcut) and PatchMerging (patch.py:44-91).
  * UnetResBlock.forward (blocks.py:298-316): conv1, norm1, act, + t_proj, conv2, norm2, [conv3, norm3 when the channel count
    changes], add, act.  UnetrUpBlock (blocks.py:90): transposed convolution, torch.cat((up, skip)), the block.

A row is a dict: ``name`` (which layer: the checker takes the module's own weights by it), ``op``, ``form`` and the dataflow fields
``src`` (buffer, channel offset, channels), ``dst`` (buffer, channel offset) and ``extra`` (every further operand by role:
``norm`` / ``res_norm`` / ``stats`` = statistics slice "<block>.st<k>", ``t`` = t_proj column offset, ``emb``, ``x`` = fp32 stream,
``y`` = pending MLP output, ``res``, ``post_add``, ``ra`` = (buffer, offset), ``up`` = coarse tensor, ``skip`` = (buffer, offset, channels)).
Buffers carry the plan's attribute names (``xin``, ``hs[i]``, ``cat[k]``, ``dec[k]``, ``e_hs[i]``, ``e_enc[k]``, ``stream[i]``, the scratch
``raw1`` / ``raw2`` / ``res3`` with their side-stream twins ``raw1b`` ..., ``win``, ``att``, ``ln2``, ``merged``, ``qkv_buf``, ``hid_buf``,
``red_buf``, ``po_buf``); ``tmp.<role>`` is a tensor linear_f32 allocates in the fp32 plan.

Forms.  What a case pins is written per case below (``CONV_FORMS``, ``GEMM_Z``, ``CONV3_Z``): the convolution kernel kind and split-K of every
3x3x3 launch, the transposed-convolution kind, the K slices of every token GEMM; the rest follows from rules restated here with
their sources (``attention_form``, ``merge_form``).  The forms were read off the launchers' own host functions for 256 CUs
(ops.conv3_form, dua_conv3d_k3_kernel_kind, dua_deconv_k2s2_kernel_kind, dua_token_gemm_workspace) and are asserted against
them on the device by the GPU test: a dispatch change fails there.
"""
F = 48
WINDOW = (7, 7, 7)
HEADS = (3, 6, 12, 24)
TOK_C = [F * 2 ** i for i in range(5)]

# blocks: name -> (level, cin as packed, cout, has conv3).  e*: the conditioning encoder; d*: the denoiser's encoder1..4 and encoder10;
# u1..u5: the residual blocks of decoder1..5.  cin of e1 / d1 is the packed input width (filled per case for d1).
ENC_BLOCKS = [("e1", 0, 8, F, True), ("e2", 1, F, F, False), ("e3", 2, 2 * F, 2 * F, False), ("e4", 3, 4 * F, 4 * F, False)]
UP_BLOCKS = [("u1", 0, 2 * F, F), ("u2", 1, 2 * F, F), ("u3", 2, 4 * F, 2 * F), ("u4", 3, 8 * F, 4 * F), ("u5", 4, 16 * F, 8 * F)]
DEC_C = [64, F, 2 * F, 4 * F, 8 * F, 16 * F]            # real channels of out (48 in a 64-channel stride), dec[1..5]

CASES = {
    # 64^3: 1024 level-0 tiles of 4x8x8 (conv2 of the level-0 blocks takes the wide form), upconv_min_tiles = 64 folds decoder1
    # (512 tiles of 8x8x8) and decoder2 (64), 16 classes: the tap first convolution and the fused MFMA tail
    "fp16-16c-64": dict(dtype="fp16", classes=16, N=1, dims=(64, 64, 64), upconv_min_tiles=64,
                        fold=[True, True, False, False, False], res_up=[True, True, False, False, False], tap=True, fused_tail=True),
    # batch 2, 64 x 32 x 32: token grids 32x16x16 (padded 7^3 windows), 16x8x8 (padded), 8x4x4 (window (7, 4, 4), shift (3, 0, 0)),
    # 4x2x2 (clipped, unshifted); 256 level-0 tiles fold decoder1, decoder2 (32 tiles) runs deconv_k2s2 and the plain conv1
    "fp16-3c-b2": dict(dtype="fp16", classes=3, N=2, dims=(64, 32, 32), upconv_min_tiles=200,
                       fold=[True, False, False, False, False], res_up=[True, False, False, False, False], tap=False, fused_tail=False),
    "fp32-2c": dict(dtype="fp32", classes=2, N=1, dims=(32, 32, 64), upconv_min_tiles=200,
                    fold=[False] * 5, res_up=[False] * 5, tap=False, fused_tail=False),
}


# ---- the pinned forms ------------------------------------------------------------------------------------------------------------
# 3x3x3 convolutions: block -> (conv1, conv2) as "<kernel kind>[/split]" (kinds of dua_conv3d_k3_kernel_kind: "v2", "first" = the
# resident-weight first-layer kernel, "wide" = the wide-tile form; "/split" = split-K with a finish launch); conv1 of a folded
# block is upconv_k3 and has no entry.  Transposed convolutions: "deconv<dua_deconv_k2s2_kernel_kind>".
# fp16-16c-64: the wide form is taken by conv2 of e1 and u1; d1 runs on the side stream with background=True, where the launcher
# keeps one workgroup per CU and stays with v2, so its conv2 is pinned as v2.
_SPLIT = ("v2/split", "v2/split")
CONV_FORMS = {
    "fp16-16c-64": dict(e1=("v2", "wide"), e2=("v2", "v2"), e3=_SPLIT, e4=_SPLIT, d1=("first", "v2"), d2=("v2", "v2"), d3=_SPLIT, d4=_SPLIT,
                        d10=_SPLIT, u5=_SPLIT, u4=_SPLIT, u3=_SPLIT, u2=(None, "v2"), u1=(None, "wide"),
                        up5="deconv0", up4="deconv1", up3="deconv0"),
    "fp16-3c-b2": dict(e1=("v2", "v2"), e2=_SPLIT, e3=_SPLIT, e4=_SPLIT, d1=("v2", "v2"), d2=_SPLIT, d3=_SPLIT, d4=_SPLIT,
                       d10=_SPLIT, u5=_SPLIT, u4=_SPLIT, u3=_SPLIT, u2=_SPLIT, u1=(None, "v2"),
                       up5="deconv0", up4="deconv1", up3="deconv0", up2="deconv0"),
    "fp32-2c": dict(e1=("v2", "v2"), e2=_SPLIT, e3=_SPLIT, e4=_SPLIT, d1=("v2", "v2"), d2=_SPLIT, d3=_SPLIT, d4=_SPLIT,
                    d10=_SPLIT, u5=_SPLIT, u4=_SPLIT, u3=_SPLIT, u2=_SPLIT, u1=("v2", "v2"),
                    up5="deconv0", up4="deconv0", up3="deconv1", up2="deconv0", up1="deconv0"),
}
# token GEMMs (fp16 plans; the same in both fp16 cases and both networks): K slices z of dua_token_gemm_workspace
# (= workspace bytes / (4 M N); 0 = the single-launch form) by (stage, layer); every other layer is 0.  conv3 of u5: 6.
GEMM_Z = {(1, "red"): 6, (2, "fc2"): 6, (2, "red"): 12, (3, "fc2"): 12, (3, "red"): 16}
CONV3_Z = {"u5": 6, "u4": 0, "u3": 0}
GEMM_MODE = dict(qkv="plain", proj="plain", fc1="gelu", fc2="residual", red="plain", conv3="plain")


def _form(c, name):
    parts = name.split(".")
    if parts[0] in ("enc", "den"):                       # <net>.s<i>[.b<k>].<layer>
        z = GEMM_Z.get((int(parts[1][1]), parts[-1]), 0)
        return f"{GEMM_MODE[parts[-1]]}/z{z}"
    forms = CONV_FORMS[c["case"]]
    if len(parts) == 1:
        return forms[name]
    if parts[1] == "conv3":
        return f"plain/z{CONV3_Z[parts[0]]}"
    return forms[parts[0]][0 if parts[1] == "conv1" else 1]


def clip_window(dims):
    """attention.py:225-251 get_window_size for the 7^3 window and its 3^3 shift."""
    ws = tuple(d if d <= 7 else 7 for d in dims)
    ss = tuple(0 if d <= 7 else 3 for d in dims)
    return ws, ss


def level_dims(dims, l):
    return tuple(d >> l for d in dims)


def t_offsets(classes):
    """Column offset of every t_proj in the timestep table: swinViT.t_proj[0..4], then encoder1..4, encoder10, decoder1..5's blocks,
    each padded to a multiple of 8 columns."""
    widths = [("vit0", F), ("vit1", 2 * F), ("vit2", 4 * F), ("vit3", 8 * F), ("vit4", 16 * F), ("d1", F), ("d2", F), ("d3", 2 * F),
              ("d4", 4 * F), ("d10", 16 * F), ("u1", F), ("u2", F), ("u3", 2 * F), ("u4", 4 * F), ("u5", 8 * F)]
    out, o = {}, 0
    for name, w in widths:
        out[name] = o
        o += -(-w // 8) * 8
    return out, o


def attention_form(windows, heads, shifted):
    """csrc/window_attention.hip: one workgroup per (window, head) from 1024 pairs on, else query blocks split over z; the mask of
    a shifted block comes from region ids."""
    return ("one-workgroup" if windows * heads >= 1024 else "split") + ("+region" if shifted else "")


def merge_form(C, ntok):
    """csrc/swin_ops.hip:154: a workgroup per token when ntok < 2048 and 8 C % 256 == 0, else a wave per token."""
    return "wide" if ntok < 2048 and (8 * C) % 256 == 0 else "wave"


def _row(name, op, form, src, dst, **extra):
    return dict(name=name, op=op, form=form, src=src, dst=dst, extra={k: v for k, v in extra.items() if v is not None})


def _swin_rows(c, net, xin, cin_packed, toff, emb, outs, after_stage=None):
    """SwinTransformer.forward.  ``outs[i]`` = (buffer, channel offset) of hidden state i; ``after_stage(i)`` -> rows issued once
    hidden state i is enqueued (the denoiser's side-stream blocks)."""
    fp16, N = c["dtype"] == "fp16", c["N"]
    rows = []
    t = (lambda i: None) if toff is None else (lambda i: toff[f"vit{i}"])
    e = (lambda i: None) if emb is None else (lambda i: emb[i])
    rows.append(_row(f"{net}.pe", "patch_embed", "mfma" if fp16 else "fmaf", (xin, 0, cin_packed), outs[0], t=t(0), emb=e(0), x="stream[0]"))
    rows += after_stage(0) if after_stage else []
    for i in range(4):
        C, dims = TOK_C[i], level_dims(c["dims"], i + 1)
        ws, ss = clip_window(dims)
        nw = 1
        for a in range(3):
            nw *= -(-dims[a] // ws[a])
        fused, wide = fp16 and C <= 48, fp16 and C > 48
        x, y = f"stream[{i}]", None
        lin = "token_linear" if fused else "token_gemm" if wide else "linear_f32"
        qkv = "qkv_buf" if fp16 else "tmp.qkv"
        for k in range(2):
            b = f"{net}.s{i}.b{k}"
            shifted = k == 1 and any(ss)
            geom = f"w{ws[0]}.{ws[1]}.{ws[2]} s{ss[0] if shifted else 0}.{ss[1] if shifted else 0}.{ss[2] if shifted else 0}"
            rows.append(_row(f"{b}.gather", "window_gather_norm", geom, (x, 0, C), ("win", 0), y=y))
            rows.append(_row(f"{b}.qkv", lin, _form(c, f"{b}.qkv") if wide else "plain", ("win", 0, C), (qkv, 0)))
            rows.append(_row(f"{b}.attn", "window_attention", attention_form(N * nw, HEADS[i], shifted), (qkv, 0, 3 * C), ("att", 0)))
            if fused:
                rows.append(_row(f"{b}.proj", "token_linear", "scatter " + geom, ("att", 0, C), ("ln2", 0), x=x))
                rows.append(_row(f"{b}.mlp", "swin_mlp", "fused", ("ln2", 0, C), (x, 0)))
            else:
                po, hid = ("po_buf", "hid_buf") if wide else ("tmp.po", "tmp.h")
                rows.append(_row(f"{b}.proj", lin, _form(c, f"{b}.proj") if wide else "plain", ("att", 0, C), (po, 0)))
                rows.append(_row(f"{b}.scatter", "window_scatter_add_norm", geom, (po, 0, C), ("ln2", 0), x=x))
                rows.append(_row(f"{b}.fc1", lin, _form(c, f"{b}.fc1") if wide else "gelu", ("ln2", 0, C), (hid, 0)))
                if wide:
                    rows.append(_row(f"{b}.fc2", lin, _form(c, f"{b}.fc2"), (hid, 0, 4 * C), (x, 0)))
                else:
                    rows.append(_row(f"{b}.fc2", lin, "plain", (hid, 0, 4 * C), ("tmp.y", 0)))
                    y = "tmp.y"
        ntok = N
        for d in dims:
            ntok *= (d + 1) // 2
        red = "red_buf" if fp16 else "tmp.red"
        rows.append(_row(f"{net}.s{i}.merge", "patch_merge_norm", merge_form(C, ntok), (x, 0, C), ("merged", 0), y=y))
        rows.append(_row(f"{net}.s{i}.red", "token_gemm" if fp16 else "linear_f32", _form(c, f"{net}.s{i}.red") if fp16 else "plain",
                         ("merged", 0, 8 * C), (red, 0)))
        rows.append(_row(f"{net}.s{i}.out", "stage_out", "", (red, 0, 2 * C), outs[i + 1], t=t(i + 1), emb=e(i + 1),
                         x=f"stream[{i + 1}]" if i < 3 else None))
        rows += after_stage(i + 1) if after_stage else []
    return rows


def _res_rows(c, name, cin, cout, has3, x, out, out_off=0, t=None, post_add=None, ra=None, side=False, defer=False, up=None,
              res_up=False, tap=False, up_c=None):
    """UnetResBlock.forward on channels [0, cin) of ``x``."""
    fp16 = c["dtype"] == "fp16"
    raw1, raw2, res3 = ("raw1b", "raw2b", "res3b") if side else ("raw1", "raw2", "res3")
    bg = "/bg" if side else ""
    rows = []
    if up is not None:
        rows.append(_row(f"{name}.conv1", "upconv_k3", "fold", (x, cin - cout, cout), (raw1, 0), up=up, stats=f"{name}.st0"))
    else:
        rows.append(_row(f"{name}.conv1", "conv3d_k3", _form(c, f"{name}.conv1") + ("/tap" if tap else "") + bg, (x, 0, cin), (raw1, 0),
                         stats=f"{name}.st0"))
    rows.append(_row(f"{name}.conv2", "conv3d_k3", _form(c, f"{name}.conv2") + bg, (raw1, 0, cout), (raw2, 0), norm=f"{name}.st0", t=t,
                     stats=f"{name}.st1"))
    res, res_norm = x, None
    if has3:
        res, res_norm = res3, f"{name}.st2"
        if up is not None and res_up:
            rows.append(_row(f"{name}.conv3", "deconv_res", "res", (up, 0, up_c), (res3, 0), skip=(x, cin - cout, cout), stats=f"{name}.st2"))
        elif fp16 and cout <= 64 and cin <= 384:
            rows.append(_row(f"{name}.conv3", "token_linear", "stats", (x, 0, cin), (res3, 0), stats=f"{name}.st2"))     # background_conv3 = 0
        else:
            rows.append(_row(f"{name}.conv3", "token_gemm" if fp16 else "linear_f32", _form(c, f"{name}.conv3") if fp16 else "plain",
                             (x, 0, cin), (res3, 0)))
            rows.append(_row(f"{name}.sums3", "instnorm_stats", "", (res3, 0, cout), (f"{name}.st2", 0)))
    if not defer:
        rows.append(_row(f"{name}.tail", "residual_norm_act", "bg" if side else "", (raw2, 0, cout), (out, out_off), norm=f"{name}.st1",
                         res=res, res_norm=res_norm, post_add=post_add, ra=ra))
    return rows


def encoder_rows(case):
    c = dict(CASES[case], case=case)
    outs = [(f"e_hs[{i}]", 0) for i in range(5)]
    rows = _swin_rows(c, "enc", "img_in", 8, None, None, outs)
    srcs = ["img_in", "e_hs[0]", "e_hs[1]", "e_hs[2]"]
    for (name, _, cin, cout, has3), x, k in zip(ENC_BLOCKS, srcs, range(4)):
        rows += _res_rows(c, name, cin, cout, has3, x, f"e_enc[{k}]")
    return rows


def denoiser_rows(case):
    c = dict(CASES[case], case=case)
    toff, _ = t_offsets(c["classes"])
    cin0 = -(-(c["classes"] + 1) // 8) * 8
    outs = [("hs[0]", 0), ("hs[1]", 0), ("hs[2]", 0), ("cat[4]", 8 * F), ("hs[4]", 0)]
    den = [("d1", cin0, F, True, "xin"), ("d2", F, F, False, "hs[0]"), ("d3", 2 * F, 2 * F, False, "hs[1]"), ("d4", 4 * F, 4 * F, False, "hs[2]")]

    def side(i):                       # encoder4, 3, 2, 1 go to the side stream once hidden state 2 is enqueued: smallest first
        rows = []
        if i == 2:
            for k in (3, 2, 1, 0):
                name, cin, cout, has3, x = den[k]
                rows += _res_rows(c, name, cin, cout, has3, x, f"cat[{k}]", cout, t=toff[name], post_add=f"e_enc[{k}]", side=True,
                                  tap=c["tap"] and k == 0)
        return rows

    rows = _swin_rows(c, "den", "xin", cin0, toff, [f"e_hs[{i}]" for i in range(5)], outs, side)
    rows += _res_rows(c, "d10", 16 * F, 16 * F, False, "hs[4]", "dec[5]", t=toff["d10"])
    for k in (4, 3, 2, 1, 0):
        name, _, cin, cout = UP_BLOCKS[k]
        if not c["res_up"][k]:
            rows.append(_row(f"up{k + 1}", "deconv_k2s2", _form(c, f"up{k + 1}"), (f"dec[{k + 1}]", 0, DEC_C[k + 1]), (f"cat[{k}]", 0)))
        ra = (f"cat[{k}]", cout) if k < 4 else None
        up = f"dec[{k + 1}]" if c["fold"][k] else None
        defer = k == 0 and c["fused_tail"]
        rows += _res_rows(c, name, cin, cout, True, f"cat[{k}]", f"dec[{k}]", t=toff[name], ra=ra, defer=defer, up=up,
                          res_up=c["res_up"][k], up_c=DEC_C[k + 1])
    if c["fused_tail"]:
        rows.append(_row("out", "final_conv_sampler", "mfma residual", ("raw2", 0, F), ("logits", 0), norm="u1.st1", res="res3",
                         res_norm="u1.st2", ra=("cat[0]", F)))
    else:
        rows.append(_row("out", "final_conv_sampler", "valu identity", ("dec[0]", 0, 64), ("logits", 0)))
    return rows


def sequence(case, network):
    return encoder_rows(case) if network == "encoder" else denoiser_rows(case)


def key(row):
    """What the recorded and the expected row are compared by (everything but the ratio)."""
    return (row["name"], row["op"], row["form"], tuple(row["src"]), tuple(row["dst"]), tuple(sorted((k, str(v)) for k, v in row["extra"].items())))
