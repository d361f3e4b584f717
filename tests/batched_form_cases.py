"""The 3x3x3 convolution forms that only a batch reaches, at the smallest shapes that reach them: cases, inputs and the fp64
reference over EVERY output voxel.  Shared by tests/test_batched_forms_fp64.py (GPU: the kernels against the reference) and
tests/test_batched_forms_defects.py (CPU: the same inputs, the reference with one planted batch mix-up at a time).

A plain helper module of the suite.  The reference is the one of tests/fp64ref.py -- exact operands, weights rounded as the packer
rounds them, the fused transform emulated in the kernel's arithmetic, the same ``bound`` -- written as 27 shifted products over a
zero-padded activation tensor instead of a gather per point, so that every voxel of a volume is affordable and the padding planes
are a tensor a test can tamper with.  It runs on whatever device the padded tensor lives on.

Why these shapes (dua_conv3d_k3_form, fp16, policy 0, 256 compute units, the split-K workspace of the 96^3 plan of that batch):
the form is chosen from the workgroup count tiles x output-channel tiles x N.

* 12^3 256 -> 256 has 8 tiles of 4x8x8 and 4 channel tiles: 32 N workgroups.  N = 1 splits K (V2_4_KD); N = 2 takes two-deep tiles
  with kd planes (V2_2_KD, 192 workgroups); N = 3 and 4 have 288 / 384 two-deep workgroups, past the 256 the kd-plane kernel is
  kept to: V2_2.  10^3 has the same tile counts at N = 4 (20 two-deep tiles, 320 workgroups) and ragged tiles on every axis.
* 6^3 512 -> 512 always splits K; the split falls with N (16, 8, 5, 4) while grid_z = N * ksplit stays near 16.
* 24^3 has 54 four-deep tiles: N = 1 takes two-deep kd-plane tiles, N >= 2 four-deep tiles without a split (V2_4).
* The wide-tile form needs 48^3 at N = 1 or 2, 40^3 at N = 3 and 32^3 at N = 4 (24^3 stays V2_4): 64 tiles x 2 channel tiles x 4.
"""
from __future__ import annotations

import itertools
import zlib

import torch

import conv_form_cases as K
import fp64ref as R

F16 = torch.float16

# name -> (N, dims, Cin, Cout, fused producer, (kernel, tile depth, ksplit), grid)
CONV_CASES = {
    "v2_2-12c-256-fused": (4, (12, 12, 12), 256, 256, True, ("V2_2", 2, 1), (24, 4, 4)),          # d3b / u3b at N = 4
    "v2_2-12c-512": (4, (12, 12, 12), 512, 256, False, ("V2_2", 2, 1), (24, 4, 4)),               # u3a at N = 4
    "v2_2-10c-256-fused": (4, (10, 10, 10), 256, 256, True, ("V2_2", 2, 1), (20, 4, 4)),
    "v2_2_kd-12c-256-fused": (2, (12, 12, 12), 256, 256, True, ("V2_2_KD", 2, 1), (24, 4, 2)),    # d3b / u3b at N = 2
    "v2_2_kd-10c-256-fused": (2, (10, 10, 10), 256, 256, True, ("V2_2_KD", 2, 1), (20, 4, 2)),
    "v2_4_kd-6c-512-split4-fused": (4, (6, 6, 6), 512, 512, True, ("V2_4_KD", 4, 4), (2, 8, 16)),  # d4b at N = 4
    "v2_4-24c-128-128-fused": (2, (24, 24, 24), 128, 128, True, ("V2_4", 4, 1), (54, 2, 2)),      # d2b / u2b at N = 2
    "v2_4-24c-128-256-fused": (2, (24, 24, 24), 128, 256, True, ("V2_4", 4, 1), (54, 4, 2)),
    "v2_4-24c-256-256-fused": (2, (24, 24, 24), 256, 256, True, ("V2_4", 4, 1), (54, 4, 2)),
    "wide-32c-64-128": (4, (32, 32, 32), 64, 128, False, ("WIDE", 8, 1), (64, 2, 4)),
    "wide-32c-128-128-fused": (4, (32, 32, 32), 128, 128, True, ("WIDE", 8, 1), (64, 2, 4)),
}
# the folded up-convolution at 24^3 with 27 * 4 * 2 = 216 tiles: (N, fine dims, Cskip, coarse channels Cu, Cmid of the transposed
# convolution, Cout).  All 27 border classes of the bias table occur at 24^3.
FOLD_CASE = (4, (24, 24, 24), 128, 128, 128, 128)
ADD_PAD = 8                                # the add rows are wider than the slice a consumer reads


def plan_workspace(nv, N):
    """Bytes of split-K workspace the default-width fp16 96^3 plan of batch N allocates: the largest dua_conv3d_k3_workspace of its
    convolutions (engine.Plan._alloc_stats)."""
    import ctypes
    exp = dict(N=N, dims=(96, 96, 96), dtype=F16, fold=[True, True, False, False], layout=(True, True, True))
    return max([16] + [int(nv.lib().dua_conv3d_k3_workspace(ctypes.byref(nv.Conv3Desc(*d))))
                       for _, kind, d, _, _ in K.plan_launches("", exp) if kind == "conv"])


def per_sample(x):
    """Sample n scaled by 1 + 0.5 n and moved by 0.3 n - 0.2: InstanceNorm scales go with 1 / std, shifts with the mean."""
    for n in range(x.shape[0]):
        x[n] = x[n] * (1 + 0.5 * n) + (0.3 * n - 0.2)
    return x


def conv_inputs(name):
    """Host tensors of a case: x fp16 [N, D, H, W, Cin] (the raw tensor of a producer if fused, else the activation), w, b of the
    convolution, gamma, beta of the producer and its per-sample add rows [N, Cin + ADD_PAD]."""
    N, dims, cin, cout, fused = CONV_CASES[name][:5]
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    x = per_sample(torch.randn(N, *dims, cin, generator=g)).half()
    w = torch.randn(cout, cin, 3, 3, 3, generator=g) / (27 * cin) ** 0.5
    b = torch.randn(cout, generator=g) * 0.5
    gamma = torch.rand(cin, generator=g) + 0.5
    beta = torch.randn(cin, generator=g) * 0.5
    add = torch.randn(N, cin + ADD_PAD, generator=g)
    return dict(x=x, w=w, b=b, gamma=gamma, beta=beta, add=add)


def fold_inputs():
    """Host tensors of FOLD_CASE: skip [N, D, H, W, Cskip] fp16 (an activation), u [N, D/2, H/2, W/2, Cu] fp16 (the raw coarse tensor of
    a producer), wc / bc of the convolution over cat(skip, upsampled), wd / bd of the transposed convolution, the producer's
    gamma, beta and add rows."""
    N, dims, cskip, cu, cmid, cout = FOLD_CASE
    g = torch.Generator().manual_seed(zlib.crc32(b"fold-24c"))
    skip = per_sample(torch.randn(N, *dims, cskip, generator=g)).half()
    u = per_sample(torch.randn(N, *(s // 2 for s in dims), cu, generator=g)).half()
    wc = torch.randn(cout, cskip + cmid, 3, 3, 3, generator=g) / (27 * (cskip + cmid)) ** 0.5
    bc = torch.randn(cout, generator=g) * 0.5
    wd = torch.randn(cu, cmid, 2, 2, 2, generator=g) / cu ** 0.5
    bd = torch.randn(cmid, generator=g) * 0.5
    gamma = torch.rand(cu, generator=g) + 0.5
    beta = torch.randn(cu, generator=g) * 0.5
    add = torch.randn(N, cu + ADD_PAD, generator=g)
    return dict(skip=skip, u=u, wc=wc, bc=bc, wd=wd, bd=bd, gamma=gamma, beta=beta, add=add)


def host_consts(raw, gamma, beta, add):
    """fp32 (scale, shift, add) [N, C] of a producer from fp64 sums of its raw tensor: what the consumers' preamble forms, to the
    preamble's rounding (the GPU tests take the preamble's own values from ops.instnorm_finalize)."""
    C = gamma.numel()
    sc, sh, _, _ = R.finalize(R.channel_sums(raw), gamma, beta, raw[0, ..., 0].numel())
    return sc.float(), sh.float(), add[:, :C].float()


def activation(raw, consts, rows=None):
    """float64 activation a kernel multiplies: raw (fp16, host) through the emulated transform with sample n using the constants of
    sample rows[n] (None: its own); ``consts`` None: raw is the activation."""
    if consts is None:
        return raw.double()
    N, C = raw.shape[0], raw.shape[-1]
    idx = torch.arange(N) if rows is None else torch.as_tensor(rows)
    shape = (N,) + (1,) * (raw.dim() - 2) + (C,)
    sc, sh, ad = (t[idx].reshape(shape) for t in consts)
    return R.transform(raw.double(), sc, sh, ad, F16)


def padded(act, d_halo_from_neighbours=False):
    """[N, D + 2, H + 2, W + 2, C]: the activation inside zeros.  ``d_halo_from_neighbours``: the planes before the first and behind
    the last plane of a sample hold what lies there in memory -- the last plane of the sample before, the first of the next --
    instead of zeros (the first sample's low face and the last one's high face have no neighbour in the buffer)."""
    N, D, H, W, C = act.shape
    p = torch.zeros((N, D + 2, H + 2, W + 2, C), dtype=torch.float64, device=act.device)
    p[:, 1:-1, 1:-1, 1:-1] = act
    if d_halo_from_neighbours:
        p[1:, 0, 1:-1, 1:-1] = act[:-1, D - 1]
        p[:-1, D + 1, 1:-1, 1:-1] = act[1:, 0]
    return p


def conv3_sums(pad, Wm, bias=None, sel=None):
    """3x3x3 convolution of a padded activation tensor with Wm [27 Cin, Cout] (fp64ref.conv3_weights) as 27 shifted products:
    (sum, sum |terms|, sum terms^2), each [N D H W, Cout] in fp64ref.all_voxels order -- or [P, Cout] at the voxels ``sel`` [P, 4].
    The bias is one more term of the sum."""
    N, Dp, Hp, Wp, C = pad.shape
    D, H, W = Dp - 2, Hp - 2, Wp - 2
    Wm = Wm.to(pad.device)
    ref = ab = sq = 0
    for t, (kd, kh, kw) in enumerate(itertools.product(range(3), repeat=3)):
        xs = pad[:, kd:kd + D, kh:kh + H, kw:kw + W]
        xs = xs.reshape(-1, C) if sel is None else xs[sel[:, 0], sel[:, 1], sel[:, 2], sel[:, 3]]
        Wt = Wm[t * C:(t + 1) * C]
        ref = ref + xs @ Wt
        ab = ab + xs.abs() @ Wt.abs()
        sq = sq + (xs * xs) @ (Wt * Wt)
    if bias is not None:
        bb = bias.detach().double().to(pad.device)[None]
        ref, ab = ref + bb, ab + bb.abs()
    return ref, ab, sq


def split_rows(cin, units_per_split, part):
    """Rows of Wm [27 Cin, Cout] that split-K partial ``part`` contracts: units u = chunk * 3 + kd of 32 channels x one kd plane,
    units [part * units_per_split, (part + 1) * units_per_split) (csrc/conv3d_igemm.hip)."""
    nch = -(-cin // 32)
    keep = torch.zeros(27, cin, dtype=torch.bool)
    for u in range(part * units_per_split, min(3 * nch, (part + 1) * units_per_split)):
        chunk, kd = divmod(u, 3)
        keep[kd * 9:(kd + 1) * 9, chunk * 32:min(cin, (chunk + 1) * 32)] = True
    return keep.reshape(-1)


def conv_bound(ref, ab, sq, cin, fused, ksplit):
    """fp64ref.bound of a 27 Cin contraction.  With split-K every partial is a chain no longer than the whole contraction's and the
    finish kernel adds the ksplit partials to the bias one after the other: ksplit more links."""
    return R.bound(ref, ab, sq, R.chain_length(27 * cin, F16, ksplit if ksplit > 1 else 0), F16, emulated_in=F16 if fused else None)


def fold_sums(skip_sums, dims, u_act, Wp, bias_rows, bias_abs):
    """The folded up-convolution over every voxel: the skip half as a 3x3x3 convolution (``skip_sums`` = conv3_sums of it without a
    bias, left unchanged), the composed weights Wp[(phi, delta)] [Cout, Cu] (fp64ref.decode_fold_weights / compose_fold) over the
    eight parents m + delta - 1 + phi of output voxel 2 m + phi (zero outside the coarse volume), the border-class bias rows
    [27, Cout].  Returns (sum, sum |terms|, sum terms^2, the bias rows' |terms|) as [N, D, H, W, Cout]."""
    N, (D, H, W) = u_act.shape[0], dims
    dev = skip_sums[0].device
    ref, ab, sq = (t.reshape(N, D, H, W, -1).clone() for t in skip_sums)
    up = padded(u_act.to(dev))
    Dc, Hc, Wc = D // 2, H // 2, W // 2
    for phi in itertools.product(range(2), repeat=3):
        for delta in itertools.product(range(2), repeat=3):
            o = [p + d for p, d in zip(phi, delta)]            # padded index of parent m + delta - 1 + phi is m + delta + phi
            xs = up[:, o[0]:o[0] + Dc, o[1]:o[1] + Hc, o[2]:o[2] + Wc]
            m = Wp[phi + delta].to(dev).t()
            view = (slice(None), slice(phi[0], None, 2), slice(phi[1], None, 2), slice(phi[2], None, 2))
            ref[view] += xs @ m
            ab[view] += xs.abs() @ m.abs()
            sq[view] += (xs * xs) @ (m * m)
    cls = R.border_class(R.all_voxels(N, (D, H, W)), (D, H, W)).to(dev)
    rows = bias_rows.to(dev)[cls].reshape(N, D, H, W, -1)
    arows = bias_abs.to(dev)[cls].reshape(N, D, H, W, -1)
    return ref + rows, ab + arows, sq, arows
