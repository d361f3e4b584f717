"""dua_deconv_k2s2_fwd / dua_deconv_k2s2_pad_fwd in each of their three forms -- one tap per workgroup, k-split, all taps (128-voxel
tiles) -- against an fp64 reference on the operands the kernel read, per element, within the bound derived from the
form's arithmetic (tests/fp64ref.py: deconv_fwd_chain, bound; the CPU controls are in test_deconv_materialize_fp64ref.py).  fp16
and fp32, with and without a fused producer transform (per-sample statistics rows and additive term, N = 2), with and without
replicate-pad planes, channels-last and 16-channel-block output, channel slices inside wider buffers.  Every case asserts the form it
reached (the launcher's own answer), that channels outside its slice keep their sentinel and that a second launch is bit-equal.
Every output voxel is checked up to 32 768 voxels per sample, above that the structured sample of fp64ref.sample_voxels.

One printed row per case: form, shape, points, max |err| / bound and the worst element."""
import ctypes
import zlib

import pytest
import torch

import fp64ref as R

pytestmark = pytest.mark.gpu

F16, F32 = torch.float16, torch.float32
ONE_TAP, KSPLIT, ALL128 = range(3)                         # dua_deconv_form.kernel
FORM = {ONE_TAP: "one_tap", KSPLIT: "ksplit", ALL128: "alltaps"}
KIND = {ONE_TAP: 0, KSPLIT: 1, ALL128: 2}                  # dua_deconv_k2s2_kernel_kind
NAME = {ONE_TAP: "one-tap", KSPLIT: "k-split", ALL128: "all-taps 128"}
CIN_OFF, COUT_OFF, SENTINEL = 8, 16, 9.0


def _ops():
    from diff_unet_amos_amd import ops
    return ops


@pytest.fixture
def deconv_policy(request):
    """ops.CONV_POLICY for one case, restored afterwards."""
    ops = _ops()
    ops.CONV_POLICY = request.param
    yield request.param
    ops.CONV_POLICY = 0


def _case(kernel, dtype, N, cin, cout, dims, fused=False, pad=(0, 0, 0), blocked=False):
    dt = "f16" if dtype == F16 else "f32"
    tag = f"{NAME[kernel]} {dt} {N}x{'x'.join(map(str, dims))} {cin}->{cout}{' fused' if fused else ''}"
    if any(pad):
        tag += f" pad{''.join(map(str, pad))}"
    if blocked:
        tag += " blocked"
    return pytest.param(0, kernel, dtype, N, cin, cout, dims, fused, pad, blocked, id=tag.replace(" ", "-"))


def _both(kernel, dtype, cin, cout, dims, N=1):
    """unfused at N, and fused with two samples"""
    return [_case(kernel, dtype, N, cin, cout, dims), _case(kernel, dtype, 2, cin, cout, dims, fused=True)]


PADS = [(0, 0, 1), (1, 1, 0), (1, 1, 1)]
CASES = []
for _dt in (F16, F32):
    # one tap per workgroup: ragged chunk, ragged voxel tile, two output-channel tiles (the second 8 wide); a second, ragged voxel
    # tile; just under the all-taps threshold of 32 768 coarse voxels (a large grid)
    CASES += _both(ONE_TAP, _dt, 40, 72, (2, 4, 6), N=2) + _both(ONE_TAP, _dt, 64, 32, (7, 9, 5)) + _both(ONE_TAP, _dt, 32, 24, (31, 32, 33))
    # all taps, 128-voxel tiles: exact tiles; ragged in every way
    CASES += _both(ALL128, _dt, 64, 64, (32, 32, 32)) + _both(ALL128, _dt, 40, 72, (30, 34, 36))
    CASES += [_case(k, _dt, 2, 40, 72, (2, 4, 6), fused=True, pad=p) for k in (ONE_TAP,) for p in PADS]
    CASES += [_case(ALL128, _dt, 2, 40, 72, (30, 34, 36), fused=True, pad=p) for p in PADS]
    CASES += [_case(ALL128, _dt, 1, 64, 64, (32, 32, 32), blocked=True), _case(ALL128, _dt, 2, 40, 72, (30, 34, 36), fused=True, blocked=True)]
# 17 chunks: past the k-split range, back on one tap per workgroup (fp16: 544 channels, fp32: 272)
CASES += _both(ONE_TAP, F16, 544, 40, (2, 2, 3)) + _both(ONE_TAP, F32, 272, 72, (2, 3, 3), N=2)
# k-split (8..16 chunks): ragged last chunk; the 6^3 x 512 layer; 16 chunks; fp32: 9 chunks of 16, 16 chunks
CASES += _both(KSPLIT, F16, 272, 72, (2, 3, 3), N=2) + _both(KSPLIT, F16, 512, 256, (6, 6, 6)) + _both(KSPLIT, F16, 512, 40, (2, 2, 3))
CASES += _both(KSPLIT, F32, 136, 64, (3, 4, 5)) + _both(KSPLIT, F32, 256, 72, (2, 3, 3), N=2)
CASES += [_case(KSPLIT, F16, 2, 272, 72, (2, 3, 3), fused=True, pad=p) for p in PADS]
CASES += [_case(KSPLIT, F32, 2, 136, 64, (3, 4, 5), fused=True, pad=p) for p in PADS]
# all taps: 4 chunks, the limit (fp16 128 channels; fp32 64 channels is the 64 -> 64 case above)
CASES += _both(ALL128, F16, 128, 32, (32, 32, 32))


def _producer(x, cin, dtype, g):
    """A producer whose raw output is channels [CIN_OFF, CIN_OFF + cin) of x: its statistics words spread over the replica rows
    (per sample), affine parameters away from (1, 0), a per-sample additive term in rows wider than the slice."""
    ops = _ops()
    N = x.shape[0]
    v = x[..., CIN_OFF:CIN_OFF + cin].double().reshape(N, -1, cin)
    stats = ops.stats_buffer(N, cin, "cuda")
    for r in range(8):
        stats[:, r] = ops.stats_encode(R.channel_sums(v[:, r::8]))[:, 0].cuda()
    gamma = (torch.rand(cin, generator=g) + 0.5).cuda()
    beta = (torch.randn(cin, generator=g) * 0.5).cuda()
    add = torch.randn(N, cin + 8, generator=g).cuda()
    return ops.Norm(stats, gamma, beta, v.shape[1], add=add, add_stride=cin + 8)


def _consts(norm, N, tag):
    """The preamble's fp32 scale / shift (ops.instnorm_finalize), held to fp64 values from the decoded statistics words, and add."""
    ops = _ops()
    stats, gamma, beta, add = norm.keep
    C = gamma.numel()
    sc64, sh64, b_sc, b_sh = R.finalize(ops.stats_decode(stats).cpu(), gamma.cpu(), beta.cpu(), norm.c.count, norm.c.eps)
    sc, sh = (t.cpu() for t in ops.instnorm_finalize(norm, N, C))
    for what, got, ref, b in (("scale", sc, sc64, b_sc), ("shift", sh, sh64, b_sh)):
        r = R.check(got, ref, b)
        assert r.ratio <= 1, f"{tag}: InstanceNorm {what} of the preamble: {r}"
    return sc, sh, add.cpu()[:, :C]


@pytest.mark.parametrize("deconv_policy,kernel,dtype,N,cin,cout,dims,fused,pad,blocked", CASES, indirect=["deconv_policy"])
def test_deconv_forward_within_fp64_bound(deconv_policy, kernel, dtype, N, cin, cout, dims, fused, pad, blocked, request):
    from diff_unet_amos_amd import _native as nv
    ops = _ops()
    tag = request.node.callspec.id
    g = torch.Generator().manual_seed(zlib.crc32(tag.encode()))
    D, H, W = dims
    out_dims = tuple(2 * s + p for s, p in zip(dims, pad))
    cs_in = CIN_OFF + cin + 8
    cs_out = -(-(COUT_OFF + cout + 16) // 16) * 16
    x = torch.randn(N, D, H, W, cs_in, generator=g) * 1.5 + 0.25
    if N == 2:
        x[1] = x[1] * 1.7 - 0.5                              # another mean and variance per sample
    x = x.to(dtype).cuda()
    w = torch.randn(cin, cout, 2, 2, 2, generator=g) / cin ** 0.5
    b = torch.randn(cout, generator=g)
    norm = _producer(x, cin, dtype, g) if fused else None
    wp, bp = ops.pack_deconv_weights(w.cuda(), b.cuda(), dtype)

    # the form this very launch takes, by the launcher's own rule
    d = nv.Conv3Desc(nv.dt_code(dtype), N, D, H, W, cin, cs_in, CIN_OFF, cout, cs_out, COUT_OFF, 0, 0,
                     nv.OUT_BLOCKED if blocked else 0, deconv_policy)
    f = nv.DeconvForm()
    nv.check(nv.lib().dua_deconv_k2s2_form(ctypes.byref(d), 1 if fused else 0, *out_dims, ctypes.byref(f)), "dua_deconv_k2s2_form")
    assert f.kernel == kernel, f"{tag}: the launcher takes form {f.kernel}, the case is meant for {kernel}"
    assert ops.deconv_kernel_kind(dtype, N, D, H, W, cin, cout) == KIND[kernel]

    def launch():
        y = torch.full((N, *out_dims, cs_out), SENTINEL, dtype=dtype, device="cuda")
        ops.deconv_k2s2(x, cin, CIN_OFF, wp, bp, cout, y, COUT_OFF, norm=norm, out_blocked=blocked)
        return y
    y = launch()
    y2 = launch()
    torch.cuda.synchronize()
    assert torch.equal(y, y2), f"{tag}: two launches differ"
    yc = ops.from_blocked(y) if blocked else y
    outside = torch.cat([yc[..., :COUT_OFF], yc[..., COUT_OFF + cout:]], -1)
    assert bool((outside == SENTINEL).all()), f"{tag}: channels outside the slice were written"

    nvox = out_dims[0] * out_dims[1] * out_dims[2]
    pts = R.all_voxels(N, out_dims) if nvox <= 32768 else R.sample_voxels(N, out_dims, n_random=1000, seed=zlib.crc32(tag.encode()))
    parent, child = R.deconv_sources(pts, dims)
    A = R.gather_points(x, parent, CIN_OFF, cin)
    if fused:
        sc, sh, ad = _consts(norm, N, tag)
        n = pts[:, 0]
        A = R.transform(A, sc[n], sh[n], ad[n], dtype)
    ref, ab, sq = R.deconv_ref_by_child(A, w, b, dtype, child)
    bnd = R.bound(ref, ab, sq, R.deconv_fwd_chain(FORM[kernel], cin, dtype), dtype, emulated_in=dtype if fused else None)
    res = R.check(R.gather_points(yc, pts, COUT_OFF, cout), ref, bnd, pts)
    print(f"\n{NAME[kernel]:13s} {'f16' if dtype == F16 else 'f32'} {N}x{D}x{H}x{W} {cin}->{cout} -> {'x'.join(map(str, out_dims))}"
          f"{' fused' if fused else ''}{' blocked' if blocked else ''} samples={len(pts)} {res}")
    assert res.ratio <= 1, f"{tag}: {res}"


def test_every_form_appears_in_both_types_fused_padded_and_blocked():
    seen = {(p.values[1], p.values[2], p.values[7], any(p.values[8]), p.values[9]) for p in CASES}
    for k in (ONE_TAP, KSPLIT, ALL128):
        for dt in (F16, F32):
            assert (k, dt, False, False, False) in seen and (k, dt, True, False, False) in seen, (k, dt)
            assert (k, dt, True, True, False) in seen, (k, dt)
    for dt in (F16, F32):
        assert any(s[0] == ALL128 and s[1] == dt and s[4] for s in seen), dt
