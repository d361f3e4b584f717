"""dua_materialize standalone: every element against LeakyReLU(raw scale + shift) + add (+ emb) in fp64 on the kernel's own fp32
constants (which are themselves held to fp64 values from the statistics words), within fp64ref.materialize_bound; the pooled output
bit-equal to the floor MaxPool3d(2) of the stored output and within the window's largest bound of the fp64 maximum.  fp16 and fp32,
channels-last and (fp16) 16-channel-block output, every buffer wider than the slice, two samples with different statistics, with
and without the embedding and the per-sample additive term, even and odd extents, and one case whose channels have mean ~50 and
standard deviation ~0.5 (scale x raw and shift cancel).  CPU controls: test_deconv_materialize_fp64ref.py."""
import zlib

import pytest
import torch
import torch.nn.functional as F

import fp64ref as R

pytestmark = pytest.mark.gpu

F16, F32 = torch.float16, torch.float32
SENTINEL = 4.0
EXTENTS = [(2, 3, 2), (4, 6, 8), (7, 11, 13), (33, 35, 40)]
# C, out_off, emb, add, pool
VARIANTS = [(24, 8, True, True, True), (24, 8, False, False, False), (32, 16, True, False, True), (32, 16, False, True, False)]
LAYOUTS = [(F16, False), (F32, False), (F16, True)]
CASES = [pytest.param(dt, blk, dims, *v, False, id=f"{'f16' if dt == F16 else 'f32'}{'-blocked' if blk else ''}-{'x'.join(map(str, dims))}-"
                      f"C{v[0]}{'-emb' if v[2] else ''}{'-add' if v[3] else ''}{'-pool' if v[4] else ''}")
         for dt, blk in LAYOUTS for dims in EXTENTS for v in VARIANTS if not blk or v[0] % 16 == 0]
CASES += [pytest.param(dt, False, (7, 11, 13), 24, 8, True, True, True, True, id=f"{'f16' if dt == F16 else 'f32'}-cancellation")
          for dt in (F16, F32)]


def _ops():
    from diff_unet_amos_amd import ops
    return ops


@pytest.mark.parametrize("dtype,blocked,dims,C,out_off,with_emb,with_add,pool,cancel", CASES)
def test_materialize_within_fp64_bound(dtype, blocked, dims, C, out_off, with_emb, with_add, pool, cancel, request):
    ops = _ops()
    tag = request.node.callspec.id
    g = torch.Generator().manual_seed(zlib.crc32(tag.encode()))
    N, (D, H, W) = 2, dims
    rs, es, ps = C + 8, C + 16, C + 8
    os_ = -(-(out_off + C + 16) // 16) * 16
    raw = torch.randn(N, D, H, W, rs, generator=g)
    if cancel:
        raw = raw * 0.5 + 50.0
    else:
        raw = raw * torch.tensor([1.5, 2.5]).view(2, 1, 1, 1, 1) + torch.tensor([0.25, -0.5]).view(2, 1, 1, 1, 1)
    raw = raw.to(dtype).cuda()
    emb = torch.randn(N, D, H, W, es, generator=g).to(dtype).cuda() if with_emb else None
    V = D * H * W
    v = raw[..., :C].double().reshape(N, V, C).cpu()
    stats = ops.stats_buffer(N, C, "cuda")
    for r in range(8):
        stats[:, r] = ops.stats_encode(R.channel_sums(v[:, r::8]))[:, 0].cuda()
    gamma = (torch.rand(C, generator=g) + 0.5).cuda()
    beta = (torch.randn(C, generator=g) * 0.5).cuda()
    add = torch.randn(N, C + 8, generator=g).cuda() if with_add else None
    norm = ops.Norm(stats, gamma, beta, V, add=add, add_stride=C + 8 if with_add else 0)

    # the constants the kernel derives, held to fp64 values from the words it reads
    sc64, sh64, b_sc, b_sh = R.finalize(ops.stats_decode(stats).cpu(), gamma.cpu(), beta.cpu(), V, norm.c.eps)
    sc, sh = (t.cpu() for t in ops.instnorm_finalize(norm, N, C))
    for what, got, ref, b in (("scale", sc, sc64, b_sc), ("shift", sh, sh64, b_sh)):
        r = R.check(got, ref, b)
        assert r.ratio <= 1, f"{tag}: InstanceNorm {what} of the preamble: {r}"
    ad = add.cpu()[:, :C] if with_add else torch.zeros(N, C)

    out = torch.full((N, D, H, W, os_), SENTINEL, dtype=dtype, device="cuda")
    pooled = torch.full((N, D // 2, H // 2, W // 2, ps), SENTINEL, dtype=dtype, device="cuda") if pool else None
    ops.materialize(raw, C, norm, out, out_off, emb=emb, pooled=pooled, out_blocked=blocked)
    torch.cuda.synchronize()
    oc = (ops.from_blocked(out) if blocked else out).cpu()
    assert bool((oc[..., :out_off] == SENTINEL).all()) and bool((oc[..., out_off + C:] == SENTINEL).all()), f"{tag}: wrote outside its slice"

    b5 = lambda t: t[:, None, None, None, :]          # noqa: E731
    ref, mag = R.materialize_ref(raw[..., :C].cpu().double(), b5(sc), b5(sh), b5(ad), emb[..., :C].cpu().double() if with_emb else None)
    bnd = R.materialize_bound(ref, mag, dtype)
    got = oc[..., out_off:out_off + C]
    res = R.check(got, ref, bnd)
    if pool:
        pc = pooled.cpu()
        assert bool((pc[..., C:] == SENTINEL).all()), f"{tag}: pooled wrote outside its slice"
        want = F.max_pool3d(got.float().permute(0, 4, 1, 2, 3), 2).permute(0, 2, 3, 4, 1)
        assert torch.equal(pc[..., :C].float(), want), f"{tag}: pooled is not the floor max-pool of the stored output"
        pr, pb = R.pool_ref(ref, bnd)
        rp = R.check(pc[..., :C], pr, pb)
        if rp.ratio > res.ratio:
            res = rp
    print(f"\nmaterialize {tag} {N}x{D}x{H}x{W} elements={ref.numel()} {res}")
    assert res.ratio <= 1, f"{tag}: {res}"
