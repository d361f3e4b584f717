"""dua_head_fwd (the training head's forward pass) at the shapes of test_head_forward_backward_match_torch, both types: every
element against the fp64 contraction of the operands as the kernel rounds them (fp16 with 32 or 64 channels: the weights go
through fp16 MFMA operands; otherwise they stay fp32), within fp64ref.bound with the chain read off csrc/head.hip
(fp64ref.head_fwd_chain).  Channels of a wider logits buffer beyond K keep their sentinel.  CPU controls:
test_deconv_materialize_fp64ref.py."""
import pytest
import torch

import fp64ref as R

pytestmark = pytest.mark.gpu

SHAPES = [(2, 8, 8, 8, 64, 16), (1, 3, 5, 7, 8, 2), (2, 6, 4, 10, 32, 13), (1, 5, 7, 9, 64, 16), (2, 4, 4, 5, 64, 11),
          (1, 16, 24, 20, 64, 16)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("shape", SHAPES)
def test_head_forward_within_fp64_bound(dtype, shape):
    from diff_unet_amos_amd import ops
    N, D, H, W, C, K = shape
    g = torch.Generator().manual_seed(sum(shape))
    u = (torch.randn(N, D, H, W, C, generator=g) * 1.5 + 0.25).to(dtype).cuda()
    w = (torch.randn(K, C, generator=g) * 0.2).cuda()
    b = torch.randn(K, generator=g).cuda()
    out = ops.head_fwd(u, w, b)
    wide = torch.full((N, D, H, W, K + 3), 5.0, dtype=dtype, device="cuda")
    ops.head_fwd(u, w, b, out=wide)
    torch.cuda.synchronize()
    assert torch.equal(wide[..., :K], out) and bool((wide[..., K:] == 5.0).all())
    ref, ab, sq = R.head_fwd_ref(u.cpu().double().reshape(-1, C), w, b, dtype)
    bnd = R.bound(ref, ab, sq, R.head_fwd_chain(C, dtype), dtype)
    res = R.check(out.cpu().reshape(-1, K), ref, bnd)
    print(f"\nhead fwd {R.head_fwd_route(C, dtype)} {dtype} {N}x{D}x{H}x{W} {C}->{K} elements={ref.numel()} {res}")
    assert res.ratio <= 1, res
