"""The 3x3x3 convolution forms that only a batch reaches (tests/batched_form_cases.py: V2_2 without kd planes under 256- and 512-
channel transform tables, V2_2_KD at 12^3, split-K with grid_z = 16 and a finish over four samples, four-deep V2_4 tiles at 24^3
with two and four output-channel tiles, the wide-tile form with two channel tiles and four samples) and the folded up-convolution at
24^3, each at the smallest shape that reaches it: fp16, policy 0, the split-K workspace of the 96^3 plan of that batch.  Every
case first asserts the form the launcher itself states for the call (kernel, tile depth, split, grid), then holds EVERY output
element to the fp64 reference on the operands the kernel read within the derived bound (tests/fp64ref.py) and the statistics words
to fp64 sums of what was stored.  The samples differ in scale and offset and, where a case is fused, carry per-sample statistics,
and add rows: tests/test_batched_forms_defects.py shows on the same inputs that a row, halo or partial of a neighbouring sample
is hundreds of bounds away.

One printed row per case: form, grid, shape, max |err| / bound, statistics likewise, the worst element."""
import pytest
import torch

import batched_form_cases as B
import fp64ref as R
from test_launch_sequence_fp64 import form_names

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _ops():
    from diff_unet_amos_amd import _native as nv
    from diff_unet_amos_amd import ops
    return nv, ops


def _producer(raw, gamma, beta, add):
    """ops.Norm of a producer whose raw output is ``raw`` (device, fp16): statistics words spread over the eight replica rows per
    sample, the per-sample add rows wider than the slice."""
    nv, ops = _ops()
    N, C = raw.shape[0], raw.shape[-1]
    v = raw.double().reshape(N, -1, C)
    stats = ops.stats_buffer(N, C, DEV)
    for r in range(8):
        stats[:, r] = ops.stats_encode(R.channel_sums(v[:, r::8]))[:, 0]
    return ops.Norm(stats, gamma.to(DEV), beta.to(DEV), v.shape[1], add=add.to(DEV).contiguous(), add_stride=add.shape[1])


def _consts(norm, N, tag):
    """The preamble's own fp32 scale / shift (ops.instnorm_finalize), held to the fp64 values from the decoded words, and add."""
    nv, ops = _ops()
    stats, gamma, beta, add = norm.keep
    C = gamma.numel()
    sc64, sh64, b_sc, b_sh = R.finalize(ops.stats_decode(stats).cpu(), gamma.cpu(), beta.cpu(), norm.c.count, norm.c.eps)
    sc, sh = (t.cpu() for t in ops.instnorm_finalize(norm, N, C))
    for what, got, ref, b in (("scale", sc, sc64, b_sc), ("shift", sh, sh64, b_sh)):
        r = R.check(got, ref, b)
        assert r.ratio <= 1, f"{tag}: InstanceNorm {what} of the preamble: {r}"
    return sc, sh, add.cpu()[:, :C]


def _stats_ratio(y, stats):
    """statistics words against fp64 sums of the stored output, per sample and channel"""
    nv, ops = _ops()
    N, cout = y.shape[0], y.shape[-1]
    v = y.double().reshape(N, -1, cout)
    S, Q, A = v.sum(1), (v * v).sum(1), v.abs().sum(1)
    words = ops.stats_decode(stats)[:, :cout]
    bs, bq = R.stats_bound(A, Q, B.F16, v.shape[1])
    return float(torch.maximum(((words[..., 0] - S).abs() / bs).max(), ((words[..., 1] - Q).abs() / bq).max()))


@pytest.mark.parametrize("name", list(B.CONV_CASES))
def test_batched_conv_form_within_fp64_bound(name):
    nv, ops = _ops()
    N, dims, cin, cout, fused, want, grid = B.CONV_CASES[name]
    D, H, W = dims
    t = B.conv_inputs(name)
    x = t["x"].to(DEV)
    wp, bp = ops.pack_conv3_weights(t["w"].to(DEV).contiguous(), t["b"].to(DEV), B.F16)
    norm = _producer(x, t["gamma"], t["beta"], t["add"]) if fused else None
    ws = torch.empty(B.plan_workspace(nv, N) // 4, dtype=torch.float32, device=DEV)
    ws_bytes = ws.numel() * 4

    # the form this very launch takes, by the launcher's own rule on this device
    assert ops.CONV_POLICY == 0
    d = nv.Conv3Desc(nv.dt_code(B.F16), N, D, H, W, cin, cin, 0, cout, cout, 0, 0, 0, 0, 0)
    f = ops.conv3_form(d, fused, ws_bytes)
    got_form = (form_names(nv)[f.kernel], f.tile_depth, f.ksplit)
    assert got_form == want and (f.grid_x, f.grid_y, f.grid_z) == grid, f"{name}: the launcher takes {got_form} {(f.grid_x, f.grid_y, f.grid_z)}"
    assert f.workspace_needed <= ws_bytes and f.grid_z == N * f.ksplit and f.finish == (1 if f.ksplit > 1 else 0)

    def launch():
        y = torch.full((N, D, H, W, cout), float("nan"), dtype=B.F16, device=DEV)
        stats = ops.stats_buffer(N, cout, DEV)
        ops.conv3d_k3(x, cin, 0, wp, bp, cout, y, 0, stats, norm=norm, workspace=ws)
        return y, stats
    y, stats = launch()
    y2, stats2 = launch()
    torch.cuda.synchronize()
    assert torch.equal(y, y2) and torch.equal(stats, stats2), f"{name}: two launches differ"

    consts = _consts(norm, N, name) if fused else None
    act = B.activation(t["x"], consts).to(DEV)
    ref, ab, sq = B.conv3_sums(B.padded(act), R.conv3_weights(t["w"], B.F16), t["b"])
    bnd = B.conv_bound(ref, ab, sq, cin, fused, f.ksplit)
    res = R.check(y.reshape(-1, cout), ref, bnd, R.all_voxels(N, dims))
    sr = _stats_ratio(y, stats)
    print(f"\n{name:<30} {'{} d{} k{}'.format(*got_form):<16} grid {str(grid):<13} {N}x{D}x{H}x{W} {cin}->{cout}{' fused' if fused else ''}"
          f" elements={ref.numel()} stats={sr:.3f} {res}")
    assert res.ratio <= 1, f"{name}: {res}"
    assert sr <= 1, f"{name}: statistics words off the sums of the stored output: {sr}"


def test_folded_upconv_at_24_cubed_batch_4_within_fp64_bound():
    """dua_upconv_k3_fwd at 4 x 24^3, skip 128 + coarse 128 (12^3, fused producer) -> 128: 27 * 4 * 2 = 216 tiles, every one of the
    27 border classes of the bias table.  The composed weights are held to the fp64 composition as in the per-launch check."""
    nv, ops = _ops()
    N, dims, cskip, cu, cmid, cout = B.FOLD_CASE
    D, H, W = dims
    assert ops.upconv_supported(B.F16, N, D, H, W, cskip, cskip, cu, cu, cout, cout)
    t = B.fold_inputs()
    skip, u = t["skip"].to(DEV), t["u"].to(DEV)
    w_skip, wu, btab = ops.pack_upconv_weights(t["wc"].to(DEV).contiguous(), t["bc"].to(DEV), t["wd"].to(DEV).contiguous(), t["bd"].to(DEV), cskip)
    norm = _producer(u, t["gamma"], t["beta"], t["add"])

    def launch():
        y = torch.full((N, D, H, W, cout), float("nan"), dtype=B.F16, device=DEV)
        stats = ops.stats_buffer(N, cout, DEV)
        ops.upconv_k3(skip, cskip, 0, u, cu, 0, norm, w_skip, wu, btab, cout, y, 0, stats)
        return y, stats
    y, stats = launch()
    y2, stats2 = launch()
    torch.cuda.synchronize()
    assert torch.equal(y, y2) and torch.equal(stats, stats2), "two launches differ"

    Wp = R.decode_fold_weights(wu, cout, cu)
    comp = R.compose_fold(t["wc"][:, cskip:], t["wd"])
    for k, (m, mabs) in comp.items():                  # the packer's composed weights: the fp64 composition rounded once to fp16
        wb = R.U16 * m.abs() + R.FLOOR16 + R.U32 * (8 * m.shape[1] + 1) * mabs
        r = R.check(Wp[k], m, wb)
        assert r.ratio <= 1, f"composed weights {k}: {r}"
    rows, arows = R.fold_bias_table(t["wc"][:, cskip:], t["bc"], t["bd"])
    cls = R.border_class(R.all_voxels(N, dims), dims)
    assert sorted(set(cls.tolist())) == list(range(27))
    act = B.activation(t["u"], _consts(norm, N, "fold"))
    skip_sums = B.conv3_sums(B.padded(skip.double()), R.conv3_weights(t["wc"][:, :cskip], B.F16))
    ref, ab, sq, ar = B.fold_sums(skip_sums, dims, act, Wp, rows, arows)
    bnd = R.bound(ref, ab, sq, R.chain_length(27 * cskip + 8 * cu, B.F16), B.F16, emulated_in=B.F16, extra=R.U32 * (27 * cmid + 1) * ar)
    res = R.check(y.reshape(-1, cout), ref.reshape(-1, cout), bnd.reshape(-1, cout), R.all_voxels(N, dims))
    sr = _stats_ratio(y, stats)
    print(f"\nfold {N}x{D}x{H}x{W} {cskip}+{cu}->{cout} fused elements={ref.numel()} stats={sr:.3f} {res}")
    assert res.ratio <= 1, str(res)
    assert sr <= 1, f"statistics words off the sums of the stored output: {sr}"
