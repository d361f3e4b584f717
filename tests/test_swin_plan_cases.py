"""tests/swin_plan_cases.py without a device: every table builds, and its counts follow from the networks' structure -- depths
(2, 2, 2, 2) make 8 Swin blocks per network, the conditioning encoder has 4 residual blocks and the denoiser 5 + 5, one tail,
transposed convolutions only where the residual branch is not folded -- and the dataflow is closed: a launch reads only what an
earlier launch of the same pass wrote, or an input of the network."""
import pytest

import swin_plan_cases as P

CASES = list(P.CASES)


def _count(rows, op):
    return sum(1 for r in rows if r["op"] == op)


@pytest.mark.parametrize("case", CASES)
def test_counts_follow_from_the_structure(case):
    c = P.CASES[case]
    enc, den = P.sequence(case, "encoder"), P.sequence(case, "denoiser")
    for rows in (enc, den):
        assert _count(rows, "window_attention") == 8 and _count(rows, "window_gather_norm") == 8
        assert _count(rows, "patch_embed") == 1 and _count(rows, "patch_merge_norm") == 4 and _count(rows, "stage_out") == 4
        assert len({r["name"] for r in rows}) == len(rows)                       # every launch has its own name
    blocks = lambda rows: [r["name"].split(".")[0] for r in rows if r["name"].endswith(".conv2")]  # noqa: E731
    assert blocks(enc) == ["e1", "e2", "e3", "e4"]
    assert blocks(den) == ["d4", "d3", "d2", "d1", "d10", "u5", "u4", "u3", "u2", "u1"]       # the side stream takes the smallest first
    assert _count(enc, "final_conv_sampler") == 0 and _count(den, "final_conv_sampler") == 1 and den[-1]["op"] == "final_conv_sampler"
    ups = {int(r["name"][2:]) - 1 for r in den if r["op"] == "deconv_k2s2"}
    assert ups == {k for k in range(5) if not c["res_up"][k]} and _count(enc, "deconv_k2s2") == 0
    assert _count(den, "upconv_k3") == sum(c["fold"]) and _count(den, "deconv_res") == sum(c["res_up"])
    assert all(f or not r for f, r in zip(c["fold"], c["res_up"]))                # the residual branch folds only where conv1 does
    # a residual block ends in residual_norm_act, except decoder1's under the fused tail
    assert _count(enc, "residual_norm_act") == 4 and _count(den, "residual_norm_act") == 10 - c["fused_tail"]
    # conv3 + norm3 only where the channel count changes: e1, d1, u1..u5
    with3 = {r["name"].split(".")[0] for r in enc + den if r["name"].endswith(".conv3")}
    assert with3 == {"e1", "d1", "u1", "u2", "u3", "u4", "u5"}


@pytest.mark.parametrize("case", CASES)
def test_dtype_decides_the_gemm_entry_points(case):
    rows = P.sequence(case, "encoder") + P.sequence(case, "denoiser")
    if P.CASES[case]["dtype"] == "fp32":
        assert _count(rows, "token_linear") == _count(rows, "token_gemm") == _count(rows, "swin_mlp") == 0
        assert _count(rows, "upconv_k3") == _count(rows, "deconv_res") == 0
        assert _count(rows, "linear_f32") == 2 * (8 * 4 + 4) + 1 + 6                 # qkv, proj, fc1, fc2 per block; reductions; conv3s
        assert sum(1 for r in rows if r["extra"].get("y") == "tmp.y") == 2 * (4 + 4)  # y handed to the next gather / the merge
    else:
        assert _count(rows, "linear_f32") == 0 and _count(rows, "swin_mlp") == 2 * 2   # stage 0 only
        assert sum(1 for r in rows if r["op"] == "token_linear" and r["form"].startswith("scatter")) == 2 * 2
        assert sum(1 for r in rows if r["op"] == "token_linear" and r["form"] == "stats") == 4 - sum(P.CASES[case]["res_up"])     # e1, d1, and u1 / u2 where their residual branch is not folded
    assert all(("/tap" in r["form"]) == (P.CASES[case]["tap"] and r["name"] == "d1.conv1") for r in rows if r["op"] == "conv3d_k3")


@pytest.mark.parametrize("case", CASES)
def test_t_columns_are_disjoint_and_reach_every_consumer(case):
    toff, width = P.t_offsets(P.CASES[case]["classes"])
    offs = sorted(toff.values())
    assert offs[0] == 0 and len(set(offs)) == 15 and all(o % 8 == 0 for o in offs) and width == offs[-1] + 8 * P.F
    den = P.sequence(case, "denoiser")
    used = [r["extra"]["t"] for r in den if "t" in r["extra"]]
    assert sorted(used) == offs                                                   # 5 of the transformer, 10 residual blocks, once each
    assert not any("t" in r["extra"] or "emb" in r["extra"] for r in P.sequence(case, "encoder"))


@pytest.mark.parametrize("network", ["encoder", "denoiser"])
@pytest.mark.parametrize("case", CASES)
def test_every_launch_reads_what_an_earlier_launch_wrote(case, network):
    rows = P.sequence(case, network)
    written = {"img_in"} if network == "encoder" else {"xin"} | {f"e_hs[{i}]" for i in range(5)} | {f"e_enc[{k}]" for k in range(4)}
    for r in rows:
        e = r["extra"]
        reads = [r["src"][0]] + [e[k] for k in ("norm", "res_norm", "y", "res", "post_add", "emb", "up") if k in e]
        reads += [e[k][0] for k in ("ra", "skip") if k in e]
        if r["op"] in ("token_linear", "token_gemm", "swin_mlp", "window_scatter_add_norm", "window_gather_norm") and "x" in e:
            reads.append(e["x"])                                                  # read-modify-write on the fp32 stream
        if r["op"] in ("swin_mlp", "token_gemm") and r["dst"][0].startswith("stream"):
            reads.append(r["dst"][0])
        for b in reads:
            assert b in written, f"{case} {network} {r['name']}: reads {b}, which nothing has written yet"
        written.add(r["dst"][0])
        written.update(e[k] for k in ("x", "stats") if k in e)
    # the side-stream blocks keep to their own scratch set, everything else to the main one
    for r in rows:
        side = r["name"].split(".")[0] in ("d1", "d2", "d3", "d4") and network == "denoiser"
        for b in [r["src"][0], r["dst"][0], r["extra"].get("res", "")]:
            if b.rstrip("b") in ("raw1", "raw2", "res3"):
                assert b.endswith("b") == side, (r["name"], b)


def test_the_skip_half_sits_behind_the_upsampled_half():
    for case in CASES:
        for r in P.sequence(case, "denoiser"):
            blk = r["name"].split(".")[0]
            if r["op"] == "residual_norm_act" and blk in ("d1", "d2", "d3", "d4"):
                k = int(blk[1:]) - 1
                assert r["dst"] == (f"cat[{k}]", P.UP_BLOCKS[k][3]) and r["extra"]["post_add"] == f"e_enc[{k}]"
            if r["op"] == "residual_norm_act" and blk in ("u1", "u2", "u3", "u4"):
                k = int(blk[1:]) - 1
                assert r["extra"]["ra"] == (f"cat[{k}]", P.UP_BLOCKS[k][3]) and r["dst"] == (f"dec[{k}]", 0)
            if r["op"] == "residual_norm_act" and blk == "u5":
                assert "ra" not in r["extra"]                                     # decoder5's skip is hidden state 3: no r_k
            if r["op"] == "upconv_k3":
                k = int(blk[1:]) - 1
                assert r["src"] == (f"cat[{k}]", P.UP_BLOCKS[k][3], P.UP_BLOCKS[k][3]) and r["extra"]["up"] == f"dec[{k + 1}]"
            if r["name"] == "den.s2.out":
                assert r["dst"] == ("cat[4]", 8 * P.F)                            # hidden state 3 is decoder5's skip half


def test_each_case_reaches_what_it_is_there_for():
    forms = lambda case, net, op: [(r["name"], r["form"]) for r in P.sequence(case, net) if r["op"] == op]  # noqa: E731
    # fp16-16c-64: the tap first convolution, the wide form for conv2 of the level-0 blocks on the main stream, both folds with
    # both residual branches folded, the fused MFMA tail on the deferred block
    conv = dict(forms("fp16-16c-64", "denoiser", "conv3d_k3") + forms("fp16-16c-64", "encoder", "conv3d_k3"))
    assert conv["d1.conv1"] == "first/tap/bg" and conv["e1.conv2"] == "wide" and conv["u1.conv2"] == "wide" and conv["d1.conv2"] == "v2/bg"
    assert [n for n, _ in forms("fp16-16c-64", "denoiser", "upconv_k3")] == ["u2.conv1", "u1.conv1"]
    assert [n for n, _ in forms("fp16-16c-64", "denoiser", "deconv_k2s2")] == ["up5", "up4", "up3"]
    assert forms("fp16-16c-64", "denoiser", "final_conv_sampler") == [("out", "mfma residual")]
    assert not any(r["name"] == "u1.tail" for r in P.sequence("fp16-16c-64", "denoiser"))
    # fp16-3c-b2: every window-clipping kind, level 0 folded and level 1 not, a materialised decoder1 with ra, the VALU tail
    geoms = [f for _, f in forms("fp16-3c-b2", "denoiser", "window_gather_norm")]
    assert geoms == ["w7.7.7 s0.0.0", "w7.7.7 s3.3.3"] * 2 + ["w7.4.4 s0.0.0", "w7.4.4 s3.0.0", "w4.2.2 s0.0.0", "w4.2.2 s0.0.0"]
    den = {r["name"]: r for r in P.sequence("fp16-3c-b2", "denoiser")}
    assert den["u1.conv1"]["op"] == "upconv_k3" and den["u2.conv1"]["op"] == "conv3d_k3" and den["up2"]["op"] == "deconv_k2s2"
    assert den["u2.conv3"]["op"] == "token_linear" and den["u3.conv3"]["op"] == "token_gemm" and den["u3.sums3"]["op"] == "instnorm_stats"
    assert den["u1.tail"]["extra"]["ra"] == ("cat[0]", P.F) and den["out"]["form"] == "valu identity" and den["out"]["src"] == ("dec[0]", 0, 64)
    assert not any("/tap" in r["form"] for r in den.values())
    # fp32-2c: the MLP output travels as y
    enc = {r["name"]: r for r in P.sequence("fp32-2c", "encoder")}
    assert enc["enc.s0.b1.gather"]["extra"]["y"] == "tmp.y" and enc["enc.s0.merge"]["extra"]["y"] == "tmp.y"
    assert "y" not in enc["enc.s0.b0.gather"]["extra"]
