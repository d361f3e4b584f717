"""Descriptors of the launch-form checks: every 3x3x3 and transposed convolution of the plans tests/test_launch_sequence_fp64.py
pins (built from the plan's geometry on the host, no device needed) and the regimes of tests/test_kernels_gpu.py.  Shared by
tests/test_conv3_form.py (CPU: the library's form query) and tools/conv_form_trace.py (GPU: what the launchers really launch)."""
import itertools

FEATURES = (64, 64, 128, 256, 512, 64)
CLASSES = 16
F32, F16 = 0, 1                           # DUA_F32, DUA_F16
IN_BLOCKED, OUT_BLOCKED = 1, 2
POLICIES = (0, 2, 3, 6, 7)
PLAN_POLICIES = (0, 6, 7)                 # what plans run with (ops.CONV_POLICY of a whole-loop A/B)
FIELDS = ("dtype", "N", "D", "H", "W", "Cin", "Cin_stride", "Cin_off", "Cout", "Cout_stride", "Cout_off", "tap_channel_plus1",
          "background", "layout", "policy")


def desc(dtype, N, dims, cin, cout, cin_stride=None, cin_off=0, cout_stride=None, cout_off=0, tap=None, background=0, layout=0,
         policy=0):
    """Field values of a dua_conv3_desc, in declaration order."""
    D, H, W = dims
    return (dtype, N, D, H, W, cin, cin_stride or cin, cin_off, cout, cout_stride or cout, cout_off, 0 if tap is None else tap + 1,
            background, layout, policy)


def plan_launches(case, expected):
    """[(name, 'conv' | 'deconv', descriptor fields, fused, output dims or None)] of one EXPECTED entry of
    tests/test_launch_sequence_fp64.py: diff_unet_amos_amd.engine.Plan.denoiser_body written as descriptors (level extents floor,
    the transposed convolution writes the upper channels of the concat buffer, the first layer takes the tap form in fp16).  A
    level whose ``fold`` entry is set (any of the four) has neither its transposed convolution nor its first convolution in the
    list: the folded launch is no dua_conv3_desc."""
    import torch
    f, N = FEATURES, expected["N"]
    dt = F16 if expected["dtype"] == torch.float16 else F32
    S = [tuple(e >> l for e in expected["dims"]) for l in range(5)]
    up = (f[1], f[2] // 2, f[3] // 2, f[4] // 2)
    dec_out = (f[5], f[1], f[2], f[3])
    cin0 = -(-(CLASSES + 1) // 8) * 8
    blk_raw, blk_cat, blk_u = expected["layout"]
    out = []
    cin = cin0
    for l in range(5):
        first = l == 0
        out.append((f"d{l}a", "conv", desc(dt, N, S[l], cin, f[l], tap=CLASSES if first and dt == F16 else None,
                                         layout=OUT_BLOCKED if first and blk_raw else 0), False, None))
        out.append((f"d{l}b", "conv", desc(dt, N, S[l], f[l], f[l], layout=IN_BLOCKED if first and blk_raw else 0), True, None))
        cin = f[l]
    src_c, fused = f[4], False
    for l in (3, 2, 1, 0):
        cat_c = f[l] + up[l]
        if not expected["fold"][l]:
            out.append((f"up{l}", "deconv", desc(dt, N, S[l + 1], src_c, up[l], cout_stride=cat_c, cout_off=f[l],
                                                layout=OUT_BLOCKED if l == 0 and blk_cat else 0), fused, S[l]))
            out.append((f"u{l}a", "conv", desc(dt, N, S[l], cat_c, dec_out[l],
                                             layout=(IN_BLOCKED if l == 0 and blk_cat else 0) | (OUT_BLOCKED if l == 0 and blk_u else 0)),
                        False, None))
        out.append((f"u{l}b", "conv", desc(dt, N, S[l], dec_out[l], dec_out[l], layout=IN_BLOCKED if l == 0 and blk_u else 0), True, None))
        src_c, fused = dec_out[l], True
    return out


# the regimes tests/test_kernels_gpu.py states in comments: (name, descriptor fields at policy 0)
REGIMES = [
    ("24^3 64->128 fp16", desc(F16, 1, (24, 24, 24), 64, 128)),
    ("24^3 64->128 fp32", desc(F32, 1, (24, 24, 24), 64, 128)),
    ("12^3 256->256 N=1", desc(F16, 1, (12, 12, 12), 256, 256)),
    ("12^3 256->256 N=4", desc(F16, 4, (12, 12, 12), 256, 256)),
    ("16x16x32 48->48", desc(F16, 1, (16, 16, 32), 48, 48)),
    ("64^3 64->64", desc(F16, 1, (64, 64, 64), 64, 64)),
    ("tap 16 + 1", desc(F16, 1, (16, 24, 8), 24, 64, tap=16)),
]


def with_fields(d, **kw):
    return tuple(kw.get(n, v) for n, v in zip(FIELDS, d))


def voxels(d):
    return d[2] * d[3] * d[4]


def conv_descriptors(expected_table):
    """Every distinct convolution descriptor (policy 0) of the pinned plans and the regimes, with the name it was first seen under."""
    seen = {}
    for case, exp in expected_table.items():
        for name, kind, d, _, _ in plan_launches(case, exp):
            if kind == "conv":
                seen.setdefault(d, f"{case}/{name}")
    for name, d in REGIMES:
        seen.setdefault(d, name)
    return [(name, d) for d, name in seen.items()]


def deconv_launches(expected_table):
    return [(f"{case}/{name}", d, fused, dims) for case, exp in expected_table.items()
            for name, kind, d, fused, dims in plan_launches(case, exp) if kind == "deconv"]


def product(descriptors):
    """(name, descriptor with the policy set, fused) over policies x fused"""
    for (name, d), policy, fused in itertools.product(descriptors, POLICIES, (0, 1)):
        yield name, with_fields(d, policy=policy), fused
