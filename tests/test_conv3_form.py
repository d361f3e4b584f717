"""The launch form of every convolution is decided by one host function (csrc/conv3_form.hpp) that the launchers run and
dua_conv3d_k3_form / dua_deconv_k2s2_form export.  No GPU needed: the queries answer for 256 compute units without a device.
Pins which kernel, tile depth and split the launches of the plans of tests/test_launch_sequence_fp64.py and the regimes of
tests/test_kernels_gpu.py take, and holds the properties that tie the form to the other queries (kernel kind, workspace size,
registered LDS limits) and to the launcher's rejections."""
import ctypes as C

import pytest

import conv_form_cases as K
from test_launch_sequence_fp64 import EXPECTED, FORMS, KIND_NAMES, form_names

CUS = 256
HUGE = 1 << 40


@pytest.fixture(scope="module")
def nv():
    from diff_unet_amos_amd import _native
    _native.lib()
    return _native


def _form(nv, d, fused=0, ws=0, cus=CUS):
    f = nv.Conv3Form()
    rc = nv.lib().dua_conv3d_k3_form(C.byref(nv.Conv3Desc(*d)), fused, ws, cus, C.byref(f))
    return rc, f


def _dform(nv, d, fused=0, dims=(0, 0, 0)):
    f = nv.DeconvForm()
    rc = nv.lib().dua_deconv_k2s2_form(C.byref(nv.Conv3Desc(*d)), fused, *dims, C.byref(f))
    return rc, f


def _kind(nv, f):
    """dua_conv3d_k3_kernel_kind as a projection of the form"""
    return 1 if f.kernel == nv.CONV3_FIRST else 2 if f.kernel in (nv.CONV3_WIDE, nv.CONV3_WIDE_BWD) else 0


def _workspace(nv, d):
    return int(nv.lib().dua_conv3d_k3_workspace(C.byref(nv.Conv3Desc(*d))))


@pytest.mark.parametrize("case", list(EXPECTED))
def test_plan_launches_take_the_pinned_kind_and_split(nv, case):
    """Kind and split of every convolution / transposed convolution of a plan equal its EXPECTED rows, and kernel, tile depth and
    ksplit of every convolution its FORMS row, asked with the workspace the plan allocates (the largest dua_conv3d_k3_workspace of
    its layers): a policy change that moves a launch of a batched plan fails here, without a GPU."""
    launches = K.plan_launches(case, EXPECTED[case])
    ws = max([16] + [_workspace(nv, d) for _, kind, d, _, _ in launches if kind == "conv"])
    want = {name: (kind, split) for name, kind, split in EXPECTED[case]["seq"]}
    names = form_names(nv)
    assert sorted(FORMS[case]) == sorted(name for name, kind, _, _, _ in launches if kind == "conv")
    checked = 0
    for name, kind, d, fused, dims in launches:
        if kind == "conv":
            rc, f = _form(nv, d, fused, ws)
            assert rc == 0, name
            assert (KIND_NAMES[_kind(nv, f)], f.ksplit > 1) == want[name], (case, name)
            assert (names[f.kernel], f.tile_depth, f.ksplit) == FORMS[case][name], (case, name)
            if f.kernel != nv.CONV3_FIRST:                          # (the first-layer kernel walks all samples from one grid)
                assert f.grid_z == d[1] * f.ksplit, (case, name)      # one slice of the grid per sample and split
            assert f.finish == (1 if f.ksplit > 1 else 0)
        else:
            rc, f = _dform(nv, d, fused, dims)
            assert rc == 0, name
            assert (f"deconv{min(f.kernel, 2)}", False) == want[name], (case, name)
            assert int(nv.lib().dua_deconv_k2s2_kernel_kind(C.byref(nv.Conv3Desc(*d)))) == min(f.kernel, 2)
        checked += 1
    assert checked == sum(1 for _, kind, _ in EXPECTED[case]["seq"] if kind in ("v2", "first", "wide") or kind.startswith("deconv"))


def test_plan_launches_drop_the_two_launches_of_a_folded_level_at_any_level():
    """A fold takes the transposed convolution and the convolution behind it out of the descriptor list at the level it is set
    for -- level 2 as well as 0 and 1 (no shipped plan folds level 2 today: its coarse tensor is 256 channels wide, the folded
    kernel takes 128) -- and leaves every other descriptor as it was."""
    base = dict(EXPECTED["fp16-96-b4"], fold=[False] * 4)
    plain = K.plan_launches("", base)
    for level in range(4):
        fold = [l == level for l in range(4)]
        got = K.plan_launches("", dict(base, fold=fold))
        assert got == [row for row in plain if row[0] not in (f"up{level}", f"u{level}a")]
        assert [row[0] for row in got].count(f"u{level}b") == 1 and len(got) == len(plain) - 2


def test_tile_depth_and_kd_plane_regimes(nv):
    """The regimes tests/test_kernels_gpu.py names in comments, as the library states them."""
    R = dict(K.REGIMES)

    def kernel(name, policy, fused=0, ws=0):
        rc, f = _form(nv, K.with_fields(R[name], policy=policy), fused, ws)
        assert rc == 0, (name, policy)
        return f

    for name in ("24^3 64->128 fp16", "24^3 64->128 fp32"):          # 108 workgroups of 4x8x8: 2-deep tiles
        for policy, want in ((0, nv.CONV3_V2_2_KD), (2, nv.CONV3_V2_2_KD), (6, nv.CONV3_V2_2), (3, nv.CONV3_V2_2)):
            f = kernel(name, policy)
            assert (f.kernel, f.tile_depth, f.ksplit) == (want, 2, 1), (name, policy)
            assert (f.grid_x, f.grid_y, f.grid_z) == (12 * 3 * 3, 2, 1)
    # 12^3 256 -> 256: 32 workgroups at N = 1 split K when given a workspace; without one, 2-deep tiles need > 64 workgroups
    need = _workspace(nv, R["12^3 256->256 N=1"])
    f = kernel("12^3 256->256 N=1", 0, ws=need)
    assert (f.kernel, f.tile_depth, f.finish) == (nv.CONV3_V2_4_KD, 4, 1) and f.ksplit > 1
    assert kernel("12^3 256->256 N=1", 6, ws=need).kernel == nv.CONV3_V2_4 and kernel("12^3 256->256 N=1", 6, ws=need).ksplit > 1
    assert kernel("12^3 256->256 N=1", 0).kernel == nv.CONV3_V2_4
    # N = 4: 128 workgroups of 4x8x8 -> 2-deep tiles, 384 workgroups: past the 256 the kd-plane form is kept to
    f = kernel("12^3 256->256 N=4", 0, ws=HUGE)
    assert (f.kernel, f.tile_depth, f.ksplit) == (nv.CONV3_V2_2, 2, 1)
    assert f.grid_x * f.grid_y * f.grid_z == 384
    assert kernel("16x16x32 48->48", 0).kernel == nv.CONV3_V2_4_HALF
    for policy, want in ((0, nv.CONV3_WIDE), (7, nv.CONV3_V2_4)):
        f = kernel("64^3 64->64", policy)
        assert f.kernel == want and f.tile_depth == (4 if policy == 7 else 8), policy
    assert kernel("tap 16 + 1", 0).kernel == nv.CONV3_FIRST
    for policy in K.POLICIES[1:]:
        assert kernel("tap 16 + 1", policy).kernel == nv.CONV3_TAP1, policy


def test_form_properties_over_the_product(nv):
    """descriptors x policies x fused x workspace {none, exactly what the form asks for, far more}"""
    L = nv.lib()
    n = 0
    for name, d, fused in K.product(K.conv_descriptors(EXPECTED)):
        policy = d[-1]
        desc = nv.Conv3Desc(*d)
        rc0, f0 = _form(nv, d, fused, 0)
        kind = int(L.dua_conv3d_k3_kernel_kind(C.byref(desc), fused, 0))
        if rc0:                                   # e.g. the tap form with a fused producer, blocked buffers off the wide form
            assert rc0 == nv.ERR_ARG and kind == nv.ERR_ARG, (name, policy, fused)
            continue
        assert f0.ksplit == 1
        if policy in K.PLAN_POLICIES:
            assert f0.workspace_needed <= _workspace(nv, K.with_fields(d, policy=0)), (name, policy)
        for ws in (0, f0.workspace_needed, HUGE):
            rc, f = _form(nv, d, fused, ws)
            assert rc == 0
            assert kind == _kind(nv, f) == int(L.dua_conv3d_k3_kernel_kind(C.byref(desc), fused, 1)), (name, policy, fused, ws)
            assert f.workspace_needed == f0.workspace_needed
            assert (f.ksplit > 1) == (f.workspace_needed > 0 and ws >= f.workspace_needed), (name, policy, fused, ws)
            assert f.finish == (1 if f.ksplit > 1 else 0)
            assert 0 < f.lds_bytes <= f.lds_limit, (name, policy, fused, ws, f.kernel, f.lds_bytes)
            assert f.ksplit * f.units_per_split >= 3 * -(-d[5] // (32 if d[0] == K.F16 else 16)) > (f.ksplit - 1) * f.units_per_split
            n += 1
        nf = _form(nv, K.with_fields(d, policy=policy | nv.POLICY_NO_FINISH), fused, HUGE)[1]
        assert nf.finish == 0 and nf.ksplit == _form(nv, d, fused, HUGE)[1].ksplit
        bg = _form(nv, K.with_fields(d, background=1), fused, 0)
        if bg[0] == 0:
            assert bg[1].lds_bytes <= bg[1].lds_limit and _kind(nv, bg[1]) != 2, (name, policy)
    assert n > 500


def test_unknown_policies_are_rejected_by_the_query_and_the_launcher(nv):
    L = nv.lib()
    one = C.c_void_p(16)
    base = K.desc(K.F16, 1, (8, 8, 8), 16, 64)
    for policy in (5, 8, 9, 10, 1, 4, 255, 512, 1 << 16, 2 | 1024):         # 8, 9: the retired persistent wide forms
        d = K.with_fields(base, policy=policy)
        assert _form(nv, d)[0] == nv.ERR_ARG, policy
        desc = nv.Conv3Desc(*d)
        assert L.dua_conv3d_k3_kernel_kind(C.byref(desc), 0, 0) == nv.ERR_ARG
        assert L.dua_conv3d_k3_fwd(C.byref(desc), one, one, one, None, one, one, None, 0, None) == nv.ERR_ARG, policy
    for policy in (2, 3, 7, 5):                                       # the transposed convolution knows 0 and 6
        d = K.with_fields(base, policy=policy)
        assert _dform(nv, d)[0] == nv.ERR_ARG
        assert L.dua_deconv_k2s2_fwd(C.byref(nv.Conv3Desc(*d)), one, one, one, None, one, None) == nv.ERR_ARG
    assert _form(nv, K.with_fields(base, policy=nv.POLICY_NO_FINISH))[0] == 0
    assert _dform(nv, K.with_fields(base, policy=6))[0] == 0


def test_rejections(nv):
    L = nv.lib()
    one = C.c_void_p(16)
    wide = K.desc(K.F16, 1, (64, 64, 64), 64, 64)
    small = K.desc(K.F16, 1, (16, 16, 16), 64, 64)

    def conv_rejected(d, fused=0):
        return (_form(nv, d, fused)[0] == nv.ERR_ARG and
                L.dua_conv3d_k3_fwd(C.byref(nv.Conv3Desc(*d)), one, one, one, None, one, one, None, 0, None) == nv.ERR_ARG)

    assert _form(nv, K.with_fields(wide, layout=K.IN_BLOCKED | K.OUT_BLOCKED))[0] == 0
    assert conv_rejected(K.with_fields(small, layout=K.IN_BLOCKED))                          # blocked input, not the wide form
    assert conv_rejected(K.with_fields(wide, layout=K.IN_BLOCKED, policy=7))
    assert conv_rejected(K.with_fields(small, layout=K.OUT_BLOCKED))                         # blocked output, v2 form
    assert conv_rejected(K.with_fields(dict(K.REGIMES)["tap 16 + 1"], layout=K.OUT_BLOCKED, policy=6))   # ... and the tap form
    assert _form(nv, K.with_fields(dict(K.REGIMES)["tap 16 + 1"], layout=K.OUT_BLOCKED))[0] == 0         # the first-layer kernel writes blocks
    assert conv_rejected(K.with_fields(wide, layout=K.IN_BLOCKED, Cin_stride=72))            # misaligned blocked stride / offset
    assert conv_rejected(K.with_fields(wide, layout=K.OUT_BLOCKED, Cout_stride=128, Cout_off=8))
    assert _form(nv, K.desc(K.F16, 1, (8, 8, 8), 1032, 64))[0] == nv.ERR_ARG               # more than 1024 packed input channels
    assert _form(nv, dict(K.REGIMES)["tap 16 + 1"], fused=1)[0] == nv.ERR_ARG                # tap form: no fused producer
    assert _form(nv, K.desc(K.F32, 1, (16, 24, 8), 24, 64, tap=16))[0] == nv.ERR_ARG        # ... fp16 only
    assert _form(nv, K.desc(K.F16, 1, (16, 24, 8), 32, 64, tap=16))[0] == nv.ERR_ARG        # ... Cin = tap channel + 8
    assert _form(nv, dict(K.REGIMES)["tap 16 + 1"], cus=0)[0] in (0, nv.ERR_ARG)             # cus = 0 asks the device: none here is an error, not a crash
    # backward sums ride on the shipped wide form only
    sup = L.dua_conv3d_k3_dgrad_reduce_supported
    assert sup(C.byref(nv.Conv3Desc(*wide))) == 1
    for d in (small, K.with_fields(wide, policy=7), K.with_fields(wide, dtype=K.F32),
              K.with_fields(wide, layout=K.IN_BLOCKED), K.with_fields(wide, background=1)):
        assert sup(C.byref(nv.Conv3Desc(*d))) == 0, d
    # the transposed convolution: never reads blocks, writes them from the all-taps kernel only
    big = K.desc(K.F16, 1, (32, 32, 32), 64, 64, cout_stride=128, cout_off=64)
    assert _dform(nv, K.with_fields(big, layout=K.OUT_BLOCKED))[0] == 0
    for d in (K.with_fields(big, layout=K.IN_BLOCKED), K.with_fields(big, layout=K.OUT_BLOCKED, Cout_off=8),
              K.with_fields(K.desc(K.F16, 1, (8, 8, 8), 64, 64), layout=K.OUT_BLOCKED)):
        assert _dform(nv, d)[0] == nv.ERR_ARG
        assert L.dua_deconv_k2s2_fwd(C.byref(nv.Conv3Desc(*d)), one, one, one, None, one, None) == nv.ERR_ARG
        assert L.dua_deconv_k2s2_pad_fwd(C.byref(nv.Conv3Desc(*d)), 2 * d[2] + 1, 2 * d[3], 2 * d[4], one, one, one, None, one, None) == nv.ERR_ARG


def test_deconv_forms(nv):
    """all-taps tiles of 128 voxels under both policies, Cin chunks over the waves from 256 channels (not under policy 6), one
    tap per workgroup otherwise; grids and LDS within the registered limits"""
    cases = [(K.desc(K.F16, 1, (48, 48, 48), 64, 64), 0, nv.DECONV_ALLTAPS_128, (864, 1, 1)),
             (K.desc(K.F16, 1, (48, 48, 48), 64, 64), 6, nv.DECONV_ALLTAPS_128, (864, 1, 1)),
             (K.desc(K.F16, 2, (12, 12, 12), 256, 128), 0, nv.DECONV_KSPLIT, (27, 16, 2)),
             (K.desc(K.F16, 2, (12, 12, 12), 256, 128), 6, nv.DECONV_ONE_TAP, (7, 16, 2)),
             (K.desc(K.F32, 1, (8, 8, 8), 512, 256), 0, nv.DECONV_ONE_TAP, (2, 32, 1)),
             (K.desc(K.F16, 1, (24, 24, 24), 128, 64), 0, nv.DECONV_ONE_TAP, (54, 8, 1))]
    for d, policy, kernel, grid in cases:
        for fused in (0, 1):
            rc, f = _dform(nv, K.with_fields(d, policy=policy), fused)
            assert rc == 0 and f.kernel == kernel, (d, policy)
            assert (f.grid_x, f.grid_y, f.grid_z) == grid
            assert 0 < f.lds_bytes <= f.lds_limit
