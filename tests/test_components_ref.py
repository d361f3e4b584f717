"""Connected components without a GPU: the numpy restatement of the contract (tests/components_ref.py) reproduces the golden
file that tools/make_components_golden.py wrote from scipy.ndimage.label bit for bit (and scipy itself on fresh volumes where
scipy imports), the Python layer of diff_unet_amos_amd/postprocess.py refuses bad arguments and CPU tensors, and every
dua_cc_* entry point returns DUA_ERR_ARG for a bad argument before anything is launched (only the library is loaded)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import components_ref as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "components_golden.npz")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def _unpack(bits, shape):
    return np.unpackbits(bits)[:int(np.prod(shape))].reshape(shape)


@pytest.mark.parametrize("si", range(len(CR.RANDOM_SHAPES)))
def test_restatement_reproduces_the_golden_random_volumes(golden, si):
    for fi in range(len(CR.RANDOM_FILLS)):
        masks = CR.random_masks(si, fi)
        assert np.array_equal(_unpack(golden[f"random_s{si}_f{fi}_mask"], masks.shape), masks)
        for c in CR.CONNECTIVITIES:
            want, counts, sizes = (golden[f"random_s{si}_f{fi}_c{c}_{k}"] for k in ("labels", "counts", "sizes"))
            for v in range(CR.RANDOM_VOLUMES):
                lab, n = CR.label(masks[v], c)
                assert n == counts[v] and np.array_equal(lab, want[v].astype(np.int32)), (si, fi, c, v)
                assert np.array_equal(CR.sizes(lab, sizes.shape[1]), sizes[v])


@pytest.mark.parametrize("name", sorted(CR.SPECIAL_MASKS))
def test_restatement_reproduces_the_golden_special_volumes(golden, name):
    mask = CR.SPECIAL_MASKS[name]()
    assert tuple(golden[f"{name}_shape"]) == mask.shape
    assert np.array_equal(_unpack(golden[f"{name}_mask"], mask.shape), mask)
    for c in CR.CONNECTIVITIES:
        lab, n = CR.label(mask, c)
        assert n == golden[f"{name}_c{c}_counts"][0] and np.array_equal(lab, golden[f"{name}_c{c}_labels"].astype(np.int32))
        assert np.array_equal(CR.sizes(lab, max(n, 1)), golden[f"{name}_c{c}_sizes"])


def test_special_volumes_are_what_their_names_say(golden):
    serp = CR.serpentine()
    for c in CR.CONNECTIVITIES:
        assert golden[f"serpentine_c{c}_counts"][0] == 1 and golden[f"serpentine_c{c}_sizes"][0] == serp.sum()
    checker = CR.checkerboard()
    assert golden["checkerboard_c1_counts"][0] == checker.sum()
    assert golden["checkerboard_c2_counts"][0] == 1 and golden["checkerboard_c3_counts"][0] == 1
    iso = CR.isolated()
    assert golden["isolated_c3_counts"][0] == iso.sum()
    roots = np.flatnonzero(iso.ravel()) // 1024                    # the numbering scan works on blocks of 1024 voxels
    assert len(set(roots.tolist())) >= 3


@pytest.mark.parametrize("name", sorted(CR.FILTER_CASES))
def test_restatement_reproduces_the_golden_filter_cases(golden, name):
    make, c, k, min_size, cap = CR.FILTER_CASES[name]
    mask = make()
    got = CR.keep_largest_components(mask, c, k, min_size, cap=cap)
    assert np.array_equal(got, _unpack(golden[f"filter_{name}"], mask.shape))


def test_filter_cases_keep_what_the_contract_says():
    b = CR.blobs()
    lab, n = CR.label(b, 1)
    assert n == 6 and CR.sizes(lab, 6).tolist() == [12, 30, 12, 5, 1, 12]
    kept = lambda **kw: sorted(set(lab[CR.keep(lab, n, **kw) != 0].tolist()))      # noqa: E731
    assert kept(num_components=1) == [2]
    assert kept(num_components=2) == [1, 2]                        # 12 voxels three times: the first in raster order
    assert kept(num_components=3) == [1, 2, 3]
    assert kept(num_components=0, min_size=12) == [1, 2, 3, 6]     # exactly min_size voxels: kept
    assert kept(num_components=0, min_size=13) == [2]
    assert kept(num_components=1, cap=1) == [1]                    # overflow: only the first cap labels are considered
    t = CR.ties()
    lab, n = CR.label(t, 1)
    assert CR.sizes(lab, 3).tolist() == [3, 9, 9] and set(lab[CR.keep(lab, n, 1) != 0].tolist()) == {2}


def test_channels_pass_through_in_the_restatement():
    m = np.stack([CR.blobs() * 3, CR.blobs(), CR.blobs()])[None]                 # [1, 3, D, H, W]; channel 0 holds 0 / 3
    out = CR.keep_largest_components(m, channels=[1, 2])
    assert np.array_equal(out[0, 0], CR.blobs()) and out[0, 1].sum() == 30 and out[0, 2].sum() == 30


def test_restatement_equals_scipy_on_fresh_volumes():
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(77)
    for shape in ((3, 5, 9), (4, 4, 67), (1, 7, 30)):
        for fill in (0.25, 0.45, 0.6):
            m = (rng.random(shape) < fill).astype(np.uint8)
            for c in CR.CONNECTIVITIES:
                want, n = ndimage.label(m, ndimage.generate_binary_structure(3, c))
                lab, count = CR.label(m, c)
                assert count == n and np.array_equal(lab, want)


# ---- the Python layer ---------------------------------------------------------------------------------------------------------

def test_postprocess_refuses_bad_arguments_and_cpu_tensors():
    from diff_unet_amos_amd import postprocess as pp
    m = torch.zeros(2, 3, 4, 5, 6, dtype=torch.uint8)
    for fn, args in ((pp.label_components, (m,)), (pp.keep_largest_components, (m,)), (pp.remove_small_components, (m, 3)),
                     (pp.component_sizes, (m.int(), torch.zeros(2, 3, dtype=torch.int32)))):
        with pytest.raises(RuntimeError, match="no CPU path"):
            fn(*args)
    for bad in (0, 4, True, "1"):
        with pytest.raises(ValueError, match="connectivity"):
            pp.label_components(m, connectivity=bad)
        with pytest.raises(ValueError, match="connectivity"):
            pp.keep_largest_components(m, connectivity=bad)
    with pytest.raises(ValueError, match="D, H, W"):
        pp.label_components(torch.zeros(4, 5))
    with pytest.raises(ValueError, match="D, H, W"):
        pp.keep_largest_components(torch.zeros(0, 4, 5))
    with pytest.raises(ValueError, match="num_components"):
        pp.keep_largest_components(m, num_components=-1)
    with pytest.raises(ValueError, match="num_components"):
        pp.keep_largest_components(m, num_components=1.5)
    with pytest.raises(ValueError, match="min_size"):
        pp.remove_small_components(m, -2)
    for bad in (0, pp.nv.CC_MAX_CAP + 1, 2.0):
        with pytest.raises(ValueError, match="cap"):
            pp.keep_largest_components(m, cap=bad)
        with pytest.raises(ValueError, match="cap"):
            pp.component_sizes(m.int(), torch.zeros(2, 3, dtype=torch.int32), cap=bad)
    with pytest.raises(ValueError, match="channels"):
        pp.keep_largest_components(m, channels=[3])
    with pytest.raises(ValueError, match="channels"):
        pp.keep_largest_components(m[0, 0], channels=[0])
    with pytest.raises(ValueError, match="int32"):
        pp.component_sizes(m, torch.zeros(2, 3, dtype=torch.int32))
    with pytest.raises(ValueError, match="count"):
        pp.component_sizes(m.int(), torch.zeros(2, dtype=torch.int32))
    with pytest.raises(TypeError):
        pp.label_components(np.zeros((3, 4, 5)))
    assert 1 <= pp.DEFAULT_CAP <= pp.nv.CC_MAX_CAP


def test_inference_refuses_a_bad_postprocess_argument():
    from diff_unet_amos_amd import inference
    image = torch.zeros(1, 1, 8, 8, 8)
    with pytest.raises(ValueError, match="postprocess"):
        inference.infer(None, image, postprocess={"largest": 1})
    with pytest.raises(ValueError, match="postprocess"):
        inference.infer(None, image, postprocess=[1])
    with pytest.raises(RuntimeError, match="no CPU path"):
        inference.evaluate_volume(None, image, postprocess={"num_components": 1})


# ---- the C ABI: argument errors, no device needed -----------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    from diff_unet_amos_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "diff_unet_amos_amd", "csrc"), "-j4"], check=True)
    return _native.lib()


def test_cc_entry_points_reject_bad_arguments_without_a_device(lib):
    """Every call below carries exactly one bad argument and must return ERR_ARG before anything is launched."""
    from diff_unet_amos_amd import _native as nv
    E = nv.ERR_ARG
    one, odd, byte = C.c_void_p(256), C.c_void_p(260), C.c_void_p(257)    # 256-byte, 4-byte and 1-byte aligned addresses
    V, D, H, W, cap = 2, 3, 4, 5, 8
    vox = D * H * W
    need = lib.dua_cc_scratch_bytes(V, D, H, W, cap)
    assert need > 0 and need % 256 == 0 and need >= V * vox * 4 + V * cap
    assert lib.dua_cc_scratch_bytes(V, D, H, W, 1) <= need
    for bad in ((0, D, H, W, cap), (65536, D, H, W, cap), (V, 0, H, W, cap), (V, D, -1, W, cap), (V, D, H, 0, cap),
                (V, 2048, 1024, 1024, cap), (V, 1, 1, 2 ** 31 - 1, cap), (V, D, H, W, 0), (V, D, H, W, nv.CC_MAX_CAP + 1)):
        assert lib.dua_cc_scratch_bytes(*bad) == E, bad

    def label(V=V, D=D, H=H, W=W, mask=one, dtype=nv.U8, vs=vox, conn=1, select=None, labels=one, counts=one, ws=one, nbytes=need):
        return lib.dua_cc_label(V, D, H, W, mask, dtype, vs, conn, select, labels, counts, ws, nbytes, None)

    for kw in (dict(V=0), dict(V=65536), dict(D=0), dict(H=0), dict(W=-3), dict(D=2048, H=1024, W=1024), dict(mask=None),
               dict(labels=None), dict(counts=None), dict(ws=None), dict(dtype=nv.F16), dict(dtype=7), dict(vs=vox - 1),
               dict(conn=0), dict(conn=4), dict(nbytes=V * vox * 4), dict(ws=odd), dict(labels=byte), dict(counts=byte),
               dict(mask=byte, dtype=nv.F32)):
        assert label(**kw) == E, kw

    def sizes(V=V, D=D, H=H, W=W, labels=one, cap=cap, out=one):
        return lib.dua_cc_sizes(V, D, H, W, labels, cap, out, None)

    for kw in (dict(V=0), dict(D=0), dict(W=2 ** 31 - 1, D=1, H=1), dict(labels=None), dict(out=None), dict(cap=0),
               dict(cap=nv.CC_MAX_CAP + 1), dict(labels=byte), dict(out=byte)):
        assert sizes(**kw) == E, kw

    def filt(V=V, D=D, H=H, W=W, labels=one, counts=one, sizes=one, cap=cap, k=1, min_size=0, apply=None, mask=None, mdtype=0,
             mvs=0, out=one, ref=None, rdtype=0, label_map=0, Cn=1, tallies=None, ws=one, nbytes=need):
        return lib.dua_cc_filter(V, D, H, W, labels, counts, sizes, cap, k, min_size, apply, mask, mdtype, mvs, out, ref, rdtype,
                                 label_map, Cn, tallies, ws, nbytes, None)

    for kw in (dict(V=0), dict(H=0), dict(D=2048, H=1024, W=1024), dict(labels=None), dict(counts=None), dict(sizes=None),
               dict(out=None), dict(ws=None), dict(cap=0), dict(cap=nv.CC_MAX_CAP + 1), dict(k=-1), dict(nbytes=need - 256),
               dict(ws=odd), dict(labels=byte), dict(sizes=byte), dict(counts=byte),
               dict(apply=one),                                                   # a pass-through flag without the mask
               dict(apply=one, mask=one, mdtype=nv.U8, mvs=vox - 1), dict(mask=one, mdtype=nv.F16, mvs=vox),
               dict(mask=byte, mdtype=nv.F32, mvs=vox),
               dict(ref=one), dict(tallies=one),                                  # reference and tallies come together
               dict(ref=one, tallies=one, rdtype=nv.F16), dict(ref=one, tallies=one, rdtype=nv.F32, label_map=1),
               dict(ref=one, tallies=one, rdtype=nv.U8, Cn=0), dict(ref=one, tallies=one, rdtype=nv.U8, Cn=3),
               dict(ref=one, tallies=one, rdtype=nv.U8, Cn=nv.BLEND_MAX_CLASSES + 1, V=nv.BLEND_MAX_CLASSES + 1, nbytes=1 << 30),
               dict(ref=one, tallies=odd, rdtype=nv.U8), dict(ref=byte, tallies=one, rdtype=nv.F32)):
        assert filt(**kw) == E, kw
