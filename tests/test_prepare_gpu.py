"""Case preparation on the device (csrc/volume_prep.hip, diff_unet_amos_amd/prepare.py) against the fp64 restatement of the
contract (tests/prepare_ref.py): the foreground box against numpy, the prepared label and the restored masks bit for bit, the
prepared image within the bound the restatement derives from the operation count.  The shapes are the smallest at which the
kernels can go wrong: odd extents, rows that are and are not a multiple of the 4-voxel run, an output extent of 1, several
workgroups for the box pass."""
import numpy as np
import pytest
import torch

import prepare_ref as R
from diff_unet_amos_amd import ops, prepare
from diff_unet_amos_amd.augment import DeviceBatchProducer, DeviceVolume

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SHAPE = (13, 10, 7)
SPACING = (0.78, 2.9, 5.0)
PIXDIM = (1.5, 1.5, 2.0)
DTYPES = {"int16": np.int16, "fp32": np.float32}


def _case(shape=SHAPE, seed=0, air=0.3, dtype=np.int16):
    """A scan with air (below a_min), soft tissue and bone (above a_max), and a label map of 5 classes."""
    rng = np.random.default_rng(seed)
    image = rng.integers(-400, 500, size=shape).astype(np.float64)
    if dtype == np.float32:
        image = image + rng.random(shape)                    # fp32 sources are not whole Hounsfield units
    image[rng.random(shape) < air] = -1000
    return image.astype(dtype), rng.integers(0, 5, size=shape).astype(np.uint8)


def _box_words(image, a_min=-175.0):
    idx = np.nonzero(image > a_min)
    return [int(i.min()) for i in idx] + [int(i.max()) for i in idx] + [int(idx[0].size), 0]


def _check_case(image, label, affine, pixdim=PIXDIM, axcodes="RAS", what=""):
    """prepare_case against the restatement: geometry and label exactly, image within the derived bound."""
    ref = R.prepare(image, label, affine, pixdim, axcodes)
    case = prepare.prepare_case(image, label, affine=affine, pixdim=pixdim, axcodes=axcodes, device=DEV)
    assert case.box == ref["box"] and case.source_shape == image.shape and case.orientation == (ref["perm"], ref["flip"])
    assert tuple(case.image.shape) == ref["shape"] and case.image.dtype == torch.float32 and case.image.is_contiguous()
    assert np.allclose(case.affine, ref["affine"], rtol=0, atol=1e-12)
    if label is not None:
        assert case.label.dtype == torch.uint8 and np.array_equal(case.label.cpu().numpy(), ref["label"]), f"label {what}"
    else:
        assert case.label is None
    err = float(np.abs(case.image.cpu().numpy().astype(np.float64) - ref["image"]).max())
    print(f"{what}: prepared {ref['shape']}, max |device - fp64| = {err:.3e}, bound {R.image_bound():.3e}")
    assert err <= R.image_bound(), what
    return case, ref


# ---- the foreground box ----

def _box_cases(dtype):
    air = np.full(SHAPE, -1000, dtype=dtype)
    single = air.copy()
    single[5, 3, 2] = 40
    faces = air.copy()
    for idx in ((0, 4, 3), (12, 5, 3), (6, 0, 2), (6, 9, 4), (7, 5, 0), (5, 4, 6)):
        faces[idx] = 10
    whole = np.full(SHAPE, 100, dtype=dtype)
    edge = air.copy()
    edge[3, 2, 1] = -174                                     # just above a_min; -175 itself is not foreground
    edge[9, 9, 6] = -175
    edge[4, 7, 5] = -174
    big, _ = _case((70, 65, 40), seed=5, air=0.7, dtype=dtype)
    big[:3] = big[:, :, 38:] = big[:, 60:] = -1000
    return dict(single=single, faces=faces, whole=whole, edge=edge, big=big)


@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_foreground_box_against_numpy(dtype):
    for name, image in _box_cases(DTYPES[dtype]).items():
        got = ops.prep_foreground_box(torch.from_numpy(image).to(DEV), -175.0).tolist()
        assert got == _box_words(image), (dtype, name)
    assert _box_words(_box_cases(DTYPES[dtype])["big"])[:6] != [0, 0, 0, 69, 64, 39]


@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_no_foreground_raises(dtype):
    image = np.full(SHAPE, -175, dtype=DTYPES[dtype])        # none above a_min
    words = ops.prep_foreground_box(torch.from_numpy(image).to(DEV), -175.0).tolist()
    assert words == [2 ** 31 - 1] * 3 + [-1] * 3 + [0, 0]
    with pytest.raises(ValueError, match="no voxel above a_min"):
        prepare.prepare_case(image, affine=np.eye(4), device=DEV)


# ---- the fused gather ----

@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("perm,signs", R.all_signed_permutations())
def test_resample_all_orientations(perm, signs, dtype):
    """13 x 10 x 7 with spacings (0.78, 2.9, 5.0): whichever source axis lands on a prepared axis, the run mixes refined and
    coarsened axes; the crop is not the whole volume, so base and the flipped strides matter."""
    image, label = _case(seed=7, dtype=DTYPES[dtype])
    image[0] = -1000
    image[:, :, 6] = -1000
    image[1, 4, 2] = image[12, 0, 0] = image[6, 9, 5] = 60
    affine = R.signed_permutation_affine(perm, signs, SPACING, origin=(5.0, -3.0, 11.0))
    _check_case(image, label, affine, what=f"{dtype} perm {perm} signs {signs}")


@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_resample_output_extent_one_and_other_axis_codes(dtype):
    image, label = _case(seed=8, dtype=DTYPES[dtype])
    # source axis 2 (7 voxels of 0.1 mm) collapses to one prepared voxel: 6 * 0.1 / 1.5 = 0.4 -> 0
    for perm, signs in (((0, 1, 2), (1, 1, 1)), ((2, 0, 1), (-1, 1, -1)), ((1, 2, 0), (1, -1, 1))):
        affine = R.signed_permutation_affine(perm, signs, (0.78, 2.9, 0.1))
        for code in ("RAS", "LPI", "SAR", "PIL"):
            case, ref = _check_case(image, label, affine, (1.5, 1.5, 1.5), code, what=f"{dtype} extent-1 {perm} {signs} {code}")
            assert 1 in ref["shape"]
    single = np.full((1, 1, 1), 30, dtype=DTYPES[dtype])     # one voxel in, one voxel out
    case, _ = _check_case(single, np.full((1, 1, 1), 3, dtype=np.uint8), np.diag([0.8, 0.8, 2.5, 1.0]), what=f"{dtype} one voxel")
    assert tuple(case.image.shape) == (1, 1, 1)
    _check_case(image, None, R.signed_permutation_affine((0, 1, 2), (1, 1, 1), SPACING), what=f"{dtype} no label")


@pytest.mark.parametrize("w_out,s_out", [(63, 1.016), (65, 0.984), (64, 1.0)])
def test_resample_row_lengths_around_the_run(w_out, s_out):
    """Prepared rows of 63, 65 and 64 voxels: a last run of 3, of 1, and the 16-byte store path."""
    image, label = _case((5, 6, 64), seed=9)
    image[0, 0, 0] = image[4, 5, 63] = 50
    for dtype in sorted(DTYPES):
        case, ref = _check_case(image.astype(DTYPES[dtype]), label, np.eye(4), (1.0, 0.7, s_out), what=f"{dtype} W = {w_out}")
        assert ref["shape"][2] == w_out and ref["shape"][0] == 5


def test_tie_table_on_the_device():
    """n_in = 9, s_in = 1, s_out = 2.5: coordinates 0, 2.5, 5, 7.5 read indices 0, 2, 5, 8 (half to even), on every axis."""
    for axis in range(3):
        shape = [3, 4, 5]
        shape[axis] = 9
        image = np.full(shape, 100, dtype=np.int16)
        label = np.zeros(shape, dtype=np.uint8)
        view = [None, None, None]
        view[axis] = slice(None)
        label += (np.arange(9, dtype=np.uint8) + 1)[tuple(view)]            # the label names its index along the axis
        pixdim = [1.0, 1.0, 1.0]
        pixdim[axis] = 2.5
        case, ref = _check_case(image, label, np.eye(4), pixdim, what=f"ties on axis {axis}")
        line = np.moveaxis(case.label.cpu().numpy(), axis, 0).reshape(4, -1)
        assert (line == np.array([[1], [3], [6], [9]])).all()


# ---- restore ----

def _restore_operands():
    """A 13 x 10 x 7 scan whose foreground box is not the whole volume, and its label map."""
    image, label = _case(seed=11)
    image[:2] = -1000
    image[:, 9] = -1000
    image[:, :, 0] = -1000
    image[2, 0, 1] = image[12, 8, 6] = 70
    return image, label


@pytest.mark.parametrize("perm,signs,pixdim,one_to_one", [
    ((0, 1, 2), (1, 1, 1), (0.7, 0.7, 0.7), True), ((2, 0, 1), (-1, 1, -1), (0.78, 0.78, 0.78), True),
    ((1, 2, 0), (1, -1, -1), PIXDIM, False), ((2, 1, 0), (-1, -1, 1), (3.0, 0.5, 6.0), False)])
def test_restore(perm, signs, pixdim, one_to_one):
    image, label = _restore_operands()
    affine = R.signed_permutation_affine(perm, signs, SPACING)
    case, ref = _check_case(image, label, affine, pixdim, what=f"restore {perm} {signs} {pixdim}")
    got = case.restore(case.label)
    assert got.dtype == torch.uint8 and tuple(got.shape) == image.shape
    got = got.cpu().numpy()
    assert np.array_equal(got, R.restore(ref["label"], ref))
    inside = tuple(slice(lo, hi) for lo, hi in ref["box"])
    outside = np.ones(image.shape, dtype=bool)
    outside[inside] = False
    assert outside.any() and not got[outside].any()
    if one_to_one:                                           # s_out <= s_in on every axis: the way back finds every source voxel
        assert all(so <= si for so, si in zip(pixdim, ref["s_in"]))
        assert np.array_equal(got[inside], label[inside])
    # three channels in one call, bool and uint8
    stack = torch.stack([case.label, (case.label == 2).to(torch.uint8), 255 - case.label])
    many = case.restore(stack).cpu().numpy()
    assert many.shape == (3,) + image.shape and np.array_equal(many, R.restore(stack.cpu().numpy(), ref))
    assert np.array_equal(case.restore(case.label == 2).cpu().numpy(), many[1])
    with pytest.raises(ValueError, match="mask"):
        case.restore(torch.zeros((2, 2, 2), dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError, match="mask"):
        case.restore(case.image)


# ---- DeviceVolume.from_raw ----

def test_device_volume_from_raw():
    """40 x 36 x 33 at (1, 2, 3) mm: every coordinate i s_out / s_in is exact in fp64, so the restatement and the fp32 tables
    agree on which interpolated voxels are exactly 0 and the candidate counts can be compared exactly."""
    image, label = _case((40, 36, 33), seed=13, air=0.5)
    image[:3] = -1000
    image[:, :, 30:] = -1000
    label[image <= -175] = 0
    affine = R.signed_permutation_affine((1, 0, 2), (-1, 1, 1), (1.0, 2.0, 3.0), origin=(10.0, 20.0, -30.0))
    ref = R.prepare(image, label, affine, PIXDIM)
    volume = DeviceVolume.from_raw(image, label, affine, device=DEV, num_classes=5)
    want = DeviceVolume(torch.from_numpy(ref["image"].astype(np.float32)), torch.from_numpy(ref["label"]), device=DEV, num_classes=5)
    assert volume.shape == want.shape == ref["shape"]
    err = float((volume.image.double() - torch.from_numpy(ref["image"]).to(DEV)).abs().max())
    print(f"from_raw: prepared {ref['shape']}, max |device - fp64| = {err:.3e}, bound {R.image_bound():.3e}")
    assert err <= R.image_bound()
    assert torch.equal(volume.label, want.label)
    assert (volume.fg_count, volume.bg_count) == (want.fg_count, want.bg_count) and volume.fg_count > 0 and volume.bg_count > 0
    assert torch.equal(volume.class_counts, want.class_counts)
    assert volume.prepared.box == ref["box"] and np.allclose(volume.prepared.affine, ref["affine"], rtol=0, atol=1e-12)
    producer = DeviceBatchProducer([volume], roi=(16, 16, 16), class_ids=range(5), seed=1)
    images, labels = producer.next([0, 0, 0])
    assert tuple(images.shape) == (3, 1, 16, 16, 16) and tuple(labels.shape) == (3, 5, 16, 16, 16) and producer.status == 0
    assert float(images.min()) >= -0.25 and float(labels.sum(1).min()) == 1.0
    # from_hu is untouched: the window alone, on the same scan
    hu = DeviceVolume.from_hu(torch.from_numpy(image), torch.from_numpy(label), device=DEV)
    assert hu.shape == image.shape


# ---- argument errors ----

def test_argument_errors():
    image, label = _case()
    eye = np.eye(4)
    with pytest.raises(ValueError, match="image"):
        prepare.prepare_case(image[0], label[0], affine=eye, device=DEV)                     # wrong rank
    with pytest.raises(ValueError, match="image"):
        prepare.prepare_case(image.astype(np.int32), affine=eye, device=DEV)
    with pytest.raises(ValueError, match="label"):
        prepare.prepare_case(image, label[:, :, :5], affine=eye, device=DEV)                 # mismatched label shape
    with pytest.raises(ValueError, match="label"):
        prepare.prepare_case(image, label.astype(np.int16), affine=eye, device=DEV)
    bad = eye.copy()
    bad[1, 1] = np.inf
    with pytest.raises(ValueError, match="affine"):
        prepare.prepare_case(image, label, affine=bad, device=DEV)                           # non-finite affine
    with pytest.raises(ValueError, match="affine"):
        prepare.prepare_case(image, label, device=DEV)
    with pytest.raises(ValueError, match="device"):
        prepare.prepare_case(image, label, affine=eye, device="cpu")                         # a CPU device
    with pytest.raises(ValueError, match="axcodes"):
        prepare.prepare_case(image, label, affine=eye, axcodes="RAX", device=DEV)
    with pytest.raises(ValueError, match="a_min"):
        prepare.prepare_case(image, label, affine=eye, a_min=10.0, a_max=10.0, device=DEV)
    with pytest.raises(ValueError, match="label"):
        DeviceVolume.from_raw(image, None, eye, device=DEV)
    # the entry points reject what could read outside the source before the device is touched
    import ctypes as C
    from diff_unet_amos_amd import _native as nv
    one = C.c_void_p(16)
    g = nv.PrepGeom((C.c_int * 3)(13, 10, 7), (C.c_int * 3)(7, 18, 16), (C.c_long * 3)(70, 7, 1), 1, 910)    # last corner past the end
    assert nv.lib().dua_prep_resample(nv.I16, one, None, C.byref(g), one, one, one, -175.0, 425.0, one, None, None) == nv.ERR_ARG
    g = nv.PrepGeom((C.c_int * 3)(13, 10, 7), (C.c_int * 3)(7, 18, 16), (C.c_long * 3)(-70, 7, 1), 0, 910)   # flipped without its base
    assert nv.lib().dua_prep_resample(nv.I16, one, None, C.byref(g), one, one, one, -175.0, 425.0, one, None, None) == nv.ERR_ARG
    assert nv.lib().dua_prep_foreground_box(nv.F16, one, 13, 10, 7, -175.0, one, None) == nv.ERR_ARG
    assert nv.lib().dua_prep_restore(one, 0, 1, 13, 10, 7, one, one, one, one, None) == nv.ERR_ARG
