"""Surface-distance metrics (diff_unet_amos_amd.metrics, csrc/surface.hip) against an fp64 restatement of medpy's hd / hd95 /
asd / assd behind the reference's wrappers (light_training/evaluation/metric.py:314-390).

_surface_ref restates the semantics independently of the kernels: the erosion by padded shifts, the distances by a brute-force
minimum over all surface pairs from explicit squared differences in fp64 (no matmul form), np.percentile for hd95.  The
fixture tests/golden/surface_metrics_golden.npz holds the same metrics computed with scipy (tools/make_surface_golden.py)."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "surface_metrics_golden.npz")
KEYS = ("hd", "hd95", "asd", "assd")


# ---- the fp64 restatement -------------------------------------------------------------------------------------------------

def _footprint(k):
    return [(dz, dy, dx) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)
            if 0 < (dz != 0) + (dy != 0) + (dx != 0) <= k]


def _erode(x, k):
    """One binary erosion of a bool [D, H, W] tensor with generate_binary_structure(3, k), border_value 0."""
    D, H, W = x.shape
    p = torch.zeros((D + 2, H + 2, W + 2), dtype=torch.bool, device=x.device)
    p[1:-1, 1:-1, 1:-1] = x
    out = x.clone()
    for dz, dy, dx in _footprint(k):
        out &= p[1 + dz:1 + dz + D, 1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
    return out


def _border(x, k):
    return x & ~_erode(x, k)


def _sds(ba, bb, spacing, chunk=2048):
    """For every voxel of ba, the fp64 distance to the nearest voxel of bb (explicit squared differences, chunked)."""
    s = torch.tensor(spacing, dtype=torch.float64, device=ba.device)
    pa = ba.nonzero().double() * s
    pb = bb.nonzero().double() * s
    out = torch.empty(pa.shape[0], dtype=torch.float64, device=ba.device)
    for i in range(0, pa.shape[0], chunk):
        q = pa[i:i + chunk]
        d2 = (q[:, None, 0] - pb[None, :, 0]) ** 2 + (q[:, None, 1] - pb[None, :, 1]) ** 2 + (q[:, None, 2] - pb[None, :, 2]) ** 2
        out[i:i + chunk] = d2.min(dim=1).values
    return out.sqrt()


def _exists(a, b):
    return bool(a.any()) and not bool(a.all()) and bool(b.any()) and not bool(b.all())


def _surface_ref(a, b, spacing=(1.0, 1.0, 1.0), k=1, nan_for_nonexisting=True):
    """medpy hd / hd95 / asd / assd of one 3-D pair behind the reference wrapper, plus the two hd95 order statistics."""
    a, b = a.bool(), b.bool()
    if not _exists(a, b):
        r = float("nan") if nan_for_nonexisting else 0.0
        return dict(hd=r, hd95=r, asd=r, assd=r, lo=r, hi=r)
    ba, bb = _border(a, k), _border(b, k)
    sab, sba = _sds(ba, bb, spacing), _sds(bb, ba, spacing)
    both = torch.cat((sab, sba))
    srt = both.sort().values.cpu().numpy()
    n = srt.shape[0]
    kl = int(math.floor((n - 1) * 0.95))
    return dict(hd=float(max(sab.max(), sba.max())), hd95=float(np.percentile(both.cpu().numpy(), 95)),
                asd=float(sab.mean()), assd=float((sab.mean() + sba.mean()) / 2), lo=float(srt[kl]),
                hi=float(srt[min(kl + 1, n - 1)]))


def _golden_cases():
    z = np.load(GOLDEN)
    out = []
    for i, name in enumerate(z["names"]):
        shape = tuple(int(v) for v in z["shapes"][i])
        n = int(np.prod(shape))
        o0, o1 = int(z["offsets"][i]), int(z["offsets"][i + 1])
        a = np.unpackbits(z["test"][o0:o1])[:n].reshape(shape).astype(bool)
        b = np.unpackbits(z["reference"][o0:o1])[:n].reshape(shape).astype(bool)
        out.append((str(name), torch.from_numpy(a), torch.from_numpy(b)))
    return out, z["spacings"], z["connectivities"], z["expected"]


def _close(got, want, rel):
    if math.isnan(want):
        return math.isnan(got)
    return abs(got - want) <= rel * max(1.0, abs(want))


# ---- CPU ------------------------------------------------------------------------------------------------------------------

def test_restatement_matches_the_golden():
    cases, spacings, conns, expected = _golden_cases()
    assert len(cases) == 8
    for i, (name, a, b) in enumerate(cases):
        for j, sp in enumerate(spacings):
            for m, k in enumerate(conns):
                r = _surface_ref(a, b, tuple(sp), int(k))
                for q, key in enumerate(KEYS):
                    assert _close(r[key], float(expected[i, j, m, q]), 1e-12), (name, tuple(sp), int(k), key, r[key],
                                                                               expected[i, j, m, q])


def test_restatement_matches_scipy():
    ndimage = pytest.importorskip("scipy.ndimage")
    g = torch.Generator().manual_seed(5)
    for shape, sp, k in [((11, 13, 9), (1.0, 1.0, 1.0), 1), ((14, 9, 12), (2.0, 1.5, 1.5), 2), ((8, 10, 7), (0.7, 1.3, 2.1), 3)]:
        a = torch.rand(shape, generator=g) > 0.6
        b = torch.rand(shape, generator=g) > 0.7
        fp = ndimage.generate_binary_structure(3, k)
        for x in (a, b):
            want = x.numpy() & ~ndimage.binary_erosion(x.numpy(), structure=fp, iterations=1, border_value=0)
            assert np.array_equal(_border(x, k).numpy(), want)
        ba, bb = _border(a, k), _border(b, k)
        want = ndimage.distance_transform_edt(~bb.numpy(), sampling=sp)[ba.numpy()]
        got = _sds(ba, bb, sp).numpy()
        assert np.allclose(got, want, rtol=1e-12, atol=1e-12)


def test_wrapper_rule_in_the_restatement():
    z = torch.zeros((6, 7, 5), dtype=torch.bool)
    blob = z.clone(); blob[2:4, 2:5, 1:3] = True
    full = torch.ones_like(z)
    for a, b in [(z, blob), (blob, z), (full, blob), (blob, full), (z, z)]:
        assert all(math.isnan(v) for v in _surface_ref(a, b).values())
        assert all(v == 0 for v in _surface_ref(a, b, nan_for_nonexisting=False).values())
    assert _surface_ref(blob, blob)["hd"] == 0.0


def test_cpu_tensors_have_no_path():
    from diff_unet_amos_amd import metrics
    a = torch.zeros((1, 1, 4, 4, 4))
    with pytest.raises(RuntimeError, match="no CPU path"):
        metrics.surface_distance_table(a, a)
    for fn in (metrics.hausdorff_distance, metrics.hausdorff_distance_95, metrics.avg_surface_distance,
               metrics.avg_surface_distance_symmetric):
        with pytest.raises(RuntimeError, match="no CPU path"):
            fn(a[0, 0], a[0, 0], voxel_spacing=1.5, connectivity=1)


@pytest.fixture(scope="module")
def lib():
    from diff_unet_amos_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "diff_unet_amos_amd", "csrc"), "-j4"], check=True)
    return _native.lib()


def test_surface_entry_points_reject_bad_arguments_without_a_device(lib):
    from diff_unet_amos_amd import _native as nv
    one = C.c_void_p(256)
    E = nv.ERR_ARG
    F, U = nv.F32, nv.U8
    vox = 6 * 7 * 8

    def masks(V=2, D=6, H=7, W=8, a=one, ta=F, b=one, tb=U, k=1, surf=one, counts=one):
        return lib.dua_surface_masks(V, D, H, W, a, ta, vox, b, tb, vox, k, surf, vox, counts, None)

    def edt(D=6, sd=1.0, sh=1.0, sw=1.0, seeds=one, out=one):
        return lib.dua_surface_edt_sq(2, D, 7, 8, seeds, vox, 1, sd, sh, sw, out, None)

    need = lib.dua_surface_scratch_bytes(2, 6, 7, 8)
    assert need > 2 * 2 * vox * 8

    def table(D=6, k=1, sd=1.0, sh=1.0, sw=1.0, a=one, b=one, counts=one, out=one, ws=one, wsb=need, ta=F):
        return lib.dua_surface_distance_table(2, D, 7, 8, a, ta, vox, b, U, vox, k, sd, sh, sw, 1, counts, out, ws, wsb, None)

    for k in (0, 4, -1):                                                   # connectivity outside 1..3
        assert masks(k=k) == E and table(k=k) == E
    for bad in (0.0, -1.0, float("nan"), float("inf")):                    # spacing <= 0 or non-finite
        assert edt(sd=bad) == E and edt(sh=bad) == E and edt(sw=bad) == E
        assert table(sd=bad) == E and table(sh=bad) == E and table(sw=bad) == E
    for ext in [dict(V=0), dict(D=0), dict(H=0), dict(W=0), dict(D=-3)]:   # an extent < 1
        assert masks(**ext) == E
    assert edt(D=0) == E and table(D=0) == E
    assert lib.dua_surface_scratch_bytes(2, 0, 7, 8) == E and lib.dua_surface_scratch_bytes(0, 6, 7, 8) == E
    for kw in [dict(a=None), dict(b=None), dict(surf=None), dict(counts=None)]:   # null pointers
        assert masks(**kw) == E
    assert edt(seeds=None) == E and edt(out=None) == E
    for kw in [dict(a=None), dict(b=None), dict(counts=None), dict(out=None), dict(ws=None)]:
        assert table(**kw) == E
    assert masks(ta=1) == E and table(ta=7) == E                           # masks are fp32 or uint8
    assert table(wsb=need - 1) == E                                        # workspace smaller than the query


# ---- GPU ------------------------------------------------------------------------------------------------------------------

def _random_blobs(shape, gen, thresh, sigma=1.5):
    """Smooth random fields, normalised per volume and thresholded: blobs with ragged surfaces, on the CPU, deterministic."""
    x = torch.randn(shape, generator=gen, dtype=torch.float64)
    r = int(2 * sigma) + 1
    t = torch.arange(-r, r + 1, dtype=torch.float64)
    k = torch.exp(-t * t / (2 * sigma * sigma)); k /= k.sum()
    lead = x.shape[:-3]
    y = x.reshape(-1, 1, *x.shape[-3:])
    for ax in range(3):
        shp = [1, 1, 1, 1, 1]; shp[2 + ax] = k.numel()
        pad = [0, 0, 0, 0, 0, 0]; pad[2 * (2 - ax)] = pad[2 * (2 - ax) + 1] = r
        y = torch.nn.functional.conv3d(torch.nn.functional.pad(y, pad, mode="replicate"), k.reshape(shp))
    y = y / y.flatten(1).std(dim=1).reshape(-1, 1, 1, 1, 1)                  # thresholds in standard deviations
    return y.reshape(*lead, *x.shape[-3:]) > thresh


def _ellipsoid(shape, centre, radii, device="cpu"):
    g = torch.meshgrid(*[torch.arange(n, dtype=torch.float64, device=device) for n in shape], indexing="ij")
    return sum(((x - c) / r) ** 2 for x, c, r in zip(g, centre, radii)) <= 1.0


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(35, 33, 40), (17, 64, 9), (1, 5, 7)])
def test_surface_pass_is_bit_exact(shape):
    from diff_unet_amos_amd import ops
    g = torch.Generator().manual_seed(sum(shape))
    a = _random_blobs((2, 3, *shape), g, 0.0, sigma=1.2)
    b = _random_blobs((2, 3, *shape), g, 0.1, sigma=1.2)
    b[1, 2] = True                                                           # one full reference volume
    a[0, 1] = False                                                          # one empty test volume
    for k in (1, 2, 3):
        for ta, tb in [(a.float(), b.to(torch.uint8)), (a, b.float())]:
            surf, counts = ops.surface_masks(ta.cuda(), tb.cuda(), connectivity=k)
            surf, counts = surf.cpu(), counts.cpu()
            for v in range(6):
                x, y = a.reshape(6, *shape)[v], b.reshape(6, *shape)[v]
                bx, by = _border(x, k), _border(y, k)
                want = bx.to(torch.uint8) | (by.to(torch.uint8) << 1)
                assert torch.equal(surf[v], want), (shape, k, v)
                assert counts[v].tolist() == [int(x.sum()), int(y.sum()), int((x & y).sum()), int(bx.sum()), int(by.sum())]


def _edt_brute(seeds, spacing):
    """fp64 squared distance of every voxel to the nearest seed, brute force on the GPU (explicit squared differences)."""
    D, H, W = seeds.shape
    s = torch.tensor(spacing, dtype=torch.float64, device=seeds.device)
    ps = seeds.nonzero().double() * s
    if ps.shape[0] == 0:
        return torch.full((D, H, W), float("inf"), dtype=torch.float64, device=seeds.device)
    allp = torch.ones((D, H, W), dtype=torch.bool, device=seeds.device).nonzero().double() * s
    out = torch.empty(allp.shape[0], dtype=torch.float64, device=seeds.device)
    for i in range(0, allp.shape[0], 4096):
        q = allp[i:i + 4096]
        d2 = (q[:, None, 0] - ps[None, :, 0]) ** 2 + (q[:, None, 1] - ps[None, :, 1]) ** 2 + (q[:, None, 2] - ps[None, :, 2]) ** 2
        out[i:i + 4096] = d2.min(dim=1).values
    return out.reshape(D, H, W)


def _check_edt(got, want, rel):
    inf = torch.isinf(want)
    assert torch.equal(torch.isinf(got), inf)
    d = (got[~inf] - want[~inf]).abs()
    assert bool((d <= rel * want[~inf].clamp(min=1.0)).all()), float(d.max())


@pytest.mark.gpu
@pytest.mark.parametrize("spacing,rel", [((1.0, 1.0, 1.0), 1e-12), ((2.0, 1.5, 1.5), 1e-9)])
def test_edt_matches_brute_force(spacing, rel):
    from diff_unet_amos_amd import ops
    shape = (21, 30, 26)
    vols = []
    one = torch.zeros(shape, dtype=torch.uint8); one[0, 0, 0] = 1                        # a single seed in a corner
    vols.append(one)
    face = torch.zeros(shape, dtype=torch.uint8); face[:, :, -1] = 1                     # seeds only on one face
    vols.append(face)
    vols.append(torch.zeros(shape, dtype=torch.uint8))                                  # no seeds: +inf
    for v in (vols[0], vols[1], vols[2]):
        got = ops.surface_edt_sq(v[None].cuda(), spacing)[0]
        _check_edt(got, _edt_brute(v.cuda().bool(), spacing), rel)
    g = torch.Generator().manual_seed(11)
    batch = torch.stack([(torch.rand(shape, generator=g) < p).to(torch.uint8) for p in (0.001, 0.01, 0.05, 0.0003, 0.2, 0.0)])
    batch[3, 20, 29, 25] = 1
    got = ops.surface_edt_sq(batch.cuda(), spacing)
    for v in range(6):
        _check_edt(got[v], _edt_brute(batch[v].cuda().bool(), spacing), rel)


@pytest.mark.gpu
def test_metric_table_matches_golden_and_restatement():
    from diff_unet_amos_amd import metrics
    cases, spacings, conns, expected = _golden_cases()
    for i, (name, a, b) in enumerate(cases):
        for j, sp in enumerate(spacings):
            for m, k in enumerate(conns):
                sp3, k = tuple(float(x) for x in sp), int(k)
                t = metrics.surface_distance_table(a[None, None].float().cuda(), b[None, None].cuda(), voxel_spacing=sp3,
                                                   connectivity=k)
                r = _surface_ref(a, b, sp3, k)
                for q, key in enumerate(KEYS):
                    got = float(t[key][0, 0])
                    assert _close(got, float(expected[i, j, m, q]), 1e-9), (name, sp3, k, key, got, expected[i, j, m, q])
                    assert _close(got, r[key], 1e-9), (name, sp3, k, key)
                assert float(t["tp"][0, 0]) == int((a & b).sum()) and float(t["fp"][0, 0]) == int((a & ~b).sum())
                assert float(t["fn"][0, 0]) == int((~a & b).sum()) and float(t["tn"][0, 0]) == int((~a & ~b).sum())
                # the reference's per-mask functions agree with the table
                for fn, key in ((metrics.hausdorff_distance, "hd"), (metrics.hausdorff_distance_95, "hd95"),
                                (metrics.avg_surface_distance, "asd"), (metrics.avg_surface_distance_symmetric, "assd")):
                    v = fn(a.cuda(), b.to(torch.uint8).cuda(), voxel_spacing=sp3, connectivity=k)
                    assert isinstance(v, float)
                    assert (math.isnan(v) and math.isnan(float(t[key][0, 0]))) or v == float(t[key][0, 0]), (name, key)
    # the wrapper rule with nan_for_nonexisting=False
    name, a, b = cases[5]
    t = metrics.surface_distance_table(a[None, None].cuda(), b[None, None].cuda(), nan_for_nonexisting=False)
    assert all(float(t[key][0, 0]) == 0.0 for key in KEYS)


@pytest.mark.gpu
def test_metric_table_batched_and_reproducible():
    from diff_unet_amos_amd import metrics
    g = torch.Generator().manual_seed(4)
    a = _random_blobs((2, 3, 30, 27, 22), g, 0.05)
    b = _random_blobs((2, 3, 30, 27, 22), g, 0.0)
    b[0, 2] = False
    sp = (2.0, 1.5, 1.5)
    t1 = metrics.surface_distance_table(a.cuda(), b.float().cuda(), voxel_spacing=sp, connectivity=2)
    t2 = metrics.surface_distance_table(a.cuda(), b.float().cuda(), voxel_spacing=sp, connectivity=2)
    for key in t1:
        assert torch.equal(t1[key].isnan(), t2[key].isnan())
        assert torch.equal(t1[key].nan_to_num(), t2[key].nan_to_num()), key           # bit-identical
    for n in range(2):
        for c in range(3):
            r = _surface_ref(a[n, c], b[n, c], sp, 2)
            for key in KEYS:
                assert _close(float(t1[key][n, c]), r[key], 1e-9), (n, c, key)


def _check_at_size(test, reference, spacing, k):
    from diff_unet_amos_amd import _native as nv, ops
    _, table = ops.surface_distance_table(test, reference, spacing, k)
    table = table.cpu()
    col = {name: i for i, name in enumerate(nv.SURFACE_FIELDS)}
    for v in range(test.shape[1]):
        r = _surface_ref(test[0, v], reference[0, v], spacing, k)
        for key, field in (("hd", "hd"), ("asd", "asd"), ("lo", "hd95_lo"), ("hi", "hd95_hi"), ("hd95", "hd95"), ("assd", "assd")):
            assert _close(float(table[v, col[field]]), r[key], 1e-9), (v, key, float(table[v, col[field]]), r[key])


@pytest.mark.gpu
def test_at_size_random_blobs():
    g = torch.Generator().manual_seed(21)
    a = _random_blobs((1, 16, 96, 96, 96), g, 1.0, sigma=3.0).cuda()
    b = _random_blobs((1, 16, 96, 96, 96), g, 1.0, sigma=3.0).cuda()
    _check_at_size(a, b, (1.0, 1.0, 1.0), 1)


@pytest.mark.gpu
def test_at_size_ellipsoids():
    s = (256, 256, 192)
    a = torch.stack([_ellipsoid(s, (128, 120, 96), (90, 70, 60), "cuda"), _ellipsoid(s, (60, 60, 50), (30, 20, 25), "cuda")])
    b = torch.stack([_ellipsoid(s, (124, 126, 92), (86, 74, 63), "cuda"), _ellipsoid(s, (66, 58, 47), (26, 24, 22), "cuda")])
    _check_at_size(a[None], b[None].float(), (2.0, 1.5, 1.5), 3)


@pytest.mark.gpu
def test_end_to_end_after_infer():
    from diff_unet_amos_amd import inference, metrics
    from diff_unet_amos_amd.diff_unet import DiffUNet
    torch.manual_seed(3)
    net = DiffUNet(in_channels=1, out_channels=2, features=(8, 8, 16, 32, 64, 8), sample_steps=4,
                   compute_dtype=torch.float32).cuda().eval()
    g = torch.Generator().manual_seed(9)
    image = torch.rand(1, 1, 40, 40, 40, generator=g).cuda()
    labels = _random_blobs((1, 2, 40, 40, 40), g, 0.2, sigma=2.0).float().cuda()
    pred = inference.infer(lambda x, **kw: net(image=x, **kw), image, roi_size=(32, 32, 32), sw_batch_size=1, overlap=0.25)
    t = metrics.surface_distance_table(pred, labels, voxel_spacing=(1.5, 1.0, 1.0))
    for c in range(2):
        r = _surface_ref(pred[0, c], labels[0, c], (1.5, 1.0, 1.0), 1)
        for key in KEYS:
            assert _close(float(t[key][0, c]), r[key], 1e-9), (c, key)
