"""Buffer contract of the loss, the surface metrics, connected components and hole filling (see
tests/test_buffer_contract_conv_gpu.py for the four checks and tests/buffer_contract.py for the three runs).

Every entry point here promises the same bits on every run, so check 2 covers every result:

  seg_loss terms reduce / finish      include/dua_hip.h:384-385 (partials added in workgroup order, no floating-point atomics)
  seg_loss terms gradient             one thread per element of the same constants (test_loss_terms_gpu holds two calls equal)
  seg_loss_boundary_reduce            include/dua_hip.h:419-421 (same inputs, same bits)
  signed_distance_maps                include/dua_hip.h:1770 (exact, the same bits on every run)
  multi_neighbor_partials             include/dua_hip.h:344 (deterministic, integer atomics only)
  surface tables                      include/dua_hip.h:908, 962 (fixed-order sums, integer atomics: two calls agree bit for bit)
  components                          include/dua_hip.h:998 (integer-only: every output is exact)
  fill holes                          include/dua_hip.h:1077 (every operation is an integer one)

UNSPECIFIED is the table of regions check 2 leaves out.  It is empty: cc_sizes zeroes its rows beyond the component count
itself (include/dua_hip.h:1022, "the call zeroes it first"), the absent classes of surface_map_report get the rows of a pair of
empty masks, and a volume without foreground still has every output written.
"""
import numpy as np
import pytest
import torch

import boundary_fp64ref as BR
import buffer_contract as BC
import components_ref as CR
import fill_holes_ref as FR
import labelmap_eval_ref as LR
import loss_terms_fp64ref as LT
import sdf_ref
import surface_dice_ref as SDR
import test_boundary_loss_gpu as TBL
import test_labelmap_surface_gpu as TLS
import test_loss_terms_gpu as TLT
import test_multi_neighbor as TMN
import test_surface_dice_gpu as TSD
import test_surface_metrics as TSM

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F16, F32 = torch.float16, torch.float32
UNSPECIFIED = {}


def _ops():
    from diff_unet_amos_amd import ops
    return ops


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a
    return t.to(DEV) if dtype is None else t.to(DEV, dtype)


# ---- loss ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,other", [(TLT.SHAPES[1], TLT.SHAPES[0]), (TLT.SHAPES[2], TLT.MORE_GROUPS[1])], ids=["f16", "f32"])
def test_seg_loss_terms_reduce_and_grad(shape, other):
    """All six terms at the smallest shape of test_loss_terms_gpu (2 x 5 channels in rows of 8, 6 x 5 x 7) with a class absent
    from one sample: the reduce scratch, the sums and constants, the (L, dcomb) pair and the gradient come from the allocator."""
    logits, labels = TLT._inputs(shape, "class_absent", "randn")
    r = LT.reduce_ref(logits, labels)
    lo, la = TLT._inputs(other, "soft", "saturated")

    def run():
        L, buf, dcomb, g, grad = TLT._seg_loss(logits, labels, TLT.ALL6, "log", TLT.SCALE)
        return dict(L=L, buf=buf, dcomb=dcomb, grad=grad, g=torch.tensor(g, dtype=torch.float64))

    outs, _ = BC.run_modes(run, lambda: TLT._seg_loss(lo, la, TLT.ALL6, "sum", TLT.SCALE))
    o = outs["b"]
    TLT._check_results(logits, labels, (o["L"], o["buf"], o["dcomb"], float(o["g"]), o["grad"]), TLT.ALL6, "log", "0xFF-filled", r=r)
    BC.same_bits(outs, unspecified=UNSPECIFIED)


@pytest.mark.parametrize("dtype", [F16, F32], ids=["f16", "f32"])
def test_signed_distance_maps_and_boundary_reduce(dtype):
    """signed_distance_maps without a caller scratch, then seg_loss_boundary_reduce and the one-pass gradient on its maps, at the
    small shape of boundary_fp64ref (2 x 3 x 5 x 7 x 9, rows padded by 5 channels)."""
    ops = _ops()
    names, combine = ("mse", "bce", "dice"), "mean"
    config = (BR.SHAPES[0], dtype, 5)
    c = TBL._case(*config)                                         # operands, the maps of an unguarded call, the fp64 reduce
    logits, labels = c["logits"], c["labels"]
    want_phi = torch.from_numpy(sdf_ref.contract(labels.cpu().numpy())[0])
    alpha = torch.tensor(BR.ALPHA, dtype=F32, device=DEV)
    scale = torch.tensor(TBL.SCALE, dtype=F32, device=DEV)
    big = TBL._case(BR.SHAPES[1], dtype, 0)

    def case(logits, labels):
        def run():
            phi = ops.signed_distance_maps(labels)
            L, buf, dcomb, B = ops.seg_loss_boundary_reduce(logits, labels, names, combine, phi, alpha)
            grad = ops.seg_loss_boundary_grad(logits, labels, buf, scale * dcomb, names, phi, scale * alpha)
            return dict(phi=phi, L=L, buf=buf, dcomb=dcomb, B=B, grad=grad)
        return run

    outs, _ = BC.run_modes(case(logits, labels), case(big["logits"], big["labels"]))
    o = outs["b"]
    assert torch.equal(o["phi"].cpu().view(torch.int32), want_phi.view(torch.int32))
    TBL._check_results(config, dict(c, phi=o["phi"]), names, combine, alpha, o["B"], o["L"], o["buf"], o["dcomb"], o["grad"], None)
    BC.same_bits(outs, unspecified=UNSPECIFIED)


def test_multi_neighbor_partials():
    ops = _ops()

    def case(i):
        N, C, K, D, H, W, dtype, Cs = TMN.SHAPES[i]
        logits, labels = TMN._random_case(100 + i, N, C, D, H, W, multi_hot=i % 3 == 2)
        x, y = TMN._channels_last(logits, dtype, Cs), labels.to(DEV).contiguous()
        return (lambda: dict(partials=ops.multi_neighbor_partials(x, y, K))), logits, labels, K

    run, logits, labels, K = case(0)
    outs, _ = BC.run_modes(run, case(2)[0])
    want = float(TMN.multi_neighbor_restated(logits, labels, K))
    part = outs["b"]["partials"].cpu()
    got = float(part[:, :K].sum() / part[:, K].sum())
    assert abs(got - want) <= 1e-5 * abs(want), (got, want)
    BC.same_bits(outs, unspecified=UNSPECIFIED)


# ---- surface metrics --------------------------------------------------------------------------------------------------------------
SPACING, CONN = (2.0, 1.5, 1.5), 2
ROWS = [[1.5, 4.0], [0.0, 2.5], [3.0, 2.0], [1.0, 6.0]]


def _surface_volumes(shape, seed):
    """V = 4 volume pairs [1, 4, D, H, W]: two of random blobs, one whose test mask is empty, one whose reference is full."""
    g = torch.Generator().manual_seed(seed)
    a = SDR.random_blobs((1, 4, *shape), g, 0.05)
    b = SDR.random_blobs((1, 4, *shape), g, 0.0)
    a[0, 2] = False
    b[0, 3] = True
    return a, b


def _surface_run(a, b):
    ops = _ops()
    ad, bd = a.to(DEV), b.float().to(DEV)

    def run():
        out = {}
        out["table_counts"], out["table"] = ops.surface_distance_table(ad, bd, SPACING, CONN)
        for bounded in (True, False):
            out[f"dice_counts_{bounded}"], out[f"within_{bounded}"], out[f"nsd_{bounded}"] = \
                ops.surface_dice_table(ad, bd, ROWS, SPACING, CONN, True, bounded=bounded)
        out["report_counts"], out["report_table"], out["report_within"], out["report_nsd"] = \
            ops.surface_report(ad, bd, ROWS, SPACING, CONN)
        return out
    return run


@pytest.mark.parametrize("shape,other", [((1, 5, 7), (17, 64, 9)), ((17, 64, 9), (1, 5, 7))], ids=["1x5x7", "17x64x9"])
def test_surface_tables(shape, other):
    from diff_unet_amos_amd import _native as nv
    from diff_unet_amos_amd import metrics
    a, b = _surface_volumes(shape, sum(shape))
    outs, _ = BC.run_modes(_surface_run(a, b), _surface_run(*_surface_volumes(other, 3)))
    o = outs["b"]
    col = {name: i for i, name in enumerate(nv.SURFACE_FIELDS)}
    for v in range(4):
        r = TSM._surface_ref(a[0, v], b[0, v], SPACING, CONN)
        for table in (o["table"], o["report_table"]):
            for key, field in (("hd", "hd"), ("asd", "asd"), ("lo", "hd95_lo"), ("hi", "hd95_hi"), ("hd95", "hd95"), ("assd", "assd")):
                assert TSM._close(float(table[v, col[field]]), r[key], 1e-9), (v, key, float(table[v, col[field]]), r[key])
    for counts, within, nsd in ((o["dice_counts_True"], o["within_True"], o["nsd_True"]),
                                (o["dice_counts_False"], o["within_False"], o["nsd_False"]),
                                (o["report_counts"], o["report_within"], o["report_nsd"])):
        TSD._check_against_ref(metrics._dice_dict(counts, within, nsd, 1, 4), a.to(DEV), b.to(DEV), ROWS, SPACING, CONN)
    assert bool(torch.isnan(o["table"][2, col["hd"]])) and bool(torch.isnan(o["table"][3, col["hd"]]))      # the two early exits
    BC.same_bits(outs, unspecified=UNSPECIFIED)


def _surface_map_run(shape):
    ops = _ops()
    test, reference = TLS._pair(shape)
    classes = list(LR.SURFACE_CLASSES)
    tol = [list(TLS.TOLERANCES)] * len(classes)
    boxes = [[int(x) for x in row] for row in ops.surface_map_boxes(test, reference, max(classes) + 1)[:, classes].reshape(-1, 6).tolist()]

    def run():
        counts, table, within, nsd = ops.surface_map_report(test, reference, classes, boxes, tol, LR.SURFACE_SPACING, 1)
        return dict(boxes=ops.surface_map_boxes(test, reference, max(classes) + 1), counts=counts, table=table, within=within, nsd=nsd)
    return run, test, reference, classes, tol


def test_surface_map_report():
    """The smallest of labelmap_eval_ref.SURFACE_SHAPES: a class absent from the test map and one absent from both (the rows that
    skip the border pass and the transform)."""
    from diff_unet_amos_amd import _native as nv
    from diff_unet_amos_amd import metrics
    run, test, reference, classes, tol = _surface_map_run(LR.SURFACE_SHAPES[0])
    outs, _ = BC.run_modes(run, _surface_map_run(LR.SURFACE_SHAPES[1])[0])
    o = outs["b"]
    N, K = test.shape[0], len(classes)
    col = {name: i for i, name in enumerate(nv.SURFACE_FIELDS)}
    got = {k: o["table"][:, col[k]].reshape(N, K) for k in metrics.TABLE_KEYS}
    got.update(metrics._dice_dict(o["counts"], o["within"], o["nsd"], N, K))
    want = metrics.surface_report(TLS._expand(test, classes), TLS._expand(reference, classes), tol, LR.SURFACE_SPACING, 1)
    TLS._compare(got, want, "0xFF-filled")
    BC.same_bits(outs, unspecified=UNSPECIFIED)


# ---- components and hole filling ------------------------------------------------------------------------------------------------
SMALLEST = min(range(len(CR.RANDOM_SHAPES)), key=lambda i: int(np.prod(CR.RANDOM_SHAPES[i])))
C_MAP = 4                      # classes of the label maps below: values 1..3 are foreground, 4 is a value >= C


def _masks(kind):
    """uint8 [V, D, H, W]: the random volumes of the smallest shape (fill 0.35, and 0.7 so that holes exist) or the isolated
    pattern, each followed by an all-zero volume."""
    if kind == "random":
        m = np.concatenate([CR.random_masks(SMALLEST, 1), CR.random_masks(SMALLEST, 3)[:1]])
    else:
        m = CR.isolated()[None]
    return np.concatenate([m, np.zeros_like(m[:1])])


def _maps(masks):
    """A label map per mask: the foreground takes the values 1 .. C_MAP in slabs along W (so components of different classes
    touch), and a reference map shifted by one voxel."""
    w = np.arange(masks.shape[-1])
    maps = (masks * (1 + (w // 9) % C_MAP)).astype(np.uint8)
    return maps, np.roll(maps, 1, axis=-1)


FILL_CONN = 1                  # the connectivity of the hole filling: 6 neighbours, so that three planes of noise enclose holes


def _cc_run(masks, conn, k, min_size):
    ops = _ops()
    m = _dev(masks)
    maps, ref_maps = (_dev(x) for x in _maps(masks))
    onehot = _dev((np.roll(masks, 1, axis=-2) != 0).astype(np.uint8))
    V = masks.shape[0]
    cap = max(int(CR.label(v, conn)[1]) for v in masks) + 3

    def run():
        o = {}
        o["labels"], o["counts"] = ops.cc_label(m, conn)
        o["sizes"] = ops.cc_sizes(o["labels"], cap)
        o["kept"], o["kept_tallies"] = ops.cc_filter(o["labels"], o["counts"], o["sizes"], k, min_size, reference=onehot, classes=1)
        o["map_labels"], o["map_counts"] = ops.cc_label_map(maps, C_MAP, conn)
        o["map_sizes"] = ops.cc_sizes(o["map_labels"], cap)
        o["map_kept"], o["map_tallies"] = ops.cc_filter_map(maps, C_MAP, o["map_labels"], o["map_counts"], o["map_sizes"], k, min_size,
                                                            reference=ref_maps)
        o["filled"], o["filled_count"], o["filled_tallies"] = ops.fill_holes_mask(m, FILL_CONN, reference=onehot, classes=1)
        o["filled_map"], o["filled_map_count"], o["filled_map_tallies"] = ops.fill_holes_map(maps, C_MAP, FILL_CONN, reference=ref_maps)
        return o
    return run, cap, V


def _eq(got, want, what):
    want = torch.from_numpy(np.ascontiguousarray(want)).to(got.dtype)
    assert got.shape == want.shape and torch.equal(got.cpu(), want), (what, got.cpu().tolist() if got.numel() < 64 else None)


@pytest.mark.parametrize("kind,other,conn", [("random", "isolated", 2), ("isolated", "random", 1)], ids=["random", "isolated"])
def test_components_and_hole_filling(kind, other, conn):
    k, min_size = 2, 2
    masks = _masks(kind)
    maps, ref_maps = _maps(masks)
    onehot = (np.roll(masks, 1, axis=-2) != 0).astype(np.uint8)
    run, cap, V = _cc_run(masks, conn, k, min_size)
    outs, _ = BC.run_modes(run, _cc_run(_masks(other), 3, 1, 0)[0])
    o = outs["b"]
    lab = [CR.label(v, conn) for v in masks]
    _eq(o["labels"], np.stack([l for l, _ in lab]), "labels")
    _eq(o["counts"], np.array([n for _, n in lab]), "counts")
    _eq(o["sizes"], np.stack([CR.sizes(l, cap) for l, _ in lab]), "sizes")
    kept = np.stack([CR.keep(l, n, k, min_size, cap) for l, n in lab])
    _eq(o["kept"], kept, "cc_filter")
    _eq(o["kept_tallies"], FR.tallies_mask(kept[:, None], onehot[:, None]), "cc_filter tallies")
    mlab = [LR.label_map(v, C_MAP, conn) for v in maps]
    _eq(o["map_labels"], np.stack([l for l, _, _ in mlab]), "map labels")
    _eq(o["map_counts"], np.array([n for _, n, _ in mlab]), "map counts")
    _eq(o["map_sizes"], np.stack([CR.sizes(l, cap) for l, _, _ in mlab]), "map sizes")
    mkept = np.stack([LR.filter_map(v, C_MAP, conn, k, min_size, cap=cap) for v in maps])
    _eq(o["map_kept"], mkept, "cc_filter_map")
    _eq(o["map_tallies"], LR.tallies(mkept, ref_maps, C_MAP), "cc_filter_map tallies")
    filled = [FR.fill_mask(v, FILL_CONN) for v in masks]
    fmask = np.stack([f for f, _ in filled]).astype(np.uint8)
    _eq(o["filled"], fmask, "fill_holes_mask")
    _eq(o["filled_count"], np.array([n for _, n in filled]), "filled voxels")
    _eq(o["filled_tallies"], FR.tallies_mask(fmask[:, None], onehot[:, None]), "fill_holes_mask tallies")
    fmaps = [FR.fill_map(v, C_MAP, FILL_CONN) for v in maps]
    fmap = np.stack([f for f, _ in fmaps])
    _eq(o["filled_map"], fmap, "fill_holes_map")
    _eq(o["filled_map_count"], np.sum([n for _, n in fmaps], axis=0), "filled voxels per class")
    _eq(o["filled_map_tallies"], FR.tallies_map(fmap, ref_maps, C_MAP), "fill_holes_map tallies")
    if kind == "random":
        assert int(o["filled_count"].sum()) > 0 and int(o["counts"][-1]) == 0          # holes exist; the empty volume's early exit
    BC.same_bits(outs, unspecified=UNSPECIFIED)
