"""A plain numpy restatement of the label-map evaluation contract (include/dua_hip.h "Components of a label map" and "surface
report of two label maps"), written from the contract and independent of the kernels: the per-class labelling with the joint
numbering by first voxel (on the flood fill of components_ref), the per-class filter rule, the box rule of the surface report
and its workspace arithmetic.  Also the maps of the test cases, shared by tools/make_labelmap_eval_golden.py (which labels them
with scipy.ndimage.label) and the tests.

Every function takes ``defect``: None states the contract; a name plants one deviation from it, so that the tests can show that
their cases tell the two apart (DEFECTS)."""
import numpy as np

import components_ref as CR

C = 5                       # classes of the test maps: values 1..4 are foreground, 0 background, 5 and 6 are values >= C
DEFECTS = ("fused_classes", "topk_over_all_classes", "box_without_margin", "tn_from_box", "large_value_zeroed")
CONNECTIVITIES = (1, 2, 3)


# ---- components ---------------------------------------------------------------------------------------------------------------

def label_map(m, num_classes, connectivity=1, defect=None):
    """(labels int32 like m, count, cls) of one 3-D map: cls[l - 1] is the class of label l.  Per class the components of
    (m == c), all numbered together by their first voxel in raster order."""
    m = np.asarray(m)
    found = []                                          # (first voxel, class, the class's own labels, the label there)
    if defect == "fused_classes":                       # the equal-value test removed from the merge: touching organs fuse
        lab, n = CR.label((m >= 1) & (m < num_classes), connectivity)
        flat = lab.ravel()
        for l in range(1, n + 1):
            first = int(np.flatnonzero(flat == l)[0])
            found.append((first, int(m.ravel()[first]), lab, l))
    else:
        for c in range(1, num_classes):
            lab, n = CR.label(m == c, connectivity)
            flat = lab.ravel()
            firsts = {}
            for p in np.flatnonzero(flat):
                firsts.setdefault(int(flat[p]), int(p))
            for l in range(1, n + 1):
                found.append((firsts[l], c, lab, l))
    found.sort(key=lambda t: t[0])
    out = np.zeros(m.shape, np.int32)
    for new, (_, _, lab, l) in enumerate(found, start=1):
        out[lab == l] = new
    return out, len(found), np.asarray([c for _, c, _, _ in found], np.uint8)


def restrict(labels, m, c):
    """The joint labels on (m == c), renumbered 1, 2, ... in increasing order: what scipy.ndimage.label(m == c) gives."""
    x = np.where(np.asarray(m) == c, labels, 0)
    values = np.unique(x[x > 0])
    out = np.zeros(x.shape, np.int32)
    out[x > 0] = np.searchsorted(values, x[x > 0]) + 1
    return out, len(values)


def filter_map(m, num_classes, connectivity=1, num_components=1, min_size=0, classes=None, cap=None, defect=None):
    """uint8 like m: the filtered map of one 3-D map."""
    m = np.asarray(m)
    lab, count, cls = label_map(m, num_classes, connectivity, defect)
    cap = max(count, 1) if cap is None else cap
    n = min(count, cap)
    sz = CR.sizes(lab, cap)[:n].astype(np.int64)
    order = np.argsort(-sz, kind="stable")
    kept = set()
    if defect == "topk_over_all_classes":
        chosen = order[:num_components] if num_components > 0 else order
        kept.update(int(l) + 1 for l in chosen if sz[l] >= min_size)
    else:
        for c in range(1, num_classes):
            of_c = [int(l) for l in order if cls[l] == c]
            chosen = of_c[:num_components] if num_components > 0 else of_c
            kept.update(l + 1 for l in chosen if sz[l] >= min_size)
    filtered = set(range(1, num_classes)) if classes is None else set(classes)
    out = m.copy()
    drop = np.isin(m, sorted(filtered)) & ~np.isin(lab, sorted(kept))
    out[drop] = 0
    if defect == "large_value_zeroed":
        out[m >= num_classes] = 0
    return out


def tallies(out, reference, num_classes):
    """int64 [C, 3] = (|A & B|, |A|, |B|) per class of two maps (any leading dimensions); a value >= C counts nowhere."""
    out, reference = np.asarray(out), np.asarray(reference)
    t = np.zeros((num_classes, 3), np.int64)
    for c in range(num_classes):
        a, b = out == c, reference == c
        t[c] = ((a & b).sum(), a.sum(), b.sum())
    return t


# ---- the box rule of the surface report ---------------------------------------------------------------------------------------

def box_of(test, reference, c):
    """(d0, h0, w0, d1, h1, w1), half-open, of (test == c) | (reference == c) in one pair of 3-D maps; an absent class: the row
    the device leaves, (INT_MAX x 3, 0 x 3)."""
    idx = np.nonzero((np.asarray(test) == c) | (np.asarray(reference) == c))
    if idx[0].size == 0:
        return [2 ** 31 - 1] * 3 + [0] * 3
    return [int(i.min()) for i in idx] + [int(i.max()) + 1 for i in idx]


def grown(box, shape, defect=None):
    """(origin, extents) of the box grown by one voxel per side and clamped to ``shape``; None for an absent class."""
    if box[3] == 0:
        return None
    margin = 0 if defect == "box_without_margin" else 1
    o = [max(box[i] - margin, 0) for i in range(3)]
    n = [min(box[3 + i] + margin, shape[i]) - o[i] for i in range(3)]
    return o, n


def border(mask, connectivity=1):
    """mask & ~erode(mask) with generate_binary_structure(3, connectivity) and border_value 0, on the grid of ``mask``: a voxel
    on a face of the grid is always a border voxel."""
    fg = np.asarray(mask, bool)
    D, H, W = fg.shape
    pad = np.zeros((D + 2, H + 2, W + 2), bool)
    pad[1:-1, 1:-1, 1:-1] = fg
    eroded = fg.copy()
    for dz, dy, dx in CR.offsets(connectivity):
        eroded &= pad[1 + dz:1 + dz + D, 1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
    return fg & ~eroded


def box_counts(test, reference, c, connectivity=1, defect=None):
    """What the report of class c counts when it works inside the class's box: dict of tp, fp, fn, tn, surface_test,
    surface_reference and the two border masks placed back on the full grid."""
    test, reference = np.asarray(test), np.asarray(reference)
    g = grown(box_of(test, reference, c), test.shape, defect)
    full = int(np.prod(test.shape))
    ba, bb = np.zeros(test.shape, bool), np.zeros(test.shape, bool)
    if g is None:
        return dict(tp=0, fp=0, fn=0, tn=full, surface_test=0, surface_reference=0, border_test=ba, border_reference=bb)
    (d, h, w), (nd, nh, nw) = g
    sl = (slice(d, d + nd), slice(h, h + nh), slice(w, w + nw))
    a, b = test[sl] == c, reference[sl] == c
    ba[sl], bb[sl] = border(a, connectivity), border(b, connectivity)
    tp, na, nb = int((a & b).sum()), int(a.sum()), int(b.sum())
    total = nd * nh * nw if defect == "tn_from_box" else full
    return dict(tp=tp, fp=na - tp, fn=nb - tp, tn=total - na - nb + tp, surface_test=int(ba.sum()), surface_reference=int(bb.sum()),
                border_test=ba, border_reference=bb)


def full_counts(test, reference, c, connectivity=1):
    """The same quantities on the full extent, from the one-hot masks: what ``surface_report`` on the expansion counts."""
    a, b = np.asarray(test) == c, np.asarray(reference) == c
    ba, bb = border(a, connectivity), border(b, connectivity)
    tp, na, nb = int((a & b).sum()), int(a.sum()), int(b.sum())
    return dict(tp=tp, fp=na - tp, fn=nb - tp, tn=a.size - na - nb + tp, surface_test=int(ba.sum()), surface_reference=int(bb.sum()),
                border_test=ba, border_reference=bb)


# ---- the workspace arithmetic (csrc/surface.hip: scratch_layout for one volume of the grown box) ----------------------------------

def _align(x, a=256):
    return (x + a - 1) // a * a


def _cols_lds(L, wc, gather):
    f = _align(L * wc * 8, 16)
    q = _align(L * wc, 16) if gather else 0
    return 256 * 8 + f + q + wc * 4


def _cols_wc(L, W, gather):
    wc = 64
    while wc > 1 and _cols_lds(L, wc, gather) > 48 * 1024:
        wc >>= 1
    while wc > 1 and wc // 2 >= W:
        wc >>= 1
    return wc


def table_workspace_bytes(D, H, W):
    """Workspace of the distance table for ONE volume [D][H][W]: the surface bytes, two fp64 distance volumes, the per-block
    partial sums of the gathering D pass, two maxima, a 256-bin histogram, the select state and the next-larger key."""
    vox = D * H * W
    wc = _cols_wc(D, W, True)
    P = H * ((W + wc - 1) // wc)
    off = _align(_align(vox))                           # surf
    off = _align(off + 2 * vox * 8)                     # dist
    off = _align(off + 2 * P * 8)                       # partial
    off = _align(off + 2 * 8)                           # maxbits
    off = _align(off + 256 * 4)                         # hist
    off = _align(off + 4 * 8)                           # sel
    return _align(off + 8)                              # nextmin


def workspace_bytes(shape, boxes, defect=None):
    """The largest over the rows of ``boxes`` that are not absent of the table's workspace on the grown box: the rows run one
    after the other and share one region."""
    largest = 0
    for box in boxes:
        g = grown(box, shape, defect)
        if g is not None:
            largest = max(largest, table_workspace_bytes(*g[1]))
    return largest


def expansion_workspace_bytes(shape, volumes):
    """Workspace of ``surface_report`` on ``volumes`` one-hot volumes over the full extent (scratch_layout with V volumes)."""
    D, H, W = shape
    vox = D * H * W
    wc = _cols_wc(D, W, True)
    P = H * ((W + wc - 1) // wc)
    off = _align(volumes * _align(vox))
    off = _align(off + 2 * volumes * vox * 8)
    off = _align(off + 2 * volumes * P * 8)
    off = _align(off + 2 * volumes * 8)
    off = _align(off + volumes * 256 * 4)
    off = _align(off + volumes * 4 * 8)
    return _align(off + volumes * 8)


# ---- the maps of the test cases -----------------------------------------------------------------------------------------------

RANDOM_SHAPES = ((5, 6, 67), (6, 8, 130))               # W crosses one and two wave edges


def random_maps(shape_index):
    """uint8 [2, D, H, W]: blocks of 2 x 2 x 5 voxels of one value in 0..C+1 (values >= C too), a sixth of the voxels redrawn."""
    rng = np.random.default_rng(4200 + shape_index)
    shape = RANDOM_SHAPES[shape_index]
    coarse = rng.integers(0, C + 2, size=(2, *(-(-s // b) for s, b in zip(shape, (2, 2, 5)))))
    m = np.kron(coarse, np.ones((1, 2, 2, 5), dtype=np.int64))[:, :shape[0], :shape[1], :shape[2]]
    redraw = rng.random(m.shape) < 1.0 / 6.0
    m[redraw] = rng.integers(0, C + 2, size=int(redraw.sum()))
    return m.astype(np.uint8)


def checkerboard_maps(shape=(6, 6, 66)):
    """uint8 [2, D, H, W]: two classes alternating voxel by voxel (1 / 2, and 3 / 4 in the second map).  At connectivity 1 every
    voxel is its own component; at 2 and 3 there is one component per class, never merged with the other."""
    even = CR.checkerboard(shape).astype(bool)
    return np.stack([np.where(even, 1, 2), np.where(even, 4, 3)]).astype(np.uint8)


def serpentine_maps(shape=(8, 16, 72)):
    """uint8 [2, D, H, W]: the serpentine of components_ref as class 2 embedded in class 1 (and as class 3 in background)."""
    s = CR.serpentine(shape).astype(bool)
    return np.stack([np.where(s, 2, 1), np.where(s, 3, 0)]).astype(np.uint8)


def touching_maps(shape=(6, 8, 70)):
    """uint8 [2, D, H, W]: organs of different classes that touch, several components per class of different sizes, a value >= C
    inside an organ and a tie in size.  Map 0 is the prediction of the filter cases, map 1 their reference."""
    m = np.zeros((2, *shape), np.uint8)
    a = m[0]
    a[0:3, 0:4, 2:30] = 1             # class 1, large: 336 voxels
    a[0:3, 4:8, 2:30] = 2             # class 2, touches class 1 along H: 336
    a[4, 1, 60:66] = 1                # class 1, small (6), crosses a wave edge
    a[5, 5, 10:16] = 1                # class 1, small (6): a tie with the one before
    a[4:6, 6:8, 40:50] = 2            # class 2, second (40)
    a[3, 0:2, 66:70] = 3              # class 3, only component (8), ends a row
    a[1, 1, 5:9] = C + 1              # a value >= C inside class 1
    a[5, 0, 0] = C                    # and one alone
    b = m[1]
    b[0:3, 0:4, 4:32] = 1
    b[0:3, 4:8, 2:28] = 2
    b[3, 0:2, 64:70] = 3
    b[4:6, 2:4, 20:24] = 4            # class 4 only in the reference
    b[2, 2, 2] = C + 1
    return m


MAPS = {"random0": lambda: random_maps(0), "random1": lambda: random_maps(1), "checkerboard": checkerboard_maps,
        "serpentine": serpentine_maps, "touching": touching_maps}

# (map maker name, connectivity, num_components, min_size, classes) of the filter cases stored in the golden file (cap: none)
FILTER_CASES = {
    "touching_k1": ("touching", 1, 1, 0, None),
    "touching_k2": ("touching", 1, 2, 0, None),
    "touching_k1_c3": ("touching", 3, 1, 0, None),
    "touching_min7": ("touching", 1, 0, 7, None),
    "touching_k1_only2": ("touching", 1, 1, 0, (2,)),
    "random0_k1": ("random0", 1, 1, 0, None),
    "random1_k2_min3_c2": ("random1", 2, 2, 3, None),
    "random1_k1_13": ("random1", 1, 1, 0, (1, 3)),
    "checker_c1_k2": ("checkerboard", 1, 2, 0, None),
    "checker_c2_k1": ("checkerboard", 2, 1, 0, None),
    "serpentine_k1": ("serpentine", 1, 1, 0, None),
}


# ---- the maps of the surface cases ----------------------------------------------------------------------------------------------

SURFACE_SHAPES = ((7, 9, 70), (12, 10, 66))
SURFACE_SPACING = (5.0, 0.7, 0.7)
SURFACE_CLASSES = (1, 2, 3, 4, 5)


def surface_maps(shape):
    """(test, reference) uint8 [D, H, W] with six classes' worth of situations: class 1 touches faces of the volume in both maps,
    class 2 lies inside, displaced between the maps, class 3 is absent from the test, class 4 from both, class 5 has two parts
    far apart in the test and one in the reference; scattered single voxels of class 2 around it make the surfaces ragged."""
    D, H, W = shape
    rng = np.random.default_rng(D * 1000 + W)
    t, r = np.zeros(shape, np.uint8), np.zeros(shape, np.uint8)
    t[0:3, 0:4, 0:20] = 1
    r[0:4, 0:3, 0:22] = 1
    t[2:5, 4:8, 30:44] = 2
    r[3:6, 3:7, 32:47] = 2
    r[D - 2:D, H - 3:H, W - 6:W] = 3
    t[D - 1, 0:2, 0:3] = 5
    t[1:3, 5:7, W - 5:W] = 5
    r[1:4, 5:8, W - 7:W - 1] = 5
    speck = np.zeros(shape, bool)
    speck[1:6, 2:9, 24:56] = rng.random((5, 7, 32)) < 0.03        # near the organ: the class's box stays a part of the volume
    t[speck & (t == 0)] = 2
    return t, r


def full_class_maps(shape):
    """(test, reference): class 1 fills the test's whole volume; the reference has it everywhere but one corner block."""
    t = np.ones(shape, np.uint8)
    r = np.ones(shape, np.uint8)
    r[0:2, 0:2, 0:3] = 0
    return t, r
