"""The label map on the grid of the scan (include/dua_hip.h, "label map on the grid of the scan"; csrc/labelmap.hip): an fp64
restatement of the contract from the inputs the kernel reads -- sum volume, divisor, crop offsets, per-axis tables --, the bound
on an interpolated probability, the acceptance rule the tests apply, an op-for-op fp32 emulation of the kernel with a ``defect=``
argument, and the cases the CPU and GPU tests share.  A plain helper module (``import labelmap_ref``); numpy only, except for
``loss_fp64ref`` (the sigmoid's error and its one measured constant) and, in ``make_case``, the package's host geometry.

The bound e on one interpolated probability (u = 2^-24; every value lies in [0, 1] up to the error already made), per channel:
  logit   : q~ = fl(sum / divisor) = q (1 + d), |d| <= u (the count product is an integer below 2^24 and converts exactly; wsum
            is read as stored).  A logit off by u |q| moves the sigmoid by at most s (1 - s) u |q| (first order; the factor
            SECOND_ORDER of loss_fp64ref covers the rest).
  sigmoid : 1 / (1 + __expf(-q~)) against the exact sigmoid of q~: loss_fp64ref.sigmoid_err -- the argument's rounding by the
            fp32 log2(e), and EPS_SIG for v_exp_f32 + the add + the division, the project's one measured constant.
  corner  : e0 = SECOND_ORDER (s (1 - s) u |q| + sigmoid_err(q, s)) per corner and channel.
  lerp    : fmaf(w, fl(b - a), a) with the inputs off by at most e: the convex combination a + w (b - a) is off by at most the
            same convex combination of the inputs' errors; the rounded difference adds w |b - a| u <= u (1 + 2 e) and the
            fmaf's rounding u (1 + e).  tests/prepare_ref.py allows 3 u (1 + 2 e) per level because its table weight is
            rounded against an fp64 one; here the reference reads the fp32 weight the kernel reads, and 3 u (1 + 2 e) is kept
            as the (larger) allowance: e -> lerp(e) + 3 u (1 + 2 e).
  tree    : three levels, so e = (the trilinear interpolation of e0) + 9 u (1 + 2^-20) -- about 5.4e-7 + 2.5e-7 s.

Acceptance rule: a voxel is exempt only if, in the fp64 reference, the gap between its two largest probabilities is at most 2 e,
or -- with min_prob set -- the gap between the largest probability and min_prob is; e is the largest bound over the voxel's
channels.  Every other voxel must carry the reference's label: two probabilities more than 2 e apart cannot swap when each moves
by at most e.  At most 1 % of a case's voxels may be exempt."""
import numpy as np

import loss_fp64ref as LR

U32 = 2.0 ** -24
F32 = np.float32
LOG2E_32 = F32(1.4426950408889634)
EXEMPT_CAP = 0.01
DEFECTS = ("lerp_axes_swapped", "wrong_neighbour", "flip_ignored", "crop_offset_dropped", "tie_to_highest", "min_prob_le")


# ---- the tables, restated -------------------------------------------------------------------------------------------------------

def tables_ref(source_shape, box, perm, flip, n_in, s_in, pixdim, shape):
    """Per SOURCE axis (lo int64 with -1 outside the box, weight fp64 unrounded, step, prepared axis), from the header's text."""
    stride = (shape[1] * shape[2], shape[2], 1)
    out = [None] * 3
    for j in range(3):
        p, (b0, b1), n = perm[j], box[perm[j]], shape[j]
        lo, wt = np.full(source_shape[p], -1, dtype=np.int64), np.zeros(source_shape[p], dtype=np.float64)
        for x in range(b0, b1):
            k = b1 - 1 - x if flip[j] else x - b0
            y = min(k * s_in[j] / pixdim[j], float(n - 1))
            lower = np.floor(y)
            lo[x], wt[x] = int(lower) * stride[j], y - lower
        out[p] = (lo, wt, stride[j] if n > 1 else 0, j)
    return out


# ---- the shared part of both restatements: which prepared voxels a source voxel reads ---------------------------------------------

def _axes(case, flip_ignored=False):
    """Per PREPARED axis j: (lower index, upper index, weight) as arrays broadcastable over the source grid, and the mask of the
    voxels inside the box."""
    X, shape = case["source_shape"], case["spatial"]
    tstride = (shape[1] * shape[2], shape[2], 1)
    per_axis, inside = [None] * 3, np.ones(X, dtype=bool)
    for p in range(3):
        lo, wt, j = np.asarray(case["lo"][p]).astype(np.int64), np.asarray(case["weight"][p]), case["axis"][p]
        if flip_ignored and case["flip"][j]:                  # the defect: a flipped axis read front to back
            b0, b1 = case["box"][p]
            lo, wt = lo.copy(), wt.copy()
            lo[b0:b1], wt[b0:b1] = lo[b0:b1][::-1].copy(), wt[b0:b1][::-1].copy()
        view = [1, 1, 1]
        view[p] = X[p]
        lower = np.maximum(lo, 0) // tstride[j]
        upper = np.minimum(lower + (1 if case["step"][p] else 0), shape[j] - 1)
        per_axis[j] = (lower.reshape(view), upper.reshape(view), wt.reshape(view))
        inside = inside & (lo >= 0).reshape(view)
    return per_axis, inside


def _corner(case, per_axis, bits, dtype, crop=True):
    """(sum [C, *source], divisor [*source]) at the corner ``bits`` = (bz, by, bx) of every source voxel's prepared cell."""
    o = case["crop_lo"] if crop else (0, 0, 0)
    z, y, x = (per_axis[j][b] + o[j] for j, b in enumerate(bits))
    z, y, x = np.broadcast_arrays(z, y, x)
    s = case["sum"][:, z, y, x].astype(dtype)
    if case["wsum"] is not None:
        return s, case["wsum"][z, y, x].astype(dtype)
    nd, nh, nw = case["counts"]
    return s, (nd[z] * nh[y] * nw[x]).astype(dtype)


def labels_of(prob, inside, min_prob=0.0, tie_to_highest=False, le=False):
    """Rules 5 and 6 and the box rule on probabilities [C, *source]: ascending channels, strict >, a NaN never wins."""
    best, label = np.full(prob.shape[1:], -1.0, dtype=prob.dtype), np.zeros(prob.shape[1:], dtype=np.uint8)
    for c in range(prob.shape[0]):
        with np.errstate(invalid="ignore"):
            take = prob[c] >= best if tie_to_highest else prob[c] > best
        best, label = np.where(take, prob[c], best), np.where(take, c, label).astype(np.uint8)
    below = best <= prob.dtype.type(min_prob) if le else best < prob.dtype.type(min_prob)
    label[below] = 0
    label[~inside] = 0
    return label


# ---- fp64 ---------------------------------------------------------------------------------------------------------------------------

def reference(case, min_prob=0.0):
    """dict(prob fp64 [C, *source], bound fp64 [C, *source], inside, label uint8 [*source]) of one case."""
    per_axis, inside = _axes(case)
    w = [per_axis[j][2].astype(np.float64) for j in range(3)]
    val, err = {}, {}
    for bits in np.ndindex(2, 2, 2):
        s, den = _corner(case, per_axis, bits, np.float64)
        q = s / den
        p = 1.0 / (1.0 + np.exp(-q))
        val[bits] = p
        err[bits] = LR.SECOND_ORDER * (p * (1 - p) * U32 * np.abs(q) + _sigmoid_err(q, p))

    def lerp(a, b, wt):
        return a + wt * (b - a)

    def tree(v, grow):
        r = {(bz, by): lerp(v[bz, by, 0], v[bz, by, 1], w[2]) for bz in (0, 1) for by in (0, 1)}
        r = {k: grow(x) for k, x in r.items()}
        s = {bz: grow(lerp(r[bz, 0], r[bz, 1], w[1])) for bz in (0, 1)}
        return grow(lerp(s[0], s[1], w[0]))

    prob = tree(val, lambda x: x)
    bound = tree(err, lambda e: e + 3 * U32 * (1 + 2 * e))
    return dict(prob=prob, bound=bound, inside=inside, label=labels_of(prob, inside, min_prob))


def _sigmoid_err(q, s):
    """loss_fp64ref.sigmoid_err on numpy arrays (that module states it for tensors)."""
    import torch
    return LR.sigmoid_err(torch.from_numpy(np.ascontiguousarray(q)), torch.from_numpy(np.ascontiguousarray(s))).numpy()


def exempt(ref, min_prob=0.0):
    """The voxels the acceptance rule exempts (module docstring)."""
    top = np.sort(ref["prob"], axis=0)
    e = ref["bound"].max(axis=0)
    out = np.zeros(top.shape[1:], dtype=bool)
    if top.shape[0] > 1:
        out |= top[-1] - top[-2] <= 2 * e
    if min_prob > 0:
        out |= np.abs(top[-1] - min_prob) <= 2 * e
    return out & ref["inside"]


def check(got, ref, min_prob=0.0, what=""):
    """The acceptance rule: prints the figures, then asserts; returns (exempt voxels, mismatches outside them)."""
    got = np.asarray(got)
    ex = exempt(ref, min_prob)
    wrong = (got != ref["label"]) & ~ex
    top = np.sort(ref["prob"], axis=0)
    gap = float((top[-1] - top[-2])[ref["inside"]].min()) if top.shape[0] > 1 and ref["inside"].any() else float("nan")
    print(f"{what}: {got.size} voxels, {int(ref['inside'].sum())} inside the box, exempt {int(ex.sum())}, wrong outside the "
          f"exemption {int(wrong.sum())} (inside it {int(((got != ref['label']) & ex).sum())}); smallest top-two gap {gap:.3e}, "
          f"largest bound e {float(ref['bound'].max()):.3e}")
    assert got.shape == ref["label"].shape and got.dtype == np.uint8, what
    assert int(ex.sum()) <= EXEMPT_CAP * got.size, f"{what}: {int(ex.sum())} of {got.size} voxels exempt"
    assert not wrong.any(), f"{what}: {int(wrong.sum())} labels differ from the fp64 reference outside the exemption"
    return int(ex.sum()), int(wrong.sum())


# ---- fp32, op for op ---------------------------------------------------------------------------------------------------------------

def _fma32(w, d, a):
    """fmaf(w, d, a) on fp32 arrays: the product of two fp32 numbers is exact in fp64, the sum rounds there and once more to fp32."""
    return (w.astype(np.float64) * d.astype(np.float64) + a.astype(np.float64)).astype(F32)


def emulate(case, min_prob=0.0, defect=None):
    """The kernel's operations in numpy fp32 (csrc/labelmap.hip): fp32 division, -q times the fp32 log2(e), an exponential, the
    add and the division of the sigmoid, seven fmaf lerps, the strict ascending scan.  ``defect``: one of DEFECTS.  Returns
    (label uint8 [*source], the winning interpolated probability fp32 [*source])."""
    assert defect is None or defect in DEFECTS, defect
    per_axis, inside = _axes(case, flip_ignored=defect == "flip_ignored")
    w = [per_axis[j][2].astype(F32) for j in range(3)]
    if defect == "lerp_axes_swapped":
        w = [w[2], w[1], w[0]]
    val = {}
    for bits in np.ndindex(2, 2, 2):
        s, den = _corner(case, per_axis, bits, F32, crop=defect != "crop_offset_dropped")
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            q = s / den
            e = np.exp2(((-q) * LOG2E_32).astype(np.float64)).astype(F32)
            val[bits] = F32(1) / (F32(1) + e)

    def lerp(a, b, wt):
        wt = np.broadcast_to(wt, a.shape[1:])
        if defect == "wrong_neighbour":
            a, b = b, a
        return _fma32(wt, b - a, a)

    r = {(bz, by): lerp(val[bz, by, 0], val[bz, by, 1], w[2]) for bz in (0, 1) for by in (0, 1)}
    s = {bz: lerp(r[bz, 0], r[bz, 1], w[1]) for bz in (0, 1)}
    prob = lerp(s[0], s[1], w[0])
    label = labels_of(prob, inside, F32(min_prob), tie_to_highest=defect == "tie_to_highest", le=defect == "min_prob_le")
    return label, np.where(inside, prob.max(axis=0), F32(0))


# ---- the cases --------------------------------------------------------------------------------------------------------------------

def signed_permutation_affine(axis_of_source, signs, spacing):
    a = np.zeros((4, 4))
    a[3, 3] = 1
    for p in range(3):
        a[axis_of_source[p], p] = signs[p] * spacing[p]
    a[:3, 3] = (5.0, -3.0, 11.0)
    return a


PIXDIM = (1.5, 1.5, 2.0)
# name: (source extent, box, world axis of each source axis, its sign, its spacing, C, pad before, pad after, prepared extent)
GEOMETRIES = {
    # prepared axis j shows source axis (2, 0, 1)[j], flipped (True, False, True); the box strictly inside on every side
    "case1": ((17, 14, 12), ((2, 15), (1, 13), (1, 11)), (1, 2, 0), (1, -1, -1), (1.02, 1.06, 1.65), 5, (2, 1, 1), (3, 2, 0),
              (11, 9, 7)),
    "case2": ((9, 11, 7), ((0, 9), (0, 11), (0, 7)), (0, 1, 2), (1, 1, 1), (0.9, 0.63, 0.9), 16, (0, 0, 0), (0, 0, 0), (6, 5, 4)),
    "case2_x8": ((9, 11, 8), ((0, 9), (0, 11), (0, 8)), (0, 1, 2), (1, 1, 1), (0.9, 0.63, 0.9), 16, (0, 0, 0), (0, 0, 0),
                 (6, 5, 4)),
    "case3": ((1, 13, 20), ((0, 1), (0, 13), (0, 20)), (0, 1, 2), (1, 1, 1), (1.0, 0.9, 0.84), 3, (0, 0, 0), (0, 0, 0), (1, 8, 9)),
}
SEEDS = {"case1": 11, "case2": 12, "case2_x8": 13, "case3": 14}


def make_case(name, weighted=False, seed=None):
    """The inputs of one case as numpy arrays: sum fp32 [C, *padded] = logits N(0, 2) times the divisor, the divisor (non-uniform
    count vectors, or a weight-sum volume), crop offsets, and the tables of the package's host geometry for it."""
    from diff_unet_amos_amd import prepare
    X, box, world, signs, spacing, C, before, after, want = GEOMETRIES[name]
    geom = prepare.prepared_geometry(X, box, signed_permutation_affine(world, signs, spacing), PIXDIM)
    assert geom.shape == want, (name, geom.shape)
    t = prepare.linear_restore_tables(geom)
    padded = tuple(b + n + a for b, n, a in zip(before, geom.shape, after))
    rng = np.random.default_rng(SEEDS[name] if seed is None else seed)
    logits = rng.normal(0.0, 2.0, size=(C, *padded)).astype(F32)
    counts = tuple(rng.integers(1, 5, size=n).astype(np.int32) for n in padded)
    wsum = rng.uniform(0.5, 3.0, size=padded).astype(F32) if weighted else None
    den = wsum if weighted else (counts[0][:, None, None] * counts[1][None, :, None] * counts[2][None, None, :]).astype(F32)
    return dict(name=name, sum=(logits * den).astype(F32), counts=None if weighted else counts, wsum=wsum, crop_lo=before,
                spatial=geom.shape, source_shape=X, box=box, flip=geom.flip, perm=geom.perm, geometry=geom, C=C, lo=t["lo"],
                weight=t["weight"], step=t["step"], axis=t["axis"])


def identity_case(spatial, C, seed, pad=(0, 0, 0)):
    """A volume that is its own grid: identity tables, every weight 0."""
    rng = np.random.default_rng(seed)
    padded = tuple(n + 2 * p for n, p in zip(spatial, pad))
    stride = (spatial[1] * spatial[2], spatial[2], 1)
    counts = tuple(rng.integers(1, 5, size=n).astype(np.int32) for n in padded)
    den = (counts[0][:, None, None] * counts[1][None, :, None] * counts[2][None, None, :]).astype(F32)
    logits = rng.normal(0.0, 2.0, size=(C, *padded)).astype(F32)
    return dict(name="identity", sum=(logits * den).astype(F32), counts=counts, wsum=None, crop_lo=pad, spatial=tuple(spatial),
                source_shape=tuple(spatial), box=tuple((0, n) for n in spatial), flip=(False,) * 3, perm=(0, 1, 2), C=C,
                lo=tuple((np.arange(n) * s).astype(np.int32) for n, s in zip(spatial, stride)),
                weight=tuple(np.zeros(n, dtype=F32) for n in spatial), step=tuple(s if n > 1 else 0 for n, s in zip(spatial, stride)),
                axis=(0, 1, 2))


def plant_tie(case, low, high):
    """Channel ``high`` becomes a bit copy of channel ``low``: an exact tie at every voxel, which the lower channel keeps."""
    case["sum"][high] = case["sum"][low]
    return case


def plant_half(case, channel, others=-6.0):
    """Every sum of ``channel`` becomes 0 -- its probability is exactly 0.5 at every corner and after every lerp, on any
    hardware -- and every other channel's logit becomes ``others``: with min_prob = 0.5 the label is ``channel``, not 0."""
    den = case["wsum"] if case["wsum"] is not None else \
        (case["counts"][0][:, None, None] * case["counts"][1][None, :, None] * case["counts"][2][None, None, :]).astype(F32)
    case["sum"][:] = (F32(others) * den).astype(F32)
    case["sum"][channel] = 0
    return case
