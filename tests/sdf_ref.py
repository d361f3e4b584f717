"""The contract of dua_sdf_maps (include/dua_hip.h) restated in numpy, for tests/test_sdf_ref.py (CPU) and tests/test_sdf_gpu.py.

  brute_d2        the integer squared distance of every voxel to the nearest voxel of the OTHER set, by exhaustive search
  contract        phi (fp32) and d2 (int32) as the header defines them -- what the device must equal bit for bit
  fp64_formula    Kervadec's edt(neg) neg - (edt(pos) - 1) pos in fp64, and bound(): 2^-23 max(1, sqrt(d2)) per voxel
  emulate         the kernel's three passes over one signed word per voxel, with the defects of DEFECTS planted on request;
                  emulate(defect=None) equals contract()
  make_labels     the label kinds of KINDS on the shapes of SHAPES, from a seeded legacy RandomState (stable across numpy versions)

numpy only: scipy is used by tools/make_sdf_golden.py alone, which stores its d2 in tests/golden/sdf_golden.npz (load_golden).
"""
import numpy as np

# (N, C, D, H, W): ragged; extent 1 twice; W past one wave; the ragged training shape; two where d2 passes 2^16
SHAPES = ((2, 3, 5, 7, 9), (1, 2, 1, 6, 11), (1, 1, 12, 1, 5), (1, 2, 9, 17, 70), (2, 4, 33, 35, 40), (1, 1, 2, 3, 512),
          (1, 1, 512, 2, 3))
# device tests only: every kind, and a small blob in one corner, so that the outward search runs the full line of 96
BIG_SHAPE = (1, 2, 96, 96, 96)
KINDS = ("random30", "absent", "full", "single", "checkerboard", "box3", "partition", "soft")
BIG_KINDS = ("corner_blob",) + KINDS
HALF_UP = np.nextafter(np.float32(0.5), np.float32(1))

NONE = 1 << 30        # SDF_NONE of csrc/sdf.hip


def make_labels(shape, kind, seed=0):
    """fp32 [N, C, D, H, W]."""
    N, C, D, H, W = shape
    rng = np.random.RandomState(1000 * seed + 17 * KINDS.index(kind) if kind in KINDS else 999 + seed)
    y = np.zeros(shape, np.float32)
    if kind == "random30":
        y[:] = rng.rand(*shape) < 0.3
    elif kind == "absent":
        pass
    elif kind == "full":
        y[:] = 1
    elif kind == "single":
        for n in range(N):
            for c in range(C):
                y[n, c, rng.randint(D), rng.randint(H), rng.randint(W)] = 1
    elif kind == "checkerboard":
        z, h, w = np.ogrid[:D, :H, :W]
        y[:] = ((z + h + w) % 2).astype(np.float32)
    elif kind == "box3":                               # a box that lies on three faces of the patch
        y[:, :, :(D + 1) // 2, :(H + 1) // 2, :(W + 1) // 2] = 1
    elif kind == "partition":                          # argmax one-hot: every voxel to the nearest of C seeds
        z, h, w = np.ogrid[:D, :H, :W]
        for n in range(N):
            seeds = np.stack([rng.randint(D, size=C), rng.randint(H, size=C), rng.randint(W, size=C)], 1)
            dist = np.stack([(z - s[0]) ** 2 + (h - s[1]) ** 2 + (w - s[2]) ** 2 for s in seeds])
            y[n] = np.arange(C)[:, None, None, None] == dist.argmin(0)[None]
    elif kind == "soft":                               # exactly 0.5 (outside: the comparison is strict) and the next float (inside)
        values = np.array([0.0, 0.25, 0.5, HALF_UP, 0.75, 1.0], np.float32)
        y[:] = values[rng.randint(len(values), size=shape)]
    elif kind == "corner_blob":
        y[:, :, :3, :2, :3] = 1
        y[:, :, 0, 0, 0] = 0
    else:
        raise ValueError(kind)
    return y


def load_golden(path):
    """tests/golden/sdf_golden.npz (tools/make_sdf_golden.py) -> {(shape index, kind): (packed mask bits, scipy's d2 int32)}.
    The file holds every case's mask bits end to end ("masks") and every case's int32 d2 -- as it is, or as its differences along
    W where "delta" says so -- end to end in ONE xz stream ("d2_xz"): a distance field is smooth, and the stream of all of them
    packs to a third of what per-array deflate gives."""
    import lzma
    g = np.load(path)
    words = np.frombuffer(lzma.decompress(g["d2_xz"].tobytes()), np.int32)
    masks, delta = g["masks"], g["delta"]
    out, at, mat = {}, 0, 0
    for i, (si, kind) in enumerate((si, kind) for si in range(len(SHAPES)) for kind in KINDS):
        n = int(np.prod(SHAPES[si]))
        d2 = words[at:at + n].reshape(SHAPES[si])
        if delta[i]:
            d2 = np.cumsum(d2, -1, dtype=np.int32)
        nb = (n + 7) // 8
        out[si, kind] = (masks[mat:mat + nb], np.ascontiguousarray(d2))
        at, mat = at + n, mat + nb
    assert at == words.size and mat == masks.size
    return out


def _pairwise_d2(queries, targets):
    """min over targets of |q - t|^2 for integer points [Q, 3], [T, 3]: int64 [Q]."""
    out = np.empty(len(queries), np.int64)
    step = max(1, 4_000_000 // max(1, len(targets)))
    t = targets.astype(np.int64)
    for a in range(0, len(queries), step):
        q = queries[a:a + step].astype(np.int64)
        out[a:a + step] = ((q[:, None, :] - t[None, :, :]) ** 2).sum(-1).min(1)
    return out


def _axis_min(f, axis, matrix=None):
    """g(l) = min over l' of f(l') + (l - l')^2 along ``axis``, exhaustively (every l' for every l); ``matrix``: the [L, L]
    table of admissible (l, l') costs, default (l - l')^2."""
    L = f.shape[axis]
    i = np.arange(L, dtype=np.int64)
    m = ((i[:, None] - i[None, :]) ** 2 if matrix is None else matrix).astype(f.dtype)
    g = np.moveaxis(f, axis, 0).reshape(L, -1)
    out = np.empty_like(g)
    step = max(1, 8_000_000 // (L * L))
    for a in range(0, g.shape[1], step):
        out[:, a:a + step] = (g[None, :, a:a + step] + m[:, :, None]).min(1)
    return np.moveaxis(out.reshape((L,) + tuple(np.delete(f.shape, axis))), 0, axis)


def _separable_d2(target):
    """squared distance of every voxel of a [D, H, W] volume to the nearest True voxel of ``target`` (>= NONE: none).  int32
    holds it: NONE + 3 * 511^2 < 2^31."""
    f = np.where(target, 0, NONE).astype(np.int32)
    for axis in (2, 1, 0):
        f = _axis_min(f, axis)
    return f


def brute_d2(pos):
    """pos: bool [D, H, W].  int32 [D, H, W]: for v in pos the squared distance to the nearest voxel outside it, for the rest
    the squared distance to the nearest voxel of pos; 0 everywhere when either set is empty.  All pairs when that is
    affordable, else exhaustively per axis (every entry of a line against every other)."""
    pos = np.asarray(pos, bool)
    npos = int(pos.sum())
    if npos == 0 or npos == pos.size:
        return np.zeros(pos.shape, np.int32)
    out = np.empty(pos.shape, np.int64)
    if npos * (pos.size - npos) <= 50_000_000:
        p, q = np.argwhere(pos), np.argwhere(~pos)
        out[pos] = _pairwise_d2(p, q)
        out[~pos] = _pairwise_d2(q, p)
    else:
        out[pos] = _separable_d2(~pos)[pos]
        out[~pos] = _separable_d2(pos)[~pos]
    return out.astype(np.int32)


def contract(labels, threshold=0.5):
    """(phi fp32, d2 int32), both [N, C, D, H, W], as include/dua_hip.h defines them."""
    labels = np.asarray(labels, np.float32)
    pos = labels > np.float32(threshold)
    d2 = np.zeros(labels.shape, np.int32)
    for n in range(labels.shape[0]):
        for c in range(labels.shape[1]):
            d2[n, c] = brute_d2(pos[n, c])
    return phi_of(d2, pos), d2


def phi_of(d2, pos):
    """The fp32 tail of the contract: sqrt(float(d2)) outside, 1 - that inside; 0 where both sets are not there."""
    r = np.sqrt(d2.astype(np.float32))
    assert r.dtype == np.float32
    empty = (pos.sum((2, 3, 4), keepdims=True) == 0) | (pos.sum((2, 3, 4), keepdims=True) == pos[0, 0].size)
    phi = np.where(pos, np.float32(1) - r, r).astype(np.float32)
    return np.where(empty, np.float32(0), phi)


def fp64_formula(d2, pos):
    """Kervadec's edt(neg) neg - (edt(pos) - 1) pos in fp64 from the integer d2 (0 for a volume without both sets)."""
    r = np.sqrt(d2.astype(np.float64))
    empty = (pos.sum((2, 3, 4), keepdims=True) == 0) | (pos.sum((2, 3, 4), keepdims=True) == pos[0, 0].size)
    return np.where(empty, 0.0, np.where(pos, 1.0 - r, r))


def bound(d2):
    """|phi_fp32 - phi_fp64| <= 2^-23 max(1, sqrt(d2)): a correctly rounded square root is within 2^-24 r of r, the rounded
    subtraction 1 - r adds at most 2^-24 max(1, r) (|1 - r| <= max(1, r)); (float)d2 is exact below 2^24."""
    return 2.0 ** -23 * np.maximum(1.0, np.sqrt(d2.astype(np.float64)))


DEFECTS = ("ge_threshold", "minus_r_inside", "sign_flipped", "sentinel_leaks", "d2_16bit", "axis_skipped", "search_short",
           "line_runs_on")


def _word_pass(w, axis, matrix=None):
    """One pass of the kernel over the signed words: out(l) = min over l' of [sign differs ? 0 : |w(l')|] + (l - l')^2, for each
    membership separately."""
    inside = w < 0
    mag = np.abs(w)
    best_in = _axis_min(np.where(inside, mag, 0), axis, matrix)        # seen from a voxel inside: outside entries are at 0
    best_out = _axis_min(np.where(inside, 0, mag), axis, matrix)
    best = np.minimum(np.where(inside, best_in, best_out), NONE)
    return np.where(inside, -best, best)


def emulate(labels, threshold=0.5, defect=None):
    """The three passes of csrc/sdf.hip on [N, C, D, H, W] labels: (phi fp32, d2 int32).  ``defect``: one of DEFECTS."""
    assert defect is None or defect in DEFECTS
    labels = np.asarray(labels, np.float32)
    N, C, D, H, W = labels.shape
    t = np.float32(threshold)
    pos = labels >= t if defect == "ge_threshold" else labels > t

    def costs(L):
        i = np.arange(L, dtype=np.int64)
        m = (i[:, None] - i[None, :]) ** 2
        if defect == "search_short":                   # l + k < L - 1: the last entry of a line is never looked at from below
            m[:L - 1, L - 1] = 4 * NONE
        return m

    # the W pass: nearest entry of the other membership in the row; a word is never 0
    w = np.where(pos, -NONE, NONE).astype(np.int64)
    vols = w.reshape(N * C, D, H, W)
    vols = _word_pass(vols, 3, costs(W))
    if defect != "axis_skipped":
        vols = _word_pass(vols, 2, costs(H))
    if defect == "line_runs_on":                       # the D lines of all volumes laid end to end
        vols = _word_pass(vols.reshape(1, N * C * D, H, W), 1, costs(N * C * D)).reshape(N * C, D, H, W)
    else:
        vols = _word_pass(vols, 1, costs(D))
    w = vols.reshape(labels.shape)
    inside = w < 0
    d2 = np.abs(w)
    none = d2 >= NONE
    if defect == "sentinel_leaks":
        none = np.zeros_like(none)
    if defect == "d2_16bit":
        d2 = d2 & 0xFFFF
    r = np.sqrt(d2.astype(np.float32))
    one = np.float32(0) if defect == "minus_r_inside" else np.float32(1)
    phi = np.where(inside, one - r, r).astype(np.float32)
    if defect == "sign_flipped":
        phi = -phi
    return np.where(none, np.float32(0), phi), np.where(none, 0, d2).astype(np.int32)
