"""CPU restatement of the intensity-augmentation contract of include/dua_hip.h ("training input: intensity augmentation"),
written from that text and sharing no code with the package.  The Philox generator comes from tests/augment_ref.py; this module
adds

  * the draw of the rows in numpy integers and float32 (``config``, ``draw_rows``; ``make_rows`` builds rows by hand);
  * the transform of one patch in fp64 together with a bound on |device - fp64| for every voxel (``transform``; ``reference``
    does a batch);
  * an fp32 emulation of the same operations in the same order, with planted defects (``emulate``, ``DEFECTS``).

The bound is derived, not measured, stage by stage.  u = 2^-24 is the unit roundoff of fp32; an fp32 operation that is rounded
correctly contributes u |result|.  e is the bound the input of a stage carries per voxel; the stage's own bound is first order
in u and e, and SLACK = 1.001 covers the second-order terms (products of two relative errors of at most 1e-4 each) and the
restatement's own fp64 roundings.

  functions   logf, sincosf, powf: HIP documents 1 ulp for each; ULP_FN = 2 ulp is allowed, and an ulp is at most 2 u relative.
              sqrtf and the division are the correctly rounded ones (allowed: 1 ulp = 2 u).
  noise       L = ln u1; r = sqrt(-2 L) carries r u (ULP_FN + 2) (half of logf's relative error, plus the root's rounding).  The
              angle fl(fl(2 pi) u2) is within 2 u theta of theta = 2 pi u2, so cos and sin carry 2 u theta + 2 u ULP_FN |cos|, and
              z = fl(r cos) carries  ez = u ((3 ULP_FN + 3) |z| + 2 r theta).  x' = fl(x + fl(std z)):
              e = std ez + u |std z| + u |x'|.
  blur        one pass is a dot product of 2 R + 1 terms with taps that carry u each: against the exact pass on the exact input
              it is off by at most  blur(e) + (2 R + 3) u blur(|x| + e)  (the error of a sum of k products is at most k u sum |terms|
              to first order), three times over.  R and the fp64 taps are the same numbers on both sides.
  brightness  e' = f e + u |x f|.
  statistics  of values v known to e: the mean moves by at most mean(e), the minimum and the maximum by at most max(e), the
              population deviation by at most rms(e) (it is a norm of v - mean(v), scaled by 1 / sqrt(n)); rounding to fp32 adds
              u |statistic| (nothing for minimum and maximum, which are stored values).  The fp64 accumulation of n terms is off by at
              most n 2^-53 sum |terms|: negligible for the mean, and for the deviation, where sum of squares / n - mean^2
              cancels, dvar = 4 n 2^-53 mean(v^2) moves it by at most min(sqrt(dvar), dvar / (2 s)).
  contrast    c = x - m, t = c f, v = t + m, each rounded, with m known to dm:  ev = f (e + dm + u |c|) + u |t| + dm + u |v|; the
              clamp is 1-Lipschitz in v, lo and hi:  e' = max(ev, dlo, dhi).
  gamma       a = x - lo, g = hi - lo, t = a / (g + 1e-7), p = t^gamma, y = p g + lo, then w = y - m', q = w / (s' + 1e-8), r = q s,
              x = r + m: the product and quotient rules with the statistics' bounds from above.  For the power, t lies in [0, 1):
              gamma >= 1: |dp| <= gamma (t + dt)^(gamma - 1) dt;  gamma < 1: t^gamma is concave with
              |a^gamma - b^gamma| <= |a - b|^gamma, so |dp| <= min(dt^gamma, gamma (t - dt)^(gamma - 1) dt) and no voxel near t = 0
              has to be left out; plus powf's 2 u ULP_FN p.  Inversion negates exactly.

The gamma-below-1 share: a row has gamma < 1 iff it has the gamma event and took the lower branch, ``0.5 * gamma_prob`` of rows
for a range that straddles 1 (``gamma_below_share``)."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from augment_ref import philox4x32_10  # noqa: E402

F32, F64 = np.float32, np.float64
U = 2.0 ** -24
ULP_FN = 2.0
SLACK = 1.001
WORDS, MAX_RADIUS = 16, 4
NOISE, BLUR, BRIGHTNESS, CONTRAST, GAMMA, INVERT = 1, 2, 4, 8, 16, 32
EVENT_NAMES = ("noise", "blur", "brightness", "contrast", "gamma", "invert")
C_EVENTS, C_STD, C_SIGMA, C_BRIGHT, C_CONTRAST, C_GAMMA, C_CALL_LO, C_CALL_HI, C_SAMPLE = range(9)
DRAW_TAG, NOISE_TAG = 0x40000000, 0x80000000
DEFAULTS = dict(noise_prob=0.1, noise_std=(0.0, 0.1), blur_prob=0.2, blur_sigma=(0.5, 1.0), brightness_prob=0.15,
                brightness_range=(0.75, 1.25), contrast_prob=0.15, contrast_range=(0.75, 1.25), gamma_prob=0.3,
                gamma_range=(0.7, 1.5), gamma_invert_prob=0.25)
ALL_ON = dict(DEFAULTS, noise_prob=1.0, blur_prob=1.0, brightness_prob=1.0, contrast_prob=1.0, gamma_prob=1.0)
# the statistics case of tests/test_augment_intensity_gpu.py; tests/test_augment_intensity_ref.py checks this seed with the
# restatement alone
STATS_SEED, STATS_CALLS, STATS_B = 2026, 2000, 10
DEFECTS = ("reflect_index", "radius_off_by_one", "stats_before_brightness", "sample_deviation", "invert_once", "noise_block_shift")


def patch(shape, seed, kind="ct"):
    """A windowed-CT-like patch in [0, 1]: smooth structure plus texture; 'flat' is a constant."""
    if kind == "flat":
        return np.full(shape, 0.375, dtype=np.float32)
    g = np.random.default_rng(seed)
    d, h, w = np.meshgrid(*[np.linspace(0, 1, s) for s in shape], indexing="ij")
    x = 0.5 + 0.3 * np.sin(5 * d + 1) * np.cos(4 * h) + 0.15 * w + 0.05 * g.standard_normal(shape)
    return np.clip(x, 0, 1).astype(np.float32)


# every stage alone and all together; R = 2 and R = 4; gamma on both sides of 1, with and without inversion
STAGE_CASES = {
    "none": {},
    "noise": dict(noise=0.08),
    "blur_r2": dict(blur=0.5),
    "blur_r3": dict(blur=0.7),
    "blur_r4": dict(blur=1.0),
    "brightness": dict(brightness=1.2),
    "contrast": dict(contrast=1.25),
    "contrast_low": dict(contrast=0.75),
    "gamma_below": dict(gamma=0.7),
    "gamma_above": dict(gamma=1.5),
    "gamma_below_invert": dict(gamma=0.8, invert=True),
    "gamma_above_invert": dict(gamma=1.4, invert=True),
    "all": dict(noise=0.1, blur=0.9, brightness=0.8, contrast=1.2, gamma=0.75, invert=True),
    "all_above": dict(noise=0.05, blur=0.6, brightness=1.25, contrast=0.8, gamma=1.45),
}

def gamma_below_share(cfg):
    lo, hi = cfg["gamma_range"]
    return 0.5 * cfg["gamma_prob"] if lo < 1 < hi else (cfg["gamma_prob"] if hi <= 1 and lo < 1 else 0.0)


def _key(seed):
    return int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF


def _unit(x):
    return F32(int(x) >> 8) * F32(2.0 ** -24)


def _between(lo, span, x):
    """fadd(fmul(span, u), lo), each rounded to fp32."""
    t = F32(F32(span) * _unit(x))
    return F32(t + F32(lo))


def config(**kw):
    """The fp32 fields of dua_aug_intensity_config as the host fills them: every span max - min in fp64, rounded once."""
    c = dict(DEFAULTS, **kw)
    out = {k: F32(c[k]) for k in ("noise_prob", "blur_prob", "brightness_prob", "contrast_prob", "gamma_prob", "gamma_invert_prob")}
    for name, key in (("noise_std", "noise_std"), ("blur_sigma", "blur_sigma"), ("brightness", "brightness_range"),
                      ("contrast", "contrast_range")):
        lo, hi = (float(v) for v in c[key])
        out[name + "_min"], out[name + "_span"] = F32(lo), F32(hi - lo)
    lo, hi = (float(v) for v in c["gamma_range"])
    out["gamma_min"], out["gamma_span_below"], out["gamma_span_above"] = F32(lo), F32(min(hi, 1.0) - lo), F32(hi - max(lo, 1.0))
    return out


def _row_bits(mask, values, call, b):
    row = np.zeros(WORDS, dtype=F32)
    row[C_STD:C_GAMMA + 1] = values
    bits = row.view(np.int32)
    bits[C_EVENTS] = mask
    bits[C_CALL_LO:C_SAMPLE + 1] = np.array([int(call) & 0xFFFFFFFF, (int(call) >> 32) & 0xFFFFFFFF, b], dtype=np.uint32).view(np.int32)
    return row


def draw_rows(B, counter, seed=0, **kw):
    """float32 [B, 16]: the rows of call ``counter``."""
    c = config(**kw)
    ctr = np.zeros((B, 3, 4), dtype=np.uint64)
    ctr[:, :, 0] = int(counter) & 0xFFFFFFFF
    ctr[:, :, 1] = (int(counter) >> 32) & 0xFFFFFFFF
    ctr[:, :, 2] = np.arange(B, dtype=np.uint64)[:, None]
    ctr[:, :, 3] = DRAW_TAG + np.arange(3, dtype=np.uint64)[None, :]
    words = philox4x32_10(ctr, _key(seed))
    rows = np.zeros((B, WORDS), dtype=F32)
    for b in range(B):
        w = words[b]
        mask, std, sigma, bright, contrast, gamma = 0, F32(0), F32(0), F32(1), F32(1), F32(1)
        if _unit(w[0][0]) < c["noise_prob"]:
            mask, std = mask | NOISE, _between(c["noise_std_min"], c["noise_std_span"], w[0][1])
        if _unit(w[0][2]) < c["blur_prob"]:
            mask, sigma = mask | BLUR, _between(c["blur_sigma_min"], c["blur_sigma_span"], w[0][3])
        if _unit(w[1][0]) < c["brightness_prob"]:
            mask, bright = mask | BRIGHTNESS, _between(c["brightness_min"], c["brightness_span"], w[1][1])
        if _unit(w[1][2]) < c["contrast_prob"]:
            mask, contrast = mask | CONTRAST, _between(c["contrast_min"], c["contrast_span"], w[1][3])
        if _unit(w[2][0]) < c["gamma_prob"]:
            mask |= GAMMA
            if _unit(w[2][1]) < F32(0.5) and c["gamma_min"] < F32(1):
                gamma = _between(c["gamma_min"], c["gamma_span_below"], w[2][2])
            else:
                gamma = _between(max(c["gamma_min"], F32(1)), c["gamma_span_above"], w[2][2])
            if _unit(w[2][3]) < c["gamma_invert_prob"]:
                mask |= INVERT
        rows[b] = _row_bits(mask, [std, sigma, bright, contrast, gamma], counter, b)
    return rows


def make_rows(specs, call=0):
    """Hand-built rows: one dict per sample with any of noise=std, blur=sigma, brightness=f, contrast=f, gamma=g, invert=True
    (and call=, sample= for the noise key; default ``call`` and the row's index)."""
    rows = []
    for b, s in enumerate(specs):
        mask = sum(bit for bit, name in zip((NOISE, BLUR, BRIGHTNESS, CONTRAST, GAMMA), EVENT_NAMES) if name in s)
        mask |= INVERT if s.get("invert") else 0
        values = [s.get("noise", 0.0), s.get("blur", 0.0), s.get("brightness", 1.0), s.get("contrast", 1.0), s.get("gamma", 1.0)]
        rows.append(_row_bits(mask, values, s.get("call", call), s.get("sample", b)))
    return np.stack(rows)


def split(row):
    bits = np.ascontiguousarray(row).view(np.int32)
    call = (int(bits[C_CALL_LO]) & 0xFFFFFFFF) | ((int(bits[C_CALL_HI]) & 0xFFFFFFFF) << 32)
    return int(bits[C_EVENTS]), [F32(v) for v in row[C_STD:C_GAMMA + 1]], call, int(bits[C_SAMPLE])


def noise_words(n, seed, call, b, shift=0):
    """uint64 [n, 2]: the word pair (a, b) of every voxel and which of the pair's two normals it takes (0: cos, 1: sin)."""
    i = np.arange(n, dtype=np.uint64) + np.uint64(shift)
    q = i >> np.uint64(2)
    ctr = np.zeros((n, 4), dtype=np.uint64)
    ctr[:, 0], ctr[:, 1], ctr[:, 2], ctr[:, 3] = call & 0xFFFFFFFF, (call >> 32) & 0xFFFFFFFF, b, np.uint64(NOISE_TAG) + q
    w = philox4x32_10(ctr, _key(seed))
    e = (i & np.uint64(3)).astype(np.int64)
    pair = e >> 1
    a = np.where(pair == 0, w[:, 0], w[:, 2])
    bb = np.where(pair == 0, w[:, 1], w[:, 3])
    return a, bb, e & 1


def normals(n, seed, call, b):
    """(z fp64 [n], ez [n]): the exact normals of the contract and the bound on the device's."""
    a, bb, second = noise_words(n, seed, call, b)
    u1 = ((a >> np.uint64(8)).astype(F64) + 1.0) * 2.0 ** -24
    u2 = (bb >> np.uint64(8)).astype(F64) * 2.0 ** -24
    r, theta = np.sqrt(-2.0 * np.log(u1)), 2.0 * math.pi * u2
    z = r * np.where(second == 1, np.sin(theta), np.cos(theta))
    return z, U * ((3 * ULP_FN + 3) * np.abs(z) + 2.0 * r * theta)


def radius_and_taps(sigma):
    """R = floor(4 sigma + 0.5) capped at MAX_RADIUS, and the 2 R + 1 normalised taps in fp64 from the fp32 sigma."""
    s = float(F32(sigma))
    R = int(min(max(math.floor(4.0 * s + 0.5), 0), MAX_RADIUS)) if s > 0 else 0
    i = np.arange(-R, R + 1, dtype=F64)
    e = np.exp(-(i * i) / (2.0 * s * s)) if R > 0 else np.ones(1)
    return R, e / e.sum()


def _reflect_index(n, R, defect=False):
    idx = np.arange(-R, n + R)
    if defect:                                             # the mirror that does not repeat the edge voxel
        idx = np.where(idx < 0, -idx, idx)
        return np.where(idx >= n, 2 * n - 2 - idx, idx)
    idx = np.where(idx < 0, -1 - idx, idx)
    return np.where(idx >= n, 2 * n - 1 - idx, idx)


def blur_axis(x, taps, R, axis, defect=False):
    """One pass along ``axis`` in the dtype of x / taps: sum over i of taps[i] x[reflect(j + i)]."""
    n = x.shape[axis]
    p = np.take(x, _reflect_index(n, R, defect), axis=axis)
    out = np.zeros_like(x)
    for i in range(2 * R + 1):
        out = out + taps[i] * np.take(p, np.arange(i, i + n), axis=axis)
    return out


def blur(x, sigma):
    """The blur of the contract in fp64 (x: [D, H, W])."""
    R, taps = radius_and_taps(sigma)
    for axis in (2, 1, 0):
        x = blur_axis(x, taps, R, axis)
    return x


def _stats(v, e):
    """(mean, dev, lo, hi) of v in fp64 and the bounds (dmean, ddev, dlohi) on the device's fp32 statistics."""
    n = v.size
    mean, dev, lo, hi = v.mean(), v.std(), v.min(), v.max()
    tiny = n * 2.0 ** -53
    dmean = e.mean() + U * abs(mean) + tiny * np.abs(v).mean()
    dvar = 4.0 * tiny * (v * v).mean()
    ddev = math.sqrt((e * e).mean()) + U * dev + (min(math.sqrt(dvar), dvar / (2.0 * dev)) if dev > 0 else math.sqrt(dvar))
    return (mean, dev, lo, hi), (dmean, ddev, e.max())


def transform(x, row, seed):
    """One patch x (float32 [D, H, W]) through ``row``: (fp64 result, bound on |device - result| per voxel)."""
    mask, (std, sigma, bright, contrast, gamma), call, b = split(row)
    v, e = np.asarray(x, dtype=F32).astype(F64), np.zeros(x.shape)
    if mask & NOISE:
        z, ez = normals(v.size, seed, call, b)
        t = float(std) * z.reshape(v.shape)
        v = v + t
        e = float(std) * ez.reshape(v.shape) + U * np.abs(t) + U * np.abs(v)
    if mask & BLUR:
        R, taps = radius_and_taps(sigma)
        for axis in (2, 1, 0):
            e = blur_axis(e, taps, R, axis) + (2 * R + 3) * U * blur_axis(np.abs(v) + e, taps, R, axis)
            v = blur_axis(v, taps, R, axis)
    if mask & BRIGHTNESS:
        f = float(bright)
        v = v * f
        e = f * e + U * np.abs(v)
    if mask & CONTRAST:
        f = float(contrast)
        (m, _, lo, hi), (dm, _, dlh) = _stats(v, e)
        c = v - m
        t = c * f
        w = t + m
        ev = f * (e + dm + U * np.abs(c)) + U * np.abs(t) + dm + U * np.abs(w)
        v, e = np.clip(w, lo, hi), np.maximum(ev, dlh)
    if mask & GAMMA:
        g = float(gamma)
        if mask & INVERT:
            v = -v
        (m, s, lo, hi), (dm, ds, dlh) = _stats(v, e)
        rng, drng = hi - lo, 2 * dlh + U * (hi - lo)
        den = rng + float(F32(1e-7))
        dden = drng + U * den
        a = v - lo
        da = e + dlh + U * np.abs(a)
        den_min = max(den - dden, 1e-7 * (1 - U))          # the device's denominator is at least fl(0 + 1e-7f)
        t = a / den
        dt = da / den_min + t * dden / den_min + 2 * U * t
        p = t ** g
        if g >= 1:
            dp = g * (t + dt) ** (g - 1) * dt
        else:
            inner = np.where(t > dt, g * np.maximum(t - dt, 1e-300) ** (g - 1) * dt, np.inf)
            dp = np.minimum(dt ** g, inner)
        dp = dp + 2 * U * ULP_FN * (p + dp)
        q = p * rng
        y = q + lo
        dy = (rng + drng) * dp + p * drng + U * np.abs(q) + dlh + U * np.abs(y)
        (m2, s2, _, _), (dm2, ds2, _) = _stats(y, dy)
        w = y - m2
        dw = dy + dm2 + U * np.abs(w)
        den2 = s2 + float(F32(1e-8))
        dden2 = ds2 + U * den2
        qq = w / den2
        den2_min = max(den2 - dden2, 1e-8 * (1 - U))
        dq = dw / den2_min + np.abs(qq) * dden2 / den2_min + 2 * U * np.abs(qq)
        r = qq * s
        dr = (s + ds) * dq + np.abs(qq) * ds + U * np.abs(r)       # dq is not small beside q on a flat patch: no first order here
        v = r + m
        e = dr + dm + U * np.abs(v)
        if mask & INVERT:
            v = -v
    return v, e * SLACK if mask else e


def reference(images, rows, seed):
    """A batch: images float32 [B, 1, D, H, W], rows float32 [B, 16] -> (fp64 [B, 1, D, H, W], bound of the same shape)."""
    pairs = [transform(images[b, 0], rows[b], seed) for b in range(images.shape[0])]
    return np.stack([p[0] for p in pairs])[:, None], np.stack([p[1] for p in pairs])[:, None]


def worst_ratio(got, want, bound):
    """max over voxels of |got - want| / bound (0 / 0 counts as 0: a voxel that must be reproduced exactly and is)."""
    diff = np.abs(np.asarray(got, dtype=F64) - want)
    if not np.all(np.isfinite(diff)):
        return math.inf
    ratio = np.where(diff == 0, 0.0, diff / np.maximum(bound, 1e-300))
    return float(ratio.max())


def _stats32(v, sample=False):
    """The statistics as the contract takes them: fp64 sums over the stored fp32 values, each statistic rounded to fp32 once."""
    d = v.astype(F64)
    n = d.size
    mean = d.sum() / n
    var = max((d * d).sum() / n - mean * mean, 0.0)
    if sample:
        var = var * n / (n - 1)
    return F32(mean), F32(math.sqrt(var)), F32(d.min()), F32(d.max())


def emulate(x, row, seed, defect=None):
    """One patch in fp32, operation by operation as the contract orders them (numpy float32 arithmetic rounds every operation
    once).  ``defect``: one of DEFECTS, a deliberate departure from the contract that the bound has to catch."""
    assert defect is None or defect in DEFECTS
    mask, (std, sigma, bright, contrast, gamma), call, b = split(row)
    v = np.asarray(x, dtype=F32).copy()
    before_brightness = None
    if mask & NOISE:
        a, bb, second = noise_words(v.size, seed, call, b, shift=1 if defect == "noise_block_shift" else 0)
        u1 = ((a >> np.uint64(8)) + np.uint64(1)).astype(F32) * F32(2.0 ** -24)
        u2 = (bb >> np.uint64(8)).astype(F32) * F32(2.0 ** -24)
        r = np.sqrt(F32(-2.0) * np.log(u1))
        theta = F32(2.0 * math.pi) * u2
        z = (r * np.where(second == 1, np.sin(theta), np.cos(theta))).astype(F32)
        v = v + (std * z).reshape(v.shape)
    if mask & BLUR:
        R, taps = radius_and_taps(sigma)
        if defect == "radius_off_by_one":
            R, taps = R - 1, taps[1:-1] / taps[1:-1].sum()
        for axis in (2, 1, 0):
            v = blur_axis(v, taps.astype(F32), R, axis, defect == "reflect_index")
    assert v.dtype == F32
    if mask & BRIGHTNESS:
        before_brightness = v
        v = v * bright
    if mask & CONTRAST:
        m, _, lo, hi = _stats32(before_brightness if defect == "stats_before_brightness" and before_brightness is not None else v)
        v = np.minimum(np.maximum((v - m) * contrast + m, lo), hi)
    if mask & GAMMA:
        if mask & INVERT:
            v = -v
        m, s, lo, hi = _stats32(v, sample=defect == "sample_deviation")
        rng = F32(hi - lo)
        t = (v - lo) / F32(rng + F32(1e-7))
        y = np.power(t, gamma) * rng + lo
        m2, s2, _, _ = _stats32(y)
        v = (y - m2) / F32(s2 + F32(1e-8)) * s + m
        if mask & INVERT and defect != "invert_once":
            v = -v
    assert v.dtype == F32
    return v


def check_statistics(rows, cfg):
    """Event frequencies within five binomial standard deviations of their probabilities and every value inside its range, over
    drawn rows float32 [n, 16]; invert is counted among the rows that have the gamma event."""
    n = len(rows)
    bits = np.ascontiguousarray(rows).view(np.int32)
    mask = bits[:, C_EVENTS]
    assert np.all((mask & ~63) == 0) and np.all(rows[:, C_SAMPLE + 1:] == 0)
    assert np.all((mask & INVERT == 0) | (mask & GAMMA != 0)), "invert only with a gamma event"

    def within(name, count, total, p):
        sd = math.sqrt(total * p * (1 - p))
        print(f"{name}: {count} of {total}, expected {total * p:.0f} +- {5 * sd:.0f}")
        assert abs(count - total * p) <= 5 * sd, (name, count, total * p)

    for bit, name in zip((NOISE, BLUR, BRIGHTNESS, CONTRAST, GAMMA), EVENT_NAMES):
        within(name, int(np.sum(mask & bit != 0)), n, cfg[name + "_prob"])
    ngamma = int(np.sum(mask & GAMMA != 0))
    within("invert", int(np.sum(mask & INVERT != 0)), ngamma, cfg["gamma_invert_prob"])
    within("gamma below 1", int(np.sum((mask & GAMMA != 0) & (rows[:, C_GAMMA] < 1))), n, gamma_below_share(cfg))
    neutral = (0.0, 0.0, 1.0, 1.0, 1.0)
    for col, bit, key, off in zip(range(C_STD, C_GAMMA + 1), (NOISE, BLUR, BRIGHTNESS, CONTRAST, GAMMA),
                                  ("noise_std", "blur_sigma", "brightness_range", "contrast_range", "gamma_range"), neutral):
        on = mask & bit != 0
        lo, hi = cfg[key]
        vals = rows[on, col]
        assert np.all(rows[~on, col] == F32(off)), key
        # fadd(fmul(span, u), lo) with u < 1 ends at most one rounding above hi
        assert np.all(vals >= F32(lo)) and np.all(vals <= F32(hi) * (1 + 2 * U)), (key, vals.min(), vals.max())
        print(f"{key}: {vals.min():.4f} .. {vals.max():.4f} in ({lo}, {hi})")
