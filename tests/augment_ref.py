"""CPU restatement of the augmented-batch contract of include/dua_hip.h ("training input: augmented batches from
device-resident volumes"), written from that text and sharing no code with the package: Philox4x32-10 in numpy integers, the
draw rules with torch.nonzero for the candidate lists, the patch transform with torch operators.  The GPU tests compare the
kernels with it bit for bit; tests/test_augment_ref.py pins it down first."""
import math

import numpy as np
import torch

M32 = np.uint64(0xFFFFFFFF)
DEFAULTS = dict(roi=(96, 96, 96), class_ids=tuple(range(16)), pos=1, neg=1, flip_prob=0.1, rot90_prob=0.1, max_k=3,
                scale_prob=0.1, scale_factors=0.1, shift_prob=0.5, shift_offsets=0.1, seed=0)


def philox4x32_10(counter, key):
    """counter: integer array [..., 4]; key: (k0, k1).  Returns uint64 [..., 4] holding the four 32-bit output words."""
    c = np.asarray(counter, dtype=np.uint64) & M32
    k0, k1 = np.uint64(key[0]) & M32, np.uint64(key[1]) & M32
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[..., 0]
        p1 = np.uint64(0xCD9E8D57) * c[..., 2]
        c = np.stack([((p1 >> np.uint64(32)) ^ c[..., 1] ^ k0) & M32, p1 & M32,
                      ((p0 >> np.uint64(32)) ^ c[..., 3] ^ k1) & M32, p0 & M32], axis=-1)
        k0 = (k0 + np.uint64(0x9E3779B9)) & M32
        k1 = (k1 + np.uint64(0xBB67AE85)) & M32
    return c


def unit(x):
    """u = (x >> 8) * 2^-24, exact in fp32."""
    return np.float32(int(x) >> 8) * np.float32(2.0 ** -24)


def mulhi(x, n):
    return (int(x) * int(n)) >> 32


def symmetric(half_width, x):
    """fadd(fmul(2 * half_width, u), -half_width), each operation rounded to fp32."""
    hw = np.float32(half_width)
    t = np.float32(np.float32(2.0) * hw) * unit(x)
    return np.float32(t + np.float32(-hw))


class RefVolume:
    """image fp32 [D, H, W], label uint8 [D, H, W] on the CPU, with both candidate lists (ascending linear index)."""

    def __init__(self, image, label, image_threshold=0.0):
        self.image, self.label = image.float().contiguous(), label.to(torch.uint8).contiguous()
        flat_l, flat_i = self.label.reshape(-1), self.image.reshape(-1)
        self.fg = torch.nonzero(flat_l > 0).reshape(-1).numpy()
        self.bg = torch.nonzero((flat_l == 0) & (flat_i > image_threshold)).reshape(-1).numpy()
        self.shape = tuple(self.image.shape)


def draw(volumes, volume_ids, counter, seed=0, roi=(96, 96, 96), pos=1, neg=1, flip_prob=0.1, rot90_prob=0.1, max_k=3,
         scale_prob=0.1, scale_factors=0.1, shift_prob=0.5, shift_offsets=0.1, return_centres=False, **_):
    """(int32 [B, 6]: volume, start_d, start_h, start_w, flip_bits, k; float32 [B, 2]: scale, shift) of call ``counter``."""
    B = len(volume_ids)
    ctr = np.zeros((B, 3, 4), dtype=np.uint64)
    ctr[:, :, 0] = int(counter) & 0xFFFFFFFF
    ctr[:, :, 1] = (int(counter) >> 32) & 0xFFFFFFFF
    ctr[:, :, 2] = np.arange(B, dtype=np.uint64)[:, None]
    ctr[:, :, 3] = np.arange(3, dtype=np.uint64)[None, :]
    words = philox4x32_10(ctr, (int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF))
    ints = np.zeros((B, 6), dtype=np.int32)
    floats = np.zeros((B, 2), dtype=np.float32)
    centres = []
    pos_fraction = np.float32(float(pos) / (float(pos) + float(neg)))
    for b, vid in enumerate(volume_ids):
        vol, w = volumes[int(vid)], words[b]
        if len(vol.fg) == 0:
            chosen, is_fg = vol.bg, False
        elif len(vol.bg) == 0:
            chosen, is_fg = vol.fg, True
        else:
            is_fg = bool(unit(w[0][0]) < pos_fraction)
            chosen = vol.fg if is_fg else vol.bg
        centre = int(chosen[mulhi(w[0][1], len(chosen))])
        D, H, W = vol.shape
        cd, ch, cw = centre // (H * W), (centre // W) % H, centre % W
        starts = [min(max(c - r // 2, 0), s - r) for c, r, s in zip((cd, ch, cw), roi, (D, H, W))]
        flip = 0
        for axis, x in enumerate((w[0][2], w[0][3], w[1][0])):
            if unit(x) < np.float32(flip_prob):
                flip |= 1 << axis
        k = 1 + mulhi(w[1][2], max_k) if unit(w[1][1]) < np.float32(rot90_prob) else 0
        scale = symmetric(scale_factors, w[2][0]) if unit(w[1][3]) < np.float32(scale_prob) else np.float32(0)
        shift = symmetric(shift_offsets, w[2][2]) if unit(w[2][1]) < np.float32(shift_prob) else np.float32(0)
        ints[b] = [int(vid)] + starts + [flip, k]
        floats[b] = [scale, shift]
        centres.append((is_fg, centre))
    return (ints, floats, centres) if return_centres else (ints, floats)


def apply(volumes, ints, floats, roi, class_ids):
    """(images fp32 [B, 1, *roi], labels fp32 [B, C, *roi]) for the rows of ``draw``."""
    images, labels = [], []
    ids = torch.tensor(list(class_ids), dtype=torch.int64).view(-1, 1, 1, 1)
    for (vid, sd, sh, sw, flip, k), (scale, shift) in zip(np.asarray(ints).tolist(), np.asarray(floats, dtype=np.float32)):
        vol = volumes[vid]
        window = (slice(sd, sd + roi[0]), slice(sh, sh + roi[1]), slice(sw, sw + roi[2]))
        p, q = vol.image[window], vol.label[window]
        for ax in (0, 1, 2):
            if flip >> ax & 1:
                p, q = p.flip(ax), q.flip(ax)
        p, q = torch.rot90(p, k, (0, 1)), torch.rot90(q, k, (0, 1))
        factor = torch.tensor(1.0, dtype=torch.float32) + torch.tensor(float(scale), dtype=torch.float32)
        images.append(((p * factor) + torch.tensor(float(shift), dtype=torch.float32))[None])
        labels.append((q.to(torch.int64)[None] == ids).float())
    return torch.stack(images).contiguous(), torch.stack(labels).contiguous()


def synthetic_volume(shape, seed, kind="both", classes=16):
    """A seeded test volume: blobs of class ids on a background whose image is partly above and partly below zero.
    kind: 'both' | 'no_fg' (label all zero) | 'no_bg' (every voxel labelled) | 'corner' (one foreground voxel at the far corner,
    no background candidate)."""
    g = torch.Generator().manual_seed(seed)
    image = torch.rand(shape, generator=g) - 0.3                       # ~30 % of the voxels at or below the threshold 0
    if kind == "no_fg":
        label = torch.zeros(shape, dtype=torch.uint8)
    elif kind == "no_bg":
        label = torch.randint(1, classes, shape, generator=g).to(torch.uint8)
    elif kind == "corner":
        label = torch.zeros(shape, dtype=torch.uint8)
        label[-1, -1, -1] = 5
        image = -image.abs() - 0.1                                    # nothing above the threshold: foreground is the only set
    else:
        coarse = torch.randint(0, classes * 3, tuple(-(-s // 8) for s in shape), generator=g)
        coarse = torch.where(coarse < classes, coarse, torch.zeros_like(coarse))       # two thirds background
        label = coarse.repeat_interleave(8, 0).repeat_interleave(8, 1).repeat_interleave(8, 2)
        label = label[:shape[0], :shape[1], :shape[2]].to(torch.uint8).contiguous()
    return image.contiguous(), label


def stats_volume():
    """The volume of the statistics case: foreground only in the slab d < 12, background candidates only in d >= 28, so that
    with roi_d = 16 the chosen set shows in the row itself (start_d <= 3 for a foreground centre, >= 20 for a background one)."""
    shape = (40, 36, 44)
    g = torch.Generator().manual_seed(4)
    label = torch.zeros(shape, dtype=torch.uint8)
    label[:12] = torch.randint(1, 16, (12,) + shape[1:], generator=g).to(torch.uint8)
    image = -torch.rand(shape, generator=g) - 0.1
    image[28:] = torch.rand((12,) + shape[1:], generator=g) + 0.1
    return image.contiguous(), label


# the statistics case of tests/test_augment_gpu.py; tests/test_augment_ref.py checks this seed with the restatement alone
STATS_SEED, STATS_CALLS, STATS_B = 2024, 2000, 10


def event_counts(rows_int, rows_float, centres_fg):
    """The counts the statistics test bounds, from drawn rows."""
    k = rows_int[:, 5]
    return {"foreground": int(np.sum(centres_fg)), "flip0": int(np.sum(rows_int[:, 4] & 1 != 0)),
            "flip1": int(np.sum(rows_int[:, 4] & 2 != 0)), "flip2": int(np.sum(rows_int[:, 4] & 4 != 0)),
            "rotation": int(np.sum(k > 0)), "scale": int(np.sum(rows_float[:, 0] != 0)),
            "shift": int(np.sum(rows_float[:, 1] != 0)), "k1": int(np.sum(k == 1)), "k2": int(np.sum(k == 2)),
            "k3": int(np.sum(k == 3))}


def check_event_counts(counts, n, cfg):
    """Every count within n p +- 5 sqrt(n p (1 - p)) of its configured probability; each k within the same bound of a third of
    the rotations that happened.  A correct generator leaves such a bound with probability below 1e-6 per count."""
    probs = {"foreground": cfg["pos"] / (cfg["pos"] + cfg["neg"]), "flip0": cfg["flip_prob"], "flip1": cfg["flip_prob"],
             "flip2": cfg["flip_prob"], "rotation": cfg["rot90_prob"], "scale": cfg["scale_prob"], "shift": cfg["shift_prob"]}
    for name, p in probs.items():
        print(f"{name}: {counts[name]} of {n}, expected {n * p:.0f} +- {5 * math.sqrt(n * p * (1 - p)):.0f}")
        assert abs(counts[name] - n * p) <= 5 * math.sqrt(n * p * (1 - p)), (name, counts[name], n * p)
    rot = counts["rotation"]
    for name in ("k1", "k2", "k3"):
        print(f"{name}: {counts[name]} of {rot} rotations, expected {rot / 3:.0f} +- {5 * math.sqrt(rot * 2 / 9):.0f}")
        assert abs(counts[name] - rot / 3) <= 5 * math.sqrt(rot * (1 / 3) * (2 / 3)), (name, counts[name], rot)
