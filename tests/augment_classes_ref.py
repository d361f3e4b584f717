"""CPU restatement of the class-balanced crop centres of include/dua_hip.h ("training input: class-balanced crop centres"),
written from that text and sharing no code with the package.  The Philox generator, u, mulhi, the volumes and the draw of every
other column come from tests/augment_ref.py; this module adds

  * the candidate sets per class (``class_sets``, ``RefClassVolume``) and their per-chunk exclusive prefix tables
    (``prefix_table``), by numpy.nonzero and numpy.bincount;
  * ``cum``: the effective weights, their fp64 running sum, one division, one rounding to fp32;
  * ``choose``: the smallest k with u < cum_k;
  * ``draw_classes``: the rows of a call, with the class choice and the uniform event of word 2.3.
"""
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from augment_ref import RefVolume, draw, mulhi, philox4x32_10, unit  # noqa: E402

CHUNK = 1024
UNIFORM, BAD = -1, -2


def class_sets(image, label, num_classes, image_threshold=0.0):
    """[K] arrays of ascending linear voxel indices: class 0 = label == 0 and image > threshold, class k = label == k."""
    flat_l = np.asarray(label, dtype=np.int64).reshape(-1)
    flat_i = np.asarray(image, dtype=np.float32).reshape(-1)
    sets = [np.nonzero((flat_l == 0) & (flat_i > np.float32(image_threshold)))[0]]
    return sets + [np.nonzero(flat_l == k)[0] for k in range(1, num_classes)]


def prefix_table(sets, voxels):
    """int64 [K, nchunks + 1]: entry c of row k = candidates of class k in chunks [0, c); the last entry the total."""
    nchunks = -(-voxels // CHUNK)
    out = np.zeros((len(sets), nchunks + 1), dtype=np.int64)
    for k, s in enumerate(sets):
        out[k, 1:] = np.cumsum(np.bincount(s // CHUNK, minlength=nchunks))
    return out


class RefClassVolume(RefVolume):
    """augment_ref.RefVolume with the candidate list of every class."""

    def __init__(self, image, label, num_classes, image_threshold=0.0):
        super().__init__(image, label, image_threshold)
        self.num_classes = int(num_classes)
        self.classes = class_sets(self.image.numpy(), self.label.numpy(), self.num_classes, image_threshold)
        self.counts = [len(s) for s in self.classes]


def ratios_of(class_ratios, num_classes):
    """``"present"`` = (0, 1, .., 1); otherwise the sequence itself."""
    if isinstance(class_ratios, str):
        assert class_ratios == "present"
        return [0.0] + [1.0] * (num_classes - 1)
    return [float(r) for r in class_ratios]


def effective(ratios, counts):
    return [float(r) if n > 0 else 0.0 for r, n in zip(ratios, counts)]


def cum(ratios, counts):
    """float32 [K].  E == 0 (no class with a positive ratio has a candidate) raises ValueError."""
    e = effective(ratios, counts)
    E = np.float64(0.0)
    for x in e:
        E = E + np.float64(x)
    if E == 0.0:
        raise ValueError("E == 0: no class with a positive ratio has a candidate")
    last = max(k for k, x in enumerate(e) if x > 0.0)
    out = np.zeros(len(e), dtype=np.float32)
    run = np.float64(0.0)
    for k, x in enumerate(e):
        run = run + np.float64(x)
        out[k] = np.float32(1.0) if k >= last else np.float32(run / E)
    return out


def choose(cum_row, u):
    """The smallest k with u < cum_k."""
    for k, c in enumerate(cum_row):
        if np.float32(u) < np.float32(c):
            return k
    raise AssertionError("u <= 1 - 2^-24 < 1 = cum of the last weighted class: the rule always chooses")


def _words(B, counter, seed):
    ctr = np.zeros((B, 3, 4), dtype=np.uint64)
    ctr[:, :, 0] = int(counter) & 0xFFFFFFFF
    ctr[:, :, 1] = (int(counter) >> 32) & 0xFFFFFFFF
    ctr[:, :, 2] = np.arange(B, dtype=np.uint64)[:, None]
    ctr[:, :, 3] = np.arange(3, dtype=np.uint64)[None, :]
    return philox4x32_10(ctr, (int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF))


def draw_classes(volumes, volume_ids, counter, seed=0, class_ratios=None, uniform_prob=0.0, roi=(96, 96, 96), return_ranks=False,
                 **base):
    """(ints int32 [B, 6], floats float32 [B, 2], chosen int32 [B]) of call ``counter``.  Every column but the starts is
    augment_ref.draw's; the centre is voxel mulhi(0.1, D H W) of the volume when u(2.3) < uniform_prob (chosen = -1), otherwise
    candidate mulhi(0.1, n_k) of the class k = choose(cum, u(0.0)) (chosen = k).  ``class_ratios=None``: the pos / neg set of
    augment_ref.draw when the uniform event does not happen (chosen = 1 for the foreground set, 0 for the background set: the
    device reports nothing then).  ``return_ranks``: also [(rank, set size)] per sample."""
    ints, floats, centres = draw(volumes, volume_ids, counter, seed=seed, roi=roi, return_centres=True, **base)
    words = _words(len(volume_ids), counter, seed)
    chosen = np.zeros(len(volume_ids), dtype=np.int32)
    ranks = []
    for b, vid in enumerate(volume_ids):
        vol, w = volumes[int(vid)], words[b]
        D, H, W = vol.shape
        if unit(w[2][3]) < np.float32(uniform_prob):
            rank, size = mulhi(w[0][1], D * H * W), D * H * W
            centre, chosen[b] = rank, UNIFORM
        elif class_ratios is not None:
            k = choose(cum(ratios_of(class_ratios, vol.num_classes), vol.counts), unit(w[0][0]))
            rank, size = mulhi(w[0][1], vol.counts[k]), vol.counts[k]
            centre, chosen[b] = int(vol.classes[k][rank]), k
        else:
            is_fg, centre = centres[b]
            size = len(vol.fg) if is_fg else len(vol.bg)
            rank, chosen[b] = mulhi(w[0][1], size), int(is_fg)
        ranks.append((rank, size))
        c = (centre // (H * W), (centre // W) % H, centre % W)
        ints[b, 1:4] = [min(max(x - r // 2, 0), s - r) for x, r, s in zip(c, roi, (D, H, W))]
    return (ints, floats, chosen, ranks) if return_ranks else (ints, floats, chosen)


def class_probabilities(ratios, counts, uniform_prob):
    """[K + 1]: the probability of every class and, last, of the uniform event."""
    e = effective(ratios, counts)
    E = sum(e)
    return [x / E * (1.0 - uniform_prob) for x in e] + [float(uniform_prob)]


def layered_volume(shape, num_classes, seed, absent=(), threshold_part=True):
    """A seeded volume for the table and draw tests: blobs of the ids in [0, num_classes) minus ``absent``, an image that lies
    partly at or below 0 (so that the threshold removes part of class 0), then by hand: the first voxel is the only one of class
    1, the last voxel the only one of class 2, and class 3 lives only in the last, partial chunk (where the class counts allow).
    Returns (image fp32, label uint8)."""
    g = torch.Generator().manual_seed(seed)
    image = torch.rand(shape, generator=g) - (0.3 if threshold_part else -0.1)
    ids = [k for k in range(num_classes) if k not in absent and k not in (1, 2, 3)] or [0]
    coarse = torch.randint(0, len(ids), tuple(-(-s // 4) for s in shape), generator=g)
    label = torch.tensor(ids, dtype=torch.uint8)[coarse]
    label = label.repeat_interleave(4, 0).repeat_interleave(4, 1).repeat_interleave(4, 2)[:shape[0], :shape[1], :shape[2]].contiguous()
    flat = label.reshape(-1)
    n = flat.numel()
    if num_classes > 3 and 3 not in absent:
        tail = (n - 1) // CHUNK * CHUNK                       # first voxel of the last chunk
        flat[tail + (n - tail) // 3:tail + 2 * (n - tail) // 3] = 3
    if num_classes > 1 and 1 not in absent:
        flat[0] = 1
    if num_classes > 2 and 2 not in absent:
        flat[n - 1] = 2
    return image.contiguous(), label


# the frequency case: tests/test_augment_classes_ref.py bounds the restated frequencies of this seed,
# tests/test_augment_classes_gpu.py draws the same calls on the device
FREQ = dict(shape=(19, 23, 29), K=6, volume_seed=11, absent=(4,), ratios=[1.0, 0.0, 3.0, 2.0, 5.0, 1.0], uniform_prob=0.25, seed=31,
            calls=100, B=200, roi=(8, 8, 8))


def frequency_volume():
    image, label = layered_volume(FREQ["shape"], FREQ["K"], FREQ["volume_seed"], absent=FREQ["absent"])
    return RefClassVolume(image, label, FREQ["K"])


def check_frequencies(chosen, vol):
    n = len(chosen)
    probs = class_probabilities(FREQ["ratios"], vol.counts, FREQ["uniform_prob"])
    for k, p in enumerate(probs):
        got = int(np.sum(chosen == (k if k < FREQ["K"] else UNIFORM)))
        bound = 5 * math.sqrt(n * p * (1 - p)) + 1
        print(f"{'uniform' if k == FREQ['K'] else f'class {k}'}: {got} of {n}, expected {n * p:.0f} +- {bound:.0f}")
        assert abs(got - n * p) <= bound, (k, got, n * p)
        if p == 0:
            assert got == 0, k
