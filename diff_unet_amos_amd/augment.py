"""Augmented training batches produced on the device from cached volumes.

The reference builds a batch on the host: MONAI's RandCropByPosNegLabeld, three RandFlipd, RandRotate90d,
RandScaleIntensityd and RandShiftIntensityd (utils.py:143-160), then Engine.convert_labels (engine.py:157-165) expands the
label map into one-hot channels.  Here the volumes the reference caches (after its deterministic transforms) live in device
memory, and two launches per batch (csrc/augment.hip) write exactly the two tensors ``NativeConvTrainer.step`` takes::

    producer = DeviceBatchProducer([DeviceVolume(image, label) for image, label in cases])
    images, labels = producer.next(ids)          # no host-to-device copy of voxels, no host synchronisation
    trainer.step(images, labels)

What the random words decide and how the patch is transformed is fixed in include/dua_hip.h ("training input"), not by
MONAI's source; tests/augment_ref.py restates it independently.

The reference's second label form, centroid-distance label smoothing (dataset/cache_dataset.py:105-153, ``label_smoothing:
true``), comes from the same two launches: the cached case stays a uint8 label map plus three floats per class, and the
smoothed channels are evaluated where the patch is written::

    volumes = [DeviceVolume(image, label, num_classes=14) for image, label in cases]
    producer = DeviceBatchProducer(volumes, class_ids=range(1, 14), smoothing=LabelSmoothing())

``class_ids=range(1, K)`` is the reference's ``labels[:, 1:]`` for training (engine.py:159-160).  tests/label_smoothing_ref.py
restates the definition; tests/golden/label_smoothing_golden.npz holds the reference's own outputs.

Random rotation and zoom, the two spatial augmentations that resample (the reference has neither; nnU-Net and MONAI's
RandAffined / RandZoomd apply them by default), come from the same two launches as well::

    producer = DeviceBatchProducer(volumes, rotate_prob=0.2, rotate_range=(0.52, 0.52, 0.52), zoom_prob=0.2,
                                   zoom_range=(0.7, 1.4))
    images, labels = producer.next(ids)          # trilinear image, nearest label, pad_value outside the volume

include/dua_hip.h ("random rotation and zoom") fixes them; tests/augment_affine_ref.py restates that text.

The intensity half of that recipe (nnU-Net's defaults: Gaussian noise, Gaussian blur, multiplicative brightness, contrast, gamma
with and without inversion) is a stage of its own after ``apply``, on the images alone (csrc/augment_intensity.hip: one draw
launch, one tiled noise-and-blur pass, four pointwise passes separated by deterministic reductions)::

    aug = IntensityAugmenter(roi=(96, 96, 96), seed=7)
    producer = DeviceBatchProducer(volumes, intensity=aug)
    images, labels = producer.next(ids)          # labels untouched; producer.intensity_rows holds the rows, for logging
    images = aug(images)                         # or on any fp32 [B, 1, *roi] batch, without a producer

include/dua_hip.h ("training input: intensity augmentation") fixes it; tests/augment_intensity_ref.py restates that text.

Crop centres can be balanced by class instead of by foreground and background: a class is drawn first, then a voxel of that
class, so that a small organ is the centre of a patch as often as a large one (MONAI's ``RandCropByLabelClassesd(ratios=...)``;
nnU-Net's oversampling picks among the classes that occur in the case and otherwise crops anywhere)::

    volumes = [DeviceVolume(image, label, num_classes=16) for image, label in cases]
    producer = DeviceBatchProducer(volumes, class_ratios=[0, 1, 1, 4, ...])               # MONAI's ratios, one per class
    producer = DeviceBatchProducer(volumes, class_ratios="present", uniform_prob=0.67)    # nnU-Net's rule
    images, labels = producer.next(ids)          # producer.chosen_classes, producer.class_tally: what was drawn, on the device

Still one draw launch and one apply launch; a row drawn this way is an ordinary ``params`` row.  include/dua_hip.h ("training
input: class-balanced crop centres") fixes it; tests/augment_classes_ref.py restates that text.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import math

import torch

from . import _native as nv
from . import ops

PARAM_COLUMNS = ("volume", "start_d", "start_h", "start_w", "flip_bits", "k", "scale", "shift")


def split_params(params):
    """``params`` (int32 [B, 8]) as (int32 [B, 6]: volume, start_d, start_h, start_w, flip_bits, k; fp32 [B, 2]: scale, shift)."""
    assert params.dtype == torch.int32 and params.dim() == 2 and params.shape[1] == nv.AUG_PARAM_WORDS
    return params[:, :nv.AUG_SCALE], params[:, nv.AUG_SCALE:].contiguous().view(torch.float32)


def pack_params(ints, floats, device=None):
    """The inverse of ``split_params``: a params tensor from [B, 6] integers and [B, 2] floats (hand-built or logged rows)."""
    ints = torch.as_tensor(ints, dtype=torch.int32).reshape(-1, nv.AUG_SCALE)
    floats = torch.as_tensor(floats, dtype=torch.float32).reshape(-1, nv.AUG_PARAM_WORDS - nv.AUG_SCALE)
    if ints.shape[0] != floats.shape[0]:
        raise ValueError("pack_params: as many rows of floats as of integers")
    out = torch.cat([ints.cpu(), floats.cpu().contiguous().view(torch.int32)], dim=1).contiguous()
    return out.to(device) if device is not None else out


AFFINE_COLUMNS = ("matrix", "tan_half", "zoom", "events", "pad_value")


def split_affine(affine):
    """``affine`` (fp32 [B, 16]) as (matrix fp32 [B, 3, 3]: source offset = matrix @ output offset; tan_half fp32 [B, 3]: the
    tangent of half the rotation angle about d, h, w; zoom fp32 [B]; events int32 [B]: bit 0 rotation, bit 1 zoom; pad_value
    fp32 [B])."""
    assert affine.dtype == torch.float32 and affine.dim() == 2 and affine.shape[1] == nv.AUG_AFFINE_WORDS
    events = affine[:, nv.AUG_AFFINE_EVENTS:nv.AUG_AFFINE_EVENTS + 1].contiguous().view(torch.int32)[:, 0]
    return (affine[:, :nv.AUG_AFFINE_T].reshape(-1, 3, 3), affine[:, nv.AUG_AFFINE_T:nv.AUG_AFFINE_ZOOM],
            affine[:, nv.AUG_AFFINE_ZOOM], events, affine[:, nv.AUG_AFFINE_PAD])


INTENSITY_COLUMNS = ("events", "noise_std", "blur_sigma", "brightness", "contrast", "gamma", "call", "sample")
INTENSITY_EVENTS = ("noise", "blur", "brightness", "contrast", "gamma", "invert")


def split_intensity(rows):
    """``rows`` (fp32 [B, 16]) as a dict on the host: ``events`` int32 [B] (bit i = ``INTENSITY_EVENTS[i]``), ``noise_std``,
    ``blur_sigma``, ``brightness``, ``contrast``, ``gamma`` fp32 [B], ``call`` (a list of Python integers: the 64-bit call counter
    the row was drawn with) and ``sample`` int32 [B] (its index in that call).  Reads the rows: a host synchronisation."""
    assert rows.dtype == torch.float32 and rows.dim() == 2 and rows.shape[1] == nv.AUG_INTENSITY_WORDS
    r = rows.detach().cpu().contiguous()
    bits = r.view(torch.int32)
    lo, hi = bits[:, nv.AUG_INTENSITY_CALL_LO].tolist(), bits[:, nv.AUG_INTENSITY_CALL_HI].tolist()
    return {"events": bits[:, nv.AUG_INTENSITY_EVENTS].clone(), "noise_std": r[:, nv.AUG_INTENSITY_STD].clone(),
            "blur_sigma": r[:, nv.AUG_INTENSITY_SIGMA].clone(), "brightness": r[:, nv.AUG_INTENSITY_BRIGHT].clone(),
            "contrast": r[:, nv.AUG_INTENSITY_CONTRAST_F].clone(), "gamma": r[:, nv.AUG_INTENSITY_GAMMA_V].clone(),
            "call": [((h & 0xFFFFFFFF) << 32) | (l & 0xFFFFFFFF) for l, h in zip(lo, hi)],
            "sample": bits[:, nv.AUG_INTENSITY_SAMPLE].clone()}


class IntensityAugmenter:
    """Gaussian noise, Gaussian blur, brightness, contrast and gamma (with and without inversion) on ``images`` fp32
    [B, 1, *roi], each with its own probability per sample, in that order; the defaults are nnU-Net's.  ``draw(B)`` returns the
    decisions as ``rows`` (fp32 [B, 16] on the device; ``split_intensity`` names the columns), ``apply(images, rows)`` the
    transformed images, ``aug(images)`` both.  Deterministic for a given (seed, call counter): the call counter is a 64-bit
    device word the draw launch itself advances, so a captured call moves on with every replay, and a logged ``rows`` tensor
    with the seed replays its batch bit for bit, the noise included.  No host read, no allocation inside ``apply`` once the
    scratch for a batch size exists (call ``apply`` once before capturing it).

    noise: x += N(0, std^2), std from ``noise_std``; blur: ``scipy.ndimage.gaussian_filter(x, sigma, mode="reflect")`` with
    sigma from ``blur_sigma`` (at most 1: a radius of 4 voxels); brightness: x *= f; contrast: x = clamp((x - mean) f + mean,
    min, max); gamma: batchgenerators' gamma transform with ``retain_stats``, the exponent from the part of ``gamma_range``
    below 1 half of the time, on -x with probability ``gamma_invert_prob``.  Statistics are per patch."""

    def __init__(self, roi, seed=0, noise_prob=0.1, noise_std=(0.0, 0.1), blur_prob=0.2, blur_sigma=(0.5, 1.0), brightness_prob=0.15,
                 brightness_range=(0.75, 1.25), contrast_prob=0.15, contrast_range=(0.75, 1.25), gamma_prob=0.3,
                 gamma_range=(0.7, 1.5), gamma_invert_prob=0.25, device="cuda"):
        try:
            roi = tuple(int(r) for r in roi)
        except (TypeError, ValueError):
            raise ValueError(f"IntensityAugmenter: roi is three extents, got {roi}") from None
        if len(roi) != 3 or min(roi) < 4 or roi[0] * roi[1] * roi[2] >= 2 ** 31:
            raise ValueError(f"IntensityAugmenter: roi is three extents, each at least 4, fewer than 2^31 voxels, got {roi}")
        probs = dict(noise_prob=noise_prob, blur_prob=blur_prob, brightness_prob=brightness_prob, contrast_prob=contrast_prob,
                     gamma_prob=gamma_prob, gamma_invert_prob=gamma_invert_prob)
        for name, p in probs.items():
            try:
                ok = 0.0 <= float(p) <= 1.0
            except (TypeError, ValueError):
                ok = False
            if not ok:
                raise ValueError(f"IntensityAugmenter: {name} is a probability, got {p}")
        ranges = dict(noise_std=noise_std, blur_sigma=blur_sigma, brightness_range=brightness_range, contrast_range=contrast_range,
                      gamma_range=gamma_range)
        for name, r in ranges.items():
            try:
                r = tuple(float(v) for v in r)
            except (TypeError, ValueError):
                r = ()
            if len(r) != 2 or not (math.isfinite(r[0]) and math.isfinite(r[1]) and r[0] <= r[1] and abs(r[1]) <= 3.0e38):
                raise ValueError(f"IntensityAugmenter: {name} is (min, max) with min <= max, finite, got {ranges[name]}")
            ranges[name] = r
        if ranges["noise_std"][0] < 0:
            raise ValueError(f"IntensityAugmenter: noise_std is not negative, got {noise_std}")
        if not 0 < ranges["blur_sigma"][0] or ranges["blur_sigma"][1] > 1.0:
            raise ValueError(f"IntensityAugmenter: blur_sigma lies in (0, 1] (a radius of at most {nv.AUG_INTENSITY_MAX_RADIUS} voxels), "
                             f"got {blur_sigma}")
        for name in ("brightness_range", "contrast_range", "gamma_range"):
            if not ranges[name][0] > 0:
                raise ValueError(f"IntensityAugmenter: {name} is positive, got {ranges[name]}")
        device = torch.device(device)
        if device.type != "cuda":
            raise ValueError(f"IntensityAugmenter: a GPU device, not {device}")
        self.roi, self.seed, self.device = roi, int(seed), device
        self.settings = dict(probs, **ranges)
        g0, g1 = ranges["gamma_range"]
        span = lambda r: r[1] - r[0]                          # in fp64, rounded to fp32 once by the structure
        self.cfg = nv.AugIntensityConfig(
            float(noise_prob), ranges["noise_std"][0], span(ranges["noise_std"]),
            float(blur_prob), ranges["blur_sigma"][0], span(ranges["blur_sigma"]),
            float(brightness_prob), ranges["brightness_range"][0], span(ranges["brightness_range"]),
            float(contrast_prob), ranges["contrast_range"][0], span(ranges["contrast_range"]),
            float(gamma_prob), g0, min(g1, 1.0) - g0, g1 - max(g0, 1.0), float(gamma_invert_prob), 0)
        self._counter = self._scratch = None

    def _state(self):
        if self._counter is None:
            self._counter = torch.zeros(1, dtype=torch.int64, device=self.device)
        return self._counter

    @property
    def counter(self):
        """The call counter the next ``draw`` will use (reads the device word: a host synchronisation)."""
        return int(self._state().item()) & (2 ** 64 - 1)

    def draw(self, B, counter=None):
        """The decisions of one batch as ``rows`` (fp32 [B, 16] on the device).  ``counter=None`` uses and advances the
        augmenter's device-resident call counter; an integer is used for this call only."""
        B = int(B)
        if B < 1:
            raise ValueError(f"IntensityAugmenter.draw: at least one sample, got B = {B}")
        rows = torch.empty((B, nv.AUG_INTENSITY_WORDS), dtype=torch.float32, device=self.device)
        return ops.aug_intensity_draw(self.cfg, self.seed, self._state(), rows, counter_value=counter)

    def apply(self, images, rows, out=None):
        """``images`` (fp32 [B, 1, *roi]) through ``rows``; ``out`` may be ``images`` (in place), default a new tensor."""
        if not (torch.is_tensor(images) and images.is_cuda and images.dtype == torch.float32 and images.dim() == 5 and
                tuple(images.shape[1:]) == (1,) + self.roi):
            raise ValueError(f"IntensityAugmenter.apply: images is a float32 device tensor [B, 1, {self.roi[0]}, {self.roi[1]}, "
                             f"{self.roi[2]}]")
        B = images.shape[0]
        need = ops.aug_intensity_scratch_bytes(B, self.roi)
        if self._scratch is None or self._scratch.numel() < need or self._scratch.device != images.device:
            self._scratch = torch.empty(need, dtype=torch.uint8, device=images.device)
        if out is None:
            out = torch.empty_like(images)
        return ops.aug_intensity_apply(images, rows, self.seed, out, self._scratch)

    def __call__(self, images, out=None):
        return self.apply(images, self.draw(images.shape[0]), out=out)


@dataclasses.dataclass(frozen=True)
class LabelSmoothing:
    """Centroid-distance label smoothing (dataset/cache_dataset.py:105-153, the ``rational`` form): channel k of a voxel at
    distance d from the centroid of class k holds ``| [label == k] - alpha / (d ** order + epsilon) |``; the defaults are the
    reference's (utils.py:112-113, cache_dataset.py:43-47).

    The value is unbounded near a centroid, as it is in the reference: a class of one voxel has d = 0 there and the value is
    ``|1 - alpha / epsilon|``, 3e5 with the defaults.  ``max_value=None`` keeps that; a number clamps every channel from above
    and changes nothing else.  Pass one when training with fp16 activations (``NativeConvTrainer``'s default): ``2 * label - 1``
    leaves the fp16 range above 32 752."""
    alpha: float = 0.3
    order: float = 1.0
    epsilon: float = 1e-6
    max_value: float | None = None

    def __post_init__(self):
        if not (math.isfinite(self.alpha) and self.alpha >= 0):
            raise ValueError(f"LabelSmoothing: alpha is finite and not negative, got {self.alpha}")
        if not (math.isfinite(self.order) and self.order > 0):
            raise ValueError(f"LabelSmoothing: order is finite and positive, got {self.order}")
        if not (math.isfinite(self.epsilon) and self.epsilon >= 2.0 ** -126):
            raise ValueError(f"LabelSmoothing: epsilon is a positive normal fp32 number, got {self.epsilon}")
        if self.max_value is not None and not self.max_value > 0:
            raise ValueError(f"LabelSmoothing: max_value is None or positive, got {self.max_value}")

    def native(self):
        return nv.AugSmoothing(self.alpha, self.order, self.epsilon, math.inf if self.max_value is None else self.max_value)


def class_cum(ratios, counts):
    """The ``cum`` row of include/dua_hip.h ("class-balanced crop centres") as a list of K Python floats, to be rounded to fp32
    once: ``ratios`` where the class has candidates (``counts`` > 0) and 0 elsewhere, summed in class order in fp64, the running
    sum divided by the total, and exactly 1.0 from the last weighted class on.  None when no weighted class has a candidate."""
    e = [float(r) if int(n) > 0 else 0.0 for r, n in zip(ratios, counts)]
    total = 0.0
    for x in e:
        total += x
    if total == 0.0:
        return None
    last = max(k for k, x in enumerate(e) if x > 0.0)
    run, cum = 0.0, []
    for k, x in enumerate(e):
        run += x
        cum.append(1.0 if k >= last else run / total)
    return cum


class DeviceVolume:
    """One cached case on the device: ``image`` fp32 [D, H, W] (or [1, D, H, W]) and ``label`` uint8 [D, H, W] of class ids,
    with the candidate sets of RandCropByPosNegLabel counted once (foreground = label > 0; background = label == 0 and
    image > image_threshold) and their per-chunk prefix tables left on the device.

    ``num_classes`` (background included) also computes, once, what label smoothing needs: ``centroids`` fp32 [K, 3] (the mean
    index of every class, zeros for an absent one, as in the reference), ``class_counts`` int64 [K] and ``class_sums`` int64
    [K, 3], all on the device.  A label map that holds an id >= num_classes is refused."""

    def __init__(self, image, label, image_threshold=0.0, device="cuda", num_classes=None):
        if not (torch.is_tensor(image) and torch.is_tensor(label)):
            raise ValueError("DeviceVolume: image and label are tensors")
        if image.dim() == 4 and image.shape[0] == 1:
            image = image[0]
        if label.dim() == 4 and label.shape[0] == 1:
            label = label[0]
        if image.dtype != torch.float32 or label.dtype != torch.uint8:
            raise ValueError(f"DeviceVolume: image must be float32 and label uint8, got {image.dtype} and {label.dtype}")
        if image.dim() != 3 or image.shape != label.shape or image.numel() == 0:
            raise ValueError(f"DeviceVolume: image and label are [D, H, W] of one shape, got {tuple(image.shape)} and "
                             f"{tuple(label.shape)}")
        if image.numel() >= 2 ** 31:
            raise ValueError("DeviceVolume: a volume holds fewer than 2^31 voxels")
        if num_classes is not None and not 1 <= int(num_classes) <= 256:
            raise ValueError(f"DeviceVolume: num_classes counts the ids of a uint8 label map (1 .. 256), got {num_classes}")
        if num_classes is not None and max(image.shape) > 2 ** 24:
            raise ValueError("DeviceVolume: label smoothing takes voxel indices in fp32: extents up to 2^24")
        device = torch.device(device)
        if device.type != "cuda":
            raise ValueError(f"DeviceVolume: a GPU device, not {device}")
        self.image = image.to(device).contiguous()
        self.label = label.to(device).contiguous()
        self.image_threshold = float(image_threshold)
        self.prefix = ops.aug_count_candidates(self.image, self.label, self.image_threshold)
        self.num_classes = None if num_classes is None else int(num_classes)
        self.centroids = self.class_counts = self.class_sums = None
        self.class_prefix = self.class_candidate_counts = self._class_candidate_totals = None
        totals = self.prefix[:, -1].to(torch.int64)
        if self.num_classes is not None:
            sums, self.centroids = ops.aug_class_centroids(self.label, self.num_classes)
            self.class_counts, self.class_sums = sums[:self.num_classes, 0], sums[:self.num_classes, 1:]
            totals = torch.cat([totals, sums[self.num_classes, :1]])
        totals = totals.tolist()                              # the one host read, at construction
        self.fg_count, self.bg_count = int(totals[0]), int(totals[1])
        if self.num_classes is not None and totals[2] != 0:
            raise ValueError(f"DeviceVolume: {totals[2]} voxels of the label map hold an id >= num_classes = {self.num_classes}")
        if self.fg_count == 0 and self.bg_count == 0:
            raise ValueError("DeviceVolume: no crop centre: the label map has no foreground and no voxel of the image is above "
                             f"image_threshold = {self.image_threshold}")

    @classmethod
    def from_hu(cls, image_hu, label, a_min=-175.0, a_max=250.0, image_threshold=0.0, device="cuda", num_classes=None):
        """ScaleIntensityRanged(a_min, a_max, b_min=0, b_max=1, clip=True) of the reference's deterministic transforms, applied
        once with torch operators, then ``DeviceVolume``."""
        x = torch.as_tensor(image_hu).to(device=device, dtype=torch.float32)
        x = ((x - a_min) / (a_max - a_min)).clamp_(0.0, 1.0)
        return cls(x, label, image_threshold=image_threshold, device=device, num_classes=num_classes)

    @classmethod
    def from_raw(cls, image, label, affine, pixdim=(1.5, 1.5, 2.0), axcodes="RAS", a_min=-175.0, a_max=250.0, image_threshold=0.0,
                 device="cuda", num_classes=None):
        """The whole deterministic front of the reference's transforms (utils.py:125-136: window, foreground crop, orientation,
        spacing) on the device -- ``prepare.prepare_case`` on a scan as a reader hands it over (int16 or fp32 ``image``, uint8
        ``label``, 4x4 ``affine``) -- then ``DeviceVolume``.  The ``PreparedCase`` (prepared affine, ``restore``) is kept as
        ``volume.prepared``."""
        from . import prepare
        if label is None:
            raise ValueError("DeviceVolume.from_raw: label is required (prepare.prepare_case prepares an image on its own)")
        case = prepare.prepare_case(image, label, affine=affine, pixdim=pixdim, axcodes=axcodes, a_min=a_min, a_max=a_max,
                                    device=device)
        volume = cls(case.image, case.label, image_threshold=image_threshold, device=device, num_classes=num_classes)
        volume.prepared = case
        return volume

    @property
    def shape(self):
        return tuple(self.image.shape)

    @property
    def device(self):
        return self.image.device

    def class_candidates(self):
        """The candidate sets per class for class-balanced crop centres (class 0 = label == 0 and image > image_threshold,
        class k = label == k), counted once, on first use: ``class_prefix`` int32 [num_classes, nchunks + 1], the per-chunk
        exclusive prefix table of every class, which is returned, and ``class_candidate_counts`` int64 [num_classes], both on the
        device.  Reads the counts once (a host synchronisation at that point)."""
        if self.class_prefix is None:
            if self.num_classes is None:
                raise ValueError("DeviceVolume.class_candidates: the volume was built without num_classes")
            if self.num_classes > nv.AUG_MAX_CLASSES:
                raise ValueError(f"DeviceVolume.class_candidates: at most {nv.AUG_MAX_CLASSES} classes, the volume has num_classes = "
                                 f"{self.num_classes}")
            prefix = ops.aug_count_class_candidates(self.image, self.label, self.num_classes, self.image_threshold)
            counts = prefix[:, -1].to(torch.int64)
            self._class_candidate_totals = counts.tolist()    # the one host read
            self.class_prefix, self.class_candidate_counts = prefix, counts
        return self.class_prefix

    def table_row(self):
        D, H, W = self.shape
        n = self.prefix.shape[1]
        return nv.AugVolume(self.image.data_ptr(), self.label.data_ptr(), self.prefix.data_ptr(), self.prefix.data_ptr() + 4 * n,
                            D, H, W, n - 1, self.fg_count, self.bg_count, self.image_threshold, 0)


class DeviceBatchProducer:
    """Random patches of ``volumes`` as training batches: ``next(volume_ids)`` returns ``images`` fp32 [B, 1, *roi] and
    ``labels`` fp32 [B, len(class_ids), *roi] (one-hot of ``class_ids``), NCDHW contiguous, in two launches with no host read.
    Deterministic for a given (seed, call counter, volume_ids); the call counter is a 64-bit device word the draw launch
    itself advances, so a captured ``next`` produces a new batch on every replay.

    ``smoothing`` (a ``LabelSmoothing``) makes ``labels`` the centroid-distance smoothed channels of ``class_ids`` instead of
    the one-hot ones: same launches, same ``params``, and ``apply`` of a logged row reproduces the smoothed batch.  Every volume
    then needs ``num_classes`` (one value for all).  ``class_ids=range(1, K)`` gives the channels the reference trains on
    (``labels[:, 1:]``, engine.py:159-160).  Crop centres come from the hard label map either way.

    ``rotate_prob`` / ``zoom_prob`` above 0 turn on the augmentations that resample, about the centre of the cropped window and
    on voxel indices (not millimetres), before the flips and the 90-degree rotation: with probability ``rotate_prob`` a rotation
    about each axis d, h, w by an angle within ``+-rotate_range[axis]`` (radians, each in [0, pi / 2]); with probability
    ``zoom_prob`` a zoom drawn uniformly from ``zoom_range = (min, max)`` (above 1 magnifies).  The image is interpolated
    trilinearly, the label map taken at the nearest voxel (class 0 outside the volume), and a voxel outside the volume holds
    ``pad_value`` (0 is air after the intensity window).  The rotation is drawn as the tangent of half its angle, uniformly, so
    that the matrix needs no sine or cosine and is reproducible bit for bit: the angle is therefore not uniform, its density
    rises by tan(angle / 2)^2 towards the ends of the range (7 % at +-30 degrees).  Then ``draw`` returns ``(params, affine)``
    (``split_affine`` names the columns of the second), ``apply`` takes both, and a logged pair replays its batch.  With both
    probabilities 0 (the default) nothing changes: the same launches, the same objects, the same bits.

    ``intensity`` (an ``IntensityAugmenter`` of the producer's roi and device) makes ``next`` run it, in place, on the images
    ``apply`` wrote; the rows of that call stay in ``producer.intensity_rows`` for logging.  ``draw`` and ``apply`` of the producer
    do not change, and ``None`` (the default) changes nothing.

    ``class_ratios`` draws the crop centre by class instead of by ``pos`` / ``neg`` (which must then keep their defaults): a
    sequence of ``num_classes`` non-negative numbers, MONAI's ``ratios`` -- class k is chosen with a probability proportional to
    ``class_ratios[k]`` among the classes that occur in the volume (class 0 = background above ``image_threshold``), then a voxel
    of it uniformly -- or the string ``"present"`` for ``(0, 1, .., 1)``, nnU-Net's uniform choice among the foreground classes
    of the case.  Every volume needs one ``num_classes`` (at most 64); a volume in which no class with a positive ratio occurs
    is refused.  ``uniform_prob`` is the probability that the centre is instead any voxel of the volume (nnU-Net: 0.67; works
    without ``class_ratios`` too).  Same two launches; ``draw`` returns what it returns otherwise and a row is an ordinary row.
    ``chosen_classes`` (int32 [B], device) holds the classes of the last draw, -1 for a uniform centre; ``class_tally`` (int64
    [num_classes + 1], device, the last entry the uniform centres) counts every draw since ``reset_class_tally()``; the producer
    reads neither.  ``chosen_classes`` is allocated by the first draw of a batch size: draw once before capturing ``next``.  With
    ``class_ratios=None, uniform_prob=0`` (the default) nothing changes: the same launch, the same objects, the same bits."""

    def __init__(self, volumes, roi=(96, 96, 96), class_ids=range(16), pos=1, neg=1, flip_prob=0.1, rot90_prob=0.1, max_k=3,
                 scale_prob=0.1, scale_factors=0.1, shift_prob=0.5, shift_offsets=0.1, seed=0, smoothing=None, rotate_prob=0.0,
                 rotate_range=(0.0, 0.0, 0.0), zoom_prob=0.0, zoom_range=(1.0, 1.0), pad_value=0.0, intensity=None,
                 class_ratios=None, uniform_prob=0.0):
        volumes = list(volumes)
        if not volumes or not all(isinstance(v, DeviceVolume) for v in volumes):
            raise ValueError("DeviceBatchProducer: a non-empty list of DeviceVolume")
        self.device = volumes[0].device
        if any(v.device != self.device for v in volumes):
            raise ValueError("DeviceBatchProducer: every volume on one device")
        roi = tuple(int(r) for r in roi)
        if len(roi) != 3 or min(roi) < 1:
            raise ValueError(f"DeviceBatchProducer: roi is three positive extents, got {roi}")
        for i, v in enumerate(volumes):
            if any(s < r for s, r in zip(v.shape, roi)):
                raise ValueError(f"DeviceBatchProducer: volume {i} of shape {v.shape} is smaller than roi {roi}")
        class_ids = [int(c) for c in class_ids]
        if not 1 <= len(class_ids) <= nv.AUG_MAX_CLASSES:
            raise ValueError(f"DeviceBatchProducer: 1 .. {nv.AUG_MAX_CLASSES} class ids, got {len(class_ids)}")
        if any(c < 0 or c > 255 for c in class_ids):
            raise ValueError("DeviceBatchProducer: class ids are values of a uint8 label map (0 .. 255)")
        probs = dict(flip_prob=flip_prob, rot90_prob=rot90_prob, scale_prob=scale_prob, shift_prob=shift_prob,
                     rotate_prob=rotate_prob, zoom_prob=zoom_prob)
        for name, p in probs.items():
            if not 0.0 <= float(p) <= 1.0:
                raise ValueError(f"DeviceBatchProducer: {name} is a probability, got {p}")
        if float(pos) < 0 or float(neg) < 0 or float(pos) + float(neg) <= 0:
            raise ValueError("DeviceBatchProducer: pos and neg are non-negative and not both zero")
        if float(scale_factors) < 0 or float(shift_offsets) < 0:
            raise ValueError("DeviceBatchProducer: scale_factors and shift_offsets are non-negative half-widths")
        if int(max_k) not in (1, 2, 3):
            raise ValueError(f"DeviceBatchProducer: max_k is 1, 2 or 3, got {max_k}")
        if float(rot90_prob) > 0 and roi[0] != roi[1]:
            raise ValueError(f"DeviceBatchProducer: the rotation is in the plane of the first two axes and needs roi[0] == roi[1] "
                             f"(roi = {roi}); pass rot90_prob=0")
        try:
            rotate_range = tuple(float(r) for r in rotate_range)
            zoom_range = tuple(float(z) for z in zoom_range)
            pad_value = float(pad_value)
        except (TypeError, ValueError):
            raise ValueError("DeviceBatchProducer: rotate_range is three angles, zoom_range two factors, pad_value a number") from None
        if len(rotate_range) != 3 or not all(0.0 <= r <= math.pi / 2 for r in rotate_range):
            raise ValueError(f"DeviceBatchProducer: rotate_range is three angles in radians, each in [0, pi / 2], got {rotate_range}")
        if len(zoom_range) != 2 or not (0.0 < zoom_range[0] <= zoom_range[1] and math.isfinite(zoom_range[1])):
            raise ValueError(f"DeviceBatchProducer: zoom_range is (min, max) with 0 < min <= max, finite, got {zoom_range}")
        if not math.isfinite(pad_value) or abs(pad_value) > 3.0e38:
            raise ValueError(f"DeviceBatchProducer: pad_value is a finite fp32 number, got {pad_value}")
        self.affine = float(rotate_prob) > 0 or float(zoom_prob) > 0
        if self.affine and max(max(v.shape) for v in volumes) > 2 ** 22:
            raise ValueError("DeviceBatchProducer: rotation and zoom take voxel indices in fp32: extents up to 2^22")
        # tan(angle / 2) in fp64, rounded once (at most 1 for pi / 2); fp32(max - min) likewise
        self.affine_cfg = nv.AugAffineConfig(float(rotate_prob), (C.c_float * 3)(*[min(math.tan(r / 2), 1.0) for r in rotate_range]),
                                             float(zoom_prob), zoom_range[0], zoom_range[1] - zoom_range[0], pad_value, 0)
        if smoothing is not None:
            if not isinstance(smoothing, LabelSmoothing):
                raise ValueError("DeviceBatchProducer: smoothing is a LabelSmoothing or None")
            missing = [i for i, v in enumerate(volumes) if v.centroids is None]
            if missing:
                raise ValueError(f"DeviceBatchProducer: smoothing needs class centroids, volumes {missing} were built without "
                                 "num_classes")
            if len({v.num_classes for v in volumes}) != 1:
                raise ValueError("DeviceBatchProducer: smoothing needs one num_classes for every volume, got "
                                 f"{sorted({v.num_classes for v in volumes})}")
            if max(class_ids) >= volumes[0].num_classes:
                raise ValueError(f"DeviceBatchProducer: class id {max(class_ids)} has no centroid (num_classes = "
                                 f"{volumes[0].num_classes})")
        if intensity is not None:
            if not isinstance(intensity, IntensityAugmenter):
                raise ValueError("DeviceBatchProducer: intensity is an IntensityAugmenter or None")
            same_device = intensity.device.type == self.device.type and intensity.device.index in (None, self.device.index)
            if intensity.roi != roi or not same_device:
                raise ValueError(f"DeviceBatchProducer: intensity was built for roi {intensity.roi} on {intensity.device}, the "
                                 f"producer has roi {roi} on {self.device}")
        try:
            uniform_prob = float(uniform_prob)
        except (TypeError, ValueError):
            uniform_prob = math.nan
        if not 0.0 <= uniform_prob <= 1.0:
            raise ValueError(f"DeviceBatchProducer: uniform_prob is a probability, got {uniform_prob}")
        self.uniform_prob = uniform_prob
        self.class_ratios = self.class_cum = self.class_draw_table = self.chosen_classes = self.class_tally = None
        if class_ratios is not None:
            if float(pos) != 1.0 or float(neg) != 1.0:
                raise ValueError("DeviceBatchProducer: class_ratios replaces the pos / neg rule: leave pos and neg at their defaults, "
                                 f"got pos = {pos}, neg = {neg}")
            missing = [i for i, v in enumerate(volumes) if v.num_classes is None]
            if missing:
                raise ValueError(f"DeviceBatchProducer: class_ratios needs num_classes, volumes {missing} were built without it")
            if len({v.num_classes for v in volumes}) != 1:
                raise ValueError("DeviceBatchProducer: class_ratios needs one num_classes for every volume, got "
                                 f"{sorted({v.num_classes for v in volumes})}")
            K = volumes[0].num_classes
            if K > nv.AUG_MAX_CLASSES:
                raise ValueError(f"DeviceBatchProducer: class_ratios takes at most {nv.AUG_MAX_CLASSES} classes, the volumes have {K}")
            if isinstance(class_ratios, str):
                if class_ratios != "present":
                    raise ValueError(f"DeviceBatchProducer: class_ratios is a sequence of numbers or \"present\", got {class_ratios!r}")
                ratios = [0.0] + [1.0] * (K - 1)
            else:
                try:
                    ratios = [float(r) for r in class_ratios]
                except (TypeError, ValueError):
                    raise ValueError("DeviceBatchProducer: class_ratios is a sequence of numbers or \"present\"") from None
            if len(ratios) != K:
                raise ValueError(f"DeviceBatchProducer: class_ratios has one entry per class: {K} for num_classes = {K}, got {len(ratios)}")
            if not all(math.isfinite(r) and r >= 0.0 for r in ratios) or not math.isfinite(sum(ratios)):
                raise ValueError(f"DeviceBatchProducer: class_ratios are non-negative and finite (and so is their sum), got {ratios}")
            cums = []
            for i, v in enumerate(volumes):
                v.class_candidates()
                cum = class_cum(ratios, v._class_candidate_totals)
                if cum is None:
                    raise ValueError(f"DeviceBatchProducer: volume {i} holds no voxel of a class with a positive ratio (class_ratios = "
                                     f"{ratios}, candidates per class = {v._class_candidate_totals})")
                cums.append(cum)
            self.class_ratios = tuple(ratios)
        self.intensity, self.intensity_rows = intensity, None
        self.smoothing = smoothing
        self.volumes, self.roi, self.class_ids, self.seed = volumes, roi, tuple(class_ids), int(seed)
        self.cfg = nv.AugConfig((C.c_int * 3)(*roi), int(max_k), float(pos) / (float(pos) + float(neg)), float(flip_prob),
                                float(rot90_prob), float(scale_prob), float(scale_factors), float(shift_prob),
                                float(shift_offsets), 0)
        rows = (nv.AugVolume * len(volumes))(*[v.table_row() for v in volumes])
        self.table = torch.frombuffer(bytearray(bytes(rows)), dtype=torch.uint8).reshape(len(volumes), -1).to(self.device)
        self.class_table = torch.tensor(class_ids, dtype=torch.uint8).to(self.device)
        self._counter = torch.zeros(1, dtype=torch.int64, device=self.device)
        self._status = torch.zeros(1, dtype=torch.int32, device=self.device)
        if self.class_ratios is not None:
            self.class_cum = torch.tensor(cums, dtype=torch.float64).to(torch.float32).to(self.device)     # fp32 [volumes, K]: rounded once
            K = len(self.class_ratios)
            crows = (nv.AugClassVolume * len(volumes))(*[nv.AugClassVolume(v.class_prefix.data_ptr(), self.class_cum.data_ptr() + 4 * K * i)
                                                          for i, v in enumerate(volumes)])
            self.class_draw_table = torch.frombuffer(bytearray(bytes(crows)), dtype=torch.uint8).reshape(len(volumes), -1).to(self.device)
            self.class_tally = torch.zeros(K + 1, dtype=torch.int64, device=self.device)
        if smoothing is not None:
            self.centroids = torch.stack([v.centroids for v in volumes]).contiguous()       # fp32 [volumes, num_classes, 3]
            self._smoothing = smoothing.native()

    @property
    def counter(self):
        """The call counter the next ``draw`` will use (reads the device word: a host synchronisation)."""
        return int(self._counter.item()) & (2 ** 64 - 1)

    @property
    def status(self):
        """Non-zero once any launch met a row it had to skip: a volume id outside the table, or a params row that would read
        outside its volume (reads the device word: a host synchronisation)."""
        return int(self._status.item())

    def reset_class_tally(self):
        """Zero ``class_tally`` (a producer with ``class_ratios``)."""
        if self.class_tally is None:
            raise ValueError("DeviceBatchProducer.reset_class_tally: the producer was built without class_ratios")
        self.class_tally.zero_()

    def _ids(self, volume_ids):
        if torch.is_tensor(volume_ids):
            if not volume_ids.is_cuda:
                volume_ids = volume_ids.tolist()
            else:
                assert volume_ids.dtype == torch.int32 and volume_ids.dim() == 1 and volume_ids.numel() >= 1 and \
                    volume_ids.device == self.device and volume_ids.is_contiguous(), \
                    "volume_ids: a host sequence, or a contiguous int32 [B] tensor on the producer's device"
                return volume_ids
        ids = [int(i) for i in volume_ids]
        if not ids or any(i < 0 or i >= len(self.volumes) for i in ids):
            raise ValueError(f"volume_ids: at least one id, each in [0, {len(self.volumes)})")
        return torch.tensor(ids, dtype=torch.int32).to(self.device)

    def draw(self, volume_ids, counter=None):
        """The random decisions of one batch as ``params`` (int32 [B, 8] on the device; ``split_params`` names the columns).
        ``counter=None`` uses and advances the producer's device-resident call counter; an integer is used for this call only.
        A producer with rotation or zoom returns ``(params, affine)``: the same ``params`` and fp32 [B, 16] rows that
        ``split_affine`` names."""
        ids = self._ids(volume_ids)
        params = torch.empty((ids.numel(), nv.AUG_PARAM_WORDS), dtype=torch.int32, device=self.device)
        affine = torch.empty((ids.numel(), nv.AUG_AFFINE_WORDS), dtype=torch.float32, device=self.device) if self.affine else None
        if self.class_ratios is not None or self.uniform_prob > 0.0:
            K = len(self.class_ratios) if self.class_ratios is not None else 0
            if K and (self.chosen_classes is None or self.chosen_classes.numel() != ids.numel()):
                self.chosen_classes = torch.empty(ids.numel(), dtype=torch.int32, device=self.device)
            with torch.cuda.device(self.device):
                return ops.aug_draw_classes(self.table, ids, self.cfg, self.seed, self._counter, params, self._status,
                                            counter_value=counter, affine_cfg=self.affine_cfg if self.affine else None, affine=affine,
                                            class_table=self.class_draw_table, num_classes=K, uniform_prob=self.uniform_prob,
                                            chosen=self.chosen_classes if K else None, tally=self.class_tally)
        with torch.cuda.device(self.device):
            return ops.aug_draw(self.table, ids, self.cfg, self.seed, self._counter, params, self._status, counter_value=counter,
                                affine_cfg=self.affine_cfg if self.affine else None, affine=affine)

    def apply(self, params, out_images=None, out_labels=None, affine=None):
        """The batch ``params`` describes: (images fp32 [B, 1, *roi], labels fp32 [B, len(class_ids), *roi]); the labels are
        one-hot, or smoothed when the producer was built with ``smoothing``.  A producer with rotation or zoom needs the
        ``affine`` rows of the same ``draw``; any producer resamples through rows it is given."""
        assert torch.is_tensor(params) and params.is_cuda and params.device == self.device, "params: a tensor on the producer's device"
        if self.affine and affine is None:
            raise ValueError("DeviceBatchProducer.apply: this producer rotates or zooms: pass the affine rows of draw() as affine=")
        B = params.shape[0]
        if out_images is None:
            out_images = torch.empty((B, 1) + self.roi, dtype=torch.float32, device=self.device)
        if out_labels is None:
            out_labels = torch.empty((B, len(self.class_ids)) + self.roi, dtype=torch.float32, device=self.device)
        assert affine is None or (torch.is_tensor(affine) and affine.is_cuda and affine.device == self.device), \
            "affine: a tensor on the producer's device"
        centroids, smoothing = (self.centroids, self._smoothing) if self.smoothing is not None else (None, None)
        with torch.cuda.device(self.device):
            return ops.aug_apply(self.table, params, self.roi, self.class_table, out_images, out_labels, self._status,
                                 affine=affine, centroids=centroids, smoothing=smoothing)

    def next(self, volume_ids, out_images=None, out_labels=None):
        drawn = self.draw(volume_ids)
        params, affine = drawn if self.affine else (drawn, None)
        images, labels = self.apply(params, out_images, out_labels, affine=affine)
        if self.intensity is not None:
            self.intensity_rows = self.intensity.draw(images.shape[0])
            self.intensity.apply(images, self.intensity_rows, out=images)
        return images, labels
