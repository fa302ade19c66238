"""Online self-training on the HIP engine: a mean teacher, ClassMix and a confidence-weighted CE (DACS).

The stage after offline pseudo-labels (adaptsegnet_amd/pseudo.py): an exponential moving average of
the generator (the teacher) labels every target batch as it arrives, half of the classes present in
a source image are pasted — image and label — onto the target image, and the student trains on the
mixed image with a cross entropy whose target pixels are down-weighted by the teacher's confidence
(``StepConfig.lambda_mix``, adaptsegnet_amd/train.py).  Everything stays on the device and nothing
returns to the host between the teacher's forward and the step:

* ``ema_update`` / ``EmaTeacher.update``: ``t = fmaf(a, t, (1 - a) * s)`` over the whole parameter
  arena in one launch and over the remaining float tensors (frozen BatchNorm affines, running
  statistics) a table of pointers at a time (csrc/mix.hip).
* ``classmix``: two launches.  Pass 1 counts, per image, the source pixels of every class and the
  target pixels whose confidence reaches ``tau`` (integer atomics: exact).  Pass 2 selects, in every
  block, the ``ceil(k / 2)`` of the k present classes with the smallest ``(key, class index)`` pairs
  — ``keys`` are the caller's uint32 random numbers, one per image and class (``ClassMixSampler``):
  a uniformly random half without ``torch.unique`` / ``randperm`` and their host syncs — and writes
  ``mixed_image = m ? source : target``, ``mixed_label = m ? source label : teacher's class`` and
  ``mixed_weight = m ? 1 : q``, where m = "the source pixel's label is a selected class" and
  ``q = nconf / (H * W)`` in fp32.
* ``functional.cross_entropy2d(..., pixel_weight=mixed_weights)`` is the loss.
* ``strong_augment`` / ``EmaTeacher.mix(..., augment=StrongAugSampler())``: DACS's colour jitter (brightness,
  contrast, saturation, hue in a random order) and Gaussian blur of the mixed images, each per image and
  optional, in one launch for the batch (csrc/strongaug.hip).  The host draws the parameters and the
  blur's half kernel; the device runs fp32 ``+ - * / floor``, compares and selects only.

* ``mask_patches`` / ``EmaTeacher.mask(images_t, PatchMaskSampler())``: Masked Image Consistency (MIC, Hoyer et
  al., CVPR 2023), the stage built on DACS.  The student sees the target image with random square patches set
  to 0 (the mean colour of this image space) and must reproduce the labels the teacher gave the WHOLE image,
  weighted by ``q`` (``StepConfig.lambda_mic``).  Two launches (csrc/mic.hip): ``conf_count``, ClassMix's
  ``nconf`` on its own (skipped when the caller passes ClassMix's), and ``patch_mask``: a patch is masked iff
  its uint32 key (``PatchMaskSampler``, one per patch) is below ``floor(ratio * 2^32)``, the labels are the
  teacher's classes and are not masked, the weights are ``q`` with ``ignore_top`` / ``ignore_bottom`` rows
  zeroed (DAFormer's ``pseudo_weight_ignore_top / bottom``: the rows still count in ``nconf`` and ``H * W``).

tests/classmix_ref.py, tests/strongaug_ref.py and tests/mic_ref.py restate the rules in numpy;
tests/test_classmix_gpu.py, tests/test_strongaug_gpu.py and tests/test_mic_gpu.py compare bit for bit.

Deliberate differences from DACS:

* ``q`` is per image, not per batch, so a sample's weights do not depend on its batch mates or on
  how a batch is sharded over ranks.  At batch 1 the two coincide.
* The loss's mean divides by the number of valid pixels, not by all pixels (``cross_entropy2d``'s
  ``mean_or_zero``, like every other CE term of the step).
* The jitter's and the blur's parameters are drawn per image, not per batch, for the same reason as ``q``.
* The blur has one radius, ``min(ceil(6 sigma), (ceil(0.1 min(H, W)) - 1) // 2)``: DACS's kernel-size rule
  applied to the shorter side where DACS sizes each axis on its own (the two coincide once both sides are
  >= 141), and trimmed to the taps that matter in fp32 (the mass beyond 6 sigma is below 2^-24 of the sum).

Deliberate differences from MIC's code:

* The patch grid has ``ceil(H / patch)`` x ``ceil(W / patch)`` cells and pixel (y, x) belongs to cell ``(y //
  patch, x // patch)``; MIC draws ``round(H / b)`` cells and stretches them with a nearest resize.  The two
  coincide when ``patch`` divides H and W.
* ``q`` is per image, not per batch, for the reason given above.
* The loss's mean is ``mean_or_zero`` over the valid pixels, like every other CE term of the step.
* The keys come from the host (PCG64, resumable), not from ``torch.rand`` on the device.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from ._lib import BLUR_MAX_RADIUS
from .data import IMG_MEAN
from .evaluate import predict_tta
from .ops import OPS


def ema_update(dst: torch.Tensor, src: torch.Tensor, alpha: float) -> torch.Tensor:
    """In place ``dst = fmaf(alpha, dst, (1 - alpha) * src)`` (float32, contiguous, one size), one launch.
    ``alpha == 0`` copies ``src`` bit for bit; ``alpha == 1`` leaves ``dst`` untouched."""
    _check_alpha(alpha)
    if dst.shape != src.shape:
        raise RuntimeError(f"ema_update: dst {tuple(dst.shape)} vs src {tuple(src.shape)}")
    OPS.ema(src, dst, float(alpha))
    return dst


def _check_alpha(alpha):
    if not 0.0 <= float(alpha) <= 1.0:
        raise ValueError(f"EMA alpha {alpha!r} (expected 0 <= alpha <= 1)")


def _keys_tensor(keys, shape, device, what="classmix"):
    """The uint32 keys of ``shape`` as an int32 device tensor of the same bits (pinned staging: no sync)."""
    if isinstance(keys, np.ndarray):
        if keys.dtype != np.uint32 or keys.shape != shape:
            raise ValueError(f"{what}: keys are {keys.dtype} {keys.shape}, expected uint32 {shape}")
        t = torch.from_numpy(np.ascontiguousarray(keys).view(np.int32))
        if torch.device(device).type == "cuda":
            t = t.pin_memory()
        return t.to(device, non_blocking=True)
    if not isinstance(keys, torch.Tensor) or keys.dtype not in (torch.int32, torch.uint32) \
            or tuple(keys.shape) != shape:
        got = f"{keys.dtype} {tuple(keys.shape)}" if isinstance(keys, torch.Tensor) else type(keys).__name__
        raise ValueError(f"{what}: keys are {got}, expected uint32 / int32 {shape}")
    return keys.contiguous().view(torch.int32).to(device)


def classmix(images_s, labels_s, images_t, pred_t, conf_t, keys, num_classes=19, tau=0.968, ignore_label=255,
             return_mask=False, return_stats=False):
    """ClassMix of a source batch onto a target batch of the same size.

    images_s, images_t: float32 [N, 3, H, W]; labels_s: int64 [N, H, W]; pred_t (uint8) and conf_t
    (float32) [N, H, W]: the teacher's class map and confidence (``EmaTeacher.predict``); keys: uint32
    [N, num_classes] (``ClassMixSampler.sample``).  Returns ``(mixed_images, mixed_labels,
    mixed_weights)`` — float32 [N, 3, H, W], int64 [N, H, W], float32 [N, H, W] — then, with
    ``return_mask``, the uint8 [N, num_classes] selection and, with ``return_stats``, the int32 ``count``
    [N, num_classes] and ``nconf`` [N] of pass 1.  Any memory layout is accepted (a non-contiguous
    input is copied first)."""
    c = int(num_classes)
    if not 1 <= c <= 256:
        raise ValueError(f"classmix: num_classes {num_classes!r} (expected 1..256)")
    if not 0 <= int(ignore_label) <= 255:
        raise ValueError(f"classmix: ignore_label {ignore_label!r} (expected 0..255)")
    if images_s.dim() != 4 or images_s.shape[1] != 3 or images_s.dtype != torch.float32:
        raise RuntimeError(f"classmix: images_s is {images_s.dtype} {tuple(images_s.shape)}, expected float32 "
                           "[N, 3, H, W]")
    n, _, h, w = images_s.shape
    if images_t.shape != images_s.shape:
        raise ValueError(f"classmix: target images {tuple(images_t.shape)} vs source images {tuple(images_s.shape)}: "
                         "ClassMix pastes pixel on pixel, the sizes must agree")
    if h * w >= 1 << 24:
        raise ValueError(f"classmix: {h} x {w} pixels per image (expected H * W < 2^24)")
    dev = images_s.device
    keys = _keys_tensor(keys, (n, c), dev)   # checked before anything is launched
    images_s, labels_s, images_t = images_s.contiguous(), labels_s.contiguous(), images_t.contiguous()
    pred_t, conf_t = pred_t.contiguous(), conf_t.contiguous()
    count = torch.empty((n, c), dtype=torch.int32, device=dev)
    nconf = torch.empty((n,), dtype=torch.int32, device=dev)
    OPS.classmix_stats(labels_s, conf_t, float(tau), c, count, nconf)
    mixed_images = torch.empty_like(images_s)
    mixed_labels = torch.empty((n, h, w), dtype=torch.int64, device=dev)
    mixed_weights = torch.empty((n, h, w), dtype=torch.float32, device=dev)
    mask = torch.empty((n, c), dtype=torch.uint8, device=dev) if return_mask else None
    OPS.classmix_apply(images_s, labels_s, images_t, pred_t, count, nconf, keys, int(ignore_label), mixed_images,
                       mixed_labels, mixed_weights, mask)
    out = (mixed_images, mixed_labels, mixed_weights)
    if return_mask:
        out += (mask,)
    if return_stats:
        out += (count, nconf)
    return out


class ClassMixSampler:
    """Draws ClassMix's per-image, per-class uint32 keys on the host.

    numpy's PCG64 seeded from (seed, rank), like ``data.AugmentSampler``: every rank draws its own
    reproducible sequence, and ``get_state`` / ``set_state`` let a resumed run continue it."""

    def __init__(self, seed=1234, rank=0):
        self.rng = np.random.Generator(np.random.PCG64(np.random.SeedSequence([int(seed), int(rank)])))

    def sample(self, n: int, num_classes: int = 19) -> np.ndarray:
        return self.rng.integers(0, 1 << 32, size=(int(n), int(num_classes)), dtype=np.uint32)

    def get_state(self) -> dict:
        return self.rng.bit_generator.state

    def set_state(self, state: dict) -> None:
        self.rng.bit_generator.state = state


def blur_radius(sigma: float, h: int, w: int) -> int:
    """``min(ceil(6 sigma), (ceil(0.1 min(h, w)) - 1) // 2)``: the taps that matter in fp32, under DACS's
    kernel-size rule on the shorter side (0.1 of it, made odd downwards)."""
    side = min(int(h), int(w))
    return max(0, min(math.ceil(6.0 * float(sigma)), (math.ceil(0.1 * side) - 1) // 2))


def blur_weights(sigma: float, radius: int) -> np.ndarray:
    """The half kernel w[0..7] (float32, zero beyond ``radius``) of a Gaussian over d = -R..R: ``exp(-d^2 / 2
    sigma^2)`` normalised in fp64, then rounded.  w[d] serves both d and -d: symmetric by construction."""
    d = np.arange(0, int(radius) + 1, dtype=np.float64)
    g = np.exp(-(d * d) / (2.0 * float(sigma) * float(sigma)))
    total = g[0] + 2.0 * g[1:].sum()
    out = np.zeros(BLUR_MAX_RADIUS + 1, dtype=np.float32)
    out[:int(radius) + 1] = (g / total).astype(np.float32)
    return out


AUG_OPS = ("brightness", "contrast", "saturation", "hue")   # the op codes 0..3 of ``params["order"]``
_PERMS = None


def _perms():
    global _PERMS
    if _PERMS is None:
        import itertools
        _PERMS = np.array(list(itertools.permutations(range(4))), dtype=np.uint8)
    return _PERMS


class StrongAugSampler:
    """Draws ``strong_augment``'s per-image parameters on the host.

    numpy's PCG64 seeded from (seed, rank), like ``ClassMixSampler``; ``get_state`` / ``set_state`` let a
    resumed run continue the sequence.  Every image takes eight variates whatever they decide (two
    on/off draws, four jitter factors, the order, sigma), so the stream's position after ``sample``
    depends on ``n`` alone."""

    def __init__(self, seed=1234, rank=0, strength=0.2, p_jitter=0.8, p_blur=0.5, sigma=(0.15, 1.15)):
        if not 0.0 <= float(strength) < 1.0:
            raise ValueError(f"StrongAugSampler: strength {strength!r} (expected 0 <= strength < 1)")
        for name, p in (("p_jitter", p_jitter), ("p_blur", p_blur)):
            if not 0.0 <= float(p) <= 1.0:
                raise ValueError(f"StrongAugSampler: {name} {p!r} (expected 0 <= p <= 1)")
        lo, hi = float(sigma[0]), float(sigma[1])
        if not 0.0 < lo <= hi:
            raise ValueError(f"StrongAugSampler: sigma {sigma!r} (expected 0 < low <= high)")
        self.strength, self.p_jitter, self.p_blur, self.sigma = float(strength), float(p_jitter), float(p_blur), (lo, hi)
        self.rng = np.random.Generator(np.random.PCG64(np.random.SeedSequence([int(seed), int(rank)])))

    def sample(self, n: int, h: int, w: int) -> dict:
        """The parameters of ``n`` images of ``h`` x ``w`` pixels: ``jitter`` bool [n]; ``db``, ``fc``, ``fs``,
        ``fh`` float32 [n] (``db``, ``fc - 1``, ``fs - 1`` and ``fh`` uniform in [-strength, strength]);
        ``order`` uint8 [n, 4], a permutation of the op codes (``AUG_OPS``); ``sigma`` float64 [n]; ``radius``
        int32 [n] (0: no blur); ``weights`` float32 [n, 8], the half kernels (``blur_weights``)."""
        n = int(n)
        u = self.rng.random((n, 8))   # a fixed number of variates per image
        s = self.strength
        jit = (2.0 * u[:, 2:6] - 1.0) * s
        sigma = self.sigma[0] + u[:, 7] * (self.sigma[1] - self.sigma[0])
        blur = u[:, 1] < self.p_blur
        radius = np.array([blur_radius(sg, h, w) if on else 0 for sg, on in zip(sigma, blur)], dtype=np.int32)
        radius = np.minimum(radius, BLUR_MAX_RADIUS).astype(np.int32)
        weights = np.stack([blur_weights(sg, r) for sg, r in zip(sigma, radius)]) if n else np.zeros((0, 8), np.float32)
        order = _perms()[np.minimum((u[:, 6] * 24).astype(np.int64), 23)]
        return {"jitter": u[:, 0] < self.p_jitter,
                "db": jit[:, 0].astype(np.float32), "fc": (1.0 + jit[:, 1]).astype(np.float32),
                "fs": (1.0 + jit[:, 2]).astype(np.float32), "fh": jit[:, 3].astype(np.float32),
                "order": order, "sigma": sigma, "radius": radius, "weights": weights}

    def get_state(self) -> dict:
        return self.rng.bit_generator.state

    def set_state(self, state: dict) -> None:
        self.rng.bit_generator.state = state


def _aug_tables(params, n, h, w):
    """(host controls, 4 ints per image; the [16 n] float32 table ``OPS.strong_augment`` uploads), after checking
    everything the kernel indexes or branches with: what is wrong raises here, before any launch."""
    def col(key, dtype, shape):
        a = np.asarray(params[key])
        if a.shape != shape:
            raise ValueError(f"strong_augment: params[{key!r}] is {a.shape}, expected {shape}")
        return a.astype(dtype)
    on = col("jitter", np.int32, (n,)) != 0
    radius = col("radius", np.int64, (n,))
    order = col("order", np.int64, (n, 4))
    fac = np.stack([col(k, np.float32, (n,)) for k in ("db", "fc", "fs", "fh")], axis=1)
    weights = col("weights", np.float32, (n, BLUR_MAX_RADIUS + 1))
    cap = min(BLUR_MAX_RADIUS, min(h, w) - 1)
    if ((radius < 0) | (radius > cap)).any():
        raise ValueError(f"strong_augment: radius {radius.tolist()} on {h} x {w} images (expected 0 <= R <= "
                         f"min({BLUR_MAX_RADIUS}, min(H, W) - 1) = {cap})")
    if not (np.sort(order, axis=1) == np.arange(4)).all():
        raise ValueError(f"strong_augment: order {order.tolist()}: every row must be a permutation of 0..3")
    if not (np.isfinite(fac).all() and np.isfinite(weights).all()):
        raise ValueError("strong_augment: a jitter factor or a blur weight is not finite")
    if (weights * (np.arange(BLUR_MAX_RADIUS + 1) > radius[:, None])).any():
        raise ValueError("strong_augment: a blur weight beyond its image's radius is not zero")
    ctl = np.zeros((n, 4), dtype=np.int32)
    ctl[:, 0] = on
    ctl[:, 1] = (order << (2 * np.arange(4))).sum(axis=1)
    ctl[:, 2] = radius
    table = np.concatenate([ctl.view(np.float32).ravel(), fac.ravel(), weights.ravel()])
    return ctl.ravel().tolist(), table


def strong_augment(images: torch.Tensor, params: dict, mean=IMG_MEAN) -> torch.Tensor:
    """DACS's colour jitter, then Gaussian blur, per image of a float32 [N, 3, H, W] batch (BGR minus ``mean``, what
    ``classmix`` returns), in one launch.  ``params``: ``StrongAugSampler.sample(N, H, W)`` (or a dictionary of
    that form).  An image with its jitter off and radius 0 is copied bit for bit.  Any memory layout is accepted;
    the result is a new contiguous tensor.  The tables reach the device through pinned staging: no sync."""
    if images.dim() != 4 or images.shape[1] != 3 or images.dtype != torch.float32:
        raise RuntimeError(f"strong_augment: images is {images.dtype} {tuple(images.shape)}, expected float32 "
                           "[N, 3, H, W]")
    n, _, h, w = images.shape
    if n < 1 or h < 1 or w < 1 or h * w >= 1 << 24:
        raise ValueError(f"strong_augment: {n} images of {h} x {w} pixels (expected N, H, W >= 1, H * W < 2^24)")
    mean = [float(v) for v in np.asarray(mean, dtype=np.float32).reshape(-1)]
    if len(mean) != 3 or not all(math.isfinite(v) for v in mean):
        raise ValueError(f"strong_augment: mean {mean!r} (expected three finite floats, B G R)")
    ctl, table = _aug_tables(params, n, h, w)
    t = torch.from_numpy(table)
    if images.device.type == "cuda":
        t = t.pin_memory()
    t = t.to(images.device, non_blocking=True)
    images = images.contiguous()
    out = torch.empty_like(images)
    OPS.strong_augment(images, mean, ctl, t, out)
    return out


def mask_threshold(ratio: float) -> int:
    """``floor(ratio * 2^32)``, exact in fp64: a patch is masked iff its uint32 key is below it."""
    ratio = float(ratio)
    if not 0.0 <= ratio <= 1.0:
        raise ValueError(f"mask ratio {ratio!r} (expected 0 <= ratio <= 1)")
    return int(math.floor(ratio * 4294967296.0))


def _check_patch(patch):
    if isinstance(patch, bool) or int(patch) != patch or int(patch) < 1:
        raise ValueError(f"mask patch {patch!r} (expected an integer, at least 1)")
    return int(patch)


def mask_patches(images_t, pred_t, conf_t, keys, patch=64, ratio=0.7, num_classes=19, tau=0.968, ignore_label=255,
                 ignore_top=0, ignore_bottom=0, nconf=None):
    """MIC's masked target batch and the teacher's labels of the whole images.

    images_t: float32 [N, 3, H, W]; pred_t (uint8) and conf_t (float32) [N, H, W]: ``EmaTeacher.predict``; keys:
    uint32 [N, ceil(H / patch), ceil(W / patch)] (``PatchMaskSampler.sample``).  Returns ``(masked_images,
    masked_labels, masked_weights)`` — float32 [N, 3, H, W], int64 [N, H, W], float32 [N, H, W]: the images with
    every patch whose key is below ``floor(ratio * 2^32)`` set to 0 (the mean colour), the teacher's classes
    (``ignore_label`` from ``num_classes`` on; not masked), and ``q = nconf / (H * W)`` with the first
    ``ignore_top`` and the last ``ignore_bottom`` rows zeroed.  ``nconf``: int32 [N], the pixels with ``conf_t >=
    tau``, e.g. from ``classmix(..., return_stats=True)`` on the same teacher output and ``tau``; the count launch
    is then skipped (``conf_t`` and ``tau`` are not read).  Any memory layout is accepted (a non-contiguous
    input is copied first); what is wrong raises on the host, before any launch."""
    patch = _check_patch(patch)
    threshold = mask_threshold(ratio)
    c = int(num_classes)
    if not 1 <= c <= 256:
        raise ValueError(f"mask_patches: num_classes {num_classes!r} (expected 1..256)")
    if not 0 <= int(ignore_label) <= 255:
        raise ValueError(f"mask_patches: ignore_label {ignore_label!r} (expected 0..255)")
    top, bottom = int(ignore_top), int(ignore_bottom)
    if top < 0 or bottom < 0 or top != ignore_top or bottom != ignore_bottom:
        raise ValueError(f"mask_patches: ignore_top {ignore_top!r}, ignore_bottom {ignore_bottom!r} (expected "
                         "integers, at least 0)")
    if images_t.dim() != 4 or images_t.shape[1] != 3 or images_t.dtype != torch.float32:
        raise RuntimeError(f"mask_patches: images_t is {images_t.dtype} {tuple(images_t.shape)}, expected float32 "
                           "[N, 3, H, W]")
    n, _, h, w = images_t.shape
    if n < 1 or h < 1 or w < 1 or h * w >= 1 << 24 or n > 65535:
        raise ValueError(f"mask_patches: {n} images of {h} x {w} pixels (expected 1 <= N <= 65535, H, W >= 1, "
                         "H * W < 2^24)")
    if pred_t.dtype != torch.uint8 or tuple(pred_t.shape) != (n, h, w):
        raise ValueError(f"mask_patches: pred_t is {pred_t.dtype} {tuple(pred_t.shape)}, expected uint8 {(n, h, w)}")
    dev = images_t.device
    if nconf is None:
        if conf_t.dtype != torch.float32 or tuple(conf_t.shape) != (n, h, w):
            raise ValueError(f"mask_patches: conf_t is {conf_t.dtype} {tuple(conf_t.shape)}, expected float32 "
                             f"{(n, h, w)}")
    elif not isinstance(nconf, torch.Tensor) or nconf.dtype != torch.int32 or tuple(nconf.shape) != (n,) \
            or nconf.device != dev:
        got = f"{nconf.dtype} {tuple(nconf.shape)} on {nconf.device}" if isinstance(nconf, torch.Tensor) \
            else type(nconf).__name__
        raise ValueError(f"mask_patches: nconf is {got}, expected int32 {(n,)} on {dev}")
    keys = _keys_tensor(keys, (n, -(-h // patch), -(-w // patch)), dev, "mask_patches")   # before any launch
    images_t, pred_t = images_t.contiguous(), pred_t.contiguous()
    if nconf is None:
        nconf = torch.empty((n,), dtype=torch.int32, device=dev)
        OPS.conf_count(conf_t.contiguous(), float(tau), nconf)
    masked_images = torch.empty_like(images_t)
    labels = torch.empty((n, h, w), dtype=torch.int64, device=dev)
    weights = torch.empty((n, h, w), dtype=torch.float32, device=dev)
    OPS.patch_mask(images_t, pred_t, nconf.contiguous(), keys, patch, threshold, c, int(ignore_label), top, bottom,
                   masked_images, labels, weights)
    return masked_images, labels, weights


class PatchMaskSampler:
    """Draws MIC's per-patch uint32 keys on the host: a patch is masked iff its key is below ``threshold`` =
    ``floor(ratio * 2^32)``, so every patch is masked with probability ``ratio`` on its own (MIC's ``rand >
    ratio`` on integers; 0 masks nothing, 1 everything).

    numpy's PCG64 seeded from (seed, rank), like ``ClassMixSampler``; ``get_state`` / ``set_state`` let a
    resumed run continue the sequence."""

    def __init__(self, seed=1234, rank=0, patch=64, ratio=0.7):
        self.patch = _check_patch(patch)
        self.threshold = mask_threshold(ratio)
        self.ratio = float(ratio)
        self.rng = np.random.Generator(np.random.PCG64(np.random.SeedSequence([int(seed), int(rank)])))

    def sample(self, n: int, h: int, w: int) -> np.ndarray:
        """uint32 [n, ceil(h / patch), ceil(w / patch)]: the keys of ``n`` images of ``h`` x ``w`` pixels."""
        n, h, w = int(n), int(h), int(w)
        if n < 0 or h < 1 or w < 1:
            raise ValueError(f"PatchMaskSampler: {n} images of {h} x {w} pixels")
        return self.rng.integers(0, 1 << 32, size=(n, -(-h // self.patch), -(-w // self.patch)), dtype=np.uint32)

    def get_state(self) -> dict:
        return self.rng.bit_generator.state

    def set_state(self, state: dict) -> None:
        self.rng.bit_generator.state = state


class EmaTeacher:
    """The mean teacher of a generator on the HIP engine.

    ``teacher_model``: a second instance of the generator's class, made by the caller; it is put in
    eval mode and its parameters stop requiring gradients.  ``update(model, i_iter)`` after every
    ``AdaptSegTrainer.step`` moves it towards the student with ``a = min(1 - 1 / (i_iter + 1), alpha)``
    (DACS's rule: at ``i_iter = 0`` a = 0 and the teacher becomes the student bit for bit): the
    parameter arena in one launch, the float tensors outside it (frozen BatchNorm affines, running
    statistics) through the multi-tensor kernel, ``num_batches_tracked`` copied.  The two arenas
    must have one layout (checked at the first update: ``ValueError``)."""

    def __init__(self, teacher_model, alpha=0.99):
        _check_alpha(alpha)
        if not hasattr(teacher_model, "_ensure_arena"):
            raise ValueError("EmaTeacher: the teacher must be a generator of this package (DeeplabMulti, DeeplabVGG)")
        self.teacher, self.alpha = teacher_model, float(alpha)
        teacher_model.eval()
        for p in teacher_model.parameters():
            p.requires_grad = False
        self._plan = None

    # -- layout -----------------------------------------------------------------------------------
    def _build_arena_like(self, model, device):
        """The teacher's arena with the student's layout: an arena holds the trainable parameters,
        so it is built under the student's requires_grad flags, which are then cleared again."""
        t = self.teacher
        flags = {k: p.requires_grad for k, p in model.named_parameters()}
        tp = dict(t.named_parameters())
        if set(tp) != set(flags):
            raise ValueError("EmaTeacher: teacher and student have different parameters: "
                             f"{sorted(set(tp) ^ set(flags))[:4]} ...")
        for k, p in tp.items():
            p.requires_grad = flags[k]
        t._arena_valid = False
        try:
            t._ensure_arena(device)
        finally:
            for p in tp.values():
                p.requires_grad = False

    def _layout(self, model):
        """(arena-less float pairs, integer pairs) of teacher / student tensors, after checking the arenas."""
        t = self.teacher
        dev = next(model.parameters()).device
        model._ensure_arena(dev)
        A = model.arena
        key = (id(model), id(A), id(t.arena) if getattr(t, "_arena_valid", False) else None)
        if self._plan is not None and self._plan[0] == key:
            return self._plan[1]
        if next(t.parameters()).device != dev:
            raise ValueError(f"EmaTeacher: the teacher is on {next(t.parameters()).device}, the student on {dev}")

        def same(B):
            return (B is not None and B.numel == A.numel and B.offsets == A.offsets
                    and [tuple(p.shape) for p in B.params] == [tuple(p.shape) for p in A.params])
        if not (getattr(t, "_arena_valid", False) and same(t.arena)):
            self._build_arena_like(model, dev)
        T = t.arena
        if not same(T):
            raise ValueError(f"EmaTeacher: the teacher's parameter arena ({T.numel} elements, {len(T.params)} "
                             f"parameters) does not have the student's layout ({A.numel} elements, {len(A.params)} "
                             "parameters): both must be instances of one generator class with one configuration")
        in_arena = {id(p) for p in T.params}
        sp, sb = dict(model.named_parameters()), dict(model.named_buffers())
        tb = dict(t.named_buffers())
        if set(tb) != set(sb):
            raise ValueError(f"EmaTeacher: teacher and student have different buffers: {sorted(set(tb) ^ set(sb))[:4]}")
        floats, ints = [], []
        for k, p in t.named_parameters():
            if id(p) not in in_arena:
                floats.append((p.data, sp[k].data))
        counter = (hasattr(t, "_bn_counter") and hasattr(model, "_bn_counter")
                   and t._bn_counter.shape == model._bn_counter.shape)
        if counter:   # DeeplabMulti keeps every num_batches_tracked in one tensor
            ints.append((t._bn_counter, model._bn_counter))
        for k, b in tb.items():
            if b.shape != sb[k].shape or b.dtype != sb[k].dtype:
                raise ValueError(f"EmaTeacher: buffer {k} is {b.dtype} {tuple(b.shape)} in the teacher, "
                                 f"{sb[k].dtype} {tuple(sb[k].shape)} in the student")
            if b.dtype == torch.float32:
                floats.append((b, sb[k]))
            elif not (counter and k.endswith("num_batches_tracked")):
                ints.append((b, sb[k]))
        for d, s in floats:
            if d.shape != s.shape or not (d.is_contiguous() and s.is_contiguous()):
                raise ValueError("EmaTeacher: a tensor outside the arena differs in shape or is not contiguous")
        plan = ([d for d, _ in floats], [s for _, s in floats], ints)
        self._plan = ((id(model), id(A), id(T)), plan)
        return plan

    # -- the update ---------------------------------------------------------------------------------
    def momentum(self, i_iter: int) -> float:
        return min(1.0 - 1.0 / (int(i_iter) + 1), self.alpha)

    @torch.no_grad()
    def update(self, model, i_iter: int) -> None:
        a = self.momentum(i_iter)
        dst, src, ints = self._layout(model)
        OPS.ema(model.arena.data, self.teacher.arena.data, a)
        if dst:
            OPS.ema_multi(src, dst, a)
        for d, s in ints:
            d.copy_(s)

    # -- the teacher's labels -------------------------------------------------------------------------
    @torch.no_grad()
    def predict(self, images_t: torch.Tensor, size):
        """(class map uint8, confidence float32), [N, H, W] at ``size`` = (W, H): one eval-mode forward of the
        teacher, upsampled, softmaxed and arg-maxed by one fused launch."""
        return predict_tta(self.teacher, images_t, (1.0,), False, (int(size[1]), int(size[0])),
                           return_confidence=True)

    def mix(self, images, labels, images_t, sampler, num_classes=19, tau=0.968, ignore_label=255, augment=None,
            mean=IMG_MEAN, teacher=None):
        """``predict`` on the target batch at the source batch's size, then ``classmix`` with ``sampler``'s keys:
        the ``(mixed_images, mixed_labels, mixed_weights)`` a ``lambda_mix > 0`` batch ends with.  ``augment``: a
        ``StrongAugSampler``; the mixed images then go through ``strong_augment`` with its next draw (labels and
        weights stay as they are).  ``mean``: what the images had subtracted (B, G, R), for the jitter.
        ``teacher``: a ``(pred, conf)`` pair that ``predict`` gave for these target images at this size, used
        instead of a forward of its own (one teacher forward shared with ``mask``)."""
        n, _, h, w = images.shape
        pred, conf = self.predict(images_t, (w, h)) if teacher is None else teacher
        out = classmix(images, labels, images_t, pred, conf, sampler.sample(n, num_classes), num_classes, tau,
                       ignore_label)
        if augment is None:
            return out
        return (strong_augment(out[0], augment.sample(n, h, w), mean),) + out[1:]

    def mask(self, images_t, sampler, num_classes=19, tau=0.968, ignore_label=255, augment=None, mean=IMG_MEAN,
             ignore_top=0, ignore_bottom=0, teacher=None):
        """``predict`` on the target batch at its own size, then ``mask_patches`` with ``sampler``'s (a
        ``PatchMaskSampler``'s) patch, ratio and next draw: the ``(masked_images, masked_labels, masked_weights)``
        a ``lambda_mic > 0`` batch ends with.  The teacher labels the whole images; only the student's copy is
        masked.  ``augment``: a ``StrongAugSampler``; the images go through ``strong_augment`` with its next draw
        BEFORE the masking (MIC's colour augmentation; the teacher sees the plain images).  ``teacher``: a
        ``(pred, conf)`` pair to use instead of the forward, as in ``mix``."""
        if not isinstance(sampler, PatchMaskSampler):
            raise ValueError(f"EmaTeacher.mask: sampler is {type(sampler).__name__}, expected a PatchMaskSampler")
        if images_t.dim() != 4:
            raise RuntimeError(f"EmaTeacher.mask: images_t is {tuple(images_t.shape)}, expected [N, 3, H, W]")
        n, _, h, w = images_t.shape
        pred, conf = self.predict(images_t, (w, h)) if teacher is None else teacher
        if augment is not None:
            images_t = strong_augment(images_t, augment.sample(n, h, w), mean)
        return mask_patches(images_t, pred, conf, sampler.sample(n, h, w), sampler.patch, sampler.ratio, num_classes,
                            tau, ignore_label, ignore_top, ignore_bottom)

    # -- checkpoints -----------------------------------------------------------------------------------
    def state_dict(self) -> dict:
        return {"alpha": self.alpha, "model": self.teacher.state_dict()}

    def load_state_dict(self, state: dict) -> None:
        _check_alpha(state["alpha"])
        self.alpha = float(state["alpha"])
        self.teacher.load_state_dict(state["model"])
