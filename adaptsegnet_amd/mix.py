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

tests/classmix_ref.py restates the rules in numpy; tests/test_classmix_gpu.py compares bit for bit.

Deliberate differences from DACS:

* ``q`` is per image, not per batch, so a sample's weights do not depend on its batch mates or on
  how a batch is sharded over ranks.  At batch 1 the two coincide.
* The loss's mean divides by the number of valid pixels, not by all pixels (``cross_entropy2d``'s
  ``mean_or_zero``, like every other CE term of the step).
* DACS's colour jitter and Gaussian blur of the mixed image are out of scope.
"""
from __future__ import annotations

import numpy as np
import torch

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


def _keys_tensor(keys, n, c, device):
    """The uint32 [n, c] keys as an int32 device tensor of the same bits (pinned staging: no sync)."""
    if isinstance(keys, np.ndarray):
        if keys.dtype != np.uint32 or keys.shape != (n, c):
            raise ValueError(f"classmix: keys are {keys.dtype} {keys.shape}, expected uint32 {(n, c)}")
        t = torch.from_numpy(np.ascontiguousarray(keys).view(np.int32))
        if torch.device(device).type == "cuda":
            t = t.pin_memory()
        return t.to(device, non_blocking=True)
    if keys.dtype not in (torch.int32, torch.uint32) or tuple(keys.shape) != (n, c):
        raise ValueError(f"classmix: keys are {keys.dtype} {tuple(keys.shape)}, expected uint32 / int32 {(n, c)}")
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
    keys = _keys_tensor(keys, n, c, dev)   # checked before anything is launched
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

    def mix(self, images, labels, images_t, sampler, num_classes=19, tau=0.968, ignore_label=255):
        """``predict`` on the target batch at the source batch's size, then ``classmix`` with ``sampler``'s keys:
        the ``(mixed_images, mixed_labels, mixed_weights)`` a ``lambda_mix > 0`` batch ends with."""
        n, _, h, w = images.shape
        pred, conf = self.predict(images_t, (w, h))
        return classmix(images, labels, images_t, pred, conf, sampler.sample(n, num_classes), num_classes, tau,
                        ignore_label)

    # -- checkpoints -----------------------------------------------------------------------------------
    def state_dict(self) -> dict:
        return {"alpha": self.alpha, "model": self.teacher.state_dict()}

    def load_state_dict(self, state: dict) -> None:
        _check_alpha(state["alpha"])
        self.alpha = float(state["alpha"])
        self.teacher.load_state_dict(state["model"])
