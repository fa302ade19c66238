"""Class-balanced pseudo-labels for self-training on the HIP engine (the CBST / BDL recipe).

The stage after adversarial adaptation: predict the target set, keep per class the most confident
``portion`` of its pixels (a per-class threshold, capped), and train on those labels beside the
adversarial loss (``StepConfig.lambda_st``, adaptsegnet_amd/train.py).  Everything stays on the
device: ``evaluate.predict_tta(..., return_confidence=True)`` gives a uint8 class map and the
winning class's fused probability, and three kernels (csrc/pseudo.hip, integer atomics only, so
every result is exact and order-independent) consume them:

* ``ConfidenceHistogram``: int64 [C, nbins] counts of the confidences per predicted class.  A pixel
  counts when ``pred < C`` and ``conf >= 0`` (a NaN or negative confidence does not);
  ``bin = nbins-1 if conf >= 1 else int(conf * nbins)`` in fp32, exact because nbins is a power of two.
* ``thresholds(portion, cap)``: per class with T pixels, ``K = ceil(portion * T)`` and b* the largest
  bin whose suffix sum reaches K; ``thr = min(b* / nbins, cap)``, or ``cap`` for an empty class
  (portion 0.5 and cap 0.9: BDL's rule at bin resolution).
* ``pseudo_labels``: int64 labels, ``pred`` where ``conf >= thr[pred]``, else ``ignore_label``.

Two passes over the target set: ``fit_thresholds`` (pass 1), then the caller's loop of
``predict_tta`` + ``pseudo_labels`` (pass 2).  tests/pseudo_ref.py restates the three rules in numpy;
tests/test_pseudo_gpu.py compares bit for bit.
"""
from __future__ import annotations

import torch
import torch.distributed as dist

from .evaluate import predict_tta
from .ops import OPS


class ConfidenceHistogram:
    """Device-side per-class histogram of prediction confidences, accumulated over ``update`` calls."""

    def __init__(self, num_classes=19, nbins=512, device="cuda"):
        self.n, self.nbins = int(num_classes), int(nbins)
        if not 1 <= self.n <= 256:
            raise ValueError(f"ConfidenceHistogram: num_classes {num_classes!r} (expected 1..256)")
        if not (2 <= self.nbins <= 4096 and self.nbins & (self.nbins - 1) == 0):
            raise ValueError(f"ConfidenceHistogram: nbins {nbins!r} (expected a power of two in 2..4096)")
        self.hist = torch.zeros((self.n, self.nbins), dtype=torch.int64, device=device)

    def update(self, pred: torch.Tensor, conf: torch.Tensor) -> None:
        """pred: uint8 class map(s); conf: fp32 confidence map(s) of the same number of pixels."""
        if pred.dtype != torch.uint8 or conf.dtype != torch.float32:
            raise RuntimeError("ConfidenceHistogram.update: uint8 predictions and float32 confidences expected")
        if pred.numel() != conf.numel():
            raise RuntimeError(f"ConfidenceHistogram.update: {pred.numel()} predictions vs {conf.numel()} confidences")
        OPS.conf_hist(pred.contiguous(), conf.contiguous(), self.n, self.nbins, self.hist)

    def thresholds(self, portion=0.5, cap=0.9) -> torch.Tensor:
        """float32 [C] device tensor of per-class thresholds (one launch, no host sync)."""
        _check_unit(portion, "portion")
        _check_unit(cap, "cap")
        thr = torch.empty(self.n, dtype=torch.float32, device=self.hist.device)
        OPS.pseudo_thresholds(self.hist, float(portion), float(cap), thr)
        return thr

    def reset(self) -> None:
        self.hist.zero_()

    def all_reduce(self, group=None) -> None:
        """SUM of the counts over the ranks (each rank histograms its shard of the target set)."""
        if dist.is_available() and dist.is_initialized():
            dist.all_reduce(self.hist, op=dist.ReduceOp.SUM, group=group)


def _check_unit(v, name):
    if not 0.0 < float(v) <= 1.0:
        raise ValueError(f"pseudo-label {name} {v!r} (expected 0 < {name} <= 1)")


def pseudo_labels(pred: torch.Tensor, conf: torch.Tensor, thresholds: torch.Tensor, ignore_label=255,
                  return_kept=False):
    """int64 labels of ``pred``'s shape: ``pred`` where the pixel is valid and ``conf >= thresholds[pred]``,
    else ``ignore_label`` (they feed ``cross_entropy2d`` and the step's ``labels_t`` as they are).
    ``return_kept``: also the int64 [C] number of pixels kept per class."""
    if pred.dtype != torch.uint8 or conf.dtype != torch.float32:
        raise RuntimeError("pseudo_labels: uint8 predictions and float32 confidences expected")
    if pred.numel() != conf.numel():
        raise RuntimeError(f"pseudo_labels: {pred.numel()} predictions vs {conf.numel()} confidences")
    if thresholds.dtype != torch.float32 or thresholds.dim() != 1 or not 1 <= thresholds.numel() <= 256:
        raise RuntimeError(f"pseudo_labels: thresholds are {thresholds.dtype} {tuple(thresholds.shape)}, "
                           "expected float32 [C], C <= 256")
    if not 0 <= int(ignore_label) <= 255:
        raise ValueError(f"pseudo_labels: ignore_label {ignore_label!r} (expected 0..255)")
    pred = pred.contiguous()
    labels = torch.empty(pred.shape, dtype=torch.int64, device=pred.device)
    kept = torch.zeros(thresholds.numel(), dtype=torch.int64, device=pred.device) if return_kept else None
    OPS.pseudo_label(pred, conf.contiguous(), thresholds.contiguous(), int(ignore_label), labels, kept)
    return (labels, kept) if return_kept else labels


def fit_thresholds(model, image_batches, scales=(1.0,), mirror=True, out_hw=(1024, 2048), portion=0.5, cap=0.9,
                   num_classes=19, nbins=512):
    """Pass 1 over a target set: ``predict_tta(..., return_confidence=True)`` and ``update`` per batch of
    ``image_batches`` (an iterable of [N, 3, H, W] device tensors).  Returns (thresholds, histogram);
    with several ranks, call ``histogram.all_reduce()`` and ``histogram.thresholds()`` afterwards."""
    hist = None
    for images in image_batches:
        if hist is None:
            hist = ConfidenceHistogram(num_classes, nbins, images.device)
        pred, conf = predict_tta(model, images, scales, mirror, out_hw, return_confidence=True)
        hist.update(pred, conf)
    if hist is None:
        raise ValueError("fit_thresholds: no image batches")
    return hist.thresholds(portion, cap), hist
