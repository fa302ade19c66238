"""Fourier Domain Adaptation (FDA, Yang & Soatto, CVPR 2020): low-frequency spectral style transfer.

FDA aligns the *inputs* of the two domains: the low-frequency amplitude spectrum of every source
image is replaced by a target image's, the phase stays, and the generator trains on the result.
With ``b = floor(min(H, W) * beta)`` only the ``(2b+1)^2`` coefficients with ``|u|, |v| <= b`` change, so
no full FFT runs: ``fda_source_to_target`` is a separable partial DFT of both images and a separable
synthesis added to the source (``csrc/fda.hip``), four launches, deterministic.

FDA's second part, the robust entropy term, is ``functional.entropy_loss2d(x, eta=...)`` and
``StepConfig.ent_eta``.  The call goes between ``preprocess`` and the step.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib
from .data import IMG_MEAN
from .ops import OPS

__all__ = ["fda_source_to_target", "fda_band", "twiddles"]

_TABLES: dict = {}   # (n, device) -> float32 [n, 2] of (cos, sin)(2 pi k / n)
_MEANS: dict = {}    # (mean values, device) -> float32 [C]


def fda_band(h: int, w: int, beta: float) -> int:
    """``b = floor(min(h, w) * beta)``, the half width of the swapped window (FDA's own rule)."""
    return int(math.floor(min(int(h), int(w)) * float(beta)))


def twiddles(n: int, device) -> torch.Tensor:
    """The table float32 [n, 2] of (cos, sin)(2 pi k / n) on ``device``: made in fp64, rounded to fp32, kept."""
    device = torch.device(device)
    key = (int(n), device.type, device.index)
    t = _TABLES.get(key)
    if t is None:
        ang = 2.0 * np.pi * np.arange(int(n), dtype=np.float64) / float(n)
        tab = np.stack([np.cos(ang), np.sin(ang)], axis=1).astype(np.float32)
        t = _TABLES[key] = torch.from_numpy(tab).to(device)
    return t


def _mean_tensor(mean, c: int, device, default: bool):
    if mean is None:
        return None
    vals = tuple(float(v) for v in np.asarray(mean, dtype=np.float32).reshape(-1))
    if len(vals) != c:
        hint = " (the default mean is the pipeline's B G R mean: pass mean=None or C values)" if default else ""
        raise ValueError(f"fda_source_to_target: mean has {len(vals)} values for {c} channels{hint}")
    if not all(math.isfinite(v) for v in vals):
        raise ValueError(f"fda_source_to_target: mean {vals!r} is not finite")
    key = (vals, device.type, device.index)
    t = _MEANS.get(key)
    if t is None:
        t = _MEANS[key] = torch.tensor(vals, dtype=torch.float32).to(device)
    return t


def fda_source_to_target(images_s: torch.Tensor, images_t: torch.Tensor, beta: float = 0.01,
                         mean=IMG_MEAN) -> torch.Tensor:
    """``images_s`` with the low-frequency amplitude spectrum of ``images_t``: image ``i`` of the source takes
    the style of image ``i`` of the target.  Both float32 ``[N, C, H, W]``, contiguous, one shape, one device
    (FDA resizes the two domains to one size first; that is the caller's job).

    The window is ``|u|, |v| <= b`` with ``b = floor(min(H, W) * beta)`` and needs ``2b + 1 <= min(H, W)``;
    ``b = 0`` swaps the DC amplitude only.  The semantics are the numpy formulation of FDA's code (window centred
    after ``fftshift``, real part of ``ifft2``).  ``mean``: the pipeline's images are BGR minus mean while FDA is
    defined on raw intensities, so the spectra are taken of ``x + mean[c]`` (only the DC coefficient sees that)
    and the result stays in the mean-subtracted domain; a length-``C`` sequence, or ``None`` for zeros.

    Returns a new float32 tensor, not clipped, without autograd: an input transform.  No host sync."""
    for name, t in (("images_s", images_s), ("images_t", images_t)):
        if not isinstance(t, torch.Tensor) or t.dim() != 4:
            raise RuntimeError(f"fda_source_to_target: {name} is not a [N, C, H, W] tensor")
        if t.dtype != torch.float32:
            raise RuntimeError(f"fda_source_to_target: {name} is {t.dtype}, expected float32")
    if tuple(images_s.shape) != tuple(images_t.shape):
        raise RuntimeError(f"fda_source_to_target: source {tuple(images_s.shape)} vs target {tuple(images_t.shape)}: "
                           "the spectra are swapped coefficient on coefficient, resize both domains to one size first")
    if images_s.device != images_t.device:
        raise RuntimeError(f"fda_source_to_target: source on {images_s.device}, target on {images_t.device}")
    for name, t in (("images_s", images_s), ("images_t", images_t)):
        if not t.is_contiguous():
            raise RuntimeError(f"fda_source_to_target: {name} is not contiguous (expected NCHW-contiguous)")
    n, c, h, w = images_s.shape
    if n < 1 or c < 1 or h < 1 or w < 1 or h * w >= 1 << 24 or w > _lib.FDA_MAX_W or n * c > 65535:
        raise ValueError(f"fda_source_to_target: {n} x {c} images of {h} x {w} pixels (expected N, C, H, W >= 1, "
                         f"H * W < 2^24, W <= {_lib.FDA_MAX_W}, N * C <= 65535)")
    beta = float(beta)
    if not math.isfinite(beta) or beta < 0:
        raise ValueError(f"fda_source_to_target: beta {beta!r} (expected a finite beta >= 0)")
    b = fda_band(h, w, beta)
    if 2 * b + 1 > min(h, w):
        raise ValueError(f"fda_source_to_target: beta {beta!r} gives b = {b} on {h} x {w} images "
                         f"(expected 2 b + 1 <= min(H, W) = {min(h, w)})")
    dev = images_s.device
    m = _mean_tensor(mean, c, dev, mean is IMG_MEAN)
    out = torch.empty_like(images_s)
    OPS.fda_transfer(images_s.detach(), images_t.detach(), b, m, twiddles(w, dev), twiddles(h, dev), out)
    return out
