"""Evaluation on the HIP engine: prediction maps and the mIoU confusion matrix.

Restates the per-image body of /root/reference/evaluate_cityscapes.py:153-169 and the
metric of compute_iou.py:15-61:

* ``predict(model, images)``: eval-mode forward, ``interp`` to (1024, 2048) (bilinear,
  align_corners=True) and the class argmax, fused into ONE kernel that reads the 1/8-scale
  logits and writes one byte per output pixel (the reference materialises the 19x1024x2048
  fp32 upsampled map, copies it to the host and runs numpy argmax).
* ``predict_tta(model, images, scales, mirror)``: multi-scale / mirrored testing (the DeepLab-v2
  protocol; the reference script runs one scale): one forward per scale and flip, then ONE kernel
  (``fuse_argmax``) that samples every map per output pixel, averages the softmaxes (or sums the
  logits) and writes the class byte and, on request, the winning class's averaged probability.
* ``ConfusionMatrix``: ``label_mapping`` (a 256-entry id -> trainId LUT) + ``fast_hist``
  accumulated on the device in int64; ``per_class_iu`` / ``miou`` on the 19x19 host copy.

Parity: tests/test_eval.py (golden vectors from the reference's compute_iou functions),
tests/test_tta_gpu.py (the fused kernel against an fp64 composition and the fp64 oracle network).
"""
from __future__ import annotations


import numpy as np
import torch

from . import _lib
from . import kernels as K
from .functional import interp
from .ops import OPS

# Cityscapes id -> trainId (the devkit's label2train; 19 classes of dataset/gta5_dataset.py:27-29)
CITYSCAPES_TRAIN_IDS = {7: 0, 8: 1, 11: 2, 12: 3, 13: 4, 17: 5, 19: 6, 20: 7, 21: 8, 22: 9, 23: 10,
                        24: 11, 25: 12, 26: 13, 27: 14, 28: 15, 31: 16, 32: 17, 33: 18}


def label_lut(mapping=None, device="cuda") -> torch.Tensor:
    """int32[256] LUT of compute_iou.label_mapping: listed ids map, other ids keep their value.
    ``mapping``: iterable of (id, trainId) pairs; default = Cityscapes label2train (all 34 ids,
    void ids -> 255)."""
    if mapping is None:
        mapping = [(i, CITYSCAPES_TRAIN_IDS.get(i, 255)) for i in range(34)]
    lut = np.arange(256, dtype=np.int32)
    for src, dst in mapping:
        lut[int(src)] = int(dst)
    return torch.from_numpy(lut).to(device)


def upsample_argmax(logits: torch.Tensor, out_hw) -> torch.Tensor:
    """[N, C, h, w] fp32 logits (any layout) -> uint8 [N, H, W] class map."""
    if not logits.is_cuda or logits.dtype != torch.float32:
        raise RuntimeError("upsample_argmax: expected a float32 HIP tensor")
    x = K.nhwc_view(logits)
    n, h, w, c = x.shape
    oh, ow = int(out_hw[0]), int(out_hw[1])
    out = torch.empty((n, oh, ow), dtype=torch.uint8, device=logits.device)
    OPS.upsample_argmax(x, out)
    return out


@torch.no_grad()
def predict(model, images: torch.Tensor, out_hw=(1024, 2048)) -> torch.Tensor:
    """evaluate_cityscapes.py:158-169: DeeplabMulti -> output2, DeeplabVGG -> its single map."""
    model.eval()
    out = model(images)
    logits = out if getattr(model, "single_output", False) else out[1]
    return upsample_argmax(logits, out_hw)


FUSE_MAX_MAPS = _lib.FUSE_MAX_MAPS
_FUSE_MODES = {"prob": _lib.FUSE_PROB, "logit": _lib.FUSE_LOGIT}


def tta_sizes(hw, scales) -> list:
    """Input sizes of multi-scale testing: (int(H*s + 0.5), int(W*s + 0.5)) per scale."""
    h, w = int(hw[0]), int(hw[1])
    sizes = []
    for s in scales:
        if not s > 0:
            raise ValueError(f"tta_sizes: scale {s!r} (expected > 0)")
        sizes.append((int(h * s + 0.5), int(w * s + 0.5)))
    return sizes


def _fuse_mode(mode, return_confidence, what):
    if mode not in _FUSE_MODES:
        raise ValueError(f"{what}: mode {mode!r} (expected 'prob' or 'logit')")
    if return_confidence and mode == "logit":
        raise ValueError(f"{what}: the confidence is the fused probability of the winning class; "
                         "mode='logit' has none")
    return _FUSE_MODES[mode]


def fuse_argmax(maps, mirrored=None, out_hw=(1024, 2048), mode="prob", return_confidence=False):
    """Fuse up to 8 logit maps [N, C, h_s, w_s] (fp32, any layout, sizes may differ) into one uint8
    [N, H, W] class map in ONE kernel: per output pixel every map is sampled bilinearly
    (align_corners=True; ``mirrored[s]`` reads map s flipped along W), then
    ``mode='prob'``: the softmaxes are averaged, ``mode='logit'``: the logits are summed, and the
    first maximal class wins.  ``return_confidence``: also the fp32 [N, H, W] averaged
    probability of that class ('prob' only).  No upsampled map is ever written."""
    maps = list(maps)
    mirrored = [False] * len(maps) if mirrored is None else [bool(m) for m in mirrored]
    m = _fuse_mode(mode, return_confidence, "fuse_argmax")
    if not 1 <= len(maps) <= FUSE_MAX_MAPS:
        raise ValueError(f"fuse_argmax: {len(maps)} maps (expected 1..{FUSE_MAX_MAPS})")
    if len(mirrored) != len(maps):
        raise ValueError(f"fuse_argmax: {len(mirrored)} mirror flags for {len(maps)} maps")
    for t in maps:
        if t.dim() != 4 or t.shape[:2] != maps[0].shape[:2]:
            raise ValueError(f"fuse_argmax: map {tuple(t.shape)} vs {tuple(maps[0].shape)}: "
                             "every map is [N, C, h, w] with the same N and C")
    for t in maps:
        if not t.is_cuda or t.dtype != torch.float32:
            raise RuntimeError("fuse_argmax: expected float32 HIP tensors")
    xs = [K.nhwc_view(t) for t in maps]
    n = xs[0].shape[0]
    oh, ow = int(out_hw[0]), int(out_hw[1])
    out = torch.empty((n, oh, ow), dtype=torch.uint8, device=xs[0].device)
    conf = torch.empty((n, oh, ow), dtype=torch.float32, device=xs[0].device) if return_confidence else None
    OPS.fuse_argmax(xs, mirrored, m, out, conf)
    return (out, conf) if return_confidence else out


@torch.no_grad()
def predict_tta(model, images: torch.Tensor, scales=(1.0,), mirror=True, out_hw=(1024, 2048), mode="prob",
                return_confidence=False):
    """Multi-scale, mirrored testing (the DeepLab-v2 evaluation protocol): one eval-mode forward per
    scale (in the order given; the input resized with ``interp`` unless the size is unchanged) and,
    with ``mirror``, one more on the input flipped along W, all fused by ONE ``fuse_argmax`` call.
    Returns the uint8 class map, or (map, confidence)."""
    _fuse_mode(mode, return_confidence, "predict_tta")
    sizes = tta_sizes(images.shape[2:], scales)
    nmaps = len(sizes) * (2 if mirror else 1)
    if not 1 <= nmaps <= FUSE_MAX_MAPS:
        raise ValueError(f"predict_tta: {len(sizes)} scales{' x 2 (mirror)' if mirror else ''} = {nmaps} maps "
                         f"(expected 1..{FUSE_MAX_MAPS})")
    model.eval()
    single = getattr(model, "single_output", False)
    maps, mirrored = [], []
    for hw in sizes:
        x = images if hw == tuple(images.shape[2:]) else interp(images, hw)
        for flip in (False, True) if mirror else (False,):
            out = model(torch.flip(x, dims=[3]) if flip else x)
            maps.append(out if single else out[1])
            mirrored.append(flip)
    return fuse_argmax(maps, mirrored, out_hw, mode, return_confidence)


class ConfusionMatrix:
    """Device-side ``hist += fast_hist(label_mapping(gt), pred, n)`` (compute_iou.py:54)."""

    def __init__(self, num_classes=19, mapping=None, device="cuda"):
        self.n = int(num_classes)
        self.hist = torch.zeros((self.n, self.n), dtype=torch.int64, device=device)
        self.lut = label_lut(mapping, device)

    def update(self, gt_ids: torch.Tensor, pred: torch.Tensor) -> None:
        """gt_ids: uint8 label-id map(s); pred: uint8 class map(s) of the same number of pixels.
        (compute_iou skips an image whose sizes differ; so does this: it raises.)"""
        if gt_ids.dtype != torch.uint8 or pred.dtype != torch.uint8:
            raise RuntimeError("ConfusionMatrix.update: uint8 label ids and predictions expected")
        if gt_ids.numel() != pred.numel():
            raise RuntimeError(f"ConfusionMatrix.update: {gt_ids.numel()} labels vs {pred.numel()} predictions")
        gt_ids, pred = gt_ids.contiguous(), pred.contiguous()
        OPS.confusion_hist(gt_ids, self.lut, pred, self.n, self.hist)

    def numpy(self) -> np.ndarray:
        return self.hist.cpu().numpy()

    def per_class_iu(self) -> np.ndarray:
        h = self.numpy().astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.diag(h) / (h.sum(1) + h.sum(0) - np.diag(h))

    def miou(self) -> float:
        return float(np.nanmean(self.per_class_iu()))
