"""Rare class sampling (RCS; Hoyer et al., DAFormer, CVPR 2022, section 3.2) for the SOURCE side of the input
pipeline: which labelled images a self-training run (DACS, MIC) draws, and where each is cropped.

  ClassStats        per image the number of pixels of every class, counted on the GPU (``label_class_count``)
  RareClassSampler  draws (image, class) pairs so that rare classes appear often
  crop_class_count  scores K candidate windows of ``data.preprocess_augmented`` per sample by the pixels of the
                    sample's class that the window would hold, in one read of the uint8 labels: nothing is resized
  choose_crops      DAFormer's rule on those scores: the first candidate with enough pixels, else the last
  RcsCrop           the two together behind an ``AugmentSampler``

The step and the trainer are unchanged: RCS only changes which batch the step receives."""
from __future__ import annotations

import collections

import numpy as np
import torch

from . import _lib
from .data import check_augment_params
from .ops import OPS

MAX_CANDIDATES = _lib.RCS_MAX_CANDIDATES


def _labels(labels_u8: torch.Tensor) -> torch.Tensor:
    if labels_u8.dtype != torch.uint8 or labels_u8.dim() != 3:
        raise ValueError("labels must be uint8 [n, H, W] (the decoded label files)")
    if not labels_u8.is_cuda:
        raise ValueError("the class counts run on the GPU: move the decoded labels to the device first")
    return labels_u8.contiguous()


def label_class_count(labels_u8: torch.Tensor, num_classes: int = 19, lut: torch.Tensor | None = None) -> torch.Tensor:
    """int64 [n, num_classes] on the device: per image the number of pixels of every trainId.

    labels_u8: uint8 [n, H, W] on the device; lut: int32 [256] id -> trainId (``data.trainid_lut``), or None for
    labels that hold trainIds already.  Ids that map outside [0, num_classes) count nowhere."""
    labels_u8 = _labels(labels_u8)
    if not 1 <= int(num_classes) <= 255:
        raise ValueError(f"num_classes {num_classes} (expected 1..255)")
    counts = torch.empty((labels_u8.shape[0], int(num_classes)), dtype=torch.int64, device=labels_u8.device)
    OPS.label_class_count(labels_u8, lut, int(num_classes), counts)
    return counts


class ClassStats:
    """``counts``: host int64 [N, C], the pixels of class c in image i of a labelled dataset, in dataset order."""

    def __init__(self, counts):
        counts = np.asarray(counts)
        if counts.ndim != 2 or counts.dtype.kind not in "iu":
            raise ValueError(f"counts must be an integer array [N, C], got {counts.dtype} {counts.shape}")
        self.counts = np.ascontiguousarray(counts, dtype=np.int64)

    @property
    def num_classes(self) -> int:
        return self.counts.shape[1]

    def __len__(self) -> int:
        return self.counts.shape[0]

    @classmethod
    def from_batches(cls, label_batches, num_classes: int = 19, lut: torch.Tensor | None = None, device="cuda"):
        """Counts an iterable of decoded uint8 label batches [n, H, W] (host or device; moved to ``device``) with
        ``label_class_count`` and concatenates them in order."""
        parts = []
        for batch in label_batches:
            batch = torch.as_tensor(batch)
            if not batch.is_cuda:
                batch = batch.to(device)
            parts.append(label_class_count(batch, num_classes, lut).cpu().numpy())
        if not parts:
            return cls(np.zeros((0, int(num_classes)), np.int64))
        return cls(np.concatenate(parts, axis=0))

    def save(self, path) -> None:
        np.savez(path, counts=self.counts)

    @classmethod
    def load(cls, path):
        with np.load(path, allow_pickle=False) as f:
            return cls(f["counts"])


class RareClassSampler:
    """Draws (image index, class) pairs: the class from ``class_prob``, then uniformly one of the images that hold
    more than ``min_pixels`` pixels of it.

    With n_c the pixels of class c in the whole dataset and f_c = n_c / sum_c' n_c', a class is ELIGIBLE iff at
    least one image has more than ``min_pixels`` pixels of it, and ``class_prob`` (fp64 [C]) is
    softmax((1 - f_c) / temperature) over the eligible classes (computed with the maximum subtracted), 0 elsewhere.
    This differs from DAFormer, which takes the softmax over every class that occurs and then fails when it draws a
    class that occurs but has no image with enough pixels of it; here such a class is never drawn.

    ``sample`` draws two variates per sample in a fixed order from numpy's PCG64 seeded with
    SeedSequence([seed, rank]), as the other samplers do, so every rank draws its own reproducible sequence;
    ``get_state`` / ``set_state`` let a resumed run continue it."""

    def __init__(self, stats: ClassStats, temperature: float = 0.01, min_pixels: int = 3000, seed: int = 1234,
                 rank: int = 0):
        counts = stats.counts if isinstance(stats, ClassStats) else ClassStats(stats).counts
        if not temperature > 0:
            raise ValueError(f"temperature {temperature} (expected > 0)")
        self.temperature = float(temperature)
        self.min_pixels = int(min_pixels)
        ncls = counts.shape[1]
        self.images_with = [np.flatnonzero(counts[:, c] > self.min_pixels).astype(np.int64) for c in range(ncls)]
        eligible = np.array([len(ix) > 0 for ix in self.images_with], dtype=bool)
        if not eligible.any():
            raise ValueError(f"no class has an image with more than {self.min_pixels} pixels of it")
        total = counts.sum(axis=0).astype(np.float64)
        freq = total / total.sum()
        z = (1.0 - freq) / self.temperature
        e = np.where(eligible, np.exp(z - z[eligible].max()), 0.0)
        self.eligible = eligible
        self.class_prob = e / e.sum()
        self.cdf = np.cumsum(self.class_prob)
        self.cdf[np.flatnonzero(eligible)[-1]] = 1.0
        self.rng = np.random.Generator(np.random.PCG64(np.random.SeedSequence([int(seed), int(rank)])))
        self.pending: collections.deque = collections.deque()

    def sample(self, n: int):
        """(indices int64 [n], classes int64 [n]).  Per sample u = rng.random(), the class is the first c with
        cdf[c] > u; then j = rng.integers(len(images_with[c])) and the index is images_with[c][j]."""
        idx = np.zeros(n, np.int64)
        cls = np.zeros(n, np.int64)
        for i in range(n):
            u = self.rng.random()
            c = int(np.argmax(self.cdf > u))
            j = int(self.rng.integers(len(self.images_with[c])))
            idx[i] = self.images_with[c][j]
            cls[i] = c
        return idx, cls

    def get_state(self) -> dict:
        return self.rng.bit_generator.state

    def set_state(self, state: dict) -> None:
        self.rng.bit_generator.state = state

    def batch_iter(self, batch_size: int):
        """An endless generator of index lists, usable as a DataLoader's ``batch_sampler``.  Each batch's classes
        (int64 [batch_size]) are appended to ``self.pending``; the training loop pops them in order, because a
        DataLoader yields batches in sampler order."""
        while True:
            idx, cls = self.sample(batch_size)
            self.pending.append(cls)
            yield idx.tolist()


def _candidates(candidates, n, in_h, in_w) -> np.ndarray:
    c = np.asarray(candidates)
    if c.dtype.kind not in "iu" or c.ndim != 3 or c.shape[0] != n or c.shape[2] != 5:
        raise ValueError(f"candidates must be an integer array [{n}, K, 5] = (sw, sh, ox, oy, mirror), "
                         f"got {c.dtype} {c.shape}")
    k = c.shape[1]
    if not 1 <= k <= MAX_CANDIDATES:
        raise ValueError(f"{k} candidates per sample (expected 1..{MAX_CANDIDATES})")
    return check_augment_params(c.reshape(n * k, 5), n * k, in_h, in_w).reshape(n, k, 5)


def crop_class_count(labels_u8: torch.Tensor, classes, candidates, crop_size,
                     lut: torch.Tensor | None = None) -> torch.Tensor:
    """int64 [n, K] on the device: counts[i][k] = the number of pixels equal to classes[i] in the label window that
    ``data.preprocess_augmented(images, labels, crop_size, candidates[:, k])`` returns for sample i, bit-exact,
    without resizing an image or materialising a window (adaptseg_crop_class_count).

    labels_u8: uint8 [n, H, W] on the device; classes: n integers in [0, 255] (host sequence or tensor);
    candidates: integer array [n, K, 5] = (sw, sh, ox, oy, mirror) on the host, K <= 16; crop_size: (W, H);
    lut: as ``label_class_count`` (None: the labels hold trainIds already)."""
    labels_u8 = _labels(labels_u8)
    n, h, w = labels_u8.shape
    cand = _candidates(candidates, n, h, w)
    cw, ch = int(crop_size[0]), int(crop_size[1])
    if cw < 1 or ch < 1 or cw * ch >= 1 << 31:
        raise ValueError(f"crop_size {crop_size} (expected positive sides with W * H < 2^31)")
    if isinstance(classes, torch.Tensor) and classes.is_cuda:
        cls = classes.to(torch.int32).contiguous()
    else:
        chost = np.asarray(classes.cpu() if isinstance(classes, torch.Tensor) else classes)
        if chost.shape != (n,) or chost.dtype.kind not in "iu":
            raise ValueError(f"classes must be {n} integers, got {chost.dtype} {chost.shape}")
        if ((chost < 0) | (chost > 255)).any():
            raise ValueError("classes must lie in [0, 255]")
        cls = torch.from_numpy(chost.astype(np.int32)).to(labels_u8.device)
    if tuple(cls.shape) != (n,):
        raise ValueError(f"classes must be {n} integers, got {tuple(cls.shape)}")
    counts = torch.empty((n, cand.shape[1]), dtype=torch.int64, device=labels_u8.device)
    OPS.crop_class_count(labels_u8, lut, cls, cand.reshape(-1).tolist(), ch, cw, counts)
    return counts


def select_crops(counts, min_crop_pixels: int) -> np.ndarray:
    """int64 [n]: per row of the host count table [n, K] the first k with counts[k] > min_crop_pixels, else K - 1."""
    counts = np.asarray(counts)
    ok = counts > min_crop_pixels
    return np.where(ok.any(axis=1), ok.argmax(axis=1), counts.shape[1] - 1).astype(np.int64)


def choose_crops(labels_u8: torch.Tensor, classes, candidates, crop_size, min_crop_pixels: int = 1500,
                 lut: torch.Tensor | None = None):
    """(params int32 [n, 5], chosen int64 [n], counts int64 [n, K]), all on the host: per sample the first
    candidate whose window holds more than ``min_crop_pixels`` pixels of the sample's class, else the last one.

    This is DAFormer's rule (up to 10 tries, keep the last; its threshold is min_pixels * 0.5).  The [n, K] counts
    come back to the host in one copy, because ``preprocess_augmented`` takes its parameters as host integers: one
    small device-to-host copy (and the synchronisation it implies) per batch in the input pipeline."""
    counts = crop_class_count(labels_u8, classes, candidates, crop_size, lut).cpu().numpy()
    chosen = select_crops(counts, min_crop_pixels)
    cand = np.asarray(candidates)
    params = cand[np.arange(cand.shape[0]), chosen].astype(np.int32)
    return params, chosen, counts


class RcsCrop:
    """Class-aware crops behind an ``AugmentSampler``: ``tries`` parameter sets are drawn per sample and
    ``choose_crops`` keeps one.  The sampler's stream advances by exactly n * tries draws per call, whichever
    candidates are kept, so a resumed run (``aug_sampler.get_state`` / ``set_state``) continues it."""

    def __init__(self, aug_sampler, tries: int = 10, min_crop_pixels: int = 1500):
        if not 1 <= int(tries) <= MAX_CANDIDATES:
            raise ValueError(f"tries {tries} (expected 1..{MAX_CANDIDATES})")
        self.aug_sampler = aug_sampler
        self.tries = int(tries)
        self.min_crop_pixels = int(min_crop_pixels)

    def params(self, labels_u8: torch.Tensor, classes, lut: torch.Tensor | None = None) -> np.ndarray:
        """int32 [n, 5], the parameters to hand to ``data.preprocess_augmented`` with the sampler's crop size."""
        n = labels_u8.shape[0]
        cand = self.aug_sampler.sample(n * self.tries).reshape(n, self.tries, 5)
        return choose_crops(labels_u8, classes, cand, self.aug_sampler.crop_size, self.min_crop_pixels, lut)[0]
