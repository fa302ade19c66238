"""Input pipeline: the reference's dataset classes with the per-image
arithmetic moved to the GPU.

Reference: dataset/gta5_dataset.py (GTA5DataSet) and the target loader the training script
builds (train_gta2cityscapes_multi.py:333-336, 520-523; ``dataset/cityscapes_dataset.py`` is
absent from the reference tree — its call site passes the same crop/mean/mirror arguments and
the loader is the image half of GTA5DataSet).

Split of the work:
  * ``__getitem__`` (DataLoader worker, CPU) only decodes the files, exactly as the reference
    opens them (``Image.open(img).convert('RGB')``, ``Image.open(label)``), and returns uint8
    arrays at the file's own size — no resize, remap or float conversion on the host;
  * ``preprocess`` (training process, GPU) runs the rest of __getitem__ (:54-68) on the whole
    batch in one library call (adaptseg_gta5_preprocess): Pillow-exact bicubic / nearest
    resize, id -> trainId LUT, RGB -> BGR, ``-= IMG_MEAN``, CHW — bit-identical to the
    reference's output (tests/test_data.py);
  * ``preprocess_augmented`` is the same call with a per-sample random scale, crop / pad window
    and horizontal mirror (adaptseg_gta5_preprocess_augment) — the augmentation the reference's
    ``--random-scale`` / ``--random-mirror`` flags name and its dataset drops; the parameters
    come from ``AugmentSampler`` on the host (tests/test_augment_*.py).
"""
from __future__ import annotations

import os.path as osp

import numpy as np
import torch

from .ops import OPS

IMG_MEAN = np.array((104.00698793, 116.66876762, 122.67891434), dtype=np.float32)  # train:30
ID_TO_TRAINID = {7: 0, 8: 1, 11: 2, 12: 3, 13: 4, 17: 5, 19: 6, 20: 7, 21: 8, 22: 9, 23: 10, 24: 11,
                 25: 12, 26: 13, 27: 14, 28: 15, 31: 16, 32: 17, 33: 18}      # gta5_dataset.py:27-29

_LUTS: dict = {}


def trainid_lut(device, mapping=None, ignore_label=255) -> torch.Tensor:
    """int32[256] id -> trainId table on ``device`` (255 for ids outside the mapping)."""
    mapping = ID_TO_TRAINID if mapping is None else mapping
    key = (str(device), tuple(sorted(mapping.items())), ignore_label)
    t = _LUTS.get(key)
    if t is None:
        lut = np.full(256, ignore_label, np.int32)
        for k, v in mapping.items():
            lut[k] = v
        t = _LUTS[key] = torch.from_numpy(lut).to(device)
    return t


def _prepare(images, labels, crop_size, lut):
    """Argument checks and output allocation shared by ``preprocess`` and ``preprocess_augmented``."""
    if images.dtype != torch.uint8 or images.dim() != 4 or images.shape[-1] != 3:
        raise ValueError("images must be uint8 [n, H, W, 3]")
    if not images.is_cuda:
        raise ValueError("preprocess runs on the GPU: move the decoded batch to the device first")
    images = images.contiguous()
    n, h, w, _ = images.shape
    ow, oh = crop_size
    out = torch.empty((n, 3, oh, ow), device=images.device, dtype=torch.float32)
    lab_out = None
    if labels is not None:
        if labels.dtype != torch.uint8 or tuple(labels.shape) != (n, h, w):
            raise ValueError("labels must be uint8 [n, H, W] matching images")
        labels = labels.contiguous()
        lab_out = torch.empty((n, oh, ow), device=images.device, dtype=torch.int64)
        if lut is None:
            lut = trainid_lut(images.device)
    return images, labels, out, lab_out, lut if labels is not None else None


def preprocess(images: torch.Tensor, labels: torch.Tensor | None = None, crop_size=(1280, 720),
               mean=IMG_MEAN, lut: torch.Tensor | None = None):
    """GTA5DataSet.__getitem__ :54-68 on a decoded batch, on the GPU.

    images: uint8 [n, H, W, 3] RGB (device); labels: uint8 [n, H, W] class ids or None.
    crop_size: (W, H) as the reference's ``crop_size``.  Returns (float32 [n, 3, h, w] BGR
    minus ``mean``, int64 [n, h, w] trainIds or None) — the reference's image / label after
    ``.long()`` (train:595)."""
    images, labels, out, lab_out, lut = _prepare(images, labels, crop_size, lut)
    m = np.asarray(mean, dtype=np.float32)
    OPS.gta5_preprocess(images, [float(m[0]), float(m[1]), float(m[2])], out, labels, lut, lab_out)
    return out, lab_out


_AUG_LIMIT = 1 << 20    # sw, sh, |ox|, |oy| stay below it (include/adaptseg.h)
_MAX_DOWNSCALE_TAPS = 64


def check_augment_params(params, n, in_h, in_w) -> np.ndarray:
    """``params`` as an int32 [n, 5] array of (sw, sh, ox, oy, mirror), or ValueError: the
    checks adaptseg_gta5_preprocess_augment makes on the host, made before the library is called."""
    p = np.asarray(params)
    if p.dtype.kind not in "iu" or p.shape != (n, 5):
        raise ValueError(f"augment params must be an integer array [{n}, 5] = (sw, sh, ox, oy, mirror), "
                         f"got {p.dtype} {p.shape}")
    p64 = p.astype(np.int64)
    sw, sh, ox, oy, mir = p64.T
    if ((sw < 1) | (sh < 1) | (sw >= _AUG_LIMIT) | (sh >= _AUG_LIMIT)).any():
        raise ValueError("augment params: scaled sizes sw, sh must be in [1, 2^20)")
    if ((abs(ox) >= _AUG_LIMIT) | (abs(oy) >= _AUG_LIMIT)).any():
        raise ValueError("augment params: offsets |ox|, |oy| must be below 2^20")
    if ((mir != 0) & (mir != 1)).any():
        raise ValueError("augment params: mirror must be 0 or 1")
    for size, scaled in ((in_w, sw), (in_h, sh)):
        taps = np.ceil(2.0 * np.maximum(size / scaled, 1.0)) * 2 + 1
        if (taps > _MAX_DOWNSCALE_TAPS).any():
            raise ValueError("augment params: downscale factor above 15 not supported")
    return p64.astype(np.int32)


def preprocess_augmented(images: torch.Tensor, labels: torch.Tensor | None, crop_size, params,
                         mean=IMG_MEAN, lut: torch.Tensor | None = None, ignore_label=255):
    """``preprocess`` with a per-sample random scale, crop / pad window and horizontal mirror, in
    one library call (adaptseg_gta5_preprocess_augment).

    params: integer array [n, 5] = (sw, sh, ox, oy, mirror), on the host (``AugmentSampler``
    draws them).  Sample i is resized to (sw, sh) exactly as ``preprocess`` would, flipped
    left-right if ``mirror``, and the ``crop_size`` window whose top-left corner is (ox, oy) is
    returned; where the window leaves the scaled image the image is 0.0 (a pixel equal to the
    mean) and the label ``ignore_label``.  With (sw, sh) = crop_size, offset 0 and no mirror the
    result equals ``preprocess`` bit for bit."""
    images, labels, out, lab_out, lut = _prepare(images, labels, crop_size, lut)
    n, h, w, _ = images.shape
    p = check_augment_params(params, n, h, w)
    m = np.asarray(mean, dtype=np.float32)
    OPS.gta5_preprocess_augment(images, [float(m[0]), float(m[1]), float(m[2])], p.reshape(-1).tolist(),
                                int(ignore_label), out, labels, lut, lab_out)
    return out, lab_out


class AugmentSampler:
    """Draws the per-sample parameters of ``preprocess_augmented`` on the host.

    Per sample: a factor f uniform from ``scales``; sw = int(cw * f + 0.5), sh likewise; ox a
    uniform integer in [0, sw - cw] when the scaled image is at least as wide as the crop, else
    0 (the crop is padded on the right / bottom), oy likewise; mirror a fair coin when enabled.
    The generator is numpy's PCG64 seeded from (seed, rank), so every rank draws its own
    reproducible sequence; ``get_state`` / ``set_state`` let a resumed run continue it."""

    def __init__(self, crop_size, scales=(0.5, 0.6, 0.7, 0.8, 0.9, 1.0, 1.1, 1.2, 1.3, 1.4, 1.5), mirror=True,
                 seed=1234, rank=0):
        self.crop_size = (int(crop_size[0]), int(crop_size[1]))
        self.scales = tuple(float(f) for f in scales)
        if not self.scales or min(self.scales) <= 0:
            raise ValueError("scales must be a non-empty sequence of positive factors")
        self.mirror = bool(mirror)
        self.rng = np.random.Generator(np.random.PCG64(np.random.SeedSequence([int(seed), int(rank)])))

    def sample(self, n: int) -> np.ndarray:
        cw, ch = self.crop_size
        out = np.zeros((n, 5), np.int32)
        for i in range(n):
            f = self.scales[int(self.rng.integers(len(self.scales)))]
            sw, sh = int(cw * f + 0.5), int(ch * f + 0.5)
            ox = int(self.rng.integers(sw - cw + 1)) if sw >= cw else 0
            oy = int(self.rng.integers(sh - ch + 1)) if sh >= ch else 0
            mir = int(self.rng.integers(2)) if self.mirror else 0
            out[i] = (sw, sh, ox, oy, mir)
        return out

    def get_state(self) -> dict:
        return self.rng.bit_generator.state

    def set_state(self, state: dict) -> None:
        self.rng.bit_generator.state = state


def _decode_rgb(path):
    from PIL import Image
    return np.asarray(Image.open(path).convert("RGB"), dtype=np.uint8)


def _decode_ids(path):
    from PIL import Image
    return np.asarray(Image.open(path), dtype=np.uint8)


class GTA5DataSet(torch.utils.data.Dataset):
    """Same constructor and file list as the reference (gta5_dataset.py:14-45).  Items are
    the decoded uint8 image / label at file size plus the name; ``collate`` stacks a batch of
    equally sized files and ``preprocess`` turns it into the reference's tensors on the GPU.

    ``scale`` and ``mirror`` are stored and ignored, as the reference's dataset ignores them
    (gta5_dataset.py:18,21); they default to True, so honouring them would change what an
    unchanged caller gets.  Random scale / crop / mirror is opt-in per batch: pass
    ``AugmentSampler(crop_size).sample(n)`` as ``preprocess(..., augment=...)``."""

    def __init__(self, root, list_path, max_iters=None, crop_size=(321, 321), mean=(128, 128, 128),
                 scale=True, mirror=True, ignore_label=255):
        self.root, self.list_path = root, list_path
        self.crop_size, self.scale, self.ignore_label = crop_size, scale, ignore_label
        self.mean, self.is_mirror = mean, mirror
        self.img_ids = [i_id.strip() for i_id in open(list_path)]
        if max_iters is not None:
            self.img_ids = self.img_ids * int(np.ceil(float(max_iters) / len(self.img_ids)))
        self.id_to_trainid = dict(ID_TO_TRAINID)
        self.files = [{"img": osp.join(root, "images/%s" % name), "label": osp.join(root, "labels/%s" % name),
                       "name": name} for name in self.img_ids]

    def __len__(self):
        return len(self.files)

    def __getitem__(self, index):
        f = self.files[index]
        return _decode_rgb(f["img"]), _decode_ids(f["label"]), f["name"]

    def preprocess(self, images, labels, device=None, augment=None):
        """The device half of __getitem__ for a collated batch (numpy or tensors).  ``augment``:
        None (the reference's behaviour: resize to ``crop_size``), or an [n, 5] parameter array
        (``AugmentSampler.sample``) for ``preprocess_augmented``."""
        dev = device or torch.device("cuda", torch.cuda.current_device())
        im = torch.as_tensor(images).to(dev, non_blocking=True)
        lb = torch.as_tensor(labels).to(dev, non_blocking=True)
        lut = trainid_lut(dev, self.id_to_trainid, self.ignore_label)
        if augment is not None:
            return preprocess_augmented(im, lb, self.crop_size, augment, self.mean, lut, self.ignore_label)
        return preprocess(im, lb, self.crop_size, self.mean, lut)


class cityscapesDataSet(torch.utils.data.Dataset):  # noqa: N801  (the reference's class name)
    """The target loader of train_gta2cityscapes_multi.py:333-336 / 520-523 (its module is
    absent from the reference tree): list of ``leftImg8bit/<set>/<name>`` images; items are the
    decoded uint8 image at file size, the device half resizes to ``crop_size`` (BICUBIC),
    flips to BGR and subtracts ``mean`` like GTA5DataSet's image path.  ``scale`` / ``mirror``
    are stored and ignored as in GTA5DataSet; ``preprocess(..., augment=...)`` augments."""

    def __init__(self, root, list_path, max_iters=None, crop_size=(321, 321), mean=(128, 128, 128),
                 scale=True, mirror=True, ignore_label=255, set="val"):  # noqa: A002
        self.root, self.list_path, self.set = root, list_path, set
        self.crop_size, self.scale, self.ignore_label = crop_size, scale, ignore_label
        self.mean, self.is_mirror = mean, mirror
        self.img_ids = [i_id.strip() for i_id in open(list_path)]
        if max_iters is not None:
            self.img_ids = self.img_ids * int(np.ceil(float(max_iters) / len(self.img_ids)))
        self.files = [{"img": osp.join(root, "leftImg8bit/%s/%s" % (set, name)), "name": name}
                      for name in self.img_ids]

    def __len__(self):
        return len(self.files)

    def __getitem__(self, index):
        f = self.files[index]
        return _decode_rgb(f["img"]), f["name"]

    def preprocess(self, images, device=None, augment=None):
        """``augment``: None, or an [n, 5] parameter array as in GTA5DataSet.preprocess."""
        dev = device or torch.device("cuda", torch.cuda.current_device())
        im = torch.as_tensor(images).to(dev, non_blocking=True)
        if augment is not None:
            return preprocess_augmented(im, None, self.crop_size, augment, self.mean)[0]
        return preprocess(im, None, self.crop_size, self.mean)[0]


def collate(batch):
    """Stack decoded items of one size: (uint8 [n,H,W,3], uint8 [n,H,W] or None, names)."""
    imgs = np.stack([b[0] for b in batch])
    if len(batch[0]) == 3:
        return imgs, np.stack([b[1] for b in batch]), [b[2] for b in batch]
    return imgs, None, [b[1] for b in batch]


__all__ = ["IMG_MEAN", "ID_TO_TRAINID", "preprocess", "preprocess_augmented", "AugmentSampler",
           "check_augment_params", "trainid_lut", "GTA5DataSet", "cityscapesDataSet", "collate"]
