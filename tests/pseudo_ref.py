"""The pseudo-label rules of adaptsegnet_amd/pseudo.py restated in numpy (the tests' reference).

A pixel is VALID when ``pred < ncls`` and ``conf >= 0`` (a NaN or negative confidence is not).
  bin        = nbins-1 if conf >= 1 else int(float32(conf) * float32(nbins))
  hist[c][b] = number of valid pixels of class c in bin b
  threshold  : T = sum_b hist[c][b]; T == 0 -> cap; else K = ceil(portion * T), b* = the largest bin
               whose suffix sum is >= K, thr = min(float32(b*) / float32(nbins), float32(cap))
  label      = pred if valid and conf >= thr[pred] else ignore_label; kept[c] = pixels kept of class c
"""
import math

import numpy as np


def valid(pred, conf, ncls):
    with np.errstate(invalid="ignore"):
        return (pred.astype(np.int64) < ncls) & (conf.astype(np.float32) >= np.float32(0))


def bin_of(conf, nbins):
    """Bins of VALID confidences (float32 array, every value >= 0)."""
    conf = conf.astype(np.float32)
    prod = conf * np.float32(nbins)
    assert prod.dtype == np.float32
    top = conf >= np.float32(1)
    return np.where(top, nbins - 1, np.where(top, 0, prod).astype(np.int64))


def conf_hist(pred, conf, ncls, nbins):
    pred, conf = pred.reshape(-1), conf.reshape(-1)
    ok = valid(pred, conf, ncls)
    hist = np.zeros((ncls, nbins), dtype=np.int64)
    np.add.at(hist, (pred[ok].astype(np.int64), bin_of(conf[ok], nbins)), 1)
    return hist


def threshold_bins(hist, portion):
    """b* per class (None for an empty class)."""
    out = []
    for row in hist:
        total = int(row.sum())
        if total == 0:
            out.append(None)
            continue
        k = math.ceil(portion * total)
        suffix = np.cumsum(row[::-1])[::-1]
        out.append(int(np.nonzero(suffix >= k)[0].max()))
    return out


def thresholds(hist, portion, cap):
    nbins = hist.shape[1]
    cap = np.float32(cap)
    thr = np.empty(hist.shape[0], dtype=np.float32)
    for c, b in enumerate(threshold_bins(hist, portion)):
        thr[c] = cap if b is None else min(np.float32(b) / np.float32(nbins), cap)
    return thr


def labels(pred, conf, thr, ignore_label=255):
    """(int64 labels of pred's shape, int64 [C] kept counts)."""
    ncls = thr.shape[0]
    flat_p, flat_c = pred.reshape(-1), conf.reshape(-1).astype(np.float32)
    ok = valid(flat_p, flat_c, ncls)
    cls = np.where(ok, flat_p, 0).astype(np.int64)
    with np.errstate(invalid="ignore"):
        keep = ok & (flat_c >= thr.astype(np.float32)[cls])
    lab = np.where(keep, flat_p.astype(np.int64), np.int64(ignore_label))
    kept = np.bincount(cls[keep], minlength=ncls).astype(np.int64)
    return lab.reshape(pred.shape), kept


def mixed_input(shape, ncls=19, nbins=512, seed=5, empty_class=7):
    """uint8 class map and float32 confidences of ``shape``: Beta(5, 1) confidences, no pixel of
    ``empty_class``, and (as far as the pixel count allows, at most half of it) 50 pixels at 1.0,
    10 at 0.0, 10 NaN, 10 negative and 10 exactly on a bin edge."""
    rng = np.random.Generator(np.random.PCG64(seed))
    n = int(np.prod(shape))
    classes = np.array([c for c in range(ncls) if c != empty_class], dtype=np.uint8)
    pred = classes[rng.integers(0, len(classes), n)]
    conf = rng.beta(5.0, 1.0, n).astype(np.float32)
    edges = (rng.integers(1, nbins, 10).astype(np.float32) / np.float32(nbins)).tolist()
    special = [1.0] * 50 + [0.0] * 10 + [float("nan")] * 10 + [-0.25] * 10 + edges
    special = np.array(special, dtype=np.float32)[rng.permutation(len(special))][:n // 2]
    conf[rng.permutation(n)[:len(special)]] = special
    return pred.reshape(shape), conf.reshape(shape)
