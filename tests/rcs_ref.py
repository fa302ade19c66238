"""Numpy restatement of rare class sampling (adaptsegnet_amd/rcs.py and csrc/rcs.hip).  Imports nothing from
adaptsegnet_amd: the class counts, the nearest-coordinate walk of the augmented label window (a sequential fp64
loop, as the pipeline's), the window's label map, the crop counts, the class probabilities, the two-variate draw
and the selection rule, each written the plainest way."""
import numpy as np


def apply_lut(ids, lut):
    ids = np.asarray(ids)
    return ids.astype(np.int64) if lut is None else np.asarray(lut, dtype=np.int64)[ids]


def class_counts(ids, num_classes, lut=None):
    """int64 [n, num_classes]: per image the pixels of every trainId in [0, num_classes)."""
    t = apply_lut(ids, lut)
    out = np.zeros((t.shape[0], num_classes), np.int64)
    for i in range(t.shape[0]):
        for c in range(num_classes):
            out[i, c] = int((t[i] == c).sum())
    return out


def nearest_walk(in_size, out_size):
    """Source index of every position of a nearest resize in_size -> out_size: v = 0.5 * scale, then v += scale
    per position (a sequential fp64 accumulation, not (o + 0.5) * scale), index min(int(v), in_size - 1)."""
    scale = np.float64(in_size) / np.float64(out_size)
    v = np.float64(0.5) * scale
    idx = np.empty(out_size, np.int64)
    for o in range(out_size):
        idx[o] = min(int(v), in_size - 1)
        v = v + scale
    return idx


def window_tables(in_h, in_w, ch, cw, param):
    """(nx int64 [cw], ny int64 [ch]): the source column / row each window position reads, -1 for padding."""
    sw, sh, ox, oy, mirror = (int(v) for v in param)
    wx, wy = nearest_walk(in_w, sw), nearest_walk(in_h, sh)
    nx = np.full(cw, -1, np.int64)
    ny = np.full(ch, -1, np.int64)
    for x in range(cw):
        r = x + ox
        if 0 <= r < sw:
            nx[x] = wx[sw - 1 - r if mirror else r]
    for y in range(ch):
        r = y + oy
        if 0 <= r < sh:
            ny[y] = wy[r]
    return nx, ny


def label_window(ids2d, ch, cw, param, lut=None, ignore_label=255):
    """int64 [ch, cw]: the label window of the augmented pipeline for one sample."""
    in_h, in_w = ids2d.shape
    nx, ny = window_tables(in_h, in_w, ch, cw, param)
    t = apply_lut(ids2d, lut)
    out = np.full((ch, cw), ignore_label, np.int64)
    ys, xs = np.flatnonzero(ny >= 0), np.flatnonzero(nx >= 0)
    if len(ys) and len(xs):
        out[np.ix_(ys, xs)] = t[np.ix_(ny[ys], nx[xs])]
    return out


def crop_counts(ids, classes, candidates, ch, cw, lut=None):
    """int64 [n, K]: the pixels equal to classes[i] inside the scaled image of every candidate's label window
    (padding counts for no class, whatever the ignore label)."""
    ids = np.asarray(ids)
    cand = np.asarray(candidates)
    n, k = cand.shape[:2]
    out = np.zeros((n, k), np.int64)
    for i in range(n):
        t = apply_lut(ids[i], lut)
        for j in range(k):
            nx, ny = window_tables(ids.shape[1], ids.shape[2], ch, cw, cand[i, j])
            ys, xs = ny[ny >= 0], nx[nx >= 0]
            if len(ys) and len(xs):
                out[i, j] = int((t[np.ix_(ys, xs)] == int(classes[i])).sum())
    return out


def class_prob(counts, temperature, min_pixels):
    """(prob fp64 [C], eligible bool [C], images_with list of int64 arrays)."""
    counts = np.asarray(counts, dtype=np.int64)
    ncls = counts.shape[1]
    images_with = [np.array([i for i in range(counts.shape[0]) if counts[i, c] > min_pixels], np.int64)
                   for c in range(ncls)]
    eligible = np.array([len(v) > 0 for v in images_with])
    total = counts.sum(axis=0).astype(np.float64)
    freq = total / total.sum()
    z = (1.0 - freq) / temperature
    zmax = max(z[c] for c in range(ncls) if eligible[c])
    e = np.array([np.exp(z[c] - zmax) if eligible[c] else 0.0 for c in range(ncls)], np.float64)
    return e / e.sum(), eligible, images_with


def draw(rng, prob, eligible, images_with, n):
    """Two variates per sample: u = rng.random() picks the first class with cdf > u (the last eligible entry of
    the cdf is 1.0), then rng.integers picks one of its images."""
    cdf = np.cumsum(prob)
    cdf[max(c for c in range(len(prob)) if eligible[c])] = 1.0
    idx, cls = np.zeros(n, np.int64), np.zeros(n, np.int64)
    for i in range(n):
        u = rng.random()
        c = next(c for c in range(len(cdf)) if cdf[c] > u)
        j = int(rng.integers(len(images_with[c])))
        idx[i], cls[i] = images_with[c][j], c
    return idx, cls


def select(counts, min_crop_pixels):
    """Per row the first candidate with count > min_crop_pixels, else the last."""
    out = []
    for row in np.asarray(counts):
        k = len(row) - 1
        for j, v in enumerate(row):
            if v > min_crop_pixels:
                k = j
                break
        out.append(k)
    return np.array(out, np.int64)
