"""The ClassMix rules of adaptsegnet_amd/mix.py restated in numpy (the tests' reference).

Per image n, with C classes:
  count[n][c] = number of source-label pixels equal to c, 0 <= c < C                      (int32)
  nconf[n]    = number of target pixels with float32(conf) >= float32(tau); a NaN does not count
  present     = the classes with count > 0, k of them
  selected    = the ceil(k / 2) present classes with the smallest (key, class index) pairs (k = 0: none)
  q_n         = float32(nconf[n]) / float32(H * W), one float32 division
and per pixel p, m = (0 <= label_s[p] < C and label_s[p] is selected):
  mixed_image[:, p] = image_s[:, p] if m else image_t[:, p]
  mixed_label[p]    = label_s[p] if m else (pred_t[p] if pred_t[p] < C else ignore_label)     (int64)
  mixed_weight[p]   = 1 if m else q_n                                                          (float32)
"""
import numpy as np


def stats(labels_s, conf_t, tau, ncls):
    """(count int32 [N, C], nconf int32 [N])."""
    n = labels_s.shape[0]
    count = np.zeros((n, ncls), dtype=np.int32)
    for i in range(n):
        lab = labels_s[i].reshape(-1)
        ok = (lab >= 0) & (lab < ncls)
        count[i] = np.bincount(lab[ok], minlength=ncls).astype(np.int32)
    with np.errstate(invalid="ignore"):
        nconf = (conf_t.astype(np.float32) >= np.float32(tau)).reshape(n, -1).sum(axis=1).astype(np.int32)
    return count, nconf


def select(count_row, key_row):
    """uint8 [C] selection of one image from its counts and uint32 keys."""
    ncls = len(count_row)
    present = [c for c in range(ncls) if count_row[c] > 0]
    order = sorted(present, key=lambda c: (int(key_row[c]), c))
    sel = np.zeros(ncls, dtype=np.uint8)
    sel[order[:(len(present) + 1) // 2]] = 1
    return sel


def q_of(nconf, hw):
    q = np.float32(nconf) / np.float32(hw)
    assert q.dtype == np.float32
    return q


def apply(images_s, labels_s, images_t, pred_t, count, nconf, keys, ignore_label=255):
    """(mixed_images float32, mixed_labels int64, mixed_weights float32, mask uint8 [N, C])."""
    n, ncls = count.shape
    hw = labels_s.shape[1] * labels_s.shape[2]
    mask = np.stack([select(count[i], keys[i]) for i in range(n)])
    mi = np.empty_like(images_s, dtype=np.float32)
    ml = np.empty(labels_s.shape, dtype=np.int64)
    mw = np.empty(labels_s.shape, dtype=np.float32)
    for i in range(n):
        lab = labels_s[i]
        ok = (lab >= 0) & (lab < ncls)
        m = ok & (mask[i][np.where(ok, lab, 0)] != 0)
        pred = pred_t[i].astype(np.int64)
        mi[i] = np.where(m[None], images_s[i], images_t[i])
        ml[i] = np.where(m, lab, np.where(pred < ncls, pred, np.int64(ignore_label)))
        mw[i] = np.where(m, np.float32(1), q_of(nconf[i], hw))
    return mi, ml, mw, mask


def classmix(images_s, labels_s, images_t, pred_t, conf_t, keys, ncls=19, tau=0.968, ignore_label=255):
    """The whole of ``mix.classmix``: (mixed_images, mixed_labels, mixed_weights, mask, count, nconf)."""
    count, nconf = stats(labels_s, conf_t, tau, ncls)
    return apply(images_s, labels_s, images_t, pred_t, count, nconf, keys, ignore_label) + (count, nconf)
