"""Rare class sampling (RCS) on the GPU: the kernels of csrc/rcs.hip and the Python surface around them.  Every
comparison is bit-exact (integer counts).

A. ``label_class_count`` against the numpy restatement tests/rcs_ref.py: the scalar and the 16-byte paths, more
   than one block per image, with and without the id table, a one-class map (the contention case of the LDS bins),
   a map whose ids all map to 255, one class and nineteen, a second call into the same output.
B. ``crop_class_count`` against two yardsticks at once, the restatement and the existing pipeline
   ``(data.preprocess_augmented(...)[1] == c).sum()``, on hand-picked candidates: down- and upscaling by more than
   2, mirror, windows partly outside on each of the four sides and wholly outside, the identity; a class that is
   absent, a one-class image (the multiplicity sums on their own), different classes per sample, ids used as
   trainIds, a label buffer that is not 16-byte aligned; the workload's geometry.
C. ``choose_crops`` and ``RcsCrop`` on constructed inputs, ``ClassStats.from_batches``.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rcs_ref as RR  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
CITY_IDS = (7, 8, 11, 12, 13, 17, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 31, 32)   # every mapped id but 33
OTHER_IDS = (0, 1, 4, 6, 34, 200, 255)                                             # ids the table maps to 255


def _lut_np():
    from adaptsegnet_amd import data
    lut = np.full(256, 255, np.int64)
    for k, v in data.ID_TO_TRAINID.items():
        lut[k] = v
    return lut


def _lut_dev():
    from adaptsegnet_amd import data
    return data.trainid_lut(torch.device(DEV))


def _ids(n, h, w, seed):
    """Random label files: blocks of a few pixels, so that neighbouring pixels often agree, of every mapped id but
    33 (trainId 18 stays absent) and some unmapped ones."""
    rng = np.random.default_rng(seed)
    pool = np.array(CITY_IDS + OTHER_IDS, np.uint8)
    coarse = pool[rng.integers(len(pool), size=(n, (h + 2) // 3, (w + 4) // 5))]
    ids = np.ascontiguousarray(np.repeat(np.repeat(coarse, 3, axis=1), 5, axis=2)[:, :h, :w])
    ids[:, 0, 0], ids[:, -1, -1] = 7, 26          # the corners are road and car, whatever was drawn
    return ids


# ---- A. label_class_count ------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 5, 7), (3, 37, 83), (2, 64, 128), (2, 300, 517)])
@pytest.mark.parametrize("use_lut", [True, False])
def test_label_class_count_matches_the_restatement(shape, use_lut):
    from adaptsegnet_amd import rcs
    ids = _ids(*shape, seed=sum(shape))
    if not use_lut:
        ids = (ids % 23).astype(np.uint8)            # trainIds 0..22: 19..22 count nowhere
    dev = torch.from_numpy(ids).to(DEV)
    for ncls in (19, 1):
        got = rcs.label_class_count(dev, ncls, _lut_dev() if use_lut else None)
        assert got.dtype == torch.int64 and tuple(got.shape) == (shape[0], ncls) and got.is_cuda
        want = RR.class_counts(ids, ncls, _lut_np() if use_lut else None)
        np.testing.assert_array_equal(got.cpu().numpy(), want)
        assert ncls != 19 or want.sum() > 0


def test_label_class_count_one_class_all_ignored_and_overwrite():
    from adaptsegnet_amd import rcs
    from adaptsegnet_amd.ops import OPS
    lut = _lut_dev()
    for h, w in ((64, 128), (37, 83)):
        one = torch.full((2, h, w), 26, dtype=torch.uint8, device=DEV)        # all car: one LDS bin takes every add
        got = rcs.label_class_count(one, 19, lut).cpu().numpy()
        want = np.zeros((2, 19), np.int64)
        want[:, 13] = h * w
        np.testing.assert_array_equal(got, want)
        none = torch.full((2, h, w), 4, dtype=torch.uint8, device=DEV)        # every id maps to 255
        assert int(rcs.label_class_count(none, 19, lut).abs().sum()) == 0
        assert int(rcs.label_class_count(torch.full_like(none, 255), 19, None).abs().sum()) == 0
    ids = _ids(2, 64, 128, seed=2)
    out = torch.full((2, 19), 12345, dtype=torch.int64, device=DEV)
    OPS.label_class_count(torch.from_numpy(ids).to(DEV), lut, 19, out)
    first = out.clone()
    OPS.label_class_count(torch.from_numpy(ids).to(DEV), lut, 19, out)        # overwritten, not accumulated
    np.testing.assert_array_equal(out.cpu().numpy(), RR.class_counts(ids, 19, _lut_np()))
    assert torch.equal(out, first)


def test_class_stats_from_batches_concatenates_in_order():
    from adaptsegnet_amd import rcs
    a, b = _ids(2, 37, 83, seed=5), _ids(3, 37, 83, seed=6)
    stats = rcs.ClassStats.from_batches([torch.from_numpy(a), torch.from_numpy(b).to(DEV)], 19, _lut_dev())
    want = np.concatenate([RR.class_counts(a, 19, _lut_np()), RR.class_counts(b, 19, _lut_np())])
    np.testing.assert_array_equal(stats.counts, want)
    assert stats.counts.dtype == np.int64 and len(stats) == 5


# ---- B. crop_class_count -------------------------------------------------------------------------------
def _hand_candidates(in_h, in_w, cw, ch):
    """Sixteen parameter sets (sw, sh, ox, oy, mirror) that between them cover the cases of the module docstring."""
    c = [
        (cw, ch, 0, 0, 0),                                        # the identity of the pipeline: scaled size = crop
        (in_w // 3, in_h // 3, 0, 0, 0),                          # downscale by 3 and more; padded right / bottom
        (2 * in_w + in_w // 2 + 1, 3 * in_h, in_w // 2, in_h, 1),  # upscale by more than 2 on both axes, mirrored
        (in_w // 3 + 1, in_h // 2, -5, 3, 1),                     # mirrored downscale, outside on the left
        (cw + 10, ch + 7, -11, -6, 0),                            # outside on the left and the top
        (cw + 10, ch + 7, 25, 17, 1),                             # outside on the right and the bottom
        (cw, ch, cw + 3, 0, 0),                                   # wholly outside, to the right: 0
        (cw, ch, 0, -ch - 2, 1),                                  # wholly outside, above: 0
        (3 * in_w, in_h, in_w, 0, 1),                             # upscale by 3 on x alone
        (max(1, in_w // 7), max(1, in_h // 7), -3, -2, 0),        # downscale by 7 and more
        (in_w, in_h, 0, 0, 0),                                    # the source's own size
        (in_w, in_h, in_w - cw // 2, in_h - ch // 2, 1),          # its bottom-right corner
        (in_w, in_h * 5 // 2, 3, in_h, 0),                        # upscale by 2.5 on y alone
        (2 * cw, 2 * ch, cw // 2, ch // 2, 1),
        (max(cw // 2 + 1, in_w // 10 + 1), max(ch // 2 + 1, in_h // 10 + 1), -(cw // 4), -(ch // 4), 0),
        (2 * in_w + 1, 2 * in_h + 1, -1, -1, 1),
    ]
    return np.array(c, np.int32)


def _pipeline_counts(images, labels, crop, cand, classes, lut):
    """counts [n, K] by the existing pipeline: K augmented label windows, materialised and compared."""
    from adaptsegnet_amd import data
    cls = torch.as_tensor(np.asarray(classes), device=DEV).view(-1, 1, 1)
    cols = []
    for k in range(cand.shape[1]):
        win = data.preprocess_augmented(images, labels, crop, cand[:, k], lut=lut)[1]
        cols.append((win == cls).sum((1, 2)))
    return torch.stack(cols, dim=1).cpu().numpy()


@pytest.mark.parametrize("source", [(37, 83), (64, 128), (300, 517)])
@pytest.mark.parametrize("crop", [(48, 32), (130, 70)])
def test_crop_class_count_matches_the_restatement_and_the_pipeline(source, crop):
    from adaptsegnet_amd import rcs
    in_h, in_w = source
    cw, ch = crop
    hand = _hand_candidates(in_h, in_w, cw, ch)
    ids_all = _ids(3, in_h, in_w, seed=in_h + cw)
    lut, lut_np = _lut_dev(), _lut_np()
    classes_all = [0, 13, 5]                                     # road, car, pole: another class per sample
    nonzero = 0
    for n in (1, 3):
        ids = ids_all[:n]
        labels = torch.from_numpy(ids).to(DEV)
        images = torch.zeros((n, in_h, in_w, 3), dtype=torch.uint8, device=DEV)
        for K in (1, 10, 16):
            # sample i starts at hand[5 i], so K = 1 is not always the identity
            cand = np.stack([np.roll(hand, -5 * i, axis=0)[:K] for i in range(n)])
            classes = classes_all[:n]
            got = rcs.crop_class_count(labels, classes, cand, crop, lut)
            assert got.dtype == torch.int64 and tuple(got.shape) == (n, K) and got.is_cuda
            got = got.cpu().numpy()
            np.testing.assert_array_equal(got, RR.crop_counts(ids, classes, cand, ch, cw, lut_np))
            np.testing.assert_array_equal(got, _pipeline_counts(images, labels, crop, cand, classes, lut))
            nonzero += int((got > 0).sum())
            if K == 16:
                assert got[0, 6] == 0 and got[0, 7] == 0         # the windows wholly outside
    assert nonzero > 20
    # a class absent from the image (trainId 18: no id 33 anywhere): all zeros
    labels = torch.from_numpy(ids_all[:1]).to(DEV)
    got = rcs.crop_class_count(labels, [18], hand[None], crop, lut).cpu().numpy()
    assert (RR.crop_counts(ids_all[:1], [18], hand[None], ch, cw, lut_np) == 0).all() and (got == 0).all()


@pytest.mark.parametrize("source", [(37, 83), (64, 128)])
def test_crop_class_count_one_class_image_counts_the_window_inside(source):
    from adaptsegnet_amd import rcs
    in_h, in_w = source
    cw, ch = 48, 32
    hand = _hand_candidates(in_h, in_w, cw, ch)
    ids = np.full((2, in_h, in_w), 26, np.uint8)                 # all car
    labels = torch.from_numpy(ids).to(DEV)
    cand = np.stack([hand, hand[::-1]])
    got = rcs.crop_class_count(labels, torch.tensor([13, 13], device=DEV), cand, (cw, ch), _lut_dev()).cpu().numpy()
    # the number of window pixels inside the scaled image: the multiplicity sums, whatever the walk
    sw, sh, ox, oy = (cand[..., j].astype(np.int64) for j in range(4))
    inside_x = np.clip(np.minimum(cw, sw - ox) - np.maximum(0, -ox), 0, None)
    inside_y = np.clip(np.minimum(ch, sh - oy) - np.maximum(0, -oy), 0, None)
    np.testing.assert_array_equal(got, inside_x * inside_y)
    np.testing.assert_array_equal(got, RR.crop_counts(ids, [13, 13], cand, ch, cw, _lut_np()))
    other = rcs.crop_class_count(labels, [13, 0], cand, (cw, ch), _lut_dev()).cpu().numpy()
    np.testing.assert_array_equal(other[0], got[0])
    assert (other[1] == 0).all()


def test_crop_class_count_without_a_table_and_on_an_unaligned_buffer():
    from adaptsegnet_amd import rcs
    in_h, in_w, cw, ch = 37, 83, 48, 32
    hand = _hand_candidates(in_h, in_w, cw, ch)
    ids = (_ids(2, in_h, in_w, seed=9) % 21).astype(np.uint8)    # trainIds, a few of them outside 0..18
    cand = np.stack([hand, np.roll(hand, 3, axis=0)])
    classes = [2, 17]
    want = RR.crop_counts(ids, classes, cand, ch, cw, None)
    identity = torch.arange(256, dtype=torch.int32, device=DEV)
    images = torch.zeros((2, in_h, in_w, 3), dtype=torch.uint8, device=DEV)
    for shift in (0, 1, 7, 15):                                  # the label buffer's first byte past a 16-byte line
        store = torch.zeros(2 * in_h * in_w + 64, dtype=torch.uint8, device=DEV)
        labels = store[shift:shift + 2 * in_h * in_w].view(2, in_h, in_w)
        labels.copy_(torch.from_numpy(ids))
        assert labels.data_ptr() % 16 == shift and labels.is_contiguous()
        got = rcs.crop_class_count(labels, classes, cand, (cw, ch), None).cpu().numpy()
        np.testing.assert_array_equal(got, want)
        np.testing.assert_array_equal(rcs.label_class_count(labels, 19, None).cpu().numpy(),
                                      RR.class_counts(ids, 19, None))
    np.testing.assert_array_equal(want, _pipeline_counts(images, labels, (cw, ch), cand, classes, identity))
    assert want.sum() > 0


def test_crop_class_count_at_the_workload_geometry():
    from adaptsegnet_amd import data, rcs
    n, in_h, in_w, crop, K = 2, 1052, 1914, (1024, 512), 10
    ids = _ids(n, in_h, in_w, seed=1)
    cand = data.AugmentSampler(crop, seed=7).sample(n * K).reshape(n, K, 5)
    classes = [13, 0]
    labels = torch.from_numpy(ids).to(DEV)
    images = torch.zeros((n, in_h, in_w, 3), dtype=torch.uint8, device=DEV)
    got = rcs.crop_class_count(labels, classes, cand, crop, _lut_dev()).cpu().numpy()
    np.testing.assert_array_equal(got, RR.crop_counts(ids, classes, cand, crop[1], crop[0], _lut_np()))
    np.testing.assert_array_equal(got, _pipeline_counts(images, labels, crop, cand, classes, _lut_dev()))
    assert (got > 0).all()


# ---- C. choose_crops, RcsCrop --------------------------------------------------------------------------
def test_choose_crops_takes_the_first_passing_candidate_else_the_last():
    from adaptsegnet_amd import rcs
    in_h, in_w, cw, ch = 64, 128, 48, 32
    ids = np.full((2, in_h, in_w), 7, np.uint8)
    ids[0, :, 64:] = 8                       # sample 0: sidewalk on the right half only
    ids[1, 10:15, 20:25] = 11                # sample 1: 25 pixels of building
    classes = [1, 2]
    cand = np.array([[(in_w, in_h, 0, 0, 0), (in_w, in_h, 8, 16, 1), (in_w, in_h, 70, 20, 0), (in_w, in_h, 80, 32, 0)],
                     [(in_w, in_h, 0, 0, 0), (in_w, in_h, 10, 0, 1), (2 * in_w, 2 * in_h, 30, 10, 0),
                      (in_w, in_h, 80, 32, 1)]], np.int32)
    want = RR.crop_counts(ids, classes, cand, ch, cw, _lut_np())
    # the condition this test is about, on the restatement alone
    assert want[0, 0] <= 1000 < want[0, 1] and (want[0, 2:] > 1000).all()
    assert (want[1] <= 1000).all() and want[1].max() > 0
    params, chosen, counts = rcs.choose_crops(torch.from_numpy(ids).to(DEV), classes, cand, (cw, ch),
                                              min_crop_pixels=1000, lut=_lut_dev())
    np.testing.assert_array_equal(counts, want)
    np.testing.assert_array_equal(chosen, [1, 3])
    np.testing.assert_array_equal(chosen, RR.select(want, 1000))
    np.testing.assert_array_equal(params, cand[[0, 1], [1, 3]])
    assert params.dtype == np.int32 and chosen.dtype == np.int64 and isinstance(counts, np.ndarray)


def test_rcs_crop_params_give_a_window_with_the_reported_count():
    from adaptsegnet_amd import data, rcs
    n, in_h, in_w, crop, tries = 3, 64, 128, (48, 32), 10
    ids = _ids(n, in_h, in_w, seed=4)
    labels = torch.from_numpy(ids).to(DEV)
    images = torch.zeros((n, in_h, in_w, 3), dtype=torch.uint8, device=DEV)
    classes = [0, 13, 8]
    sampler, twin = data.AugmentSampler(crop, seed=3), data.AugmentSampler(crop, seed=3)
    params = rcs.RcsCrop(sampler, tries=tries, min_crop_pixels=150).params(labels, classes, _lut_dev())
    cand = twin.sample(n * tries).reshape(n, tries, 5)
    assert sampler.get_state() == twin.get_state()
    want_params, chosen, counts = rcs.choose_crops(labels, classes, cand, crop, 150, _lut_dev())
    np.testing.assert_array_equal(params, want_params)
    window = data.preprocess_augmented(images, labels, crop, params, lut=_lut_dev())[1]
    in_window = (window == torch.tensor(classes, device=DEV).view(-1, 1, 1)).sum((1, 2)).cpu().numpy()
    np.testing.assert_array_equal(in_window, counts[np.arange(n), chosen])
    np.testing.assert_array_equal(counts, RR.crop_counts(ids, classes, cand, crop[1], crop[0], _lut_np()))
