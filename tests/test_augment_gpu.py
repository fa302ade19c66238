"""Random scale / crop / mirror augmentation on the GPU (data.preprocess_augmented) — bit-exact
against the CPU oracle composed here from oracle.reference_data.gta5_item:

  1. R = gta5_item(image, label, (sw, sh))     today's pipeline at the sample's own size;
  2. if mirror: flip R left-right, image and label alike (after the resize);
  3. out[:, y, x] = R[:, y + oy, x + ox] inside R; 0.0f (image) / ignore_label (label) elsewhere.

float32 bit patterns and int64 labels are compared exactly.  Label ids come from the 19 mapped
ids, so 255 appears only as padding, and the padded share of each label map must equal the
oracle's (a kernel that pads everything cannot pass).
"""
import numpy as np
import pytest
import torch

from oracle import reference_data as D

pytestmark = pytest.mark.gpu

IGNORE = 255
MAPPED = np.array(sorted(D.ID_TO_TRAINID), np.uint8)

# (source (H, W), crop (W, H), [(sw, sh, ox, oy, mirror), ...])
SMALL = ((37, 53), (48, 32), [(72, 48, 24, 16, 1),     # up-scale; window flush with the right/bottom edge
                              (24, 16, 0, 0, 0),       # scaled image smaller than the crop: pad right/bottom
                              (48, 32, 0, 0, 0),       # identity
                              (53, 37, -7, 3, 1)])     # negative offset pads left; bottom overhang
ODD = ((100, 130), (47, 33), [(24, 17, -5, -9, 1),     # strong down-scale, wide taps; pad on all four sides
                              (71, 50, 24, 17, 0),     # window flush with the right/bottom edge
                              (47, 33, 0, 0, 1)])      # pure mirror
SINGLE = [(hw, crop, p) for hw, crop, ps in (SMALL, ODD) for p in ps]


def _img(rng, h, w):
    """Natural-ish image: smooth ramps + noise + hard edges (exercises clamping)."""
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([(x * 255 // max(w - 1, 1)), (y * 255 // max(h - 1, 1)), ((x + y) % 256)], -1)
    noise = rng.integers(-40, 41, (h, w, 3))
    edges = ((x // 7 + y // 5) % 2) * 200
    return np.clip(base + noise + edges[..., None] - 100, 0, 255).astype(np.uint8)


def _source(hw, n, seed):
    rng = np.random.default_rng(seed)
    imgs = np.stack([_img(rng, *hw) for _ in range(n)])
    labs = MAPPED[rng.integers(0, len(MAPPED), (n,) + hw)]
    return imgs, labs


def oracle(img, lab, crop, p):
    """The three steps of the module docstring for one sample."""
    (cw, ch), (sw, sh, ox, oy, mirror) = crop, p
    image, label, _ = D.gta5_item(img, lab, (sw, sh))
    if mirror:
        image = image[:, :, ::-1]
        label = None if label is None else label[:, ::-1]
    out = np.zeros((3, ch, cw), np.float32)
    out_lab = np.full((ch, cw), IGNORE, np.int64)
    y0, y1 = max(0, -oy), min(ch, sh - oy)
    x0, x1 = max(0, -ox), min(cw, sw - ox)
    if y0 < y1 and x0 < x1:
        out[:, y0:y1, x0:x1] = image[:, y0 + oy:y1 + oy, x0 + ox:x1 + ox]
        if label is not None:
            out_lab[y0:y1, x0:x1] = label[y0 + oy:y1 + oy, x0 + ox:x1 + ox].astype(np.int64)
    return out, (out_lab if lab is not None else None)


def _run(imgs, labs, crop, params):
    from adaptsegnet_amd import data
    dev = torch.device("cuda", 0)
    image, label = data.preprocess_augmented(torch.from_numpy(imgs).to(dev),
                                             None if labs is None else torch.from_numpy(labs).to(dev),
                                             crop, np.asarray(params, np.int32))
    torch.cuda.synchronize()
    return image.cpu().numpy(), None if label is None else label.cpu().numpy()


def _check(imgs, labs, crop, params, image, label):
    for b, p in enumerate(params):
        ref_img, ref_lab = oracle(imgs[b], None if labs is None else labs[b], crop, p)
        got = image[b]
        assert got.dtype == np.float32 and got.shape == ref_img.shape
        assert np.array_equal(got.view(np.int32), ref_img.view(np.int32)), \
            f"sample {b} {p}: {int((got.view(np.int32) != ref_img.view(np.int32)).sum())} values differ"
        if labs is not None:
            assert label[b].dtype == np.int64
            pad, ref_pad = float((label[b] == IGNORE).mean()), float((ref_lab == IGNORE).mean())
            assert pad == ref_pad, f"sample {b} {p}: padded share {pad} != {ref_pad}"
            assert np.array_equal(label[b], ref_lab), f"sample {b} {p}"


@pytest.mark.parametrize("hw,crop,p", SINGLE)
def test_single_sample_bit_exact(hw, crop, p):
    imgs, labs = _source(hw, 1, 11)
    image, label = _run(imgs, labs, crop, [p])
    _check(imgs, labs, crop, [p], image, label)


@pytest.mark.parametrize("hw,crop,params", [SMALL, ODD])
def test_batch_with_per_sample_tables(hw, crop, params):
    imgs, labs = _source(hw, len(params), 12)
    image, label = _run(imgs, labs, crop, params)
    _check(imgs, labs, crop, params, image, label)


def test_identity_equals_preprocess():
    from adaptsegnet_amd import data
    hw, crop, _ = SMALL
    imgs, labs = _source(hw, 2, 13)
    dev = torch.device("cuda", 0)
    ti, tl = torch.from_numpy(imgs).to(dev), torch.from_numpy(labs).to(dev)
    want_i, want_l = data.preprocess(ti, tl, crop)
    got_i, got_l = data.preprocess_augmented(ti, tl, crop, np.array([[crop[0], crop[1], 0, 0, 0]] * 2, np.int32))
    assert torch.equal(got_i.view(torch.int32), want_i.view(torch.int32))
    assert torch.equal(got_l, want_l)


@pytest.mark.parametrize("p", [(72, 48, 72 + 3, 0, 0), (72, 48, 0, -40, 1), (24, 16, -60, 50, 1)])
def test_window_wholly_outside_is_all_padding(p):
    hw, crop, _ = SMALL
    imgs, labs = _source(hw, 1, 14)
    image, label = _run(imgs, labs, crop, [p])
    assert not image.view(np.int32).any() and (label == IGNORE).all()
    _check(imgs, labs, crop, [p], image, label)


def test_image_only_and_dataset_surface(tmp_path):
    from adaptsegnet_amd import data
    hw, crop, params = SMALL
    imgs, labs = _source(hw, len(params), 15)
    image, label = _run(imgs, None, crop, params)
    assert label is None
    _check(imgs, None, crop, params, image, None)
    (tmp_path / "list.txt").write_text("a.png\n")
    mean = tuple(float(v) for v in D.IMG_MEAN)
    city = data.cityscapesDataSet(str(tmp_path), str(tmp_path / "list.txt"), crop_size=crop, mean=mean)
    got = city.preprocess(imgs, augment=np.asarray(params, np.int32)).cpu().numpy()
    assert np.array_equal(got.view(np.int32), image.view(np.int32))
    gta = data.GTA5DataSet(str(tmp_path), str(tmp_path / "list.txt"), crop_size=crop, mean=mean)
    gi, gl = gta.preprocess(imgs, labs, augment=np.asarray(params, np.int32))
    _check(imgs, labs, crop, params, gi.cpu().numpy(), gl.cpu().numpy())
    pi, pl = gta.preprocess(imgs, labs)                      # augment=None: today's path
    wi, wl = data.preprocess(torch.from_numpy(imgs).cuda(), torch.from_numpy(labs).cuda(), crop, mean)
    assert torch.equal(pi.view(torch.int32), wi.view(torch.int32)) and torch.equal(pl, wl)


def test_malformed_params_raise_value_error():
    from adaptsegnet_amd import data
    hw, crop, _ = SMALL
    imgs, _ = _source(hw, 1, 16)
    img = torch.from_numpy(imgs).cuda()
    good = np.array([[48, 32, 0, 0, 0]], np.int32)
    for bad in (good[0], np.zeros((2, 5), np.int32), good.astype(np.float32), [[0, 32, 0, 0, 0]]):
        with pytest.raises(ValueError):
            data.preprocess_augmented(img, None, crop, bad)
    with pytest.raises(ValueError):
        data.preprocess_augmented(img.cpu(), None, crop, good)


def test_real_geometry():
    """GTA5's 1914x1052 at factor 1.5 of the (1280, 720) crop, a mid-image window, mirrored: the
    64-bit index arithmetic and the grid-stride loops only matter at this size."""
    hw, crop = (1052, 1914), (1280, 720)
    p = (1920, 1080, 317, 181, 1)
    imgs, labs = _source(hw, 1, 17)
    image, label = _run(imgs, labs, crop, [p])
    _check(imgs, labs, crop, [p], image, label)
