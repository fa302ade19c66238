"""``mix.strong_augment`` on the GPU: every case bit for bit against the float32 numpy restatement
(tests/strongaug_ref.py).

Inputs are uint8 values minus ``IMG_MEAN`` with planted grey, black, saturated and tied pixels.  Every
randomised case of at least two images asserts that the restatement itself went through what can go
wrong: the three ``mx ==`` branches, ``d == 0``, ``mx == 0``, the clamp's ends and a hue wrap in each
direction (``SR.STATS``).  One end cannot be reached from such inputs: contrast clamps at 0 only for a
negative ``u``, and ``u = (x + mean) / 255 >= 0`` for a uint8 minus the same mean with ``fc > 0``; the
non-default-mean case, where ``u`` does go negative, asserts that end.
"""
import functools
import itertools
import os
import sys

import numpy as np
import pytest
import torch

from oracle import reference_torch as R

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import strongaug_ref as SR  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
IDENTITY = dict(db=0.0, fc=1.0, fs=1.0, fh=0.0)
PLANTED = [(0, 0, 0), (128, 128, 128), (255, 255, 255), (17, 17, 17), (255, 0, 0), (0, 255, 0), (0, 0, 255),
           (255, 255, 0), (0, 255, 255), (255, 0, 255), (200, 200, 50), (200, 50, 200), (50, 200, 200), (90, 30, 30),
           (1, 0, 0), (254, 255, 255)]


def _input(n, h, w, seed, mean=SR.IMG_MEAN):
    """uint8 colours (random, with the planted ones spread over every image) minus the mean, float32 [n, 3, h, w]."""
    rng = np.random.Generator(np.random.PCG64(seed))
    u8 = rng.integers(0, 256, (n, 3, h, w), dtype=np.uint8)
    flat = u8.reshape(n, 3, h * w)
    pos = np.linspace(0, h * w - 1, num=min(len(PLANTED), h * w)).astype(int)
    for k, p in enumerate(pos):
        flat[:, :, p] = np.array(PLANTED[k], dtype=np.uint8)[None, :]
    return (u8.astype(np.float32) - np.asarray(mean, np.float32)[None, :, None, None]).astype(np.float32)


def _params(n, h, w, seed, jitter=True, radius=None, strength=0.2, **fixed):
    """Sampled parameters with the on/off decisions and radii fixed by the case; the signs of db, fc - 1 and fh
    alternate over the images (even: up, odd: down), so that two images reach both ends of every clamp and wrap."""
    from adaptsegnet_amd.mix import StrongAugSampler, blur_weights
    p = StrongAugSampler(seed=seed, strength=strength, p_jitter=1.0, p_blur=1.0).sample(n, 4096, 4096)
    sign = np.where(np.arange(n) % 2 == 0, 1.0, -1.0).astype(np.float32)
    p["db"] = np.abs(p["db"]) * sign
    p["fc"] = (1 + np.abs(p["fc"] - 1) * sign).astype(np.float32)
    p["fh"] = np.abs(p["fh"]) * sign
    for k, v in fixed.items():
        p[k] = np.full(n, v, dtype=np.float32) if np.ndim(v) == 0 else np.asarray(v)
    p["jitter"] = np.broadcast_to(np.asarray(jitter, dtype=bool), (n,)).copy()
    if radius is not None:
        p["radius"] = np.broadcast_to(np.asarray(radius, dtype=np.int32), (n,)).copy()
    p["radius"] = np.minimum(p["radius"], min(h, w) - 1).astype(np.int32)
    p["weights"] = np.stack([blur_weights(s, r) for s, r in zip(p["sigma"], p["radius"])])
    return p


def _gpu(x, params, mean=SR.IMG_MEAN, layout=None):
    from adaptsegnet_amd.mix import strong_augment
    t = torch.from_numpy(x).to(DEV)
    if layout == "channels_last":
        t = t.contiguous(memory_format=torch.channels_last)
    elif layout == "strided":
        big = torch.full((x.shape[0], 3, x.shape[2] + 3, x.shape[3] + 5), 7.0, device=DEV)
        big[:, :, 1:-2, 2:-3] = t
        t = big[:, :, 1:-2, 2:-3]
        assert not t.is_contiguous()
    out = strong_augment(t, params, mean)
    assert out.is_contiguous() and out.dtype == torch.float32 and tuple(out.shape) == x.shape
    assert out.data_ptr() != t.data_ptr()
    return out.cpu().numpy()


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.int32),
                                                 np.ascontiguousarray(b).view(np.int32))


def _assert_bits(got, ref, tag=""):
    if not _same_bits(got, ref):
        bad = np.argwhere(got.view(np.int32) != ref.view(np.int32))
        i = tuple(bad[0])
        raise AssertionError(f"{tag}: {len(bad)} of {got.size} elements differ, first at {i}: got {got[i]!r}, "
                             f"restatement {ref[i]!r}")


def _covered(stats, both_signs=True):
    need = ["max_r", "max_g", "max_b", "grey", "black", "contrast_hi"]
    need += ["bright_lo", "bright_hi", "wrap_up", "wrap_down"] if both_signs else []
    missing = [k for k in need if stats.get(k, 0) == 0]
    assert not missing, (missing, stats)


def _check(x, params, mean=SR.IMG_MEAN, tag="", cover=None):
    ref = SR.strong_augment(x, params, mean)
    stats = dict(SR.STATS)
    if cover is None:
        cover = x.shape[0] >= 2 and x.shape[2] * x.shape[3] >= 384 and bool(params["jitter"].all())
    if cover:
        _covered(stats)
    got = _gpu(x, params, mean)
    _assert_bits(got, ref, tag)
    return got, stats


# ---- shapes --------------------------------------------------------------------------------------------
SHAPES = [
    ((1, 3, 1, 1), 0),             # one pixel
    ((1, 3, 8, 8), 7),             # the reflection spans the whole image
    ((2, 3, 41, 57), 0),           # odd plane: the scalar per-pixel path
    ((2, 3, 40, 52), 0),           # the 16-byte per-pixel path
    ((2, 3, 41, 57), (3, 5)),      # tiles that end inside the image, two radii in one launch
    ((1, 3, 3, 4099), 2),          # a long thin image: 65 tiles in a row, the last one 3 columns wide
    ((2, 3, 33, 129), 7),          # one pixel past a tile multiple both ways: seams and borders together
    ((2, 3, 16, 24), (1, 7)),      # smaller than a tile
]


@pytest.mark.parametrize("shape,radius", SHAPES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_matches_the_numpy_restatement(shape, radius):
    n, _, h, w = shape
    x = _input(n, h, w, seed=h * 1000 + w)
    params = _params(n, h, w, seed=h + w, radius=radius)
    assert params["radius"].tolist() == np.broadcast_to(radius, (n,)).tolist()
    _check(x, params, tag=str(shape))
    if (h, w) == (3, 4099):   # one image, one sign: the other direction too
        for k in ("db", "fh"):
            params[k] = -params[k]
        params["fc"] = (2 - params["fc"]).astype(np.float32)
        _check(x, params, tag=f"{shape} down")


def test_jitter_off_with_a_blur_matches():
    x = _input(2, 33, 129, seed=21)
    _check(x, _params(2, 33, 129, seed=22, jitter=False, radius=(7, 4)), tag="blur only")


def test_all_24_orders():
    perms = np.array(list(itertools.permutations(range(4))), dtype=np.uint8)
    x = np.repeat(_input(1, 16, 24, seed=31), 24, axis=0)
    for sign in (1.0, -1.0):
        params = _params(24, 16, 24, seed=32, radius=0, db=0.15 * sign, fc=1 + 0.18 * sign, fs=1 - 0.17 * sign,
                         fh=0.12 * sign, order=perms)
        got, _ = _check(x, params, tag=f"orders {sign:+.0f}", cover=False)
        # the order matters: the 24 results are not one image
        assert len({got[i].tobytes() for i in range(24)}) > 12
    both = _params(24, 16, 24, seed=32, radius=0, fs=0.83, order=perms)   # alternating signs over the batch
    _check(x, both, tag="orders", cover=True)


@pytest.mark.parametrize("op", ["db", "fc", "fs", "fh"])
def test_each_op_alone(op):
    x = _input(4, 16, 24, seed=41)
    mag = {"db": (0.2, -0.2, 0.07, -0.01), "fc": (1.2, 0.8, 1.05, 0.99), "fs": (1.2, 0.8, 0.0, 1.0),
           "fh": (0.2, -0.2, 0.5, -1e-9)}[op]
    params = _params(4, 16, 24, seed=42, radius=0, **(IDENTITY | {op: np.array(mag, dtype=np.float32)}))
    got, stats = _check(x, params, tag=op, cover=False)
    if op == "db":
        assert stats["bright_lo"] and stats["bright_hi"]
    if op == "fc":
        assert stats["contrast_hi"]
    if op == "fh":
        assert stats["wrap_up"] and stats["wrap_down"]
    assert not _same_bits(got[0], got[1])


def test_a_batch_of_four_in_one_call():
    """neither, jitter only, blur only, both: one launch, checked per image."""
    x = _input(4, 40, 70, seed=51)
    params = _params(4, 40, 70, seed=52, jitter=[False, True, False, True], radius=[0, 0, 5, 6])
    got, _ = _check(x, params, tag="four", cover=False)
    assert _same_bits(got[0], x[0])                      # neither: the input's bits
    for i in range(4):
        one = {k: v[i:i + 1] for k, v in params.items()}
        _assert_bits(got[i:i + 1], SR.strong_augment(x[i:i + 1], one), f"image {i}")
        if i:
            assert not _same_bits(got[i], x[i])
    # a signed zero, a denormal and an infinity pass through "neither" untouched
    x[0, 0, 0, :3] = (-0.0, 1e-40, np.inf)
    assert _same_bits(_gpu(x, params)[0], x[0])


def test_non_default_mean():
    mean = np.array((110.5, 99.25, 131.0), dtype=np.float32)
    x = _input(2, 16, 24, seed=61)   # minus IMG_MEAN: with another mean u leaves [0, 1] on both sides
    params = _params(2, 16, 24, seed=62, radius=(0, 3), order=np.array([[1, 0, 2, 3], [2, 1, 3, 0]], np.uint8))
    ref_default = SR.strong_augment(x, params)
    got, stats = _check(x, params, mean=mean, tag="mean", cover=False)   # no black: u_b > 0 under this mean
    assert stats["contrast_lo"] > 0          # u < 0 reaches the contrast clamp's lower end
    assert all(stats[k] > 0 for k in ("contrast_hi", "bright_lo", "bright_hi", "max_r", "max_g", "max_b"))
    assert not _same_bits(got, ref_default)


@pytest.mark.parametrize("layout", ["channels_last", "strided"])
def test_layouts_give_the_contiguous_bits(layout):
    x = _input(2, 20, 36, seed=71)
    params = _params(2, 20, 36, seed=72, radius=(0, 4))
    assert _same_bits(_gpu(x, params, layout=layout), _gpu(x, params))


def test_mirror_commutes_and_repeats_are_identical():
    x = _input(2, 33, 70, seed=81)
    for jitter in (False, True):
        params = _params(2, 33, 70, seed=82, jitter=jitter, radius=(7, 3))
        out = _gpu(x, params)
        assert _same_bits(_gpu(np.ascontiguousarray(x[..., ::-1]), params), out[..., ::-1])
        assert _same_bits(_gpu(np.ascontiguousarray(x[:, :, ::-1]), params), out[:, :, ::-1])
        assert _same_bits(_gpu(x, params), out)


def test_input_is_left_alone_and_aliasing_is_refused():
    from adaptsegnet_amd.ops import OPS
    from adaptsegnet_amd import mix
    x = _input(1, 16, 24, seed=91)
    params = _params(1, 16, 24, seed=92, radius=2)
    t = torch.from_numpy(x).to(DEV)
    mix.strong_augment(t, params)
    assert _same_bits(t.cpu().numpy(), x)
    ctl, table = mix._aug_tables(params, 1, 16, 24)
    with pytest.raises(RuntimeError, match="images_in"):
        OPS.strong_augment(t, [float(v) for v in SR.IMG_MEAN], ctl, torch.from_numpy(table).to(DEV), t)


# ---- EmaTeacher.mix ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _teacher():
    from adaptsegnet_amd.mix import EmaTeacher
    from adaptsegnet_amd.model import DeeplabVGG
    state = R.det_state(R.vgg_specs(), 4242)
    m = DeeplabVGG(19)
    m.load_state_dict({k: torch.from_numpy(v.copy()) if v.dtype == np.int64 else torch.from_numpy(v.copy()).float()
                       for k, v in state.items()})
    return EmaTeacher(m.to(DEV), alpha=0.99)


def test_ema_teacher_mix_with_and_without_augment():
    from adaptsegnet_amd.mix import ClassMixSampler, StrongAugSampler, classmix, strong_augment
    ema = _teacher()
    n, h, w = 2, 41, 57
    xs = torch.from_numpy(_input(n, h, w, seed=101)).to(DEV)
    xt = torch.from_numpy(_input(n, h, w, seed=102)).to(DEV)
    lab = torch.from_numpy(R.det_labels((n, h, w), 12)).to(DEV)
    pred, conf = ema.predict(xt, (w, h))
    tau = float(conf.median())
    plain = classmix(xs, lab, xt, pred, conf, ClassMixSampler(seed=3).sample(n, 19), 19, tau, 255)
    # augment=None: today's path
    out = ema.mix(xs, lab, xt, ClassMixSampler(seed=3), tau=tau)
    assert len(out) == 3 and all(torch.equal(a, b) for a, b in zip(out, plain))
    out = ema.mix(xs, lab, xt, ClassMixSampler(seed=3), tau=tau, augment=None)
    assert all(torch.equal(a, b) for a, b in zip(out, plain))
    # a sampler: the images go through strong_augment with its next draw; labels and weights are untouched
    kw = dict(seed=4, p_jitter=1.0, p_blur=1.0)
    aug = ema.mix(xs, lab, xt, ClassMixSampler(seed=3), tau=tau, augment=StrongAugSampler(**kw))
    params = StrongAugSampler(**kw).sample(n, h, w)
    assert (params["radius"] > 0).all()
    want = strong_augment(plain[0], params)
    assert len(aug) == 3 and torch.equal(aug[0], want) and not torch.equal(aug[0], plain[0])
    assert torch.equal(aug[1], plain[1]) and torch.equal(aug[2], plain[2])
    _assert_bits(aug[0].cpu().numpy(), SR.strong_augment(plain[0].cpu().numpy(), params), "mix")
