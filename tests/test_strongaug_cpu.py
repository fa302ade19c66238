"""DACS's colour jitter and Gaussian blur (``mix.strong_augment``), host side (no GPU): the numpy restatement
(tests/strongaug_ref.py) against ``colorsys`` and ``scipy.ndimage`` in float64 and its exact properties in
float32, the parameter sampler, the op registration and the C ABI's argument checks.
"""
import colorsys
import ctypes
import itertools
import math
import os
import sys

import numpy as np
import pytest
import torch

from adaptsegnet_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import strongaug_ref as SR  # noqa: E402


# ---- the restatement against independent implementations (float64) ------------------------------------
def _colours():
    """[K, 3] float64 in [0, 1]: random colours, greys (d = 0), blacks (mx = 0), two-way ties, primaries."""
    rng = np.random.Generator(np.random.PCG64(1))
    rnd = rng.random((400, 3))
    g = rng.random(20)
    grey = np.stack([g, g, g], axis=1)
    black = np.zeros((2, 3))
    ties = []
    for hi, lo in ((0.8, 0.3), (0.3, 0.8), (1.0, 0.0), (0.0, 1.0), (0.5, 0.25)):
        ties += [(hi, hi, lo), (hi, lo, hi), (lo, hi, hi)]
    prim = list(itertools.product((0.0, 1.0), repeat=3))
    return np.concatenate([rnd, grey, black, np.array(ties), np.array(prim)])


def _hue_distance(a, b):
    d = np.abs(a - b)
    return np.minimum(d, 1.0 - d)


def test_hsv_round_trip_agrees_with_colorsys():
    c = _colours()
    h, s, v = SR.rgb_to_hsv(c[:, 0], c[:, 1], c[:, 2])
    assert h.dtype == np.float64
    ref = np.array([colorsys.rgb_to_hsv(*row) for row in c])
    assert np.abs(s - ref[:, 1]).max() <= 1e-12 and np.abs(v - ref[:, 2]).max() <= 1e-12
    assert _hue_distance(h, ref[:, 0]).max() <= 1e-12
    assert ((h >= 0) & (h <= 1)).all()
    back = np.stack(SR.hsv_to_rgb(h, s, v), axis=1)
    ref_back = np.array([colorsys.hsv_to_rgb(*row) for row in ref])
    assert np.abs(back - ref_back).max() <= 1e-12
    assert np.abs(back - c).max() <= 1e-12
    # every sector, from colorsys's own hsv triples
    hsv = np.random.Generator(np.random.PCG64(2)).random((300, 3))
    got = np.stack(SR.hsv_to_rgb(hsv[:, 0], hsv[:, 1], hsv[:, 2]), axis=1)
    assert np.abs(got - np.array([colorsys.hsv_to_rgb(*row) for row in hsv])).max() <= 1e-12
    assert set(np.floor(hsv[:, 0] * 6).astype(int)) == set(range(6))


def test_hue_of_exactly_one_is_hue_zero():
    """The restatement is total: h == 1 (reachable by rounding) takes sector 0 with f == 0."""
    for t in (np.float32, np.float64):
        one, s, v = np.array([1.0], dtype=t), np.array([0.75], dtype=t), np.array([0.5], dtype=t)
        at_one = SR.hsv_to_rgb(one, s, v)
        at_zero = SR.hsv_to_rgb(np.zeros(1, dtype=t), s, v)
        assert [float(x[0]) for x in at_one] == [float(x[0]) for x in at_zero] == [0.5, 0.125, 0.125]
    # a tiny negative hue shift of a pure red rounds h - floor(h) up to 1 in float32
    r, g, b = (np.array([x], dtype=np.float32) for x in (0.5, 0.125, 0.125))
    out = SR.op_hue(r, g, b, np.float32(-1e-9))
    assert [float(x[0]) for x in out] == [0.5, 0.125, 0.125]


@pytest.mark.parametrize("factor", [0.8, 1.0, 1.2, 0.0, 3.0])
def test_saturation_op_agrees_with_colorsys(factor):
    c = _colours()
    got = np.stack(SR.op_saturation(c[:, 0], c[:, 1], c[:, 2], np.float64(factor)), axis=1)
    ref = []
    for row in c:
        h, s, v = colorsys.rgb_to_hsv(*row)
        ref.append(colorsys.hsv_to_rgb(h, min(max(s * factor, 0.0), 1.0), v))
    assert np.abs(got - np.array(ref)).max() <= 1e-12


@pytest.mark.parametrize("shift", [-0.2, -0.05, 0.0, 0.05, 0.2])
def test_hue_op_agrees_with_colorsys(shift):
    c = _colours()
    got = np.stack(SR.op_hue(c[:, 0], c[:, 1], c[:, 2], np.float64(shift)), axis=1)
    ref = []
    for row in c:
        h, s, v = colorsys.rgb_to_hsv(*row)
        ref.append(colorsys.hsv_to_rgb((h + shift) % 1.0, s, v))
    assert np.abs(got - np.array(ref)).max() <= 1e-12


def test_brightness_and_contrast_are_add_and_multiply_with_a_clamp():
    c = _colours()
    for f in (-0.2, 0.2):
        got = np.stack(SR.op_brightness(c[:, 0], c[:, 1], c[:, 2], np.float64(f)), axis=1)
        assert np.array_equal(got, np.clip(c + f, 0.0, 1.0))
    for f in (0.8, 1.2):
        got = np.stack(SR.op_contrast(c[:, 0], c[:, 1], c[:, 2], np.float64(f)), axis=1)
        assert np.array_equal(got, np.clip(c * f, 0.0, 1.0))


def _full_kernel(w, radius):
    w = np.asarray(w, dtype=np.float64)
    return np.concatenate([w[radius:0:-1], w[:radius + 1]])


@pytest.mark.parametrize("radius,shape", [(1, (3, 5, 7)), (3, (3, 9, 6)), (7, (3, 8, 8)), (7, (3, 20, 33)), (2, (3, 3, 40))])
def test_blur_agrees_with_scipy_mirror_correlation(radius, shape):
    from scipy import ndimage
    from adaptsegnet_amd.mix import blur_weights
    x = np.random.Generator(np.random.PCG64(3)).uniform(-120, 140, shape)
    w = blur_weights(1.0, radius)
    k = _full_kernel(w, radius)
    for axis in (1, 2):
        got = SR.blur_axis(x, w.astype(np.float64), radius, axis)
        assert np.abs(got - ndimage.correlate1d(x, k, axis=axis, mode="mirror")).max() <= 1e-12 * 140
    both = ndimage.correlate1d(ndimage.correlate1d(x, k, axis=2, mode="mirror"), k, axis=1, mode="mirror")
    assert np.abs(SR.blur(x, w, radius, np.float64) - both).max() <= 1e-12 * 140


# ---- exact properties of the float32 restatement ---------------------------------------------------------
def _images(n, h, w, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    return (rng.integers(0, 256, (n, 3, h, w)).astype(np.float32) - SR.IMG_MEAN[None, :, None, None]).astype(np.float32)


def test_float32_blur_commutes_with_a_mirror_bit_for_bit():
    from adaptsegnet_amd.mix import blur_weights
    x = _images(1, 13, 22, 4)[0]
    for radius, sigma in ((1, 0.3), (4, 0.9), (7, 1.15)):
        w = blur_weights(sigma, radius)
        a = SR.blur(x[..., ::-1], w, radius)
        b = SR.blur(x, w, radius)[..., ::-1]
        assert a.dtype == np.float32 and np.array_equal(a.view(np.int32), np.ascontiguousarray(b).view(np.int32))
        a = SR.blur(x[:, ::-1], w, radius)
        b = SR.blur(x, w, radius)[:, ::-1]
        assert np.array_equal(np.ascontiguousarray(a).view(np.int32), np.ascontiguousarray(b).view(np.int32))


def test_neither_returns_the_input_bits():
    x = _images(2, 5, 6, 5)
    x[0, 0, 0, 0], x[1, 2, 4, 5] = -0.0, np.float32(1e-40)   # a signed zero and a denormal survive a copy
    params = {"jitter": np.zeros(2, bool), "radius": np.zeros(2, np.int32), "db": np.zeros(2, np.float32),
              "fc": np.ones(2, np.float32), "fs": np.ones(2, np.float32), "fh": np.zeros(2, np.float32),
              "order": np.tile(np.arange(4, dtype=np.uint8), (2, 1)), "weights": np.zeros((2, 8), np.float32)}
    out = SR.strong_augment(x, params)
    assert out.dtype == np.float32 and np.array_equal(out.view(np.int32), x.view(np.int32))
    # ... while an identity jitter is a normalise / renormalise round trip, which is allowed to move bits
    params["jitter"][:] = True
    assert np.abs(SR.strong_augment(x, params) - x).max() < 1e-4


def test_blur_radius_must_fit_the_image():
    with pytest.raises(ValueError, match="radius"):
        SR.blur(np.zeros((3, 4, 9), np.float32), np.ones(8, np.float32), 4)


# ---- the sampler ------------------------------------------------------------------------------------------
def _rule(sigma, h, w):
    return min(math.ceil(6 * sigma), (math.ceil(0.1 * min(h, w)) - 1) // 2)


def test_sampler_fields_rates_and_orders():
    from adaptsegnet_amd.mix import StrongAugSampler
    n = 4000
    p = StrongAugSampler(seed=7).sample(n, 512, 1024)
    assert p["jitter"].dtype == np.bool_ and p["jitter"].shape == (n,)
    for k in ("db", "fc", "fs", "fh"):
        assert p[k].dtype == np.float32 and p[k].shape == (n,)
    assert np.abs(p["db"]).max() <= 0.2 and np.abs(p["fh"]).max() <= 0.2
    assert np.abs(p["fc"].astype(np.float64) - 1).max() <= 0.2 + 2.0 ** -24
    assert np.abs(p["fs"].astype(np.float64) - 1).max() <= 0.2 + 2.0 ** -24
    for k in ("db", "fc", "fs", "fh"):   # ... and spread over the range, not stuck in a part of it
        v = p[k].astype(np.float64) - (1 if k in ("fc", "fs") else 0)
        assert v.min() < -0.19 and v.max() > 0.19 and abs(v.mean()) < 4 * 0.2 / math.sqrt(3 * n)
    assert ((p["sigma"] >= 0.15) & (p["sigma"] <= 1.15)).all() and p["sigma"].min() < 0.2 and p["sigma"].max() > 1.1
    for flags, prob in ((p["jitter"], 0.8), (p["radius"] > 0, 0.5)):
        se = math.sqrt(prob * (1 - prob) / n)
        assert abs(flags.mean() - prob) <= 4 * se, (flags.mean(), prob)
    assert p["order"].dtype == np.uint8 and p["order"].shape == (n, 4)
    assert (np.sort(p["order"], axis=1) == np.arange(4)).all()
    assert len({tuple(o) for o in p["order"].tolist()}) == 24
    # custom probabilities and strength
    q = StrongAugSampler(seed=7, strength=0.05, p_jitter=0.0, p_blur=1.0).sample(200, 512, 1024)
    assert not q["jitter"].any() and (q["radius"] > 0).all() and np.abs(q["db"]).max() <= 0.05


def test_sampler_radius_rule_and_weights():
    from adaptsegnet_amd.mix import StrongAugSampler, blur_radius, blur_weights
    assert _lib.BLUR_MAX_RADIUS == 7
    for h, w in ((512, 1024), (8, 8), (35, 35), (35, 400), (141, 141), (64, 50)):
        p = StrongAugSampler(seed=8, p_blur=1.0).sample(300, h, w)
        rad = p["radius"]
        assert rad.dtype == np.int32
        assert rad.tolist() == [_rule(s, h, w) for s in p["sigma"]]
        assert rad.max() <= min(7, min(h, w) - 1)
        if (h, w) == (8, 8):
            assert (rad == 0).all()
        if min(h, w) == 35:
            assert rad.max() <= 1 and rad.max() == 1
        if (h, w) == (512, 1024):
            assert rad.max() == 7 and rad.min() == 1   # ceil(6 * 1.15) = 7, ceil(6 * 0.15) = 1
        wt = p["weights"]
        assert wt.dtype == np.float32 and wt.shape == (300, 8)
        for i in range(300):
            r = int(rad[i])
            assert (wt[i, r + 1:] == 0).all() and (wt[i, :r + 1] > 0).all()
            total = float(wt[i, 0]) + 2.0 * float(wt[i, 1:].astype(np.float64).sum())
            assert abs(total - 1.0) <= 8 * 2.0 ** -24
            assert (np.diff(wt[i, :r + 1]) < 0).all() or r == 0
    p = StrongAugSampler(seed=8, p_blur=0.0).sample(5, 512, 1024)
    assert (p["radius"] == 0).all() and (p["weights"][:, 0] == 1).all() and (p["weights"][:, 1:] == 0).all()
    # the trim to ceil(6 sigma): the mass it drops is far below fp32's 2^-24 of the sum
    for sigma in (0.15, 0.4, 1.0, 1.15):
        r = math.ceil(6 * sigma)
        d = np.arange(r + 1, 60, dtype=np.float64)
        dropped = 2 * np.exp(-d * d / (2 * sigma * sigma)).sum()
        assert dropped < 2.0 ** -24 and blur_radius(sigma, 4096, 4096) == r <= 7
    assert blur_weights(0.5, 0).tolist() == [1.0] + [0.0] * 7


def test_sampler_is_deterministic_resumable_and_decision_free():
    from adaptsegnet_amd.mix import StrongAugSampler

    def same(a, b):
        return all(np.array_equal(a[k], b[k]) for k in a)
    a, b = StrongAugSampler(seed=5), StrongAugSampler(seed=5)
    pa = a.sample(3, 64, 96)
    assert same(pa, b.sample(3, 64, 96))
    assert not same(pa, StrongAugSampler(seed=6).sample(3, 64, 96))
    assert not same(pa, StrongAugSampler(seed=5, rank=1).sample(3, 64, 96))
    state = a.get_state()
    nxt = a.sample(2, 64, 96)
    c = StrongAugSampler(seed=99)
    c.set_state(state)
    assert same(c.sample(2, 64, 96), nxt)
    # the stream position after sample() depends on n alone: not on the probabilities, not on the image size
    ends = []
    for kw, (h, w) in ((dict(), (64, 96)), (dict(p_jitter=0.0, p_blur=0.0), (64, 96)), (dict(p_jitter=1.0, p_blur=1.0), (8, 8))):
        s = StrongAugSampler(seed=5, **kw)
        s.sample(3, h, w)
        ends.append(s.get_state()["state"])
        assert same(s.sample(2, 64, 96), nxt) or kw   # the default continues as `a` did
    assert ends[0] == ends[1] == ends[2] == state["state"]
    for bad in (dict(strength=1.0), dict(strength=-0.1), dict(p_jitter=1.5), dict(p_blur=-0.1), dict(sigma=(0.0, 1.0)),
                dict(sigma=(1.0, 0.5))):
        with pytest.raises(ValueError):
            StrongAugSampler(**bad)


# ---- registration and the C ABI -------------------------------------------------------------------------------
def test_op_is_registered_in_a_list_of_its_own():
    from adaptsegnet_amd import ops
    assert ops.AUG_NAMES == ["strong_augment"]
    assert "strong_augment" not in set(ops.NAMES) | set(ops.LOSS_NAMES) | set(ops.MIX_NAMES)
    op = torch.ops.adaptseg.strong_augment.default
    assert torch._C._dispatch_has_kernel_for_dispatch_key(op.name(), "CUDA")
    assert not torch._C._dispatch_has_kernel_for_dispatch_key(op.name(), "CPU")
    schema = op._schema
    assert len(schema.returns) == 0
    assert any(a.alias_info is not None and a.alias_info.is_write for a in schema.arguments)
    assert ops.OPS.strong_augment is op


def test_entry_point_is_declared_and_exported():
    s = "adaptseg_strong_augment"
    assert s in _lib.header_symbols() and s in _lib._SIGS and hasattr(_lib.lib(), s)
    assert f"#define ADAPTSEG_BLUR_MAX_RADIUS {_lib.BLUR_MAX_RADIUS}" in open(_lib.HEADER_PATH).read()


def _code(order):
    return sum(int(o) << (2 * k) for k, o in enumerate(order))


def test_abi_argument_checks_run_on_the_host():
    L = _lib.lib()
    p = ctypes.c_void_p(256)   # never dereferenced: every call below is rejected before a launch
    err = lambda: L.adaptseg_last_error().decode()  # noqa: E731
    mean = (ctypes.c_float * 3)(104.0, 116.0, 122.0)

    def ctl(rows):
        return (ctypes.c_int32 * (4 * len(rows)))(*[v for r in rows for v in (r[0], r[1], r[2], 0)])
    good = ctl([(1, _code((0, 1, 2, 3)), 0), (0, _code((3, 1, 0, 2)), 3)])

    def call(n=2, h=8, w=8, c=good, **kw):
        a = dict(images_in=p, mean=mean, ctl=p, jitter=p, weights=p, images_out=ctypes.c_void_p(4096)) | kw
        return L.adaptseg_strong_augment(n, h, w, a["images_in"], a["mean"], c, a["ctl"], a["jitter"], a["weights"],
                                         a["images_out"], None)
    for shape in ((0, 8, 8), (-1, 8, 8), (2, 0, 8), (2, 8, -3)):
        assert call(*shape) == 1 and "strong_augment" in err(), shape
    assert call(1, 4096, 4096) == 1 and "2^24" in err()
    for k in ("images_in", "mean", "ctl", "jitter", "weights", "images_out"):
        assert call(**{k: None}) == 1 and "strong_augment" in err() and "null" in err(), k
    assert call(c=None) == 1 and "null" in err()
    assert call(images_out=p) == 1 and "strong_augment" in err() and "images_in" in err()   # in == out
    for r in (-1, 8, 100):
        assert call(c=ctl([(1, _code((0, 1, 2, 3)), 0), (1, _code((0, 1, 2, 3)), r)])) == 1
        assert "strong_augment" in err() and "image 1" in err() and "radius" in err(), r
    assert call(h=5, w=40, c=ctl([(0, _code((0, 1, 2, 3)), 5)] * 2)) == 1   # R > min(h, w) - 1
    assert "strong_augment" in err() and "radius 5" in err() and "min(h, w) - 1" in err()
    assert call(h=40, w=5, c=ctl([(0, _code((0, 1, 2, 3)), 4), (0, _code((0, 1, 2, 3)), 7)])) == 1 and "image 1" in err()
    for bad in (_code((0, 0, 1, 2)), _code((3, 3, 3, 3)), 0, 256 + _code((0, 1, 2, 3)), -1):
        assert call(c=ctl([(1, bad, 0), (1, _code((0, 1, 2, 3)), 0)])) == 1
        assert "strong_augment" in err() and "permutation" in err() and "image 0" in err(), bad


def test_python_surface_validates_before_any_launch():
    from adaptsegnet_amd import mix
    x = torch.zeros(2, 3, 8, 10)
    good = mix.StrongAugSampler(seed=1, p_blur=0.0).sample(2, 8, 10)
    with pytest.raises(NotImplementedError, match="adaptseg::strong_augment"):   # no CPU kernel, no fallback
        mix.strong_augment(x, good)
    with pytest.raises(RuntimeError, match="float32"):
        mix.strong_augment(x.double(), good)
    with pytest.raises(RuntimeError, match=r"\[N, 3, H, W\]"):
        mix.strong_augment(torch.zeros(2, 4, 8, 10), good)
    with pytest.raises(ValueError, match="mean"):
        mix.strong_augment(x, good, mean=(1.0, 2.0))

    def but(**kw):
        return {k: v.copy() for k, v in good.items()} | kw
    with pytest.raises(ValueError, match="radius"):
        mix.strong_augment(x, but(radius=np.array([0, 8], np.int32)))
    with pytest.raises(ValueError, match="radius"):   # 6 > min(H, W) - 1
        mix.strong_augment(torch.zeros(2, 3, 6, 10), but(radius=np.array([6, 0], np.int32)))
    with pytest.raises(ValueError, match="permutation"):
        mix.strong_augment(x, but(order=np.array([[0, 1, 2, 3], [0, 1, 1, 3]], np.uint8)))
    with pytest.raises(ValueError, match="finite"):
        mix.strong_augment(x, but(fc=np.array([1.0, np.nan], np.float32)))
    w = np.zeros((2, 8), np.float32)
    w[:, 0], w[1, 3] = 1.0, 0.1
    with pytest.raises(ValueError, match="beyond"):
        mix.strong_augment(x, but(weights=w))
    with pytest.raises(ValueError, match="expected"):
        mix.strong_augment(x, but(db=np.zeros(3, np.float32)))
    # the uploaded table: controls' bits, factors, half kernels, one after the other
    prm = mix.StrongAugSampler(seed=2, p_jitter=1.0, p_blur=1.0).sample(3, 64, 64)
    ctl, table = mix._aug_tables(prm, 3, 64, 64)
    assert table.dtype == np.float32 and table.shape == (48,) and len(ctl) == 12
    assert table[:12].view(np.int32).tolist() == ctl
    for i in range(3):
        assert ctl[4 * i:4 * i + 4] == [1, _code(prm["order"][i]), int(prm["radius"][i]), 0]
        assert table[12 + 4 * i:16 + 4 * i].tolist() == [prm[k][i] for k in ("db", "fc", "fs", "fh")]
        assert np.array_equal(table[24 + 8 * i:32 + 8 * i], prm["weights"][i])
