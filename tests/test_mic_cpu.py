"""Masked image consistency (MIC), host side (no GPU): the numpy restatement's rules on hand-written cases, the
key sampler and its masked fraction, the trainer's configuration and batch checks (raised before any launch),
the Python surface's argument checks, the op registration and the C ABI's argument checks.
"""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

from adaptsegnet_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mic_ref as MR  # noqa: E402

SYMS = ("adaptseg_conf_count", "adaptseg_patch_mask")
OPS = ["conf_count", "patch_mask"]


# ---- the rule ----------------------------------------------------------------------------------------
def _case(n, h, w, patch, fill=7.0):
    gh, gw = MR.grid_of(h, w, patch)
    x = np.full((n, 3, h, w), fill, dtype=np.float32)
    pred = np.zeros((n, h, w), dtype=np.uint8)
    keys = np.zeros((n, gh, gw), dtype=np.uint32)
    return x, pred, keys


def test_threshold_is_floor_of_ratio_times_2_32():
    assert MR.threshold_of(0.0) == 0 and MR.threshold_of(1.0) == 1 << 32
    assert MR.threshold_of(0.5) == 1 << 31 and MR.threshold_of(0.25) == 1 << 30
    assert MR.threshold_of(0.7) == math.floor(0.7 * 2 ** 32) == 3006477107
    from adaptsegnet_amd.mix import mask_threshold
    for r in (0.0, 0.3, 0.5, 0.7, 1.0, 1e-12, 1 - 2 ** -40):
        assert mask_threshold(r) == MR.threshold_of(r)


def test_key_edges_and_the_two_end_ratios():
    x, pred, keys = _case(1, 4, 8, 4)
    thr = MR.threshold_of(0.7)
    keys[0, 0] = [thr - 1, thr]          # the left patch is masked, the right one is not
    nconf = np.array([32], dtype=np.int32)
    mi, ml, mw = MR.patch_mask(x, pred, nconf, keys, 4, thr)
    assert (mi[0, :, :, :4] == 0).all() and (mi[0, :, :, 4:] == 7).all()
    assert (ml == 0).all() and (mw == 1).all()          # labels and weights do not see the mask
    keys[:] = 0                                          # the smallest key
    assert (MR.patch_mask(x, pred, nconf, keys, 4, MR.threshold_of(0.0))[0] == 7).all()    # ratio 0: nothing
    keys[:] = 0xFFFFFFFF                                 # the largest key
    assert (MR.patch_mask(x, pred, nconf, keys, 4, MR.threshold_of(1.0))[0] == 0).all()    # ratio 1: everything
    assert (MR.patch_mask(x, pred, nconf, keys, 4, (1 << 32) - 1)[0] == 7).all()


def test_kept_pixels_are_copied_bit_for_bit_and_masked_ones_are_plus_zero():
    x, pred, keys = _case(1, 2, 4, 2)
    x[0, 0, 0] = np.array([0x7FC01234, 0x80000000, 0xFFC00001, 0x80000000], dtype=np.uint32).view(np.float32)
    keys[0, 0] = [5, 0]                   # threshold 1: the right patch is masked
    mi, _, _ = MR.patch_mask(x, pred, np.array([0], dtype=np.int32), keys, 2, 1)
    assert mi.view(np.uint32)[0, 0, 0].tolist() == [0x7FC01234, 0x80000000, 0, 0]


def test_ragged_grids_and_a_patch_larger_than_the_image():
    x, pred, keys = _case(1, 5, 7, 3)     # 2 x 3 cells, the last row 2 pixels high, the last column 1 wide
    assert keys.shape == (1, 2, 3)
    keys[0] = [[9, 9, 0], [0, 9, 9]]
    m = MR.pixel_mask(keys, 5, 7, 3, 1)[0]
    want = np.zeros((5, 7), dtype=bool)
    want[:3, 6] = True
    want[3:, :3] = True
    assert np.array_equal(m, want)
    x, pred, keys = _case(2, 5, 7, 64)    # a 1 x 1 grid: an image is masked as a whole
    assert keys.shape == (2, 1, 1)
    keys[1] = 1
    mi, _, _ = MR.patch_mask(x, pred, np.zeros(2, dtype=np.int32), keys, 64, 1)
    assert (mi[0] == 0).all() and (mi[1] == 7).all()


def test_weights_labels_and_the_confidence_count():
    x, pred, keys = _case(1, 6, 4, 2)
    conf = np.full((1, 6, 4), 0.9, dtype=np.float32)
    conf[0, 0] = [np.nan, 0.5, np.float32(0.8), np.nextafter(np.float32(0.8), np.float32(0))]
    conf[0, 5] = 0.1                      # an ignored row's pixels still count (or not) by their confidence
    pred[0, 0] = [0, 18, 19, 255]
    mi, ml, mw, nconf = MR.mask_patches(x, pred, conf, keys, patch=2, ratio=0.0, ncls=19, tau=0.8, ignore_label=250,
                                        ignore_top=1, ignore_bottom=2)
    assert nconf.tolist() == [24 - 3 - 4]   # the NaN, 0.5, one ulp below tau, and row 5
    assert ml[0, 0].tolist() == [0, 18, 250, 250] and ml.dtype == np.int64
    q = np.float32(17) / np.float32(24)
    assert mw.dtype == np.float32 and (mw[0, 0] == 0).all() and (mw[0, 4:] == 0).all() and (mw[0, 1:4] == q).all()
    for top, bottom in ((6, 0), (0, 6), (3, 3), (4, 5), (100, 0)):   # ignore_top + ignore_bottom >= H
        assert (MR.mask_patches(x, pred, conf, keys, 2, 0.0, 19, 0.8, 255, top, bottom)[2] == 0).all()
    assert (MR.mask_patches(x, pred, conf, keys, 2, 0.0, 19, 0.8, 255, 2, 3)[2][0, :, 0] == [0, 0, q, 0, 0, 0]).all()


# ---- the sampler -------------------------------------------------------------------------------------
def test_sampler_is_deterministic_and_resumable():
    from adaptsegnet_amd.mix import PatchMaskSampler
    a, b = PatchMaskSampler(seed=5), PatchMaskSampler(seed=5)
    assert (a.patch, a.ratio, a.threshold) == (64, 0.7, MR.threshold_of(0.7))
    ka = a.sample(3, 130, 258)
    assert ka.dtype == np.uint32 and ka.shape == (3, 3, 5)          # ceil(130 / 64), ceil(258 / 64)
    assert np.array_equal(ka, b.sample(3, 130, 258))
    assert not np.array_equal(ka, PatchMaskSampler(seed=6).sample(3, 130, 258))
    assert not np.array_equal(ka, PatchMaskSampler(seed=5, rank=1).sample(3, 130, 258))
    state = a.get_state()
    nxt = a.sample(2, 64, 128)
    assert nxt.shape == (2, 1, 2)
    c = PatchMaskSampler(seed=99)
    c.set_state(state)
    assert np.array_equal(c.sample(2, 64, 128), nxt)
    s = PatchMaskSampler(patch=5)
    assert s.sample(1, 41, 57).shape == (1, 9, 12) and s.sample(1, 40, 55).shape == (1, 8, 11)
    assert PatchMaskSampler(patch=1).sample(1, 3, 4).shape == (1, 3, 4)
    assert PatchMaskSampler(patch=100).sample(2, 3, 4).shape == (2, 1, 1)
    assert int(PatchMaskSampler(seed=1, patch=1).sample(1, 64, 64).max()) > 1 << 31   # the whole uint32 range


@pytest.mark.parametrize("ratio", [0.0, 0.3, 0.5, 0.7, 1.0])
def test_masked_fraction_follows_the_ratio(ratio):
    from adaptsegnet_amd.mix import PatchMaskSampler
    s = PatchMaskSampler(seed=1234, rank=0, patch=8, ratio=ratio)
    keys = s.sample(4, 512, 1024)
    assert keys.size == 32768
    frac = float((keys.astype(np.uint64) < np.uint64(s.threshold)).mean())
    sigma = math.sqrt(ratio * (1 - ratio) / keys.size)
    print(f"ratio {ratio}: masked fraction {frac:.5f}, |dev| {abs(frac - ratio):.5f}, 4 sigma {4 * sigma:.5f}")
    if ratio in (0.0, 1.0):
        assert frac == ratio
    else:
        assert abs(frac - ratio) <= 4 * sigma


# ---- the trainer -------------------------------------------------------------------------------------
class _NoModel(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))


def _make(warper=None, **cfg):
    from adaptsegnet_amd.train import AdaptSegTrainer, StepConfig
    return AdaptSegTrainer(_NoModel(), None, _NoModel(), StepConfig(**cfg), warper=warper)


def test_step_config_defaults_and_validation():
    from adaptsegnet_amd.train import AdaptSegTrainer, StepConfig
    assert StepConfig().lambda_mic == 0.0
    with pytest.raises(ValueError, match="lambda_mic"):
        _make(lambda_mic=-0.5)
    with pytest.raises(ValueError, match="lambda_mic > 0 with a warper"):
        _make(warper=_NoModel(), lambda_mic=1.0)
    _make(warper=None, lambda_mic=1.0)
    _make(warper=None, lambda_mic=1.0, lambda_mix=1.0, lambda_st=1.0, lambda_ent=1.0)
    AdaptSegTrainer(_NoModel(), None, None, StepConfig(level="source-only", lambda_mic=1.0))
    AdaptSegTrainer(_NoModel(), None, None, StepConfig(level="source-only", lambda_mic=1.0, lambda_mix=1.0))


class _NoOpt:
    param_groups = [{"lr": 0.0}, {"lr": 0.0}]

    def zero_grad(self):
        raise AssertionError("a malformed batch must raise before the step touches anything")


def _stub_trainer(**cfg):
    """The trainer as tests/test_classmix_cpu.py builds it: no models, the step's host logic only."""
    from adaptsegnet_amd import train
    tr = train.AdaptSegTrainer.__new__(train.AdaptSegTrainer)
    tr.cfg = train.StepConfig(input_size=(8, 4), input_size_target=(6, 5), **cfg)
    tr.model = tr.D1 = tr.D2 = tr.warper = None
    tr.pg, tr.world, tr._pending, tr._consts = None, 1, [], {}
    tr.opt, tr.opt_D1, tr.opt_D2 = _NoOpt(), None, None
    return tr


TRIPLE = "masked_images, masked_labels, masked_weights"


@pytest.mark.parametrize("lambda_mix", [0.0, 1.0], ids=["mic", "mix+mic"])
@pytest.mark.parametrize("level,lambda_st", [("single-level", 0.0), ("single-level", 1.0), ("multi-level", 0.0),
                                             ("multi-level", 1.0), ("source-only", 0.0)])
def test_masked_batches_are_checked_before_the_step(level, lambda_st, lambda_mix):
    tr = _stub_trainer(level=level, lambda_mic=1.0, lambda_st=lambda_st, lambda_mix=lambda_mix)
    x, lab, xt = torch.zeros(2, 3, 4, 8), torch.zeros(2, 4, 8, dtype=torch.int64), torch.zeros(2, 3, 5, 6)
    size = (4, 8) if level == "single-level" else (5, 6)      # what the target prediction is upsampled to
    lt = torch.zeros((2,) + size, dtype=torch.int64)
    head = (x, lab) if level == "source-only" else (x, lab, xt, lt) if lambda_st else (x, lab, xt)
    if lambda_mix:
        head += (torch.zeros(2, 3, 4, 8), torch.zeros(2, 4, 8, dtype=torch.int64), torch.zeros(2, 4, 8))
    mi, ml, mw = torch.zeros(2, 3, 5, 6), torch.zeros(2, 5, 6, dtype=torch.int64), torch.zeros(2, 5, 6)
    with pytest.raises(ValueError, match=TRIPLE):
        tr._step_body(0, [head])
    with pytest.raises(ValueError, match=TRIPLE):
        tr._step_body(0, [head + (mi, ml)])
    with pytest.raises(ValueError, match=TRIPLE):
        tr._step_body(0, [head + (mi, ml, mw, mw)])
    # a triple at input_size is not one at input_size_target
    with pytest.raises(ValueError, match=r"masked_images is .*expected torch.float32 \(2, 3, 5, 6\), at "
                                         r"input_size_target"):
        tr._step_body(0, [head + (torch.zeros(2, 3, 4, 8), ml, mw)])
    with pytest.raises(ValueError, match=r"masked_images is torch.float64"):
        tr._step_body(0, [head + (mi.double(), ml, mw)])
    with pytest.raises(ValueError, match=r"masked_labels is torch.int32"):
        tr._step_body(0, [head + (mi, ml.int(), mw)])
    with pytest.raises(ValueError, match=r"masked_labels is .*expected torch.int64 \(2, 5, 6\)"):
        tr._step_body(0, [head + (mi, ml[:1], mw)])
    with pytest.raises(ValueError, match=r"masked_weights is .*expected torch.float32 \(2, 5, 6\)"):
        tr._step_body(0, [head + (mi, ml, mw[:, :3])])
    with pytest.raises(ValueError, match="masked_weights is ndarray"):
        tr._step_body(0, [head + (mi, ml, mw.numpy())])
    if lambda_mix:   # the mixed triple in front of it is still checked, against input_size
        bad = head[:-3] + (torch.zeros(2, 3, 5, 6),) + head[-2:]
        with pytest.raises(ValueError, match=r"mixed_images is .*expected torch.float32 \(2, 3, 4, 8\), at input_size "):
            tr._step_body(0, [bad + (mi, ml, mw)])
    # the second sub-batch is checked before the first one runs
    with pytest.raises(ValueError, match=TRIPLE):
        tr._step_body(0, [head + (mi, ml, mw), head])
    # a well-formed batch gets past the checks, to the first thing the step touches
    with pytest.raises(AssertionError, match="before the step touches anything"):
        tr._step_body(0, [head + (mi, ml, mw)])


def test_lambda_mic_zero_keeps_the_batch_shapes():
    """With the default, three more elements are not a masked triple: the checks see too many elements."""
    x, lab = torch.zeros(2, 3, 4, 8), torch.zeros(2, 4, 8, dtype=torch.int64)
    trip = (x, lab, torch.zeros(2, 4, 8))
    tr = _stub_trainer(level="single-level", lambda_st=1.0)
    with pytest.raises(ValueError, match=r"\(images, labels, images_target, labels_target\); got 7"):
        tr._step_body(0, [(x, lab, x, lab) + trip])
    tr = _stub_trainer(level="single-level", lambda_mix=1.0)
    with pytest.raises(ValueError, match=r"lambda_mix > 0: every batch ends with \(mixed_images, mixed_labels, "
                                         r"mixed_weights\) after its 3 other elements; got 9"):
        tr._step_body(0, [(x, lab, x) + trip + trip])
    assert tr._extra_branches() == [("mixed", "lambda_mix", 1.0, (8, 4), "input_size")]
    assert _stub_trainer(level="single-level")._extra_branches() == []


# ---- the Python surface ---------------------------------------------------------------------------------
def test_sampler_validates_its_arguments():
    from adaptsegnet_amd.mix import PatchMaskSampler
    for patch in (0, -1, 2.5, True):
        with pytest.raises(ValueError, match="patch"):
            PatchMaskSampler(patch=patch)
    for ratio in (-0.1, 1.0001, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="ratio"):
            PatchMaskSampler(ratio=ratio)
    with pytest.raises(ValueError):
        PatchMaskSampler().sample(1, 0, 4)
    assert PatchMaskSampler(ratio=0).threshold == 0 and PatchMaskSampler(ratio=1).threshold == 1 << 32


def test_mask_patches_validates_on_the_host():
    from adaptsegnet_amd import mix
    x = torch.zeros(2, 3, 4, 8)
    pred, conf = torch.zeros(2, 4, 8, dtype=torch.uint8), torch.zeros(2, 4, 8)
    keys = np.zeros((2, 2, 4), dtype=np.uint32)
    ok = dict(patch=2)
    for kw in (dict(num_classes=0), dict(num_classes=257), dict(ignore_label=256), dict(ignore_label=-1),
               dict(patch=0), dict(patch=1.5), dict(ratio=-0.01), dict(ratio=1.5), dict(ratio=float("nan")),
               dict(ignore_top=-1), dict(ignore_bottom=-2), dict(ignore_top=1.5)):
        with pytest.raises(ValueError):
            mix.mask_patches(x, pred, conf, keys, **(ok | kw))
    with pytest.raises(RuntimeError, match="images_t"):
        mix.mask_patches(x[:, :2], pred, conf, keys, **ok)
    with pytest.raises(RuntimeError, match="images_t"):
        mix.mask_patches(x.double(), pred, conf, keys, **ok)
    with pytest.raises(ValueError, match="pred_t"):
        mix.mask_patches(x, pred.int(), conf, keys, **ok)
    with pytest.raises(ValueError, match="pred_t"):
        mix.mask_patches(x, pred[:, :3], conf, keys, **ok)
    with pytest.raises(ValueError, match="conf_t"):
        mix.mask_patches(x, pred, conf.double(), keys, **ok)
    with pytest.raises(ValueError, match="conf_t"):
        mix.mask_patches(x, pred, conf[:1], keys, **ok)
    with pytest.raises(ValueError, match="keys"):
        mix.mask_patches(x, pred, conf, keys[:, :1], **ok)
    with pytest.raises(ValueError, match="keys"):
        mix.mask_patches(x, pred, conf, keys.astype(np.int64), **ok)
    with pytest.raises(ValueError, match=r"keys.*\(2, 1, 1\)"):     # the default patch, 64: a 1 x 1 grid
        mix.mask_patches(x, pred, conf, keys)
    with pytest.raises(ValueError, match="keys"):
        mix.mask_patches(x, pred, conf, torch.zeros(2, 2, 4, dtype=torch.int64), **ok)
    for bad in (torch.zeros(2, dtype=torch.int64), torch.zeros(3, dtype=torch.int32), np.zeros(2, dtype=np.int32)):
        with pytest.raises(ValueError, match="nconf"):
            mix.mask_patches(x, pred, conf, keys, nconf=bad, **ok)
    with pytest.raises(ValueError, match="2\\^24"):
        mix.mask_patches(torch.zeros(1, 3, 4096, 4096), pred, conf, keys, **ok)
    # no CPU kernel, no fallback: a well-formed call reaches the ops
    with pytest.raises(NotImplementedError, match="adaptseg::conf_count"):
        mix.mask_patches(x, pred, conf, keys, **ok)
    with pytest.raises(NotImplementedError, match="adaptseg::patch_mask"):
        mix.mask_patches(x, pred, conf, keys, nconf=torch.zeros(2, dtype=torch.int32), **ok)


def test_teacher_mask_validates_on_the_host():
    from adaptsegnet_amd.mix import ClassMixSampler, EmaTeacher, PatchMaskSampler
    from adaptsegnet_amd.model import DeeplabVGG
    ema = EmaTeacher(DeeplabVGG(num_classes=19))
    x = torch.zeros(2, 3, 4, 8)
    teacher = (torch.zeros(2, 4, 8, dtype=torch.uint8), torch.zeros(2, 4, 8))
    with pytest.raises(ValueError, match="PatchMaskSampler"):
        ema.mask(x, ClassMixSampler(), teacher=teacher)
    with pytest.raises(RuntimeError, match="images_t"):
        ema.mask(x[0], PatchMaskSampler(), teacher=teacher)
    with pytest.raises(ValueError, match="pred_t"):
        ema.mask(x, PatchMaskSampler(), teacher=(teacher[0][:, :2], teacher[1]))
    with pytest.raises(ValueError, match="ignore_top"):
        ema.mask(x, PatchMaskSampler(), teacher=teacher, ignore_top=-3)
    sampler = PatchMaskSampler(patch=3)
    state = sampler.get_state()
    with pytest.raises(NotImplementedError, match="adaptseg::conf_count"):   # the sampler's patch reached the keys
        ema.mask(x, sampler, teacher=teacher)
    assert sampler.get_state() != state     # and one draw was taken


# ---- registration and the C ABI ---------------------------------------------------------------------
def test_entry_points_are_declared_and_exported():
    for s in SYMS:
        assert s in _lib.header_symbols(), s
        assert s in _lib._SIGS, s
        assert hasattr(_lib.lib(), s), s
    text = open(_lib.HEADER_PATH).read()
    assert f"#define ADAPTSEG_MIC_MAX_BLOCKS {_lib.MIC_MAX_BLOCKS}" in text
    assert f"#define ADAPTSEG_MIC_COUNT_MAX_BLOCKS {_lib.MIC_COUNT_MAX_BLOCKS}" in text
    assert set(_lib.header_symbols()) == set(_lib._SIGS)


def test_ops_are_registered_beside_the_other_lists():
    from adaptsegnet_amd import ops
    assert ops.MIC_NAMES == OPS
    others = set(ops.NAMES) | set(ops.LOSS_NAMES) | set(ops.MIX_NAMES) | set(ops.AUG_NAMES) | set(ops.FDA_NAMES)
    assert not set(OPS) & others       # the other op sets are as they were
    for name in ops.MIC_NAMES:
        op = getattr(torch.ops.adaptseg, name).default
        assert torch._C._dispatch_has_kernel_for_dispatch_key(op.name(), "CUDA"), name
        assert not torch._C._dispatch_has_kernel_for_dispatch_key(op.name(), "CPU"), name
        schema = op._schema
        assert len(schema.returns) == 0, name
        assert any(a.alias_info is not None and a.alias_info.is_write for a in schema.arguments), name
        assert getattr(ops.OPS, name) is op


def test_abi_argument_checks_run_on_the_host():
    L = _lib.lib()
    p = ctypes.c_void_p(256)   # never dereferenced: every call below is rejected before a launch
    err = lambda: L.adaptseg_last_error().decode()  # noqa: E731

    def count(n, h, w, conf=p, nconf=p):
        return L.adaptseg_conf_count(n, h, w, conf, 0.968, nconf, None)

    def mask(n, h, w, patch=64, threshold=1 << 31, ncls=19, ignore=255, top=0, bottom=0, **kw):
        a = dict(images_t=p, pred_t=p, nconf=p, keys=p, masked_images=p, labels=p, weights=p) | kw
        return L.adaptseg_patch_mask(n, h, w, patch, threshold, ncls, ignore, top, bottom, a["images_t"], a["pred_t"],
                                     a["nconf"], a["keys"], a["masked_images"], a["labels"], a["weights"], None)
    for fn, name in ((count, "conf_count"), (mask, "patch_mask")):
        assert fn(0, 8, 8) == 1 and name in err()
        assert fn(65536, 8, 8) == 1 and name in err() and "65535" in err()
        assert fn(1, 0, 8) == 1 and fn(1, 8, -1) == 1
        assert fn(1, 4096, 4096) == 1 and name in err() and "2^24" in err()     # H * W = 2^24
        assert fn(1, 1 << 23, 2) == 1 and "2^24" in err()
    assert count(2, 8, 8, conf=None) == 1 and "null" in err()
    assert count(2, 8, 8, nconf=None) == 1 and "null" in err()
    assert mask(2, 8, 8, patch=0) == 1 and "patch 0" in err()
    assert mask(2, 8, 8, patch=-4) == 1
    assert mask(2, 8, 8, threshold=-1) == 1 and "threshold" in err()
    assert mask(2, 8, 8, threshold=(1 << 32) + 1) == 1 and "threshold" in err()
    assert mask(2, 8, 8, ncls=0) == 1 and "num_classes 0" in err()
    assert mask(2, 8, 8, ncls=257) == 1 and "num_classes 257" in err()
    assert mask(2, 8, 8, ignore=256) == 1 and "ignore_label" in err()
    assert mask(2, 8, 8, ignore=-1) == 1
    assert mask(2, 8, 8, top=-1) == 1 and "ignore rows" in err()
    assert mask(2, 8, 8, bottom=-1) == 1 and "ignore rows" in err()
    for k in ("images_t", "pred_t", "nconf", "keys", "masked_images", "labels", "weights"):
        assert mask(2, 8, 8, **{k: None}) == 1 and "null" in err(), k


def test_fake_tensor_tracing():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from adaptsegnet_amd import mix
    from adaptsegnet_amd.ops import OPS as O
    with FakeTensorMode():
        x = torch.empty(2, 3, 40, 68, device="cuda")
        pred = torch.empty(2, 40, 68, dtype=torch.uint8, device="cuda")
        conf = torch.empty(2, 40, 68, device="cuda")
        keys = torch.empty(2, 7, 12, dtype=torch.int32, device="cuda")
        nconf = torch.empty(2, dtype=torch.int32, device="cuda")
        assert O.conf_count(conf, 0.968, nconf) is None
        out = (torch.empty_like(x), torch.empty(2, 40, 68, dtype=torch.int64, device="cuda"), torch.empty_like(conf))
        assert O.patch_mask(x, pred, nconf, keys, 6, 1 << 32, 19, 255, 1, 2, *out) is None
        mi, ml, mw = mix.mask_patches(x, pred, conf, keys, patch=6, ratio=0.7, ignore_top=1, ignore_bottom=2)
        assert mi.shape == x.shape and mi.dtype == torch.float32
        assert ml.shape == (2, 40, 68) and ml.dtype == torch.int64
        assert mw.shape == (2, 40, 68) and mw.dtype == torch.float32
        assert mix.mask_patches(x, pred, conf, keys, patch=6, nconf=nconf)[0].shape == x.shape
