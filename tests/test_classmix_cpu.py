"""Online self-training (EMA teacher, ClassMix, pixel-weighted CE), host side (no GPU): the numpy
restatement's selection rule on hand-written cases, the key sampler, the trainer's configuration and
batch checks (raised before any launch), the op registration and the C ABI's argument checks.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from adaptsegnet_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import classmix_ref as CR  # noqa: E402

SYMS = ("adaptseg_ema", "adaptseg_ema_multi", "adaptseg_classmix_stats", "adaptseg_classmix_apply",
        "adaptseg_softmax_ce_pw_fwd", "adaptseg_softmax_ce_pw_bwd")
OPS = {"ema", "ema_multi", "classmix_stats", "classmix_apply", "softmax_ce_pw_fwd", "softmax_ce_pw_bwd"}


# ---- the selection rule ----------------------------------------------------------------------------
def _sel(count, keys):
    return CR.select(np.array(count, dtype=np.int32), np.array(keys, dtype=np.uint32)).tolist()


def test_selection_rule_on_hand_written_cases():
    assert _sel([0, 0, 0, 0], [3, 2, 1, 0]) == [0, 0, 0, 0]                 # k = 0: nothing
    assert _sel([0, 0, 7, 0], [3, 2, 4000000000, 0]) == [0, 0, 1, 0]         # k = 1: that class, whatever its key
    assert _sel([5, 1, 0, 9], [30, 10, 0, 20]) == [0, 1, 0, 1]               # k = 3 (odd): ceil(3 / 2) = 2 smallest keys
    assert _sel([5, 1, 2, 9], [30, 10, 40, 20]) == [0, 1, 0, 1]              # k = 4 (even): 2
    assert _sel([5, 1, 2, 9, 1], [30, 10, 40, 20, 5]) == [0, 1, 0, 1, 1]     # k = 5: 3
    # an absent class's key never counts, however small
    assert _sel([5, 0, 2, 9], [30, 0, 40, 20]) == [1, 0, 0, 1]
    # ties: the smaller class index first
    assert _sel([1, 1, 1, 1], [7, 7, 7, 7]) == [1, 1, 0, 0]
    assert _sel([1, 1, 1], [7, 7, 7]) == [1, 1, 0]
    assert _sel([1, 1, 1, 1], [9, 7, 7, 9]) == [0, 1, 1, 0]
    assert _sel([1, 1, 1, 1, 1], [9, 7, 7, 9, 9]) == [1, 1, 1, 0, 0]
    # keys are compared as unsigned 32-bit numbers
    assert _sel([1, 1], [0x80000000, 0x7fffffff]) == [0, 1]


def test_reference_on_a_tiny_batch():
    """One image, by hand: classes 0 and 2 present (of 3), keys pick class 2; tau counts 2 of 4 target pixels."""
    xs = np.arange(12, dtype=np.float32).reshape(1, 3, 2, 2)
    xt = -np.ones((1, 3, 2, 2), dtype=np.float32)
    ls = np.array([[[0, 2], [255, -1]]], dtype=np.int64)
    pred = np.array([[[1, 1], [7, 0]]], dtype=np.uint8)
    conf = np.array([[[0.5, 0.2], [np.nan, 0.5]]], dtype=np.float32)
    keys = np.array([[9, 0, 3]], dtype=np.uint32)
    mi, ml, mw, mask, count, nconf = CR.classmix(xs, ls, xt, pred, conf, keys, ncls=3, tau=0.5, ignore_label=255)
    assert count.tolist() == [[1, 0, 1]] and nconf.tolist() == [2] and mask.tolist() == [[0, 0, 1]]
    assert ml.tolist() == [[[1, 2], [255, 0]]]
    assert mw.tolist() == [[[0.5, 1.0], [0.5, 0.5]]] and mw.dtype == np.float32
    assert mi[0, :, 0, 1].tolist() == [1.0, 5.0, 9.0] and (np.delete(mi.reshape(3, 4), 1, axis=1) == -1).all()
    assert ml.dtype == np.int64 and mi.dtype == np.float32 and count.dtype == np.int32 and nconf.dtype == np.int32


# ---- the sampler -----------------------------------------------------------------------------------
def test_sampler_is_deterministic_and_resumable():
    from adaptsegnet_amd.mix import ClassMixSampler
    a, b = ClassMixSampler(seed=5), ClassMixSampler(seed=5)
    ka = a.sample(3, 19)
    assert ka.dtype == np.uint32 and ka.shape == (3, 19)
    assert np.array_equal(ka, b.sample(3, 19))
    assert not np.array_equal(ka, ClassMixSampler(seed=6).sample(3, 19))
    assert not np.array_equal(ka, ClassMixSampler(seed=5, rank=1).sample(3, 19))
    state = a.get_state()
    nxt = a.sample(2, 256)
    assert nxt.shape == (2, 256) and not np.array_equal(nxt[:, :19], ka[:2])
    c = ClassMixSampler(seed=99)
    c.set_state(state)
    assert np.array_equal(c.sample(2, 256), nxt)
    assert int(ClassMixSampler(seed=1).sample(64, 256).max()) > 1 << 31   # the whole uint32 range


# ---- the trainer -----------------------------------------------------------------------------------
class _NoModel(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))


def _make(warper=None, **cfg):
    from adaptsegnet_amd.train import AdaptSegTrainer, StepConfig
    return AdaptSegTrainer(_NoModel(), None, _NoModel(), StepConfig(**cfg), warper=warper)


def test_step_config_defaults_and_validation():
    from adaptsegnet_amd.train import StepConfig
    assert StepConfig().lambda_mix == 0.0
    with pytest.raises(ValueError, match="lambda_mix"):
        _make(lambda_mix=-0.5)
    with pytest.raises(ValueError, match="warper"):
        _make(warper=_NoModel(), lambda_mix=1.0)
    _make(warper=None, lambda_mix=1.0)
    from adaptsegnet_amd.train import AdaptSegTrainer
    AdaptSegTrainer(_NoModel(), None, None, StepConfig(level="source-only", lambda_mix=1.0))   # plain DACS


class _NoOpt:
    param_groups = [{"lr": 0.0}, {"lr": 0.0}]

    def zero_grad(self):
        raise AssertionError("a malformed batch must raise before the step touches anything")


def _stub_trainer(**cfg):
    """The trainer as tests/test_pseudo_cpu.py builds it: no models, the step's host logic only."""
    from adaptsegnet_amd import train
    tr = train.AdaptSegTrainer.__new__(train.AdaptSegTrainer)
    tr.cfg = train.StepConfig(input_size=(8, 4), input_size_target=(6, 5), **cfg)
    tr.model = tr.D1 = tr.D2 = tr.warper = None
    tr.pg, tr.world, tr._pending, tr._consts = None, 1, [], {}
    tr.opt, tr.opt_D1, tr.opt_D2 = _NoOpt(), None, None
    return tr


@pytest.mark.parametrize("level,lambda_st", [("single-level", 0.0), ("multi-level", 1.0), ("source-only", 0.0)])
def test_mixed_batches_are_checked_before_the_step(level, lambda_st):
    tr = _stub_trainer(level=level, lambda_mix=1.0, lambda_st=lambda_st)
    x, lab, xt = torch.zeros(2, 3, 4, 8), torch.zeros(2, 4, 8, dtype=torch.int64), torch.zeros(2, 3, 5, 6)
    lt = torch.zeros(2, 5, 6, dtype=torch.int64)
    head = (x, lab) if level == "source-only" else (x, lab, xt, lt) if lambda_st else (x, lab, xt)
    mi, ml, mw = torch.zeros(2, 3, 4, 8), torch.zeros(2, 4, 8, dtype=torch.int64), torch.zeros(2, 4, 8)
    with pytest.raises(ValueError, match="mixed_images, mixed_labels, mixed_weights"):
        tr._step_body(0, [head])
    with pytest.raises(ValueError, match="mixed_images, mixed_labels, mixed_weights"):
        tr._step_body(0, [head + (mi, ml)])
    with pytest.raises(ValueError, match=r"mixed_images is .*expected torch.float32 \(2, 3, 4, 8\)"):
        tr._step_body(0, [head + (torch.zeros(2, 3, 5, 6), ml, mw)])
    with pytest.raises(ValueError, match=r"mixed_images is torch.float64"):
        tr._step_body(0, [head + (mi.double(), ml, mw)])
    with pytest.raises(ValueError, match=r"mixed_labels is torch.int32"):
        tr._step_body(0, [head + (mi, ml.int(), mw)])
    with pytest.raises(ValueError, match=r"mixed_labels is .*expected torch.int64 \(2, 4, 8\)"):
        tr._step_body(0, [head + (mi, ml[:1], mw)])
    with pytest.raises(ValueError, match=r"mixed_weights is .*expected torch.float32 \(2, 4, 8\)"):
        tr._step_body(0, [head + (mi, ml, mw[:, :3])])
    with pytest.raises(ValueError, match="mixed_weights is ndarray"):
        tr._step_body(0, [head + (mi, ml, mw.numpy())])
    # the second sub-batch is checked before the first one runs
    with pytest.raises(ValueError, match="mixed_images, mixed_labels, mixed_weights"):
        tr._step_body(0, [head + (mi, ml, mw), head])


def test_lambda_mix_zero_keeps_the_batch_shapes():
    """With the default, a batch with three more elements is not a mixed batch: the self-training check sees 7."""
    tr = _stub_trainer(level="single-level", lambda_st=1.0)
    x, lab = torch.zeros(2, 3, 4, 8), torch.zeros(2, 4, 8, dtype=torch.int64)
    with pytest.raises(ValueError, match=r"\(images, labels, images_target, labels_target\); got 7"):
        tr._step_body(0, [(x, lab, x, lab, x, lab, torch.zeros(2, 4, 8))])


def test_module_functions_validate_on_the_host():
    from adaptsegnet_amd import mix
    from adaptsegnet_amd.functional import cross_entropy2d
    x, lab = torch.zeros(2, 3, 4, 8), torch.zeros(2, 4, 8, dtype=torch.int64)
    pred, conf = torch.zeros(2, 4, 8, dtype=torch.uint8), torch.zeros(2, 4, 8)
    keys = np.zeros((2, 19), dtype=np.uint32)
    for kw in (dict(num_classes=0), dict(num_classes=257), dict(ignore_label=256)):
        with pytest.raises(ValueError):
            mix.classmix(x, lab, x, pred, conf, keys, **kw)
    with pytest.raises(ValueError, match="sizes must agree"):
        mix.classmix(x, lab, torch.zeros(2, 3, 5, 6), pred, conf, keys)
    with pytest.raises(ValueError, match="keys"):
        mix.classmix(x, lab, x, pred, conf, keys[:, :18])
    with pytest.raises(ValueError, match="keys"):
        mix.classmix(x, lab, x, pred, conf, keys.astype(np.int64))
    for alpha in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="alpha"):
            mix.ema_update(torch.zeros(4), torch.zeros(4), alpha)
        with pytest.raises(ValueError, match="alpha"):
            mix.EmaTeacher(_NoModel(), alpha)
    with pytest.raises(ValueError, match="generator"):
        mix.EmaTeacher(_NoModel())
    with pytest.raises(NotImplementedError, match="adaptseg::ema"):   # no CPU kernel, no fallback
        mix.ema_update(torch.zeros(4), torch.zeros(4), 0.5)
    with pytest.raises(NotImplementedError, match="adaptseg::classmix_stats"):
        mix.classmix(x, lab, x, pred, conf, keys)
    logits = torch.zeros(2, 19, 4, 8)
    with pytest.raises(RuntimeError, match="HIP device only"):
        cross_entropy2d(logits, lab, pixel_weight=conf)


def test_teacher_is_frozen_and_in_eval_mode():
    from adaptsegnet_amd.mix import EmaTeacher
    from adaptsegnet_amd.model import DeeplabVGG
    t = DeeplabVGG(num_classes=19).train()
    ema = EmaTeacher(t, alpha=0.9)
    assert not t.training and not any(p.requires_grad for p in t.parameters())
    assert [ema.momentum(i) for i in (0, 1, 3)] == [0.0, 0.5, 0.75] and ema.momentum(10 ** 6) == 0.9
    sd = ema.state_dict()
    assert sd["alpha"] == 0.9 and set(sd["model"]) == set(t.state_dict())
    other = EmaTeacher(DeeplabVGG(num_classes=19), alpha=0.5)
    other.load_state_dict(sd)
    assert other.alpha == 0.9
    for k, v in other.teacher.state_dict().items():
        assert torch.equal(v, sd["model"][k]), k


# ---- registration and the C ABI ---------------------------------------------------------------------
def test_entry_points_are_declared_and_exported():
    for s in SYMS:
        assert s in _lib.header_symbols(), s
        assert s in _lib._SIGS, s
        assert hasattr(_lib.lib(), s), s
    text = open(_lib.HEADER_PATH).read()
    for name, v in (("ADAPTSEG_EMA_MAX_BLOCKS", _lib.EMA_MAX_BLOCKS), ("ADAPTSEG_EMA_CHUNK", _lib.EMA_CHUNK),
                    ("ADAPTSEG_CLASSMIX_MAX_BLOCKS", _lib.CLASSMIX_MAX_BLOCKS)):
        assert f"#define {name} {v}" in text, name


def test_ops_are_registered_beside_the_other_lists():
    from adaptsegnet_amd import ops
    assert set(ops.MIX_NAMES) == OPS and len(ops.MIX_NAMES) == len(OPS)
    assert not OPS & (set(ops.NAMES) | set(ops.LOSS_NAMES))   # the engine's and the loss terms' op sets are as they were
    for name in ops.MIX_NAMES:
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

    def stats(n, h, w, c, lab=p, conf=p, count=p, nconf=p):
        return L.adaptseg_classmix_stats(n, h, w, c, lab, conf, 0.968, count, nconf, None)

    def apply(n, h, w, c, ignore=255, **kw):
        a = dict(images_s=p, labels_s=p, images_t=p, pred_t=p, count=p, nconf=p, keys=p, mixed_images=p, mixed_labels=p,
                 mixed_weights=p, mask=p) | kw
        return L.adaptseg_classmix_apply(n, h, w, c, a["images_s"], a["labels_s"], a["images_t"], a["pred_t"],
                                         a["count"], a["nconf"], a["keys"], ignore, a["mixed_images"],
                                         a["mixed_labels"], a["mixed_weights"], a["mask"], None)
    for fn, name in ((stats, "classmix_stats"), (apply, "classmix_apply")):
        assert fn(2, 8, 8, 0) == 1 and name in err() and "ncls 0" in err()          # C = 0
        assert fn(2, 8, 8, 257) == 1 and name in err() and "ncls 257" in err()      # C = 257
        assert fn(1, 4096, 4096, 19) == 1 and name in err() and "2^24" in err()     # H * W = 2^24
        assert fn(1, 1 << 23, 2, 19) == 1 and "2^24" in err()
        assert fn(0, 8, 8, 19) == 1 and name in err()
        assert fn(1, 0, 8, 19) == 1 and fn(1, 8, -1, 19) == 1
    assert stats(2, 8, 8, 19, lab=None) == 1 and "null" in err()
    assert stats(2, 8, 8, 19, nconf=None) == 1
    assert apply(2, 8, 8, 19, ignore=256) == 1 and "ignore_label" in err()
    assert apply(2, 8, 8, 19, ignore=-1) == 1
    for k in ("images_s", "labels_s", "images_t", "pred_t", "count", "nconf", "keys", "mixed_images", "mixed_labels",
              "mixed_weights"):
        assert apply(2, 8, 8, 19, **{k: None}) == 1 and "null" in err(), k
    # EMA
    assert L.adaptseg_ema(-1, 0.5, p, p, None) == 1 and "ema" in err()
    assert L.adaptseg_ema(16, -0.25, p, p, None) == 1 and "alpha" in err()
    assert L.adaptseg_ema(16, 1.5, p, p, None) == 1 and "alpha" in err()
    assert L.adaptseg_ema(16, float("nan"), p, p, None) == 1 and "alpha" in err()
    assert L.adaptseg_ema(16, 0.5, None, p, None) == 1 and "null" in err()
    assert L.adaptseg_ema(16, 0.5, p, None, None) == 1
    assert L.adaptseg_ema(0, 0.5, None, None, None) == 0       # nothing to do: no launch
    assert L.adaptseg_ema(16, 1.0, p, p, None) == 0            # alpha = 1 leaves dst as it is: no launch
    ptrs, lens = (ctypes.c_void_p * 2)(256, 512), (ctypes.c_int64 * 2)(4, 8)
    assert L.adaptseg_ema_multi(-1, ptrs, ptrs, lens, 0.5, None) == 1 and "ema_multi" in err()
    assert L.adaptseg_ema_multi(2, None, ptrs, lens, 0.5, None) == 1 and "null" in err()
    assert L.adaptseg_ema_multi(2, ptrs, ptrs, None, 0.5, None) == 1
    assert L.adaptseg_ema_multi(2, ptrs, ptrs, lens, 2.0, None) == 1 and "alpha" in err()
    assert L.adaptseg_ema_multi(2, ptrs, ptrs, (ctypes.c_int64 * 2)(4, 1 << 31), 0.5, None) == 1 and "tensor 1" in err()
    assert L.adaptseg_ema_multi(2, ptrs, (ctypes.c_void_p * 2)(256, None), lens, 0.5, None) == 1 and "tensor 1" in err()
    assert L.adaptseg_ema_multi(0, None, None, None, 0.5, None) == 0
    assert L.adaptseg_ema_multi(2, ptrs, ptrs, lens, 1.0, None) == 0
    # pixel-weighted CE
    b = ctypes.c_size_t(0)
    assert L.adaptseg_ce_workspace_size(64, ctypes.byref(b)) == 0
    assert L.adaptseg_softmax_ce_pw_fwd(0, 19, p, p, 255, None, p, p, p, b.value, None) == 1 and "ce_pw_fwd" in err()
    assert L.adaptseg_softmax_ce_pw_fwd(64, 0, p, p, 255, None, p, p, p, b.value, None) == 1
    assert L.adaptseg_softmax_ce_pw_fwd(64, 19, p, p, 255, None, None, p, p, b.value, None) == 1 and "null" in err()
    assert L.adaptseg_softmax_ce_pw_fwd(64, 19, p, p, 255, None, p, p, None, 0, None) == 4 and "workspace" in err()
    assert L.adaptseg_softmax_ce_pw_bwd(64, 19, p, p, 255, None, None, p, p, p, 0, None) == 1 and "ce_pw_bwd" in err()
    assert L.adaptseg_softmax_ce_pw_bwd(-1, 19, p, p, 255, None, p, p, p, p, 0, None) == 1


def test_fake_tensor_tracing():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from adaptsegnet_amd import kernels as K
    with FakeTensorMode():
        x = torch.empty(2, 8, 10, 19, device="cuda")
        lab = torch.empty(2, 8, 10, dtype=torch.int64, device="cuda")
        pw = torch.empty(2, 8, 10, device="cuda")
        out = K.ce_fwd(x, lab, 255, None, pw)
        assert out.shape == (2,)
        assert K.ce_bwd(x, lab, out, torch.empty(1, device="cuda"), pixel_weight=pw).shape == x.shape
