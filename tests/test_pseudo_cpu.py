"""Pseudo-labels and the self-training term, host side (no GPU): the three C-ABI entry points and
their host validation, the trainer's configuration and batch checks (raised before any launch),
and the two properties of the numpy restatement (tests/pseudo_ref.py) the GPU tests compare with.
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
import pseudo_ref as PR  # noqa: E402

SYMS = ("adaptseg_conf_hist", "adaptseg_pseudo_thresholds", "adaptseg_pseudo_label")


def test_entry_points_are_declared_and_exported():
    for s in SYMS:
        assert s in _lib.header_symbols(), s
        assert s in _lib._SIGS, s
        assert hasattr(_lib.lib(), s), s


def _ops_registered():
    from adaptsegnet_amd import ops
    return ops


def test_ops_are_registered():
    ops = _ops_registered()
    for name in ("conf_hist", "pseudo_thresholds", "pseudo_label"):
        assert name in ops.NAMES
    assert str(torch.ops.adaptseg.pseudo_label.default._schema) == (
        "adaptseg::pseudo_label(Tensor pred, Tensor conf, Tensor thr, int ignore_label, Tensor(a!) labels, "
        "Tensor(b!)? kept) -> ()")


# never dereferenced: every case below is rejected on the host
P = 4096


def _hist(L, npix=100, pred=P, conf=P, ncls=19, nbins=512, hist=P):
    return L.adaptseg_conf_hist(npix, pred, conf, ncls, nbins, hist, None)


def _thr(L, hist=P, ncls=19, nbins=512, portion=0.5, cap=0.9, thr=P):
    return L.adaptseg_pseudo_thresholds(hist, ncls, nbins, portion, cap, thr, None)


def _lab(L, npix=100, pred=P, conf=P, thr=P, ncls=19, ignore=255, labels=P, kept=None):
    return L.adaptseg_pseudo_label(npix, pred, conf, thr, ncls, ignore, labels, kept, None)


BAD = {
    "hist-null-pred": (_hist, dict(pred=None)),
    "hist-null-conf": (_hist, dict(conf=None)),
    "hist-null-hist": (_hist, dict(hist=None)),
    "hist-nbins-1": (_hist, dict(nbins=1)),
    "hist-nbins-0": (_hist, dict(nbins=0)),
    "hist-nbins-negative": (_hist, dict(nbins=-512)),
    "hist-nbins-500": (_hist, dict(nbins=500)),
    "hist-nbins-8192": (_hist, dict(nbins=8192)),
    "hist-ncls-0": (_hist, dict(ncls=0)),
    "hist-ncls-257": (_hist, dict(ncls=257)),
    "hist-npix-negative": (_hist, dict(npix=-1)),
    "thr-null-hist": (_thr, dict(hist=None)),
    "thr-null-thr": (_thr, dict(thr=None)),
    "thr-nbins-3": (_thr, dict(nbins=3)),
    "thr-nbins-8192": (_thr, dict(nbins=8192)),
    "thr-ncls-0": (_thr, dict(ncls=0)),
    "thr-ncls-257": (_thr, dict(ncls=257)),
    "thr-portion-0": (_thr, dict(portion=0.0)),
    "thr-portion-negative": (_thr, dict(portion=-0.5)),
    "thr-portion-above-1": (_thr, dict(portion=1.0000001)),
    "thr-portion-nan": (_thr, dict(portion=float("nan"))),
    "thr-cap-0": (_thr, dict(cap=0.0)),
    "thr-cap-above-1": (_thr, dict(cap=1.5)),
    "thr-cap-nan": (_thr, dict(cap=float("nan"))),
    "label-null-pred": (_lab, dict(pred=None)),
    "label-null-conf": (_lab, dict(conf=None)),
    "label-null-thr": (_lab, dict(thr=None)),
    "label-null-labels": (_lab, dict(labels=None)),
    "label-ncls-0": (_lab, dict(ncls=0)),
    "label-ncls-257": (_lab, dict(ncls=257)),
    "label-ignore-negative": (_lab, dict(ignore=-1)),
    "label-ignore-256": (_lab, dict(ignore=256)),
}


@pytest.mark.parametrize("case", sorted(BAD))
def test_host_validation_without_gpu(case):
    """Every bad argument is rejected before any launch: status 1 and a message that says so."""
    L = _lib.lib()
    fn, kw = BAD[case]
    assert L.adaptseg_timing_reserve(-1) == 1   # the thread's last error now speaks of something else
    assert fn(L, **kw) == 1, case
    err = L.adaptseg_last_error()
    name = {_hist: b"conf_hist", _thr: b"pseudo_thresholds", _lab: b"pseudo_label"}[fn]
    assert err.startswith(name + b": bad"), err


def test_no_pixels_is_ok_without_a_launch():
    L = _lib.lib()
    assert _hist(L, npix=0, pred=None, conf=None, hist=None) == 0
    assert _lab(L, npix=0, pred=None, conf=None, thr=None, labels=None) == 0


def test_python_argument_checks():
    from adaptsegnet_amd.pseudo import ConfidenceHistogram, pseudo_labels
    for kw in (dict(nbins=500), dict(nbins=1), dict(nbins=8192), dict(num_classes=0), dict(num_classes=257)):
        with pytest.raises(ValueError):
            ConfidenceHistogram(device="cpu", **kw)
    h = ConfidenceHistogram(19, 512, device="cpu")
    assert h.hist.shape == (19, 512) and h.hist.dtype == torch.int64
    pred, conf = torch.zeros(4, 6, dtype=torch.uint8), torch.zeros(4, 6)
    with pytest.raises(RuntimeError, match="uint8"):
        h.update(pred.long(), conf)
    with pytest.raises(RuntimeError, match="float32"):
        h.update(pred, conf.double())
    with pytest.raises(RuntimeError, match="24 predictions vs 12"):
        h.update(pred, conf[:2])
    for kw in (dict(portion=0.0), dict(portion=1.5), dict(cap=0.0), dict(cap=1.01)):
        with pytest.raises(ValueError):
            h.thresholds(**kw)
    h.all_reduce()   # no process group: a no-op
    h.reset()
    thr = torch.full((19,), 0.5)
    with pytest.raises(RuntimeError, match="uint8"):
        pseudo_labels(pred.int(), conf, thr)
    with pytest.raises(RuntimeError, match="predictions vs"):
        pseudo_labels(pred, conf[:1], thr)
    with pytest.raises(RuntimeError, match="thresholds"):
        pseudo_labels(pred, conf, thr.double())
    with pytest.raises(ValueError, match="ignore_label"):
        pseudo_labels(pred, conf, thr, ignore_label=256)
    with pytest.raises(NotImplementedError, match="adaptseg::pseudo_label"):   # no CPU kernel, no fallback
        pseudo_labels(pred, conf, thr)


# ---- the trainer -----------------------------------------------------------------------------
def test_lambda_st_defaults_to_zero():
    from adaptsegnet_amd.train import StepConfig
    assert StepConfig().lambda_st == 0.0


def test_cross_entropy_reductions():
    from adaptsegnet_amd.functional import cross_entropy2d
    with pytest.raises(ValueError, match="mean_or_zero"):
        cross_entropy2d(torch.zeros(1, 19, 2, 2), torch.zeros(1, 2, 2, dtype=torch.int64), reduction="none")


def test_source_only_has_no_self_training_term():
    from adaptsegnet_amd.model import DeeplabMulti
    from adaptsegnet_amd.train import AdaptSegTrainer, StepConfig
    with pytest.raises(ValueError, match="lambda_st"):
        AdaptSegTrainer(DeeplabMulti(num_classes=19), None, None, StepConfig(level="source-only", lambda_st=1.0))
    with pytest.raises(ValueError, match="lambda_st"):
        AdaptSegTrainer(DeeplabMulti(num_classes=19), None, None, StepConfig(level="source-only", lambda_st=-1.0))


class _NoOpt:
    param_groups = [{"lr": 0.0}, {"lr": 0.0}]

    def zero_grad(self):
        raise AssertionError("a malformed batch must raise before the step touches anything")


def _stub_trainer(**cfg):
    """The trainer as tests/test_dist_stub_cpu.py builds it: no models, the step's host logic only."""
    from adaptsegnet_amd import train
    tr = train.AdaptSegTrainer.__new__(train.AdaptSegTrainer)
    tr.cfg = train.StepConfig(input_size=(8, 4), input_size_target=(6, 5), **cfg)
    tr.model = tr.D1 = tr.D2 = tr.warper = None
    tr.pg, tr.world, tr._pending, tr._consts = None, 1, [], {}
    tr.opt, tr.opt_D1, tr.opt_D2 = _NoOpt(), None, None
    return tr


@pytest.mark.parametrize("level,hw", [("single-level", (4, 8)), ("multi-level", (5, 6))])
def test_self_training_batches_are_checked_before_the_step(level, hw):
    tr = _stub_trainer(level=level, lambda_st=1.0)
    assert tr._target_size() == (hw[1], hw[0])
    x, lab, xt = torch.zeros(2, 3, 4, 8), torch.zeros(2, 4, 8, dtype=torch.int64), torch.zeros(2, 3, 5, 6)
    with pytest.raises(ValueError, match="labels_target"):
        tr._step_body(0, [(x, lab, xt)])
    other = (5, 6) if hw == (4, 8) else (4, 8)
    with pytest.raises(ValueError, match=rf"expected int64 \(2, {hw[0]}, {hw[1]}\)"):
        tr._step_body(0, [(x, lab, xt, torch.zeros(2, *other, dtype=torch.int64))])
    with pytest.raises(ValueError, match=rf"expected int64 \(2, {hw[0]}, {hw[1]}\)"):
        tr._step_body(0, [(x, lab, xt, torch.zeros(2, *hw, dtype=torch.int32))])
    # the second sub-batch is checked before the first one runs
    good = torch.zeros(2, *hw, dtype=torch.int64)
    with pytest.raises(ValueError, match="labels_target"):
        tr._step_body(0, [(x, lab, xt, good), (x, lab, xt)])


# ---- the reference -----------------------------------------------------------------------------
C, NBINS, SHAPE = 19, 512, (2, 37, 53)


def test_mixed_input_holds_what_it_says():
    pred, conf = PR.mixed_input(SHAPE, C, NBINS)
    assert pred.dtype == np.uint8 and conf.dtype == np.float32 and pred.shape == conf.shape == SHAPE
    assert not (pred == 7).any() and set(np.unique(pred)) == set(range(C)) - {7}
    assert int((conf == 1).sum()) >= 50 and int((conf == 0).sum()) == 10
    assert int(np.isnan(conf).sum()) == 10 and int((conf < 0).sum()) == 10
    hist = PR.conf_hist(pred, conf, C, NBINS)
    assert int(hist.sum()) == pred.size - 20 and int(hist[7].sum()) == 0
    assert int(hist[:, NBINS - 1].sum()) >= 50 and int(hist[:, 0].sum()) == 10


@pytest.mark.parametrize("cap", [0.9, 1.0])
@pytest.mark.parametrize("portion", [0.2, 0.5, 1.0])
def test_reference_keeps_the_portion_and_no_bin_more(portion, cap):
    """Per class: at least ceil(portion * T) pixels are kept, and (uncapped) dropping the threshold's
    bin would keep fewer than that: the threshold is the highest bin edge that keeps the portion."""
    pred, conf = PR.mixed_input(SHAPE, C, NBINS)
    hist = PR.conf_hist(pred, conf, C, NBINS)
    thr = PR.thresholds(hist, portion, cap)
    assert thr.dtype == np.float32
    lab, kept = PR.labels(pred, conf, thr)
    assert int(kept.sum()) == int((lab != 255).sum())
    for c in range(C):
        total = int(hist[c].sum())
        if total == 0:
            assert thr[c] == np.float32(cap) and kept[c] == 0
            continue
        k = math.ceil(portion * total)
        assert kept[c] >= k, (c, kept[c], k)
        if cap == 1.0:
            b = int(thr[c] * NBINS)
            assert np.float32(b) / np.float32(NBINS) == thr[c]
            assert kept[c] - hist[c][b] < k, (c, kept[c], hist[c][b], k)
