"""The AdaptSegNet adversarial training step on the HIP engine (single- and multi-level).

Restates the per-iteration body of /root/reference/train_gta2cityscapes_multi.py:
  single-level  :379-464  (G: seg loss on source, adversarial loss on target through the
                            frozen D2; D2: source -> 0, target -> 1, each loss / 2)
  multi-level   :570-683  (two heads, two discriminators, loss_seg2 + lambda_seg*loss_seg1)
  poly LR       :162-177,  SGD(momentum .9, wd 5e-4) + Adam(.9, .99)  :532-540
Resolved reference gaps:
  * the multi-level call ``model(images)`` (:597,615) lacks ``input_size`` and raises in the
    reference; here source predictions are upsampled to ``input_size`` and target ones to
    ``input_size_target`` (``target_size='target'``), or to the source size as the fork's
    single-level branch does (:421, ``target_size='source'``, the single-level default);
  * ``SOURCE_ONLY = True`` (:24) is not hard-wired: ``StepConfig.level`` selects the
    adversarial steps or ``"source-only"`` (:259-286, segmentation loss only);
  * the fork's warper (:217-220, 271-275, 401-405) is applied when a ``Warper`` is given: its
    field warps the source predictions (source-only and single-level).  The reference's
    single-level branch reuses the source field for the target prediction (:421) and then
    crashes in the target backward (the field's graph was freed by the source backward); here
    the target is warped by the same field, detached.  The warper's parameters are in no
    optimiser (:244,347,532), so their gradients only accumulate, as in the reference.
Differences that do not change results: loss scalings (``lambda * loss / iter_size``) are
passed as the initial gradient of ``backward`` instead of multiplying the loss tensors, the
constant label tensors (:621, ...) are folded into the loss kernels, and the per-loss
``.item()`` host syncs are deferred to ``StepLosses.values()``.

Beyond the reference: ``StepConfig.lambda_st > 0`` adds a self-training term to the target branch,
the cross entropy of the target prediction(s) against pseudo-labels given as a fourth batch
element (adaptsegnet_amd/pseudo.py; the CBST / BDL stage after adaptation).  At 0, the default,
the step is the reference's.  ``StepConfig.d_input="entropy"`` and ``StepConfig.lambda_ent > 0`` are the
two halves of entropy-based adaptation (ADVENT): the discriminators see the weighted self-information
map of a prediction instead of its softmax, and the target branch adds an entropy-minimisation loss.
``StepConfig.lambda_mix > 0`` is online self-training (DACS; adaptsegnet_amd/mix.py): a third generator
forward on a ClassMix image made by a mean teacher, trained with a confidence-weighted cross entropy.
``StepConfig.lambda_mic > 0`` is masked image consistency (MIC) on top: one more generator forward, on the
target image with random patches blanked, trained the same way on the teacher's labels of the whole image.

Data parallel (one process per GPU): every rank runs the step on its own shard, and SUM
all-reduces of the gradient arenas replace DataParallel's gradient gather
(train_gta2cityscapes_multi.py:224-225); the 1/world average is folded into the optimiser.
DeeplabMulti's 178 MB arena is reduced in buckets (``bucket_mb``) launched from inside the
step's last generator backward as each bucket's weight gradients are queued (layer6 and layer4
first), so the collectives overlap the rest of that backward; the discriminators' arenas follow
their last backward.  BN statistics stay per-rank, as in the reference's per-replica
DataParallel semantics.
"""
from __future__ import annotations

import contextlib
from dataclasses import dataclass, field

import torch
import torch.distributed as dist

from . import engine
from . import functional as F
from . import kernels as K
from .optim import SGD, Adam, lr_poly


@dataclass
class StepConfig:
    level: str = "single-level"          # or "multi-level", "source-only"
    gan: str = "Vanilla"                 # "Vanilla" (BCEWithLogits) or "LS" (MSE)
    num_classes: int = 19
    input_size: tuple = (1024, 512)      # (W, H) of source images
    input_size_target: tuple = (1024, 512)
    target_size: str = "auto"            # "source" | "target" | "auto" (single: source, multi: target)
    iter_size: int = 1
    learning_rate: float = 2.5e-4
    learning_rate_D: float = 1e-4
    momentum: float = 0.9
    weight_decay: float = 5e-4
    power: float = 0.9
    num_steps: int = 250000
    lambda_seg: float = 0.1
    lambda_adv_target1: float = 0.0002
    lambda_adv_target2: float = 0.001
    ignore_label: int = 255
    # self-training (the CBST / BDL stage after adaptation): with lambda_st > 0 every batch is
    # (images, labels, images_target, labels_target) and the target branch adds
    # lambda_st * CE(pred_target2, labels_target) (multi-level: + lambda_seg * lambda_st * CE on
    # pred_target1), the mean over the pixels that are not ``ignore_label``, 0 when none is left.
    # labels_target: int64 [N, H, W] at the size the target prediction is upsampled to
    # (``_target_size()``), e.g. adaptsegnet_amd.pseudo.pseudo_labels.  0: the step as it was
    lambda_st: float = 0.0
    # entropy-based adaptation (ADVENT).  d_input: what the discriminators see of a prediction,
    # "softmax" (the reference) or "entropy", the weighted self-information map -p log p / ln C
    # (AdvEnt; functional.selfinfo2d), at every discriminator input of the step.  lambda_ent > 0
    # (MinEnt) adds lambda_ent * entropy_loss2d(pred_target2) to the target branch's backward
    # (multi-level: + lambda_seg * lambda_ent * entropy_loss2d(pred_target1), lambda_st's
    # weighting of head 1); batches keep their shape.  The defaults are the step as it was
    d_input: str = "softmax"
    lambda_ent: float = 0.0
    # FDA's robust entropy term: with ent_eta the lambda_ent term is entropy_loss2d(pred, eta=ent_eta), the
    # mean over pixels of (e^2 + 1e-8)^ent_eta on the normalised pixel entropy e (FDA: lambda_ent = 0.005,
    # ent_eta = 2.0).  It shapes lambda_ent's term, so it needs lambda_ent > 0.  None: the plain entropy loss
    ent_eta: float | None = None
    # online self-training (DACS: mean teacher + ClassMix, adaptsegnet_amd/mix.py).  With
    # lambda_mix > 0 every batch ends with three more elements, after the optional labels_target:
    # (mixed_images float32 [N, 3, H, W], mixed_labels int64 [N, H, W], mixed_weights float32
    # [N, H, W]) at ``input_size`` (``EmaTeacher.mix``), and the sub-iteration gains a third generator
    # forward, on mixed_images, whose backward is lambda_mix * cross_entropy2d(pred2, mixed_labels,
    # reduction="mean_or_zero", pixel_weight=mixed_weights) (multi-level: + lambda_seg * lambda_mix *
    # the same on pred1).  It runs on the main stream after the target branch's backward and is then
    # the sub-iteration's last generator backward.  Allowed at every level: "source-only" with it
    # is plain DACS, its batches (images, labels, mixed_images, mixed_labels, mixed_weights).
    # 0: the step as it was
    lambda_mix: float = 0.0
    # masked image consistency (MIC, the stage built on DACS; adaptsegnet_amd/mix.py).  With lambda_mic > 0
    # every batch ends with three more elements after everything else, the mixed triple included:
    # (masked_images float32 [N, 3, Ht, Wt], masked_labels int64 [N, Ht, Wt], masked_weights float32
    # [N, Ht, Wt]) at ``input_size_target`` (``EmaTeacher.mask``), and the sub-iteration gains one more
    # generator forward, on masked_images, upsampled to ``input_size_target``, whose backward is lambda_mic *
    # cross_entropy2d(pred2, masked_labels, reduction="mean_or_zero", pixel_weight=masked_weights)
    # (multi-level: + lambda_seg * lambda_mic * the same on pred1).  It runs on the main stream after the
    # mixed branch if there is one and is then the sub-iteration's last generator backward.  Allowed at every
    # level: "source-only" batches are (images, labels[, mixed triple], masked triple).  0: the step as it was
    lambda_mic: float = 0.0
    # run the target-domain generator forward (+ its D forward) on a second HIP stream while
    # the source-domain backward executes (independent: same weights, read-only, separate
    # gradient kernels); the target backward then waits for the source backward.  Results are
    # bit-identical to the sequential order (tests/test_model_gpu.py).  "auto" (the default):
    # on for DeeplabMulti — the backward alone does not fill the chip, the forward beside it
    # does: c2 +1.3 %, c3 +1.1 %, c5 +3.6 % (profiles/r5/overlap_ab.txt) — off for DeeplabVGG
    # (c4 -0.6 %).
    overlap_domains: bool | str = "auto"
    # with overlap_domains: enqueue the target forward BEFORE the source backward, so its kernels
    # are in the side stream's queue when the backward starts instead of after the host has
    # issued the whole backward (≈1,000 launches); same kernels, same inputs, bit-identical.
    # Off: within ±0.6 % at c2 / c3 / c5 (profiles/r5/target_first_ab.txt) — the host already
    # runs far enough ahead of the GPU
    target_first: bool = False
    # run the discriminator step (its forwards on the detached predictions and its backwards,
    # train:435-461 / 642-679) on its own HIP stream as soon as the target forward is done, beside
    # the step's last generator backward: it reads only the detached predictions and D's weights
    # (unchanged until the optimisers), and writes only D's gradient arena, which that backward
    # does not touch (D's parameters are frozen while its graph is built).  Results are
    # bit-identical to the sequential order (tests/test_model_gpu.py).
    overlap_d: bool = False
    # D's own step on the target prediction reuses the forward the generator's adversarial loss
    # ran (same input, same weights: bit-identical, engine.DiscForward) instead of running D and
    # its softmax again — one D forward per discriminator and step fewer
    d_reuse: bool = True
    # single-level: DeeplabMulti computes only the head the step uses (the reference's
    # ``_, pred2 = model(...)`` discards layer5's; ResNetMulti.forward(first_head=False))
    second_head_only: bool = True
    # data parallel: size of the generator's gradient all-reduce buckets (DeeplabMulti); 0 =
    # one all-reduce of the whole arena after its last backward
    bucket_mb: float = 32.0
    # HIP stream priority of the step's main chain (None: the caller's stream; "auto": high
    # for DeeplabMulti, the caller's stream for DeeplabVGG); see step()
    main_priority: int | str | None = "auto"

    def __post_init__(self):
        if self.ent_eta is not None and not self.lambda_ent > 0:
            raise ValueError(f"ent_eta {self.ent_eta!r} with lambda_ent {self.lambda_ent!r}: ent_eta shapes the "
                             "entropy term, which lambda_ent > 0 turns on")


@dataclass
class StepLosses:
    tensors: dict = field(default_factory=dict)

    def add(self, name, t, scale):
        self.tensors.setdefault(name, []).append((t, scale))

    def values(self) -> dict:
        """Host values (one device sync), summed like the reference's *_value accumulators."""
        return {k: sum(float(t.detach()) * s for t, s in v) for k, v in self.tensors.items()}


class AdaptSegTrainer:
    """Owns the optimisers and runs one adversarial iteration per ``step()`` call."""

    def __init__(self, model, model_D1, model_D2, cfg: StepConfig, process_group=None, warper=None):
        self.model, self.D1, self.D2, self.cfg = model, model_D1, model_D2, cfg
        self.warper = warper
        if cfg.level not in ("single-level", "multi-level", "source-only"):
            raise ValueError(f"unknown level {cfg.level!r}")
        if cfg.level == "multi-level" and model_D1 is None:
            raise ValueError("multi-level needs model_D1")
        if cfg.level == "multi-level" and getattr(model, "single_output", False):
            raise ValueError("multi-level needs a two-head generator (DeeplabMulti)")
        if cfg.lambda_st < 0:
            raise ValueError(f"lambda_st {cfg.lambda_st!r} (expected >= 0)")
        if cfg.lambda_st > 0 and cfg.level == "source-only":
            raise ValueError("lambda_st > 0: the self-training term belongs to the target branch of the "
                             "single-level / multi-level steps; the source-only step has none")
        if cfg.d_input not in ("softmax", "entropy"):
            raise ValueError(f"unknown d_input {cfg.d_input!r} (expected 'softmax' or 'entropy')")
        if cfg.lambda_ent < 0:
            raise ValueError(f"lambda_ent {cfg.lambda_ent!r} (expected >= 0)")
        if cfg.lambda_ent > 0 and cfg.level == "source-only":
            raise ValueError("lambda_ent > 0: the entropy term belongs to the target branch of the "
                             "single-level / multi-level steps; the source-only step has none")
        cfg.__post_init__()   # ent_eta needs lambda_ent > 0 (a config changed after it was made)
        if cfg.ent_eta is not None and not 0.0 < cfg.ent_eta <= 16.0:
            raise ValueError(f"ent_eta {cfg.ent_eta!r} (expected None or 0 < ent_eta <= 16)")
        if cfg.lambda_mix < 0:
            raise ValueError(f"lambda_mix {cfg.lambda_mix!r} (expected >= 0)")
        if cfg.lambda_mix > 0 and warper is not None:
            raise ValueError("lambda_mix > 0 with a warper: the mixed image has no flow field of its own "
                             "(the warper's field belongs to the source image)")
        if cfg.lambda_mic < 0:
            raise ValueError(f"lambda_mic {cfg.lambda_mic!r} (expected >= 0)")
        if cfg.lambda_mic > 0 and warper is not None:
            raise ValueError("lambda_mic > 0 with a warper: the masked image has no flow field of its own "
                             "(the warper's field belongs to the source image)")
        if cfg.level != "source-only" and model_D2 is None:
            raise ValueError(f"{cfg.level} needs model_D2")
        if warper is not None and (cfg.level == "multi-level" or getattr(model, "single_output", False)):
            raise ValueError("the warper applies to DeeplabMulti's source-only and single-level steps "
                             "(train_gta2cityscapes_multi.py:271-275, 401-405)")
        self.opt = SGD(model, cfg.learning_rate, cfg.momentum, cfg.weight_decay)
        self.opt_D1 = Adam(model_D1, cfg.learning_rate_D, betas=(0.9, 0.99)) if model_D1 is not None else None
        self.opt_D2 = Adam(model_D2, cfg.learning_rate_D, betas=(0.9, 0.99)) if model_D2 is not None else None
        self.kind = F.BCE if cfg.gan == "Vanilla" else F.MSE
        self.pg = process_group
        self.world = dist.get_world_size(process_group) if (dist.is_available() and dist.is_initialized()) else 1
        self._consts = {}
        self._pending = []

    # -- helpers -------------------------------------------------------------------------
    def _c(self, v: float, device):
        key = (float(v), device)
        t = self._consts.get(key)
        if t is None:
            t = self._consts[key] = torch.full((), float(v), dtype=torch.float32, device=device)
        return t

    # -- stream overlap of the two domains -----------------------------------------------------
    _streams: dict = {}

    def _overlap_domains(self) -> bool:
        ov = self.cfg.overlap_domains
        if ov == "auto":
            return not getattr(self.model, "single_output", False)
        return bool(ov)

    def _overlap_begin(self, device):
        """After the source forward: returns (main, side, event) or None (overlap off / CPU)."""
        if not self._overlap_domains() or device.type != "cuda":
            return None
        side = AdaptSegTrainer._streams.get(device.index)
        if side is None:
            side = AdaptSegTrainer._streams[device.index] = torch.cuda.Stream(device)
        main = torch.cuda.current_stream(device)
        ev = torch.cuda.Event()
        ev.record(main)   # the target pass starts after the source forward (BN running stats)
        return main, side, ev

    def _target_ctx(self, ov):
        if ov is None:
            return contextlib.nullcontext()
        main, side, ev = ov
        side.wait_event(ev)
        return torch.cuda.stream(side)

    @staticmethod
    def _join_source(ov):
        """Before the target-domain G backward: the source backward (main stream) must have
        finished writing the gradient arena it accumulates into."""
        if ov is not None:
            ov[1].wait_stream(ov[0])

    _d_streams: dict = {}

    def _d_fork(self, device):
        """After the target forward (+ its D forward), on the stream that ran it: an event the
        discriminator step's stream waits on, or None (overlap_d off / CPU)."""
        if not self.cfg.overlap_d or device.type != "cuda":
            return None
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(device))
        return ev

    def _d_ctx(self, ev, device, *tensors):
        """The discriminator step's stream context: waits for ``ev`` only; ``tensors`` (made on
        other streams) are marked used on it.  The main stream joins it before the optimisers."""
        if ev is None:
            return contextlib.nullcontext()
        ds = AdaptSegTrainer._d_streams.get(device.index)
        if ds is None:
            ds = AdaptSegTrainer._d_streams[device.index] = torch.cuda.Stream(device)
        ds.wait_event(ev)
        for t in tensors:
            t.record_stream(ds)
        self.__dict__.setdefault("_d_used", set()).add(device.index)
        return torch.cuda.stream(ds)

    def _d_join(self, device):
        if device.index in self.__dict__.get("_d_used", ()):
            torch.cuda.current_stream(device).wait_stream(AdaptSegTrainer._d_streams[device.index])
            self._d_used.discard(device.index)

    @staticmethod
    def _overlap_end(ov, *tensors):
        if ov is None:
            return
        main, side, _ = ov
        main.wait_stream(side)
        for t in tensors:
            t.record_stream(main)   # produced on the side stream, read on the main stream

    def _d_keep(self, D):
        """A DiscForward to keep D's target forward in (d_reuse, HIP-engine discriminators)."""
        return engine.DiscForward() if self.cfg.d_reuse and hasattr(D, "_convs") else None

    @staticmethod
    def _d_out(D, x, keep):
        return D(x) if keep is None else engine.discriminator_forward(D, x, keep=keep)

    def _d_in(self, pred):
        """What a discriminator sees of a prediction (cfg.d_input)."""
        return F.selfinfo2d(pred) if self.cfg.d_input == "entropy" else F.softmax2d(pred)

    def _ent_loss(self, pred_target):
        """[entropy_loss2d(pred_target)] (FDA's robust form with cfg.ent_eta) with lambda_ent > 0, else []."""
        return [F.entropy_loss2d(pred_target, eta=self.cfg.ent_eta)] if self.cfg.lambda_ent > 0 else []

    def _d_again(self, D, pred, keep):
        """D on the detached target prediction for D's own step: the kept forward when there is one."""
        return D(self._d_in(pred)) if keep is None else engine.discriminator_replay(D, keep)

    @staticmethod
    def _kept(*keeps):
        return [t for k in keeps if k is not None for t in k.tensors()]

    def _backward(self, losses, scales):
        dev = losses[0].device
        torch.autograd.backward(list(losses), grad_tensors=[self._c(s, dev) for s in scales])

    @staticmethod
    def _set_requires_grad(model, flag):
        for p in model.parameters():
            p.requires_grad = flag

    def adjust_learning_rate(self, i_iter):
        c = self.cfg
        lr = lr_poly(c.learning_rate, i_iter, c.num_steps, c.power)
        self.opt.param_groups[0]["lr"] = lr
        self.opt.param_groups[1]["lr"] = lr * 10
        lr_d = lr_poly(c.learning_rate_D, i_iter, c.num_steps, c.power)
        for o in (self.opt_D1, self.opt_D2):
            if o is not None:
                o.param_groups[0]["lr"] = lr_d

    def _target_size(self):
        c = self.cfg
        mode = c.target_size
        if mode == "auto":
            mode = "source" if c.level == "single-level" else "target"
        return c.input_size if mode == "source" else c.input_size_target

    def sync_gradients(self):
        """SUM all-reduce of each parameter arena's gradients (RCCL on ROCm), blocking."""
        self._start_sync((self.model, self.D1, self.D2))
        self._finish_sync()

    def _start_sync(self, models):
        """Launch the arena all-reduces of ``models`` asynchronously.  RCCL orders them after
        the work already queued on the current stream (the gradients they read) and runs them
        on its own stream, so they overlap whatever the step launches next."""
        if self.world == 1:
            return
        pending = self.__dict__.setdefault("_pending", [])
        for m in models:
            if m is not None and m.arena is not None:
                pending.append(dist.all_reduce(m.arena.grad, op=dist.ReduceOp.SUM,
                                                     group=self.pg, async_op=True))

    def _g_sync_begin(self):
        """Before the step's last generator backward: install the bucketed all-reduce hook on
        a generator that supports it (DeeplabMulti).  Returns the hook or None."""
        if self.world == 1 or self.cfg.bucket_mb <= 0 or not hasattr(self.model, "_grad_buckets"):
            return None
        if getattr(self.model, "_arena", None) is None:
            return None
        hook = _BucketAllReduce(self, self.model.arena.grad,
                                self.model._grad_buckets(int(self.cfg.bucket_mb * 2 ** 20)))
        self.model._grad_hook = hook
        return hook

    def _g_sync_end(self, hook):
        """After the step's last generator backward: every bucket (or the whole arena) has its
        all-reduce in flight."""
        if hook is None:
            self._start_sync((self.model,))
            return
        self.model._grad_hook = None
        hook(None, None)
        self.g_allreduce_ranges = list(hook.launched)   # (start, end) arena ranges, launch order

    def _finish_sync(self):
        """Make the current stream wait for every launched all-reduce (no host sync)."""
        for w in self.__dict__.get("_pending", ()):
            w.wait()
        self._pending = []

    # -- the step --------------------------------------------------------------------------
    _hp_streams: dict = {}

    def step(self, i_iter, batches):
        """One iteration.  The step's main chain (forwards, data gradients, BN, losses,
        optimisers) runs on a HIP stream of priority ``cfg.main_priority`` (-1, high, for
        DeeplabMulti), so the hardware scheduler favours it over the weight-gradient side stream
        that fills the gaps the HBM-bound BN passes leave: +0.9 % c2, +0.2 % c3, ±0 c5, but
        -1.7 % for DeeplabVGG (c4: no BN, so it runs on the caller's stream).  The caller's
        stream waits for it at the end.  ``main_priority=None`` runs on the caller's stream."""
        prio = self.cfg.main_priority
        if prio == "auto":   # VGG has no BN passes for the side stream to fill: -1.7 % with it
            prio = None if getattr(self.model, "single_output", False) else -1
        dev = next(self.model.parameters()).device
        # each conv's weight pack is built once per step (the optimisers, the only writers of the
        # weights, run after the step's last conv): kernels.weight_pack_scope
        if prio is None or dev.type != "cuda":
            with K.weight_pack_scope():
                return self._step_body(i_iter, batches)
        batches = list(batches)
        key = (dev.index, prio)
        hp = AdaptSegTrainer._hp_streams.get(key)
        if hp is None:
            hp = AdaptSegTrainer._hp_streams[key] = torch.cuda.Stream(dev, priority=prio)
        cur = torch.cuda.current_stream(dev)
        hp.wait_stream(cur)
        with torch.cuda.stream(hp), K.weight_pack_scope():
            L = self._step_body(i_iter, batches)
        cur.wait_stream(hp)
        return L

    def _step_body(self, i_iter, batches):
        """batches: iterable of ``iter_size`` tuples (images, labels, images_target), or with
        ``cfg.lambda_st > 0`` (images, labels, images_target, labels_target); with
        ``cfg.lambda_mix > 0`` each ends with (mixed_images, mixed_labels, mixed_weights) besides, and with
        ``cfg.lambda_mic > 0`` with (masked_images, masked_labels, masked_weights) after that.

        Multi-GPU: the generator's gradients are final after its adversarial backward of the
        last sub-iteration, so their all-reduce (the 178 MB arena) is launched right there and
        overlaps the discriminator forward/backward passes; the discriminators' (11 MB each)
        follow their last backward.  The optimisers wait for both."""
        c = self.cfg
        batches = list(batches)
        tsize = self._target_size()
        branches = self._extra_branches()
        if c.lambda_st > 0:   # a malformed self-training batch raises before anything is launched
            for batch in batches:
                self._st_labels(batch, tsize, branches)
        # and so does a malformed mixed or masked triple; each batch's triples are taken apart once, here
        extras = [self._extra_elements(batch, branches) for batch in batches] if branches else None
        L = StepLosses()
        self.opt.zero_grad()
        for o in (self.opt_D1, self.opt_D2):
            if o is not None:
                o.zero_grad()
        self.adjust_learning_rate(i_iter)
        inv = 1.0 / c.iter_size
        self._pending = []
        for idx, batch in enumerate(batches):
            g_done = _GSync(self) if idx == len(batches) - 1 else None
            extra = extras[idx] if branches else None
            if c.level == "source-only":
                self._sub_source_only(batch[0], batch[1], inv, L, g_done, extra)
                continue
            images, labels, images_t = batch[:3]
            labels_t = batch[3] if c.lambda_st > 0 else None
            if c.level == "single-level":
                self._sub_single(images, labels, images_t, inv, tsize, L, g_done, labels_t, extra)
            else:
                self._sub_multi(images, labels, images_t, inv, tsize, L, g_done, labels_t, extra)
        if not batches:
            self._start_sync((self.model,))
        if batches and c.level != "source-only":
            self._d_join(next(self.model.parameters()).device)
        self._start_sync((self.D1, self.D2))
        self._finish_sync()
        gs = 1.0 / self.world
        self.opt.step(grad_scale=gs)
        for o in (self.opt_D1, self.opt_D2):
            if o is not None:
                o.step(grad_scale=gs)
        return L

    def _extra_branches(self):
        """The branches that follow the target branch, in the order they run and their triples end a batch:
        (kind, lambda's name, lambda, (W, H) of the triple and of the branch's predictions, that size's name)."""
        c = self.cfg
        out = []
        if c.lambda_mix > 0:
            out.append(("mixed", "lambda_mix", c.lambda_mix, c.input_size, "input_size"))
        if c.lambda_mic > 0:
            out.append(("masked", "lambda_mic", c.lambda_mic, c.input_size_target, "input_size_target"))
        return out

    @staticmethod
    def _triple_names(branches):
        return ", ".join(f"{b[0]}_images, {b[0]}_labels, {b[0]}_weights" for b in branches)

    @staticmethod
    def _st_labels(batch, tsize, branches=()):
        """The fourth element of a self-training batch, checked against the target prediction's size
        (``branches``: whose triples follow it, lambda_mix's and lambda_mic's)."""
        if len(batch) != 4 + 3 * len(branches):
            raise ValueError(f"lambda_st > 0: every batch is (images, labels, images_target, labels_target"
                             f"{', ' + AdaptSegTrainer._triple_names(branches) if branches else ''}); "
                             f"got {len(batch)} elements")
        images_t, labels_t = batch[2], batch[3]
        want = (images_t.shape[0], int(tsize[1]), int(tsize[0]))
        if labels_t.dtype != torch.int64 or tuple(labels_t.shape) != want:
            raise ValueError(f"labels_target is {labels_t.dtype} {tuple(labels_t.shape)}: expected int64 {want}, "
                             f"[N, H, W] at the size the target prediction is upsampled to (W, H) = {tuple(tsize)}")
        return labels_t

    def _extra_elements(self, batch, branches):
        """The triples a batch ends with, one per branch of ``branches`` (lambda_mix's at ``input_size``, then
        lambda_mic's at ``input_size_target``), checked: [(branch, (images, labels, weights))]."""
        c = self.cfg
        base = (2 if c.level == "source-only" else 3) + (1 if c.lambda_st > 0 else 0)
        if len(batch) != base + 3 * len(branches):
            raise ValueError(f"{', '.join(b[1] for b in branches)} > 0: every batch ends with "
                             f"({self._triple_names(branches)}) after its {base} other elements; got {len(batch)} "
                             "elements")
        out = []
        for k, branch in enumerate(branches):
            kind, _, _, size, size_name = branch
            triple = tuple(batch[base + 3 * k:base + 3 * k + 3])
            # a masked triple belongs to the target batch, a mixed one (and a source-only one) to the source batch
            n = batch[2 if kind == "masked" and c.level != "source-only" else 0].shape[0]
            w, h = int(size[0]), int(size[1])
            for name, t, dtype, want in ((f"{kind}_images", triple[0], torch.float32, (n, 3, h, w)),
                                         (f"{kind}_labels", triple[1], torch.int64, (n, h, w)),
                                         (f"{kind}_weights", triple[2], torch.float32, (n, h, w))):
                if not isinstance(t, torch.Tensor) or t.dtype != dtype or tuple(t.shape) != want:
                    got = f"{t.dtype} {tuple(t.shape)}" if isinstance(t, torch.Tensor) else type(t).__name__
                    raise ValueError(f"{name} is {got}: expected {dtype} {want}, at {size_name} (W, H) = "
                                     f"{tuple(size)}")
            out.append((branch, triple))
        return out

    def _sub_extras(self, extras, inv, L, g_done):
        """The branches after the target branch, in order: the mixed one (lambda_mix > 0), then the masked one
        (lambda_mic > 0).  The last of them is the sub-iteration's last generator backward: ``g_done`` wraps
        it, and no branch before it."""
        for k, (branch, triple) in enumerate(extras):
            self._sub_extra(branch, triple, inv, L, g_done if k == len(extras) - 1 else None)

    def _sub_extra(self, branch, triple, inv, L, g_done):
        """One more generator forward, on the ClassMix image (the mixed branch) or on the masked target image
        (the masked branch), and the confidence-weighted CE against the triple's labels.  On the main stream,
        after the target branch's backward and the side stream's join (its BatchNorm running-statistics
        updates must not race the overlapped target forward).  The discriminator step does not depend on it."""
        c = self.cfg
        kind, _, lam, size, _ = branch
        tag = "mix" if kind == "mixed" else "mic"
        mi, ml, mw = triple
        if c.level == "multi-level":
            pred1, pred2 = self.model(mi, size)
            preds, scales, names = [pred2, pred1], [lam * inv, c.lambda_seg * lam * inv], \
                [f"loss_{tag}2", f"loss_{tag}1"]
        else:
            preds, scales, names = [self._pred_single(mi, size)], [lam * inv], [f"loss_{tag}2"]
        losses = [F.cross_entropy2d(p, ml, c.ignore_label, reduction="mean_or_zero", pixel_weight=mw) for p in preds]
        if g_done is not None:
            g_done.begin()
        self._backward(losses, scales)
        for name, t in zip(names, losses):
            L.add(name, t, inv)
        if g_done is not None:
            g_done.end()

    def _st_loss(self, pred_target, labels_t, ov):
        """CE of a target prediction against the pseudo-labels, on the stream the target branch runs
        on.  ``labels_t`` was made on the caller's stream, which the step's streams are ordered
        after (step(): hp.wait_stream; _target_ctx: the side stream waits for the main one); it is
        marked used on the side stream like the other tensors that cross streams."""
        if ov is not None:
            labels_t.record_stream(ov[1])
        return F.cross_entropy2d(pred_target, labels_t, self.cfg.ignore_label, reduction="mean_or_zero")

    def _pred_single(self, images, size, flow=None):
        """The single-level prediction at ``size`` = (W, H): DeeplabMulti's second head (warped
        by ``flow`` when given), or a single-map model (DeeplabVGG, config c4) followed by the
        caller-side ``interp``."""
        if getattr(self.model, "single_output", False):
            return F.interp(self.model(images), (size[1], size[0]))
        if self.cfg.second_head_only and getattr(self.model, "second_head_only_ok", False):
            return self.model(images, size, flow, first_head=False)[1]
        return self.model(images, size, flow)[1]

    def _flow(self, images):
        return None if self.warper is None else self.warper(images)[0]

    def _sub_source_only(self, images, labels, inv, L, g_done=None, extras=None):
        """train_gta2cityscapes_multi.py:259-286: warper (if any), segmentation loss on the
        second head, backward; the step is the generator's SGD only."""
        pred2 = self._pred_single(images, self.cfg.input_size, self._flow(images))
        loss_seg2 = F.cross_entropy2d(pred2, labels, self.cfg.ignore_label)
        last = g_done if extras is None else None   # else the last mixed / masked branch is the last backward
        if last is not None:
            last.begin()
        self._backward([loss_seg2], [inv])
        L.add("loss_seg2", loss_seg2, inv)
        if last is not None:
            last.end()
        if extras is not None:
            self._sub_extras(extras, inv, L, g_done)

    def _sub_single(self, images, labels, images_t, inv, tsize, L, g_done=None, labels_t=None, extras=None):
        """train_gta2cityscapes_multi.py:385-461."""
        c, D2 = self.cfg, self.D2
        self._set_requires_grad(D2, False)
        flow = self._flow(images)
        pred2 = self._pred_single(images, c.input_size, flow)
        loss_seg2 = F.cross_entropy2d(pred2, labels, c.ignore_label)
        ov = self._overlap_begin(pred2.device)
        keep2 = self._d_keep(D2)

        def target_forward():
            with self._target_ctx(ov):
                pt2 = self._pred_single(images_t, tsize, None if flow is None else flow.detach())
                adv2 = F.adv_loss(self._d_out(D2, self._d_in(pt2), keep2), 0.0, self.kind)
                st = [] if labels_t is None else [self._st_loss(pt2, labels_t, ov)]
                return pt2, adv2, st, self._ent_loss(pt2)

        first = ov is not None and c.target_first
        if first:
            pred_target2, loss_adv_target2, loss_st, loss_ent = target_forward()
        self._backward([loss_seg2], [inv])
        L.add("loss_seg2", loss_seg2, inv)
        if not first:
            pred_target2, loss_adv_target2, loss_st, loss_ent = target_forward()

        with self._target_ctx(ov):
            dev_ = loss_adv_target2.device
            dfork = self._d_fork(dev_)
            self._join_source(ov)
            last = g_done if extras is None else None   # else the last mixed / masked branch is the last backward
            if last is not None:
                last.begin()
            self._backward([loss_adv_target2] + loss_st + loss_ent,
                           [c.lambda_adv_target2 * inv] + [c.lambda_st * inv] * len(loss_st)
                           + [c.lambda_ent * inv] * len(loss_ent))
            L.add("loss_adv_target2", loss_adv_target2, inv)
            for t in loss_st:
                L.add("loss_st2", t, inv)
            for t in loss_ent:
                L.add("loss_ent2", t, inv)
            if last is not None:
                last.end()
        self._overlap_end(ov, pred_target2, loss_adv_target2, *loss_st, *loss_ent, *self._kept(keep2))
        if extras is not None:
            self._sub_extras(extras, inv, L, g_done)

        self._set_requires_grad(D2, True)
        pred2 = pred2.detach()
        pred_target2 = pred_target2.detach()
        with self._d_ctx(dfork, dev_, pred2, pred_target2, *self._kept(keep2)):
            loss_d2 = F.adv_loss(D2(self._d_in(pred2)), 0.0, self.kind)
            self._backward([loss_d2], [inv / 2])
            L.add("loss_D2", loss_d2, inv / 2)
            loss_d2 = F.adv_loss(self._d_again(D2, pred_target2, keep2), 1.0, self.kind)
            self._backward([loss_d2], [inv / 2])
            L.add("loss_D2", loss_d2, inv / 2)

    def _sub_multi(self, images, labels, images_t, inv, tsize, L, g_done=None, labels_t=None, extras=None):
        """train_gta2cityscapes_multi.py:578-679."""
        c, D1, D2 = self.cfg, self.D1, self.D2
        self._set_requires_grad(D1, False)
        self._set_requires_grad(D2, False)
        pred1, pred2 = self.model(images, c.input_size)
        loss_seg1 = F.cross_entropy2d(pred1, labels, c.ignore_label)
        loss_seg2 = F.cross_entropy2d(pred2, labels, c.ignore_label)
        ov = self._overlap_begin(pred2.device)
        keep1, keep2 = self._d_keep(D1), self._d_keep(D2)

        def target_forward():
            with self._target_ctx(ov):
                pt1, pt2 = self.model(images_t, tsize)
                adv1 = F.adv_loss(self._d_out(D1, self._d_in(pt1), keep1), 0.0, self.kind)
                adv2 = F.adv_loss(self._d_out(D2, self._d_in(pt2), keep2), 0.0, self.kind)
                st = [] if labels_t is None else [self._st_loss(pt1, labels_t, ov), self._st_loss(pt2, labels_t, ov)]
                return pt1, pt2, adv1, adv2, st, self._ent_loss(pt1) + self._ent_loss(pt2)

        first = ov is not None and c.target_first
        if first:
            pred_target1, pred_target2, loss_adv1, loss_adv2, loss_st, loss_ent = target_forward()
        self._backward([loss_seg2, loss_seg1], [inv, c.lambda_seg * inv])
        L.add("loss_seg1", loss_seg1, inv)
        L.add("loss_seg2", loss_seg2, inv)
        if not first:
            pred_target1, pred_target2, loss_adv1, loss_adv2, loss_st, loss_ent = target_forward()

        with self._target_ctx(ov):
            dev_ = loss_adv2.device
            dfork = self._d_fork(dev_)
            self._join_source(ov)
            last = g_done if extras is None else None   # else the last mixed / masked branch is the last backward
            if last is not None:
                last.begin()
            st_scales = [c.lambda_seg * c.lambda_st * inv, c.lambda_st * inv][:len(loss_st)]
            ent_scales = [c.lambda_seg * c.lambda_ent * inv, c.lambda_ent * inv][:len(loss_ent)]
            self._backward([loss_adv1, loss_adv2] + loss_st + loss_ent,
                           [c.lambda_adv_target1 * inv, c.lambda_adv_target2 * inv] + st_scales + ent_scales)
            L.add("loss_adv_target1", loss_adv1, inv)
            L.add("loss_adv_target2", loss_adv2, inv)
            for name, t in zip(("loss_st1", "loss_st2"), loss_st):
                L.add(name, t, inv)
            for name, t in zip(("loss_ent1", "loss_ent2"), loss_ent):
                L.add(name, t, inv)
            if last is not None:
                last.end()
        self._overlap_end(ov, pred_target1, pred_target2, loss_adv1, loss_adv2, *loss_st, *loss_ent,
                          *self._kept(keep1, keep2))
        if extras is not None:
            self._sub_extras(extras, inv, L, g_done)

        self._set_requires_grad(D1, True)
        self._set_requires_grad(D2, True)
        pred1, pred2 = pred1.detach(), pred2.detach()
        pred_target1, pred_target2 = pred_target1.detach(), pred_target2.detach()
        with self._d_ctx(dfork, dev_, pred1, pred2, pred_target1, pred_target2, *self._kept(keep1, keep2)):
            loss_d1 = F.adv_loss(D1(self._d_in(pred1)), 0.0, self.kind)
            loss_d2 = F.adv_loss(D2(self._d_in(pred2)), 0.0, self.kind)
            self._backward([loss_d1], [inv / 2])
            self._backward([loss_d2], [inv / 2])
            L.add("loss_D1", loss_d1, inv / 2)
            L.add("loss_D2", loss_d2, inv / 2)
            loss_d1 = F.adv_loss(self._d_again(D1, pred_target1, keep1), 1.0, self.kind)
            loss_d2 = F.adv_loss(self._d_again(D2, pred_target2, keep2), 1.0, self.kind)
            self._backward([loss_d1], [inv / 2])
            self._backward([loss_d2], [inv / 2])
            L.add("loss_D1", loss_d1, inv / 2)
            L.add("loss_D2", loss_d2, inv / 2)


class _GSync:
    """begin() / end() around the step's last generator backward (the gradients are final
    after it): bucketed all-reduces launched from inside that backward, or one whole-arena
    all-reduce after it."""

    def __init__(self, trainer):
        self.tr, self.hook = trainer, None

    def begin(self):
        self.hook = self.tr._g_sync_begin()

    def end(self):
        self.tr._g_sync_end(self.hook)


class _BucketAllReduce:
    """The generator backward's data-parallel hook (DeeplabMulti._grad_hook).

    ``buckets`` = DeeplabMulti._grad_buckets(): [(last_unit_ordinal, [(start, end), ...])] in
    completion order.  hook(ordinal, stream) launches the SUM all-reduce of every bucket whose
    last backward unit is <= ordinal (units skipped by this backward, e.g. layer5 in the
    single-level step, ride with the next unit); hook(None, _) launches the rest.  The
    collectives are issued with ``stream`` (the weight-gradient side stream) current, so the
    process group orders them after the weight-gradient GEMMs already queued there and they run
    while the backward continues; the optimiser's stream waits for them in _finish_sync."""

    def __init__(self, trainer, grad, buckets):
        self.tr, self.grad, self.buckets, self.next = trainer, grad, buckets, 0
        self.launched = []           # (start, end) ranges, in launch order (tests)

    def __call__(self, ordinal, stream):
        while self.next < len(self.buckets) and (ordinal is None or self.buckets[self.next][0] <= ordinal):
            ctx = torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()
            with ctx:
                for a, b in self.buckets[self.next][1]:
                    self.tr._pending.append(dist.all_reduce(self.grad[a:b], op=dist.ReduceOp.SUM,
                                                            group=self.tr.pg, async_op=True))
                    self.launched.append((a, b))
            self.next += 1
