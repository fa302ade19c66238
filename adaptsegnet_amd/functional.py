"""Autograd Functions for the step's memory-bound ops (softmax, CE, adversarial losses).

Tensors at this boundary are NCHW-shaped, as in the reference; internally they are NHWC
(channels_last) buffers, and a non-channels_last input is converted by the native
``adaptseg_to_nhwc`` kernel.  Reference call sites:
  F.softmax(pred)                               train_gta2cityscapes_multi.py:423,442,454,617-618
  nn.CrossEntropyLoss(ignore_index=255)         train_gta2cityscapes_multi.py:359,546,599-600
  CrossEntropy2d                                utils/loss.py:14-36
  BCEWithLogitsLoss / MSELoss vs const target   train_gta2cityscapes_multi.py:542-545,620-624
  nn.Upsample(bilinear, align_corners=True)     train_gta2cityscapes_multi.py:237-238 (interp),
                                                model/deeplab_multi.py:188-189
Beyond the reference: ``selfinfo2d`` and ``entropy_loss2d``, the two halves of entropy-based
adaptation (ADVENT), each fused from the logits; ``entropy_loss2d(x, eta=...)`` is
FDA's robust entropy term on the same kernels.
"""
from __future__ import annotations

import torch

from . import kernels as K

BCE, MSE = 0, 1


def _check(x, what):
    if not x.is_cuda:
        raise RuntimeError(f"{what}: adaptsegnet_amd ops run on the HIP device only (got {x.device})")
    if x.dtype != torch.float32:
        raise RuntimeError(f"{what}: expected float32, got {x.dtype}")


class _Softmax2d(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        y = K.softmax_fwd(K.nhwc_view(x))
        ctx.save_for_backward(y)
        return K.as_nchw(y)

    @staticmethod
    def backward(ctx, g):
        (y,) = ctx.saved_tensors
        return K.as_nchw(K.softmax_bwd(y, K.nhwc_view(g)))


def softmax2d(x: torch.Tensor) -> torch.Tensor:
    """Softmax over the channel dim of an [N, C, H, W] tensor (F.softmax's implicit dim=1)."""
    _check(x, "softmax2d")
    return _Softmax2d.apply(x)


class _SelfInfo2d(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        xv = K.nhwc_view(x)
        ctx.save_for_backward(xv)   # the logits only: the backward recomputes p from them
        return K.as_nchw(K.selfinfo_fwd(xv))

    @staticmethod
    def backward(ctx, g):
        (xv,) = ctx.saved_tensors
        return K.as_nchw(K.selfinfo_bwd(xv, K.nhwc_view(g)))


def selfinfo2d(x: torch.Tensor) -> torch.Tensor:
    """The weighted self-information map of [N, C, H, W] logits: ``-p * log(p) / ln(C)`` per channel
    with ``p = softmax(x, dim=1)``, each value in [0, 1/(e ln C)] (0 where p underflows) — what
    the discriminators see under ``StepConfig.d_input="entropy"`` (ADVENT's AdvEnt).  Fused from
    the logits in one kernel; the backward keeps nothing but the logits."""
    _check(x, "selfinfo2d")
    if x.dim() != 4 or x.shape[1] < 2:
        raise RuntimeError(f"selfinfo2d: expected [N, C, H, W] logits with C >= 2, got {tuple(x.shape)}")
    return _SelfInfo2d.apply(x)


class _EntropyLoss2d(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        xv = K.nhwc_view(x)
        ctx.save_for_backward(xv)
        return K.entropy_fwd(xv)[0]

    @staticmethod
    def backward(ctx, g):
        (xv,) = ctx.saved_tensors
        if g.dim() == 0:
            g = g.reshape(1)
        return K.as_nchw(K.entropy_bwd(xv, g.contiguous()))


class _EntropyRhoLoss2d(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, eta, eps):
        xv = K.nhwc_view(x)
        ctx.save_for_backward(xv)
        ctx.eta, ctx.eps = eta, eps
        return K.entropy_rho_fwd(xv, eta, eps)[0]

    @staticmethod
    def backward(ctx, g):
        (xv,) = ctx.saved_tensors
        if g.dim() == 0:
            g = g.reshape(1)
        return K.as_nchw(K.entropy_rho_bwd(xv, ctx.eta, ctx.eps, g.contiguous())), None, None


def entropy_loss2d(x: torch.Tensor, eta: float | None = None, eps: float = 1e-8) -> torch.Tensor:
    """The entropy-minimisation loss of [N, C, H, W] logits (ADVENT's MinEnt): the mean over pixels
    of ``-sum_c p log p``, divided by ``ln C`` (1 for a uniform prediction, 0 for a one-hot one).
    With ``eta``: FDA's robust form, the mean over pixels of ``(e^2 + eps)^eta`` with ``e`` that
    normalised pixel entropy (a Charbonnier penalty; FDA trains with ``eta = 2``); ``eta=None`` is
    the plain loss on its own kernels, and ``eps`` is then unused.  Returns a 0-dim device tensor;
    deterministic (block partials + one ordered fp64 sum); the backward keeps only the logits."""
    _check(x, "entropy_loss2d")
    if x.dim() != 4 or x.shape[1] < 2:
        raise RuntimeError(f"entropy_loss2d: expected [N, C, H, W] logits with C >= 2, got {tuple(x.shape)}")
    if eta is None:
        return _EntropyLoss2d.apply(x)
    eta, eps = float(eta), float(eps)
    if not (0.0 < eta <= 16.0 and 0.0 < eps <= 1.0):
        raise ValueError(f"entropy_loss2d: eta {eta!r}, eps {eps!r} (expected 0 < eta <= 16 and 0 < eps <= 1)")
    return _EntropyRhoLoss2d.apply(x, eta, eps)


class _CrossEntropy2d(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels, ignore, weight, reduction):
        x = K.nhwc_view(logits)
        out = K.ce_fwd(x, labels, ignore, weight)   # [mean, denominator]
        ctx.save_for_backward(x, labels, out, weight)
        ctx.ignore, ctx.total = ignore, reduction == "sum"
        if ctx.total:   # reduction='sum': mean * denominator; an empty selection sums to 0
            return torch.where(out[1] > 0, out[0] * out[1], torch.zeros_like(out[0]))
        if reduction == "mean_or_zero":   # the mean, and 0 (not 0/0) over an empty selection; its
            # gradient needs nothing more: the backward kernels write 0 for every ignored pixel
            return torch.where(out[1] > 0, out[0], torch.zeros_like(out[0]))
        return out[0]

    @staticmethod
    def backward(ctx, g):
        x, labels, out, weight = ctx.saved_tensors
        if g.dim() == 0:
            g = g.reshape(1)
        if ctx.total:   # d(sum)/dlogits = denominator * d(mean)/dlogits
            g = g * out[1:2]
        dl = K.ce_bwd(x, labels, out, g.contiguous(), ctx.ignore, weight)
        return K.as_nchw(dl), None, None, None, None


class _CrossEntropy2dPW(torch.autograd.Function):
    """_CrossEntropy2d with a weight per pixel on the numerator (no gradient to the weights)."""

    @staticmethod
    def forward(ctx, logits, labels, ignore, weight, reduction, pixel_weight):
        x = K.nhwc_view(logits)
        out = K.ce_fwd(x, labels, ignore, weight, pixel_weight)   # [weighted mean, denominator]
        ctx.save_for_backward(x, labels, out, weight, pixel_weight)
        ctx.ignore, ctx.total = ignore, reduction == "sum"
        if ctx.total:
            return torch.where(out[1] > 0, out[0] * out[1], torch.zeros_like(out[0]))
        if reduction == "mean_or_zero":
            return torch.where(out[1] > 0, out[0], torch.zeros_like(out[0]))
        return out[0]

    @staticmethod
    def backward(ctx, g):
        x, labels, out, weight, pixel_weight = ctx.saved_tensors
        if g.dim() == 0:
            g = g.reshape(1)
        if ctx.total:
            g = g * out[1:2]
        dl = K.ce_bwd(x, labels, out, g.contiguous(), ctx.ignore, weight, pixel_weight=pixel_weight)
        return K.as_nchw(dl), None, None, None, None, None


def cross_entropy2d(logits: torch.Tensor, labels: torch.Tensor, ignore_index: int = 255,
                    weight: torch.Tensor | None = None, reduction: str = "mean",
                    pixel_weight: torch.Tensor | None = None) -> torch.Tensor:
    """Softmax cross entropy over pixels whose label is >= 0 and != ignore_index.

    logits: [N, C, H, W] fp32; labels: [N, H, W] int64.  reduction 'mean' (weighted by
    ``weight[label]`` when given), 'sum' or 'mean_or_zero'.  Returns a 0-dim device tensor; an
    all-ignored batch gives NaN for the mean (like the reference) and 0 for the sum
    (F.cross_entropy); 'mean_or_zero' is the mean, but 0 with a zero gradient for an all-ignored
    batch (the self-training term: a batch of pseudo-labels may keep no pixel).

    pixel_weight: float32 [N, H, W] or None.  Each valid pixel's term is multiplied by its weight;
    the mean still divides by the valid pixels (their summed class weights), not by the summed
    pixel weights: ``sum_i pw_i w_i nll_i / sum_i w_i``, so all-ones weights give the unweighted
    loss and down-weighted pixels shrink it (the confidence weights of ``mix.classmix``).  The
    weights get no gradient.  None runs the code path without them.
    """
    if reduction not in ("mean", "sum", "mean_or_zero"):
        raise ValueError(f"cross_entropy2d: reduction {reduction!r} (expected 'mean', 'sum' or 'mean_or_zero')")
    _check(logits, "cross_entropy2d")
    if labels.dtype != torch.int64:
        raise RuntimeError(f"cross_entropy2d: labels must be int64 (got {labels.dtype})")
    n, c, h, w = logits.shape
    if labels.shape != (n, h, w):
        raise RuntimeError(f"cross_entropy2d: labels {tuple(labels.shape)} vs logits {tuple(logits.shape)}")
    labels = labels.contiguous()
    if weight is not None:
        weight = weight.to(device=logits.device, dtype=torch.float32).contiguous()
    if pixel_weight is not None:
        if pixel_weight.dtype != torch.float32 or pixel_weight.shape != (n, h, w):
            raise RuntimeError(f"cross_entropy2d: pixel_weight is {pixel_weight.dtype} {tuple(pixel_weight.shape)}, "
                               f"expected float32 {(n, h, w)}")
        if pixel_weight.device != logits.device:
            raise RuntimeError(f"cross_entropy2d: pixel_weight is on {pixel_weight.device}, logits on {logits.device}")
        return _CrossEntropy2dPW.apply(logits, labels, int(ignore_index), weight, reduction,
                                       pixel_weight.detach().contiguous())
    return _CrossEntropy2d.apply(logits, labels, int(ignore_index), weight, reduction)


class _AdvLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, target, kind):
        xc = x.contiguous() if not (x.is_contiguous() or x.is_contiguous(memory_format=torch.channels_last)) else x
        loss = K.adv_fwd(xc, target, kind)
        ctx.save_for_backward(xc)
        ctx.target, ctx.kind = target, kind
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        if g.dim() == 0:
            g = g.reshape(1)
        return K.adv_bwd(x, ctx.target, ctx.kind, g.contiguous()), None, None


def adv_loss(d_out: torch.Tensor, target: float, kind: int) -> torch.Tensor:
    """mean(BCEWithLogits(d_out, target)) (kind=BCE) or mean((d_out-target)^2) (kind=MSE)."""
    _check(d_out, "adv_loss")
    return _AdvLoss.apply(d_out, float(target), int(kind))


def bce_with_logits_const(d_out, target: float):
    return adv_loss(d_out, target, BCE)


def mse_const(d_out, target: float):
    return adv_loss(d_out, target, MSE)


class _Interp(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, oh, ow):
        xv = K.nhwc_view(x)
        ctx.hw = (xv.shape[1], xv.shape[2])
        return K.as_nchw(K.upsample_fwd(xv, oh, ow))

    @staticmethod
    def backward(ctx, g):
        h, w = ctx.hw
        return K.as_nchw(K.upsample_bwd(K.nhwc_view(g), h, w)), None, None


def interp(x: torch.Tensor, size) -> torch.Tensor:
    """``nn.Upsample(size=(H, W), mode='bilinear', align_corners=True)(x)`` for [N, C, h, w]."""
    _check(x, "interp")
    return _Interp.apply(x, int(size[0]), int(size[1]))
