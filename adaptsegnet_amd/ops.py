"""``torch.ops.adaptseg``: the native op surface as PyTorch custom operators.

Every compute launch of the package goes through one of these operators (registered with
``torch.library``: a schema, a CUDA (= HIP on ROCm) kernel and a fake/meta kernel), so the
launches are visible to the dispatcher — torch.profiler records them by name, FakeTensor /
``torch.library.opcheck`` can trace them — while the native boundary stays the C ABI of
include/adaptseg.h: each CUDA kernel below is a thin ctypes call into libadaptseg.so.

There is no CPU kernel: calling an op on CPU tensors raises NotImplementedError from the
dispatcher (the product path has no fallback).  All ops are out-variant: outputs (and
state such as BN running statistics or optimiser buffers) are caller-allocated and declared
mutable (``Tensor(a!)``) in the schema, every op returns ``()``, and ``adaptsegnet_amd.kernels``
allocates and calls them.  Activations are NHWC buffers ``[n, h, w, c]`` (the physical layout
of channels_last NCHW tensors) unless an argument says otherwise; conv weights are any
tensors whose memory is [Cout][KH][KW][Cin] (the modules' NCHW-shaped channels_last
parameters), their logical shape given by ``w_shape`` = [Cout, Cin, KH, KW].  Some engine
calls alias a read-only input with a mutable output (in-place BN backward, residual folded
into the data-gradient output); the kernels support that, and it is why these ops are not
meant for torch.compile's functionalization.

Reference call sites the ops stand in for (file:line in /root/reference):
  conv2d_*            nn.Conv2d in model/deeplab_multi.py:64-75,112,128 / discriminator.py:10-14
                      (conv2d_wpack: the per-step weight pack, optimiser train:532-540 between steps)
  bn_*                nn.BatchNorm2d (+ReLU, residual)  model/deeplab_multi.py:65-101,130-135
  maxpool2d_*         nn.MaxPool2d(3, 2, 1)             model/deeplab_multi.py:135
  upsample_bilinear_* nn.Upsample(bilinear, align_corners=True)  model/deeplab_multi.py:188-189
  softmax_*           F.softmax(pred)                   train_gta2cityscapes_multi.py:617-618
  softmax_ce_*        nn.CrossEntropyLoss(ignore_index=255) / CrossEntropy2d  train:546, utils/loss.py:7-36
  adv_loss_*          BCEWithLogitsLoss / MSELoss vs a constant label  train:542-545,620-624
  sgd_step/adam_step  optim.SGD / optim.Adam            train:532-540
Beyond the reference (``LOSS_NAMES``, registered like the rest but never part of an engine program):
  selfinfo_*          the weighted self-information map -p log p / ln C (ADVENT's discriminator input)
  entropy_loss_*      the entropy-minimisation loss mean(-sum_c p log p) / ln C
and, in ``MIX_NAMES``, online self-training (DACS; adaptsegnet_amd/mix.py):
  ema / ema_multi     the mean teacher's update over an arena / a list of small tensors
  classmix_*          ClassMix: per-image statistics, then selection + paste in one launch
  softmax_ce_pw_*     softmax_ce_* with a weight per pixel on the numerator
and, in ``MIC_NAMES``, masked image consistency (MIC; adaptsegnet_amd/mix.py):
  conf_count          per image the number of target pixels whose confidence reaches tau
  patch_mask          patches blanked by the caller's keys, the teacher's labels, the confidence weights
and, in ``AUG_NAMES``, DACS's strong transform of the mixed images:
  strong_augment      per image a colour jitter, then a Gaussian blur, one launch for the batch
and, in ``FDA_NAMES``, Fourier Domain Adaptation (adaptsegnet_amd/fda.py):
  fda_transfer        a source batch with the low-frequency amplitude spectrum of a target batch
  entropy_rho_loss_*  entropy_loss_* with FDA's robust penalty ((H / ln C)^2 + eps)^eta per pixel
and, in ``RCS_NAMES``, rare class sampling (DAFormer's RCS; adaptsegnet_amd/rcs.py):
  label_class_count   per image the number of pixels of every trainId of a decoded label batch
  crop_class_count    per sample and candidate window the pixels of the sample's class in the augmented label window
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib
from ._lib import CONV_BWD_DATA, CONV_BWD_WEIGHT, CONV_FWD, MATH_F32X3, ConvDesc, check

LIB = torch.library.Library("adaptseg", "DEF")


def _stream() -> ctypes.c_void_p:
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _pf(t, n, what):
    """fp32 operand pointer, checked on the host before any launch: float32 and exactly ``n``
    elements (a tensor of the wrong dtype or size must raise here, not fault on the GPU)."""
    if t is None:
        return None
    if t.dtype != torch.float32 or t.numel() != n:
        raise RuntimeError(f"{what}: expected a float32 tensor of {n} elements, got {t.dtype} {tuple(t.shape)}")
    return ctypes.c_void_p(t.data_ptr())


def _pc(t, n, what):
    """Operand-copy pointer (bf16 image of n elements, or the 3n of F32X3 term images)."""
    if t is None:
        return None
    if t.dtype != torch.bfloat16 or t.numel() not in (n, 3 * n):
        raise RuntimeError(f"{what}: expected a bf16 copy of {n} (or 3 x {n}) elements, got {t.dtype} "
                           f"{tuple(t.shape)}")
    return ctypes.c_void_p(t.data_ptr())


def _pfb(t, n, what):
    """(fp32 pointer, bf16 pointer) of a tensor of n elements stored as either."""
    if t is None:
        return None, None
    if t.dtype == torch.bfloat16:
        return None, _pc(t, n, what)
    return _pf(t, n, what), None


def _pbits(t, n, what):
    """Mask-bitmap pointer: int32 words, one bit per element of an n-element tensor."""
    if t is None:
        return None
    if t.dtype != torch.int32 or t.numel() * 32 != n:
        raise RuntimeError(f"{what}: expected an int32 bitmap of {n // 32} words, got {t.dtype} {tuple(t.shape)}")
    return ctypes.c_void_p(t.data_ptr())


def _ptrs(ts):
    return _lib.ptr_array([None if t is None else t.data_ptr() for t in ts])


# One growing scratch buffer per (device, stream): ops on one stream run in order, so reusing
# it across consecutive calls is race-free.  Caller-owned from the C ABI's point of view.
_WS: dict = {}


def workspace(nbytes: int, device: torch.device):
    if nbytes == 0:
        return None
    key = (device.index, torch.cuda.current_stream(device).cuda_stream)
    buf = _WS.get(key)
    if buf is None or buf.numel() < nbytes:
        cap = max(nbytes, 0 if buf is None else int(buf.numel() * 1.25))
        buf = torch.empty(cap, dtype=torch.uint8, device=device)
        _WS[key] = buf
    return buf


def _ws_args(nbytes: int, device):
    w = workspace(nbytes, device)
    return (ctypes.c_void_p(w.data_ptr()) if w is not None else None), ctypes.c_size_t(nbytes)


# ---------------------------------------------------------------------------------------
# Conv descriptors (host planning only: no GPU needed)
# ---------------------------------------------------------------------------------------
_DESC_CACHE: dict = {}
_CONV_MATH = [MATH_F32X3]   # the library's default (adaptseg_conv_get_math)
OPT_X3H, OPT_G16_WIDE = 1, 2   # adaptseg_conv_option
_OPTS: dict = {}               # adaptseg_conv_get_option, read on first use (the library reads the environment)


def get_option(opt: int) -> int:
    if opt not in _OPTS:
        m = ctypes.c_int(0)
        check(_lib.lib().adaptseg_conv_get_option(int(opt), ctypes.byref(m)), "conv_get_option")
        _OPTS[opt] = m.value
    return _OPTS[opt]


def set_option(opt: int, value: int) -> None:
    check(_lib.lib().adaptseg_conv_set_option(int(opt), int(value)), "conv_set_option")
    _OPTS[opt] = int(value)


def conv_desc(n, c, h, w, strides, cout, kh, kw, stride, pads, dils):
    """(ConvDesc, {op: workspace bytes}, oh, ow) of one conv product, cached."""
    key = (n, c, h, w, strides, cout, kh, kw, stride, pads, dils, _CONV_MATH[0], get_option(OPT_X3H),
           get_option(OPT_G16_WIDE))
    d = _DESC_CACHE.get(key)
    if d is None:
        p, dl = pads[0], dils[0]
        oh = (h + 2 * p - dl * (kh - 1) - 1) // stride + 1
        ow = (w + 2 * p - dl * (kw - 1) - 1) // stride + 1
        desc = ConvDesc()
        desc.n, desc.c, desc.h, desc.w = n, c, h, w
        for i in range(4):
            desc.in_stride[i] = strides[i]
        desc.k, desc.oh, desc.ow = cout, oh, ow
        desc.kh, desc.kw, desc.stride, desc.nseg = kh, kw, stride, len(pads)
        for i in range(len(pads)):
            desc.pad[i] = pads[i]
            desc.dil[i] = dils[i]
        ws = {}
        for op in (CONV_FWD, CONV_BWD_DATA, CONV_BWD_WEIGHT):
            b = ctypes.c_size_t(0)
            check(_lib.lib().adaptseg_conv2d_workspace_size(ctypes.byref(desc), op, ctypes.byref(b)),
                  "conv2d_workspace_size")
            ws[op] = b.value
        d = _DESC_CACHE[key] = (desc, ws, oh, ow)
    return d


def set_math(math: int) -> None:
    check(_lib.lib().adaptseg_conv_set_math(int(math)), "conv_set_math")
    _CONV_MATH[0] = int(math)


def _wdesc(in_shape, in_stride, w_shape, stride, pad, dil):
    co, _ci, kh, kw = w_shape
    n, c, h, w = in_shape
    return conv_desc(n, c, h, w, tuple(in_stride), co, kh, kw, stride, tuple(pad), tuple(dil))


def _prod(shape):
    out = 1
    for v in shape:
        out *= int(v)
    return out


def _nhwc_strides(n, h, w, c):
    return (h * w * c, 1, w * c, c)


# ---------------------------------------------------------------------------------------
# Registration
# ---------------------------------------------------------------------------------------
def _fake(*args, **kwargs):
    return None


NAMES: list = []        # the ops the engine and the step's own kernels launch
LOSS_NAMES: list = []   # ops of the optional loss terms around the step (engine=False): never in an engine program
MIX_NAMES: list = []    # ops of online self-training (adaptsegnet_amd/mix.py, names=MIX_NAMES): likewise
MIC_NAMES: list = []    # ops of masked image consistency (mix.mask_patches, names=MIC_NAMES): likewise
AUG_NAMES: list = []    # the mixed images' colour jitter and blur (mix.strong_augment, names=AUG_NAMES): likewise
FDA_NAMES: list = []    # FDA's spectral transfer and robust entropy term (adaptsegnet_amd/fda.py, names=FDA_NAMES): likewise
RCS_NAMES: list = []    # rare class sampling's class statistics and crop scores (adaptsegnet_amd/rcs.py, names=RCS_NAMES): likewise


def _op(schema, engine=True, names=None):
    """Define adaptseg::<schema> with the decorated function as its CUDA kernel."""
    name = schema.split("(", 1)[0]

    def deco(fn):
        (names if names is not None else NAMES if engine else LOSS_NAMES).append(name)
        LIB.define(schema)
        LIB.impl(name, fn, "CUDA")
        torch.library.register_fake(f"adaptseg::{name}", _fake, lib=LIB)
        return fn
    return deco


# ---- convolution ------------------------------------------------------------------------
@_op("conv2d_wpack(Tensor[] weight, Tensor(a!) pack, int[] in_shape, int[] in_stride, int[] w_shape, int stride, "
     "int[] pad, int[] dil, int op) -> ()")
def _conv2d_wpack(weight, pack, in_shape, in_stride, w_shape, stride, pad, dil, op):
    d, _, _, _ = _wdesc(in_shape, in_stride, w_shape, stride, pad, dil)
    check(_lib.lib().adaptseg_conv2d_wpack(ctypes.byref(d), int(op), _ptrs(weight), _p(pack), pack.numel(),
                                           _stream()), "conv2d_wpack")


@_op("conv2d_fwd(Tensor? x, Tensor? xb, Tensor[] weight, Tensor? wpack, Tensor?[] bias, Tensor? res, "
     "Tensor(a!)? out, Tensor(b!)? outb, int[] in_shape, int[] in_stride, int[] w_shape, int stride, int[] pad, "
     "int[] dil, int flags) -> ()")
def _conv2d_fwd(x, xb, weight, wpack, bias, res, out, outb, in_shape, in_stride, w_shape, stride, pad, dil, flags):
    d, ws, oh, ow = _wdesc(in_shape, in_stride, w_shape, stride, pad, dil)
    wp, wsz = _ws_args(ws[CONV_FWD], (out if out is not None else outb).device)
    nx, ny = _prod(in_shape), in_shape[0] * oh * ow * w_shape[0]
    check(_lib.lib().adaptseg_conv2d_fwd_x(
        ctypes.byref(d), _pf(x, nx, "conv2d_fwd x"), _pc(xb, nx, "conv2d_fwd xb"), _ptrs(weight), _p(wpack),
        _ptrs(bias) if len(bias) else None, _pf(res, ny, "conv2d_fwd res"),
        _pf(out, ny, "conv2d_fwd out"), _pc(outb, ny, "conv2d_fwd outb"), flags, wp, wsz, _stream()), "conv2d_fwd")


@_op("conv2d_fwd_bnstats(Tensor? x, Tensor? xb, Tensor[] weight, Tensor? wpack, Tensor(a!)? out, Tensor(c!)? outb, "
     "Tensor(b!) stats, int[] in_shape, int[] in_stride, int[] w_shape, int stride, int[] pad, int[] dil, "
     "int ntiles) -> ()")
def _conv2d_fwd_bnstats(x, xb, weight, wpack, out, outb, stats, in_shape, in_stride, w_shape, stride, pad, dil,
                        ntiles):
    d, ws, oh, ow = _wdesc(in_shape, in_stride, w_shape, stride, pad, dil)
    wp, wsz = _ws_args(ws[CONV_FWD], stats.device)
    nt = ctypes.c_int(0)
    nx, ny = _prod(in_shape), in_shape[0] * oh * ow * w_shape[0]
    check(_lib.lib().adaptseg_conv2d_fwd_bnstats_x(
        ctypes.byref(d), _pf(x, nx, "conv2d_fwd_bnstats x"), _pc(xb, nx, "conv2d_fwd_bnstats xb"), _ptrs(weight),
        _p(wpack), _pf(out, ny, "conv2d_fwd_bnstats out"), _pc(outb, ny, "conv2d_fwd_bnstats outb"), _p(stats),
        ctypes.c_size_t(stats.numel() * 4), ctypes.byref(nt), wp, wsz, _stream()), "conv2d_fwd_bnstats")
    if nt.value != ntiles:
        raise RuntimeError(f"conv2d_fwd_bnstats: planned {ntiles} statistics tiles, the launch produced "
                           f"{nt.value} (unaligned operand?)")


def _abn(mean, invstd, bnw, bnb):
    return _lib.OperandBN(mean.data_ptr(), invstd.data_ptr(), None if bnw is None else bnw.data_ptr(),
                          None if bnb is None else bnb.data_ptr())


_ABN_OK: dict = {}


def operand_bn_ok(in_shape, in_stride, w_shape, stride, pad, dil, op) -> bool:
    """adaptseg_conv2d_operand_bn_ok, cached per product (host planning, no GPU)."""
    key = (tuple(in_shape), tuple(in_stride), tuple(w_shape), stride, tuple(pad), tuple(dil), op, _CONV_MATH[0],
           get_option(OPT_X3H), get_option(OPT_G16_WIDE))
    v = _ABN_OK.get(key)
    if v is None:
        d = _wdesc(in_shape, in_stride, w_shape, stride, pad, dil)[0]
        ok = ctypes.c_int(0)
        check(_lib.lib().adaptseg_conv2d_operand_bn_ok(ctypes.byref(d), int(op), ctypes.byref(ok)), "operand_bn_ok")
        v = _ABN_OK[key] = bool(ok.value)
    return v


@_op("conv2d_fwd_bnstats_abn(Tensor x_pre, Tensor mean, Tensor invstd, Tensor? bnw, Tensor? bnb, Tensor[] weight, "
     "Tensor? wpack, Tensor(a!) out, Tensor(b!) stats, int[] in_shape, int[] in_stride, int[] w_shape, int stride, "
     "int[] pad, int[] dil, int ntiles) -> ()")
def _conv2d_fwd_bnstats_abn(x_pre, mean, invstd, bnw, bnb, weight, wpack, out, stats, in_shape, in_stride, w_shape,
                            stride, pad, dil, ntiles):
    """conv2d_fwd_bnstats on relu(bn(x_pre)) — the operand BN folded into the gather
    (adaptseg_conv2d_fwd_bnstats_abn)."""
    d, ws, oh, ow = _wdesc(in_shape, in_stride, w_shape, stride, pad, dil)
    wp, wsz = _ws_args(ws[CONV_FWD], stats.device)
    nt = ctypes.c_int(0)
    nx, ny = _prod(in_shape), in_shape[0] * oh * ow * w_shape[0]
    a = _abn(mean, invstd, bnw, bnb)
    check(_lib.lib().adaptseg_conv2d_fwd_bnstats_abn(
        ctypes.byref(d), _pf(x_pre, nx, "conv2d_fwd_bnstats_abn x_pre"), ctypes.byref(a), _ptrs(weight), _p(wpack),
        _pf(out, ny, "conv2d_fwd_bnstats_abn out"), _p(stats), ctypes.c_size_t(stats.numel() * 4), ctypes.byref(nt),
        wp, wsz, _stream()), "conv2d_fwd_bnstats_abn")
    if nt.value != ntiles:
        raise RuntimeError(f"conv2d_fwd_bnstats_abn: planned {ntiles} statistics tiles, the launch produced "
                           f"{nt.value} (unaligned operand?)")


@_op("conv2d_bwd_weight_abn(Tensor dy, Tensor x_pre, Tensor mean, Tensor invstd, Tensor? bnw, Tensor? bnb, "
     "Tensor(a!)[] dw, int[] in_shape, int[] in_stride, int[] w_shape, int stride, int[] pad, int[] dil, "
     "int flags) -> ()")
def _conv2d_bwd_weight_abn(dy, x_pre, mean, invstd, bnw, bnb, dw, in_shape, in_stride, w_shape, stride, pad, dil,
                           flags):
    """conv2d_bwd_weight with the x operand relu(bn(x_pre)) (adaptseg_conv2d_bwd_weight_abn)."""
    d, ws, oh, ow = _wdesc(in_shape, in_stride, w_shape, stride, pad, dil)
    wp, wsz = _ws_args(ws[CONV_BWD_WEIGHT], dw[0].device)
    nx, ny = _prod(in_shape), in_shape[0] * oh * ow * w_shape[0]
    a = _abn(mean, invstd, bnw, bnb)
    check(_lib.lib().adaptseg_conv2d_bwd_weight_abn(
        ctypes.byref(d), _pf(dy, ny, "conv2d_bwd_weight_abn dy"), _pf(x_pre, nx, "conv2d_bwd_weight_abn x_pre"),
        ctypes.byref(a), _ptrs(dw), flags, wp, wsz, _stream()), "conv2d_bwd_weight_abn")


@_op("bn_fwd_train_tiles_stats(Tensor stats, int ntiles, int rows, int c, Tensor(a!)? running_mean, "
     "Tensor(b!)? running_var, Tensor(d!) mean, Tensor(e!) invstd, float momentum, float eps) -> ()")
def _bn_fwd_train_tiles_stats(stats, ntiles, rows, c, running_mean, running_var, mean, invstd, momentum, eps):
    check(_lib.lib().adaptseg_bn_fwd_train_tiles_stats(
        int(rows), int(c), _p(stats), int(ntiles), _p(running_mean), _p(running_var), float(momentum), float(eps),
        _p(mean), _p(invstd), _stream()), "bn_fwd_train_tiles_stats")


@_op("conv2d_bwd_data(Tensor? dy, Tensor? dyb, Tensor[] weight, Tensor? wpack, Tensor? res, Tensor? resbits, "
     "Tensor? aux, Tensor(a!)? dx, Tensor(b!)? dxb, int[] in_shape, int[] w_shape, int stride, int[] pad, "
     "int[] dil, int flags) -> ()")
def _conv2d_bwd_data(dy, dyb, weight, wpack, res, resbits, aux, dx, dxb, in_shape, w_shape, stride, pad, dil, flags):
    """res: fp32 or bf16, masked by the bitmap resbits (int32 [rows, Cin / 32]) when given; dx None:
    the output is stored in bf16 only (dxb) — bf16 gradient storage (adaptseg_conv2d_bwd_data_xg)."""
    n, c, h, w = in_shape
    d, ws, oh, ow = _wdesc(in_shape, _nhwc_strides(n, h, w, c), w_shape, stride, pad, dil)
    wp, wsz = _ws_args(ws[CONV_BWD_DATA], (dx if dx is not None else dxb).device)
    nx, ny = n * h * w * c, n * oh * ow * w_shape[0]
    check(_lib.lib().adaptseg_conv2d_bwd_data_xg(
        ctypes.byref(d), _pf(dy, ny, "conv2d_bwd_data dy"), _pc(dyb, ny, "conv2d_bwd_data dyb"), _ptrs(weight),
        _p(wpack), *_pfb(res, nx, "conv2d_bwd_data res"), _pbits(resbits, nx, "conv2d_bwd_data resbits"),
        _pf(aux, nx, "conv2d_bwd_data aux"),
        _pf(dx, nx, "conv2d_bwd_data dx"), _pc(dxb, nx, "conv2d_bwd_data dxb"), flags, wp, wsz, _stream()),
        "conv2d_bwd_data")


@_op("conv2d_bwd_data_bnsum(Tensor? dy, Tensor? dyb, Tensor[] weight, Tensor? wpack, Tensor? res, Tensor? resbits, "
     "Tensor(a!)? dx, Tensor(b!)? dxb, int[] in_shape, int[] w_shape, int stride, int[] pad, int[] dil, int flags, "
     "Tensor bnx, Tensor mean, Tensor invstd, Tensor? bnw, Tensor? bnb, Tensor? bits, int mask, Tensor(c!) partial, "
     "int ntiles) -> ()")
def _conv2d_bwd_data_bnsum(dy, dyb, weight, wpack, res, resbits, dx, dxb, in_shape, w_shape, stride, pad, dil, flags,
                           bnx, mean, invstd, bnw, bnb, bits, mask, partial, ntiles):
    """conv2d_bwd_data that also writes the fused BN backward sums of its output (the BN whose
    incoming gradient it is; adaptseg_conv2d_bwd_data_bnsum) into partial [2][Cin][ntiles]."""
    n, c, h, w = in_shape
    d, ws, oh, ow = _wdesc(in_shape, _nhwc_strides(n, h, w, c), w_shape, stride, pad, dil)
    wp, wsz = _ws_args(ws[CONV_BWD_DATA], partial.device)
    nx, ny = n * h * w * c, n * oh * ow * w_shape[0]
    if partial.dtype != torch.float32 or partial.numel() != 2 * c * ntiles:
        raise RuntimeError(f"conv2d_bwd_data_bnsum: partial must be float32 [2][{c}][{ntiles}]")
    bs = _lib.BnSumDesc()
    bs.x, bs.x_bf16 = _pfb(bnx, nx, "conv2d_bwd_data_bnsum bnx")
    bs.mean, bs.invstd, bs.weight, bs.bias = _p(mean), _p(invstd), _p(bnw), _p(bnb)
    bs.bits = _pbits(bits, nx, "conv2d_bwd_data_bnsum bits")
    bs.mask = int(mask)
    bs.partial = _p(partial)
    bs.partial_bytes = partial.numel() * 4
    nt = ctypes.c_int(0)
    check(_lib.lib().adaptseg_conv2d_bwd_data_bnsum(
        ctypes.byref(d), _pf(dy, ny, "conv2d_bwd_data_bnsum dy"), _pc(dyb, ny, "conv2d_bwd_data_bnsum dyb"),
        _ptrs(weight), _p(wpack), *_pfb(res, nx, "conv2d_bwd_data_bnsum res"),
        _pbits(resbits, nx, "conv2d_bwd_data_bnsum resbits"), _pf(dx, nx, "conv2d_bwd_data_bnsum dx"),
        _pc(dxb, nx, "conv2d_bwd_data_bnsum dxb"), flags, ctypes.byref(bs), ctypes.byref(nt), wp, wsz, _stream()),
        "conv2d_bwd_data_bnsum")
    if nt.value != ntiles:
        raise RuntimeError(f"conv2d_bwd_data_bnsum: planned {ntiles} BN-sum tiles, the launch produced {nt.value} "
                           f"(unaligned operand?)")


@_op("conv2d_bwd_weight(Tensor? dy, Tensor? dyb, Tensor? x, Tensor? xb, Tensor(a!)[] dw, Tensor(b!)[] db, "
     "int[] in_shape, int[] in_stride, int[] w_shape, int stride, int[] pad, int[] dil, int flags) -> ()")
def _conv2d_bwd_weight(dy, dyb, x, xb, dw, db, in_shape, in_stride, w_shape, stride, pad, dil, flags):
    d, ws, oh, ow = _wdesc(in_shape, in_stride, w_shape, stride, pad, dil)
    if flags & WGRAD_DEFER_SUM:
        # a deferred split-K sum reads this call's partial outputs at the flush: a workspace of
        # its own, kept until splitk_flush (allocated on the current stream, where the flush runs)
        nb = ws[CONV_BWD_WEIGHT]
        w = torch.empty(nb, dtype=torch.uint8, device=dw[0].device) if nb else None
        if w is not None:
            _DEFERRED_WS.setdefault(torch.cuda.current_stream(dw[0].device).cuda_stream, []).append(w)
        wp, wsz = (ctypes.c_void_p(w.data_ptr()) if w is not None else None), ctypes.c_size_t(nb)
    else:
        wp, wsz = _ws_args(ws[CONV_BWD_WEIGHT], dw[0].device)
    nx, ny = _prod(in_shape), in_shape[0] * oh * ow * w_shape[0]
    check(_lib.lib().adaptseg_conv2d_bwd_weight_x(
        ctypes.byref(d), _pf(dy, ny, "conv2d_bwd_weight dy"), _pc(dyb, ny, "conv2d_bwd_weight dyb"),
        _pf(x, nx, "conv2d_bwd_weight x"), _pc(xb, nx, "conv2d_bwd_weight xb"), _ptrs(dw),
        _ptrs(db) if len(db) else None, flags, wp, wsz, _stream()), "conv2d_bwd_weight")


WGRAD_DEFER_SUM = 64   # adaptseg.h ADAPTSEG_WGRAD_DEFER_SUM
_DEFERRED_WS: dict = {}   # stream handle -> workspaces of the weight gradients whose sums are pending


def splitk_flush(device=None) -> None:
    """adaptseg_splitk_flush on the current stream: launch the split-K sums the weight gradients
    issued with WGRAD_DEFER_SUM left pending on it, then release their workspaces (freed in
    stream order: the caching allocator reuses them only after the sums on this stream)."""
    s = torch.cuda.current_stream(device)
    check(_lib.lib().adaptseg_splitk_flush(ctypes.c_void_p(s.cuda_stream)), "splitk_flush")
    _DEFERRED_WS.pop(s.cuda_stream, None)


def splitk_pending(device=None) -> int:
    n = ctypes.c_int(0)
    s = torch.cuda.current_stream(device)
    check(_lib.lib().adaptseg_splitk_pending(ctypes.c_void_p(s.cuda_stream), ctypes.byref(n)), "splitk_pending")
    return n.value


# ---- batch norm (x as [rows, C]: the NHWC buffer) ------------------------------------------
_BN_WS: dict = {}


def bn_ws_bytes(rows, c):
    v = _BN_WS.get((rows, c))
    if v is None:
        b = ctypes.c_size_t(0)
        check(_lib.lib().adaptseg_bn_workspace_size(rows, c, ctypes.byref(b)), "bn_workspace_size")
        v = _BN_WS[(rows, c)] = b.value
    return v


def _rc(t):
    c = t.shape[-1]
    return t.numel() // c, c


def _fb(t):
    """(fp32 pointer, bf16 pointer) of an activation operand stored as either."""
    if t is None:
        return None, None
    return (None, _p(t)) if t.dtype == torch.bfloat16 else (_p(t), None)


@_op("bn_fwd_train(Tensor x, Tensor? weight, Tensor? bias, Tensor(a!)? running_mean, Tensor(b!)? running_var, "
     "Tensor? res, Tensor(c!)? y, Tensor(f!)? yb, Tensor(g!)? ybits, Tensor(d!) mean, Tensor(e!) invstd, "
     "float momentum, float eps, int act) -> ()")
def _bn_fwd_train(x, weight, bias, running_mean, running_var, res, y, yb, ybits, mean, invstd, momentum, eps, act):
    """x / res: fp32 or bf16 (bf16 activation storage, config c5); ybits: the ReLU mask bitmap of y
    (int32 [rows, C / 32]) or None."""
    rows, c = _rc(x)
    n = rows * c
    wp, wsz = _ws_args(bn_ws_bytes(rows, c), x.device)
    check(_lib.lib().adaptseg_bn_fwd_train_xm(
        rows, c, *_pfb(x, n, "bn_fwd_train x"), _p(weight), _p(bias), _p(running_mean), _p(running_var),
        float(momentum), float(eps), _p(mean), _p(invstd), *_pfb(res, n, "bn_fwd_train res"),
        _pf(y, n, "bn_fwd_train y"), _pc(yb, n, "bn_fwd_train yb"), _pbits(ybits, n, "bn_fwd_train ybits"),
        int(act), wp, wsz, _stream()), "bn_fwd_train")


@_op("bn_fwd_train_tiles(Tensor x, Tensor stats, int ntiles, Tensor? weight, Tensor? bias, "
     "Tensor(a!)? running_mean, Tensor(b!)? running_var, Tensor? res, Tensor(c!)? y, Tensor(f!)? yb, "
     "Tensor(g!)? ybits, Tensor(d!) mean, Tensor(e!) invstd, float momentum, float eps, int act) -> ()")
def _bn_fwd_train_tiles(x, stats, ntiles, weight, bias, running_mean, running_var, res, y, yb, ybits, mean, invstd,
                        momentum, eps, act):
    rows, c = _rc(x)
    n = rows * c
    check(_lib.lib().adaptseg_bn_fwd_train_tiles_xm(
        rows, c, _p(stats), int(ntiles), *_pfb(x, n, "bn_fwd_train_tiles x"), _p(weight), _p(bias),
        _p(running_mean), _p(running_var), float(momentum), float(eps), _p(mean), _p(invstd),
        *_pfb(res, n, "bn_fwd_train_tiles res"), _pf(y, n, "bn_fwd_train_tiles y"),
        _pc(yb, n, "bn_fwd_train_tiles yb"), _pbits(ybits, n, "bn_fwd_train_tiles ybits"), int(act), _stream()),
        "bn_fwd_train_tiles")


@_op("bn_fwd_infer(Tensor x, Tensor? weight, Tensor? bias, Tensor running_mean, Tensor running_var, "
     "Tensor? res, Tensor(a!)? y, Tensor(b!)? yb, Tensor(c!)? ybits, float eps, int act) -> ()")
def _bn_fwd_infer(x, weight, bias, running_mean, running_var, res, y, yb, ybits, eps, act):
    rows, c = _rc(x)
    n = rows * c
    check(_lib.lib().adaptseg_bn_fwd_infer_xm(
        rows, c, *_pfb(x, n, "bn_fwd_infer x"), _p(weight), _p(bias), _p(running_mean), _p(running_var),
        float(eps), *_pfb(res, n, "bn_fwd_infer res"), _pf(y, n, "bn_fwd_infer y"), _pc(yb, n, "bn_fwd_infer yb"),
        _pbits(ybits, n, "bn_fwd_infer ybits"), int(act), _stream()), "bn_fwd_infer")


@_op("bn_bwd(Tensor dy, Tensor? dybits, Tensor? y, Tensor? x, Tensor? weight, Tensor? bias, Tensor? mean, "
     "Tensor invstd, Tensor(a!)? dx, Tensor(c!)? dxb, Tensor(b!)? dres, int act, bool train) -> ()")
def _bn_bwd(dy, dybits, y, x, weight, bias, mean, invstd, dx, dxb, dres, act, train):
    """y / x (the saved activations): fp32 or bf16; dy and dres fp32, or both bf16 (bf16 gradient
    storage, adaptseg_bn_bwd_xg); dx fp32; dybits: a mask bitmap applied to dy (or None)."""
    rows, c = _rc(dy)
    n = rows * c
    wp, wsz = _ws_args(bn_ws_bytes(rows, c) if train else 0, dy.device)
    check(_lib.lib().adaptseg_bn_bwd_xg(
        rows, c, *_pfb(dy, n, "bn_bwd dy"), _pbits(dybits, n, "bn_bwd dybits"), *_pfb(y, n, "bn_bwd y"),
        *_pfb(x, n, "bn_bwd x"), _p(weight), _p(bias), _p(mean), _p(invstd), _pf(dx, n, "bn_bwd dx"),
        _pc(dxb, n, "bn_bwd dxb"), *_pfb(dres, n, "bn_bwd dres"), int(act), 1 if train else 0, wp, wsz, _stream()),
        "bn_bwd")


@_op("bn_bwd_sums(Tensor dy, Tensor? dybits, Tensor? y, Tensor? x, Tensor? weight, Tensor? bias, Tensor mean, "
     "Tensor invstd, Tensor(a!)? dx, Tensor(c!)? dxb, Tensor(b!)? dres, int act, Tensor partial, int ntiles) -> ()")
def _bn_bwd_sums(dy, dybits, y, x, weight, bias, mean, invstd, dx, dxb, dres, act, partial, ntiles):
    """bn_bwd in train mode whose reduction the producing data gradient's epilogue already did
    (conv2d_bwd_data_bnsum): adaptseg_bn_bwd_sums."""
    rows, c = _rc(dy)
    n = rows * c
    if partial.dtype != torch.float32 or partial.numel() != 2 * c * ntiles:
        raise RuntimeError(f"bn_bwd_sums: partial must be float32 [2][{c}][{ntiles}]")
    wp, wsz = _ws_args(bn_ws_bytes(rows, c), dy.device)
    check(_lib.lib().adaptseg_bn_bwd_sums(
        rows, c, *_pfb(dy, n, "bn_bwd_sums dy"), _pbits(dybits, n, "bn_bwd_sums dybits"), *_pfb(y, n, "bn_bwd_sums y"),
        *_pfb(x, n, "bn_bwd_sums x"), _p(weight), _p(bias), _p(mean), _p(invstd), _pf(dx, n, "bn_bwd_sums dx"),
        _pc(dxb, n, "bn_bwd_sums dxb"), *_pfb(dres, n, "bn_bwd_sums dres"), int(act), _p(partial), int(ntiles), wp,
        wsz, _stream()), "bn_bwd_sums")


@_op("bn_bwd_affine(Tensor dy, Tensor? y, Tensor x, Tensor? weight, Tensor? bias, Tensor mean, "
     "Tensor invstd, Tensor(a!) dx, int act, Tensor(b!)? dweight, Tensor(c!)? dbias) -> ()")
def _bn_bwd_affine(dy, y, x, weight, bias, mean, invstd, dx, act, dweight, dbias):
    rows, c = _rc(dy)
    wp, wsz = _ws_args(bn_ws_bytes(rows, c), dy.device)
    check(_lib.lib().adaptseg_bn_bwd_affine(
        rows, c, _p(dy), _p(y), _p(x), _p(weight), _p(bias), _p(mean), _p(invstd), _p(dx), None, int(act),
        _p(dweight), _p(dbias), wp, wsz, _stream()), "bn_bwd_affine")


# ---- warper -------------------------------------------------------------------------------
@_op("up2_relu_cat_fwd(Tensor? s, Tensor d, Tensor(a!) out) -> ()")
def _up2_relu_cat_fwd(s, d, out):
    n, h, w, cd = d.shape
    cs = 0 if s is None else s.shape[-1]
    check(_lib.lib().adaptseg_up2_relu_cat_fwd(n, h, w, cs, cd, _p(s), _p(d), _p(out), _stream()),
          "up2_relu_cat_fwd")


@_op("up2_relu_cat_bwd(Tensor? s, Tensor d, Tensor dout, Tensor(a!)? ds, Tensor(b!) dd) -> ()")
def _up2_relu_cat_bwd(s, d, dout, ds, dd):
    n, h, w, cd = d.shape
    cs = 0 if s is None else s.shape[-1]
    check(_lib.lib().adaptseg_up2_relu_cat_bwd(n, h, w, cs, cd, _p(s), _p(d), _p(dout), _p(ds), _p(dd),
                                               _stream()), "up2_relu_cat_bwd")


@_op("grid_warp_fwd(Tensor flow, Tensor? x1, Tensor x2, Tensor(a!)? y1, Tensor(b!) y2) -> ()")
def _grid_warp_fwd(flow, x1, x2, y1, y2):
    n, h, w, c = x2.shape
    check(_lib.lib().adaptseg_grid_warp_fwd(n, c, h, w, flow.shape[-1], _p(flow), _p(x1), _p(x2), _p(y1),
                                            _p(y2), _stream()), "grid_warp_fwd")


@_op("grid_warp_bwd(Tensor flow, Tensor? x1, Tensor? x2, Tensor? dy1, Tensor? dy2, Tensor(a!)? dflow, "
     "Tensor(b!)? dx1, Tensor(c!)? dx2) -> ()")
def _grid_warp_bwd(flow, x1, x2, dy1, dy2, dflow, dx1, dx2):
    ref = dy2 if dy2 is not None else dy1
    n, h, w, c = ref.shape
    nbytes = 0
    if dx1 is not None or dx2 is not None:
        b = ctypes.c_size_t(0)
        check(_lib.lib().adaptseg_grid_warp_bwd_workspace_size(n, c, h, w, ctypes.byref(b)),
              "grid_warp_bwd_workspace_size")
        nbytes = b.value
    wp, wsz = _ws_args(nbytes, ref.device)
    check(_lib.lib().adaptseg_grid_warp_bwd(
        n, c, h, w, flow.shape[-1], _p(flow), _p(x1), _p(x2), _p(dy1), _p(dy2), _p(dflow), _p(dx1), _p(dx2),
        wp, wsz, _stream()), "grid_warp_bwd")


# ---- pooling / interpolation / softmax / losses ------------------------------------------
@_op("maxpool2d_fwd(Tensor x, Tensor(a!) y, Tensor(b!) argmax, Tensor(c!)? y_terms, int k, int s, int p) -> ()")
def _maxpool2d_fwd(x, y, argmax, y_terms, k, s, p):
    """y_terms: the pooled output's F32X3 term images [n, oh, ow, 3, c] (bf16) or None."""
    n, h, w, c = x.shape
    oh, ow = y.shape[1], y.shape[2]
    check(_lib.lib().adaptseg_maxpool2d_fwd_x(n, c, h, w, oh, ow, k, s, p, _p(x), _p(y), _p(argmax), _p(y_terms),
                                              _stream()), "maxpool2d_fwd")


@_op("maxpool2d_bwd(Tensor dy, Tensor argmax, Tensor(a!) dx, Tensor(b!)? dx_terms, int k, int s, int p) -> ()")
def _maxpool2d_bwd(dy, argmax, dx, dx_terms, k, s, p):
    """dx_terms: the routed gradient's F32X3 term images [n, h, w, 3, c] (bf16) or None."""
    n, oh, ow, c = dy.shape
    h, w = dx.shape[1], dx.shape[2]
    check(_lib.lib().adaptseg_maxpool2d_bwd_x(n, c, h, w, oh, ow, k, s, p, _p(dy), _p(argmax), _p(dx), _p(dx_terms),
                                              _stream()), "maxpool2d_bwd")


@_op("upsample_bilinear_fwd(Tensor x, Tensor(a!) y) -> ()")
def _upsample_bilinear_fwd(x, y):
    n, h, w, c = x.shape
    check(_lib.lib().adaptseg_upsample_bilinear_fwd(n, c, h, w, y.shape[1], y.shape[2], _p(x), _p(y), _stream()),
          "upsample_bilinear_fwd")


@_op("upsample_bilinear_bwd(Tensor dy, Tensor(a!) dx, bool accumulate) -> ()")
def _upsample_bilinear_bwd(dy, dx, accumulate):
    n, oh, ow, c = dy.shape
    h, w = dx.shape[1], dx.shape[2]
    wp, wsz = _ws_args(n * oh * w * c * 4, dy.device)
    check(_lib.lib().adaptseg_upsample_bilinear_bwd(n, c, h, w, oh, ow, _p(dy), _p(dx),
                                                    _lib.EPI_ACCUMULATE if accumulate else 0, wp, wsz,
                                                    _stream()), "upsample_bilinear_bwd")


@_op("softmax_fwd(Tensor x, Tensor(a!) y) -> ()")
def _softmax_fwd(x, y):
    rows, c = _rc(x)
    check(_lib.lib().adaptseg_softmax_fwd(rows, c, _p(x), _p(y), _stream()), "softmax_fwd")


@_op("softmax_bwd(Tensor y, Tensor dy, Tensor(a!) dx, bool accumulate) -> ()")
def _softmax_bwd(y, dy, dx, accumulate):
    rows, c = _rc(y)
    check(_lib.lib().adaptseg_softmax_bwd(rows, c, _p(y), _p(dy), _p(dx),
                                          _lib.EPI_ACCUMULATE if accumulate else 0, _stream()), "softmax_bwd")


@_op("softmax_ce_fwd(Tensor logits, Tensor labels, int ignore, Tensor? weight, Tensor(a!) out) -> ()")
def _softmax_ce_fwd(logits, labels, ignore, weight, out):
    rows, c = _rc(logits)
    b = ctypes.c_size_t(0)
    check(_lib.lib().adaptseg_ce_workspace_size(rows, ctypes.byref(b)), "ce_workspace_size")
    wp, wsz = _ws_args(b.value, logits.device)
    check(_lib.lib().adaptseg_softmax_ce_fwd(rows, c, _p(logits), _p(labels), int(ignore), _p(weight), _p(out),
                                             wp, wsz, _stream()), "softmax_ce_fwd")


@_op("softmax_ce_bwd(Tensor logits, Tensor labels, Tensor out, Tensor grad_loss, int ignore, Tensor? weight, "
     "Tensor(a!) dlogits, bool accumulate) -> ()")
def _softmax_ce_bwd(logits, labels, out, grad_loss, ignore, weight, dlogits, accumulate):
    rows, c = _rc(logits)
    check(_lib.lib().adaptseg_softmax_ce_bwd(rows, c, _p(logits), _p(labels), int(ignore), _p(weight), _p(out),
                                             _p(grad_loss), _p(dlogits),
                                             _lib.EPI_ACCUMULATE if accumulate else 0, _stream()),
          "softmax_ce_bwd")


@_op("adv_loss_fwd(Tensor x, float target, int kind, Tensor(a!) loss) -> ()")
def _adv_loss_fwd(x, target, kind, loss):
    n = x.numel()
    b = ctypes.c_size_t(0)
    check(_lib.lib().adaptseg_adv_workspace_size(n, ctypes.byref(b)), "adv_workspace_size")
    wp, wsz = _ws_args(b.value, x.device)
    check(_lib.lib().adaptseg_adv_loss_fwd(n, _p(x), float(target), int(kind), _p(loss), wp, wsz, _stream()),
          "adv_loss_fwd")


@_op("adv_loss_bwd(Tensor x, float target, int kind, Tensor grad_loss, Tensor(a!) dx, bool accumulate) -> ()")
def _adv_loss_bwd(x, target, kind, grad_loss, dx, accumulate):
    check(_lib.lib().adaptseg_adv_loss_bwd(x.numel(), _p(x), float(target), int(kind), _p(grad_loss), _p(dx),
                                           _lib.EPI_ACCUMULATE if accumulate else 0, _stream()), "adv_loss_bwd")


# ---- entropy-based adaptation (ADVENT): x = logits [..., c], see include/adaptseg.h -------------
@_op("selfinfo_fwd(Tensor x, Tensor(a!) y) -> ()", engine=False)
def _selfinfo_fwd(x, y):
    rows, c = _rc(x)
    n = rows * c
    check(_lib.lib().adaptseg_selfinfo_fwd(rows, c, _pf(x, n, "selfinfo_fwd x"), _pf(y, n, "selfinfo_fwd y"),
                                           _stream()), "selfinfo_fwd")


@_op("selfinfo_bwd(Tensor x, Tensor dy, Tensor(a!) dx, bool accumulate) -> ()", engine=False)
def _selfinfo_bwd(x, dy, dx, accumulate):
    rows, c = _rc(x)
    n = rows * c
    check(_lib.lib().adaptseg_selfinfo_bwd(rows, c, _pf(x, n, "selfinfo_bwd x"), _pf(dy, n, "selfinfo_bwd dy"),
                                           _pf(dx, n, "selfinfo_bwd dx"),
                                           _lib.EPI_ACCUMULATE if accumulate else 0, _stream()), "selfinfo_bwd")


@_op("entropy_loss_fwd(Tensor x, Tensor(a!) loss) -> ()", engine=False)
def _entropy_loss_fwd(x, loss):
    rows, c = _rc(x)
    b = ctypes.c_size_t(0)
    check(_lib.lib().adaptseg_entropy_workspace_size(rows, ctypes.byref(b)), "entropy_workspace_size")
    wp, wsz = _ws_args(b.value, x.device)
    check(_lib.lib().adaptseg_entropy_loss_fwd(rows, c, _pf(x, rows * c, "entropy_loss_fwd x"),
                                               _pf(loss, 1, "entropy_loss_fwd loss"), wp, wsz, _stream()),
          "entropy_loss_fwd")


@_op("entropy_loss_bwd(Tensor x, Tensor grad_loss, Tensor(a!) dx, bool accumulate) -> ()", engine=False)
def _entropy_loss_bwd(x, grad_loss, dx, accumulate):
    rows, c = _rc(x)
    n = rows * c
    check(_lib.lib().adaptseg_entropy_loss_bwd(rows, c, _pf(x, n, "entropy_loss_bwd x"),
                                               _pf(grad_loss, 1, "entropy_loss_bwd grad_loss"),
                                               _pf(dx, n, "entropy_loss_bwd dx"),
                                               _lib.EPI_ACCUMULATE if accumulate else 0, _stream()),
          "entropy_loss_bwd")


# ---- optimisers and plumbing ----------------------------------------------------------------
@_op("sgd_step(Tensor(a!) param, Tensor grad, Tensor(b!) momentum_buffer, float lr, float momentum, "
     "float weight_decay, float grad_scale, int multiplicity, bool first_step) -> ()")
def _sgd_step(param, grad, momentum_buffer, lr, momentum, weight_decay, grad_scale, multiplicity, first_step):
    check(_lib.lib().adaptseg_sgd_step(param.numel(), _p(param), _p(grad), _p(momentum_buffer), float(lr),
                                       float(momentum), float(weight_decay), float(grad_scale), int(multiplicity),
                                       1 if first_step else 0, _stream()), "sgd_step")


@_op("adam_step(Tensor(a!) param, Tensor grad, Tensor(b!) exp_avg, Tensor(c!) exp_avg_sq, float lr, "
     "float beta1, float beta2, float eps, int step, float grad_scale) -> ()")
def _adam_step(param, grad, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, step, grad_scale):
    check(_lib.lib().adaptseg_adam_step(param.numel(), _p(param), _p(grad), _p(exp_avg), _p(exp_avg_sq),
                                        float(lr), float(beta1), float(beta2), float(eps), int(step),
                                        float(grad_scale), _stream()), "adam_step")


@_op("zero(Tensor(a!) t) -> ()")
def _zero(t):
    check(_lib.lib().adaptseg_zero(_p(t), t.numel() * t.element_size(), _stream()), "zero")


@_op("to_nhwc(Tensor x, Tensor(a!) out) -> ()")
def _to_nhwc(x, out):
    n, c, h, w = x.shape
    st = (ctypes.c_int64 * 4)(*x.stride())
    check(_lib.lib().adaptseg_to_nhwc(n, c, h, w, st, _p(x), _p(out), _stream()), "to_nhwc")


@_op("to_nhwc_pad(Tensor x, Tensor(a!) out, bool accumulate) -> ()")
def _to_nhwc_pad(x, out, accumulate):
    """out [n, h, w, c_dst] (=|+=) x (NCHW-shaped, any strides), channels >= c zero."""
    n, c, h, w = x.shape
    st = (ctypes.c_int64 * 4)(*x.stride())
    check(_lib.lib().adaptseg_to_nhwc_pad(n, c, h, w, st, _p(x), out.shape[-1], _p(out),
                                          _lib.EPI_ACCUMULATE if accumulate else 0, _stream()), "to_nhwc_pad")


@_op("axpy(float alpha, Tensor src, Tensor(a!) dst, bool accumulate) -> ()")
def _axpy(alpha, src, dst, accumulate):
    check(_lib.lib().adaptseg_axpy(src.numel(), float(alpha), _p(src), _p(dst),
                                   _lib.EPI_ACCUMULATE if accumulate else 0, _stream()), "axpy")


@_op("add_i64(Tensor(a!) t, int v) -> ()")
def _add_i64(t, v):
    check(_lib.lib().adaptseg_add_i64(_p(t), t.numel(), int(v), _stream()), "add_i64")


# ---- input pipeline and evaluation -----------------------------------------------
@_op("gta5_preprocess(Tensor images, float[] mean, Tensor(a!) out, Tensor? labels, Tensor? lut, "
     "Tensor(b!)? labels_out) -> ()")
def _gta5_preprocess(images, mean, out, labels, lut, labels_out):
    n, h, w, _ = images.shape
    oh, ow = out.shape[2], out.shape[3]
    b = ctypes.c_size_t(0)
    check(_lib.lib().adaptseg_preprocess_workspace_size(n, h, w, oh, ow, ctypes.byref(b)),
          "preprocess_workspace_size")
    wp, wsz = _ws_args(b.value, images.device)
    check(_lib.lib().adaptseg_gta5_preprocess(
        n, h, w, oh, ow, _p(images), float(mean[0]), float(mean[1]), float(mean[2]), _p(out), _p(labels),
        _p(lut) if labels is not None else None, _p(labels_out), wp, wsz, _stream()), "gta5_preprocess")


@_op("gta5_preprocess_augment(Tensor images, float[] mean, int[] params, int ignore_label, Tensor(a!) out, "
     "Tensor? labels, Tensor? lut, Tensor(b!)? labels_out) -> ()")
def _gta5_preprocess_augment(images, mean, params, ignore_label, out, labels, lut, labels_out):
    """params: the flattened host array [n][5] = (sw, sh, ox, oy, mirror) of include/adaptseg.h."""
    n, h, w, _ = images.shape
    oh, ow = out.shape[2], out.shape[3]
    if len(params) != 5 * n:
        raise RuntimeError(f"gta5_preprocess_augment: expected {5 * n} params for {n} images, got {len(params)}")
    pa = (ctypes.c_int32 * (5 * n))(*params)
    b = ctypes.c_size_t(0)
    check(_lib.lib().adaptseg_preprocess_augment_workspace_size(n, h, w, oh, ow, pa, ctypes.byref(b)),
          "preprocess_augment_workspace_size")
    wp, wsz = _ws_args(b.value, images.device)
    check(_lib.lib().adaptseg_gta5_preprocess_augment(
        n, h, w, oh, ow, _p(images), float(mean[0]), float(mean[1]), float(mean[2]), _p(out), _p(labels),
        _p(lut) if labels is not None else None, _p(labels_out), pa, int(ignore_label), wp, wsz, _stream()),
        "gta5_preprocess_augment")


@_op("upsample_argmax(Tensor x, Tensor(a!) out) -> ()")
def _upsample_argmax(x, out):
    n, h, w, c = x.shape
    check(_lib.lib().adaptseg_upsample_argmax(n, c, h, w, out.shape[1], out.shape[2], _p(x), _p(out), _stream()),
          "upsample_argmax")


@_op("fuse_argmax(Tensor[] maps, int[] mirror, int mode, Tensor(a!) out, Tensor(b!)? conf) -> ()")
def _fuse_argmax(maps, mirror, mode, out, conf):
    """maps: NHWC fp32 buffers [n, h_s, w_s, c]; mirror: one flag per map; mode: _lib.FUSE_PROB / FUSE_LOGIT."""
    if not 1 <= len(maps) <= _lib.FUSE_MAX_MAPS or len(mirror) != len(maps):
        raise RuntimeError(f"fuse_argmax: {len(maps)} maps (1..{_lib.FUSE_MAX_MAPS}) with {len(mirror)} mirror flags")
    n, _, _, c = maps[0].shape
    d = _lib.FuseDesc()
    d.n, d.c, d.oh, d.ow, d.nmaps, d.mode = n, c, out.shape[1], out.shape[2], len(maps), int(mode)
    for s, x in enumerate(maps):
        if x.dim() != 4 or x.shape[0] != n or x.shape[3] != c or not x.is_contiguous():
            raise RuntimeError(f"fuse_argmax: map {s} is {tuple(x.shape)}, expected a contiguous [{n}, h, w, {c}]")
        d.h[s], d.w[s], d.mirror[s] = x.shape[1], x.shape[2], int(bool(mirror[s]))
        d.x[s] = _pf(x, x.numel(), f"fuse_argmax map {s}").value
    if out.dtype != torch.uint8 or out.shape[0] != n or not out.is_contiguous():
        raise RuntimeError(f"fuse_argmax: out is {out.dtype} {tuple(out.shape)}, expected contiguous uint8 [{n}, H, W]")
    if conf is not None and (conf.shape != out.shape or not conf.is_contiguous()):
        raise RuntimeError(f"fuse_argmax: conf is {tuple(conf.shape)}, expected contiguous {tuple(out.shape)}")
    check(_lib.lib().adaptseg_fuse_argmax(ctypes.byref(d), _p(out), _pf(conf, out.numel(), "fuse_argmax conf"),
                                          _stream()), "fuse_argmax")


@_op("confusion_hist(Tensor gt_ids, Tensor lut, Tensor pred, int num_classes, Tensor(a!) hist) -> ()")
def _confusion_hist(gt_ids, lut, pred, num_classes, hist):
    check(_lib.lib().adaptseg_confusion_hist(gt_ids.numel(), _p(gt_ids), _p(lut), _p(pred), int(num_classes),
                                             _p(hist), _stream()), "confusion_hist")


# ---- pseudo-labels for self-training (adaptsegnet_amd/pseudo.py) ---------------------------------
def _pseudo_maps(pred, conf, what):
    if pred.dtype != torch.uint8 or not pred.is_contiguous():
        raise RuntimeError(f"{what}: pred is {pred.dtype} {tuple(pred.shape)}, expected a contiguous uint8 class map")
    if not conf.is_contiguous():
        raise RuntimeError(f"{what}: conf {tuple(conf.shape)} is not contiguous")
    return _p(pred), _pf(conf, pred.numel(), f"{what} conf")


def _pi64(t, shape, what):
    if t.dtype != torch.int64 or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise RuntimeError(f"{what}: expected a contiguous int64 {tuple(shape)}, got {t.dtype} {tuple(t.shape)}")
    return _p(t)


@_op("conf_hist(Tensor pred, Tensor conf, int num_classes, int nbins, Tensor(a!) hist) -> ()")
def _conf_hist(pred, conf, num_classes, nbins, hist):
    """hist int64 [num_classes, nbins] += the per-class confidence histogram of (pred, conf)."""
    pp, pc = _pseudo_maps(pred, conf, "conf_hist")
    ph = _pi64(hist, (num_classes, nbins), "conf_hist hist")
    check(_lib.lib().adaptseg_conf_hist(pred.numel(), pp, pc, int(num_classes), int(nbins), ph, _stream()),
          "conf_hist")


@_op("pseudo_thresholds(Tensor hist, float portion, float cap, Tensor(a!) thr) -> ()")
def _pseudo_thresholds(hist, portion, cap, thr):
    """hist int64 [C, nbins] -> thr float32 [C] (include/adaptseg.h: adaptseg_pseudo_thresholds)."""
    if hist.dim() != 2:
        raise RuntimeError(f"pseudo_thresholds: hist is {tuple(hist.shape)}, expected [C, nbins]")
    c, nbins = hist.shape
    ph = _pi64(hist, (c, nbins), "pseudo_thresholds hist")
    if not thr.is_contiguous():
        raise RuntimeError("pseudo_thresholds: thr is not contiguous")
    check(_lib.lib().adaptseg_pseudo_thresholds(ph, c, nbins, float(portion), float(cap),
                                                _pf(thr, c, "pseudo_thresholds thr"), _stream()), "pseudo_thresholds")


@_op("pseudo_label(Tensor pred, Tensor conf, Tensor thr, int ignore_label, Tensor(a!) labels, Tensor(b!)? kept) -> ()")
def _pseudo_label(pred, conf, thr, ignore_label, labels, kept):
    """labels int64 (pred's shape) = pred where conf >= thr[pred], else ignore_label; kept int64 [C] += counts."""
    pp, pc = _pseudo_maps(pred, conf, "pseudo_label")
    c = thr.numel()
    if not thr.is_contiguous():
        raise RuntimeError("pseudo_label: thr is not contiguous")
    pl = _pi64(labels, pred.shape, "pseudo_label labels")
    pk = None if kept is None else _pi64(kept, (c,), "pseudo_label kept")
    check(_lib.lib().adaptseg_pseudo_label(pred.numel(), pp, pc, _pf(thr, c, "pseudo_label thr"), c,
                                           int(ignore_label), pl, pk, _stream()), "pseudo_label")


# ---- online self-training: mean teacher, ClassMix, pixel-weighted CE (adaptsegnet_amd/mix.py) -----
def _pt(t, dtype, shape, what):
    """Pointer of a contiguous tensor of exactly this dtype and shape, checked on the host."""
    if t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise RuntimeError(f"{what}: expected a contiguous {dtype} {tuple(shape)}, got {t.dtype} {tuple(t.shape)}"
                           f"{'' if t.is_contiguous() else ' (not contiguous)'}")
    return _p(t)


@_op("softmax_ce_pw_fwd(Tensor logits, Tensor labels, int ignore, Tensor? weight, Tensor pixel_weight, "
     "Tensor(a!) out) -> ()", names=MIX_NAMES)
def _softmax_ce_pw_fwd(logits, labels, ignore, weight, pixel_weight, out):
    """softmax_ce_fwd with pixel_weight float32 [rows] on the numerator (adaptseg_softmax_ce_pw_fwd)."""
    rows, c = _rc(logits)
    b = ctypes.c_size_t(0)
    check(_lib.lib().adaptseg_ce_workspace_size(rows, ctypes.byref(b)), "ce_workspace_size")
    wp, wsz = _ws_args(b.value, logits.device)
    check(_lib.lib().adaptseg_softmax_ce_pw_fwd(
        rows, c, _pf(logits, rows * c, "softmax_ce_pw_fwd logits"), _p(labels), int(ignore), _p(weight),
        _pf(pixel_weight, rows, "softmax_ce_pw_fwd pixel_weight"), _pf(out, 2, "softmax_ce_pw_fwd out"), wp, wsz,
        _stream()), "softmax_ce_pw_fwd")


@_op("softmax_ce_pw_bwd(Tensor logits, Tensor labels, Tensor out, Tensor grad_loss, int ignore, Tensor? weight, "
     "Tensor pixel_weight, Tensor(a!) dlogits, bool accumulate) -> ()", names=MIX_NAMES)
def _softmax_ce_pw_bwd(logits, labels, out, grad_loss, ignore, weight, pixel_weight, dlogits, accumulate):
    rows, c = _rc(logits)
    check(_lib.lib().adaptseg_softmax_ce_pw_bwd(
        rows, c, _pf(logits, rows * c, "softmax_ce_pw_bwd logits"), _p(labels), int(ignore), _p(weight),
        _pf(pixel_weight, rows, "softmax_ce_pw_bwd pixel_weight"), _pf(out, 2, "softmax_ce_pw_bwd out"),
        _pf(grad_loss, 1, "softmax_ce_pw_bwd grad_loss"), _pf(dlogits, rows * c, "softmax_ce_pw_bwd dlogits"),
        _lib.EPI_ACCUMULATE if accumulate else 0, _stream()), "softmax_ce_pw_bwd")


@_op("ema(Tensor src, Tensor(a!) dst, float alpha) -> ()", names=MIX_NAMES)
def _ema(src, dst, alpha):
    """dst = fmaf(alpha, dst, (1 - alpha) * src) over two contiguous float32 tensors of one size (adaptseg_ema)."""
    n = dst.numel()
    if not (src.is_contiguous() and dst.is_contiguous()):
        raise RuntimeError("ema: src and dst must be contiguous")
    check(_lib.lib().adaptseg_ema(n, float(alpha), _pf(src, n, "ema src"), _pf(dst, n, "ema dst"), _stream()), "ema")


@_op("ema_multi(Tensor[] src, Tensor(a!)[] dst, float alpha) -> ()", names=MIX_NAMES)
def _ema_multi(src, dst, alpha):
    """ema over a list of (small) tensor pairs in ceil(len / _lib.EMA_CHUNK) launches (adaptseg_ema_multi)."""
    if len(src) != len(dst):
        raise RuntimeError(f"ema_multi: {len(src)} sources for {len(dst)} destinations")
    m = len(dst)
    ps, pd, pn = (ctypes.c_void_p * m)(), (ctypes.c_void_p * m)(), (ctypes.c_int64 * m)()
    for i, (s, d) in enumerate(zip(src, dst)):
        if not (s.is_contiguous() and d.is_contiguous()):
            raise RuntimeError(f"ema_multi: tensor {i} is not contiguous")
        n = d.numel()
        ps[i], pd[i], pn[i] = _pf(s, n, f"ema_multi src {i}").value, _pf(d, n, f"ema_multi dst {i}").value, n
    check(_lib.lib().adaptseg_ema_multi(m, ps, pd, pn, float(alpha), _stream()), "ema_multi")


@_op("classmix_stats(Tensor labels_s, Tensor conf_t, float tau, int num_classes, Tensor(a!) count, "
     "Tensor(b!) nconf) -> ()", names=MIX_NAMES)
def _classmix_stats(labels_s, conf_t, tau, num_classes, count, nconf):
    """count int32 [N, C] = source pixels per class, nconf int32 [N] = target pixels with conf >= tau."""
    if labels_s.dim() != 3:
        raise RuntimeError(f"classmix_stats: labels_s is {tuple(labels_s.shape)}, expected [N, H, W]")
    n, h, w = labels_s.shape
    c = int(num_classes)
    check(_lib.lib().adaptseg_classmix_stats(
        n, h, w, c, _pt(labels_s, torch.int64, (n, h, w), "classmix_stats labels_s"),
        _pt(conf_t, torch.float32, (n, h, w), "classmix_stats conf_t"), float(tau),
        _pt(count, torch.int32, (n, c), "classmix_stats count"), _pt(nconf, torch.int32, (n,), "classmix_stats nconf"),
        _stream()), "classmix_stats")


@_op("classmix_apply(Tensor images_s, Tensor labels_s, Tensor images_t, Tensor pred_t, Tensor count, Tensor nconf, "
     "Tensor keys, int ignore_label, Tensor(a!) mixed_images, Tensor(b!) mixed_labels, Tensor(c!) mixed_weights, "
     "Tensor(d!)? mask) -> ()", names=MIX_NAMES)
def _classmix_apply(images_s, labels_s, images_t, pred_t, count, nconf, keys, ignore_label, mixed_images, mixed_labels,
                    mixed_weights, mask):
    """keys: the uint32 [N, C] random numbers, held in an int32 tensor (torch has no arithmetic on uint32)."""
    if images_s.dim() != 4 or images_s.shape[1] != 3:
        raise RuntimeError(f"classmix_apply: images_s is {tuple(images_s.shape)}, expected [N, 3, H, W]")
    n, _, h, w = images_s.shape
    if count.dim() != 2:
        raise RuntimeError(f"classmix_apply: count is {tuple(count.shape)}, expected [N, C]")
    c = count.shape[1]
    if tuple(images_t.shape) != (n, 3, h, w):
        raise RuntimeError(f"classmix_apply: target images {tuple(images_t.shape)} vs source images "
                           f"{tuple(images_s.shape)}: ClassMix pastes pixel on pixel, the sizes must agree")
    what = "classmix_apply"
    check(_lib.lib().adaptseg_classmix_apply(
        n, h, w, c, _pt(images_s, torch.float32, (n, 3, h, w), f"{what} images_s"),
        _pt(labels_s, torch.int64, (n, h, w), f"{what} labels_s"),
        _pt(images_t, torch.float32, (n, 3, h, w), f"{what} images_t"),
        _pt(pred_t, torch.uint8, (n, h, w), f"{what} pred_t"), _pt(count, torch.int32, (n, c), f"{what} count"),
        _pt(nconf, torch.int32, (n,), f"{what} nconf"), _pt(keys, torch.int32, (n, c), f"{what} keys"),
        int(ignore_label), _pt(mixed_images, torch.float32, (n, 3, h, w), f"{what} mixed_images"),
        _pt(mixed_labels, torch.int64, (n, h, w), f"{what} mixed_labels"),
        _pt(mixed_weights, torch.float32, (n, h, w), f"{what} mixed_weights"),
        None if mask is None else _pt(mask, torch.uint8, (n, c), f"{what} mask"), _stream()), what)


@_op("conf_count(Tensor conf_t, float tau, Tensor(a!) nconf) -> ()", names=MIC_NAMES)
def _conf_count(conf_t, tau, nconf):
    """nconf int32 [N] = target pixels with conf >= tau (adaptseg_conf_count): classmix_stats's nconf on its own."""
    if conf_t.dim() != 3:
        raise RuntimeError(f"conf_count: conf_t is {tuple(conf_t.shape)}, expected [N, H, W]")
    n, h, w = conf_t.shape
    check(_lib.lib().adaptseg_conf_count(
        n, h, w, _pt(conf_t, torch.float32, (n, h, w), "conf_count conf_t"), float(tau),
        _pt(nconf, torch.int32, (n,), "conf_count nconf"), _stream()), "conf_count")


@_op("patch_mask(Tensor images_t, Tensor pred_t, Tensor nconf, Tensor keys, int patch, int threshold, int num_classes, "
     "int ignore_label, int ignore_top, int ignore_bottom, Tensor(a!) masked_images, Tensor(b!) labels, "
     "Tensor(c!) weights) -> ()", names=MIC_NAMES)
def _patch_mask(images_t, pred_t, nconf, keys, patch, threshold, num_classes, ignore_label, ignore_top, ignore_bottom,
                masked_images, labels, weights):
    """keys: the uint32 [N, ceil(H / patch), ceil(W / patch)] random numbers, held in an int32 tensor;
    threshold = floor(ratio * 2^32), 0 .. 2^32 (adaptseg_patch_mask)."""
    if images_t.dim() != 4 or images_t.shape[1] != 3:
        raise RuntimeError(f"patch_mask: images_t is {tuple(images_t.shape)}, expected [N, 3, H, W]")
    n, _, h, w = images_t.shape
    patch = int(patch)
    if patch < 1:
        raise RuntimeError(f"patch_mask: patch {patch} (expected at least 1)")
    grid = (n, -(-h // patch), -(-w // patch))
    what = "patch_mask"
    check(_lib.lib().adaptseg_patch_mask(
        n, h, w, patch, int(threshold), int(num_classes), int(ignore_label), int(ignore_top), int(ignore_bottom),
        _pt(images_t, torch.float32, (n, 3, h, w), f"{what} images_t"),
        _pt(pred_t, torch.uint8, (n, h, w), f"{what} pred_t"), _pt(nconf, torch.int32, (n,), f"{what} nconf"),
        _pt(keys, torch.int32, grid, f"{what} keys"),
        _pt(masked_images, torch.float32, (n, 3, h, w), f"{what} masked_images"),
        _pt(labels, torch.int64, (n, h, w), f"{what} labels"),
        _pt(weights, torch.float32, (n, h, w), f"{what} weights"), _stream()), what)


@_op("strong_augment(Tensor images, float[] mean, int[] ctl, Tensor table, Tensor(a!) out) -> ()", names=AUG_NAMES)
def _strong_augment(images, mean, ctl, table, out):
    """Colour jitter, then Gaussian blur, per image (adaptseg_strong_augment).  ``ctl``: the host copy of the
    controls, 4 ints per image (jitter flag, order code, radius, 0).  ``table``: 16 four-byte words per image on
    the device, three tables one after the other: the controls' bits [N, 4], (db, fc, fs, fh) [N, 4] and the half
    kernels [N, 8]."""
    if images.dim() != 4 or images.shape[1] != 3:
        raise RuntimeError(f"strong_augment: images is {tuple(images.shape)}, expected [N, 3, H, W]")
    n, _, h, w = images.shape
    if len(mean) != 3 or len(ctl) != 4 * n:
        raise RuntimeError(f"strong_augment: {len(mean)} means (expected 3), {len(ctl)} controls (expected {4 * n})")
    what = "strong_augment"
    base = _pt(table, torch.float32, (16 * n,), f"{what} table").value
    check(_lib.lib().adaptseg_strong_augment(
        n, h, w, _pt(images, torch.float32, (n, 3, h, w), f"{what} images"), (ctypes.c_float * 3)(*mean),
        (ctypes.c_int32 * (4 * n))(*ctl), ctypes.c_void_p(base), ctypes.c_void_p(base + 16 * n),
        ctypes.c_void_p(base + 32 * n), _pt(out, torch.float32, (n, 3, h, w), f"{what} out"), _stream()), what)


# ---- Fourier Domain Adaptation (adaptsegnet_amd/fda.py, functional.entropy_loss2d(eta=...)) --------
@_op("fda_transfer(Tensor src, Tensor trg, int b, Tensor? mean, Tensor tw_w, Tensor tw_h, Tensor(a!) out) -> ()",
     names=FDA_NAMES)
def _fda_transfer(src, trg, b, mean, tw_w, tw_h, out):
    """out = src with the low-frequency amplitudes (|u|, |v| <= b) of trg (adaptseg_fda_transfer).  ``mean``: float32
    [C] on the device or None; ``tw_w`` / ``tw_h``: the (cos, sin) tables float32 [W, 2] / [H, 2] (fda.twiddles)."""
    if src.dim() != 4:
        raise RuntimeError(f"fda_transfer: src is {tuple(src.shape)}, expected [N, C, H, W]")
    n, c, h, w = src.shape
    what = "fda_transfer"
    b = int(b)
    sz = ctypes.c_size_t(0)
    check(_lib.lib().adaptseg_fda_workspace_size(n, c, h, w, b, ctypes.byref(sz)), "fda_workspace_size")
    wp, wsz = _ws_args(sz.value, src.device)
    check(_lib.lib().adaptseg_fda_transfer(
        n, c, h, w, b, _pt(src, torch.float32, (n, c, h, w), f"{what} src"),
        _pt(trg, torch.float32, (n, c, h, w), f"{what} trg"),
        None if mean is None else _pt(mean, torch.float32, (c,), f"{what} mean"),
        _pt(tw_w, torch.float32, (w, 2), f"{what} tw_w"), _pt(tw_h, torch.float32, (h, 2), f"{what} tw_h"),
        _pt(out, torch.float32, (n, c, h, w), f"{what} out"), wp, wsz, _stream()), what)


@_op("entropy_rho_loss_fwd(Tensor x, float eta, float eps, Tensor(a!) loss) -> ()", names=FDA_NAMES)
def _entropy_rho_loss_fwd(x, eta, eps, loss):
    """entropy_loss_fwd with FDA's robust term: loss = mean over rows of ((H / ln c)^2 + eps)^eta."""
    rows, c = _rc(x)
    b = ctypes.c_size_t(0)
    check(_lib.lib().adaptseg_entropy_workspace_size(rows, ctypes.byref(b)), "entropy_workspace_size")
    wp, wsz = _ws_args(b.value, x.device)
    check(_lib.lib().adaptseg_entropy_rho_loss_fwd(rows, c, float(eta), float(eps),
                                                   _pf(x, rows * c, "entropy_rho_loss_fwd x"),
                                                   _pf(loss, 1, "entropy_rho_loss_fwd loss"), wp, wsz, _stream()),
          "entropy_rho_loss_fwd")


@_op("entropy_rho_loss_bwd(Tensor x, float eta, float eps, Tensor grad_loss, Tensor(a!) dx, bool accumulate) -> ()",
     names=FDA_NAMES)
def _entropy_rho_loss_bwd(x, eta, eps, grad_loss, dx, accumulate):
    rows, c = _rc(x)
    n = rows * c
    check(_lib.lib().adaptseg_entropy_rho_loss_bwd(rows, c, float(eta), float(eps),
                                                   _pf(x, n, "entropy_rho_loss_bwd x"),
                                                   _pf(grad_loss, 1, "entropy_rho_loss_bwd grad_loss"),
                                                   _pf(dx, n, "entropy_rho_loss_bwd dx"),
                                                   _lib.EPI_ACCUMULATE if accumulate else 0, _stream()),
          "entropy_rho_loss_bwd")


# ---- rare class sampling: class statistics and class-aware crops (adaptsegnet_amd/rcs.py) ------------
def _rcs_labels(labels, what):
    if labels.dtype != torch.uint8 or labels.dim() != 3 or not labels.is_contiguous():
        raise RuntimeError(f"{what}: labels are {labels.dtype} {tuple(labels.shape)}, expected a contiguous uint8 "
                           "[N, H, W]")
    return labels.shape


def _rcs_lut(lut, what):
    return None if lut is None else _pt(lut, torch.int32, (256,), f"{what} lut")


@_op("label_class_count(Tensor labels, Tensor? lut, int num_classes, Tensor(a!) counts) -> ()", names=RCS_NAMES)
def _label_class_count(labels, lut, num_classes, counts):
    """counts int64 [N, num_classes] = per image the pixels of every trainId (adaptseg_label_class_count)."""
    what = "label_class_count"
    n, h, w = _rcs_labels(labels, what)
    check(_lib.lib().adaptseg_label_class_count(
        n, h, w, _p(labels), _rcs_lut(lut, what), int(num_classes),
        _pi64(counts, (n, int(num_classes)), f"{what} counts"), _stream()), what)


@_op("crop_class_count(Tensor labels, Tensor? lut, Tensor classes, int[] params, int crop_h, int crop_w, "
     "Tensor(a!) counts) -> ()", names=RCS_NAMES)
def _crop_class_count(labels, lut, classes, params, crop_h, crop_w, counts):
    """counts int64 [N, K] = the pixels of classes[i] in the label window of every candidate; params: the flattened
    host array [N][K][5] = (sw, sh, ox, oy, mirror) of include/adaptseg.h (adaptseg_crop_class_count)."""
    what = "crop_class_count"
    n, h, w = _rcs_labels(labels, what)
    if counts.dim() != 2 or counts.shape[0] != n:
        raise RuntimeError(f"{what}: counts is {tuple(counts.shape)}, expected [{n}, K]")
    k = counts.shape[1]
    if len(params) != 5 * n * k:
        raise RuntimeError(f"{what}: expected {5 * n * k} params for {n} samples x {k} candidates, got {len(params)}")
    pa = (ctypes.c_int32 * (5 * n * k))(*params)
    b = ctypes.c_size_t(0)
    check(_lib.lib().adaptseg_crop_class_count_workspace_size(n, h, w, int(crop_h), int(crop_w), k, pa,
                                                              ctypes.byref(b)), "crop_class_count_workspace_size")
    wp, wsz = _ws_args(b.value, labels.device)
    check(_lib.lib().adaptseg_crop_class_count(
        n, h, w, int(crop_h), int(crop_w), k, _p(labels), _rcs_lut(lut, what),
        _pt(classes, torch.int32, (n,), f"{what} classes"), pa, _pi64(counts, (n, k), f"{what} counts"), wp, wsz,
        _stream()), what)


class _Overloads:
    """torch.ops.adaptseg.<name>.default for every op (skips the packet's overload lookup)."""


OPS = _Overloads()
for _n in NAMES + LOSS_NAMES + MIX_NAMES + MIC_NAMES + AUG_NAMES + FDA_NAMES + RCS_NAMES:
    setattr(OPS, _n, getattr(torch.ops.adaptseg, _n).default)
