"""GPU parity of the HIP kernels against the fp64 CPU oracle (torch CPU ops), one or two shapes
each; the BatchNorm passes' channel / row layouts and numerical edges are in
test_bn_oracle_gpu.py.

Tolerances (stated per op): the kernels compute in fp32 (fp32 MFMA = an exact fp32 fmaf
chain), the oracle in fp64.  Convolutions: max|err| <= 2e-5 * max|ref| (K up to 36*2048);
pointwise / reductions: <= 1e-5 relative; integer-exact where the op is a selection
(max-pool argmax routing).
"""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"


def K():
    from adaptsegnet_amd import kernels
    return kernels


def rel(a, b):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def nhwc(t):  # NCHW cpu -> NHWC contiguous cuda fp32
    return t.permute(0, 2, 3, 1).contiguous().float().to(DEV)


def nchw(t):  # NHWC cuda -> NCHW cpu fp64
    return t.permute(0, 3, 1, 2).double().cpu()


def w_cl(w):  # [co,ci,kh,kw] cpu -> device [co,kh,kw,ci] contiguous
    return w.permute(0, 2, 3, 1).contiguous().float().to(DEV)


sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conv_cases import CONV_CASES, LARGE_CASES  # noqa: E402


def test_thin_conv_selection_and_epilogues():
    """Cout <= 4 convs run on the vector-ALU kernels (conv_thin.hip): selector 100*op + 80
    (stride-2 data gradients stay on the implicit GEMM), with the igemm epilogue semantics."""
    k = K()
    n, cin, h, w, cout = 2, 64, 12, 18, 2
    geom = k.ConvGeom(cin, cout, 3, 3, 1, (1,), (1,))
    for op in (0, 1, 2):
        assert k.conv_kernel_id(geom, n, h, w, op)[0] == 100 * op + 80
    g2 = k.ConvGeom(128, 1, 4, 4, 2, (1,), (1,))           # D classifier
    assert k.conv_kernel_id(g2, n, 8, 10, 0)[0] == 80
    assert k.conv_kernel_id(g2, n, 8, 10, 1)[0] != 180
    g = torch.Generator().manual_seed(7)
    x = torch.randn(n, cin, h, w, generator=g, dtype=torch.float64)
    wt = torch.randn(cout, cin, 3, 3, generator=g, dtype=torch.float64) * 0.1
    b = torch.randn(cout, generator=g, dtype=torch.float64)
    res = torch.randn(n, cout, h, w, generator=g, dtype=torch.float64)
    prev = torch.randn(n, cout, h, w, generator=g, dtype=torch.float64)
    ref = F.relu(F.conv2d(x, wt, b, 1, 1) + prev + res)
    out = nhwc(prev)
    k.conv_fwd(geom, nhwc(x), n, h, w, [w_cl(wt)], [b.float().to(DEV)], out=out, res=nhwc(res),
               flags=k.EPI_ACCUMULATE | k.EPI_RELU)
    assert rel(nchw(out), ref) < 2e-5
    gy = torch.randn(n, cout, h, w, generator=g, dtype=torch.float64)
    aux = torch.randn(n, cin, h, w, generator=g, dtype=torch.float64)
    prev_dx = torch.randn(n, cin, h, w, generator=g, dtype=torch.float64)
    dref = torch.nn.grad.conv2d_input(x.shape, wt, gy, 1, 1) + prev_dx
    dref = torch.where(aux > 0, dref, 0.2 * dref)
    dx = nhwc(prev_dx)
    k.conv_dgrad(geom, nhwc(gy), n, h, w, [w_cl(wt)], out=dx, aux=nhwc(aux), flags=k.EPI_ACCUMULATE)
    assert rel(nchw(dx), dref) < 2e-5



def _ref_conv(x, ws, bs, stride, pads, dils):
    out = None
    for i, (p, d) in enumerate(zip(pads, dils)):
        y = F.conv2d(x, ws[i], bs[i] if bs is not None else None, stride, p, d)
        out = y if out is None else out + y
    return out


@pytest.fixture(params=["f32", "f32x3", "f32x3_presplit"])
def conv_math(request):
    """The fp32 conv maths: exact fp32 MFMA, F32X3 (fp32 through exact 3-term bf16 splits on the
    bf16 MFMA, every operand split while staged, conv_x3.hpp) and F32X3_PRESPLIT (the same
    arithmetic on pre-split operand images by LDS-DMA where the operands allow, conv_x3g.hpp) —
    all held to the same fp64 tolerance."""
    k = K()
    k.set_conv_math({"f32": k.MATH_F32, "f32x3": k.MATH_F32X3, "f32x3_presplit": k.MATH_F32X3_PRESPLIT}[request.param])
    yield request.param
    k.set_conv_math(k.MATH_F32X3)   # the library default


@pytest.mark.parametrize("case", CONV_CASES, ids=[f"c{i}" for i in range(len(CONV_CASES))])
def test_conv_fwd_dgrad_wgrad(case, conv_math):
    k = K()
    n, cin, h, w, cout, ks, stride, pads, dils, bias = case
    g = torch.Generator().manual_seed(hash(case) % (2 ** 31))
    x = torch.randn(n, cin, h, w, generator=g, dtype=torch.float64)
    nseg = len(pads)
    ws = [torch.randn(cout, cin, ks, ks, generator=g, dtype=torch.float64) * 0.1 for _ in range(nseg)]
    bs = [torch.randn(cout, generator=g, dtype=torch.float64) for _ in range(nseg)] if bias else None
    xr = x.clone().requires_grad_(True)
    wr = [t.clone().requires_grad_(True) for t in ws]
    br = [t.clone().requires_grad_(True) for t in bs] if bias else None
    ref = _ref_conv(xr, wr, br, stride, pads, dils)
    gy = torch.randn(ref.shape, generator=g, dtype=torch.float64)
    ref.backward(gy)

    geom = k.ConvGeom(cin, cout, ks, ks, stride, pads, dils)
    xd = nhwc(x)
    wd = [w_cl(t) for t in ws]
    bd = [t.float().to(DEV) for t in bs] if bias else None
    y = k.conv_fwd(geom, xd, n, h, w, wd, bd)
    assert rel(nchw(y), ref) < 2e-5
    # NCHW-strided input (the stem reads the user's NCHW tensor directly)
    xc = x.float().to(DEV).contiguous()
    y2 = k.conv_fwd(geom, xc, n, h, w, wd, bd, strides=tuple(xc.stride()))
    assert rel(nchw(y2), ref) < 2e-5

    gyd = nhwc(gy)
    dx = k.conv_dgrad(geom, gyd, n, h, w, wd)
    assert rel(nchw(dx), xr.grad) < 2e-5
    dws = [torch.zeros_like(t) for t in wd]
    dbs = [torch.zeros(cout, device=DEV) for _ in range(nseg)] if bias else None
    k.conv_wgrad(geom, gyd, xd, n, h, w, dws, dbs)
    for i in range(nseg):
        assert rel(dws[i].permute(0, 3, 1, 2).cpu(), wr[i].grad) < 2e-5
        if bias:
            assert rel(dbs[i].cpu(), br[i].grad) < 1e-5
    # accumulate: a second wgrad doubles the result
    k.conv_wgrad(geom, gyd, xd, n, h, w, dws, dbs, accumulate=True)
    assert rel(dws[0].permute(0, 3, 1, 2).cpu(), 2 * wr[0].grad) < 2e-5


@pytest.mark.parametrize("math", ["f32x3", "bf16"])
@pytest.mark.parametrize("which", ["fwd_x", "fwd_w", "dgrad_dy", "wgrad_x"])
def test_conv_misaligned_input_downgrades(which, math):
    """An input operand one float off a 16-B boundary: the aligned plan of this product (K = 576,
    M = 256: the x3h tile under F32X3, the LDS-DMA tile under BF16, split along K, with a weight
    pack) is downgraded at launch to the generic fp32 gather kernel — another kernel, split count
    and workspace layout at once.  The generic kernel is fp32 under every maths, so the fp32
    bound holds for the BF16 cases too."""
    from test_epilogue_paths_gpu import off_by_one
    k = K()
    n, c, h, w = 1, 64, 16, 16
    geom = k.ConvGeom(c, c, 3, 3, 1, (1,), (1,))
    g = torch.Generator().manual_seed(31)
    x = torch.randn(n, c, h, w, generator=g, dtype=torch.float64)
    wt = torch.randn(c, c, 3, 3, generator=g, dtype=torch.float64) * 0.1
    xr, wr = x.clone().requires_grad_(True), wt.clone().requires_grad_(True)
    ref = F.conv2d(xr, wr, None, 1, 1)
    gy = torch.randn(ref.shape, generator=g, dtype=torch.float64)
    ref.backward(gy)
    k.set_conv_math({"f32x3": k.MATH_F32X3, "bf16": k.MATH_BF16}[math])
    try:
        op = {"fwd_x": 0, "fwd_w": 0, "dgrad_dy": 1, "wgrad_x": 2}[which]
        kid, splits = k.conv_kernel_id(geom, n, h, w, op)
        assert kid % 100 >= 85 and splits > 1, (kid, splits)   # the aligned plan: an MFMA-bf16 tile, split-K
        with k.weight_pack_scope():   # the aligned weights' pack is built; the downgraded plan ignores it
            if which == "fwd_x":
                y = k.conv_fwd(geom, off_by_one(nhwc(x)), n, h, w, [w_cl(wt)])
                assert rel(nchw(y), ref) < 2e-5
            elif which == "fwd_w":
                y = k.conv_fwd(geom, nhwc(x), n, h, w, [off_by_one(w_cl(wt))])
                assert rel(nchw(y), ref) < 2e-5
            elif which == "dgrad_dy":
                dx = k.conv_dgrad(geom, off_by_one(nhwc(gy)), n, h, w, [w_cl(wt)])
                assert rel(nchw(dx), xr.grad) < 2e-5
            else:
                dw = torch.zeros_like(w_cl(wt))
                k.conv_wgrad(geom, nhwc(gy), off_by_one(nhwc(x)), n, h, w, [dw])
                assert rel(dw.permute(0, 3, 1, 2).cpu(), wr.grad) < 2e-5
    finally:
        k.set_conv_math(k.MATH_F32X3)   # the library default


def test_conv_epilogues():
    k = K()
    g = torch.Generator().manual_seed(5)
    n, cin, h, w, cout = 2, 32, 10, 12, 64
    x = torch.randn(n, cin, h, w, generator=g, dtype=torch.float64)
    wt = torch.randn(cout, cin, 4, 4, generator=g, dtype=torch.float64) * 0.1
    b = torch.randn(cout, generator=g, dtype=torch.float64)
    geom = k.ConvGeom(cin, cout, 4, 4, 2, (1,), (1,))
    y = k.conv_fwd(geom, nhwc(x), n, h, w, [w_cl(wt)], [b.float().to(DEV)], flags=k.EPI_LEAKY)
    ref = F.leaky_relu(F.conv2d(x, wt, b, 2, 1), 0.2)
    assert rel(nchw(y), ref) < 2e-5
    # residual + accumulate on dgrad, leaky-grad multiplier
    gy = torch.randn(ref.shape, generator=g, dtype=torch.float64)
    xr = x.clone().requires_grad_(True)
    F.conv2d(xr, wt, None, 2, 1).backward(gy)
    res = torch.randn(n, cin, h, w, generator=g, dtype=torch.float64)
    out = nhwc(res)
    k.conv_dgrad(geom, nhwc(gy), n, h, w, [w_cl(wt)], out=out, res=out)
    assert rel(nchw(out), xr.grad + res) < 2e-5
    out2 = nhwc(res)
    k.conv_dgrad(geom, nhwc(gy), n, h, w, [w_cl(wt)], out=out2, flags=k.EPI_ACCUMULATE)
    assert rel(nchw(out2), xr.grad + res) < 2e-5
    aux = nhwc(res)
    dxl = k.conv_dgrad(geom, nhwc(gy), n, h, w, [w_cl(wt)], aux=aux)
    assert rel(nchw(dxl), xr.grad * torch.where(res > 0, 1.0, 0.2)) < 2e-5


@pytest.mark.parametrize("rates", [(6, 12, 18, 24), (6, 12)])
def test_aspp_tap_gemm_epilogues(rates):
    """ASPP-shaped convs (stride 1, Cout 19, Cin % 32 == 0) take the tap-GEMM path: check the
    epilogue flags through it — fwd residual / accumulate / ReLU, dgrad accumulate (the
    engine's layer5 + layer6 gradient sum) and ReLU-grad, wgrad accumulate — and that the
    selector reports the inner 1x1 GEMM."""
    k = K()
    g = torch.Generator().manual_seed(19)
    n, cin, h, w, cout = 2, 64, 11, 13, 19
    x = torch.randn(n, cin, h, w, generator=g, dtype=torch.float64)
    ws = [torch.randn(cout, cin, 3, 3, generator=g, dtype=torch.float64) * 0.1 for _ in rates]
    bs = [torch.randn(cout, generator=g, dtype=torch.float64) for _ in rates]
    geom = k.ConvGeom(cin, cout, 3, 3, 1, rates, rates)
    sel, _ = k.conv_kernel_id(geom, n, h, w, 0)
    assert sel % 100 // 10 in (0, 8, 9), sel  # a 128x128 tile of the dense 1x1 GEMM, not 256x32
    ref = _ref_conv(x, ws, bs, 1, rates, rates)
    res = torch.randn(ref.shape, generator=g, dtype=torch.float64)
    wd, bd = [w_cl(t) for t in ws], [t.float().to(DEV) for t in bs]
    y = k.conv_fwd(geom, nhwc(x), n, h, w, wd, bd, res=nhwc(res))
    assert rel(nchw(y), ref + res) < 2e-5
    y2 = nhwc(res)
    k.conv_fwd(geom, nhwc(x), n, h, w, wd, bd, out=y2, flags=k.EPI_ACCUMULATE | k.EPI_RELU)
    assert rel(nchw(y2), F.relu(ref + res)) < 2e-5
    gy = torch.randn(ref.shape, generator=g, dtype=torch.float64)
    xr = x.clone().requires_grad_(True)
    wr = [t.clone().requires_grad_(True) for t in ws]
    _ref_conv(xr, wr, None, 1, rates, rates).backward(gy)
    prev = torch.randn(n, cin, h, w, generator=g, dtype=torch.float64)
    dx = nhwc(prev)
    k.conv_dgrad(geom, nhwc(gy), n, h, w, wd, out=dx, flags=k.EPI_ACCUMULATE)
    assert rel(nchw(dx), xr.grad + prev) < 2e-5
    dxr = k.conv_dgrad(geom, nhwc(gy), n, h, w, wd, aux=nhwc(prev), flags=k.EPI_RELU_GRAD)
    assert rel(nchw(dxr), xr.grad * (prev > 0)) < 2e-5
    dws = [torch.ones_like(t) for t in wd]
    k.conv_wgrad(geom, nhwc(gy), nhwc(x), n, h, w, dws, accumulate=True)
    for i in range(len(rates)):
        assert rel(dws[i].permute(0, 3, 1, 2).cpu() - 1.0, wr[i].grad) < 2e-5


@pytest.mark.parametrize("relu,with_res", [(True, False), (False, False), (True, True)])
def test_batchnorm_train(relu, with_res):
    k = K()
    g = torch.Generator().manual_seed(7)
    n, c, h, w = 3, 64, 9, 11
    x = (torch.randn(n, c, h, w, generator=g, dtype=torch.float64) * 3 + 5)
    wt = 1 + 0.1 * torch.randn(c, generator=g, dtype=torch.float64)
    b = 0.1 * torch.randn(c, generator=g, dtype=torch.float64)
    rm, rv = torch.zeros(c, dtype=torch.float64), torch.ones(c, dtype=torch.float64)
    res = torch.randn(n, c, h, w, generator=g, dtype=torch.float64) if with_res else None
    xr = x.clone().requires_grad_(True)
    y = F.batch_norm(xr, rm, rv, wt, b, True, 0.1, 1e-5)
    if with_res:
        y = y + res
    if relu:
        y = F.relu(y)
    gy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    y.backward(gy)
    xd = nhwc(x)
    rmd, rvd = torch.zeros(c, device=DEV), torch.ones(c, device=DEV)
    yd, mean, invstd = k.bn_fwd_train(xd, wt.float().to(DEV), b.float().to(DEV), rmd, rvd, 0.1, 1e-5,
                                      res=nhwc(res) if with_res else None, relu=relu)
    assert rel(nchw(yd), y) < 1e-5
    assert rel(rmd.cpu(), rm) < 1e-5 and rel(rvd.cpu(), rv) < 1e-5
    gyd = nhwc(gy)
    dres = torch.empty_like(gyd) if with_res else None
    dx = k.bn_bwd(gyd, yd, xd, wt.float().to(DEV), mean, invstd, relu=relu, dres=dres)
    assert rel(nchw(dx), xr.grad) < 1e-5
    if with_res:
        assert rel(nchw(dres), gy * (y > 0)) < 1e-6
    if relu and not with_res:
        # ReLU mask recomputed from x (y not read): identical to the y-masked backward
        dx2 = k.bn_bwd(gyd, None, xd, wt.float().to(DEV), mean, invstd, relu=True,
                       bias=b.float().to(DEV))
        assert torch.equal(dx2, dx)


@pytest.mark.parametrize("shape", [(2, 64, 17, 23, 256, 1), (2, 64, 256, 256, 64, 1), (3, 128, 40, 44, 512, 1),
                                   (1, 32, 9, 11, 64, 3)])
def test_conv_fused_bn_statistics(shape):
    """conv_fwd_bnstats + bn_fwd_train_tiles (row-tile statistics from the conv epilogue,
    Chan-merged in fp64) == conv_fwd + bn_fwd_train, incl. partial row tiles."""
    k = K()
    n, cin, h, w, cout, ks = shape
    g = torch.Generator().manual_seed(23)
    x = torch.randn(n, cin, h, w, generator=g, dtype=torch.float64) + 0.5
    wt = torch.randn(cout, cin, ks, ks, generator=g, dtype=torch.float64) * 0.1
    geom = k.ConvGeom(cin, cout, ks, ks, 1, ((ks - 1) // 2,), (1,))
    bw = (1 + 0.1 * torch.randn(cout, generator=g, dtype=torch.float64)).float().to(DEV)
    bb = (0.1 * torch.randn(cout, generator=g, dtype=torch.float64)).float().to(DEV)
    y, tiles = k.conv_fwd_bnstats(geom, nhwc(x), n, h, w, [w_cl(wt)])
    c = F.conv2d(x, wt, None, 1, (ks - 1) // 2)
    assert rel(nchw(y), c) < 2e-5
    if tiles is None:  # split-K grid (small problems): no fused statistics, plain output
        assert n * h * w < 50000, "large convs must produce fused BN statistics"
        return
    rm1, rv1 = torch.zeros(cout, device=DEV), torch.ones(cout, device=DEV)
    rm2, rv2 = torch.zeros(cout, device=DEV), torch.ones(cout, device=DEV)
    z1, m1, i1 = k.bn_fwd_train_tiles(y, tiles, bw, bb, rm1, rv1, 0.1, 1e-5)
    z2, m2, i2 = k.bn_fwd_train(y, bw, bb, rm2, rv2, 0.1, 1e-5)
    ref = F.relu(F.batch_norm(c, None, None, bw.double().cpu(), bb.double().cpu(), True, 0.1, 1e-5))
    assert rel(nchw(z1), ref) < 1e-5
    assert rel(m1, m2) < 1e-5 and rel(i1, i2) < 1e-5
    assert rel(rm1, rm2) < 1e-5 and rel(rv1, rv2) < 1e-5


def test_batchnorm_eval_and_inplace_bwd():
    k = K()
    g = torch.Generator().manual_seed(8)
    n, c, h, w = 2, 32, 5, 7
    x = torch.randn(n, c, h, w, generator=g, dtype=torch.float64)
    wt = 1 + 0.1 * torch.randn(c, generator=g, dtype=torch.float64)
    b = 0.1 * torch.randn(c, generator=g, dtype=torch.float64)
    rm = 0.1 * torch.randn(c, generator=g, dtype=torch.float64)
    rv = 1 + 0.2 * torch.rand(c, generator=g, dtype=torch.float64)
    ref = F.relu(F.batch_norm(x, rm, rv, wt, b, False, 0.1, 1e-5))
    yd = k.bn_fwd_infer(nhwc(x), wt.float().to(DEV), b.float().to(DEV), rm.float().to(DEV),
                        rv.float().to(DEV), 1e-5, relu=True)
    assert rel(nchw(yd), ref) < 1e-5
    # in-place train backward (dx aliases dy)
    xr = x.clone().requires_grad_(True)
    y = F.relu(F.batch_norm(xr, None, None, wt, b, True, 0.1, 1e-5))
    gy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    y.backward(gy)
    xd = nhwc(x)
    yd, mean, invstd = k.bn_fwd_train(xd, wt.float().to(DEV), b.float().to(DEV), None, None, 0.1, 1e-5)
    gyd = nhwc(gy)
    k.bn_bwd(gyd, yd, xd, wt.float().to(DEV), mean, invstd, relu=True, dx=gyd)
    assert rel(nchw(gyd), xr.grad) < 1e-5


@pytest.mark.parametrize("c,ksp", [(64, (3, 2, 1)), (19, (3, 2, 1)), (64, (2, 2, 0)), (6, (2, 2, 0))],
                         ids=["stem-vec4", "stem-scalar", "vgg-vec4", "vgg-scalar"])
def test_maxpool(c, ksp):
    """nn.MaxPool2d(3, 2, 1) (deeplab_multi.py:135) and the VGG 2x2 pools (deeplab_vgg.py) on both
    kernels: four channels per thread (C % 4 == 0) and the scalar one."""
    k = K()
    ks, st, pd = ksp
    g = torch.Generator().manual_seed(9)
    x = F.relu(torch.randn(2, c, 21, 29, generator=g, dtype=torch.float64))  # ties at 0
    xr = x.clone().requires_grad_(True)
    y = F.max_pool2d(xr, ks, st, pd)
    gy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    y.backward(gy)
    yd, am = k.maxpool_fwd(nhwc(x), k=ks, s=st, p=pd)
    assert torch.equal(nchw(yd).float(), y.detach().float())
    dx = k.maxpool_bwd(nhwc(gy), am, 21, 29, k=ks, s=st, p=pd)
    # gradient routing is exact wherever the max is unique (>0); zero ties only feed ReLU zeros
    mask = (x > 0)
    assert rel(nchw(dx) * mask, xr.grad * mask) < 1e-6


def test_maxpool_vec4_matches_scalar_bitwise():
    """The float4 pool kernels against the scalar ones on the same values (a tensor one float off
    16-B alignment takes the scalar kernel): outputs, argmax (ties, NaN) and routed gradients
    bitwise."""
    k = K()
    g = torch.Generator().manual_seed(4)
    for ks, st, pd in ((3, 2, 1), (2, 2, 0)):
        x = F.relu(torch.randn(2, 21, 29, 64, generator=g)).to(DEV)
        x[0, 3, 5, 7] = float("nan")
        buf = torch.empty(x.numel() + 1, device=DEV)
        xm = buf[1:].view(x.shape)
        xm.copy_(x)
        ya, ama = k.maxpool_fwd(x, k=ks, s=st, p=pd)
        yb, amb = k.maxpool_fwd(xm, k=ks, s=st, p=pd)
        assert torch.equal(ama, amb)
        assert torch.equal(ya.nan_to_num(7.0), yb.nan_to_num(7.0))
        gy = torch.randn(ya.shape, generator=g).to(DEV)
        gbuf = torch.empty(gy.numel() + 1, device=DEV)
        gm = gbuf[1:].view(gy.shape)
        gm.copy_(gy)
        assert torch.equal(k.maxpool_bwd(gy, ama, 21, 29, k=ks, s=st, p=pd),
                           k.maxpool_bwd(gm, ama, 21, 29, k=ks, s=st, p=pd))


@pytest.mark.parametrize("hw,out", [((9, 13), (65, 97)), ((64, 128), (512, 1024)),
                                    ((90, 160), (720, 1280)), ((1, 5), (3, 9)), ((7, 7), (7, 7))])
@pytest.mark.parametrize("c", [19, 40])
def test_upsample(hw, out, c):
    k = K()
    g = torch.Generator().manual_seed(10)
    n = 2
    x = torch.randn(n, c, *hw, generator=g, dtype=torch.float64)
    xr = x.clone().requires_grad_(True)
    y = F.interpolate(xr, size=out, mode="bilinear", align_corners=True)
    gy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    y.backward(gy)
    yd = k.upsample_fwd(nhwc(x), *out)
    assert rel(nchw(yd), y) < 1e-5
    dx = k.upsample_bwd(nhwc(gy), *hw)
    assert rel(nchw(dx), xr.grad) < 1e-5


@pytest.mark.parametrize("c", [19, 40])  # LDS-tiled rows (C <= 32) and the per-thread-row path
def test_softmax_ce_adv(c):
    k = K()
    g = torch.Generator().manual_seed(11)
    n, h, w = 2, 33, 41
    x = torch.randn(n, c, h, w, generator=g, dtype=torch.float64) * 3
    lab = torch.randint(0, c, (n, h, w), generator=g)
    lab[torch.rand(n, h, w, generator=g) < 0.1] = 255
    lab[0, 0, :4] = -1  # CrossEntropy2d also drops negative labels (utils/loss.py:29)
    xr = x.clone().requires_grad_(True)
    sm = F.softmax(xr, dim=1)
    gs = torch.randn(sm.shape, generator=g, dtype=torch.float64)
    sm.backward(gs)
    yd = k.softmax_fwd(nhwc(x))
    assert rel(nchw(yd), sm) < 1e-5
    dxd = k.softmax_bwd(yd, nhwc(gs))
    assert rel(nchw(dxd), xr.grad) < 1e-5
    # CE
    from oracle.reference_torch import cross_entropy2d
    xr2 = x.clone().requires_grad_(True)
    lref = cross_entropy2d(xr2, lab)
    lref.backward(torch.tensor(0.7, dtype=torch.float64))
    xd = nhwc(x)
    labd = lab.to(DEV)
    out = k.ce_fwd(xd, labd)
    assert abs(out[0].item() - lref.item()) < 1e-5 * abs(lref.item())
    gl = torch.tensor([0.7], device=DEV)
    dl = k.ce_bwd(xd, labd, out, gl)
    assert rel(nchw(dl), xr2.grad) < 1e-5
    # all ignored -> NaN (reference behaviour)
    out2 = k.ce_fwd(xd, torch.full_like(labd, 255))
    assert torch.isnan(out2[0]).item()
    # adversarial losses
    d = torch.randn(2, 1, 16, 32, generator=g, dtype=torch.float64) * 2
    for kind, tgt in ((0, 0.0), (0, 1.0), (1, 0.0), (1, 1.0)):
        dr = d.clone().requires_grad_(True)
        t = torch.full_like(dr, tgt)
        lr_ = F.binary_cross_entropy_with_logits(dr, t) if kind == 0 else F.mse_loss(dr, t)
        lr_.backward(torch.tensor(0.3, dtype=torch.float64))
        dd = d.float().to(DEV).contiguous()
        lo = k.adv_fwd(dd, tgt, kind)
        assert abs(lo.item() - lr_.item()) < 1e-5 * max(1.0, abs(lr_.item()))
        gx = k.adv_bwd(dd, tgt, kind, torch.tensor([0.3], device=DEV))
        assert rel(gx.cpu(), dr.grad) < 1e-5


def test_sgd_multiplicity_and_adam():
    k = K()
    g = torch.Generator().manual_seed(12)
    n = 1000
    p0 = torch.randn(n, generator=g, dtype=torch.float64)
    grads = [torch.randn(n, generator=g, dtype=torch.float64) for _ in range(3)]
    for mult in (1, 3, 4):
        pr = torch.nn.Parameter(p0.clone())
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            opt = torch.optim.SGD([{"params": [pr] * mult}], lr=0.01, momentum=0.9, weight_decay=5e-4, foreach=False)
        pd = p0.float().to(DEV)
        md = torch.zeros(n, device=DEV)
        for s, gr in enumerate(grads):
            pr.grad = gr.clone()
            opt.step()
            k.sgd_step(pd, (gr * 2).float().to(DEV), md, 0.01, 0.9, 5e-4, grad_scale=0.5,
                       multiplicity=mult, first_step=(s == 0))
        assert rel(pd.cpu(), pr.detach()) < 1e-5
    pr = torch.nn.Parameter(p0.clone())
    opt = torch.optim.Adam([pr], lr=1e-3, betas=(0.9, 0.99), foreach=False)
    pd = p0.float().to(DEV)
    m, v = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    for s, gr in enumerate(grads):
        pr.grad = gr.clone()
        opt.step()
        k.adam_step(pd, gr.float().to(DEV), m, v, 1e-3, 0.9, 0.99, 1e-8, s + 1)
    assert rel(pd.cpu(), pr.detach()) < 1e-5


def test_to_nhwc_and_axpy():
    k = K()
    x = torch.randn(2, 19, 7, 9, device=DEV)
    assert torch.equal(k.to_nhwc(x), x.permute(0, 2, 3, 1).contiguous())
    a = torch.randn(100, device=DEV)
    b = torch.randn(100, device=DEV)
    c = b.clone()
    k.axpy(0.5, a, c)
    assert torch.allclose(c, b + 0.5 * a)


@pytest.mark.parametrize("case", LARGE_CASES, ids=[f"L{i}" for i in range(len(LARGE_CASES))])
def test_conv_large_grid_epilogues(case, conv_math):
    """Grids of >= 257 output tiles (the c2 / c3 / c5 layer sizes): forward and data gradient
    store from the in-kernel epilogue (no K split), so every epilogue flag the engine uses is
    checked there against fp64 torch:
      fwd   plain, EPI_RELU + EPI_RESIDUAL, EPI_ACCUMULATE, EPI_LEAKY (D convs, bias)
      dgrad plain, EPI_RESIDUAL with out == res (identity shortcut, engine.block_backward),
            EPI_ACCUMULATE (downsample + conv1, ASPP layer5 + layer6), aux RELU_GRAD (VGG),
            aux LEAKY_GRAD (D)
      wgrad accumulate (the gradient arena)."""
    k = K()
    n, cin, h, w, cout, ks, stride, pads, dils, bias = case
    geom = k.ConvGeom(cin, cout, ks, ks, stride, pads, dils)
    for op in (0, 1):
        sel, sp = k.conv_kernel_id(geom, n, h, w, op)
        assert sp == 1, (op, sel, sp)   # the unsplit large-grid path is what this test is for
    g = torch.Generator().manual_seed(4242 + LARGE_CASES.index(case))
    nseg = len(pads)
    x = torch.randn(n, cin, h, w, generator=g, dtype=torch.float64)
    ws = [torch.randn(cout, cin, ks, ks, generator=g, dtype=torch.float64) * (1.0 / (cin * ks * ks) ** 0.5)
          for _ in range(nseg)]
    bs = [torch.randn(cout, generator=g, dtype=torch.float64) for _ in range(nseg)] if bias else None
    xr = x.clone().requires_grad_(True)
    wr = [t.clone().requires_grad_(True) for t in ws]
    ref = _ref_conv(xr, wr, bs, stride, pads, dils)
    gy = torch.randn(ref.shape, generator=g, dtype=torch.float64)
    ref.backward(gy)
    ref = ref.detach()
    xd, gyd = nhwc(x), nhwc(gy)
    wd = [w_cl(t) for t in ws]
    bd = [t.float().to(DEV) for t in bs] if bias else None

    # forward
    assert rel(nchw(k.conv_fwd(geom, xd, n, h, w, wd, bd)), ref) < 2e-5
    xc = x.float().to(DEV).contiguous()
    assert rel(nchw(k.conv_fwd(geom, xc, n, h, w, wd, bd, strides=tuple(xc.stride()))), ref) < 2e-5
    res = torch.randn(ref.shape, generator=g, dtype=torch.float64)
    y = k.conv_fwd(geom, xd, n, h, w, wd, bd, res=nhwc(res), flags=k.EPI_RELU)
    assert rel(nchw(y), F.relu(ref + res)) < 2e-5
    y = nhwc(res)
    k.conv_fwd(geom, xd, n, h, w, wd, bd, out=y, flags=k.EPI_ACCUMULATE)
    assert rel(nchw(y), ref + res) < 2e-5
    y = k.conv_fwd(geom, xd, n, h, w, wd, bd, flags=k.EPI_LEAKY)
    assert rel(nchw(y), F.leaky_relu(ref, 0.2)) < 2e-5
    if nseg == 1 and not bias:   # forward with fused BN statistics (every Bottleneck conv)
        y, tiles = k.conv_fwd_bnstats(geom, xd, n, h, w, wd)
        assert tiles is not None and rel(nchw(y), ref) < 2e-5

    # data gradient
    dref = xr.grad
    assert rel(nchw(k.conv_dgrad(geom, gyd, n, h, w, wd)), dref) < 2e-5
    prev = torch.randn(n, cin, h, w, generator=g, dtype=torch.float64)
    out = nhwc(prev)
    k.conv_dgrad(geom, gyd, n, h, w, wd, out=out, res=out)
    assert rel(nchw(out), dref + prev) < 2e-5
    out = nhwc(prev)
    k.conv_dgrad(geom, gyd, n, h, w, wd, out=out, flags=k.EPI_ACCUMULATE)
    assert rel(nchw(out), dref + prev) < 2e-5
    dx = k.conv_dgrad(geom, gyd, n, h, w, wd, aux=nhwc(prev), flags=k.EPI_RELU_GRAD)
    assert rel(nchw(dx), dref * (prev > 0)) < 2e-5
    dx = k.conv_dgrad(geom, gyd, n, h, w, wd, aux=nhwc(prev))
    assert rel(nchw(dx), torch.where(prev > 0, dref, 0.2 * dref)) < 2e-5

    # weight gradient, accumulated into a non-zero arena slot
    dws = [torch.ones_like(t) for t in wd]
    k.conv_wgrad(geom, gyd, xd, n, h, w, dws, accumulate=True)
    for i in range(nseg):
        assert rel(dws[i].permute(0, 3, 1, 2).cpu() - 1.0, wr[i].grad) < 2e-5


@pytest.mark.parametrize("shape", [(4, 256, 64, 72, 64, 1), (2, 256, 96, 96, 256, 3), (2, 128, 20, 18, 48, 1)])
def test_conv_dgrad_into_bn_relu_backward(shape, conv_math):
    """The Bottleneck backward chain conv2 / conv3 data gradient -> train-mode BN+ReLU backward
    with the ReLU mask recomputed from the BN input (engine.block_backward), in place, vs
    fp64 torch autograd of conv(relu(bn(x))).  The first two shapes are unsplit large grids
    (in-kernel epilogue), the last is split along K."""
    k = K()
    n, cin, h, w, cout, ks = shape
    g = torch.Generator().manual_seed(17)
    pad = ks // 2 * (2 if ks == 3 else 1)
    geom = k.ConvGeom(cin, cout, ks, ks, 1, (pad,), (2 if ks == 3 else 1,))
    bx = torch.randn(n, cin, h, w, generator=g, dtype=torch.float64) * 2 + 0.3
    bw = torch.rand(cin, generator=g, dtype=torch.float64) + 0.5
    bb = torch.randn(cin, generator=g, dtype=torch.float64) * 0.2
    wt = torch.randn(cout, cin, ks, ks, generator=g, dtype=torch.float64) * 0.05
    xr = bx.clone().requires_grad_(True)
    a = F.relu(F.batch_norm(xr, None, None, bw, bb, True, 0.1, 1e-5))
    y = F.conv2d(a, wt, None, 1, geom.pads[0], geom.dils[0])
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    y.backward(dy)
    bxd = nhwc(bx)
    bwd, bbd = bw.float().to(DEV), bb.float().to(DEV)
    _, mean, invstd = k.bn_fwd_train(bxd, bwd, bbd, torch.zeros(cin, device=DEV), torch.ones(cin, device=DEV),
                                     0.1, 1e-5, relu=True)
    dx = k.conv_dgrad(geom, nhwc(dy), n, h, w, [w_cl(wt)])
    k.bn_bwd(dx, None, bxd, bwd, mean, invstd, relu=True, dx=dx, bias=bbd)
    assert rel(nchw(dx), xr.grad) < 1e-4


@pytest.mark.parametrize("mask", ["relu_x", "bits", "none"])
@pytest.mark.parametrize("shape", [(4, 256, 64, 72, 64, 1), (2, 256, 96, 96, 256, 3), (4, 256, 75, 61, 64, 1),
                                   (2, 64, 150, 121, 64, 3), (2, 128, 20, 18, 48, 1)],
                         ids=["1x1", "3x3-dil2", "1x1-ragged", "3x3-c64", "1x1-small"])
def test_conv_dgrad_fused_bn_sums(shape, mask, conv_math):
    """The BN backward reduction fused into the data-gradient epilogue (conv_dgrad(bnsum=...),
    adaptseg_conv2d_bwd_data_bnsum -> adaptseg_bn_bwd_sums): the data gradient is bit-identical to
    the unfused one; the per-tile sums add up to sum g' and sum g' (x - mean) (fp64 reference,
    g' = dx masked by the BN's ReLU recomputed from x / by the forward's bitmap / unmasked); and
    the BN backward that consumes them matches fp64 autograd as the unfused chain does.  The
    ragged shape ends on a partial row tile and the Cin-64 one fills half of every 128-column
    tile (both: the per-element epilogue); a split-K plan cannot fuse (the sums come back None
    and the unfused BN backward runs)."""
    k = K()
    n, cin, h, w, cout, ks = shape
    g = torch.Generator().manual_seed(23)
    pad = ks // 2 * (2 if ks == 3 else 1)
    geom = k.ConvGeom(cin, cout, ks, ks, 1, (pad,), (2 if ks == 3 else 1,))
    bx = torch.randn(n, cin, h, w, generator=g, dtype=torch.float64) * 2 + 0.3
    bw = torch.rand(cin, generator=g, dtype=torch.float64) + 0.5
    bb = torch.randn(cin, generator=g, dtype=torch.float64) * 0.2
    wt = torch.randn(cout, cin, ks, ks, generator=g, dtype=torch.float64) * 0.05
    xr = bx.clone().requires_grad_(True)
    bn_out = F.batch_norm(xr, None, None, bw, bb, True, 0.1, 1e-5)
    a = F.relu(bn_out) if mask != "none" else bn_out
    y = F.conv2d(a, wt, None, 1, geom.pads[0], geom.dils[0])
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    y.backward(dy)
    bxd = nhwc(bx)
    bwd, bbd = bw.float().to(DEV), bb.float().to(DEV)
    bits = k.mask_bits_like(bxd) if mask == "bits" else None
    yfw, mean, invstd = k.bn_fwd_train(bxd, bwd, bbd, torch.zeros(cin, device=DEV), torch.ones(cin, device=DEV),
                                       0.1, 1e-5, relu=mask != "none", ybits=bits)
    code = {"relu_x": k.BNSUM_RELU_X, "bits": k.BNSUM_BITS, "none": k.BNSUM_NONE}[mask]
    dyd, wd = nhwc(dy), [w_cl(wt)]
    plain = k.conv_dgrad(geom, dyd, n, h, w, wd)
    dx, sums = k.conv_dgrad(geom, dyd, n, h, w, wd, bnsum=k.BnSum(bxd, mean, invstd, bwd, bbd, code, bits))
    assert torch.equal(dx, plain)
    split = k.conv_kernel_id(geom, n, h, w, 1)[1] > 1
    assert (sums is None) == split
    if sums is not None:
        part, nt = sums
        assert nt == k.conv_bnsum_tiles(geom, n, h, w)
        s = part.view(2, cin, nt).double().sum(-1).cpu()
        gd = dx.double().cpu().reshape(-1, cin)
        xd = bxd.double().cpu().reshape(-1, cin)
        m64 = mean.double().cpu()
        if mask == "relu_x":
            gd = torch.where(yfw.reshape(-1, cin).cpu() > 0, gd, 0.0)   # the forward's ReLU decision
        elif mask == "bits":
            word = bits.cpu().reshape(-1, cin // 32).long() & 0xffffffff
            bit = (word.repeat_interleave(32, dim=1) >> torch.arange(cin).remainder(32)) & 1
            gd = gd * bit
        assert rel(s[0], gd.sum(0)) < 1e-5
        assert rel(s[1], (gd * (xd - m64)).sum(0)) < 1e-5
    relu = mask == "relu_x"
    k.bn_bwd(dx, None, bxd, bwd, mean, invstd, relu=relu, dx=dx, bias=bbd, dybits=bits, sums=sums)
    assert rel(nchw(dx), xr.grad) < 1e-4


@pytest.mark.parametrize("size_average", [True, False])
@pytest.mark.parametrize("weighted", [False, True])
def test_crossentropy2d_module(size_average, weighted):
    """utils/loss.py CrossEntropy2d drop-in: mean (size_average=True) and sum reductions, with
    and without class weights, value and logits gradient vs F.cross_entropy in fp64 on the
    kept pixels (target >= 0 and != 255, reference utils/loss.py:29-35)."""
    from adaptsegnet_amd.utils.loss import CrossEntropy2d
    g = torch.Generator().manual_seed(31)
    n, c, h, w = 2, 19, 21, 27
    x = torch.randn(n, c, h, w, generator=g, dtype=torch.float64) * 2
    lab = torch.randint(0, c, (n, h, w), generator=g)
    lab[torch.rand(n, h, w, generator=g) < 0.1] = 255
    lab[0, 0, :3] = -1
    cw = torch.rand(c, generator=g, dtype=torch.float64) + 0.5 if weighted else None
    xr = x.clone().requires_grad_(True)
    keep = (lab >= 0) & (lab != 255)
    ref = F.cross_entropy(xr.permute(0, 2, 3, 1)[keep], lab[keep], weight=cw,
                          reduction="mean" if size_average else "sum")
    ref.backward(torch.tensor(0.7, dtype=torch.float64))
    xd = x.float().to(DEV).requires_grad_(True)
    loss = CrossEntropy2d(size_average=size_average)(xd, lab.to(DEV),
                                                     None if cw is None else cw.float().to(DEV))
    assert abs(loss.item() - ref.item()) <= 1e-5 * abs(ref.item())
    loss.backward(torch.tensor(0.7, device=DEV))
    assert rel(xd.grad, xr.grad) < 1e-5
    if not size_average:   # an all-ignored batch sums to 0 (F.cross_entropy on no pixels)
        empty = CrossEntropy2d(size_average=False)(xd.detach(), torch.full_like(lab, 255).to(DEV))
        assert empty.item() == 0.0


def test_custom_ops_opcheck():
    """torch.library.opcheck (schema mutation annotations, fake kernels, autograd registration,
    AOT dispatch) on small cases of the hot-path ops of torch.ops.adaptseg."""
    g = torch.Generator().manual_seed(3)
    r = lambda *s: torch.randn(*s, generator=g).to(DEV)  # noqa: E731
    n, h, w, cin, cout = 2, 9, 11, 16, 32
    x = r(n, h, w, cin)
    wt = r(cout, cin, 3, 3).contiguous(memory_format=torch.channels_last)
    y = torch.empty(n, h, w, cout, device=DEV)
    ops = torch.ops.adaptseg
    cases = [
        (ops.conv2d_fwd.default, (x, None, [wt], None, [None], None, y, None, [n, cin, h, w], [h * w * cin, 1, w * cin, cin],
                                  [cout, cin, 3, 3], 1, [1], [1], 0)),
        (ops.conv2d_bwd_data.default, (r(n, h, w, cout), None, [wt], None, None, None, None, torch.empty_like(x), None, [n, cin, h, w],
                                       [cout, cin, 3, 3], 1, [1], [1], 0)),
        (ops.conv2d_bwd_weight.default, (r(n, h, w, cout), None, x, None, [torch.zeros_like(wt)], [], [n, cin, h, w],
                                         [h * w * cin, 1, w * cin, cin], [cout, cin, 3, 3], 1, [1], [1], 2)),
        (ops.bn_fwd_train.default, (r(n, h, w, cout), r(cout), r(cout), torch.zeros(cout, device=DEV),
                                    torch.ones(cout, device=DEV), None, torch.empty(n, h, w, cout, device=DEV),
                                    None, torch.empty(n * h * w, 1, device=DEV, dtype=torch.int32),
                                    torch.empty(cout, device=DEV), torch.empty(cout, device=DEV), 0.1, 1e-5, 1)),
        (ops.upsample_bilinear_fwd.default, (r(n, 4, 5, 19), torch.empty(n, 13, 17, 19, device=DEV))),
        (ops.softmax_fwd.default, (r(n, h, w, 19), torch.empty(n, h, w, 19, device=DEV))),
        (ops.softmax_ce_fwd.default, (r(n, h, w, 19), torch.randint(0, 19, (n, h, w), generator=g).to(DEV), 255,
                                      None, torch.empty(2, device=DEV))),
        (ops.adv_loss_fwd.default, (r(n, 1, 3, 4), 1.0, 0, torch.empty(1, device=DEV))),
    ]
    for op, args in cases:
        res = torch.library.opcheck(op, args)
        assert all(v == "SUCCESS" for v in res.values()), (op, res)


def test_torch_ops_conv_and_ce_vs_oracle():
    """The ops called through torch.ops.adaptseg directly (what the modules route through) vs
    fp64 torch: an atrous 3x3 conv forward and the ignore-index cross entropy."""
    g = torch.Generator().manual_seed(5)
    n, cin, h, w, cout = 2, 64, 21, 27, 96
    x = torch.randn(n, cin, h, w, generator=g, dtype=torch.float64)
    wt = torch.randn(cout, cin, 3, 3, generator=g, dtype=torch.float64) * 0.05
    ref = F.conv2d(x, wt, None, 1, 2, 2)
    y = torch.empty(n, h, w, cout, device=DEV)
    torch.ops.adaptseg.conv2d_fwd(nhwc(x), None, [wt.float().to(DEV).contiguous(memory_format=torch.channels_last)], None,
                                  [], None, y, None, [n, cin, h, w], [h * w * cin, 1, w * cin, cin], [cout, cin, 3, 3], 1,
                                  [2], [2], 0)
    assert rel(nchw(y), ref) < 2e-5
    logits = torch.randn(n, 19, h, w, generator=g, dtype=torch.float64) * 3
    lab = torch.randint(0, 19, (n, h, w), generator=g)
    lab[torch.rand(n, h, w, generator=g) < 0.1] = 255
    out = torch.empty(2, device=DEV)
    torch.ops.adaptseg.softmax_ce_fwd(nhwc(logits), lab.to(DEV), 255, None, out)
    lref = F.cross_entropy(logits, lab, ignore_index=255)
    assert abs(out[0].item() - lref.item()) < 1e-5 * lref.item()


@pytest.mark.parametrize("op", [0, 1, 2])
def test_f32x3_accuracy_matches_fp32_mfma(op):
    """F32X3 is fp32-accurate: on a layer3-shaped atrous conv (K = 2304) and a wide 1x1 (K =
    1024) its max error vs fp64 stays within 1.5x that of the exact fp32-MFMA kernel (the dropped
    split terms are below one fp32 rounding per product), for both F32X3 kernels (the
    register-staged one, selector 100*op + 95 (ADAPTSEG_OPT_X3H 0), the 256x128x32 one splitting
    fp32 rows in-kernel, + 86 (the default for these forward / data gradients), and the pre-split
    LDS-DMA one under F32X3_PRESPLIT, + 88)."""
    k = K()
    g = torch.Generator().manual_seed(77)
    errs = {}
    for n, cin, h, w, cout, ks, dil in ((2, 256, 48, 64, 256, 3, 2), (2, 1024, 32, 48, 256, 1, 1)):
        geom = k.ConvGeom(cin, cout, ks, ks, 1, ((ks // 2) * dil,), (dil,))
        x = torch.randn(n, cin, h, w, generator=g, dtype=torch.float64)
        wt = torch.randn(cout, cin, ks, ks, generator=g, dtype=torch.float64) / (cin * ks * ks) ** 0.5
        gy = torch.randn(n, cout, h, w, generator=g, dtype=torch.float64)
        if op == 0:
            ref = F.conv2d(x, wt, None, 1, geom.pads[0], dil)
        elif op == 1:
            ref = torch.nn.grad.conv2d_input(x.shape, wt, gy, 1, geom.pads[0], dil)
        else:
            ref = torch.nn.grad.conv2d_weight(x, wt.shape, gy, 1, geom.pads[0], dil)
        x3h0 = k.get_x3h()
        for math in ("f32", "f32x3", "f32x3_staged", "f32x3_presplit"):
            k.set_conv_math({"f32": k.MATH_F32, "f32x3": k.MATH_F32X3, "f32x3_staged": k.MATH_F32X3,
                             "f32x3_presplit": k.MATH_F32X3_PRESPLIT}[math])
            if math == "f32x3_staged":
                k.set_x3h(0)
            try:
                sel, _ = k.conv_kernel_id(geom, n, h, w, op)
                assert sel % 100 == {"f32": -1 if sel % 100 in (86, 87, 88, 89) or sel % 100 >= 90 else sel % 100,
                                      "f32x3": 86 if op < 2 and ks * ks * (cin if op == 0 else cout) >= 512 else 95,
                                      "f32x3_staged": 95,
                                      "f32x3_presplit": 88}[math], (math, sel)
                if op == 0:
                    out = nchw(k.conv_fwd(geom, nhwc(x), n, h, w, [w_cl(wt)]))
                elif op == 1:
                    out = nchw(k.conv_dgrad(geom, nhwc(gy), n, h, w, [w_cl(wt)]))
                else:
                    dw = torch.zeros(cout, ks, ks, cin, device=DEV)
                    k.conv_wgrad(geom, nhwc(gy), nhwc(x), n, h, w, [dw], accumulate=False)
                    out = dw.permute(0, 3, 1, 2).double().cpu()
            finally:
                k.set_conv_math(k.MATH_F32X3)   # the library default
                k.set_x3h(x3h0)
            errs[math] = rel(out, ref)
        print(f"op {op} K={cin * ks * ks}: max rel err f32 {errs['f32']:.3e}  f32x3 {errs['f32x3']:.3e}  "
              f"f32x3_staged {errs['f32x3_staged']:.3e}  f32x3_presplit {errs['f32x3_presplit']:.3e}")
        for m in ("f32x3", "f32x3_staged", "f32x3_presplit"):
            assert errs[m] <= 1.5 * errs["f32"] + 1e-7, (m, errs)


@pytest.mark.parametrize("op", [0, 1, 2])
def test_f32x3_is_unbiased(op):
    """The bf16 MFMA's internal sum does not round to nearest: addends far below the largest one
    lose their low bits (a downward bias, experiments/mfma_round.hip).  With the five cross terms
    in the same accumulator as a0*b0 that bias piled up to a mean signed error of -1.1e-8 x
    max|y| on this conv (positive data; fp32 MFMA: +-1e-10); conv_x3.hpp keeps them in their own
    accumulator.  Guard: |mean signed error| <= 1e-9 x max|ref| on all-positive operands, the
    worst case for a one-signed rounding bias."""
    k = K()
    g = torch.Generator().manual_seed(1)
    n, cin, h, w, cout = 2, 256, 32, 48, 256
    geom = k.ConvGeom(cin, cout, 3, 3, 1, (1,), (1,))
    x = torch.rand(n, cin, h, w, generator=g, dtype=torch.float64).float().double()
    wt = (torch.rand(cout, cin, 3, 3, generator=g, dtype=torch.float64) / 2304).float().double()
    gy = torch.rand(n, cout, h, w, generator=g, dtype=torch.float64).float().double()
    assert k.get_conv_math() == k.MATH_F32X3
    if op == 0:
        ref = F.conv2d(x, wt, None, 1, 1)
        out = nchw(k.conv_fwd(geom, nhwc(x), n, h, w, [w_cl(wt)]))
    elif op == 1:
        ref = torch.nn.grad.conv2d_input(x.shape, wt, gy, 1, 1)
        out = nchw(k.conv_dgrad(geom, nhwc(gy), n, h, w, [w_cl(wt)]))
    else:
        ref = torch.nn.grad.conv2d_weight(x, wt.shape, gy, 1, 1)
        dw = torch.zeros(cout, 3, 3, cin, device=DEV)
        k.conv_wgrad(geom, nhwc(gy), nhwc(x), n, h, w, [dw], accumulate=False)
        out = dw.permute(0, 3, 1, 2).double().cpu()
    bias = float(((out - ref) / ref.abs().max()).mean())
    print(f"op {op}: mean signed error {bias:+.2e} x max|ref|")
    assert abs(bias) <= 1e-9, bias


def test_to_nhwc_pad():
    """adaptseg_to_nhwc_pad: strided NCHW source -> NHWC with zero channels, and the
    accumulate form that folds a padded weight gradient back (engine._wgrad_padded)."""
    k = K()
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 19, 7, 9, generator=g)
    xd = x.to(DEV).contiguous(memory_format=torch.channels_last)[:, :, :, :]
    out = k.to_nhwc_pad(xd, 32)
    ref = torch.zeros(2, 7, 9, 32)
    ref[..., :19] = x.permute(0, 2, 3, 1)
    assert torch.equal(out.cpu(), ref)
    # fold: dst[..., :19] += src[..., :19] of a 20-channel buffer
    src = torch.randn(64, 4, 4, 20, generator=g).to(DEV)
    dst0 = torch.randn(64, 4, 4, 19, generator=g)
    dst = dst0.to(DEV)
    k.to_nhwc_pad(src.permute(0, 3, 1, 2)[:, :19], 19, out=dst, accumulate=True)
    assert torch.allclose(dst.cpu(), dst0 + src.cpu()[..., :19], rtol=0, atol=1e-6)
    # NCHW-contiguous 3-channel image -> 4 channels (the stem's weight-gradient input)
    img = torch.randn(2, 3, 11, 13, generator=g)
    p4 = k.to_nhwc_pad(img.to(DEV), 4).cpu()
    assert torch.equal(p4[..., :3], img.permute(0, 2, 3, 1)) and not p4[..., 3].any()


@pytest.mark.parametrize("case", [(4, 64, 64, 96, 64, 1), (2, 256, 48, 64, 256, 3)], ids=["1x1-192split", "3x3-l3"])
def test_folded_splitk_weight_gradient_is_deterministic(case, conv_math):
    """Split-K weight gradients sum their slabs in split order whatever order the splits
    arrive in (the default separate splitk_reduce4 launch, and the ADAPTSEG_SPLITK_FOLD=1
    experiment build's in-kernel fold: write-through slabs, release / acquire around a per-tile
    counter), so repeated launches — with the other stream's kernels shuffling the arrival
    order — are bitwise equal, and match fp64 at the parity tolerance (with accumulate into an
    existing gradient)."""
    k = K()
    n, cin, h, w, cout, ks = case
    geom = k.ConvGeom(cin, cout, ks, ks, 1, ((ks // 2) * 2,), (2,))
    kid, splits = k.conv_kernel_id(geom, n, h, w, 2)
    assert splits > 1, (kid, splits)
    g = torch.Generator().manual_seed(9)
    x = torch.randn(n, cin, h, w, generator=g, dtype=torch.float64)
    gy = torch.randn(n, cout, h, w, generator=g, dtype=torch.float64)
    w0 = torch.randn(cout, cin, ks, ks, generator=g, dtype=torch.float64)
    ref = torch.nn.grad.conv2d_weight(x, w0.shape, gy, 1, geom.pads[0], 2) + w0
    xd, gyd = nhwc(x), nhwc(gy)
    outs = []
    side = torch.cuda.Stream()
    for rep in range(4):
        dw = w_cl(w0).clone()
        if rep % 2:   # busy the chip from another stream so the splits arrive in another order
            with torch.cuda.stream(side):
                torch.randn(4096, 4096, device=DEV) @ torch.randn(4096, 4096, device=DEV)
        k.conv_wgrad(geom, gyd, xd, n, h, w, [dw], accumulate=True)
        torch.cuda.synchronize()
        outs.append(dw.permute(0, 3, 1, 2).double().cpu())
    for o in outs[1:]:
        assert torch.equal(o, outs[0])
    assert rel(outs[0], ref) < 2e-5
