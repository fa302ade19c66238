"""FDA (spectral transfer + robust entropy term): everything that needs no GPU.

A. The reference (tests/fda_ref.py) is itself: identity for trg is src, FDA's rule for b, a vanishing imaginary
   residue, and the closed form ``src + correction`` the kernel rests on equal to the fft2 route in fp64.
B. Registration (ops.FDA_NAMES), the C ABI's symbols and host-side rejections, the Python surface's argument
   errors, StepConfig.ent_eta's validation and entropy_loss2d's dispatch.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from adaptsegnet_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fda_ref as FR  # noqa: E402

FDA_OPS = ["fda_transfer", "entropy_rho_loss_fwd", "entropy_rho_loss_bwd"]


def _images(shape, seed):
    """(src, trg) fp64 on a 0..255 scale with different statistics and some smooth structure."""
    rng = np.random.Generator(np.random.PCG64(seed))
    n, c, h, w = shape
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    ramp = (yy / max(h - 1, 1) + np.sin(2 * np.pi * xx / max(w, 2))) * 20.0
    src = np.clip(rng.integers(0, 256, shape) * 0.7 + 30 + ramp, 0, 255)
    trg = np.clip(rng.integers(0, 256, shape) * 0.5 + 90 - ramp, 0, 255)
    return src, trg


# ---- A. the reference -------------------------------------------------------------------------------------
SHAPES = [((1, 3, 9, 11), 0.45), ((2, 3, 33, 47), 0.1), ((1, 1, 32, 48), 0.09), ((1, 2, 16, 16), 0.01),
          ((1, 1, 40, 30), 0.2)]


@pytest.mark.parametrize("shape,beta", SHAPES)
def test_reference_is_itself(shape, beta):
    src, trg = _images(shape, 3)
    assert np.abs(FR.fda_ref(src, src, beta) - src).max() <= 1e-9   # same amplitudes: nothing changes
    out, residue = FR.fda_ref(src, trg, beta, return_residue=True)
    assert residue <= 1e-9                                          # the swapped spectrum is still Hermitian
    assert np.abs(out - src).max() > 1.0                            # and the transfer does something
    closed, cres = FR.closed_form(src, trg, beta)
    assert np.abs(closed - out).max() <= 1e-9 and cres <= 1e-9      # the identity the kernel rests on


def test_band_follows_fdas_rule_for_odd_and_even_sizes():
    from adaptsegnet_amd.fda import fda_band
    for h, w, beta, b in ((512, 1024, 0.01, 5), (512, 1024, 0.09, 46), (720, 1280, 0.09, 64), (9, 11, 0.45, 4),
                          (33, 47, 0.1, 3), (16, 16, 0.01, 0), (70, 32, 0.05, 1), (10, 10, 0.45, 4), (11, 10, 0.05, 0)):
        assert FR.band(h, w, beta) == b == fda_band(h, w, beta), (h, w, beta)
    # the window is centred at floor(n / 2) after fftshift, for odd and even n: only |u|, |v| <= b change
    for shape in ((1, 1, 9, 12), (1, 1, 10, 9)):
        src, trg = _images(shape, 5)
        h, w = shape[2:]
        b = FR.band(h, w, 0.2)
        fo = np.fft.fft2(FR.fda_ref(src, trg, 0.2))
        fs, ft = np.fft.fft2(src), np.fft.fft2(trg)
        u = np.minimum(np.arange(h), h - np.arange(h))[:, None]
        v = np.minimum(np.arange(w), w - np.arange(w))[None, :]
        win = (u <= b) & (v <= b)
        assert np.abs(fo - fs)[..., ~win].max() <= 1e-8
        assert np.abs(np.abs(fo) - np.abs(ft))[..., win].max() <= 1e-8
        assert np.abs(np.angle(fo * np.conj(fs)))[..., win].max() <= 1e-9   # the phase stays


def test_mean_handling_of_the_reference():
    src, trg = _images((2, 3, 12, 14), 7)
    mean = np.array([104.0, 116.5, 122.75])
    m = mean[None, :, None, None]
    a = FR.fda_ref(src - m, trg - m, 0.2, mean=mean)
    assert np.abs(a - (FR.fda_ref(src, trg, 0.2) - m)).max() <= 1e-9
    closed, _ = FR.closed_form(src - m, trg - m, 0.2, mean=mean)
    assert np.abs(closed - a).max() <= 1e-9
    # the mean matters: a dark source (negative DC once the mean is off) given a bright target's amplitudes gets
    # brighter on raw intensities, but keeps its negative DC phase without the mean
    dark, bright = src * 0.2, trg * 0.2 + 190.0
    with_mean = FR.fda_ref(dark - m, bright - m, 0.2, mean=mean)
    assert np.abs(with_mean.mean(axis=(2, 3)) - (bright - m).mean(axis=(2, 3))).max() <= 1e-9
    assert np.abs(FR.fda_ref(dark - m, bright - m, 0.2) - with_mean).max() > 1.0


def test_twiddle_tables():
    from adaptsegnet_amd.fda import twiddles
    t = twiddles(47, "cpu")
    assert t.dtype == torch.float32 and tuple(t.shape) == (47, 2) and t.is_contiguous()
    ang = 2 * np.pi * np.arange(47) / 47
    assert np.array_equal(t.numpy(), np.stack([np.cos(ang), np.sin(ang)], 1).astype(np.float32))
    assert twiddles(47, "cpu") is t   # cached per (n, device)


# ---- B. registration and the C ABI ---------------------------------------------------------------------------
def test_ops_are_registered_in_a_list_of_their_own():
    from adaptsegnet_amd import ops
    assert ops.FDA_NAMES == FDA_OPS
    others = set(ops.NAMES) | set(ops.LOSS_NAMES) | set(ops.MIX_NAMES) | set(ops.AUG_NAMES)
    assert not set(FDA_OPS) & others
    for name in FDA_OPS:
        op = getattr(torch.ops.adaptseg, name).default
        assert torch._C._dispatch_has_kernel_for_dispatch_key(op.name(), "CUDA"), name
        assert not torch._C._dispatch_has_kernel_for_dispatch_key(op.name(), "CPU"), name
        assert len(op._schema.returns) == 0, name
        assert any(a.alias_info is not None and a.alias_info.is_write for a in op._schema.arguments), name
        assert getattr(ops.OPS, name) is op


def test_entry_points_are_declared_and_exported():
    for s in ("adaptseg_fda_workspace_size", "adaptseg_fda_transfer", "adaptseg_entropy_rho_loss_fwd",
              "adaptseg_entropy_rho_loss_bwd"):
        assert s in _lib.header_symbols() and s in _lib._SIGS and hasattr(_lib.lib(), s), s
    assert set(_lib.header_symbols()) == set(_lib._SIGS)


def test_fda_abi_argument_checks_run_on_the_host():
    L = _lib.lib()
    err = lambda: L.adaptseg_last_error().decode()  # noqa: E731
    src, trg, out = ctypes.c_void_p(1 << 20), ctypes.c_void_p(2 << 20), ctypes.c_void_p(3 << 20)
    tab, ws = ctypes.c_void_p(4 << 20), ctypes.c_void_p(5 << 20)   # never dereferenced: every call is rejected
    sz = ctypes.c_size_t(0)
    assert L.adaptseg_fda_workspace_size(2, 3, 32, 48, 3, ctypes.byref(sz)) == 0
    # R of both images and G: [nc][h][b+1] float2 each; D: [nc][2b+1][b+1] float2
    assert sz.value == (3 * 6 * 32 * 4 + 6 * 7 * 4) * 8
    assert L.adaptseg_fda_workspace_size(2, 3, 32, 48, 3, None) == 1 and "fda" in err()

    def call(n=2, c=3, h=32, w=48, b=3, **kw):
        a = dict(src=src, trg=trg, mean=None, tw_w=tab, tw_h=tab, out=out, ws=ws, ws_bytes=sz.value) | kw
        return L.adaptseg_fda_transfer(n, c, h, w, b, a["src"], a["trg"], a["mean"], a["tw_w"], a["tw_h"], a["out"],
                                       a["ws"], a["ws_bytes"], None)
    for shape in ((0, 3, 32, 48), (2, 0, 32, 48), (2, 3, -1, 48), (2, 3, 32, 0)):
        assert call(*shape) == 1 and "fda" in err(), shape
        assert L.adaptseg_fda_workspace_size(*shape, 0, ctypes.byref(sz)) == 1 and "fda" in err(), shape
    assert L.adaptseg_fda_workspace_size(2, 3, 32, 48, 3, ctypes.byref(sz)) == 0
    for b in (-1, 16, 1 << 30):   # 2 b + 1 > min(h, w) = 32
        assert call(b=b) == 1 and "fda" in err() and "2 b + 1" in err(), b
        assert L.adaptseg_fda_workspace_size(2, 3, 32, 48, b, ctypes.byref(sz)) == 1 and "2 b + 1" in err(), b
    assert L.adaptseg_fda_workspace_size(2, 3, 32, 48, 3, ctypes.byref(sz)) == 0
    assert call(h=31, w=48, b=15) == 4    # 2 b + 1 == min(h, w) passes the shape checks (the workspace is short)
    assert call(h=4096, w=4096) == 1 and "2^24" in err()
    assert call(h=4, w=_lib.FDA_MAX_W + 4) == 1 and "fda" in err() and str(_lib.FDA_MAX_W) in err()
    assert call(n=30000) == 1 and "65535" in err()
    for k in ("src", "trg", "tw_w", "tw_h", "out"):
        assert call(**{k: None}) == 1 and "fda" in err() and "null" in err(), k
    assert call(out=src) == 1 and "fda" in err() and "alias" in err()
    assert call(out=trg) == 1 and "alias" in err()
    assert call(out=ctypes.c_void_p((1 << 20) + 64)) == 1 and "alias" in err()   # a partial overlap
    assert call(tw_w=ctypes.c_void_p((4 << 20) + 4)) == 1 and "aligned" in err()
    for kw in (dict(ws=None), dict(ws_bytes=sz.value - 1), dict(ws_bytes=0), dict(ws=ctypes.c_void_p((5 << 20) + 4))):
        assert call(**kw) == 4 and "fda" in err() and "workspace" in err(), kw


def test_rho_abi_argument_checks_run_on_the_host():
    L = _lib.lib()
    p = ctypes.c_void_p(256)
    err = lambda: L.adaptseg_last_error().decode()  # noqa: E731
    fwd, bwd = L.adaptseg_entropy_rho_loss_fwd, L.adaptseg_entropy_rho_loss_bwd
    assert fwd(16, 1, 2.0, 1e-8, p, p, p, 64, None) == 1 and "entropy_rho_loss_fwd" in err()   # ln 1 = 0
    assert bwd(16, 1, 2.0, 1e-8, p, p, p, 0, None) == 1 and "entropy_rho_loss_bwd" in err()
    assert fwd(0, 19, 2.0, 1e-8, p, p, p, 64, None) == 1 and fwd(16, 19, 2.0, 1e-8, None, p, p, 64, None) == 1
    assert fwd(16, 19, 2.0, 1e-8, p, None, p, 64, None) == 1
    assert bwd(16, 19, 2.0, 1e-8, p, None, p, 0, None) == 1 and bwd(16, 19, 2.0, 1e-8, p, p, None, 0, None) == 1
    for eta, eps in ((0.0, 1e-8), (-1.0, 1e-8), (float("nan"), 1e-8), (17.0, 1e-8), (2.0, 0.0), (2.0, -1.0), (2.0, 2.0)):
        assert fwd(16, 19, eta, eps, p, p, p, 64, None) == 1 and "eta" in err(), (eta, eps)
        assert bwd(16, 19, eta, eps, p, p, p, 0, None) == 1 and "eta" in err(), (eta, eps)
    assert fwd(16, 19, 2.0, 1e-8, p, p, None, 0, None) == 4 and "workspace" in err()
    assert fwd(16, 19, 2.0, 1e-8, p, p, p, 4, None) == 4 and "entropy_rho_loss_fwd" in err()


# ---- the Python surface ------------------------------------------------------------------------------------------
def test_python_surface_validates_before_any_launch():
    from adaptsegnet_amd.fda import fda_source_to_target as fda
    x = torch.zeros(2, 3, 16, 20)
    with pytest.raises(NotImplementedError, match="adaptseg::fda_transfer"):   # no CPU kernel, no fallback
        fda(x, x.clone())
    with pytest.raises(NotImplementedError, match="adaptseg::fda_transfer"):
        fda(torch.zeros(1, 1, 16, 20), torch.zeros(1, 1, 16, 20), mean=None)
    with pytest.raises(RuntimeError, match="resize"):
        fda(x, torch.zeros(2, 3, 16, 24))
    with pytest.raises(RuntimeError, match="resize"):
        fda(x, torch.zeros(1, 3, 16, 20))
    with pytest.raises(RuntimeError, match="float32"):
        fda(x.double(), x.double())
    with pytest.raises(RuntimeError, match="float32"):
        fda(x, x.half())
    with pytest.raises(RuntimeError, match="N, C, H, W"):
        fda(x[0], x[0])
    with pytest.raises(RuntimeError, match="contiguous"):
        fda(x.contiguous(memory_format=torch.channels_last), x)
    with pytest.raises(RuntimeError, match="contiguous"):
        fda(x, torch.zeros(2, 3, 20, 16).transpose(2, 3))
    for beta in (-0.01, 0.5, 0.6, float("nan"), float("inf")):   # 0.5: b = 8, 2 b + 1 = 17 > 16
        with pytest.raises(ValueError, match="beta"):
            fda(x, x, beta=beta)
    with pytest.raises(ValueError, match="mean"):
        fda(x, x, mean=(1.0, 2.0))
    with pytest.raises(ValueError, match="mean"):   # the default mean has three values
        fda(torch.zeros(1, 1, 16, 20), torch.zeros(1, 1, 16, 20))
    with pytest.raises(ValueError, match="finite"):
        fda(x, x, mean=(1.0, float("nan"), 3.0))
    with pytest.raises(ValueError, match="W <="):
        fda(torch.zeros(1, 1, 2, _lib.FDA_MAX_W + 1), torch.zeros(1, 1, 2, _lib.FDA_MAX_W + 1), mean=None)


class _NoModel(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))


def test_step_config_ent_eta():
    from adaptsegnet_amd.train import AdaptSegTrainer, StepConfig
    assert StepConfig().ent_eta is None
    with pytest.raises(ValueError, match="ent_eta"):
        StepConfig(ent_eta=2.0, lambda_ent=0)
    with pytest.raises(ValueError, match="ent_eta"):
        StepConfig(ent_eta=2.0)
    cfg = StepConfig(ent_eta=2.0, lambda_ent=0.005)
    AdaptSegTrainer(_NoModel(), None, _NoModel(), cfg)
    cfg.lambda_ent = 0.0   # changed after it was made: the trainer checks again
    with pytest.raises(ValueError, match="ent_eta"):
        AdaptSegTrainer(_NoModel(), None, _NoModel(), cfg)
    for eta in (0.0, -1.0, 17.0):
        with pytest.raises(ValueError, match="ent_eta"):
            AdaptSegTrainer(_NoModel(), None, _NoModel(), StepConfig(ent_eta=eta, lambda_ent=1.0))


class _Called(Exception):
    pass


def test_entropy_loss2d_dispatch(monkeypatch):
    """eta=None is today's call on today's op; with eta the robust op runs instead."""
    from adaptsegnet_amd import functional as AF
    from adaptsegnet_amd import kernels as K
    calls = []

    class X:   # passes the function's checks without a device
        is_cuda, dtype, shape = True, torch.float32, (2, 19, 4, 5)

        def dim(self):
            return 4

    def spy(name):
        def f(*a):
            calls.append((name,) + a[1:])
            raise _Called(name)
        return f
    monkeypatch.setattr(K, "nhwc_view", lambda x: x)
    monkeypatch.setattr(K, "entropy_fwd", spy("plain"))
    monkeypatch.setattr(K, "entropy_rho_fwd", spy("rho"))
    monkeypatch.setattr(AF._EntropyLoss2d, "apply", staticmethod(lambda x: AF._EntropyLoss2d.forward(_Ctx(), x)))
    monkeypatch.setattr(AF._EntropyRhoLoss2d, "apply",
                        staticmethod(lambda x, eta, eps: AF._EntropyRhoLoss2d.forward(_Ctx(), x, eta, eps)))
    for kw in (dict(), dict(eta=None), dict(eta=None, eps=0.5)):
        with pytest.raises(_Called, match="plain"):
            AF.entropy_loss2d(X(), **kw)
    assert calls == [("plain",)] * 3
    with pytest.raises(_Called, match="rho"):
        AF.entropy_loss2d(X(), eta=2.0)
    with pytest.raises(_Called, match="rho"):
        AF.entropy_loss2d(X(), eta=0.5, eps=1e-6)
    assert calls[3:] == [("rho", 2.0, 1e-8), ("rho", 0.5, 1e-6)]
    for bad in (dict(eta=0.0), dict(eta=-1.0), dict(eta=float("nan")), dict(eta=2.0, eps=0.0)):
        with pytest.raises(ValueError, match="eta"):
            AF.entropy_loss2d(X(), **bad)


def test_rho_ops_have_no_cpu_kernel():
    from adaptsegnet_amd import kernels as K
    x = torch.zeros(2, 4, 4, 19)
    with pytest.raises(NotImplementedError, match="adaptseg::entropy_rho_loss_fwd"):
        K.entropy_rho_fwd(x, 2.0, 1e-8)
    with pytest.raises(NotImplementedError, match="adaptseg::entropy_rho_loss_bwd"):
        K.entropy_rho_bwd(x, 2.0, 1e-8, torch.ones(1))


class _Ctx:
    def save_for_backward(self, *a):
        pass
