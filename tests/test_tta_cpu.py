"""Multi-scale / mirrored inference, host side (no GPU): the C-ABI entry point and its host
validation, the size rule, the argument checks of evaluate.fuse_argmax / predict_tta (raised
before any forward or launch) and the torch op under FakeTensor.
"""
import ctypes

import pytest
import torch

from adaptsegnet_amd import _lib


def test_fuse_argmax_is_declared_and_exported():
    assert "adaptseg_fuse_argmax" in _lib.header_symbols()
    assert "adaptseg_fuse_argmax" in _lib._SIGS
    assert hasattr(_lib.lib(), "adaptseg_fuse_argmax")
    assert (_lib.FUSE_MAX_MAPS, _lib.FUSE_PROB, _lib.FUSE_LOGIT) == (8, 0, 1)
    text = open(_lib.HEADER_PATH).read()
    for line in ("#define ADAPTSEG_FUSE_MAX_MAPS 8", "#define ADAPTSEG_FUSE_PROB 0", "#define ADAPTSEG_FUSE_LOGIT 1"):
        assert line in text, line


def _desc(nmaps=2, n=1, c=19, oh=16, ow=24, mode=0, hw=(5, 7)):
    d = _lib.FuseDesc()
    d.n, d.c, d.oh, d.ow, d.nmaps, d.mode = n, c, oh, ow, nmaps, mode
    for s in range(min(max(nmaps, 0), _lib.FUSE_MAX_MAPS)):
        d.h[s], d.w[s], d.mirror[s] = hw[0], hw[1], s & 1
        d.x[s] = 4096   # never dereferenced: every case below is rejected on the host
    return d


def _null_map(d):
    d.x[1] = None


def _zero_h(d):
    d.h[1] = 0


def _neg_w(d):
    d.w[0] = -3


BAD = {
    "nmaps-0": (dict(nmaps=0), None, 64, None),
    "nmaps-9": (dict(nmaps=9), None, 64, None),
    "n-0": (dict(n=0), None, 64, None),
    "c-0": (dict(c=0), None, 64, None),
    "oh-0": (dict(oh=0), None, 64, None),
    "ow-negative": (dict(ow=-1), None, 64, None),
    "map-h-0": (dict(), _zero_h, 64, None),
    "map-w-negative": (dict(), _neg_w, 64, None),
    "c-257": (dict(c=257), None, 64, None),
    "null-map": (dict(), _null_map, 64, None),
    "null-out": (dict(), None, None, None),
    "mode-2": (dict(mode=2), None, 64, None),
    "mode-negative": (dict(mode=-1), None, 64, None),
    "conf-in-logit-mode": (dict(mode=1), None, 64, 128),
}


@pytest.mark.parametrize("case", sorted(BAD))
def test_host_validation_without_gpu(case):
    """Every bad descriptor is rejected before any launch: status 1 and a message."""
    L = _lib.lib()
    kw, edit, out, conf = BAD[case]
    d = _desc(**kw)
    if edit is not None:
        edit(d)
    assert L.adaptseg_timing_reserve(-1) == 1   # the thread's last error now speaks of something else
    st = L.adaptseg_fuse_argmax(ctypes.byref(d), ctypes.c_void_p(out) if out else None,
                                ctypes.c_void_p(conf) if conf else None, None)
    assert st == 1, (case, st)
    assert b"fuse_argmax" in L.adaptseg_last_error(), L.adaptseg_last_error()


def test_tta_sizes():
    from adaptsegnet_amd.evaluate import tta_sizes
    assert tta_sizes((512, 1024), (0.5, 0.75, 1.0, 1.25)) == [(256, 512), (384, 768), (512, 1024), (640, 1280)]
    assert tta_sizes((321, 321), (0.75,)) == [(241, 241)]
    for bad in (0, -1):
        with pytest.raises(ValueError):
            tta_sizes((64, 96), (1.0, bad))


def test_fuse_argmax_argument_checks():
    """ValueErrors come before anything touches the device (CPU tensors get that far); then a
    non-HIP or non-fp32 map is a RuntimeError."""
    from adaptsegnet_amd.evaluate import fuse_argmax
    m = torch.zeros(1, 19, 4, 6)
    with pytest.raises(ValueError, match="maps"):
        fuse_argmax([m] * 9)
    with pytest.raises(ValueError, match="maps"):
        fuse_argmax([])
    with pytest.raises(ValueError, match="same N and C"):
        fuse_argmax([m, torch.zeros(2, 19, 4, 6)])
    with pytest.raises(ValueError, match="same N and C"):
        fuse_argmax([m, torch.zeros(1, 5, 4, 6)])
    with pytest.raises(ValueError, match="logit"):
        fuse_argmax([m], mode="logit", return_confidence=True)
    with pytest.raises(ValueError, match="mode"):
        fuse_argmax([m], mode="mean")
    with pytest.raises(ValueError, match="mirror flags"):
        fuse_argmax([m, m], mirrored=[True])
    with pytest.raises(RuntimeError, match="float32 HIP"):
        fuse_argmax([m])
    with pytest.raises(RuntimeError, match="float32 HIP"):
        fuse_argmax([m.double()])


class _NoForward(torch.nn.Module):
    def forward(self, x):
        raise AssertionError("predict_tta ran a forward before checking its arguments")


def test_predict_tta_argument_checks_run_no_forward():
    from adaptsegnet_amd.evaluate import predict_tta
    x = torch.zeros(1, 3, 64, 96)
    model = _NoForward()
    with pytest.raises(ValueError, match="10 maps"):
        predict_tta(model, x, scales=(0.5, 0.75, 1.0, 1.25, 1.5), mirror=True)
    with pytest.raises(ValueError, match="9 maps"):
        predict_tta(model, x, scales=(1.0,) * 9, mirror=False)
    with pytest.raises(ValueError):
        predict_tta(model, x, scales=(), mirror=True)
    with pytest.raises(ValueError, match="scale"):
        predict_tta(model, x, scales=(1.0, 0.0))
    with pytest.raises(ValueError, match="logit"):
        predict_tta(model, x, mode="logit", return_confidence=True)
    # the stub does raise once the arguments are fine
    with pytest.raises(AssertionError, match="ran a forward"):
        predict_tta(model, x, scales=(1.0,), mirror=False)


def test_torch_op_is_registered_and_traces_under_fake_tensor():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from adaptsegnet_amd import ops
    from adaptsegnet_amd.evaluate import fuse_argmax
    assert "fuse_argmax" in ops.NAMES
    op = torch.ops.adaptseg.fuse_argmax.default
    assert torch._C._dispatch_has_kernel_for_dispatch_key(op.name(), "CUDA")
    assert not torch._C._dispatch_has_kernel_for_dispatch_key(op.name(), "CPU")
    assert str(op._schema) == ("adaptseg::fuse_argmax(Tensor[] maps, int[] mirror, int mode, Tensor(a!) out, "
                               "Tensor(b!)? conf) -> ()")
    with FakeTensorMode():
        maps = [torch.empty(2, 9, 13, 19, device="cuda"), torch.empty(2, 12, 17, 19, device="cuda")]
        out = torch.empty(2, 40, 56, dtype=torch.uint8, device="cuda")
        conf = torch.empty(2, 40, 56, device="cuda")
        assert torch.ops.adaptseg.fuse_argmax(maps, [0, 1], 0, out, conf) is None
        assert torch.ops.adaptseg.fuse_argmax(maps, [0, 1], 1, out, None) is None
        nchw = [torch.empty(2, 19, 9, 13, device="cuda"),
                torch.empty(2, 19, 12, 17, device="cuda").contiguous(memory_format=torch.channels_last)]
        pred, p = fuse_argmax(nchw, [False, True], (40, 56), return_confidence=True)
        assert pred.shape == (2, 40, 56) and pred.dtype == torch.uint8
        assert p.shape == (2, 40, 56) and p.dtype == torch.float32
        assert fuse_argmax(nchw, out_hw=(8, 8), mode="logit").shape == (2, 8, 8)
