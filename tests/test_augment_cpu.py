"""Random scale / crop / mirror augmentation of the input pipeline — host side (no GPU).

The sampler's rule and reproducibility, the op's registration and fake kernel, the host
validation of adaptseg_gta5_preprocess_augment, and that the workspace follows the crop window
rather than the scaled image.
"""
import ctypes

import numpy as np
import pytest
import torch

from adaptsegnet_amd import _lib, data

SCALES = tuple(round(0.5 + 0.1 * i, 1) for i in range(11))


def test_sampler_is_reproducible_per_seed_and_rank():
    a = data.AugmentSampler((1280, 720), seed=7, rank=0).sample(64)
    b = data.AugmentSampler((1280, 720), seed=7, rank=0).sample(64)
    c = data.AugmentSampler((1280, 720), seed=7, rank=1).sample(64)
    assert a.dtype == np.int32 and a.shape == (64, 5)
    assert np.array_equal(a, b)
    assert not np.array_equal(a, c)


def test_sampler_state_round_trip():
    s = data.AugmentSampler((321, 321), seed=3)
    s.sample(5)
    state = s.get_state()
    want = s.sample(9)
    t = data.AugmentSampler((321, 321), seed=99)
    t.set_state(state)
    assert np.array_equal(t.sample(9), want)
    s.set_state(state)
    assert np.array_equal(s.sample(9), want)


def test_sampler_follows_the_rule():
    cw, ch = 48, 32
    p = data.AugmentSampler((cw, ch), seed=1).sample(2000)
    sizes = {(int(cw * f + 0.5), int(ch * f + 0.5)) for f in SCALES}
    assert {(int(a), int(b)) for a, b in p[:, :2]} == sizes      # every scale occurs, nothing else
    for sw, sh, ox, oy, m in p:
        assert 0 <= ox <= max(sw - cw, 0) and 0 <= oy <= max(sh - ch, 0)   # window inside R, or offset 0
        assert m in (0, 1)
    assert set(p[:, 4]) == {0, 1}
    big = p[p[:, 0] > cw]
    assert big[:, 2].max() > 0 and big[:, 3].max() > 0
    assert not data.AugmentSampler((cw, ch), mirror=False).sample(500)[:, 4].any()


def test_op_is_registered_with_cuda_and_fake_kernels():
    from adaptsegnet_amd import ops
    assert "gta5_preprocess_augment" in ops.NAMES
    op = torch.ops.adaptseg.gta5_preprocess_augment.default
    assert torch._C._dispatch_has_kernel_for_dispatch_key(op.name(), "CUDA")
    assert not torch._C._dispatch_has_kernel_for_dispatch_key(op.name(), "CPU")
    assert ops.OPS.gta5_preprocess_augment is op    # the fake kernel is exercised below
    assert len(op._schema.returns) == 0
    assert sum(a.alias_info is not None and a.alias_info.is_write for a in op._schema.arguments) == 2


def test_fake_tensor_shape_propagation():
    from torch._subclasses.fake_tensor import FakeTensorMode
    params = np.array([[72, 48, 24, 16, 1], [24, 16, 0, 0, 0]], np.int32)
    with FakeTensorMode():
        img = torch.empty(2, 37, 53, 3, dtype=torch.uint8, device="cuda")
        lab = torch.empty(2, 37, 53, dtype=torch.uint8, device="cuda")
        lut = torch.empty(256, dtype=torch.int32, device="cuda")
        image, label = data.preprocess_augmented(img, lab, (48, 32), params, lut=lut)
        assert image.shape == (2, 3, 32, 48) and image.dtype == torch.float32
        assert label.shape == (2, 32, 48) and label.dtype == torch.int64
        image, label = data.preprocess_augmented(img, None, (48, 32), params)
        assert image.shape == (2, 3, 32, 48) and label is None


def test_python_rejects_malformed_params_before_the_library():
    img = torch.zeros(1, 37, 53, 3, dtype=torch.uint8)
    good = np.array([[48, 32, 0, 0, 0]], np.int32)
    with pytest.raises(ValueError, match="GPU"):
        data.preprocess_augmented(img, None, (48, 32), good)          # CPU tensors
    for bad in (good.astype(np.float32), good[0], np.zeros((2, 5), np.int32), [[0, 32, 0, 0, 0]],
                [[48, 32, 0, 0, 2]], [[48, 32, 1 << 20, 0, 0]], [[3, 32, 0, 0, 0]]):
        with pytest.raises(ValueError, match="augment params"):
            data.check_augment_params(bad, 1, 37, 53)
    assert data.check_augment_params(good.astype(np.int64), 1, 37, 53).dtype == np.int32


def _call(n, in_h, in_w, ch, cw, params, ws=None, ws_bytes=0):
    L = _lib.lib()
    pa = (ctypes.c_int32 * (5 * n))(*np.asarray(params, np.int32).reshape(-1).tolist())
    fake = ctypes.c_void_p(256)    # never dereferenced: every case below stops on the host
    return L.adaptseg_gta5_preprocess_augment(n, in_h, in_w, ch, cw, fake, 0.0, 0.0, 0.0, fake, None, None, None,
                                              pa, 255, ws, ws_bytes, None)


def test_c_abi_validates_on_the_host():
    """Bad parameters come back as ADAPTSEG_ERR_ARG (1) and a missing workspace as
    ADAPTSEG_ERR_WORKSPACE (4), before any launch (this test runs without a GPU)."""
    L = _lib.lib()
    b = ctypes.c_size_t(0)
    for params in ([[0, 32, 0, 0, 0]],        # sw = 0
                   [[48, 32, 0, 0, 2]],       # mirror = 2
                   [[3, 32, 0, 0, 0]],        # 53 / 3: downscale above 15x
                   [[48, 2, 0, 0, 0]],        # 37 / 2 likewise, vertically
                   [[48, 32, 1 << 20, 0, 0]],
                   [[48, 32, 0, -(1 << 20), 0]]):
        assert _call(1, 37, 53, 32, 48, params) == 1, params
        assert b"preprocess_augment" in L.adaptseg_last_error()
        pa = (ctypes.c_int32 * 5)(*params[0])
        assert L.adaptseg_preprocess_augment_workspace_size(1, 37, 53, 32, 48, pa, ctypes.byref(b)) == 1
    good = [[72, 48, 24, 16, 1]]
    pa = (ctypes.c_int32 * 5)(*good[0])
    assert L.adaptseg_preprocess_augment_workspace_size(1, 37, 53, 32, 48, None, ctypes.byref(b)) == 1
    assert L.adaptseg_preprocess_augment_workspace_size(1, 37, 53, 32, 48, pa, ctypes.byref(b)) == 0
    assert b.value > 0
    assert _call(1, 37, 53, 32, 48, good) == 4                                    # null workspace
    assert b"workspace" in L.adaptseg_last_error()
    assert _call(1, 37, 53, 32, 48, good, ctypes.c_void_p(256), b.value - 1) == 4   # short workspace


def test_workspace_follows_the_window_not_the_scaled_image():
    """GTA5 geometry at factor 1.5: the horizontal intermediate is at most crop-wide, so the whole
    workspace is smaller than a full-width (sw = 1920) intermediate alone."""
    n, in_h, in_w, (cw, ch) = 4, 1052, 1914, (1280, 720)
    sw, sh = int(cw * 1.5 + 0.5), int(ch * 1.5 + 0.5)
    assert (sw, sh) == (1920, 1080)
    params = np.array([[sw, sh, 320, 180, i % 2] for i in range(n)], np.int32)
    pa = (ctypes.c_int32 * (5 * n))(*params.reshape(-1).tolist())
    b = ctypes.c_size_t(0)
    assert _lib.lib().adaptseg_preprocess_augment_workspace_size(n, in_h, in_w, ch, cw, pa, ctypes.byref(b)) == 0
    assert 0 < b.value < n * in_h * sw * 3
    assert b.value < n * in_h * cw * 3 + (1 << 20)    # and no more than crop-wide rows plus the tables
