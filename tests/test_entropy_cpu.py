"""Entropy-based adaptation (selfinfo / entropy-loss ops, StepConfig.d_input / lambda_ent): host-side checks.

No GPU: the op registration (ops.LOSS_NAMES, held to what tests/test_custom_ops_cpu.py asks of
ops.NAMES), the C ABI's argument checks, which run before any launch, and the trainer's validation.
"""
import ctypes

import pytest
import torch

from adaptsegnet_amd import _lib

NEW_OPS = {"selfinfo_fwd", "selfinfo_bwd", "entropy_loss_fwd", "entropy_loss_bwd"}


def test_loss_ops_are_registered_beside_the_engine_ops():
    from adaptsegnet_amd import ops
    assert set(ops.LOSS_NAMES) == NEW_OPS and len(ops.LOSS_NAMES) == len(NEW_OPS)
    assert not NEW_OPS & set(ops.NAMES)   # the engine's traced op set is as it was
    assert {"softmax_fwd", "softmax_bwd", "softmax_ce_fwd", "adv_loss_fwd"} <= set(ops.NAMES)
    for name in ops.LOSS_NAMES:
        op = getattr(torch.ops.adaptseg, name).default
        assert torch._C._dispatch_has_kernel_for_dispatch_key(op.name(), "CUDA"), name
        assert not torch._C._dispatch_has_kernel_for_dispatch_key(op.name(), "CPU"), name
        schema = op._schema
        assert len(schema.returns) == 0, name
        assert any(a.alias_info is not None and a.alias_info.is_write for a in schema.arguments), name
        assert getattr(ops.OPS, name) is op
    for name in ops.NAMES:
        assert getattr(ops.OPS, name) is getattr(torch.ops.adaptseg, name).default


def test_cpu_tensors_raise():
    from adaptsegnet_amd import kernels as K
    x = torch.zeros(2, 4, 4, 19)
    with pytest.raises(NotImplementedError, match="adaptseg::selfinfo_fwd"):
        K.selfinfo_fwd(x)
    with pytest.raises(NotImplementedError, match="adaptseg::selfinfo_bwd"):
        K.selfinfo_bwd(x, x)
    with pytest.raises(NotImplementedError, match="adaptseg::entropy_loss_fwd"):
        K.entropy_fwd(x)
    with pytest.raises(NotImplementedError, match="adaptseg::entropy_loss_bwd"):
        K.entropy_bwd(x, torch.ones(1))


def test_fake_tensor_tracing():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from adaptsegnet_amd import kernels as K
    with FakeTensorMode():
        x = torch.empty(2, 8, 10, 19, device="cuda")
        assert K.selfinfo_fwd(x).shape == x.shape
        assert K.selfinfo_bwd(x, x).shape == x.shape
        assert K.entropy_fwd(x).shape == (1,)
        assert K.entropy_bwd(x, torch.empty(1, device="cuda")).shape == x.shape


def test_abi_argument_checks_run_on_the_host():
    L = _lib.lib()
    p = ctypes.c_void_p(256)   # never dereferenced: every call below is rejected before a launch
    err = lambda: L.adaptseg_last_error().decode()  # noqa: E731
    b = ctypes.c_size_t(0)
    assert L.adaptseg_entropy_workspace_size(4097, ctypes.byref(b)) == 0 and b.value > 0
    # the partials are capped at 4 row tiles per block: 4097 rows already loop the loss kernel
    assert b.value % 8 == 0 and (b.value // 8) * 256 < 4097
    assert L.adaptseg_entropy_workspace_size(0, ctypes.byref(b)) == 1
    assert L.adaptseg_entropy_workspace_size(16, None) == 1
    # c = 1: ln C = 0
    assert L.adaptseg_selfinfo_fwd(16, 1, p, p, None) == 1 and "selfinfo_fwd" in err()
    assert L.adaptseg_selfinfo_bwd(16, 1, p, p, p, 0, None) == 1 and "selfinfo_bwd" in err()
    assert L.adaptseg_entropy_loss_fwd(16, 1, p, p, p, 64, None) == 1 and "entropy_loss_fwd" in err()
    assert L.adaptseg_entropy_loss_bwd(16, 1, p, p, p, 0, None) == 1 and "entropy_loss_bwd" in err()
    # NULL pointers, rows <= 0
    assert L.adaptseg_selfinfo_fwd(16, 19, None, p, None) == 1 and "selfinfo_fwd" in err()
    assert L.adaptseg_selfinfo_fwd(16, 19, p, None, None) == 1
    assert L.adaptseg_selfinfo_fwd(0, 19, p, p, None) == 1
    assert L.adaptseg_selfinfo_bwd(16, 19, p, None, p, 0, None) == 1 and "selfinfo_bwd" in err()
    assert L.adaptseg_selfinfo_bwd(16, 19, p, p, None, 0, None) == 1
    assert L.adaptseg_selfinfo_bwd(-1, 19, p, p, p, 0, None) == 1
    assert L.adaptseg_entropy_loss_fwd(16, 19, None, p, p, 64, None) == 1 and "entropy_loss_fwd" in err()
    assert L.adaptseg_entropy_loss_fwd(16, 19, p, None, p, 64, None) == 1
    assert L.adaptseg_entropy_loss_bwd(16, 19, p, None, p, 0, None) == 1 and "entropy_loss_bwd" in err()
    assert L.adaptseg_entropy_loss_bwd(16, 19, p, p, None, 0, None) == 1
    # workspace: NULL or short
    assert L.adaptseg_entropy_loss_fwd(16, 19, p, p, None, 0, None) == 4 and "workspace" in err()
    assert L.adaptseg_entropy_loss_fwd(16, 19, p, p, p, 4, None) == 4 and "workspace" in err()


class _NoModel(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))


def _make(**cfg):
    from adaptsegnet_amd.train import AdaptSegTrainer, StepConfig
    return AdaptSegTrainer(_NoModel(), None, _NoModel(), StepConfig(**cfg))


def test_step_config_defaults_and_validation():
    from adaptsegnet_amd.train import StepConfig
    c = StepConfig()
    assert c.d_input == "softmax" and c.lambda_ent == 0.0
    with pytest.raises(ValueError, match="lambda_ent"):
        _make(lambda_ent=-0.5)
    with pytest.raises(ValueError, match="lambda_ent"):
        _make(level="source-only", lambda_ent=0.5)
    with pytest.raises(ValueError, match="d_input"):
        _make(d_input="probability")
