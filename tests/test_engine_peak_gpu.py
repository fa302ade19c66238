"""GPU: the peak device memory of one DeeplabMulti training forward + backward does not grow.

The engine releases each block's saved activations as soon as its backward is done
(engine.py's module docstring); a program that keeps a tensor longer, or stores one more form of
it, computes the same numbers and only shows here.  The bound per conv maths is the value this
same test measured at the commit named in tests/golden/engine_peak_bytes.json (with the torch
version, whose caching allocator rounds the sizes).

What is measured: torch.cuda.max_memory_allocated() over building the model, one train-mode
forward and its backward on a 2x3x97x129 input, minus what was allocated before (other tests'
tensors).  The per-stream conv workspaces and the weight packs are dropped first, so that the
figure does not depend on what ran earlier in the process; WGRAD_STREAM is 0, so that no free is
deferred by record_stream.

Running this module as a script rewrites the fixture (or the file named as its argument):
python tests/test_engine_peak_gpu.py [out.json]
"""
import gc
import json
import os
import sys

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "engine_peak_bytes.json")
MATHS = ("MATH_F32X3", "MATH_BF16")


def peak_bytes(math, setattr_):
    from adaptsegnet_amd import engine, kernels as K, ops
    from adaptsegnet_amd.model import DeeplabMulti
    setattr_(engine, "WGRAD_STREAM", 0)
    prev = K.get_conv_math()
    K.set_conv_math(getattr(K, math))
    try:
        K.clear_weight_packs()
        ops._WS.clear()
        gc.collect()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        torch.manual_seed(7)
        model = DeeplabMulti(num_classes=19).to("cuda").train()
        x = torch.randn(2, 3, 97, 129, device="cuda")
        y1, y2 = model(x, (129, 97))
        (y1.sum() + y2.sum()).backward()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base
    finally:
        K.set_conv_math(prev)
        ops._WS.clear()


@pytest.mark.gpu
@pytest.mark.parametrize("math", MATHS)
def test_peak_memory_does_not_grow(math, monkeypatch):
    with open(FIXTURE) as f:
        want = json.load(f)
    got = peak_bytes(math, monkeypatch.setattr)
    print(f"{math}: peak {got} bytes, recorded {want['peak_bytes'][math]} (torch {want['torch']}, now "
          f"{torch.__version__})")
    assert got <= want["peak_bytes"][math]


if __name__ == "__main__":
    import subprocess
    commit = subprocess.run(["git", "-C", REPO, "rev-parse", "--short", "HEAD"], capture_output=True, text=True)
    data = {"commit": commit.stdout.strip() or None, "torch": torch.__version__,
            "peak_bytes": {m: peak_bytes(m, setattr) for m in MATHS}}
    with open(sys.argv[1] if len(sys.argv) > 1 else FIXTURE, "w") as f:
        json.dump(data, f, indent=1)
        f.write("\n")
    print(data)
