#!/usr/bin/env python3
"""Kernel times of the entropy-adaptation ops (functional.selfinfo2d / entropy_loss2d) beside their
unfused composition.

    python tools/bench_entropy.py [--shape 4x19x512x1024] [--reps 200] [--rounds 5] [--out FILE]

Times ``selfinfo_fwd``, ``selfinfo_bwd``, ``entropy_loss_fwd`` and ``entropy_loss_bwd`` on one
N x C x H x W map of logits (NHWC in memory; the default is config c2's prediction).  The yardstick,
in the same process, is what a user would compose without them: ``softmax_fwd`` / ``softmax_bwd``
plus torch element-wise ops and reductions (``entr``, ``log``, ``mul``, ``sum``, ``mean``), with the
softmax kept for the backward as autograd would keep it.  Each figure is HIP-event time over
``--reps`` back-to-back launches after a warm-up, the median (min .. max) of ``--rounds`` rounds that
alternate between the kernels; GB/s are against the algorithmic bytes (8 rows C for the map forward,
12 rows C for its backward, 4 rows C / 8 rows C for the loss).  Prints the lines and ONE JSON line;
``--out`` also writes the lines to a file.
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def _event_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=lambda v: tuple(int(t) for t in v.split("x")), default=(4, 19, 512, 1024))
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from adaptsegnet_amd import _lib
    from adaptsegnet_amd.ops import OPS
    dev = torch.device("cuda", 0)
    n, c, h, w = args.shape
    rows = n * h * w
    k = 1.0 / math.log(c)
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(n, h, w, c, generator=g) * 3).to(dev)
    dy = torch.randn(n, h, w, c, generator=g).to(dev)
    gl = torch.ones(1, device=dev)
    y, dx, p = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
    loss = torch.empty(1, device=dev)
    OPS.softmax_fwd(x, p)   # the map the unfused backwards read (kept by autograd)

    def map_fwd_unfused():
        OPS.softmax_fwd(x, p)
        return torch.special.entr(p).mul_(k)

    def map_bwd_unfused():
        gp = torch.log(p).add_(1.0).mul_(dy).mul_(-k)
        OPS.softmax_bwd(p, gp, dx, False)

    def loss_fwd_unfused():
        OPS.softmax_fwd(x, p)
        return torch.special.entr(p).sum(dim=-1).mean().mul_(k)

    def loss_bwd_unfused():
        gp = torch.log(p).add_(1.0).mul_(gl * (-k / rows))
        OPS.softmax_bwd(p, gp, dx, False)

    e = rows * c
    kernels = {
        "selfinfo_fwd": (lambda: OPS.selfinfo_fwd(x, y), 8 * e),
        "selfinfo_fwd/unfused": (map_fwd_unfused, 8 * e),
        "selfinfo_bwd": (lambda: OPS.selfinfo_bwd(x, dy, dx, False), 12 * e),
        "selfinfo_bwd/unfused": (map_bwd_unfused, 12 * e),
        "entropy_loss_fwd": (lambda: OPS.entropy_loss_fwd(x, loss), 4 * e),
        "entropy_loss_fwd/unfused": (loss_fwd_unfused, 4 * e),
        "entropy_loss_bwd": (lambda: OPS.entropy_loss_bwd(x, gl, dx, False), 8 * e),
        "entropy_loss_bwd/unfused": (loss_bwd_unfused, 8 * e),
    }
    times = {name: [] for name in kernels}
    for fn, _ in kernels.values():   # warm-up: code objects, clocks, the allocator's blocks
        _event_ms(fn, 10)
    for _ in range(args.rounds):
        for name, (fn, _) in kernels.items():
            times[name].append(_event_ms(fn, args.reps))
    lines = [f"{_lib.lib().adaptseg_version().decode()}; {n}x{c}x{h}x{w} logits = {rows} rows of {c}; HIP-event ms "
             f"per call over {args.reps} back-to-back calls, median (min .. max) of {args.rounds} alternating rounds"]
    res = {}
    for name, (_, nbytes) in kernels.items():
        med = statistics.median(times[name])
        res[name] = {"ms": med, "min_ms": min(times[name]), "max_ms": max(times[name])}
        lines.append(f"{name:26s} {med * 1e3:9.2f} us ({min(times[name]) * 1e3:.2f} .. {max(times[name]) * 1e3:.2f})"
                     f" = {nbytes / med / 1e6:.0f} GB/s of {nbytes} algorithmic bytes")
    ratios = {}
    for name in ("selfinfo_fwd", "selfinfo_bwd", "entropy_loss_fwd", "entropy_loss_bwd"):
        ratios[name] = res[name + "/unfused"]["ms"] / res[name]["ms"]
        lines.append(f"{name}: unfused / fused = {ratios[name]:.2f}x")
    print("\n".join(lines))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    print(json.dumps({"metric": "entropy-adaptation kernel times", "unit": "ms", "shape": [n, c, h, w],
                      "reps": args.reps, "rounds": args.rounds, "kernels": res, "unfused_over_fused": ratios}),
          flush=True)


if __name__ == "__main__":
    main()
