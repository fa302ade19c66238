#!/usr/bin/env python3
"""Kernel times of online self-training's ops (adaptsegnet_amd/mix.py) beside their torch compositions.

    python tools/bench_classmix.py [--shape 4x19x512x1024] [--ema-n 44500000] [--reps 50] [--rounds 5] [--out FILE]

In one process, on one N x C x H x W problem (the default is config c2's batch) and one arena of
``--ema-n`` floats (DeeplabMulti's is 44.5 M):

* ``ema``: one launch over the arena, beside ``p.mul_(a).add_(s, alpha=1-a)`` over the arena cut into
  314 tensors (what a per-parameter loop does) and beside ``torch._foreach_mul_ / _foreach_add_``;
  ``ema_multi``: 416 small tensors (BatchNorm statistics and frozen affines) in 4 launches, beside the loop.
* ``classmix``: ``classmix_stats`` + ``classmix_apply``, beside the composition ``torch.unique`` /
  ``randperm`` per image (a host sync each), ``isin`` and three ``torch.where``.
* ``ce_pw``: ``softmax_ce_pw_fwd`` + ``softmax_ce_pw_bwd``, beside autograd over
  ``(F.cross_entropy(reduction='none') * w).sum() / valid`` on the same channels-last logits.

Each figure is HIP-event time over ``--reps`` back-to-back calls after a warm-up, the median (min .. max)
of ``--rounds`` rounds that alternate between the candidates.  GB/s are against the algorithmic bytes
(ema 12 n; stats 12, apply 57 per pixel; CE forward 4 C + 12, backward 8 C + 12 per pixel), and the
share of HBM bandwidth is that rate over the 8.0 TB/s peak and over the 6.29 TB/s a float4 copy reaches.
A working set below the 256 MB last-level cache can exceed either.  Prints the lines and ONE JSON line;
``--out`` also writes the lines to a file.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

HBM_PEAK, HBM_COPY = 8.0e12, 6.29e12   # bytes/s: the spec peak, a measured float4 copy


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
    ap.add_argument("--ema-n", type=int, default=44_500_000)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from adaptsegnet_amd import _lib
    from adaptsegnet_amd.mix import ClassMixSampler
    from adaptsegnet_amd.ops import OPS
    dev = torch.device("cuda", 0)
    n, c, h, w = args.shape
    npix = n * h * w
    g = torch.Generator().manual_seed(5)
    a = 0.99

    # ---- EMA -----------------------------------------------------------------------------------------
    en = args.ema_n
    dst, src = torch.randn(en, generator=g).to(dev), torch.randn(en, generator=g).to(dev)
    cuts = np.linspace(0, en, 315).astype(np.int64)
    dparts = [dst[int(i):int(j)] for i, j in zip(cuts[:-1], cuts[1:])]
    sparts = [src[int(i):int(j)] for i, j in zip(cuts[:-1], cuts[1:])]

    def ema_torch_loop():
        for d, s in zip(dparts, sparts):
            d.mul_(a).add_(s, alpha=1 - a)

    def ema_torch_foreach():
        torch._foreach_mul_(dparts, a)
        torch._foreach_add_(dparts, sparts, alpha=1 - a)

    small = [64, 128, 256, 512, 1024, 2048]
    sdst = [torch.randn(small[i % len(small)], generator=g).to(dev) for i in range(416)]
    ssrc = [torch.randn(t.numel(), generator=g).to(dev) for t in sdst]
    small_n = sum(t.numel() for t in sdst)

    def ema_multi_torch_loop():
        for d, s in zip(sdst, ssrc):
            d.mul_(a).add_(s, alpha=1 - a)

    # ---- ClassMix ------------------------------------------------------------------------------------
    rng = np.random.Generator(np.random.PCG64(7))
    xs = torch.randn(n, 3, h, w, generator=g).to(dev)
    xt = torch.randn(n, 3, h, w, generator=g).to(dev)
    # label maps in blocks of 32 x 32 pixels of one class (segmentation labels are piecewise constant)
    coarse = torch.from_numpy(rng.integers(0, c, (n, (h + 31) // 32, (w + 31) // 32)))
    lab = coarse.repeat_interleave(32, 1).repeat_interleave(32, 2)[:, :h, :w].contiguous()
    lab[torch.rand(n, h, w, generator=g) < 0.05] = 255
    lab = lab.to(dev)
    pred = torch.from_numpy(rng.integers(0, c, (n, h, w)).astype(np.uint8)).to(dev)
    conf = torch.rand(n, h, w, generator=g).to(dev)
    keys = torch.from_numpy(ClassMixSampler(3).sample(n, c).view(np.int32)).to(dev)
    count = torch.empty(n, c, dtype=torch.int32, device=dev)
    nconf = torch.empty(n, dtype=torch.int32, device=dev)
    mi, ml, mw = torch.empty_like(xs), torch.empty_like(lab), torch.empty_like(conf)
    tau = 0.968

    def classmix_kernels():
        OPS.classmix_stats(lab, conf, tau, c, count, nconf)
        OPS.classmix_apply(xs, lab, xt, pred, count, nconf, keys, 255, mi, ml, mw, None)

    def classmix_torch():
        masks = []
        for i in range(n):
            classes = torch.unique(lab[i])
            classes = classes[classes != 255]
            pick = classes[torch.randperm(classes.numel(), device=dev)[:(classes.numel() + 1) // 2]]
            masks.append(torch.isin(lab[i], pick))
        m = torch.stack(masks)
        q = (conf >= tau).float().mean(dim=(1, 2), keepdim=True)
        return (torch.where(m[:, None], xs, xt), torch.where(m, lab, pred.long()),
                torch.where(m, torch.ones_like(conf), q.expand_as(conf)))

    # ---- pixel-weighted CE ---------------------------------------------------------------------------
    logits = (torch.randn(n, h, w, c, generator=g) * 3).to(dev)   # NHWC: the channels-last prediction
    out2, gl = torch.empty(2, device=dev), torch.ones(1, device=dev)
    dl = torch.empty_like(logits)
    classmix_kernels()
    leaf = logits.permute(0, 3, 1, 2).detach().requires_grad_(True)   # NCHW-shaped, channels_last

    def ce_kernels():
        OPS.softmax_ce_pw_fwd(logits, ml, 255, None, mw, out2)
        OPS.softmax_ce_pw_bwd(logits, ml, out2, gl, 255, None, mw, dl, False)

    def ce_torch():
        leaf.grad = None
        nll = F.cross_entropy(leaf, ml, ignore_index=255, reduction="none")
        ((nll * mw).sum() / (ml != 255).sum()).backward()

    kernels = {
        "ema": (lambda: OPS.ema(src, dst, a), 12 * en),
        "ema/torch-loop-314": (ema_torch_loop, 12 * en),
        "ema/torch-foreach": (ema_torch_foreach, 12 * en),
        "ema_multi": (lambda: OPS.ema_multi(ssrc, sdst, a), 12 * small_n),
        "ema_multi/torch-loop-416": (ema_multi_torch_loop, 12 * small_n),
        "classmix": (classmix_kernels, (12 + 57) * npix),
        "classmix/torch": (classmix_torch, (12 + 57) * npix),
        "ce_pw": (ce_kernels, (12 * c + 24) * npix),
        "ce_pw/torch": (ce_torch, (12 * c + 24) * npix),
    }
    times = {name: [] for name in kernels}
    for fn, _ in kernels.values():   # warm-up: code objects, clocks, the allocator's blocks
        _event_ms(fn, 5)
    for _ in range(args.rounds):
        for name, (fn, _) in kernels.items():
            times[name].append(_event_ms(fn, args.reps))
    lines = [f"{_lib.lib().adaptseg_version().decode()}; {n}x{c}x{h}x{w} = {npix} pixels, EMA arena of {en} floats; "
             f"HIP-event ms per call over {args.reps} back-to-back calls, median (min .. max) of {args.rounds} "
             "alternating rounds"]
    res = {}
    for name, (_, nbytes) in kernels.items():
        med = statistics.median(times[name])
        rate = nbytes / (med * 1e-3)
        res[name] = {"ms": med, "min_ms": min(times[name]), "max_ms": max(times[name]), "bytes": nbytes,
                     "hbm_peak_share": rate / HBM_PEAK, "hbm_copy_share": rate / HBM_COPY}
        lines.append(f"{name:26s} {med * 1e3:10.2f} us ({min(times[name]) * 1e3:.2f} .. {max(times[name]) * 1e3:.2f})"
                     f" = {rate / 1e9:.0f} GB/s of {nbytes} algorithmic bytes = {100 * rate / HBM_PEAK:.1f} % of "
                     f"8.0 TB/s ({100 * rate / HBM_COPY:.1f} % of a 6.29 TB/s copy)")
    ratios = {}
    for name in kernels:
        if "/" in name:
            ratios[name] = res[name]["ms"] / res[name.split("/")[0]]["ms"]
            lines.append(f"{name} / {name.split('/')[0]} = {ratios[name]:.2f}x")
    print("\n".join(lines))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    print(json.dumps({"metric": "online self-training kernel times", "unit": "ms", "shape": [n, c, h, w],
                      "ema_n": en, "reps": args.reps, "rounds": args.rounds, "kernels": res,
                      "torch_over_kernel": ratios}), flush=True)


if __name__ == "__main__":
    main()
