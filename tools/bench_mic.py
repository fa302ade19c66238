#!/usr/bin/env python3
"""Kernel times of masked image consistency's two launches (adaptsegnet_amd/mix.py: mask_patches) beside their
torch composition and the traffic floor.

    python tools/bench_mic.py [--shape 4x512x1024] [--patch 64] [--ratio 0.7] [--reps 50] [--rounds 5]
                              [--step-iters 0] [--out profiles/mic/bench_mic.json]

In one process, on one N x 3 x H x W target batch (the default is config c2's):

* ``conf_count`` and ``patch_mask``, each on its own and the two together (what ``mask_patches`` launches; with
  ClassMix's ``nconf`` passed in, ``patch_mask`` alone).
* ``torch``: the composition of the same result: the key compare, ``repeat_interleave`` of the patch mask to
  pixels, the multiply, ``.long()`` and the ``where`` of the labels, ``(conf >= tau).sum`` and the weight fill
  with its ignored rows.  Its keys are on the device already, which favours it.
* the floor: the bytes the two launches must move (4 per pixel for the count; 12 + 1 read and 12 + 8 + 4
  written per pixel for the mask, plus the keys) at the 6.29 TB/s a float4 copy reaches and at the 8.0 TB/s peak.

Each figure is HIP-event time over ``--reps`` back-to-back calls after a warm-up, the median (min .. max) of
``--rounds`` rounds that alternate between the candidates.  The default batch's working set (86 MB) is below
the 256 MB last-level cache, so back-to-back calls can exceed the HBM rates: the fraction of the floor is
against HBM all the same.  ``--step-iters K`` also times K single-level steps of DeeplabMulti at batch 1 with
and without ``lambda_mic`` (the branch costs one more generator forward and backward), alternating, after two
warm-up steps each.  Prints the lines and ONE JSON line; ``--out`` writes that JSON to a file.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

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


def _step_times(dev, iters, patch, ratio):
    """Median wall ms of a single-level DeeplabMulti step at batch 1, 1024 x 512, without and with lambda_mic."""
    from adaptsegnet_amd.mix import PatchMaskSampler, mask_patches
    from adaptsegnet_amd.model import DeeplabMulti, FCDiscriminator
    from adaptsegnet_amd.train import AdaptSegTrainer, StepConfig
    g = torch.Generator().manual_seed(9)
    x = (torch.randn(1, 3, 512, 1024, generator=g) * 50).to(dev)
    xt = (torch.randn(1, 3, 512, 1024, generator=g) * 50).to(dev)
    lab = torch.randint(0, 19, (1, 512, 1024), generator=g).to(dev)
    pred = torch.randint(0, 19, (1, 512, 1024), generator=g).to(torch.uint8).to(dev)
    conf = torch.rand(1, 512, 1024, generator=g).to(dev)
    sampler = PatchMaskSampler(seed=1, patch=patch, ratio=ratio)
    masked = mask_patches(xt, pred, conf, sampler.sample(1, 512, 1024), patch, ratio, tau=0.5, ignore_top=15,
                          ignore_bottom=120)
    out = {}
    runs = {}
    for name, lam in (("step", 0.0), ("step+mic", 1.0)):
        torch.manual_seed(3)
        m = DeeplabMulti(num_classes=19).to(dev).train()
        d2 = FCDiscriminator(num_classes=19).to(dev)
        tr = AdaptSegTrainer(m, None, d2, StepConfig(lambda_mic=lam))
        batch = (x, lab, xt) + (tuple(masked) if lam else ())
        runs[name] = (tr, batch, [])
    for it in range(2 + iters):
        for name, (tr, batch, ts) in runs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tr.step(it, [batch])
            torch.cuda.synchronize()
            if it >= 2:
                ts.append((time.perf_counter() - t0) * 1e3)
    for name, (_, _, ts) in runs.items():
        out[name] = {"ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "iters": len(ts)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=lambda v: tuple(int(t) for t in v.split("x")), default=(4, 512, 1024))
    ap.add_argument("--patch", type=int, default=64)
    ap.add_argument("--ratio", type=float, default=0.7)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--step-iters", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from adaptsegnet_amd import _lib
    from adaptsegnet_amd.mix import PatchMaskSampler
    from adaptsegnet_amd.ops import OPS
    dev = torch.device("cuda", 0)
    n, h, w = args.shape
    patch, tau, top, bottom = args.patch, 0.968, 15, 120
    npix = n * h * w
    g = torch.Generator().manual_seed(5)
    rng = np.random.Generator(np.random.PCG64(7))
    xt = torch.randn(n, 3, h, w, generator=g).to(dev)
    pred = torch.from_numpy(rng.integers(0, 19, (n, h, w)).astype(np.uint8)).to(dev)
    conf = torch.rand(n, h, w, generator=g).to(dev)
    sampler = PatchMaskSampler(seed=3, patch=patch, ratio=args.ratio)
    keys = torch.from_numpy(sampler.sample(n, h, w).view(np.int32)).to(dev)
    threshold = sampler.threshold
    nconf = torch.empty(n, dtype=torch.int32, device=dev)
    mi = torch.empty_like(xt)
    ml = torch.empty(n, h, w, dtype=torch.int64, device=dev)
    mw = torch.empty_like(conf)

    def count():
        OPS.conf_count(conf, tau, nconf)

    def mask():
        OPS.patch_mask(xt, pred, nconf, keys, patch, threshold, 19, 255, top, bottom, mi, ml, mw)

    def both():
        count()
        mask()

    keys64 = keys.to(torch.int64) & 0xFFFFFFFF     # torch has no compare on uint32: the composition's keys, widened

    def composed():
        keep = (keys64 >= threshold).repeat_interleave(patch, 1).repeat_interleave(patch, 2)[:, :h, :w]
        images = xt * keep[:, None]
        p = pred.long()
        labels = torch.where(p < 19, p, torch.full_like(p, 255))
        q = (conf >= tau).sum(dim=(1, 2)).float() / float(h * w)
        weights = q[:, None, None].expand(n, h, w).clone()
        weights[:, :top] = 0
        weights[:, h - bottom:] = 0
        return images, labels, weights

    # the two paths give one result; compared by value: the multiply leaves -0 where it blanks a negative pixel
    both()
    ti, tl, tw = composed()
    torch.cuda.synchronize()
    if not (torch.equal(ti, mi) and torch.equal(tl, ml) and torch.equal(tw, mw)):
        raise RuntimeError("bench_mic: the torch composition and the kernels disagree")

    nkeys = keys.numel()
    nbytes = {"conf_count": 4 * npix, "patch_mask": 37 * npix + 4 * nkeys + 4 * n}
    nbytes["conf_count+patch_mask"] = nbytes["conf_count"] + nbytes["patch_mask"]
    nbytes["torch"] = nbytes["conf_count+patch_mask"]
    kernels = {"conf_count": count, "patch_mask": mask, "conf_count+patch_mask": both, "torch": composed}
    times = {name: [] for name in kernels}
    for fn in kernels.values():   # warm-up: code objects, clocks, the allocator's blocks
        _event_ms(fn, 5)
    for _ in range(args.rounds):
        for name, fn in kernels.items():
            times[name].append(_event_ms(fn, args.reps))
    lines = [f"{_lib.lib().adaptseg_version().decode()}; {n}x3x{h}x{w} = {npix} pixels, patch {patch}, ratio "
             f"{args.ratio}, {nkeys} keys; HIP-event ms per call over {args.reps} back-to-back calls, median "
             f"(min .. max) of {args.rounds} alternating rounds"]
    res = {}
    for name in kernels:
        med = statistics.median(times[name])
        rate = nbytes[name] / (med * 1e-3)
        floor_ms = nbytes[name] / HBM_COPY * 1e3
        res[name] = {"ms": med, "min_ms": min(times[name]), "max_ms": max(times[name]), "bytes": nbytes[name],
                     "gb_per_s": rate / 1e9, "floor_ms_copy": floor_ms, "floor_ms_peak": nbytes[name] / HBM_PEAK * 1e3,
                     "fraction_of_floor": floor_ms / med, "hbm_peak_share": rate / HBM_PEAK}
        lines.append(f"{name:24s} {med * 1e3:9.2f} us ({min(times[name]) * 1e3:.2f} .. {max(times[name]) * 1e3:.2f}) = "
                     f"{rate / 1e9:.0f} GB/s of {nbytes[name]} bytes; floor {floor_ms * 1e3:.2f} us at 6.29 TB/s: "
                     f"{floor_ms / med:.2f} of it ({100 * rate / HBM_PEAK:.1f} % of 8.0 TB/s)")
    ratio = res["torch"]["ms"] / res["conf_count+patch_mask"]["ms"]
    lines.append(f"torch / (conf_count + patch_mask) = {ratio:.2f}x")
    out = {"metric": "MIC masking kernel times", "unit": "ms", "shape": [n, 3, h, w], "patch": patch,
           "ratio": args.ratio, "reps": args.reps, "rounds": args.rounds, "kernels": res, "torch_over_kernels": ratio}
    if args.step_iters > 0:
        steps = _step_times(dev, args.step_iters, patch, args.ratio)
        out["step"] = steps
        for name, v in steps.items():
            lines.append(f"{name:24s} {v['ms']:9.2f} ms ({v['min_ms']:.2f} .. {v['max_ms']:.2f}), wall, median of "
                         f"{v['iters']} single-level DeeplabMulti steps at batch 1, 1024 x 512")
        lines.append(f"step+mic / step = {steps['step+mic']['ms'] / steps['step']['ms']:.3f}x")
    print("\n".join(lines))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
