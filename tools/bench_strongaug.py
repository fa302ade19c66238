#!/usr/bin/env python3
"""Kernel time of ``strong_augment`` (adaptsegnet_amd/mix.py) beside a torch composition of the same transform.

    python tools/bench_strongaug.py [--shape 4x3x512x1024] [--radius 4] [--reps 50] [--rounds 5] [--out FILE]

In one process, on one N x 3 x H x W batch (the default is config c2's), three settings of every image:
jitter only, blur only (radius ``--radius``) and both.  The torch composition is what a user would write:
denormalise, brightness / contrast as elementwise ops, saturation and hue through an rgb -> hsv -> rgb round
trip each (``torch.where`` chains), renormalise, then ``F.pad(mode="reflect")`` and a depthwise ``F.conv2d`` per
axis.  It is timed, not compared: its roundings differ from the kernel's.

Each figure is HIP-event time over ``--reps`` back-to-back calls after a warm-up, the median (min .. max) of
``--rounds`` rounds that alternate between the candidates.  GB/s are against the algorithmic 24 bytes per
pixel (three floats read, three written), and the share of HBM bandwidth is that rate over the 8.0 TB/s peak
and over the 6.29 TB/s a float4 copy reaches; a working set below the 256 MB last-level cache can exceed
either.  The kernel's figure is the launch alone (the tables are uploaded once, outside the timed loop).
Prints the lines and ONE JSON line; ``--out`` also writes the lines to a file.
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


def _rgb_to_hsv(r, g, b):
    mx, mn = torch.maximum(torch.maximum(r, g), b), torch.minimum(torch.minimum(r, g), b)
    d = mx - mn
    s = torch.where(mx > 0, d / mx.clamp_min(1e-12), torch.zeros_like(mx))
    dd = torch.where(d == 0, torch.ones_like(d), d)
    h6 = torch.where(mx == r, (g - b) / dd, torch.where(mx == g, 2 + (b - r) / dd, 4 + (r - g) / dd))
    h6 = torch.where(d == 0, torch.zeros_like(h6), h6)
    return torch.remainder(h6 / 6, 1.0), s, mx


def _hsv_to_rgb(h, s, v):
    h6 = h * 6
    i = torch.floor(h6)
    f = h6 - i
    i = torch.remainder(i, 6)
    p, q, t = v * (1 - s), v * (1 - s * f), v * (1 - s * (1 - f))
    sel = [i == k for k in range(5)]

    def pick(*c):
        out = c[5]
        for k in range(4, -1, -1):
            out = torch.where(sel[k], c[k], out)
        return out
    return pick(v, q, p, p, t, v), pick(t, v, v, q, p, p), pick(p, p, t, v, v, q)


def torch_strong_augment(x, mean, db, fc, fs, fh, kernel, radius, jitter, blur):
    """x [N, 3, H, W] BGR minus mean; db .. fh [N, 1, 1]; kernel [N, 2 R + 1]: the composition, per image."""
    if jitter:
        u = (x + mean) / 255
        r, g, b = u[:, 2], u[:, 1], u[:, 0]
        r, g, b = ((c + db).clamp(0, 1) for c in (r, g, b))
        r, g, b = ((c * fc).clamp(0, 1) for c in (r, g, b))
        h, s, v = _rgb_to_hsv(r, g, b)
        r, g, b = _hsv_to_rgb(h, (s * fs).clamp(0, 1), v)
        h, s, v = _rgb_to_hsv(r, g, b)
        r, g, b = _hsv_to_rgb(torch.remainder(h + fh, 1.0), s, v)
        x = torch.stack((b, g, r), dim=1) * 255 - mean
    if blur:
        n, c, hh, ww = x.shape
        k = kernel.repeat_interleave(3, 0)   # one filter per image and channel
        y = F.pad(x.reshape(1, n * c, hh, ww), (radius, radius, 0, 0), mode="reflect")
        y = F.conv2d(y, k[:, None, None, :], groups=n * c)
        y = F.pad(y, (0, 0, radius, radius), mode="reflect")
        x = F.conv2d(y, k[:, None, :, None], groups=n * c).reshape(n, c, hh, ww)
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=lambda v: tuple(int(t) for t in v.split("x")), default=(4, 3, 512, 1024))
    ap.add_argument("--radius", type=int, default=4)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from adaptsegnet_amd import _lib, mix
    from adaptsegnet_amd.data import IMG_MEAN
    from adaptsegnet_amd.ops import OPS
    dev = torch.device("cuda", 0)
    n, c, h, w = args.shape
    assert c == 3, "images have three channels"
    npix = n * h * w
    rng = np.random.Generator(np.random.PCG64(5))
    x = torch.from_numpy(rng.integers(0, 256, (n, 3, h, w)).astype(np.float32)
                         - IMG_MEAN[None, :, None, None]).to(dev)
    out = torch.empty_like(x)
    mean_l = [float(v) for v in IMG_MEAN]
    mean_t = torch.from_numpy(IMG_MEAN).to(dev)[None, :, None, None]
    base = mix.StrongAugSampler(seed=3, p_jitter=1.0, p_blur=1.0).sample(n, h, w)
    sigma = 0.25 * args.radius   # a radius-R kernel whose last tap still matters
    base["radius"] = np.full(n, args.radius, dtype=np.int32)
    base["weights"] = np.stack([mix.blur_weights(sigma, args.radius)] * n)
    half = base["weights"][:, :args.radius + 1]
    kernel = torch.from_numpy(np.concatenate([half[:, :0:-1], half], axis=1).copy()).to(dev)
    fac = {k: torch.from_numpy(base[k]).to(dev)[:, None, None] for k in ("db", "fc", "fs", "fh")}

    kernels = {}
    for name, jitter, blur in (("jitter", True, False), ("blur", False, True), ("both", True, True)):
        p = dict(base)
        p["jitter"] = np.full(n, jitter)
        if not blur:
            p["radius"] = np.zeros(n, dtype=np.int32)
            p["weights"] = np.stack([mix.blur_weights(1.0, 0)] * n)
        ctl, table = mix._aug_tables(p, n, h, w)
        table = torch.from_numpy(table).to(dev)
        kernels[name] = (lambda ctl=ctl, table=table: OPS.strong_augment(x, mean_l, ctl, table, out), 24 * npix)
        kernels[name + "/torch"] = (lambda jitter=jitter, blur=blur: torch_strong_augment(
            x, mean_t, fac["db"], fac["fc"], fac["fs"], fac["fh"], kernel, args.radius, jitter, blur), 24 * npix)
    times = {name: [] for name in kernels}
    for fn, _ in kernels.values():   # warm-up: code objects, clocks, the allocator's blocks
        _event_ms(fn, 5)
    for _ in range(args.rounds):
        for name, (fn, _) in kernels.items():
            times[name].append(_event_ms(fn, args.reps))
    lines = [f"{_lib.lib().adaptseg_version().decode()}; {n}x3x{h}x{w} = {npix} pixels, blur radius {args.radius}; "
             f"HIP-event ms per call over {args.reps} back-to-back calls, median (min .. max) of {args.rounds} "
             "alternating rounds"]
    res = {}
    for name, (_, nbytes) in kernels.items():
        med = statistics.median(times[name])
        rate = nbytes / (med * 1e-3)
        res[name] = {"ms": med, "min_ms": min(times[name]), "max_ms": max(times[name]), "bytes": nbytes,
                     "hbm_peak_share": rate / HBM_PEAK, "hbm_copy_share": rate / HBM_COPY}
        lines.append(f"{name:14s} {med * 1e3:10.2f} us ({min(times[name]) * 1e3:.2f} .. {max(times[name]) * 1e3:.2f})"
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
    print(json.dumps({"metric": "strong_augment kernel times", "unit": "ms", "shape": [n, 3, h, w],
                      "radius": args.radius, "reps": args.reps, "rounds": args.rounds, "kernels": res,
                      "torch_over_kernel": ratios}), flush=True)


if __name__ == "__main__":
    main()
