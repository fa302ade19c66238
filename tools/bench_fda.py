#!/usr/bin/env python3
"""Kernel time of ``fda_source_to_target`` (adaptsegnet_amd/fda.py) beside a ``torch.fft`` composition of FDA.

    python tools/bench_fda.py [--shape 4x3x512x1024] [--betas 0.01,0.05,0.09] [--reps 50] [--rounds 5] [--out FILE]

In one process, on one N x C x H x W pair of batches (the default is config c2's), for every beta: the four
launches of the transfer, and the published route on the device as a user would write it -- ``fft2`` of both
batches, ``abs`` / ``angle``, the window copied between the shifted amplitude spectra, ``polar``, ``ifft2``, the
real part.  If torch's FFT does not run on the machine the kernel is reported alone.  The composition is timed
and its distance to the kernel's result printed; it is not the reference (tests/fda_ref.py is).

Each figure is HIP-event time over ``--reps`` back-to-back calls after a warm-up, the median (min .. max) of
``--rounds`` rounds that alternate between the candidates.  The compulsory-traffic floor is src, trg and out
moved once each (12 bytes per pixel and channel) at the 6.29 TB/s a float4 copy reaches; ``floor_share`` is that
time over the kernel's (1.0 = at the floor).  A working set below the 256 MB last-level cache can beat HBM rates.
The kernel's figure includes the op's workspace lookup; the twiddle tables are made once, outside the timed loop.
Prints the lines and ONE JSON line; ``--out`` also writes the lines to a file.
"""
import argparse
import json
import os
import statistics
import sys

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


def torch_fda(src, trg, b, mean):
    """The published route with torch.fft: src, trg [N, C, H, W] minus mean [1, C, 1, 1]."""
    fs, ft = torch.fft.fft2(src + mean), torch.fft.fft2(trg + mean)
    a_s = torch.fft.fftshift(fs.abs(), dim=(-2, -1))
    a_t = torch.fft.fftshift(ft.abs(), dim=(-2, -1))
    h, w = src.shape[-2:]
    ch, cw = h // 2, w // 2
    a_s[..., ch - b:ch + b + 1, cw - b:cw + b + 1] = a_t[..., ch - b:ch + b + 1, cw - b:cw + b + 1]
    a_s = torch.fft.ifftshift(a_s, dim=(-2, -1))
    return torch.fft.ifft2(torch.polar(a_s, fs.angle())).real - mean


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=lambda v: tuple(int(t) for t in v.split("x")), default=(4, 3, 512, 1024))
    ap.add_argument("--betas", type=lambda v: tuple(float(t) for t in v.split(",")), default=(0.01, 0.05, 0.09))
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from adaptsegnet_amd import _lib
    from adaptsegnet_amd.data import IMG_MEAN
    from adaptsegnet_amd.fda import fda_band, fda_source_to_target
    dev = torch.device("cuda", 0)
    n, c, h, w = args.shape
    mean = IMG_MEAN if c == 3 else None
    mean_np = np.zeros(c, np.float32) if mean is None else IMG_MEAN
    rng = np.random.Generator(np.random.PCG64(5))
    src = torch.from_numpy(rng.integers(0, 256, (n, c, h, w)).astype(np.float32) * 0.7 + 30
                           - mean_np[None, :, None, None]).to(dev)
    trg = torch.from_numpy(rng.integers(0, 256, (n, c, h, w)).astype(np.float32) * 0.5 + 90
                           - mean_np[None, :, None, None]).to(dev)
    mean_t = torch.from_numpy(mean_np).to(dev)[None, :, None, None]
    nbytes = 12 * n * c * h * w
    floor_ms = nbytes / HBM_COPY * 1e3

    fft_ok, fft_why = True, ""
    try:
        torch_fda(src, trg, 1, mean_t)
        torch.cuda.synchronize()
    except Exception as e:  # noqa: BLE001 - whatever keeps the FFT library from running: report the kernel alone
        fft_ok, fft_why = False, f"{type(e).__name__}: {str(e).splitlines()[0][:120]}"

    cands, dist = {}, {}
    for beta in args.betas:
        b = fda_band(h, w, beta)
        cands[f"beta={beta:g}"] = (lambda beta=beta: fda_source_to_target(src, trg, beta, mean=mean), b)
        if fft_ok:
            cands[f"beta={beta:g}/torch.fft"] = (lambda b=b: torch_fda(src, trg, b, mean_t), b)
            dist[f"beta={beta:g}"] = float((fda_source_to_target(src, trg, beta, mean=mean)
                                            - torch_fda(src, trg, b, mean_t)).abs().max())
    times = {name: [] for name in cands}
    for fn, _ in cands.values():   # warm-up: code objects, clocks, the allocator's blocks, the FFT plans
        _event_ms(fn, 5)
    for _ in range(args.rounds):
        for name, (fn, _) in cands.items():
            times[name].append(_event_ms(fn, args.reps))
    lines = [f"{_lib.lib().adaptseg_version().decode()}; {n}x{c}x{h}x{w}; HIP-event ms per call over {args.reps} "
             f"back-to-back calls, median (min .. max) of {args.rounds} alternating rounds; compulsory traffic "
             f"{nbytes} bytes = {floor_ms * 1e3:.2f} us at 6.29 TB/s"]
    if not fft_ok:
        lines.append(f"torch.fft does not run here ({fft_why}): the kernel alone")
    res = {}
    for name, (_, b) in cands.items():
        med = statistics.median(times[name])
        res[name] = {"ms": med, "min_ms": min(times[name]), "max_ms": max(times[name]), "b": b,
                     "floor_share": floor_ms / med}
        lines.append(f"{name:22s} b={b:3d} {med * 1e3:10.2f} us ({min(times[name]) * 1e3:.2f} .. "
                     f"{max(times[name]) * 1e3:.2f}) = {100 * floor_ms / med:.1f} % of the traffic floor")
    ratios = {}
    for name in cands:
        if "/" in name:
            k = name.split("/")[0]
            ratios[name] = res[name]["ms"] / res[k]["ms"]
            lines.append(f"{name} / kernel = {ratios[name]:.2f}x; max |kernel - torch.fft| = {dist[k]:.3e}")
    print("\n".join(lines))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    print(json.dumps({"metric": "fda_source_to_target kernel times", "unit": "ms", "shape": [n, c, h, w],
                      "reps": args.reps, "rounds": args.rounds, "floor_bytes": nbytes, "floor_ms": floor_ms,
                      "torch_fft": fft_ok, "kernels": res, "torch_over_kernel": ratios}), flush=True)


if __name__ == "__main__":
    main()
