#!/usr/bin/env python3
"""Kernel times of the pseudo-label path (adaptsegnet_amd/pseudo.py) beside confusion_hist.

    python tools/bench_pseudo.py [--hw 1024x2048] [--classes 19] [--nbins 512] [--reps 2000] [--rounds 5]
                                 [--out FILE]

Times ``conf_hist``, ``pseudo_thresholds`` and ``pseudo_label`` (with the kept counts) on one
1 x 1024 x 2048 class map + confidence map, on two inputs: ``uniform`` (classes and confidences
drawn uniformly: almost every lane of a wave on its own bin) and ``road`` (every pixel class 0 with
confidence 1.0: every lane on ONE bin, what a real map's large confident regions look like).
``confusion_hist`` on the same number of pixels in the same process is the yardstick: the same
structure (per-block LDS bins, one 64-bit atomic per non-zero bin).  Each figure is HIP-event time
over ``--reps`` back-to-back launches after a warm-up, the median (min .. max) of ``--rounds`` rounds
that alternate between the kernels; GB/s are against the algorithmic bytes (maps read once, labels
written once).  Prints the lines and ONE JSON line; ``--out`` also writes the lines to a file.
"""
import argparse
import json
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
    ap.add_argument("--hw", type=lambda v: tuple(int(t) for t in v.split("x")), default=(1024, 2048))
    ap.add_argument("--classes", type=int, default=19)
    ap.add_argument("--nbins", type=int, default=512)
    ap.add_argument("--reps", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from adaptsegnet_amd import _lib
    from adaptsegnet_amd.ops import OPS
    dev = torch.device("cuda", 0)
    c, nbins = args.classes, args.nbins
    shape = (1,) + args.hw
    npix = shape[1] * shape[2]
    g = torch.Generator().manual_seed(5)
    inputs = {
        "uniform": (torch.randint(0, c, shape, generator=g, dtype=torch.uint8).to(dev),
                    torch.rand(shape, generator=g).to(dev)),
        "road": (torch.zeros(shape, dtype=torch.uint8, device=dev), torch.ones(shape, device=dev)),
    }
    gt = torch.randint(0, c, shape, generator=g, dtype=torch.uint8).to(dev)
    hist = torch.zeros((c, nbins), dtype=torch.int64, device=dev)
    cm = torch.zeros((c, c), dtype=torch.int64, device=dev)
    lut = torch.arange(256, dtype=torch.int32, device=dev)   # the identity label mapping
    thr = torch.empty(c, dtype=torch.float32, device=dev)
    labels = torch.empty(shape, dtype=torch.int64, device=dev)
    kept = torch.zeros(c, dtype=torch.int64, device=dev)
    kernels = {}
    for name, (pred, conf) in inputs.items():
        hist.zero_()
        OPS.conf_hist(pred, conf, c, nbins, hist)
        fixed = hist.clone()   # the thresholds of this input's own histogram
        kernels[f"conf_hist/{name}"] = (lambda p=pred, q=conf: OPS.conf_hist(p, q, c, nbins, hist), 5 * npix)
        kernels[f"pseudo_thresholds/{name}"] = (lambda h=fixed: OPS.pseudo_thresholds(h, 0.5, 0.9, thr), None)
        t = torch.empty(c, dtype=torch.float32, device=dev)
        OPS.pseudo_thresholds(fixed, 0.5, 0.9, t)
        kernels[f"pseudo_label/{name}"] = (lambda p=pred, q=conf, t=t: OPS.pseudo_label(p, q, t, 255, labels, kept),
                                           13 * npix)
        a = gt if name == "uniform" else pred   # road: every pixel on ONE bin of the confusion matrix too
        kernels[f"confusion_hist/{name}"] = (lambda a=a, p=pred: OPS.confusion_hist(a, lut, p, c, cm), 2 * npix)
    times = {k: [] for k in kernels}
    for fn, _ in kernels.values():   # warm-up: code objects, clocks
        _event_ms(fn, 50)
    for _ in range(args.rounds):
        for k, (fn, _) in kernels.items():
            times[k].append(_event_ms(fn, args.reps))
    lines = [f"{_lib.lib().adaptseg_version().decode()}; 1x{shape[1]}x{shape[2]} = {npix} pixels, {c} classes, "
             f"{nbins} bins; HIP-event ms per launch over {args.reps} launches, median (min .. max) of "
             f"{args.rounds} alternating rounds"]
    res = {}
    for k, (_, nbytes) in kernels.items():
        med = statistics.median(times[k])
        res[k] = {"ms": med, "min_ms": min(times[k]), "max_ms": max(times[k])}
        rate = "" if nbytes is None else f" = {nbytes / med / 1e6:.0f} GB/s of {nbytes} algorithmic bytes"
        lines.append(f"{k:28s} {med * 1e3:8.2f} us ({min(times[k]) * 1e3:.2f} .. {max(times[k]) * 1e3:.2f}){rate}")
    for name in inputs:
        r = res[f"conf_hist/{name}"]["ms"] / res[f"confusion_hist/{name}"]["ms"]
        lines.append(f"conf_hist / confusion_hist on '{name}': {r:.2f}x")
    lines.append(f"conf_hist road / uniform: {res['conf_hist/road']['ms'] / res['conf_hist/uniform']['ms']:.2f}x; "
                 f"confusion_hist road / uniform: "
                 f"{res['confusion_hist/road']['ms'] / res['confusion_hist/uniform']['ms']:.2f}x")
    print("\n".join(lines))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    print(json.dumps({"metric": "pseudo-label kernel times", "unit": "ms", "pixels": npix, "classes": c,
                      "nbins": nbins, "reps": args.reps, "rounds": args.rounds, "kernels": res}), flush=True)


if __name__ == "__main__":
    main()
