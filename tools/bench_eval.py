#!/usr/bin/env python3
"""Evaluation throughput: evaluate_cityscapes.py's per-image body.

    python tools/bench_eval.py [--batch 1] [--steps 10] [--warmup 2]
    python tools/bench_eval.py --scales 0.75,1.0 --mirror [--tta-out FILE]

One step = eval-mode DeeplabMulti forward on a 1024x512 image, interp of output2 to
1024x2048 + argmax (one fused kernel), and the confusion-matrix update against a uint8
label-id map (compute_iou.fast_hist).  Prints ONE JSON line; ``roofline`` is for the fused
upsample+argmax kernel (HBM-bound: algorithmic bytes = the 1/8-scale logits read once +
one byte per output pixel), timed with HIP events on its stream.  ``cpu_baseline`` = the
oracle (stock-PyTorch CPU fp32 eval forward + interp + argmax + numpy fast_hist) for 1 image.

``--scales`` (with or without ``--mirror``) adds ``tta`` to the JSON: multi-scale / mirrored
testing (evaluate.predict_tta).  The model's maps for the scaled (and flipped) inputs are fused
to the 1024x2048 class map (a) by the one fused kernel, with and without the confidence map:
achieved GB/s against algorithmic bytes = every map read once + 1 B per output pixel (+ 4 B with
the confidence), and (b) by the unfused composition of the package's own ops on the same maps in
the same process: flip, functional.interp, functional.softmax2d, add, then argmax.  ``--tta-out``
writes those two lines to a file.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
HBM_PEAK_GBS = 8000.0


def _event_ms(fn, reps, warmup=2):
    for _ in range(warmup):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def bench_tta(model, x, args, out_hw=(1024, 2048)):
    """The fused kernel against the unfused composition on the same maps (module docstring)."""
    from adaptsegnet_amd import functional as AF
    from adaptsegnet_amd.evaluate import fuse_argmax, predict_tta, tta_sizes
    model.eval()
    maps, mirrored = [], []
    with torch.no_grad():
        for hw in tta_sizes(x.shape[2:], args.scales):
            xi = x if hw == tuple(x.shape[2:]) else AF.interp(x, hw)
            for flip in (False, True) if args.mirror else (False,):
                maps.append(model(torch.flip(xi, dims=[3]) if flip else xi)[1].detach())
                mirrored.append(flip)

    def unfused():
        acc = None
        for m, mir in zip(maps, mirrored):
            p = AF.softmax2d(AF.interp(torch.flip(m, dims=[3]) if mir else m, out_hw))
            acc = p if acc is None else acc.add_(p)
        return acc.argmax(dim=1).to(torch.uint8)

    n, c = maps[0].shape[:2]
    npix = n * out_hw[0] * out_hw[1]
    map_bytes = sum(m.numel() * 4 for m in maps)
    fused_ms = _event_ms(lambda: fuse_argmax(maps, mirrored, out_hw), 20)
    conf_ms = _event_ms(lambda: fuse_argmax(maps, mirrored, out_hw, return_confidence=True), 20)
    unfused_ms = _event_ms(unfused, 5, warmup=1)
    agree = float((unfused() == fuse_argmax(maps, mirrored, out_hw)).float().mean())
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        predict_tta(model, x, args.scales, args.mirror, out_hw)
    torch.cuda.synchronize()
    tta_ms = (time.perf_counter() - t0) / args.steps * 1e3
    gbs, gbs_conf = (map_bytes + npix) / fused_ms / 1e6, (map_bytes + 5 * npix) / conf_ms / 1e6
    inter = len(maps) * npix * c * 4
    shape = f"S={len(maps)} maps {[tuple(m.shape[2:]) for m in maps]} x {c} classes -> {out_hw[0]}x{out_hw[1]}, batch {n}"
    lines = [
        f"fused   adaptseg_fuse_argmax, {shape}: {fused_ms:.3f} ms = {gbs:.1f} GB/s of {map_bytes + npix} algorithmic "
        f"bytes; with confidence {conf_ms:.3f} ms = {gbs_conf:.1f} GB/s of {map_bytes + 5 * npix} bytes "
        f"(HBM peak {HBM_PEAK_GBS:.0f} GB/s)",
        f"unfused flip + interp + softmax2d + add + argmax on the same maps, same process: {unfused_ms:.3f} ms "
        f"({inter} bytes of upsampled fp32 intermediates); fused is {unfused_ms / fused_ms:.2f}x "
        f"{'faster' if unfused_ms > fused_ms else 'SLOWER'}; class maps agree on {agree * 100:.4f} % of pixels",
    ]
    if args.tta_out:
        os.makedirs(os.path.dirname(os.path.abspath(args.tta_out)), exist_ok=True)
        with open(args.tta_out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return {"scales": list(args.scales), "mirror": bool(args.mirror), "maps": len(maps),
            "fused_ms": fused_ms, "fused_gbs": gbs, "fused_conf_ms": conf_ms, "fused_conf_gbs": gbs_conf,
            "unfused_ms": unfused_ms, "speedup": unfused_ms / fused_ms, "class_agreement": agree,
            "predict_tta_ms_per_step": tta_ms, "lines": lines}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--scales", type=lambda v: tuple(float(t) for t in v.split(",")), default=None,
                    help="comma-separated test scales: also measure the fused multi-scale kernel")
    ap.add_argument("--mirror", action="store_true", help="with --scales: add the mirrored input per scale")
    ap.add_argument("--tta-out", default=None, help="with --scales: write the fused / unfused lines here")
    args = ap.parse_args()
    from adaptsegnet_amd.evaluate import ConfusionMatrix, predict, upsample_argmax
    from adaptsegnet_amd.model import DeeplabMulti
    dev = torch.device("cuda", 0)
    torch.manual_seed(1338)
    model = DeeplabMulti(num_classes=19).to(dev)
    g = torch.Generator().manual_seed(5)
    x = (torch.rand(args.batch, 3, 512, 1024, generator=g) * 273.7 - 122.7).to(dev)
    gt = torch.randint(0, 34, (args.batch, 1024, 2048), generator=g, dtype=torch.uint8).to(dev)
    cm = ConfusionMatrix(19, device=dev)
    for _ in range(args.warmup):
        cm.update(gt, predict(model, x))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        cm.update(gt, predict(model, x))
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    # the fused kernel alone, on the model's 1/8-scale map (input-size upsample as model(image))
    logits = model(x)[1].detach()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    reps = 20
    e0.record()
    for _ in range(reps):
        upsample_argmax(logits, (1024, 2048))
    e1.record()
    torch.cuda.synchronize()
    k_ms = e0.elapsed_time(e1) / reps
    n, c, h, w = logits.shape
    alg_bytes = n * h * w * c * 4 + n * 1024 * 2048
    gbs = alg_bytes / (k_ms * 1e-3) / 1e9
    out = {"metric": "eval images/s (1024x512 -> 1024x2048 prediction + confusion update), DeeplabMulti",
           "value": args.batch * args.steps / dt, "unit": "images/s", "n_gpus": 1, "steps": args.steps,
           "warmup": args.warmup, "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True,
           "dtype": "f32", "data": "synthetic", "config": {"workload": "eval, batch %d" % args.batch},
           "miou_of_random_model": cm.miou(),
           "roofline": {"bound": "hbm", "kernel": "upsample_argmax_kernel", "achieved": gbs,
                        "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": gbs / HBM_PEAK_GBS,
                        "algorithmic_bytes_per_launch": alg_bytes, "avg_launch_ms": k_ms,
                        "traffic": None,
                        "note": "input-size logits (model(image) upsamples to 512x1024 first)"}}
    if args.scales:
        out["tta"] = bench_tta(model, x, args)
    if not args.no_cpu_baseline:
        from oracle import reference_eval as E
        from oracle import reference_torch as R
        threads = min(len(os.sched_getaffinity(0)), int(os.environ.get("OMP_NUM_THREADS", "64")))
        torch.set_num_threads(threads)
        G = R.to_torch(R.det_state(R.g_specs(), 1338), dtype=torch.float32)
        xc = x[:1].cpu()
        gtc = gt[:1].cpu().numpy()
        t0 = time.perf_counter()
        with torch.no_grad():
            _, p2 = R.g_forward(G, xc, (1024, 512), train=False)
            pred, _ = E.predict_argmax(p2.float(), (1024, 2048))
        from adaptsegnet_amd.evaluate import CITYSCAPES_TRAIN_IDS
        mapping = [(i, CITYSCAPES_TRAIN_IDS.get(i, 255)) for i in range(34)]
        E.fast_hist(E.label_mapping(gtc, mapping), pred.numpy(), 19)
        ct = time.perf_counter() - t0
        out["cpu_baseline"] = {"value": 1.0 / ct, "unit": "images/s", "cores": threads, "kind": "port",
                               "sample": f"1 image eval (oracle eval forward + interp + argmax + fast_hist); {ct:.2f} s"}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
