#!/usr/bin/env python3
"""Times of rare class sampling's two kernels (adaptsegnet_amd/rcs.py) beside the composition the crop count
replaces and a traffic floor.

    python tools/bench_rcs.py [--shape 4x1052x1914] [--crop 1024x512] [--tries 10] [--reps 50] [--rounds 5]
                              [--out profiles/rcs/bench_rcs.json]

In one process, on one decoded label batch (the default is the workload's: GTA5 label files, the c2 crop, ten
candidates per sample drawn by ``AugmentSampler`` with its default scales and a fixed seed):

* ``crop_class_count``: the op alone (its parameters a prepared list, its output allocated once) and the Python
  surface ``rcs.crop_class_count`` (which also checks and flattens the candidates and allocates the output).
* ``composition``: what it replaces, ``tries`` calls of ``data.preprocess_augmented`` on the images and labels,
  each followed by ``(labels == c).sum((1, 2))``: ten Pillow-exact bicubic resizes to learn ten counts.
* ``label_class_count``: the op alone.
* ``copy``: a device-to-device copy of 512 MiB, the rate the floors are taken against (bytes read + written).

The floor of the crop count is one read of the label rows that at least one candidate reads (found here by the
same sequential nearest walk), the floor of the class count one read of the labels.  Each figure is HIP-event
time per call over ``--reps`` back-to-back calls after a warm-up, the median (min .. max) of ``--rounds`` rounds
that alternate between the candidates.  Calls this short are bounded by the host's launch rate as much as by the
device (the crop count is two launches, the composition 4 * tries + tries), and the 8 MB label batch stays in the
last-level cache between calls: the fraction of the floor is against the measured copy rate all the same.
Prints the lines and ONE JSON line; ``--out`` writes that JSON to a file.
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


def _event_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def _rows_read(in_h, ch, cand):
    """Per sample the number of source rows that at least one candidate's window reads."""
    out = []
    for sample in cand:
        read = np.zeros(in_h, bool)
        for sw, sh, ox, oy, mirror in sample:
            scale = np.float64(in_h) / np.float64(sh)
            v = np.float64(0.5) * scale
            for o in range(int(sh)):
                if 0 <= o - oy < ch:
                    read[min(int(v), in_h - 1)] = True
                v = v + scale
        out.append(int(read.sum()))
    return out


def _dims(v):
    return tuple(int(t) for t in v.split("x"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=_dims, default=(4, 1052, 1914))
    ap.add_argument("--crop", type=_dims, default=(1024, 512), help="WxH")
    ap.add_argument("--tries", type=int, default=10)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from adaptsegnet_amd import _lib, data, rcs
    from adaptsegnet_amd.ops import OPS
    dev = torch.device("cuda", 0)
    n, h, w = args.shape
    cw, ch = args.crop
    K = args.tries
    rng = np.random.Generator(np.random.PCG64(7))
    pool = np.array(sorted(data.ID_TO_TRAINID) + [0, 1, 4, 6], np.uint8)
    coarse = pool[rng.integers(len(pool), size=(n, (h + 15) // 16, (w + 23) // 24))]
    ids = np.ascontiguousarray(np.repeat(np.repeat(coarse, 16, axis=1), 24, axis=2)[:, :h, :w])
    labels = torch.from_numpy(ids).to(dev)
    images = torch.from_numpy(rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)).to(dev)
    lut = data.trainid_lut(dev)
    cand = data.AugmentSampler((cw, ch), seed=7).sample(n * K).reshape(n, K, 5)
    classes_host = [13, 0, 5, 11, 2, 8, 1, 10][:n] if n <= 8 else [int(c) for c in rng.integers(0, 19, n)]
    classes = torch.tensor(classes_host, dtype=torch.int32, device=dev)
    flat = cand.reshape(-1).tolist()
    counts = torch.empty((n, K), dtype=torch.int64, device=dev)
    stats = torch.empty((n, 19), dtype=torch.int64, device=dev)
    cls_b = classes.to(torch.int64).view(-1, 1, 1)
    big_src = torch.empty(512 << 20, dtype=torch.uint8, device=dev).random_(0, 256)
    big_dst = torch.empty_like(big_src)

    def crop_op():
        OPS.crop_class_count(labels, lut, classes, flat, ch, cw, counts)

    def crop_py():
        return rcs.crop_class_count(labels, classes, cand, (cw, ch), lut)

    def composed():
        cols = []
        for k in range(K):
            win = data.preprocess_augmented(images, labels, (cw, ch), cand[:, k], lut=lut)[1]
            cols.append((win == cls_b).sum((1, 2)))
        return torch.stack(cols, dim=1)

    def count_op():
        OPS.label_class_count(labels, lut, 19, stats)

    def copy():
        big_dst.copy_(big_src)

    crop_op()
    want = composed()
    torch.cuda.synchronize()
    if not (torch.equal(counts, want) and torch.equal(crop_py(), want)):
        raise RuntimeError("bench_rcs: the crop count and the composition disagree")
    count_op()
    tl = lut.to(torch.int64)[labels.to(torch.int64)]
    if not torch.equal(stats, torch.stack([(tl == c).sum((1, 2)) for c in range(19)], dim=1)):
        raise RuntimeError("bench_rcs: the class count and torch disagree")

    rows = _rows_read(h, ch, cand)
    nbytes = {"crop_class_count": sum(rows) * w, "label_class_count": n * h * w, "copy": 2 * big_src.numel()}
    nbytes["crop_class_count (python surface)"] = nbytes["composition"] = nbytes["crop_class_count"]
    kernels = {"crop_class_count": crop_op, "crop_class_count (python surface)": crop_py, "composition": composed,
               "label_class_count": count_op, "copy": copy}
    reps = {name: args.reps if name != "copy" else max(4, args.reps // 5) for name in kernels}
    times = {name: [] for name in kernels}
    for name, fn in kernels.items():   # warm-up: code objects, clocks, the allocator's blocks
        _event_ms(fn, 5)
    for _ in range(args.rounds):
        for name, fn in kernels.items():
            times[name].append(_event_ms(fn, reps[name]))
    copy_rate = nbytes["copy"] / (statistics.median(times["copy"]) * 1e-3)
    lines = [f"{_lib.lib().adaptseg_version().decode()}; labels {n}x{h}x{w}, crop {cw}x{ch}, {K} candidates per "
             f"sample, rows read per sample {rows}; HIP-event ms per call over {args.reps} back-to-back calls, median "
             f"(min .. max) of {args.rounds} alternating rounds; device-to-device copy {copy_rate / 1e12:.2f} TB/s"]
    res = {}
    for name in kernels:
        med = statistics.median(times[name])
        floor_ms = nbytes[name] / copy_rate * 1e3
        res[name] = {"ms": med, "min_ms": min(times[name]), "max_ms": max(times[name]), "bytes": nbytes[name],
                     "gb_per_s": nbytes[name] / (med * 1e-3) / 1e9, "floor_ms_copy": floor_ms,
                     "fraction_of_floor": floor_ms / med}
        lines.append(f"{name:36s} {med * 1e3:9.2f} us ({min(times[name]) * 1e3:.2f} .. {max(times[name]) * 1e3:.2f}); "
                     f"{nbytes[name]} bytes, floor {floor_ms * 1e3:.2f} us at the copy rate: {floor_ms / med:.3f} of it")
    ratio = res["composition"]["ms"] / res["crop_class_count (python surface)"]["ms"]
    lines.append(f"composition / crop_class_count (python surface) = {ratio:.1f}x")
    out = {"metric": "RCS kernel times", "unit": "ms", "shape": [n, h, w], "crop": [cw, ch], "tries": K,
           "reps": args.reps, "rounds": args.rounds, "rows_read": rows, "copy_tb_per_s": copy_rate / 1e12,
           "kernels": res, "composition_over_crop_class_count": ratio}
    print("\n".join(lines))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
