"""CPU: what every conv planning query returns, for a sweep of products, maths and options,
compared against the recorded fixture tests/golden/conv_plans.json.

The planner (adaptsegnet_amd/csrc/conv_igemm.hip) is host arithmetic: a descriptor, the conv
maths and the two kernel-selection options decide the kernel (its selector), the split count, the
workspace and weight-pack bytes and the tile counts of the fused BN statistics / sums.  The
fixture pins all of them, so a change of the planner that alters any choice shows as a diff here
before it shows as a speed or workspace change on the GPU.

Running this module as a script rewrites the fixture:  python tests/test_conv_plan_snapshot.py
"""
import ctypes
import json
import os
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_plans.json")

# (cin, cout, kh, kw, stride, pads, dils), n, h, w, layout ("nchw": the user's NCHW strides)
SHAPES = [
    # the model's conv products at bench size
    ((3, 64, 7, 7, 2, (3,), (1,)), 1, 65, 129, "nchw"),          # stem on the NCHW input
    ((4, 64, 7, 7, 2, (3,), (1,)), 1, 65, 129, None),            # stem, channel-padded
    ((64, 64, 1, 1, 1, (0,), (1,)), 4, 129, 257, None),          # layer1 conv1
    ((64, 64, 3, 3, 1, (1,), (1,)), 4, 129, 257, None),          # layer1 conv2
    ((64, 256, 1, 1, 1, (0,), (1,)), 4, 129, 257, None),         # layer1 conv3 / downsample
    ((256, 128, 1, 1, 2, (0,), (1,)), 4, 129, 257, None),        # layer2 conv1 (stride 2)
    ((128, 128, 3, 3, 1, (1,), (1,)), 4, 65, 129, None),         # layer2 conv2
    ((256, 256, 3, 3, 1, (2,), (2,)), 4, 65, 129, None),         # layer3 conv2
    ((1024, 256, 1, 1, 1, (0,), (1,)), 4, 65, 129, None),        # layer3 conv1
    ((512, 512, 3, 3, 1, (4,), (4,)), 4, 65, 129, None),         # layer4 conv2
    ((512, 2048, 1, 1, 1, (0,), (1,)), 4, 65, 129, None),        # layer4 conv3
    ((1024, 19, 3, 3, 1, (6, 12, 18, 24), (6, 12, 18, 24)), 4, 65, 129, None),   # ASPP on layer3
    ((2048, 19, 3, 3, 1, (6, 12, 18, 24), (6, 12, 18, 24)), 4, 65, 129, None),   # ASPP on layer4
    ((19, 64, 4, 4, 2, (1,), (1,)), 4, 64, 128, None),           # D conv1
    ((64, 128, 4, 4, 2, (1,), (1,)), 4, 32, 64, None),           # D conv2
    ((256, 512, 4, 4, 2, (1,), (1,)), 4, 8, 16, None),           # D conv4
    ((512, 1, 4, 4, 2, (1,), (1,)), 4, 4, 8, None),              # D classifier (1 channel)
    ((64, 2, 3, 3, 1, (1,), (1,)), 2, 64, 64, None),             # warper flow head (2 channels)
    ((512, 1024, 3, 3, 1, (12,), (12,)), 8, 41, 41, None),       # VGG fc6
    # edge shapes
    ((256, 256, 3, 3, 1, (2,), (2,)), 1, 8, 8, None),            # one tile or fewer
    ((48, 64, 3, 3, 1, (1,), (1,)), 2, 17, 23, None),            # x3 but not term-tile eligible
    ((64, 128, 3, 3, 1, (1,), (1,)), 2, 33, 33, None),           # Cout 128: 128-row weight gradient
    ((64, 256, 3, 3, 1, (1,), (1,)), 2, 33, 33, None),           # Cout 256: 256-row weight gradient
    ((256, 128, 3, 3, 1, (1,), (1,)), 2, 33, 33, None),          # N 128, K >= 2048 (98 / 198 ...)
    ((128, 256, 3, 3, 1, (1,), (1,)), 2, 33, 33, None),
    ((64, 48, 3, 3, 1, (1,), (1,)), 2, 17, 23, None),            # N < 64: register-staged bf16
    ((48, 64, 4, 4, 2, (1,), (1,)), 2, 16, 24, None),            # ... and its stride-2 data gradient
    ((256, 256, 4, 4, 2, (1,), (1,)), 2, 16, 24, None),          # stride-2 data gradient, N 256
    ((6, 8, 3, 3, 1, (1,), (1,)), 2, 9, 11, None),               # per-element operands
    ((6, 8, 3, 3, 2, (1,), (1,)), 2, 9, 11, "nchw"),
    ((8, 6, 3, 3, 2, (1,), (1,)), 2, 9, 11, None),
    ((16, 24, 3, 3, 1, (1,), (1,)), 2, 9, 11, None),             # small tiles (cfg 1 - 5)
    ((24, 48, 1, 1, 1, (0,), (1,)), 2, 9, 11, None),
    ((40, 40, 3, 3, 1, (1, 2), (1, 2)), 2, 9, 11, None),         # two segments
]

MATHS = (0, 1, 2, 3, 4)       # F32, BF16, BF16_WIDE, F32X3, F32X3_PRESPLIT (include/adaptseg.h)
OPTIONS = tuple((x3h, wide) for x3h in (3, 0, 7) for wide in (1, 0, 3))

# Selectors of the table in include/adaptseg.h ("Kernel selectors") that no descriptor reaches,
# with the rule that excludes them.  Everything else the table can return is in the fixture.
UNREACHABLE = {
    87: "x3h forward has no stride-2 parity form",
    187: "stride-2 data gradients are kept off the x3h tile (choose_x3)",
    286: "the x3h weight gradient runs the 128-row tile only (the 256-row one spills)",
    89: "the term-image forward has no stride-2 parity form",
    91: "forward has no stride-2 parity form", 93: "forward has no stride-2 parity form",
    96: "forward has no stride-2 parity form",
    92: "N >= 256 products under the bf16 maths are on the LDS-DMA kernel, never the staged 128x256",
    292: "weight gradients run the 128-wide staged bf16 tile only",
    291: "weight gradients have no stride-2 parity form", 293: "weight gradients have no stride-2 parity form",
    296: "weight gradients have no stride-2 parity form",
    294: "the LDS-DMA weight gradient's tiles are 85 / 98 / 99", 297: "the LDS-DMA weight gradient's tiles are 85 / 98 / 99",
}


def named_selectors():
    """Every selector of the named tiles (85 - 99 per product) the table can return."""
    return {100 * op + i for op in (0, 1, 2) for i in range(85, 100)}


def sweep():
    from adaptsegnet_amd import _lib, kernels as K
    L = _lib.lib()
    rows = []
    saved = K.get_conv_math(), K.get_x3h(), K.get_g16_wide()
    try:
        for math in MATHS:
            K.set_conv_math(math)
            for x3h, wide in OPTIONS:
                K.set_x3h(x3h)
                K.set_g16_wide(wide)
                for si, (geom, n, h, w, lay) in enumerate(SHAPES):
                    g = K.ConvGeom(*geom)
                    st = (g.cin * h * w, h * w, w, 1) if lay == "nchw" else K.nhwc_strides(n, h, w, g.cin)
                    d = K._desc(g, n, h, w, tuple(st))[0]
                    for op in (0, 1, 2):
                        r = [math, x3h, wide, si, op]
                        r += [list(K.conv_kernel_id(g, n, h, w, op, st, copies)) for copies in (False, True)]
                        b = ctypes.c_size_t(0)
                        assert L.adaptseg_conv2d_workspace_size(ctypes.byref(d), op, ctypes.byref(b)) == 0
                        r.append(b.value)
                        b = ctypes.c_size_t(0)
                        assert L.adaptseg_conv2d_wpack_size(ctypes.byref(d), op, ctypes.byref(b)) == 0
                        r.append(b.value)
                        r.append(int(K.conv_copy_operand_only(g, n, h, w, op, st)))
                        ok = ctypes.c_int(0)
                        assert L.adaptseg_conv2d_operand_bn_ok(ctypes.byref(d), op, ctypes.byref(ok)) == 0
                        r.append(ok.value)
                        if op == 0:
                            r += [K.conv_bnstats_tiles(g, n, h, w, st, False), K.conv_bnstats_tiles(g, n, h, w, st, True)]
                        elif op == 1 and lay is None:   # (the query takes the NHWC descriptor)
                            r += [K.conv_bnsum_tiles(g, n, h, w, False), K.conv_bnsum_tiles(g, n, h, w, True)]
                        rows.append(r)
    finally:
        K.set_conv_math(saved[0])
        K.set_x3h(saved[1])
        K.set_g16_wide(saved[2])
    return rows


def write_fixture(rows):
    with open(FIXTURE, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r, separators=(",", ":")) for r in rows) + "\n]\n")


@pytest.fixture(scope="module")
def rows():
    return sweep()


def test_conv_plans_match_the_fixture(rows):
    with open(FIXTURE) as f:
        want = json.load(f)
    assert len(rows) == len(want)
    diff = [(a, b) for a, b in zip(rows, want) if a != b]
    assert not diff, f"{len(diff)} of {len(rows)} rows differ; first (now, recorded): {diff[0]}"


def test_every_selector_is_recorded(rows):
    """Each selector of the named tiles is reached by some row, or listed as unreachable: a
    selector added to the table later cannot go unrecorded.  (The fp32-MFMA ids are the formula
    10 * cfg + variant, below 85: the fixture rows pin the ones the sweep reaches.)"""
    hit = {r[5][0] for r in rows} | {r[6][0] for r in rows}
    named = named_selectors()
    assert all(0 <= s < 300 for s in hit), sorted(hit)
    assert not (hit & set(UNREACHABLE)), sorted(hit & set(UNREACHABLE))
    assert named - hit == set(UNREACHABLE) & named, sorted((named - hit) ^ (set(UNREACHABLE) & named))


if __name__ == "__main__":
    rs = sweep()
    write_fixture(rs)
    ids = sorted({r[5][0] for r in rs} | {r[6][0] for r in rs})
    print(f"{len(rs)} rows, {len(ids)} selectors: {ids}")
