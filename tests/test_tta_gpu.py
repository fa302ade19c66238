"""Multi-scale / mirrored inference on the GPU: the fused kernel (adaptseg_fuse_argmax) and
evaluate.predict_tta.

A. Kernel parity against an fp64 stock-torch composition written here (flip, F.interpolate
   align_corners=True, softmax, mean, first-max argmax), both modes.
   * class map: a pixel may differ from the reference only where the reference's top-two fused
     scores differ by <= 1e-5 of the fused score range (the rule of tests/test_eval.py); as a
     condition of the case, such pixels are at most 0.1 % of it.
   * confidence (PROB): max |conf - ref| <= max(4 E, 1e-6), E = the error of the SAME composition
     run in stock-torch fp32 against fp64 on the same inputs (computed here: the bound comes from
     the reference side only).  4 covers another exp implementation and summation order, each a
     few ulp of values <= 1, below the coordinate-rounding term that dominates E.
B. Bitwise identities: S = 1 LOGIT is upsample_argmax; a mirror flag is a flipped map; two
   copies of a map fuse to that map (x2, x0.5 are exact: pins the accumulation); layouts.
C. predict_tta plumbing against predict / fuse_argmax on the model's own maps, bitwise.
D. predict_tta against the fp64 oracle network: class map free only where the oracle's top-two
   gap is <= 1e-3 of the range, confidence within 1e-3 of the fused-probability range (the
   fp32-network-vs-fp64 figure of tests/test_eval.py).  With this deterministic state the oracle
   predicts class 0 at every pixel, so the class-map half is weak; the confidence half and C
   carry the weight.
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

DEV = "cuda"
pytestmark = pytest.mark.gpu

# (n, C, ((h, w, mirror), ...), (OH, OW))
CASES = [
    (2, 19, ((9, 13, 0), (12, 17, 1), (17, 25, 0)), (40, 56)),
    (1, 19, ((64, 128, 0), (64, 128, 1), (96, 192, 0), (32, 64, 1)), (256, 512)),
    (1, 5, ((7, 9, 1), (5, 6, 0)), (20, 33)),
    (1, 40, ((6, 7, 0), (6, 7, 1)), (17, 23)),
    (1, 19, ((8, 8, 1),), (8, 8)),                       # the identity resize
    # 532,480 pixels: more than the 2048 x 256 threads of one launch, so the grid-stride loop
    # runs a second round (and part of the grid sits it out)
    (1, 19, ((20, 33, 0), (16, 30, 1)), (520, 1024)),
    # PROB mode keeps the classes in registers up to 32 of them and walks them three times above
    (1, 32, ((5, 6, 0), (7, 9, 1)), (17, 23)),
    (1, 33, ((5, 6, 0), (7, 9, 1)), (17, 23)),
    (1, 19, tuple((4 + s, 5 + s, s & 1) for s in range(8)), (19, 27)),   # the most maps
]
IDS = ["s3-odd", "s4-256x512", "c5", "c40", "identity", "two-rounds", "c32", "c33", "s8"]


def _compose(maps, mirrored, out_hw, mode, dtype):
    """The unfused composition in stock torch: fused scores [N, C, OH, OW] in `dtype`."""
    acc = None
    for m, mir in zip(maps, mirrored):
        t = m.to(dtype)
        if mir:
            t = torch.flip(t, dims=[3])
        v = F.interpolate(t, size=tuple(out_hw), mode="bilinear", align_corners=True)
        if mode == "prob":
            v = F.softmax(v, dim=1)
        acc = v if acc is None else acc + v
    return acc / len(maps) if mode == "prob" else acc


def _ambiguous(f, top_gap):
    s = torch.sort(f, dim=1, descending=True).values
    rng = (f.amax() - f.amin()).item()
    return (s[:, 0] - s[:, 1]) <= top_gap * rng


@functools.lru_cache(maxsize=None)
def _case(i):
    """The case's fp64 maps (seed 11, drawn in list order) and its references, computed once."""
    n, c, specs, out_hw = CASES[i]
    g = torch.Generator().manual_seed(11)
    maps = [torch.randn((n, c, h, w), generator=g, dtype=torch.float64) * 3 for h, w, _ in specs]
    mirrored = [bool(m) for _, _, m in specs]
    ref = {}
    for mode in ("prob", "logit"):
        f64 = _compose(maps, mirrored, out_hw, mode, torch.float64)
        ref[mode] = (f64.argmax(dim=1).to(torch.uint8), f64.amax(dim=1), _ambiguous(f64, 1e-5))
    f32 = _compose([m.float() for m in maps], mirrored, out_hw, "prob", torch.float32)
    e = (f32.amax(dim=1).double() - ref["prob"][1]).abs().max().item()
    return maps, mirrored, ref, e


@pytest.mark.parametrize("mode", ["prob", "logit"])
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_fused_kernel_matches_fp64_composition(i, mode):
    from adaptsegnet_amd.evaluate import fuse_argmax
    maps, mirrored, ref, e = _case(i)
    out_hw = CASES[i][3]
    ref_cls, ref_conf, amb = ref[mode]
    assert amb.sum().item() <= 1e-3 * amb.numel(), "the case itself has too many tied pixels"
    dmaps = [m.float().to(DEV).contiguous(memory_format=torch.channels_last) for m in maps]
    if mode == "prob":
        got, conf = fuse_argmax(dmaps, mirrored, out_hw, mode, return_confidence=True)
        err = (conf.double().cpu() - ref_conf).abs().max().item()
        bound = max(4 * e, 1e-6)
        print(f"{IDS[i]}: confidence max err {err:.3e} (stock fp32 E {e:.3e}, bound {bound:.3e})")
    else:
        got = fuse_argmax(dmaps, mirrored, out_hw, mode)
    assert got.dtype == torch.uint8 and got.shape == ref_cls.shape
    diff = got.cpu() != ref_cls
    print(f"{IDS[i]} {mode}: {int(diff.sum())} pixels differ, {int(amb.sum())} of {amb.numel()} ambiguous")
    assert not (diff & ~amb).any(), int((diff & ~amb).sum())
    if mode == "prob":
        assert err <= bound, (err, bound)


def _rand(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * 3).to(DEV)


def test_single_map_logit_is_upsample_argmax():
    from adaptsegnet_amd.evaluate import fuse_argmax, upsample_argmax
    m = _rand((2, 19, 16, 32), 1).contiguous(memory_format=torch.channels_last)
    assert torch.equal(fuse_argmax([m], out_hw=(128, 256), mode="logit"), upsample_argmax(m, (128, 256)))


def test_mirror_flag_is_a_flipped_map():
    from adaptsegnet_amd.evaluate import fuse_argmax
    m = _rand((2, 19, 9, 13), 2)
    a, ca = fuse_argmax([m], [True], (40, 56), return_confidence=True)
    b, cb = fuse_argmax([torch.flip(m, dims=[3])], [False], (40, 56), return_confidence=True)
    assert torch.equal(a, b) and torch.equal(ca, cb)
    plain = fuse_argmax([m], [False], (40, 56))
    assert not torch.equal(a, plain)   # and the flag does something
    assert torch.equal(fuse_argmax([m], [True], (40, 56), "logit"),
                       fuse_argmax([torch.flip(m, dims=[3])], [False], (40, 56), "logit"))


def test_two_copies_fuse_to_the_map_itself():
    from adaptsegnet_amd.evaluate import fuse_argmax
    m = _rand((1, 19, 11, 13), 3)
    a, ca = fuse_argmax([m, m], out_hw=(47, 61), return_confidence=True)
    b, cb = fuse_argmax([m], out_hw=(47, 61), return_confidence=True)
    assert torch.equal(a, b) and torch.equal(ca, cb)
    assert float(cb.min()) >= 1.0 / 19 and float(cb.max()) <= 1.0


def test_register_and_three_pass_kernels_give_the_same_bits():
    """PROB mode runs one kernel up to 32 classes and another above.  A 33rd class far below the
    others has probability exactly 0 and changes no sum, so both must give the same bits."""
    from adaptsegnet_amd.evaluate import fuse_argmax
    maps = [_rand((1, 32, 6, 7), 7), _rand((1, 32, 9, 5), 8)]
    wide = [torch.cat([m, torch.full_like(m[:, :1], -1e30)], dim=1) for m in maps]
    a, ca = fuse_argmax(maps, [False, True], (17, 23), return_confidence=True)
    b, cb = fuse_argmax(wide, [False, True], (17, 23), return_confidence=True)
    assert torch.equal(a, b) and torch.equal(ca, cb)


def test_layouts_give_the_same_bits():
    from adaptsegnet_amd.evaluate import fuse_argmax
    m0, m1 = _rand((2, 19, 9, 13), 4), _rand((2, 19, 12, 17), 5)
    cl = [m.contiguous(memory_format=torch.channels_last) for m in (m0, m1)]
    assert not cl[0].is_contiguous() and m0.is_contiguous()
    a, ca = fuse_argmax([m0, m1], [False, True], (40, 56), return_confidence=True)
    b, cb = fuse_argmax(cl, [False, True], (40, 56), return_confidence=True)
    assert torch.equal(a, b) and torch.equal(ca, cb)


def test_non_fp32_map_raises_on_the_device():
    from adaptsegnet_amd.evaluate import fuse_argmax
    with pytest.raises(RuntimeError, match="float32 HIP"):
        fuse_argmax([_rand((1, 19, 4, 6), 6).half()])


# ---- predict_tta ------------------------------------------------------------------------------
def _load(model, state):
    model.load_state_dict({k: torch.from_numpy(v.copy()) if v.dtype == np.int64 else torch.from_numpy(v.copy()).float()
                           for k, v in state.items()})
    return model.to(DEV)


@pytest.fixture(scope="module")
def multi():
    """DeeplabMulti(19) in the deterministic state of tests/test_eval.py, and its 1x3x64x96 input."""
    from adaptsegnet_amd.model import DeeplabMulti
    from oracle import reference_torch as R
    state = R.det_state(R.g_specs(), 1338)
    x = torch.from_numpy(R.det_images((1, 3, 64, 96), 31))
    return _load(DeeplabMulti(19), state), state, x


def test_predict_tta_single_scale_logit_is_predict(multi):
    from adaptsegnet_amd.evaluate import predict, predict_tta
    m, _, x = multi
    xd = x.float().to(DEV)
    got = predict_tta(m, xd, scales=(1.0,), mirror=False, out_hw=(128, 192), mode="logit")
    assert torch.equal(got, predict(m, xd, (128, 192)))


def test_predict_tta_is_fuse_argmax_on_its_four_maps(multi):
    from adaptsegnet_amd import functional as AF
    from adaptsegnet_amd.evaluate import fuse_argmax, predict_tta, tta_sizes
    m, _, x = multi
    xd = x.float().to(DEV)
    got, conf = predict_tta(m, xd, scales=(0.75, 1.0), mirror=True, out_hw=(128, 192), return_confidence=True)
    assert tta_sizes((64, 96), (0.75, 1.0)) == [(48, 72), (64, 96)]
    m.eval()
    with torch.no_grad():
        maps = []
        for inp in (AF.interp(xd, (48, 72)), xd):
            maps += [m(inp)[1], m(torch.flip(inp, dims=[3]))[1]]
    assert [tuple(t.shape[2:]) for t in maps] == [(48, 72), (48, 72), (64, 96), (64, 96)]
    ref, ref_conf = fuse_argmax(maps, [False, True, False, True], (128, 192), return_confidence=True)
    assert torch.equal(got, ref) and torch.equal(conf, ref_conf)
    # the order matters: the same maps with the flags swapped are another result
    _, other = fuse_argmax(maps, [True, False, True, False], (128, 192), return_confidence=True)
    assert not torch.equal(conf, other)


def test_predict_tta_single_output_model():
    """DeeplabVGG returns one un-upsampled map (single_output); 1x3x40x56 -> a 5x7 map is the
    smallest input the suite runs this model on (tests/test_vgg.py)."""
    from adaptsegnet_amd.evaluate import predict, predict_tta
    from adaptsegnet_amd.model import DeeplabVGG
    from oracle import reference_torch as R
    m = _load(DeeplabVGG(19), R.det_state(R.vgg_specs(), 4242))
    xd = torch.from_numpy(R.det_images((1, 3, 40, 56), 3)).float().to(DEV)
    got = predict_tta(m, xd, scales=(1.0,), mirror=False, out_hw=(80, 112), mode="logit")
    assert torch.equal(got, predict(m, xd, (80, 112)))
    cls, conf = predict_tta(m, xd, scales=(1.0,), mirror=True, out_hw=(80, 112), return_confidence=True)
    assert cls.shape == conf.shape == (1, 80, 112)


def test_predict_tta_matches_fp64_oracle(multi):
    from adaptsegnet_amd.evaluate import predict_tta
    from oracle import reference_torch as R
    m, state, x = multi
    G = R.to_torch(state)
    small = F.interpolate(x, size=(48, 72), mode="bilinear", align_corners=True)
    maps = []
    with torch.no_grad():
        for inp in (small, torch.flip(small, dims=[3]), x, torch.flip(x, dims=[3])):
            _, p2 = R.g_forward(G, inp, (inp.shape[3], inp.shape[2]), train=False)
            maps.append(p2.detach())
    # each oracle map is the network's answer to the (possibly flipped) input: flags as predict_tta's
    f64 = _compose(maps, [False, True, False, True], (128, 192), "prob", torch.float64)
    got, conf = predict_tta(m, x.float().to(DEV), scales=(0.75, 1.0), mirror=True, out_hw=(128, 192),
                            return_confidence=True)
    diff = got.cpu() != f64.argmax(dim=1).to(torch.uint8)
    amb = _ambiguous(f64, 1e-3)
    rng = (f64.amax() - f64.amin()).item()
    err = (conf.double().cpu() - f64.amax(dim=1)).abs().max().item()
    print(f"oracle: {int(diff.sum())} pixels differ, {int(amb.sum())} ambiguous, confidence err {err:.3e} "
          f"of range {rng:.3e}")
    assert not (diff & ~amb).any(), int((diff & ~amb).sum())
    assert err <= 1e-3 * rng, (err, rng)
