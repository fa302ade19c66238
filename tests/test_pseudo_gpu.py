"""Pseudo-labels and the self-training term on the GPU.

A. The three kernels (csrc/pseudo.hip) against the numpy restatement tests/pseudo_ref.py, bit for
   bit: int64 counts and labels with torch.equal, float32 thresholds by their bits.  Pixel counts
   around one block's share (256 x 16), both sides of the histogram's 64 KiB LDS budget
   (ncls * nbins <= 16,384 bins: block-private bins; above: adds into the global bins).
B. predict_tta -> ConfidenceHistogram -> thresholds -> pseudo_labels end to end on the tiny input
   of tests/test_tta_gpu.py, against the restatement applied to the same pred / conf.
C. The step with lambda_st = 1 against an fp64 oracle composed here from oracle.reference_torch
   (oracle_step's order plus the target CE term): one iteration, eval-mode BN; every loss within
   1e-4 rel + 1e-7, generator updates within 2 x (the fp32 oracle's distance to fp64) + 1e-4.
D. An all-ignored labels_target: loss 0, and the step is the lambda_st = 0 step bit for bit.
E. The stream orders of the target branch do not change a bit with the term in it.
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import reference_torch as R

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pseudo_ref as PR  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same_f32(got, want):
    assert got.dtype == torch.float32 and got.shape == tuple(want.shape)
    assert torch.equal(_bits(got), torch.from_numpy(np.ascontiguousarray(want)).view(torch.int32)), (got.cpu(), want)


# ---- A. kernels -------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _input(kind):
    """(pred uint8, conf float32, ncls, nbins) of a named case, made once."""
    if kind.startswith("mixed-"):
        shape = tuple(int(v) for v in kind[6:].split("x"))
        return PR.mixed_input(shape, 19, 512) + (19, 512)
    if kind == "road":   # every pixel on one (class, bin): the contention and the clamp path; 17 blocks
        return np.zeros(70001, dtype=np.uint8), np.ones(70001, dtype=np.float32), 19, 512
    if kind == "skew":   # a real map's shape: most pixels on one key, the rest spread
        pred, conf = PR.mixed_input((9001,), 19, 512, seed=9)
        hot = np.random.Generator(np.random.PCG64(10)).uniform(0, 1, 9001) < 0.8
        return np.where(hot, 0, pred).astype(np.uint8), np.where(hot, np.float32(0.999), conf), 19, 512
    if kind == "foreign":   # class bytes >= ncls (a void id in the map) are counted nowhere
        pred, conf = PR.mixed_input((2, 37, 53), 19, 512, seed=6)
        rng = np.random.Generator(np.random.PCG64(7))
        pred = np.where(rng.uniform(0, 1, pred.shape) < 0.25, rng.integers(19, 256, pred.shape), pred)
        return pred.astype(np.uint8), conf, 19, 512
    c, nbins = {"c40-4096": (40, 4096), "c4-4096": (4, 4096), "c5-4096": (5, 4096), "c256-64": (256, 64),
                "c256-128": (256, 128), "c3-2": (3, 2)}[kind]
    return PR.mixed_input((2, 37, 53), c, nbins, seed=8, empty_class=min(7, c - 1)) + (c, nbins)


HIST_CASES = ["mixed-1", "mixed-255", "mixed-257", "mixed-4097", "mixed-2x37x53", "road", "skew", "foreign",
              "c40-4096",    # 640 KiB of bins: the global path
              "c4-4096",     # 64 KiB exactly: the last size with block-private bins
              "c5-4096",     # the first size without
              "c256-64", "c256-128", "c3-2"]


@functools.lru_cache(maxsize=None)
def _ref_hist(kind):
    pred, conf, c, nbins = _input(kind)
    return PR.conf_hist(pred, conf, c, nbins)


def _gpu_hist(kind, times=1):
    from adaptsegnet_amd.pseudo import ConfidenceHistogram
    pred, conf, c, nbins = _input(kind)
    h = ConfidenceHistogram(c, nbins, DEV)
    for _ in range(times):
        h.update(_dev(pred), _dev(conf))
    return h


@pytest.mark.parametrize("kind", HIST_CASES)
def test_histogram_matches_reference(kind):
    h = _gpu_hist(kind)
    ref = _ref_hist(kind)
    assert h.hist.dtype == torch.int64 and h.hist.shape == ref.shape
    assert torch.equal(h.hist.cpu(), torch.from_numpy(ref)), kind


@pytest.mark.parametrize("kind", ["mixed-2x37x53", "c40-4096"])
def test_histogram_accumulates_and_repeats(kind):
    ref = torch.from_numpy(_ref_hist(kind))
    a, b = _gpu_hist(kind, times=2), _gpu_hist(kind, times=2)
    assert torch.equal(a.hist.cpu(), 2 * ref)
    assert torch.equal(a.hist, b.hist)
    a.reset()
    assert int(a.hist.abs().sum()) == 0


def test_histogram_takes_any_shape_of_the_same_pixels():
    from adaptsegnet_amd.pseudo import ConfidenceHistogram
    pred, conf, c, nbins = _input("mixed-2x37x53")
    h = ConfidenceHistogram(c, nbins, DEV)
    h.update(_dev(pred).permute(0, 2, 1), _dev(conf).permute(0, 2, 1))   # made contiguous in the same order
    assert torch.equal(h.hist.cpu(), torch.from_numpy(_ref_hist("mixed-2x37x53")))
    with pytest.raises(RuntimeError, match="float32"):
        h.update(_dev(pred), _dev(conf).double())
    with pytest.raises(RuntimeError, match="predictions vs"):
        h.update(_dev(pred), _dev(conf)[:1])


PORTION_CAP = [(p, c) for p in (0.2, 0.5, 1.0) for c in (0.9, 1.0)]


@pytest.mark.parametrize("portion,cap", PORTION_CAP)
@pytest.mark.parametrize("kind", ["mixed-2x37x53", "road", "skew", "c40-4096", "c256-64", "c3-2"])
def test_thresholds_match_reference(kind, portion, cap):
    """mixed: class 7 is empty (-> cap); road: every pixel of class 0 shares the top bin, all other
    classes are empty."""
    from adaptsegnet_amd.pseudo import ConfidenceHistogram
    ref = _ref_hist(kind)
    h = ConfidenceHistogram(ref.shape[0], ref.shape[1], DEV)
    h.hist.copy_(torch.from_numpy(ref))
    want = PR.thresholds(ref, portion, cap)
    _same_f32(h.thresholds(portion, cap), want)
    if kind == "road":
        assert want[0] == min(np.float32(511 / 512), np.float32(cap)) and (want[1:] == np.float32(cap)).all()
    if kind == "mixed-2x37x53":
        assert want[7] == np.float32(cap)


@pytest.mark.parametrize("nbins", [2, 128, 256, 512, 4096])
def test_thresholds_on_drawn_histograms(nbins):
    """Histograms drawn directly: sparse rows, one-bin rows (first, last and a middle bin), an empty row, and
    counts beyond 2^32 (the sums are int64, K = ceil(portion * T) in fp64)."""
    rng = np.random.Generator(np.random.PCG64(nbins))
    hist = rng.integers(0, 50, (12, nbins)) * (rng.uniform(0, 1, (12, nbins)) < 0.3)
    hist[3] = 0
    for row, b in ((4, 0), (5, nbins - 1), (6, nbins // 2)):
        hist[row] = 0
        hist[row, b] = 977
    hist[7] = rng.integers(0, 1 << 36, nbins)
    hist = hist.astype(np.int64)
    thr = torch.empty(12, dtype=torch.float32, device=DEV)
    for portion, cap in PORTION_CAP + [(1e-9, 1.0), (0.999999, 0.5)]:
        torch.ops.adaptseg.pseudo_thresholds(_dev(hist), portion, cap, thr)
        _same_f32(thr, PR.thresholds(hist, portion, cap))


@pytest.mark.parametrize("kind", ["mixed-1", "mixed-257", "mixed-4097", "mixed-2x37x53", "road", "skew", "foreign",
                                  "c40-4096"])
def test_labels_match_reference(kind):
    from adaptsegnet_amd.pseudo import pseudo_labels
    pred, conf, c, nbins = _input(kind)
    for portion, cap, ignore in ((0.5, 0.9, 255), (0.2, 1.0, 250)):
        thr = PR.thresholds(_ref_hist(kind), portion, cap)
        want, want_kept = PR.labels(pred, conf, thr, ignore)
        got, kept = pseudo_labels(_dev(pred), _dev(conf), _dev(thr), ignore, return_kept=True)
        assert got.dtype == torch.int64 and got.shape == pred.shape
        assert torch.equal(got.cpu(), torch.from_numpy(want)), kind
        assert torch.equal(kept.cpu(), torch.from_numpy(want_kept)), kind
        assert int(kept.sum()) == int((got != ignore).sum())
        assert torch.equal(pseudo_labels(_dev(pred), _dev(conf), _dev(thr), ignore), got)   # kept == NULL


def test_a_pixel_on_its_threshold_is_kept():
    from adaptsegnet_amd.pseudo import pseudo_labels
    thr = np.linspace(0.05, 0.95, 19).astype(np.float32)
    pred = np.arange(19 * 3, dtype=np.uint8) % 19
    conf = thr[pred].copy()
    conf[19:38] = np.nextafter(conf[19:38], np.float32(0))   # one ulp below: dropped
    conf[38:] = np.nextafter(conf[38:], np.float32(2))       # one ulp above: kept
    got, kept = pseudo_labels(_dev(pred), _dev(conf), _dev(thr), return_kept=True)
    want = pred.astype(np.int64)
    want[19:38] = 255
    assert torch.equal(got.cpu(), torch.from_numpy(want))
    assert torch.equal(kept.cpu(), torch.full((19,), 2, dtype=torch.int64))


# ---- B. end to end ------------------------------------------------------------------------------
def _load(model, state):
    model.load_state_dict({k: torch.from_numpy(v.copy()) if v.dtype == np.int64 else torch.from_numpy(v.copy()).float()
                           for k, v in state.items()})
    return model.to(DEV)


@functools.lru_cache(maxsize=None)
def _state(kind, seed):
    return R.det_state({"g": R.g_specs, "d": R.d_specs, "vgg": R.vgg_specs}[kind](), seed)


def test_predict_tta_to_pseudo_labels_end_to_end():
    from adaptsegnet_amd.evaluate import predict_tta
    from adaptsegnet_amd.model import DeeplabMulti
    from adaptsegnet_amd.pseudo import fit_thresholds, pseudo_labels
    m = _load(DeeplabMulti(19), _state("g", 1338))
    x = torch.from_numpy(R.det_images((1, 3, 64, 96), 31)).float().to(DEV)
    kw = dict(scales=(0.75, 1.0), mirror=True, out_hw=(128, 192))
    thr, hist = fit_thresholds(m, [x, torch.flip(x, dims=[2])], portion=0.5, cap=0.9, **kw)
    preds = [predict_tta(m, xx, return_confidence=True, **kw) for xx in (x, torch.flip(x, dims=[2]))]
    ref_hist = sum(PR.conf_hist(p.cpu().numpy(), c.cpu().numpy(), 19, 512) for p, c in preds)
    assert int(ref_hist.sum()) == 2 * 128 * 192
    assert torch.equal(hist.hist.cpu(), torch.from_numpy(ref_hist))
    ref_thr = PR.thresholds(ref_hist, 0.5, 0.9)
    _same_f32(thr, ref_thr)
    pred, conf = preds[0]
    lab, kept = pseudo_labels(pred, conf, thr, return_kept=True)
    want, want_kept = PR.labels(pred.cpu().numpy(), conf.cpu().numpy(), ref_thr)
    assert lab.shape == (1, 128, 192)
    assert torch.equal(lab.cpu(), torch.from_numpy(want)) and torch.equal(kept.cpu(), torch.from_numpy(want_kept))
    assert 0 < int(kept.sum()) < lab.numel()


# ---- C. the step against the fp64 oracle --------------------------------------------------------
CFG = dict(input_size=(57, 41), input_size_target=(49, 33))
LEVEL_GAN = [("single-level", "Vanilla"), ("multi-level", "LS")]


@pytest.fixture(scope="module")
def data():
    """The shapes of tests/test_model_gpu.py's ``data`` and pseudo-labels (half of them ignored) at both
    sizes a target prediction can have."""
    xs = torch.from_numpy(R.det_images((2, 3, 41, 57), 11))
    lab = torch.from_numpy(R.det_labels((2, 41, 57), 12))
    xt = torch.from_numpy(R.det_images((2, 3, 33, 49), 13))
    lt = {"single-level": torch.from_numpy(R.det_labels((2, 41, 57), 14, ignore_frac=0.5)),
          "multi-level": torch.from_numpy(R.det_labels((2, 33, 49), 14, ignore_frac=0.5))}
    return xs, lab, xt, lt


def _oracle_st_step(level, gan, data, dtype, lambda_st=1.0):
    """One iteration in oracle.reference_torch.oracle_step's order (eval-mode BN, iter_size 1) with the
    target CE term added to the adversarial backward.  Returns (G, losses)."""
    xs, lab, xt, lt = data
    xs, xt, lt = xs.to(dtype), xt.to(dtype), lt[level]
    c = R.DEFAULT_CFG | CFG | dict(level=level, gan=gan)
    G = R.to_torch(_state("g", 1338), dtype=dtype, trainable=R.g_trainable)
    D1 = R.to_torch(_state("d", 2001), dtype=dtype, trainable=lambda k: True)
    D2 = R.to_torch(_state("d", 2002), dtype=dtype, trainable=lambda k: True)
    multi = level == "multi-level"
    opt, opt_d1, opt_d2 = R.make_optimizers(G, D1 if multi else None, D2, c)
    opt.zero_grad()
    lr = R.lr_poly(c["learning_rate"], 0, c["num_steps"], c["power"])
    opt.param_groups[0]["lr"], opt.param_groups[1]["lr"] = lr, lr * 10
    for o in (opt_d1, opt_d2):
        if o is not None:
            o.zero_grad()
            o.param_groups[0]["lr"] = R.lr_poly(c["learning_rate_D"], 0, c["num_steps"], c["power"])
    tsize = c["input_size_target"] if multi else c["input_size"]
    Ds = ((D1, 1), (D2, 2)) if multi else ((D2, 2),)
    rg = lambda flag: [t.requires_grad_(flag) for D, _ in Ds for t in D.values()]  # noqa: E731
    fwd = lambda x, size: R.g_forward(G, x, size, False, grad_heads=2 if multi else 1)  # noqa: E731
    vals = {}
    rg(False)
    preds = dict(zip((1, 2), fwd(xs, c["input_size"])))
    seg = {h: F.cross_entropy(preds[h], lab, ignore_index=255) for _, h in Ds}
    (seg[2] + (c["lambda_seg"] * seg[1] if multi else 0)).backward()
    pts = dict(zip((1, 2), fwd(xt, tsize)))
    adv = {h: R.adv_loss(R.d_forward(D, F.softmax(pts[h], dim=1)), 0, gan) for D, h in Ds}
    st = {h: F.cross_entropy(pts[h], lt, ignore_index=255) for _, h in Ds}
    total = c["lambda_adv_target2"] * adv[2] + lambda_st * st[2]
    if multi:
        total = total + c["lambda_adv_target1"] * adv[1] + c["lambda_seg"] * lambda_st * st[1]
    total.backward()
    for _, h in Ds:
        vals[f"loss_seg{h}"], vals[f"loss_adv_target{h}"] = seg[h].item(), adv[h].item()
        vals[f"loss_st{h}"] = st[h].item()
    rg(True)
    for src, lbl in ((preds, 0), (pts, 1)):
        for D, h in Ds:
            l_d = R.adv_loss(R.d_forward(D, F.softmax(src[h].detach(), dim=1)), lbl, gan) / 2
            l_d.backward()
            vals[f"loss_D{h}"] = vals.get(f"loss_D{h}", 0.0) + l_d.item()
    opt.step()
    if opt_d1 is not None:
        opt_d1.step()
    opt_d2.step()
    return G, vals


def _trainer(level, gan, bn_train=False, gen="multi", **cfg):
    from adaptsegnet_amd.model import DeeplabMulti, DeeplabVGG, FCDiscriminator
    from adaptsegnet_amd.train import AdaptSegTrainer, StepConfig
    m = _load(DeeplabMulti(19), _state("g", 1338)) if gen == "multi" else _load(DeeplabVGG(19), _state("vgg", 4242))
    d1 = _load(FCDiscriminator(19), _state("d", 2001)) if level == "multi-level" else None
    d2 = _load(FCDiscriminator(19), _state("d", 2002))
    m.train(bn_train)
    return AdaptSegTrainer(m, d1, d2, StepConfig(**(CFG | dict(level=level, gan=gan) | cfg))), m, d1, d2


def _batch(data, level, labels_t=None):
    xs, lab, xt, lt = data
    lt = lt[level] if labels_t is None else labels_t
    return (xs.float().to(DEV), lab.to(DEV), xt.float().to(DEV), lt.to(DEV))


def _frob(a, b):
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


@pytest.mark.parametrize("level,gan", LEVEL_GAN)
def test_self_training_step_matches_fp64_oracle(data, level, gan):
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    G, ref = _oracle_st_step(level, gan, data, torch.float64)
    G32, _ = _oracle_st_step(level, gan, data, torch.float32)
    tr, m, _, _ = _trainer(level, gan, lambda_st=1.0)
    got = tr.step(0, [_batch(data, level)]).values()
    assert set(got) == set(ref), (sorted(got), sorted(ref))
    for k, v in ref.items():
        print(f"lambda_st=1 {level} {k}: hip={got[k]:.7f} fp64={v:.7f}")
    for k, v in ref.items():
        assert abs(got[k] - v) <= 1e-4 * abs(v) + 1e-7, (k, got[k], v)
    g0, sd = _state("g", 1338), m.state_dict()
    groups = {"trunk": [], "heads": []}
    for k, v in G.items():
        if v.dtype.is_floating_point and v.requires_grad and not (k.startswith("layer5") and level == "single-level"):
            groups["heads" if k.startswith(("layer5", "layer6")) else "trunk"].append(k)
    for name, keys in groups.items():
        upd = lambda P: torch.cat([(P[k].detach().double().cpu() - torch.from_numpy(g0[k])).flatten()  # noqa: E731
                                   for k in keys])
        dref = upd(G)
        f, f32 = _frob(upd(sd), dref), _frob(upd(G32), dref)
        print(f"lambda_st=1 {level} {name} update: rel-frob {f:.3e} (fp32 oracle {f32:.3e})")
        assert f <= 2 * f32 + 1e-4, (name, f, f32)


# ---- D. nothing kept --------------------------------------------------------------------------
def _run(data, level, gan, labels_t=None, steps=1, **cfg):
    tr, m, d1, d2 = _trainer(level, gan, bn_train=True, **cfg)
    losses = [tr.step(it, [_batch(data, level, labels_t)]).values() for it in range(steps)]
    torch.cuda.synchronize()
    return losses, [{k: v.detach().cpu().clone() for k, v in mm.state_dict().items()}
                    for mm in (m, d1, d2) if mm is not None]


@pytest.mark.parametrize("level,gan", LEVEL_GAN)
def test_all_ignored_labels_give_zero_loss_and_the_plain_step(data, level, gan):
    none = torch.full_like(data[3][level], 255)
    l1, s1 = _run(data, level, gan, none, lambda_st=1.0)
    l0, s0 = _run(data, level, gan, none, lambda_st=0.0)   # the fourth element is not looked at
    st = [k for k in l1[0] if k.startswith("loss_st")]
    assert st == (["loss_st2"] if level == "single-level" else ["loss_st1", "loss_st2"])
    assert all(l1[0][k] == 0.0 for k in st)
    assert {k: v for k, v in l1[0].items() if k not in st} == l0[0]
    for a, b in zip(s0, s1):
        for k in a:
            assert torch.isfinite(b[k].double()).all(), k
            assert torch.equal(a[k], b[k]), k


def test_mean_or_zero_is_the_mean_and_zero_when_nothing_is_left(data):
    from adaptsegnet_amd.functional import cross_entropy2d
    lt = data[3]["multi-level"].to(DEV)
    x = torch.from_numpy(R.det_images((2, 19, 33, 49), 3)).float().to(DEV).requires_grad_(True)
    a, b = cross_entropy2d(x, lt), cross_entropy2d(x, lt, reduction="mean_or_zero")
    assert torch.equal(a, b)
    ga, = torch.autograd.grad(a, x)
    gb, = torch.autograd.grad(b, x)
    assert torch.equal(ga, gb)
    none = torch.full_like(lt, 255)
    assert torch.isnan(cross_entropy2d(x, none))   # 'mean' is as it was
    z = cross_entropy2d(x, none, reduction="mean_or_zero")
    gz, = torch.autograd.grad(z, x)
    assert float(z.detach()) == 0.0 and int(gz.count_nonzero()) == 0 and torch.isfinite(gz).all()


# ---- E. stream orders -------------------------------------------------------------------------
PATHS = {
    "single-level": [dict(overlap_domains=False), dict(overlap_domains=True),
                     dict(overlap_domains=True, target_first=True), dict(overlap_domains=True, overlap_d=True),
                     dict(overlap_domains=False, d_reuse=False), dict(overlap_domains=True, second_head_only=False)],
    "multi-level": [dict(overlap_domains=False), dict(overlap_domains=True, overlap_d=True, target_first=True)],
}


@pytest.mark.parametrize("level,gan", LEVEL_GAN)
def test_target_branch_paths_are_bit_identical_with_the_term(data, level, gan):
    runs = [_run(data, level, gan, steps=2, lambda_st=1.0, **p) for p in PATHS[level]]
    l0, s0 = runs[0]
    assert l0[0]["loss_st2"] > 0
    for (l1, s1), p in zip(runs[1:], PATHS[level][1:]):
        assert l0 == l1, (p, l0, l1)
        for a, b in zip(s0, s1):
            for k in a:
                assert torch.equal(a[k], b[k]), (p, k)


def test_single_map_generator_takes_the_term():
    """DeeplabVGG through _pred_single (the caller-side interp): the term is the CE of the prediction
    the step made, and it moves the weights."""
    xs = torch.from_numpy(R.det_images((1, 3, 40, 56), 3)).float().to(DEV)
    lab = torch.from_numpy(R.det_labels((1, 40, 56), 4)).to(DEV)
    lt = torch.from_numpy(R.det_labels((1, 40, 56), 5, ignore_frac=0.5)).to(DEV)
    out = []
    for lam in (1.0, 0.0):
        tr, m, _, d2 = _trainer("single-level", "Vanilla", gen="vgg", lambda_st=lam, input_size=(56, 40),
                                input_size_target=(56, 40))
        with torch.no_grad():
            want = F.cross_entropy(F.interpolate(m(xs), size=(40, 56), mode="bilinear", align_corners=True), lt,
                                   ignore_index=255)
        vals = tr.step(0, [(xs, lab, xs, lt)]).values()
        out.append((vals, {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}))
        if lam:
            assert abs(vals["loss_st2"] - float(want)) <= 1e-5 * float(want), (vals, float(want))
    assert "loss_st2" not in out[1][0]
    assert any(not torch.equal(out[0][1][k], out[1][1][k]) for k in out[0][1])
