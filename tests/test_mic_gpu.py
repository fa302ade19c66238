"""Masked image consistency (MIC) on the GPU: the two kernels of csrc/mic.hip, EmaTeacher.mask and the step's
masked branch.

A. ``mask_patches`` (conf_count + patch_mask) against the numpy restatement tests/mic_ref.py, bit for bit: the
   scalar and the 16-byte paths, ragged grids, groups of four pixels that straddle a patch column, keys at the
   threshold and one below, NaN and -0.0 in the images, classes that are none, ignored rows, and more than one
   sweep of the capped grid on either path.
B. ``conf_count`` against ``classmix_stats``'s nconf; ``mask_patches(nconf=...)`` against the call without it.
C. Memory layouts: channels-last and sliced inputs give the contiguous call's bits.
D. ``EmaTeacher.mask`` against predict -> strong_augment -> mask_patches composed by hand; ``teacher=``.
E. The step with lambda_mic > 0 against an fp64 oracle: tests/test_classmix_gpu.py's, restated here with the
   masked branch after the mixed one.  Bounds: that file's ``_check_losses`` and its update bound, as they are.
F. Bit-for-bit identities of the masked branch (no tolerance anywhere).
"""
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import reference_torch as R

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mic_ref as MR  # noqa: E402
import test_classmix_gpu as TC  # noqa: E402  (its data, oracle pieces, trainer factory and bounds)

pytestmark = pytest.mark.gpu
DEV = "cuda"
TAU = np.float32(0.968)
RATIOS = (0.0, 0.7, 1.0)


def _fbits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _tbits(t):
    return t.detach().contiguous().cpu().numpy().view(np.int32)


# ---- A. the kernels against the numpy restatement -----------------------------------------------------
SHAPES = [(1, 1, 1, 1), (1, 5, 7, 64), (2, 33, 49, 8), (3, 41, 57, 5), (1, 40, 68, 6), (2, 37, 64, 16),
          (2, 64, 128, 64), (1, 130, 258, 64)]


def _mask_case(n, h, w, patch, seed):
    """numpy inputs of one call, the keys apart: (images_t, pred_t, conf_t)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    x = rng.uniform(-120, 150, (n, 3, h, w)).astype(np.float32)
    flat = x.reshape(-1).view(np.uint32)
    special = np.array([0x7FC00000, 0x7FC01234, 0xFFC00001, 0x7F800001, 0x80000000, 0x00000000, 0x80000001],
                       dtype=np.uint32)      # NaNs with payloads, -0.0, +0.0, a negative denormal
    idx = rng.integers(0, flat.size, max(1, min(flat.size // 3, 40)))
    flat[idx] = special[np.arange(len(idx)) % len(special)]
    pred = rng.integers(0, 21, (n, h, w)).astype(np.uint8)     # 19, 20: not a class
    pred.reshape(-1)[rng.integers(0, pred.size, max(1, pred.size // 10))] = 255
    conf = rng.beta(8.0, 1.0, (n, h, w)).astype(np.float32)
    cs = np.array([TAU, np.nextafter(TAU, np.float32(0)), np.nextafter(TAU, np.float32(1)), np.nan, 1.0, 0.0],
                  dtype=np.float32)
    cflat = conf.reshape(-1)
    cidx = rng.integers(0, cflat.size, max(1, min(len(cs) * 3, cflat.size // 2)))
    cflat[cidx] = cs[np.arange(len(cidx)) % len(cs)]
    return x, pred, conf


def _keys(n, h, w, patch, ratio, seed):
    """Random keys with the threshold and the value below it planted (where they are uint32 numbers)."""
    rng = np.random.Generator(np.random.PCG64(seed + 1000))
    gh, gw = MR.grid_of(h, w, patch)
    keys = rng.integers(0, 1 << 32, (n, gh, gw), dtype=np.uint32)
    thr = MR.threshold_of(ratio)
    plant = [v for v in (thr - 1, thr) if 0 <= v < 1 << 32]
    flat = keys.reshape(-1)
    pos = rng.permutation(flat.size)[:len(plant)]
    flat[pos] = np.array(plant[:len(pos)], dtype=np.uint32)
    return keys


def _run_mask(case, keys, patch, ratio, top=0, bottom=0, ignore_label=255, layout=None, nconf=None):
    from adaptsegnet_amd.mix import mask_patches
    t = [torch.from_numpy(a).to(DEV) for a in case]
    if layout is not None:
        t = layout(t)
    out = mask_patches(*t, keys, patch=patch, ratio=ratio, num_classes=19, tau=float(TAU), ignore_label=ignore_label,
                       ignore_top=top, ignore_bottom=bottom, nconf=nconf)
    torch.cuda.synchronize()
    return out


def _check_mask(out, case, keys, patch, ratio, top=0, bottom=0, ignore_label=255):
    x, pred, conf = case
    mi, ml, mw, nconf = MR.mask_patches(x, pred, conf, keys, patch, ratio, 19, TAU, ignore_label, top, bottom)
    g_mi, g_ml, g_mw = out
    assert g_ml.dtype == torch.int64 and np.array_equal(g_ml.cpu().numpy(), ml)
    assert g_mw.dtype == torch.float32 and np.array_equal(_tbits(g_mw), _fbits(mw))
    assert g_mi.dtype == torch.float32 and g_mi.is_contiguous() and g_mi.shape == x.shape
    assert np.array_equal(_tbits(g_mi), _fbits(mi))
    return mi, ml, mw, nconf


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_mask_patches_matches_the_numpy_restatement(shape):
    from adaptsegnet_amd.ops import OPS
    n, h, w, patch = shape
    k = SHAPES.index(shape)
    case = _mask_case(n, h, w, patch, seed=50 + k)
    top, bottom = ((0, 0), (min(2, h), 3), (0, 0), (h // 3, 1))[k % 4]     # nonzero in half of the cases
    nconf = torch.empty(n, dtype=torch.int32, device=DEV)
    OPS.conf_count(torch.from_numpy(case[2]).to(DEV), float(TAU), nconf)
    assert np.array_equal(nconf.cpu().numpy(), MR.conf_count(case[2], TAU))
    for ratio in RATIOS:
        keys = _keys(n, h, w, patch, ratio, seed=k)
        thr = MR.threshold_of(ratio)
        mi, ml, mw, nc = _check_mask(_run_mask(case, keys, patch, ratio, top, bottom), case, keys, patch, ratio, top,
                                     bottom)
        m = MR.pixel_mask(keys, h, w, patch, thr)
        assert m.all() if ratio == 1.0 else not m.any() if ratio == 0.0 else True
        if ratio == 0.0:     # nothing masked: the images' bits, NaNs and -0.0 included
            assert np.array_equal(_fbits(mi), _fbits(case[0]))
        if ratio == 1.0:
            assert not _fbits(mi).any()
        if ratio == 0.7 and keys.size >= 2:     # both planted keys are there, on either side of the rule
            assert (keys == thr).any() and (keys == thr - 1).any() and m.any() and not m.all()
        if h * w >= 64:
            assert (ml == 255).any() and 0 < int(nc.min()) and int(nc.max()) < h * w
            assert (mw > 0).any() and ((mw == 0).any() == (top + bottom > 0))


def test_more_than_one_sweep_of_the_capped_grid():
    """n = 8: patch_mask runs 256 blocks per image, one sweep covers 262144 pixels on the 16-byte path and 65536 on
    the scalar one; conf_count runs 64 blocks per image, a quarter of that."""
    from adaptsegnet_amd import _lib
    per_image = _lib.MIC_MAX_BLOCKS // 8 * 256
    assert _lib.MIC_COUNT_MAX_BLOCKS <= _lib.MIC_MAX_BLOCKS
    for k, (n, h, w, patch) in enumerate([(8, 300, 1000, 64), (8, 259, 261, 7)]):
        assert h * w > per_image * (4 if w % 4 == 0 else 1)
        case = _mask_case(n, h, w, patch, seed=70 + k)
        keys = _keys(n, h, w, patch, 0.7, seed=70 + k)
        _check_mask(_run_mask(case, keys, patch, 0.7, 15, 120), case, keys, patch, 0.7, 15, 120)


def test_other_ignore_label_and_patch_one():
    n, h, w = 2, 12, 20
    case = _mask_case(n, h, w, 1, seed=90)
    keys = _keys(n, h, w, 1, 0.7, seed=90)          # a key per pixel: the grid is the image
    assert keys.shape == (n, h, w)
    mi, ml, mw, _ = _check_mask(_run_mask(case, keys, 1, 0.7, ignore_label=250), case, keys, 1, 0.7, ignore_label=250)
    assert (ml == 250).any() and not (ml == 255).any()
    for top, bottom in ((12, 0), (0, 12), (5, 7), (100, 100)):       # ignore_top + ignore_bottom >= H
        out = _run_mask(case, keys, 1, 0.7, top, bottom)
        _check_mask(out, case, keys, 1, 0.7, top, bottom)
        assert not _tbits(out[2]).any()


# ---- B. nconf ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 41, 57), (3, 40, 68)], ids=["scalar", "vector"])
def test_conf_count_is_classmix_stats_nconf(shape):
    from adaptsegnet_amd.ops import OPS
    n, h, w = shape
    x, pred, conf = _mask_case(n, h, w, 8, seed=21)
    conf[0, 0, :] = TAU                              # a row exactly at tau: it counts
    conf[1, 1, :] = np.nextafter(TAU, np.float32(0))
    cd = torch.from_numpy(conf).to(DEV)
    lab = torch.from_numpy(R.det_labels((n, h, w), 5)).to(DEV)
    count = torch.empty((n, 19), dtype=torch.int32, device=DEV)
    want = torch.empty((n,), dtype=torch.int32, device=DEV)
    OPS.classmix_stats(lab, cd, float(TAU), 19, count, want)
    got = torch.full((n,), -7, dtype=torch.int32, device=DEV)      # overwritten, not accumulated
    OPS.conf_count(cd, float(TAU), got)
    OPS.conf_count(cd, float(TAU), got)
    assert torch.equal(got, want) and np.array_equal(got.cpu().numpy(), MR.conf_count(conf, TAU))
    assert int(got[0]) >= w
    keys = _keys(n, h, w, 8, 0.7, seed=3)
    a = _run_mask((x, pred, conf), keys, 8, 0.7, 1, 2)
    b = _run_mask((x, pred, conf), keys, 8, 0.7, 1, 2, nconf=want)
    for s, t in zip(a, b):
        assert s.dtype == t.dtype and np.array_equal(_tbits(s) if s.dtype == torch.float32 else s.cpu().numpy(),
                                                     _tbits(t) if t.dtype == torch.float32 else t.cpu().numpy())
    _check_mask(b, (x, pred, conf), keys, 8, 0.7, 1, 2)


# ---- C. layouts ---------------------------------------------------------------------------------------------
def test_layouts_give_the_same_bits():
    n, h, w, patch = 2, 40, 68, 6
    case = _mask_case(n, h, w, patch, seed=11)
    keys = _keys(n, h, w, patch, 0.7, seed=11)
    base = _run_mask(case, keys, patch, 0.7, 3, 4)

    def strided(t):
        x, pred, conf = t
        big = torch.zeros(n, h, w + 3, dtype=pred.dtype, device=DEV)
        big[:, :, 1:w + 1] = pred
        wide = torch.zeros(n, 3, h + 2, w + 5, device=DEV)
        wide[:, :, 1:h + 1, 1:w + 1] = x             # a slice: not contiguous, 4 bytes off a 16-byte boundary
        return [wide[:, :, 1:h + 1, 1:w + 1], big[:, :, 1:w + 1], conf.transpose(1, 2).contiguous().transpose(1, 2)]

    def channels_last(t):
        x, pred, conf = t
        return [x.contiguous(memory_format=torch.channels_last), pred, conf]

    def off_boundary(t):
        """Contiguous maps that start 4 bytes (pred_t: 1 byte) past a 16-byte boundary: W % 4 == 0 on the scalar path."""
        out = []
        for a in t:
            buf = torch.empty(a.numel() + 1, dtype=a.dtype, device=DEV)
            v = buf[1:].view(a.shape)
            v.copy_(a)
            assert v.is_contiguous() and v.data_ptr() % 16 != 0
            out.append(v)
        return out
    tk = torch.from_numpy(keys.view(np.int32)).to(DEV)
    for other in (_run_mask(case, keys, patch, 0.7, 3, 4, layout=strided),
                  _run_mask(case, keys, patch, 0.7, 3, 4, layout=channels_last),
                  _run_mask(case, keys, patch, 0.7, 3, 4, layout=off_boundary),
                  _run_mask(case, tk, patch, 0.7, 3, 4),                                  # keys already on the device
                  _run_mask(case, tk.repeat_interleave(2, dim=2)[:, :, ::2], patch, 0.7, 3, 4)):
        _check_mask(other, case, keys, patch, 0.7, 3, 4)
        for a, b in zip(base, other):
            assert a.dtype == b.dtype and a.shape == b.shape and b.is_contiguous()
    with pytest.raises(ValueError, match="keys"):
        _run_mask(case, keys[:, :-1], patch, 0.7)


# ---- D. EmaTeacher.mask ---------------------------------------------------------------------------------------
def _teacher():
    from adaptsegnet_amd.mix import EmaTeacher
    from adaptsegnet_amd.model import DeeplabMulti
    return EmaTeacher(TC._load(DeeplabMulti(19), TC._state("g", 1338)), alpha=0.99)


def _same(a, b):
    assert len(a) == len(b)
    for s, t in zip(a, b):
        assert s.dtype == t.dtype and s.shape == t.shape
        assert np.array_equal(_tbits(s) if s.dtype == torch.float32 else s.cpu().numpy(),
                              _tbits(t) if t.dtype == torch.float32 else t.cpu().numpy())


def test_teacher_mask_is_predict_augment_mask_patches():
    from adaptsegnet_amd.mix import ClassMixSampler, PatchMaskSampler, StrongAugSampler, mask_patches, strong_augment
    ema = _teacher()
    xs, lab, _, _, _ = TC._data()
    xs, lab = xs.float().to(DEV), lab.to(DEV)
    xt = torch.from_numpy(R.det_images((2, 3, 41, 57), 15)).float().to(DEV)
    pred, conf = ema.predict(xt, (57, 41))
    tau = float(conf.median())
    for augment in (False, True):
        sampler, aug = PatchMaskSampler(seed=3, patch=8, ratio=0.5), StrongAugSampler(seed=4) if augment else None
        s0, a0 = sampler.get_state(), aug.get_state() if augment else None
        got = ema.mask(xt, sampler, tau=tau, augment=aug, ignore_top=2, ignore_bottom=5)
        again = PatchMaskSampler(seed=9, patch=8, ratio=0.5)
        again.set_state(s0)
        img = xt
        if augment:
            aug2 = StrongAugSampler(seed=77)
            aug2.set_state(a0)
            img = strong_augment(xt, aug2.sample(2, 41, 57))
        want = mask_patches(img, pred, conf, again.sample(2, 41, 57), patch=8, ratio=0.5, tau=tau, ignore_top=2,
                            ignore_bottom=5)
        _same(got, want)
        assert got[0].shape == xt.shape and got[1].shape == (2, 41, 57) and got[2].shape == (2, 41, 57)
        zero = (got[0] == 0).all(dim=1)
        assert 0.2 < float(zero.float().mean()) < 0.8                 # about half of the patches are blank
        assert float(got[2][:, :2].abs().max()) == 0 and float(got[2][:, -5:].abs().max()) == 0
        live = got[2][:, 2:-5].reshape(2, -1)
        assert torch.equal(live.min(dim=1).values, live.max(dim=1).values)      # one q per image
        assert 0.3 < float(live[:, 0].mean()) < 0.7                              # tau is the batch's median
        sampler.set_state(s0)
        if augment:
            aug.set_state(a0)
        _same(ema.mask(xt, sampler, tau=tau, augment=aug, ignore_top=2, ignore_bottom=5, teacher=(pred, conf)), got)
    # mix(teacher=...) is mix(...): one teacher forward serves both
    a = ema.mix(xs, lab, xt, ClassMixSampler(seed=3), tau=tau)
    b = ema.mix(xs, lab, xt, ClassMixSampler(seed=3), tau=tau, teacher=(pred, conf))
    _same(a, b)


# ---- E. the step against the fp64 oracle ----------------------------------------------------------------------
CFG, LEVEL_GAN = TC.CFG, TC.LEVEL_GAN


@functools.lru_cache(maxsize=None)
def _masked():
    """A masked triple at input_size_target made by tests/mic_ref.py from the oracle's target batch (no teacher:
    no argmax tie can flip a label between fp32 and fp64)."""
    xt = TC._data()[2].numpy().astype(np.float32)                       # [2, 3, 33, 49]
    pred = R.det_labels((2, 33, 49), 18).astype(np.uint8)               # 255: not a class -> ignore_label
    rng = np.random.Generator(np.random.PCG64(19))
    conf = rng.uniform(0, 1, (2, 33, 49)).astype(np.float32)
    keys = rng.integers(0, 1 << 32, (2,) + MR.grid_of(33, 49, 8), dtype=np.uint32)
    mi, ml, mw, nconf = MR.mask_patches(xt, pred, conf, keys, 8, 0.5, 19, np.float32(0.6), 255, 2, 3)
    blank = (mi == 0).all(axis=1)
    assert 0.25 < blank.mean() < 0.75 and (ml == 255).any() and (mw == 0).any() and ((mw > 0.3) & (mw < 0.5)).any()
    return torch.from_numpy(mi), torch.from_numpy(ml), torch.from_numpy(mw)


@functools.lru_cache(maxsize=None)
def _oracle_step(level, gan, dtype, lambda_mic=1.0, lambda_mix=0.0, lambda_ent=0.0, lambda_st=0.0, d_input="softmax"):
    """tests/test_classmix_gpu.py's ``_oracle_step`` (eval-mode BN, iter_size 1) with the masked branch after the
    mixed one: one more forward, on the masked images at input_size_target.  Returns (G, losses)."""
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    xs, lab, xt, lt, mixed = TC._data()
    xs, xt = xs.to(dtype), xt.to(dtype)
    extra = []
    if lambda_mix > 0:
        extra.append(("mix", lambda_mix, (mixed[0].to(dtype), mixed[1], mixed[2].to(dtype)), CFG["input_size"]))
    if lambda_mic > 0:
        mk = _masked()
        extra.append(("mic", lambda_mic, (mk[0].to(dtype), mk[1], mk[2].to(dtype)), CFG["input_size_target"]))
    c = R.DEFAULT_CFG | CFG | dict(level=level, gan=gan)
    din = TC._selfinfo_torch if d_input == "entropy" else (lambda t: F.softmax(t, dim=1))
    G = R.to_torch(TC._state("g", 1338), dtype=dtype, trainable=R.g_trainable)
    D1 = R.to_torch(TC._state("d", 2001), dtype=dtype, trainable=lambda k: True)
    D2 = R.to_torch(TC._state("d", 2002), dtype=dtype, trainable=lambda k: True)
    multi, adv = level == "multi-level", level != "source-only"
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
    for _, h in Ds:
        vals[f"loss_seg{h}"] = seg[h].item()
    if adv:
        ltl = lt[level]
        pts = dict(zip((1, 2), fwd(xt, tsize)))
        advl = {h: R.adv_loss(R.d_forward(D, din(pts[h])), 0, gan) for D, h in Ds}
        total = c["lambda_adv_target2"] * advl[2]
        if multi:
            total = total + c["lambda_adv_target1"] * advl[1]
        for lam, name, term in ((lambda_st, "st", lambda t: F.cross_entropy(t, ltl, ignore_index=255)),
                                (lambda_ent, "ent", TC._entropy_torch)):
            if lam > 0:
                for _, h in Ds:
                    v = term(pts[h])
                    total = total + (lam if h == 2 else c["lambda_seg"] * lam) * v
                    vals[f"loss_{name}{h}"] = v.item()
        total.backward()
        for _, h in Ds:
            vals[f"loss_adv_target{h}"] = advl[h].item()
    for tag, lam, (mi, ml, mw), size in extra:   # the mixed, then the masked branch: a forward and the weighted CE
        pm = dict(zip((1, 2), fwd(mi, size)))
        total = 0
        for _, h in Ds:
            v = TC._wce_torch(pm[h], ml, mw)
            total = total + (lam if h == 2 else c["lambda_seg"] * lam) * v
            vals[f"loss_{tag}{h}"] = v.item()
        total.backward()
    if adv:
        rg(True)
        for src, lbl in ((preds, 0), (pts, 1)):
            for D, h in Ds:
                l_d = R.adv_loss(R.d_forward(D, din(src[h].detach())), lbl, gan) / 2
                l_d.backward()
                vals[f"loss_D{h}"] = vals.get(f"loss_D{h}", 0.0) + l_d.item()
    opt.step()
    if adv:
        if opt_d1 is not None:
            opt_d1.step()
        opt_d2.step()
    return G, vals


def _batch(level, with_labels_t=False, mixed=False, masked=True, ignore_masked=False):
    b = TC._batch(level, with_labels_t, mixed=mixed)
    if masked:
        mi, ml, mw = _masked()
        ml = torch.full_like(ml, 255) if ignore_masked else ml
        b += (mi.to(DEV), ml.to(DEV), mw.to(DEV))
    return b


def _check_step(tag, level, gan, with_labels_t=False, **kw):
    G, ref = _oracle_step(level, gan, torch.float64, **kw)
    G32, _ = _oracle_step(level, gan, torch.float32, **kw)
    tr, m, _, _ = TC._trainer(level, gan, **kw)
    got = tr.step(0, [_batch(level, with_labels_t, mixed=kw.get("lambda_mix", 0.0) > 0)]).values()
    assert "loss_mic2" in got and ("loss_mic1" in got) == (level == "multi-level")
    assert ("loss_mix2" in got) == (kw.get("lambda_mix", 0.0) > 0)
    assert ref["loss_mic2"] > 0.3
    TC._check_losses(tag, got, ref)
    for name, (f, f32) in TC._updates(level, G, G32, m).items():
        print(f"{tag} {name} update: rel-frob {f:.3e} (fp32 oracle {f32:.3e})")
        assert f <= 2 * f32 + 1e-4, (name, f, f32)


@pytest.mark.parametrize("level,gan", LEVEL_GAN)
def test_masked_term_step_matches_fp64_oracle(level, gan):
    _check_step(f"lambda_mic=1 {level}", level, gan, lambda_mic=1.0)


def test_all_options_together_match_fp64_oracle():
    _check_step("mic+mix+st+ent", "single-level", "Vanilla", with_labels_t=True, lambda_mic=1.0, lambda_mix=1.0,
                lambda_st=1.0, lambda_ent=1.0)


# ---- F. bit-for-bit identities -----------------------------------------------------------------------------------
def _states(*models):
    return [{k: v.detach().cpu().clone() for k, v in mm.state_dict().items()} for mm in models if mm is not None]


def _same_states(a, b, tag):
    assert len(a) == len(b)
    for sa, sb in zip(a, b):
        assert set(sa) == set(sb)
        for k in sa:
            assert sa[k].dtype == sb[k].dtype and torch.equal(sa[k], sb[k]) if not sa[k].dtype.is_floating_point \
                else TC._bits_equal(sa[k], sb[k]), (tag, k)


@pytest.mark.parametrize("level,gan", LEVEL_GAN)
def test_masked_branch_is_the_mixed_branch_on_the_same_triple(level, gan):
    """input_size == input_size_target and one triple T: lambda_mic with T as the masked triple is lambda_mix with T
    as the mixed triple (parameters, D parameters, loss values)."""
    size = dict(input_size=(57, 41), input_size_target=(57, 41))
    xs, lab, _, _, T = TC._data()
    xt = torch.from_numpy(R.det_images((2, 3, 41, 57), 15)).float().to(DEV)
    head = (xs.float().to(DEV), lab.to(DEV)) + (() if level == "source-only" else (xt,))
    batch = head + tuple(t.to(DEV) for t in T)
    out = []
    for lam in ("lambda_mic", "lambda_mix"):
        tr, m, d1, d2 = TC._trainer(level, gan, bn_train=True, **(size | {lam: 0.75}))
        vals = tr.step(0, [batch]).values()
        torch.cuda.synchronize()
        out.append(({k.replace("loss_mic", "loss_mix"): v for k, v in vals.items()}, _states(m, d1, d2)))
    assert out[0][0] == out[1][0] and out[0][0]["loss_mix2"] > 0, (out[0][0], out[1][0])
    _same_states(out[0][1], out[1][1], level)


def test_default_is_the_step_as_it_was():
    b = TC._batch("single-level", mixed=False)
    TC._same_runs(TC._run("single-level", "Vanilla", steps=1, batch=b),
                  TC._run("single-level", "Vanilla", steps=1, batch=b, lambda_mic=0.0), "lambda_mic=0")
    b = TC._batch("multi-level", mixed=True)
    TC._same_runs(TC._run("multi-level", "LS", steps=1, batch=b, lambda_mix=1.0),
                  TC._run("multi-level", "LS", steps=1, batch=b, lambda_mix=1.0, lambda_mic=0.0), "lambda_mic=0, mix")


@pytest.mark.parametrize("level,gan", LEVEL_GAN)
def test_all_ignored_masked_labels_leave_the_step_as_it_was(level, gan):
    tr, m, d1, d2 = TC._trainer(level, gan, lambda_mic=1.0)
    got = tr.step(0, [_batch(level, ignore_masked=True)]).values()
    tr0, m0, d10, d20 = TC._trainer(level, gan)
    want = tr0.step(0, [_batch(level, masked=False)]).values()
    torch.cuda.synchronize()
    assert got["loss_mic2"] == 0.0 and got.get("loss_mic1", 0.0) == 0.0
    assert {k: v for k, v in got.items() if not k.startswith("loss_mic")} == want
    _same_states(_states(m, d1, d2), _states(m0, d10, d20), level)


@pytest.mark.parametrize("level,gan", LEVEL_GAN[:2])
def test_stream_orders_are_bit_identical_with_the_masked_branch(level, gan):
    batch = _batch(level, mixed=level == "multi-level")
    cfg = dict(lambda_mic=1.0, lambda_mix=1.0 if level == "multi-level" else 0.0)
    runs = [TC._run(level, gan, batch=batch, **cfg, **p) for p in TC.PATHS[level]]
    assert runs[0][0][0]["loss_mic2"] > 0 and runs[0][0][1]["loss_mic2"] != runs[0][0][0]["loss_mic2"]
    for r, p in zip(runs[1:], TC.PATHS[level][1:]):
        TC._same_runs(runs[0], r, p)


def _end_to_end():
    from adaptsegnet_amd.mix import PatchMaskSampler
    tr, m, _, d2 = TC._trainer("single-level", "Vanilla", bn_train=True, lambda_mic=1.0, input_size_target=(57, 41))
    ema = _teacher()
    sampler = PatchMaskSampler(seed=3, patch=8, ratio=0.7)
    state = sampler.get_state()
    xs, lab, _, _, _ = TC._data()
    xs, lab = xs.float().to(DEV), lab.to(DEV)
    xt = torch.from_numpy(R.det_images((2, 3, 41, 57), 15)).float().to(DEV)
    tau = float(ema.predict(xt, (57, 41))[1].median())
    losses, images = [], []
    for it in range(2):
        ema.update(m, it)
        masked = ema.mask(xt, sampler, tau=tau, ignore_top=1, ignore_bottom=4)
        images.append(masked[0].detach().cpu().clone())
        losses.append(tr.step(it, [(xs, lab, xt) + tuple(masked)]).values())
    torch.cuda.synchronize()
    assert sampler.get_state() != state
    return losses, _states(m, d2, ema.teacher), images


def test_end_to_end_two_iterations_repeat_bit_for_bit():
    a, b = _end_to_end(), _end_to_end()
    losses, states, images = a
    assert all(math.isfinite(v) for vals in losses for v in vals.values()), losses
    assert all(vals["loss_mic2"] > 0 for vals in losses)
    assert not torch.equal(images[0], images[1])              # the second draw masks other patches
    for im in images:
        assert 0.4 < float((im == 0).all(dim=1).float().mean()) < 0.95
    assert a[0] == b[0], (a[0], b[0])
    _same_states(a[1], b[1], "end to end")
    for ia, ib in zip(a[2], b[2]):
        assert TC._bits_equal(ia, ib)
