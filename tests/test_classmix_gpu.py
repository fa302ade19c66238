"""Online self-training on the GPU: the EMA, ClassMix and pixel-weighted CE kernels, the step's mixed branch.

A. EMA (csrc/mix.hip): alpha = 0 copies the source's bits, alpha = 1 leaves dst's bits, a general alpha
   within the two roundings of dst = fmaf(a, dst, (1 - a) * src), |err| <= 2 * 2^-24 * (|a dst| + |(1 - a) src|)
   against fp64, on both kernels (16-byte and scalar), the tail, more than one grid sweep and the
   multi-tensor form; EmaTeacher.update on a DeeplabMulti.
B. ClassMix against the numpy restatement tests/classmix_ref.py, bit for bit.
C. The pixel-weighted cross entropy against an fp64 closed form, values and gradients, at the
   tolerances tests/test_ops_gpu.py holds cross_entropy2d to (1e-5 relative, rel-Frobenius 1e-5).
D. The step with lambda_mix = 1 against an fp64 oracle composed here from oracle.reference_torch
   (tests/test_entropy_gpu.py's composition with the mixed branch added); bounds as there.
E. Two iterations of EmaTeacher.mix -> step -> update, end to end, twice: the same bits.
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
import classmix_ref as CR  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 2.0 ** -24


def _frob(a, b):
    a, b = a.detach().double().cpu().flatten(), b.detach().double().cpu().flatten()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _bits(t):
    return t.detach().contiguous().cpu().view(torch.int32)


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


# ---- A. EMA ---------------------------------------------------------------------------------------
def _ema_sizes():
    from adaptsegnet_amd import _lib
    sweep = _lib.EMA_MAX_BLOCKS * 256 * 4   # elements one sweep of the capped grid covers (adaptseg.h)
    return [1, 63, 4097, sweep + 4099]


def _ema_pair(n, seed, offset=0):
    """(dst, src) fp32 CPU tensors of n elements; offset 1: views 4 bytes off a 16-byte boundary."""
    g = torch.Generator().manual_seed(seed)
    d = torch.randn(n + offset, generator=g) * 3
    s = torch.randn(n + offset, generator=g) * 3
    return d[offset:], s[offset:]


def _ema_check(got, d0, s, alpha):
    a32 = np.float32(alpha)
    b32 = np.float32(1) - a32
    a, b = float(a32), float(b32)
    ref = a * d0.double() + b * s.double()
    bound = 2 * EPS * ((a * d0.double()).abs() + (b * s.double()).abs())
    err = (got.double().cpu() - ref).abs()
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"ema n={d0.numel()} alpha={alpha}: max err / bound = {worst:.3f}")
    assert (err <= bound).all(), worst


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "unaligned"])
@pytest.mark.parametrize("n", _ema_sizes())
def test_ema_follows_the_rule(n, offset):
    from adaptsegnet_amd.mix import ema_update
    d0, s = _ema_pair(n, 100 + n % 1000, offset)
    for alpha in (0.99, 0.37):
        buf, sbuf = torch.empty(n + offset, device=DEV), torch.empty(n + offset, device=DEV)
        dd, sd = buf[offset:], sbuf[offset:]
        dd.copy_(d0)
        sd.copy_(s)
        assert (dd.data_ptr() % 16 == 0) == (offset == 0)
        out = ema_update(dd, sd, alpha)
        assert out.data_ptr() == dd.data_ptr()
        _ema_check(dd, d0, s, alpha)
        assert _bits_equal(sd, s)   # the source is only read
    # the end points: bits, not values
    d1, s1 = d0.clone(), s.clone()
    special = torch.tensor([-0.0, 0.0, float("inf"), float("-inf"), float("nan"), 1e-45, -1e-45])[:min(7, n)]
    s1[:special.numel()] = special
    d1[:special.numel()] = special.flip(0)
    buf, sbuf = torch.empty(n + offset, device=DEV), torch.empty(n + offset, device=DEV)
    dd, sd = buf[offset:], sbuf[offset:]
    dd.copy_(d1)
    sd.copy_(s1)
    ema_update(dd, sd, 1.0)
    assert _bits_equal(dd, d1)
    ema_update(dd, sd, 0.0)
    assert _bits_equal(dd, s1)


def test_ema_multi_tensor_form():
    from adaptsegnet_amd import _lib
    from adaptsegnet_amd.ops import OPS
    g = torch.Generator().manual_seed(7)
    sizes = [1, 63, 64, 2048, 300, 0, 64 * 256 + 17] + [1 + (i * 37) % 513 for i in range(2 * _lib.EMA_CHUNK)]
    assert len(sizes) > 2 * _lib.EMA_CHUNK and max(sizes) > 64 * 256   # three launches, one tensor loops its blocks
    d0 = [torch.randn(n, generator=g) * 2 for n in sizes]
    s0 = [torch.randn(n, generator=g) * 2 for n in sizes]
    dd, sd = [t.to(DEV) for t in d0], [t.to(DEV) for t in s0]
    OPS.ema_multi(sd, dd, 0.9)
    for got, d, s in zip(dd, d0, s0):
        if d.numel():
            _ema_check(got, d, s, 0.9)
    before = [t.clone() for t in dd]
    OPS.ema_multi(sd, dd, 1.0)
    assert all(_bits_equal(a, b) for a, b in zip(dd, before))
    OPS.ema_multi(sd, dd, 0.0)
    assert all(_bits_equal(a, b) for a, b in zip(dd, s0))


def _load(model, state):
    model.load_state_dict({k: torch.from_numpy(v.copy()) if v.dtype == np.int64 else torch.from_numpy(v.copy()).float()
                           for k, v in state.items()})
    return model.to(DEV)


@functools.lru_cache(maxsize=None)
def _state(kind, seed):
    return R.det_state({"g": R.g_specs, "d": R.d_specs, "vgg": R.vgg_specs}[kind](), seed)


def test_ema_teacher_update_on_deeplab_multi():
    from adaptsegnet_amd.mix import EmaTeacher
    from adaptsegnet_amd.model import DeeplabMulti, DeeplabVGG
    s_state = dict(_state("g", 1338))
    for i, k in enumerate(k for k in s_state if k.endswith("num_batches_tracked")):
        s_state[k] = np.array(3 + i, dtype=np.int64)
    student = _load(DeeplabMulti(19), s_state).train()
    teacher = _load(DeeplabMulti(19), _state("g", 77))
    ema = EmaTeacher(teacher, alpha=0.99)
    flags = {k: p.requires_grad for k, p in student.named_parameters()}
    t0 = {k: v.detach().cpu().clone() for k, v in teacher.state_dict().items()}
    s0 = {k: v.detach().cpu().clone() for k, v in student.state_dict().items()}
    assert ema.momentum(5) == 1 - 1 / 6
    ema.update(student, 5)
    torch.cuda.synchronize()
    assert teacher.arena.numel == student.arena.numel and teacher.arena.offsets == student.arena.offsets
    assert teacher.arena.numel > 40_000_000   # the whole generator, one launch
    got = teacher.state_dict()
    assert set(got) == set(s0)
    nfloat = 0
    a32 = np.float32(1 - 1 / 6)
    a, b = float(a32), float(np.float32(1) - a32)
    for k, v in got.items():
        v = v.detach().cpu()
        if v.dtype.is_floating_point:
            nfloat += 1
            ref = a * t0[k].double() + b * s0[k].double()
            bound = 2 * EPS * ((a * t0[k].double()).abs() + (b * s0[k].double()).abs())
            assert ((v.double() - ref).abs() <= bound).all(), k
            assert not torch.equal(v, t0[k]) or torch.equal(t0[k], s0[k]), k   # it did move
        else:
            assert k.endswith("num_batches_tracked") and torch.equal(v, s0[k]) and int(v) >= 3, k
    assert nfloat > 500
    # the student is only read, and keeps its flags; the teacher stays frozen, in eval mode
    for k, v in student.state_dict().items():
        assert torch.equal(v.detach().cpu(), s0[k]), k
    assert {k: p.requires_grad for k, p in student.named_parameters()} == flags
    assert not teacher.training and not any(p.requires_grad for p in teacher.parameters())
    # i_iter = 0: the teacher becomes the student, bit for bit
    ema.update(student, 0)
    for k, v in teacher.state_dict().items():
        v = v.detach().cpu()
        assert _bits_equal(v, s0[k]) if v.dtype.is_floating_point else torch.equal(v, s0[k]), k
    # and it still predicts: class map and confidence at the size asked for
    x = torch.from_numpy(R.det_images((1, 3, 33, 41), 3)).float().to(DEV)
    pred, conf = ema.predict(x, (45, 37))
    assert pred.dtype == torch.uint8 and pred.shape == (1, 37, 45) and conf.shape == (1, 37, 45)
    assert int(pred.max()) < 19 and float(conf.min()) > 0 and float(conf.max()) <= 1
    with pytest.raises(ValueError, match="different parameters"):
        EmaTeacher(DeeplabVGG(19).to(DEV)).update(student, 1)


# ---- B. ClassMix ------------------------------------------------------------------------------------
TAU = np.float32(0.968)


def _mix_case(n, h, w, c, seed, labels="random", equal_keys=False):
    """numpy inputs of one ClassMix call: (images_s, labels_s, images_t, pred_t, conf_t, keys)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    xs = rng.uniform(-120, 150, (n, 3, h, w)).astype(np.float32)
    xt = rng.uniform(-120, 150, (n, 3, h, w)).astype(np.float32)
    if labels == "random":       # every class and, here and there, ignore, labels >= C and negative ones
        lab = rng.integers(0, c, (n, h, w)).astype(np.int64)
        u = rng.uniform(0, 1, (n, h, w))
        lab[u < 0.1] = 255 if c <= 255 else 300
        lab[(u >= 0.1) & (u < 0.13)] = c + 3
        lab[(u >= 0.13) & (u < 0.16)] = -1
        lab[(u >= 0.16) & (u < 0.17)] = -(2 ** 40)
        lab[(u >= 0.17) & (u < 0.18)] = 2 ** 40 + 1
        if n > 1:                # image 1 holds a few classes only: some are absent
            lab[1] = np.where(lab[1] >= 0, lab[1] % min(c, 5), lab[1])
    elif labels == "ignore":
        lab = np.full((n, h, w), 255 if c <= 255 else 300, dtype=np.int64)
    else:                        # a single class
        lab = np.full((n, h, w), int(labels), dtype=np.int64)
    pred = rng.integers(0, min(c + 2, 256), (n, h, w)).astype(np.uint8)   # c, c + 1: not a class -> ignore_label
    conf = rng.beta(8.0, 1.0, (n, h, w)).astype(np.float32)
    special = np.array([TAU, np.nextafter(TAU, np.float32(0)), np.nextafter(TAU, np.float32(1)), np.nan, 1.0, 0.0],
                       dtype=np.float32)
    flat = conf.reshape(-1)
    idx = rng.permutation(flat.size)[:min(len(special) * 3, flat.size // 2)]
    flat[idx] = special[np.arange(len(idx)) % len(special)]
    keys = rng.integers(0, 1 << 32, (n, c), dtype=np.uint32)
    if equal_keys:
        keys[:] = 12345
    return xs, lab, xt, pred, conf, keys


def _run_mix(case, c, ignore_label=255, layout=None):
    from adaptsegnet_amd.mix import classmix
    xs, lab, xt, pred, conf, keys = case
    t = [torch.from_numpy(a).to(DEV) for a in (xs, lab, xt, pred, conf)]
    if layout is not None:
        t = layout(t)
    out = classmix(*t, keys, num_classes=c, tau=float(TAU), ignore_label=ignore_label, return_mask=True,
                   return_stats=True)
    torch.cuda.synchronize()
    return out


def _check_mix(out, case, c, ignore_label=255):
    xs, lab, xt, pred, conf, keys = case
    mi, ml, mw, mask, count, nconf = CR.classmix(xs, lab, xt, pred, conf, keys, c, TAU, ignore_label)
    g_mi, g_ml, g_mw, g_mask, g_count, g_nconf = out
    assert g_count.dtype == torch.int32 and np.array_equal(g_count.cpu().numpy(), count)
    assert g_nconf.dtype == torch.int32 and np.array_equal(g_nconf.cpu().numpy(), nconf)
    assert g_mask.dtype == torch.uint8 and np.array_equal(g_mask.cpu().numpy(), mask)
    assert g_ml.dtype == torch.int64 and np.array_equal(g_ml.cpu().numpy(), ml)
    assert g_mw.dtype == torch.float32 and np.array_equal(g_mw.cpu().numpy().view(np.int32), mw.view(np.int32))
    assert g_mi.dtype == torch.float32 and g_mi.is_contiguous()
    assert np.array_equal(g_mi.cpu().numpy().view(np.int32), mi.view(np.int32))
    return mi, ml, mw, mask, count, nconf


def _mix_shapes():
    from adaptsegnet_amd import _lib
    sweep = _lib.CLASSMIX_MAX_BLOCKS * 256   # pixels per sweep of the capped grid: x 4 on the 16-byte path
    big4 = (1, 513, 4 * sweep // 512 + 4, 19)      # H * W % 4 == 0, more than one 16-byte sweep
    big1 = (1, 363, (sweep // 363 + 5) | 1, 19)    # odd H * W, more than one scalar sweep
    assert big4[1] * big4[2] % 4 == 0 and big4[1] * big4[2] > 4 * sweep
    assert (big1[1] * big1[2]) % 2 == 1 and big1[1] * big1[2] > sweep
    return [(1, 1, 1, 19), (2, 41, 57, 19), (1, 3, 4099, 19), (3, 64, 64, 1), (2, 37, 53, 256), (2, 40, 52, 19),
            big4, big1]


@pytest.mark.parametrize("shape", _mix_shapes(), ids=lambda s: "x".join(map(str, s)))
def test_classmix_matches_the_numpy_restatement(shape):
    n, h, w, c = shape
    case = _mix_case(n, h, w, c, seed=31 + h)
    mi, ml, mw, mask, count, nconf = _check_mix(_run_mix(case, c), case, c)
    if h * w >= 64:   # the case does exercise the rule: something pasted, something kept, labels dropped
        assert 0 < int(mask.sum()) and (mw == 1).any() and (mw != 1).any()
        assert int(count.sum()) < n * h * w
        if c < 255:
            assert (ml == 255).any()
    assert ((mw >= 0) & (mw <= 1)).all()


def test_classmix_label_patterns():
    n, h, w, c = 2, 41, 57, 19
    # all-ignore: nothing is pasted, the output is the target
    case = _mix_case(n, h, w, c, 5, labels="ignore")
    mi, ml, mw, mask, count, nconf = _check_mix(_run_mix(case, c), case, c)
    assert int(mask.sum()) == 0 and int(count.sum()) == 0 and np.array_equal(mi, case[2])
    assert np.array_equal(ml, np.where(case[3] < c, case[3], 255).astype(np.int64))
    assert np.array_equal(mw, np.broadcast_to((nconf.astype(np.float32) / np.float32(h * w))[:, None, None], mw.shape))
    # a single class: k = 1, it is selected, everything is pasted
    case = _mix_case(n, h, w, c, 6, labels=7)
    mi, ml, mw, mask, count, nconf = _check_mix(_run_mix(case, c), case, c)
    assert mask.sum(axis=1).tolist() == [1, 1] and (mask[:, 7] == 1).all()
    assert np.array_equal(mi, case[0]) and (ml == 7).all() and (mw == 1).all()
    # all keys equal: the smaller class indices win
    case = _mix_case(n, h, w, c, 7, equal_keys=True)
    mi, ml, mw, mask, count, nconf = _check_mix(_run_mix(case, c), case, c)
    for i in range(n):
        present = np.nonzero(count[i] > 0)[0]
        assert np.array_equal(np.nonzero(mask[i])[0], present[:(len(present) + 1) // 2])
    # another ignore label
    case = _mix_case(n, h, w, c, 8)
    mi, ml, mw, mask, count, nconf = _check_mix(_run_mix(case, c, ignore_label=250), case, c, ignore_label=250)
    assert (ml == 250).any() and not (ml == 255).any()


def test_classmix_confidence_threshold_edges():
    """conf exactly tau counts, one ulp below does not, a NaN does not."""
    below = np.nextafter(TAU, np.float32(0))
    xs, lab, xt, pred, conf, keys = _mix_case(1, 2, 4, 19, 9, labels="ignore")
    conf[:] = np.array([[TAU, below, np.nan, 1.0], [0.0, TAU, below, np.inf]], dtype=np.float32)
    case = (xs, lab, xt, pred, conf, keys)
    mi, ml, mw, mask, count, nconf = _check_mix(_run_mix(case, 19), case, 19)
    assert nconf.tolist() == [4] and (mw == np.float32(0.5)).all()
    conf[:] = below
    assert _check_mix(_run_mix(case, 19), case, 19)[5].tolist() == [0]
    conf[:] = np.nan
    out = _check_mix(_run_mix(case, 19), case, 19)
    assert out[5].tolist() == [0] and (out[2] == 0).all()


def test_classmix_layouts_give_the_same_bits():
    n, h, w, c = 2, 40, 52, 19
    case = _mix_case(n, h, w, c, 11)
    base = _run_mix(case, c)

    def strided(t):
        xs, lab, xt, pred, conf = t
        big = torch.zeros(n, h, w + 3, dtype=pred.dtype, device=DEV)
        big[:, :, 1:w + 1] = pred
        return [xs.contiguous(memory_format=torch.channels_last), lab.transpose(1, 2).contiguous().transpose(1, 2),
                xt.contiguous(memory_format=torch.channels_last), big[:, :, 1:w + 1],
                conf.transpose(1, 2).contiguous().transpose(1, 2)]
    other = _run_mix(case, c, layout=strided)
    for a, b in zip(base, other):
        assert a.dtype == b.dtype and torch.equal(_bits(a) if a.dtype == torch.float32 else a.cpu(),
                                                  _bits(b) if b.dtype == torch.float32 else b.cpu())
    _check_mix(other, case, c)
    with pytest.raises(ValueError, match="sizes must agree"):
        _run_mix((case[0], case[1], case[2][:, :, :-1], case[3], case[4], case[5]), c)


# ---- C. pixel-weighted cross entropy ------------------------------------------------------------------
def _wce_closed(x, lab, pw, cw, ignore=255):
    """x [rows, C] fp64 (a leaf), lab [rows], pw [rows] fp64, cw [C] fp64 or None -> (num, den) fp64."""
    c = x.shape[1]
    keep = (lab >= 0) & (lab != ignore) & (lab < c)
    nll = F.cross_entropy(x[keep], lab[keep], reduction="none")
    wt = cw[lab[keep]] if cw is not None else torch.ones_like(nll)
    return (pw[keep] * wt * nll).sum(), wt.sum()


@functools.lru_cache(maxsize=None)
def _ce_case(c, rows, weighted):
    g = torch.Generator().manual_seed(1000 * c + rows)
    x = (torch.randn(rows, c, generator=g, dtype=torch.float64) * 3).float()
    lab = torch.randint(0, c, (rows,), generator=g)
    if rows > 8:
        lab[torch.rand(rows, generator=g) < 0.1] = 255
        lab[3] = -1
        lab[5] = c + 2
        lab[rows - 1] = c - 1
    pw = torch.rand(rows, generator=g, dtype=torch.float64).float()
    if rows > 8:
        pw[1], pw[2] = 0.0, 1.0
    cw = (0.5 + torch.rand(c, generator=g, dtype=torch.float64)).float() if weighted else None
    ref = {}
    for red in ("mean", "sum", "mean_or_zero"):
        xr = x.double().requires_grad_(True)
        num, den = _wce_closed(xr, lab, pw.double(), None if cw is None else cw.double())
        loss = num if red == "sum" else num / den
        loss.backward(torch.tensor(0.7, dtype=torch.float64))
        ref[red] = (float(loss.detach()), xr.grad.clone())
    return x, lab, pw, cw, ref


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "class-weights"])
@pytest.mark.parametrize("rows", [1, 257, 4097])
@pytest.mark.parametrize("c", [19, 33])
def test_weighted_ce_matches_the_fp64_closed_form(c, rows, weighted):
    from adaptsegnet_amd.functional import cross_entropy2d
    x, lab, pw, cw, ref = _ce_case(c, rows, weighted)
    shape = (1, 1, rows)
    xd = x.reshape(1, rows, c).permute(0, 2, 1).reshape(1, c, 1, rows).to(DEV)
    labd, pwd = lab.reshape(shape).to(DEV), pw.reshape(shape).to(DEV)
    cwd = None if cw is None else cw.to(DEV)
    for red in ("mean", "sum", "mean_or_zero"):
        lref, gref = ref[red]
        for layout in (torch.contiguous_format, torch.channels_last):
            xr = xd.detach().contiguous(memory_format=layout).clone().requires_grad_(True)
            loss = cross_entropy2d(xr, labd, 255, cwd, red, pixel_weight=pwd)
            loss.backward(torch.tensor(0.7, device=DEV))
            lv = float(loss.detach())
            got = xr.grad.permute(0, 2, 3, 1).reshape(rows, c)
            f = _frob(got, gref)
            print(f"C={c} rows={rows} {red}: loss hip={lv:.7f} fp64={lref:.7f}; grad rel-frob {f:.2e}")
            assert loss.dim() == 0 and abs(lv - lref) < 1e-5 * abs(lref), (red, lv, lref)
            assert f < 1e-5, (red, f)
            assert pwd.grad is None
    # pixel_weight=None is the call without the argument, bit for bit; all-ones weights give its gradient bit
    # for bit (the denominator holds no pixel weight) and its loss: bit for bit without class weights (1 * nll
    # is exact), to a rounding with them (the plain kernel may fuse cw * nll into its sum, the weighted one
    # rounds the product first)
    ones = torch.ones(shape, device=DEV)
    for red in ("mean", "sum", "mean_or_zero"):
        res = []
        for kw in (dict(), dict(pixel_weight=None), dict(pixel_weight=ones)):
            xr = xd.detach().clone().requires_grad_(True)
            loss = cross_entropy2d(xr, labd, 255, cwd, red, **kw)
            loss.backward(torch.tensor(0.7, device=DEV))
            res.append((loss.detach().reshape(1), xr.grad))
        assert _bits_equal(res[0][0], res[1][0]) and _bits_equal(res[0][1], res[1][1]), red
        assert _bits_equal(res[0][1], res[2][1]), red
        if cw is None:
            assert _bits_equal(res[0][0], res[2][0]), red
        else:
            assert abs(float(res[0][0]) - float(res[2][0])) <= 4 * EPS * abs(float(res[0][0])), red


@pytest.mark.parametrize("c", [19, 33])
def test_weighted_ce_zero_weights_and_all_ignored(c):
    from adaptsegnet_amd import kernels as K
    from adaptsegnet_amd.functional import cross_entropy2d
    x, lab, pw, cw, _ = _ce_case(c, 257, True)
    xd = x.reshape(1, 257, c).permute(0, 2, 1).reshape(1, c, 1, 257).to(DEV)
    labd = lab.reshape(1, 1, 257).to(DEV)
    for red in ("mean", "sum", "mean_or_zero"):
        xr = xd.clone().requires_grad_(True)
        loss = cross_entropy2d(xr, labd, 255, cw.to(DEV), red, pixel_weight=torch.zeros(1, 1, 257, device=DEV))
        loss.backward()
        assert float(loss.detach()) == 0.0 and float(xr.grad.abs().max()) == 0.0, red
    xr = xd.clone().requires_grad_(True)
    ignored = torch.full_like(labd, 255)
    loss = cross_entropy2d(xr, ignored, 255, None, "mean_or_zero", pixel_weight=pw.reshape(1, 1, 257).to(DEV))
    loss.backward()
    assert float(loss.detach()) == 0.0 and float(xr.grad.abs().max()) == 0.0
    assert float(cross_entropy2d(xd, ignored, 255, None, "sum", pixel_weight=pw.reshape(1, 1, 257).to(DEV))) == 0.0
    assert math.isnan(float(cross_entropy2d(xd, ignored, 255, None, "mean", pixel_weight=pw.reshape(1, 1, 257).to(DEV))))
    # accumulate = a plain launch + an add; runs repeat
    xv, pwd, gl = K.nhwc_view(xd), pw.to(DEV), torch.tensor([0.7], device=DEV)
    out = K.ce_fwd(xv, labd, 255, None, pwd)
    assert _bits_equal(out, K.ce_fwd(xv, labd, 255, None, pwd))
    dl = K.ce_bwd(xv, labd, out, gl, pixel_weight=pwd)
    d0 = torch.randn(xv.shape, generator=torch.Generator().manual_seed(5)).to(DEV)
    assert _bits_equal(K.ce_bwd(xv, labd, out, gl, dl=d0.clone(), accumulate=True, pixel_weight=pwd), d0 + dl)
    with pytest.raises(RuntimeError, match="pixel_weight"):
        cross_entropy2d(xd, labd, pixel_weight=torch.zeros(1, 257, device=DEV))
    with pytest.raises(RuntimeError, match="pixel_weight"):
        cross_entropy2d(xd, labd, pixel_weight=torch.zeros(1, 1, 257, device=DEV, dtype=torch.float64))


# ---- D. the step against the fp64 oracle -------------------------------------------------------------
CFG = dict(input_size=(57, 41), input_size_target=(49, 33))
LEVEL_GAN = [("single-level", "Vanilla"), ("multi-level", "LS"), ("source-only", "Vanilla")]


@functools.lru_cache(maxsize=None)
def _data():
    """tests/test_entropy_gpu.py's data, and a mixed triple made by tests/classmix_ref.py from R.det_images /
    R.det_labels (no teacher: no argmax tie can flip a label between fp32 and fp64)."""
    xs = torch.from_numpy(R.det_images((2, 3, 41, 57), 11))
    lab = torch.from_numpy(R.det_labels((2, 41, 57), 12))
    xt = torch.from_numpy(R.det_images((2, 3, 33, 49), 13))
    lt = {"single-level": torch.from_numpy(R.det_labels((2, 41, 57), 14, ignore_frac=0.5)),
          "multi-level": torch.from_numpy(R.det_labels((2, 33, 49), 14, ignore_frac=0.5))}
    xt_mix = R.det_images((2, 3, 41, 57), 15).astype(np.float32)
    pred = R.det_labels((2, 41, 57), 16).astype(np.uint8)            # 255: not a class -> ignore_label
    rng = np.random.Generator(np.random.PCG64(17))
    conf = rng.uniform(0, 1, (2, 41, 57)).astype(np.float32)
    keys = rng.integers(0, 1 << 32, (2, 19), dtype=np.uint32)
    mi, ml, mw, mask, _, nconf = CR.classmix(xs.numpy().astype(np.float32), lab.numpy(), xt_mix, pred, conf, keys, 19,
                                             np.float32(0.6), 255)
    assert 0 < mask.sum() < mask.size and (ml == 255).any() and (mw == 1).any() and ((mw > 0.3) & (mw < 0.5)).any()
    mixed = (torch.from_numpy(mi), torch.from_numpy(ml), torch.from_numpy(mw))
    return xs, lab, xt, lt, mixed


def _selfinfo_torch(x):
    logp = F.log_softmax(x, dim=1)
    return -(logp.exp() * logp) / math.log(x.shape[1])


def _entropy_torch(x):
    return _selfinfo_torch(x).sum(dim=1).mean()


def _wce_torch(pred, ml, mw):
    """sum_i pw_i nll_i / #valid (0 when none is valid): cross_entropy2d(..., 'mean_or_zero', pixel_weight)."""
    nll = F.cross_entropy(pred, ml, ignore_index=255, reduction="none")
    valid = ((ml >= 0) & (ml != 255)).sum()
    return (nll * mw.to(nll.dtype)).sum() / valid if int(valid) else nll.sum() * 0


@functools.lru_cache(maxsize=None)
def _oracle_step(level, gan, dtype, lambda_mix=1.0, lambda_ent=0.0, lambda_st=0.0, d_input="softmax"):
    """tests/test_entropy_gpu.py's ``_oracle_step`` (eval-mode BN, iter_size 1) with the mixed branch after the
    target branch's backward, and a source-only level.  Returns (G, losses); computed once per argument set."""
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    xs, lab, xt, lt, mixed = _data()
    xs, xt = xs.to(dtype), xt.to(dtype)
    mi, ml, mw = mixed[0].to(dtype), mixed[1], mixed[2].to(dtype)
    c = R.DEFAULT_CFG | CFG | dict(level=level, gan=gan)
    din = _selfinfo_torch if d_input == "entropy" else (lambda t: F.softmax(t, dim=1))
    G = R.to_torch(_state("g", 1338), dtype=dtype, trainable=R.g_trainable)
    D1 = R.to_torch(_state("d", 2001), dtype=dtype, trainable=lambda k: True)
    D2 = R.to_torch(_state("d", 2002), dtype=dtype, trainable=lambda k: True)
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
                                (lambda_ent, "ent", _entropy_torch)):
            if lam > 0:
                for _, h in Ds:
                    v = term(pts[h])
                    total = total + (lam if h == 2 else c["lambda_seg"] * lam) * v
                    vals[f"loss_{name}{h}"] = v.item()
        total.backward()
        for _, h in Ds:
            vals[f"loss_adv_target{h}"] = advl[h].item()
    if lambda_mix > 0:   # the mixed branch: a third forward, the confidence-weighted CE
        pm = dict(zip((1, 2), fwd(mi, c["input_size"])))
        total = 0
        for _, h in Ds:
            v = _wce_torch(pm[h], ml, mw)
            total = total + (lambda_mix if h == 2 else c["lambda_seg"] * lambda_mix) * v
            vals[f"loss_mix{h}"] = v.item()
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


def _trainer(level, gan, bn_train=False, gen="multi", **cfg):
    from adaptsegnet_amd.model import DeeplabMulti, DeeplabVGG, FCDiscriminator
    from adaptsegnet_amd.train import AdaptSegTrainer, StepConfig
    m = _load(DeeplabMulti(19), _state("g", 1338)) if gen == "multi" else _load(DeeplabVGG(19), _state("vgg", 4242))
    d1 = _load(FCDiscriminator(19), _state("d", 2001)) if level == "multi-level" else None
    d2 = _load(FCDiscriminator(19), _state("d", 2002)) if level != "source-only" else None
    m.train(bn_train)
    return AdaptSegTrainer(m, d1, d2, StepConfig(**(CFG | dict(level=level, gan=gan) | cfg))), m, d1, d2


def _batch(level, with_labels_t=False, mixed=True, ignore_mixed=False):
    xs, lab, xt, lt, mx = _data()
    b = (xs.float().to(DEV), lab.to(DEV))
    if level != "source-only":
        b += (xt.float().to(DEV),)
        if with_labels_t:
            b += (lt[level].to(DEV),)
    if mixed:
        ml = torch.full_like(mx[1], 255) if ignore_mixed else mx[1]
        b += (mx[0].to(DEV), ml.to(DEV), mx[2].to(DEV))
    return b


def _updates(level, G, G32, m):
    """{group: (rel-Frobenius of the HIP update to the fp64 one, of the fp32 oracle's to the fp64 one)}."""
    g0, sd = _state("g", 1338), m.state_dict()
    groups = {"trunk": [], "heads": []}
    for k, v in G.items():
        if v.dtype.is_floating_point and v.requires_grad and not (k.startswith("layer5") and level != "multi-level"):
            groups["heads" if k.startswith(("layer5", "layer6")) else "trunk"].append(k)
    out = {}
    for name, keys in groups.items():
        upd = lambda P: torch.cat([(P[k].detach().double().cpu() - torch.from_numpy(g0[k])).flatten()  # noqa: E731
                                   for k in keys])
        dref = upd(G)
        out[name] = (_frob(upd(sd), dref), _frob(upd(G32), dref))
    return out


def _check_losses(tag, got, ref):
    assert set(got) == set(ref), (sorted(got), sorted(ref))
    for k, v in ref.items():
        print(f"{tag} {k}: hip={got[k]:.7f} fp64={v:.7f}")
    for k, v in ref.items():
        assert abs(got[k] - v) <= 1e-4 * abs(v) + 1e-7, (k, got[k], v)


def _check_step(tag, level, gan, with_labels_t=False, **kw):
    G, ref = _oracle_step(level, gan, torch.float64, **kw)
    G32, _ = _oracle_step(level, gan, torch.float32, **kw)
    tr, m, _, _ = _trainer(level, gan, **kw)
    got = tr.step(0, [_batch(level, with_labels_t)]).values()
    assert "loss_mix2" in got and ("loss_mix1" in got) == (level == "multi-level")
    assert ref["loss_mix2"] > 0.5
    _check_losses(tag, got, ref)
    for name, (f, f32) in _updates(level, G, G32, m).items():
        print(f"{tag} {name} update: rel-frob {f:.3e} (fp32 oracle {f32:.3e})")
        assert f <= 2 * f32 + 1e-4, (name, f, f32)


@pytest.mark.parametrize("level,gan", LEVEL_GAN)
def test_mixed_term_step_matches_fp64_oracle(level, gan):
    _check_step(f"lambda_mix=1 {level}", level, gan, lambda_mix=1.0)


def test_all_options_together_match_fp64_oracle():
    _check_step("mix+st+ent+entropy-D", "single-level", "Vanilla", with_labels_t=True, lambda_mix=1.0, lambda_st=1.0,
                lambda_ent=1.0, d_input="entropy")


@pytest.mark.parametrize("level,gan", LEVEL_GAN)
def test_all_ignored_mixed_labels_leave_the_step_as_it_was(level, gan):
    tr, m, d1, d2 = _trainer(level, gan, lambda_mix=1.0)
    got = tr.step(0, [_batch(level, ignore_mixed=True)]).values()
    tr0, m0, d10, d20 = _trainer(level, gan)
    want = tr0.step(0, [_batch(level, mixed=False)]).values()
    torch.cuda.synchronize()
    assert got["loss_mix2"] == 0.0 and got.get("loss_mix1", 0.0) == 0.0
    assert {k: v for k, v in got.items() if not k.startswith("loss_mix")} == want
    for a, b in ((m, m0), (d1, d10), (d2, d20)):
        if a is not None:
            sa, sb = a.state_dict(), b.state_dict()
            for k in sa:
                assert torch.equal(sa[k], sb[k]), k


def _run(level, gan, steps=2, gen="multi", batch=None, **cfg):
    tr, m, d1, d2 = _trainer(level, gan, bn_train=True, gen=gen, **cfg)
    batch = batch if batch is not None else _batch(level)
    losses = [tr.step(it, [batch]).values() for it in range(steps)]
    torch.cuda.synchronize()
    return losses, [{k: v.detach().cpu().clone() for k, v in mm.state_dict().items()}
                    for mm in (m, d1, d2) if mm is not None]


def _same_runs(a, b, tag):
    assert a[0] == b[0], (tag, a[0], b[0])
    for sa, sb in zip(a[1], b[1]):
        for k in sa:
            assert torch.equal(sa[k], sb[k]), (tag, k)


PATHS = {
    "single-level": [dict(overlap_domains=False), dict(overlap_domains=True),
                     dict(overlap_domains=True, target_first=True), dict(overlap_domains=True, overlap_d=True)],
    "multi-level": [dict(overlap_domains=False), dict(overlap_domains=True, overlap_d=True, target_first=True)],
}


@pytest.mark.parametrize("level,gan", LEVEL_GAN[:2])
def test_stream_orders_are_bit_identical_with_the_mixed_branch(level, gan):
    runs = [_run(level, gan, lambda_mix=1.0, **p) for p in PATHS[level]]
    assert runs[0][0][0]["loss_mix2"] > 0 and runs[0][0][1]["loss_mix2"] != runs[0][0][0]["loss_mix2"]
    for r, p in zip(runs[1:], PATHS[level][1:]):
        _same_runs(runs[0], r, p)


def test_default_is_the_step_as_it_was():
    _same_runs(_run("single-level", "Vanilla", steps=1, batch=_batch("single-level", mixed=False)),
               _run("single-level", "Vanilla", steps=1, batch=_batch("single-level", mixed=False), lambda_mix=0.0),
               "lambda_mix=0")


def test_single_map_generator_takes_the_mixed_term():
    xs = torch.from_numpy(R.det_images((1, 3, 40, 56), 3)).float().to(DEV)
    lab = torch.from_numpy(R.det_labels((1, 40, 56), 4)).to(DEV)
    case = _mix_case(1, 40, 56, 19, 21)
    mi, ml, mw, _, _, _ = CR.classmix(xs.cpu().numpy(), lab.cpu().numpy(), *case[2:], 19, np.float32(0.9), 255)
    mixed = tuple(torch.from_numpy(a).to(DEV) for a in (mi, ml, mw))
    tr, m, _, _ = _trainer("single-level", "Vanilla", gen="vgg", lambda_mix=1.0, input_size=(56, 40),
                           input_size_target=(56, 40))
    with torch.no_grad():
        up = F.interpolate(m(mixed[0]), size=(40, 56), mode="bilinear", align_corners=True).double()
        want = float(_wce_torch(up, mixed[1], mixed[2].double()))
    vals = tr.step(0, [(xs, lab, xs) + mixed]).values()
    assert "loss_mix2" in vals and all(math.isfinite(v) for v in vals.values()), vals
    assert want > 0 and abs(vals["loss_mix2"] - want) <= 1e-5 * want, (vals, want)
    assert all(torch.isfinite(v.double()).all() for v in m.state_dict().values())


# ---- E. end to end --------------------------------------------------------------------------------------
def _end_to_end():
    from adaptsegnet_amd.mix import ClassMixSampler, EmaTeacher
    from adaptsegnet_amd.model import DeeplabMulti
    tr, m, _, d2 = _trainer("single-level", "Vanilla", bn_train=True, lambda_mix=1.0, input_size_target=(57, 41))
    ema = EmaTeacher(_load(DeeplabMulti(19), _state("g", 1338)), alpha=0.99)
    sampler = ClassMixSampler(seed=3)
    xs, lab, _, _, _ = _data()
    xs, lab = xs.float().to(DEV), lab.to(DEV)
    xt = torch.from_numpy(R.det_images((2, 3, 41, 57), 15)).float().to(DEV)
    # tau: the median of the (randomly initialised) teacher's confidences, so that about half of them count
    tau = float(ema.predict(xt, (57, 41))[1].median())
    losses, weights = [], []
    for it in range(2):
        mixed = ema.mix(xs, lab, xt, sampler, tau=tau)
        assert mixed[0].shape == xs.shape and mixed[1].dtype == torch.int64 and mixed[2].dtype == torch.float32
        weights.append(mixed[2].detach().cpu().clone())
        losses.append(tr.step(it, [(xs, lab, xt) + tuple(mixed)]).values())
        ema.update(m, it)
    torch.cuda.synchronize()
    states = [{k: v.detach().cpu().clone() for k, v in mm.state_dict().items()} for mm in (m, d2, ema.teacher)]
    return losses, states, weights


def test_end_to_end_two_iterations_repeat_bit_for_bit():
    a, b = _end_to_end(), _end_to_end()
    losses, states, weights = a
    assert all(math.isfinite(v) for vals in losses for v in vals.values()), losses
    assert all("loss_mix2" in vals for vals in losses)
    for w in weights:
        assert float(w.min()) >= 0.0 and float(w.max()) <= 1.0
        assert (w == 1).any()                      # pasted source pixels
    assert ((weights[0] > 0) & (weights[0] < 1)).any()   # target pixels at q: iteration 0's tau is its median
    # after update(m, 0) the teacher was the student; one more step and update moved it half way
    assert not all(torch.equal(states[0][k], states[2][k]) for k in states[0] if states[0][k].dtype.is_floating_point)
    _same_runs((a[0], a[1]), (b[0], b[1]), "end to end")
    for wa, wb in zip(a[2], b[2]):
        assert torch.equal(wa, wb)
