"""Entropy-based adaptation on the GPU: the selfinfo / entropy-loss kernels and the two StepConfig options.

A. The four kernels against the closed forms of DESIGN.md evaluated in fp64 on the CPU (cross-checked
   here against fp64 autograd of entr(softmax(x)) / ln C on the rows where no p underflows: autograd
   gives NaN on the others): C on both sides of the LDS-tile limit (32 | 33), row counts around one
   256-row tile, planted rows (all-equal, one-hot at +200, entries at -1e4, a -inf entry).
   rel-Frobenius < 1e-5 and |loss - ref| < 1e-5 |ref|, the bound tests/test_ops_gpu.py holds the
   softmax / CE kernels of the same structure to.
B. The block loops (more rows than one sweep of the grid), accumulate = a plain launch + an add,
   run-to-run bits, NCHW-contiguous = channels_last input.
C. The autograd Functions keep nothing but the logits' own storage.
D. adv_loss(D(selfinfo2d(logits))) through the HIP discriminator against the fp64 oracle.
E. The step with lambda_ent = 1 against an fp64 oracle composed here from oracle.reference_torch
   (tests/test_pseudo_gpu.py's composition with the entropy term in the CE term's place); bounds as there.
F. The step with d_input="entropy": the heads' update at lambda_adv_target2 = 1 (at the default 0.001
   the discriminator input moves the update by 1e-6, below fp32 noise), and the wiring, counted exactly.
G. The defaults are the step as it was, bit for bit; the stream orders of the target branch agree.
"""
import functools
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import reference_torch as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _frob(a, b):
    a, b = a.detach().double().cpu().flatten(), b.detach().double().cpu().flatten()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.detach().contiguous().view(torch.int32),
                                              b.detach().contiguous().view(torch.int32))


# ---- the closed forms, fp64 ---------------------------------------------------------------------
def _closed(x, dy=None, g=None):
    """x [rows, C] fp64 -> dict(y, loss, H[, dx (map backward of dy)][, dl (loss backward of g)])."""
    rows, c = x.shape
    k = 1.0 / math.log(c)
    m = x.max(dim=1, keepdim=True).values
    lse = m + torch.log(torch.exp(x - m).sum(dim=1, keepdim=True))
    logp = x - lse
    p = torch.exp(logp)
    plp = torch.where(p == 0, torch.zeros_like(p), p * torch.where(p == 0, torch.zeros_like(p), logp))
    h = -plp.sum(dim=1)
    out = dict(y=-k * plp, H=h, loss=k * h.mean(), p=p)
    if dy is not None:
        t = -k * dy * (plp + p)
        out["dx"] = t - p * t.sum(dim=1, keepdim=True)
    if g is not None:
        out["dl"] = -(g * k / rows) * (plp + p * h[:, None])
    return out


SHAPES = [(1,), (255,), (256,), (257,), (2, 33, 41)]
CS = [2, 19, 32, 33]   # 32: the last LDS-tiled size, 33: the first per-thread-row size
G_LOSS = 0.7


@functools.lru_cache(maxsize=None)
def _case(c, shape):
    """(x fp32 [*shape, c], dy fp32, planted row indices by name, fp64 reference), made once."""
    g = torch.Generator().manual_seed(1000 * c + int(np.prod(shape)))
    rows = int(np.prod(shape))
    x = torch.randn(rows, c, generator=g, dtype=torch.float64) * 3
    planted = {}
    if rows >= 8:   # first rows of the first tile and the last row of the last
        planted = {"equal": 0, "onehot": 1, "low": 2, "inf": rows - 1}
        x[0] = 0.7
        x[1] = 0.0
        x[1, c // 2] = 200.0
        x[2, 0] = -1e4
        x[2, c - 1 if c > 2 else 0] = -1e4
        x[rows - 1, 1] = -math.inf
    x = x.float()
    dy = torch.randn(rows, c, generator=g, dtype=torch.float64).float()
    ref = _closed(x.double(), dy.double(), G_LOSS)
    # the closed forms against fp64 autograd, on the rows autograd can do (no p == 0)
    clean = (ref["p"] > 0).all(dim=1)
    assert int(clean.sum()) >= rows - 3
    xa = x.double()[clean].requires_grad_(True)
    ya = torch.special.entr(F.softmax(xa, dim=1)) / math.log(c)
    gx, = torch.autograd.grad(ya, xa, dy.double()[clean], retain_graph=True)
    gl, = torch.autograd.grad(ya.sum(dim=1).mean(), xa, torch.tensor(G_LOSS, dtype=torch.float64))
    sub = _closed(x.double()[clean], dy.double()[clean], G_LOSS)
    assert (ya.detach() - sub["y"]).abs().max() <= 1e-12 and (gx - sub["dx"]).abs().max() <= 1e-12
    assert abs(float(ya.detach().sum(dim=1).mean()) - float(sub["loss"])) <= 1e-12
    assert (gl - sub["dl"]).abs().max() <= 1e-12
    return x.reshape(*shape, c), dy.reshape(*shape, c), planted, ref


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("c", CS)
def test_ops_match_the_fp64_closed_forms(c, shape):
    from adaptsegnet_amd import kernels as K
    x, dy, planted, ref = _case(c, shape)
    xd, dyd = x.to(DEV), dy.to(DEV)
    gl = torch.tensor([G_LOSS], device=DEV)
    y = K.selfinfo_fwd(xd).cpu().reshape(-1, c)
    dx = K.selfinfo_bwd(xd, dyd).cpu().reshape(-1, c)
    loss = float(K.entropy_fwd(xd).cpu()[0])
    dl = K.entropy_bwd(xd, gl).cpu().reshape(-1, c)
    fy, fdx, fdl = _frob(y, ref["y"]), _frob(dx, ref["dx"]), _frob(dl, ref["dl"])
    lref = float(ref["loss"])
    print(f"C={c} rows={y.shape[0]}: y {fy:.2e} dx {fdx:.2e} dloss {fdl:.2e} loss {abs(loss - lref) / abs(lref):.2e}")
    assert fy < 1e-5 and fdx < 1e-5 and fdl < 1e-5, (fy, fdx, fdl)
    assert abs(loss - lref) < 1e-5 * abs(lref), (loss, lref)
    for t in (y, dx, dl):
        assert torch.isfinite(t).all()
    assert math.isfinite(loss)
    if planted:
        r = planted["onehot"]
        assert (y[r] == 0).all() and (dx[r] == 0).all() and (dl[r] == 0).all(), (y[r], dx[r], dl[r])
        r = planted["equal"]
        assert (y[r] - 1.0 / c).abs().max() <= 1e-6, y[r]


@pytest.mark.parametrize("c", CS)
def test_uniform_rows_have_entropy_one(c):
    from adaptsegnet_amd import kernels as K
    x = torch.full((300, c), -2.5, device=DEV)
    assert abs(float(K.entropy_fwd(x).cpu()[0]) - 1.0) <= 1e-6
    assert (K.selfinfo_fwd(x).cpu() - 1.0 / c).abs().max() <= 1e-6
    onehot = torch.zeros((300, c), device=DEV)
    onehot[:, c - 1] = 200.0
    assert float(K.entropy_fwd(onehot).cpu()[0]) == 0.0


# ---- B. loops, accumulate, bits --------------------------------------------------------------------
def test_map_kernels_loop_over_more_rows_than_one_grid_sweep():
    from adaptsegnet_amd import kernels as K
    rows, c = 8192 * 256 + 257, 2   # the grid is capped at 8192 blocks of 256 rows
    g = torch.Generator().manual_seed(77)
    x = (torch.randn(rows, c, generator=g) * 3)
    dy = torch.randn(rows, c, generator=g)
    ref = _closed(x.double(), dy.double(), G_LOSS)
    xd, dyd = x.to(DEV), dy.to(DEV)
    y, dx = K.selfinfo_fwd(xd), K.selfinfo_bwd(xd, dyd)
    assert _frob(y, ref["y"]) < 1e-5 and _frob(dx, ref["dx"]) < 1e-5
    assert _frob(y[-300:], ref["y"][-300:]) < 1e-5 and _frob(dx[-300:], ref["dx"][-300:]) < 1e-5
    assert _bits_equal(y, K.selfinfo_fwd(xd)) and _bits_equal(dx, K.selfinfo_bwd(xd, dyd))
    dx0 = torch.randn(rows, c, generator=g).to(DEV)
    acc = K.selfinfo_bwd(xd, dyd, out=dx0.clone(), accumulate=True)
    assert _bits_equal(acc, dx0 + dx)
    gl = torch.tensor([G_LOSS], device=DEV)
    dl = K.entropy_bwd(xd, gl)
    assert _frob(dl, ref["dl"]) < 1e-5
    assert _bits_equal(K.entropy_bwd(xd, gl, dx=dx0.clone(), accumulate=True), dx0 + dl)
    loss = K.entropy_fwd(xd)
    assert abs(float(loss.cpu()[0]) - float(ref["loss"])) < 1e-5 * float(ref["loss"])
    assert _bits_equal(loss, K.entropy_fwd(xd))


@pytest.mark.parametrize("c", [19, 33])
def test_loss_kernel_loops_at_4097_rows(c):
    import ctypes
    from adaptsegnet_amd import _lib
    from adaptsegnet_amd import kernels as K
    rows = 4097
    b = ctypes.c_size_t(0)
    assert _lib.lib().adaptseg_entropy_workspace_size(rows, ctypes.byref(b)) == 0
    assert (b.value // 8) * 256 < rows   # fewer blocks than row tiles: every block loops
    g = torch.Generator().manual_seed(78)
    x = torch.randn(rows, c, generator=g) * 3
    ref = _closed(x.double())
    xd = x.to(DEV)
    loss = K.entropy_fwd(xd)
    assert abs(float(loss.cpu()[0]) - float(ref["loss"])) < 1e-5 * float(ref["loss"])
    assert _bits_equal(loss, K.entropy_fwd(xd))


@pytest.mark.parametrize("c", CS)
def test_accumulate_is_a_launch_plus_an_add_and_runs_repeat(c):
    from adaptsegnet_amd import kernels as K
    x, dy, _, _ = _case(c, (2, 33, 41))
    xd, dyd = x.to(DEV), dy.to(DEV)
    gl = torch.tensor([G_LOSS], device=DEV)
    dx0 = torch.randn(x.shape, generator=torch.Generator().manual_seed(5)).to(DEV)
    dx, dl = K.selfinfo_bwd(xd, dyd), K.entropy_bwd(xd, gl)
    assert _bits_equal(K.selfinfo_bwd(xd, dyd, out=dx0.clone(), accumulate=True), dx0 + dx)
    assert _bits_equal(K.entropy_bwd(xd, gl, dx=dx0.clone(), accumulate=True), dx0 + dl)
    assert _bits_equal(K.selfinfo_fwd(xd), K.selfinfo_fwd(xd))
    assert _bits_equal(dx, K.selfinfo_bwd(xd, dyd)) and _bits_equal(dl, K.entropy_bwd(xd, gl))
    assert _bits_equal(K.entropy_fwd(xd), K.entropy_fwd(xd))


def _fn_results(x, gy):
    """selfinfo2d / entropy_loss2d of the NCHW-shaped x: (map, map gradient of gy, loss, loss gradient)."""
    from adaptsegnet_amd.functional import entropy_loss2d, selfinfo2d
    x = x.detach().requires_grad_(True)
    y = selfinfo2d(x)
    gx, = torch.autograd.grad(y, x, gy)
    loss = entropy_loss2d(x)
    gl, = torch.autograd.grad(loss, x)
    return [t.detach().contiguous() for t in (y, gx, loss.reshape(1), gl)]


def test_nchw_and_channels_last_inputs_give_the_same_bits():
    g = torch.Generator().manual_seed(9)
    x = (torch.randn(2, 19, 33, 41, generator=g) * 3).to(DEV)
    gy = torch.randn(2, 19, 33, 41, generator=g).to(DEV)
    a = _fn_results(x.contiguous(), gy)
    b = _fn_results(x.contiguous(memory_format=torch.channels_last), gy.contiguous(memory_format=torch.channels_last))
    assert a[2].dim() == 1 and a[0].shape == x.shape
    for u, v in zip(a, b):
        assert _bits_equal(u, v)
    ref = _closed(x.permute(0, 2, 3, 1).reshape(-1, 19).double().cpu(),
                  gy.permute(0, 2, 3, 1).reshape(-1, 19).double().cpu(), 1.0)
    assert _frob(a[0].permute(0, 2, 3, 1).reshape(-1, 19), ref["y"]) < 1e-5
    assert _frob(a[1].permute(0, 2, 3, 1).reshape(-1, 19), ref["dx"]) < 1e-5
    assert _frob(a[3].permute(0, 2, 3, 1).reshape(-1, 19), ref["dl"]) < 1e-5


# ---- C. saved state --------------------------------------------------------------------------------
def test_functions_save_only_the_logits():
    from adaptsegnet_amd.functional import entropy_loss2d, selfinfo2d
    x = torch.randn(2, 19, 9, 11, device=DEV).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    for out in (selfinfo2d(x), entropy_loss2d(x)):
        saved = out.grad_fn.saved_tensors
        assert len(saved) == 1
        for t in saved:
            assert t.untyped_storage().data_ptr() == x.untyped_storage().data_ptr()
            assert t.numel() == x.numel()
    assert entropy_loss2d(x).dim() == 0


# ---- D. the adversarial branch through D ----------------------------------------------------------------
def _load(model, state):
    model.load_state_dict({k: torch.from_numpy(v.copy()) if v.dtype == np.int64 else torch.from_numpy(v.copy()).float()
                           for k, v in state.items()})
    return model.to(DEV)


@functools.lru_cache(maxsize=None)
def _state(kind, seed):
    return R.det_state({"g": R.g_specs, "d": R.d_specs, "vgg": R.vgg_specs}[kind](), seed)


def _selfinfo_torch(x):
    """The closed-form map with torch ops (differentiable; for predictions without underflow)."""
    logp = F.log_softmax(x, dim=1)
    return -(logp.exp() * logp) / math.log(x.shape[1])


def _entropy_torch(x):
    return _selfinfo_torch(x).sum(dim=1).mean()


@pytest.mark.parametrize("gan", ["Vanilla", "LS"])
def test_adversarial_loss_through_the_discriminator(gan):
    from adaptsegnet_amd import functional as AF
    from adaptsegnet_amd.model import FCDiscriminator
    g = torch.Generator().manual_seed(21)
    logits = (torch.randn(2, 19, 33, 49, generator=g, dtype=torch.float64) * 3).float()
    res = {}
    for dtype in (torch.float64, torch.float32):
        D = R.to_torch(_state("d", 2002), dtype=dtype, trainable=lambda k: False)
        xr = logits.clone().to(dtype).requires_grad_(True)   # (a copy: .to(float32) alone is logits itself)
        loss = R.adv_loss(R.d_forward(D, _selfinfo_torch(xr)), 0, gan)
        loss.backward()
        res[dtype] = (float(loss.detach()), xr.grad.double())
    d = _load(FCDiscriminator(19), _state("d", 2002))
    for p in d.parameters():
        p.requires_grad = False
    xd = logits.to(DEV).requires_grad_(True)
    loss = AF.adv_loss(d(AF.selfinfo2d(xd)), 0.0, AF.BCE if gan == "Vanilla" else AF.MSE)
    loss.backward()
    lref, gref = res[torch.float64]
    f, f32 = _frob(xd.grad, gref), _frob(res[torch.float32][1], gref)
    lv = float(loss.detach())
    print(f"D({gan}) through selfinfo2d: loss hip={lv:.7f} fp64={lref:.7f}; grad rel-frob {f:.3e} "
          f"(fp32 oracle {f32:.3e})")
    assert abs(lv - lref) <= 1e-5 * abs(lref), (lv, lref)
    assert f <= 2 * f32 + 1e-5, (f, f32)


# ---- E / F. the step against the fp64 oracle ------------------------------------------------------------
CFG = dict(input_size=(57, 41), input_size_target=(49, 33))
LEVEL_GAN = [("single-level", "Vanilla"), ("multi-level", "LS")]


@functools.lru_cache(maxsize=None)
def _data():
    """The shapes of tests/test_pseudo_gpu.py's ``data``."""
    xs = torch.from_numpy(R.det_images((2, 3, 41, 57), 11))
    lab = torch.from_numpy(R.det_labels((2, 41, 57), 12))
    xt = torch.from_numpy(R.det_images((2, 3, 33, 49), 13))
    lt = {"single-level": torch.from_numpy(R.det_labels((2, 41, 57), 14, ignore_frac=0.5)),
          "multi-level": torch.from_numpy(R.det_labels((2, 33, 49), 14, ignore_frac=0.5))}
    return xs, lab, xt, lt


@functools.lru_cache(maxsize=None)
def _oracle_step(level, gan, dtype, lambda_ent=0.0, lambda_st=0.0, d_input="softmax", lambda_adv2=None):
    """One iteration in oracle.reference_torch.oracle_step's order (eval-mode BN, iter_size 1) with the
    entropy term (and the self-training CE term) added to the adversarial backward and the
    discriminators fed by ``d_input``.  Returns (G, losses); computed once per argument set."""
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    xs, lab, xt, lt = _data()
    xs, xt, lt = xs.to(dtype), xt.to(dtype), lt[level]
    c = R.DEFAULT_CFG | CFG | dict(level=level, gan=gan)
    if lambda_adv2 is not None:
        c["lambda_adv_target2"] = lambda_adv2
    din = _selfinfo_torch if d_input == "entropy" else (lambda t: F.softmax(t, dim=1))
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
    adv = {h: R.adv_loss(R.d_forward(D, din(pts[h])), 0, gan) for D, h in Ds}
    total = c["lambda_adv_target2"] * adv[2]
    if multi:
        total = total + c["lambda_adv_target1"] * adv[1]
    for lam, name, term in ((lambda_st, "st", lambda t: F.cross_entropy(t, lt, ignore_index=255)),
                            (lambda_ent, "ent", _entropy_torch)):
        if lam > 0:
            for _, h in Ds:
                v = term(pts[h])
                total = total + (lam if h == 2 else c["lambda_seg"] * lam) * v
                vals[f"loss_{name}{h}"] = v.item()
    total.backward()
    for _, h in Ds:
        vals[f"loss_seg{h}"], vals[f"loss_adv_target{h}"] = seg[h].item(), adv[h].item()
    rg(True)
    for src, lbl in ((preds, 0), (pts, 1)):
        for D, h in Ds:
            l_d = R.adv_loss(R.d_forward(D, din(src[h].detach())), lbl, gan) / 2
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


def _batch(level, with_labels_t=False):
    xs, lab, xt, lt = _data()
    b = (xs.float().to(DEV), lab.to(DEV), xt.float().to(DEV))
    return b + (lt[level].to(DEV),) if with_labels_t else b


def _updates(level, G, G32, m):
    """{group: (rel-Frobenius of the HIP update to the fp64 one, of the fp32 oracle's to the fp64 one)}."""
    g0, sd = _state("g", 1338), m.state_dict()
    groups = {"trunk": [], "heads": []}
    for k, v in G.items():
        if v.dtype.is_floating_point and v.requires_grad and not (k.startswith("layer5") and level == "single-level"):
            groups["heads" if k.startswith(("layer5", "layer6")) else "trunk"].append(k)
    out = {}
    for name, keys in groups.items():
        upd = lambda P: torch.cat([(P[k].detach().double().cpu() - torch.from_numpy(g0[k])).flatten()  # noqa: E731
                                   for k in keys])
        dref = upd(G)
        out[name] = (_frob(upd(sd), dref), _frob(upd(G32), dref), dref)
    return out


def _check_losses(tag, got, ref):
    assert set(got) == set(ref), (sorted(got), sorted(ref))
    for k, v in ref.items():
        print(f"{tag} {k}: hip={got[k]:.7f} fp64={v:.7f}")
    for k, v in ref.items():
        assert abs(got[k] - v) <= 1e-4 * abs(v) + 1e-7, (k, got[k], v)


@pytest.mark.parametrize("level,gan", LEVEL_GAN)
def test_entropy_term_step_matches_fp64_oracle(level, gan):
    G, ref = _oracle_step(level, gan, torch.float64, lambda_ent=1.0)
    G32, _ = _oracle_step(level, gan, torch.float32, lambda_ent=1.0)
    tr, m, _, _ = _trainer(level, gan, lambda_ent=1.0)
    got = tr.step(0, [_batch(level)]).values()
    assert "loss_ent2" in got and ("loss_ent1" in got) == (level == "multi-level")
    _check_losses(f"lambda_ent=1 {level}", got, ref)
    for name, (f, f32, _) in _updates(level, G, G32, m).items():
        print(f"lambda_ent=1 {level} {name} update: rel-frob {f:.3e} (fp32 oracle {f32:.3e})")
        assert f <= 2 * f32 + 1e-4, (name, f, f32)


def test_all_options_together_match_fp64_oracle():
    level, gan = "single-level", "Vanilla"
    kw = dict(lambda_ent=1.0, lambda_st=1.0, d_input="entropy")
    G, ref = _oracle_step(level, gan, torch.float64, **kw)
    G32, _ = _oracle_step(level, gan, torch.float32, **kw)
    tr, m, _, _ = _trainer(level, gan, **kw)
    got = tr.step(0, [_batch(level, with_labels_t=True)]).values()
    assert "loss_ent2" in got and "loss_st2" in got
    _check_losses("ent+st+entropy-D", got, ref)
    for name, (f, f32, _) in _updates(level, G, G32, m).items():
        print(f"ent+st+entropy-D {name} update: rel-frob {f:.3e} (fp32 oracle {f32:.3e})")
        assert f <= 2 * f32 + 1e-4, (name, f, f32)


def test_entropy_d_input_step_matches_fp64_oracle():
    level, gan = "single-level", "Vanilla"
    kw = dict(d_input="entropy", lambda_adv2=1.0)
    G, ref = _oracle_step(level, gan, torch.float64, **kw)
    G32, _ = _oracle_step(level, gan, torch.float32, **kw)
    Gsm, _ = _oracle_step(level, gan, torch.float64, d_input="softmax", lambda_adv2=1.0)
    tr, m, _, _ = _trainer(level, gan, d_input="entropy", lambda_adv_target2=1.0)
    got = tr.step(0, [_batch(level)]).values()
    _check_losses("d_input=entropy", got, ref)
    f, f32, dref = _updates(level, G, G32, m)["heads"]
    bound = 2 * f32 + 1e-4
    moved = _frob(_updates(level, Gsm, G32, m)["heads"][2], dref)   # the softmax-fed oracle's update vs the entropy-fed
    print(f"d_input=entropy heads update: rel-frob {f:.3e} (fp32 oracle {f32:.3e}, bound {bound:.3e}); "
          f"softmax-fed fp64 oracle differs by {moved:.3e}")
    assert moved >= 3 * bound, f"the bound {bound:.3e} no longer tells the two inputs apart ({moved:.3e})"
    assert f <= bound, (f, f32)


@pytest.mark.parametrize("level,gan", LEVEL_GAN)
@pytest.mark.parametrize("d_reuse", [True, False])
@pytest.mark.parametrize("d_input", ["entropy", "softmax"])
def test_every_discriminator_input_goes_through_d_input(monkeypatch, level, gan, d_reuse, d_input):
    from adaptsegnet_amd import functional as AF
    calls = {"softmax2d": 0, "selfinfo2d": 0}

    def spy(name):
        real = getattr(AF, name)

        def f(x):
            calls[name] += 1
            return real(x)
        return f
    for name in calls:
        monkeypatch.setattr(AF, name, spy(name))
    tr, _, _, _ = _trainer(level, gan, d_input=d_input, d_reuse=d_reuse)
    vals = tr.step(0, [_batch(level)]).values()
    assert all(math.isfinite(v) for v in vals.values())
    n = (2 if d_reuse else 3) * (2 if level == "multi-level" else 1)
    used, other = ("selfinfo2d", "softmax2d") if d_input == "entropy" else ("softmax2d", "selfinfo2d")
    assert calls[used] == n and calls[other] == 0, calls


# ---- G. defaults and paths --------------------------------------------------------------------------
def _run(level, gan, steps=2, gen="multi", **cfg):
    tr, m, d1, d2 = _trainer(level, gan, bn_train=True, gen=gen, **cfg)
    losses = [tr.step(it, [_batch(level)]).values() for it in range(steps)]
    torch.cuda.synchronize()
    return losses, [{k: v.detach().cpu().clone() for k, v in mm.state_dict().items()}
                    for mm in (m, d1, d2) if mm is not None]


def _same_runs(a, b, tag):
    assert a[0] == b[0], (tag, a[0], b[0])
    for sa, sb in zip(a[1], b[1]):
        for k in sa:
            assert torch.equal(sa[k], sb[k]), (tag, k)


@pytest.mark.parametrize("level,gan", LEVEL_GAN)
def test_explicit_defaults_are_the_default_step(level, gan):
    _same_runs(_run(level, gan), _run(level, gan, d_input="softmax", lambda_ent=0.0), "defaults")


PATHS = {
    "single-level": [dict(overlap_domains=False), dict(overlap_domains=True),
                     dict(overlap_domains=True, target_first=True), dict(overlap_domains=True, overlap_d=True),
                     dict(overlap_domains=False, d_reuse=False), dict(overlap_domains=True, second_head_only=False)],
    "multi-level": [dict(overlap_domains=False), dict(overlap_domains=True, overlap_d=True, target_first=True)],
}


@pytest.mark.parametrize("level,gan", LEVEL_GAN)
def test_target_branch_paths_are_bit_identical_with_both_options(level, gan):
    runs = [_run(level, gan, d_input="entropy", lambda_ent=1.0, **p) for p in PATHS[level]]
    assert runs[0][0][0]["loss_ent2"] > 0
    for r, p in zip(runs[1:], PATHS[level][1:]):
        _same_runs(runs[0], r, p)


def test_single_map_generator_takes_both_options():
    xs = torch.from_numpy(R.det_images((1, 3, 40, 56), 3)).float().to(DEV)
    lab = torch.from_numpy(R.det_labels((1, 40, 56), 4)).to(DEV)
    tr, m, _, _ = _trainer("single-level", "Vanilla", gen="vgg", d_input="entropy", lambda_ent=1.0,
                           input_size=(56, 40), input_size_target=(56, 40))
    with torch.no_grad():
        want = float(_entropy_torch(F.interpolate(m(xs), size=(40, 56), mode="bilinear", align_corners=True).double()))
    vals = tr.step(0, [(xs, lab, xs)]).values()
    assert "loss_ent2" in vals and all(math.isfinite(v) for v in vals.values()), vals
    assert abs(vals["loss_ent2"] - want) <= 1e-5 * want, (vals, want)
    assert all(torch.isfinite(v.double()).all() for v in m.state_dict().values())
