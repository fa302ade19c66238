"""fp32-storage BatchNorm passes (csrc/bn.hip) against an fp64 restatement, across the channel
and row layouts of the launch planner, plus the statistics' numerical edges and the row-tile
merge (bn_tiles_final_kernel) on hand-made tiles.

Layouts.  A block is tc channel quads x tr row lanes; rows are split over blockIdx.y.  The channel
counts below give (tc, channel blocks, tr) = 4:(1,1,256) 12:(2,2,128) 20:(4,2,64) 48:(8,2,32)
100:(16,2,16) 260:(64,2,4) 512:(64,2,4) 2048:(64,8,4): several channel blocks, a partly idle last
block (12, 20, 48, 100, 260) and tr from 4 to 256.  rows = 20*tr + 3 gives 3 reduction and 6
apply splits whose lengths are no multiple of 4*tr (a masked tail iteration inside a split);
rows 2, 3, 5 are fewer than the row lanes.  The plan itself is not asserted.

Data.  Channel c has its own mean, scale, weight and bias, so statistics or coefficients read
from another channel or another block miss by orders of magnitude.  The saved mean is an fp32
output: it carries up to 2^-24 |mean|, which the apply passes see as 2^-24 |mean| / scale in
xhat.  The scales span 0.01 .. 10 and the means +-50, paired so that |mean| <= 16 * scale: that
term stays below 1e-6 and the 1e-5 bound is attainable by an fp32 implementation.  For the same
reason the 2 / 3 / 5-row inputs spread their rows deterministically (a chance near-tie of two
rows would make xhat arbitrarily sensitive to the mean's last bit) and keep |mean| <= scale:
their backward is a difference of nearly equal terms (on 2 rows the result is eps / (var + eps)
of them), which amplifies that 2^-24 |mean| / scale about tenfold.

Tolerance: the project's 1e-5 for pointwise ops and reductions (tests/test_ops_gpu.py): outputs
relative to the tensor's max (dx per channel: its magnitude follows 1/scale, a tensor-wide max
would blind the wide channels), mean relative to 1 + max|mean|, invstd and running_var per
channel, running_mean like mean, dweight / dbias relative to the tensor's max.

ReLU / LeakyReLU backward: a pre-activation within rounding of zero may take another sign in
fp32, and one flipped element moves mean(g) of its channel.  The reference gradient therefore
uses the kernel's own forward sign (y_gpu > 0), guarded by: every element whose sign disagrees
with the fp64 pre-activation lies within 1e-5 * max|pre|, and the mask recomputed from x is
bitwise the mask from y wherever there is no residual.
"""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
EPS = 1e-5
TOL = 1e-5
TR = {4: 256, 12: 128, 20: 64, 48: 32, 100: 16, 260: 4, 512: 4, 2048: 4}
LAYOUTS = [(20 * TR[c] + 3, c) for c in (4, 12, 20, 48, 100, 260, 512, 2048)] + \
          [(r, c) for c in (4, 64, 2048) for r in (2, 3, 5)]
LAYOUT_IDS = [f"r{r}-c{c}" for r, c in LAYOUTS]


def K():
    from adaptsegnet_amd import kernels
    return kernels


def dev(t):
    return None if t is None else t.float().to(DEV)


def host(t):
    return t.detach().double().cpu()


def err_max(got, ref):
    """max|got - ref| / max|ref| over the tensor."""
    got, ref = host(got), host(ref)
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


def err_chan(got, ref):
    """[rows, C]: the largest per-channel max|err| / max|ref| (a channel whose reference is below
    1e-3 of the tensor's max is measured against that floor)."""
    got, ref = host(got), host(ref)
    den = ref.abs().amax(0).clamp_min(1e-3 * float(ref.abs().max()) + 1e-30)
    return float(((got - ref).abs().amax(0) / den).max())


def err_dx(got, ref):
    """dx: per channel; on 2 / 3 / 5 rows relative to the tensor's max, the project's stated
    measure.  BN backward projects g off span{1, xhat}; with rows - 2 <= 3 dimensions left a
    channel's own result is, by chance, far below the terms it is the difference of (on 2 rows
    it is all cancellation, (g0 - g1) / 2 * eps / (var + eps)), so its own magnitude says
    nothing about the rounding it carries."""
    return err_chan(got, ref) if ref.shape[0] > 5 else err_max(got, ref)


def err_mean(got, ref):
    got, ref = host(got), host(ref)
    return float((got - ref).abs().max() / (1 + ref.abs().max()))


def err_rel(got, ref):
    """per-element relative error of a strictly positive reference (invstd, running_var)"""
    got, ref = host(got), host(ref)
    return float(((got - ref) / ref).abs().max())


@functools.lru_cache(maxsize=None)
def case(rows, c):
    """The shared inputs of a layout, fp64 on the CPU holding fp32-representable values; never
    modified by a test."""
    g = torch.Generator().manual_seed(1000 * rows + c)
    scale = 10.0 ** (torch.linspace(-2, 1, c, dtype=torch.float64)[torch.randperm(c, generator=g)])
    u = torch.rand(c, generator=g, dtype=torch.float64) * 2 - 1
    mean = u * torch.minimum(torch.full_like(scale, 50.0), (16.0 if rows > 5 else 1.0) * scale)
    if rows <= 5:
        z = torch.linspace(-1, 1, rows, dtype=torch.float64)[:, None] + \
            0.3 * (torch.rand(rows, c, generator=g, dtype=torch.float64) * 2 - 1)
    else:
        z = torch.randn(rows, c, generator=g, dtype=torch.float64)
    f32 = lambda t: t.float().double()   # noqa: E731
    d = {
        "x": f32(mean + scale * z),
        "w": f32((0.5 + torch.rand(c, generator=g, dtype=torch.float64)) *
                 torch.where(torch.rand(c, generator=g) < 0.25, -1.0, 1.0).double()),
        "b": f32(torch.rand(c, generator=g, dtype=torch.float64) - 0.5),
        "res": f32(torch.randn(rows, c, generator=g, dtype=torch.float64)),
        "dy": f32(torch.randn(rows, c, generator=g, dtype=torch.float64)),
        "rm": f32(torch.randn(c, generator=g, dtype=torch.float64) * 3),
        "rv": f32(torch.rand(c, generator=g, dtype=torch.float64) * 4 + 0.1),
    }
    xd = d["x"]
    d["mean"] = xd.mean(0)
    d["var"] = xd.var(0, unbiased=False)
    d["invstd"] = 1.0 / torch.sqrt(d["var"] + EPS)
    d["xhat"] = (xd - d["mean"]) * d["invstd"]
    return d


def act_ref(v, act):
    return v if act == 0 else v.clamp_min(0) if act == 1 else torch.where(v > 0, v, 0.2 * v)


def check_mask(y_gpu, pre):
    """The kernel's forward sign against the fp64 pre-activation's: disagreements only within
    rounding of zero.  Returns the kernel's mask (fp64 0/1, CPU)."""
    m = host(y_gpu) > 0
    bad = m != (pre > 0)
    if bool(bad.any()):
        worst = float(pre[bad].abs().max())
        assert worst <= TOL * float(pre.abs().max()), f"sign flip at |pre| = {worst:.3e}"
    return m.double()


def bwd_ref(d, g, train=True, invstd=None):
    """Closed-form BN backward of the masked gradient g on the fp64 statistics."""
    if not train:
        return g * d["w"] * invstd
    xh = d["xhat"]
    return d["w"] * d["invstd"] * (g - g.mean(0) - xh * (g * xh).mean(0))


# ------------------------------------------------------------------------------------------
# 1. layout matrix
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,c", LAYOUTS, ids=LAYOUT_IDS)
def test_forward_train(rows, c):
    k, d = K(), case(rows, c)
    xg, wg, bg = dev(d["x"]), dev(d["w"]), dev(d["b"])
    for act, with_res, mom in ((0, False, 0.1), (1, False, 0.3), (2, False, 0.1),
                               (1, True, 0.1), (0, True, 0.3), (2, True, 0.3)):
        rm, rv = dev(d["rm"]), dev(d["rv"])
        y, mean, invstd = k.bn_fwd_train(xg, wg, bg, rm, rv, mom, EPS, res=dev(d["res"]) if with_res else None,
                                         relu=act)
        pre = d["xhat"] * d["w"] + d["b"] + (d["res"] if with_res else 0)
        tag = (rows, c, act, with_res)
        assert err_max(y, act_ref(pre, act)) < TOL, tag
        assert err_mean(mean, d["mean"]) < TOL, tag
        assert err_rel(invstd, d["invstd"]) < TOL, tag
        assert err_mean(rm, (1 - mom) * d["rm"] + mom * d["mean"]) < TOL, tag
        assert err_rel(rv, (1 - mom) * d["rv"] + mom * d["var"] * rows / (rows - 1)) < TOL, tag


@pytest.mark.parametrize("c", [4, 64])
def test_forward_train_one_row_raises(c):
    k = K()
    x = torch.ones(1, c, device=DEV)
    o = torch.ones(c, device=DEV)
    with pytest.raises(RuntimeError):
        k.bn_fwd_train(x, o, o.clone(), o.clone(), o.clone(), 0.1, EPS)
    torch.cuda.synchronize()


@pytest.mark.parametrize("rows,c", LAYOUTS, ids=LAYOUT_IDS)
def test_forward_infer(rows, c):
    k, d = K(), case(rows, c)
    # running statistics near the data's (else every output saturates one side of the activation)
    rm, rv = (d["mean"] + 0.1 / d["invstd"]).float().double(), (d["var"] * 1.3 + 1e-3).float().double()
    for act, with_res in ((1, False), (0, True), (2, False), (1, True)):
        y = k.bn_fwd_infer(dev(d["x"]), dev(d["w"]), dev(d["b"]), dev(rm), dev(rv), EPS,
                           res=dev(d["res"]) if with_res else None, relu=act)
        pre = (d["x"] - rm) / torch.sqrt(rv + EPS) * d["w"] + d["b"] + (d["res"] if with_res else 0)
        assert err_max(y, act_ref(pre, act)) < TOL, (rows, c, act, with_res)


@pytest.mark.parametrize("rows,c", LAYOUTS, ids=LAYOUT_IDS)
def test_backward_train(rows, c):
    """bn_bwd: mask from y / recomputed from x / none, with dres, in place."""
    k, d = K(), case(rows, c)
    xg, wg, bg, dyg = dev(d["x"]), dev(d["w"]), dev(d["b"]), dev(d["dy"])
    pre0 = d["xhat"] * d["w"] + d["b"]
    # no residual: mask from y, and recomputed from x
    y, mean, invstd = k.bn_fwd_train(xg, wg, bg, None, None, 0.1, EPS, relu=1)
    g = d["dy"] * check_mask(y, pre0)
    ref = bwd_ref(d, g)
    dx_y = k.bn_bwd(dyg, y, xg, wg, mean, invstd, relu=1)
    assert err_dx(dx_y, ref) < TOL
    dx_x = k.bn_bwd(dyg, None, xg, wg, mean, invstd, relu=1, bias=bg)
    assert torch.equal(dx_x, dx_y)
    # ... the latter in place, with the residual gradient
    buf, dres = dyg.clone(), torch.full_like(dyg, float("nan"))
    out = k.bn_bwd(buf, None, xg, wg, mean, invstd, relu=1, bias=bg, dx=buf, dres=dres)
    assert out is buf and torch.equal(buf, dx_y)
    assert torch.equal(host(dres), g)
    # no mask, in place
    buf = dyg.clone()
    k.bn_bwd(buf, None, xg, wg, mean, invstd, relu=0, dx=buf)
    assert err_dx(buf, bwd_ref(d, d["dy"])) < TOL
    # residual block: mask from y only, dres; out of place and in place
    y, mean, invstd = k.bn_fwd_train(xg, wg, bg, None, None, 0.1, EPS, res=dev(d["res"]), relu=1)
    g = d["dy"] * check_mask(y, pre0 + d["res"])
    ref = bwd_ref(d, g)
    dres = torch.full_like(dyg, float("nan"))
    dx = k.bn_bwd(dyg, y, xg, wg, mean, invstd, relu=1, dres=dres)
    assert err_dx(dx, ref) < TOL
    assert torch.equal(host(dres), g)
    buf = dyg.clone()
    k.bn_bwd(buf, y, xg, wg, mean, invstd, relu=1, dx=buf)
    assert torch.equal(buf, dx)
    assert torch.equal(host(dyg), d["dy"])   # the out-of-place calls left dy alone


@pytest.mark.parametrize("rows,c", LAYOUTS, ids=LAYOUT_IDS)
def test_backward_affine(rows, c):
    """bn_bwd_affine: act 0 / ReLU / LeakyReLU, mask from y and from x, dweight / dbias
    accumulated into non-zero buffers."""
    k, d = K(), case(rows, c)
    xg, wg, bg, dyg = dev(d["x"]), dev(d["w"]), dev(d["b"]), dev(d["dy"])
    g0 = torch.Generator().manual_seed(c)
    dw0 = torch.randn(c, generator=g0).double()
    db0 = torch.randn(c, generator=g0).double()
    pre = d["xhat"] * d["w"] + d["b"]
    for act in (0, 1, 2):
        y, mean, invstd = k.bn_fwd_train(xg, wg, bg, None, None, 0.1, EPS, relu=act)
        assert err_max(y, act_ref(pre, act)) < TOL
        m = check_mask(y, pre) if act else torch.ones_like(pre)
        g = d["dy"] * (m if act < 2 else 0.2 + 0.8 * m)
        ref = bwd_ref(d, g)
        outs = []
        for y_src in (y, None):   # mask from y out of place, mask from x in place
            dw, db = dev(dw0), dev(db0)
            buf = dyg.clone()
            dx = k.bn_bwd_affine(buf, y_src, xg, wg, bg, mean, invstd, act, dw, db, dx=buf if y_src is None else None)
            tag = (rows, c, act, y_src is None)
            assert (dx is buf) == (y_src is None)
            assert err_dx(dx, ref) < TOL, tag
            assert err_max(host(dw) - dw0, (g * d["xhat"]).sum(0)) < TOL, tag
            assert err_max(host(db) - db0, g.sum(0)) < TOL, tag
            outs.append((dx, dw, db))
        assert all(torch.equal(a, b) for a, b in zip(*outs))   # mask from x == mask from y, bitwise


@pytest.mark.parametrize("rows,c", LAYOUTS, ids=LAYOUT_IDS)
def test_backward_eval(rows, c):
    k, d = K(), case(rows, c)
    xg, wg, bg, dyg = dev(d["x"]), dev(d["w"]), dev(d["b"]), dev(d["dy"])
    rm, rv = (d["mean"] + 0.1 / d["invstd"]).float().double(), (d["var"] * 1.3 + 1e-3).float().double()
    inv = (1.0 / torch.sqrt(rv + EPS)).float().double()
    pre = (d["x"] - rm) / torch.sqrt(rv + EPS) * d["w"] + d["b"]
    for act, with_res in ((1, False), (0, False), (1, True)):
        p = pre + (d["res"] if with_res else 0)
        y = k.bn_fwd_infer(xg, wg, bg, dev(rm), dev(rv), EPS, res=dev(d["res"]) if with_res else None, relu=act)
        g = d["dy"] * (check_mask(y, p) if act else 1.0)
        dres = torch.full_like(dyg, float("nan")) if with_res else None
        dx = k.bn_bwd(dyg, y if act else None, xg, wg, dev(rm), dev(inv), relu=act, dres=dres, train=False)
        assert err_dx(dx, bwd_ref(d, g, train=False, invstd=inv)) < TOL, (rows, c, act, with_res)
        if with_res:
            assert torch.equal(host(dres), g)


# ------------------------------------------------------------------------------------------
# 2. statistics numerics at the edges
# ------------------------------------------------------------------------------------------
def stats_ref(x):
    mean = x.mean(0)
    var = x.var(0, unbiased=False)
    return mean, var, 1.0 / torch.sqrt(var + EPS)


def affine(c):
    i = torch.arange(c, dtype=torch.float64)
    return (0.75 + 0.5 * i / c).float().double(), (0.3 * torch.cos(i)).float().double()


@pytest.mark.parametrize("kk", [10, 100])
@pytest.mark.parametrize("c", [8, 64])
def test_stats_pivot_outlier(c, kk):
    """x ~ N(5, 1) with one row at 5 + K in every channel: the same multiset with that row first
    or at 1777 has the same statistics, and both must meet 1e-5 (torch's fp32 CPU batch norm is
    within 4e-7 on these inputs).

    Measured on an MI355X, relative error of invstd (outlier at row 0 / at row 1777), with the
    statistics pass shifting by x[0][c]: C 8 K 10 1.1e-5 / 4.5e-7, C 8 K 100 3.0e-4 / 1.9e-7,
    C 64 K 10 3.4e-6 / 6.5e-8, C 64 K 100 9.5e-5 / 1.1e-7 (three of the four cases failed);
    with the finalize re-summing a channel whose pivot lies more than 6 sigma from its mean:
    5.7e-8 / 4.5e-7, 5.2e-8 / 1.9e-7, 5.6e-8 / 6.5e-8, 5.4e-8 / 1.1e-7.
    """
    k = K()
    rows = 4099
    g = torch.Generator().manual_seed(17 * c + kk)
    base = (5 + torch.randn(rows, c, generator=g, dtype=torch.float64)).float().double()
    base[0] = 5.0 + kk
    w, b = affine(c)
    errs = {}
    for at in (0, 1777):
        x = base.clone()
        x[[0, at]] = x[[at, 0]]
        mean, var, invstd = stats_ref(x)
        y, m, i = k.bn_fwd_train(dev(x), dev(w), dev(b), None, None, 0.1, EPS, relu=0)
        errs[at] = (err_mean(m, mean), err_rel(i, invstd), err_max(y, (x - mean) * invstd * w + b))
        print(f"pivot outlier C={c} K={kk} at row {at}: mean {errs[at][0]:.2e} invstd {errs[at][1]:.2e} "
              f"y {errs[at][2]:.2e}")
    for at, e in errs.items():
        assert max(e) < TOL, (c, kk, at, e)


def test_stats_outlier_in_every_row():
    """The same, for the outlier (K = 100) in each row in turn of a 1031-row, 8-channel tensor:
    whichever rows the statistics pass leans on, none may be able to spoil it.  Mean and invstd
    only (one truth for all placements), compared on the device in fp64."""
    k = K()
    rows, c = 1031, 8
    g = torch.Generator().manual_seed(5)
    base = (5 + torch.randn(rows, c, generator=g, dtype=torch.float64)).float().double()
    base[0] = 105.0
    mean, var, invstd = (t.to(DEV) for t in stats_ref(base))
    w, b = affine(c)
    wg, bg, xg = dev(w), dev(b), dev(base)
    worst_m, worst_i = torch.zeros((), device=DEV, dtype=torch.float64), torch.zeros((), device=DEV,
                                                                                     dtype=torch.float64)
    for at in range(rows):
        if at:   # move the outlier one row down
            xg[[at - 1, at]] = xg[[at, at - 1]]
        _, m, i = k.bn_fwd_train(xg, wg, bg, None, None, 0.1, EPS, relu=0)
        worst_m = torch.maximum(worst_m, (m.double() - mean).abs().max())
        worst_i = torch.maximum(worst_i, ((i.double() - invstd) / invstd).abs().max())
    em, ei = float(worst_m) / (1 + float(mean.abs().max())), float(worst_i)
    print(f"outlier in every row: worst mean {em:.2e} invstd {ei:.2e}")
    assert em < TOL and ei < TOL


@pytest.mark.parametrize("c", [8, 64])
def test_stats_large_mean_small_spread(c):
    """x = 1000 + 0.01 randn (truth from the fp32-rounded data): var ~ 1e-4 next to eps = 1e-5, so
    invstd is sensitive to the variance.  mean and invstd at 1e-5.  y additionally carries the
    saved mean's fp32 rounding, which no fp32 mean output avoids: |mean_gpu - mean| <= 2^-14 (one
    fp32 ulp at 1000: half for the final rounding, the rest far above the summation's error), and
    the apply pass turns that into |w| * invstd * 2^-14 (~6e-3 of ~4), so y is held to
    1e-5 * max|y| + max|w * invstd| * |mean_gpu - mean| with the mean itself held to one ulp."""
    k = K()
    rows = 4099
    g = torch.Generator().manual_seed(c)
    x = (1000 + 0.01 * torch.randn(rows, c, generator=g, dtype=torch.float64)).float().double()
    w, b = affine(c)
    mean, var, invstd = stats_ref(x)
    y, m, i = k.bn_fwd_train(dev(x), dev(w), dev(b), None, None, 0.1, EPS, relu=0)
    dm = float((host(m) - mean).abs().max())
    ref = (x - mean) * invstd * w + b
    ey = float((host(y) - ref).abs().max())
    print(f"large mean C={c}: mean abs {dm:.2e} invstd {err_rel(i, invstd):.2e} y abs {ey:.2e}")
    assert err_mean(m, mean) < TOL and dm <= 2.0 ** -14
    assert err_rel(i, invstd) < TOL
    assert ey <= TOL * float(ref.abs().max()) + float((w * invstd).abs().max()) * dm


@pytest.mark.parametrize("rows", [4099, 2])
@pytest.mark.parametrize("c", [8, 64])
def test_stats_constant_channels(c, rows):
    """Channels holding exactly one value: var = 0, invstd = 1/sqrt(eps), y = bias, and the
    backward stays finite (and equal to the closed form, xhat = 0)."""
    k = K()
    g = torch.Generator().manual_seed(c + rows)
    z = torch.randn(rows, c, generator=g, dtype=torch.float64)
    if rows == 2:   # two rows well apart (see the module docstring)
        z = torch.tensor([[-1.0], [1.0]], dtype=torch.float64) + 0.3 * (torch.rand(2, c, generator=g).double() * 2 - 1)
    x = (2 + 3 * z).float().double()
    consts = {0: -3.5, 1: 0.0, 5: 1000.1, c - 1: 7e-3}
    for ch, v in consts.items():
        x[:, ch] = torch.tensor(v).float().double()
    idx = sorted(consts)
    w, b = affine(c)
    mean, var, invstd = stats_ref(x)
    var[idx] = 0.0
    invstd[idx] = 1.0 / math.sqrt(EPS)
    rv0 = torch.full((c,), 2.0, dtype=torch.float64)
    rv = dev(rv0)
    y, m, i = k.bn_fwd_train(dev(x), dev(w), dev(b), None, rv, 0.1, EPS, relu=0)
    assert torch.equal(host(m)[idx], x[0, idx])
    assert float(((host(i)[idx] - 1.0 / math.sqrt(EPS)) * math.sqrt(EPS)).abs().max()) < 1e-6
    assert float((host(rv)[idx] - 0.9 * 2.0).abs().max()) < 1e-6 * 1.8     # var = 0
    assert float((host(y)[:, idx] - b[idx]).abs().max()) <= TOL * float(b.abs().max())
    assert err_mean(m, mean) < TOL and err_rel(i, invstd) < TOL
    assert err_max(y, (x - mean) * invstd * w + b) < TOL
    dy = torch.randn(rows, c, generator=g, dtype=torch.float64).float().double()
    dx = k.bn_bwd(dev(dy), None, dev(x), dev(w), m, i, relu=0)
    assert bool(torch.isfinite(dx).all())
    xh = (x - mean) * invstd
    ref = w * invstd * (dy - dy.mean(0) - xh * (dy * xh).mean(0))
    assert err_max(dx[:, idx], ref[:, idx]) < TOL


# ------------------------------------------------------------------------------------------
# 3. bn_tiles_final_kernel on hand-made tiles
# ------------------------------------------------------------------------------------------
def tile_cases():
    out = []
    for nt in (1, 2, 63, 64, 65, 130):
        for c in (4, 20, 260):
            out.append((nt, c, "full"))
            if nt >= 2:
                out.append((nt, c, "tile0"))
                out.append((nt, c, "one"))
            if nt > 5 + 64:          # a lane with more than one tile
                out.append((nt, c, "lane5"))
            elif nt > 5 and c == 20:
                out.append((nt, c, "lane5"))
    return out


@pytest.mark.parametrize("nt,c,empty", tile_cases(), ids=lambda v: str(v))
def test_tiles_final(nt, c, empty):
    """(count, mean, M2) row tiles of unequal size, computed in fp64 and stored fp32 in the
    kernel's layout cnt[nt], mu[C][nt], m2[C][nt]; tile means several sigma apart so the
    d^2 n nb / nn term of the merge carries weight.  Empty tiles (count 0) hold garbage in mu / m2,
    which the merge never reads into the result.  Against fp64 statistics of the whole tensor."""
    k = K()
    g = torch.Generator().manual_seed(100 * nt + c + len(empty))
    sizes = torch.randint(1, 10, (nt,), generator=g)
    if empty == "tile0":
        sizes[0] = 0
    elif empty == "lane5":
        sizes[5::64] = 0
    elif empty == "one":
        keep = nt // 2
        sizes[:keep] = 0
        sizes[keep + 1:] = 0
        sizes[keep] = 7
    rows = int(sizes.sum())
    assert rows > 1
    scale = 10.0 ** (torch.linspace(-2, 1, c, dtype=torch.float64)[torch.randperm(c, generator=g)])
    cmean = (torch.rand(c, generator=g, dtype=torch.float64) * 2 - 1) * torch.minimum(torch.full_like(scale, 50.0),
                                                                                     16.0 * scale)
    off = torch.repeat_interleave(5 * torch.randn(nt, generator=g, dtype=torch.float64), sizes)
    x = cmean + scale * (torch.randn(rows, c, generator=g, dtype=torch.float64) + off[:, None])
    cnt = sizes.double()
    mu = torch.full((c, nt), 1e6, dtype=torch.float64)
    m2 = torch.full((c, nt), 3e6, dtype=torch.float64)
    r = 0
    for t in range(nt):
        n = int(sizes[t])
        if n:
            xt = x[r:r + n]
            mu[:, t] = xt.mean(0)
            m2[:, t] = ((xt - xt.mean(0)) ** 2).sum(0)
        r += n
    stats = torch.cat([cnt, mu.reshape(-1), m2.reshape(-1)]).float().to(DEV)
    mean, var, invstd = stats_ref(x)
    g2 = torch.Generator().manual_seed(nt)
    rm0 = (torch.randn(c, generator=g2) * 3).double()
    rv0 = (torch.rand(c, generator=g2) * 4 + 0.1).double()
    shape = torch.empty(rows, c, device=DEV)
    outs = []
    for mom in (0.1, 0.25, 0.1):
        rm, rv = dev(rm0), dev(rv0)
        m, i = k.bn_fwd_train_tiles_stats(shape, (stats, nt), rm, rv, mom, EPS)
        outs.append((m, i, rm, rv))
        assert err_mean(m, mean) < TOL
        assert err_rel(i, invstd) < TOL
        assert err_mean(rm, (1 - mom) * rm0 + mom * mean) < TOL
        assert err_rel(rv, (1 - mom) * rv0 + mom * var * rows / (rows - 1)) < TOL
    assert all(torch.equal(a, b) for a, b in zip(outs[0], outs[2]))   # fixed merge order
