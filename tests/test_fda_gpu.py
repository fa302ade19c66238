"""FDA on the GPU: ``fda_source_to_target`` against tests/fda_ref.py (fp64 numpy), the robust entropy term against
an fp64 torch restatement, and StepConfig.ent_eta's wiring.

Accuracy bound of the transfer.  For each case the test computes on the CPU the max-abs error of an fp32
``torch.fft`` composition of the same formula against the fp64 reference on the same inputs; the kernel's max-abs
error must be <= 4 x max(that error, one fp32 ulp of max|ref|).  Direct summation grows its error like sqrt(n), an
FFT like log n, which is what the factor allows for; the yardstick is the reference side only.  The phase of a
vanishing coefficient is arbitrary in the reference itself, so each case asserts min |S(u, v)| >= 1 over its window.

Shapes: the smallest at which each path can go wrong -- the window at its size limit, odd sizes, rows shorter than a
wave, W % 4 != 0 (scalar staging) and W % 4 == 0 (16-byte staging), H > W, C = 1, a row longer than one staged chunk
and than one block of columns (1030 = 4 x 256 + 6), a column longer than one block's rows (300), b = 0, and the two
thresholds past the tuned range: more than 64 frequencies (the column stage loops) and more than 256 (the row
stage makes a second pass).
"""
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fda_ref as FR  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
IMG_MEAN = (104.00698793, 116.66876762, 122.67891434)
OTHER_MEAN = (90.5, 100.25, 110.0)

#        N  C  H    W     beta   mean
CASES = [(1, 3, 9, 11, 0.45, IMG_MEAN),        # the window reaches the size limit, b = 4
         (2, 3, 33, 47, 0.1, IMG_MEAN),        # odd sizes, W < 64
         (3, 3, 32, 70, 0.05, IMG_MEAN),       # W no multiple of the wave size, W % 4 != 0
         (1, 1, 70, 32, 0.05, None),           # H > W, C = 1, no mean
         (2, 3, 24, 1030, 0.1, IMG_MEAN),      # a row longer than one block's chunk
         (1, 3, 300, 40, 0.1, IMG_MEAN),       # a column longer than one block's chunk
         (2, 3, 128, 256, 0.09, OTHER_MEAN),   # b = 11, 16-byte path, a non-default mean
         (1, 3, 16, 16, 0.01, IMG_MEAN),       # b = 0: DC only
         (1, 1, 140, 136, 0.49, None),         # b = 66: more than 64 frequencies
         (1, 1, 520, 516, 0.499, None)]        # b = 257: more than 256 frequencies
IDS = ["x".join(map(str, c[:4])) + f"-b{FR.band(c[2], c[3], c[4])}" for c in CASES]


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.detach().contiguous().view(torch.int32),
                                              b.detach().contiguous().view(torch.int32))


def _images(n, c, h, w, mean, seed):
    """(src, trg) float32 [n, c, h, w], 0..255 images minus ``mean``: seeded noise of different statistics on smooth
    structure (a vertical ramp and a horizontal wave, opposite in the two domains)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    ramp = (yy / max(h - 1, 1) + np.sin(2 * np.pi * xx / max(w, 2))) * 20.0
    src = np.clip(rng.integers(0, 256, (n, c, h, w)) * 0.7 + 30 + ramp, 0, 255)
    trg = np.clip(rng.integers(0, 256, (n, c, h, w)) * 0.5 + 90 - ramp, 0, 255)
    m = np.zeros(c) if mean is None else np.asarray(mean, dtype=np.float64)
    m = m[None, :, None, None]
    return (src - m).astype(np.float32), (trg - m).astype(np.float32)


def _fft32(src, trg, b, mean):
    """The published route in fp32 with torch.fft on the CPU: the accuracy yardstick."""
    s, t = torch.from_numpy(src), torch.from_numpy(trg)
    m = torch.zeros(s.shape[1]) if mean is None else torch.tensor(mean, dtype=torch.float32)
    m = m[None, :, None, None]
    fs, ft = torch.fft.fft2(s + m), torch.fft.fft2(t + m)
    a_s = torch.fft.fftshift(fs.abs(), dim=(-2, -1))
    a_t = torch.fft.fftshift(ft.abs(), dim=(-2, -1))
    h, w = s.shape[-2:]
    ch, cw = h // 2, w // 2
    a_s[..., ch - b:ch + b + 1, cw - b:cw + b + 1] = a_t[..., ch - b:ch + b + 1, cw - b:cw + b + 1]
    a_s = torch.fft.ifftshift(a_s, dim=(-2, -1))
    return (torch.fft.ifft2(torch.polar(a_s, fs.angle())).real - m).numpy()


@functools.lru_cache(maxsize=None)
def _case(i):
    """(src, trg, fp64 reference, bound) of CASES[i], made once."""
    n, c, h, w, beta, mean = CASES[i]
    src, trg = _images(n, c, h, w, mean, 100 + i)
    assert FR.window_min_abs(src, beta, mean) >= 1.0   # no vanishing coefficient: the reference's phase is defined
    ref = FR.fda_ref(src, trg, beta, mean)
    err32 = float(np.abs(_fft32(src, trg, FR.band(h, w, beta), mean).astype(np.float64) - ref).max())
    ulp = float(np.spacing(np.float32(np.abs(ref).max())))
    return src, trg, ref, err32, ulp


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_transfer_matches_the_fp64_reference(i):
    from adaptsegnet_amd.fda import fda_source_to_target
    n, c, h, w, beta, mean = CASES[i]
    src, trg, ref, err32, ulp = _case(i)
    kw = {} if mean is IMG_MEAN else dict(mean=mean)   # the default mean is the pipeline's
    out = fda_source_to_target(torch.from_numpy(src).to(DEV), torch.from_numpy(trg).to(DEV), beta, **kw)
    assert out.dtype == torch.float32 and tuple(out.shape) == (n, c, h, w) and out.is_contiguous()
    assert not out.requires_grad
    err = float(np.abs(out.cpu().numpy().astype(np.float64) - ref).max())
    bound = 4 * max(err32, ulp)
    print(f"fda {IDS[i]}: kernel max-abs err {err:.3e}, fp32 torch.fft {err32:.3e}, ulp {ulp:.3e}, "
          f"ratio to max(fft, ulp) {err / max(err32, ulp):.2f}, moved {np.abs(ref - src).max():.1f}")
    assert np.abs(ref - src).max() > 1.0   # the transfer does something in this case
    assert err <= bound, (err, err32, ulp)


# ---- bit-exact properties --------------------------------------------------------------------------------------
def test_bit_exact_properties():
    from adaptsegnet_amd.fda import fda_source_to_target as fda
    i = 2
    assert CASES[i][:5] == (3, 3, 32, 70, 0.05)
    src, trg, ref, _, _ = _case(i)
    s, t = torch.from_numpy(src).to(DEV), torch.from_numpy(trg).to(DEV)
    s0, t0 = s.clone(), t.clone()
    out = fda(s, t, 0.05)
    assert _bits_equal(fda(s, s, 0.05), s)        # images_t is images_s: D is exactly 0
    assert _bits_equal(fda(s, t, 0.05), out)      # two calls, the same bits
    for k in range(3):                            # image k of the batch = the single-image call on it
        assert _bits_equal(fda(s[k:k + 1].contiguous(), t[k:k + 1].contiguous(), 0.05), out[k:k + 1]), k
    perm = torch.tensor([2, 0, 1], device=DEV)    # ... wherever it stands in the batch
    assert _bits_equal(fda(s[perm].contiguous(), t[perm].contiguous(), 0.05), out[perm])
    assert _bits_equal(s, s0) and _bits_equal(t, t0)   # the inputs are unmodified
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        o2 = fda(s, t, 0.05)
    side.synchronize()
    assert _bits_equal(o2, out)                   # a non-default stream
    torch.cuda.synchronize()


# ---- robust entropy -----------------------------------------------------------------------------------------------
G_LOSS = 0.7


def _frob(a, b):
    a, b = a.detach().double().cpu().flatten(), b.detach().double().cpu().flatten()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


@functools.lru_cache(maxsize=None)
def _rho_case(c, rows, eta, eps=1e-8):
    """(x fp32 [rows, c], fp64 loss, fp64 dx for grad_loss = G_LOSS): mean over rows of ((H / ln C)^2 + eps)^eta."""
    g = torch.Generator().manual_seed(7000 + 10 * c + rows)
    x = (torch.randn(rows, c, generator=g, dtype=torch.float64) * 3).float()
    xa = x.double().requires_grad_(True)
    e = torch.special.entr(torch.softmax(xa, dim=1)).sum(dim=1) / math.log(c)
    loss = ((e * e + eps) ** eta).mean()
    dx, = torch.autograd.grad(loss, xa, torch.tensor(G_LOSS, dtype=torch.float64))
    return x, float(loss.detach()), dx


@pytest.mark.parametrize("rows", [1, 300, 4097])   # 4097: the loss kernel's blocks loop
@pytest.mark.parametrize("c", [2, 19])
@pytest.mark.parametrize("eta", [0.5, 2.0])
def test_robust_entropy_matches_fp64(eta, c, rows):
    from adaptsegnet_amd import kernels as K
    x, lref, dref = _rho_case(c, rows, eta)
    xd = x.to(DEV)
    gl = torch.tensor([G_LOSS], device=DEV)
    loss = K.entropy_rho_fwd(xd, eta, 1e-8)
    dx = K.entropy_rho_bwd(xd, eta, 1e-8, gl)
    lv, f = float(loss.cpu()[0]), _frob(dx, dref)
    print(f"rho eta={eta} C={c} rows={rows}: loss rel {abs(lv - lref) / abs(lref):.2e}, dx rel-frob {f:.2e}")
    assert abs(lv - lref) < 1e-5 * abs(lref), (lv, lref)
    assert f < 1e-5, f
    assert torch.isfinite(dx).all()
    assert _bits_equal(loss, K.entropy_rho_fwd(xd, eta, 1e-8)) and _bits_equal(dx, K.entropy_rho_bwd(xd, eta, 1e-8, gl))
    # ADAPTSEG_EPI_ACCUMULATE: a launch plus an add
    dx0 = torch.randn(x.shape, generator=torch.Generator().manual_seed(5)).to(DEV)
    assert _bits_equal(K.entropy_rho_bwd(xd, eta, 1e-8, gl, dx=dx0.clone(), accumulate=True), dx0 + dx)


def test_robust_entropy_function_layouts_and_plain_call():
    from adaptsegnet_amd.functional import entropy_loss2d
    g = torch.Generator().manual_seed(9)
    x = (torch.randn(2, 19, 33, 41, generator=g) * 3).to(DEV)

    def run(xx, **kw):
        xx = xx.detach().requires_grad_(True)
        loss = entropy_loss2d(xx, **kw)
        gx, = torch.autograd.grad(loss, xx)
        return loss.detach().reshape(1), gx.contiguous()
    a = run(x.contiguous(), eta=2.0)
    b = run(x.contiguous(memory_format=torch.channels_last), eta=2.0)
    assert a[0].shape == (1,) and a[1].shape == x.shape
    assert _bits_equal(a[0], b[0]) and _bits_equal(a[1], b[1])   # NCHW = channels-last, bit for bit
    xa = x.double().cpu().requires_grad_(True)
    e = torch.special.entr(torch.softmax(xa, dim=1)).sum(dim=1) / math.log(19)
    ref = ((e * e + 1e-8) ** 2.0).mean()
    gref, = torch.autograd.grad(ref, xa)
    ref = float(ref.detach())
    assert abs(float(a[0].cpu()[0]) - ref) < 1e-5 * ref and _frob(a[1], gref) < 1e-5
    # eta=None is the plain loss, bit for bit, and the backward keeps only the logits
    p, q = run(x), run(x, eta=None, eps=0.5)
    assert _bits_equal(p[0], q[0]) and _bits_equal(p[1], q[1])
    assert not _bits_equal(p[0], a[0])
    xl = x.contiguous(memory_format=torch.channels_last).requires_grad_(True)
    kept = entropy_loss2d(xl, eta=0.5)
    saved = kept.grad_fn.saved_tensors
    assert len(saved) == 1 and saved[0].untyped_storage().data_ptr() == xl.untyped_storage().data_ptr()


# ---- the step -------------------------------------------------------------------------------------------------
def test_step_reports_the_robust_entropy_term():
    """57 x 41 source, 49 x 33 target (tests/test_entropy_gpu.py's shapes), lambda_ent = 1, ent_eta = 2."""
    import test_entropy_gpu as TE
    from adaptsegnet_amd.functional import entropy_loss2d
    level, gan = "single-level", "Vanilla"
    tr, m, _, _ = TE._trainer(level, gan, lambda_ent=1.0, ent_eta=2.0)
    batch = TE._batch(level)
    with torch.no_grad():   # eval-mode BatchNorm: a forward leaves the model as it was
        want = float(entropy_loss2d(tr._pred_single(batch[2], tr._target_size()), eta=2.0))
        plain = float(entropy_loss2d(tr._pred_single(batch[2], tr._target_size())))
    got = tr.step(0, [batch]).values()
    print(f"step: loss_ent2 {got['loss_ent2']:.7f}, entropy_loss2d(eta=2) {want:.7f}, plain {plain:.7f}")
    assert all(math.isfinite(v) for v in got.values()), got
    assert abs(got["loss_ent2"] - want) <= 1e-5 * abs(want), (got["loss_ent2"], want)
    assert abs(plain - want) > 1e-3 * abs(want)   # the two terms differ here: the step took the robust one
    assert all(torch.isfinite(v.double()).all() for v in m.state_dict().values())


def test_ent_eta_none_is_the_step_without_the_field():
    import test_entropy_gpu as TE
    level, gan = "single-level", "Vanilla"
    TE._same_runs(TE._run(level, gan, lambda_ent=1.0), TE._run(level, gan, lambda_ent=1.0, ent_eta=None), "ent_eta=None")
