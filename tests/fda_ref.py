"""The test reference of FDA's spectral transfer: the numpy formulation of the FDA paper's code, in fp64.

``fft2`` -> ``abs`` / ``angle`` -> ``fftshift`` -> window copy -> ``ifftshift`` -> ``polar`` -> ``ifft2`` -> real part,
per image and channel, the window centred at ``floor(n / 2)`` with indices ``c - b .. c + b`` on both axes and
``b = floor(min(H, W) * beta)``.  ``closed_form`` is the identity the kernel rests on: the source plus
a real low-frequency correction.  Not part of the package.
"""
import numpy as np


def band(h, w, beta):
    return int(np.floor(min(h, w) * beta))


def _swap(src, trg, b):
    """[..., H, W] fp64 -> (complex ifft2 of the source spectrum with the target's window amplitudes)."""
    h, w = src.shape[-2:]
    fs, ft = np.fft.fft2(src, axes=(-2, -1)), np.fft.fft2(trg, axes=(-2, -1))
    amp_s, pha_s = np.abs(fs), np.angle(fs)
    amp_t = np.abs(ft)
    a_s = np.fft.fftshift(amp_s, axes=(-2, -1))
    a_t = np.fft.fftshift(amp_t, axes=(-2, -1))
    ch, cw = int(np.floor(h / 2.0)), int(np.floor(w / 2.0))
    a_s[..., ch - b:ch + b + 1, cw - b:cw + b + 1] = a_t[..., ch - b:ch + b + 1, cw - b:cw + b + 1]
    a_s = np.fft.ifftshift(a_s, axes=(-2, -1))
    return np.fft.ifft2(a_s * np.exp(1j * pha_s), axes=(-2, -1))


def fda_ref(src, trg, beta=0.01, mean=None, return_residue=False):
    """src, trg [N, C, H, W] (any float dtype; computed in fp64).  ``mean``: length-C or None; the spectra are
    those of ``x + mean[c]`` and the result is back in the mean-subtracted domain."""
    src, trg = np.asarray(src, dtype=np.float64), np.asarray(trg, dtype=np.float64)
    assert src.shape == trg.shape and src.ndim == 4
    h, w = src.shape[-2:]
    b = band(h, w, beta)
    assert 0 <= 2 * b + 1 <= min(h, w)
    m = np.zeros(src.shape[1]) if mean is None else np.asarray(mean, dtype=np.float64).reshape(-1)
    assert m.shape == (src.shape[1],)
    m = m[None, :, None, None]
    z = _swap(src + m, trg + m, b)
    out = z.real - m
    return (out, float(np.abs(z.imag).max())) if return_residue else out


def window_min_abs(src, beta, mean=None):
    """min |S(u, v)| over the window: where it vanishes the reference's own phase is arbitrary."""
    src = np.asarray(src, dtype=np.float64)
    h, w = src.shape[-2:]
    b = band(h, w, beta)
    m = np.zeros(src.shape[1]) if mean is None else np.asarray(mean, dtype=np.float64).reshape(-1)
    f = np.fft.fftshift(np.abs(np.fft.fft2(src + m[None, :, None, None], axes=(-2, -1))), axes=(-2, -1))
    ch, cw = h // 2, w // 2
    return float(f[..., ch - b:ch + b + 1, cw - b:cw + b + 1].min())


def closed_form(src, trg, beta=0.01, mean=None):
    """out = src + (1 / HW) sum_{|u|,|v|<=b} D(u,v) e^{+2 pi i (uy/H + vx/W)}, D = (|T| - |S|) S / |S| (S / |S| = 1
    where S == 0), by direct summation over the window in fp64: no inverse transform of the whole spectrum."""
    src, trg = np.asarray(src, dtype=np.float64), np.asarray(trg, dtype=np.float64)
    n, c, h, w = src.shape
    b = band(h, w, beta)
    m = np.zeros(c) if mean is None else np.asarray(mean, dtype=np.float64).reshape(-1)
    u = np.arange(-b, b + 1)
    ey = np.exp(-2j * np.pi * np.outer(u, np.arange(h)) / h)   # [2b+1, H]
    ex = np.exp(-2j * np.pi * np.outer(u, np.arange(w)) / w)   # [2b+1, W]
    mm = m[None, :, None, None]
    fs = np.einsum("uy,ncyx,vx->ncuv", ey, src + mm, ex)
    ft = np.einsum("uy,ncyx,vx->ncuv", ey, trg + mm, ex)
    a_s = np.abs(fs)
    phase = np.where(a_s > 0, fs / np.where(a_s > 0, a_s, 1.0), 1.0)
    d = (np.abs(ft) - a_s) * phase
    corr = np.einsum("uy,ncuv,vx->ncyx", ey.conj(), d, ex.conj()) / (h * w)
    return src + corr.real, float(np.abs(corr.imag).max())
